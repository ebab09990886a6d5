// render_lines.inc — the debug lines (Uniforms.showBoundingBox: node boxes + view frustum): r_lines_emit, r_lines_raster and the clipping they need.
// render.cu:637-688 (four coincident boxes per visible node), :1197-1223 (frustum), rasterization.cuh:5-47 (drawLine,
// drawBoundingBox), :90-183 (rasterizeLines), math.cuh:22-152.  Off by default in the reference (main.cpp:125).
using LinePlane = float[4];      // {nx, ny, nz, c}, as frustum_plane (render_visible.inc) normalises it

__device__ __forceinline__ float plane_dist(const LinePlane& p, float x, float y, float z) {
	float d = p[0] * x; d = d + p[1] * y; d = d + p[2] * z; d = d + p[3];
	return d;
}

__device__ bool frustum_contains(const LinePlane P[6], float x, float y, float z) {
	bool in = true;
	for (int i = 0; i < 6; i++) if (plane_dist(P[i], x, y, z) < 0.0f) in = false;
	return in;
}

__device__ float dist_to_plane(float ox, float oy, float oz, float dx, float dy, float dz, const LinePlane& p) {
	const float INF = __uint_as_float(0x7f800000u);
	float denom = p[0] * dx; denom = denom + p[1] * dy; denom = denom + p[2] * dz;
	if (denom < 0.0f) return INF;
	if (denom == 0.0f) return plane_dist(p, ox, oy, oz) == 0.0f ? 0.0f : INF;
	float num = ox * p[0]; num = num + oy * p[1]; num = num + oz * p[2]; num = num + p[3];
	const float t = -num / denom;
	return t >= 0.0f ? t : INF;
}

__device__ void frustum_intersect_ray(const LinePlane P[6], float ox, float oy, float oz, float dx, float dy, float dz, float out[3]) {
	const float INF = __uint_as_float(0x7f800000u);
	float farthest = -INF;
	for (int i = 0; i < 6; i++) {
		const float d = dist_to_plane(ox, oy, oz, dx, dy, dz, P[i]);
		if (d > 0.0f && d != INF) farthest = fmaxf(farthest, d);
	}
	out[0] = ox + dx * farthest; out[1] = oy + dy * farthest; out[2] = oz + dz * farthest;
}

__device__ __forceinline__ void put_line(float4* v, uint32_t at, float ax, float ay, float az, float bx, float by, float bz, uint32_t color) {
	v[at] = make_float4(ax, ay, az, __uint_as_float(color));
	v[at + 1] = make_float4(bx, by, bz, __uint_as_float(color));
}

__global__ __launch_bounds__(TPB) void r_lines_emit(RenderArgs a, SimlodMat4 inv) {
	const uint32_t numVisible = min(*counter_at(a.mom, C_VISIBLE), SIMLOD_MAX_VISIBLE_NODES);
	const uint32_t i = blockIdx.x * TPB + threadIdx.x;
	uint32_t* count = reinterpret_cast<uint32_t*>(a.mom + FrameLayout::lines);
	float4* v = reinterpret_cast<float4*>(a.mom + FrameLayout::vertices);
	if (i == 0) {      // the view frustum as seen by the frozen visibility transform, render.cu:1197-1223
		const float fend = 0.99995f;
		const float C[8][2][3] = {{{1, 1, -1}, {1, 1, fend}}, {{1, -1, -1}, {1, -1, fend}}, {{-1, 1, -1}, {-1, 1, fend}}, {{-1, -1, -1}, {-1, -1, fend}},
		                          {{-1, -1, fend}, {1, -1, fend}}, {{-1, 1, fend}, {1, 1, fend}}, {{-1, -1, fend}, {-1, 1, fend}}, {{1, -1, fend}, {1, 1, fend}}};
		const uint32_t at = atomicAdd(count, 16u);
		for (int l = 0; l < 8; l++) {
			float p[2][3];
			for (int k = 0; k < 2; k++) {
				const float qx = dot_row(inv.rows[0], C[l][k][0], C[l][k][1], C[l][k][2]), qy = dot_row(inv.rows[1], C[l][k][0], C[l][k][1], C[l][k][2]);
				const float qz = dot_row(inv.rows[2], C[l][k][0], C[l][k][1], C[l][k][2]), qw = dot_row(inv.rows[3], C[l][k][0], C[l][k][1], C[l][k][2]);
				p[k][0] = qx / qw; p[k][1] = qy / qw; p[k][2] = qz / qw;
			}
			if (at + 2 * l + 2 <= LINE_VERTEX_CAP) put_line(v, at + 2 * l, p[0][0], p[0][1], p[0][2], p[1][0], p[1][1], p[1][2], 0x000000ffu);
		}
	}
	if (i >= numVisible) return;
	const SimlodNode* n = reinterpret_cast<const SimlodNode*>(a.mom + FrameLayout::visible) + i;
	if (n->numPoints == 0 && n->numVoxels == 0) return;
	const float scale = a.cubeSize / exp2_int(n->level);
	const float pos[3] = {a.minx + ((float)n->X + 0.5f) * scale, a.miny + ((float)n->Y + 0.5f) * scale, a.minz + ((float)n->Z + 0.5f) * scale};
	float mn[3], mx[3];
	for (int k = 0; k < 3; k++) { mn[k] = pos[k] - scale / 2.0f; mx[k] = pos[k] + scale / 2.0f; }
	const uint32_t at0 = atomicAdd(count, 96u);                  // 4 boxes x 12 edges x 2 vertices
	if (at0 + 96u > LINE_VERTEX_CAP) { atomicOr(&a.stats->dbg, SIMLOD_ERR_VISIBLE_OVERFLOW); return; }
	const int E[12][6] = {{0,0,0, 1,0,0}, {1,0,0, 1,1,0}, {1,1,0, 0,1,0}, {0,1,0, 0,0,0}, {0,0,1, 1,0,1}, {1,0,1, 1,1,1}, {1,1,1, 0,1,1}, {0,1,1, 0,0,1},
	                      {1,0,0, 1,0,1}, {1,1,0, 1,1,1}, {0,1,0, 0,1,1}, {0,0,0, 0,0,1}};
	for (int r = 0; r < 4; r++)
		for (int e = 0; e < 12; e++)
			put_line(v, at0 + (uint32_t)(r * 12 + e) * 2u, E[e][0] ? mx[0] : mn[0], E[e][1] ? mx[1] : mn[1], E[e][2] ? mx[2] : mn[2],
			         E[e][3] ? mx[0] : mn[0], E[e][4] ? mx[1] : mn[1], E[e][5] ? mx[2] : mn[2], 0x0000ff00u);
}

__device__ __forceinline__ int to_int_like_the_host(double v) {   // the oracle's cvttsd2si behaviour: out of range -> INT_MIN
	return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (int)0x80000000;
}

__global__ __launch_bounds__(TPB) void r_lines_raster(RenderArgs a) {
	const uint32_t count = min(*reinterpret_cast<const uint32_t*>(a.mom + FrameLayout::lines), LINE_VERTEX_CAP);
	const uint32_t l = blockIdx.x * TPB + threadIdx.x;
	if (2 * l + 1 >= count) return;
	const float4* v = reinterpret_cast<const float4*>(a.mom + FrameLayout::vertices);
	uint64_t* fb = reinterpret_cast<uint64_t*>(a.mom + FrameLayout::framebuffer);
	float4 s = v[2 * l], e = v[2 * l + 1];
	LinePlane P[6];
#pragma unroll
	for (int i = 0; i < 6; i++) frustum_plane(a.transform, i, P[i]);
	float dx = e.x - s.x, dy = e.y - s.y, dz = e.z - s.z;
	float d2 = dx * dx; d2 = d2 + dy * dy; d2 = d2 + dz * dz;
	const float inv = 1.0f / sqrtf(d2);                    // normalize(): v * rsqrtf(dot(v, v))
	dx = dx * inv; dy = dy * inv; dz = dz * inv;
	if (!frustum_contains(P, s.x, s.y, s.z)) { float I[3]; frustum_intersect_ray(P, s.x, s.y, s.z, dx, dy, dz, I); s.x = I[0]; s.y = I[1]; s.z = I[2]; }
	if (!frustum_contains(P, e.x, e.y, e.z)) { float I[3]; frustum_intersect_ray(P, e.x, e.y, e.z, dx * -1.0f, dy * -1.0f, dz * -1.0f, I); e.x = I[0]; e.y = I[1]; e.z = I[2]; }
	float ax = dot_row(a.transform.rows[0], s.x, s.y, s.z), ay = dot_row(a.transform.rows[1], s.x, s.y, s.z);
	const float aw = dot_row(a.transform.rows[3], s.x, s.y, s.z);
	float bx = dot_row(a.transform.rows[0], e.x, e.y, e.z), by = dot_row(a.transform.rows[1], e.x, e.y, e.z);
	const float bw = dot_row(a.transform.rows[3], e.x, e.y, e.z);
	ax = ax / aw; ay = ay / aw; bx = bx / bw; by = by / bw;
	const float sx0 = (ax * 0.5f + 0.5f) * (float)a.W, sy0 = (ay * 0.5f + 0.5f) * (float)a.H;
	const float sx1 = (bx * 0.5f + 0.5f) * (float)a.W, sy1 = (by * 0.5f + 0.5f) * (float)a.H;
	const float ddx = sx1 - sx0, ddy = sy1 - sy0;
	float st2 = ddx * ddx; st2 = st2 + ddy * ddy; st2 = st2 + 0.0f;
	float steps = sqrtf(st2);
	steps = fmaxf(0.0f, fminf(steps, 400.0f));
	const float stepSize = (float)(1.0 / (double)steps);
	const uint32_t color = __float_as_uint(s.w);
#pragma unroll 1
	for (float t = 0.0f; (double)t <= 1.0; t += stepSize) {
		const float tbx = t * bx, tby = t * by, tbw = t * bw;
		const float nx = (float)((1.0 - (double)t) * (double)ax + (double)tbx);
		const float ny = (float)((1.0 - (double)t) * (double)ay + (double)tby);
		const float depth = (float)((1.0 - (double)t) * (double)aw + (double)tbw);
		if ((double)nx < -1.0 || (double)nx > 1.0) continue;
		if ((double)ny < -1.0 || (double)ny > 1.0) continue;
		int x = to_int_like_the_host(((double)nx * 0.5 + 0.5) * (double)a.W);
		int y = to_int_like_the_host(((double)ny * 0.5 + 0.5) * (double)a.H);
		x = min(max(x, 0), a.W - 1); y = min(max(y, 0), a.H - 1);
		const unsigned long long enc = ((unsigned long long)__float_as_uint(depth) << 32) | color;
		atomicMin(reinterpret_cast<unsigned long long*>(&fb[x + a.W * y]), enc);   // rasterization.cuh:175-178
	}
}
