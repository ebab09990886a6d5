// view_rules.hpp — the view query's rules V2-V4 (include/simlod_hip.h, "view queries"): what a SimlodView and its camera must look like to be
// accepted, the frustum planes, a node's inside / screen extents from (level, X, Y, Z), its rank, and what is drawn at a bias.  No HIP in here:
// export_view.inc's kernel, the launcher (export.hip) and tests/host/view_rules_check.cpp (plain g++) read it here.
// The fp32 arithmetic of render_visible.inc (frustum_plane, intersects_frustum, node_geometry), restated operation for operation; that file is the
// rasteriser's and stays as it is — the two copies are pinned to each other by the view query's equality with a frame (rule V8, tests/test_gpu_view.py).
// No fused multiply-add (the library is built with -ffp-contract=off; the host program likewise), divisions and square roots correctly rounded,
// so that the numpy mirror (simlod_amd/octree_io.py OctreeExport.view, view_geometry) reproduces every decision bit for bit.
#pragma once
#include <stdint.h>
#include <cmath>
#include "simlod_hip.h"
#if defined(__HIPCC__)
#define SIMLOD_HD __host__ __device__
#else
#define SIMLOD_HD
#endif

namespace simlod {

constexpr uint32_t VIEW_RANKS = SIMLOD_VIEW_MAX_BIAS + 1u;          // the biases 0..20; a rank is 0..21

// What simlod_query_view refuses in its view and its camera.
inline bool view_acceptable(const SimlodView& v, const SimlodUniforms& u) {
	if ((v.flags & ~(SIMLOD_VIEW_NO_CULL | SIMLOD_VIEW_DRAW_SMALL_ROOT)) != 0u || v.reserved != 0u) return false;
	if (v.minBias > v.maxBias || v.maxBias > SIMLOD_VIEW_MAX_BIAS) return false;
	if (!std::isfinite(u.minNodeSize) || !std::isfinite(u.width) || !std::isfinite(u.height)) return false;
	for (int j = 0; j < 4; j++) {
		const simlod_float4& r = u.transform_updateBound.rows[j];
		if (!std::isfinite(r.x) || !std::isfinite(r.y) || !std::isfinite(r.z) || !std::isfinite(r.w)) return false;
	}
	return true;
}

// The camera as the kernel takes it: what launch_render puts into its RenderArgs of the same uniforms.
struct ViewGeom {
	SimlodMat4 m;                       // transform_updateBound
	float      cubeSize, minx, miny, minz;
	float      width, height, minNodeSize, pad;
};

// math.cuh:154-201 as render_visible.inc frustum_plane: plane i from the rows of the matrix, normalised
SIMLOD_HD inline void view_frustum_plane(const SimlodMat4& m, int i, float out[4]) {
	const simlod_float4* R = m.rows;
	const float m0 = R[0].x, m1 = R[1].x, m2 = R[2].x, m3 = R[3].x;
	const float m4 = R[0].y, m5 = R[1].y, m6 = R[2].y, m7 = R[3].y;
	const float m8 = R[0].z, m9 = R[1].z, m10 = R[2].z, m11 = R[3].z;
	const float m12 = R[0].w, m13 = R[1].w, m14 = R[2].w, m15 = R[3].w;
	const float P[6][4] = {
		{m3 - m0, m7 - m4, m11 - m8, m15 - m12}, {m3 + m0, m7 + m4, m11 + m8, m15 + m12},
		{m3 + m1, m7 + m5, m11 + m9, m15 + m13}, {m3 - m1, m7 - m5, m11 - m9, m15 - m13},
		{m3 - m2, m7 - m6, m11 - m10, m15 - m14}, {m3 + m2, m7 + m6, m11 + m10, m15 + m14}};
	const float x = P[i][0], y = P[i][1], z = P[i][2], w = P[i][3];
	float d2 = x * x; d2 = d2 + y * y; d2 = d2 + z * z;
	const float len = sqrtf(d2);
	out[0] = x / len; out[1] = y / len; out[2] = z / len; out[3] = w / len;
}

SIMLOD_HD inline bool view_intersects_frustum(const float (*planes)[4], const float mn[3], const float mx[3]) {
	bool inside = true;
	for (int i = 0; i < 6; i++) {
		const float nx = planes[i][0], ny = planes[i][1], nz = planes[i][2], c = planes[i][3];
		const float vx = nx > 0.0f ? mx[0] : mn[0];
		const float vy = ny > 0.0f ? mx[1] : mn[1];
		const float vz = nz > 0.0f ? mx[2] : mn[2];
		float d = nx * vx; d = d + ny * vy; d = d + nz * vz; d = d + c;
		if (d < 0.0f) inside = false;
	}
	return inside;
}

SIMLOD_HD inline float view_dot_row(const simlod_float4& r, float x, float y, float z) {
	float s = r.x * x;
	s = s + r.y * y;
	s = s + r.z * z;
	s = s + r.w * 1.0f;
	return s;
}

// render.cu:760-861 as render_visible.inc node_geometry: does the cube of (level, X, Y, Z) meet the frustum, and the extents of its screen box
SIMLOD_HD inline void view_node_geometry(const ViewGeom& g, const float (*planes)[4], uint32_t level, uint32_t X, uint32_t Y, uint32_t Z, bool& inside,
                                         float& dx, float& dy) {
	const float nodeSize = g.cubeSize / ldexpf(1.0f, (int)level);                     // (2^level: exact)
	const float cmin[3] = {g.minx, g.miny, g.minz};
	const uint32_t XYZ[3] = {X, Y, Z};
	float mn[3], mx[3];
	for (int k = 0; k < 3; k++) {
		mn[k] = cmin[k] + ((float)XYZ[k] + 0.0f) * nodeSize;
		mx[k] = cmin[k] + ((float)XYZ[k] + 1.0f) * nodeSize;
	}
	float sx[8], sy[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
	for (int k = 0; k < 8; k++) {   // p000, p001, p010, p011, p100, p101, p110, p111 (render.cu:783-790)
		const float x = (k & 4) ? mx[0] : mn[0], y = (k & 2) ? mx[1] : mn[1], z = (k & 1) ? mx[2] : mn[2];
		const float cx = view_dot_row(g.m.rows[0], x, y, z);
		const float cy = view_dot_row(g.m.rows[1], x, y, z);
		const float cw = view_dot_row(g.m.rows[3], x, y, z);
		sx[k] = ((cx / cw) * 0.5f + 0.5f) * g.width;
		sy[k] = ((cy / cw) * 0.5f + 0.5f) * g.height;
	}
	const float minx = fminf(fminf(fminf(sx[0], sx[1]), fminf(sx[2], sx[3])), fminf(fminf(sx[4], sx[5]), fminf(sx[6], sx[7])));
	const float maxx = fmaxf(fmaxf(fmaxf(sx[0], sx[1]), fmaxf(sx[2], sx[3])), fmaxf(fmaxf(sx[4], sx[5]), fmaxf(sx[6], sx[7])));
	const float miny = fminf(fminf(fminf(sy[0], sy[1]), fminf(sy[2], sy[3])), fminf(fminf(sy[4], sy[5]), fminf(sy[6], sy[7])));
	const float maxy = fmaxf(fmaxf(fmaxf(sy[0], sy[1]), fmaxf(sy[2], sy[3])), fmaxf(fmaxf(sy[4], sy[5]), fmaxf(sy[6], sy[7])));
	dx = maxx - minx; dy = maxy - miny;
	inside = view_intersects_frustum(planes, mn, mx);
}

// rule V3: R = the number of biases b in 0..20 at which the node is large, (double)dx > L_b || (double)dy > L_b with L_b = 2.0 * minNodeSize * 2^b
// (render.cu:860-861 with minNodeSize * 2^b; the products are exact; a NaN extent is never large).  Either extent above L_b is the larger one
// above it — fmaxf drops a NaN, and two NaNs are above nothing.  With minNodeSize > 0 the L_b grow with b, so the node is large at the biases
// below R and at no other: R is found in five steps.  Any other minNodeSize: counted bias by bias.
SIMLOD_HD inline uint32_t view_rank(float minNodeSize, float dx, float dy) {
	const double lim = 2.0 * (double)minNodeSize, m = (double)fmaxf(dx, dy);
	if (lim > 0.0) {
		uint32_t lo = 0u, hi = VIEW_RANKS;                                           // large at every b < lo, at no b >= hi
		for (int step = 0; step < 5; step++) {
			const uint32_t mid = (lo + hi) >> 1;                                     // (lo < hi: a bias, mid <= 20)
			const bool large = m > ldexp(lim, (int)mid);
			if (lo < hi) { if (large) lo = mid + 1u; else hi = mid; }
		}
		return lo;
	}
	uint32_t r = 0;
	for (uint32_t b = 0; b < VIEW_RANKS; b++) r += m > ldexp(lim, (int)b) ? 1u : 0u;
	return r;
}
static_assert(VIEW_RANKS < (1u << 5), "view_rank: five halvings of [0, VIEW_RANKS]");

// rule V4: the biases at which a visible node of rank R under a parent of rank P (rule V3's P) is drawn are [from, to) — a leaf is drawn while it
// is large (b < R) and, like an inner node, while it is small under a large parent (R <= b < P).  from >= to: never.
SIMLOD_HD inline void view_drawn_range(uint32_t R, uint32_t P, bool leaf, uint32_t& from, uint32_t& to) {
	from = leaf ? 0u : R;
	to = leaf ? (P > R ? P : R) : P;
}
SIMLOD_HD inline bool view_drawn(uint32_t b, uint32_t R, uint32_t P, bool leaf) { return b < R ? leaf : b < P; }

}  // namespace simlod
