// render_output.inc — HQS resolve (render.cu:607-632) and the frame's last kernel: r_resolve, r_unpack, resolved_depth_bits, r_output (Stats, EDL, RGBA8).
__global__ __launch_bounds__(TPB) void r_resolve(RenderArgs a) {
	uint64_t* fb = reinterpret_cast<uint64_t*>(a.mom + FrameLayout::framebuffer);
	const uint32_t* depth = reinterpret_cast<const uint32_t*>(a.mom + a.lay.depth);
	const unsigned long long* packed = reinterpret_cast<const unsigned long long*>(a.mom + a.lay.colour);
	const uint4* overflow = reinterpret_cast<const uint4*>(a.mom + a.lay.sums);
	const uint32_t stride = gridDim.x * TPB;
	for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < a.numPixels; i += stride) {
		const unsigned long long pk = packed[i];
		uint4 s = overflow[i];                           // {R, G, B, count} of the samples beyond the 64th
		s.x += (uint32_t)((pk >> 28) & 0x3fffu); s.y += (uint32_t)((pk >> 14) & 0x3fffu); s.z += (uint32_t)(pk & 0x3fffu); s.w += (uint32_t)(pk >> 42);
		if (s.w == 0u) continue;
		const uint32_t rgba = ((s.x / s.w) & 0xffu) | (((s.y / s.w) & 0xffu) << 8) | (((s.z / s.w) & 0xffu) << 16) | (255u << 24);
		fb[i] = ((uint64_t)depth[i] << 32) | rgba;
	}
}

// ---- multi-GPU HQS: fold the packed per-pixel sums into the {R, G, B, count} plane, so that ranks can all-reduce(SUM) it ---------
__global__ __launch_bounds__(TPB) void r_unpack(RenderArgs a) {
	unsigned long long* packed = reinterpret_cast<unsigned long long*>(a.mom + a.lay.colour);
	uint4* sums = reinterpret_cast<uint4*>(a.mom + a.lay.sums);
	const uint32_t stride = gridDim.x * TPB;
	for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < a.numPixels; i += stride) {
		const unsigned long long pk = packed[i];
		if (pk == 0ull) continue;
		uint4 s = sums[i];
		s.x += (uint32_t)((pk >> 28) & 0x3fffu); s.y += (uint32_t)((pk >> 14) & 0x3fffu); s.z += (uint32_t)(pk & 0x3fffu); s.w += (uint32_t)(pk >> 42);
		sums[i] = s;
		packed[i] = 0ull;
	}
}

// ---- output: Stats (render.cu:1244-1252), EDL (:1255-1325, every full 16x16 tile), surface write (:1334-1343) ---------
// RESOLVE: the HQS resolve of r_resolve in the same pass (whole frames without debug lines: nothing but the resolve writes the
// framebuffer between the clear and this kernel).  A pixel resolves itself (and stores the word: the pre-EDL framebuffer stays what the
// reference's is); of its four neighbours EDL wants the depth only, and that is the depth plane's word whenever it is a normal number
// (its nearest sample passes its own 1 % test, so the pixel has a colour) or +inf (nothing landed: the cleared framebuffer word has the
// same high half); a denormal depth — whose own sample fails d < d * 1.01f — takes the long way.
template <bool RESOLVE>
__device__ __forceinline__ uint32_t resolved_depth_bits(const RenderArgs& a, const uint64_t* fb, int idx) {
	if (!RESOLVE) return (uint32_t)(fb[idx] >> 32);
	const uint32_t d = reinterpret_cast<const uint32_t*>(a.mom + a.lay.depth)[idx];
	if (d >= 0x00800000u) return d == 0x7f800000u ? (uint32_t)(fb[idx] >> 32) : d;
	const unsigned long long pk = reinterpret_cast<const unsigned long long*>(a.mom + a.lay.colour)[idx];
	const uint32_t count = reinterpret_cast<const uint4*>(a.mom + a.lay.sums)[idx].w + (uint32_t)(pk >> 42);
	return count != 0u ? d : (uint32_t)(fb[idx] >> 32);
}

// One workgroup per 64 x 16-pixel tile, four pixels per thread (rows ty, ty + 4, ty + 8, ty + 12: everything they read is requested
// before the first value is used).  EDL wants log2 of the depth of a pixel and of its four neighbours: every pixel's logarithm is taken
// ONCE, by its own thread, and passed on through LDS (plus a rim of 160 pixels around the tile).  The reference's neighbours are INDEX
// neighbours (i +- 1, i +- W, clamped to the frame: render.cu:1296-1300): the left neighbour of a row's first pixel is the last pixel of
// the row before; the rim is addressed the same way, and a pixel in the frame's last column or row that is not in its tile's last
// column or row reads that one neighbour directly.
static constexpr int OUT_TW = 64, OUT_TH = 16, OUT_PX = 4;
static_assert(OUT_TW * OUT_TH == (int)TPB * OUT_PX && 2 * OUT_TW + 2 * OUT_TH <= (int)TPB, "four pixels per thread; one rim pixel per thread");
template <bool RESOLVE>
__global__ __launch_bounds__(TPB) void r_output(RenderArgs a) {
	uint64_t* fb = reinterpret_cast<uint64_t*>(a.mom + FrameLayout::framebuffer);
	if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
		SimlodStats* s = a.stats;
		s->numVisibleNodes = min(*counter_at(a.mom, C_VISIBLE), SIMLOD_MAX_VISIBLE_NODES);
		s->numVisibleInner = *counter_at(a.mom, C_INNER);
		s->numVisibleLeaves = *counter_at(a.mom, C_LEAVES);
		s->numVisiblePoints = *counter_at(a.mom, C_POINTS);
		s->numVisibleVoxels = *counter_at(a.mom, C_VOXELS);
		s->frameID = a.frameCounter;
	}
	if (a.colorbuffer == nullptr) return;
	constexpr int PITCH = OUT_TW + 2, ROWS_PER_STEP = OUT_TH / OUT_PX;
	__shared__ float sh_log[(OUT_TH + 2) * PITCH];
	const int edlW = (a.W / 16) * 16, edlH = (a.H / 16) * 16;
	const int last = (int)a.numPixels - 1;
	const int tx = (int)threadIdx.x % OUT_TW, ty0 = (int)threadIdx.x / OUT_TW;
	const int x0 = (int)blockIdx.x * OUT_TW, y0 = (int)blockIdx.y * OUT_TH;
	const int x = x0 + tx;
	auto log_at = [&](int idx) -> float {                    // log2 of the depth EDL sees at pixel idx (clamped like the reference's index)
		idx = idx < 0 ? 0 : (idx > last ? last : idx);
		return __log2f(__uint_as_float(resolved_depth_bits<RESOLVE>(a, fb, idx)));
	};
	bool inside[OUT_PX];
	uint64_t enc[OUT_PX];
	unsigned long long pk[OUT_PX];
	uint4 sums[OUT_PX];
	uint32_t own[OUT_PX];
#pragma unroll
	for (int q = 0; q < OUT_PX; q++) {
		const int y = y0 + ty0 + q * ROWS_PER_STEP;
		inside[q] = x < a.W && y < a.H;
		const int i = inside[q] ? y * a.W + x : 0;
		enc[q] = fb[i];
		if (RESOLVE) { pk[q] = reinterpret_cast<const unsigned long long*>(a.mom + a.lay.colour)[i]; sums[q] = reinterpret_cast<const uint4*>(a.mom + a.lay.sums)[i]; own[q] = reinterpret_cast<const uint32_t*>(a.mom + a.lay.depth)[i]; }
	}
	float rim = 0.0f;
	int rimSlot = -1;
	if ((int)threadIdx.x < 2 * OUT_TW + 2 * OUT_TH) {       // the rim: the index neighbours of the tile's border pixels
		const int h = (int)threadIdx.x;
		int cx, cy, off, slot;                                // the border pixel (tile coordinates), its neighbour's index offset, the rim's LDS slot
		if (h < OUT_TW) { cx = h; cy = 0; off = -a.W; slot = cx + 1; }
		else if (h < 2 * OUT_TW) { cx = h - OUT_TW; cy = OUT_TH - 1; off = a.W; slot = (OUT_TH + 1) * PITCH + cx + 1; }
		else if (h < 2 * OUT_TW + OUT_TH) { cx = 0; cy = h - 2 * OUT_TW; off = -1; slot = (cy + 1) * PITCH; }
		else { cx = OUT_TW - 1; cy = h - 2 * OUT_TW - OUT_TH; off = 1; slot = (cy + 1) * PITCH + OUT_TW + 1; }
		if (x0 + cx < edlW && y0 + cy < edlH) { rim = log_at((y0 + cy) * a.W + x0 + cx + off); rimSlot = slot; }      // (only pixels EDL shades ask)
	}
#pragma unroll
	for (int q = 0; q < OUT_PX; q++) {
		if (!inside[q]) continue;
		if (RESOLVE) {                                                                          // as r_resolve
			uint4 s = sums[q];
			s.x += (uint32_t)((pk[q] >> 28) & 0x3fffu); s.y += (uint32_t)((pk[q] >> 14) & 0x3fffu); s.z += (uint32_t)(pk[q] & 0x3fffu); s.w += (uint32_t)(pk[q] >> 42);
			if (s.w != 0u) {
				const uint32_t rgba = ((s.x / s.w) & 0xffu) | (((s.y / s.w) & 0xffu) << 8) | (((s.z / s.w) & 0xffu) << 16) | (255u << 24);
				enc[q] = ((uint64_t)own[q] << 32) | rgba;
				fb[(y0 + ty0 + q * ROWS_PER_STEP) * a.W + x] = enc[q];
			}
		}
		sh_log[(ty0 + q * ROWS_PER_STEP + 1) * PITCH + tx + 1] = __log2f(__uint_as_float((uint32_t)(enc[q] >> 32)));
	}
	if (rimSlot >= 0) sh_log[rimSlot] = rim;
	__syncthreads();
#pragma unroll
	for (int q = 0; q < OUT_PX; q++) {
		if (!inside[q]) continue;
		const int ty = ty0 + q * ROWS_PER_STEP, y = y0 + ty, i = y * a.W + x;
		uint32_t color = (uint32_t)enc[q];
		if (x < edlW && y < edlH) {
			const float lp = sh_log[(ty + 1) * PITCH + tx + 1];
			// the four neighbours int(1.5 * sin/cos(k * 3.1415 / 2)) of render.cu:1296-1300: (0,+1), (+1,0), (0,-1), (-1,0)
			float ln[4];
			ln[0] = (y == a.H - 1 && ty != OUT_TH - 1) ? log_at(i + a.W) : sh_log[(ty + 2) * PITCH + tx + 1];
			ln[1] = (x == a.W - 1 && tx != OUT_TW - 1) ? log_at(i + 1) : sh_log[(ty + 1) * PITCH + tx + 2];
			ln[2] = sh_log[ty * PITCH + tx + 1];
			ln[3] = sh_log[(ty + 1) * PITCH + tx];
			float sum = 0.0f;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const float d = lp - ln[k];
				sum = sum + (d > 0.0f ? d : 0.0f);                 // max(NaN, 0) = 0
			}
			const float response = sum / 50.0f;
			const float shade = __expf((float)((double)(-response) * 300.0 * (double)0.4f));
			const uint32_t R = (uint32_t)(shade * (float)(color & 0xffu));
			const uint32_t G = (uint32_t)(shade * (float)((color >> 8) & 0xffu));
			const uint32_t B = (uint32_t)(shade * (float)((color >> 16) & 0xffu));
			color = R | (G << 8) | (B << 16) | (255u << 24);
		}
		a.colorbuffer[i] = color;
	}
}
