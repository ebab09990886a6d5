// render_draw.inc — the draw passes: the colour overrides, DrawCtx, the hot table, draw_sample / draw_wave / draw_staged / draw_item, tile_clear / tile_flush, r_draw.
__device__ __forceinline__ uint32_t lod_color(int level) {   // render.cu:38-59
	const uint32_t SPECTRAL[8] = {0x4f3ed5, 0x436df4, 0x61aefd, 0x8be0fe, 0x98f5e6, 0xa4ddab, 0xa5c266, 0xbd8832};
	int index = (int)((float)(8 - level) * 1.8f);
	index = index < 0 ? 0 : (index > 7 ? 7 : index);
	return SPECTRAL[index];
}

__device__ uint32_t node_color(const SimlodNode* n) {   // (getID() % 127) * 123456789, structures.cuh:118-141, render.cu:75
	uint64_t id = (uint64_t)(int64_t)(n->name[0] == 'r' ? 1 : 0);
	for (int i = 1; i <= 9; i++) id |= (uint64_t)(int64_t)(int32_t)(((uint32_t)((int)n->name[i] - '0')) << (3 * i));
	for (int i = 10; i <= 17; i++) id |= ((uint64_t)(int64_t)((int)n->name[i] - '0')) << (3 * i);
	id |= ((uint64_t)(int64_t)((int)n->name[18] - '0')) << 53;
	return (uint32_t)((id % 127ull) * 123456789ull);
}

enum { MODE_MIN64 = 0, MODE_DEPTH = 1, MODE_COLOR = 2 };

struct DrawCtx {
	simlod_float4 r0, r1, r3;
	float  width, height;
	double wlim, hlim;
	int    W, H, pointSize;
	uint32_t numPixels;
	uint64_t* fb;
	uint32_t* depth;
	unsigned long long* color;   // HQS colour sums, packed: B (14 bits) | G << 14 | R << 28 | count << 42
	unsigned long long* overflow;// 2 x u64 per pixel {R | G << 32, B | count << 32}: samples beyond the 64th of a pixel
	unsigned long long* tile;    // LDS, TILE*TILE entries: MIN64 the 64-bit minimum, COLOR the packed sums (DEPTH uses tile32)
	uint32_t* tile32;            // LDS, TILE*TILE entries: DEPTH the minimum of the depth bits
	int tileX, tileY;            // tile origin; tileX < 0: no tile
	int tileW, tileH;            // tile extent
	bool tileExact;              // COLOR: two words per pixel {R | G << 32, B | count << 32} instead of the packed word
	struct HotTable* hot;        // COLOR, packed tile: the pixels of the item that took more than 64 samples (LDS; nullptr in the other passes)
};

// The packed tile word of the colour pass holds 64 samples of a pixel (64 x 255 < 2^14); what comes beyond used to go to the pixel's words in the
// global {R, G, B, count} plane, two device-scope atomics per sample — on ONE address when the pixel is hot, and the memory system retires ~70 M
// same-address atomics a second: on the 500 M-point octree of BASELINE config 4 a handful of items with a few hot pixels each (ridges seen edge-on:
// thousands of samples on a pixel) took 100-300 us where their neighbours took 20, and set the colour pass's length (bird: 220 us against 64 for the
// depth pass; tools/raster_big.py).  Now the 65th sample onwards of a pixel goes into a small LDS table of the item's hot pixels — tile index ->
// exact 32-bit sums — which the flush adds to the global plane with two atomics per hot PIXEL.  No room in the table: the global words, as before.
static constexpr uint32_t HOT_CAP = 512, HOT_EMPTY = 0xffffffffu;
struct HotTable { uint32_t key[HOT_CAP]; unsigned long long rg[HOT_CAP], bc[HOT_CAP]; };
template <int MODE> struct HotStore { __device__ __forceinline__ HotTable* table() { return nullptr; } };
template <> struct HotStore<2> { HotTable t; __device__ __forceinline__ HotTable* table() { return &t; } };      // (MODE_COLOR)
__device__ __forceinline__ void beyond_64(const DrawCtx& c, uint32_t t, uint32_t pixel, unsigned long long r, unsigned long long g, unsigned long long b) {
	if (c.hot != nullptr) {
		uint32_t h = (t * 2654435761u) >> (32 - 9);
#pragma unroll 1
		for (int probe = 0; probe < 8; probe++) {
			uint32_t k = c.hot->key[h];
			if (k == HOT_EMPTY) { k = atomicCAS(&c.hot->key[h], HOT_EMPTY, t); if (k == HOT_EMPTY) k = t; }
			if (k == t) { atomicAdd(&c.hot->rg[h], r | (g << 32)); atomicAdd(&c.hot->bc[h], b | (1ull << 32)); return; }
			h = (h + 1u) & (HOT_CAP - 1u);
		}
	}
	atomicAdd(&c.overflow[2 * pixel + 0], r | (g << 32));
	atomicAdd(&c.overflow[2 * pixel + 1], b | (1ull << 32));
}

template <int MODE>
__device__ __forceinline__ void draw_sample(const DrawCtx& c, const float4 p, const uint32_t overrideColor, const bool useOverride, uint32_t& outside) {
	// render.cu:62-70 — transform, perspective divide, pixel in fp64
	const float cx = dot_row(c.r0, p.x, p.y, p.z);
	const float cy = dot_row(c.r1, p.x, p.y, p.z);
	const float depth = dot_row(c.r3, p.x, p.y, p.z);
	const float nx = cx / depth, ny = cy / depth;
	const double fx = ((double)nx * 0.5 + 0.5) * (double)c.width;
	const double fy = ((double)ny * 0.5 + 0.5) * (double)c.height;
	const int x = (int)fx, y = (int)fy;                 // v_cvt_i32_f64 saturates; NaN -> 0: rejected below either way
	if (!(x > 1 && (double)x < c.wlim)) return;
	if (!(y > 1 && (double)y < c.hlim)) return;
	if (MODE != MODE_MIN64 && !(depth > 0.0f)) return;   // render.cu:295, 371, 456, 558
	const uint32_t dbits = __float_as_uint(depth);
	const uint32_t color = useOverride ? overrideColor : __float_as_uint(p.w);
	for (int ox = 0; ox < c.pointSize; ox++)
	for (int oy = 0; oy < c.pointSize; oy++) {
		const int px = min(max(x + ox, 0), c.W), py = min(max(y + oy, 0), c.H);   // render.cu:91-92 clamps to W, not W-1
		const uint32_t pixel = (uint32_t)px + (uint32_t)c.W * (uint32_t)py;
		if (pixel >= c.numPixels) continue;                 // only reachable for pointSize >= 4 (out of bounds in the reference)
		if (c.tileX >= 0) {                                 // LDS-staged accumulation for nodes that are small on screen
			const unsigned tx = (unsigned)(px - c.tileX), ty = (unsigned)(py - c.tileY);
			if (tx < (unsigned)c.tileW && ty < (unsigned)c.tileH) {
				const unsigned t = tx + ty * (unsigned)c.tileW;
				if (MODE == MODE_MIN64) {
					const unsigned long long enc = ((unsigned long long)dbits << 32) | color;
					if (enc < c.tile[t]) atomicMin(&c.tile[t], enc);
				} else if (MODE == MODE_DEPTH) {
					if (dbits < c.tile32[t]) atomicMin(&c.tile32[t], dbits);
				} else if (depth < __uint_as_float(c.depth[pixel]) * 1.01f && c.tileExact) {
					atomicAdd(&c.tile[2 * t + 0], (unsigned long long)(color & 0xffu) | ((unsigned long long)((color >> 8) & 0xffu) << 32));
					atomicAdd(&c.tile[2 * t + 1], (unsigned long long)((color >> 16) & 0xffu) | (1ull << 32));
				} else if (depth < __uint_as_float(c.depth[pixel]) * 1.01f) {
					// the packed sums of the global plane, in LDS: B | G << 14 | R << 28 | count << 42; the 65th sample of a pixel
					// inside one item takes its addend back and goes to the global overflow plane (exact for any count)
					const unsigned long long r = color & 0xffu, g = (color >> 8) & 0xffu, b = (color >> 16) & 0xffu;
					const unsigned long long pk = b | (g << 14) | (r << 28) | (1ull << 42);
					const unsigned long long old = atomicAdd(&c.tile[t], pk);
					if ((old >> 42) >= 64ull) { atomicAdd(&c.tile[t], 0ull - pk); beyond_64(c, t, pixel, r, g, b); }
				}
				continue;
			}
		}
		outside += 1u;
		if (MODE == MODE_MIN64) {
			const unsigned long long enc = ((unsigned long long)dbits << 32) | color;
			if (enc < c.fb[pixel]) atomicMin(reinterpret_cast<unsigned long long*>(&c.fb[pixel]), enc);   // render.cu:95-100
		} else if (MODE == MODE_DEPTH) {
			if (dbits < c.depth[pixel]) atomicMin(&c.depth[pixel], dbits);                                // render.cu:304-308
		} else {
			const float fbDepth = __uint_as_float(c.depth[pixel]);
			if (depth < fbDepth * 1.01f) {                                                                 // render.cu:485-493
				// ONE 64-bit atomic per accepted sample: the sums of R, G, B and the count share a word (14 + 14 + 14 + 22 bits).
				// The first 64 samples of a pixel fit without carry (64 * 255 < 2^14); a sample that finds count >= 64 takes its
				// addend back and goes to the 32-bit-per-channel overflow plane.  All arithmetic is modular, so transient carries
				// of samples that are about to retract do not disturb the final sums (at most 64 samples ever stay).
				const unsigned long long r = color & 0xffu, g = (color >> 8) & 0xffu, b = (color >> 16) & 0xffu;
				const unsigned long long pk = b | (g << 14) | (r << 28) | (1ull << 42);
				const unsigned long long old = atomicAdd(&c.color[pixel], pk);
				if ((old >> 42) >= 64ull) {
					atomicAdd(&c.color[pixel], 0ull - pk);
					atomicAdd(&c.overflow[2 * pixel + 0], r | (g << 32));
					atomicAdd(&c.overflow[2 * pixel + 1], b | (1ull << 32));
				}
			}
		}
	}
}

// One sample per lane, the whole wave in step (point size 1, tile in use): when every lane that hits the tile hits the SAME pixel —
// the rule in BASELINE config 5, where thousands of samples of a node fall on one pixel — the wave reduces its values with
// cross-lane shuffles and ONE lane issues the LDS atomic (64 same-address LDS atomics serialise).  Otherwise every lane issues its
// own, as draw_sample does.  Same test-before-atomic rules, same values: the tile ends up identical.
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
	for (int o = 32; o > 0; o >>= 1) {
		const unsigned long long w = ((unsigned long long)__shfl_xor((uint32_t)(v >> 32), o, 64) << 32) | __shfl_xor((uint32_t)v, o, 64);
		v = w < v ? w : v;
	}
	return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
	for (int o = 32; o > 0; o >>= 1) { const uint32_t w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
	return v;
}

template <int MODE>
__device__ __forceinline__ void draw_wave(const DrawCtx& c, const float4 p, const bool have, const uint32_t overrideColor, const bool useOverride, uint32_t& outside) {
	const float cx = dot_row(c.r0, p.x, p.y, p.z);
	const float cy = dot_row(c.r1, p.x, p.y, p.z);
	const float depth = dot_row(c.r3, p.x, p.y, p.z);
	const float nx = cx / depth, ny = cy / depth;
	const double fx = ((double)nx * 0.5 + 0.5) * (double)c.width;
	const double fy = ((double)ny * 0.5 + 0.5) * (double)c.height;
	const int x = (int)fx, y = (int)fy;
	bool valid = have && (x > 1 && (double)x < c.wlim) && (y > 1 && (double)y < c.hlim);
	if (MODE != MODE_MIN64) valid = valid && depth > 0.0f;
	const uint32_t dbits = __float_as_uint(depth);
	const uint32_t color = useOverride ? overrideColor : __float_as_uint(p.w);
	const int px = min(max(x, 0), c.W), py = min(max(y, 0), c.H);
	const uint32_t pixel = (uint32_t)px + (uint32_t)c.W * (uint32_t)py;
	valid = valid && pixel < c.numPixels;
	const unsigned tx = (unsigned)(px - c.tileX), ty = (unsigned)(py - c.tileY);
	const bool inTile = valid && tx < (unsigned)c.tileW && ty < (unsigned)c.tileH;
	const unsigned t = tx + ty * (unsigned)c.tileW;
	bool accept = true;
	if (MODE == MODE_COLOR) accept = valid && depth < __uint_as_float(c.depth[valid ? pixel : 0u]) * 1.01f;
	const bool mine = inTile && accept;
	const unsigned long long mask = __ballot(mine);
	bool uniform = false;
	unsigned t0 = 0;
	if (mask != 0ull && (MODE != MODE_COLOR || c.tileExact)) {
		t0 = (unsigned)__shfl((int)t, (int)(__ffsll((long long)mask) - 1), 64);
		uniform = __popcll(mask) >= 8 && __ballot(mine && t == t0) == mask;
	}
	if (uniform) {                                   // wave-uniform branch: every lane takes part in the shuffles
		const bool leader = (unsigned)lane_id() == (unsigned)(__ffsll((long long)mask) - 1);
		if (MODE == MODE_MIN64) {
			const unsigned long long v = wave_min_u64(mine ? (((unsigned long long)dbits << 32) | color) : ~0ull);
			if (leader && v < c.tile[t0]) atomicMin(&c.tile[t0], v);
		} else if (MODE == MODE_DEPTH) {
			const uint32_t v = wave_min_u32(mine ? dbits : 0xffffffffu);
			if (leader && v < c.tile32[t0]) atomicMin(&c.tile32[t0], v);
		} else {
			uint32_t rg = mine ? ((color & 0xffu) | (((color >> 8) & 0xffu) << 16)) : 0u, bc = mine ? (((color >> 16) & 0xffu) | (1u << 16)) : 0u;
			for (int o = 32; o > 0; o >>= 1) { rg += __shfl_xor(rg, o, 64); bc += __shfl_xor(bc, o, 64); }   // 64 x 255 < 2^16: no carry between the halves
			if (leader) {
				atomicAdd(&c.tile[2 * t0 + 0], (unsigned long long)(rg & 0xffffu) | ((unsigned long long)(rg >> 16) << 32));
				atomicAdd(&c.tile[2 * t0 + 1], (unsigned long long)(bc & 0xffffu) | ((unsigned long long)(bc >> 16) << 32));
			}
		}
	} else if (mine) {
		if (MODE == MODE_MIN64) {
			const unsigned long long enc = ((unsigned long long)dbits << 32) | color;
			if (enc < c.tile[t]) atomicMin(&c.tile[t], enc);
		} else if (MODE == MODE_DEPTH) {
			if (dbits < c.tile32[t]) atomicMin(&c.tile32[t], dbits);
		} else if (c.tileExact) {
			atomicAdd(&c.tile[2 * t + 0], (unsigned long long)(color & 0xffu) | ((unsigned long long)((color >> 8) & 0xffu) << 32));
			atomicAdd(&c.tile[2 * t + 1], (unsigned long long)((color >> 16) & 0xffu) | (1ull << 32));
		} else {
			const unsigned long long r = color & 0xffu, g = (color >> 8) & 0xffu, b = (color >> 16) & 0xffu;
			const unsigned long long pk = b | (g << 14) | (r << 28) | (1ull << 42);
			const unsigned long long old = atomicAdd(&c.tile[t], pk);
			if ((old >> 42) >= 64ull) { atomicAdd(&c.tile[t], 0ull - pk); beyond_64(c, t, pixel, r, g, b); }
		}
	}
	if (valid && !inTile) {                          // outside the tile: the global path of draw_sample
		outside += 1u;
		if (MODE == MODE_MIN64) {
			const unsigned long long enc = ((unsigned long long)dbits << 32) | color;
			if (enc < c.fb[pixel]) atomicMin(reinterpret_cast<unsigned long long*>(&c.fb[pixel]), enc);
		} else if (MODE == MODE_DEPTH) {
			if (dbits < c.depth[pixel]) atomicMin(&c.depth[pixel], dbits);
		} else if (accept) {
			const unsigned long long r = color & 0xffu, g = (color >> 8) & 0xffu, b = (color >> 16) & 0xffu;
			const unsigned long long pk = b | (g << 14) | (r << 28) | (1ull << 42);
			const unsigned long long old = atomicAdd(&c.color[pixel], pk);
			if ((old >> 42) >= 64ull) {
				atomicAdd(&c.color[pixel], 0ull - pk);
				atomicAdd(&c.overflow[2 * pixel + 0], r | (g << 32));
				atomicAdd(&c.overflow[2 * pixel + 1], b | (1ull << 32));
			}
		}
	}
}

// Point size 1, tile in use — the common case — DU samples per lane in three stages, so that nothing in the loop waits for anything:
//   1. project all DU samples (pure arithmetic; HQS colour: the DU depth-buffer loads go out together),
//   2. tiles of a few pixels only (BASELINE config 5: thousands of samples of a node on one pixel): draw_wave, which merges a wave's
//      samples with shuffles when they all hit the same pixel,
//   3. otherwise every lane issues its LDS atomics straight away — no read-compare first: an LDS atomic that does not change the word
//      costs what the read would, and returns nothing to wait for.  min and add commute: the tile ends up identical.
template <int MODE, uint32_t DU>
__device__ __forceinline__ void draw_staged(const DrawCtx& c, const float4 (&p)[DU], const bool (&have)[DU], const uint32_t overrideColor, const bool useOverride, uint32_t& outside) {
	uint32_t pixel[DU], t[DU], dbits[DU], color[DU];
	float depth[DU];
	bool valid[DU], inTile[DU], accept[DU];
#pragma unroll
	for (uint32_t u = 0; u < DU; u++) {
		const float cx = dot_row(c.r0, p[u].x, p[u].y, p[u].z);
		const float cy = dot_row(c.r1, p[u].x, p[u].y, p[u].z);
		depth[u] = dot_row(c.r3, p[u].x, p[u].y, p[u].z);
		const float nx = cx / depth[u], ny = cy / depth[u];
		const double fx = ((double)nx * 0.5 + 0.5) * (double)c.width;
		const double fy = ((double)ny * 0.5 + 0.5) * (double)c.height;
		const int x = (int)fx, y = (int)fy;
		valid[u] = have[u] && (x > 1 && (double)x < c.wlim) && (y > 1 && (double)y < c.hlim);
		if (MODE != MODE_MIN64) valid[u] = valid[u] && depth[u] > 0.0f;
		dbits[u] = __float_as_uint(depth[u]);
		color[u] = useOverride ? overrideColor : __float_as_uint(p[u].w);
		const int px = min(max(x, 0), c.W), py = min(max(y, 0), c.H);
		pixel[u] = (uint32_t)px + (uint32_t)c.W * (uint32_t)py;
		valid[u] = valid[u] && pixel[u] < c.numPixels;
		const unsigned tx = (unsigned)(px - c.tileX), ty = (unsigned)(py - c.tileY);
		inTile[u] = valid[u] && tx < (unsigned)c.tileW && ty < (unsigned)c.tileH;
		t[u] = tx + ty * (unsigned)c.tileW;
		accept[u] = true;
	}
	uint32_t ref[DU];
	if (MODE == MODE_COLOR) {
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) ref[u] = c.depth[valid[u] ? pixel[u] : 0u];
	}
	if (MODE == MODE_COLOR) {
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) accept[u] = valid[u] && depth[u] < __uint_as_float(ref[u]) * 1.01f;          // render.cu:485-493
	}
#pragma unroll
	for (uint32_t u = 0; u < DU; u++) {
		if (inTile[u] && accept[u]) {
			if (MODE == MODE_MIN64) atomicMin(&c.tile[t[u]], ((unsigned long long)dbits[u] << 32) | color[u]);
			else if (MODE == MODE_DEPTH) atomicMin(&c.tile32[t[u]], dbits[u]);
			else if (c.tileExact) {
				atomicAdd(&c.tile[2 * t[u] + 0], (unsigned long long)(color[u] & 0xffu) | ((unsigned long long)((color[u] >> 8) & 0xffu) << 32));
				atomicAdd(&c.tile[2 * t[u] + 1], (unsigned long long)((color[u] >> 16) & 0xffu) | (1ull << 32));
			} else {
				const unsigned long long r = color[u] & 0xffu, g = (color[u] >> 8) & 0xffu, b = (color[u] >> 16) & 0xffu;
				const unsigned long long pk = b | (g << 14) | (r << 28) | (1ull << 42);
				const unsigned long long old = atomicAdd(&c.tile[t[u]], pk);
				if ((old >> 42) >= 64ull) { atomicAdd(&c.tile[t[u]], 0ull - pk); beyond_64(c, t[u], pixel[u], r, g, b); }
			}
		}
	}
#pragma unroll
	for (uint32_t u = 0; u < DU; u++) {
		if (valid[u] && !inTile[u]) {                  // outside the tile: the global path of draw_sample
			outside += 1u;
			// No read-compare first (render.cu:95-100, 304-308 test before they exchange): a node close to the camera is larger than any tile, a
			// sixth of the close-up frame's samples come this way, and a wave that waits for a framebuffer read per sample draws at half the speed
			// (measured: r_draw 157 us with the reads — in flight together or not —, against 69 us for a frame whose samples stay in their
			// tiles).  The atomic returns nothing to wait for; min is idempotent: the framebuffer ends up identical.
			if (MODE == MODE_MIN64) atomicMin(reinterpret_cast<unsigned long long*>(&c.fb[pixel[u]]), ((unsigned long long)dbits[u] << 32) | color[u]);
			else if (MODE == MODE_DEPTH) atomicMin(&c.depth[pixel[u]], dbits[u]);
			else if (accept[u]) {
				const unsigned long long r = color[u] & 0xffu, g = (color[u] >> 8) & 0xffu, b = (color[u] >> 16) & 0xffu;
				const unsigned long long pk = b | (g << 14) | (r << 28) | (1ull << 42);
				const unsigned long long old = atomicAdd(&c.color[pixel[u]], pk);
				if ((old >> 42) >= 64ull) {
					atomicAdd(&c.color[pixel[u]], 0ull - pk);
					atomicAdd(&c.overflow[2 * pixel[u] + 0], r | (g << 32));
					atomicAdd(&c.overflow[2 * pixel[u] + 1], b | (1ull << 32));
				}
			}
		}
	}
}

template <int MODE, typename POLICY>
__device__ __forceinline__ void draw_item(const DrawCtx& c, const SimlodChunk* const* dir, uint32_t count, uint32_t overrideColor, bool useOverride, uint32_t& outside, const POLICY& clip) {
	// render.cu:106-159: chunk i holds samples [1000 i, 1000 i + 1000); the chunk addresses come from the frame's directory (staged in LDS).
	// Four samples per thread are loaded before the first is drawn: the loads overlap instead of queueing behind the atomics.
	constexpr uint32_t DU = 4;
	// (an item without a tile — a node that reaches behind the camera — is staged like the others: all its samples take the global path,
	// DU of a lane in flight together; sample by sample such an item took 60-150 us and was the frame's makespan in the close-up preset)
	const bool wave = c.pointSize == 1;
	const bool merge = c.tileX >= 0 && c.tileW * c.tileH <= 64;     // a node a few pixels across: most lanes of a wave hit the same pixel
	for (uint32_t base = 0; base < count; base += DTPB * DU) {          // uniform trip count: the whole wave stays in step
		float4 p[DU];
		bool have[DU];
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) {
			const uint32_t s = base + u * DTPB + threadIdx.x;
			have[u] = s < count;
			p[u] = have[u] ? reinterpret_cast<const float4*>(dir[s / SIMLOD_POINTS_PER_CHUNK]->points)[s % SIMLOD_POINTS_PER_CHUNK] : make_float4(0, 0, 0, 0);
		}
		clip.test(p, have);                                                 // (the three draw paths below see what the frame's clip left)
		if (wave && merge) {
#pragma unroll
			for (uint32_t u = 0; u < DU; u++) draw_wave<MODE>(c, p[u], have[u], overrideColor, useOverride, outside);
		} else if (wave) {
			draw_staged<MODE, DU>(c, p, have, overrideColor, useOverride, outside);
		} else {
#pragma unroll
			for (uint32_t u = 0; u < DU; u++) if (have[u]) draw_sample<MODE>(c, p[u], overrideColor, useOverride, outside);
		}
	}
}

// (render_bins.inc)
template <int MODE, typename POLICY>
__device__ __forceinline__ void bin_item(const DrawCtx& c, const RenderArgs& a, uint32_t* lds, const SimlodChunk* const* dir, uint32_t count, uint32_t overrideColor, bool useOverride,
                                         uint32_t& outside, const POLICY& clip);

template <int MODE>
__device__ __forceinline__ void tile_clear(const DrawCtx& c) {
	const int words = c.tileW * c.tileH * (MODE == MODE_COLOR && c.tileExact ? 2 : 1);
	for (int t = threadIdx.x; t < words; t += DTPB) {
		if (MODE == MODE_DEPTH) c.tile32[t] = 0xffffffffu; else c.tile[t] = MODE == MODE_COLOR ? 0ull : ~0ull;
	}
	if (MODE == MODE_COLOR && c.hot != nullptr && !c.tileExact)
		for (uint32_t h = threadIdx.x; h < HOT_CAP; h += DTPB) { c.hot->key[h] = HOT_EMPTY; c.hot->rg[h] = 0ull; c.hot->bc[h] = 0ull; }
}

// One global atomic per TOUCHED pixel of the tile.
template <int MODE>
__device__ __forceinline__ void tile_flush(const DrawCtx& c) {
	for (int t = threadIdx.x; t < c.tileW * c.tileH; t += DTPB) {
		const int px = c.tileX + (t % c.tileW), py = c.tileY + (t / c.tileW);
		if (px > c.W || py > c.H) continue;
		const uint32_t pixel = (uint32_t)px + (uint32_t)c.W * (uint32_t)py;
		if (pixel >= c.numPixels) continue;
		if (MODE == MODE_MIN64) {
			// no read-compare first: a thread flushes up to 16 pixels, and 16 dependent framebuffer reads were most of an item's time;
			// the atomic returns nothing to wait for, and a node's pixels are mostly its own, so few of them would have been spared
			const unsigned long long v = c.tile[t];
			if (v != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(&c.fb[pixel]), v);
		} else if (MODE == MODE_DEPTH) {
			const uint32_t v = c.tile32[t];
			if (v != 0xffffffffu) atomicMin(&c.depth[pixel], v);
		} else if (c.tileExact) {
			const unsigned long long rg = c.tile[2 * t], bc = c.tile[2 * t + 1];
			if ((bc >> 32) != 0ull) { atomicAdd(&c.overflow[2 * pixel + 0], rg); atomicAdd(&c.overflow[2 * pixel + 1], bc); }
		} else {
			const unsigned long long pk = c.tile[t];
			if (pk != 0ull) {                                 // exact: resolve adds the packed plane and the {R, G, B, count} plane
				atomicAdd(&c.overflow[2 * pixel + 0], ((pk >> 28) & 0x3fffull) | (((pk >> 14) & 0x3fffull) << 32));
				atomicAdd(&c.overflow[2 * pixel + 1], (pk & 0x3fffull) | ((pk >> 42) << 32));
			}
		}
	}
	if (MODE == MODE_COLOR && c.hot != nullptr && !c.tileExact) {      // the item's hot pixels: what they took beyond their 64th sample
		for (uint32_t h = threadIdx.x; h < HOT_CAP; h += DTPB) {
			const uint32_t t = c.hot->key[h];
			if (t == HOT_EMPTY) continue;
			const uint32_t pixel = (uint32_t)(c.tileX + (int)(t % (uint32_t)c.tileW)) + (uint32_t)c.W * (uint32_t)(c.tileY + (int)(t / (uint32_t)c.tileW));
			atomicAdd(&c.overflow[2 * pixel + 0], c.hot->rg[h]);
			atomicAdd(&c.overflow[2 * pixel + 1], c.hot->bc[h]);
		}
	}
}

// (one definition for both kinds of frame, as r_visible: r_draw<MODE>(a) and r_draw<MODE>(a, k) under a clip, the planes in LDS beside the tile and the hot table)
template <int MODE, typename... CLIP>
__global__ __launch_bounds__(DTPB) void r_draw(RenderArgs a, CLIP... k) {
	ClipStore<sizeof...(CLIP) != 0> sh_clip;
	auto clip = sh_clip.policy(k...);
	if (MODE == MODE_DEPTH) clear_colour_planes(a);
	if (!a.showPoints) return;
	__shared__ uint32_t sh_idx;
	__shared__ const SimlodChunk* sh_dir[ITEM_CHUNKS];
	constexpr uint32_t BIN_WORDS = 2 * BIN_MAX_TILES + 32;                                  // bin_item's counters, in the tile's place
	__shared__ unsigned long long sh_tile[MODE == MODE_DEPTH ? (TILE * TILE > BIN_WORDS ? TILE * TILE : BIN_WORDS) / 2 : TILE * TILE];
	__shared__ HotStore<MODE> sh_hot;
	DrawCtx c;
	c.hot = sh_hot.table();
	c.tile = sh_tile; c.tile32 = reinterpret_cast<uint32_t*>(sh_tile); c.tileX = -1; c.tileY = -1; c.tileW = TILE; c.tileH = TILE; c.tileExact = false;
	c.r0 = a.transform.rows[0]; c.r1 = a.transform.rows[1]; c.r3 = a.transform.rows[3];
	c.width = a.width; c.height = a.height;
	c.wlim = (double)a.width - 2.0; c.hlim = (double)a.height - 2.0;
	c.W = a.W; c.H = a.H; c.pointSize = a.pointSize; c.numPixels = a.numPixels;
	c.fb = reinterpret_cast<uint64_t*>(a.mom + FrameLayout::framebuffer);
	c.depth = reinterpret_cast<uint32_t*>(a.mom + a.lay.depth);
	c.color = reinterpret_cast<unsigned long long*>(a.mom + a.lay.colour);
	c.overflow = reinterpret_cast<unsigned long long*>(a.mom + a.lay.sums);
	uint32_t* work = work_words(a.mom, a.lay);
	uint32_t* cursor = work + W_CURSOR0 + MODE;
	if (MODE != MODE_COLOR && blockIdx.x == 0 && threadIdx.x == 0 && a.binFeedback != nullptr) *a.binFeedback = work[W_SORTING_NODES];
	uint32_t classEnd[ITEM_CLASSES];                                                       // position q of the cursor: class c while q < classEnd[c]
	for (int cl = 0; cl < ITEM_CLASSES; cl++) classEnd[cl] = (cl > 0 ? classEnd[cl - 1] : 0u) + min(work[W_ITEMS0 + cl], a.itemCap);
	const uint32_t numItems = classEnd[ITEM_CLASSES - 1];
	const DrawItem* items = reinterpret_cast<const DrawItem*>(a.mom + a.lay.items);
	const SimlodNode* visible = reinterpret_cast<const SimlodNode*>(a.mom + FrameLayout::visible);
	// Workgroup-level queue of draw items.  The first item of a workgroup is its own index, the following ones come from a shared
	// cursor that starts behind the statically assigned range.
	uint32_t idx = blockIdx.x;
	uint32_t outside = 0;                                                                   // samples of this thread that went down the global-atomic path
	while (idx < numItems) {
		uint32_t cl = 0;
		while (idx >= classEnd[cl]) cl++;
		const uint64_t itemAt = (uint64_t)cl * a.itemCap + (idx - (cl > 0u ? classEnd[cl - 1u] : 0u));
		const DrawItem it = items[itemAt];
		const uint64_t itemStart = SIMLOD_MEASURE != 0 && threadIdx.x == 0 ? wall_clock64() : 0ull;
		uint32_t overrideColor = 0; bool useOverride = false;
		if (MODE != MODE_DEPTH && (a.colorByNode || a.colorByLOD)) {
			const SimlodNode* node = visible + it.visibleIdx;
			overrideColor = a.colorByNode ? node_color(node) : lod_color((int)node->level);
			useOverride = true;
		}
		if constexpr (decltype(clip)::ON) {
			// the class of the item's node, from its visible record: every lane computes the same, and the branches on it are scalar
			const SimlodNode* node = visible + min(it.visibleIdx, VISIBLE_NODES - 1u);
			uint32_t act = __builtin_amdgcn_readfirstlane(clip.action_of(node->level, node->X, node->Y, node->Z));
			if (MODE == MODE_DEPTH && (act == CLIP_ACT_COLOUR_PASSING || act == CLIP_ACT_COLOUR_ALL)) act = CLIP_ACT_NONE;      // (the depth pass reads no colour)
			if (act == CLIP_ACT_COLOUR_ALL) { overrideColor = clip.k.color; useOverride = true; }
			clip.action = act;
		}
		const bool binned = it.tileX == TILE_BINNED;
		c.tileX = binned ? -1 : it.tileX; c.tileY = it.tileY; c.tileW = (int)(it.tileWH & 0xffffu); c.tileH = (int)(it.tileWH >> 16);
		if (it.tileX < 0) { c.tileW = 0; c.tileH = 0; }                                       // no tile: nothing is inside it
		c.tileExact = c.tileW * c.tileH <= TILE_EXACT_AREA;
		bool gap = false;
		if (threadIdx.x < ITEM_CHUNKS && threadIdx.x * SIMLOD_POINTS_PER_CHUNK < it.samples) {
			const uint64_t where = (uint64_t)it.chunks;           // the frame's chunk directory, or (bit 0) a row of the builder's packed chunk table from slot (bits 1..7) on
			const SimlodChunk* ch = (where & 1ull) != 0ull ? leaf_row_get(reinterpret_cast<const uint8_t*>(where & ~255ull), a.leafTablePers, 0, (uint32_t)((where >> 1) & 127ull) + threadIdx.x)
			                                               : it.chunks[threadIdx.x];
			sh_dir[threadIdx.x] = ch;
			gap = ch == nullptr;
		}
		if (it.tileX >= 0) tile_clear<MODE>(c);
		uint32_t samples = it.samples;
		if (__syncthreads_or(gap ? 1 : 0)) {             // a table row with a gap (never seen; rows are complete while their stamp is valid): draw what precedes it
			uint32_t whole = 0;
			while (whole < ITEM_CHUNKS && whole * SIMLOD_POINTS_PER_CHUNK < it.samples && sh_dir[whole] != nullptr) whole++;
			samples = min(samples, whole * SIMLOD_POINTS_PER_CHUNK);
		}
		if (binned) bin_item<MODE>(c, a, reinterpret_cast<uint32_t*>(sh_tile), sh_dir, samples, overrideColor, useOverride, outside, clip);
		else draw_item<MODE>(c, sh_dir, samples, overrideColor, useOverride, outside, clip);
		if (it.tileX >= 0) { __syncthreads(); tile_flush<MODE>(c); }
		__syncthreads();
		if (SIMLOD_MEASURE != 0 && threadIdx.x == 0) const_cast<DrawItem*>(items)[itemAt].took = (uint32_t)(wall_clock64() - itemStart);
		if (threadIdx.x == 0) sh_idx = gridDim.x + atomicAdd(cursor, 1u);
		__syncthreads();
		idx = sh_idx;
	}
	if (MODE != MODE_COLOR) {                                                               // (the colour pass draws the same samples again)
		outside = wave_sum_u32(outside);
		if (lane_id() == 0 && outside != 0u) atomicAdd(counter_at(a.mom, C_OUTSIDE_TILES), outside);
	}
}
