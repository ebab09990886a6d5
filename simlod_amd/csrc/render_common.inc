// render_common.inc — what every pass of the rasteriser shares: RenderArgs, DrawItem, BinSeg, the tile and bin constants, the probe macros, dot_row, the DPP
// wave sums, the clears with the frame-ready handshake (clear_frame, clear_colour_planes, clear_counters, wait_frame_ready), and the clip policies
// (NoClip, Clip, ClipStore).
static constexpr uint32_t TPB = 256;

struct RenderArgs {
	uint8_t*     mom;
	SimlodNode*  nodes;
	SimlodStats* stats;
	uint32_t*    colorbuffer;
	uint64_t*    frameStart;
	SimlodMat4   transform, transformUpdate;
	float        width, height, cubeSize, minx, miny, minz, minNodeSize;
	int32_t      W, H, pointSize;
	uint32_t     numPixels, nodeCapacity, frameCounter;
	uint8_t      showPoints, colorByNode, colorByLOD, hqs;
	FrameLayout  lay;                               // where everything lies in `mom` for this frame (render_layout.hpp)
	uint32_t     itemCap, useTiles, launchSeq;
	uint32_t     useBins, binPoolCap, binMinArea, binsPossible;   // screen bins of the samples that leave their item's tile (r_overflow); binPoolCap: entries in the pool
	uint32_t*    binFeedback;                       // page-locked: the frame's first draw pass stores here how many nodes sort, or would (launch_render)
	// the builder's leaf chunk table (simlod_internal.hpp LeafTableRef), or table == nullptr: r_visible walks every list
	const uint8_t* leafTable;                          // packed rows (simlod_internal.hpp leaf_row_get), offsets into leafTablePers
	const uint8_t* leafTablePers;
	const uint32_t* leafTableMagic;
	const uint32_t* leafTableBatch;
	const uint64_t* leafTableNodes;
	const uint64_t* leafTableSig;
	uint32_t     leafTableMagicValue, leafTableSlots, leafTableRows;
};

// Draw items are queued by size, biggest first (longest-processing-time order): the draw workgroups take items from one shared
// cursor, and a 64 000-sample item taken last would keep one CU busy long after the others ran dry (measured on the bench frame:
// average workgroup 55 us, slowest 92 us with the items in emission order).  Class of an item = its chunk count: > 16, > 8, > 4, rest;
// class c has its own array (itemCap entries) and counter, position q of the cursor maps to the classes in order.
__device__ __forceinline__ uint32_t item_class(uint32_t chunks) { return chunks > 16u ? 0u : (chunks > 8u ? 1u : (chunks > 4u ? 2u : 3u)); }
// A draw item = up to 32 consecutive chunks (32 000 samples) of one visible node's list (a full leaf is two items; 64 per item: 5 % slower
// on the bench frame, the biggest item is a fifth of a workgroup's whole share; 16: 10 % slower, twice the tile clears and flushes).
// ONE workgroup draws an item, accumulating in a 128 x 128-pixel LDS tile laid over the node's screen box: the LOD rule draws a node
// while its box spans 64..128 pixels (render.cu:893-901), so nearly every sample of a node lands in the tile, pixels that several
// samples of the node hit (five per pixel on average for a full leaf) cost LDS atomics, and the framebuffer sees one global atomic per
// TOUCHED pixel and item instead of one per sample.  Samples outside the tile take the global path.
static constexpr uint32_t ITEM_CHUNKS = 32;
static constexpr uint32_t DTPB = 1024;              // draw workgroup: 16 waves share one tile (128 KB of LDS: one workgroup per CU)

struct DrawItem {
	const SimlodChunk* const* chunks;               // the item's chunk addresses: in the frame's chunk directory, or straight in a row of the builder's chunk table
	uint32_t samples, visibleIdx;
	int32_t  tileX, tileY;                          // origin of the LDS tile, or tileX < 0: no tile
	uint32_t tileWH;                                // its extent, width | height << 16: the node's screen box, at most TILE x TILE
	uint32_t took;                                  // measurement aid (tools/raster_items.py): how long the item's workgroup took over it in the frame's last draw pass, in 10 ns
};
static constexpr int TILE = 128;
// Screen bins.  A node close to the camera is larger on screen than any LDS tile and its samples are thinly spread (fewer than one per
// pixel): each of them used to be one device-scope atomic on the framebuffer, and ~25 G scattered 64-bit atomics per second is all the
// memory system does (measured: 2 M such samples = 80 us whatever the number of CUs that issue them — the whole close-up frame took twice
// the time of the bird's-eye frame with fewer samples).  The draw items of such a node do not rasterise: they SORT — every sample becomes a
// 16-byte entry in the queue of the 64 x 64-pixel screen bin it falls into (two passes over the item's samples: count per tile in LDS,
// ONE reservation per item and tile, then store) — and r_overflow gives every screen tile one workgroup that rasterises the tile's queue in
// LDS and merges it into the plane with plain loads and stores (the tile's pixels are nobody else's in that kernel).
static constexpr int TILE_BINNED = -2;                     // DrawItem::tileX of such an item
static constexpr uint32_t BIN_ITEM_CHUNKS = 8;            // a sorting item: 8000 samples, 8 per thread — kept in registers between the count and the store (16: r_draw<MODE_MIN64> spills)
static constexpr uint32_t OVERFLOW_STRIDE = 10007;         // prime, larger than any bin count
struct BinSeg { uint32_t base, count; };
static constexpr uint32_t OTPB = 1024;                     // r_overflow's workgroup (512: 31 us for the close-up's bins, 256: 55; 1024: 25)
static constexpr int TILE_EXACT_AREA = TILE * TILE / 2;   // HQS colour: tiles up to this area keep two 64-bit words per pixel (exact 32-bit sums)

#ifdef VAR_PROBE
#define R_PROBE_MAX(k) do { if (lane_id() == 0) reinterpret_cast<unsigned long long*>(a.mom + FrameLayout::probe)[(k) * 8192u + blockIdx.x * (TPB / 64u) + threadIdx.x / 64u] = (unsigned long long)wall_clock64(); } while (0)
#define R_PROBE_MIN(k) R_PROBE_MAX(k)
#else
#define R_PROBE_MAX(k) do {} while (0)
#define R_PROBE_MIN(k) do {} while (0)
#endif

__device__ __forceinline__ float dot_row(const simlod_float4& r, float x, float y, float z) {
	float s = r.x * x;
	s = s + r.y * y;
	s = s + r.z * z;
	s = s + r.w * 1.0f;
	return s;
}

// Wave-wide sums by DPP (row shifts inside the 16-lane rows, then the rows' totals broadcast from lanes 15 and 31): six VALU operations.
// Through ds_bpermute (__shfl_up / __shfl_xor) every step is an LDS round trip; r_visible's dozen scans in a row were 2.5 us of its 19.
__device__ __forceinline__ uint32_t wave_inclusive_u32(uint32_t v) {
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);      // row_shr:1
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);      // row_shr:2
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);      // row_shr:4
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);      // row_shr:8
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
	return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_u32(v), 63); }
__device__ __forceinline__ uint32_t wave_prefix_u32(uint32_t v) { return wave_inclusive_u32(v) - v; }      // exclusive prefix sum over the wave
__device__ __forceinline__ uint32_t wave_prefix_u32(uint32_t v, uint32_t& total) {                          // ... and the wave's total
	const uint32_t incl = wave_inclusive_u32(v);
	total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
	return incl - v;
}

// ---- clear (render.cu:1126-1131, 233-241) ---------------------------------------------------------------------
// Part of r_visible's launch: the planes are cleared by ALL its workgroups (a thousand, of which the octree's nodes keep a few dozen busy
// for three dependent memory round trips), the frame's counters by thread 0 of workgroup 0, which then publishes the launch's
// sequence number; a wave reads that word before its first reservation (by then it has long been there).
__device__ __forceinline__ void wait_frame_ready(const RenderArgs& a) {
	while (__hip_atomic_load(frame_ready_word(a.mom, a.lay), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != a.launchSeq) __builtin_amdgcn_s_sleep(1);
}
__device__ __forceinline__ void clear_frame(const RenderArgs& a) {
	// 16-byte stores (every plane starts 16-byte aligned): the planes are 8, 4, 8 and 16 bytes per pixel
	const uint32_t stride = gridDim.x * TPB, first = blockIdx.x * TPB + threadIdx.x;
	auto fill = [&](uint64_t offset, uint64_t bytes, uint4 value, uint64_t tailWord, uint32_t tailBytes) {
		uint4* q = reinterpret_cast<uint4*>(a.mom + offset);
		const uint32_t n16 = (uint32_t)(bytes / 16);
		for (uint32_t i = first; i < n16; i += stride) q[i] = value;
		if (first == 0 && bytes % 16 != 0) {                           // an odd pixel count leaves one 4- or 8-byte element
			if (tailBytes == 8) *reinterpret_cast<uint64_t*>(a.mom + offset + (uint64_t)n16 * 16) = tailWord;
			else for (uint64_t b = (uint64_t)n16 * 16; b < bytes; b += 4) *reinterpret_cast<uint32_t*>(a.mom + offset + b) = (uint32_t)tailWord;
		}
	};
	const uint32_t lo = (uint32_t)SIMLOD_CLEAR_PIXEL, hi = (uint32_t)(SIMLOD_CLEAR_PIXEL >> 32);
	fill(FrameLayout::framebuffer, (uint64_t)a.numPixels * 8, make_uint4(lo, hi, lo, hi), SIMLOD_CLEAR_PIXEL, 8);
	if (a.useBins) { uint32_t* segCount = reinterpret_cast<uint32_t*>(a.mom + a.lay.binSegCount); for (uint32_t i = first; i < a.lay.binTiles; i += stride) segCount[i] = 0u; }
	if (a.hqs) fill(a.lay.depth, (uint64_t)a.numPixels * 4, make_uint4(0x7f800000u, 0x7f800000u, 0x7f800000u, 0x7f800000u), 0x7f800000u, 4);
}
// The planes of the HQS colour pass — 24 bytes per pixel, two thirds of what a frame clears — are cleared by the DEPTH pass's draw workgroups
// before they take their first item: stores nobody waits for, in a kernel that is bound by LDS atomics.  In r_visible they queued in
// front of the node loads on its critical path: 6 us of that kernel.
__device__ __forceinline__ void clear_colour_planes(const RenderArgs& a) {
	const uint32_t stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x;
	uint4* q = reinterpret_cast<uint4*>(a.mom + a.lay.colour);                     // the packed plane and the {R, G, B, count} plane are neighbours
	const uint64_t bytes = (a.lay.sums - a.lay.colour) + (uint64_t)a.numPixels * 16;
	for (uint64_t i = first; i < bytes / 16; i += stride) q[i] = make_uint4(0, 0, 0, 0);
}
__device__ __forceinline__ void clear_counters(const RenderArgs& a) {     // one thread
	*a.frameStart = wall_ns();                                        // render.cu:1100-1102
	for (int k = 0; k < C_COUNT; k++) *counter_at(a.mom, k) = 0;
	uint32_t* work = work_words(a.mom, a.lay);
	for (int k = 0; k < W_COUNT; k++) work[k] = 0;
	uint32_t* lines = reinterpret_cast<uint32_t*>(a.mom + FrameLayout::lines);
	lines[0] = 0;                                                      // lines->count = 0, render.cu:1118
	__hip_atomic_store(frame_ready_word(a.mom, a.lay), a.launchSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the frame's clip (include/simlod_hip.h, "clip regions"; clip_rules.hpp) ------------------------------------------------------------------
// r_visible, r_draw and what they call take a policy.  NoClip: nothing — the instantiations of a frame without a clip are what they were before
// there was one.  Clip: the kernel's second argument (the box, the mode, the colour) and the planes, which the workgroup stages in LDS once
// (512 bytes): a node's class is computed from (level, X, Y, Z) where it is needed — by r_visible's lane for its node, by r_draw once per item from
// the item's visible record, every lane the same — and the per-sample test sits right behind the sample load, one plane at a time.
struct NoClip {
	static constexpr bool ON = false;
	__device__ __forceinline__ bool empties(uint32_t, uint32_t, uint32_t, uint32_t) const { return false; }
	template <uint32_t DU> __device__ __forceinline__ void test(float4 (&)[DU], bool (&)[DU]) const {}
};
struct Clip {
	static constexpr bool ON = true;
	const ClipArgs& k;                   // (the scalars are read from the kernel's argument block where they are used)
	const double (*pl)[4];               // LDS
	uint32_t action;                     // r_draw: CLIP_ACT_* of the item in hand — the same for the whole workgroup
	__device__ __forceinline__ uint32_t action_of(uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) const {
		return clip_action(k.mode, classify_node(k.min, k.size, k.numPlanes, pl, level, X, Y, Z));
	}
	__device__ __forceinline__ bool empties(uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) const { return action_of(level, X, Y, Z) == CLIP_ACT_EMPTY; }
	// behind the load of DU samples per lane: a removed sample is one the lane does not have; a highlighted one carries the clip's colour
	template <uint32_t DU> __device__ __forceinline__ void test(float4 (&p)[DU], bool (&have)[DU]) const {
		if (action != CLIP_ACT_KEEP_PASSING && action != CLIP_ACT_KEEP_FAILING && action != CLIP_ACT_COLOUR_PASSING) return;      // (uniform)
		bool ok[DU];
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) ok[u] = true;
#pragma unroll 1
		for (uint32_t q = 0; q < k.numPlanes; q++) {
#pragma unroll
			for (uint32_t u = 0; u < DU; u++) ok[u] = ok[u] && plane_passes(pl[q], p[u].x, p[u].y, p[u].z);
		}
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) {
			if (action == CLIP_ACT_KEEP_PASSING) have[u] = have[u] && ok[u];
			else if (action == CLIP_ACT_KEEP_FAILING) have[u] = have[u] && !ok[u];
			else if (ok[u]) p[u].w = __uint_as_float(k.color);
		}
	}
};
// the policy of a kernel from its trailing arguments: none -> NoClip; the ClipArgs -> Clip, with the planes staged in the workgroup's LDS
template <bool ON> struct ClipStore { __device__ __forceinline__ NoClip policy() const { return NoClip(); } };
template <> struct ClipStore<true> {
	__device__ __forceinline__ Clip policy(const ClipArgs& k) const {
		__shared__ double sh_planes[SIMLOD_REGION_MAX_PLANES][4];
		if (threadIdx.x < 4u * SIMLOD_REGION_MAX_PLANES) sh_planes[threadIdx.x / 4u][threadIdx.x % 4u] = k.pl[threadIdx.x / 4u][threadIdx.x % 4u];
		__syncthreads();
		return Clip{k, sh_planes, CLIP_ACT_NONE};
	}
};
