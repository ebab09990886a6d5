// render_bins.inc — the screen bins: bin_item (what a sorting item of r_draw does with its samples) and the r_overflow kernel that rasterises the bins.
// One item of a node that is much larger than a tile (DrawItem::tileX == TILE_BINNED): its samples are sorted into the screen bins.  Every
// thread projects its <= 8 samples ONCE and keeps {bin, pixel inside it, value} in registers, counting per bin in LDS; then the workgroup
// scans the counters, takes ALL its entries from the pool with ONE atomic (every item of the frame reserves on that word: one atomic per
// item and bin on it took 11 ns each, 200 us a frame) and lists one segment per bin with samples; then every sample writes its entry.
// Value: depth | colour (plain frames), depth (HQS depth pass), colour of an ACCEPTED sample (HQS colour pass, render.cu:485-493).  Pool
// exhausted: the item's samples take the device-scope atomics, as before; a bin's list full: that bin's.
template <int MODE, typename POLICY>
__device__ __forceinline__ void bin_item(const DrawCtx& c, const RenderArgs& a, uint32_t* lds, const SimlodChunk* const* dir, uint32_t count, uint32_t overrideColor, bool useOverride,
                                         uint32_t& outside, const POLICY& clip) {
	// (opaque to the optimiser: what depends on the thread only — chunk and offset of each of its 16 samples, the addresses of its bins' words —
	// was hoisted out of r_draw's item loop and occupied 40 registers for the whole kernel: every draw path spilled)
	uint32_t tid = threadIdx.x;
	asm volatile("" : "+v"(tid));
	uint32_t* cnt = lds;                           // [binTiles]: samples of this item per bin, then the cursor inside the segment
	uint32_t* base = lds + BIN_MAX_TILES;          // [binTiles]: first pool entry of the item's segment in that bin, or NONE
	uint32_t* scratch = lds + 2 * BIN_MAX_TILES;   // [16] sums of the waves, [16] the item's first pool entry
	constexpr uint32_t NONE = 0xffffffffu, DU = 4, SLOTS = (BIN_ITEM_CHUNKS * SIMLOD_POINTS_PER_CHUNK + DTPB - 1) / DTPB;
	static_assert(SLOTS % DU == 0, "a thread's samples come in batches of DU loads");
	uint32_t* work = work_words(a.mom, a.lay);
	uint32_t* segCount = reinterpret_cast<uint32_t*>(a.mom + a.lay.binSegCount);
	BinSeg* segs = reinterpret_cast<BinSeg*>(a.mom + a.lay.binSegs);
	uint4* pool = reinterpret_cast<uint4*>(a.mom + a.lay.binPool);
	for (uint32_t t = tid; t < a.lay.binTiles; t += DTPB) cnt[t] = 0u;
	__syncthreads();
	uint32_t key[SLOTS], lo[SLOTS], hi[SLOTS];     // bin << 10 | pixel inside the bin, or NONE; the value's halves
#pragma unroll
	for (uint32_t r = 0; r < SLOTS / DU; r++) {
		float4 p[DU];
		bool have[DU];
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) {
			const uint32_t sIdx = (r * DU + u) * DTPB + tid;
			have[u] = sIdx < count;
			p[u] = have[u] ? reinterpret_cast<const float4*>(dir[sIdx / SIMLOD_POINTS_PER_CHUNK]->points)[sIdx % SIMLOD_POINTS_PER_CHUNK] : make_float4(0, 0, 0, 0);
		}
		clip.test(p, have);                                                 // (before a sample becomes a bin entry)
		uint32_t pixel[DU];
		float depth[DU];
		bool valid[DU];
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) {
			const uint32_t k = r * DU + u;
			const float cx = dot_row(c.r0, p[u].x, p[u].y, p[u].z);
			const float cy = dot_row(c.r1, p[u].x, p[u].y, p[u].z);
			depth[u] = dot_row(c.r3, p[u].x, p[u].y, p[u].z);
			const float nx = cx / depth[u], ny = cy / depth[u];
			const double fx = ((double)nx * 0.5 + 0.5) * (double)c.width;
			const double fy = ((double)ny * 0.5 + 0.5) * (double)c.height;
			const int x = (int)fx, y = (int)fy;
			valid[u] = have[u] && (x > 1 && (double)x < c.wlim) && (y > 1 && (double)y < c.hlim);
			if (MODE != MODE_MIN64) valid[u] = valid[u] && depth[u] > 0.0f;
			const int px = min(max(x, 0), c.W), py = min(max(y, 0), c.H);
			pixel[u] = (uint32_t)px + (uint32_t)c.W * (uint32_t)py;
			valid[u] = valid[u] && pixel[u] < c.numPixels;
			const uint32_t bin = ((uint32_t)py >> BIN_SHIFT) * a.lay.binTilesX + ((uint32_t)px >> BIN_SHIFT);
			key[k] = (bin << (2 * BIN_SHIFT)) | (((uint32_t)py & (BIN - 1u)) << BIN_SHIFT) | ((uint32_t)px & (BIN - 1u));
			const uint32_t color = useOverride ? overrideColor : __float_as_uint(p[u].w);
			lo[k] = MODE == MODE_DEPTH ? __float_as_uint(depth[u]) : color;
			hi[k] = MODE == MODE_MIN64 ? __float_as_uint(depth[u]) : 0u;
		}
		if (MODE == MODE_COLOR) {                                           // render.cu:485-493
			uint32_t ref[DU];
#pragma unroll
			for (uint32_t u = 0; u < DU; u++) ref[u] = c.depth[valid[u] ? pixel[u] : 0u];
#pragma unroll
			for (uint32_t u = 0; u < DU; u++) valid[u] = valid[u] && depth[u] < __uint_as_float(ref[u]) * 1.01f;
		}
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) {
			const uint32_t k = r * DU + u;
			if (valid[u]) atomicAdd(&cnt[key[k] >> (2 * BIN_SHIFT)], 1u); else key[k] = NONE;
		}

	}
	__syncthreads();
	// exclusive scan of the counters over the workgroup -> every bin's offset inside the item's reservation
	uint32_t carry = 0;
	for (uint32_t t0 = 0; t0 < a.lay.binTiles; t0 += DTPB) {               // uniform
		const uint32_t t = t0 + tid;
		const uint32_t n = t < a.lay.binTiles ? cnt[t] : 0u;
		uint32_t waveTotal;
		const uint32_t before = wave_prefix_u32(n, waveTotal);
		if (lane_id() == 0) scratch[tid / 64u] = waveTotal;
		__syncthreads();
		uint32_t waveBase = 0, roundTotal = 0;
		for (uint32_t w = 0; w < DTPB / 64u; w++) { const uint32_t v = scratch[w]; waveBase += w < tid / 64u ? v : 0u; roundTotal += v; }
		if (t < a.lay.binTiles) base[t] = carry + waveBase + before;
		carry += roundTotal;
		__syncthreads();
	}
	// the item's entries and, per bin, a place in the bin's list: all reservations in flight together (a list place taken in vain — pool
	// exhausted — holds an empty segment)
	constexpr uint32_t ROUNDS = (BIN_MAX_TILES + DTPB - 1) / DTPB;
	uint32_t seg[ROUNDS];
#pragma unroll
	for (uint32_t q = 0; q < ROUNDS; q++) {
		const uint32_t t = q * DTPB + tid;
		seg[q] = t < a.lay.binTiles && cnt[t] != 0u ? atomicAdd(&segCount[t], 1u) : NONE;
	}
	if (tid == 0) {
		uint32_t at = NONE;
		if (carry != 0u) { at = atomicAdd(work + W_POOL_TAKEN, carry); if ((unsigned long long)at + carry > a.binPoolCap) at = NONE; }
		scratch[16] = at;
	}
	__syncthreads();
	const uint32_t itemBase = scratch[16];
	uint32_t binned = 0;
#pragma unroll
	for (uint32_t q = 0; q < ROUNDS; q++) {
		const uint32_t t = q * DTPB + tid;
		if (t >= a.lay.binTiles) continue;
		const uint32_t n = cnt[t];
		uint32_t b = NONE;
		if (seg[q] < BIN_SEG_CAP) {
			if (itemBase != NONE) { b = itemBase + base[t]; binned += n; }
			segs[(uint64_t)t * BIN_SEG_CAP + seg[q]] = BinSeg{b != NONE ? b : 0u, b != NONE ? n : 0u};
		}
		base[t] = b; cnt[t] = 0u;
	}
	if (MODE != MODE_COLOR) { binned = wave_sum_u32(binned); if (lane_id() == 0 && binned != 0u) atomicAdd(work + W_BINNED, binned); }
	__syncthreads();
#pragma unroll
	for (uint32_t k = 0; k < SLOTS; k++) {
		if (key[k] == NONE) continue;
		const uint32_t bin = key[k] >> (2 * BIN_SHIFT), local = key[k] & (BIN * BIN - 1u);
		const uint32_t b = base[bin];
		if (b != NONE) { pool[b + atomicAdd(&cnt[bin], 1u)] = make_uint4(lo[k], hi[k], local, 0u); continue; }
		outside += 1u;                                                     // no room in the bins: the global path of draw_sample
		const uint32_t px = ((bin % a.lay.binTilesX) << BIN_SHIFT) | (local & (BIN - 1u)), py = ((bin / a.lay.binTilesX) << BIN_SHIFT) | (local >> BIN_SHIFT);
		const uint32_t pixel = px + (uint32_t)c.W * py;
		if (MODE == MODE_MIN64) atomicMin(reinterpret_cast<unsigned long long*>(&c.fb[pixel]), ((unsigned long long)hi[k] << 32) | lo[k]);
		else if (MODE == MODE_DEPTH) atomicMin(&c.depth[pixel], lo[k]);
		else {
			const unsigned long long r = lo[k] & 0xffu, g = (lo[k] >> 8) & 0xffu, bl = (lo[k] >> 16) & 0xffu;
			const unsigned long long pk = bl | (g << 14) | (r << 28) | (1ull << 42);
			const unsigned long long old = atomicAdd(&c.color[pixel], pk);
			if ((old >> 42) >= 64ull) {
				atomicAdd(&c.color[pixel], 0ull - pk);
				atomicAdd(&c.overflow[2 * pixel + 0], r | (g << 32));
				atomicAdd(&c.overflow[2 * pixel + 1], bl | (1ull << 32));
			}
		}
	}
}

// ---- overflow: the screen bins (what the sorting items of r_draw queued) into the planes -----------------------------------------------
// One workgroup per 32 x 32-pixel bin: the bin's pixels in LDS, every wave takes segments of the bin's list — consecutive 16-byte entries, four
// of a lane in flight —, LDS atomics; then the touched pixels are merged into the plane with PLAIN loads and stores: r_draw has ended, and
// in this kernel a pixel belongs to one workgroup.  The colour pass keeps exact 32-bit sums (two 64-bit words per pixel).  Leaves the bins
// empty for the next pass.
template <int MODE>
__global__ __launch_bounds__(OTPB) void r_overflow(RenderArgs a) {
	uint32_t* work = work_words(a.mom, a.lay);
	uint32_t* segCount = reinterpret_cast<uint32_t*>(a.mom + a.lay.binSegCount);
	// (workgroup -> bin by a stride that is coprime to every bin count: the full bins of a frame are neighbours — a band of the screen — and
	// in launch order they would all start late, behind a thousand empty ones)
	const uint32_t T = (uint32_t)(((uint64_t)blockIdx.x * OVERFLOW_STRIDE) % a.lay.binTiles);
	const uint32_t numSegs = min(segCount[T], BIN_SEG_CAP);
	const uint64_t started = SIMLOD_MEASURE != 0 && threadIdx.x == 0u ? wall_clock64() : 0ull;
	if (T == 0u && threadIdx.x == 0u) work[W_POOL_TAKEN] = 0u;                 // (nobody appends in this kernel; this pass's entries stay where they are until the next pass overwrites them)
	if (numSegs == 0u) return;
	// (one workgroup per bin of the SCREEN, most of which find nothing.  Round 5 measured the alternative VERDICT r4 asked for — r_draw lists the bins
	// it opens, a fixed grid of 1 024 workgroups visits the listed ones —: 25.4 us against 20.8 per pass on the close-up, same box, same run: the
	// list costs two more dependent loads in front of every bin's segments, the empty workgroups cost less than that.  Persistent workgroups that
	// loop over bins: 30 us against 24, round 4.)
	constexpr uint32_t PIXELS = BIN * BIN, DU = 4;
	__shared__ unsigned long long sh_tile[MODE == MODE_DEPTH ? PIXELS / 2 : MODE == MODE_COLOR ? 2 * PIXELS : PIXELS];
	__shared__ BinSeg sh_segs[BIN_SEG_CAP];
	uint32_t* tile32 = reinterpret_cast<uint32_t*>(sh_tile);
	const uint4* pool = reinterpret_cast<const uint4*>(a.mom + a.lay.binPool);
	__shared__ uint32_t sh_first[BIN_SEG_CAP + 1], sh_waves[OTPB / 64];      // first chunk of every segment; [numSegs] = chunks in all
	static_assert(BIN_SEG_CAP <= OTPB, "one thread per segment");
	uint64_t* fb = reinterpret_cast<uint64_t*>(a.mom + FrameLayout::framebuffer);
	uint32_t* depth = reinterpret_cast<uint32_t*>(a.mom + a.lay.depth);
	unsigned long long* overflow = reinterpret_cast<unsigned long long*>(a.mom + a.lay.sums);
	const BinSeg* segs = reinterpret_cast<const BinSeg*>(a.mom + a.lay.binSegs) + (uint64_t)T * BIN_SEG_CAP;
	{
		BinSeg seg = BinSeg{0u, 0u};
		if (threadIdx.x < numSegs) { seg = segs[threadIdx.x]; sh_segs[threadIdx.x] = seg; }
		const uint32_t n = (seg.count + 64u * DU - 1u) / (64u * DU);
		uint32_t waveTotal;
		const uint32_t before = wave_prefix_u32(n, waveTotal);
		if (lane_id() == 0) sh_waves[threadIdx.x / 64u] = waveTotal;
		__syncthreads();
		uint32_t waveBase = 0;
		for (uint32_t w = 0; w < threadIdx.x / 64u; w++) waveBase += sh_waves[w];
		if (threadIdx.x < numSegs) sh_first[threadIdx.x] = waveBase + before;
		if (threadIdx.x + 1u == numSegs) sh_first[numSegs] = waveBase + before + n;
	}
	for (uint32_t t = threadIdx.x; t < PIXELS * (MODE == MODE_COLOR ? 2u : 1u); t += OTPB) {
		if (MODE == MODE_DEPTH) tile32[t] = 0xffffffffu; else sh_tile[t] = MODE == MODE_COLOR ? 0ull : ~0ull;
	}
	__syncthreads();
	const uint32_t numChunks = sh_first[numSegs];
	// the list as chunks of 64 x DU entries: chunk c belongs to the segment whose first chunk is the last one <= c; waves take chunks in turn
	// (a segment per wave left most waves idle: a bin lists 10-20 segments of 50 to 5000 entries)
	// Two chunks of a wave in flight: the entries of the next one are requested before the current one's go into the tile.  Measured on the
	// close-up's full bins (28 000 entries): the loads alone 7.5 us, the LDS work alone 7 us, one after the other 18 — a wave does not
	// overlap them by itself; with two chunks in flight 14 (with 8 entries per lane and chunk the second set of registers halved the
	// workgroups per CU and gained nothing: 4 entries).
	auto fetch = [&](const uint32_t c, uint4 (&e)[DU], bool (&have)[DU]) {
		uint32_t sgLo = 0, sgHi = numSegs;                       // sh_first[sgLo] <= c < sh_first[sgHi]
		while (sgHi - sgLo > 1u) { const uint32_t mid = (sgLo + sgHi) / 2u; if (sh_first[mid] <= c) sgLo = mid; else sgHi = mid; }
		const BinSeg seg = sh_segs[sgLo];
		const uint32_t first = (c - sh_first[sgLo]) * 64u * DU;
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) {
			const uint32_t i = first + u * 64u + lane_id();
			have[u] = c < numChunks && i < seg.count;
			e[u] = have[u] ? pool[seg.base + i] : make_uint4(0, 0, 0, 0);
		}
	};
	auto apply = [&](const uint4 (&e)[DU], const bool (&have)[DU]) {
#pragma unroll
		for (uint32_t u = 0; u < DU; u++) {
			if (!have[u]) continue;
			const uint32_t local = e[u].z & (PIXELS - 1u);
			// (a full bin has 20-30 entries per pixel: most entries are not their pixel's minimum, and a read that says so is cheaper than
			// the atomic it saves: 16.5 -> 13.5 us for 28 000 entries)
			if (MODE == MODE_MIN64) { const unsigned long long v = ((unsigned long long)e[u].y << 32) | e[u].x; if (v < sh_tile[local]) atomicMin(&sh_tile[local], v); }
			else if (MODE == MODE_DEPTH) { if (e[u].x < tile32[local]) atomicMin(&tile32[local], e[u].x); }
			else {
				atomicAdd(&sh_tile[2 * local + 0], (unsigned long long)(e[u].x & 0xffu) | ((unsigned long long)((e[u].x >> 8) & 0xffu) << 32));
				atomicAdd(&sh_tile[2 * local + 1], (unsigned long long)((e[u].x >> 16) & 0xffu) | (1ull << 32));
			}
		}
	};
	{
		constexpr uint32_t WAVES = OTPB / 64u;
		uint4 eA[DU], eB[DU];
		bool haveA[DU], haveB[DU];
		uint32_t c = threadIdx.x / 64u;
		if (c < numChunks) fetch(c, eA, haveA);
		while (c < numChunks) {                                  // wave-uniform
			fetch(c + WAVES, eB, haveB);                        // (past the end: nothing is loaded)
			apply(eA, haveA);
			c += WAVES;
			if (c >= numChunks) break;
			fetch(c + WAVES, eA, haveA);
			apply(eB, haveB);
			c += WAVES;
		}
	}
	__syncthreads();
	const int x0 = (int)(T % a.lay.binTilesX) * (int)BIN, y0 = (int)(T / a.lay.binTilesX) * (int)BIN;
	for (uint32_t t = threadIdx.x; t < PIXELS; t += OTPB) {
		const int px = x0 + (int)(t & (BIN - 1u)), py = y0 + (int)(t >> BIN_SHIFT);
		if (px >= a.W || py >= a.H) continue;                 // (a valid sample's pixel is inside (1, W - 2) x (1, H - 2): never a pixel of another bin's row)
		const uint32_t pixel = (uint32_t)px + (uint32_t)a.W * (uint32_t)py;
		if (MODE == MODE_MIN64) {
			const unsigned long long v = sh_tile[t];
			if (v != ~0ull && v < fb[pixel]) fb[pixel] = v;
		} else if (MODE == MODE_DEPTH) {
			const uint32_t v = tile32[t];
			if (v != 0xffffffffu && v < depth[pixel]) depth[pixel] = v;
		} else {
			const unsigned long long rg = sh_tile[2 * t], bc = sh_tile[2 * t + 1];
			if ((bc >> 32) != 0ull) { overflow[2 * pixel + 0] += rg; overflow[2 * pixel + 1] += bc; }      // exact: resolve adds the packed plane and the {R, G, B, count} plane
		}
	}
	if (threadIdx.x == 0u) {
		segCount[T] = 0u;
		if (SIMLOD_MEASURE != 0) {                                     // tools/raster_bins.py: {entries, segments << 20 | 10 ns}
			uint32_t entries = 0;
			for (uint32_t k = 0; k < numSegs; k++) entries += sh_segs[k].count;
			BinSeg* stat = reinterpret_cast<BinSeg*>(a.mom + a.lay.binStats);
			stat[T] = BinSeg{entries, (numSegs << 20) | min((uint32_t)(wall_clock64() - started), 0xfffffu)};
		}
	}
}
