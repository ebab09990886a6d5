// export_delta.inc — part of export.hip: view deltas.  DeltaLayout, DeltaArgs, k_d_match, k_d_scan, delta_pieces, k_d_dir, k_d_drop, MergeArgs,
// k_d_merge_scan, k_d_merge_dir.
// ---- view delta -------------------------------------------------------------------------------------------------------------------------
// simlod_query_view_delta (simlod_hip.h, "view deltas"): k_v_hier and k_v_scan exactly as simlod_query_view runs them for a count-only call —
// they leave the table and the view's counts —, then on the same stream
//   k_d_match  one lane per table entry: rule D2's search of the entry's key in the held table (delta_rules.hpp delta_find), the state by rules
//              D3-D5, the entry's record without firstDelta, and the entry's index into mark[h] of the held entry found.
//   k_d_scan   ONE workgroup: the exclusive scans of numDelta (-> firstDelta) and of the copy pieces per entry (-> first[], free again after
//              k_v_scan), the capacity checks, the delta's half of the counts.
//   k_d_dir    one wave per entry, as k_q_dir: CopyItems for the samples [numKept, n) of the entry's chunk list; the first may begin in the
//              middle of a chunk.
//   k_copy     as it is.
//   k_d_drop   ONE workgroup: rule D6's list, an ordered compaction of the held entries — ballot ranks inside a wave, the waves' counts
//              through LDS, a running base over the turns.
// mark[] is never cleared: k_d_match stores mark[h] = t for the one entry t that found h, and k_d_drop believes a word m only if m < n and
// entries[m].held == h — which no other word can make true, since entry m found one h and stored m there.
// simlod_merge_view_delta: k_d_merge_scan (ONE workgroup: the pieces per entry, the capacity check, the counts) -> k_d_merge_dir (one lane per
// entry: CopyItems of its kept part and of its delta part) -> k_copy.

// scratch: Layout's header | map | par | first, then mark u32[numHeld], then the items up to the buffer's end
struct DeltaLayout {
	Layout   x;
	uint64_t mark;
	__host__ __device__ DeltaLayout(uint32_t cap, uint32_t numHeld) {
		x = Layout(cap, 0u);
		mark = x.items;
		x.items = mark + align256(4ull * numHeld);
	}
};
// the pieces of at most 1 000 samples a result of `sampleBound` samples in `cap` entries has: a delta's parts begin and end inside a chunk
// (<= n_i / 1000 + 1 each, as the export's), a merge's entries have a kept and a delta part (<= n_i / 1000 + 2)
__host__ __device__ inline uint64_t delta_item_bound(uint32_t cap, uint64_t sampleBound) { return sampleBound / SIMLOD_POINTS_PER_CHUNK + 2ull * cap + 1u; }

struct DeltaArgs {
	ExportArgs              x;          // as launch_view fills it for a count-only call; x.lay: DeltaLayout's, the items with the rest of the buffer
	const SimlodExportNode* held;
	uint32_t                numHeld, deltaFlags;
	uint64_t                mark;       // offset of mark[] in the scratch buffer
	SimlodDeltaEntry*       entries;
	SimlodPoint*            delta;
	uint64_t                deltaCap;
	uint32_t*               dropped;
	uint32_t                droppedCap, pad;
	SimlodDeltaCounts*      counts;
};

__global__ __launch_bounds__(LANE_TPB) void k_d_match(DeltaArgs d) {
	const Header* hdr = reinterpret_cast<const Header*>(d.x.scratch);
	uint32_t* mark = reinterpret_cast<uint32_t*>(d.x.scratch + d.mark);
	const uint32_t t = blockIdx.x * LANE_TPB + threadIdx.x;
	if (t >= hdr->numListed) return;
	const SimlodExportNode& e = d.x.table[t];
	const uint32_t n = e.numSamples, flags = e.flags;
	const uint32_t h = delta_find(d.held, d.numHeld, e.level, e.X, e.Y, e.Z);
	uint32_t heldFlags = 0u, hs = 0u;
	if (h != NONE) { heldFlags = d.held[h].flags; hs = d.held[h].numSamples; mark[h] = t; }
	uint32_t kept = 0u, state = delta_state(flags, n, h != NONE, heldFlags, hs, d.deltaFlags, kept);
	uint32_t nd = n - kept;
	if (hdr->error & SIMLOD_EXPORT_ERR_BUDGET) { state = SIMLOD_DELTA_NONE; kept = 0u; nd = 0u; }     // rule D1
	SimlodDeltaEntry& de = d.entries[t];                                    // (firstDelta is k_d_scan's)
	de.held = h; de.state = state; de.numKept = kept; de.numDelta = nd;
}

// the pieces of the samples [kept, kept + nd) of a chunk list: the chunks floor(kept / 1000) .. ceil((kept + nd) / 1000) - 1
__device__ __forceinline__ uint32_t delta_pieces(uint32_t kept, uint32_t nd) {
	return nd == 0u ? 0u : ceil_chunks((uint64_t)kept + nd) - kept / SIMLOD_POINTS_PER_CHUNK;
}

__global__ __launch_bounds__(WG_TPB) void k_d_scan(DeltaArgs d) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ unsigned long long sh_tot[3];                                // the lanes' shares summed up: kept samples, KEPT | GROWN << 32 entries, ADDED entries
	const ExportArgs& a = d.x;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(a.scratch + a.lay.first);
	const uint32_t n = hdr->numListed;
	if (threadIdx.x < 3u) sh_tot[threadIdx.x] = 0ull;                       // (the scans' barriers lie between this and the sums)
	uint64_t samples = 0u, items = 0u, keptSamples = 0u, keptGrown = 0u, added = 0u;   // (this lane's share of the last three; keptGrown: KEPT entries, GROWN ones from bit 32)
	for (uint32_t base = 0; base < n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		uint32_t state = SIMLOD_DELTA_NONE, kept = 0u, nd = 0u;
		if (t < n) { const SimlodDeltaEntry& de = d.entries[t]; state = de.state; kept = de.numKept; nd = de.numDelta; }
		uint64_t totS, totI;
		const uint64_t offS = block_scan<uint64_t>(nd, totS, sh_scan);
		const uint64_t offI = block_scan<uint64_t>(delta_pieces(kept, nd), totI, sh_scan);
		if (t < n) { d.entries[t].firstDelta = samples + offS; first[t] = (uint32_t)(items + offI); }
		samples += totS; items += totI;
		keptSamples += kept;
		keptGrown += state == SIMLOD_DELTA_KEPT ? 1ull : state == SIMLOD_DELTA_GROWN ? 1ull << 32 : 0ull;
		added += state == SIMLOD_DELTA_ADDED ? 1u : 0u;
	}
	__syncthreads();                                                        // (n == 0: no scan has run)
	if (keptSamples != 0u) atomicAdd(&sh_tot[0], (unsigned long long)keptSamples);
	if (keptGrown != 0u) atomicAdd(&sh_tot[1], (unsigned long long)keptGrown);
	if (added != 0u) atomicAdd(&sh_tot[2], (unsigned long long)added);
	__syncthreads();
	if (threadIdx.x == 0) {
		const uint64_t totK = sh_tot[0], totC = sh_tot[1], totA = sh_tot[2];
		const bool write = d.delta != nullptr;                                  // (a count-only call: no capacity to miss)
		uint32_t err = hdr->error;
		if (write && (samples > d.deltaCap || items > a.lay.itemCap)) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		first[n] = (uint32_t)items;
		hdr->error = err;
		hdr->numItems = (!write || (err & (SIMLOD_EXPORT_ERR_CAPACITY | SIMLOD_EXPORT_ERR_BUDGET))) ? 0u : items;
		// (k_v_scan wrote the walk's error bits there; k_d_dir and k_d_drop add theirs with atomics)
		atomicOr(&d.counts->view.error, err);
		d.counts->numDeltaSamples = samples; d.counts->numKeptSamples = totK;
		d.counts->numKept = (uint32_t)totC; d.counts->numGrown = (uint32_t)(totC >> 32); d.counts->numAdded = (uint32_t)totA;
	}
}

// One WAVE per table entry, as k_q_dir: while the builder's table is valid lane k looks chunk k up, all at once; what the rows do not give lane 0
// follows by `next`.  Chunk k of the list gives piece k - k0, k0 = numKept / 1000 the chunk the first missing sample lies in.
__global__ __launch_bounds__(LANE_TPB) void k_d_dir(DeltaArgs d) {
	const ExportArgs& a = d.x;
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const uint32_t* map = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.map);
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.first);
	CopyItem* items = reinterpret_cast<CopyItem*>(a.scratch + a.lay.items);
	const uint32_t t = blockIdx.x * (LANE_TPB / SIMLOD_WAVE) + threadIdx.x / SIMLOD_WAVE;
	const uint32_t lane = (uint32_t)lane_id();
	if (t >= hdr->numListed || hdr->numItems == 0u) return;                // (everything up to the lookups is the same for the whole wave)
	const SimlodDeltaEntry& de = d.entries[t];
	const uint32_t kept = de.numKept, nd = de.numDelta;
	if (nd == 0u) return;
	const uint32_t ns = kept + nd, src = map[t];
	const SimlodNode* n = a.nodes + src;
	const bool leaf = (a.table[t].flags & SIMLOD_EXPORT_FLAG_LEAF) != 0u;
	const SimlodChunk* head = leaf ? n->points : n->voxelChunks;
	const bool rows = leaf_rows_valid(a, src, head, leaf);
	const uint32_t nch = ceil_chunks(ns), k0 = kept / SIMLOD_POINTS_PER_CHUNK, f = first[t];
	const uint64_t dst0 = reinterpret_cast<uint64_t>(d.delta + de.firstDelta);
	auto put = [&](uint32_t k, const SimlodChunk* c) {                      // k >= k0
		const uint32_t off = k == k0 ? kept - k0 * SIMLOD_POINTS_PER_CHUNK : 0u;            // the first piece may begin inside its chunk
		CopyItem it;
		it.src = reinterpret_cast<uint64_t>(c->points + off);
		it.dst = dst0 + ((uint64_t)k * SIMLOD_POINTS_PER_CHUNK + off - kept) * sizeof(SimlodPoint);
		it.count = min(ns - k * SIMLOD_POINTS_PER_CHUNK, SIMLOD_POINTS_PER_CHUNK) - off;
		it.pad0 = 0; it.pad1 = 0;
		items[f + (k - k0)] = it;
	};
	uint32_t good = 0;                       // chunks the rows gave: 0 .. good - 1
	bool shortList = false;
	if (rows) {
		const uint32_t kr = min(min(nch, a.ltSlots), (uint32_t)SIMLOD_WAVE);
		const SimlodChunk* c = lane == 0u ? head : lane < kr ? leaf_row_get(a.lt, a.ltPers, src, lane) : nullptr;
		const uint64_t missing = __ballot(lane < kr && c == nullptr);
		good = missing != 0ull ? (uint32_t)__ffsll((long long)missing) - 1u : kr;
		if (lane >= k0 && lane < good) put(lane, c);
		shortList = good < kr;
	}
	if (lane != 0u) return;
	uint32_t k = good;
	const SimlodChunk* c = good == 0u ? nullptr : good == 1u ? head : leaf_row_get(a.lt, a.ltPers, src, good - 1u);   // the chunk in front of chunk k
	for (; k < nch && !shortList; k++) {
		c = k == 0u ? head : c->next;
		if (c == nullptr) { shortList = true; break; }
		if (k >= k0) put(k, c);
	}
	if (shortList) {
		atomicOr(&d.counts->view.error, SIMLOD_EXPORT_ERR_SHORT_LIST);
		for (k = max(k, k0); k < nch; k++) items[f + (k - k0)] = CopyItem{0, 0, 0, 0, 0};
	}
}

// rule D6 in ONE workgroup: turn by turn WG_TPB held entries; a qualifying entry's place is the running base + the counts of the waves in front
// of its own + the ballot's bits below its lane.
__global__ __launch_bounds__(WG_TPB) void k_d_drop(DeltaArgs d) {
	__shared__ uint32_t sh_wave[2][WG_WAVES];
	const Header* hdr = reinterpret_cast<const Header*>(d.x.scratch);
	const uint32_t* mark = reinterpret_cast<const uint32_t*>(d.x.scratch + d.mark);
	const uint32_t n = hdr->numListed;
	const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x / SIMLOD_WAVE;
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t base = 0u, turn = 0u;
	for (uint32_t h0 = 0; h0 < d.numHeld; h0 += WG_TPB) {
		const uint32_t h = h0 + threadIdx.x;
		bool drop = false;
		if (h < d.numHeld) {
			const SimlodExportNode& e = d.held[h];
			drop = (e.flags & SIMLOD_EXPORT_FLAG_SELECTED) != 0u && e.numSamples > 0u;
			const uint32_t m = mark[h];                                         // (a word nobody stored to: believed only if entry m says so)
			if (drop && m < n) {
				const SimlodDeltaEntry& de = d.entries[m];
				if (de.held == h && (de.state == SIMLOD_DELTA_KEPT || de.state == SIMLOD_DELTA_GROWN)) drop = false;
			}
		}
		const uint64_t b = __ballot(drop);
		if (lane == 0u) sh_wave[turn][w] = (uint32_t)__popcll(b);
		__syncthreads();                        // (two buffers: the next turn's writes cannot overtake this turn's reads)
		uint32_t before = 0u, all = 0u;
		for (uint32_t k = 0; k < WG_WAVES; k++) { const uint32_t c = sh_wave[turn][k]; before += k < w ? c : 0u; all += c; }
		const uint32_t at = base + before + (uint32_t)__popcll(b & below);
		if (drop && at < d.droppedCap) d.dropped[at] = h;
		base += all;
		turn ^= 1u;
	}
	if (threadIdx.x == 0) {
		d.counts->numDropped = base;
		if (d.dropped != nullptr && base > d.droppedCap) atomicOr(&d.counts->view.error, SIMLOD_EXPORT_ERR_CAPACITY);
	}
}
static_assert(WG_TPB / SIMLOD_WAVE == WG_WAVES, "k_d_drop: threadIdx.x / SIMLOD_WAVE < WG_WAVES indexes sh_wave");

// ---- merge ------------------------------------------------------------------------------------------------------------------------------
// scratch: Layout's header | first u32[numNodes + 1] (where Layout has it) | the items behind DeltaLayout's mark (unused here)
struct MergeArgs {
	const SimlodExportNode* held;
	uint32_t                numHeld, n;
	const SimlodPoint*      heldSamples;
	const SimlodExportNode* table;
	const SimlodDeltaEntry* entries;
	const SimlodPoint*      delta;
	uint8_t*                scratch;
	Layout                  lay;
	SimlodPoint*            samples;
	uint64_t                sampleCap;
	SimlodExportCounts*     counts;
};

// the parts of entry t as the merge takes them: nothing of an entry without a state, nothing of one whose held index is out of range
__device__ __forceinline__ bool merge_parts(const MergeArgs& m, uint32_t t, uint32_t& kept, uint32_t& nd) {
	const SimlodDeltaEntry& de = m.entries[t];
	kept = de.numKept; nd = de.numDelta;
	if (de.state == SIMLOD_DELTA_NONE) { kept = 0u; nd = 0u; }
	if (kept != 0u && de.held >= m.numHeld) { kept = 0u; nd = 0u; return false; }
	return true;
}

__global__ __launch_bounds__(WG_TPB) void k_d_merge_scan(MergeArgs m) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	Header* hdr = reinterpret_cast<Header*>(m.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(m.scratch + m.lay.first);
	uint64_t samples = 0u, items = 0u, bad = 0u;                            // bad (this lane's): 1 an entry out of range, 2 one beyond the capacity
	for (uint32_t base = 0; base < m.n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		uint32_t kept = 0u, nd = 0u;
		if (t < m.n) {
			if (!merge_parts(m, t, kept, nd)) bad |= 1u;
			if (kept + nd != 0u && m.table[t].firstSample + kept + nd > m.sampleCap) bad |= 2u;
		}
		uint64_t totS, totI;
		block_scan<uint64_t>((uint64_t)kept + nd, totS, sh_scan);
		const uint64_t offI = block_scan<uint64_t>(ceil_chunks(kept) + ceil_chunks(nd), totI, sh_scan);
		if (t < m.n) first[t] = (uint32_t)(items + offI);
		samples += totS; items += totI;
	}
	// (the flags of every lane: a sum of at most WG_TPB ones per flag, 32 bits apart)
	uint64_t totB;
	block_scan<uint64_t>((bad & 1u) | (bad & 2u) << 31, totB, sh_scan);
	if (threadIdx.x == 0) {
		uint32_t err = 0u;
		if (totB & 0xffffffffull) err |= SIMLOD_EXPORT_ERR_SHORT_LIST;
		if ((totB >> 32) != 0u || items > m.lay.itemCap) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		first[m.n] = (uint32_t)items;
		hdr->error = err; hdr->numListed = m.n;
		hdr->numItems = (err & SIMLOD_EXPORT_ERR_CAPACITY) ? 0u : items;
		SimlodExportCounts c;
		c.numNodes = m.n; c.error = err; c.numSamples = samples;
		*m.counts = c;
	}
}

__global__ __launch_bounds__(LANE_TPB) void k_d_merge_dir(MergeArgs m) {
	const Header* hdr = reinterpret_cast<const Header*>(m.scratch);
	const uint32_t* first = reinterpret_cast<const uint32_t*>(m.scratch + m.lay.first);
	CopyItem* items = reinterpret_cast<CopyItem*>(m.scratch + m.lay.items);
	const uint32_t t = blockIdx.x * LANE_TPB + threadIdx.x;
	if (t >= m.n || hdr->numItems == 0u) return;
	uint32_t kept, nd;
	merge_parts(m, t, kept, nd);
	if (kept + nd == 0u) return;
	const SimlodDeltaEntry& de = m.entries[t];
	uint32_t f = first[t];
	const SimlodPoint* dst = m.samples + m.table[t].firstSample;
	auto part = [&](const SimlodPoint* src, uint32_t count) {
		for (uint32_t o = 0; o < count; o += SIMLOD_POINTS_PER_CHUNK) {
			CopyItem it;
			it.src = reinterpret_cast<uint64_t>(src + o); it.dst = reinterpret_cast<uint64_t>(dst + o);
			it.count = min(count - o, (uint32_t)SIMLOD_POINTS_PER_CHUNK); it.pad0 = 0; it.pad1 = 0;
			items[f++] = it;
		}
		dst += count;
	};
	if (kept != 0u) part(m.heldSamples + m.held[de.held].firstSample, kept);
	if (nd != 0u) part(m.delta + de.firstDelta, nd);
}
