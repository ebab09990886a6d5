// construct_count.inc — part of construct.hip (included there, inside namespace simlod::build; not a translation unit of its own): the front half's first two kernels: k_count (descent, per-leaf counts, crossing leaves) and k_queue (slots, node slots and spill space by prefix sums), with the reservation word and the chunk accounting of exact groups (account_group).

// ---- count: leaf lookup + per-leaf arrival counters + spill detection (voxels.cu:124-229) ---------------------
static constexpr uint32_t PPT = 4;                 // points per thread per chunk
static constexpr uint32_t PPB = TPB * PPT;         // points per workgroup chunk

// Split slots.  A leaf that has to split in this batch owns a SLOT: a record of what was reserved for it and a 512-bin histogram
// — the three octree levels below it — of everything that lies in it (its stored points and the batch's samples).  The cascade is
// decided from the histogram alone (k_expand), three levels per round.  Afterwards the same 512 words are the slot's MAP: bin ->
// the node that bin's samples ended up in.  A sample of a slot is relabelled by rewriting its cached-leaf word as
// LEAF_FLAG | slot << 9 | bin: whoever needs its leaf later (k_insert, the next round) reads ONE word of the map.
// the cached-leaf words of a group: one per sample of the group (two copies by the group's parity — k_count of the next group fills
// its copy while k_insert of this one still reads) and one per moved point (one copy: k_hist writes them after k_insert of the group before)
struct LeafWords {
	uint32_t* grp; uint32_t* mov; uint32_t cap;
	__device__ __forceinline__ LeafWords(const BuildArgs& a, uint32_t ordinal)
		: grp(at<uint32_t>(a, a.offLeafOf) + (uint64_t)(ordinal & 1u) * a.leafOfStride), mov(at<uint32_t>(a, a.offLeafOf) + 2 * a.leafOfStride), cap(a.groupCap) {}
	__device__ __forceinline__ uint32_t& operator[](uint32_t i) const { return i < cap ? grp[i] : mov[i - cap]; }     // i: sample of the group, or groupCap + moved point
};
static constexpr uint32_t SLOT_CAP = 2048;                  // slots per batch (12 bits of a relabelled word and of the reservation word)
static constexpr uint32_t HIST_BINS = 512;
// The histograms exist HIST_SHARDS times: a workgroup flushes its LDS counts into copy blockIdx & 3 (consecutive workgroups run on different XCDs), the
// readers (k_expand) add the copies.  A batch's splitting leaves are a dozen, their hot bins a few hundred words, and five hundred workgroups flush
// into them within the same microseconds: a memory-side atomic of k_hist spent ~3 000 cycles in flight against 500-700 in every other kernel
// (profiles/r04, TCC_EA0_ATOMIC_LEVEL / TCC_EA0_ATOMIC: same-address atomics retire one after the other).
// Only the first HIST_SHARDED slots of a batch have the copies — a batch of a stream splits a dozen leaves; a batch that splits hundreds
// (a coalesced group, scattered points) spreads its adds over that many histograms anyway —: 1.5 MB of the momentary buffer instead of 12.
#ifndef HIST_SHARDS_N
#define HIST_SHARDS_N 4          // measured on one box, ms per 36 M ingest: 1 copy 3.69, 4 copies 3.65, 8 copies 3.79 (cycles in flight per memory-side atomic of k_hist: 2 965 / 1 150 / 846)
#endif
static constexpr uint32_t HIST_SHARDS = HIST_SHARDS_N, HIST_SHARDED = 256;
static_assert(HIST_SHARDS >= 1u && (HIST_SHARDS & (HIST_SHARDS - 1u)) == 0u, "a workgroup picks its copy with blockIdx & (HIST_SHARDS - 1)");
static constexpr uint64_t HIST_EXTRA_WORDS = (uint64_t)(HIST_SHARDS - 1u) * HIST_SHARDED * HIST_BINS;      // copies 1..3 of slots 0..255, behind the SLOT_CAP x HIST_BINS words of copy 0
// word of (slot << 9 | bin) in copy `shard`
__device__ __forceinline__ uint64_t hist_word(uint32_t key, uint32_t shard) {
	return (shard == 0u || (key >> 9) >= HIST_SHARDED) ? (uint64_t)key : (uint64_t)SLOT_CAP * HIST_BINS + (uint64_t)(shard - 1u) * HIST_SHARDED * HIST_BINS + key;
}
static constexpr uint32_t LEAF_FLAG = 0x80000000u;          // cached-leaf word: FLAG | slot << 9 | bin   (else: node index | bin below that node << 19, as k_count left it)
static constexpr uint32_t LEAF_BIN_SHIFT = 19;              // node indices travel in 19 bits (simlod_context_set_node_capacity: <= 2^19 nodes)
static constexpr uint32_t LEAF_NODE_MASK = (1u << LEAF_BIN_SHIFT) - 1u;
static constexpr uint32_t MAP_LISTED = 0x80000000u;         // map entry: LISTED | level << 16 | slot of the NEXT round   (else: a node index)
static constexpr uint32_t NONE = 0xffffffffu;
struct SlotRec { uint32_t node, level, childBase, spillBase, stored, born, pad1, pad2; };   // node == NONE: nothing could be reserved, the leaf stays as it is | born: NONE for a leaf that existed when the group began; else (an exact group, a node the cascade queued for its next round) the batch of the group in which the node split — when its children were created
__device__ __forceinline__ SlotRec* slot_recs(const BuildArgs& a, uint32_t ordinal) { return at<SlotRec>(a, a.offSlots) + (uint64_t)(ordinal & 1u) * SLOT_CAP; }   // (by parity, as the clear list)

// the three child choices below a node at `level`, most significant first (levels beyond MAX_DEPTH contribute zero bits)
__device__ __forceinline__ uint32_t bin_of(uint32_t X, uint32_t Y, uint32_t Z, uint32_t level) {
	uint32_t b = 0;
#pragma unroll
	for (uint32_t k = 0; k < 3; k++) {
		const uint32_t lv = level + k;
		b = (b << 3) | (lv < (uint32_t)SIMLOD_MAX_DEPTH ? (uint32_t)child_index(X, Y, Z, (int)lv) : 0u);
	}
	return b;
}

// One arrival-counter update for `cnt` samples (voxels.cu:203-218).  Returns CROSSED for exactly one caller per leaf and batch: the one
// that has to queue the leaf for splitting — whoever sees its counter cross the limit, or, if it is already over the limit because
// an earlier batch could not split it (spill space, node array or slots exhausted: the split is deferred, nothing is lost), whoever
// touches it first in this batch; the exchange on the per-node tag decides.  And FIRST for exactly one caller per leaf and batch too
// (another per-node tag): that caller puts the leaf on the batch's list of leaves with new samples (k_expand allocates their chunks from it).
// Node.numPoints is NOT looked at: the back half of the batch before (k_insert) may still be advancing it.  What the leaf held when this
// batch began — its counter before anybody's add — is the smallest `old` any caller sees: kept per node as tag << 32 | ~old under an
// atomic max (a newer batch's tag beats an older one, a smaller `old` a larger one).
static constexpr uint32_t CROSSED = 1u, FIRST = 2u;
// (in two halves, so that a caller with several leaves — the samples of a thread that found no room in the workgroup's table: a batch scattered
// over thousands of leaves — has all its loads and adds in flight before it looks at any of them)
struct CountPending { uint32_t touchSeen, old; unsigned long long startSeen; };
__device__ __forceinline__ CountPending count_issue(const BuildArgs& a, uint32_t leafIdx, uint32_t cnt) {
	// A batch that is scattered over thousands of leaves (BASELINE config 5: 4 096 leaves, every workgroup meets most of them) makes every workgroup
	// a caller for every leaf: the add is the work, the two tag words are bookkeeping that only the FIRST callers of a leaf change.  So the tag
	// words are looked at with plain loads first (in flight beside the add): a word that already carries this batch's tag — and, for the counter
	// at batch start, a value no larger than this caller's — cannot be changed by this caller, and its atomic is skipped.  A stale read (the
	// XCDs' L2s are not coherent) can only show an OLDER state: the atomic is then issued as before.  Config 5, 200 M points: k_count issued
	// 2.0 M memory-side atomics per batch (250 us) before, 0.73 M after; profiles/r05/config5_*.
	CountPending p;
	p.touchSeen = __hip_atomic_load(at<uint32_t>(a, a.offTouchTag) + leafIdx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	p.startSeen = __hip_atomic_load(at<unsigned long long>(a, a.offStartOf) + leafIdx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	p.old = atomicAdd(&a.nodes[leafIdx].counter, cnt);
	return p;
}
__device__ __forceinline__ uint32_t count_finish(const BuildArgs& a, const BatchCtl* bc, uint32_t leafIdx, uint32_t cnt, const CountPending& p) {
	SimlodNode* leaf = a.nodes + leafIdx;
	const uint32_t old = p.old;
	const uint32_t before = p.touchSeen == bc->tag ? bc->tag : atomicExch(at<uint32_t>(a, a.offTouchTag) + leafIdx, bc->tag);
	const unsigned long long mine = ((unsigned long long)bc->tag << 32) | (0xffffffffu - old);
	if (p.startSeen < mine) atomicMax(at<unsigned long long>(a, a.offStartOf) + leafIdx, mine);
	uint32_t flags = before != bc->tag ? FIRST : 0u;
	bool over = old + cnt > SIMLOD_MAX_POINTS_PER_NODE;
	if (!over && trunk_any(a)) over = trunk_forced(a, leaf->level, leaf->X, leaf->Y, leaf->Z);      // (a multi-GPU job's shared upper node: splits by the global count)
	// A node at MAX_DEPTH cannot be subdivided (the descent stops there): it keeps growing instead of spilling.
	if (over && leaf->level < SIMLOD_MAX_DEPTH && atomicExch(at<uint32_t>(a, a.offRetryTag) + leafIdx, bc->tag) != bc->tag) flags |= CROSSED;
	return flags;
}
__device__ __forceinline__ uint32_t count_into(const BuildArgs& a, const BatchCtl* bc, uint32_t leafIdx, uint32_t cnt) {
	return count_finish(a, bc, leafIdx, cnt, count_issue(a, leafIdx, cnt));
}
// what a leaf held when batch `tag` began (valid once the batch's k_count is complete)
__device__ __forceinline__ uint32_t stored_at_start(const BuildArgs& a, uint32_t tag, uint32_t leafIdx) {
	const unsigned long long v = at<const unsigned long long>(a, a.offStartOf)[leafIdx];
	return (uint32_t)(v >> 32) == tag ? 0xffffffffu - (uint32_t)v : 0u;
}

struct SpillWork {
	const SimlodChunk* chunk;
	uint32_t slot, dstBase, count, level;
	uint32_t pad0, pad1;
};

// Reserve `slots` split slots, `nodes` node slots and `spill` points of spill space TOGETHER (one 64-bit word: slots << 52 | nodes in use
// << 32 | spill in use), before anything is modified: a leaf that cannot be served now stays a leaf — too full, but intact — and is
// queued again by a later batch.
static constexpr int RSV_SLOT_SHIFT = 52;
__device__ __forceinline__ uint32_t slots_in_use(const BatchCtl* bc) {
	return (uint32_t)(__hip_atomic_load(&bc->reserve, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> RSV_SLOT_SHIFT);
}
// -> 0, or the error bit of what did not fit (nothing is raised: reserve() below does that; a caller that asks for several things at once decides itself)
__device__ __forceinline__ uint32_t reserve_try(const BuildArgs& a, BatchCtl* bc, uint32_t slots, uint32_t nodes, uint32_t spill, uint32_t& slotBase, uint32_t& nodeBase, uint32_t& spillBase) {
	// ONE add on the packed word hands out the three ranges; a caller that finds any of them beyond its capacity takes its add back and fails.  While such
	// a failed add stands, every other caller sees that field beyond its capacity too and fails as well (conservatively: the leaf stays as it is and is
	// queued again later) — so a caller that SUCCEEDS never got its ranges on top of amounts that are taken back afterwards.  The fields have room for
	// what can stand at once: a round has at most (group + moved samples) / 50 000 nodes that ask for a slot, and at most one cascade per workgroup
	// (<= 8 x 72 nodes each) that asks for nodes.  (Rounds 2-5: a compare-and-swap loop — forty cascades of a group of batches queued behind each other
	// on this word, a round trip each: 35 of k_expand's 56 us per slot.)
	const unsigned long long inc = ((unsigned long long)slots << RSV_SLOT_SHIFT) + ((unsigned long long)nodes << 32) + spill;
	const unsigned long long old = atomicAdd(&bc->reserve, inc);
	slotBase = (uint32_t)(old >> RSV_SLOT_SHIFT); nodeBase = (uint32_t)(old >> 32) & 0xfffffu; spillBase = (uint32_t)old;
	const bool okSlots = slotBase + slots <= SLOT_CAP, okNodes = nodeBase + nodes <= a.nodeCapacity, okSpill = (unsigned long long)spillBase + spill <= a.spilledCap;
	if (okSlots && okNodes && okSpill) { atomicAdd(&a.stats->numNodes, nodes); return 0u; }       // voxels.cu:317
	atomicAdd(&bc->reserve, 0ull - inc);
	return !okSlots ? SIMLOD_ERR_SPILLING_OVERFLOW : !okNodes ? SIMLOD_ERR_NODES_EXHAUSTED : SIMLOD_ERR_SPILLED_OVERFLOW;      // more leaves cross the limit at once than a batch has slots for | node array full | spill space
}
__device__ __forceinline__ bool reserve(const BuildArgs& a, Ctl* ctl, BatchCtl* bc, uint32_t slots, uint32_t nodes, uint32_t spill, uint32_t& slotBase, uint32_t& nodeBase, uint32_t& spillBase) {
	const uint32_t err = reserve_try(a, bc, slots, nodes, spill, slotBase, nodeBase, spillBase);
	if (err != 0u) raise(ctl, err);
	return err == 0u;
}

// the occupancy grid of a node that splits in this batch: allocated if the node has none (voxels.cu:363-365), cleared in any case
// (:371-382, also the root's, which has one from the reset on) — by k_insert, through this list; the grids are first read by k_voxelize
// (two copies of the list, by the batch's parity: k_queue of the next batch fills its list while k_insert of this one is still clearing)
__device__ __forceinline__ SimlodOccupancyGrid** clear_list(const BuildArgs& a, uint32_t ordinal) { return at<SimlodOccupancyGrid*>(a, a.offClear) + (uint64_t)(ordinal & 1u) * a.clearCap; }
__device__ __forceinline__ void note_clear(const BuildArgs& a, const BatchCtl* bc, uint32_t c, SimlodOccupancyGrid* g) {
	if (c < a.clearCap) clear_list(a, bc->ordinal)[c] = g;
	else {                                                        // (never: the list holds a grid per node slot a batch can create)
		uint4* w = reinterpret_cast<uint4*>(g->values);
		for (uint32_t i = 0; i < SIMLOD_GRID_NUM_WORDS / 4; i++) w[i] = make_uint4(0, 0, 0, 0);
	}
}
// the grids of `count` such nodes at once (k_expand: a slot's splitting children and grandchildren and its next-round nodes): ONE allocation (the counted form: the allocator's offset advances as by `count` single ones) and ONE add on the list's length;
// grid k of them is grid_of_many(mem, k), and its list entry clearBase + k (note_clear)
__device__ __forceinline__ uint8_t* grids_for_splits(const BuildArgs& a, BatchCtl* bc, uint32_t count, uint32_t& clearBase) {
	uint8_t* mem = persistent_alloc(a.pers, sizeof(SimlodOccupancyGrid), count);          // (two independent atomics with a return value: one round trip)
	clearBase = atomicAdd(&bc->numClear, count);
	return mem;
}
__device__ __forceinline__ SimlodOccupancyGrid* grid_of_many(uint8_t* mem, uint32_t k) { return reinterpret_cast<SimlodOccupancyGrid*>(mem + (uint64_t)k * SIMLOD_ALLOC_ROUND(sizeof(SimlodOccupancyGrid))); }

// Queue leaf `nodeIdx` for splitting: ONE WAVE (k_queue).  Everything the split needs is reserved here, before anything is modified: a slot (and
// with it a histogram), eight node slots and the spill space for the stored points together, the occupancy grid.  Then the leaf's
// chunk list becomes spill-copy work items (chunk k comes from the leaf chunk table, not from a walk) and goes back to the recycle
// stack (voxels.cu:346-357; nothing pops before alloc_points in k_expand).  (voxels.cu:308-383 doSplitting, first half)
// sum over the wave and the sum of the lanes below (every lane of the wave calls)
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t& total) {
	const uint32_t lane = (uint32_t)lane_id();
	uint32_t x = v;
#pragma unroll
	for (uint32_t o = 1; o < 64u; o <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64); if (lane >= o) x += y; }
	total = (uint32_t)__shfl((int)x, 63, 64);
	return x - v;
}
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
	return ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, 64);
}

// What a crossing leaf needs reserved — a slot, eight node slots, spill space for its stored points, places in the work list and on the recycle
// stack for its chunks — follows from ITS PLACE IN THE LIST: entry e takes slot e, the nodes from 8 e on, and the spill / work / stack ranges behind
// those of the entries before it (a prefix sum over the list, which every wave computes for itself from the leaves' stored counts: plain loads, no
// atomic).  Round 5 reserved per leaf with a compare-and-swap on one word: forty leaves of a group of batches queued behind each other, a round trip
// each (k_queue: 55 us per group of five batches).  An entry is served iff everything up to and including it fits (slots, node array, spill
// space): once one does not, none behind it does — those leaves stay as they are, too full but intact, and are queued again by a later batch.
struct CrossPrefix { uint32_t stored, chunks, storedBefore, chunksBefore; bool ok; };
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
	return v;
}
// entry e of the list: its own numbers and the sums over the entries before it (every lane of the wave calls; all get the result)
__device__ CrossPrefix cross_prefix(const BuildArgs& a, const BatchCtl* bc, const uint32_t* crossList, uint32_t numCross, uint32_t e, uint32_t slots0, uint32_t nodes0, uint32_t spill0) {
	const uint32_t lane = (uint32_t)lane_id();
	CrossPrefix r{0u, 0u, 0u, 0u, false};
	for (uint32_t c0 = 0; c0 <= e; c0 += 64u) {
		const uint32_t idx = c0 + lane;
		uint32_t st = 0, ch = 0;
		if (idx < numCross && idx <= e) {
			const uint32_t leaf = crossList[idx];
			// (not Node.numPoints, which the back half of the group before may still be advancing — and which is reset, with the list's head,
			// by k_expand, after that back half: this kernel runs beside it); between batches stored == counter, so the list holds exactly ceil(stored / 1000) chunks
			st = stored_at_start(a, bc->tag, leaf);
			ch = a.nodes[leaf].points != nullptr ? (st + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK : 0u;
		}
		if (e - c0 < 64u) {        // the chunk that holds entry e
			r.stored = (uint32_t)__shfl((int)st, (int)(e - c0), 64); r.chunks = (uint32_t)__shfl((int)ch, (int)(e - c0), 64);
			r.storedBefore += wave_sum_u32(idx < e ? st : 0u); r.chunksBefore += wave_sum_u32(idx < e ? ch : 0u);
		} else { r.storedBefore += wave_sum_u32(st); r.chunksBefore += wave_sum_u32(ch); }
	}
	r.ok = slots0 + e + 1u <= SLOT_CAP && nodes0 + 8u * (e + 1u) <= a.nodeCapacity && (unsigned long long)spill0 + r.storedBefore + r.stored <= a.spilledCap;
	return r;
}

__device__ void queue_split(const BuildArgs& a, Ctl* ctl, BatchCtl* bc, const uint32_t* crossList, uint32_t numCross, uint32_t e) {
	const uint32_t lane = (uint32_t)lane_id();
	const uint32_t nodeIdx = crossList[e];
	SimlodNode* node = a.nodes + nodeIdx;
	// the leaf's row of the chunk table, a lane per chunk: asked for now, needed after the prefix (one round trip less on a kernel that is a chain of them)
	SimlodChunk* const rowChunk = lane < LEAF_SLOTS ? const_cast<SimlodChunk*>(leaf_row_get(a.mom + a.offLeafChunks, a.pers, nodeIdx, lane)) : nullptr;
	const uint32_t level = node->level;
	SimlodOccupancyGrid* grid = node->grid;
	const unsigned long long base = bc->reserve0;          // as k_count's first workgroup left it (bc->reserve itself: the list's totals, written below by the wave of entry 0)
	const uint32_t slots0 = (uint32_t)(base >> RSV_SLOT_SHIFT), nodes0 = (uint32_t)(base >> 32) & 0xfffffu, spill0 = (uint32_t)base;
	const CrossPrefix cp = cross_prefix(a, bc, crossList, numCross, e, slots0, nodes0, spill0);
	if (!cp.ok) {
		if (lane == 0u) raise(ctl, slots0 + e + 1u > SLOT_CAP ? SIMLOD_ERR_SPILLING_OVERFLOW : nodes0 + 8u * (e + 1u) > a.nodeCapacity ? SIMLOD_ERR_NODES_EXHAUSTED : SIMLOD_ERR_SPILLED_OVERFLOW);
		return;
	}
	const uint32_t slot = slots0 + e, childBase = nodes0 + 8u * e, spillBase = spill0 + cp.storedBefore, stored = cp.stored, numChunks = cp.chunks, w0 = cp.chunksBefore;
	const unsigned long long top = (unsigned long long)bc->acctAlloc0 - cp.chunksBefore;      // Stats.numAllocatedChunks as this leaf's turn finds it (voxels.cu:346-357)
	if (lane == 0u) {
		if (grid == nullptr) {                                                               // voxels.cu:363-365
			SimlodAllocatorGlobal* alloc = reinterpret_cast<SimlodAllocatorGlobal*>(a.pers);
			grid = reinterpret_cast<SimlodOccupancyGrid*>(a.pers + atomicAdd(reinterpret_cast<unsigned long long*>(&alloc->offset), (unsigned long long)SIMLOD_ALLOC_ROUND(sizeof(SimlodOccupancyGrid))));
			node->grid = grid;
		}
		note_clear(a, bc, e, grid);
		slot_recs(a, bc->ordinal)[slot] = SlotRec{nodeIdx, level, childBase, spillBase, stored, NONE, 0u, 0u};
		at<unsigned long long>(a, a.offSplitTag)[nodeIdx] = ((unsigned long long)bc->tag << 32) | (level << 16) | slot;      // (the group's tag: unique while the octree lives, like every tag word)
	}
	// the slot's histogram starts from zero
	{
		for (uint32_t sd = 0; sd < (slot < HIST_SHARDED ? HIST_SHARDS : 1u); sd++) {
			uint4* h = reinterpret_cast<uint4*>(at<uint32_t>(a, a.offHist) + hist_word(slot << 9, sd));
			h[lane] = make_uint4(0, 0, 0, 0); h[lane + 64] = make_uint4(0, 0, 0, 0);
		}
		if (bc->acct != 0u) {      // (an exact group: the slot's histograms per batch)
			uint4* hb = reinterpret_cast<uint4*>(at<uint32_t>(a, a.offHistB) + (uint64_t)slot * HIST_BINS * a.groupMax);
			for (uint32_t i = lane; i < HIST_BINS / 4u * a.groupMax; i += 64u) hb[i] = make_uint4(0, 0, 0, 0);
		}
	}
	SimlodChunk** chunkQueue = at<SimlodChunk*>(a, a.offQueue);
	SpillWork* work = at<SpillWork>(a, a.offWork);
	auto emit = [&](uint32_t ci, SimlodChunk* chunk) {
		if (w0 + ci < a.workCap) {
			SpillWork w;
			w.chunk = chunk; w.slot = slot; w.dstBase = spillBase + ci * SIMLOD_POINTS_PER_CHUNK;
			w.count = min(stored - ci * SIMLOD_POINTS_PER_CHUNK, SIMLOD_POINTS_PER_CHUNK); w.level = level; w.pad0 = 0; w.pad1 = 0;
			work[w0 + ci] = w;
		} else raise(ctl, SIMLOD_ERR_SPILLED_OVERFLOW);
		const unsigned long long q = top - numChunks + ci;
		if (q < CHUNK_QUEUE_CAPACITY) chunkQueue[q] = chunk; else raise(ctl, SIMLOD_ERR_CHUNK_QUEUE_OVERFLOW);
	};
	SimlodChunk* beyond = nullptr;                      // chunk #LEAF_SLOTS of a leaf whose split was deferred and that kept growing
	if (lane == 0 && numChunks > LEAF_SLOTS) beyond = leaf_row_get(a.mom + a.offLeafChunks, a.pers, nodeIdx, LEAF_SLOTS - 1)->next;
	if (lane < min(numChunks, LEAF_SLOTS)) {                          // (LEAF_SLOTS <= 64: one chunk per lane)
		emit(lane, rowChunk);
		rowChunk->next = nullptr;
	}
	if (lane == 0) {
		for (uint32_t ci = LEAF_SLOTS; ci < numChunks && beyond != nullptr; ci++) {   // the table has no slot for these: walk
			SimlodChunk* next = beyond->next;
			emit(ci, beyond);
			beyond->next = nullptr;
			beyond = next;
		}
	}
}
// the list's totals (the wave that takes entry 0): how many entries are served — everything up to the first that does not fit — and what they take
__device__ void queue_totals(const BuildArgs& a, Ctl* ctl, BatchCtl* bc, const uint32_t* crossList, uint32_t numCross) {
	const uint32_t lane = (uint32_t)lane_id();
	const unsigned long long base = bc->reserve0;
	const uint32_t slots0 = (uint32_t)(base >> RSV_SLOT_SHIFT), nodes0 = (uint32_t)(base >> 32) & 0xfffffu, spill0 = (uint32_t)base;
	uint32_t served = 0, stored = 0, chunks = 0;
	bool open = true;
	for (uint32_t c0 = 0; c0 < numCross && open; c0 += 64u) {
		const uint32_t idx = c0 + lane;
		uint32_t st = 0, ch = 0;
		if (idx < numCross) {
			const uint32_t leaf = crossList[idx];
			st = stored_at_start(a, bc->tag, leaf);
			ch = a.nodes[leaf].points != nullptr ? (st + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK : 0u;
		}
		uint32_t totSt, totCh;
		const uint32_t exSt = wave_exclusive(st, totSt), exCh = wave_exclusive(ch, totCh);
		const bool ok = idx < numCross && slots0 + idx + 1u <= SLOT_CAP && nodes0 + 8u * (idx + 1u) <= a.nodeCapacity && (unsigned long long)spill0 + stored + exSt + st <= a.spilledCap;
		// the served entries of this chunk are a prefix of it: the lanes below the first that does not fit
		const unsigned long long okMask = __ballot(ok), valid = __ballot(idx < numCross), firstFail = ~okMask & valid;
		const uint32_t here = firstFail != 0ull ? (uint32_t)__ffsll((long long)firstFail) - 1u : (uint32_t)__popcll(valid);
		served += here;
		stored += here < 64u ? (uint32_t)__shfl((int)exSt, (int)here, 64) : totSt;
		chunks += here < 64u ? (uint32_t)__shfl((int)exCh, (int)here, 64) : totCh;
		if (firstFail != 0ull) open = false;
	}
	if (lane == 0u) {
		bc->reserve = base + ((unsigned long long)served << RSV_SLOT_SHIFT) + ((unsigned long long)(8u * served) << 32) + stored;
		if (served != 0u) atomicAdd(&a.stats->numNodes, 8u * served);                        // voxels.cu:317
		if (chunks != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(&a.stats->numAllocatedChunks), (unsigned long long)(-(long long)chunks));   // voxels.cu:346-357
		bc->numClear = served; bc->numWork = chunks; bc->numSpilled = stored;
	}
}

// ---- exact groups of several batches: the allocator / chunk-pool counters of batch-by-batch ingestion -----------------------------------
// In EXACT mode a launch that finds several pending batches ingests up to groupMax of them as ONE group — one descent, one insert, one voxel
// pass over all their samples, the throughput regime of the chip — where the reference ingests them one after the other (voxels.cu:883-949).
// Topology, per-node sample multisets, occupancy grids, voxel positions and counts do not depend on that granularity (a leaf splits iff what
// lies in its cell exceeds 50 000; a grid holds the cells of every sample that passed through the node).  What does:
//   * Node.counter of an inner node — what lay in its cell after the batch in which it split (voxels.cu:203-218: later batches descend past it);
//   * Stats.numAllocatedChunks' excursions, hence Stats.chunkPoolSize (its high-water mark, voxels.cu:535-537) and how many point chunks came
//     FRESH from the allocator instead of the recycle stack, hence Stats.allocatedBytes_persistent: a node that is created by one batch of the
//     group and split by a later one held chunks in between; a leaf takes its chunks batch by batch.
// Both follow from COUNTS PER BATCH alone: k_count keeps the samples per (leaf, batch of the group), k_hist / k_expand the 512-bin histograms
// per batch, and k_expand derives, for every node of a cascade, the batch it was created in (= the batch its parent split in), the batch it
// split in (the first in which its running count exceeds the limit), its counter at that moment, and the chunks it took and gave back in every
// batch: BatchCtl.acctD[k] / acctF[k] = point chunks batch k of the group takes / returns, summed over all nodes.  account_group() then replays
// voxels.cu:346-357 / 505-516 on those numbers — a stack pointer and a high-water mark — and makes the real counters agree: the chunks the
// batch-by-batch run would have taken fresh beyond what the group did are allocated now and put on the recycle stack, where that run would have
// left them.  The replay must end at the chunk count the octree really has (every chunk in use is in use in both runs): SIMLOD_ERR_ACCOUNTING otherwise.
struct Phantom { uint32_t base, count; unsigned long long mem; };      // recycle-stack entries [base, base + count) = fresh chunks from `mem` on (written by the whole workgroup)
__device__ Phantom account_group(const BuildArgs& a, Ctl* ctl, BatchCtl* g) {
	SimlodStats* s = a.stats;
	Phantom ph{0u, 0u, 0ull};
	if (g != nullptr && g->acct != 0u && g->accounted == 0u && ctl->abortBatch == 0u) {
		long long A = (long long)g->acctAlloc0, P = (long long)g->acctPool0;
		for (uint32_t k = 0; k < g->groupBatches; k++) {
			A -= (long long)g->acctF[k];            // voxels.cu:346-357: the batch's splits return their leaves' chunks first ...
			A += (long long)g->acctD[k];            // ... then its leaves take what they need (voxels.cu:505-516), from the stack while it has any
			if (A > P) P = A;                       // voxels.cu:535-537
		}
		const long long Areal = (long long)s->numAllocatedChunks;
		if (A != Areal) raise(ctl, SIMLOD_ERR_ACCOUNTING);
		const long long Preal = max((long long)g->acctPool0, Areal);          // what the group's own allocations made of the pool
		if (P > Preal && P <= (long long)CHUNK_QUEUE_CAPACITY) {
			ph.base = (uint32_t)Preal; ph.count = (uint32_t)(P - Preal);
			ph.mem = (unsigned long long)persistent_alloc(a.pers, sizeof(SimlodChunk), ph.count);
		}
		s->chunkPoolSize = (uint64_t)max(P, Preal);
		g->accounted = 1u;
	} else if (s->numAllocatedChunks > s->chunkPoolSize) s->chunkPoolSize = s->numAllocatedChunks;      // voxels.cu:535-537
	return ph;
}
__device__ __forceinline__ void phantom_fill(const BuildArgs& a, const Phantom& ph) {      // (every thread of the workgroup)
	SimlodChunk** chunkQueue = at<SimlodChunk*>(a, a.offQueue);
	for (uint32_t i = threadIdx.x; i < ph.count; i += blockDim.x) {
		SimlodChunk* c = reinterpret_cast<SimlodChunk*>(ph.mem + (unsigned long long)i * SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk)));
		c->next = nullptr;
		chunkQueue[ph.base + i] = c;
	}
}
// batch of the group that sample i belongs to
__device__ __forceinline__ uint32_t batch_of_sample(const BatchCtl* bc, uint32_t i) {
	uint32_t k = min(i / (uint32_t)SIMLOD_MAX_BATCH_SIZE, bc->groupBatches - 1u);
	while (k + 1u < bc->groupBatches && i >= bc->start[k + 1u]) k++;
	return k;
}
static constexpr uint32_t ACCT_BATCH_SHIFT = 21;       // keys of an exact group's LDS tables: (slot << 9 | bin) | batch << 21  (k_hist, k_expand); leaf | batch << 19 (k_count)
static constexpr uint32_t ACCT_MOVED = 31u;            // "batch" of a stored point a split moves: it was there before the group

// k_count takes more points per thread than k_insert (PPT): its cost is the flush of the per-workgroup counts into a few dozen
// hot leaf counters, and fewer, fatter workgroups mean fewer same-address atomics (measured: 8 -> -3.5 us, in k_insert +14 us)
#ifndef COUNT_CPT
#define COUNT_CPT 8
#endif
#ifndef HIST_CPT
#define HIST_CPT 8
#endif
static constexpr uint32_t CPT = COUNT_CPT;
static constexpr uint32_t HCPT = HIST_CPT, CPB = TPB * HCPT;         // (k_hist)

static constexpr uint32_t TOUCH_CAP = 512;         // leaves one workgroup can be the first to touch in one batch (more: appended one by one)

// The descents of a thread's P samples in lockstep, one level per step, through the child words (KID_*): P independent 4-byte loads in flight per step, and a
// step into a child that its parent's word marks as a leaf ends the descent without a load of its own.
template <int P>
__device__ __forceinline__ void descend_kids(const SimlodNode* nodes, const uint32_t* kid, uint32_t (&cur)[P], uint32_t (&level)[P], const uint32_t (&X)[P], const uint32_t (&Y)[P],
                                             const uint32_t (&Z)[P], bool (&walking)[P]) {
	bool any = true;
#pragma unroll 1
	for (int step = 0; step < SIMLOD_MAX_DEPTH && any; ++step) {
		uint32_t w[P];
#pragma unroll
		for (int j = 0; j < P; j++) w[j] = walking[j] && level[j] < (uint32_t)SIMLOD_MAX_DEPTH ? kid[cur[j]] : 0u;
		any = false;
#pragma unroll
		for (int j = 0; j < P; j++) {
			if (w[j] == 0u) { walking[j] = false; continue; }
			const uint32_t ci = (uint32_t)child_index(X[j], Y[j], Z[j], (int)level[j]);
			if (w[j] == KID_IRREGULAR) {                                      // (an image whose children are not eight consecutive nodes)
				const SimlodNode* c = nodes[cur[j]].children[ci];
				if (c == nullptr) { walking[j] = false; continue; }
				cur[j] = (uint32_t)(c - nodes); level[j] += 1u; any = true;
				continue;
			}
			cur[j] = (w[j] & LEAF_NODE_MASK) + ci; level[j] += 1u;
			if (((w[j] >> (KID_LEAF_SHIFT + ci)) & 1u) != 0u) walking[j] = false; else any = true;
		}
	}
}

template <uint32_t BT, bool SINGLE>
__global__ __launch_bounds__(BT) void k_count(BuildArgs a, uint32_t ordinal) {
	constexpr uint32_t CPB = BT * CPT;
	Ctl* ctl = ctl_of(a);
	BatchCtl* bc = batch_of(ctl, ordinal);
	if (bc == nullptr) return;
	constexpr uint32_t REP = 8;
	__shared__ SpreadTable<REP> tbl;
	__shared__ uint32_t sh_touch[TOUCH_CAP];
	__shared__ uint32_t sh_numTouch, sh_touchBase;
	const uint32_t n = bc->batchSize;
	const Samples<SINGLE> pts(a, bc);
	const LeafWords leafOf(a, ordinal);
	uint32_t* touched = at<uint32_t>(a, a.offTouched);
	uint32_t* crossList = at<uint32_t>(a, a.offCross);
	const uint32_t numChunks = (n + CPB - 1) / CPB;
	if (blockIdx.x == 0) {
		__shared__ Phantom sh_phantom;
		if (threadIdx.x == 0) {
			// what had to wait for k_expand of the group before: voxels.cu:535-537 — the chunk pool's high-water mark follows that group's
			// allocations, before this one recycles or takes a chunk (an exact group of several batches: account_group) — and the node array's fill,
			// where this group's reservations start (k_queue)
			sh_phantom = account_group(a, ctl, ordinal > 0u ? batch_of(ctl, ordinal - 1u) : nullptr);
			bc->acctAlloc0 = (uint32_t)a.stats->numAllocatedChunks; bc->acctPool0 = (uint32_t)a.stats->chunkPoolSize;
			bc->reserve = (unsigned long long)a.stats->numNodes << 32; bc->reserve0 = bc->reserve;
			if (ordinal == 0u) ctl->tableMagic = 0;     // the octree changes from here on: the side tables' stamp is valid again once k_finish has run (k_begin only reads it)
		}
		__syncthreads();
		phantom_fill(a, sh_phantom);
	}
	const bool acct = bc->acct != 0u;
	uint32_t* cntB = at<uint32_t>(a, a.offCntB);
	const bool trunkPass = blockIdx.x == 0 && trunk_any(a);     // (also for a group without samples: how a host flushes a mask it has just widened)
	if (blockIdx.x >= numChunks && !trunkPass) return;
	Phase ph(ctl, blockIdx.x == 0);
	auto counted = [&](uint32_t leafIdx, uint32_t flags) {
		if ((flags & FIRST) != 0u) {
			const uint32_t k = atomicAdd(&sh_numTouch, 1u);
			if (k < TOUCH_CAP) sh_touch[k] = leafIdx;
			else touched[atomicAdd(&bc->numTouched, 1u)] = leafIdx;       // (at most one entry per node and batch: the list has room for every node)
		}
		if ((flags & CROSSED) != 0u) {                                     // (rare: a handful per batch) k_queue reserves, lists and empties them
			const uint32_t k = atomicAdd(&bc->numCross, 1u);
			if (k < a.crossCap) crossList[k] = leafIdx;
			else { at<uint32_t>(a, a.offRetryTag)[leafIdx] = 0u; raise(ctl, SIMLOD_ERR_SPILLING_OVERFLOW); }   // deferred: a later batch queues it again
		}
	};
	// The LDS table lives for the whole workgroup: no barrier inside the chunk loop, so the waves never wait for each
	// other's slowest descent; one flush at the end.
	spread_init(tbl);
	if (threadIdx.x == 0) sh_numTouch = 0;
	__syncthreads();
	if (trunkPass && threadIdx.x < TRUNK_NODES) {
		// the upper nodes the host's mask names (simlod_context_set_trunk_mask): one that exists and is still a leaf is queued for splitting
		// whether this group has a sample for it or not — "counted" with zero samples, so the exchange on its tag makes ONE caller queue it
		const uint32_t t = threadIdx.x, level = t == 0u ? 0u : t < 9u ? 1u : 2u, code = t == 0u ? 0u : t < 9u ? t - 1u : t - 9u;
		if ((((t < 64u ? a.trunkLo : a.trunkHi) >> (t & 63u)) & 1ull) != 0ull) {
			uint32_t cur = 0;
			for (uint32_t lv = 0; lv < level && cur != NONE; lv++) {
				const SimlodNode* c = a.nodes[cur].children[(code >> (3u * (level - 1u - lv))) & 7u];
				cur = c != nullptr ? (uint32_t)(c - a.nodes) : NONE;
			}
			if (cur != NONE && node_is_leaf(a.nodes + cur)) counted(cur, count_into(a, bc, cur, 0u));
		}
	}
	for (uint32_t chunk = blockIdx.x; chunk < numChunks; chunk += gridDim.x) {
		float4 p[CPT];
		const float4* base; uint32_t kspan;
		const bool oneBatch = pts.span(chunk * CPB, min(n, (chunk + 1u) * CPB) - 1u, base, kspan);      // (workgroup-uniform)
#pragma unroll
		for (uint32_t j = 0; j < CPT; j++) {
			const uint32_t i = chunk * CPB + j * BT + threadIdx.x;
			p[j] = i < n ? (oneBatch ? base[i] : pts[i]) : make_float4(0, 0, 0, 0);
		}
		// the eight descents of a thread in lockstep, one level per step: eight L2 round trips in flight instead of eight chains of 5-8
		// dependent loads one after the other (that was the kernel: 21 us)
		uint32_t X[CPT], Y[CPT], Z[CPT], cur[CPT], level[CPT];
		bool walking[CPT];
#pragma unroll
		for (uint32_t j = 0; j < CPT; j++) {
			X[j] = quantize(F_GRID, p[j].x, a.minx, a.size); Y[j] = quantize(F_GRID, p[j].y, a.miny, a.size); Z[j] = quantize(F_GRID, p[j].z, a.minz, a.size);
			walking[j] = chunk * CPB + j * BT + threadIdx.x < n;
		}
		{   // the descent starts at the deepest node of level <= 5 above the sample (the top table: the eight loads go out together)
			const uint32_t* top = at<const uint32_t>(a, a.offTop);
			uint32_t e[CPT];
#pragma unroll
			for (uint32_t j = 0; j < CPT; j++) e[j] = walking[j] ? top[top_cell(X[j], Y[j], Z[j])] : 0u;
#pragma unroll
			for (uint32_t j = 0; j < CPT; j++) { cur[j] = e[j] & LEAF_NODE_MASK; level[j] = (e[j] >> 19) & 31u; walking[j] = walking[j] && (e[j] & TOP_LEAF) == 0u; }
		}
		descend_kids<(int)CPT>(a.nodes, at<const uint32_t>(a, a.offKid), cur, level, X, Y, Z, walking);
#pragma unroll
		for (uint32_t j = 0; j < CPT; j++) {
			const uint32_t i = chunk * CPB + j * BT + threadIdx.x;
			if (i >= n) continue;
			const uint32_t leafIdx = cur[j];
			leafOf.grp[i] = leafIdx | (bin_of(X[j], Y[j], Z[j], level[j]) << LEAF_BIN_SHIFT);      // the bin is what k_hist needs should this leaf split: it never reads the sample
			// (no room in the workgroup's table — a batch scattered over more leaves than it has keys —: the leaf's counters directly, one sample after the
			// other.  Round 5 measured all of a thread's spilled samples with their loads and adds in flight together: config 5 went from 60 to 71 ms)
			const uint32_t kb = !acct ? 0u : oneBatch ? kspan : batch_of_sample(bc, i);              // (an exact group: counts per leaf AND batch)
			if (!spread_add(tbl, leafIdx | (kb << LEAF_BIN_SHIFT), threadIdx.x & (REP - 1u))) {
				counted(leafIdx, count_into(a, bc, leafIdx, 1u));
				if (acct) atomicAdd(cntB + (uint64_t)leafIdx * a.groupMax + kb, 1u);
			}
		}
	}
	__syncthreads();
	ph.mark(0);
	for (uint32_t e = threadIdx.x; e < (uint32_t)TBL_CAP; e += BT) {
		const uint32_t key = tbl.keys[e];
		if (key == TBL_EMPTY) continue;
		const uint32_t leafIdx = key & LEAF_NODE_MASK, cnt = spread_sum(tbl, e);
		counted(leafIdx, count_into(a, bc, leafIdx, cnt));
		if (acct) atomicAdd(cntB + (uint64_t)leafIdx * a.groupMax + (key >> LEAF_BIN_SHIFT), cnt);
	}
	__syncthreads();
	ph.mark(1);
	// the leaves this workgroup was the first to touch in this batch go on the batch's list (one reservation per workgroup)
	const uint32_t numTouch = min(sh_numTouch, TOUCH_CAP);
	if (threadIdx.x == 0 && numTouch != 0u) sh_touchBase = atomicAdd(&bc->numTouched, numTouch);
	__syncthreads();
	for (uint32_t e = threadIdx.x; e < numTouch; e += BT) touched[sh_touchBase + e] = sh_touch[e];
	if (ph.on) ctl->phaseNs[3] += 1;
}

// ---- queue: the leaves k_count saw cross the limit are reserved, listed and emptied (voxels.cu:308-383 doSplitting, first half) -------------
// One wave per leaf.  Runs beside the back half of the batch BEFORE (whose k_insert may still be storing points into these very leaves): it
// reads what k_count and the allocator know — the counter at batch start, the chunk table — and writes only chunk links, the recycle stack
// and reservations; k_hist, which moves the points, is the kernel that waits for that k_insert.
__global__ __launch_bounds__(TPB) void k_queue(BuildArgs a, uint32_t ordinal) {
	Ctl* ctl = ctl_of(a);
	BatchCtl* bc = batch_of(ctl, ordinal);
	if (bc == nullptr || ctl->abortBatch) return;
	const uint32_t numCross = min(bc->numCross, a.crossCap);
	if (numCross == 0u) return;
	// SIMLOD_DEBUG_FORCE_BARRIER_TIMEOUT: behave as if k_expand's grid barrier had given up, before anything is modified (tests the abort path)
	if ((ctl->debugFlags & 1u) != 0u) { if (blockIdx.x == 0 && threadIdx.x == 0) panic(ctl, SIMLOD_ERR_BARRIER_TIMEOUT); return; }
	const uint32_t* crossList = at<const uint32_t>(a, a.offCross);
	const uint32_t wave = (blockIdx.x * TPB + threadIdx.x) / 64u, numWaves = gridDim.x * TPB / 64u;
	for (uint32_t e = wave; e < numCross; e += numWaves) queue_split(a, ctl, bc, crossList, numCross, e);
	if (wave == 0u) queue_totals(a, ctl, bc, crossList, numCross);
}
