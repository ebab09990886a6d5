// construct_expand.inc — part of construct.hip (included there, inside namespace simlod::build; not a translation unit of its own): k_voxelize's work items, the chunks of the leaves with new samples (alloc_points), k_hist and k_expand: the split cascade by histogram.

// ---- k_voxelize's work items (filled by the chunk allocation below) -----------------------------------------------------
static constexpr uint32_t VTPB = 1024;
#ifndef VOX_SPT_N
#define VOX_SPT_N 8
#endif
static constexpr uint32_t VOX_SPT = VOX_SPT_N;                  // samples per thread, kept in registers across both passes
static constexpr uint32_t VOX_PIECE = VTPB * VOX_SPT;           // 8192 samples per workgroup
static constexpr uint32_t VOX_BIG_ITEMS = 65536;                // entries of the item array for k_voxelize's pieces; the rest: one small item per leaf
static constexpr uint32_t VOX_SMALL = 512;                      // a leaf with fewer new samples than this takes the wave-per-leaf path ...
static constexpr uint32_t VOX_SMALL_PIECE = 128;                // ... in items of at most this many samples (two steps of a wave)
static constexpr uint32_t LDS_LEVELS = 7;                       // ancestors d = 1..7 own a cube of side 128 >> d; from d = 8 on: one cell
static constexpr uint32_t CUBE_WORDS = 8192 + 1024 + 256 + 64 + 16 + 4 + 4;
struct VoxItem { uint32_t leaf, s0, s1, ptBase, ptFirst; };   // samples [s0, s1) of the leaf's storage; its chunk directory; leaf = node index | level << 24   (20 bytes: the leaf's coordinates come from its node)
__device__ __forceinline__ VoxItem* vox_items(const BuildArgs& a, const BatchCtl* bc) { return at<VoxItem>(a, a.offVoxItems) + (uint64_t)(bc->ordinal & 1u) * a.voxItemCap; }

// ---- chunks for the leaves with new samples ----------------------------------------------------------------------------
// The point chunks of the leaves with new samples and their share of k_voxelize's work list (voxels.cu:485-538), for ALLOC_LEAVES entries
// of the batch's list: ONE WORKGROUP.
//   phase 1, the first `waves` waves, one leaf per lane: how many chunks, directory entries and work items each leaf needs; the reservations of the wave's
//     leaves — directory entries, chunks off the recycle stack (voxels.cu:505-516), work items, memory for the chunks the stack cannot
//     serve — are summed over the wave and made with ONE atomic each (the words they advance are shared by every leaf of the batch, and
//     device-scope atomics on one word retire at ~88 M/s here);
//   phase 2, all waves, one NEW CHUNK per lane: fetch it (stack or fresh memory), link it, enter it in the chunk directory and the leaf
//     chunk table.  A leaf the batch has filled from nothing needs 50 chunks; taken one after the other by the leaf's lane that was 50
//     dependent round trips (the whole of round 2's allocation kernel: 13 us), taken side by side it is two.
// The number of waves that take leaves is a RUN-TIME argument of a call (64 leaves per wave): the lists of touched leaves and the ordinary slot (8.7 fresh
// leaves on average) take one wave — its four wave-wide sums and four atomics are the whole of phase 1 —, a slot whose cascade made more than 64 fresh
// leaves takes a wave per 64 of them in ONE turn (a group of several batches hands a root's or a flooded leaf's cascade over at once: up to 584 nodes; with
// one wave that was nine turns of ~5 us each, one behind the other).  ALLOC_WAVES_N is the most a call can ask for: enough for every node a slot can create.
#ifndef ALLOC_WAVES_N
#define ALLOC_WAVES_N 10
#endif
static constexpr uint32_t ALLOC_WAVES = ALLOC_WAVES_N, ALLOC_LEAVES = 64 * ALLOC_WAVES;      // waves, leaves of a call at most
struct AllocRec {
	uint32_t node, existing, additional, fromPool;
	uint32_t dirNew, prefix;                                // directory entry of the leaf's first new chunk | new chunks of the lanes below
	unsigned long long firstIdx, mem;                       // recycle-stack index of the first new chunk | memory of the first one the stack could not serve
	SimlodChunk* head; SimlodChunk* tail;                   // the list as it is (nullptr: empty)
};
struct AllocShared { uint32_t waveTotal[ALLOC_WAVES]; };
struct FreshLeaf { uint32_t node, samples, level, X, Y, Z; };      // a leaf a cascade has just made: what alloc_points would otherwise read back from the node it was written to a moment ago

// Entry k is taken when firstEntry + lane < numEntries.  `touched` (global memory): the leaves k_count found new samples for — what
// each held when the batch began comes from stored_at_start().  `fresh` (LDS): {node, samples} of the empty leaves a cascade has
// just made (nothing about them has to be read back).  One of the two lists is given.
// (rec: 64 * waves records in LDS — k_expand lends the words of its hash table; waves <= ALLOC_WAVES, the same for every thread of the workgroup)
__device__ void alloc_points(const BuildArgs& a, Ctl* ctl, BatchCtl* bc, AllocShared& sh, AllocRec* rec, const uint32_t* touched, const FreshLeaf* fresh, uint32_t firstEntry, uint32_t numEntries, uint32_t waves) {
	const bool fresh_leaves = fresh != nullptr;
	NodeDir* nodeDir = at<NodeDir>(a, a.offNodeDir);
	SimlodChunk** chunkDir = chunk_dir(a, bc);
	SimlodChunk** chunkQueue = at<SimlodChunk*>(a, a.offQueue);
	uint8_t* const leafChunks = a.mom + a.offLeafChunks;
	if (threadIdx.x < 64u * waves) {
		const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
		firstEntry += wv * 64u;                                         // (this wave's 64 entries)
		// (Node.numPoints is not looked at: the back half of the batch before may still be advancing it)
		const unsigned long long pool = a.stats->chunkPoolSize;         // raised only by prepare_batch, between the groups' allocations (asked for here: in flight beside everything below)
		FreshLeaf fl = FreshLeaf{NONE, 0u, 0u, 0u, 0u, 0u};
		if (firstEntry + lane < numEntries) { if (fresh_leaves) fl = fresh[firstEntry + lane]; else fl.node = touched[firstEntry + lane]; }
		const uint2 entry = make_uint2(fl.node, fl.samples);
		const uint32_t i = entry.x, stored = (fresh_leaves || i == NONE) ? 0u : stored_at_start(a, bc->tag, i);
		SimlodNode* node = a.nodes + (i != NONE ? i : 0u);
		uint32_t counter = 0;
		bool need = false;
		SimlodChunk* head = nullptr;
		if (i != NONE && fresh_leaves) { counter = entry.y; need = counter != 0u; }
		else if (i != NONE) {
			// (a leaf that k_count's tail has queued for splitting still looks like a leaf until k_expand gives it children: not this one's business)
			const bool queued = (uint32_t)(at<const unsigned long long>(a, a.offSplitTag)[i] >> 32) == bc->tag;
			counter = node->counter; head = node->points; need = !queued && stored < counter && node_is_leaf(node);
		}
		if (bc->acct != 0u && !fresh_leaves) {
			// An exact group of several batches: a leaf takes its chunks batch by batch (voxels.cu:485-538) — batch k of the group brings it from
			// ceil(count before / 1000) to ceil(count after / 1000) chunks; k_count kept the leaf's samples per batch.  Summed over the wave, one add per
			// batch (account_group replays them).  The row is left as it was found: zero.  (The nodes of a cascade: k_expand, from the histograms.)
			uint32_t* row = at<uint32_t>(a, a.offCntB) + (uint64_t)(i != NONE ? i : 0u) * a.groupMax;
			uint32_t c = stored, have = (stored + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
			for (uint32_t k = 0; k < bc->groupBatches; k++) {
				uint32_t delta = 0;
				if (i != NONE) {
					c += row[k]; row[k] = 0u;
					const uint32_t want = (c + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
					if (need) delta = want - have;
					have = want;
				}
				uint32_t sum;
				(void)wave_exclusive(delta, sum);
				if (lane == 0u && sum != 0u) atomicAdd(&bc->acctD[k], sum);
			}
		}
		const uint32_t required = (counter + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
		const uint32_t existing = need ? (stored + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK : 0u;
		const uint32_t first = stored / SIMLOD_POINTS_PER_CHUNK;       // chunk that receives slot `stored`
		const uint32_t entries = need ? required - first : 0u;
		const uint32_t additional = need ? required - existing : 0u;
		const uint32_t fresh = need ? counter - stored : 0u;
		SimlodChunk* tail = existing > 0u ? tail_of(head) : nullptr;
		if (existing == 0u) head = nullptr;
		// the leaf's new samples [stored, counter) are k_voxelize's work, in pieces one workgroup takes — or, when they are few,
		// voxelize_small's, one wave per leaf (big items: the first VOX_BIG_ITEMS entries of the item array — a piece has at least
		// VOX_SMALL samples or is the last of its leaf, so they cover 33 M samples; small items behind them: one per leaf at most)
		const uint32_t pieces = fresh < VOX_SMALL ? 0u : (fresh + VOX_PIECE - 1) / VOX_PIECE;
		if (i == 0u && pieces != 0u) bc->rootPieces = pieces;          // (the root as a leaf: k_voxroot's pieces)
		const uint32_t small = need && pieces == 0u ? (fresh + VOX_SMALL_PIECE - 1) / VOX_SMALL_PIECE : 0u;
		uint32_t totEntries, totAdditional, totPieces, totSmall;
		const uint32_t exEntries = wave_exclusive(entries, totEntries), exAdditional = wave_exclusive(additional, totAdditional);
		const uint32_t exPieces = wave_exclusive(pieces, totPieces), exSmall = wave_exclusive(small, totSmall);
		uint32_t dirBase = 0, itemBase = 0, smallBase = 0;
		unsigned long long chunkBase = 0;
		if (lane == 0u) {                                              // (four independent atomics with a return value: one round trip)
			if (totEntries != 0u) dirBase = atomicAdd(&bc->dirCount, totEntries);
			if (totAdditional != 0u) chunkBase = atomicAdd(reinterpret_cast<unsigned long long*>(&a.stats->numAllocatedChunks), (unsigned long long)totAdditional);
			if (totPieces != 0u) itemBase = atomicAdd(&bc->numVoxItems, totPieces);
			if (totSmall != 0u) smallBase = atomicAdd(&bc->numVoxSmall, totSmall);
			sh.waveTotal[wv] = totAdditional;
		}
		dirBase = (uint32_t)__shfl((int)dirBase, 0, 64); itemBase = (uint32_t)__shfl((int)itemBase, 0, 64); smallBase = (uint32_t)__shfl((int)smallBase, 0, 64);
		chunkBase = shfl64(chunkBase, 0);
		// pop from the recycle stack, allocate what the stack cannot serve
		const unsigned long long firstIdx = chunkBase + exAdditional;
		const uint32_t fromPool = firstIdx >= pool ? 0u : (uint32_t)min((unsigned long long)additional, pool - firstIdx);
		uint32_t totNew;
		const uint32_t exNew = wave_exclusive(additional - fromPool, totNew);
		unsigned long long mem = 0;
		if (lane == 0u && totNew != 0u) mem = (unsigned long long)persistent_alloc(a.pers, sizeof(SimlodChunk), totNew);
		mem = shfl64(mem, 0) + (unsigned long long)exNew * SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk));
		const uint32_t base = dirBase + exEntries;
		const uint32_t itemAt = pieces != 0u ? itemBase + exPieces : VOX_BIG_ITEMS + smallBase + exSmall;
		bool ok = need;
		if (need && base + entries > a.dirCap) { panic(ctl, SIMLOD_ERR_DIRECTORY_FULL); ok = false; }
		if (need && (pieces != 0u ? itemAt + pieces > VOX_BIG_ITEMS : itemAt + small > a.voxItemCap)) { panic(ctl, SIMLOD_ERR_DIRECTORY_FULL); ok = false; }   // a batch + moved points beyond 33 M samples
		uint32_t e = 0;
		if (ok) {
			if (first < existing) chunkDir[base + e++] = tail;          // the partially filled tail chunk
			NodeDir& d = nodeDir[i];
			d.ptBase = base; d.ptFirst = first; d.ptTag = bc->tag;
			VoxItem* items = vox_items(a, bc);
			const uint32_t nl = fresh_leaves ? fl.level : node->level;
			if (pieces == 0u) for (uint32_t q = 0; q < small; q++) items[itemAt + q] = VoxItem{i | nl << 24, stored + q * VOX_SMALL_PIECE, min(stored + (q + 1u) * VOX_SMALL_PIECE, counter), base, first};
			else for (uint32_t q = 0; q < pieces; q++) items[itemAt + q] = VoxItem{i | nl << 24, stored + q * VOX_PIECE, min(stored + (q + 1u) * VOX_PIECE, counter), base, first};
		}
		AllocRec& r = rec[threadIdx.x];
		r.node = i; r.existing = existing; r.additional = ok ? additional : 0u; r.fromPool = fromPool; r.dirNew = base + e; r.prefix = exAdditional;
		r.firstIdx = firstIdx; r.mem = mem; r.head = head; r.tail = tail;
	}
	__syncthreads();
	// phase 2: new chunk q of the workgroup = chunk k of the leaf whose prefix covers q
	uint32_t total = 0;
	for (uint32_t w = 0; w < waves; w++) total += sh.waveTotal[w];
	for (uint32_t q0 = threadIdx.x; q0 < total; q0 += blockDim.x) {
		uint32_t q = q0, wv = 0;                                         // the wave whose leaves new chunk q0 belongs to, and its number among that wave's
		while (wv + 1u < waves && q >= sh.waveTotal[wv]) { q -= sh.waveTotal[wv]; wv++; }
		uint32_t lo = wv * 64u, hi = lo + 64u;                           // the last leaf with prefix <= q (leaves without new chunks share their successor's prefix)
		while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (rec[mid].prefix <= q) lo = mid; else hi = mid; }
		const AllocRec r = rec[lo];
		const uint32_t k = q - r.prefix;
		if (k >= r.additional) continue;                                 // (a leaf that could not be served: its reservation stays unused)
		auto chunk_at = [&](uint32_t j) -> SimlodChunk* {
			return j < r.fromPool ? chunkQueue[r.firstIdx + j] : reinterpret_cast<SimlodChunk*>(r.mem + (unsigned long long)(j - r.fromPool) * SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk)));
		};
		SimlodChunk* c = chunk_at(k);
		SimlodChunk* next = k + 1u < r.additional ? chunk_at(k + 1u) : nullptr;
		SimlodChunk* first = r.head != nullptr ? r.head : (k == 0u ? c : (k + 1u == r.additional ? chunk_at(0u) : nullptr));
		c->next = next;
		chunkDir[r.dirNew + k] = c;
		if (r.existing + k < LEAF_SLOTS) leaf_row_set(leafChunks, a.pers, r.node, r.existing + k, c);
		if (k == 0u) { if (r.tail == nullptr) a.nodes[r.node].points = c; else r.tail->next = c; }
		if (k + 1u == r.additional) tail_of(first) = c;
	}
}

// ---- hist: round 0 of the split cascade's histograms (voxels.cu:245-289) ---------------------------------------------------------
// Every CU takes part (an ordinary launch; the rounds that follow, if any, run inside k_expand).  Index space: first the stored points
// of the queued leaves — element e = point (e % 1000) of work item (e / 1000), one chunk per item: they move into the spill buffer
// (voxels.cu:253-289) — then the batch's samples.  Whatever lies in a queued leaf is added to the leaf's histogram (per workgroup in LDS
// first, one global add per workgroup and bin) and its cached-leaf word is relabelled FLAG | slot | bin.  Exits at once when k_queue
// queued nothing.
__global__ __launch_bounds__(TPB) void k_hist(BuildArgs a, uint32_t ordinal) {
	Ctl* ctl = ctl_of(a);
	BatchCtl* bc = batch_of(ctl, ordinal);
	if (bc == nullptr || ctl->abortBatch) return;
	const uint32_t n = bc->batchSize, tag = bc->tag, numWork = bc->numWork;      // (asked for beside the slot count: one round trip, not two)
	const uint32_t slots0 = slots_in_use(bc);
	if (blockIdx.x == 0 && threadIdx.x == 0) bc->slotsRound0 = slots0;
	if (blockIdx.x + 1u == gridDim.x && threadIdx.x == 0) prepare_batch(a, ctl, ordinal + 1u);     // (a workgroup without samples, as a rule)
	if (slots0 == 0u) return;
	__shared__ BlockTable tbl;
	const LeafWords leafOf(a, ordinal);
	const unsigned long long* slotOf = at<const unsigned long long>(a, a.offSplitTag);   // per node: batch tag << 32 | level << 16 | slot
	uint32_t* hist = at<uint32_t>(a, a.offHist);
	const uint32_t shard = blockIdx.x & (HIST_SHARDS - 1u);                                    // this workgroup's copy
	const SpillWork* work = at<const SpillWork>(a, a.offWork);
	float4* spilled = at<float4>(a, a.offSpilled);
	const uint32_t moved = min(numWork, a.workCap) * SIMLOD_POINTS_PER_CHUNK;
	const uint32_t total = moved + n;
	const uint32_t numChunks = (total + CPB - 1) / CPB;
	if (blockIdx.x >= numChunks) return;
	Phase ph(ctl, blockIdx.x == 0);
	table_init(tbl);
	__syncthreads();
	// An exact group of several batches (acct) keeps a slot's histogram PER BATCH: a sample of batch k of the group goes into histB[(slot, bin)][k], a
	// stored point that moves — it was there before the group — into the plain histogram; a bin's count is the sum of both (bin_total).  The LDS
	// table's key carries the batch above the (slot, bin) bits.
	const bool acct = bc->acct != 0u;
	uint32_t* histB = at<uint32_t>(a, a.offHistB);
	const uint32_t GB = a.groupMax;
	auto flush = [&](uint32_t key, uint32_t cnt) {
		const uint32_t kb = key >> ACCT_BATCH_SHIFT, k21 = key & 0x1fffffu;
		if (acct && kb != ACCT_MOVED) atomicAdd(histB + (uint64_t)k21 * GB + kb, cnt);
		else atomicAdd(hist + hist_word(k21, shard), cnt);
	};
	auto add = [&](uint32_t key, uint32_t kb) {
		uint32_t rank;
		if (acct) key |= kb << ACCT_BATCH_SHIFT;
		if (table_add(tbl, key, 1u, &rank) < 0) flush(key, 1u);
	};
	const Samples<false> grp(a, bc);
	for (uint32_t chunk = blockIdx.x; chunk < numChunks; chunk += gridDim.x) {
		// (an exact group: which batch of the group the tile's samples belong to — one lookup per tile where the tile lies in one batch)
		const float4* unusedBase; uint32_t kspan = 0;
		const uint32_t e0 = max(chunk * CPB, moved), e1 = min(total, (chunk + 1u) * CPB);
		const bool oneBatch = acct && e0 < e1 && grp.span(e0 - moved, e1 - 1u - moved, unusedBase, kspan);      // (workgroup-uniform)
		// stage by stage, eight elements per thread.  A SAMPLE of the group is never read here: its word holds the leaf k_count found and the
		// bin below that leaf (node | bin << 19) — if the leaf was queued, the word becomes FLAG | slot | bin and the bin is counted.  A STORED
		// point of a queued leaf is read, binned and moved to the spill buffer.
		uint32_t ent[HCPT], dst[HCPT], v[HCPT];              // moved points: ent = level << 16 | slot (or NONE), dst = spill index; samples: v = the cached-leaf word (or NONE)
		const float4* src[HCPT];
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) {
			const uint32_t e = chunk * CPB + j * TPB + threadIdx.x;
			ent[j] = NONE; src[j] = nullptr; dst[j] = 0; v[j] = NONE;
			if (e < moved) {
				const SpillWork item = work[e / SIMLOD_POINTS_PER_CHUNK];
				const uint32_t k = e % SIMLOD_POINTS_PER_CHUNK;
				if (k < item.count) { ent[j] = (item.level << 16) | item.slot; src[j] = reinterpret_cast<const float4*>(item.chunk->points) + k; dst[j] = item.dstBase + k; }
			} else if (e < total) v[j] = leafOf.grp[e - moved];
		}
		unsigned long long info[HCPT];
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) info[j] = v[j] != NONE ? slotOf[v[j] & LEAF_NODE_MASK] : 0ull;
		float4 p[HCPT];
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) p[j] = ent[j] != NONE ? *src[j] : make_float4(0, 0, 0, 0);
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) {
			if (v[j] == NONE || (uint32_t)(info[j] >> 32) != tag) continue;
			const uint32_t key = (((uint32_t)info[j] & 0xffffu) << 9) | (v[j] >> LEAF_BIN_SHIFT);
			const uint32_t i = chunk * CPB + j * TPB + threadIdx.x - moved;
			leafOf.grp[i] = LEAF_FLAG | key;
			add(key, !acct ? 0u : oneBatch ? kspan : batch_of_sample(bc, i));
		}
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) {
			if (ent[j] == NONE) continue;
			const uint32_t X = quantize(F_GRID, p[j].x, a.minx, a.size), Y = quantize(F_GRID, p[j].y, a.miny, a.size), Z = quantize(F_GRID, p[j].z, a.minz, a.size);
			const uint32_t key = ((ent[j] & 0xffffu) << 9) | bin_of(X, Y, Z, ent[j] >> 16);
			spilled[dst[j]] = p[j]; leafOf.mov[dst[j]] = LEAF_FLAG | key;                       // a stored point moves
			add(key, ACCT_MOVED);
		}
	}
	__syncthreads();
	ph.mark(4);
	for (uint32_t e = threadIdx.x; e < (uint32_t)TBL_CAP; e += TPB) {
		const uint32_t key = tbl.keys[e];
		if (key != TBL_EMPTY) flush(key, tbl.vals[e]);
	}
	ph.mark(5);
	if (ph.on) ctl->phaseNs[6] += 1;
}

// ---- expand: split the queued leaves, cascades included (voxels.cu:385-415, 245-289, 308-383) ---------------------------
// Persistent, hand-rolled grid barrier; exits at once when `count` queued nothing.  The reference counts, splits ONE level, counts
// again, ... with ~8 grid.sync() per level.  Here a round settles THREE levels:
//   H) all workgroups: the stored points of the round's slots move to the spill buffer (work items, round 0 only) and every batch
//      sample / moved point that lies in a slot's node is added to the slot's 512-bin histogram (LDS first, one global add per
//      workgroup and bin); its cached-leaf word becomes FLAG | slot | bin;
//   -- barrier --
//   D) one workgroup per slot: from the histogram alone, which children, grandchildren hold more than 50 000 and split in turn;
//      all their nodes at once (counters filled in, grids allocated, ancestor paths, parents), the slot's map; great-grandchildren
//      that are still too full get a slot of their own for the next round.
//   Every workgroup can tell from the histograms whether a next round is possible; if not, the kernel ends after D without
//   another barrier (the common case: one barrier per batch).
static constexpr uint32_t ETPB = 1024;             // k_expand: at most one workgroup per CU (grid barrier participants), 16 waves each
static constexpr int HT_BITS = 12;
static constexpr uint32_t HT_CAP = 1u << HT_BITS;
static constexpr uint32_t LOCAL_NODES = 8 + 64 + 512;          // nodes a slot can create: local numbering t = 0..7 | 8..71 | 72..583

__device__ __forceinline__ uint32_t hist_sum(const uint32_t* hist, uint64_t word) {      // a bin's count: the sum of its copies
	uint32_t v = hist[word];
	if ((word >> 9) < HIST_SHARDED) {
#pragma unroll
		for (uint32_t sd = 1; sd < HIST_SHARDS; sd++) v += hist[hist_word((uint32_t)word, sd)];
	}
	return v;
}

// ... of an exact group of several batches (acct): the stored points that moved (the plain histogram) + the group's samples, kept per batch
__device__ __forceinline__ uint32_t bin_total(const BuildArgs& a, const uint32_t* hist, uint64_t word, bool acct) {
	uint32_t v = hist_sum(hist, word);
	if (acct) {
		const uint32_t* hb = at<const uint32_t>(a, a.offHistB) + word * a.groupMax;
		for (uint32_t k = 0; k < a.groupMax; k++) v += hb[k];
	}
	return v;
}
static constexpr uint32_t ACCT_MAX_GROUP = 12;     // batches an exact group can have: k_expand keeps a slot's 512 + 64 + 8 per-batch rows in the LDS words of its hash table
static constexpr uint32_t NEVER = 0xffu;

struct ExpandShared {
	union {
		struct { uint32_t keys[HT_CAP], vals[HT_CAP]; };      // H: (slot << 9 | bin) -> count.  D, exact groups: rows of per-batch counts (keys and vals as one array: acct_rows)
		AllocRec allocRec[ALLOC_LEAVES];                       // ... and, when those are done with, alloc_points' records
	};
	uint32_t bins[HIST_BINS], c2[64], c1[8];
	uint32_t base2[8], base3[64];                  // first child of split child j / grandchild jk
	uint32_t listed[LOCAL_NODES];                  // map entry override of a node that got a slot for the next round, or NONE
	FreshLeaf fresh[LOCAL_NODES];                  // the cascade's nodes that hold samples — they get their chunks before the kernel ends
	uint32_t LX, LY, LZ;                           // the slot node's own coordinates, name and grid, read once per slot
	uint8_t nameL[20];
	SimlodOccupancyGrid* gridL;
	uint32_t numFresh, numFill;
	uint32_t part[ETPB / 64u];                     // block_exclusive's word per wave
	uint32_t nextGranted, nextSlot, nextChild, clearBase;      // the slots of the next round this slot's nodes got: how many, the first, its children; the grids' first entry of the clear list
	uint8_t* gridMem;                              // ... and the grids themselves (the splitting children and grandchildren first, then the nodes with a slot)
	uint32_t fillStart[LOCAL_NODES];               // first cell of fill[j] among all the cells to fill
	// new leaves at level <= 3 whose cells of the top table the whole workgroup fills: {node | level << 19, X, Y, Z}.  The ROOT's cascade can make all of its
	// 8 + 64 + 512 nodes such leaves (rounds 3-6 had 72 entries here: a terrain's first batch lists ~120, the entries beyond the array landed in whatever
	// followed it — alloc_points' records while those stood there, harmlessly; the grids' pointers once they did not: a wild pointer in a path entry, a fault
	// in k_voxelize once in a hundred ingests)
	uint4 fill[LOCAL_NODES];
	AllocShared alloc;
	SimlodOccupancyGrid* grid[8 + 64];             // grids of the children / grandchildren that split here
	unsigned long long pathL[PATH_WORDS];          // the slot node's own ancestor path
	uint32_t mask1, extraBase, ok, more;
	unsigned long long mask2;
	// exact groups of several batches (acct): per local node, the batch of the group in which it split (NEVER: it did not) and its counter after that batch;
	// [LOCAL_NODES] = the slot's own node.  The upper nodes the trunk mask names (they split as soon as they exist).  Chunks taken / returned per batch.
	uint8_t splitAt[LOCAL_NODES + 8];
	uint32_t counterAt[LOCAL_NODES + 1];
	uint32_t forced1;
	unsigned long long forced2;
	uint32_t accD[SIMLOD_MAX_BATCHES_PER_LAUNCH], accF[SIMLOD_MAX_BATCHES_PER_LAUNCH];
};
static_assert(offsetof(ExpandShared, vals) == offsetof(ExpandShared, keys) + sizeof(uint32_t) * HT_CAP && (HIST_BINS + 64u + 8u) * ACCT_MAX_GROUP <= 2u * HT_CAP, "acct_rows");

// one table entry of k_expand's in-kernel histogram pass -> global memory.  key: slot << 9 | bin, and in an exact group (acct) above them the batch the
// samples belong to (ACCT_MOVED: stored points that moved): a sample of batch k counts in histB[(slot, bin)][k], a moved point in the plain histogram
__device__ __forceinline__ void hist_flush(const BuildArgs& a, uint32_t key, uint32_t cnt, bool acct) {
	const uint32_t kb = key >> ACCT_BATCH_SHIFT, k21 = key & 0x1fffffu;
	if (acct && kb != ACCT_MOVED) atomicAdd(at<uint32_t>(a, a.offHistB) + (uint64_t)k21 * a.groupMax + kb, cnt);
	else atomicAdd(at<uint32_t>(a, a.offHist) + hist_word(k21, blockIdx.x & (HIST_SHARDS - 1u)), cnt);
}
__device__ __forceinline__ void hist_add(const BuildArgs& a, ExpandShared& sh, uint32_t key, uint32_t cnt, bool acct) {
	uint32_t h = (key * 2654435761u) >> (32 - HT_BITS);
#pragma unroll 1
	for (int probe = 0; probe < 16; ++probe) {
		uint32_t k = sh.keys[h];
		if (k == TBL_EMPTY) { k = atomicCAS(&sh.keys[h], TBL_EMPTY, key); if (k == TBL_EMPTY) k = key; }
		if (k == key) { atomicAdd(&sh.vals[h], cnt); return; }
		h = (h + 1) & (HT_CAP - 1);
	}
	hist_flush(a, key, cnt, acct);          // no room in the table: straight to the histogram (this workgroup's copy)
}
// sum of `v` over the threads of the workgroup below this one, and over all of them (every thread calls: two barriers; part: a word per wave in LDS)
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* part, uint32_t& total) {
	uint32_t waveTotal;
	const uint32_t ex = wave_exclusive(v, waveTotal), wv = threadIdx.x >> 6;
	__syncthreads();
	if ((threadIdx.x & 63u) == 0u) part[wv] = waveTotal;
	__syncthreads();
	uint32_t before = 0;
	total = 0;
	for (uint32_t w = 0; w < ETPB / 64u; w++) { const uint32_t c = part[w]; if (w < wv) before += c; total += c; }
	return before + ex;
}
// local node number t of a slot -> depth below the slot's node (1..3) and the octants chosen on the way
__device__ __forceinline__ uint32_t local_depth(uint32_t t) { return t < 8u ? 1u : t < 72u ? 2u : 3u; }

#ifndef EXPAND_U
#define EXPAND_U 4      /* samples of a thread in flight in the in-kernel histogram pass of rounds >= 1 (only the instantiation that has such a pass: k_expand<false>).  Round 6, exact groups, ms per
                         36 M (same box): 4: 2.594, 8: 2.637, 16: 2.80.  Registers of k_expand<false> at the 128-VGPR cap of 1024 threads: 4: 119 VGPRs, 8: 128, both without scratch memory; 16: 128 and
                         292 bytes per lane.  (Round 6 blamed this pass for 104 bytes per lane with 4: those were values of the build phase hoisted out of its slot loop — see `t` there — and
                         the round-0 instantiation, which has no pass, carried them too) */
#endif
// Rounds [firstRound, lastRound) of the cascade.  A launch that takes its batches one by one runs all rounds in ONE instance (0, MAX), the later rounds' histogram passes inside the
// kernel behind grid barriers.  A launch that takes GROUPS runs round 0 in one instance (0, 1), the histogram pass of round 1 — a group's first cascades meet fresh territory with
// four batches' worth of samples: four of nine groups of the terrain need it — as a kernel of its own over the whole chip (k_hist2), and round 1 and whatever follows in a second
// instance (1, MAX): the two grid barriers and the 128-workgroup pass of the one-instance form cost ~100 us per second round, a kernel boundary costs nothing on one queue
// (DESIGN §2) and an instance that finds nothing to do ~4 us.
// ROUND0: the instance (0, 1) of a launch that takes groups, as an instantiation of its own — it never runs a histogram pass, never meets a grid barrier and never waits
// for the other slots' decisions, and carries no code for any of them (the arguments firstRound / lastRound are ignored: 0 and 1).
template <bool ROUND0>
__global__ __launch_bounds__(ETPB) void k_expand(BuildArgs a, uint32_t ordinal, uint32_t firstRound, uint32_t lastRound) {
	if (ROUND0) { firstRound = 0u; lastRound = 1u; }
	Ctl* ctl = ctl_of(a);
	BatchCtl* bc = batch_of(ctl, ordinal);
	if (bc == nullptr || ctl->abortBatch) return;
	if (firstRound != 0u && slots_in_use(bc) <= min(bc->slotsRound0, SLOT_CAP)) return;      // (round 0 queued nothing for a round 1)
	__shared__ ExpandShared sh;
	if (firstRound == 0u) {
		// The chunks of the leaves that k_count found new samples for and that do not split (voxels.cu:485-538 allocatePointChunks; the nodes of
		// a cascade get theirs below, from the workgroup that builds them): 64 leaves per list, list #k to the k-th workgroup FROM THE END —
		// the first workgroups are the ones that build the cascades — beside the cascade and off k_insert's path.
		const uint32_t numTouched = min(bc->numTouched, a.nodeCapacity);
		const uint32_t allocBlocks = (numTouched + 63u) / 64u;
		for (uint32_t blk = gridDim.x - 1u - blockIdx.x; blk < allocBlocks; blk += gridDim.x) {
			__syncthreads();
			alloc_points(a, ctl, bc, sh.alloc, sh.allocRec, at<const uint32_t>(a, a.offTouched), nullptr, blk * 64u, numTouched, 1u);
		}
		__syncthreads();
	}
	if (bc->slotsRound0 == 0u) return;         // slots handed out by k_count's tail, as k_hist found them: stable while this kernel hands out more
	// SIMLOD_DEBUG_FORCE_BARRIER_TIMEOUT: behave as if the grid barrier had given up (tests the abort path); either way the octree is
	// not to be trusted any more (k_count's tail has already emptied the queued leaves): fatal, sticky until a reset
	if ((ctl->debugFlags & 1u) != 0u) { if (threadIdx.x == 0) panic(ctl, SIMLOD_ERR_BARRIER_TIMEOUT); return; }

	const LeafWords leafOf(a, ordinal);
	uint32_t* parentOf = at<uint32_t>(a, a.offParent);
	uint32_t* kidOf = at<uint32_t>(a, a.offKid);
	const bool irregularKids = (ctl->debugFlags & 8u) != 0u;      // SIMLOD_DEBUG_IRREGULAR_CHILDREN: child words that send the descent through Node.children (a test of that path)
	unsigned long long* paths = at<unsigned long long>(a, a.offPaths);
	SlotRec* slots = slot_recs(a, ordinal);
	uint32_t* hist = at<uint32_t>(a, a.offHist);
	uint32_t* map = at<uint32_t>(a, a.offMap);        // (not the histogram's words: other workgroups may still be peeking at those)
	const float4* spilled = at<const float4>(a, a.offSpilled);
	const Samples<false> pts(a, bc);
	const uint32_t n = bc->batchSize;
	uint32_t generation = 0;
	const bool acct = bc->acct != 0u;                      // an exact group of several batches: histograms per batch, counters and chunk accounting as batch-by-batch ingestion leaves them (account_group)
	const uint32_t GB = bc->groupBatches, GBS = a.groupMax;      // batches of the group | stride of the per-batch rows

	const bool timer = SIMLOD_MEASURE != 0 && blockIdx.x == 0 && threadIdx.x == 0;
	if (timer) ctl->expandNs[6] += 1;

	uint32_t sb = 0, se = min(bc->slotsRound0, SLOT_CAP);
	if (firstRound != 0u) { sb = se; se = min(slots_in_use(bc), SLOT_CAP); }      // (the instance behind k_hist2: the slots round 0 queued)
	for (uint32_t round = firstRound; round < min(lastRound, (uint32_t)SIMLOD_MAX_EXPAND_ROUNDS) && sb < se; ++round) {
		uint64_t t0 = timer ? wall_ns() : 0, t1;
		// -- H: histograms (this instance's first round: k_hist / k_hist2 have built them) --------------------------------------------------
		const bool histHere = !ROUND0 && round > firstRound;
		if (histHere) {
			for (uint32_t i = threadIdx.x; i < HT_CAP; i += ETPB) { sh.keys[i] = TBL_EMPTY; sh.vals[i] = 0u; }
			__syncthreads();
		}
		if (histHere) {
			// the batch's samples and the moved points, eight per thread at a time, stage by stage: the cached-leaf words are in flight
			// together, then the map words of those that were relabelled, then the points of those whose node was queued again
			const uint32_t stride = gridDim.x * ETPB;
			const uint32_t total = n + min(bc->numSpilled, a.spilledCap);
			constexpr uint32_t U = EXPAND_U;
			for (uint32_t first = blockIdx.x * ETPB + threadIdx.x; first < total; first += U * stride) {
				uint32_t idx[U], v[U], ent[U];
				float4 p[U];
#pragma unroll
				for (uint32_t q = 0; q < U; q++) {
					const uint32_t t = first + q * stride;
					idx[q] = t < n ? t : a.groupCap + (t - n);
					v[q] = t < total ? leafOf[idx[q]] : 0u;
				}
#pragma unroll
				for (uint32_t q = 0; q < U; q++) {
					// ent = level << 16 | slot of the round's slot this sample lies in, or NONE
					ent[q] = NONE;
					if ((v[q] & LEAF_FLAG) == 0u) continue;
					const uint32_t e = map[v[q] & 0x1fffffu];                         // the map of an earlier round
					if ((e & MAP_LISTED) != 0u) ent[q] = e & 0x7fffffffu;
				}
#pragma unroll
				for (uint32_t q = 0; q < U; q++) {
					const uint32_t t = first + q * stride;
					p[q] = ent[q] != NONE ? (t < n ? pts[t] : spilled[t - n]) : make_float4(0, 0, 0, 0);
				}
#pragma unroll
				for (uint32_t q = 0; q < U; q++) {
					if (ent[q] == NONE) continue;
					const uint32_t X = quantize(F_GRID, p[q].x, a.minx, a.size), Y = quantize(F_GRID, p[q].y, a.miny, a.size), Z = quantize(F_GRID, p[q].z, a.minz, a.size);
					const uint32_t key = ((ent[q] & 0xffffu) << 9) | bin_of(X, Y, Z, ent[q] >> 16);
					leafOf[idx[q]] = LEAF_FLAG | key;
					const uint32_t t = first + q * stride;
					hist_add(a, sh, acct ? key | ((t < n ? batch_of_sample(bc, t) : ACCT_MOVED) << ACCT_BATCH_SHIFT) : key, 1u, acct);
				}
			}
		}
		if (histHere) {
			__syncthreads();
			for (uint32_t e = threadIdx.x; e < HT_CAP; e += ETPB) {
				const uint32_t key = sh.keys[e];
				if (key != TBL_EMPTY) hist_flush(a, key, sh.vals[e], acct);
			}
			if (timer) { t1 = wall_ns(); ctl->expandNs[0] += t1 - t0; t0 = t1; }
			if (!grid_barrier(&bc->barrierCount, generation, gridDim.x)) { if (threadIdx.x == 0) panic(ctl, SIMLOD_ERR_BARRIER_TIMEOUT); return; }
			if (timer) { t1 = wall_ns(); ctl->expandNs[1] += t1 - t0; t0 = t1; }
		}

		// -- D: decide and build ---------------------------------------------------------------------------------------------
		Phase pd(ctl, blockIdx.x == 0);      // (measure builds: slots 32..39 of Ctl.phaseNs — where workgroup 0's D phase goes; tools/probe.py)
		for (uint32_t s = sb + blockIdx.x; s < se; s += gridDim.x) {
			uint32_t t = threadIdx.x;
			// (opaque to the optimiser: what a thread derives from its number alone — its local node's octants, masks' bits, addresses — is the same for every slot
			// of the loop, and hoisted in front of the loop it stayed live across the whole body: 18 values per lane went to scratch memory at the loop's head and
			// came back where they were used, 104 bytes per lane.  Computed per slot they cost a few ALU operations and the kernel needs no scratch memory: 102 VGPRs
			// in the round-0 instantiation, 119 in the other)
			asm volatile("" : "+v"(t));
			uint64_t before[6] = {0, 0, 0, 0, 0, 0};      // (measure builds: the phase sums as this slot found them)
			if (pd.on) for (uint32_t k = 0; k < 6u; k++) before[k] = ctl->phaseNs[32u + k];
			const uint32_t myBin = t < HIST_BINS ? hist_sum(hist, (uint64_t)s * HIST_BINS + t) : 0u;      // (needs the slot's number only: in flight beside its record)
			const SlotRec rec = slots[s];
			if (rec.node == NONE) { if (t == 0u) atomicAdd(&bc->decided, 1u); continue; }      // nothing could be reserved for this leaf (and it queues nothing)
			const uint32_t L = rec.node, l = rec.level;
			const uint32_t K = min(3u, (uint32_t)SIMLOD_MAX_DEPTH - l);         // levels below L that exist
			__syncthreads();
			uint32_t* const B3 = sh.keys; uint32_t* const B2 = B3 + HIST_BINS * GBS; uint32_t* const B1 = B2 + 64u * GBS;      // acct_rows: per-batch counts of the 512 bins, the 64 grandchildren, the 8 children
			uint32_t binTotal = myBin;
			if (acct && t < HIST_BINS) {       // an exact group: myBin = the stored points that moved; the group's samples per batch
				const uint32_t* hb = at<const uint32_t>(a, a.offHistB) + ((uint64_t)s * HIST_BINS + t) * GBS;
				for (uint32_t k = 0; k < GB; k++) { const uint32_t r = hb[k]; B3[t * GBS + k] = r; binTotal += r; }
			}
			if (t < HIST_BINS) sh.bins[t] = binTotal;
			if (t < SIMLOD_MAX_BATCHES_PER_LAUNCH) { sh.accD[t] = 0; sh.accF[t] = 0; }
			if (t < PATH_WORDS) {      // the slot node's WHOLE path: its row, and for a node below level PATH_ROW the entries its row continues in (path_far)
				unsigned long long e = t < PATH_ROW ? paths[(uint64_t)L * PATH_ROW + t] : 0ull;
				if (t >= PATH_ROW && t < l) e = path_far(paths, L, t, a.nodeCapacity);
				sh.pathL[t] = e;
			}
			// the slot node's coordinates, name and grid: one round trip here, beside its path, instead of one in every phase that wants them
			if (t == 64u) { const SimlodNode* nl = a.nodes + L; sh.LX = nl->X; sh.LY = nl->Y; sh.LZ = nl->Z; sh.gridL = nl->grid; }
			if (t >= 96u && t < 116u) sh.nameL[t - 96u] = a.nodes[L].name[t - 96u];
			for (uint32_t i = t; i < LOCAL_NODES; i += ETPB) sh.listed[i] = NONE;
			if (t < 72u) sh.grid[t] = nullptr;
			if (t == 0u) { sh.numFresh = 0; sh.numFill = 0; }
			__syncthreads();
			if (t < 64u) { uint32_t c = 0; for (uint32_t k = 0; k < 8; k++) c += sh.bins[t * 8 + k]; sh.c2[t] = c; }
			__syncthreads();
			if (t < 8u) { uint32_t c = 0; for (uint32_t k = 0; k < 8; k++) c += sh.c2[t * 8 + k]; sh.c1[t] = c; }
			__syncthreads();
			if (t < 64u) {
				// a child splits when it holds more than 50 000 and is above MAX_DEPTH (K >= 2 <=> level l + 1 <= 19); a grandchild likewise
				// (or when it is an upper node of a multi-GPU job that the host's mask names: trunk_forced)
				bool f1 = false, f2 = false;
				if (trunk_any(a) && l + 1u < TRUNK_LEVELS) {
					// lane t < 8 as child t; every lane as grandchild t = child (t >> 3), octant (t & 7) below it
					const uint32_t LX = sh.LX, LY = sh.LY, LZ = sh.LZ, j = t >> 3, k = t & 7u;
					f1 = t < 8u && trunk_forced(a, l + 1u, 2u * LX + ((t >> 2) & 1u), 2u * LY + ((t >> 1) & 1u), 2u * LZ + (t & 1u));
					f2 = trunk_forced(a, l + 2u, 4u * LX + 2u * ((j >> 2) & 1u) + ((k >> 2) & 1u), 4u * LY + 2u * ((j >> 1) & 1u) + ((k >> 1) & 1u), 4u * LZ + 2u * (j & 1u) + (k & 1u));
				}
				{ const unsigned long long bf1 = __ballot(f1), bf2 = __ballot(f2); if (t == 0u) { sh.forced1 = (uint32_t)bf1 & 0xffu; sh.forced2 = bf2; } }
				const bool s1 = t < 8u && K >= 2u && (sh.c1[t & 7u] > SIMLOD_MAX_POINTS_PER_NODE || f1);
				uint32_t mask1 = (uint32_t)__ballot(s1) & 0xffu;
				const bool s2 = K >= 3u && ((mask1 >> (t >> 3)) & 1u) != 0u && (sh.c2[t] > SIMLOD_MAX_POINTS_PER_NODE || f2);
				unsigned long long mask2 = __ballot(s2);
				uint32_t n1 = (uint32_t)__popc(mask1), n2 = (uint32_t)__popcll(mask2);
				uint32_t extraBase = 0, granted = n1 + n2;
				if (t == 0 && n1 + n2 > 0u) {
					uint32_t noSlot, noSpill;
					if (!reserve(a, ctl, bc, 0u, 8u * (n1 + n2), 0u, noSlot, extraBase, noSpill)) {
						// no room in the node array for the whole cascade: as many of its splits as still fit, children first (the others stay too full: deferred)
						const uint32_t inUse = (uint32_t)(__hip_atomic_load(&bc->reserve, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32) & 0xfffffu;
						granted = a.nodeCapacity > inUse ? min((a.nodeCapacity - inUse) / 8u, n1 + n2) : 0u;
						if (granted == 0u || !reserve(a, ctl, bc, 0u, 8u * granted, 0u, noSlot, extraBase, noSpill)) { granted = 0u; extraBase = NONE; }
					}
				}
				extraBase = __shfl(extraBase, 0); granted = __shfl(granted, 0);
				if (granted < n1 + n2) {
					// the first `granted` splits in order: the children by octant, then the grandchildren of the children that do split
					uint32_t keep1 = 0, left = granted;
					for (uint32_t j = 0; j < 8u && left != 0u; j++) if (((mask1 >> j) & 1u) != 0u) { keep1 |= 1u << j; left--; }
					unsigned long long keep2 = 0ull;
					for (uint32_t jk = 0; jk < 64u && left != 0u; jk++) if (((mask2 >> jk) & 1ull) != 0ull && ((keep1 >> (jk >> 3)) & 1u) != 0u) { keep2 |= 1ull << jk; left--; }
					mask1 = keep1; mask2 = keep2; n1 = (uint32_t)__popc(mask1); n2 = (uint32_t)__popcll(mask2);
				}
				if (extraBase == NONE) { mask1 = 0; mask2 = 0ull; n1 = 0; n2 = 0; }
				if (t < 8u) sh.base2[t] = extraBase + 8u * (uint32_t)__popc(mask1 & ((1u << t) - 1u));
				sh.base3[t] = extraBase + 8u * (n1 + (uint32_t)__popcll(mask2 & ((1ull << t) - 1ull)));
				if (t == 0) { sh.mask1 = mask1; sh.mask2 = mask2; }
			}
			__syncthreads();
			pd.mark(32);      // histograms in, counts summed, splits decided, node slots reserved
			const uint32_t mask1 = sh.mask1;
			const unsigned long long mask2 = sh.mask2;
			// local node t: does it exist, how many samples, does it split here
			auto exists = [&](uint32_t u) { return u < 8u ? true : u < 72u ? ((mask1 >> ((u - 8u) >> 3)) & 1u) != 0u : ((mask2 >> ((u - 72u) >> 3)) & 1ull) != 0ull; };
			auto countOf = [&](uint32_t u) { return u < 8u ? sh.c1[u] : u < 72u ? sh.c2[u - 8u] : sh.bins[u - 72u]; };
			auto splits = [&](uint32_t u) { return u < 8u ? ((mask1 >> u) & 1u) != 0u : u < 72u ? ((mask2 >> (u - 8u)) & 1ull) != 0ull : false; };
			auto indexOf = [&](uint32_t u) { return u < 8u ? rec.childBase + u : u < 72u ? sh.base2[(u - 8u) >> 3] + ((u - 8u) & 7u) : sh.base3[(u - 72u) >> 3] + ((u - 72u) & 7u); };
			// ---- an exact group of several batches: WHEN each node of the cascade split, what it held then, the chunks it took and returned meanwhile ----
			// Local node u's row: its samples per batch of the group.  The node is created in the batch its parent split in (`born`), holds what lay in its
			// cell up to and including that batch (the stored points that moved + the group's samples so far), and — if it splits at all — splits in the first
			// batch from then on after which it holds more than 50 000 (a node the trunk mask names: at once).  While it is a leaf it has ceil(count / 1000)
			// chunks (voxels.cu:485-538), all of which it returns when it splits (voxels.cu:346-357).
			auto rowOf = [&](uint32_t u) -> const uint32_t* { return u < 8u ? B1 + u * GBS : u < 72u ? B2 + (u - 8u) * GBS : B3 + (u - 72u) * GBS; };
			// -> the batch in which u splits (`willSplit`: it does, in this round or as a slot of the next) and its counter after that batch
			auto split_time = [&](uint32_t u, uint32_t born, bool forced, uint32_t& counterThen) -> uint32_t {
				const uint32_t* row = rowOf(u);
				uint32_t c = countOf(u);
				for (uint32_t k = 0; k < GB; k++) c -= row[k];                     // the stored points that moved into u's cell
				for (uint32_t k = 0; k <= born; k++) c += row[k];                   // what u is created with
				uint32_t k = born;
				while (!forced && c <= SIMLOD_MAX_POINTS_PER_NODE && k + 1u < GB) { k++; c += row[k]; }
				counterThen = c;
				return k;
			};
			// the chunks u takes, batch by batch, while it is a leaf: from `born` until `splitAt` (NEVER: the end of the group), and returns then
			auto leaf_chunks = [&](uint32_t u, uint32_t born, uint32_t splitAt) {
				const uint32_t* row = rowOf(u);
				uint32_t c = countOf(u);
				for (uint32_t k = 0; k < GB; k++) c -= row[k];
				for (uint32_t k = 0; k < born; k++) c += row[k];
				uint32_t have = 0;
				for (uint32_t k = born; k < min(splitAt, GB); k++) {
					c += row[k];
					const uint32_t want = (c + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
					if (want != have) atomicAdd(&sh.accD[k], want - have);
					have = want;
				}
				if (splitAt < GB && have != 0u) atomicAdd(&sh.accF[splitAt], have);
			};
			if (acct) {
				for (uint32_t i = t; i < 64u * GB; i += ETPB) { const uint32_t jk = i / GB, k = i % GB; uint32_t c = 0; for (uint32_t q = 0; q < 8; q++) c += B3[(jk * 8u + q) * GBS + k]; B2[jk * GBS + k] = c; }
				__syncthreads();
				for (uint32_t i = t; i < 8u * GB; i += ETPB) { const uint32_t j = i / GB, k = i % GB; uint32_t c = 0; for (uint32_t q = 0; q < 8; q++) c += B2[(j * 8u + q) * GBS + k]; B1[j * GBS + k] = c; }
				__syncthreads();
				if (t == 0u) {
					// the slot's own node.  One the cascade queued for this round (born != NONE): settled by the round that queued it.  A leaf of the octree as the
					// group found it: it holds rec.stored points in ceil(stored / 1000) chunks, grows batch by batch, and splits in the first batch that takes it
					// over the limit (a leaf already over it — a split that had to wait —: in the first batch that touches it; one the trunk mask names: at once)
					uint32_t sL = rec.born, cThen = 0;
					if (rec.born == NONE) {
						const bool forcedL = trunk_any(a) && trunk_forced(a, l, sh.LX, sh.LY, sh.LZ);
						uint32_t c = rec.stored;
						sL = GB - 1u;
						for (uint32_t k = 0; k < GB; k++) {
							uint32_t g = 0;
							for (uint32_t j = 0; j < 8; j++) g += B1[j * GBS + k];
							if (forcedL || (g != 0u && c + g > SIMLOD_MAX_POINTS_PER_NODE)) { sL = k; break; }
							c += g;
						}
						c = rec.stored;
						uint32_t have = (c + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
						for (uint32_t k = 0; k <= sL; k++) {
							uint32_t g = 0;
							for (uint32_t j = 0; j < 8; j++) g += B1[j * GBS + k];
							c += g;
							if (k == sL) break;
							const uint32_t want = (c + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
							if (want != have) atomicAdd(&sh.accD[k], want - have);
							have = want;
						}
						if (have != 0u) atomicAdd(&sh.accF[sL], have);
						cThen = c;
					}
					sh.splitAt[LOCAL_NODES] = (uint8_t)sL; sh.counterAt[LOCAL_NODES] = cThen;
					if (L == 0u && rec.born == NONE) bc->rootSplitAt = sL;      // (the batches before it found the root a leaf: k_rootpre)
				}
				__syncthreads();
				if (t < 8u) {                                                      // the children: created when the slot's node split
					const uint32_t born = sh.splitAt[LOCAL_NODES];
					uint32_t cThen = 0;
					const uint32_t at = splits(t) ? split_time(t, born, ((sh.forced1 >> t) & 1u) != 0u, cThen) : NEVER;
					sh.splitAt[t] = (uint8_t)at; sh.counterAt[t] = cThen;
					leaf_chunks(t, born, at);
				}
				__syncthreads();
				if (t >= 8u && t < 72u && exists(t)) {                             // the grandchildren: created when their parent split
					const uint32_t born = sh.splitAt[(t - 8u) >> 3];
					uint32_t cThen = 0;
					const uint32_t at = splits(t) ? split_time(t, born, ((sh.forced2 >> (t - 8u)) & 1ull) != 0ull, cThen) : NEVER;
					sh.splitAt[t] = (uint8_t)at; sh.counterAt[t] = cThen;
					leaf_chunks(t, born, at);
				}
				__syncthreads();
			}
			else if (t == 0u && L == 0u && rec.born == NONE && GB > 1u) {
				// coalesced groups keep no counts per batch, but a root that is still a leaf is the whole octree: every sample of batch k of the group lies in it.
				// The batch it splits in — by the rule above — follows from the batches' sizes alone, and the batches in front of it met the root's grid as a
				// leaf's (voxels.cu:449-463) before the split cleared it (voxels.cu:371-382): k_rootpre replays that, as for exact groups
				const bool forcedL = trunk_any(a) && trunk_forced(a, l, sh.LX, sh.LY, sh.LZ);
				uint32_t c = rec.stored, sL = GB - 1u;
				for (uint32_t k = 0; k < GB; k++) {
					const uint32_t g = bc->start[k + 1u] - bc->start[k];
					if (forcedL || (g != 0u && c + g > SIMLOD_MAX_POINTS_PER_NODE)) { sL = k; break; }
					c += g;
				}
				bc->rootSplitAt = sL;
			}
			pd.mark(33);      // exact groups: when every node split, chunks taken and returned per batch
			// ---- the slots of the next round and every grid this slot needs, in ONE go ----
			// A great-grandchild that is still too full after three levels gets a slot of its own for the next round (its eight children reserved now, no stored
			// points).  The root's cascade, or a flood into a fresh leaf, lists dozens of them: they are COUNTED (a prefix sum over the workgroup, local-node
			// order), thread 0 reserves slots and children for all of them with one add on the reservation word — when that fails: as many as still fit, the
			// first in local-node order, the others stay too full (deferred) —, and allocates the grids of the children and grandchildren that split here
			// and of the nodes that got a slot (like a queued leaf's, before its children exist) with one counted allocation and one add on the clear list's
			// length.  Then the WHOLE WORKGROUP zeroes the new slots' histograms (consecutive slots: consecutive words in every copy), a uint4 per thread and step.
			// (Rounds 2-6: a returning atomic per listed node, and that one lane zeroed its slot's 4 copies + per-batch rows, 16 KB, word by word.)
			const bool wants = t >= 72u && t < LOCAL_NODES && exists(t) && countOf(t) > SIMLOD_MAX_POINTS_PER_NODE && l + 3u < (uint32_t)SIMLOD_MAX_DEPTH;
			uint32_t numWant;
			const uint32_t wantRank = block_exclusive(wants ? 1u : 0u, sh.part, numWant);
			const uint32_t n1 = (uint32_t)__popc(mask1), numSplit = n1 + (uint32_t)__popcll(mask2);
			if (t == 0u) {
				uint32_t granted = numWant, slot0 = 0, child0 = 0, dummy;
				if (numWant != 0u && reserve_try(a, bc, numWant, 8u * numWant, 0u, slot0, child0, dummy) != 0u) {
					const unsigned long long w = __hip_atomic_load(&bc->reserve, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					const uint32_t slotsUsed = (uint32_t)(w >> RSV_SLOT_SHIFT), nodesUsed = (uint32_t)(w >> 32) & 0xfffffu;
					const uint32_t fitSlots = SLOT_CAP > slotsUsed ? SLOT_CAP - slotsUsed : 0u, fitNodes = a.nodeCapacity > nodesUsed ? (a.nodeCapacity - nodesUsed) / 8u : 0u;
					granted = min(numWant, min(fitSlots, fitNodes));
					if (granted != 0u && reserve_try(a, bc, granted, 8u * granted, 0u, slot0, child0, dummy) != 0u) granted = 0u;
					if (granted < numWant) raise(ctl, fitSlots <= fitNodes ? SIMLOD_ERR_SPILLING_OVERFLOW : SIMLOD_ERR_NODES_EXHAUSTED);      // (what the first node left out ran into)
				}
				uint32_t clearBase = 0;
				uint8_t* mem = numSplit + granted != 0u ? grids_for_splits(a, bc, numSplit + granted, clearBase) : nullptr;
				sh.nextGranted = granted; sh.nextSlot = slot0; sh.nextChild = child0; sh.gridMem = mem; sh.clearBase = clearBase;
			}
			__syncthreads();
			const uint32_t numNext = sh.nextGranted, slot0 = sh.nextSlot;
			if (t < 72u && splits(t)) {
				const uint32_t k = t < 8u ? (uint32_t)__popc(mask1 & ((1u << t) - 1u)) : n1 + (uint32_t)__popcll(mask2 & ((1ull << (t - 8u)) - 1ull));
				SimlodOccupancyGrid* g = grid_of_many(sh.gridMem, k);
				note_clear(a, bc, sh.clearBase + k, g);
				sh.grid[t] = g;
			} else if (wants && wantRank < numNext) {
				const uint32_t slot = slot0 + wantRank, level = l + 3u;
				note_clear(a, bc, sh.clearBase + numSplit + wantRank, grid_of_many(sh.gridMem, numSplit + wantRank));
				uint32_t born = NONE, cThen = 0;
				if (acct) born = split_time(t, sh.splitAt[8u + ((t - 72u) >> 3)], false, cThen);      // (an exact group: the batch in which this node splits — when its children are created)
				slots[slot] = SlotRec{indexOf(t), level, sh.nextChild + 8u * wantRank, 0u, 0u, born, 0u, 0u};
				sh.listed[t] = MAP_LISTED | (level << 16) | slot;
			}
			if (numNext != 0u) {
				auto zero = [&](uint32_t* words, uint32_t count) {      // (every range starts at a slot's first bin: 2 KB aligned)
					uint4* w = reinterpret_cast<uint4*>(words);
					for (uint32_t i = t; i < count / 4u; i += ETPB) w[i] = make_uint4(0, 0, 0, 0);
				};
				zero(hist + (uint64_t)slot0 * HIST_BINS, numNext * HIST_BINS);
				if (slot0 < HIST_SHARDED) for (uint32_t sd = 1; sd < HIST_SHARDS; sd++) zero(hist + hist_word(slot0 << 9, sd), (min(slot0 + numNext, HIST_SHARDED) - slot0) * HIST_BINS);
				if (acct) zero(at<uint32_t>(a, a.offHistB) + (uint64_t)slot0 * HIST_BINS * GBS, numNext * HIST_BINS * GBS);      // (an exact group: the slots' histograms per batch)
			}
			__syncthreads();
			// this slot's reservations for the next round are made (the workgroup's threads have their answers, the new slots' histograms are zero): say so — see "is there a next round" below
			if (t == 0u) atomicAdd(&bc->decided, 1u);
			pd.mark(34);      // grids, slots of the next round
			if (t < LOCAL_NODES && exists(t)) {
				const uint32_t depth = local_depth(t), level = l + depth, idx = indexOf(t);
				// octants chosen below L, first to last
				const uint32_t rel = t < 8u ? t : t < 72u ? t - 8u : t - 72u;
				uint32_t oct[3] = {0, 0, 0};
				for (uint32_t k = 0; k < depth; k++) oct[k] = (rel >> (3u * (depth - 1u - k))) & 7u;
				uint32_t X = sh.LX, Y = sh.LY, Z = sh.LZ;
				for (uint32_t k = 0; k < depth; k++) { X = 2u * X + ((oct[k] >> 2) & 1u); Y = 2u * Y + ((oct[k] >> 1) & 1u); Z = 2u * Z + (oct[k] & 1u); }
				const bool split = splits(t);
				const bool nextRound = sh.listed[t] != NONE;
				// written field by field straight to the node array (a 152-byte local would live in scratch memory); voxels.cu:318-343
				SimlodNode& c = a.nodes[idx];
				const uint32_t firstChild = !split ? 0u : t < 8u ? sh.base2[t] : sh.base3[t - 8u];
				for (uint32_t k = 0; k < 8; k++) c.children[k] = split ? a.nodes + firstChild + k : nullptr;
				// its child word: the first child and which of the eight stay leaves in this round (a child's children: t < 8: local nodes 8 + 8 t + k, whose
				// splits are bits 8 t + k of mask2; the great-grandchildren never split in the round that makes them)
				kidOf[idx] = !split ? 0u : irregularKids ? KID_IRREGULAR : firstChild | ((t < 8u ? ~(uint32_t)(mask2 >> (8u * t)) & 0xffu : 0xffu) << KID_LEAF_SHIFT);
				uint32_t counter = countOf(t);
				if (acct) {
					// what the node held after the batch in which it split (later batches of the group went past it, voxels.cu:169-187); a great-grandchild
					// is settled here (whether it got a slot for the next round is known now), the levels above it were on the way
					if (depth == 3u) {
						const uint32_t born = sh.splitAt[8u + ((t - 72u) >> 3)];
						uint32_t cThen = 0;
						const uint32_t at = nextRound ? split_time(t, born, false, cThen) : NEVER;
						sh.splitAt[t] = (uint8_t)at; sh.counterAt[t] = cThen;
						leaf_chunks(t, born, at);
					}
					if (sh.splitAt[t] != NEVER) counter = sh.counterAt[t];
				}
				c.counter = counter; c.numPoints = 0;
				c.level = level; c.X = X; c.Y = Y; c.Z = Z;
				c.countIteration = 0; c.countFlag = 0;
				for (int k = 0; k < 20; k++) c.name[k] = sh.nameL[k];
				for (uint32_t k = 0; k < depth; k++) if (l + 1u + k < 20u) c.name[l + 1u + k] = (uint8_t)('0' + oct[k]);
				c.visible = 0; c.isFiltered = 0; c.isLeaf = 1; c.isLarge = 0;
				c.grid = split ? sh.grid[t] : nullptr; c.points = nullptr; c.voxelChunks = nullptr;
				c.numVoxels = 0; c.numVoxelsStored = 0;
				if (nextRound) c.grid = grid_of_many(sh.gridMem, numSplit + wantRank);                                 // (its grid: like a queued leaf's, before its children exist)
				// parent, and the ancestor path: parent first, ..., then L, then L's own ancestors
				const uint32_t parentLocal = depth == 1u ? NONE : depth == 2u ? (t - 8u) >> 3 : 8u + ((t - 72u) >> 3);
				const uint32_t parentIdx = depth == 1u ? L : indexOf(parentLocal);
				parentOf[idx] = parentIdx;
				// (its row: the first PATH_ROW of them, zero-terminated when there are fewer — the others are found through the row of the last one: path_far)
				unsigned long long* mine = paths + (uint64_t)idx * PATH_ROW;
				uint32_t w = 0;
				if (depth >= 3u) { const uint32_t g = 8u + ((t - 72u) >> 3); mine[w++] = path_pack(a.pers, indexOf(g), l + 2u, sh.grid[g]); }
				if (depth >= 2u) { const uint32_t ch = depth == 2u ? (t - 8u) >> 3 : (t - 72u) >> 6; mine[w++] = path_pack(a.pers, indexOf(ch), l + 1u, sh.grid[ch]); }
				mine[w++] = path_pack(a.pers, L, l, sh.gridL);
				for (uint32_t k = 0; w < PATH_ROW; k++) {
					const unsigned long long e = sh.pathL[k];       // (pathL[20] is zero: k < PATH_ROW <= 20)
					mine[w++] = e;
					if (e == 0ull) break;
				}
				if (t < 8u) a.nodes[L].children[t] = a.nodes + idx;
				// the nodes of the cascade that hold samples and stay leaves (one that was queued again is none by the time its chunks would be used)
				if (!split && countOf(t) != 0u && !nextRound) sh.fresh[atomicAdd(&sh.numFresh, 1u)] = FreshLeaf{idx, countOf(t), level, X, Y, Z};
				// the top table (where k_count's descent starts): a new node at level <= 5 that has no children in the table's range takes over the cells it covers
				// (a node two or more levels above the table's — 64 to 4096 cells, the first batches over a region — is filled by the whole workgroup, below)
				if (level <= TOP_LEVEL && (!split || level == TOP_LEVEL)) {
					const uint32_t mark = split ? 0u : TOP_LEAF;
					if (TOP_LEVEL - level <= 1u) top_fill(at<uint32_t>(a, a.offTop), idx, level, X, Y, Z, mark);
					else sh.fill[atomicAdd(&sh.numFill, 1u)] = make_uint4(idx | (level << 19) | mark, X, Y, Z);
				}
			}
			if (t == 0u) {
				// the slot node's child word; it is no leaf any more: its bit in its parent's word goes (siblings may be splitting in other workgroups: an atomic;
				// the parent's word was written by an earlier launch or an earlier round), and a top-table entry that names it (a node at the table's level) loses its mark
				kidOf[L] = irregularKids ? KID_IRREGULAR : rec.childBase | ((~mask1 & 0xffu) << KID_LEAF_SHIFT);
				if (L != 0u) {
					const uint32_t P = parentOf[L];
					if (P != NONE && kidOf[P] != KID_IRREGULAR) atomicAnd(&kidOf[P], ~(1u << (KID_LEAF_SHIFT + octant_of(sh.LX, sh.LY, sh.LZ))));
				}
				if (l == TOP_LEVEL) at<uint32_t>(a, a.offTop)[(sh.LX << (2u * TOP_LEVEL)) | (sh.LY << TOP_LEVEL) | sh.LZ] = L | (l << 19);
				a.nodes[L].numPoints = 0; a.nodes[L].points = nullptr;          // voxels.cu:359-360 (its points are in the spill buffer, its chunks on the recycle stack: k_queue, k_hist)
				if (acct && rec.born == NONE) a.nodes[L].counter = sh.counterAt[LOCAL_NODES];      // (k_count added the whole group's samples: the batches after the split went to the children)
			}
			// the slot's map: bin -> the deepest node that exists above it (or the slot that node got for the next round)
			if (t < HIST_BINS) {
				const uint32_t j = t >> 6, jk = t >> 3;
				const uint32_t u = ((mask1 >> j) & 1u) == 0u ? j : ((mask2 >> jk) & 1ull) == 0ull ? 8u + jk : 72u + t;
				const uint32_t ls = sh.listed[u];
				map[(uint64_t)s * HIST_BINS + t] = ls != NONE ? ls : indexOf(u);
			}
			// ... and their chunks, 64 leaves at a time (voxels.cu:485-538; the nodes written above are this workgroup's own stores: visible after the barrier)
			__syncthreads();
			pd.mark(35);      // nodes, paths, map
			if (acct && t < GB) {
				if (sh.accD[t] != 0u) atomicAdd(&bc->acctD[t], sh.accD[t]);
				if (sh.accF[t] != 0u) atomicAdd(&bc->acctF[t], sh.accF[t]);
			}
			if (sh.numFill != 0u) {
				// the top table's cells under the big new leaves: ALL entries' cells as one index space over the workgroup (an entry has 64, 512 or 4096 cells: a wave's
				// 64 cells lie in one entry, which it finds by bisection in the entries' prefix sums).  A root's cascade lists dozens of entries; one after the other,
				// each was a loop of its own with most of the workgroup idle.
				const uint32_t nf = sh.numFill;
				uint32_t cells;
				const uint32_t start = block_exclusive(t < nf ? 1u << (3u * (TOP_LEVEL - ((sh.fill[t].x >> 19) & 31u))) : 0u, sh.part, cells);
				if (t < nf) sh.fillStart[t] = start;
				__syncthreads();
				uint32_t* top = at<uint32_t>(a, a.offTop);
				for (uint32_t i = t; i < cells; i += ETPB) {
					uint32_t lo = 0, hi = nf;                                          // the last entry that starts at or before cell i
					while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (sh.fillStart[mid] <= i) lo = mid; else hi = mid; }
					const uint4 f = sh.fill[lo];
					const uint32_t k = TOP_LEVEL - ((f.x >> 19) & 31u), side = 1u << k, c = i - sh.fillStart[lo];
					const uint32_t dx = c >> (2u * k), dy = (c >> k) & (side - 1u), dz = c & (side - 1u);
					top[(((f.y << k) + dx) << (2u * TOP_LEVEL)) | (((f.z << k) + dy) << TOP_LEVEL) | ((f.w << k) + dz)] = f.x;
				}
			}
			pd.mark(36);      // top table
			{
				const uint32_t waves = min((sh.numFresh + 63u) / 64u, ALLOC_WAVES);      // (one wave for the ordinary slot; a big cascade: all its leaves in one turn)
				for (uint32_t first = 0; first < sh.numFresh; first += 64u * waves) {
					alloc_points(a, ctl, bc, sh.alloc, sh.allocRec, nullptr, sh.fresh, first, sh.numFresh, waves);
					__syncthreads();
				}
			}
			pd.mark(37);      // the fresh leaves' chunks
			if (pd.on) {
				ctl->phaseNs[38] += sh.numFresh; ctl->phaseNs[39] += 1;
				// the SLOWEST slot this workgroup has built since the host cleared the clocks: its six phases (40..45), fresh leaves | top-table entries << 16 |
				// next-round slots << 32 (46), their sum (47) — the mean above hides the few slots of a root's cascade or a flood into a fresh leaf
				uint64_t sum = 0;
				for (uint32_t k = 0; k < 6u; k++) sum += ctl->phaseNs[32u + k] - before[k];
				if (sum > ctl->phaseNs[47]) {
					for (uint32_t k = 0; k < 6u; k++) ctl->phaseNs[40u + k] = ctl->phaseNs[32u + k] - before[k];
					ctl->phaseNs[46] = (uint64_t)sh.numFresh | ((uint64_t)sh.numFill << 16) | ((uint64_t)numNext << 32);
					ctl->phaseNs[47] = sum;
				}
			}
		}
		// -- is there a next round?  Only a great-grandchild that is still over the limit makes one, and such a node has reserved its slot by now: once every slot of
		//    this round is past its reservations (a counter; the workgroups without a slot wait here for the ones that have one — they are resident together, as for the
		//    barrier below, and a slot's workgroup passes that point ~12 us into its build phase), the reservation word says.  (Rounds 2-6: every workgroup read every
		//    histogram of the round up front to predict it — 10-14 us per round in front of the build phase.)
		if (ROUND0 || round + 1u >= lastRound) break;      // (the next round belongs to another instance: the kernel's end is the meeting point, the reservation word tells that instance)
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t good = 1;
			const uint64_t w0 = wall_clock64();
			while (__hip_atomic_load(&bc->decided, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < se) {
				__builtin_amdgcn_s_sleep(4);
				if (wall_clock64() - w0 > 200000000ull) { good = 0; break; }      // 2 s at 100 MHz: as the grid barrier
			}
			sh.more = good == 0u ? 2u : slots_in_use(bc) > se ? 1u : 0u;
		}
		__syncthreads();
		if (sh.more == 2u) { if (threadIdx.x == 0) panic(ctl, SIMLOD_ERR_BARRIER_TIMEOUT); return; }
		const bool more = sh.more != 0u;
		if (timer) { t1 = wall_ns(); ctl->expandNs[2] += t1 - t0; t0 = t1; ctl->expandNs[5] += 1; }
		if (!more) break;
		if (!grid_barrier(&bc->barrierCount, generation, gridDim.x)) { if (threadIdx.x == 0) panic(ctl, SIMLOD_ERR_BARRIER_TIMEOUT); return; }
		if (timer) { t1 = wall_ns(); ctl->expandNs[3] += t1 - t0; }
		sb = se;
		se = min(slots_in_use(bc), SLOT_CAP);
	}
}

// ---- hist2: the histogram pass of round 1 of a group's cascade, as a kernel over the whole chip (between the two k_expand instances of a launch that takes groups) ----
// What k_expand's in-kernel pass does for rounds >= 1 with one workgroup per two CUs — the group's samples and the moved points: a relabelled one (FLAG | slot | bin) whose map entry
// says its node was queued again is read, binned three levels below that node, relabelled, counted — with k_hist's geometry.  Leaves at once when round 0 queued nothing.
__global__ __launch_bounds__(TPB) void k_hist2(BuildArgs a, uint32_t ordinal) {
	Ctl* ctl = ctl_of(a);
	BatchCtl* bc = batch_of(ctl, ordinal);
	if (bc == nullptr || ctl->abortBatch) return;
	if (slots_in_use(bc) <= min(bc->slotsRound0, SLOT_CAP) || bc->slotsRound0 == 0u) return;
	__shared__ BlockTable tbl;
	const LeafWords leafOf(a, ordinal);
	const uint32_t* map = at<const uint32_t>(a, a.offMap);
	const float4* spilled = at<const float4>(a, a.offSpilled);
	const Samples<false> pts(a, bc);
	const uint32_t n = bc->batchSize, total = n + min(bc->numSpilled, a.spilledCap);
	const bool acct = bc->acct != 0u;
	const uint32_t numChunks = (total + CPB - 1) / CPB;
	if (blockIdx.x >= numChunks) return;
	table_init(tbl);
	__syncthreads();
	for (uint32_t chunk = blockIdx.x; chunk < numChunks; chunk += gridDim.x) {
		uint32_t idx[HCPT], v[HCPT], ent[HCPT];
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) {
			const uint32_t t = chunk * CPB + j * TPB + threadIdx.x;
			idx[j] = t < n ? t : a.groupCap + (t - n);
			v[j] = t < total ? leafOf[idx[j]] : 0u;
		}
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) {
			ent[j] = NONE;                                                       // level << 16 | slot of round 1's slot this sample lies in
			if ((v[j] & LEAF_FLAG) == 0u) continue;
			const uint32_t e = map[v[j] & 0x1fffffu];                           // round 0's map
			if ((e & MAP_LISTED) != 0u) ent[j] = e & 0x7fffffffu;
		}
		float4 p[HCPT];
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) {
			const uint32_t t = chunk * CPB + j * TPB + threadIdx.x;
			p[j] = ent[j] != NONE ? (t < n ? pts[t] : spilled[t - n]) : make_float4(0, 0, 0, 0);
		}
#pragma unroll
		for (uint32_t j = 0; j < HCPT; j++) {
			if (ent[j] == NONE) continue;
			const uint32_t X = quantize(F_GRID, p[j].x, a.minx, a.size), Y = quantize(F_GRID, p[j].y, a.miny, a.size), Z = quantize(F_GRID, p[j].z, a.minz, a.size);
			uint32_t key = ((ent[j] & 0xffffu) << 9) | bin_of(X, Y, Z, ent[j] >> 16);
			leafOf[idx[j]] = LEAF_FLAG | key;
			const uint32_t t = chunk * CPB + j * TPB + threadIdx.x;
			if (acct) key |= (t < n ? batch_of_sample(bc, t) : ACCT_MOVED) << ACCT_BATCH_SHIFT;
			uint32_t rank;
			if (table_add(tbl, key, 1u, &rank) < 0) hist_flush(a, key, 1u, acct);
		}
	}
	__syncthreads();
	for (uint32_t e = threadIdx.x; e < (uint32_t)TBL_CAP; e += TPB) {
		const uint32_t key = tbl.keys[e];
		if (key != TBL_EMPTY) hist_flush(a, key, tbl.vals[e], acct);
	}
}

// cell-centre position of a voxel, voxels.cu:103-114, operation by operation (no contraction): cell (cx, cy, cz) of the 128^3 grid of the
// level-`level` node with coordinates (nX, nY, nZ)
__device__ __forceinline__ float4 voxel_at(const BuildArgs& a, int level, uint32_t nX, uint32_t nY, uint32_t nZ, uint32_t cx, uint32_t cy, uint32_t cz, float colorBits) {
	return voxel_centre(a.size, a.minx, a.miny, a.minz, level, nX, nY, nZ, cx, cy, cz, colorBits);      // (simlod_device.hpp; the import rebuilds root voxels with it)
}
// ... of the cell a sample with 28-bit coordinates (pX, pY, pZ) falls into
__device__ __forceinline__ float4 voxel_of(const BuildArgs& a, int level, uint32_t pX, uint32_t pY, uint32_t pZ, float colorBits) {
	const uint32_t sh = (uint32_t)(SIMLOD_MAX_DEPTH + 1 - level);
	const uint32_t cx = (pX >> sh) & 127u, cy = (pY >> sh) & 127u, cz = (pZ >> sh) & 127u;
	// Node.X/Y/Z of the level-`level` node that contains the sample: the top `level` bits of its 28-bit coordinate (the
	// 2^20 grid the nodes are indexed in is the same fp32 quotient scaled by an exact power of two, simlod_device.hpp quantize)
	const uint32_t nsh = 28u - (uint32_t)level;
	// masked to `level` bits: a coordinate exactly on the max face quantises to 2^20 (2^28 here) and the reference's descent, which
	// looks at bits 19..0 only, files it under node coordinate 0 on that axis (voxels.cu:171-179) — the voxel sits at the LOW face
	const uint32_t nmask = (1u << (uint32_t)level) - 1u;
	return voxel_at(a, level, (pX >> nsh) & nmask, (pY >> nsh) & nmask, (pZ >> nsh) & nmask, cx, cy, cz, colorBits);
}
