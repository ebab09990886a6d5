// construct_state.inc — part of construct.hip (included there, inside namespace simlod::build; not a translation unit of its own): per-group and per-launch state (BatchCtl, Ctl, BuildArgs), the trunk mask, LDS key -> count tables, the side tables' formats (paths, top table, child words), prepare_batch, the group's samples.

// Per-group state (BatchCtl), BATCH_COPIES copies in the control block, group #ordinal of a launch in copy ordinal & 3.
static constexpr uint32_t SLOT_CAP_GRIDS = 256;  // (memory guard's slack: grids one group's splits may allocate; more than that many splits per group and the guard is a group late)
static constexpr uint32_t BATCH_COPIES = 4;      // per-batch state of batch b lives in copy b & 3: the front half of batch b + 1 (count .. expand) and the back halves of
                                                 // batches b and b - 1 (insert, voxelize) are under way together, and batch b + 2 is being prepared
struct BatchCtl {
	uint32_t active, batchSize, ringSlot, batchIndex;
	uint32_t ordinal, tag, slotsRound0, numSpilled;   // tag = batch index + 1 (NodeDir); slotsRound0: slots handed out by k_count's tail, snapshot by k_hist: k_expand's first round
	uint32_t numWork, numClear, numTouched, numCross;    // spill-copy work items | grids k_insert has to clear | leaves with new samples (k_expand allocates their chunks) | leaves k_count saw cross the limit (k_queue)
	uint32_t barrierCount, rootPieces, numVoxItems, numVoxSmall;     // rootPieces: pieces of a root that is still a leaf (k_voxroot)
	uint32_t groupBatches, dirCount, acct, accounted;      // ring batches taken together: 1 in exact mode, up to groupMax in coalesced mode; batchSize = all their samples | acct: an EXACT group of several batches — counts and histograms are kept per batch, the allocator / chunk-pool counters are brought to what batch-by-batch ingestion leaves (account_group) | accounted: that has happened
	uint32_t start[SIMLOD_MAX_BATCHES_PER_LAUNCH + 1];   // sample index of the first sample of batch k of the group (start[groupBatches] = batchSize)
	uint32_t slot[SIMLOD_MAX_BATCHES_PER_LAUNCH];        // its ring slot
	uint32_t decided;                  // k_expand: slots (of all rounds so far) whose workgroup is past its reservations for the NEXT round — once all of a round's are, `reserve` says whether there is one
	unsigned long long reserve;        // split slots << 52 | nodes in use << 32 | spilled points of this batch — ONE word, so a split reserves all or nothing
	unsigned long long reserve0;       // ... as the group began (k_count's first workgroup): what k_queue's entries count from
	// per-batch chunk accounting of an exact group (acct): point chunks batch k of the group would have taken / given back had the batches been ingested one
	// by one (voxels.cu:346-357, 485-538), filled by k_expand; the chunk counters as they stood when the group began (k_count's first workgroup)
	uint32_t acctAlloc0, acctPool0, rootSplitAt, pad5;      // rootSplitAt: a group of several batches (exact or coalesced) in which the ROOT splits: the batch of the group it splits in (k_rootpre); NONE otherwise
	uint32_t acctD[SIMLOD_MAX_BATCHES_PER_LAUNCH], acctF[SIMLOD_MAX_BATCHES_PER_LAUNCH];
};

// Control block at byte 0 of kernel_construct's momentary buffer.  Lives only for the duration of one launch
// (the recycle stack behind it, like the reference's chunkQueue, must survive between launches).
struct Ctl {
	uint32_t uploaded, firstBatch, numBatches, stop;
	uint32_t errors, abortBatch, rebuildLeafChunks, debugFlags;   // rebuildLeafChunks: this launch found its side tables stale (first launch, reset, wiped or re-laid-out momentary buffer): k_rebuild / k_paths clear the tag words and refill parents, chunk table, paths and the top table — otherwise they are what the launch before left
	uint32_t processed, budgetUs, consumed, groupMax;   // groups completed in this launch | its time budget in us (voxels.cu:22: 10 ms; SIMLOD_DEBUG_BUDGET_US overrides) | ring batches taken so far | batches per group (1: exact mode)
	uint64_t startNs;
	uint32_t statCounters[8];
	uint32_t tableMagic, tableBatch;   // leaf chunk table is valid for the octree as it was after batch #tableBatch (k_finish) ...
	uint64_t tableNodes, tablePers;    // ... of THIS octree (node array, persistent buffer)
	uint64_t tableSig;                 // table_signature() of the Stats the table belongs to
	uint64_t tableLayout;              // layout_signature() of the momentary buffer the side tables were built in
	uint64_t pointsTaken;              // samples of all batches taken so far, this launch's included (Stats.numPointsProcessed follows when their back halves have run)
	uint32_t chainCap, segLen;         // a chained launch (simlod_launch_construct_chain): batches it may take in all | ... per SEGMENT — what one of the launches it stands for would take; a plain launch is one segment
	uint64_t unused1;
	uint64_t expandNs[8];              // byte 152: k_expand phase times of workgroup 0 (in-kernel histogram pass, barrier, decide + build, barrier, [4] = groups ingested so far (bench.py), rounds, calls; tools/probe.py), [7] = spilled points so far (bench.py)
	uint64_t voxT[SIMLOD_MAX_BATCHES_PER_LAUNCH][3];   // byte 216: k_voxelize of group #ordinal of the last launch: first workgroup in, last piece done, last workgroup out (tools/probe.py)
	uint64_t phaseNs[48];              // byte 696: phase times of one workgroup per kernel, summed over the launches since the host last cleared them (tools/probe.py)
	BatchCtl batch[BATCH_COPIES];
	uint32_t tagOf[SIMLOD_MAX_BATCHES_PER_LAUNCH];     // tag of group #ordinal of this launch (whoever closes a group's voxel lists later needs it: its parity copy is recycled by then)
	// when the SEGMENT of group #ordinal began (prepare_batch of the segment's first group; the groups behind it copy it): what end_of_batch measures the time
	// budget from.  Per ordinal, not per launch: the back half lags the front, which may have begun the next segment already.  (BatchCtl has no room for
	// 8 more bytes — tools read it by offset — so the group's copy lives here)
	uint64_t segStart[SIMLOD_MAX_BATCHES_PER_LAUNCH];
};
static_assert(offsetof(Ctl, voxT) == 216 && offsetof(Ctl, phaseNs) == 696, "tools/probe.py reads Ctl.voxT at byte 216, Ctl.phaseNs at byte 696");
static_assert(offsetof(Ctl, expandNs) == 152, "bench.py / tools read Ctl.expandNs at byte 152");
static_assert(offsetof(Ctl, batch) == 1080 && sizeof(BatchCtl) == 440, "tools/batch_shape.py reads Ctl.batch at byte 1080");
static_assert(sizeof(Ctl) <= 4096, "control block");

struct BuildArgs {
	SimlodPoint* ring;
	uint8_t*     mom;
	uint8_t*     pers;
	SimlodNode*  nodes;
	SimlodStats* stats;
	uint64_t*    frameStart;
	uint32_t*    numBatchesUploaded;
	uint32_t*    batchSizes;
	float        minx, miny, minz, size;
	uint64_t     persCapacity, frameCounter, scratchBytes;
	uint64_t     offQueue, offSlots, offHist, offMap, offClear, offTouched, offSplitTag, offRetryTag, offParent, offNodeDir, offChunkDir, offLeafChunks, offPaths, offWork, offLeafOf, offVoxItems, offSpilled, offHashDir, offTouchTag, offStartOf, offCross, offTop, offKid, leafOfStride;
	uint32_t     nodeCapacity, spilledCap, dirCap, workCap, voxItemCap, clearCap, hashCap, groupCap, groupMax, crossCap;   // groupCap = groupMax * 1 000 000: where the moved points' words start in leafOf
	uint64_t     trunkLo, trunkHi;   // simlod_context_set_trunk_mask: nodes of levels 0-2 that split whatever they hold (multi-GPU: the shared upper levels); zero on one GPU
	uint64_t     offCntB, offHistB;  // exact groups (acct): per node, samples of batch k of the group (groupMax words) | per (slot, bin), likewise
	uint32_t     acct, pad;          // exact mode with groups of several batches (groupMax > 1): see account_group
};

// ---- the shared upper levels of a multi-GPU job (include/simlod_hip.h simlod_context_set_trunk_mask; no counterpart in the reference, which is
// single-GPU) ----  Ranks own level-3 cells of one global cube; the nodes of levels 0-2 exist on every rank.  A rank that split them by ITS counts
// would keep one as a leaf where the single-GPU octree of the whole data set has an inner node (voxels.cu:209-217: a leaf splits when the count
// under it crosses 50 000 — the GLOBAL count there), and kernel_render would draw that rank's points where the single GPU draws voxels
// (render.cu:918-932).  So the host names the upper nodes whose global count exceeds the limit: such a node splits as soon as it exists.
// Bit 0: the root; 1 + c: the level-1 node with cell code c = x << 2 | y << 1 | z; 9 + c: the level-2 node, c = the level-1 octant << 3 | the octant below.
static constexpr uint32_t TRUNK_LEVELS = 3, TRUNK_NODES = 1 + 8 + 64;
__device__ __forceinline__ bool trunk_any(const BuildArgs& a) { return (a.trunkLo | a.trunkHi) != 0ull; }
__device__ __forceinline__ uint32_t trunk_index(uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	return level == 0u ? 0u : level == 1u ? 1u + ((X & 1u) << 2 | (Y & 1u) << 1 | (Z & 1u))
	                        : 9u + ((((X >> 1) & 1u) << 2 | ((Y >> 1) & 1u) << 1 | ((Z >> 1) & 1u)) << 3 | ((X & 1u) << 2 | (Y & 1u) << 1 | (Z & 1u)));
}
__device__ __forceinline__ bool trunk_forced(const BuildArgs& a, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	if (level >= TRUNK_LEVELS) return false;
	const uint32_t i = trunk_index(level, X, Y, Z);
	return (((i < 64u ? a.trunkLo : a.trunkHi) >> (i & 63u)) & 1ull) != 0ull;
}


// ---- workgroup-level key -> count aggregation in LDS ------------------------------------------------------------------
// A device-scope atomic on ONE address retires at ~88 M/s on this chip (MI355X_MICROARCH.md, rows fanin / dequeue), and a
// spatially compact 1 M-point batch funnels most of its points into a few dozen leaves: per-wave aggregation still
// leaves ~16 k atomics per hot counter per batch.  So every counter update of the build (leaf arrival counters, slot
// reservations, voxel counters) is first combined per WORKGROUP in an open-addressing LDS table and flushed with one
// global atomic per (workgroup, node).  table_add returns the entry and the value the entry's counter had before
// (= rank of this caller inside the workgroup), or -1 when 16 probes found no room; a key that failed once keeps
// failing (entries are never removed), so callers can fall back to a direct global atomic consistently.
static constexpr uint32_t TBL_EMPTY = 0xffffffffu;
static constexpr int TBL_BITS = 10;
static constexpr int TBL_CAP = 1 << TBL_BITS;

struct BlockTable {
	uint32_t keys[TBL_CAP];
	uint32_t vals[TBL_CAP];
};

__device__ __forceinline__ void table_init(BlockTable& t) {
	for (uint32_t i = threadIdx.x; i < (uint32_t)TBL_CAP; i += blockDim.x) { t.keys[i] = TBL_EMPTY; t.vals[i] = 0u; }
}

__device__ __forceinline__ uint32_t table_hash(uint32_t key) { return (key * 2654435761u) >> (32 - TBL_BITS); }

__device__ __forceinline__ int table_add(BlockTable& t, uint32_t key, uint32_t inc, uint32_t* rank) {
	uint32_t h = table_hash(key);
#pragma unroll 1
	for (int probe = 0; probe < 16; ++probe) {
		uint32_t k = t.keys[h];
		if (k == TBL_EMPTY) { k = atomicCAS(&t.keys[h], TBL_EMPTY, key); if (k == TBL_EMPTY) k = key; }
		if (k == key) { *rank = atomicAdd(&t.vals[h], inc); return (int)h; }
		h = (h + 1) & (TBL_CAP - 1);
	}
	return -1;
}

// The same table with every counter REP times (k_count): a swath-ordered batch sends most lanes of a wave to a handful of leaves, and the LDS
// serialises atomics of one instruction on one address lane by lane (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE was 0.88 in k_count).  Lane l
// adds to copy l % REP — REP consecutive words, REP different banks — and the flush sums the copies.
template <uint32_t REP>
struct SpreadTable {
	uint32_t keys[TBL_CAP];
	uint32_t vals[TBL_CAP * REP];
};
template <uint32_t REP>
__device__ __forceinline__ void spread_init(SpreadTable<REP>& t) {
	for (uint32_t i = threadIdx.x; i < (uint32_t)TBL_CAP; i += blockDim.x) t.keys[i] = TBL_EMPTY;
	for (uint32_t i = threadIdx.x; i < (uint32_t)TBL_CAP * REP; i += blockDim.x) t.vals[i] = 0u;
}
template <uint32_t REP>
__device__ __forceinline__ bool spread_add(SpreadTable<REP>& t, uint32_t key, uint32_t copy) {
	uint32_t h = table_hash(key);
#pragma unroll 1
	for (int probe = 0; probe < 16; ++probe) {
		uint32_t k = t.keys[h];
		if (k == TBL_EMPTY) { k = atomicCAS(&t.keys[h], TBL_EMPTY, key); if (k == TBL_EMPTY) k = key; }
		if (k == key) { atomicAdd(&t.vals[h * REP + copy], 1u); return true; }
		h = (h + 1) & (TBL_CAP - 1);
	}
	return false;
}
template <uint32_t REP>
__device__ __forceinline__ uint32_t spread_sum(const SpreadTable<REP>& t, uint32_t e) {
	uint32_t s = 0;
#pragma unroll
	for (uint32_t r = 0; r < REP; r++) s += t.vals[e * REP + r];
	return s;
}

__device__ __forceinline__ int table_find(const BlockTable& t, uint32_t key) {
	uint32_t h = table_hash(key);
#pragma unroll 1
	for (int probe = 0; probe < 16; ++probe) {
		const uint32_t k = t.keys[h];
		if (k == key) return (int)h;
		if (k == TBL_EMPTY) return -1;
		h = (h + 1) & (TBL_CAP - 1);
	}
	return -1;
}



static constexpr uint32_t TPB = 256;

struct NodeDir {          // per node, valid for the batch whose tag it carries: where the leaf's chunks stand in the batch's chunk directory
	uint32_t ptBase, ptFirst, ptTag, pad0;
};

// Leaf chunk table: slot k of leaf i's point list -> chunk, LEAF_SLOTS entries per node.  A leaf that can still split stores
// at most MAX_POINTS_PER_NODE points between batches (= 50 chunks), so the split reads its whole list from here with all
// lanes at once instead of chasing 50 `next` pointers (~1 us each) with one.  Kept up to date by alloc_points (k_expand); survives between
// launches like the recycle stack does, and is refilled by k_rebuild whenever k_begin finds its stamp stale.
static constexpr uint32_t LEAF_SLOTS = LEAF_ROW_SLOTS;      // (rows are packed: simlod_internal.hpp leaf_row_get / leaf_row_set)
static constexpr uint32_t TABLE_MAGIC = 0x51ab1e05u;
static_assert(LEAF_SLOTS <= 64, "queue_split hands a leaf's chunks out one per lane");

// Ancestor paths: a row of PATH_DIRECT 64-bit entries per node, entry k = the k-th ancestor (parent first), zero-terminated when the node has
// fewer than PATH_DIRECT ancestors.
// An entry packs everything `sample` and `insert` need to know about that ancestor — its occupancy grid (offset into the
// persistent buffer), level and node index — so a sample reads its whole root path with independent loads instead of chasing
// parent -> node -> grid pointers level by level.
// A node deeper than PATH_DIRECT levels continues in the row of its PATH_DIRECT-th ancestor (the node its row's last entry names), whose row
// holds that ancestor's ancestors, and so on: entry k >= PATH_DIRECT of a node is entry k - PATH_DIRECT of that ancestor (path_far) — one more
// dependent load per PATH_DIRECT levels, paid only by leaves below level PATH_DIRECT.  (Rounds 1-7: a row held all 20 possible ancestors,
// 168 bytes per node; the terrain's leaves lie at levels 5-7, a hotspot's around 10 — more than half of every row was never read.)
// Rebuilt for every node when the side tables are stale (rebuild_side_tables), extended for the eight children at a split (k_expand).
#ifndef PATH_DIRECT
#define PATH_DIRECT 12      /* `make variant DEFS=-DPATH_DIRECT=...` */
#endif
static constexpr uint32_t PATH_WORDS = SIMLOD_MAX_DEPTH + 1;      // a whole path in LDS: up to 20 ancestors and the terminator
static constexpr uint32_t PATH_ROW = PATH_DIRECT;                 // entries of a node's row in the table
static_assert(PATH_ROW >= 3u && PATH_ROW <= (uint32_t)SIMLOD_MAX_DEPTH, "k_expand writes up to three entries of a new node's row before it copies the slot node's path");
static constexpr unsigned long long PATH_VALID = 1ull << 63;

__device__ __forceinline__ unsigned long long path_pack(const uint8_t* pers, uint32_t nodeIdx, uint32_t level, const SimlodOccupancyGrid* grid) {
	const unsigned long long off = (unsigned long long)(reinterpret_cast<const uint8_t*>(grid) - pers) >> 4;     // grids are 16-byte aligned allocations
	return PATH_VALID | ((unsigned long long)nodeIdx << 41) | ((unsigned long long)level << 36) | off;
}
__device__ __forceinline__ uint32_t path_node(unsigned long long e) { return (uint32_t)(e >> 41) & 0x7ffffu; }
__device__ __forceinline__ uint32_t path_level(unsigned long long e) { return (uint32_t)(e >> 36) & 31u; }
__device__ __forceinline__ SimlodOccupancyGrid* path_grid(uint8_t* pers, unsigned long long e) {
	return reinterpret_cast<SimlodOccupancyGrid*>(pers + ((e & 0xfffffffffull) << 4));
}
// entry k >= PATH_ROW of `node`'s path, for a node that has more than k ancestors (so every row on the way is full): through the continuation rows.
// (A last entry that names no node of this table — an image whose node is not where its level says — ends the path.)
__device__ inline unsigned long long path_far(const unsigned long long* paths, uint32_t node, uint32_t k, uint32_t nodeCapacity) {
	while (k >= PATH_ROW) {
		const unsigned long long last = paths[(uint64_t)node * PATH_ROW + (PATH_ROW - 1u)];
		node = path_node(last); k -= PATH_ROW;
		if (last == 0ull || node >= nodeCapacity) return 0ull;
	}
	return paths[(uint64_t)node * PATH_ROW + k];
}

// Top table: for every cell of the 32^3 grid of level 5, the deepest node at level <= 5 that contains it, as node | level << 19 — where k_count's
// descent STARTS (one load instead of up to five dependent ones; nodes are never removed, so an entry is always a valid starting point).
// Rebuilt at the start of every launch (k_paths), kept current by k_expand: only a split of a leaf at level <= 4 makes nodes that belong in
// it, which a stream does in its first batches over a region and hardly ever again (the 36 M terrain: leaves live at levels 6 to 8).
// (Round 3 measured the same idea one level deeper — 64^3, level 6 — and dropped it: every other split had to update it, +3.4 us in k_expand.)
static constexpr uint32_t TOP_LEVEL = 5, TOP_SIDE = 1u << TOP_LEVEL, TOP_CELLS = TOP_SIDE * TOP_SIDE * TOP_SIDE;
__device__ __forceinline__ uint32_t top_cell(uint32_t X, uint32_t Y, uint32_t Z) {      // X, Y, Z: 20-bit grid coordinates (bits 19..0 count, as in the descent)
	const uint32_t s = (uint32_t)SIMLOD_MAX_DEPTH - TOP_LEVEL;
	return (((X >> s) & (TOP_SIDE - 1u)) << (2u * TOP_LEVEL)) | (((Y >> s) & (TOP_SIDE - 1u)) << TOP_LEVEL) | ((Z >> s) & (TOP_SIDE - 1u));
}
// node `idx` at `level` <= TOP_LEVEL with coordinates (X, Y, Z) becomes the entry of every cell it covers
__device__ __forceinline__ void top_fill(uint32_t* top, uint32_t idx, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z, uint32_t mark) {      // mark: TOP_LEAF for a node without children
	const uint32_t k = TOP_LEVEL - level, side = 1u << k, x0 = X << k, y0 = Y << k, z0 = Z << k, e = idx | (level << 19) | mark;      // (sides are powers of two: shifts, no division)
	for (uint32_t i = 0; i < (1u << (3u * k)); i++) {
		const uint32_t dx = i >> (2u * k), dy = (i >> k) & (side - 1u), dz = i & (side - 1u);
		top[((x0 + dx) << (2u * TOP_LEVEL)) | ((y0 + dy) << TOP_LEVEL) | (z0 + dz)] = e;
	}
}

// Child words: ONE 32-bit word per node instead of its eight 8-byte child pointers spread over a 152-byte record — what k_count's descent reads.  A node that
// splits gets all eight children at once, in eight consecutive node slots (voxels.cu:316-343: atomicAdd(&stats->numNodes, 8); here: k_queue / reserve()), so
// the word holds the FIRST child's index (19 bits) and, above it, which of the eight are leaves (8 bits): a sample that steps into a child marked as a leaf
// is done without looking at that child.  0: the node has no children.  KID_IRREGULAR: children that are not eight consecutive nodes (an image neither this
// builder nor the reference made): that node is descended through Node.children as before.  The 36 M terrain's 4 425 nodes: 17 KB, L1-resident, against
// 4 425 x 152 B of records of which a step used 8 bytes.  Kept current by k_expand (a node that splits clears its bit in its parent's word), restored from
// the node array with the other side tables (rebuild_side_tables).  The top table's entries carry the same mark (TOP_LEAF).
static constexpr uint32_t KID_IRREGULAR = 0xffffffffu, KID_LEAF_SHIFT = 19, TOP_LEAF = 0x80000000u;
__device__ __forceinline__ uint32_t octant_of(uint32_t X, uint32_t Y, uint32_t Z) { return ((X & 1u) << 2) | ((Y & 1u) << 1) | (Z & 1u); }      // a node's place among its parent's children (voxels.cu:320-322)

__device__ __forceinline__ Ctl* ctl_of(const BuildArgs& a) { return reinterpret_cast<Ctl*>(a.mom); }
template <class T> __device__ __forceinline__ T* at(const BuildArgs& a, uint64_t off) { return reinterpret_cast<T*>(a.mom + off); }

// the per-batch state of batch #ordinal of this launch, or nullptr when that batch does not exist (the copy of its parity may still
// hold an earlier batch: the launch enqueues kernels for 20 batches whether they exist or not)
__device__ __forceinline__ BatchCtl* batch_of(Ctl* ctl, uint32_t ordinal) {
	BatchCtl* bc = &ctl->batch[ordinal % BATCH_COPIES];
	return bc->active != 0u && bc->ordinal == ordinal ? bc : nullptr;
}

// phase timer of ONE thread of one workgroup per kernel: adds the time since `t` to slot k and restarts `t` (builds with SIMLOD_MEASURE only: `on` is a
// compile-time false in the product library and every mark() folds away)
struct Phase {
	Ctl* ctl; bool on; uint64_t t;
	__device__ __forceinline__ Phase(Ctl* c, bool who) : ctl(c), on(SIMLOD_MEASURE != 0 && who && threadIdx.x == 0), t(on ? wall_ns() : 0) {}
	__device__ __forceinline__ void mark(uint32_t k) { if (on) { const uint64_t n = wall_ns(); ctl->phaseNs[k] += n - t; t = n; } }
};

// The chunk directory, k_voxelize's work items and the cached-leaf words of a batch exist twice, by the parity of the batch's ordinal: batch
// b + 1's are written by its front half (k_count .. k_expand) while the back half of batch b (k_insert, k_voxelize) is still reading its own.
struct VoxItem;
__device__ __forceinline__ SimlodChunk** chunk_dir(const BuildArgs& a, const BatchCtl* bc) { return at<SimlodChunk*>(a, a.offChunkDir) + (uint64_t)(bc->ordinal & 1u) * a.dirCap; }
__device__ __forceinline__ VoxItem* vox_items(const BuildArgs& a, const BatchCtl* bc);

__device__ __forceinline__ void raise(Ctl* ctl, uint32_t bit) { atomicOr(&ctl->errors, bit); }
// conditions after which the batch cannot be completed: the rest of the chain does nothing, Stats.dbg keeps the bit until a reset
__device__ __forceinline__ void panic(Ctl* ctl, uint32_t bit) { atomicOr(&ctl->errors, bit); ctl->abortBatch = 1; ctl->stop = 1; }

// Worst case of what the voxel half of a batch can still add to the persistent buffer (voxel chunks: every sample can colour one voxel per
// level, every inner node can start one more chunk).  The memory guard of voxels.cu:896-912 looks at the allocator after the WHOLE previous
// batch; here a batch is prepared while the voxel halves of the TWO batches before it may still be running, so within this distance of the
// guard a launch takes one batch only: the next launch's k_begin runs after everything and decides exactly.
__host__ __device__ inline unsigned long long group_slack_bytes(unsigned long long samples, unsigned long long numNodes);
__device__ __forceinline__ unsigned long long slack_for(const BuildArgs& a, unsigned long long samples) { return group_slack_bytes(samples, a.stats->numNodes); }
__host__ __device__ inline unsigned long long group_slack_bytes(unsigned long long samples, unsigned long long numNodes) {
	// (+ the point chunks and grids the group before has yet to allocate: its k_expand runs after this look at the allocator)
	return (2ull * (samples * SIMLOD_MAX_DEPTH / SIMLOD_POINTS_PER_CHUNK + numNodes + 1ull) + samples / SIMLOD_POINTS_PER_CHUNK + 4096ull) * SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk))
	       + (unsigned long long)SLOT_CAP_GRIDS * SIMLOD_ALLOC_ROUND(sizeof(SimlodOccupancyGrid));
}
__device__ __forceinline__ unsigned long long voxel_half_slack(const BuildArgs& a, const BatchCtl* prev) {
	return slack_for(a, (unsigned long long)prev->batchSize + prev->numSpilled);
}

// Make group #ordinal of this launch current (in copy ordinal & 3), or leave it inactive (progressive_octree_voxels.cu:890-912).  Runs on the
// FRONT stream: k_begin for the first group, one thread of k_hist of the group before for the others (so that k_count can follow k_expand
// without a kernel in between; what depends on that k_expand — the node array's fill, the chunk pool's high-water mark — is set by
// k_count's first workgroup).
// Exact mode: a group is ONE ring batch, the reference's granularity.  Coalesced mode (simlod_set_ingest_mode(1)): the next groupMax
// pending batches are counted, split, stored and voxelized as one; the memory guard is looked at once per group.
__device__ void prepare_batch(const BuildArgs& a, Ctl* ctl, uint32_t ordinal) {
	BatchCtl* bc = &ctl->batch[ordinal % BATCH_COPIES];
	bc->active = 0;
	if (ordinal >= SIMLOD_MAX_BATCHES_PER_LAUNCH || ctl->consumed >= ctl->numBatches) return;
	if (__hip_atomic_load(&ctl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;      // (set by the back half of an earlier group: time budget, abort)
	const SimlodAllocatorGlobal* alloc = reinterpret_cast<const SimlodAllocatorGlobal*>(a.pers);
	if (ordinal > 0u && alloc->offset + SIMLOD_MEM_SAFETY_MARGIN + voxel_half_slack(a, &ctl->batch[(ordinal - 1u) % BATCH_COPIES]) >= a.persCapacity) { ctl->stop = 1; return; }
	const bool full = alloc->offset + SIMLOD_MEM_SAFETY_MARGIN >= a.persCapacity;
	a.stats->memCapacityReached = full ? 1 : 0;
	if (full) { ctl->stop = 1; return; }
	const uint32_t batchIndex = ctl->firstBatch + ctl->consumed;       // (Stats.batchletIndex itself is advanced by the back half, which may lag)
	// (a chain: no group straddles a segment boundary — the groups are those of the launches the chain stands for, and so are the voxel colours)
	const uint32_t intoSegment = ctl->consumed % ctl->segLen;
	uint32_t take = min(min(ctl->groupMax, ctl->numBatches - ctl->consumed), ctl->segLen - intoSegment);
	// voxels.cu:936-949: the 10 ms are a launch's — here a segment's: stamped when its first group is prepared (the chain's first: the launch's own start)
	ctl->segStart[ordinal] = ordinal == 0u ? ctl->startNs : intoSegment == 0u ? wall_ns() : ctl->segStart[ordinal - 1u];
	if (a.acct != 0u && take > 1u) {
		// An EXACT group of several batches is taken only where the reference's guard — looked at before EVERY batch (voxels.cu:896-912) — cannot
		// trip inside it: the allocator must be a worst-case group away from it.  Closer than that, the launch goes batch by batch as before.
		unsigned long long samples = 0;
		for (uint32_t k = 0; k < take; k++) samples += min(a.batchSizes[(batchIndex + k) % SIMLOD_BATCH_STREAM_SIZE], (uint32_t)SIMLOD_MAX_BATCH_SIZE);
		// (stored points a split moves are sampled again: at most what the octree holds, at most what the spill buffer takes)
		samples += min((unsigned long long)a.spilledCap, (unsigned long long)ctl->pointsTaken);
		const unsigned long long before = ordinal > 0u ? voxel_half_slack(a, &ctl->batch[(ordinal - 1u) % BATCH_COPIES]) : 0ull;
		if (alloc->offset + SIMLOD_MEM_SAFETY_MARGIN + before + slack_for(a, samples) >= a.persCapacity) take = 1u;
	}
	uint32_t total = 0;
	for (uint32_t k = 0; k < take; k++) {
		const uint32_t slot = (batchIndex + k) % SIMLOD_BATCH_STREAM_SIZE;
		uint32_t size = a.batchSizes[slot];
		if (size > SIMLOD_MAX_BATCH_SIZE) size = SIMLOD_MAX_BATCH_SIZE;
		bc->start[k] = total; bc->slot[k] = slot;
		total += size;
	}
	bc->start[take] = total;
	ctl->consumed += take;
	ctl->pointsTaken += total;
	bc->groupBatches = take;
	bc->batchIndex = batchIndex;
	bc->ringSlot = bc->slot[0];
	bc->batchSize = total;
	bc->ordinal = ordinal;
	bc->tag = batchIndex + 1u;
	ctl->tagOf[ordinal] = bc->tag;
	bc->slotsRound0 = 0;
	bc->numSpilled = 0;
	bc->numWork = 0;
	bc->numClear = 0;
	bc->numTouched = 0;
	bc->numCross = 0;
	bc->barrierCount = 0;      // every k_expand instance counts its barrier generations from zero
	bc->decided = 0;
	bc->numVoxItems = 0;
	bc->numVoxSmall = 0;
	bc->rootPieces = 0;
	bc->dirCount = 0;
	bc->reserve = 0;           // (k_count's first workgroup: the node array as k_expand of the group before leaves it)
	bc->acct = a.acct != 0u && take > 1u ? 1u : 0u;
	bc->accounted = 0;
	bc->rootSplitAt = 0xffffffffu;
	for (uint32_t k = 0; k < SIMLOD_MAX_BATCHES_PER_LAUNCH; k++) { bc->acctD[k] = 0; bc->acctF[k] = 0; }
	bc->active = 1;
}

// The samples of the current group: batch k of the group holds samples [start[k], start[k + 1]) in its ring slot (a batch holds at most
// 1 000 000 samples, so batch i / 1 000 000 is the first candidate).  Exact mode — one batch per group — is a plain array.
// (SINGLE: the kernel was launched for exact mode — the host knows — and carries no trace of the group lookup)
template <bool SINGLE>
struct Samples {
	const float4* ring; const float4* only; const BatchCtl* bc; uint32_t batches;
	__device__ __forceinline__ Samples(const BuildArgs& a, const BatchCtl* b) : ring(reinterpret_cast<const float4*>(a.ring)), bc(b), batches(b->groupBatches) {
		only = ring + (size_t)b->ringSlot * SIMLOD_MAX_BATCH_SIZE;
	}
	__device__ __forceinline__ const float4* ptr(uint32_t i) const {
		if (SINGLE || batches == 1u) return only + i;
		uint32_t k = min(i / SIMLOD_MAX_BATCH_SIZE, batches - 1u);
		while (k + 1u < batches && i >= bc->start[k + 1u]) k++;
		return ring + (size_t)bc->slot[k] * SIMLOD_MAX_BATCH_SIZE + (i - bc->start[k]);
	}
	__device__ __forceinline__ float4 operator[](uint32_t i) const { return *ptr(i); }
	// Do the samples i0 .. i1 of the group lie in ONE ring batch (a workgroup's tile of consecutive samples does, as a rule: a batch has up to a million)?
	// Then sample i is base[i] and its batch of the group is k — without a lookup per sample (the walk through start[] in front of every load was a
	// dependent round trip in front of the kernels' first HBM access).
	__device__ __forceinline__ bool span(uint32_t i0, uint32_t i1, const float4*& base, uint32_t& k) const {
		k = 0; base = only;
		if (SINGLE || batches == 1u) return true;
		k = min(i0 / SIMLOD_MAX_BATCH_SIZE, batches - 1u);
		while (k + 1u < batches && i0 >= bc->start[k + 1u]) k++;
		base = ring + (size_t)bc->slot[k] * SIMLOD_MAX_BATCH_SIZE - bc->start[k];
		return i1 < bc->start[k + 1u];
	}
};

// what the stamp remembers of the momentary buffer's layout: side tables of another node capacity / buffer size / group size / path row format are not these
// (rows of PATH_ROW entries with continuation: a stamp left by a build with whole-path rows, which had no such term, or with another row length does not match)
__host__ __device__ inline uint64_t layout_signature(const BuildArgs& a) {
	return a.scratchBytes ^ ((uint64_t)a.nodeCapacity << 40) ^ ((uint64_t)a.groupMax << 59) ^ (a.offSpilled * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)PATH_ROW * 0xC2B2AE3D27D4EB4Full);
}
