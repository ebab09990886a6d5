// construct_voxelize.inc — part of construct.hip (included there, inside namespace simlod::build; not a translation unit of its own): the voxel half: voxel chunks on demand (hash directory), k_voxelize (pieces, small items, a root that is still a leaf), the end-of-batch bookkeeping.

// ---- voxel chunks, on demand (voxels.cu:641-698 allocateVoxelChunks + insertVoxels in one pass) ------------------------------------------
// A reservation in a node's voxel list is the return value of the add to Node.numVoxels (voxels.cu:101): slots [old, old + n).  Whoever
// holds slot k * 1000 allocates chunk k of the list (voxel chunks never come from the recycle stack, voxels.cu:656-659), publishes it in
// a hash directory of the batch ((node, k) -> chunk) and links it behind its predecessor; whoever holds another slot of chunk k looks it up —
// or takes the list's old tail, if the chunk existed when the batch began (Node.numVoxelsStored and the tail pointer in the head chunk stay
// as they were until k_voxdone).  An allocator publishes everything it owns BEFORE it waits for anybody (its predecessor's allocator, whose
// add came first and who is therefore already running), so every wait ends.
struct DirEntry { unsigned long long key; SimlodChunk* ptr; };
static constexpr unsigned long long DIR_BUSY = 1ull << 62;
__device__ __forceinline__ unsigned long long dir_key(uint32_t tag, uint32_t node, uint32_t k) {
	return (1ull << 63) | ((unsigned long long)(tag & 0xfffffu) << 42) | ((unsigned long long)node << 22) | (k & 0x3fffffu);
}
__device__ __forceinline__ uint32_t dir_tag(unsigned long long key) { return (uint32_t)(key >> 42) & 0xfffffu; }
__device__ __forceinline__ uint32_t dir_hash(const BuildArgs& a, unsigned long long key) {
	key ^= key >> 29; key *= 0x9e3779b97f4a7c15ull; key ^= key >> 32;
	return (uint32_t)key & (a.hashCap - 1u);
}
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ void dir_insert(const BuildArgs& a, Ctl* ctl, uint32_t tag, uint32_t node, uint32_t k, SimlodChunk* c) {
	DirEntry* dir = at<DirEntry>(a, a.offHashDir);
	const unsigned long long key = dir_key(tag, node, k);
	uint32_t h = dir_hash(a, key);
	for (uint32_t probe = 0; probe < a.hashCap; probe++, h = (h + 1u) & (a.hashCap - 1u)) {
		unsigned long long cur = ld_agent(&dir[h].key);
		while (cur == 0ull || ((cur >> 63) != 0ull && dir_tag(cur) != (tag & 0xfffffu))) {           // free, or left over from an earlier batch
			const unsigned long long prev = atomicCAS(&dir[h].key, cur, DIR_BUSY);
			if (prev == cur) {
				// pointer first, key second: a reader that sees the key must see the pointer (write-through stores, drained in between)
				__hip_atomic_store(reinterpret_cast<unsigned long long*>(&dir[h].ptr), (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__hip_atomic_store(&dir[h].key, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				return;
			}
			cur = prev;
		}
	}
	panic(ctl, SIMLOD_ERR_DIRECTORY_FULL);
}
// non-blocking lookup; nullptr when the entry is not (yet) there
__device__ SimlodChunk* dir_find(const BuildArgs& a, uint32_t tag, uint32_t node, uint32_t k) {
	const DirEntry* dir = at<const DirEntry>(a, a.offHashDir);
	const unsigned long long key = dir_key(tag, node, k);
	uint32_t h = dir_hash(a, key);
	for (uint32_t probe = 0; probe < a.hashCap; probe++, h = (h + 1u) & (a.hashCap - 1u)) {
		const unsigned long long cur = ld_agent(&dir[h].key);
		if (cur == key) return reinterpret_cast<SimlodChunk*>(ld_agent(reinterpret_cast<const unsigned long long*>(&dir[h].ptr)));
		if (cur == 0ull) return nullptr;
		if ((cur >> 63) != 0ull && dir_tag(cur) != (tag & 0xfffffu)) return nullptr;
	}
	return nullptr;
}
// blocking lookup (see above: it ends; the bound is a guard against a broken device)
__device__ SimlodChunk* dir_wait(const BuildArgs& a, Ctl* ctl, uint32_t tag, uint32_t node, uint32_t k) {
	for (uint32_t spin = 0;; spin++) {
		SimlodChunk* c = dir_find(a, tag, node, k);
		if (c != nullptr) return c;
		__builtin_amdgcn_s_sleep(2);
		if ((spin & 255u) == 255u && __hip_atomic_load(&ctl->abortBatch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return nullptr;
		if (spin > (1u << 22)) { panic(ctl, SIMLOD_ERR_DIRECTORY_FULL); return nullptr; }
	}
}
// chunk k of node's voxel list exists from now on (the caller holds slot k * 1000)
__device__ __forceinline__ void vox_chunk_publish(const BuildArgs& a, Ctl* ctl, uint32_t tag, uint32_t node, uint32_t k, SimlodChunk* c) {
	// an inner node's row of the leaf chunk table lists its voxel chunks: the rasteriser reads the list from there (render.hip r_visible) — never
	// the root's: its row may still be read as a LEAF's by the next batch's k_count, which splits a root that was still a leaf
	if (k < LEAF_SLOTS && node != 0u) leaf_row_set(a.mom + a.offLeafChunks, a.pers, node, k, c);
	dir_insert(a, ctl, tag, node, k, c);
}
// ... and hangs behind its predecessor: the head pointer, the old tail, or a chunk of this batch (which may have to be waited for).
// Every `next` field has ONE writer per kernel — the allocator of the chunk behind it, or, for the list's last chunk, k_voxdone (the L2s of
// the eight XCDs are not coherent with each other for plain stores: an allocator that cleared its own chunk's `next` could overwrite, at
// write-back time, the link its successor's allocator has made from another XCD).
__device__ __forceinline__ void vox_chunk_link(const BuildArgs& a, Ctl* ctl, uint32_t tag, uint32_t node, uint32_t k, uint32_t existing, SimlodChunk* oldTail, SimlodChunk* c) {
	if (k == 0u) a.nodes[node].voxelChunks = c;
	else {
		SimlodChunk* pred = k - 1u < existing ? oldTail : dir_wait(a, ctl, tag, node, k - 1u);
		if (pred != nullptr) pred->next = c;
	}
}
// A wave stores one voxel per `go` lane: lane's slot in `node`'s voxel list (lanes may name different nodes).  All allocations of the
// wave come before any of its waits (a lane may wait for a chunk another lane of the same wave opens).
__device__ __forceinline__ void store_voxels_wave(const BuildArgs& a, Ctl* ctl, uint32_t tag, bool go, uint32_t node, uint32_t slot, const float4& vox) {
	const uint32_t k = slot / SIMLOD_POINTS_PER_CHUNK, r = slot % SIMLOD_POINTS_PER_CHUNK;
	const uint32_t existing = go ? (a.nodes[node].numVoxelsStored + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK : 0u;
	SimlodChunk* mine = nullptr;
	if (go && r == 0u) {
		mine = reinterpret_cast<SimlodChunk*>(persistent_alloc(a.pers, sizeof(SimlodChunk), 1));
		vox_chunk_publish(a, ctl, tag, node, k, mine);             // (its `next`: see vox_chunk_link)
	}
	if (go) {
		SimlodChunk* oldTail = existing > 0u ? tail_of(a.nodes[node].voxelChunks) : nullptr;
		if (mine != nullptr) vox_chunk_link(a, ctl, tag, node, k, existing, oldTail, mine);
		SimlodChunk* c = mine != nullptr ? mine : k < existing ? oldTail : dir_wait(a, ctl, tag, node, k);
		if (c != nullptr) reinterpret_cast<float4*>(c->points)[r] = vox;
	}
}

// ---- voxelize: 128^3 occupancy test-and-set on every inner node of the root-to-leaf path (voxels.cu:50-121, 417-483) ----------------
// The reference offers every sample to the grid of EVERY node of its path, root first.  Two properties make that cheap here:
//  * Occupancy is hierarchical: a cell of a node covers exactly 2x2x2 cells of the child below it, and every sample that ever set a bit
//    in a node had, in the same pass, been offered to all its ancestors — so "bit set in node N" implies "covering bit set in every
//    ancestor of N".  A sample therefore climbs BOTTOM-UP and stops at the first cell that is already set.  The same argument covers the
//    points a split moved into new leaves (voxels.cu:325-415 re-samples them from the split node's level down): above the split node
//    their cells were set when they first arrived, so their climb ends there by itself.
//  * After k_insert the new samples of a leaf lie together in its chunks, and the part of an ancestor's grid a leaf can touch is a
//    small cube: 64^3 cells of the parent, 32^3 of the grandparent, ... one cell from the 8th ancestor on — 37 KB of bits in all.
// So this kernel runs AFTER k_insert, one workgroup per (leaf, range of <= 8192 new samples): it loads the leaf's cubes into LDS, keeps
// its 8 samples per thread in registers, and does the whole test-and-set in LDS.  Round 1 sampled BEFORE the insert, per batch sample,
// with device-scope atomicOr: a 1 M-point batch is spatially compact, nearly every sample of a freshly entered region found its cell
// clear at the same moment, and a thousand workgroups queued their atomics on the same few hundred words (measured: one wave waited
// 55-190 us for a single level's atomics; the kernel took 80-90 us with the memory system idle; more samples in flight per thread, or
// fewer workgroups, both made it SLOWER).  Here the global memory sees one atomicOr per touched WORD and piece — it returns which of
// the new cells are really new (the pieces of one leaf share cubes; different leaves never share a cell below the 8th ancestor) —
// and nothing in the two passes over the samples leaves the CU.
//   level 1    every sample (eight per thread, in registers): test-and-set of its cell in the parent's cube; the samples that found their cell
//              clear are the level's WINNERS: they go on a list (LDS) — cell and sample number in one word
//   level d    the winners of level d - 1, DENSELY (a list entry per lane, not a sample per lane: three samples in four lose at level 1 and
//              would idle through six more levels): test-and-set in cube d, winners on the list of level d.  The lists shrink with the cubes
//              (<= 4096, 512, 64, 8, 1 winners from d = 3 on); from the 8th ancestor on the leaf is ONE cell: the last winner climbs alone
//   write-back  old = atomicOr(grid word, bits set here); won = those & ~old; Node.numVoxels += popcount(won)   (voxels.cu:96-101).  What a
//              thread set = its LDS words now minus the same words as it loaded them (kept in registers): no second bit plane
//   reserve    per ancestor with won cells: slot range from atomicAdd(Node.numVoxels); chunks the range starts are allocated here and now
//   store      a winner whose cell is still marked won colours the voxel — position from the CELL (list entry + the leaf's coordinates),
//              colour from the sample (which sample of a cell does is scheduling dependent in the reference too, SURVEY.md H6) —
//              into slot base + rank (voxels.cu:674-698), through the hash directory of chunks
static constexpr uint32_t VOX_CHUNKS = VOX_PIECE / SIMLOD_POINTS_PER_CHUNK + 2;   // chunks a piece's voxels of one ancestor can span
// winner lists: level d holds at most min(8192, (128 >> d)^3) entries
static constexpr uint32_t VOX_LIST_WORDS = 2 * VOX_PIECE + 4096 + 512 + 64 + 8 + 8;
__device__ __forceinline__ uint32_t list_offset(uint32_t d) { return d == 1u ? 0u : d == 2u ? VOX_PIECE : d == 3u ? 2u * VOX_PIECE : d == 4u ? 2u * VOX_PIECE + 4096u : d == 5u ? 2u * VOX_PIECE + 4608u : d == 6u ? 2u * VOX_PIECE + 4672u : 2u * VOX_PIECE + 4680u; }
struct VoxShared {
	uint32_t occ[CUBE_WORDS];                                   // cubes d = 1..7: rows of (128 >> d) x-bits; d = 1: two words per row.  After the write-back: the cells this piece WON
	uint32_t list[VOX_LIST_WORDS];                              // winner = cell inside the leaf's level-1 cube (6 bits per axis) | sample << 18
	uint32_t listCount[8];                                      // winners of level d
	uint32_t hiOcc[PATH_WORDS], hiFresh[PATH_WORDS];            // ancestors d >= 8: the ONE cell the whole leaf falls into
	uint32_t hiSample;                                          // the sample that climbs beyond the 7th ancestor
	unsigned long long anc[PATH_WORDS];
	uint32_t cnt[PATH_WORDS];
	uint32_t first[PATH_WORDS], rank[PATH_WORDS];               // the slots this piece reserved in ancestor d's voxel list: [first, first + cnt); how many of them are taken
	SimlodChunk* chunkOf[PATH_WORDS][VOX_CHUNKS];               // ... and the chunks they lie in, from chunk first / 1000 on
	float color[VOX_PIECE];                                     // the samples' colours
};
__device__ __forceinline__ uint32_t cube_offset(uint32_t d) {          // word offset of cube d in VoxShared::occ / fresh
	return d == 1u ? 0u : d == 2u ? 8192u : d == 3u ? 9216u : d == 4u ? 9472u : d == 5u ? 9536u : d == 6u ? 9552u : 9556u;
}
__device__ __forceinline__ uint32_t grid_cell(uint32_t level, uint32_t pX, uint32_t pY, uint32_t pZ) {   // voxels.cu:78-92
	const uint32_t shf = (uint32_t)(SIMLOD_MAX_DEPTH + 1) - level;
	return ((pX >> shf) & 127u) + ((pY >> shf) & 127u) * SIMLOD_GRID_SIZE + ((pZ >> shf) & 127u) * SIMLOD_GRID_SIZE * SIMLOD_GRID_SIZE;
}
// A winner names its cell by the cell's position inside the leaf's level-1 cube: code = lx | ly << 6 | lz << 12 (six bits per axis: the
// leaf is 64^3 cells of its parent's grid).  The cell above it in ancestor d's cube (side 128 >> d, aligned to its side) is code >> (d - 1)
// per axis: word and bit in the LDS cubes.
__device__ __forceinline__ void cube_cell_from(uint32_t d, uint32_t code, uint32_t& word, uint32_t& bit) {
	const uint32_t s = d - 1u;
	const uint32_t lx = (code & 63u) >> s, row = (((code >> 6) & 63u) >> s) + ((((code >> 12) & 63u) >> s) << (7u - d));
	if (d == 1u) { word = row * 2u + (lx >> 5); bit = lx & 31u; }
	else { word = cube_offset(d) + row; bit = lx; }
}
// the voxel of that cell in ancestor d of the leaf (LX, LY, LZ) at level leafLevel: the cube starts at cell (L & (2^d - 1)) * side of the
// ancestor's grid, the ancestor's own coordinates are L >> d   (the same cell, hence the same voxel, as voxel_of() finds for any sample in it)
__device__ __forceinline__ float4 voxel_from(const BuildArgs& a, uint32_t d, uint32_t code, uint32_t leafLevel, uint32_t LX, uint32_t LY, uint32_t LZ, float colorBits) {
	const uint32_t s = d - 1u, side = 128u >> d, m = (1u << d) - 1u;
	const uint32_t cx = (LX & m) * side + ((code & 63u) >> s), cy = (LY & m) * side + (((code >> 6) & 63u) >> s), cz = (LZ & m) * side + (((code >> 12) & 63u) >> s);
	return voxel_at(a, (int)(leafLevel - d), LX >> d, LY >> d, LZ >> d, cx, cy, cz, colorBits);
}
// LDS word w of the cubes -> which ancestor's grid word it mirrors: d (0: none), the word's index in that grid, the bit offset of the
// cube's row inside the word, and the row's mask
__device__ __forceinline__ uint32_t cube_word(uint32_t w, uint32_t LX, uint32_t LY, uint32_t LZ, uint32_t& gridWord, uint32_t& shift, uint32_t& mask) {
	const uint32_t d = w < 8192u ? 1u : w < 9216u ? 2u : w < 9472u ? 3u : w < 9536u ? 4u : w < 9552u ? 5u : w < 9556u ? 6u : w < 9557u ? 7u : 0u;
	if (d == 0u) { gridWord = 0; shift = 0; mask = 0; return 0u; }
	const uint32_t side = 128u >> d, ox = (LX & ((1u << d) - 1u)) * side, oy = (LY & ((1u << d) - 1u)) * side, oz = (LZ & ((1u << d) - 1u)) * side;
	const uint32_t rel = w - cube_offset(d), row = d == 1u ? rel >> 1 : rel, ly = row % side, lz = row / side;
	const uint32_t cell = ox + 128u * (oy + ly) + 16384u * (oz + lz);
	gridWord = (cell >> 5) + (d == 1u ? (rel & 1u) : 0u);
	shift = d <= 2u ? 0u : (cell & 31u);
	mask = side >= 32u ? 0xffffffffu : (1u << side) - 1u;
	return d;
}

// Leaves that received only a few samples (a batch that is NOT spatially compact — uniformly scattered points, a sparse overview
// scan — touches tens of thousands of leaves with a few dozen samples each): loading 38 KB of cubes per leaf would cost far more
// than the samples, and there is nothing to contend for.  One WAVE per leaf, the round-1 way: every sample probes its ancestors' grids
// bottom-up with plain loads and claims with atomicOr, four samples per lane in flight; the winners of one level of one leaf share
// the ancestor, so Node.numVoxels takes one add per (leaf, level, step).  The waves of k_voxelize's workgroups do this after their
// pieces.  (Measured: without this path the uniformly scattered
// 350 M-point replay of the C++ harness, 40 000 leaves touched per batch, took 408 ms of kernel time instead of 157 ms.)
__device__ __forceinline__ void voxelize_small(const BuildArgs& a, Ctl* ctl, BatchCtl* bc, const uint32_t wave, const uint32_t numWaves) {
	const uint32_t numSmall = min(bc->numVoxSmall, a.voxItemCap - VOX_BIG_ITEMS);
	if (numSmall == 0u) return;
	const VoxItem* items = vox_items(a, bc);
	SimlodChunk* const* chunkDir = chunk_dir(a, bc);
	const uint32_t tag = bc->tag;
	const uint32_t lane = (uint32_t)lane_id();
	constexpr uint32_t U = 4;                              // items a wave works on together when there are more items than waves: a scattered batch leaves ~25 samples in each of tens of thousands of leaves
	const uint32_t per = numSmall > numWaves / 4u ? U : 1u;          // (several items of a wave in flight once the items outnumber a quarter of the waves: config 5 has 8 192 items per batch for 8 192 waves of which half are resident — one item per wave took two rounds of ~80 us)
	for (uint32_t k0 = wave * per; k0 < numSmall; k0 += numWaves * per) {
		VoxItem it[U];
		unsigned long long mine[U];
		uint32_t itemIndex[U], count[U], depth[U];
		uint32_t maxCount = 0, maxDepth = 0;
#pragma unroll
		for (uint32_t u = 0; u < U; u++) {
			itemIndex[u] = VOX_BIG_ITEMS + min(k0 + u, numSmall - 1u);
			it[u] = items[itemIndex[u]];
		}
#pragma unroll
		for (uint32_t u = 0; u < U; u++) {
			const uint32_t leafIdx = it[u].leaf & 0xffffffu;
			count[u] = u < per && k0 + u < numSmall ? it[u].s1 - it[u].s0 : 0u;
			// the leaf's path, one entry per lane (entry d - 1 = ancestor d; a root that is still a leaf samples itself, voxels.cu:449-463)
			mine[u] = 0ull;
			if (leafIdx == 0u) { SimlodOccupancyGrid* g = a.nodes[0].grid; if (lane == 0u && g != nullptr) mine[u] = path_pack(a.pers, 0u, 0u, g); }
			else {
				const unsigned long long* paths = at<const unsigned long long>(a, a.offPaths);
				if (lane < PATH_ROW) mine[u] = paths[(uint64_t)leafIdx * PATH_ROW + lane];
				// (a leaf below level PATH_ROW: the entries its row continues in — the item says so, the same for the whole wave)
				if ((it[u].leaf >> 24) > PATH_ROW && lane >= PATH_ROW && lane < (it[u].leaf >> 24)) mine[u] = path_far(paths, leafIdx, lane, a.nodeCapacity);
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < U; u++) {
			const unsigned long long present = __ballot(mine[u] != 0ull);
			depth[u] = count[u] != 0u ? (uint32_t)__ffsll((long long)~present) - 1u : 0u;      // entries up to the terminator
			maxCount = max(maxCount, count[u]); maxDepth = max(maxDepth, depth[u]);
		}
		for (uint32_t base = 0; base < maxCount; base += 64u) {
			uint32_t pX[U], pY[U], pZ[U];
			float color[U];
			bool go[U];
			{
				float4 p[U];
#pragma unroll
				for (uint32_t u = 0; u < U; u++) {
					const uint32_t rel = base + lane, i = it[u].s0 + rel;
					go[u] = rel < count[u];
					p[u] = go[u] ? reinterpret_cast<const float4*>(chunkDir[it[u].ptBase + (i / SIMLOD_POINTS_PER_CHUNK - it[u].ptFirst)]->points)[i % SIMLOD_POINTS_PER_CHUNK] : make_float4(0, 0, 0, 0);
				}
#pragma unroll
				for (uint32_t u = 0; u < U; u++) {
					pX[u] = quantize(F_FULL, p[u].x, a.minx, a.size); pY[u] = quantize(F_FULL, p[u].y, a.miny, a.size); pZ[u] = quantize(F_FULL, p[u].z, a.minz, a.size);
					color[u] = p[u].w;
				}
			}
			for (uint32_t d = 1; d <= maxDepth; d++) {                                   // bottom-up, the whole wave one level at a time
				bool any = false;
#pragma unroll
				for (uint32_t u = 0; u < U; u++) { go[u] = go[u] && d <= depth[u]; any = any || go[u]; }
				if (__ballot(any) == 0ull) break;
				unsigned long long ent[U];
				uint32_t* word[U]; uint32_t bit[U], seen[U], level[U];
#pragma unroll
				for (uint32_t u = 0; u < U; u++) {
					ent[u] = ((unsigned long long)(uint32_t)__shfl((int)(mine[u] >> 32), (int)d - 1, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)mine[u], (int)d - 1, 64);
					level[u] = path_level(ent[u]);
					go[u] = go[u] && ent[u] != 0ull && level[u] < (uint32_t)SIMLOD_MAX_DEPTH;   // voxels.cu:449: levels 0..19 only
					const uint32_t cell = grid_cell(level[u], pX[u], pY[u], pZ[u]);
					word[u] = &path_grid(a.pers, ent[u])->values[cell >> 5]; bit[u] = cell & 31u;
					seen[u] = go[u] ? *word[u] : 0xffffffffu;
				}
#pragma unroll
				for (uint32_t u = 0; u < U; u++) { go[u] = go[u] && ((seen[u] >> bit[u]) & 1u) == 0u; seen[u] = go[u] ? atomicOr(word[u], 1u << bit[u]) : 0xffffffffu; }   // voxels.cu:93-96
#pragma unroll
				for (uint32_t u = 0; u < U; u++) {
					go[u] = go[u] && ((seen[u] >> bit[u]) & 1u) == 0u;                  // lost: the winner climbs on
					// the winners share the ancestor: one add per (leaf, level) reserves their slots in its voxel list (voxels.cu:101), and each stores
					// its voxel — the cell's centre in the sample's colour (voxels.cu:103-114, 674-698) — right away
					const unsigned long long wm = __ballot(go[u]);
					if (wm == 0ull) continue;
					const uint32_t node = path_node(ent[u]);
					uint32_t first = 0;
					if (lane == 0u) first = atomicAdd(&a.nodes[node].numVoxels, (uint32_t)__popcll(wm));
					first = (uint32_t)__shfl((int)first, 0, 64);
					store_voxels_wave(a, ctl, tag, go[u], node, first + (uint32_t)__popcll(wm & ((1ull << lane) - 1ull)), voxel_of(a, (int)level[u], pX[u], pY[u], pZ[u], color[u]));
				}
			}
		}
	}
}

// ---- end of batch: bookkeeping (voxels.cu:535-537, 925-949), then make the next batch current ------------------
// One thread of k_voxelize, the kernel behind the group's k_insert: the group's points are stored and its ring slots no longer read
// (nothing the rest of that launch reads is touched here: the kernels know their group by its parity copy).
__device__ void end_of_batch(const BuildArgs& a, Ctl* ctl, BatchCtl* bc) {
	if (ctl->abortBatch) __hip_atomic_store(&ctl->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // scratch overflow: this batch is lost, report through Stats.dbg
	else {
		a.stats->batchletIndex += bc->groupBatches;
		a.stats->numPointsProcessed += bc->batchSize;
		ctl->processed += 1;
		ctl->expandNs[7] += min(bc->numSpilled, a.spilledCap);   // measurement aid: stored points moved by splits so far (bench.py)
		ctl->expandNs[4] += 1;                                   // ... and groups of batches ingested so far: the launches of a per-group kernel that had work (bench.py's roofline)
		// voxels.cu:936-949: no further batch once the launch has run for 10 ms.  The front half of the next batch (or two) may be under way
		// already; what has been prepared is completed, nothing more is prepared.
		// (a chained launch: 10 ms per SEGMENT, from this group's own copy of its segment's start — the front half may have begun the next segment)
		const float elapsedMs = (float)(wall_ns() - ctl->segStart[bc->ordinal]) / 1000000.0f;
		if (elapsedMs > (float)ctl->budgetUs / 1000.0f) __hip_atomic_store(&ctl->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// On the library's side stream, while the next batch is already counted and split on the caller's.  A root that is still a leaf (the whole
// octree holds fewer than 50 000 points) is sampled here like every other leaf — into its own grid: the next batch may split that root, but
// the grid is cleared by that batch's k_insert (voxels.cu:371-382), which waits for this kernel.  No other grid is touched by both: a leaf
// that k_expand splits gets a NEW grid, and nothing samples into a leaf's own grid.
static constexpr uint32_t VOXROOT_WGS = 8;         // the last workgroups of k_voxelize's grid: the pieces of a root that is still a leaf (voxroot_pieces)
__device__ __forceinline__ void voxroot_pieces(const BuildArgs& a, Ctl* ctl, BatchCtl* bc, VoxShared& sh, uint32_t wg, uint32_t numWgs);

__global__ __launch_bounds__(VTPB) void k_voxelize(BuildArgs a, uint32_t ordinal) {
	Ctl* ctl = ctl_of(a);
	BatchCtl* bc = batch_of(ctl, ordinal);
	if (bc == nullptr || ctl->abortBatch) return;
	__shared__ VoxShared sh;
	const uint32_t numWgs = gridDim.x - VOXROOT_WGS;          // (the host launches VOXROOT_WGS more than it has pieces for)
	if (blockIdx.x >= numWgs) {
		if (bc->rootPieces != 0u) voxroot_pieces(a, ctl, bc, sh, blockIdx.x - numWgs, VOXROOT_WGS);
		return;
	}
	// the group's points are stored (k_insert has ended: nobody reads its ring slots any more): voxels.cu:925-949
	if (blockIdx.x == 0 && threadIdx.x == 0) end_of_batch(a, ctl, bc);
	const uint32_t numItems = min(bc->numVoxItems, VOX_BIG_ITEMS);
	const VoxItem* items = vox_items(a, bc);
	SimlodChunk* const* chunkDir = chunk_dir(a, bc);
	const uint32_t tag = bc->tag;
	static_assert(VTPB == 1024 && CUBE_WORDS <= 9216 + VTPB, "k_voxelize: thread t owns the LDS cube words t + 1024 k (k < 8: cube 1), 8192 + t (cube 2), 9216 + t (cubes 3..7)");
	const uint32_t lane = (uint32_t)lane_id();
	Phase ph(ctl, blockIdx.x == ((ctl->debugFlags >> 8) & 0xffffu));     // (SIMLOD_DEBUG_PHASE_WG: whose phase times tools/probe.py prints; default workgroup 0)
	const bool clocked = SIMLOD_MEASURE != 0 && (ctl->debugFlags & 2u) != 0u;       // SIMLOD_DEBUG_VOXELIZE_CLOCK (tools/probe.py): when the first workgroup came, the last piece was done, the last workgroup left
	if (clocked && blockIdx.x == 0 && threadIdx.x == 0) ctl->voxT[ordinal][0] = wall_ns();
	for (uint32_t item = blockIdx.x; item < numItems; item += numWgs) {
		// Global memory is touched in six steps, each one round trip with everything it needs in flight together: the item; the leaf's
		// path; chunk addresses + cube words; the samples; the write-back atomics; the slot reservations and voxel chunks.
		VoxItem it = items[item];
		const uint32_t leafLevel = it.leaf >> 24;
		it.leaf &= 0xffffffu;
		if (it.leaf == 0u) continue;                              // (the root as a leaf: voxroot_pieces)
		const uint32_t LX = a.nodes[it.leaf].X, LY = a.nodes[it.leaf].Y, LZ = a.nodes[it.leaf].Z;      // (in flight beside the leaf's path)
		const unsigned long long* rec = at<const unsigned long long>(a, a.offPaths) + (uint64_t)it.leaf * PATH_ROW;
		__syncthreads();                                       // the previous item's LDS state is no longer read
		if (threadIdx.x < PATH_WORDS) {
			// ancestor d (1 = parent) is anc[d - 1].  (A root that is still a leaf samples ITSELF, voxels.cu:449-463 — the whole octree holds fewer
			// than 50 000 points —: voxroot_pieces, skipped here.)  A leaf below level PATH_ROW finds the ancestors beyond its row through path_far:
			// the item knows the level, so every other leaf takes no branch that depends on a load.
			unsigned long long e = threadIdx.x < PATH_ROW ? rec[threadIdx.x] : 0ull;
			if (leafLevel > PATH_ROW && threadIdx.x >= PATH_ROW && threadIdx.x < leafLevel) e = path_far(at<const unsigned long long>(a, a.offPaths), it.leaf, threadIdx.x, a.nodeCapacity);
			sh.anc[threadIdx.x] = e; sh.cnt[threadIdx.x] = 0; sh.hiOcc[threadIdx.x] = 0; sh.hiFresh[threadIdx.x] = 0; sh.rank[threadIdx.x] = 0;
			if (threadIdx.x < 8u) sh.listCount[threadIdx.x] = 0;
		}
		const SimlodChunk* chunk[VOX_SPT];
		bool live[VOX_SPT];
#pragma unroll
		for (uint32_t j = 0; j < VOX_SPT; j++) {
			const uint32_t i = it.s0 + j * VTPB + threadIdx.x;
			live[j] = i < it.s1;
			chunk[j] = live[j] ? chunkDir[it.ptBase + (i / SIMLOD_POINTS_PER_CHUNK - it.ptFirst)] : nullptr;
		}
		__syncthreads();
		ph.mark(24);
		uint32_t depth = 0;
		while (depth < PATH_WORDS - 1 && sh.anc[depth] != 0ull) depth++;
		// voxels.cu:449: the traverse loop samples levels 0..19 only — an ancestor is at level 19 at most (leaves are at most at 20)
		const uint32_t ldsDepth = min(depth, LDS_LEVELS);

		// the leaf's cubes, as the grids hold them now (each thread keeps what it loaded: the write-back needs it); the single cells of the
		// ancestors above; the samples
		// LDS word w of the cubes belongs to thread w % 1024: eight words of cube 1 (the parent's grid: words g1 + k * 4096 — the 64 x-bits of one
		// (y, z) row are a pair of words —), one of cube 2 (the grandparent's: g2), and for w >= 9216 one of the small cubes 3..7 (cube_word).
		// (Round 4 ran the general cube_word() for all ten words, twice, and kept its results: 128 VGPRs and 40 bytes of scratch per lane.)
		const uint32_t g1 = ((((LX & 1u) * 64u) + 128u * ((LY & 1u) * 64u) + 16384u * ((LZ & 1u) * 64u)) >> 5) + ((threadIdx.x >> 1) & 63u) * 4u + (threadIdx.x >> 7) * 512u + (threadIdx.x & 1u);
		const uint32_t g2 = (((LX & 3u) * 32u) + 128u * ((LY & 3u) * 32u + (threadIdx.x & 31u)) + 16384u * ((LZ & 3u) * 32u + (threadIdx.x >> 5))) >> 5;
		const uint32_t w3 = 9216u + threadIdx.x;
		uint32_t gw3, sft3, msk3;
		const uint32_t d3 = cube_word(w3, LX, LY, LZ, gw3, sft3, msk3);
		const bool have3 = d3 != 0u && d3 <= ldsDepth;
		uint32_t* const grid1 = ldsDepth >= 1u ? path_grid(a.pers, sh.anc[0])->values : nullptr;
		uint32_t* const grid2 = ldsDepth >= 2u ? path_grid(a.pers, sh.anc[1])->values : nullptr;
		uint32_t* const grid3 = have3 ? path_grid(a.pers, sh.anc[d3 - 1u])->values : nullptr;
		uint32_t snap1[8], snap2, snap3;
		{
#pragma unroll
			for (uint32_t k = 0; k < 8; k++) snap1[k] = ldsDepth >= 1u ? grid1[g1 + k * 4096u] : 0u;
			snap2 = ldsDepth >= 2u ? grid2[g2] : 0u;
			snap3 = have3 ? grid3[gw3] : 0u;
			uint32_t hi = 0;
			const bool hiMine = threadIdx.x >= LDS_LEVELS && threadIdx.x < depth;   // d = threadIdx.x + 1 >= 8: every sample of the leaf has the same cell
			if (hiMine) {
				const unsigned long long ent = sh.anc[threadIdx.x];
				const uint32_t d = threadIdx.x + 1u, level = path_level(ent);
				// the leaf's own corner stands for all its samples: 2^(28 - leafLevel) fine units per leaf, leafLevel = level + d
				const uint32_t s2 = 28u - (level + d), cell = grid_cell(level, LX << s2, LY << s2, LZ << s2);
				hi = (path_grid(a.pers, ent)->values[cell >> 5] >> (cell & 31u)) & 1u;
			}
			float4 p[VOX_SPT];
#pragma unroll
			for (uint32_t j = 0; j < VOX_SPT; j++)
				p[j] = live[j] ? reinterpret_cast<const float4*>(chunk[j]->points)[(it.s0 + j * VTPB + threadIdx.x) % SIMLOD_POINTS_PER_CHUNK] : make_float4(0, 0, 0, 0);
			snap3 = have3 ? (snap3 >> sft3) & msk3 : 0u;
#pragma unroll
			for (uint32_t k = 0; k < 8; k++) sh.occ[k * VTPB + threadIdx.x] = snap1[k];
			sh.occ[8192u + threadIdx.x] = snap2;
			if (w3 < CUBE_WORDS) sh.occ[w3] = snap3;
			if (hiMine) sh.hiOcc[threadIdx.x] = hi;
			__syncthreads();
			ph.mark(25);

			// level 1: every sample, from registers.  Its cell inside the leaf's cube of the parent's grid: six bits per axis below the leaf's
			// own bits (the parent's grid cell is coordinate >> (21 - parentLevel), voxels.cu:78-92)
			{
				const uint32_t shf = (uint32_t)(SIMLOD_MAX_DEPTH + 2) - leafLevel;
				uint32_t code[VOX_SPT], word[VOX_SPT], bit[VOX_SPT], old[VOX_SPT];
#pragma unroll
				for (uint32_t j = 0; j < VOX_SPT; j++) {
					const uint32_t pX = quantize(F_FULL, p[j].x, a.minx, a.size), pY = quantize(F_FULL, p[j].y, a.miny, a.size), pZ = quantize(F_FULL, p[j].z, a.minz, a.size);
					code[j] = ((pX >> shf) & 63u) | (((pY >> shf) & 63u) << 6) | (((pZ >> shf) & 63u) << 12);
					sh.color[j * VTPB + threadIdx.x] = p[j].w;
					cube_cell_from(1u, code[j], word[j], bit[j]);
					old[j] = live[j] ? sh.occ[word[j]] : 0xffffffffu;
				}
#pragma unroll
				for (uint32_t j = 0; j < VOX_SPT; j++) if (((old[j] >> bit[j]) & 1u) == 0u) old[j] = atomicOr(&sh.occ[word[j]], 1u << bit[j]);   // voxels.cu:93-96
				// the thread's winners go on the list (the losers' cells had been set: their climb ends here): one reservation per wave
				uint32_t wins = 0;
#pragma unroll
				for (uint32_t j = 0; j < VOX_SPT; j++) if (((old[j] >> bit[j]) & 1u) == 0u) wins |= 1u << j;
				uint32_t total;
				const uint32_t before = wave_exclusive((uint32_t)__popc(wins), total);
				uint32_t base = 0;
				if (lane == 0u && total != 0u) base = atomicAdd(&sh.listCount[1], total);
				base = (uint32_t)__shfl((int)base, 0, 64) + before;
#pragma unroll
				for (uint32_t j = 0; j < VOX_SPT; j++) if (((wins >> j) & 1u) != 0u) sh.list[base++] = code[j] | ((j * VTPB + threadIdx.x) << 18);
			}
		}
		__syncthreads();
		ph.mark(26);
		// levels 2 .. 7: the winners of level 1, a list entry per lane, climb on INSIDE their wave — no workgroup barrier per level (six of them
		// cost more than the climbing): a wave takes four entries per lane, tests and sets their cells level by level while any of them still
		// finds its cell clear, and appends each level's winners to that level's list (one reservation per wave and level).  Waves never need
		// each other: the cubes of different levels are different words, and a cell has ONE winner whoever gets there first.
		{
			const uint32_t n1 = sh.listCount[1];
			const uint32_t* src = sh.list + list_offset(1u);
			for (uint32_t i0 = 0; i0 < n1 && ldsDepth >= 2u; i0 += 4u * VTPB) {
				uint32_t e[4];
				bool go[4];
#pragma unroll
				for (uint32_t q = 0; q < 4; q++) { const uint32_t i = i0 + q * VTPB + threadIdx.x; go[q] = i < n1; e[q] = go[q] ? src[i] : 0u; }
				for (uint32_t d = 2; d <= ldsDepth; d++) {
					if (__ballot(go[0] || go[1] || go[2] || go[3]) == 0ull) break;      // (wave-uniform)
					uint32_t* dst = sh.list + list_offset(d);
					uint32_t word[4], bit[4], old[4];
#pragma unroll
					for (uint32_t q = 0; q < 4; q++) { cube_cell_from(d, e[q] & 0x3ffffu, word[q], bit[q]); old[q] = go[q] ? sh.occ[word[q]] : 0xffffffffu; }
#pragma unroll
					for (uint32_t q = 0; q < 4; q++) if (((old[q] >> bit[q]) & 1u) == 0u) old[q] = atomicOr(&sh.occ[word[q]], 1u << bit[q]);
#pragma unroll
					for (uint32_t q = 0; q < 4; q++) {
						go[q] = ((old[q] >> bit[q]) & 1u) == 0u;                    // lost: the winner climbs on
						const unsigned long long wm = __ballot(go[q]);
						if (wm != 0ull) {
							uint32_t base = 0;
							if (lane == 0u) base = atomicAdd(&sh.listCount[d], (uint32_t)__popcll(wm));
							base = (uint32_t)__shfl((int)base, 0, 64);
							if (go[q]) dst[base + (uint32_t)__popcll(wm & ((1ull << lane) - 1ull))] = e[q];
						}
					}
				}
			}
			__syncthreads();
		}
		// from the 8th ancestor on the whole leaf is one cell: the winner of the 7th cube (there is at most one) climbs alone
		if (threadIdx.x == 0u && depth > LDS_LEVELS && sh.listCount[LDS_LEVELS] != 0u) {
			sh.hiSample = sh.list[list_offset(LDS_LEVELS)] >> 18;
			for (uint32_t d = LDS_LEVELS + 1u; d <= depth; d++) {
				if (sh.hiOcc[d - 1u] != 0u) break;
				sh.hiOcc[d - 1u] = 1u; sh.hiFresh[d - 1u] = 1u;
			}
		}
		__syncthreads();
		ph.mark(27);

		// write-back: the grids learn the new cells and tell which of them are new for everybody (pieces of one leaf share the cubes):
		// every thread's atomics are in flight together.  What this piece set in a word = the word now minus the word as it was loaded.
		{
			uint32_t f1[8], old1[8], f2, old2 = 0, f3, old3 = 0;
#pragma unroll
			for (uint32_t k = 0; k < 8; k++) {
				f1[k] = sh.occ[k * VTPB + threadIdx.x] & ~snap1[k];
				old1[k] = f1[k] != 0u ? atomicOr(&grid1[g1 + k * 4096u], f1[k]) : 0u;                                  // voxels.cu:96
			}
			f2 = sh.occ[8192u + threadIdx.x] & ~snap2;
			if (f2 != 0u) old2 = atomicOr(&grid2[g2], f2);
			f3 = w3 < CUBE_WORDS ? sh.occ[w3] & ~snap3 : 0u;
			if (f3 != 0u) old3 = atomicOr(&grid3[gw3], f3 << sft3);
			uint32_t won1 = 0;
#pragma unroll
			for (uint32_t k = 0; k < 8; k++) {
				const uint32_t won = f1[k] & ~old1[k];
				sh.occ[k * VTPB + threadIdx.x] = won;                               // from here on: the cells this piece won
				won1 += (uint32_t)__popc(won);
			}
			if (won1 != 0u) atomicAdd(&sh.cnt[1], won1);
			{ const uint32_t won = f2 & ~old2; sh.occ[8192u + threadIdx.x] = won; if (won != 0u) atomicAdd(&sh.cnt[2], (uint32_t)__popc(won)); }
			if (w3 < CUBE_WORDS) { const uint32_t won = f3 & ~(old3 >> sft3); sh.occ[w3] = won; if (won != 0u) atomicAdd(&sh.cnt[d3], (uint32_t)__popc(won)); }
			const bool hiMine = threadIdx.x >= LDS_LEVELS && threadIdx.x < depth;
			if (hiMine && sh.hiFresh[threadIdx.x] != 0u) {
				const unsigned long long ent = sh.anc[threadIdx.x];
				const uint32_t d = threadIdx.x + 1u, level = path_level(ent), s2 = 28u - (level + d), cell = grid_cell(level, LX << s2, LY << s2, LZ << s2);
				const uint32_t o = atomicOr(&path_grid(a.pers, ent)->values[cell >> 5], 1u << (cell & 31u));
				const uint32_t won = ((o >> (cell & 31u)) & 1u) ^ 1u;
				sh.hiFresh[threadIdx.x] = won;
				sh.cnt[d] = won;
			}
		}
		__syncthreads();
		ph.mark(28);
		// The cells this piece won in ancestor d become voxels: the add to Node.numVoxels (voxels.cu:101) reserves their slots in d's voxel
		// list, and the chunks those slots lie in are made or found here (see "voxel chunks, on demand") — one lane per ancestor, all in
		// wave 0: first every lane allocates and publishes what it owns, then every lane links / looks up (which may wait for another piece).
		{
			const uint32_t d = threadIdx.x;
			const bool mineD = d >= 1u && d <= depth && sh.cnt[d] != 0u;
			uint32_t node = 0, first = 0, existing = 0, kFirst = 0, ownFirst = 0, own = 0;
			SimlodChunk* mem = nullptr;
			if (mineD) {
				node = path_node(sh.anc[d - 1u]);
				const uint32_t cnt = sh.cnt[d];
				first = atomicAdd(&a.nodes[node].numVoxels, cnt);
				existing = (a.nodes[node].numVoxelsStored + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
				kFirst = first / SIMLOD_POINTS_PER_CHUNK;
				const uint32_t kLast = (first + cnt - 1u) / SIMLOD_POINTS_PER_CHUNK;
				ownFirst = first % SIMLOD_POINTS_PER_CHUNK == 0u ? kFirst : kFirst + 1u;           // chunk k is this piece's to make when it holds slot k * 1000
				own = kLast + 1u > ownFirst ? kLast + 1u - ownFirst : 0u;
				if (own != 0u) mem = reinterpret_cast<SimlodChunk*>(persistent_alloc(a.pers, sizeof(SimlodChunk), own));   // voxel chunks never come from the pool (voxels.cu:656-659)
				for (uint32_t q = 0; q < own; q++) {
					SimlodChunk* c = reinterpret_cast<SimlodChunk*>(reinterpret_cast<uint8_t*>(mem) + (uint64_t)q * SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk)));
					if (q + 1u < own) c->next = reinterpret_cast<SimlodChunk*>(reinterpret_cast<uint8_t*>(c) + SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk)));   // (the last one's: vox_chunk_link)
					vox_chunk_publish(a, ctl, tag, node, ownFirst + q, c);
					sh.chunkOf[d][ownFirst + q - kFirst] = c;
				}
				sh.first[d] = first;
			}
			if (mineD) {
				SimlodChunk* oldTail = existing > 0u ? tail_of(a.nodes[node].voxelChunks) : nullptr;
				if (own != 0u) vox_chunk_link(a, ctl, tag, node, ownFirst, existing, oldTail, mem);
				if (ownFirst != kFirst) sh.chunkOf[d][0] = kFirst < existing ? oldTail : dir_wait(a, ctl, tag, node, kFirst);
			}
		}
		__syncthreads();
		ph.mark(29);

		// store: every winner whose cell is still marked won (nobody else had it) becomes a voxel — the cell's centre in the winner's colour
		// (voxels.cu:103-114, 674-698) — in the next free slot of the piece's range in that ancestor's list.  Level 1: the thread's own samples;
		// levels 2..7: the lists, an entry per lane; beyond: the one sample that climbed alone.
		auto store = [&](uint32_t d, const float4& vox) {
			const uint32_t slot = sh.first[d] + atomicAdd(&sh.rank[d], 1u);
			SimlodChunk* c = sh.chunkOf[d][slot / SIMLOD_POINTS_PER_CHUNK - sh.first[d] / SIMLOD_POINTS_PER_CHUNK];
			if (c != nullptr) reinterpret_cast<float4*>(c->points)[slot % SIMLOD_POINTS_PER_CHUNK] = vox;
		};
		for (uint32_t d = 1; d <= ldsDepth; d++) {
			const uint32_t n = sh.listCount[d];
			const uint32_t* src = sh.list + list_offset(d);
			for (uint32_t i = threadIdx.x; i < n; i += VTPB) {
				const uint32_t e = src[i];
				uint32_t word, bit;
				cube_cell_from(d, e & 0x3ffffu, word, bit);
				if (((sh.occ[word] >> bit) & 1u) != 0u) store(d, voxel_from(a, d, e & 0x3ffffu, leafLevel, LX, LY, LZ, sh.color[e >> 18]));
			}
		}
		if (threadIdx.x >= LDS_LEVELS && threadIdx.x < depth && sh.hiFresh[threadIdx.x] != 0u) {
			const uint32_t d = threadIdx.x + 1u, level = leafLevel - d, s2 = 28u - leafLevel;
			store(d, voxel_of(a, (int)level, LX << s2, LY << s2, LZ << s2, sh.color[sh.hiSample]));
		}
		ph.mark(30);
		if (ph.on) ctl->phaseNs[31] += 1;
	}
	if (clocked && threadIdx.x == 0 && blockIdx.x < numItems) atomicMax(reinterpret_cast<unsigned long long*>(&ctl->voxT[ordinal][1]), (unsigned long long)wall_ns());
	// then, wave by wave, the leaves with few new samples — handed out from the LAST wave down: the workgroups that had no piece start at once
	voxelize_small(a, ctl, bc, numWgs * VTPB / 64u - 1u - (blockIdx.x * VTPB + threadIdx.x) / 64u, numWgs * VTPB / 64u);
	if (clocked) { __syncthreads(); if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long*>(&ctl->voxT[ordinal][2]), (unsigned long long)wall_ns()); }
}

// ---- voxroot: a root that is still a leaf (the whole octree holds fewer than 50 000 points) samples ITSELF (voxels.cu:449-463: every node of the
// path that has a grid is sampled, and the root has one from the reset on) — into its own grid, sample by sample with device-scope atomics: the
// first batch or two of an octree, at most seven pieces.  The LAST workgroups of k_voxelize's launch (a path of its own, not a case of the main
// path: that cost the main path scratch memory; as a kernel of its own behind k_voxelize it cost every batch a launch); they leave at once when
// the group has no such piece.  Uses entry 0 of the piece state (cnt, first, rank, chunkOf).
__device__ __forceinline__ void voxroot_pieces(const BuildArgs& a, Ctl* ctl, BatchCtl* bc, VoxShared& sh, uint32_t wg, uint32_t numWgs) {
	const uint32_t numItems = min(bc->numVoxItems, VOX_BIG_ITEMS);
	const VoxItem* items = vox_items(a, bc);
	SimlodChunk* const* chunkDir = chunk_dir(a, bc);
	const uint32_t tag = bc->tag;
	for (uint32_t item = wg; item < numItems; item += numWgs) {
		VoxItem it = items[item];
		it.leaf &= 0xffffffu;
		if (it.leaf != 0u) continue;
		__syncthreads();
		if (threadIdx.x == 0u) { sh.cnt[0] = 0; sh.rank[0] = 0; }
		__syncthreads();
		SimlodOccupancyGrid* const g = a.nodes[0].grid;
		const unsigned long long ent = g != nullptr ? path_pack(a.pers, 0u, 0u, g) : 0ull;
		// a root that is still a leaf (fewer than 50 000 points in the whole octree): its own grid, sample by sample, one after the other
		// (this path runs for the first batch of an octree at most: nothing here is worth a register of the main path); the winners
		// share ONE voxel list (the root's): one reservation for the whole piece
		auto sample = [&](uint32_t j, uint32_t& pX, uint32_t& pY, uint32_t& pZ) -> float {
			const uint32_t i = it.s0 + j * VTPB + threadIdx.x;
			const float4 q = reinterpret_cast<const float4*>(chunkDir[it.ptBase + (i / SIMLOD_POINTS_PER_CHUNK - it.ptFirst)]->points)[i % SIMLOD_POINTS_PER_CHUNK];
			pX = quantize(F_FULL, q.x, a.minx, a.size); pY = quantize(F_FULL, q.y, a.miny, a.size); pZ = quantize(F_FULL, q.z, a.minz, a.size);
			return q.w;
		};
		uint32_t wonMask = 0;
		if (ent != 0ull) {
#pragma unroll 1
			for (uint32_t j = 0; j < VOX_SPT; j++) {
				if (it.s0 + j * VTPB + threadIdx.x >= it.s1) continue;
				uint32_t pX, pY, pZ;
				(void)sample(j, pX, pY, pZ);
				const uint32_t cell = grid_cell(0u, pX, pY, pZ), bit = cell & 31u;
				uint32_t* word = &path_grid(a.pers, ent)->values[cell >> 5];
				if (((*word >> bit) & 1u) != 0u) continue;                                         // voxels.cu:93-94
				if (((atomicOr(word, 1u << bit) >> bit) & 1u) != 0u) continue;                     // voxels.cu:96
				wonMask |= 1u << j;
				atomicAdd(&sh.cnt[0], 1u);
			}
		}
		__syncthreads();
		if (threadIdx.x == 0u && sh.cnt[0] != 0u) {
			const uint32_t cnt = sh.cnt[0];
			const uint32_t first = atomicAdd(&a.nodes[0].numVoxels, cnt);
			const uint32_t existing = (a.nodes[0].numVoxelsStored + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
			const uint32_t kFirst = first / SIMLOD_POINTS_PER_CHUNK, kLast = (first + cnt - 1u) / SIMLOD_POINTS_PER_CHUNK;
			const uint32_t ownFirst = first % SIMLOD_POINTS_PER_CHUNK == 0u ? kFirst : kFirst + 1u;
			const uint32_t own = kLast + 1u > ownFirst ? kLast + 1u - ownFirst : 0u;
			SimlodChunk* mem = own != 0u ? reinterpret_cast<SimlodChunk*>(persistent_alloc(a.pers, sizeof(SimlodChunk), own)) : nullptr;
			for (uint32_t q = 0; q < own; q++) {
				SimlodChunk* c = reinterpret_cast<SimlodChunk*>(reinterpret_cast<uint8_t*>(mem) + (uint64_t)q * SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk)));
				if (q + 1u < own) c->next = reinterpret_cast<SimlodChunk*>(reinterpret_cast<uint8_t*>(c) + SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk)));
				vox_chunk_publish(a, ctl, tag, 0u, ownFirst + q, c);
				sh.chunkOf[0][ownFirst + q - kFirst] = c;
			}
			SimlodChunk* oldTail = existing > 0u ? tail_of(a.nodes[0].voxelChunks) : nullptr;
			if (own != 0u) vox_chunk_link(a, ctl, tag, 0u, ownFirst, existing, oldTail, mem);
			if (ownFirst != kFirst) sh.chunkOf[0][0] = kFirst < existing ? oldTail : dir_wait(a, ctl, tag, 0u, kFirst);
			sh.first[0] = first;
		}
		__syncthreads();
#pragma unroll 1
		for (uint32_t j = 0; j < VOX_SPT; j++) {
			if (((wonMask >> j) & 1u) == 0u) continue;
			uint32_t pX, pY, pZ;
			const float colour = sample(j, pX, pY, pZ);
			const uint32_t slot = sh.first[0] + atomicAdd(&sh.rank[0], 1u);
			SimlodChunk* c = sh.chunkOf[0][slot / SIMLOD_POINTS_PER_CHUNK - sh.first[0] / SIMLOD_POINTS_PER_CHUNK];
			if (c != nullptr) reinterpret_cast<float4*>(c->points)[slot % SIMLOD_POINTS_PER_CHUNK] = voxel_of(a, 0, pX, pY, pZ, colour);
		}
	}
}
