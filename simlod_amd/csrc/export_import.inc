// export_import.inc — part of export.hip: the import.  ImportArgs, octant_of, link_chunk_list, k_i_validate, k_i_nodes, k_i_finish.
// ---- import -------------------------------------------------------------------------------------------------------------------------
struct ImportArgs {
	const SimlodExportNode* table;
	uint32_t                n;
	const SimlodPoint*      samples;
	uint64_t                numSamples;
	uint8_t*                scratch;
	Layout                  lay;
	uint8_t*                pers;
	uint64_t                persCap;
	SimlodNode*             nodes;
	SimlodStats*            stats;
	// the buildable import (launch_import_buildable): the box as the builder derives it (construct.hip), and what k_reset also writes
	uint32_t                buildable;
	float                   minx, miny, minz, size;
	uint32_t*               numBatchesUploaded;
	uint32_t*               batchSizes;
	uint32_t*               feedback;
	uint32_t                feedbackSeq, frameCounter;
};

__device__ __forceinline__ uint32_t octant_of(const SimlodExportNode& e) { return ((e.X & 1u) << 2) | ((e.Y & 1u) << 1) | (e.Z & 1u); }

// Chunk k of a list of nch consecutive chunks from byte `base` of the persistent buffer, linked: `next` as the builder leaves it (the last
// one NULL), the head's size / padding_0 the tail's address (construct_begin.inc tail_of), the other chunks' 0.
__device__ __forceinline__ SimlodChunk* link_chunk_list(uint8_t* pers, uint64_t base, uint32_t first, uint32_t nch, uint32_t k) {
	SimlodChunk* c = reinterpret_cast<SimlodChunk*>(pers + base + (uint64_t)(first + k) * CHUNK_STRIDE);
	c->next = k + 1u < nch ? reinterpret_cast<SimlodChunk*>(reinterpret_cast<uint8_t*>(c) + CHUNK_STRIDE) : nullptr;
	*reinterpret_cast<uint64_t*>(&c->size) = k == 0u ? reinterpret_cast<uint64_t>(pers + base + (uint64_t)(first + nch - 1u) * CHUNK_STRIDE) : 0ull;
	return c;
}
__global__ __launch_bounds__(WG_TPB) void k_i_validate(ImportArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ uint32_t sh_bad;
	__shared__ uint32_t sh_cnt[7];
	__shared__ uint32_t sh_lvFirst[SIMLOD_MAX_DEPTH], sh_lvEnd[SIMLOD_MAX_DEPTH];
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(a.scratch + a.lay.first);
	uint32_t* gridOf = reinterpret_cast<uint32_t*>(a.scratch + a.lay.map);     // buildable: table index -> grid ordinal (NONE: a leaf below the root)
	if (threadIdx.x < 7) sh_cnt[threadIdx.x] = 0u;
	if (threadIdx.x < (uint32_t)SIMLOD_MAX_DEPTH) { sh_lvFirst[threadIdx.x] = NONE; sh_lvEnd[threadIdx.x] = 0u; }
	if (threadIdx.x == 0) sh_bad = 0u;
	__syncthreads();
	uint64_t samples = 0, chunks = 0, children = 1, grids = 0;        // (the root is nobody's child)
	for (uint32_t base = 0; base < a.n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		const bool act = t < a.n;
		SimlodExportNode e{};
		bool bad = false;
		if (act) {
			e = a.table[t];
			bad |= e.level > (uint32_t)SIMLOD_MAX_DEPTH || e.reserved != 0 || (e.flags & ~(SIMLOD_EXPORT_FLAG_LEAF | SIMLOD_EXPORT_FLAG_SELECTED)) != 0;
			if (t == 0u) bad |= e.parent != NONE || e.level != 0u || e.X != 0u || e.Y != 0u || e.Z != 0u;
			else if (e.parent >= t) bad = true;
			else {
				// level and coordinates follow from the parent, and the parent lists this entry where its octant says
				const SimlodExportNode p = a.table[e.parent];
				const uint32_t k = octant_of(e);
				bad |= e.level != p.level + 1u || (e.X >> 1) != p.X || (e.Y >> 1) != p.Y || (e.Z >> 1) != p.Z;
				bad |= !(p.childMask & (1u << k)) || p.firstChild == NONE || t != p.firstChild + (uint32_t)__popc(p.childMask & ((1u << k) - 1u));
			}
			if (e.childMask == 0u) bad |= e.firstChild != NONE;
			else bad |= e.firstChild == NONE || e.firstChild <= t || (uint64_t)e.firstChild + (uint32_t)__popc(e.childMask) > a.n || e.level >= (uint32_t)SIMLOD_MAX_DEPTH;
			if (a.buildable) {
				// a full export of an octree the builder made: every sample present, the leaf flag as the children say, eight children or none
				bad |= (e.flags & SIMLOD_EXPORT_FLAG_SELECTED) == 0u || ((e.flags & SIMLOD_EXPORT_FLAG_LEAF) != 0u) != (e.childMask == 0u);
				bad |= e.childMask != 0u && e.childMask != 0xffu;
				if (e.level < (uint32_t)SIMLOD_MAX_DEPTH) { atomicMin(&sh_lvFirst[e.level], t); atomicMax(&sh_lvEnd[e.level], t + 1u); }
			}
		}
		const uint64_t kids = (uint64_t)__popc(e.childMask), ns = act ? e.numSamples : 0u, nch = act ? ceil_chunks(ns) : 0u;
		const bool hasGrid = act && a.buildable != 0u && (t == 0u || e.childMask != 0u);
		uint64_t totK, totS, totC, totG;
		const uint64_t offK = block_scan<uint64_t>(kids, totK, sh_scan);
		const uint64_t offS = block_scan<uint64_t>(ns, totS, sh_scan);
		const uint64_t offC = block_scan<uint64_t>(nch, totC, sh_scan);
		const uint64_t offG = block_scan<uint64_t>(hasGrid ? 1u : 0u, totG, sh_scan);
		if (act && a.buildable) gridOf[t] = hasGrid ? (uint32_t)(grids + offG) : NONE;
		if (act) {
			// breadth-first order: an entry's children come right after the children of the entries before it
			if (e.childMask != 0u) bad |= (uint64_t)e.firstChild != children + offK;
			bad |= e.firstSample != samples + offS;
			if (samples + offS + ns <= a.numSamples && chunks + offC < a.lay.itemCap) first[t] = (uint32_t)(chunks + offC);
			const bool leaf = e.childMask == 0u;
			const uint32_t c[7] = {leaf ? 0u : 1u, leaf ? 1u : 0u, leaf && ns > 0u ? 1u : 0u, leaf ? (uint32_t)ns : 0u, leaf ? 0u : (uint32_t)ns,
			                       leaf ? (uint32_t)nch : 0u, leaf ? 0u : (uint32_t)nch};
			for (int q = 0; q < 7; q++) if (c[q] != 0u) atomicAdd(&sh_cnt[q], c[q]);
		}
		if (bad) atomicOr(&sh_bad, 1u);
		children += totK; samples += totS; chunks += totC; grids += totG;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		bool bad = sh_bad != 0u || a.n == 0u || children != a.n || samples != a.numSamples || chunks > a.lay.itemCap;
		// persistent layout: the chunks, then (buildable) the grids, then the voxel list of a root that is still a leaf (<= one voxel per point)
		uint64_t end = CHUNK_BASE + chunks * CHUNK_STRIDE;
		hdr->gridBase = end;
		if (a.buildable) {
			end += grids * GRID_STRIDE;
			hdr->rootVoxBase = end;
			if (a.n != 0u && a.table[0].childMask == 0u) end += (uint64_t)ceil_chunks(a.table[0].numSamples) * CHUNK_STRIDE;
		}
		bad |= end > a.persCap;
		hdr->ok = bad ? 0u : 1u;
		hdr->numItems = bad ? 0u : chunks;
		hdr->totalChunks = chunks;
		hdr->numGrids = (uint32_t)grids; hdr->gridBad = 0u; hdr->rootVoxels = 0u;
		for (int l = 0; l < SIMLOD_MAX_DEPTH; l++) { hdr->lvFirst[l] = sh_lvFirst[l]; hdr->lvEnd[l] = sh_lvEnd[l]; }
		for (int q = 0; q < 7; q++) hdr->counts[q] = sh_cnt[q];
		if (bad) a.stats->dbg |= SIMLOD_ERR_IMPORT;
		else first[a.n] = (uint32_t)chunks;
	}
}

__global__ __launch_bounds__(LANE_TPB) void k_i_nodes(ImportArgs a) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const uint32_t t = blockIdx.x * LANE_TPB + threadIdx.x;
	if (t >= a.n || hdr->ok == 0u) return;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.first);
	CopyItem* items = reinterpret_cast<CopyItem*>(a.scratch + a.lay.items);
	const SimlodExportNode e = a.table[t];
	const bool leaf = e.childMask == 0u;
	const uint32_t ns = e.numSamples, nch = ceil_chunks(ns), f = first[t];
	SimlodChunk* head = ns != 0u ? reinterpret_cast<SimlodChunk*>(a.pers + CHUNK_BASE + (uint64_t)f * CHUNK_STRIDE) : nullptr;
	SimlodNode nd;
	uint32_t r = 0;
	for (int k = 0; k < 8; k++) nd.children[k] = (e.childMask & (1u << k)) ? a.nodes + e.firstChild + r++ : nullptr;
	nd.counter = leaf ? ns : 0u;
	nd.numPoints = leaf ? ns : 0u;
	nd.level = e.level; nd.X = e.X; nd.Y = e.Y; nd.Z = e.Z;
	nd.countIteration = 0u; nd.countFlag = 0u;
	// 'r' and one digit per level below the root, the octant the path takes there (construct_expand.inc: the builder's names)
	for (int k = 0; k < 20; k++) nd.name[k] = 0;
	nd.name[0] = 'r';
	for (uint32_t l = 1; l <= e.level && l < 20u; l++) {
		const uint32_t s = e.level - l;
		nd.name[l] = (uint8_t)('0' + ((((e.X >> s) & 1u) << 2) | (((e.Y >> s) & 1u) << 1) | ((e.Z >> s) & 1u)));
	}
	nd.visible = 0; nd.isFiltered = 0; nd.isLeaf = 0; nd.isLarge = 0;
	nd.grid = nullptr;
	if (a.buildable) {
		const uint32_t g = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.map)[t];
		if (g != NONE) nd.grid = reinterpret_cast<SimlodOccupancyGrid*>(a.pers + hdr->gridBase + (uint64_t)g * GRID_STRIDE);
	}
	nd.points = leaf ? head : nullptr;
	nd.voxelChunks = leaf ? nullptr : head;
	nd.numVoxels = leaf ? 0u : ns;
	nd.numVoxelsStored = nd.numVoxels;
	a.nodes[t] = nd;
	const uint64_t src0 = reinterpret_cast<uint64_t>(a.samples + e.firstSample);
	for (uint32_t k = 0; k < nch; k++) {
		SimlodChunk* c = link_chunk_list(a.pers, CHUNK_BASE, f, nch, k);
		CopyItem it;
		it.src = src0 + (uint64_t)k * SIMLOD_POINTS_PER_CHUNK * sizeof(SimlodPoint);
		it.dst = reinterpret_cast<uint64_t>(c->points);
		it.count = min(ns - k * SIMLOD_POINTS_PER_CHUNK, SIMLOD_POINTS_PER_CHUNK);
		it.pad0 = 0; it.pad1 = 0;
		items[f + k] = it;
	}
}

__global__ void k_i_finish(ImportArgs a) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	// buildable: what the next kernel_construct launch is sized by (simlod_hip.cpp launch_plan), as k_reset reports it — nothing ingested, nothing uploaded
	if (a.buildable && a.feedback != nullptr) {
		a.feedback[0] = 0u; a.feedback[1] = 0u; a.feedback[2] = 1u;
		__hip_atomic_store(a.feedback + 3, a.feedbackSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
	if (hdr->ok == 0u) return;
	const uint32_t rootVoxChunks = ceil_chunks(hdr->rootVoxels);
	SimlodAllocatorGlobal* alloc = reinterpret_cast<SimlodAllocatorGlobal*>(a.pers);
	alloc->buffer = a.pers;
	alloc->offset = a.buildable ? hdr->rootVoxBase + (uint64_t)rootVoxChunks * CHUNK_STRIDE : CHUNK_BASE + hdr->totalChunks * CHUNK_STRIDE;
	SimlodStats s{};
	s.numNodes = a.n;
	s.numInner = hdr->counts[0]; s.numLeaves = hdr->counts[1]; s.numNonemptyLeaves = hdr->counts[2];
	// (the voxels of a root that is still a leaf are not counted: the builder's Stats count the lists of inner nodes only)
	s.numPoints = hdr->counts[3]; s.numVoxels = hdr->counts[4];
	s.numChunksPoints = hdr->counts[5]; s.numChunksVoxels = hdr->counts[6];
	s.allocatedBytes_persistent = alloc->offset;
	if (a.buildable) {
		// the builder's counters start as after a reset (batchletIndex, numPointsProcessed: 0), with an empty recycle stack: numAllocatedChunks is the
		// stack pointer a split returns its leaf's chunks below (voxels.cu:346-357), so it counts the point chunks in use, and chunkPoolSize (its
		// high-water mark) equals it — 0 would send the first split's chunks below the stack's bottom (SIMLOD_ERR_CHUNK_QUEUE_OVERFLOW)
		s.numAllocatedChunks = hdr->counts[5]; s.chunkPoolSize = hdr->counts[5];
		s.frameID = a.frameCounter;
		s.dbg = hdr->gridBad != 0u ? SIMLOD_ERR_IMPORT_GRID : 0u;
		*a.numBatchesUploaded = 0u;
		for (uint32_t k = 0; k < SIMLOD_BATCH_STREAM_SIZE; k++) a.batchSizes[k] = 0u;
	}
	*a.stats = s;
}
