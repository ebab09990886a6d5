// construct_begin.inc — part of construct.hip (included there, inside namespace simlod::build; not a translation unit of its own): k_begin: the launch's bookkeeping; the side tables restored from the node array when their stamp is stale.

// ---- begin: snapshot the upload counter, stamp the frame start (voxels.cu:823-825, 870-885); restore the side tables when they are stale -------
// The side tables — parents, ancestor paths, the top table, the chunk table, the recycle stack — and the per-node tag words survive between
// launches: k_expand keeps them current split by split, and every tag is a batch index + 1, which only grows while an octree lives.  They
// are rebuilt only when the stamp k_finish left does not name THIS octree in THIS state in THIS layout: the first launch, after a reset, an
// uploaded image, an aborted batch, a wiped or resized momentary buffer.  (Tags travel in 20 bits through the hash directory of voxel chunks: a
// full clear every 2^19 batches keeps them unambiguous.)  Every thread of the launch reads the stamp for itself — nobody writes those words
// while k_begin runs: the stamp is taken off by the launch's first k_count —, so the decision needs no second kernel (round 4: a memset and two
// kernels per launch; round 5, first: two kernels that exited at once; 9 us each on a chain that is one batch long).
// The tag-wrap test asks for the clear from the first launch that BEGINS within TAG_WRAP_WINDOW batches behind a multiple of 2^19: no launch may step
// over that window, so it is as wide as the most any device launch can take — a chained launch (simlod_launch_construct_chain) holds up to 20 groups
// of up to 20 batches.  WIDENED from 20 for chains (rather than cutting chains at the boundary): a plain launch that follows a chain across the wrap
// must see it too, and the price is a rebuild for a few launches once in 524 288 batches.
static constexpr uint32_t TAG_WRAP_WINDOW = 512;
static_assert(TAG_WRAP_WINDOW >= SIMLOD_MAX_BATCHES_PER_LAUNCH * SIMLOD_MAX_BATCHES_PER_LAUNCH, "a device launch takes at most 20 groups of at most 20 batches");
__device__ __forceinline__ bool stamp_is_stale(const BuildArgs& a, const Ctl* ctl) {
	const uint32_t first = a.stats->batchletIndex;
	return ctl->tableMagic != TABLE_MAGIC || ctl->tableBatch != first || ctl->tableNodes != (uint64_t)a.nodes || ctl->tablePers != (uint64_t)a.pers ||
	       ctl->tableLayout != layout_signature(a) || ctl->tableSig != table_signature(a.stats) ||
	       (first >= 0x80000u && (first & 0x7ffffu) < TAG_WRAP_WINDOW);
}

// (the 8 spare bytes Chunk::size / padding_0 of a list's HEAD chunk: the address of the list's last chunk)
__device__ __forceinline__ SimlodChunk*& tail_of(SimlodChunk* head) { return *reinterpret_cast<SimlodChunk**>(&head->size); }

// The side tables of an octree this buffer does not describe.  The per-node tag words and the hash directory are zeroed (offSplitTag .. offParent:
// a stale word could pass for a tag of this octree's batches), parents come from the children pointers, the rows of the chunk table from the
// lists, the top table and every node's ancestor list from a descent from the root (a node knows its level and cell: the ancestor at level l is
// entry level - 1 - l of its list — no pass has to wait for the parent table).
__device__ void rebuild_side_tables(const BuildArgs& a, bool irregular) {      // irregular: SIMLOD_DEBUG_IRREGULAR_CHILDREN — every inner node's child word says "look at Node.children" (tests the path of an image with scattered children)
	const uint64_t first = (uint64_t)blockIdx.x * TPB + threadIdx.x, stride = (uint64_t)gridDim.x * TPB;
	{
		uint4* w = reinterpret_cast<uint4*>(a.mom + a.offSplitTag);
		const uint64_t n = (a.offParent - a.offSplitTag) / 16;                 // (the offsets are 256-byte aligned)
		for (uint64_t i = first; i < n; i += stride) w[i] = make_uint4(0, 0, 0, 0);
	}
	const uint32_t numNodes = min(a.stats->numNodes, a.nodeCapacity);
	uint32_t* parentOf = at<uint32_t>(a, a.offParent);
	for (uint64_t i = first; i < TOP_CELLS; i += stride) {      // the top table: cell i's deepest node at level <= TOP_LEVEL
		const uint32_t s = (uint32_t)SIMLOD_MAX_DEPTH - TOP_LEVEL;
		const uint32_t X = ((uint32_t)i >> (2u * TOP_LEVEL)) << s, Y = (((uint32_t)i >> TOP_LEVEL) & (TOP_SIDE - 1u)) << s, Z = ((uint32_t)i & (TOP_SIDE - 1u)) << s;
		uint32_t cur = 0, level = 0;
		while (level < TOP_LEVEL) {
			const SimlodNode* c = a.nodes[cur].children[child_index(X, Y, Z, (int)level)];
			if (c == nullptr) break;
			cur = (uint32_t)(c - a.nodes); level++;
		}
		at<uint32_t>(a, a.offTop)[i] = cur | (level << 19) | (node_is_leaf(a.nodes + cur) ? TOP_LEAF : 0u);
	}
	for (uint64_t i = first; i < numNodes; i += stride) {
		if (i == 0) parentOf[0] = 0xffffffffu;
		const SimlodNode* n = a.nodes + i;
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const SimlodNode* c = n->children[k];
			if (c != nullptr) parentOf[(uint32_t)(c - a.nodes)] = (uint32_t)i;
		}
		{   // the node's child word
			const SimlodNode* c0 = n->children[0];
			uint32_t word = 0u, some = 0u;
			bool regular = c0 != nullptr;
#pragma unroll
			for (int k = 0; k < 8; k++) {
				const SimlodNode* c = n->children[k];
				if (c != nullptr) some++;
				if (c == nullptr || c != c0 + k) regular = false;
				else if (node_is_leaf(c)) word |= 1u << (KID_LEAF_SHIFT + (uint32_t)k);
			}
			at<uint32_t>(a, a.offKid)[i] = some == 0u ? 0u : regular && !irregular ? (word | (uint32_t)(c0 - a.nodes)) : KID_IRREGULAR;
		}
		// a leaf's row: its point chunks; an inner node's row: its voxel chunks (for the rasteriser).  And the word this builder keeps in the spare
		// bytes of a list's HEAD chunk, the address of the list's last chunk (O(1) append): an image built elsewhere — by the reference — has
		// none; found by walking the list once, here.
		uint8_t* const table = a.mom + a.offLeafChunks;
		const bool leaf = node_is_leaf(n);
		SimlodChunk* const head = leaf ? n->points : n->voxelChunks;
		const uint32_t inList = ((leaf ? n->numPoints : n->numVoxelsStored) + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
		SimlodChunk* c = head;
		for (uint32_t k = 0; c != nullptr && k < max(inList, 1u); k++) {      // (not beyond the list's last chunk: whether its `next` is null is the other builder's business)
			if (k < LEAF_SLOTS) leaf_row_set(table, a.pers, i, k, c);
			if (k + 1u == inList) tail_of(head) = c;
			c = c->next;
		}
		// (a LEAF that also has a voxel list — the root while it is still a leaf samples itself, voxels.cu:449-463 —: that list's tail word too;
		// voxroot_pieces / voxelize_small append behind it.  ADVICE r5: an image built elsewhere with fewer than 50 000 points)
		if (leaf && n->voxelChunks != nullptr) {
			const uint32_t inVox = (n->numVoxelsStored + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
			SimlodChunk* v = n->voxelChunks;
			for (uint32_t k = 0; v != nullptr && k < max(inVox, 1u); k++) {
				if (k + 1u >= inVox) { tail_of(n->voxelChunks) = v; break; }
				v = v->next;
			}
		}
		// the ancestors, parent first: the first PATH_ROW of them, zero-terminated when there are fewer (the others stand in the rows of the node's
		// PATH_ROW-th ancestor and of that one's, which their own threads write: path_far)
		unsigned long long* rec = at<unsigned long long>(a, a.offPaths) + i * PATH_ROW;
		const uint32_t L = min(n->level, PATH_WORDS - 1u), s = (uint32_t)SIMLOD_MAX_DEPTH - L;
		const uint32_t X = n->X << s, Y = n->Y << s, Z = n->Z << s;        // (child_index() takes coordinates at full depth)
		uint32_t cur = 0, l = 0;
		for (; l < L; l++) {
			const SimlodNode* anc = a.nodes + cur;
			if (L - 1u - l < PATH_ROW) rec[L - 1u - l] = path_pack(a.pers, cur, anc->level, anc->grid);
			const SimlodNode* c = anc->children[child_index(X, Y, Z, (int)l)];
			if (c == nullptr) break;                                         // (an image whose node is not where its coordinates say: entries below stay as they are, the list ends)
			cur = (uint32_t)(c - a.nodes);
		}
		if (L < PATH_ROW) rec[L] = 0;
	}
}

__global__ __launch_bounds__(TPB) void k_begin(BuildArgs a, uint32_t momentaryTooSmall, uint32_t batchLimit, uint32_t debugFlags, uint32_t budgetUs, uint32_t groupMax, uint32_t chainCap, uint32_t segLen) {
	Ctl* ctl = ctl_of(a);
	const bool stale = momentaryTooSmall != 0u || (debugFlags & 4u) != 0u || stamp_is_stale(a, ctl);      // (debugFlags bit 2: the host knows the image was replaced — simlod_octree_image_replaced, a reset)
	if (threadIdx.x == 0 && blockIdx.x == 0) {
		// sticky until the host resets the octree (the import bits: a buildable import whose table or grids failed its checks)
		const uint32_t fatal = a.stats->dbg & (SIMLOD_ERR_BARRIER_TIMEOUT | SIMLOD_ERR_DIRECTORY_FULL | SIMLOD_ERR_IMPORT | SIMLOD_ERR_IMPORT_GRID);
		ctl->errors = momentaryTooSmall ? SIMLOD_ERR_MOMENTARY_TOO_SMALL : 0u;
		ctl->stop = (momentaryTooSmall || fatal) ? 1u : 0u;
		ctl->abortBatch = 0;
		ctl->processed = 0;
		ctl->consumed = 0;
		ctl->pointsTaken = a.stats->numPointsProcessed;
		ctl->groupMax = groupMax;
		ctl->debugFlags = debugFlags;
		ctl->budgetUs = budgetUs != 0u ? budgetUs : (uint32_t)(SIMLOD_MAX_PROCESSING_MS * 1000.0f);
		ctl->startNs = wall_ns();
		*a.frameStart = ctl->startNs;
		// written concurrently by the upload stream (main_progressive_octree.cpp:1047-1050): device-scope load
		const uint32_t uploaded = __hip_atomic_load(a.numBatchesUploaded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const uint32_t first = a.stats->batchletIndex;
		uint32_t n = uploaded - first;
		if ((int32_t)n < 0) n = 0;
		if (n > chainCap) n = chainCap;      // voxels.cu:883: 20 — a chained launch: 20 (or the context's limit) per launch it stands for
		if (n > batchLimit) n = batchLimit;
		ctl->chainCap = chainCap; ctl->segLen = max(segLen, 1u);
		ctl->uploaded = uploaded;
		ctl->firstBatch = first;
		ctl->numBatches = n;
		for (int i = 0; i < 8; i++) ctl->statCounters[i] = 0;
		ctl->rebuildLeafChunks = stale ? 1u : 0u;
		if (momentaryTooSmall != 0u) ctl->tableMagic = 0;    // (a launch that does nothing: its k_finish leaves no stamp)
		for (uint32_t i = 0; i < BATCH_COPIES; i++) ctl->batch[i].active = 0;
		for (uint32_t i = 0; i < SIMLOD_MAX_BATCHES_PER_LAUNCH; i++) { ctl->voxT[i][0] = ~0ull; ctl->voxT[i][1] = 0; ctl->voxT[i][2] = 0; }
		prepare_batch(a, ctl, 0);
	}
	if (stale && momentaryTooSmall == 0u) rebuild_side_tables(a, (debugFlags & 8u) != 0u);
}
