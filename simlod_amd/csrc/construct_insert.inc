// construct_insert.inc — part of construct.hip (included there, inside namespace simlod::build; not a translation unit of its own): k_voxdone, k_rootpre, k_insert, k_stats, k_finish.

// ---- alloc: grow the chunk lists to their new lengths, build the per-batch chunk directory ----------------------
// (voxels.cu:485-538 allocatePointChunks, :641-672 allocateVoxelChunks, :298-300 countIteration stamp)

// ---- voxdone: the voxel lists are complete (voxels.cu:674-698: numVoxelsStored catches up with numVoxels) -------------------------------------
// After a batch's k_voxelize.  A node whose list grew gets its new tail: the last chunk's `next` is cleared and the head chunk remembers it
// (O(1) append next time).  `tag`: the batch whose hash directory names the new chunks.  Runs as part of the NEXT batch's k_insert (the
// first kernel on the caller's stream that has waited for the side stream; some workgroups at the end of its grid, which have no samples)
// and once more, as a kernel of its own, at the end of the launch.  Nodes the next batch has created meanwhile have no voxels: skipped.
__device__ void voxdone_nodes(const BuildArgs& a, Ctl* ctl, uint32_t tag, uint32_t numNodes, uint32_t first, uint32_t stride, bool skipRoot = false) {
	for (uint32_t i = first; i < numNodes; i += stride) {
		if (skipRoot && i == 0u) continue;
		SimlodNode* node = a.nodes + i;
		const uint32_t numVoxels = node->numVoxels, stored = node->numVoxelsStored;
		if (numVoxels == stored) continue;
		const uint32_t existing = (stored + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK, last = (numVoxels - 1u) / SIMLOD_POINTS_PER_CHUNK;
		if (last >= existing) {
			SimlodChunk* tail = dir_find(a, tag, i, last);
			if (tail != nullptr) { tail->next = nullptr; tail_of(node->voxelChunks) = tail; } else raise(ctl, SIMLOD_ERR_NULL_CHUNK);
		}
		node->numVoxelsStored = numVoxels;
	}
}
__global__ __launch_bounds__(TPB) void k_voxdone(BuildArgs a) {
	Ctl* ctl = ctl_of(a);
	if (ctl->processed == 0u || ctl->abortBatch) return;
	voxdone_nodes(a, ctl, ctl->tagOf[ctl->processed - 1u], min(a.stats->numNodes, a.nodeCapacity), blockIdx.x * TPB + threadIdx.x, gridDim.x * TPB);   // (the launch's last group)
}

// ---- rootpre: a group of several batches (exact or coalesced) in which the ROOT splits ------------------------------------------------------------------
// A root that is still a leaf samples ITSELF (voxels.cu:449-463: every node of the path that has a grid, and the root has one from the reset on), and the
// batch that splits it clears that grid and samples everything again from nothing (voxels.cu:371-382): the root's voxel list keeps what the batches
// before the split put there AND gets every cell again.  Ingested batch by batch that is what happens; in a group, the batches in front of the
// splitting one (k_expand knows which: BatchCtl.rootSplitAt) have to meet the root's grid as those batches would have — before k_insert clears it.
// One workgroup on the back stream in front of k_insert; leaves at once in every group but the one or two of an octree's life that split its root.
__global__ __launch_bounds__(1024) void k_rootpre(BuildArgs a, uint32_t ordinal) {
	Ctl* ctl = ctl_of(a);
	BatchCtl* bc = batch_of(ctl, ordinal);
	if (bc == nullptr || ctl->abortBatch || bc->groupBatches <= 1u) return;      // (exact groups: k_expand's accounting names the batch; coalesced groups: from the batches' sizes)
	const uint32_t sR = bc->rootSplitAt;
	if (sR == NONE || sR == 0u) return;
	// the root's voxel list as the group before left it (its k_voxelize has ended: stream order): closed here, in front of this group's first voxels
	if (threadIdx.x == 0u && ordinal > 0u) voxdone_nodes(a, ctl, ctl->tagOf[ordinal - 1u], 1u, 0u, 1u);
	__threadfence();
	__syncthreads();
	const uint32_t n = bc->start[min(sR, bc->groupBatches)], lane = (uint32_t)lane_id();
	const Samples<false> pts(a, bc);
	SimlodOccupancyGrid* const g = a.nodes[0].grid;
	if (g == nullptr) return;
	for (uint32_t base = 0; base < n; base += blockDim.x) {
		const uint32_t i = base + threadIdx.x;
		bool go = i < n;
		const float4 p = go ? pts[i] : make_float4(0, 0, 0, 0);
		const uint32_t pX = quantize(F_FULL, p.x, a.minx, a.size), pY = quantize(F_FULL, p.y, a.miny, a.size), pZ = quantize(F_FULL, p.z, a.minz, a.size);
		const uint32_t cell = grid_cell(0u, pX, pY, pZ), bit = cell & 31u;
		uint32_t* word = &g->values[cell >> 5];
		go = go && ((*word >> bit) & 1u) == 0u;                                                  // voxels.cu:93-94
		go = go && ((atomicOr(word, go ? 1u << bit : 0u) >> bit) & 1u) == 0u;                      // voxels.cu:96
		const unsigned long long wm = __ballot(go);
		if (wm == 0ull) continue;
		uint32_t first = 0;
		if (lane == 0u) first = atomicAdd(&a.nodes[0].numVoxels, (uint32_t)__popcll(wm));       // voxels.cu:101
		first = (uint32_t)__shfl((int)first, 0, 64);
		store_voxels_wave(a, ctl, bc->tag, go, 0u, first + (uint32_t)__popcll(wm & ((1ull << lane) - 1ull)), voxel_of(a, 0, pX, pY, pZ, p.w));
	}
}

// ---- insert: points into leaf chunks, regenerated voxels into voxel chunks (voxels.cu:540-639, 674-698) --------
struct InsertShared {
	BlockTable tbl;                       // node -> count (step 1), then node -> running cursor (step 3)
	uint32_t base[TBL_CAP];               // first slot of the range this workgroup reserved in the node
	uint32_t dirBase[TBL_CAP];            // chunk-directory base of the node for this batch, or 0xffffffff
	uint32_t dirFirst[TBL_CAP];
};

// The points go into their leaves (before k_voxelize, which reads them back leaf by leaf), and with them what used to be kernels of their
// own: the clearing of the grids of the nodes this batch split, the end-of-batch bookkeeping.  The chunks are there already (k_hist,
// k_expand).  In steps: (1) everybody counts its samples per leaf in an LDS table — a relabelled sample finds its leaf in its slot's map —
// (2) reserves one slot range per (workgroup, leaf) with one global atomic each, (3) stores: the slot inside the range comes from an
// LDS cursor.  Barriers are paid per workgroup, not per chunk.
template <bool SINGLE>
__global__ __launch_bounds__(TPB) void k_insert(BuildArgs a, uint32_t ordinal) {
	Ctl* ctl = ctl_of(a);
	BatchCtl* bc = batch_of(ctl, ordinal);
	if (bc == nullptr) return;
	if (ctl->abortBatch) {                                  // an earlier kernel gave up: the batch is not counted (Stats.dbg says why)
		if (blockIdx.x == 0 && threadIdx.x == 0) end_of_batch(a, ctl, bc);
		return;
	}
	__shared__ InsertShared sh;
	const uint32_t n = bc->batchSize;
	const uint32_t total = n + min(bc->numSpilled, a.spilledCap);
	const Samples<SINGLE> pts(a, bc);
	const float4* spilled = at<const float4>(a, a.offSpilled);
	const LeafWords leafOf(a, ordinal);
	const NodeDir* nodeDir = at<const NodeDir>(a, a.offNodeDir);
	SimlodChunk* const* chunkDir = chunk_dir(a, bc);
	const uint32_t tag = bc->tag;
	const uint32_t numChunks = (total + PPB - 1) / PPB;

	{
		Phase ph(ctl, blockIdx.x == 0 || blockIdx.x + 1u == numChunks);
		const uint32_t pb = blockIdx.x == 0 ? 8u : 16u;
		// (The end-of-batch bookkeeping — voxels.cu:925-949: Stats.batchletIndex, numPointsProcessed, the time budget — is k_voxelize's first act:
		// a host that watches Stats.batchletIndex outside stream order, as the reference's uploader does with its back-pressure rule
		// (main_progressive_octree.cpp:1012), may refill the group's ring slots the moment the index moves, and until this kernel has ENDED
		// its workgroups may still be reading them.  Counting the workgroups in with an atomic each was measured: 2 048 adds on one word,
		// 4.7 ms per ingest instead of 3.7.)
		// ... and the 32 before it close the voxel lists of the previous batch (voxdone_nodes: this kernel has waited for its k_voxelize)
		{
			constexpr uint32_t DONE_WGS = 32;
			const uint32_t back = gridDim.x - 1u - blockIdx.x;
			if (back >= 1u && back <= DONE_WGS && bc->ordinal != 0u)
				voxdone_nodes(a, ctl, ctl->tagOf[bc->ordinal - 1u], min(a.stats->numNodes, a.nodeCapacity), (back - 1u) * TPB + threadIdx.x, DONE_WGS * TPB,
				              bc->groupBatches > 1u && bc->rootSplitAt != 0xffffffffu && bc->rootSplitAt != 0u);      // (k_rootpre has closed the root's list and appended to it since)
		}
		ph.mark(pb + 0);
		// the occupancy grids of the nodes this batch split (k_count's tail and k_expand listed them): cleared here, by everybody, before
		// k_voxelize samples into them (voxels.cu:371-382) — 256 KB each, the stores ride along with the loads below
		const uint32_t numClear = min(bc->numClear, a.clearCap);
		SimlodOccupancyGrid* const* clearList = clear_list(a, ordinal);
		constexpr uint32_t W4 = SIMLOD_GRID_NUM_WORDS / 4;
		for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < numClear * W4; i += gridDim.x * TPB)
			reinterpret_cast<uint4*>(clearList[i / W4]->values)[i % W4] = make_uint4(0, 0, 0, 0);
		if (blockIdx.x >= numChunks) return;

		ph.mark(pb + 1);
		// (1) samples per leaf
		table_init(sh.tbl);
		__syncthreads();
		const uint32_t* map = at<const uint32_t>(a, a.offMap);
		for (uint32_t chunk = blockIdx.x; chunk < numChunks; chunk += gridDim.x) {
			uint32_t v[PPT];
#pragma unroll
			for (uint32_t j = 0; j < PPT; j++) {
				const uint32_t t = chunk * PPB + j * TPB + threadIdx.x;
				v[j] = t < total ? leafOf[t < n ? t : a.groupCap + (t - n)] : NONE;
			}
#pragma unroll
			for (uint32_t j = 0; j < PPT; j++) {
				// a sample that k_hist / k_expand relabelled (slot, bin): its leaf is one word of the slot's map; any other: the leaf k_count found
				if (v[j] == NONE) continue;
				if ((v[j] & LEAF_FLAG) == 0u) { v[j] &= LEAF_NODE_MASK; continue; }
				uint32_t e = map[v[j] & 0x1fffffu];
				if ((e & MAP_LISTED) != 0u) e = slot_recs(a, ordinal)[e & 0xffffu].node;      // (a node that got a slot but no round any more: it stays a leaf)
				v[j] = e;
				const uint32_t t = chunk * PPB + j * TPB + threadIdx.x;
				leafOf[t < n ? t : a.groupCap + (t - n)] = e;
			}
#pragma unroll
			for (uint32_t j = 0; j < PPT; j++) {
				if (v[j] == NONE) continue;
				uint32_t rank;
				(void)table_add(sh.tbl, v[j], 1u, &rank);
			}
		}
		__syncthreads();
		ph.mark(pb + 2);
		// (2) one slot range per (workgroup, leaf)
		for (uint32_t e = threadIdx.x; e < (uint32_t)TBL_CAP; e += TPB) {
			const uint32_t key = sh.tbl.keys[e];
			if (key == TBL_EMPTY) continue;
			const NodeDir d = nodeDir[key];
			sh.base[e] = atomicAdd(&a.nodes[key].numPoints, sh.tbl.vals[e]);                      // voxels.cu:593
			sh.tbl.vals[e] = 0;                                                                    // becomes the cursor
			sh.dirBase[e] = d.ptTag == tag ? d.ptBase : 0xffffffffu;
			sh.dirFirst[e] = d.ptFirst;
		}
		__syncthreads();
		ph.mark(pb + 3);
		for (uint32_t chunk = blockIdx.x; chunk < numChunks; chunk += gridDim.x) {
			float4 p[PPT];
			const float4* base = nullptr; uint32_t kspan;
			const bool oneBatch = chunk * PPB < n && pts.span(chunk * PPB, min(n, (chunk + 1u) * PPB) - 1u, base, kspan);      // (workgroup-uniform)
#pragma unroll
			for (uint32_t j = 0; j < PPT; j++) {
				const uint32_t t = chunk * PPB + j * TPB + threadIdx.x;
				p[j] = t >= total ? make_float4(0, 0, 0, 0) : (t < n ? (oneBatch ? base[t] : pts[t]) : spilled[t - n]);
			}
#pragma unroll
			for (uint32_t j = 0; j < PPT; j++) {
				const uint32_t t = chunk * PPB + j * TPB + threadIdx.x;
				if (t >= total) continue;
				const uint32_t leafIdx = leafOf[t < n ? t : a.groupCap + (t - n)] & LEAF_NODE_MASK;
				const int e = table_find(sh.tbl, leafIdx);
				uint32_t slot, base, first;
				if (e >= 0) { slot = sh.base[e] + atomicAdd(&sh.tbl.vals[e], 1u); base = sh.dirBase[e]; first = sh.dirFirst[e]; }
				else {                                                                                // table had no room for this leaf
					const NodeDir d = nodeDir[leafIdx];
					slot = atomicAdd(&a.nodes[leafIdx].numPoints, 1u); base = d.ptTag == tag ? d.ptBase : 0xffffffffu; first = d.ptFirst;
				}
				if (base == 0xffffffffu) { raise(ctl, SIMLOD_ERR_NULL_CHUNK); continue; }           // voxels.cu:599-604
				SimlodChunk* c = chunkDir[base + (slot / SIMLOD_POINTS_PER_CHUNK - first)];
				reinterpret_cast<float4*>(c->points)[slot % SIMLOD_POINTS_PER_CHUNK] = p[j];
			}
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		ph.mark(pb + 5);
		if (ph.on) ctl->phaseNs[pb + 6] += 1;
	}
}

// ---- stats pass (voxels.cu:957-1009) -------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	return v;
}

__global__ __launch_bounds__(TPB) void k_stats(BuildArgs a) {
	Ctl* ctl = ctl_of(a);
	const uint32_t numNodes = min(a.stats->numNodes, a.nodeCapacity);
	uint32_t v[7] = {0, 0, 0, 0, 0, 0, 0};   // inner, leaves, nonempty, points, voxels, chunksP, chunksV
	for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < numNodes; i += gridDim.x * TPB) {      // (a grid for the nodes that exist, not for the node capacity)
		SimlodNode* n = a.nodes + i;
		// voxels.cu:298-300: every counting pass stamps every node with (index of the batch + 1); what the host can see is the last stamp
		if (ctl->processed != 0u) n->countIteration = a.stats->batchletIndex;
		if (node_is_leaf(n)) {
			v[1] += 1; v[3] += n->numPoints; v[5] += (n->numPoints + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
			v[2] += n->numPoints > 0 ? 1u : 0u;
		} else {
			v[0] += 1; v[4] += n->numVoxels; v[6] += (n->numVoxels + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK;
		}
	}
	for (int k = 0; k < 7; k++) {
		const uint32_t s = wave_sum(v[k]);
		if (lane_id() == 0 && s != 0u) atomicAdd(&ctl->statCounters[k], s);
	}
}

__global__ void k_finish(BuildArgs a, uint32_t fits, uint32_t* feedback, const uint32_t* numBatchesUploaded, uint32_t launchSeq) {
	if (blockIdx.x != 0) return;
	Ctl* ctl = ctl_of(a);
	SimlodStats* s = a.stats;
	__shared__ Phantom sh_phantom;
	// voxels.cu:535-537 for the launch's last group (k_count's first workgroup: the others); an exact group of several batches: account_group
	if (threadIdx.x == 0) sh_phantom = account_group(a, ctl, ctl->processed != 0u ? batch_of(ctl, ctl->processed - 1u) : nullptr);
	__syncthreads();
	phantom_fill(a, sh_phantom);
	if (threadIdx.x != 0) return;
	if (feedback != nullptr) {      // what the next launch sizes itself by (groups_for_launch): page-locked host memory
		feedback[0] = s->batchletIndex; feedback[1] = *numBatchesUploaded;
		// ... and whether its batches can go in groups (exact mode, prepare_batch decides for every group; a launch whose groups would each be cut down to
		// one batch had better enqueue one group of kernels per batch): the allocator is a worst-case full group away from the guard
		const SimlodAllocatorGlobal* alloc = reinterpret_cast<const SimlodAllocatorGlobal*>(a.pers);
		feedback[2] = a.acct != 0u &&
		              alloc->offset + SIMLOD_MEM_SAFETY_MARGIN + slack_for(a, (unsigned long long)a.groupCap + min((unsigned long long)a.spilledCap, (unsigned long long)s->numPointsProcessed)) < a.persCapacity ? 1u : 0u;
		__hip_atomic_store(feedback + 3, launchSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);      // (last: a reader that sees this launch's number sees its report)
	}
	s->numInner = ctl->statCounters[0];
	s->numLeaves = ctl->statCounters[1];
	s->numNonemptyLeaves = ctl->statCounters[2];
	s->numPoints = ctl->statCounters[3];
	s->numVoxels = ctl->statCounters[4];
	s->numChunksPoints = ctl->statCounters[5];
	s->numChunksVoxels = ctl->statCounters[6];
	s->allocatedBytes_momentary = a.scratchBytes;
	s->allocatedBytes_persistent = reinterpret_cast<const SimlodAllocatorGlobal*>(a.pers)->offset;
	s->frameID = (uint32_t)a.frameCounter;
	s->dbg |= ctl->errors;
	if (fits && !ctl->abortBatch) {              // the side tables describe THIS octree as it is after THIS batch
		ctl->tableBatch = s->batchletIndex;
		ctl->tableNodes = (uint64_t)a.nodes;
		ctl->tablePers = (uint64_t)a.pers;
		ctl->tableSig = table_signature(s);
		ctl->tableLayout = layout_signature(a);
		ctl->tableMagic = TABLE_MAGIC;
	}
}
