// export_table.inc — part of export.hip: the export's table.  hier_walk (the breadth-first walk every call family starts with), NoEntry, k_x_hier,
// k_x_scan, k_x_dir.

// The breadth-first walk of k_x_hier and, QUERY, of k_q_hier: there a child that lies outside the region is not listed (it counts as cut off
// for the node-count check), and cls[t] gets the class of every listed entry; numSamples then holds the samples BEFORE the test.
// classify(level, X, Y, Z): the class of that cube (QUERY only; NoRegion where there is no region to ask).
// entry(t, e, srcLeaf): what a walk does per listed entry on top, with the entry as it is about to be written (k_v_hier, export_view.inc: the
// entries of the levels above are written, and a barrier lies in between); NoEntry: nothing.
// QUERY is false (WALK_EXPORT), true (WALK_QUERY) or WALK_INVERSE (the inverse selections, export_inverse.inc): the classes are written, but no
// child is asked and none is left out — the table is the export's —, and an entry of class Q_EMPTIED loses its samples as an outside root does.
constexpr uint32_t WALK_EXPORT = 0u, WALK_QUERY = 1u, WALK_INVERSE = 2u;
struct NoEntry { __device__ __forceinline__ void operator()(uint32_t, const SimlodExportNode&, bool) const {} };
template <uint32_t QUERY, typename Classify, typename Entry = NoEntry>
__device__ __forceinline__ void hier_walk(const ExportArgs& a, Classify classify, uint32_t* cls, Entry entry = Entry()) {
	__shared__ uint32_t sh_scan[WG_WAVES];
	__shared__ uint32_t sh_err, sh_trunc;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* map = reinterpret_cast<uint32_t*>(a.scratch + a.lay.map);
	uint32_t* par = reinterpret_cast<uint32_t*>(a.scratch + a.lay.par);
	const uint32_t numNodes = a.stats->numNodes;
	const uint32_t maxLevel = min(a.maxLevel, (uint32_t)SIMLOD_MAX_DEPTH);
	if (threadIdx.x == 0) {
		sh_err = numNodes == 0u ? SIMLOD_EXPORT_ERR_NODE_COUNT : a.cap == 0u ? SIMLOD_EXPORT_ERR_CAPACITY : 0u;
		sh_trunc = 0u;
		if (sh_err == 0u) { map[0] = 0u; par[0] = NONE; }
	}
	__syncthreads();
	uint32_t lo = 0u, hi = sh_err == 0u ? 1u : 0u;
	for (uint32_t L = 0; L <= maxLevel && lo < hi; L++) {
		uint32_t next = hi;
		for (uint32_t base = lo; base < hi; base += WG_TPB) {
			const uint32_t t = base + threadIdx.x;
			const bool act = t < hi;
			const uint32_t src = act ? map[t] : 0u;
			const SimlodNode* n = a.nodes + src;
			uint32_t child[8], mask = 0u;
			bool srcLeaf = true;
			if (act) {
#pragma unroll
				for (int k = 0; k < 8; k++) {
					const SimlodNode* c = n->children[k];
					child[k] = 0u;
					if (c == nullptr) continue;
					srcLeaf = false;
					const uint64_t idx = (uint64_t)(c - a.nodes);
					if (c < a.nodes || idx >= numNodes) { atomicOr(&sh_err, SIMLOD_EXPORT_ERR_NODE_COUNT); continue; }
					child[k] = (uint32_t)idx;
					if (L >= maxLevel) continue;
					// (the child's cube follows from its parent's: no load of the child's record, which would put eight dependent loads in a row)
					if (QUERY == WALK_QUERY && classify(n->level + 1u, 2u * n->X + ((k >> 2) & 1), 2u * n->Y + ((k >> 1) & 1), 2u * n->Z + (k & 1)) == Q_OUTSIDE) {
						atomicOr(&sh_trunc, 1u);
						continue;
					}
					mask |= 1u << k;
				}
				if (!srcLeaf && L >= maxLevel) atomicOr(&sh_trunc, 1u);
			}
			uint32_t total;
			const uint32_t off = block_scan<uint32_t>((uint32_t)__popc(mask), total, sh_scan);
			const uint32_t fc = next + off;
			if (act) {
				uint32_t r = 0;
				for (int k = 0; k < 8; k++) {
					if (!(mask & (1u << k))) continue;
					if (fc + r < a.cap) { map[fc + r] = child[k]; par[fc + r] = t; }
					else atomicOr(&sh_err, SIMLOD_EXPORT_ERR_CAPACITY);
					r++;
				}
				const uint32_t parent = par[t];
				bool sel = true;
				if (a.select == SIMLOD_EXPORT_CUT) sel = srcLeaf || L == maxLevel;
				else if (a.select == SIMLOD_EXPORT_VISIBLE) {
					// render.cu:905-935 as r_visible decides it (render.hip visible_nodes): drawn = visible && (large ? leaf : parent large)
					const bool parentLarge = parent != NONE && a.nodes[map[parent]].isLarge != 0;
					sel = n->visible != 0 && (n->isLarge != 0 ? srcLeaf : parentLarge);
				}
				SimlodExportNode e;
				e.level = n->level; e.X = n->X; e.Y = n->Y; e.Z = n->Z;
				e.parent = parent;
				e.firstChild = mask != 0u ? fc : NONE;
				e.childMask = (uint8_t)mask;
				e.flags = (uint8_t)((srcLeaf ? SIMLOD_EXPORT_FLAG_LEAF : 0u) | (sel ? SIMLOD_EXPORT_FLAG_SELECTED : 0u));
				e.reserved = 0;
				e.numSamples = sel ? (srcLeaf ? n->numPoints : n->numVoxels) : 0u;
				e.firstSample = 0;
				if (QUERY) {
					const uint32_t c = classify(e.level, e.X, e.Y, e.Z);              // (only the root can be outside here)
					if (c == Q_OUTSIDE || (QUERY == WALK_INVERSE && c == Q_EMPTIED)) e.numSamples = 0u;
					cls[t] = c;
				}
				entry(t, e, srcLeaf);
				a.table[t] = e;
			}
			next += total;
		}
		__syncthreads();                         // (the children's map entries, written by other lanes, are read next level)
		lo = hi;
		hi = min(next, a.cap);
		if (sh_err & SIMLOD_EXPORT_ERR_CAPACITY) break;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t err = sh_err;
		const uint32_t listed = (err & SIMLOD_EXPORT_ERR_CAPACITY) ? lo : hi;        // entries written
		// every node is reached exactly once from the root: all of them when nothing was cut off, no more than all of them otherwise
		if (sh_trunc == 0u ? listed != numNodes : listed > numNodes) err |= SIMLOD_EXPORT_ERR_NODE_COUNT;
		hdr->error = err;
		hdr->numListed = listed;
	}
}

// (the walk of the export and of the ray query: no region, nothing is asked)
struct NoRegion { __device__ uint32_t operator()(uint32_t, uint32_t, uint32_t, uint32_t) const { return Q_COPIED; } };
__global__ __launch_bounds__(WG_TPB) void k_x_hier(ExportArgs a) { hier_walk<false>(a, NoRegion(), nullptr); }

__global__ __launch_bounds__(WG_TPB) void k_x_scan(ExportArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	const TableScan s = scan_table(a, sh_scan, [](uint32_t) {});
	if (threadIdx.x == 0) {
		const uint32_t err = s.err | (s.samples > a.sampleCap ? SIMLOD_EXPORT_ERR_CAPACITY : 0u);
		hdr->numItems = (err & SIMLOD_EXPORT_ERR_CAPACITY) ? 0u : s.items;     // a sample array that is too small gets nothing
		SimlodExportCounts c;
		c.numNodes = s.n; c.error = err; c.numSamples = s.samples;
		*a.counts = c;
	}
}

__global__ __launch_bounds__(LANE_TPB) void k_x_dir(ExportArgs a) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const uint32_t* map = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.map);
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.first);
	CopyItem* items = reinterpret_cast<CopyItem*>(a.scratch + a.lay.items);
	const uint32_t t = blockIdx.x * LANE_TPB + threadIdx.x;
	if (t >= hdr->numListed || hdr->numItems == 0u) return;
	const SimlodExportNode& e = a.table[t];
	const uint32_t ns = e.numSamples;
	if (ns == 0u) return;
	const uint32_t src = map[t];
	const SimlodNode* n = a.nodes + src;
	const bool leaf = (e.flags & SIMLOD_EXPORT_FLAG_LEAF) != 0u;
	const SimlodChunk* c = leaf ? n->points : n->voxelChunks;
	const bool rows = leaf_rows_valid(a, src, c, leaf);
	const uint32_t nch = ceil_chunks(ns), f = first[t];
	const uint64_t dst0 = reinterpret_cast<uint64_t>(a.samples + e.firstSample);
	uint32_t k = 0;
	for (; k < nch; k++) {
		if (k > 0u) c = rows && k < a.ltSlots ? leaf_row_get(a.lt, a.ltPers, src, k) : c->next;
		if (c == nullptr) { atomicOr(&a.counts->error, SIMLOD_EXPORT_ERR_SHORT_LIST); break; }
		CopyItem it;
		it.src = reinterpret_cast<uint64_t>(c->points);
		it.dst = dst0 + (uint64_t)k * SIMLOD_POINTS_PER_CHUNK * sizeof(SimlodPoint);
		it.count = min(ns - k * SIMLOD_POINTS_PER_CHUNK, SIMLOD_POINTS_PER_CHUNK);
		it.pad0 = 0; it.pad1 = 0;
		items[f + k] = it;
	}
	for (; k < nch; k++) items[f + k] = CopyItem{0, 0, 0, 0, 0};
}
