// export_view.inc — part of export.hip: view queries.  ViewArgs, k_v_hier, k_v_scan.
// ---- view query -------------------------------------------------------------------------------------------------------------------------
// simlod_query_view (simlod_hip.h, "view queries"): four launches on the caller's stream, two of them the export's own.
//   k_v_hier   ONE workgroup: k_x_hier's walk (every listed entry selected, numSamples the node's count), and per entry rules V2 and V3 from
//              view_rules.hpp: the rank R goes into the entry's word of first[] — free until the scan — where the level below reads its
//              parents' ranks after the level's barrier.  A visible node is drawn at the biases [from, to) (rule V4), which go into the word
//              too: the ladder S(b) is kept in LDS in difference form — add at `from`, subtract at `to`, LDS atomics — and summed up at the
//              end; one lane then chooses the bias (rule V6) and writes the counts.  A second sweep over the entries' words takes SELECTED
//              and numSamples from what is not drawn at that bias.
//   k_v_scan   ONE workgroup: k_x_scan's scans (scan_table), and its counts — the first 16 bytes of SimlodViewCounts — with the view's rules for
//              the items: none in a count-only call, none when no bias fits the budget.
//   k_x_dir, k_copy   as simlod_export_octree runs them.
// The source is only read (rule V9).
struct ViewArgs {
	ExportArgs        x;                // (x.counts: the head of `counts` — numNodes, error, numSamples lie where SimlodExportCounts has them)
	ViewGeom          g;
	uint32_t          flags, minBias, maxBias, pad;
	uint64_t          budget;
	SimlodViewCounts* counts;
};
static_assert(offsetof(SimlodViewCounts, numNodes) == offsetof(SimlodExportCounts, numNodes) && offsetof(SimlodViewCounts, error) == offsetof(SimlodExportCounts, error) &&
              offsetof(SimlodViewCounts, numSamples) == offsetof(SimlodExportCounts, numSamples), "k_v_scan, k_x_dir: the view's counts begin as the export's");

// an entry's word: R in bits 0-7, a source leaf in bit 9, and the biases [from, to) at which it is drawn in bits 10-14 and 15-19 (both 0: never)
constexpr uint32_t VIEW_RANK_MASK = 0xffu, VIEW_LEAF = 0x200u, VIEW_FROM_SHIFT = 10u, VIEW_TO_SHIFT = 15u, VIEW_BIAS_MASK = 0x1fu;
static_assert(VIEW_RANKS == 21u && VIEW_RANKS <= VIEW_RANK_MASK && VIEW_RANKS <= VIEW_BIAS_MASK, "k_v_hier: 21 biases; a rank, a `from` and a `to` fit their bits");
constexpr uint32_t VIEW_SWEEP = 8u;                                                 // the second sweep: that many words of a lane in flight
// The ladder's counters, VIEW_COPIES times: the nodes of a level mostly share their `from` and `to`, and atomics of one wave on one LDS word go
// one after the other.  A lane adds to the copy of its number modulo VIEW_COPIES — two lanes of a wave per word at most —, and the copies are
// summed up once.  An odd stride in 8-byte words (21) spreads the copies over the banks.
constexpr uint32_t VIEW_COPIES = 32u;
static_assert((VIEW_COPIES & (VIEW_COPIES - 1u)) == 0u && WG_TPB % VIEW_COPIES == 0u, "k_v_hier: threadIdx.x & (VIEW_COPIES - 1) names a copy");

__global__ __launch_bounds__(WG_TPB) void k_v_hier(ViewArgs v) {
	__shared__ float sh_planes[6][4];
	__shared__ unsigned long long sh_samples[VIEW_COPIES][VIEW_RANKS];   // the ladder S(b) in difference form, per copy; [0][b] is S(b) once lane 0 has summed up
	__shared__ uint32_t sh_nodes[VIEW_COPIES][VIEW_RANKS + 1u];          // ... and the nodes drawn at b; [copy][VIEW_RANKS]: the visible nodes
	__shared__ uint32_t sh_bias;
	const ExportArgs& a = v.x;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* rank = reinterpret_cast<uint32_t*>(a.scratch + a.lay.first);
	const uint32_t copy = threadIdx.x & (VIEW_COPIES - 1u);
	for (uint32_t i = threadIdx.x; i < VIEW_COPIES * VIEW_RANKS; i += WG_TPB) (&sh_samples[0][0])[i] = 0ull;
	for (uint32_t i = threadIdx.x; i < VIEW_COPIES * (VIEW_RANKS + 1u); i += WG_TPB) (&sh_nodes[0][0])[i] = 0u;
	// the planes are the same for every node: normalised once (render_visible.inc r_visible does the same, a lane per plane)
#pragma unroll
	for (int i = 0; i < 6; i++) if (threadIdx.x == (uint32_t)i) view_frustum_plane(v.g.m, i, sh_planes[i]);
	__syncthreads();
	const uint32_t rootP = (v.flags & SIMLOD_VIEW_DRAW_SMALL_ROOT) ? VIEW_RANKS : 0u;
	hier_walk<false>(a, NoRegion(), nullptr, [&](uint32_t t, const SimlodExportNode& e, bool srcLeaf) {
		const uint32_t P = e.parent == NONE ? rootP : min(rank[e.parent] & VIEW_RANK_MASK, VIEW_RANKS);    // (on its way during the geometry)
		bool inside;
		float dx, dy;
		view_node_geometry(v.g, sh_planes, e.level, e.X, e.Y, e.Z, inside, dx, dy);
		const uint32_t R = view_rank(v.g.minNodeSize, dx, dy);
		const bool visible = (inside || (v.flags & SIMLOD_VIEW_NO_CULL)) && e.numSamples > 0u;
		uint32_t from, to;
		view_drawn_range(R, P, srcLeaf, from, to);
		const bool ever = visible && from < to;                  // (from < to <= VIEW_RANKS: `from` indexes the ladder, `to` where it is below VIEW_RANKS)
		rank[t] = R | (srcLeaf ? VIEW_LEAF : 0u) | (ever ? from << VIEW_FROM_SHIFT | to << VIEW_TO_SHIFT : 0u);
		if (visible) atomicAdd(&sh_nodes[copy][VIEW_RANKS], 1u);
		if (!ever) return;
		atomicAdd(&sh_samples[copy][from], (unsigned long long)e.numSamples);
		atomicAdd(&sh_nodes[copy][from], 1u);
		if (to < VIEW_RANKS) {
			atomicAdd(&sh_samples[copy][to], 0ull - (unsigned long long)e.numSamples);
			atomicAdd(&sh_nodes[copy][to], 0u - 1u);
		}
	});
	__syncthreads();
	// the second sweep's words and what lane 0 needs of the header, on their way while the ladder is summed up (the words of entries that are
	// not listed are loaded — first[] has a word for every entry up to the capacity — and not used)
	uint32_t w[VIEW_SWEEP];
#pragma unroll
	for (uint32_t j = 0; j < VIEW_SWEEP; j++) { const uint32_t t = threadIdx.x + j * WG_TPB; w[j] = t < a.cap ? rank[t] : 0u; }
	const uint32_t n = hdr->numListed, errWalk = hdr->error;
	if (threadIdx.x <= VIEW_RANKS) {                             // lane b sums the copies of its rung up (lane VIEW_RANKS: of the visible nodes)
		unsigned long long s = 0ull;
		uint32_t k = 0u;
		for (uint32_t c = 0; c < VIEW_COPIES; c++) {
			if (threadIdx.x < VIEW_RANKS) s += sh_samples[c][threadIdx.x];
			k += sh_nodes[c][threadIdx.x];
		}
		if (threadIdx.x < VIEW_RANKS) sh_samples[0][threadIdx.x] = s;    // (a lane reads and writes its own column only)
		sh_nodes[0][threadIdx.x] = k;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		SimlodViewCounts c;
		unsigned long long runS = 0ull;
		uint32_t runN = 0u;
		for (uint32_t b = 0; b < VIEW_RANKS; b++) {
			runS += sh_samples[0][b]; runN += sh_nodes[0][b];
			sh_samples[0][b] = runS; sh_nodes[0][b] = runN;
			c.samplesAt[b] = runS;
		}
		// rule V6: the smallest bias of the range that fits; none: the coarsest, and an error
		const uint32_t hiB = min(v.maxBias, (uint32_t)SIMLOD_VIEW_MAX_BIAS), loB = min(v.minBias, hiB);
		uint32_t bias = VIEW_RANKS;
		for (uint32_t b = hiB + 1u; b-- > loB;) if (sh_samples[0][b] <= v.budget) bias = b;
		uint32_t err = errWalk;
		if (bias == VIEW_RANKS) { bias = hiB; err |= SIMLOD_EXPORT_ERR_BUDGET; }
		hdr->error = err;
		sh_bias = bias;
		c.numNodes = n; c.error = err; c.numSamples = sh_samples[0][bias];
		c.bias = bias; c.numSelected = sh_nodes[0][bias]; c.numInside = sh_nodes[0][VIEW_RANKS]; c.reserved = 0u;
		*v.counts = c;
	}
	__syncthreads();
	// rule V7: what is not drawn at the chosen bias is not selected
	const uint32_t bias = sh_bias;
	for (uint32_t base = 0; base < n; base += VIEW_SWEEP * WG_TPB) {
#pragma unroll
		for (uint32_t j = 0; j < VIEW_SWEEP; j++) {
			const uint32_t t = base + threadIdx.x + j * WG_TPB;
			if (base != 0u) w[j] = t < n ? rank[t] : 0u;
			if (t >= n || (bias >= ((w[j] >> VIEW_FROM_SHIFT) & VIEW_BIAS_MASK) && bias < ((w[j] >> VIEW_TO_SHIFT) & VIEW_BIAS_MASK))) continue;
			a.table[t].flags = (uint8_t)((w[j] & VIEW_LEAF) ? SIMLOD_EXPORT_FLAG_LEAF : 0u);
			a.table[t].numSamples = 0u;
		}
	}
}
static_assert(SIMLOD_VIEW_MAX_BIAS + 1u == VIEW_RANKS, "k_v_hier: bias <= SIMLOD_VIEW_MAX_BIAS indexes the ladder");

__global__ __launch_bounds__(WG_TPB) void k_v_scan(ExportArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	const TableScan s = scan_table(a, sh_scan, [](uint32_t) {});
	if (threadIdx.x == 0) {
		const bool write = a.samples != nullptr;                                // (a count-only call: no capacity to miss)
		const uint32_t err = s.err | (write && s.samples > a.sampleCap ? SIMLOD_EXPORT_ERR_CAPACITY : 0u);
		hdr->numItems = (!write || (err & (SIMLOD_EXPORT_ERR_CAPACITY | SIMLOD_EXPORT_ERR_BUDGET))) ? 0u : s.items;
		SimlodExportCounts c;
		c.numNodes = s.n; c.error = err; c.numSamples = s.samples;
		*a.counts = c;
	}
}
