// export_lasso.inc — part of export.hip: lasso queries.  LassoGeom, LassoArgs, LassoPaintArgs, LassoSummaryArgs, stage_edges, Lasso (rule L1),
// k_l_hier, k_l_count, k_l_write, k_el_paint, k_ls_partial.
// ---- lasso query ------------------------------------------------------------------------------------------------------------------------
// simlod_query_lasso / simlod_paint_lasso / simlod_query_summary_lasso (simlod_hip.h, "lasso queries"): the footprint query's launches with a
// polygon on the screen of a perspective camera in the extruded polygon's place.
//   k_l_hier   k_q_hier with the class of a node combined from the planes (classify) and the lasso (classify_lasso, lasso_rules.hpp), as k_f_hier
//              combines them.  A lane keeps (U, V, W) of the eight corners of its node in registers and evaluates c eight times per edge.
//   k_q_dir, k_q_scan, k_s_final   as they are.
//   k_l_count, k_l_write, k_el_paint, k_ls_partial   q_count's, q_write's, e_paint's and s_partial's bodies with rule L1 behind the planes' test.
// The polygon lies in the caller's scratch where the footprint's would, in FootEdge's layout, and is staged in LDS once per workgroup; all lanes
// then read the same edge in the same iteration (a broadcast read).  The rules themselves in lasso_rules.hpp: fp64 from the fp32 inputs, every
// sum in the order the header states, no fused multiply-add, no division — OctreeExport.crop(lasso=) reproduces every decision bit for bit.
static_assert(sizeof(LassoEdge) == sizeof(FootEdge) && SIMLOD_LASSO_MAX_VERTICES == SIMLOD_FOOTPRINT_MAX_VERTICES, "the lasso's polygon fits the footprint's block");

struct LassoGeom {
	double   rows[3][4];                // rowU, rowV, rowW
	uint64_t edges;                     // offset of LassoEdge[n] in the scratch buffer
	uint32_t n, pad;
};
struct LassoArgs {
	QueryArgs q;
	LassoGeom l;
};
struct LassoPaintArgs   { LassoArgs f; PaintOp p; };
struct LassoSummaryArgs { LassoArgs f; SummaryOp s; };

__device__ __forceinline__ const QueryArgs& query_of(const LassoArgs& la) { return la.q; }
__device__ __forceinline__ const QueryArgs& query_of(const LassoPaintArgs& pa) { return pa.f.q; }
__device__ __forceinline__ const QueryArgs& query_of(const LassoSummaryArgs& sa) { return sa.f.q; }

// the polygon from the scratch buffer into LDS (any block size); the barrier is the caller's
__device__ __forceinline__ void stage_edges(const LassoArgs& la, LassoEdge* sh) {
	const LassoEdge* e = reinterpret_cast<const LassoEdge*>(la.q.x.scratch + la.l.edges);
	for (uint32_t i = threadIdx.x; i < la.l.n; i += blockDim.x) sh[i] = e[i];
}

// what the lasso's kernels ask of a sample behind the planes: (U, V, W) of the sample, then rule L1
struct Lasso {
	const LassoGeom& l;
	const LassoEdge* sh;
	__device__ __forceinline__ bool operator()(const u32x4& p) const {
		const double x = (double)__uint_as_float(p.x), y = (double)__uint_as_float(p.y), z = (double)__uint_as_float(p.z);
		return lasso_inside(sh, l.n, lasso_row(l.rows[0], x, y, z), lasso_row(l.rows[1], x, y, z), lasso_row(l.rows[2], x, y, z));
	}
};

__global__ __launch_bounds__(WG_TPB) void k_l_hier(LassoArgs la) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	const ExportArgs& a = la.q.x;
	uint32_t* cls = reinterpret_cast<uint32_t*>(a.scratch + la.q.cls);
	stage_edges(la, sh_edges);
	__syncthreads();
	hier_walk<true>(a, [&](uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
		// outside by either; copied iff copied by both; else filtered
		const uint32_t p = classify(la.q.g, level, X, Y, Z);
		if (p == Q_OUTSIDE) return (uint32_t)Q_OUTSIDE;
		const uint32_t c = classify_lasso(la.q.g.min, la.q.g.size, la.l.rows, sh_edges, la.l.n, level, X, Y, Z);
		return c == LASSO_NODE_OUTSIDE ? (uint32_t)Q_OUTSIDE : (p == Q_COPIED && c == LASSO_NODE_COPIED) ? (uint32_t)Q_COPIED : (uint32_t)Q_FILTERED;
	}, cls);
	__syncthreads();
	query_totals(a, cls, sh_scan);
}
static_assert(LASSO_NODE_OUTSIDE == Q_OUTSIDE && LASSO_NODE_FILTERED == Q_FILTERED && LASSO_NODE_COPIED == Q_COPIED, "lasso_rules.hpp: the classes");

__global__ __launch_bounds__(LANE_TPB) void k_l_count(LassoArgs la) {
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	stage_edges(la, sh_edges);
	__syncthreads();
	q_count<const LassoArgs&>(la, Lasso{la.l, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_l_write(LassoArgs la) {
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	stage_edges(la, sh_edges);
	__syncthreads();
	q_write<const LassoArgs&>(la, Lasso{la.l, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_el_paint(LassoPaintArgs pa) {
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	stage_edges(pa.f, sh_edges);
	__syncthreads();
	e_paint<LassoPaintArgs>(pa, Lasso{pa.f.l, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_ls_partial(LassoSummaryArgs sa) {
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	stage_edges(sa.f, sh_edges);
	__syncthreads();
	s_partial<LassoSummaryArgs>(sa, Lasso{sa.f.l, sh_edges});
}
