// export_inverse.inc — part of export.hip: inverse selections.  k_iq_hier, k_if_hier, k_il_hier, and the inverse instances of q_count, q_write,
// e_paint and s_partial for the planes, the footprint and the lasso.
// ---- inverse selections -------------------------------------------------------------------------------------------------------------------
// simlod_query_inverse / simlod_paint_inverse / simlod_query_summary_inverse (simlod_hip.h, "inverse selections"): the region's, the footprint's
// or the lasso's launches with every verdict turned round.
//   k_iq_hier, k_if_hier, k_il_hier   the walk WITHOUT the culling (hier_walk<WALK_INVERSE>: no child is asked, every node is listed, as
//              k_x_hier lists them), the class of an entry from the positive classifiers as k_q_hier / k_f_hier / k_l_hier combine them, mapped
//              last by rule I2 (inverse_rules.hpp): outside -> copied, copied -> emptied, filtered stays.  An emptied entry keeps its place in
//              the table with numSamples 0, so k_q_dir makes no item for it and query_totals counts it nowhere.  One classification per node
//              where the positive walk has nine (the node's own and its eight children's).
//   k_q_dir, k_q_scan, k_s_final   as they are.
//   k_i*_count, k_i*_write, k_ie*_paint, k_i*s_partial   q_count's, q_write's, e_paint's and s_partial's bodies with INVERT set: a sample of a
//              filtered chunk is taken iff it FAILS passes(planes) && extra(polygon) — the same fp64 operations in the same order, the verdict
//              negated under the same k < count guard.  A copied chunk (a node the positive query culls) goes through copy_chunk, and a SET
//              paint without `previous` stores to it without a load, as for a copied chunk of the positive calls.
// The argument blocks are the positive kernels' (QueryArgs, FootArgs, LassoArgs and their paint and summary blocks), handed on whole and in the
// same way as there.
static_assert(INVERSE_NODE_OUTSIDE == Q_OUTSIDE && INVERSE_NODE_FILTERED == Q_FILTERED && INVERSE_NODE_COPIED == Q_COPIED && INVERSE_NODE_EMPTIED == Q_EMPTIED,
              "inverse_rules.hpp: the classes");

// rule F4 / L4 as k_f_hier / k_l_hier combine the planes' class with the polygon's: outside by either; copied iff copied by both; else filtered
__device__ __forceinline__ uint32_t combine_classes(uint32_t planes, uint32_t polygon) {
	return polygon == Q_OUTSIDE ? (uint32_t)Q_OUTSIDE : (planes == Q_COPIED && polygon == Q_COPIED) ? (uint32_t)Q_COPIED : (uint32_t)Q_FILTERED;
}

__global__ __launch_bounds__(WG_TPB) void k_iq_hier(QueryArgs q) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const ExportArgs& a = q.x;
	uint32_t* cls = reinterpret_cast<uint32_t*>(a.scratch + q.cls);
	hier_walk<WALK_INVERSE>(a, [&](uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) { return inverse_class(classify(q.g, level, X, Y, Z)); }, cls);
	__syncthreads();
	query_totals(a, cls, sh_scan);
}

__global__ __launch_bounds__(WG_TPB) void k_if_hier(FootArgs fa) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	const ExportArgs& a = fa.q.x;
	uint32_t* cls = reinterpret_cast<uint32_t*>(a.scratch + fa.q.cls);
	stage_edges(fa, sh_edges);
	__syncthreads();
	hier_walk<WALK_INVERSE>(a, [&](uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
		const uint32_t p = classify(fa.q.g, level, X, Y, Z);
		if (p == Q_OUTSIDE) return inverse_class(Q_OUTSIDE);
		return inverse_class(combine_classes(p, classify_footprint(fa.q.g, fa.f, sh_edges, level, X, Y, Z)));
	}, cls);
	__syncthreads();
	query_totals(a, cls, sh_scan);
}

__global__ __launch_bounds__(WG_TPB) void k_il_hier(LassoArgs la) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	const ExportArgs& a = la.q.x;
	uint32_t* cls = reinterpret_cast<uint32_t*>(a.scratch + la.q.cls);
	stage_edges(la, sh_edges);
	__syncthreads();
	hier_walk<WALK_INVERSE>(a, [&](uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
		const uint32_t p = classify(la.q.g, level, X, Y, Z);
		if (p == Q_OUTSIDE) return inverse_class(Q_OUTSIDE);
		return inverse_class(combine_classes(p, classify_lasso(la.q.g.min, la.q.g.size, la.l.rows, sh_edges, la.l.n, level, X, Y, Z)));
	}, cls);
	__syncthreads();
	query_totals(a, cls, sh_scan);
}

// ---- the planes alone ----
__global__ __launch_bounds__(LANE_TPB) void k_iq_count(QueryArgs q) { q_count<const QueryArgs&, true>(q, NoFootprint()); }
__global__ __launch_bounds__(LANE_TPB) void k_iq_write(QueryArgs q) { q_write<const QueryArgs, true>(q, NoFootprint()); }
__global__ __launch_bounds__(LANE_TPB) void k_ie_paint(PaintArgs pa) { e_paint<PaintArgs, true>(pa, NoFootprint()); }
__global__ __launch_bounds__(LANE_TPB) void k_is_partial(SummaryArgs sa) { s_partial<SummaryArgs, true>(sa, NoFootprint()); }

// ---- a footprint on top ----
__global__ __launch_bounds__(LANE_TPB) void k_if_count(FootArgs fa) {
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	stage_edges(fa, sh_edges);
	__syncthreads();
	q_count<const FootArgs&, true>(fa, Footprint{fa.f, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_if_write(FootArgs fa) {
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	stage_edges(fa, sh_edges);
	__syncthreads();
	q_write<const FootArgs&, true>(fa, Footprint{fa.f, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_ief_paint(FootPaintArgs pa) {
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	stage_edges(pa.f, sh_edges);
	__syncthreads();
	e_paint<FootPaintArgs, true>(pa, Footprint{pa.f.f, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_ifs_partial(FootSummaryArgs sa) {
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	stage_edges(sa.f, sh_edges);
	__syncthreads();
	s_partial<FootSummaryArgs, true>(sa, Footprint{sa.f.f, sh_edges});
}

// ---- a lasso on top ----
__global__ __launch_bounds__(LANE_TPB) void k_il_count(LassoArgs la) {
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	stage_edges(la, sh_edges);
	__syncthreads();
	q_count<const LassoArgs&, true>(la, Lasso{la.l, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_il_write(LassoArgs la) {
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	stage_edges(la, sh_edges);
	__syncthreads();
	q_write<const LassoArgs&, true>(la, Lasso{la.l, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_iel_paint(LassoPaintArgs pa) {
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	stage_edges(pa.f, sh_edges);
	__syncthreads();
	e_paint<LassoPaintArgs, true>(pa, Lasso{pa.f.l, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_ils_partial(LassoSummaryArgs sa) {
	__shared__ LassoEdge sh_edges[SIMLOD_LASSO_MAX_VERTICES];
	stage_edges(sa.f, sh_edges);
	__syncthreads();
	s_partial<LassoSummaryArgs, true>(sa, Lasso{sa.f.l, sh_edges});
}
