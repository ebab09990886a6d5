// export.hip — octree export / import (include/simlod_hip.h, "octree export / import"; no counterpart in the reference).
//
// Export: four launches on the caller's stream.
//   k_x_hier   ONE workgroup: the breadth-first walk, level by level (at most 21 levels, none past maxLevel).  Per level one lane per node:
//              the node's child mask from its non-null children, a workgroup exclusive scan of the popcounts gives the children's table
//              indices, the lane writes its table entry (everything but firstSample) and its children's source indices.  Config 2 has
//              4 425 nodes: five rounds of 1 024 lanes in all; no grid-wide barrier.
//   k_x_scan   ONE workgroup: exclusive scans of numSamples (-> firstSample) and of the chunks per node (-> the node's first copy item);
//              the capacity check of the samples; SimlodExportCounts.
//   k_x_dir    one lane per table entry: the node's chunk addresses — the first <= 50 from the builder's chunk table while that is valid
//              (the stamp check r_visible does, render.hip), the rest (or all) by `next` — as copy items {source, destination, count}.
//   k_copy     the hot path: one workgroup per chunk at a time (grid-stride), 16-byte loads and stores, four per lane in flight.
// Import: k_i_validate (ONE workgroup: every check, the scans, the Stats counts) -> k_i_nodes (one lane per node: Node record, the chunk
// headers of its list, its copy items) -> k_copy (the same kernel, samples -> chunks) -> k_i_finish (allocator header, Stats).
// The buildable import (simlod_import_octree_buildable): the same four kernels — the validation with the buildability checks, the Node records
// with grid pointers — and, between k_copy and k_i_finish, the occupancy grids rebuilt from the samples: k_i_gleaf, k_i_gdown per level,
// k_i_groot (export_grids.inc); k_i_finish then also writes the builder's counters as k_reset does.
// Region query (simlod_query_region): k_q_hier -> k_q_dir -> k_q_count -> k_q_scan -> k_q_write, described in export_region.inc.
// Footprint query (simlod_query_footprint): k_f_hier -> k_q_dir -> k_f_count -> k_q_scan -> k_f_write, the region query's sequence with an extruded
// polygon on top of the planes, in export_footprint.inc.
// Paint (simlod_paint_region): that sequence as a count-only call, then k_e_paint / k_ef_paint, which write colour words into the octree's own
// chunks, in export_paint.inc; the rules in paint_rules.hpp.
// Summary (simlod_query_summary): that sequence as a count-only call, then k_s_partial / k_fs_partial and k_s_final, which reduce the selected
// samples to one SimlodSummary record, in export_summary.inc; the rules in summary_rules.hpp.
// Lasso query, paint and summary (simlod_query_lasso, simlod_paint_lasso, simlod_query_summary_lasso): the footprint's sequences with a polygon on
// the screen of a perspective camera in the extruded polygon's place — k_l_hier, k_l_count, k_l_write, k_el_paint, k_ls_partial — in
// export_lasso.inc; the rules themselves in lasso_rules.hpp.
// Inverse selections (simlod_query_inverse, simlod_paint_inverse, simlod_query_summary_inverse): the region's, the footprint's or the lasso's
// sequences with every verdict turned round — k_iq_hier / k_if_hier / k_il_hier, which list every node as k_x_hier does, and the inverse instances
// of the per-sample kernels — in export_inverse.inc; the rules themselves in inverse_rules.hpp.
// Profile query (simlod_query_profile): k_pr_hier -> k_q_dir -> k_pr_count -> k_q_scan -> k_pr_write, the same sequence with a corridor along a
// polyline on top of the planes and a record per returned sample, in export_profile.inc; the rules themselves in profile_rules.hpp.
// View query (simlod_query_view): k_v_hier -> k_v_scan -> k_x_dir -> k_copy, the export's sequence with the camera's rules in the walk, in
// export_view.inc; the rules themselves in view_rules.hpp.
// View delta (simlod_query_view_delta): k_v_hier -> k_v_scan -> k_d_match -> k_d_scan -> k_d_dir -> k_copy -> k_d_drop; its merge
// (simlod_merge_view_delta): k_d_merge_scan -> k_d_merge_dir -> k_copy, in export_delta.inc; the rules in delta_rules.hpp.
// Packed samples (simlod_pack_samples / simlod_unpack_samples): k_pk_scan -> k_pk_dir -> k_pk_pack / k_pk_unpack, in export_pack.inc; the rules
// in pack_rules.hpp.  They read a table and a sample array, no octree.
// Pair queries: k_p_hier -> k_q_dir -> k_p_pairs<Q, count> -> k_p_scan<Q> -> k_p_pairs<Q, fill> -> Q's test kernel -> Q's reduce kernel; the pipeline
// is written once over a query trait Q, in export_pairs.inc.  Ray query (simlod_query_rays): RayQuery, k_r_test, k_r_reduce, in export_rays.inc.
// Neighbour query (simlod_query_neighbours): NbQuery, k_n_test, k_n_reduce, in export_neighbours.inc.
// Everything in between lives in the caller's scratch buffer (export_min_bytes), never in kernel_construct's momentary buffer: the builder's
// recycle stack and the chunk table export reads are there.
// One translation unit: the device code lies in export_*.inc, the host side — the scratch bounds and the launchers — here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "simlod_device.hpp"
#include "simlod_hip.h"
#include "simlod_internal.hpp"
#include "view_rules.hpp"
#include "delta_rules.hpp"
#include "profile_rules.hpp"
#include "pack_rules.hpp"
#include "paint_rules.hpp"
#include "summary_rules.hpp"
#include "lasso_rules.hpp"
#include "inverse_rules.hpp"

namespace simlod {
namespace {

// The device code, family by family (textual parts of THIS translation unit; each names what it holds in its first line):
#include "export_common.inc"   // constants, Header, Layout, block_scan, ExportArgs, leaf_rows_valid, scan_table, load_chunk4, copy_chunk, k_copy
#include "export_table.inc"    // hier_walk, k_x_hier, k_x_scan, k_x_dir
#include "export_region.inc"   // QueryGeom, classify, QItem, QueryLayout, QueryArgs, k_q_hier, k_q_dir, k_q_count, k_q_scan, k_q_write
#include "export_footprint.inc"  // FootEdge, FootGeom, FootArgs, stage_edges, Footprint, classify_footprint, k_f_hier, k_f_count, k_f_write
#include "export_paint.inc"    // PaintOp, PaintArgs, FootPaintArgs, paint_colour, e_paint, k_e_paint, k_ef_paint
#include "export_summary.inc"  // SummaryPart, SummaryOp, SummaryArgs, FootSummaryArgs, hist_add, s_partial, k_s_partial, k_fs_partial, k_s_final
#include "export_lasso.inc"    // LassoGeom, LassoArgs, LassoPaintArgs, LassoSummaryArgs, Lasso, k_l_hier, k_l_count, k_l_write, k_el_paint, k_ls_partial
#include "export_inverse.inc"  // k_iq_hier, k_if_hier, k_il_hier, the inverse instances of q_count, q_write, e_paint and s_partial
#include "export_profile.inc"  // ProfGeom, ProfArgs, stage_segments, Profile, k_pr_hier, k_pr_count, locate_record, k_pr_write
#include "export_view.inc"     // ViewArgs, k_v_hier, k_v_scan
#include "export_delta.inc"    // DeltaLayout, DeltaArgs, k_d_match, k_d_scan, k_d_dir, k_d_drop, MergeArgs, k_d_merge_scan, k_d_merge_dir
#include "export_pack.inc"     // PackItem, PackLayout, PackArgs, k_pk_scan, k_pk_dir, pack_reduce, k_pk_pack, k_pk_unpack
#include "export_pairs.inc"    // the pair records, PairLayout, PairArgs, k_p_hier, wave_descend, k_p_pairs, k_p_scan, TestView, test_chunk
#include "export_rays.inc"     // RayArgs, ray_load, slab, sample_t, RayQuery, k_r_test, k_r_reduce
#include "export_neighbours.inc"  // NbArgs, sphere_load, sphere_cube, sphere_d2, NbQuery, k_n_test, k_n_reduce
#include "export_import.inc"   // ImportArgs, link_chunk_list, k_i_validate, k_i_nodes, k_i_finish
#include "export_grids.inc"    // the buildable import's grids: k_i_gleaf, k_i_gdown, k_i_groot

uint32_t copy_grid(uint64_t itemCap) {
	const uint64_t g = (uint64_t)device_info().numCUs * 8u;                 // 8 workgroups of 256 lanes per CU
	return (uint32_t)(itemCap < g ? (itemCap == 0u ? 1u : itemCap) : g);
}

// the builder's chunk table of `nodes`, where there is one whose rows k_x_dir / k_q_dir can read (else a.lt stays nullptr: every list is walked)
void bind_leaf_table(Context& ctx, const SimlodNode* nodes, ExportArgs& a) {
	LeafTableRef lt;
	if (!find_leaf_table(ctx, nodes, lt) || lt.slots > LEAF_ROW_SLOTS) return;
	a.lt = lt.table; a.ltPers = lt.pers; a.ltMagic = lt.magic; a.ltBatch = lt.batch; a.ltNodes = lt.tableNodes; a.ltSig = lt.sig;
	a.ltMagicValue = lt.magicValue; a.ltSlots = lt.slots; a.ltRows = lt.rows;
}

}  // namespace

uint64_t export_min_bytes(uint32_t nodeCapacity, uint64_t sampleCapacity) { return Layout(nodeCapacity, sampleCapacity).bytes; }

int launch_export(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                  SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity, SimlodExportCounts* counts, hipStream_t stream) {
	if (nodes == nullptr || stats == nullptr || scratch == nullptr || table == nullptr || counts == nullptr || (samples == nullptr && sampleCapacity != 0u))
		return (int)hipErrorInvalidValue;
	if (select > SIMLOD_EXPORT_VISIBLE || scratchBytes < export_min_bytes(tableCapacity, sampleCapacity)) return (int)hipErrorInvalidValue;
	if (select == SIMLOD_EXPORT_VISIBLE && !array_state(ctx, nodes).rendered) return (int)hipErrorInvalidValue;
	ExportArgs a{};
	a.nodes = nodes; a.stats = stats; a.maxLevel = maxLevel; a.select = select; a.cap = tableCapacity;
	a.scratch = reinterpret_cast<uint8_t*>(scratch); a.table = table; a.samples = samples; a.sampleCap = sampleCapacity; a.counts = counts;
	a.lay = Layout(tableCapacity, sampleCapacity);
	bind_leaf_table(ctx, nodes, a);
	SIMLOD_LAUNCH(k_x_hier, dim3(1), dim3(WG_TPB), stream, a);
	SIMLOD_LAUNCH(k_x_scan, dim3(1), dim3(WG_TPB), stream, a);
	if (tableCapacity != 0u) SIMLOD_LAUNCH(k_x_dir, dim3((tableCapacity + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, a);
	SIMLOD_LAUNCH(k_copy, dim3(copy_grid(a.lay.itemCap)), dim3(LANE_TPB), stream, (const uint8_t*)a.scratch, a.lay.items);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t query_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound) {
	return QueryLayout(nodeCapacity).x.items + (sampleBound / SIMLOD_POINTS_PER_CHUNK + nodeCapacity + 1u) * sizeof(QItem);
}

namespace {

// What the region and the footprint query share in front of their launches: the checks of simlod_query_region and the kernels' arguments.
// `frontBytes` of the scratch buffer are kept free in front of the items (the footprint's polygon; 0: the region query's layout).
int prepare_query(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region, uint32_t maxLevel,
                  uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples,
                  uint64_t sampleCapacity, SimlodQueryCounts* counts, uint64_t frontBytes, QueryArgs& q) {
	if (nodes == nullptr || stats == nullptr || u == nullptr || region == nullptr || scratch == nullptr || table == nullptr || counts == nullptr)
		return (int)hipErrorInvalidValue;
	if (region->numPlanes > SIMLOD_REGION_MAX_PLANES || region->reserved[0] != 0u || region->reserved[1] != 0u || region->reserved[2] != 0u)
		return (int)hipErrorInvalidValue;
	if ((select != SIMLOD_EXPORT_ALL && select != SIMLOD_EXPORT_CUT) || scratchBytes < query_min_bytes(tableCapacity, 0u) + frontBytes) return (int)hipErrorInvalidValue;
	for (uint32_t p = 0; p < region->numPlanes; p++)
		for (int k = 0; k < 4; k++) {
			if (!std::isfinite(region->planes[p][k])) return (int)hipErrorInvalidValue;
			q.g.pl[p][k] = (double)region->planes[p][k];
		}
	q.g.numPlanes = region->numPlanes;
	float size, minx, miny, minz;
	octree_box(u, size, minx, miny, minz);                                      // voxels.cu:860-863
	q.g.size = (double)size; q.g.min[0] = (double)minx; q.g.min[1] = (double)miny; q.g.min[2] = (double)minz;
	ExportArgs& a = q.x;
	a.nodes = nodes; a.stats = stats; a.maxLevel = maxLevel; a.select = select; a.cap = tableCapacity;
	a.scratch = reinterpret_cast<uint8_t*>(scratch); a.table = table; a.samples = samples; a.sampleCap = sampleCapacity;
	const QueryLayout ql(tableCapacity);
	a.lay = ql.x; a.lay.items += frontBytes; a.lay.take_rest(scratchBytes);
	q.cls = ql.cls;
	q.counts = counts;
	bind_leaf_table(ctx, nodes, a);
	return 0;
}

// The selection every call of the family starts with, on `stream`: hier -> k_q_dir -> count -> k_q_scan.  `k_hier` and `k_count` are the region
// query's, the footprint's or the lasso's and take `args`; k_q_dir and k_q_scan take the QueryArgs `q` in it.  (A macro: SIMLOD_LAUNCH names
// the kernel it launches.)
#define SIMLOD_LAUNCH_SELECTION(k_hier, k_count, args, q, tableCapacity, grid, stream)                                           \
	do {                                                                                                                         \
		constexpr uint32_t perWg = LANE_TPB / SIMLOD_WAVE; /* k_q_dir: one wave per table entry */                                \
		SIMLOD_LAUNCH(k_hier, dim3(1), dim3(WG_TPB), stream, args);                                                              \
		if ((tableCapacity) != 0u) SIMLOD_LAUNCH(k_q_dir, dim3(((tableCapacity) + perWg - 1u) / perWg), dim3(LANE_TPB), stream, q); \
		SIMLOD_LAUNCH(k_count, dim3(grid), dim3(LANE_TPB), stream, args);                                                        \
		SIMLOD_LAUNCH(k_q_scan, dim3(1), dim3(WG_TPB), stream, q);                                                               \
	} while (0)

// A polygon on top of the planes — a footprint's or a lasso's: its edges widened to fp64 on the host, and where they go.  Both kinds use
// FootEdge's layout and the same 8 KB block of the scratch buffer, filled by the same copy on the caller's stream.
struct PolygonEdges {
	union {
		FootEdge  foot[SIMLOD_FOOTPRINT_MAX_VERTICES];
		LassoEdge lasso[SIMLOD_LASSO_MAX_VERTICES];
	};
	uint32_t n = 0u;
	// into the block that starts `front` bytes in front of the items -> its offset in the scratch buffer
	// (pageable host memory: the runtime has read the edges when the call returns)
	hipError_t upload(const QueryArgs& q, uint64_t front, hipStream_t stream, uint64_t& offset) const {
		offset = q.x.lay.items - front;
		return hipMemcpyAsync(q.x.scratch + offset, foot, (size_t)n * sizeof(FootEdge), hipMemcpyHostToDevice, stream);
	}
};

// Rule F7's refusals of the footprint itself (false), else its axes and its edges widened to fp64.
bool footprint_edges(const SimlodFootprint* fp, FootGeom& f, PolygonEdges& pe) {
	if (fp == nullptr || fp->numVertices < 3u || fp->numVertices > SIMLOD_FOOTPRINT_MAX_VERTICES) return false;
	if (fp->reserved[0] != 0u || fp->reserved[1] != 0u || fp->reserved[2] != 0u) return false;
	const uint32_t n = fp->numVertices;
	for (int k = 0; k < 4; k++) {
		if (!std::isfinite(fp->axisU[k]) || !std::isfinite(fp->axisV[k])) return false;
		f.axU[k] = (double)fp->axisU[k]; f.axV[k] = (double)fp->axisV[k];
	}
	for (uint32_t i = 0; i < n; i++) {
		if (!std::isfinite(fp->vertices[i][0]) || !std::isfinite(fp->vertices[i][1])) return false;
		const uint32_t j = i + 1u == n ? 0u : i + 1u;
		const double au = (double)fp->vertices[i][0], av = (double)fp->vertices[i][1];
		pe.foot[i] = FootEdge{au, av, (double)fp->vertices[j][0] - au, (double)fp->vertices[j][1] - av};
	}
	f.n = pe.n = n;
	return true;
}

// Rule L7's refusals of the lasso itself (false), else its rows and its edges widened to fp64 (lasso_rules.hpp).
bool lasso_edges(const SimlodLasso* ls, LassoGeom& l, PolygonEdges& pe) {
	if (ls == nullptr || !lasso_acceptable(*ls)) return false;
	lasso_widen(*ls, l.rows, pe.lasso);
	l.n = pe.n = ls->numVertices;
	return true;
}

}  // namespace

int launch_query(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region, uint32_t maxLevel,
                 uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples,
                 uint64_t sampleCapacity, SimlodQueryCounts* counts, hipStream_t stream) {
	QueryArgs q{};
	const int rc = prepare_query(ctx, nodes, stats, u, region, maxLevel, select, scratch, scratchBytes, table, tableCapacity, samples, sampleCapacity, counts, 0u, q);
	if (rc != 0) return rc;
	const uint32_t grid = copy_grid(q.x.lay.itemCap);
	SIMLOD_LAUNCH_SELECTION(k_q_hier, k_q_count, q, q, tableCapacity, grid, stream);
	if (samples != nullptr) SIMLOD_LAUNCH(k_q_write, dim3(grid), dim3(LANE_TPB), stream, q);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t footprint_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound) { return query_min_bytes(nodeCapacity, sampleBound) + FOOT_BLOCK_BYTES; }

// simlod_query_footprint with a footprint (without one the entry point forwards to launch_query): the polygon, widened to fp64 edges, goes into
// the scratch buffer's block in front of the items by a copy on `stream`; then the region query's sequence with k_f_hier / k_f_count / k_f_write.
int launch_footprint(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region,
                     const SimlodFootprint* fp, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table,
                     uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity, SimlodQueryCounts* counts, hipStream_t stream) {
	FootArgs fa{};
	PolygonEdges pe;
	if (!footprint_edges(fp, fa.f, pe)) return (int)hipErrorInvalidValue;
	const int rc = prepare_query(ctx, nodes, stats, u, region, maxLevel, select, scratch, scratchBytes, table, tableCapacity, samples, sampleCapacity, counts,
	                             FOOT_BLOCK_BYTES, fa.q);
	if (rc != 0) return rc;
	const hipError_t e = pe.upload(fa.q, FOOT_BLOCK_BYTES, stream, fa.f.edges);
	if (e != hipSuccess) return (int)e;
	const uint32_t grid = copy_grid(fa.q.x.lay.itemCap);
	SIMLOD_LAUNCH_SELECTION(k_f_hier, k_f_count, fa, fa.q, tableCapacity, grid, stream);
	if (samples != nullptr) SIMLOD_LAUNCH(k_f_write, dim3(grid), dim3(LANE_TPB), stream, fa);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

// simlod_query_lasso with a lasso (without one the entry point forwards to launch_query): launch_footprint with the lasso's rows and kernels; the
// polygon lies in the same block.
uint64_t lasso_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound) { return footprint_min_bytes(nodeCapacity, sampleBound); }

int launch_lasso(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region,
                 const SimlodLasso* lasso, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table,
                 uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity, SimlodQueryCounts* counts, hipStream_t stream) {
	LassoArgs la{};
	PolygonEdges pe;
	if (!lasso_edges(lasso, la.l, pe)) return (int)hipErrorInvalidValue;
	const int rc = prepare_query(ctx, nodes, stats, u, region, maxLevel, select, scratch, scratchBytes, table, tableCapacity, samples, sampleCapacity, counts,
	                             FOOT_BLOCK_BYTES, la.q);
	if (rc != 0) return rc;
	const hipError_t e = pe.upload(la.q, FOOT_BLOCK_BYTES, stream, la.l.edges);
	if (e != hipSuccess) return (int)e;
	const uint32_t grid = copy_grid(la.q.x.lay.itemCap);
	SIMLOD_LAUNCH_SELECTION(k_l_hier, k_l_count, la, la.q, tableCapacity, grid, stream);
	if (samples != nullptr) SIMLOD_LAUNCH(k_l_write, dim3(grid), dim3(LANE_TPB), stream, la);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

// simlod_query_inverse: the region's, the footprint's or the lasso's launches with the inverse walk and the inverse per-sample kernels.  The
// polygon's block is kept free in front of the items whether there is a polygon or not: one minimum for the three (rule I9).
uint64_t inverse_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound) { return footprint_min_bytes(nodeCapacity, sampleBound); }

int launch_inverse(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region,
                   const SimlodFootprint* fp, const SimlodLasso* lasso, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                   SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity, SimlodQueryCounts* counts, hipStream_t stream) {
	if (!inverse_polygons_acceptable(fp, lasso)) return (int)hipErrorInvalidValue;
	FootGeom fg{};
	LassoGeom lg{};
	PolygonEdges pe;
	if (fp != nullptr && !footprint_edges(fp, fg, pe)) return (int)hipErrorInvalidValue;
	if (lasso != nullptr && !lasso_edges(lasso, lg, pe)) return (int)hipErrorInvalidValue;
	QueryArgs q{};
	const int rc = prepare_query(ctx, nodes, stats, u, region, maxLevel, select, scratch, scratchBytes, table, tableCapacity, samples, sampleCapacity, counts,
	                             FOOT_BLOCK_BYTES, q);
	if (rc != 0) return rc;
	const uint32_t grid = copy_grid(q.x.lay.itemCap);
	if (fp != nullptr) {
		const hipError_t e = pe.upload(q, FOOT_BLOCK_BYTES, stream, fg.edges);
		if (e != hipSuccess) return (int)e;
		const FootArgs fa{q, fg};
		SIMLOD_LAUNCH_SELECTION(k_if_hier, k_if_count, fa, q, tableCapacity, grid, stream);
		if (samples != nullptr) SIMLOD_LAUNCH(k_if_write, dim3(grid), dim3(LANE_TPB), stream, fa);
	} else if (lasso != nullptr) {
		const hipError_t e = pe.upload(q, FOOT_BLOCK_BYTES, stream, lg.edges);
		if (e != hipSuccess) return (int)e;
		const LassoArgs la{q, lg};
		SIMLOD_LAUNCH_SELECTION(k_il_hier, k_il_count, la, q, tableCapacity, grid, stream);
		if (samples != nullptr) SIMLOD_LAUNCH(k_il_write, dim3(grid), dim3(LANE_TPB), stream, la);
	} else {
		SIMLOD_LAUNCH_SELECTION(k_iq_hier, k_iq_count, q, q, tableCapacity, grid, stream);
		if (samples != nullptr) SIMLOD_LAUNCH(k_iq_write, dim3(grid), dim3(LANE_TPB), stream, q);
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

constexpr uint64_t PAINT_BLOCK_BYTES = 256u * sizeof(uint32_t);                     // the ramp's table, in front of the items (behind the polygon's block)

uint64_t paint_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound) { return footprint_min_bytes(nodeCapacity, sampleBound) + PAINT_BLOCK_BYTES; }

// simlod_paint_region / simlod_paint_lasso: the footprint's or the lasso's launches as a count-only call (maxLevel 20, every node selected), the
// polygon and the ramp's table in the scratch buffer's blocks in front of the items, then k_e_paint (no polygon), k_ef_paint or k_el_paint.
// At most one of `fp` and `lasso`.  `inverse` (simlod_paint_inverse): the inverse selection's kernels in their places.
int launch_paint(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region,
                 const SimlodFootprint* fp, const SimlodLasso* lasso, const SimlodPaint* paint, void* scratch, uint64_t scratchBytes, SimlodExportNode* table,
                 uint32_t tableCapacity, const uint32_t* colors, uint32_t* previous, uint64_t colorCapacity, SimlodQueryCounts* counts, hipStream_t stream, bool inverse) {
	if (paint == nullptr || !paint_acceptable(*paint, colors != nullptr) || (fp != nullptr && lasso != nullptr)) return (int)hipErrorInvalidValue;
	FootGeom fg{};
	LassoGeom lg{};
	PolygonEdges pe;
	if (fp != nullptr && !footprint_edges(fp, fg, pe)) return (int)hipErrorInvalidValue;
	if (lasso != nullptr && !lasso_edges(lasso, lg, pe)) return (int)hipErrorInvalidValue;
	constexpr uint64_t front = FOOT_BLOCK_BYTES + PAINT_BLOCK_BYTES;
	QueryArgs q{};
	const int rc = prepare_query(ctx, nodes, stats, u, region, SIMLOD_MAX_DEPTH, SIMLOD_EXPORT_ALL, scratch, scratchBytes, table, tableCapacity, nullptr, 0u,
	                             counts, front, q);
	if (rc != 0) return rc;
	PaintOp p{};
	p.mode = paint->mode; p.color = paint->color; p.strength = paint->strength; p.z0 = paint->z0; p.scale = paint->scale;
	p.table = q.x.lay.items - PAINT_BLOCK_BYTES;
	p.colors = paint->mode == SIMLOD_PAINT_ARRAY ? colors : nullptr;
	p.previous = previous; p.colorCap = colorCapacity; p.checkCap = (colors != nullptr || previous != nullptr) ? 1u : 0u;
	// (pageable host memory: the runtime has read `paint` and the edges when the calls return)
	if (paint->mode == SIMLOD_PAINT_RAMP) {
		const hipError_t e = hipMemcpyAsync(q.x.scratch + p.table, paint->table, PAINT_BLOCK_BYTES, hipMemcpyHostToDevice, stream);
		if (e != hipSuccess) return (int)e;
	}
	const uint32_t grid = copy_grid(q.x.lay.itemCap);
	if (fp != nullptr) {
		const hipError_t e = pe.upload(q, front, stream, fg.edges);
		if (e != hipSuccess) return (int)e;
		const FootPaintArgs fa{{q, fg}, p};
		if (inverse) {
			SIMLOD_LAUNCH_SELECTION(k_if_hier, k_if_count, fa.f, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_ief_paint, dim3(grid), dim3(LANE_TPB), stream, fa);
		} else {
			SIMLOD_LAUNCH_SELECTION(k_f_hier, k_f_count, fa.f, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_ef_paint, dim3(grid), dim3(LANE_TPB), stream, fa);
		}
	} else if (lasso != nullptr) {
		const hipError_t e = pe.upload(q, front, stream, lg.edges);
		if (e != hipSuccess) return (int)e;
		const LassoPaintArgs la{{q, lg}, p};
		if (inverse) {
			SIMLOD_LAUNCH_SELECTION(k_il_hier, k_il_count, la.f, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_iel_paint, dim3(grid), dim3(LANE_TPB), stream, la);
		} else {
			SIMLOD_LAUNCH_SELECTION(k_l_hier, k_l_count, la.f, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_el_paint, dim3(grid), dim3(LANE_TPB), stream, la);
		}
	} else {
		const PaintArgs pa{q, p};
		if (inverse) {
			SIMLOD_LAUNCH_SELECTION(k_iq_hier, k_iq_count, q, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_ie_paint, dim3(grid), dim3(LANE_TPB), stream, pa);
		} else {
			SIMLOD_LAUNCH_SELECTION(k_q_hier, k_q_count, q, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_e_paint, dim3(grid), dim3(LANE_TPB), stream, pa);
		}
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t summary_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound) { return footprint_min_bytes(nodeCapacity, sampleBound) + SUMMARY_BLOCK_BYTES; }

namespace {

// k_s_partial's grid: four workgroups of 256 lanes per CU (the kernel is bound by its arithmetic from there on: DESIGN §11 has the times by
// grid), SUMMARY_MAX_PARTS at most (the scratch buffer's block holds that many parts), no more than the buffer can hold items, and no more
// than the caller allows (0: no limit of the caller's)
uint32_t summary_grid(uint64_t itemCap, uint32_t maxWorkgroups) {
	uint64_t g = std::min<uint64_t>((uint64_t)device_info().numCUs * 4u, SUMMARY_MAX_PARTS);
	g = std::min<uint64_t>(g, itemCap == 0u ? 1u : itemCap);
	if (maxWorkgroups != 0u) g = std::min<uint64_t>(g, maxWorkgroups);
	return (uint32_t)std::max<uint64_t>(g, 1u);
}

}  // namespace

// simlod_query_summary / simlod_query_summary_lasso: the footprint's or the lasso's launches as a count-only call with the caller's maxLevel and
// select, the polygon and the partial records in the scratch buffer's blocks in front of the items, then k_s_partial (no polygon), k_fs_partial or
// k_ls_partial, then k_s_final.  At most one of `fp` and `lasso`.  `inverse` (simlod_query_summary_inverse): the inverse selection's kernels in
// their places.
int launch_summary(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region,
                   const SimlodFootprint* fp, const SimlodLasso* lasso, const SimlodSummaryParams* params, uint32_t maxLevel, uint32_t select, void* scratch,
                   uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, SimlodSummary* summary, SimlodQueryCounts* counts, hipStream_t stream,
                   bool inverse) {
	if (params == nullptr || summary == nullptr || !summary_acceptable(*params) || (reinterpret_cast<uintptr_t>(summary) & 7u) != 0u) return (int)hipErrorInvalidValue;
	if (fp != nullptr && lasso != nullptr) return (int)hipErrorInvalidValue;
	FootGeom fg{};
	LassoGeom lg{};
	PolygonEdges pe;
	if (fp != nullptr && !footprint_edges(fp, fg, pe)) return (int)hipErrorInvalidValue;
	if (lasso != nullptr && !lasso_edges(lasso, lg, pe)) return (int)hipErrorInvalidValue;
	constexpr uint64_t front = FOOT_BLOCK_BYTES + SUMMARY_BLOCK_BYTES;
	QueryArgs q{};
	const int rc = prepare_query(ctx, nodes, stats, u, region, maxLevel, select, scratch, scratchBytes, table, tableCapacity, nullptr, 0u, counts, front, q);
	if (rc != 0) return rc;
	SummaryOp s{};
	s.inv = summary_inv((float)q.g.size); s.z0 = params->z0; s.scale = params->scale;
	s.parts = q.x.lay.items - SUMMARY_BLOCK_BYTES;
	const uint32_t grid = copy_grid(q.x.lay.itemCap), sgrid = summary_grid(q.x.lay.itemCap, params->maxWorkgroups);
	const SummaryFinalArgs fin{q.x.scratch, s.parts, sgrid, 0u, counts, summary};
	// (pageable host memory: the runtime has read the edges when the call returns)
	if (fp != nullptr) {
		const hipError_t e = pe.upload(q, front, stream, fg.edges);
		if (e != hipSuccess) return (int)e;
		const FootSummaryArgs fa{{q, fg}, s};
		if (inverse) {
			SIMLOD_LAUNCH_SELECTION(k_if_hier, k_if_count, fa.f, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_ifs_partial, dim3(sgrid), dim3(LANE_TPB), stream, fa);
		} else {
			SIMLOD_LAUNCH_SELECTION(k_f_hier, k_f_count, fa.f, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_fs_partial, dim3(sgrid), dim3(LANE_TPB), stream, fa);
		}
	} else if (lasso != nullptr) {
		const hipError_t e = pe.upload(q, front, stream, lg.edges);
		if (e != hipSuccess) return (int)e;
		const LassoSummaryArgs la{{q, lg}, s};
		if (inverse) {
			SIMLOD_LAUNCH_SELECTION(k_il_hier, k_il_count, la.f, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_ils_partial, dim3(sgrid), dim3(LANE_TPB), stream, la);
		} else {
			SIMLOD_LAUNCH_SELECTION(k_l_hier, k_l_count, la.f, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_ls_partial, dim3(sgrid), dim3(LANE_TPB), stream, la);
		}
	} else {
		const SummaryArgs sa{q, s};
		if (inverse) {
			SIMLOD_LAUNCH_SELECTION(k_iq_hier, k_iq_count, q, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_is_partial, dim3(sgrid), dim3(LANE_TPB), stream, sa);
		} else {
			SIMLOD_LAUNCH_SELECTION(k_q_hier, k_q_count, q, q, tableCapacity, grid, stream);
			SIMLOD_LAUNCH(k_s_partial, dim3(sgrid), dim3(LANE_TPB), stream, sa);
		}
	}
	SIMLOD_LAUNCH(k_s_final, dim3(SUMMARY_FINAL_HIST_WGS + 1u), dim3(WG_TPB), stream, fin);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t profile_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound) { return query_min_bytes(nodeCapacity, sampleBound) + PROFILE_BLOCK_BYTES; }

// simlod_query_profile with a profile (without one the entry point forwards to launch_query): the segments of rule P0 go into the scratch
// buffer's block in front of the items by a copy on `stream`; then the region query's sequence with k_pr_hier / k_pr_count / k_pr_write.
int launch_profile(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region,
                   const SimlodProfile* pf, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table,
                   uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity, SimlodProfileSample* records, SimlodQueryCounts* counts,
                   hipStream_t stream) {
	if (pf == nullptr || !profile_acceptable(*pf) || (records != nullptr && samples == nullptr)) return (int)hipErrorInvalidValue;
	ProfileSegment segs[PROFILE_MAX_SEGMENTS];
	if (!profile_segments(*pf, segs)) return (int)hipErrorInvalidValue;
	ProfArgs pa{};
	for (int k = 0; k < 4; k++) { pa.f.axU[k] = (double)pf->axisU[k]; pa.f.axV[k] = (double)pf->axisV[k]; pa.f.axH[k] = (double)pf->axisH[k]; }
	const int rc = prepare_query(ctx, nodes, stats, u, region, maxLevel, select, scratch, scratchBytes, table, tableCapacity, samples, sampleCapacity, counts,
	                             PROFILE_BLOCK_BYTES, pa.q);
	if (rc != 0) return rc;
	pa.f.n = pf->numVertices - 1u;
	pa.f.segs = pa.q.x.lay.items - PROFILE_BLOCK_BYTES;
	pa.records = records;
	// (pageable host memory: the runtime has read `segs` when the call returns)
	const hipError_t e = hipMemcpyAsync(pa.q.x.scratch + pa.f.segs, segs, (size_t)pa.f.n * sizeof(ProfileSegment), hipMemcpyHostToDevice, stream);
	if (e != hipSuccess) return (int)e;
	const uint32_t grid = copy_grid(pa.q.x.lay.itemCap);
	SIMLOD_LAUNCH(k_pr_hier, dim3(1), dim3(WG_TPB), stream, pa);
	constexpr uint32_t perWg = LANE_TPB / SIMLOD_WAVE;                        // k_q_dir: one wave per table entry
	if (tableCapacity != 0u) SIMLOD_LAUNCH(k_q_dir, dim3((tableCapacity + perWg - 1u) / perWg), dim3(LANE_TPB), stream, pa.q);
	SIMLOD_LAUNCH(k_pr_count, dim3(grid), dim3(LANE_TPB), stream, pa);
	SIMLOD_LAUNCH(k_q_scan, dim3(1), dim3(WG_TPB), stream, pa.q);
	if (samples != nullptr) SIMLOD_LAUNCH(k_pr_write, dim3(grid), dim3(LANE_TPB), stream, pa);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

// simlod_query_view: the export's launches with k_v_hier / k_v_scan in the place of k_x_hier / k_x_scan.  The scratch buffer is the export's; the
// chunk items take what it has behind the table's part, and the device reports a buffer that holds too few of them.
int launch_view(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodView* view, uint32_t maxLevel,
                void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity,
                SimlodViewCounts* counts, hipStream_t stream) {
	if (nodes == nullptr || stats == nullptr || u == nullptr || view == nullptr || scratch == nullptr || table == nullptr || counts == nullptr)
		return (int)hipErrorInvalidValue;
	if (!view_acceptable(*view, *u) || scratchBytes < export_min_bytes(tableCapacity, 0u)) return (int)hipErrorInvalidValue;
	ViewArgs v{};
	ExportArgs& a = v.x;
	a.nodes = nodes; a.stats = stats; a.maxLevel = maxLevel; a.select = SIMLOD_EXPORT_ALL; a.cap = tableCapacity;   // (the walk lists and selects everything: k_v_hier takes away)
	a.scratch = reinterpret_cast<uint8_t*>(scratch); a.table = table; a.samples = samples; a.sampleCap = samples != nullptr ? sampleCapacity : 0u;
	a.counts = reinterpret_cast<SimlodExportCounts*>(counts);
	a.lay = Layout(tableCapacity, 0u); a.lay.take_rest(scratchBytes);
	if (samples == nullptr) a.lay.itemCap = 0xffffffffull;                      // count only: no item is written, none can be missing
	bind_leaf_table(ctx, nodes, a);
	v.g.m = u->transform_updateBound;
	octree_box(u, v.g.cubeSize, v.g.minx, v.g.miny, v.g.minz);                  // render.cu:1135-1137, as launch_render
	v.g.width = u->width; v.g.height = u->height; v.g.minNodeSize = u->minNodeSize;
	v.flags = view->flags; v.minBias = view->minBias; v.maxBias = view->maxBias; v.budget = view->sampleBudget;
	v.counts = counts;
	SIMLOD_LAUNCH(k_v_hier, dim3(1), dim3(WG_TPB), stream, v);
	SIMLOD_LAUNCH(k_v_scan, dim3(1), dim3(WG_TPB), stream, a);
	if (samples != nullptr) {
		if (tableCapacity != 0u) SIMLOD_LAUNCH(k_x_dir, dim3((tableCapacity + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, a);
		SIMLOD_LAUNCH(k_copy, dim3(copy_grid(a.lay.itemCap)), dim3(LANE_TPB), stream, (const uint8_t*)a.scratch, a.lay.items);
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t view_delta_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound, uint32_t numHeld) {
	return DeltaLayout(nodeCapacity, numHeld).x.items + delta_item_bound(nodeCapacity, sampleBound) * sizeof(CopyItem);
}

// simlod_query_view_delta: the view query's two single-workgroup kernels with the arguments of a count-only call, then the delta's own.
int launch_view_delta(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodView* view, uint32_t maxLevel,
                      const SimlodExportNode* held, uint32_t numHeld, uint32_t deltaFlags, void* scratch, uint64_t scratchBytes, SimlodExportNode* table,
                      uint32_t tableCapacity, SimlodDeltaEntry* entries, SimlodPoint* delta, uint64_t deltaCapacity, uint32_t* dropped,
                      uint32_t droppedCapacity, SimlodDeltaCounts* counts, hipStream_t stream) {
	if (nodes == nullptr || stats == nullptr || u == nullptr || view == nullptr || scratch == nullptr || table == nullptr || entries == nullptr || counts == nullptr)
		return (int)hipErrorInvalidValue;
	if (!view_acceptable(*view, *u) || !delta_acceptable(deltaFlags, held, numHeld, dropped, droppedCapacity)) return (int)hipErrorInvalidValue;
	if (scratchBytes < view_delta_min_bytes(tableCapacity, 0u, numHeld)) return (int)hipErrorInvalidValue;
	const DeltaLayout dl(tableCapacity, numHeld);
	ViewArgs v{};
	ExportArgs& a = v.x;
	a.nodes = nodes; a.stats = stats; a.maxLevel = maxLevel; a.select = SIMLOD_EXPORT_ALL; a.cap = tableCapacity;
	a.scratch = reinterpret_cast<uint8_t*>(scratch); a.table = table; a.samples = nullptr; a.sampleCap = 0u;    // (k_v_scan: a count-only call)
	a.counts = reinterpret_cast<SimlodExportCounts*>(&counts->view);
	a.lay = dl.x; a.lay.take_rest(scratchBytes);
	bind_leaf_table(ctx, nodes, a);
	v.g.m = u->transform_updateBound;
	octree_box(u, v.g.cubeSize, v.g.minx, v.g.miny, v.g.minz);
	v.g.width = u->width; v.g.height = u->height; v.g.minNodeSize = u->minNodeSize;
	v.flags = view->flags; v.minBias = view->minBias; v.maxBias = view->maxBias; v.budget = view->sampleBudget;
	v.counts = &counts->view;
	DeltaArgs d{};
	d.x = a;                                                                    // (the delta's kernels: the items the buffer really has)
	d.held = held; d.numHeld = numHeld; d.deltaFlags = deltaFlags; d.mark = dl.mark; d.entries = entries;
	d.delta = delta; d.deltaCap = delta != nullptr ? deltaCapacity : 0u; d.dropped = dropped; d.droppedCap = droppedCapacity; d.counts = counts;
	a.lay.itemCap = 0xffffffffull;                                              // k_v_scan's items are not written: none can be missing
	SIMLOD_LAUNCH(k_v_hier, dim3(1), dim3(WG_TPB), stream, v);
	SIMLOD_LAUNCH(k_v_scan, dim3(1), dim3(WG_TPB), stream, a);
	if (tableCapacity != 0u) SIMLOD_LAUNCH(k_d_match, dim3((tableCapacity + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, d);
	SIMLOD_LAUNCH(k_d_scan, dim3(1), dim3(WG_TPB), stream, d);
	if (delta != nullptr) {
		constexpr uint32_t perWg = LANE_TPB / SIMLOD_WAVE;                      // k_d_dir: one wave per table entry
		if (tableCapacity != 0u) SIMLOD_LAUNCH(k_d_dir, dim3((tableCapacity + perWg - 1u) / perWg), dim3(LANE_TPB), stream, d);
		SIMLOD_LAUNCH(k_copy, dim3(copy_grid(d.x.lay.itemCap)), dim3(LANE_TPB), stream, (const uint8_t*)d.x.scratch, d.x.lay.items);
	}
	SIMLOD_LAUNCH(k_d_drop, dim3(1), dim3(WG_TPB), stream, d);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

int launch_merge_view_delta(const SimlodExportNode* held, uint32_t numHeld, const SimlodPoint* heldSamples, const SimlodExportNode* table,
                            const SimlodDeltaEntry* entries, uint32_t numNodes, const SimlodPoint* delta, void* scratch, uint64_t scratchBytes,
                            SimlodPoint* samples, uint64_t sampleCapacity, SimlodExportCounts* counts, hipStream_t stream) {
	if (table == nullptr || entries == nullptr || scratch == nullptr || counts == nullptr) return (int)hipErrorInvalidValue;
	if ((held == nullptr && numHeld != 0u) || (samples == nullptr && sampleCapacity != 0u)) return (int)hipErrorInvalidValue;
	if (scratchBytes < view_delta_min_bytes(numNodes, 0u, numHeld)) return (int)hipErrorInvalidValue;
	MergeArgs m{};
	m.held = held; m.numHeld = numHeld; m.n = numNodes; m.heldSamples = heldSamples; m.table = table; m.entries = entries; m.delta = delta;
	m.scratch = reinterpret_cast<uint8_t*>(scratch);
	m.lay = DeltaLayout(numNodes, numHeld).x; m.lay.take_rest(scratchBytes);
	m.samples = samples; m.sampleCap = sampleCapacity; m.counts = counts;
	SIMLOD_LAUNCH(k_d_merge_scan, dim3(1), dim3(WG_TPB), stream, m);
	if (numNodes != 0u) SIMLOD_LAUNCH(k_d_merge_dir, dim3((numNodes + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, m);
	SIMLOD_LAUNCH(k_copy, dim3(copy_grid(m.lay.itemCap)), dim3(LANE_TPB), stream, (const uint8_t*)m.scratch, m.lay.items);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t pack_min_bytes(uint32_t numNodes, uint64_t sampleBound) {
	return PackLayout(numNodes).items + pack_item_bound(numNodes, sampleBound) * sizeof(PackItem);
}

// simlod_pack_samples (unpack false) and simlod_unpack_samples: the checks, then k_pk_scan -> k_pk_dir -> the hot kernel.  The items take what
// the buffer has behind the words per entry; the device reports a buffer that holds too few of them.
int launch_pack(bool unpack, const SimlodUniforms* u, const SimlodExportNode* table, const SimlodDeltaEntry* entries, uint32_t numNodes, const void* in,
                uint64_t sampleCapacity, void* scratch, uint64_t scratchBytes, void* out, SimlodPackCounts* counts, hipStream_t stream) {
	if (u == nullptr || table == nullptr || in == nullptr || scratch == nullptr || out == nullptr || counts == nullptr || numNodes == 0u)
		return (int)hipErrorInvalidValue;
	if (scratchBytes < pack_min_bytes(numNodes, 0u)) return (int)hipErrorInvalidValue;
	PackArgs a{};
	const float mn[3] = {u->boxMin.x, u->boxMin.y, u->boxMin.z}, mx[3] = {u->boxMax.x, u->boxMax.y, u->boxMax.z};
	if (!pack_box(mn, mx, a.box)) return (int)hipErrorInvalidValue;
	const PackLayout pl(numNodes);
	a.table = table; a.entries = entries; a.n = numNodes; a.sampleCap = sampleCapacity; a.scratch = reinterpret_cast<uint8_t*>(scratch);
	a.first = pl.first; a.items = pl.items; a.itemCap = std::min<uint64_t>((scratchBytes - pl.items) / sizeof(PackItem), 0xffffffffull);
	a.in = in; a.out = out; a.counts = counts;
	SIMLOD_LAUNCH(k_pk_scan, dim3(1), dim3(WG_TPB), stream, a);
	SIMLOD_LAUNCH(k_pk_dir, dim3((numNodes + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, a);
	if (unpack) SIMLOD_LAUNCH(k_pk_unpack, dim3(copy_grid(a.itemCap)), dim3(LANE_TPB), stream, a);
	else SIMLOD_LAUNCH(k_pk_pack, dim3(copy_grid(a.itemCap)), dim3(LANE_TPB), stream, a);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

namespace {

// what a pair query (export_pairs.inc) needs for its layout, its chunk items and, behind them, its pairs and their partials of `partBytes` each
uint64_t pairs_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound, uint32_t numQueries, uint64_t partBytes, uint64_t numPairs, uint64_t numCandidates) {
	const uint64_t pairsOff = PairLayout(nodeCapacity, numQueries).x.items + (sampleBound / SIMLOD_POINTS_PER_CHUNK + nodeCapacity + 1u) * sizeof(QItem);
	return pair_need(pairsOff, numPairs, numCandidates, partBytes);
}

// The pair pipeline for query Q after its front end's own checks; `q` comes with Q's own fields set.  results(qGrid, itemGrid): the launches
// of Q's test and reduce kernels.
template <class Q, class Results>
int launch_pairs(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, uint32_t numQueries, uint32_t maxLevel,
                 uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, typename Q::Args& q,
                 hipStream_t stream, Results results) {
	if (nodes == nullptr || stats == nullptr || u == nullptr || scratch == nullptr || select > SIMLOD_EXPORT_VISIBLE) return (int)hipErrorInvalidValue;
	if (scratchBytes < pairs_min_bytes(tableCapacity, 0u, numQueries, Q::part_bytes(q), 0u, 0u)) return (int)hipErrorInvalidValue;
	if (select == SIMLOD_EXPORT_VISIBLE && !array_state(ctx, nodes).rendered) return (int)hipErrorInvalidValue;
	const PairLayout pl(tableCapacity, numQueries);
	PairArgs& p = q.p;
	ExportArgs& a = p.x;
	a.nodes = nodes; a.stats = stats; a.maxLevel = maxLevel; a.select = select; a.cap = tableCapacity;
	a.scratch = reinterpret_cast<uint8_t*>(scratch);
	a.table = table != nullptr ? table : reinterpret_cast<SimlodExportNode*>(a.scratch + pl.tab);
	a.lay = pl.x; a.lay.take_rest(scratchBytes);
	float size, minx, miny, minz;
	octree_box(u, size, minx, miny, minz);                                      // voxels.cu:860-863
	p.size = (double)size; p.min[0] = (double)minx; p.min[1] = (double)miny; p.min[2] = (double)minz;
	p.numQueries = numQueries; p.scratchBytes = scratchBytes; p.at = pl.at;
	bind_leaf_table(ctx, nodes, a);
	QueryArgs d{};                                                              // k_q_dir's view of the same buffers
	d.x = a; d.cls = pl.at.cls;
	const uint32_t qGrid = (numQueries + PAIR_WAVES - 1u) / PAIR_WAVES;
	SIMLOD_LAUNCH(k_p_hier, dim3(1), dim3(WG_TPB), stream, p);
	constexpr uint32_t perWg = LANE_TPB / SIMLOD_WAVE;                          // k_q_dir: one wave per table entry
	if (tableCapacity != 0u) SIMLOD_LAUNCH(k_q_dir, dim3((tableCapacity + perWg - 1u) / perWg), dim3(LANE_TPB), stream, d);
	SIMLOD_LAUNCH((k_p_pairs<Q, 0>), dim3(qGrid), dim3(LANE_TPB), stream, q);
	SIMLOD_LAUNCH(k_p_scan<Q>, dim3(1), dim3(WG_TPB), stream, q);
	if (Q::wants_results(q)) {
		SIMLOD_LAUNCH((k_p_pairs<Q, 1>), dim3(qGrid), dim3(LANE_TPB), stream, q);
		results(qGrid, copy_grid(a.lay.itemCap));
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

}  // namespace

uint64_t rays_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound, uint32_t numRays, uint64_t numPairs, uint64_t numCandidates) {
	return pairs_min_bytes(nodeCapacity, sampleBound, numRays, sizeof(RayPart), numPairs, numCandidates);
}

int launch_rays(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRay* rays, uint32_t numRays,
                uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity,
                SimlodRayHit* hits, SimlodRayCounts* counts, hipStream_t stream) {
	if (rays == nullptr || counts == nullptr || numRays == 0u || numRays > SIMLOD_RAYS_MAX) return (int)hipErrorInvalidValue;
	RayArgs r{};
	r.rays = rays; r.hits = hits; r.counts = counts;
	return launch_pairs<RayQuery>(ctx, nodes, stats, u, numRays, maxLevel, select, scratch, scratchBytes, table, tableCapacity, r, stream,
	                              [&](uint32_t rayGrid, uint32_t itemGrid) {
		SIMLOD_LAUNCH(k_r_test, dim3(itemGrid), dim3(LANE_TPB), stream, r);
		SIMLOD_LAUNCH(k_r_reduce, dim3(rayGrid), dim3(LANE_TPB), stream, r);
	});
}

uint64_t neighbours_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound, uint32_t numQueries, uint32_t k, uint64_t numPairs, uint64_t numCandidates) {
	return pairs_min_bytes(nodeCapacity, sampleBound, numQueries, nb_part_bytes(k), numPairs, numCandidates);
}

int launch_neighbours(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodSphere* queries,
                      uint32_t numQueries, uint32_t k, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table,
                      uint32_t tableCapacity, SimlodNeighbour* neighbours, uint32_t* within, SimlodNeighbourCounts* counts, hipStream_t stream) {
	if (queries == nullptr || counts == nullptr || (within != nullptr && neighbours == nullptr)) return (int)hipErrorInvalidValue;
	if (numQueries == 0u || numQueries > SIMLOD_NEIGHBOURS_MAX || k == 0u || k > SIMLOD_NEIGHBOURS_MAX_K) return (int)hipErrorInvalidValue;
	NbArgs n{};
	n.queries = queries; n.neighbours = neighbours; n.within = within; n.counts = counts; n.k = k;
	return launch_pairs<NbQuery>(ctx, nodes, stats, u, numQueries, maxLevel, select, scratch, scratchBytes, table, tableCapacity, n, stream,
	                             [&](uint32_t qGrid, uint32_t itemGrid) {
		SIMLOD_LAUNCH(k_n_test, dim3(itemGrid), dim3(LANE_TPB), stream, n);
		SIMLOD_LAUNCH(k_n_reduce, dim3(qGrid), dim3(LANE_TPB), stream, n);
	});
}

namespace {

// Both imports (u != nullptr: the buildable one): k_i_validate -> k_i_nodes -> k_copy -> (the grids: k_i_gleaf, k_i_gdown per level, k_i_groot)
// -> k_i_finish.
int run_import(Context& ctx, const SimlodUniforms* u, const SimlodExportNode* table, uint32_t numNodes, const SimlodPoint* samples, uint64_t numSamples,
               void* scratch, uint64_t scratchBytes, uint8_t* pers, uint64_t persCapacity, SimlodNode* nodes, SimlodStats* stats,
               uint32_t* numBatchesUploaded, uint32_t* batchSizes, hipStream_t stream) {
	if (table == nullptr || scratch == nullptr || pers == nullptr || nodes == nullptr || stats == nullptr || (samples == nullptr && numSamples != 0u))
		return (int)hipErrorInvalidValue;
	if (numNodes == 0u || numNodes > ctx.nodeCapacity.load() || scratchBytes < export_min_bytes(numNodes, numSamples)) return (int)hipErrorInvalidValue;
	ImportArgs a{};
	a.table = table; a.n = numNodes; a.samples = samples; a.numSamples = numSamples; a.scratch = reinterpret_cast<uint8_t*>(scratch);
	a.lay = Layout(numNodes, numSamples); a.pers = pers; a.persCap = persCapacity; a.nodes = nodes; a.stats = stats;
	if (u != nullptr) {
		a.buildable = 1u;
		octree_box(u, a.size, a.minx, a.miny, a.minz);                          // voxels.cu:860-863
		a.numBatchesUploaded = numBatchesUploaded; a.batchSizes = batchSizes; a.frameCounter = (uint32_t)u->frameCounter;
		// what launch_reset forgets of this node array's launches and upload counter (the counter is zeroed by k_i_finish, in stream order)
		forget_launch_history(ctx, nodes, numBatchesUploaded, &a.feedback, &a.feedbackSeq);
	}
	SIMLOD_LAUNCH(k_i_validate, dim3(1), dim3(WG_TPB), stream, a);
	SIMLOD_LAUNCH(k_i_nodes, dim3((numNodes + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, a);
	SIMLOD_LAUNCH(k_copy, dim3(copy_grid(a.lay.itemCap)), dim3(LANE_TPB), stream, (const uint8_t*)a.scratch, a.lay.items);
	if (u != nullptr) {
		SIMLOD_LAUNCH(k_i_gleaf, dim3(numNodes), dim3(G_TPB), stream, a);
		// inner nodes lie at levels 0 .. numInner - 1 at most (and below 20): one launch per level that can have any, deepest first
		const uint32_t numInner = (numNodes - 1u) / 8u;
		const uint32_t deepest = std::min<uint32_t>((uint32_t)SIMLOD_MAX_DEPTH - 1u, numInner > 0u ? numInner - 1u : 0u);
		const uint32_t wgs = std::min<uint32_t>(numNodes, device_info().numCUs * 4u);
		for (uint32_t level = deepest; level >= 1u; level--) SIMLOD_LAUNCH(k_i_gdown, dim3(wgs), dim3(G_TPB), stream, a, level);
		SIMLOD_LAUNCH(k_i_groot, dim3(1), dim3(R_TPB), stream, a);
	}
	SIMLOD_LAUNCH(k_i_finish, dim3(1), dim3(1), stream, a);
	if (profile_enabled()) profile_close(stream);
	const int rc = (int)hipGetLastError();
	if (rc != 0) return rc;
	// the builder's side tables and its chunk table describe the octree that was there (simlod_octree_image_replaced)
	octree_image_replaced(ctx, nodes);
	array_event(ctx, nodes, u != nullptr ? ARRAY_IMPORTED_BUILDABLE : ARRAY_IMPORTED);
	return 0;
}

}  // namespace

int launch_import(Context& ctx, const SimlodExportNode* table, uint32_t numNodes, const SimlodPoint* samples, uint64_t numSamples, void* scratch,
                  uint64_t scratchBytes, uint8_t* pers, uint64_t persCapacity, SimlodNode* nodes, SimlodStats* stats, hipStream_t stream) {
	return run_import(ctx, nullptr, table, numNodes, samples, numSamples, scratch, scratchBytes, pers, persCapacity, nodes, stats, nullptr, nullptr, stream);
}

int launch_import_buildable(Context& ctx, const SimlodUniforms* u, const SimlodExportNode* table, uint32_t numNodes, const SimlodPoint* samples,
                            uint64_t numSamples, void* scratch, uint64_t scratchBytes, uint8_t* pers, SimlodNode* nodes, SimlodStats* stats,
                            uint32_t* numBatchesUploaded, uint32_t* batchSizes, hipStream_t stream) {
	if (u == nullptr || numBatchesUploaded == nullptr || batchSizes == nullptr) return (int)hipErrorInvalidValue;
	return run_import(ctx, u, table, numNodes, samples, numSamples, scratch, scratchBytes, pers, u->persistentBufferCapacity, nodes, stats, numBatchesUploaded,
	                  batchSizes, stream);
}

}  // namespace simlod
