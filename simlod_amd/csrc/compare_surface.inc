// compare_surface.inc — surface queries (include/simlod_hip.h, "surface queries"; the rules N2-N9 in surface_rules.hpp), included by compare.hip
// inside its anonymous namespace: the two kernels that follow the compare queries' grid build (k_c_init .. k_c_decide, launched as they are
// by launch_grid) when the call is simlod_surface_samples.
//   k_s_test     the hot path; returns at once unless `run`.  One lane per sample of `a` (grid-stride), as k_c_test: its centre widened to
//                fp64 in registers, the 27 lookups, a loop over each cell's records with rule C2's test; a passing record's three offsets are
//                quantised (rule N2) and go into nine 64-bit integer sums in registers (rule N3; the products are 32 x 32 -> 64 multiply-adds).
//                After the loop rules N3-N8 run in registers (surface_estimate: about 250 fp64 operations a sample, nothing beside the
//                neighbour loop), the lane writes its record (two 16-byte stores) and colour, counts its bin in the workgroup's LDS
//                histogram and keeps the sums in registers.  Thresholds and table in LDS.
//   k_s_final    the test pass's partial records added up -> numEstimated, numWithin, numDegenerate, hist.  k_c_final's shape; where that
//                takes a maximum of the third number this takes a sum.  Returns at once unless `run`.
// No atomic touches global memory, no loop waits on another workgroup, and every loop is bounded by a number known at launch (the table's
// capacity, a cell's population, eight squarings, eight steps of the search).  The partial record is CmpPart: `matched` holds the estimated
// samples, `maxD2` the degenerate ones.

struct SurfTestArgs {
	CmpArgs  c;
	double   thresholds[SURFACE_THRESHOLDS];
	uint32_t table[256];
	double   invq, light[3], orient[3];
	uint32_t colourBy, orientMode;
	SimlodSurfaceRecord* records;
};
static_assert(sizeof(SurfTestArgs) <= 4096, "k_s_test: the kernel arguments");
static_assert(SURFACE_BINS == COMPARE_BINS, "the surface summary is the compare summary's layout");

__global__ __launch_bounds__(CMP_TPB) void k_s_test(SurfTestArgs t) {
	__shared__ double sh_thr[SURFACE_THRESHOLDS + 1u];
	__shared__ uint32_t sh_table[256];
	__shared__ uint32_t sh_hist[CMP_HIST_WORDS];
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = t.c;
	if (header_of(c)->run == 0u) return;                                        // rules C6, C7 (the same for every workgroup)
	for (uint32_t i = threadIdx.x; i < SURFACE_THRESHOLDS; i += CMP_TPB) sh_thr[i] = t.thresholds[i];
	for (uint32_t i = threadIdx.x; i < 256u; i += CMP_TPB) sh_table[i] = t.table[i];
	for (uint32_t i = threadIdx.x; i < CMP_HIST_WORDS; i += CMP_TPB) sh_hist[i] = 0u;
	__syncthreads();
	const CmpSlot* tab = table_of(c);
	const u32x4* cells = reinterpret_cast<const u32x4*>(c.scratch + c.cells);
	const double invq = t.invq;
	const double light[3] = {t.light[0], t.light[1], t.light[2]}, orient[3] = {t.orient[0], t.orient[1], t.orient[2]};
	uint64_t estimated = 0u, degenerate = 0u, withinSum = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numA; i += (uint64_t)gridDim.x * CMP_TPB) {
		const u32x4 s = c.a[i];
		const bool valid = compare_valid(s.x, s.y, s.z);
		uint32_t within = 0u, bin = 256u;
		float normal[3] = {0.0f, 0.0f, 0.0f};
		double lambdaNum = 0.0, lambdaDen = 0.0;
		if (valid) {
			uint32_t cell[3];
			cells_of(c, s, cell);
			const double ctr[3] = {(double)__uint_as_float(s.x), (double)__uint_as_float(s.y), (double)__uint_as_float(s.z)};
			int64_t S[SURFACE_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
			for_neighbour_cells(c, tab, cell, [&](uint32_t start, uint32_t count) {
				const uint64_t end = (uint64_t)start + count;                   // (at most numB: k_c_fill's argument)
				for (uint64_t j = start; j < end; j++) {
					const u32x4 v = cells[j];
					const double px = (double)__uint_as_float(v.x) - ctr[0], py = (double)__uint_as_float(v.y) - ctr[1], pz = (double)__uint_as_float(v.z) - ctr[2];
					if ((px * px + py * py) + pz * pz <= c.rr) {                // rule C2 (compare_d2's sum)
						const int32_t qx = surface_q(px, invq), qy = surface_q(py, invq), qz = surface_q(pz, invq);   // rule N2
						within++;
						S[SURFACE_X] += qx; S[SURFACE_Y] += qy; S[SURFACE_Z] += qz;
						S[SURFACE_XX] += (int64_t)qx * qx; S[SURFACE_XY] += (int64_t)qx * qy; S[SURFACE_XZ] += (int64_t)qx * qz;
						S[SURFACE_YY] += (int64_t)qy * qy; S[SURFACE_YZ] += (int64_t)qy * qz; S[SURFACE_ZZ] += (int64_t)qz * qz;
					}
				}
			});
			SurfaceEstimate e;
			if (surface_estimate(S, within, ctr, orient, t.orientMode, e)) {    // rules N3-N7
				double num, den;
				surface_colour_terms(e, t.colourBy, light, num, den);
				bin = surface_index(sh_thr, num, den);                          // rule N8
				normal[0] = (float)e.v[0]; normal[1] = (float)e.v[1]; normal[2] = (float)e.v[2];
				lambdaNum = e.lambdaNum; lambdaDen = e.lambdaDen;
				estimated++;
			} else {
				degenerate++;                                                   // rule N9
			}
			withinSum += within;
		}
		const uint64_t nb = (uint64_t)__double_as_longlong(lambdaNum), db = (uint64_t)__double_as_longlong(lambdaDen);
		u32x4* out = reinterpret_cast<u32x4*>(t.records + i);
		out[0] = u32x4{__float_as_uint(normal[0]), __float_as_uint(normal[1]), __float_as_uint(normal[2]), within};
		out[1] = u32x4{(uint32_t)nb, (uint32_t)(nb >> 32), (uint32_t)db, (uint32_t)(db >> 32)};
		if (c.colors != nullptr) c.colors[i] = bin < 256u ? sh_table[bin] : c.missColor;
		atomicAdd(&sh_hist[bin], 1u);
	}
	estimated = block_reduce<false>(estimated, sh);
	degenerate = block_reduce<false>(degenerate, sh);
	withinSum = block_reduce<false>(withinSum, sh);                             // (its barriers: the histogram's atomics are done as well)
	CmpPart* part = parts_of(c) + blockIdx.x;
	if (threadIdx.x == 0u) { part->matched = estimated; part->within = withinSum; part->maxD2 = degenerate; }
	for (uint32_t i = threadIdx.x; i < CMP_HIST_WORDS; i += CMP_TPB) part->hist[i] = sh_hist[i];
}

// k_c_final's division of the work: workgroup g < CMP_FINAL_HIST_WGS owns bins 64g .. 64g + 63, the last one the three sums.
__global__ __launch_bounds__(CMP_TPB) void k_s_final(CmpArgs c) {
	__shared__ uint64_t sh_bins[CMP_WAVES][CMP_FINAL_COLS];
	__shared__ uint64_t sh[CMP_WAVES];
	if (header_of(c)->run == 0u) return;
	const CmpPart* parts = parts_of(c);
	SimlodSurfaceSummary* out = reinterpret_cast<SimlodSurfaceSummary*>(c.summary);
	if (blockIdx.x < CMP_FINAL_HIST_WGS) {
		const uint32_t col = threadIdx.x % CMP_FINAL_COLS, g = threadIdx.x / CMP_FINAL_COLS, bin = blockIdx.x * CMP_FINAL_COLS + col;
		uint64_t h = 0u;
		if (bin < SURFACE_BINS)
			for (uint32_t p = g; p < c.gridA; p += CMP_WAVES) h += parts[p].hist[bin];
		sh_bins[g][col] = h;
		__syncthreads();
		if (g == 0u && bin < SURFACE_BINS) {
			uint64_t r = sh_bins[0][col];
			for (uint32_t k = 1; k < CMP_WAVES; k++) r += sh_bins[k][col];
			out->hist[bin] = r;
		}
		return;
	}
	uint64_t estimated = 0u, within = 0u, degenerate = 0u;
	for (uint32_t p = threadIdx.x; p < c.gridA; p += CMP_TPB) { estimated += parts[p].matched; within += parts[p].within; degenerate += parts[p].maxD2; }
	estimated = block_reduce<false>(estimated, sh);
	within = block_reduce<false>(within, sh);
	degenerate = block_reduce<false>(degenerate, sh);
	if (threadIdx.x == 0u) {
		out->numEstimated = (uint32_t)estimated;
		out->numWithin = within;
		out->numDegenerate = degenerate;
	}
}
