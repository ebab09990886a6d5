// compare_align.inc — align queries (include/simlod_hip.h, "align queries"; the rules A1-A7 in align_rules.hpp), included by compare.hip inside
// its anonymous namespace: one step of an ICP on the compare queries' hash grid over `b`.  A BUILD call runs k_c_init, k_c_insert, k_c_ranges
// and k_c_fill as they are and then the four kernels below; a REUSE call (SIMLOD_ALIGN_REUSE_GRID) runs the four kernels alone, on the grid
// an earlier build call left in the same scratch buffer.
//   k_a_count    k_c_count with the posed centre: rule A1's validity (numInvalidA) and the populations of the up to 27 cells around c'.
//   k_a_decide   ONE workgroup, k_c_decide's job: the partial records added up, rule C6's decision (`run`), every field of the summary but the
//                test pass's, those zeroed.  A build call also writes the stamp (rule A7), with the grid's totals in it; a reuse call takes
//                the totals from the stamp, and on a stamp that does not serve it writes error = SIMLOD_ALIGN_ERR_GRID, zeroes and run = 0.
//   k_a_test     the hot path; returns at once unless the stamp serves and `run`.  One lane per sample of `a` (grid-stride), the pose in
//                scalar registers: c' once, the 27 lookups, k_c_test's inner loop against c' with the nearest sample's coordinates kept in
//                registers beside its index.  The lane writes its record (one 16-byte store, skipped when records == NULL); a matched lane
//                quantises its pair (rule A4) and adds into its own 31 64-bit accumulators, the nine products by 32 x 32 -> 64 multiplies.
//                The accumulators are reduced across the workgroup ONCE, after the grid-stride loop (wave shuffles, then CMP_WAVES words of
//                LDS), into the workgroup's AlignPart.
//   k_a_final    ONE workgroup: the AlignPart records added up into the summary.  Returns at once unless `run`.
// A reuse call's kernels compare the stamp with their own arguments before their first read of the table: on a mismatch they read nothing
// but the header and write nothing but `run` and the summary.  No atomic touches global memory, no loop waits on another workgroup, and every
// loop is bounded by a number known at launch.  k_a_count's partial fields are CmpPart's (invalidA, candidates); the test pass has a record
// of its own, AlignPart, behind the compare layout, so CmpLayout and CmpPart stay as they are.

constexpr uint32_t ALIGN_PART_WORDS = 32u;                                    // AlignPart as 64-bit words; the last is padding
enum { AP_MATCHED = 0, AP_WITHIN, AP_MAXD2, AP_SUMMED, AP_OUTSIDE, AP_SUM_A, AP_SUM_B = AP_SUM_A + 3, AP_CROSS_LO = AP_SUM_B + 3, AP_CROSS_HI = AP_CROSS_LO + 9,
       AP_SQ_LO = AP_CROSS_HI + 9, AP_SQ_HI, AP_USED };
struct AlignPart {                     // one per workgroup of k_a_test
	uint64_t w[ALIGN_PART_WORDS];      // AP_*: sums, but AP_MAXD2 a maximum (the double's bits)
};
static_assert(AP_USED == 31 && AP_USED <= ALIGN_PART_WORDS && sizeof(AlignPart) == 256, "AlignPart");
// the summary as 64-bit words: numWithin 3, maxD2 5, then numSummed .. sqHi in AlignPart's order
static_assert(offsetof(SimlodAlignSummary, numWithin) == 24 && offsetof(SimlodAlignSummary, maxD2) == 40 &&
              offsetof(SimlodAlignSummary, numSummed) == (AP_SUMMED + 3) * 8 && offsetof(SimlodAlignSummary, sqHi) == (AP_SQ_HI + 3) * 8 &&
              sizeof(SimlodAlignSummary) == (AP_USED + 3) * 8, "k_a_final: summary word = part word + 3");
static_assert(offsetof(CmpHeader, pad) == 8 && sizeof(AlignStamp) <= sizeof(CmpHeader) - 8, "the stamp lies in the header's unused words");

struct AlignArgs {
	CmpArgs  c;                        // c.inv from gridRadius, c.rr from radius; c.summary is not used
	double   T[12], invq;
	AlignStamp want;                   // the stamp this call writes (build) or must find (reuse); its totals are not compared
	uint32_t reuse;
	uint64_t aparts;                   // the AlignPart records' offset in the scratch buffer
	SimlodAlignSummary* out;
};

__device__ __forceinline__ AlignStamp* stamp_of(const CmpArgs& c) { return reinterpret_cast<AlignStamp*>(header_of(c)->pad); }
__device__ __forceinline__ bool stamp_serves(const AlignArgs& t) { return align_stamp_serves(*stamp_of(t.c), t.want); }

// rules A1, A2: the posed centre and its three cells; false: the sample is invalid
__device__ __forceinline__ bool posed(const AlignArgs& t, const u32x4& s, double (&cp)[3], uint32_t (&cell)[3]) {
	if (!compare_valid(s.x, s.y, s.z)) return false;
	if (!align_pose(t.T, (double)__uint_as_float(s.x), (double)__uint_as_float(s.y), (double)__uint_as_float(s.z), cp)) return false;
#pragma unroll
	for (int k = 0; k < 3; k++) cell[k] = align_cell20(cp[k], t.c.min[k], t.c.inv);
	return true;
}

__global__ __launch_bounds__(CMP_TPB) void k_a_count(AlignArgs t) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = t.c;
	if (t.reuse != 0u && !stamp_serves(t)) return;                              // rule A7 (the same for every workgroup)
	const CmpSlot* tab = table_of(c);
	uint64_t invalid = 0u, candidates = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numA; i += (uint64_t)gridDim.x * CMP_TPB) {
		double cp[3];
		uint32_t cell[3];
		if (!posed(t, c.a[i], cp, cell)) { invalid++; continue; }
		for_neighbour_cells(c, tab, cell, [&](uint32_t, uint32_t count) { candidates += count; });
	}
	invalid = block_reduce<false>(invalid, sh);
	candidates = block_reduce<false>(candidates, sh);
	if (threadIdx.x == 0u) { CmpPart* part = parts_of(c) + blockIdx.x; part->invalidA = invalid; part->candidates = candidates; }
}

__global__ __launch_bounds__(CMP_TPB) void k_a_decide(AlignArgs t) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = t.c;
	uint64_t* words = reinterpret_cast<uint64_t*>(t.out);
	constexpr uint32_t SUMMARY_WORDS = sizeof(SimlodAlignSummary) / 8u;
	if (t.reuse != 0u && !stamp_serves(t)) {                                    // rule A7: nothing but the header was read
		if (threadIdx.x < SUMMARY_WORDS) words[threadIdx.x] = threadIdx.x == 0u ? (uint64_t)SIMLOD_ALIGN_ERR_GRID : 0u;   // (error: the low half of word 0)
		if (threadIdx.x == 0u) header_of(c)->run = 0u;
		return;
	}
	const CmpPart* parts = parts_of(c);
	uint64_t invalidB = 0u, cells = 0u, maxPop = 0u, invalidA = 0u, candidates = 0u;
	if (t.reuse == 0u) {
		for (uint32_t p = threadIdx.x; p < c.gridB; p += CMP_TPB) invalidB += parts[p].invalidB;
		for (uint32_t p = threadIdx.x; p < c.gridS; p += CMP_TPB) { cells += parts[p].cells; maxPop = parts[p].maxPop > maxPop ? parts[p].maxPop : maxPop; }
		invalidB = block_reduce<false>(invalidB, sh);
		cells = block_reduce<false>(cells, sh);
		maxPop = block_reduce<true>(maxPop, sh);
	} else {
		const AlignStamp* have = stamp_of(c);
		invalidB = have->numInvalidB; cells = have->numCells; maxPop = have->maxCellPopulation;
	}
	for (uint32_t p = threadIdx.x; p < c.gridA; p += CMP_TPB) { invalidA += parts[p].invalidA; candidates += parts[p].candidates; }
	invalidA = block_reduce<false>(invalidA, sh);
	candidates = block_reduce<false>(candidates, sh);
	if (threadIdx.x >= 6u && threadIdx.x < SUMMARY_WORDS) words[threadIdx.x] = 0u;   // numSummed .. sqHi
	if (threadIdx.x == 0u) {
		const bool over = c.maxCandidates != 0u && candidates > c.maxCandidates;    // rule C6
		header_of(c)->run = (c.countOnly == 0u && !over) ? 1u : 0u;
		SimlodAlignSummary* out = t.out;
		out->error = over ? SIMLOD_ALIGN_ERR_BUDGET : 0u;
		out->numCells = (uint32_t)cells;
		out->maxCellPopulation = (uint32_t)maxPop;
		out->numInvalidA = (uint32_t)invalidA;
		out->numInvalidB = (uint32_t)invalidB;
		out->numMatched = 0u;
		out->numWithin = 0u;
		out->numCandidates = candidates;
		out->maxD2 = 0.0;
		if (t.reuse == 0u) {                                                    // rule A7: the grid stands; its stamp
			AlignStamp s = t.want;
			s.numCells = cells; s.maxCellPopulation = maxPop; s.numInvalidB = invalidB;
			*stamp_of(c) = s;
		}
	}
}
static_assert(offsetof(SimlodAlignSummary, numSummed) == 48, "k_a_decide: the words it zeroes start at 6");

__global__ __launch_bounds__(CMP_TPB) void k_a_test(AlignArgs t) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = t.c;
	if (!stamp_serves(t)) return;                                               // rule A7, before anything else (the same for every workgroup)
	if (header_of(c)->run == 0u) return;                                        // rules C6, C7
	const CmpSlot* tab = table_of(c);
	const u32x4* cells = reinterpret_cast<const u32x4*>(c.scratch + c.cells);
	uint64_t acc[AP_USED];
#pragma unroll
	for (int k = 0; k < AP_USED; k++) acc[k] = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numA; i += (uint64_t)gridDim.x * CMP_TPB) {
		const u32x4 s = c.a[i];
		double best = __longlong_as_double((long long)COMPARE_MISS_D2_BITS);
		uint32_t nearest = COMPARE_MISS, within = 0u, nx = 0u, ny = 0u, nz = 0u;
		double cp[3];
		uint32_t cell[3];
		if (posed(t, s, cp, cell)) {
			for_neighbour_cells(c, tab, cell, [&](uint32_t start, uint32_t count) {
				const uint64_t end = (uint64_t)start + count;                   // (at most numB: k_c_fill's argument)
				for (uint64_t j = start; j < end; j++) {
					const u32x4 v = cells[j];
					const double d2 = compare_d2((double)__uint_as_float(v.x), (double)__uint_as_float(v.y), (double)__uint_as_float(v.z), cp[0], cp[1], cp[2]);
					if (d2 <= c.rr) {                                           // rule A3
						within++;
						if (d2 < best || (d2 == best && v.w < nearest)) { best = d2; nearest = v.w; nx = v.x; ny = v.y; nz = v.z; }   // rule C3: (d2, index)
					}
				}
			});
		}
		const uint64_t bits = (uint64_t)__double_as_longlong(best);
		if (c.records != nullptr) *reinterpret_cast<u32x4*>(c.records + i) = u32x4{(uint32_t)bits, (uint32_t)(bits >> 32), nearest, within};
		if (within != 0u) {
			acc[AP_MATCHED]++; acc[AP_WITHIN] += within; acc[AP_MAXD2] = bits > acc[AP_MAXD2] ? bits : acc[AP_MAXD2];
			const double sb[3] = {(double)__uint_as_float(nx), (double)__uint_as_float(ny), (double)__uint_as_float(nz)};
			uint32_t qa[3], qb[3];
			bool inside = true;
#pragma unroll
			for (int k = 0; k < 3; k++) {                                       // rule A4
				inside = align_q(cp[k], c.min[k], t.invq, qa[k]) && inside;
				inside = align_q(sb[k], c.min[k], t.invq, qb[k]) && inside;
			}
			if (inside) {                                                       // rule A5
				acc[AP_SUMMED]++;
#pragma unroll
				for (int k = 0; k < 3; k++) {
					acc[AP_SUM_A + k] += qa[k]; acc[AP_SUM_B + k] += qb[k];
#pragma unroll
					for (int l = 0; l < 3; l++) {
						const uint64_t P = (uint64_t)qa[k] * qb[l];
						acc[AP_CROSS_LO + 3 * k + l] += align_lo(P); acc[AP_CROSS_HI + 3 * k + l] += align_hi(P);
					}
				}
				const uint64_t E = align_sq(qa, qb);
				acc[AP_SQ_LO] += align_lo(E); acc[AP_SQ_HI] += align_hi(E);
			} else {
				acc[AP_OUTSIDE]++;
			}
		}
	}
	AlignPart* part = reinterpret_cast<AlignPart*>(c.scratch + t.aparts) + blockIdx.x;
#pragma unroll
	for (int k = 0; k < AP_USED; k++) {
		const uint64_t r = k == AP_MAXD2 ? block_reduce<true>(acc[k], sh) : block_reduce<false>(acc[k], sh);
		if (threadIdx.x == 0u) part->w[k] = r;
	}
}

// Lane l adds word l % 32 over the parts l / 32, l / 32 + 8, ...; the eight groups' sums meet in LDS and group 0 writes the summary's words.
__global__ __launch_bounds__(CMP_TPB) void k_a_final(AlignArgs t) {
	constexpr uint32_t GROUPS = CMP_TPB / ALIGN_PART_WORDS;
	__shared__ uint64_t sh_w[GROUPS][ALIGN_PART_WORDS];
	const CmpArgs& c = t.c;
	if (header_of(c)->run == 0u) return;
	const AlignPart* parts = reinterpret_cast<const AlignPart*>(c.scratch + t.aparts);
	const uint32_t w = threadIdx.x % ALIGN_PART_WORDS, g = threadIdx.x / ALIGN_PART_WORDS;
	uint64_t r = 0u;
	if (w < AP_USED)
		for (uint32_t p = g; p < c.gridA; p += GROUPS) r = w == AP_MAXD2 ? (parts[p].w[w] > r ? parts[p].w[w] : r) : r + parts[p].w[w];
	sh_w[g][w] = r;
	__syncthreads();
	if (g != 0u || w >= AP_USED) return;
	for (uint32_t k = 1; k < GROUPS; k++) r = w == AP_MAXD2 ? (sh_w[k][w] > r ? sh_w[k][w] : r) : r + sh_w[k][w];
	uint64_t* words = reinterpret_cast<uint64_t*>(t.out);
	if (w == AP_MATCHED) t.out->numMatched = (uint32_t)r;
	else if (w == AP_WITHIN) words[3] = r;
	else if (w == AP_MAXD2) words[5] = r;
	else words[w + 3u] = r;
}

uint64_t align_bytes(uint64_t numB) { return CmpLayout(numB).bytes + (uint64_t)CMP_MAX_PARTS * sizeof(AlignPart); }

// simlod_align_samples: the checks (nothing is enqueued before the last of them), then the launches listed at the top.
int launch_align_impl(const SimlodUniforms* u, const SimlodPoint* a, uint64_t numA, const SimlodPoint* b, uint64_t numB, const SimlodAlignParams* params,
                      void* scratch, uint64_t scratchBytes, SimlodCompareRecord* records, SimlodAlignSummary* summary, hipStream_t stream) {
	if (params == nullptr || !align_acceptable(*params)) return (int)hipErrorInvalidValue;
	if (!compare_count_acceptable(numA) || !compare_count_acceptable(numB) || scratchBytes < align_bytes(numB)) return (int)hipErrorInvalidValue;
	AlignArgs t{};
	CmpArgs& c = t.c;
	const CmpCall call{params->gridRadius, 0u, params->maxCandidates, params->maxWorkgroups};   // rule A2: the grid is gridRadius's
	if (!compare_prepare(u, a, numA, b, numB, call, scratch, scratchBytes, records, nullptr, reinterpret_cast<SimlodCompareSummary*>(summary), c))
		return (int)hipErrorInvalidValue;
	float size, mn[3];
	octree_box(u, size, mn[0], mn[1], mn[2]);
	c.countOnly = (params->flags & SIMLOD_ALIGN_COUNT_ONLY) != 0u ? 1u : 0u;      // rule A6: records == NULL alone is a full call
	c.rr = (double)params->radius * (double)params->radius;
	c.records = records;
	for (int k = 0; k < 12; k++) t.T[k] = params->pose[k];
	t.invq = align_invq(size);
	t.want = align_stamp(b, numB, c.inv, c.min, c.countOnly == 0u);
	t.reuse = (params->flags & SIMLOD_ALIGN_REUSE_GRID) != 0u ? 1u : 0u;
	t.aparts = CmpLayout(numB).bytes;
	t.out = summary;
	if (t.reuse == 0u) {
		SIMLOD_LAUNCH(k_c_init, dim3(c.gridS), dim3(CMP_TPB), stream, c);
		SIMLOD_LAUNCH(k_c_insert, dim3(c.gridB), dim3(CMP_TPB), stream, c);
		SIMLOD_LAUNCH(k_c_ranges, dim3(c.gridS), dim3(CMP_TPB), stream, c);
		if (c.countOnly == 0u) SIMLOD_LAUNCH(k_c_fill, dim3(c.gridB), dim3(CMP_TPB), stream, c);
	}
	SIMLOD_LAUNCH(k_a_count, dim3(c.gridA), dim3(CMP_TPB), stream, t);
	SIMLOD_LAUNCH(k_a_decide, dim3(1), dim3(CMP_TPB), stream, t);
	if (c.countOnly == 0u) {
		SIMLOD_LAUNCH(k_a_test, dim3(c.gridA), dim3(CMP_TPB), stream, t);
		SIMLOD_LAUNCH(k_a_final, dim3(1), dim3(CMP_TPB), stream, t);
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}
