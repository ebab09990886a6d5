// export_summary.inc — part of export.hip: summary queries.  SummaryPart, SummaryOp, SummaryArgs, FootSummaryArgs, SummaryFinalArgs, hist_add,
// s_partial, k_s_partial, k_fs_partial, k_s_final.
// ---- summary queries --------------------------------------------------------------------------------------------------------------------
// simlod_query_summary (simlod_hip.h, "summary queries"): the footprint query's count-only call — k_q_hier / k_f_hier -> k_q_dir -> k_q_count /
// k_f_count -> k_q_scan — and then
//   k_s_partial   the items once more, one chunk per workgroup and turn, read as k_e_paint reads them (four 16-byte non-temporal loads of a lane
//                 in flight), a filtered one tested again; the next item's loads are issued before this one's samples are counted.  Nothing is
//                 stored per sample.  A workgroup keeps the five 256-bin histograms in LDS
//                 as 32-bit counts and each lane the nine sums, the non-finite count and the six extent keys in registers; after its last item
//                 the registers are reduced across the wave by shuffles and across the four waves through LDS, and the workgroup writes ONE
//                 SummaryPart at its slot of the scratch buffer with plain stores.  A workgroup without an item writes none.
//   k_fs_partial  the same body with rule F1 behind the planes' test, the polygon staged in LDS as k_ef_paint stages it.
//   k_s_final     the parts that were written (summary_parts: the first slots) added up, the histograms widened to 64 bits, the keys
//                 turned back into floats -> SimlodSummary.  21 workgroups, each the owner of a slice of the record (64 bins, or the slots):
//                 one workgroup alone would read every part, 5 KB each, through one CU.
// No atomic touches global memory.  A histogram's bin is an integer LDS atomic — unless every selected lane of the wave has the same bin (one
// colour, one height band, the alpha byte of nearly every cloud): then a ballot finds that out and ONE lane adds the popcount, where 64 atomics
// on one address would queue up behind each other (DESIGN §11 has both timings).
// k_q_scan zeroes hdr->numItems for a count-only call: the items are hdr->totalChunks.  Rule S5's check is made by every workgroup of both
// kernels from what k_q_scan left in the counts record.
// The rules themselves (S1-S3) in summary_rules.hpp.
constexpr uint32_t SUMMARY_HISTS = 5;                                              // z, colour bytes 0..3
constexpr uint32_t SUMMARY_BINS = 256;
constexpr uint32_t SUMMARY_SLOTS = 16;                                             // sum[3], sum2[6], numNonFinite, min keys[3], max keys[3]
constexpr uint32_t SUMMARY_ADD_SLOTS = 10, SUMMARY_MIN_SLOTS = 13;                 // slots below 10 add, below 13 take the minimum, the rest the maximum
constexpr uint32_t SUMMARY_MAX_PARTS = 1024;                                       // the largest grid of k_s_partial (summary_grid)

struct SummaryPart {
	uint64_t slot[SUMMARY_SLOTS];
	uint32_t hist[SUMMARY_HISTS * SUMMARY_BINS];
};
static_assert(sizeof(SummaryPart) == 5248, "SummaryPart");
constexpr uint64_t SUMMARY_BLOCK_BYTES = (uint64_t)SUMMARY_MAX_PARTS * sizeof(SummaryPart);   // of the scratch buffer, in front of the items (behind the polygon's block)

struct SummaryOp {
	double   inv;                       // rule S2's factor
	float    z0, scale;
	uint64_t parts;                     // offset of SummaryPart[gridDim.x] in the scratch buffer
};
struct SummaryArgs     { QueryArgs q; SummaryOp s; };
struct FootSummaryArgs { FootArgs  f; SummaryOp s; };
__device__ __forceinline__ const QueryArgs& query_of(const SummaryArgs& sa) { return sa.q; }
__device__ __forceinline__ const QueryArgs& query_of(const FootSummaryArgs& sa) { return sa.f.q; }
struct SummaryFinalArgs {
	const uint8_t*           scratch;
	uint64_t                 parts;
	uint32_t                 numParts, pad;
	const SimlodQueryCounts* counts;
	SimlodSummary*           out;
};

// The workgroups of a grid of `grid` that have an item among `items`, and so the parts that are written: the first ones.  (Fewer, fuller parts
// for a small selection were measured and lost: four chunks in a row cost a workgroup more than a part costs to write and to read again.)
__device__ __forceinline__ uint32_t summary_parts(uint32_t grid, uint64_t items) { return items < (uint64_t)grid ? (uint32_t)items : grid; }

__device__ __forceinline__ uint64_t summary_combine(uint32_t slot, uint64_t a, uint64_t b) {
	return slot < SUMMARY_ADD_SLOTS ? a + b : slot < SUMMARY_MIN_SLOTS ? (a < b ? a : b) : (a > b ? a : b);
}
__device__ __forceinline__ uint64_t summary_identity(uint32_t slot) {
	return slot < SUMMARY_ADD_SLOTS ? 0u : slot < SUMMARY_MIN_SLOTS ? (uint64_t)SUMMARY_KEY_POS_INF : (uint64_t)SUMMARY_KEY_NEG_INF;
}

// hist[bin]++ for the lanes that are `on` (the whole wave calls): one add of the popcount when they all name the same bin
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t bin, bool on, int lane) {
	const uint64_t m = __ballot(on);
	if (m == 0ull) return;                                                   // (the same for the whole wave)
	const int lead = __ffsll((long long)m) - 1;                              // (a scalar: the ballot is)
	const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)bin, lead);
	if (__ballot(on && bin != first) == 0ull) {
		if (lane == lead) atomicAdd(&hist[first], (uint32_t)__popcll(m));
	} else if (on) {
		atomicAdd(&hist[bin], 1u);
	}
}

// One item and the samples of its chunk, four 16-byte non-temporal loads of a lane in flight; an item that contributes nothing (an empty slot of
// a short list, a filtered chunk of which no sample passed) comes back with count 0 and without a load.  The loads name the global address
// space: a flat load counts as an LDS access as well, and the wait in front of an LDS access of the item before would wait for them.
typedef const __attribute__((address_space(1))) u32x4* GlobalSamples;
__device__ __forceinline__ void summary_fetch(const QItem* items, uint64_t i, uint64_t numItems, QItem& it, u32x4 (&v)[4]) {
	if (i < numItems) it = items[i];                                        // (the same for the whole workgroup)
	else it = QItem{0u, 0u, 0u, 0u, Q_OUTSIDE, 0u, 0u};
	if (it.count != 0u && it.tag != Q_COPIED && (it.tag != Q_FILTERED || it.pass == 0u)) it.count = 0u;
	const GlobalSamples s = (GlobalSamples)it.src;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
		v[j] = k < it.count ? __builtin_nontemporal_load(s + k) : u32x4{0u, 0u, 0u, 0u};
	}
}

// the body of the partial kernels; extra(v) and INVERT as in q_count
template <typename Args, bool INVERT = false, typename Extra>
__device__ __forceinline__ void s_partial(const Args& args, Extra extra) {
	const QueryArgs& q = query_of(args);
	const SummaryOp& sp = args.s;
	__shared__ uint32_t sh_hist[SUMMARY_HISTS * SUMMARY_BINS];
	__shared__ uint64_t sh_red[LANE_TPB / SIMLOD_WAVE][SUMMARY_SLOTS];
	const ExportArgs& a = q.x;
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const QItem* items = reinterpret_cast<const QItem*>(a.scratch + a.lay.items);
	if (q.counts->error != 0u) return;                                       // rule S5 (the same for every workgroup)
	const uint64_t numItems = hdr->totalChunks;
	const uint32_t wgs = summary_parts(gridDim.x, numItems);
	if (blockIdx.x >= wgs) return;                                           // no item, no part: k_s_final reads the first `wgs`
	for (uint32_t i = threadIdx.x; i < SUMMARY_HISTS * SUMMARY_BINS; i += LANE_TPB) sh_hist[i] = 0u;
	__syncthreads();
	const int lane = lane_id(), w = (int)(threadIdx.x / SIMLOD_WAVE);
	uint64_t slot[SUMMARY_SLOTS];
#pragma unroll
	for (uint32_t s = 0; s < SUMMARY_SLOTS; s++) slot[s] = summary_identity(s);
	uint32_t kmin[3] = {SUMMARY_KEY_POS_INF, SUMMARY_KEY_POS_INF, SUMMARY_KEY_POS_INF};
	uint32_t kmax[3] = {SUMMARY_KEY_NEG_INF, SUMMARY_KEY_NEG_INF, SUMMARY_KEY_NEG_INF};
	// the next item's loads are in flight while this one's samples are counted
	QItem it, nxt;
	u32x4 v[4], vn[4];
	summary_fetch(items, blockIdx.x, numItems, it, v);
	for (uint64_t i = blockIdx.x; i < numItems; i += wgs) {
		summary_fetch(items, i + wgs, numItems, nxt, vn);
		const bool copied = it.tag == Q_COPIED;                             // (the same for the whole workgroup, as every branch on `it`)
		if (it.count != 0u) {
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
				bool on = k < it.count;
				if (INVERT) { if (!copied) on = on && !(passes(q.g, v[j]) && extra(v[j])); }
				else if (!copied) on = on && passes(q.g, v[j]) && extra(v[j]);
				if (on) {
					const uint32_t bits[3] = {v[j].x, v[j].y, v[j].z};
					uint32_t c16[3];
					bool finite = true;
#pragma unroll
					for (int ax = 0; ax < 3; ax++) {
						finite = finite && summary_is_finite(bits[ax]);
						if (!summary_is_nan(bits[ax])) {
							const uint32_t key = summary_key(bits[ax]);
							kmin[ax] = min(kmin[ax], key);
							kmax[ax] = max(kmax[ax], key);
						}
						const uint32_t c20 = summary_cell20(__uint_as_float(bits[ax]), q.g.min[ax], sp.inv);
						slot[ax] += c20;
						c16[ax] = c20 >> 4;
					}
					slot[3] += c16[0] * c16[0]; slot[4] += c16[1] * c16[1]; slot[5] += c16[2] * c16[2];  // (below 2^32 each)
					slot[6] += c16[0] * c16[1]; slot[7] += c16[0] * c16[2]; slot[8] += c16[1] * c16[2];
					slot[9] += finite ? 0u : 1u;
				}
				hist_add(sh_hist, paint_ramp_index(__uint_as_float(v[j].z), sp.z0, sp.scale), on, lane);
#pragma unroll
				for (uint32_t b = 0; b < 4u; b++) hist_add(sh_hist + (b + 1u) * SUMMARY_BINS, (v[j].w >> (8u * b)) & 255u, on, lane);
			}
		}
		it = nxt;
#pragma unroll
		for (int j = 0; j < 4; j++) v[j] = vn[j];
	}
#pragma unroll
	for (int ax = 0; ax < 3; ax++) { slot[SUMMARY_ADD_SLOTS + ax] = kmin[ax]; slot[SUMMARY_MIN_SLOTS + ax] = kmax[ax]; }
	// across the wave, then across the four waves
#pragma unroll
	for (int o = SIMLOD_WAVE / 2; o >= 1; o >>= 1) {
#pragma unroll
		for (uint32_t s = 0; s < SUMMARY_SLOTS; s++) slot[s] = summary_combine(s, slot[s], (uint64_t)__shfl_xor((unsigned long long)slot[s], o, SIMLOD_WAVE));
	}
	if (lane == 0) {
#pragma unroll
		for (uint32_t s = 0; s < SUMMARY_SLOTS; s++) sh_red[w][s] = slot[s];
	}
	__syncthreads();                                                        // (the histograms' atomics are done as well)
	SummaryPart* part = reinterpret_cast<SummaryPart*>(a.scratch + sp.parts) + blockIdx.x;
	if (threadIdx.x < SUMMARY_SLOTS) {
		const uint32_t s = threadIdx.x;
		uint64_t r = sh_red[0][s];
		for (uint32_t ww = 1; ww < LANE_TPB / SIMLOD_WAVE; ww++) r = summary_combine(s, r, sh_red[ww][s]);
		part->slot[s] = r;
	}
	for (uint32_t i = threadIdx.x; i < SUMMARY_HISTS * SUMMARY_BINS; i += LANE_TPB) part->hist[i] = sh_hist[i];
}

__global__ __launch_bounds__(LANE_TPB) void k_s_partial(SummaryArgs sa) { s_partial<SummaryArgs>(sa, NoFootprint()); }

__global__ __launch_bounds__(LANE_TPB) void k_fs_partial(FootSummaryArgs sa) {
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	stage_edges(sa.f, sh_edges);
	__syncthreads();
	s_partial<FootSummaryArgs>(sa, Footprint{sa.f.f, sh_edges});
}

// The parts that were written, added up.  Workgroup b < SUMMARY_FINAL_HIST_WGS owns 64 consecutive bins of the 1 280 (16 columns of four
// 32-bit counts, a 16-byte load each), the last workgroup the 16 slots; in each, lane l takes column / slot l % 16 of the parts l / 16,
// l / 16 + 64, ..., and the 64 part groups' sums meet in LDS.  Every word of the record is written by one lane of one workgroup; integer sums,
// minima and maxima: the order of adding is immaterial.
constexpr uint32_t SUMMARY_FINAL_COLS = 16, SUMMARY_FINAL_GROUPS = WG_TPB / SUMMARY_FINAL_COLS;
constexpr uint32_t SUMMARY_FINAL_TURNS = SUMMARY_MAX_PARTS / SUMMARY_FINAL_GROUPS;   // parts per lane at most
constexpr uint32_t SUMMARY_FINAL_FLIGHT = 8;
constexpr uint32_t SUMMARY_FINAL_HIST_WGS = SUMMARY_HISTS * SUMMARY_BINS / (4u * SUMMARY_FINAL_COLS);
__global__ __launch_bounds__(WG_TPB) void k_s_final(SummaryFinalArgs f) {
	__shared__ uint64_t sh[SUMMARY_FINAL_GROUPS][SUMMARY_FINAL_COLS * 4u];
	if (f.counts->error != 0u) return;                                       // rule S5
	const Header* hdr = reinterpret_cast<const Header*>(f.scratch);
	const SummaryPart* parts = reinterpret_cast<const SummaryPart*>(f.scratch + f.parts);
	const uint32_t n = summary_parts(f.numParts, hdr->totalChunks);
	const uint32_t col = threadIdx.x % SUMMARY_FINAL_COLS, g = threadIdx.x / SUMMARY_FINAL_COLS;
	if (blockIdx.x < SUMMARY_FINAL_HIST_WGS) {
		const uint32_t word = (blockIdx.x * SUMMARY_FINAL_COLS + col) * 4u;     // of the 1 280
		uint64_t h[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
		for (uint32_t t0 = 0; t0 < SUMMARY_FINAL_TURNS && g + t0 * SUMMARY_FINAL_GROUPS < n; t0 += SUMMARY_FINAL_FLIGHT) {
			u32x4 c[SUMMARY_FINAL_FLIGHT];                                   // (eight loads of the lane in flight at once)
#pragma unroll
			for (uint32_t t = 0; t < SUMMARY_FINAL_FLIGHT; t++) {
				const uint32_t p = g + (t0 + t) * SUMMARY_FINAL_GROUPS;
				c[t] = p < n ? *reinterpret_cast<const u32x4*>(parts[p].hist + word) : u32x4{0u, 0u, 0u, 0u};
			}
#pragma unroll
			for (uint32_t t = 0; t < SUMMARY_FINAL_FLIGHT; t++) { h[0] += c[t].x; h[1] += c[t].y; h[2] += c[t].z; h[3] += c[t].w; }
		}
#pragma unroll
		for (uint32_t k = 0; k < 4u; k++) sh[g][col * 4u + k] = h[k];
		__syncthreads();
		if (threadIdx.x < SUMMARY_FINAL_COLS * 4u) {
			uint64_t t = 0u;
#pragma unroll 16
			for (uint32_t gg = 0; gg < SUMMARY_FINAL_GROUPS; gg++) t += sh[gg][threadIdx.x];      // (unrolled: the LDS reads follow one another)
			uint64_t* hist = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(f.out) + offsetof(SimlodSummary, histZ));   // histZ, then histC[0..3]
			hist[blockIdx.x * SUMMARY_FINAL_COLS * 4u + threadIdx.x] = t;
		}
		return;
	}
	uint64_t s = summary_identity(col), c[SUMMARY_FINAL_TURNS];
#pragma unroll
	for (uint32_t t = 0; t < SUMMARY_FINAL_TURNS; t++) {
		const uint32_t p = g + t * SUMMARY_FINAL_GROUPS;
		c[t] = p < n ? parts[p].slot[col] : s;
	}
#pragma unroll
	for (uint32_t t = 0; t < SUMMARY_FINAL_TURNS; t++) s = summary_combine(col, s, c[t]);
	sh[g][col] = s;
	__syncthreads();
	if (threadIdx.x < SUMMARY_SLOTS) {
		const uint32_t k = threadIdx.x;
		uint64_t r = sh[0][k];
#pragma unroll 21
		for (uint32_t gg = 1; gg < SUMMARY_FINAL_GROUPS; gg++) r = summary_combine(k, r, sh[gg][k]);
		if (k < 3u) f.out->sum[k] = r;
		else if (k < 9u) f.out->sum2[k - 3u] = r;
		else if (k == 9u) f.out->numNonFinite = r;
		else if (k < SUMMARY_MIN_SLOTS) f.out->min[k - SUMMARY_ADD_SLOTS] = __uint_as_float(summary_unkey((uint32_t)r));
		else f.out->max[k - SUMMARY_MIN_SLOTS] = __uint_as_float(summary_unkey((uint32_t)r));
	}
	if (threadIdx.x == 0u) f.out->numSamples = f.counts->numSamples;
}
static_assert(offsetof(SimlodSummary, histC) == offsetof(SimlodSummary, histZ) + SUMMARY_BINS * sizeof(uint64_t), "k_s_final: histC follows histZ");
static_assert(SUMMARY_FINAL_COLS == SUMMARY_SLOTS && SUMMARY_FINAL_HIST_WGS * SUMMARY_FINAL_COLS * 4u == SUMMARY_HISTS * SUMMARY_BINS, "k_s_final: the slices");
static_assert(SUMMARY_FINAL_TURNS * SUMMARY_FINAL_GROUPS == SUMMARY_MAX_PARTS, "k_s_final: every part has a lane");
static_assert(SUMMARY_FINAL_TURNS % SUMMARY_FINAL_FLIGHT == 0, "k_s_final: whole flights");
static_assert(offsetof(SummaryPart, hist) % 16 == 0 && sizeof(SummaryPart) % 16 == 0, "k_s_final: 16-byte loads");
