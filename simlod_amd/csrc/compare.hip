// compare.hip — compare queries (include/simlod_hip.h, "compare queries"; no counterpart in the reference): for every sample of `a` the nearest
// sample of `b` within a radius, on a hash grid over `b`.  The rules themselves (C1-C5) in compare_rules.hpp.  No octree, no context: two flat
// sample arrays in, records, colours and one summary out; everything in between lives in the caller's scratch buffer (CmpLayout), whose size
// depends on numB only.
//
// Eight launches on the caller's stream, every dependency a kernel boundary: no loop waits on another workgroup, there is no grid barrier, and
// every probe loop is bounded by the table's capacity, a number known at launch.
//   k_c_init     the table's slots emptied (key = COMPARE_EMPTY_KEY, count = 0), the header zeroed.
//   k_c_insert   one lane per sample of `b` (grid-stride): rule C1, the cell's key, linear probing from the key's home slot with a 64-bit
//                compare-and-swap on the slot's key — an agent-scope load first: most samples find their cell's key already there —, then an
//                atomic add on the slot's count, whose old value is the sample's rank in its cell.  The slot and the rank are kept per
//                sample, so the fill probes nothing.  The table has at least twice as many slots as `b` has samples: a free slot always exists.
//   k_c_ranges   eight slots per lane and turn: a workgroup scan of the counts of its 2 048 slots and ONE atomic add of their sum to the cursor
//                give every occupied slot the start of its range of grid records.  (One slot per lane was measured first: 6.0 ms for the 2^27
//                slots of a 36 M-sample `b`, every turn waiting for its atomic's round trip)  Which cell gets which range depends
//                on the schedule; nothing returned does.  numCells and maxCellPopulation fall out here.
//   k_c_fill     (calls with results only) one lane per sample of `b`: the 16-byte grid record {x, y, z, index in b} at start + rank of its
//                slot.  The test pass then reads a cell as contiguous records, not as a gather through an index.
//   k_c_count    one lane per sample of `a`: the populations of the up to 27 neighbouring cells (rule C4's numCandidates), numInvalidA.
//   k_c_decide   ONE workgroup: the partial records so far added up, rule C6's decision written into the scratch header (`run`) and every
//                field of the summary but the test pass's; those are zeroed.
//   k_c_test     the hot path; returns at once unless `run`.  One lane per sample of `a`: its centre widened to fp64 in registers, the 27
//                lookups, a loop over each cell's records with rule C2's test and rule C3's order (d2, index).  The lane writes its own
//                record (one 16-byte store) and colour, counts its bin in the workgroup's LDS histogram and keeps the sums in registers.
//   k_c_final    the test pass's partial records added up -> numMatched, numWithin, maxD2, hist.  Returns at once unless `run`.
// The surface queries (compare_surface.inc, included below) run the first six launches as they are — launch_grid — and follow them with their
// own test pass and final; the cluster queries (compare_cluster.inc) run them with b = a and follow them with seven kernels of their own; the
// align queries (compare_align.inc) run the first four, or on a grid they built earlier none, and follow them with four kernels of their own.
// No atomic touches global memory for the summary: every kernel writes ONE partial record per workgroup (CmpPart, its own fields of it) with
// plain stores, as export_summary.inc does, and integer sums and maxima do not depend on the order of adding (rule C8).  d2 is never negative,
// so the maximum of its 64 bits as an unsigned integer is the maximum of the doubles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "simlod_device.hpp"
#include "simlod_hip.h"
#include "simlod_internal.hpp"
#include "compare_rules.hpp"
#include "surface_rules.hpp"
#include "cluster_rules.hpp"
#include "align_rules.hpp"

namespace simlod {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t CMP_TPB = 256;                                              // lanes per workgroup, every kernel
constexpr uint32_t CMP_WAVES = CMP_TPB / SIMLOD_WAVE;
constexpr uint32_t CMP_MAX_PARTS = 1024;                                       // the largest grid of any kernel
constexpr uint32_t CMP_RANGE_PER_LANE = 8, CMP_RANGE_SLOTS = CMP_TPB * CMP_RANGE_PER_LANE;   // k_c_ranges: slots per lane and per workgroup turn
constexpr uint32_t CMP_HIST_WORDS = 260;                                      // COMPARE_BINS rounded up to whole 16 bytes
constexpr uint32_t CMP_FINAL_HIST_WGS = 5, CMP_FINAL_COLS = 64;                // k_c_final: 64 bins per workgroup, then one for the sums

struct CmpSlot {                       // one slot of the table; {key, count, start} is one 16-byte load
	uint64_t key;                      // compare_key of the cell, or COMPARE_EMPTY_KEY
	uint32_t count;                    // valid samples of `b` in the cell
	uint32_t start;                    // the cell's first grid record
};
struct CmpHeader {
	uint32_t cursor;                   // k_c_ranges: grid records handed out
	uint32_t run;                      // k_c_decide: the test pass runs
	uint32_t pad[62];
};
struct CmpPart {                       // one per workgroup; each kernel writes its own fields
	uint64_t invalidB;                 // k_c_insert
	uint64_t cells, maxPop;            // k_c_ranges
	uint64_t invalidA, candidates;     // k_c_count
	uint64_t matched, within, maxD2;   // k_c_test (maxD2: the double's bits)
	uint32_t hist[CMP_HIST_WORDS];     // k_c_test
};
static_assert(sizeof(CmpSlot) == 16 && sizeof(CmpHeader) == 256 && sizeof(CmpPart) == 1104, "compare scratch records");
static_assert(COMPARE_BINS <= CMP_HIST_WORDS && CMP_FINAL_HIST_WGS * CMP_FINAL_COLS >= COMPARE_BINS, "compare histogram");

// the scratch buffer: offsets in bytes, each a multiple of 16
struct CmpLayout {
	uint64_t slots, table, slotOf, rank, cells, parts, bytes;
	explicit CmpLayout(uint64_t numB) {
		slots = compare_table_slots(numB);
		table = sizeof(CmpHeader);
		slotOf = table + slots * sizeof(CmpSlot);
		rank = slotOf + numB * sizeof(uint64_t);
		cells = (rank + numB * sizeof(uint32_t) + 15u) / 16u * 16u;
		parts = cells + numB * sizeof(u32x4);
		bytes = parts + (uint64_t)CMP_MAX_PARTS * sizeof(CmpPart);
	}
};

struct CmpArgs {
	const u32x4* a;
	const u32x4* b;
	uint64_t numA, numB;
	uint8_t* scratch;
	uint64_t slots, table, slotOf, rank, cells, parts;
	uint32_t log2Slots;
	uint32_t gridA, gridB, gridS;      // the grids of the kernels over `a`, over `b` and over the slots
	uint32_t countOnly, missColor;
	double   min[3], inv, rr;
	uint64_t maxCandidates;
	SimlodCompareRecord* records;
	uint32_t* colors;
	SimlodCompareSummary* summary;
};
struct CmpTestArgs {
	CmpArgs  c;
	double   t2[COMPARE_THRESHOLDS];
	uint32_t table[256];
};
static_assert(sizeof(CmpTestArgs) <= 4096, "k_c_test: the kernel arguments");

__device__ __forceinline__ CmpHeader* header_of(const CmpArgs& c) { return reinterpret_cast<CmpHeader*>(c.scratch); }
__device__ __forceinline__ CmpSlot* table_of(const CmpArgs& c) { return reinterpret_cast<CmpSlot*>(c.scratch + c.table); }
__device__ __forceinline__ CmpPart* parts_of(const CmpArgs& c) { return reinterpret_cast<CmpPart*>(c.scratch + c.parts); }

// the sum / the maximum of v over the workgroup, in every lane; sh: CMP_WAVES words of LDS that may be in use by an earlier call
template <bool MAX>
__device__ __forceinline__ uint64_t block_reduce(uint64_t v, uint64_t* sh) {
#pragma unroll
	for (int o = SIMLOD_WAVE / 2; o >= 1; o >>= 1) {
		const uint64_t t = (uint64_t)__shfl_xor((unsigned long long)v, o, SIMLOD_WAVE);
		v = MAX ? (t > v ? t : v) : v + t;
	}
	__syncthreads();
	if (lane_id() == 0) sh[threadIdx.x / SIMLOD_WAVE] = v;
	__syncthreads();
	uint64_t r = sh[0];
#pragma unroll
	for (uint32_t w = 1; w < CMP_WAVES; w++) r = MAX ? (sh[w] > r ? sh[w] : r) : r + sh[w];
	return r;
}

// rule C4: the three cells of a valid sample
__device__ __forceinline__ void cells_of(const CmpArgs& c, const u32x4& s, uint32_t (&cell)[3]) {
	cell[0] = summary_cell20(__uint_as_float(s.x), c.min[0], c.inv);
	cell[1] = summary_cell20(__uint_as_float(s.y), c.min[1], c.inv);
	cell[2] = summary_cell20(__uint_as_float(s.z), c.min[2], c.inv);
}

// the slot that holds `key`: linear probing from its home, at most `slots` steps; false when the cell is empty
__device__ __forceinline__ bool find_cell(const CmpArgs& c, const CmpSlot* tab, uint64_t key, uint32_t& start, uint32_t& count) {
	uint64_t p = compare_home(key, c.log2Slots);
	for (uint64_t n = 0; n < c.slots; n++) {
		const u32x4 v = *reinterpret_cast<const u32x4*>(tab + p);
		const uint64_t k = (uint64_t)v.x | (uint64_t)v.y << 32;
		if (k == key) { count = v.z; start = v.w; return true; }
		if (k == COMPARE_EMPTY_KEY) return false;
		p = (p + 1u) & (c.slots - 1u);
	}
	return false;
}

// f(start, count) for each occupied cell among the up to 27 around `cell` (rule C4: an offset that leaves [0, 2^20) is skipped)
template <typename F>
__device__ __forceinline__ void for_neighbour_cells(const CmpArgs& c, const CmpSlot* tab, const uint32_t (&cell)[3], F f) {
#pragma unroll 1
	for (int dz = -1; dz <= 1; dz++) {
		const int z = (int)cell[2] + dz;
		if (z < 0 || z >= (int)COMPARE_CELLS) continue;
#pragma unroll 1
		for (int dy = -1; dy <= 1; dy++) {
			const int y = (int)cell[1] + dy;
			if (y < 0 || y >= (int)COMPARE_CELLS) continue;
#pragma unroll 1
			for (int dx = -1; dx <= 1; dx++) {
				const int x = (int)cell[0] + dx;
				if (x < 0 || x >= (int)COMPARE_CELLS) continue;
				uint32_t start, count;
				if (find_cell(c, tab, compare_key((uint32_t)x, (uint32_t)y, (uint32_t)z), start, count)) f(start, count);
			}
		}
	}
}

__global__ __launch_bounds__(CMP_TPB) void k_c_init(CmpArgs c) {
	u32x4* tab = reinterpret_cast<u32x4*>(c.scratch + c.table);
	for (uint64_t p = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; p < c.slots; p += (uint64_t)gridDim.x * CMP_TPB)
		tab[p] = u32x4{0xffffffffu, 0xffffffffu, 0u, 0u};
	if (blockIdx.x == 0u && threadIdx.x < sizeof(CmpHeader) / 4u) reinterpret_cast<uint32_t*>(c.scratch)[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(CMP_TPB) void k_c_insert(CmpArgs c) {
	__shared__ uint64_t sh[CMP_WAVES];
	CmpSlot* tab = table_of(c);
	uint64_t* slotOf = reinterpret_cast<uint64_t*>(c.scratch + c.slotOf);
	uint32_t* rank = reinterpret_cast<uint32_t*>(c.scratch + c.rank);
	uint64_t invalid = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numB; i += (uint64_t)gridDim.x * CMP_TPB) {
		const u32x4 s = c.b[i];
		uint64_t slot = COMPARE_EMPTY_KEY;
		uint32_t r = 0u;
		if (compare_valid(s.x, s.y, s.z)) {
			uint32_t cell[3];
			cells_of(c, s, cell);
			const uint64_t key = compare_key(cell[0], cell[1], cell[2]);
			uint64_t p = compare_home(key, c.log2Slots);
			for (uint64_t n = 0; n < c.slots; n++) {
				unsigned long long* kp = reinterpret_cast<unsigned long long*>(&tab[p].key);
				unsigned long long old = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (old == COMPARE_EMPTY_KEY) old = atomicCAS(kp, (unsigned long long)COMPARE_EMPTY_KEY, (unsigned long long)key);
				if (old == COMPARE_EMPTY_KEY || old == key) { slot = p; break; }
				p = (p + 1u) & (c.slots - 1u);
			}
			if (slot != COMPARE_EMPTY_KEY) r = atomicAdd(&tab[slot].count, 1u);
		} else {
			invalid++;
		}
		slotOf[i] = slot;
		rank[i] = r;
	}
	invalid = block_reduce<false>(invalid, sh);
	if (threadIdx.x == 0u) parts_of(c)[blockIdx.x].invalidB = invalid;
}

__global__ __launch_bounds__(CMP_TPB) void k_c_ranges(CmpArgs c) {
	__shared__ uint64_t sh[CMP_WAVES];
	__shared__ uint32_t sh_wave[CMP_WAVES], sh_base;
	CmpSlot* tab = table_of(c);
	const int lane = lane_id();
	const uint32_t w = threadIdx.x / SIMLOD_WAVE;
	uint64_t cells = 0u, maxPop = 0u;
	// (the bound is the same for the whole workgroup: every lane reaches the barriers)
	for (uint64_t base = (uint64_t)blockIdx.x * CMP_RANGE_SLOTS; base < c.slots; base += (uint64_t)gridDim.x * CMP_RANGE_SLOTS) {
		uint32_t cnt[CMP_RANGE_PER_LANE], mine = 0u;
#pragma unroll
		for (uint32_t j = 0; j < CMP_RANGE_PER_LANE; j++) {                      // (the loads of a lane are independent: all in flight at once)
			const uint64_t p = base + (uint64_t)j * CMP_TPB + threadIdx.x;
			const u32x4 v = p < c.slots ? *reinterpret_cast<const u32x4*>(tab + p) : u32x4{0xffffffffu, 0xffffffffu, 0u, 0u};
			cnt[j] = (v.x & v.y) != 0xffffffffu ? v.z : 0u;                     // (a key has 60 bits: only the empty one is all ones)
			mine += cnt[j];
		}
		uint32_t incl = mine;
#pragma unroll
		for (int o = 1; o < SIMLOD_WAVE; o <<= 1) {
			const uint32_t t = (uint32_t)__shfl_up((int)incl, o, SIMLOD_WAVE);
			if (lane >= o) incl += t;
		}
		if (lane == SIMLOD_WAVE - 1) sh_wave[w] = incl;
		__syncthreads();
		if (threadIdx.x == 0u) {
			uint32_t total = 0u;
			for (uint32_t k = 0; k < CMP_WAVES; k++) total += sh_wave[k];
			sh_base = total != 0u ? atomicAdd(&header_of(c)->cursor, total) : 0u;
		}
		__syncthreads();
		if (mine != 0u) {
			uint32_t start = sh_base + incl - mine;
			for (uint32_t k = 0; k < w; k++) start += sh_wave[k];
#pragma unroll
			for (uint32_t j = 0; j < CMP_RANGE_PER_LANE; j++) {
				if (cnt[j] == 0u) continue;                                     // (then the slot exists: a slot past the table counts nothing)
				tab[base + (uint64_t)j * CMP_TPB + threadIdx.x].start = start;
				start += cnt[j];
				cells++;
				maxPop = cnt[j] > maxPop ? cnt[j] : maxPop;
			}
		}
		__syncthreads();                                                       // (sh_wave and sh_base are written again)
	}
	cells = block_reduce<false>(cells, sh);
	maxPop = block_reduce<true>(maxPop, sh);
	if (threadIdx.x == 0u) { CmpPart* part = parts_of(c) + blockIdx.x; part->cells = cells; part->maxPop = maxPop; }
}

__global__ __launch_bounds__(CMP_TPB) void k_c_fill(CmpArgs c) {
	const CmpSlot* tab = table_of(c);
	const uint64_t* slotOf = reinterpret_cast<const uint64_t*>(c.scratch + c.slotOf);
	const uint32_t* rank = reinterpret_cast<const uint32_t*>(c.scratch + c.rank);
	u32x4* cells = reinterpret_cast<u32x4*>(c.scratch + c.cells);
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numB; i += (uint64_t)gridDim.x * CMP_TPB) {
		const uint64_t slot = slotOf[i];
		if (slot >= c.slots) continue;                                          // an invalid sample
		// Inside the array: k_c_insert added 1 to the slot's count once per valid sample and kept the old value, so rank < count; k_c_ranges
		// gave the slots disjoint ranges [start, start + count) from a cursor that ends at the number of valid samples, at most numB.
		const uint64_t pos = (uint64_t)tab[slot].start + rank[i];
		const u32x4 s = c.b[i];
		cells[pos] = u32x4{s.x, s.y, s.z, (uint32_t)i};
	}
}

__global__ __launch_bounds__(CMP_TPB) void k_c_count(CmpArgs c) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpSlot* tab = table_of(c);
	uint64_t invalid = 0u, candidates = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numA; i += (uint64_t)gridDim.x * CMP_TPB) {
		const u32x4 s = c.a[i];
		if (!compare_valid(s.x, s.y, s.z)) { invalid++; continue; }
		uint32_t cell[3];
		cells_of(c, s, cell);
		for_neighbour_cells(c, tab, cell, [&](uint32_t, uint32_t count) { candidates += count; });
	}
	invalid = block_reduce<false>(invalid, sh);
	candidates = block_reduce<false>(candidates, sh);
	if (threadIdx.x == 0u) { CmpPart* part = parts_of(c) + blockIdx.x; part->invalidA = invalid; part->candidates = candidates; }
}

__global__ __launch_bounds__(CMP_TPB) void k_c_decide(CmpArgs c) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpPart* parts = parts_of(c);
	uint64_t invalidB = 0u, cells = 0u, maxPop = 0u, invalidA = 0u, candidates = 0u;
	for (uint32_t p = threadIdx.x; p < c.gridB; p += CMP_TPB) invalidB += parts[p].invalidB;
	for (uint32_t p = threadIdx.x; p < c.gridS; p += CMP_TPB) { cells += parts[p].cells; maxPop = parts[p].maxPop > maxPop ? parts[p].maxPop : maxPop; }
	for (uint32_t p = threadIdx.x; p < c.gridA; p += CMP_TPB) { invalidA += parts[p].invalidA; candidates += parts[p].candidates; }
	invalidB = block_reduce<false>(invalidB, sh);
	cells = block_reduce<false>(cells, sh);
	maxPop = block_reduce<true>(maxPop, sh);
	invalidA = block_reduce<false>(invalidA, sh);
	candidates = block_reduce<false>(candidates, sh);
	SimlodCompareSummary* out = c.summary;
	for (uint32_t i = threadIdx.x; i < COMPARE_BINS; i += CMP_TPB) out->hist[i] = 0u;
	if (threadIdx.x == 0u) {
		const bool over = c.maxCandidates != 0u && candidates > c.maxCandidates;    // rule C6
		header_of(c)->run = (c.countOnly == 0u && !over) ? 1u : 0u;
		out->error = over ? SIMLOD_COMPARE_ERR_BUDGET : 0u;
		out->numCells = (uint32_t)cells;
		out->maxCellPopulation = (uint32_t)maxPop;
		out->numInvalidA = (uint32_t)invalidA;
		out->numInvalidB = (uint32_t)invalidB;
		out->numMatched = 0u;
		out->numWithin = 0u;
		out->numCandidates = candidates;
		out->maxD2 = 0.0;
	}
}

__global__ __launch_bounds__(CMP_TPB) void k_c_test(CmpTestArgs t) {
	__shared__ double sh_t2[COMPARE_THRESHOLDS + 1u];
	__shared__ uint32_t sh_table[256];
	__shared__ uint32_t sh_hist[CMP_HIST_WORDS];
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = t.c;
	if (header_of(c)->run == 0u) return;                                        // rules C6, C7 (the same for every workgroup)
	for (uint32_t i = threadIdx.x; i < COMPARE_THRESHOLDS; i += CMP_TPB) sh_t2[i] = t.t2[i];
	for (uint32_t i = threadIdx.x; i < 256u; i += CMP_TPB) sh_table[i] = t.table[i];
	for (uint32_t i = threadIdx.x; i < CMP_HIST_WORDS; i += CMP_TPB) sh_hist[i] = 0u;
	__syncthreads();
	const CmpSlot* tab = table_of(c);
	const u32x4* cells = reinterpret_cast<const u32x4*>(c.scratch + c.cells);
	uint64_t matched = 0u, withinSum = 0u, maxD2 = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numA; i += (uint64_t)gridDim.x * CMP_TPB) {
		const u32x4 s = c.a[i];
		double best = __longlong_as_double((long long)COMPARE_MISS_D2_BITS);
		uint32_t nearest = COMPARE_MISS, within = 0u;
		if (compare_valid(s.x, s.y, s.z)) {
			uint32_t cell[3];
			cells_of(c, s, cell);
			const double cx = (double)__uint_as_float(s.x), cy = (double)__uint_as_float(s.y), cz = (double)__uint_as_float(s.z);
			for_neighbour_cells(c, tab, cell, [&](uint32_t start, uint32_t count) {
				const uint64_t end = (uint64_t)start + count;                   // (at most numB: k_c_fill's argument)
				for (uint64_t j = start; j < end; j++) {
					const u32x4 v = cells[j];
					const double d2 = compare_d2((double)__uint_as_float(v.x), (double)__uint_as_float(v.y), (double)__uint_as_float(v.z), cx, cy, cz);
					if (d2 <= c.rr) {                                           // rule C2
						within++;
						if (d2 < best || (d2 == best && v.w < nearest)) { best = d2; nearest = v.w; }   // rule C3: (d2, index)
					}
				}
			});
		}
		const uint32_t bin = within != 0u ? compare_index(sh_t2, best) : 256u;  // rule C5
		const uint64_t bits = (uint64_t)__double_as_longlong(best);
		*reinterpret_cast<u32x4*>(c.records + i) = u32x4{(uint32_t)bits, (uint32_t)(bits >> 32), nearest, within};
		if (c.colors != nullptr) c.colors[i] = bin < 256u ? sh_table[bin] : c.missColor;
		atomicAdd(&sh_hist[bin], 1u);
		if (within != 0u) { matched++; withinSum += within; maxD2 = bits > maxD2 ? bits : maxD2; }
	}
	matched = block_reduce<false>(matched, sh);
	withinSum = block_reduce<false>(withinSum, sh);
	maxD2 = block_reduce<true>(maxD2, sh);                                      // (its barriers: the histogram's atomics are done as well)
	CmpPart* part = parts_of(c) + blockIdx.x;
	if (threadIdx.x == 0u) { part->matched = matched; part->within = withinSum; part->maxD2 = maxD2; }
	for (uint32_t i = threadIdx.x; i < CMP_HIST_WORDS; i += CMP_TPB) part->hist[i] = sh_hist[i];
}

// Workgroup g < CMP_FINAL_HIST_WGS owns bins 64g .. 64g + 63: lane l adds bin 64g + l % 64 over the parts l / 64, l / 64 + 4, ..., and the four
// groups' sums meet in LDS; the last workgroup owns numMatched, numWithin and maxD2.  Every word is written by one lane of one workgroup.
__global__ __launch_bounds__(CMP_TPB) void k_c_final(CmpArgs c) {
	__shared__ uint64_t sh_bins[CMP_WAVES][CMP_FINAL_COLS];
	__shared__ uint64_t sh[CMP_WAVES];
	if (header_of(c)->run == 0u) return;
	const CmpPart* parts = parts_of(c);
	if (blockIdx.x < CMP_FINAL_HIST_WGS) {
		const uint32_t col = threadIdx.x % CMP_FINAL_COLS, g = threadIdx.x / CMP_FINAL_COLS, bin = blockIdx.x * CMP_FINAL_COLS + col;
		uint64_t h = 0u;
		if (bin < COMPARE_BINS)
			for (uint32_t p = g; p < c.gridA; p += CMP_WAVES) h += parts[p].hist[bin];
		sh_bins[g][col] = h;
		__syncthreads();
		if (g == 0u && bin < COMPARE_BINS) {
			uint64_t r = sh_bins[0][col];
			for (uint32_t k = 1; k < CMP_WAVES; k++) r += sh_bins[k][col];
			c.summary->hist[bin] = r;
		}
		return;
	}
	uint64_t matched = 0u, within = 0u, maxD2 = 0u;
	for (uint32_t p = threadIdx.x; p < c.gridA; p += CMP_TPB) {
		matched += parts[p].matched; within += parts[p].within;
		maxD2 = parts[p].maxD2 > maxD2 ? parts[p].maxD2 : maxD2;
	}
	matched = block_reduce<false>(matched, sh);
	within = block_reduce<false>(within, sh);
	maxD2 = block_reduce<true>(maxD2, sh);
	if (threadIdx.x == 0u) {
		c.summary->numMatched = (uint32_t)matched;
		c.summary->numWithin = within;
		c.summary->maxD2 = __longlong_as_double((long long)maxD2);
	}
}
static_assert(CMP_FINAL_COLS == SIMLOD_WAVE, "k_c_final: a wave per part group");

// the workgroups of a kernel with a lane per item of `work`: 8 per CU, but at most CMP_MAX_PARTS (on the 256 CUs of an MI355X that bound
// decides: four per CU, the best single limit measured) and at most `limit`
uint32_t compare_grid(uint64_t work, uint32_t limit) {
	uint64_t g = std::min<uint64_t>((uint64_t)device_info().numCUs * 8u, CMP_MAX_PARTS);
	g = std::min<uint64_t>(g, (work + CMP_TPB - 1u) / CMP_TPB);
	if (limit != 0u) g = std::min<uint64_t>(g, limit);
	return (uint32_t)std::max<uint64_t>(g, 1u);
}

inline bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1u)) == 0u; }

// what the compare call and the surface call share: the fields of their params records the grid needs
struct CmpCall {
	float    radius;
	uint32_t missColor;
	uint64_t maxCandidates;
	uint32_t maxWorkgroups;
};

// the checks of everything but the params record (already accepted), and the arguments of the grid's kernels; false: refused.  Enqueues nothing.
bool compare_prepare(const SimlodUniforms* u, const SimlodPoint* a, uint64_t numA, const SimlodPoint* b, uint64_t numB, const CmpCall& call, void* scratch,
                     uint64_t scratchBytes, const void* records, uint32_t* colors, SimlodCompareSummary* summary, CmpArgs& c) {
	if (u == nullptr || a == nullptr || b == nullptr || scratch == nullptr || summary == nullptr) return false;
	if (records == nullptr && colors != nullptr) return false;
	if (!compare_count_acceptable(numA) || !compare_count_acceptable(numB)) return false;
	if (!aligned(a, 16) || !aligned(b, 16) || !aligned(scratch, 16) || !aligned(records, 16) || !aligned(colors, 4) || !aligned(summary, 8)) return false;
	float size, mn[3];
	octree_box(u, size, mn[0], mn[1], mn[2]);
	if (!compare_box_acceptable(mn, size)) return false;
	const CmpLayout lay(numB);
	if (scratchBytes < lay.bytes) return false;
	c.a = reinterpret_cast<const u32x4*>(a); c.b = reinterpret_cast<const u32x4*>(b); c.numA = numA; c.numB = numB;
	c.scratch = reinterpret_cast<uint8_t*>(scratch);
	c.slots = lay.slots; c.table = lay.table; c.slotOf = lay.slotOf; c.rank = lay.rank; c.cells = lay.cells; c.parts = lay.parts;
	c.log2Slots = compare_log2(lay.slots);
	c.gridA = compare_grid(numA, call.maxWorkgroups); c.gridB = compare_grid(numB, call.maxWorkgroups);
	c.gridS = compare_grid((lay.slots + CMP_RANGE_PER_LANE - 1u) / CMP_RANGE_PER_LANE, call.maxWorkgroups);
	c.countOnly = records == nullptr ? 1u : 0u; c.missColor = call.missColor;
	for (int k = 0; k < 3; k++) c.min[k] = (double)mn[k];
	c.inv = compare_inv(call.radius, size);
	c.rr = (double)call.radius * (double)call.radius;
	c.maxCandidates = call.maxCandidates;
	c.records = nullptr; c.colors = colors; c.summary = summary;
	return true;
}

// the grid over `b` and rule C6's decision: k_c_init .. k_c_decide
void launch_grid(const CmpArgs& c, hipStream_t stream) {
	SIMLOD_LAUNCH(k_c_init, dim3(c.gridS), dim3(CMP_TPB), stream, c);
	SIMLOD_LAUNCH(k_c_insert, dim3(c.gridB), dim3(CMP_TPB), stream, c);
	SIMLOD_LAUNCH(k_c_ranges, dim3(c.gridS), dim3(CMP_TPB), stream, c);
	if (c.countOnly == 0u) SIMLOD_LAUNCH(k_c_fill, dim3(c.gridB), dim3(CMP_TPB), stream, c);
	SIMLOD_LAUNCH(k_c_count, dim3(c.gridA), dim3(CMP_TPB), stream, c);
	SIMLOD_LAUNCH(k_c_decide, dim3(1), dim3(CMP_TPB), stream, c);
}

#include "compare_surface.inc"
#include "compare_cluster.inc"
#include "compare_align.inc"

}  // namespace

uint64_t compare_slots(uint64_t numB) { return compare_count_acceptable(numB) ? compare_table_slots(numB) : 0u; }

uint64_t compare_min_bytes(uint64_t numA, uint64_t numB) {
	return compare_count_acceptable(numA) && compare_count_acceptable(numB) ? CmpLayout(numB).bytes : 0u;
}

// simlod_compare_samples: the checks (nothing is enqueued before the last of them), then the launches listed at the top.
int launch_compare(const SimlodUniforms* u, const SimlodPoint* a, uint64_t numA, const SimlodPoint* b, uint64_t numB, const SimlodCompareParams* params,
                   void* scratch, uint64_t scratchBytes, SimlodCompareRecord* records, uint32_t* colors, SimlodCompareSummary* summary, hipStream_t stream) {
	if (params == nullptr || !compare_acceptable(*params)) return (int)hipErrorInvalidValue;
	CmpTestArgs t{};
	CmpArgs& c = t.c;
	const CmpCall call{params->radius, params->missColor, params->maxCandidates, params->maxWorkgroups};
	if (!compare_prepare(u, a, numA, b, numB, call, scratch, scratchBytes, records, colors, summary, c)) return (int)hipErrorInvalidValue;
	c.records = records;
	for (uint32_t i = 0; i < COMPARE_THRESHOLDS; i++) t.t2[i] = params->thresholds2[i];
	for (uint32_t i = 0; i < 256u; i++) t.table[i] = params->table[i];
	launch_grid(c, stream);
	if (records != nullptr) {
		SIMLOD_LAUNCH(k_c_test, dim3(c.gridA), dim3(CMP_TPB), stream, t);
		SIMLOD_LAUNCH(k_c_final, dim3(CMP_FINAL_HIST_WGS + 1u), dim3(CMP_TPB), stream, c);
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

// simlod_surface_samples: the same checks and the same six launches, then compare_surface.inc's two.
int launch_surface(const SimlodUniforms* u, const SimlodPoint* a, uint64_t numA, const SimlodPoint* b, uint64_t numB, const SimlodSurfaceParams* params,
                   void* scratch, uint64_t scratchBytes, SimlodSurfaceRecord* records, uint32_t* colors, SimlodSurfaceSummary* summary, hipStream_t stream) {
	if (params == nullptr || !surface_acceptable(*params)) return (int)hipErrorInvalidValue;
	SurfTestArgs t{};
	CmpArgs& c = t.c;
	const CmpCall call{params->radius, params->missColor, params->maxCandidates, params->maxWorkgroups};
	// (the summary has SimlodCompareSummary's layout: k_c_decide writes it as it is, numDegenerate = 0 being maxD2 = 0.0's bits)
	if (!compare_prepare(u, a, numA, b, numB, call, scratch, scratchBytes, records, colors, reinterpret_cast<SimlodCompareSummary*>(summary), c))
		return (int)hipErrorInvalidValue;
	float size, mn[3];
	octree_box(u, size, mn[0], mn[1], mn[2]);
	t.records = records;
	t.invq = surface_invq(params->radius, size);
	t.colourBy = params->colourBy; t.orientMode = params->orientMode;
	for (int k = 0; k < 3; k++) { t.light[k] = (double)params->light[k]; t.orient[k] = (double)params->orient[k]; }
	for (uint32_t i = 0; i < SURFACE_THRESHOLDS; i++) t.thresholds[i] = params->thresholds[i];
	for (uint32_t i = 0; i < 256u; i++) t.table[i] = params->table[i];
	launch_grid(c, stream);
	if (records != nullptr) {
		SIMLOD_LAUNCH(k_s_test, dim3(c.gridA), dim3(CMP_TPB), stream, t);
		SIMLOD_LAUNCH(k_s_final, dim3(CMP_FINAL_HIST_WGS + 1u), dim3(CMP_TPB), stream, c);
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t cluster_min_bytes(uint64_t numA) { return cluster_bytes(numA); }

// simlod_cluster_samples: compare_cluster.inc's launcher.
int launch_cluster(const SimlodUniforms* u, const SimlodPoint* a, uint64_t numA, const SimlodClusterParams* params, void* scratch, uint64_t scratchBytes,
                   SimlodClusterRecord* records, uint32_t* colors, SimlodClusterSummary* summary, hipStream_t stream) {
	return launch_cluster_impl(u, a, numA, params, scratch, scratchBytes, records, colors, summary, stream);
}

uint64_t align_min_bytes(uint64_t numA, uint64_t numB) {
	return compare_count_acceptable(numA) && compare_count_acceptable(numB) ? align_bytes(numB) : 0u;
}

// simlod_align_samples: compare_align.inc's launcher.
int launch_align(const SimlodUniforms* u, const SimlodPoint* a, uint64_t numA, const SimlodPoint* b, uint64_t numB, const SimlodAlignParams* params,
                 void* scratch, uint64_t scratchBytes, SimlodCompareRecord* records, SimlodAlignSummary* summary, hipStream_t stream) {
	return launch_align_impl(u, a, numA, b, numB, params, scratch, scratchBytes, records, summary, stream);
}

}  // namespace simlod
