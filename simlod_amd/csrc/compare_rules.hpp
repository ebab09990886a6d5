// compare_rules.hpp — the compare queries' rules C1-C5 and their refusals (include/simlod_hip.h, "compare queries"): what a SimlodCompareParams
// record and a box must be to be accepted, the grid's cell size h and its inverse, the 60-bit key of a cell, the home slot of a key in a hash
// table of a power-of-two capacity, the threshold index of a squared distance, and the miss record's constants.  No HIP in here, and nothing of
// the library's other headers but the ABI's structs and summary_rules.hpp, whose summary_cell20 IS rule C4's cell and is not restated:
// compare.hip's kernels and launcher and tests/host/compare_rules_check.cpp (plain g++) read it here.  fp64 from the fp32 inputs, in the order
// the header states and with no fused multiply-add (the library is built with -ffp-contract=off; the host program likewise), so that the numpy
// mirror (simlod_amd/octree_io.py compare_samples) reproduces every record and every count bit for bit.
#pragma once
#include <stdint.h>
#include <cmath>
#include "simlod_hip.h"
#include "summary_rules.hpp"

namespace simlod {

constexpr uint32_t COMPARE_CELLS = SUMMARY_CELLS;                             // rule C4: cells per axis
constexpr uint32_t COMPARE_THRESHOLDS = 255u, COMPARE_BINS = 257u;            // rule C5; the last bin: unmatched and invalid samples
constexpr uint32_t COMPARE_MISS = SIMLOD_COMPARE_MISS;                        // rule C3: `nearest` of the miss record
constexpr uint64_t COMPARE_MISS_D2_BITS = 0x7ff0000000000000ull;              // rule C3: +infinity, the d2 of the miss record
constexpr uint64_t COMPARE_MAX_COUNT = 0xfffffffeull;                         // numA, numB: 1 .. 2^32 - 2
constexpr uint64_t COMPARE_EMPTY_KEY = ~0ull;                                 // no cell's key: a key has 60 bits
constexpr uint64_t COMPARE_HASH_MUL = 0x9e3779b97f4a7c15ull;                  // 2^64 / the golden ratio, odd

// the refusals of the record itself: radius (rule C1), thresholds (rule C5), the reserved word
inline bool compare_acceptable(const SimlodCompareParams& p) {
	if (!std::isfinite(p.radius) || !(p.radius >= 0.0f) || p.reserved != 0u) return false;
	for (uint32_t i = 0; i < COMPARE_THRESHOLDS; i++) {
		if (!std::isfinite(p.thresholds2[i])) return false;
		if (i != 0u && !(p.thresholds2[i] >= p.thresholds2[i - 1u])) return false;
	}
	return true;
}

// rule C4's refusals of the box: `size` is the largest fp32 extent, `mn` boxMin
inline bool compare_box_acceptable(const float (&mn)[3], float size) {
	return std::isfinite(mn[0]) && std::isfinite(mn[1]) && std::isfinite(mn[2]) && std::isfinite(size) && size > 0.0f;
}

inline bool compare_count_acceptable(uint64_t n) { return n != 0u && n <= COMPARE_MAX_COUNT; }

// rule C4: the cell size and the launcher's factor, one IEEE division on the host
inline double compare_h(float radius, float size) {
	const double a = (double)radius * (1.0 + 0x1p-10), b = (double)size * 0x1p-20;
	return a > b ? a : b;
}
inline double compare_inv(float radius, float size) { return 1.0 / compare_h(radius, size); }

// the table's capacity for numB samples: the smallest power of two >= 2 * numB (numB acceptable)
inline uint64_t compare_table_slots(uint64_t numB) {
	uint64_t s = 2u;
	while (s < 2u * numB) s <<= 1;
	return s;
}
inline uint32_t compare_log2(uint64_t slots) {
	uint32_t l = 0u;
	while ((1ull << l) < slots) l++;
	return l;
}

// rule C1
SIMLOD_HD inline bool compare_valid(uint32_t xb, uint32_t yb, uint32_t zb) { return summary_is_finite(xb) && summary_is_finite(yb) && summary_is_finite(zb); }

// rule C4: the key of the cell (cx, cy, cz), each below 2^20, and the slot a key's probing starts at in a table of 2^log2Slots slots
// (log2Slots 1 .. 33): the top bits of the key's product with an odd constant
SIMLOD_HD inline uint64_t compare_key(uint32_t cx, uint32_t cy, uint32_t cz) { return (uint64_t)cx | (uint64_t)cy << 20 | (uint64_t)cz << 40; }
SIMLOD_HD inline uint64_t compare_home(uint64_t key, uint32_t log2Slots) { return (key * COMPARE_HASH_MUL) >> (64u - log2Slots); }

// rule C2: the squared distance of the sample s from the centre c (fp32 values widened)
SIMLOD_HD inline double compare_d2(double sx, double sy, double sz, double cx, double cy, double cz) {
	const double px = sx - cx, py = sy - cy, pz = sz - cz;
	return (px * px + py * py) + pz * pz;
}

// rule C5: the number of entries of t2[0 .. 255) that are <= d2, by binary search (d2 is no NaN)
SIMLOD_HD inline uint32_t compare_index(const double* t2, double d2) {
	uint32_t lo = 0u, hi = COMPARE_THRESHOLDS;                                 // the answer lies in [lo, hi]
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (t2[mid] <= d2) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

}  // namespace simlod
