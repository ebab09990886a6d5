// align_rules.hpp — the align queries' rules A1-A7 and their refusals (include/simlod_hip.h, "align queries"): what a SimlodAlignParams record
// must be to be accepted, the pose applied to a sample, the cell of a posed centre (the double-input twin of summary_cell20), the 24-bit
// quantisation Q, the lo/hi split of a product, and the stamp a build call leaves in the scratch header with the comparison a reuse call
// makes.  No HIP in here, and nothing of the library's other headers but the ABI's structs and compare_rules.hpp, whose validity of `b`, h,
// key and d2's order of operations ARE rules A1-A3's and are not restated: compare_align.inc's kernels and launcher and
// tests/host/align_rules_check.cpp (plain g++) read it here.  Every operation is an fp64 add, subtract, multiply or compare, an integer
// operation or a conversion, with no fused multiply-add (the library is built with -ffp-contract=off; the host program likewise), so that the
// numpy mirror (simlod_amd/octree_io.py align_samples) reproduces every record and every sum bit for bit.
#pragma once
#include <stdint.h>
#include <cmath>
#include "simlod_hip.h"
#include "compare_rules.hpp"

namespace simlod {

constexpr double   ALIGN_Q_SCALE = 16777216.0;                                // rule A4: Q has 24 bits
constexpr uint32_t ALIGN_KNOWN_FLAGS = SIMLOD_ALIGN_COUNT_ONLY | SIMLOD_ALIGN_REUSE_GRID;
constexpr uint32_t ALIGN_STAMP_MAGIC = 0x414c4753u;                           // rule A7: "ALGS"

// the refusals of the record itself: radius (rule C1), gridRadius (rule A2), the pose (rule A1), the flags, the reserved word
inline bool align_acceptable(const SimlodAlignParams& p) {
	if (!std::isfinite(p.radius) || !(p.radius >= 0.0f) || !std::isfinite(p.gridRadius) || !(p.gridRadius >= p.radius)) return false;
	if ((p.flags & ~ALIGN_KNOWN_FLAGS) != 0u || p.reserved != 0u) return false;
	for (int k = 0; k < 12; k++)
		if (!std::isfinite(p.pose[k])) return false;
	return true;
}

// rule A4: the launcher's factor, one IEEE division on the host
inline double align_invq(float size) { return ALIGN_Q_SCALE / (double)size; }

SIMLOD_HD inline uint64_t align_bits(double d) {
	union { double d; uint64_t u; } v;
	v.d = d;
	return v.u;
}
SIMLOD_HD inline bool align_is_finite(double d) { return (align_bits(d) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// rule A1: c' from the widened sample (cx, cy, cz) and the pose T (3x4, row-major); false: a c'_k is not finite (the inputs are finite)
SIMLOD_HD inline bool align_pose(const double (&T)[12], double cx, double cy, double cz, double (&out)[3]) {
	out[0] = ((T[0] * cx + T[1] * cy) + T[2] * cz) + T[3];
	out[1] = ((T[4] * cx + T[5] * cy) + T[6] * cz) + T[7];
	out[2] = ((T[8] * cx + T[9] * cy) + T[10] * cz) + T[11];
	return align_is_finite(out[0]) && align_is_finite(out[1]) && align_is_finite(out[2]);
}

// rule A2: the 20-bit cell of the fp64 coordinate x — summary_cell20 with a double in the place of the widened float
SIMLOD_HD inline uint32_t align_cell20(double x, double boxMin, double inv) {
	const double t = (x - boxMin) * inv;
	return t >= (double)(COMPARE_CELLS - 1u) ? COMPARE_CELLS - 1u : t > 0.0 ? (uint32_t)t : 0u;
}

// rule A4: whether x is inside on an axis that starts at boxMin, and then its 24-bit Q
SIMLOD_HD inline bool align_q(double x, double boxMin, double invq, uint32_t& q) {
	const double t = (x - boxMin) * invq;
	const bool inside = t >= 0.0 && t < ALIGN_Q_SCALE;
	q = inside ? (uint32_t)t : 0u;
	return inside;
}

// rule A5: the two words a product or a squared residual is summed as
SIMLOD_HD inline uint64_t align_lo(uint64_t p) { return p & 0xffffffffull; }
SIMLOD_HD inline uint64_t align_hi(uint64_t p) { return p >> 32; }
// rule A5: E from the six Q of a pair
SIMLOD_HD inline uint64_t align_sq(const uint32_t (&qa)[3], const uint32_t (&qb)[3]) {
	const int64_t ex = (int64_t)qb[0] - (int64_t)qa[0], ey = (int64_t)qb[1] - (int64_t)qa[1], ez = (int64_t)qb[2] - (int64_t)qa[2];
	return (uint64_t)((ex * ex + ey * ey) + ez * ez);
}

// rule A7: what a build call writes into the scratch header's unused words (62 of them, at byte 8), and what a reuse call holds against it
struct AlignStamp {
	uint32_t magic;                    // ALIGN_STAMP_MAGIC
	uint32_t filled;                   // 1: the grid records were written (a build call with results)
	uint64_t b, numB;                  // the array the grid is over
	uint64_t inv, min[3];              // the bits of rule A2's inv and of the box's corner
	uint64_t numCells, maxCellPopulation, numInvalidB;   // the grid's totals, for the reuse call's summary
};
static_assert(sizeof(AlignStamp) == 80 && sizeof(AlignStamp) <= 62u * 4u, "AlignStamp: it fits the scratch header's unused words");

inline AlignStamp align_stamp(const void* b, uint64_t numB, double inv, const double (&mn)[3], bool filled) {
	AlignStamp s{};
	s.magic = ALIGN_STAMP_MAGIC; s.filled = filled ? 1u : 0u;
	s.b = (uint64_t)reinterpret_cast<uintptr_t>(b); s.numB = numB;
	s.inv = align_bits(inv);
	for (int k = 0; k < 3; k++) s.min[k] = align_bits(mn[k]);
	return s;
}
// the stamp `have` found in the buffer serves the call that would have written `want`: the same grid, and filled if `want` needs the records
// (the totals are not compared: they are the stamp's to give)
SIMLOD_HD inline bool align_stamp_serves(const AlignStamp& have, const AlignStamp& want) {
	return have.magic == ALIGN_STAMP_MAGIC && have.b == want.b && have.numB == want.numB && have.inv == want.inv && have.min[0] == want.min[0] &&
	       have.min[1] == want.min[1] && have.min[2] == want.min[2] && (have.filled == 1u || (have.filled == 0u && want.filled == 0u));
}

}  // namespace simlod
