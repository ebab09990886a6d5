// summary_rules.hpp — the summary queries' rules S1-S3 and S8 (include/simlod_hip.h, "summary queries"): what a SimlodSummaryParams record must be
// to be accepted, the total order the extent is taken under, and the 20-bit cell a coordinate falls into for the moments.  No HIP in here, and
// nothing of the library's other headers but the ABI's structs: export_summary.inc's kernels, the launcher (export.hip) and
// tests/host/summary_rules_check.cpp (plain g++) read it here.  The cell's fp64 product is formed without a fused multiply-add (the library is
// built with -ffp-contract=off; the host program likewise), so that the numpy mirror (simlod_amd/octree_io.py OctreeExport.summarize) reproduces
// every count bit for bit.  Rule S3's index is rule E3's, paint_ramp_index of paint_rules.hpp, and is not restated.
#pragma once
#include <stdint.h>
#include <cmath>
#include "simlod_hip.h"
#include "paint_rules.hpp"

namespace simlod {

constexpr uint32_t SUMMARY_CELLS = 1u << 20;                                   // rule S2: cells per axis
constexpr uint32_t SUMMARY_KEY_POS_INF = 0xff800000u;                          // summary_key of +inf: the minimum over no sample
constexpr uint32_t SUMMARY_KEY_NEG_INF = 0x007fffffu;                          // summary_key of -inf: the maximum over no sample

// rule S8's refusals of the record itself
inline bool summary_acceptable(const SimlodSummaryParams& p) {
	return std::isfinite(p.z0) && std::isfinite(p.scale) && p.scale > 0.0f && p.reserved == 0u;
}

// rule S1: the key of a float's bits — unsigned comparison of keys is the total order -inf < ... < -0 < +0 < ... < +inf, the NaNs with the sign
// bit set below -inf and the others above +inf
SIMLOD_HD inline uint32_t summary_key(uint32_t bits) { return bits ^ ((bits >> 31) != 0u ? 0xffffffffu : 0x80000000u); }
SIMLOD_HD inline uint32_t summary_unkey(uint32_t key) { return key ^ ((key >> 31) != 0u ? 0x80000000u : 0xffffffffu); }
SIMLOD_HD inline bool summary_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
SIMLOD_HD inline bool summary_is_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// rule S2: the launcher's factor, one IEEE division on the host
inline double summary_inv(float size) { return (double)SUMMARY_CELLS / (double)size; }

// rule S2: the 20-bit cell of coordinate x on an axis whose box starts at boxMin (a NaN: 0)
SIMLOD_HD inline uint32_t summary_cell20(float x, double boxMin, double inv) {
	const double t = ((double)x - boxMin) * inv;
	return t >= (double)(SUMMARY_CELLS - 1u) ? SUMMARY_CELLS - 1u : t > 0.0 ? (uint32_t)t : 0u;
}

}  // namespace simlod
