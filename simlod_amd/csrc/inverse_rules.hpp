// inverse_rules.hpp — the inverse selections' rules I1, I2 and I9's own refusal (include/simlod_hip.h, "inverse selections"): what a sample's and a
// node's verdict by the POSITIVE query become.  No HIP in here: export_inverse.inc's kernels, the launchers (export.hip) and
// tests/host/inverse_rules_check.cpp (plain g++) read it here.  Nothing is computed anew: the positive verdicts come from the region's, the
// footprint's or the lasso's rules as they stand, and the numpy mirror (simlod_amd/octree_io.py OctreeExport.crop(invert=True)) maps them the same way.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define SIMLOD_HD __host__ __device__
#else
#define SIMLOD_HD
#endif

namespace simlod {

// the classes of a table entry (the numbers of export_common.inc's Q_*); EMPTIED: listed, contributes nothing, its samples are not read
enum : uint32_t { INVERSE_NODE_OUTSIDE = 0u, INVERSE_NODE_FILTERED = 1u, INVERSE_NODE_COPIED = 2u, INVERSE_NODE_EMPTIED = 3u };

// rule I2: the class of a node in the inverse from its final class in the positive query.  Never OUTSIDE: nothing is culled (rule I3).
SIMLOD_HD inline uint32_t inverse_class(uint32_t positive) {
	return positive == INVERSE_NODE_OUTSIDE ? (uint32_t)INVERSE_NODE_COPIED : positive == INVERSE_NODE_COPIED ? (uint32_t)INVERSE_NODE_EMPTIED : (uint32_t)INVERSE_NODE_FILTERED;
}

// rule I1: a sample passes iff it does not pass the positive rule (a NaN coordinate fails that one, so it passes here)
SIMLOD_HD inline bool inverse_passes(bool positive) { return !positive; }

// rule I9's own refusal: a footprint and a lasso in one call
inline bool inverse_polygons_acceptable(const void* footprint, const void* lasso) { return footprint == nullptr || lasso == nullptr; }

}  // namespace simlod
