// clip_rules.hpp — the region rules as the rasteriser's clip uses them (include/simlod_hip.h, "region queries" rules 1, 3 and 4; "clip regions"): what a
// SimlodRegion / SimlodClip must look like to be accepted, the planes widened to fp64, a node's class from (level, X, Y, Z), and the per-sample test one
// plane at a time.  No HIP in here: render.hip's kernels, the C ABI's setter (simlod_hip.cpp) and tests/host/clip_rules_check.cpp (plain g++) read it here.
// fp64 from the fp32 inputs, every sum in the order the header states and no fused multiply-add (the library is built with -ffp-contract=off; the
// host program likewise), so that the numpy mirror (simlod_amd/octree_io.py classify_nodes, OctreeExport.crop) reproduces every decision bit for bit.
// export_region.inc keeps its own classify / passes: see DESIGN §5, "Clip regions".
#pragma once
#include <stdint.h>
#include <cmath>
#include "simlod_hip.h"
#if defined(__HIPCC__)
#define SIMLOD_HD __host__ __device__
#else
#define SIMLOD_HD
#endif

namespace simlod {

enum : uint32_t { CLIP_NODE_OUTSIDE = 0u, CLIP_NODE_FILTERED = 1u, CLIP_NODE_COPIED = 2u };      // (the numbers of export_common.inc's Q_*)

// What simlod_query_region and simlod_context_set_clip refuse in a region: more than 16 planes, a nonzero reserved word, a non-finite coefficient.
inline bool region_acceptable(const SimlodRegion& r) {
	if (r.numPlanes > SIMLOD_REGION_MAX_PLANES || r.reserved[0] != 0u || r.reserved[1] != 0u || r.reserved[2] != 0u) return false;
	for (uint32_t p = 0; p < r.numPlanes; p++)
		for (int k = 0; k < 4; k++) if (!std::isfinite(r.planes[p][k])) return false;
	return true;
}
// ... and in a clip: a mode above SIMLOD_CLIP_HIGHLIGHT, a nonzero reserved word, a region that is refused
inline bool clip_acceptable(const SimlodClip& c) {
	return c.mode <= SIMLOD_CLIP_HIGHLIGHT && c.reserved[0] == 0u && c.reserved[1] == 0u && region_acceptable(c.region);
}

// The clip as a frame's kernels take it (by value, a kernel argument of its own): the box, and the planes widened to fp64 ON THE HOST.
struct ClipArgs {
	uint32_t mode, color, numPlanes, pad;
	double   min[3], size;
	double   pl[SIMLOD_REGION_MAX_PLANES][4];
};
static_assert(sizeof(ClipArgs) == 16 + 32 + 512, "ClipArgs: 560 bytes of kernel arguments");

// box: min = uniforms.boxMin, size = the largest fp32 extent (simlod_internal.hpp octree_box), as the region queries take it
inline ClipArgs clip_args(const SimlodClip& c, float size, float minx, float miny, float minz) {
	ClipArgs k{};
	k.mode = c.mode; k.color = c.color; k.numPlanes = c.region.numPlanes;
	k.min[0] = (double)minx; k.min[1] = (double)miny; k.min[2] = (double)minz; k.size = (double)size;
	for (uint32_t p = 0; p < c.region.numPlanes; p++)
		for (int q = 0; q < 4; q++) k.pl[p][q] = (double)c.region.planes[p][q];
	return k;
}

// rules 1 and 4: the cube of (level, X, Y, Z) inflated by one level-20 cell against every plane.  `pl`: numPlanes rows (nx, ny, nz, d).
SIMLOD_HD inline uint32_t classify_node(const double (&mn)[3], double size, uint32_t numPlanes, const double (*pl)[4], uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	const double s = ldexp(size, -(int)level), e = ldexp(size, -20);                         // (exact: powers of two; 20 = SIMLOD_MAX_DEPTH)
	const uint32_t A[3] = {X, Y, Z};
	double lo[3], hi[3];
	for (int k = 0; k < 3; k++) {
		lo[k] = (mn[k] + (double)A[k] * s) - e;
		hi[k] = (mn[k] + ((double)A[k] + 1.0) * s) + e;
	}
	bool inside = true;
	for (uint32_t p = 0; p < numPlanes; p++) {
		const double nx = pl[p][0], ny = pl[p][1], nz = pl[p][2], d = pl[p][3];
		const double dmax = ((nx * (nx >= 0.0 ? hi[0] : lo[0]) + ny * (ny >= 0.0 ? hi[1] : lo[1])) + nz * (nz >= 0.0 ? hi[2] : lo[2])) + d;
		if (dmax < 0.0) return CLIP_NODE_OUTSIDE;
		const double dmin = ((nx * (nx >= 0.0 ? lo[0] : hi[0]) + ny * (ny >= 0.0 ? lo[1] : hi[1])) + nz * (nz >= 0.0 ? lo[2] : hi[2])) + d;
		inside = inside && dmin >= 0.0;
	}
	return inside ? CLIP_NODE_COPIED : CLIP_NODE_FILTERED;
}

// rule 3, one plane: ((nx*x + ny*y) + nz*z) + d >= 0 with the fp32 coordinates widened to fp64 (a NaN fails)
SIMLOD_HD inline bool plane_passes(const double (&pl)[4], float x, float y, float z) {
	return ((pl[0] * (double)x + pl[1] * (double)y) + pl[2] * (double)z) + pl[3] >= 0.0;
}

// What a frame does with a node of class `cls` under `mode`.  EMPTY: the node counts as holding nothing (r_visible); the others are r_draw's, per item.
enum : uint32_t { CLIP_ACT_NONE = 0u, CLIP_ACT_KEEP_PASSING = 1u, CLIP_ACT_KEEP_FAILING = 2u, CLIP_ACT_COLOUR_PASSING = 3u, CLIP_ACT_COLOUR_ALL = 4u, CLIP_ACT_EMPTY = 5u };
SIMLOD_HD inline uint32_t clip_action(uint32_t mode, uint32_t cls) {
	if (mode == SIMLOD_CLIP_INSIDE) return cls == CLIP_NODE_OUTSIDE ? CLIP_ACT_EMPTY : cls == CLIP_NODE_FILTERED ? CLIP_ACT_KEEP_PASSING : CLIP_ACT_NONE;
	if (mode == SIMLOD_CLIP_OUTSIDE) return cls == CLIP_NODE_COPIED ? CLIP_ACT_EMPTY : cls == CLIP_NODE_FILTERED ? CLIP_ACT_KEEP_FAILING : CLIP_ACT_NONE;
	if (mode == SIMLOD_CLIP_HIGHLIGHT) return cls == CLIP_NODE_COPIED ? CLIP_ACT_COLOUR_ALL : cls == CLIP_NODE_FILTERED ? CLIP_ACT_COLOUR_PASSING : CLIP_ACT_NONE;
	return CLIP_ACT_NONE;
}

}  // namespace simlod
