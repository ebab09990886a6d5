// paint_rules.hpp — the paint regions' rules E1-E3 and E9 (include/simlod_hip.h, "paint regions"): what a SimlodPaint record must be to be accepted,
// and the colour word a painted sample gets.  No HIP in here, and nothing of the library's other headers but the ABI's structs:
// export_paint.inc's kernels, the launcher (export.hip) and tests/host/paint_rules_check.cpp (plain g++) read it here.  The ramp's fp64 product
// is formed without a fused multiply-add (the library is built with -ffp-contract=off; the host program likewise), so that the numpy mirror
// (simlod_amd/octree_io.py OctreeExport.paint) reproduces every colour bit for bit.
// (las_style_rules.hpp has no value-to-index step to share: simlod_decode_las_styled forms its index inside the decode kernel, loader.hip, with
// t < 256 where rule E3 says t >= 255 — the same index for every t.)
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

// rule E9's refusals of the record itself; haveColors: the call's `colors` is not null
inline bool paint_acceptable(const SimlodPaint& p, bool haveColors) {
	if (p.mode > SIMLOD_PAINT_ARRAY || p.reserved != 0u || p.reserved2[0] != 0u || p.reserved2[1] != 0u) return false;
	if (p.mode == SIMLOD_PAINT_BLEND && (p.strength < 1u || p.strength > 255u)) return false;
	if (p.mode == SIMLOD_PAINT_RAMP && (!std::isfinite(p.z0) || !std::isfinite(p.scale) || !(p.scale > 0.0f))) return false;
	if (p.mode == SIMLOD_PAINT_ARRAY && !haveColors) return false;
	return true;
}

// rule E2: bytes 0..2 move towards those of `color` by a / 256, byte 3 stays
SIMLOD_HD inline uint32_t paint_blend(uint32_t c, uint32_t color, uint32_t a) {
	uint32_t out = c & 0xff000000u;
	for (uint32_t sh = 0u; sh < 24u; sh += 8u) {
		const uint32_t old = (c >> sh) & 0xffu, t = (color >> sh) & 0xffu;
		out |= ((old * (256u - a) + t * a + 128u) >> 8) << sh;
	}
	return out;
}

// rule E3: the table index of a sample's z
SIMLOD_HD inline uint32_t paint_ramp_index(float z, float z0, float scale) {
	const double t = ((double)z - (double)z0) * (double)scale;
	return t >= 255.0 ? 255u : t > 0.0 ? (uint32_t)t : 0u;               // a NaN: 0
}

}  // namespace simlod
