// pack_rules.hpp — the packed samples' rules K0-K8 (include/simlod_hip.h, "packed samples"): the box a call accepts, a node's frame, the samples
// of a table entry a call touches, a sample's 8-byte record and what the record decodes to.  No HIP in here, and nothing of the library's other
// headers but the ABI's structs: export_pack.inc's kernels, the launchers (export.hip) and tests/host/pack_rules_check.cpp (plain g++) read it
// here.  fp64 from the fp32 inputs, in the order the header states and with no fused multiply-add (the library is built with -ffp-contract=off;
// the host program likewise), so that the numpy mirror (simlod_amd/octree_io.py pack_samples / unpack_samples) reproduces every record and every
// count bit for bit.  The one division (rule K2's k) is formed once per node, by pack_frame.
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

// rule K0
constexpr uint32_t PACK_COLOR_BITS = SIMLOD_PACK_COLOR_BITS, PACK_POINT_BITS = SIMLOD_PACK_POINT_BITS, PACK_VOXEL_BITS = SIMLOD_PACK_VOXEL_BITS;
constexpr uint32_t PACK_SHIFT_X = SIMLOD_PACK_SHIFT_X, PACK_SHIFT_Y = SIMLOD_PACK_SHIFT_Y, PACK_SHIFT_Z = SIMLOD_PACK_SHIFT_Z;
constexpr uint32_t PACK_MAX_LEVEL = 20u;                                  // SIMLOD_MAX_DEPTH
enum : uint32_t { PACK_CLAMPED = 1u, PACK_INEXACT = 2u, PACK_ALPHA = 4u };   // what pack_sample reports of a sample

// the box of a call: min = boxMin, size = the largest fp32 extent (simlod_internal.hpp octree_box), both also widened
struct PackBox { float minf[3], sizef; double min[3], size; };

// rule K7's refusals of the box: false for a corner that is not finite and for a box without extent
inline bool pack_box(const float (&mn)[3], const float (&mx)[3], PackBox& b) {
	for (int a = 0; a < 3; a++)
		if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) return false;
	const float bx = mx[0] - mn[0], by = mx[1] - mn[1], bz = mx[2] - mn[2];
	b.sizef = fmaxf(fmaxf(bx, by), bz);
	if (!std::isfinite(b.sizef) || !(b.sizef > 0.0f)) return false;
	for (int a = 0; a < 3; a++) { b.minf[a] = mn[a]; b.min[a] = (double)mn[a]; }
	b.size = (double)b.sizef;
	return true;
}

// 2^level as fp32, level <= 20
SIMLOD_HD inline float pack_exp2(uint32_t level) {
	const uint32_t bits = (127u + level) << 23;
	float f;
	__builtin_memcpy(&f, &bits, 4);
	return f;
}

// rule K1: ns = size * 2^-level (exact)
SIMLOD_HD inline double pack_node_size(double size, uint32_t level) { return ldexp(size, -(int)level); }

// rules K1, K2 and K4 per node: the fp64 corner, k = 8192 / ns (points) or 128 / ns (voxels), and voxel_centre's fp32 corner
// (simlod_device.hpp voxel_centre, restated: nodeSize = size / 2^level, nmin = ((float)A + 0.0f) * nodeSize + min)
struct PackFrame { double nmin[3], k; float fmin[3]; };
SIMLOD_HD inline PackFrame pack_frame(const PackBox& b, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z, bool leaf) {
	PackFrame f;
	const double ns = pack_node_size(b.size, level);
	const float fns = b.sizef / pack_exp2(level);
	const uint32_t A[3] = {X, Y, Z};
	for (int a = 0; a < 3; a++) {
		f.nmin[a] = b.min[a] + (double)A[a] * ns;
		f.fmin[a] = ((float)A[a] + 0.0f) * fns + b.minf[a];
	}
	f.k = (leaf ? 8192.0 : 128.0) / ns;
	return f;
}

// rule K5 for table entry t: the range [first, first + n) of the sample array (or of the delta array, with `entries`).  false: the entry
// is not touched.  err: rule K7's bits for it — a level above 20 (skipped), a range beyond sampleCap (nothing of it is written).
SIMLOD_HD inline bool pack_entry_range(const SimlodExportNode& e, const SimlodDeltaEntry* de, uint64_t sampleCap, uint64_t& first, uint32_t& n, uint32_t& err) {
	err = 0u;
	if (de != nullptr) {
		if (de->state == SIMLOD_DELTA_NONE) return false;
		first = de->firstDelta; n = de->numDelta;
	} else {
		if ((e.flags & SIMLOD_EXPORT_FLAG_SELECTED) == 0u) return false;
		first = e.firstSample; n = e.numSamples;
	}
	if (n == 0u) return false;
	if (e.level > PACK_MAX_LEVEL) { err = SIMLOD_EXPORT_ERR_NODE_COUNT; return false; }
	if (first > sampleCap || (uint64_t)n > sampleCap - first) { err = SIMLOD_EXPORT_ERR_CAPACITY; return false; }
	return true;
}

// t -> q of rules K2 / K4 (a NaN gives 0); inside: t >= 0 && t < lim
SIMLOD_HD inline uint32_t pack_quantize(double t, double lim, bool& inside) {
	inside = t >= 0.0 && t < lim;
	return t >= 0.0 ? (t < lim ? (uint32_t)t : (uint32_t)lim - 1u) : 0u;
}

SIMLOD_HD inline uint32_t pack_float_bits(float f) {
	uint32_t u;
	__builtin_memcpy(&u, &f, 4);
	return u;
}

// rule K4's decode of one axis: voxel_centre's fp32 sequence
SIMLOD_HD inline float pack_voxel_axis(float fmin, float fns, uint32_t c) { return fmin + (fns * ((float)c + 0.5f)) / 128.0f; }
// rule K3's decode of one axis; step = ns / 8192 (exact)
SIMLOD_HD inline float pack_point_axis(double nmin, double step, uint32_t q) { return (float)(nmin + ((double)q + 0.5) * step); }

// rules K0, K2, K4 and K6 for one sample of a node with frame f (fns: the node's fp32 size, voxels only): the record, and in `what` the
// PACK_* bits that hold for it
SIMLOD_HD inline uint64_t pack_sample(const PackFrame& f, float fns, bool leaf, float x, float y, float z, uint32_t color, uint32_t& what) {
	const double lim = leaf ? 8192.0 : 128.0;
	bool ix, iy, iz;
	const uint32_t qx = pack_quantize(((double)x - f.nmin[0]) * f.k, lim, ix);
	const uint32_t qy = pack_quantize(((double)y - f.nmin[1]) * f.k, lim, iy);
	const uint32_t qz = pack_quantize(((double)z - f.nmin[2]) * f.k, lim, iz);
	what = (ix && iy && iz ? 0u : PACK_CLAMPED) | ((color >> 24) != 0xffu ? PACK_ALPHA : 0u);
	if (!leaf) {
		const bool same = pack_float_bits(pack_voxel_axis(f.fmin[0], fns, qx)) == pack_float_bits(x) &&
		                  pack_float_bits(pack_voxel_axis(f.fmin[1], fns, qy)) == pack_float_bits(y) &&
		                  pack_float_bits(pack_voxel_axis(f.fmin[2], fns, qz)) == pack_float_bits(z);
		if (!same) what |= PACK_INEXACT;
	}
	return (uint64_t)(color & 0xffffffu) | (uint64_t)qx << PACK_SHIFT_X | (uint64_t)qy << PACK_SHIFT_Y | (uint64_t)qz << PACK_SHIFT_Z;
}

// rules K3, K4 and K8 for one record: every field masked to its width, bit 63 ignored, alpha 0xff
SIMLOD_HD inline SimlodPoint unpack_sample(const PackFrame& f, double ns, float fns, bool leaf, uint64_t w) {
	const uint32_t mask = leaf ? (1u << PACK_POINT_BITS) - 1u : (1u << PACK_VOXEL_BITS) - 1u;
	const uint32_t qx = (uint32_t)(w >> PACK_SHIFT_X) & mask, qy = (uint32_t)(w >> PACK_SHIFT_Y) & mask, qz = (uint32_t)(w >> PACK_SHIFT_Z) & mask;
	SimlodPoint p;
	if (leaf) {
		const double step = ns / 8192.0;
		p.x = pack_point_axis(f.nmin[0], step, qx); p.y = pack_point_axis(f.nmin[1], step, qy); p.z = pack_point_axis(f.nmin[2], step, qz);
	} else {
		p.x = pack_voxel_axis(f.fmin[0], fns, qx); p.y = pack_voxel_axis(f.fmin[1], fns, qy); p.z = pack_voxel_axis(f.fmin[2], fns, qz);
	}
	p.color = 0xff000000u | ((uint32_t)w & 0xffffffu);
	return p;
}

}  // namespace simlod
