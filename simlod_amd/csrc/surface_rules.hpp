// surface_rules.hpp — the surface queries' rules N2-N9 and their refusals (include/simlod_hip.h, "surface queries"): what a SimlodSurfaceParams
// record must be to be accepted, the quantised offset of a neighbour, the widening D of a 64-bit sum, the moment matrix M, the power-of-two
// scaling P, the normal by eight squarings of t*I - M, its orientation, the two numbers of the surface variation and the colour index.  No HIP
// in here, and nothing of the library's other headers but the ABI's structs and compare_rules.hpp, whose validity, cell, h and key ARE rule N1's
// and are not restated: compare_surface.inc's kernel and launcher and tests/host/surface_rules_check.cpp (plain g++) read it here.  Every
// operation is an fp64 add, subtract, multiply or compare, an integer operation, a conversion or a multiplication by a power of two: no
// division and no square root but the launcher's one (surface_invq, host only), no fused multiply-add (the library is built with
// -ffp-contract=off; the host program likewise), and fp64 subnormals are kept (rule N4 relies on gradual underflow), so that the numpy mirror
// (simlod_amd/octree_io.py surface_samples) reproduces every record and every count bit for bit.
#pragma once
#include <stdint.h>
#include <cmath>
#include "simlod_hip.h"
#include "compare_rules.hpp"

namespace simlod {

constexpr uint32_t SURFACE_THRESHOLDS = 255u, SURFACE_BINS = 257u;            // rule N8; the last bin: degenerate and invalid samples
constexpr uint32_t SURFACE_MIN_WITHIN = 3u;                                   // rule N9: fewer neighbours span no plane
constexpr uint32_t SURFACE_SQUARINGS = 8u;                                    // rule N5
constexpr double   SURFACE_Q_SCALE = 16384.0;                                 // rule N2: |q| <= 2^14
// the moments' order everywhere: the nine sums, and the six unique entries of a symmetric matrix
enum { SURFACE_X = 0, SURFACE_Y, SURFACE_Z, SURFACE_XX, SURFACE_XY, SURFACE_XZ, SURFACE_YY, SURFACE_YZ, SURFACE_ZZ, SURFACE_SUMS };
enum { SYM_XX = 0, SYM_XY, SYM_XZ, SYM_YY, SYM_YZ, SYM_ZZ, SYM_ENTRIES };

// the refusals of the record itself: the compare record's (radius, thresholds, the reserved word) and the light, the orientation, the two modes
inline bool surface_acceptable(const SimlodSurfaceParams& p) {
	if (!std::isfinite(p.radius) || !(p.radius >= 0.0f) || p.reserved != 0u) return false;
	if (p.colourBy > SIMLOD_SURFACE_VARIATION || p.orientMode > SIMLOD_SURFACE_ORIENT_POSITION) return false;
	for (int k = 0; k < 3; k++)
		if (!std::isfinite(p.light[k]) || !std::isfinite(p.orient[k])) return false;
	if (p.colourBy == SIMLOD_SURFACE_SHADE && p.light[0] == 0.0f && p.light[1] == 0.0f && p.light[2] == 0.0f) return false;
	for (uint32_t i = 0; i < SURFACE_THRESHOLDS; i++) {
		if (!std::isfinite(p.thresholds[i])) return false;
		if (i != 0u && !(p.thresholds[i] >= p.thresholds[i - 1u])) return false;
	}
	return true;
}

// rule N2: the launcher's factor, one IEEE division on the host, and a neighbour's quantised offset on one axis (p = (double)s - (double)c)
inline double surface_invq(float radius, float size) { return SURFACE_Q_SCALE / compare_h(radius, size); }
SIMLOD_HD inline int32_t surface_q(double p, double invq) { return (int32_t)(p * invq); }

// rule N3: a signed 64-bit sum widened; the high word's product is exact, the add rounds once
SIMLOD_HD inline double surface_D(int64_t s) { return (double)(int32_t)(s >> 32) * 4294967296.0 + (double)(uint32_t)s; }

SIMLOD_HD inline uint64_t surface_bits(double d) {
	union { double d; uint64_t u; } v;
	v.d = d;
	return v.u;
}
SIMLOD_HD inline double surface_from_bits(uint64_t u) {
	union { double d; uint64_t u; } v;
	v.u = u;
	return v.d;
}

// rule N4: the factor 2^(1023 - e) for the largest |entry| m of a symmetric matrix, e its exponent bits; false when m == 0
SIMLOD_HD inline bool surface_factor(const double (&s)[SYM_ENTRIES], double& f) {
	double m = 0.0;
	for (int k = 0; k < SYM_ENTRIES; k++) {
		const double x = s[k] < 0.0 ? -s[k] : s[k];
		if (x > m) m = x;
	}
	const uint64_t e = (surface_bits(m) >> 52) & 0x7ffu;
	f = surface_from_bits((uint64_t)(2046u - e) << 52);
	return m != 0.0;
}
SIMLOD_HD inline bool surface_scale(double (&s)[SYM_ENTRIES]) {
	double f;
	const bool ok = surface_factor(s, f);
	for (int k = 0; k < SYM_ENTRIES; k++) s[k] *= f;
	return ok;
}

// rule N3: M = n * D(S_uv) - D(S_u) * D(S_v), n^2 times the covariance of the quantised offsets
SIMLOD_HD inline void surface_moments(const int64_t (&S)[SURFACE_SUMS], uint32_t within, double (&M)[SYM_ENTRIES]) {
	const double n = (double)within;
	const double dx = surface_D(S[SURFACE_X]), dy = surface_D(S[SURFACE_Y]), dz = surface_D(S[SURFACE_Z]);
	M[SYM_XX] = n * surface_D(S[SURFACE_XX]) - dx * dx;
	M[SYM_XY] = n * surface_D(S[SURFACE_XY]) - dx * dy;
	M[SYM_XZ] = n * surface_D(S[SURFACE_XZ]) - dx * dz;
	M[SYM_YY] = n * surface_D(S[SURFACE_YY]) - dy * dy;
	M[SYM_YZ] = n * surface_D(S[SURFACE_YZ]) - dy * dz;
	M[SYM_ZZ] = n * surface_D(S[SURFACE_ZZ]) - dz * dz;
}

struct SurfaceEstimate {
	double v[3];                       // rules N5, N6: the oriented, unnormalised normal
	double lambdaNum, lambdaDen;       // rule N7
	double vv;                         // rule N7
};

// rules N3-N7 for one sample of `a` from its nine sums; c: the sample (widened), o: rule N6's `orient` (widened).  false: degenerate (rule N9).
SIMLOD_HD inline bool surface_estimate(const int64_t (&S)[SURFACE_SUMS], uint32_t within, const double (&c)[3], const double (&orient)[3],
                                       uint32_t orientMode, SurfaceEstimate& out) {
	if (within < SURFACE_MIN_WITHIN) return false;
	double M[SYM_ENTRIES], B[SYM_ENTRIES];
	surface_moments(S, within, M);
	if (!surface_scale(M)) return false;                                        // rule N5: M <- P(M)
	const double t = (M[SYM_XX] + M[SYM_YY]) + M[SYM_ZZ];
	B[SYM_XX] = t - M[SYM_XX]; B[SYM_XY] = -M[SYM_XY]; B[SYM_XZ] = -M[SYM_XZ];
	B[SYM_YY] = t - M[SYM_YY]; B[SYM_YZ] = -M[SYM_YZ]; B[SYM_ZZ] = t - M[SYM_ZZ];
	bool ok = true;
	for (uint32_t round = 0; round < SURFACE_SQUARINGS; round++) {              // B <- P(B * B), the upper triangle
		double C[SYM_ENTRIES];
		C[SYM_XX] = (B[SYM_XX] * B[SYM_XX] + B[SYM_XY] * B[SYM_XY]) + B[SYM_XZ] * B[SYM_XZ];
		C[SYM_XY] = (B[SYM_XX] * B[SYM_XY] + B[SYM_XY] * B[SYM_YY]) + B[SYM_XZ] * B[SYM_YZ];
		C[SYM_XZ] = (B[SYM_XX] * B[SYM_XZ] + B[SYM_XY] * B[SYM_YZ]) + B[SYM_XZ] * B[SYM_ZZ];
		C[SYM_YY] = (B[SYM_XY] * B[SYM_XY] + B[SYM_YY] * B[SYM_YY]) + B[SYM_YZ] * B[SYM_YZ];
		C[SYM_YZ] = (B[SYM_XY] * B[SYM_XZ] + B[SYM_YY] * B[SYM_YZ]) + B[SYM_YZ] * B[SYM_ZZ];
		C[SYM_ZZ] = (B[SYM_XZ] * B[SYM_XZ] + B[SYM_YZ] * B[SYM_YZ]) + B[SYM_ZZ] * B[SYM_ZZ];
		ok = surface_scale(C) && ok;
		for (int k = 0; k < SYM_ENTRIES; k++) B[k] = C[k];
	}
	if (!ok) return false;
	// the column of the first largest diagonal entry
	double v0 = B[SYM_XX], v1 = B[SYM_XY], v2 = B[SYM_XZ], best = B[SYM_XX];
	if (B[SYM_YY] > best) { best = B[SYM_YY]; v0 = B[SYM_XY]; v1 = B[SYM_YY]; v2 = B[SYM_YZ]; }
	if (B[SYM_ZZ] > best) { v0 = B[SYM_XZ]; v1 = B[SYM_YZ]; v2 = B[SYM_ZZ]; }
	// rule N6
	double o[3] = {orient[0], orient[1], orient[2]};
	if (orientMode == SIMLOD_SURFACE_ORIENT_POSITION) { o[0] = orient[0] - c[0]; o[1] = orient[1] - c[1]; o[2] = orient[2] - c[2]; }
	const double s = (v0 * o[0] + v1 * o[1]) + v2 * o[2];
	if (s < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
	// rule N7
	const double w0 = (M[SYM_XX] * v0 + M[SYM_XY] * v1) + M[SYM_XZ] * v2;
	const double w1 = (M[SYM_XY] * v0 + M[SYM_YY] * v1) + M[SYM_YZ] * v2;
	const double w2 = (M[SYM_XZ] * v0 + M[SYM_YZ] * v1) + M[SYM_ZZ] * v2;
	out.v[0] = v0; out.v[1] = v1; out.v[2] = v2;
	out.lambdaNum = (v0 * w0 + v1 * w1) + v2 * w2;
	out.vv = (v0 * v0 + v1 * v1) + v2 * v2;
	out.lambdaDen = out.vv * t;
	return true;
}

// rule N8: the two numbers the thresholds are held against
SIMLOD_HD inline void surface_colour_terms(const SurfaceEstimate& e, uint32_t colourBy, const double (&L)[3], double& num, double& den) {
	if (colourBy == SIMLOD_SURFACE_SHADE) {
		const double a = (e.v[0] * L[0] + e.v[1] * L[1]) + e.v[2] * L[2];
		num = a * fabs(a);
		den = e.vv * ((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]);
	} else {
		num = e.lambdaNum;
		den = e.lambdaDen;
	}
}

// rule N8: the number of entries of t[0 .. 255) with t[i] * den <= num, by binary search (den >= 0: the products ascend with the entries)
SIMLOD_HD inline uint32_t surface_index(const double* t, double num, double den) {
	uint32_t lo = 0u, hi = SURFACE_THRESHOLDS;                                 // the answer lies in [lo, hi]
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (t[mid] * den <= num) lo = mid + 1u; else hi = mid;
	}
	return lo;
}

}  // namespace simlod
