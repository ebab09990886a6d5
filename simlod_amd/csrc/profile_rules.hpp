// profile_rules.hpp — the profile query's rules P0-P3 and P6 (include/simlod_hip.h, "profile queries"): what a SimlodProfile must look like to be
// accepted, its segments widened to the fp64 block the kernels read, the segment a point (u, v) belongs to, a sample's record, and a node's class
// by the corridor.  No HIP in here: export_profile.inc's kernels, the launcher (export.hip) and tests/host/profile_rules_check.cpp (plain g++) read
// it here.  fp64 from the fp32 inputs, every sum in the order the header states and no fused multiply-add (the library is built with
// -ffp-contract=off; the host program likewise), so that the numpy mirror (simlod_amd/octree_io.py Profile, classify_profile,
// OctreeExport.profile) reproduces every decision and every record bit for bit.  The square root and the division of rule P0 are the launcher's,
// on the host: nothing marked SIMLOD_HD divides or takes a root.
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

enum : uint32_t { PROFILE_NODE_OUTSIDE = 0u, PROFILE_NODE_FILTERED = 1u, PROFILE_NODE_COPIED = 2u };   // (the numbers of export_common.inc's Q_*)

// rule P0: segment i from a = P[i] to b = P[i + 1]
struct ProfileSegment { double au, av, du, dv, L2, W2, inv, s0; };
static_assert(sizeof(ProfileSegment) == 64, "ProfileSegment");
constexpr uint32_t PROFILE_MAX_SEGMENTS = SIMLOD_PROFILE_MAX_VERTICES - 1u;
constexpr uint64_t PROFILE_BLOCK_BYTES = 4096u;                           // of the scratch buffer, in front of the items
static_assert(PROFILE_MAX_SEGMENTS * sizeof(ProfileSegment) <= PROFILE_BLOCK_BYTES, "the segments fit their block");

// rule P6, the profile's own part (a zero-length segment: profile_segments)
inline bool profile_acceptable(const SimlodProfile& p) {
	if (p.numVertices < 2u || p.numVertices > SIMLOD_PROFILE_MAX_VERTICES || p.reserved[0] != 0u || p.reserved[1] != 0u) return false;
	if (!std::isfinite(p.halfWidth) || !(p.halfWidth > 0.0f)) return false;
	for (int k = 0; k < 4; k++)
		if (!std::isfinite(p.axisU[k]) || !std::isfinite(p.axisV[k]) || !std::isfinite(p.axisH[k])) return false;
	for (uint32_t i = 0; i < p.numVertices; i++)
		if (!std::isfinite(p.vertices[i][0]) || !std::isfinite(p.vertices[i][1])) return false;
	return true;
}

// rule P0 for an acceptable profile: seg[0 .. numVertices - 2].  false: a segment of length zero.
inline bool profile_segments(const SimlodProfile& p, ProfileSegment* seg) {
	const double w = (double)p.halfWidth;
	double s0 = 0.0;
	for (uint32_t i = 0; i + 1u < p.numVertices; i++) {
		const double au = (double)p.vertices[i][0], av = (double)p.vertices[i][1];
		const double du = (double)p.vertices[i + 1u][0] - au, dv = (double)p.vertices[i + 1u][1] - av;
		const double L2 = du * du + dv * dv;
		if (L2 == 0.0) return false;
		const double len = std::sqrt(L2);
		seg[i] = ProfileSegment{au, av, du, dv, L2, (w * w) * L2, 1.0 / len, s0};
		s0 = s0 + len;
	}
	return true;
}

// rule P1: the lowest segment (u, v) is in, or n: in none (a NaN is in none).  al and c are that segment's.
SIMLOD_HD inline uint32_t profile_locate(const ProfileSegment* seg, uint32_t n, double u, double v, double& al, double& c) {
	for (uint32_t i = 0; i < n; i++) {
		const double au = seg[i].au, av = seg[i].av, du = seg[i].du, dv = seg[i].dv;
		const double pu = u - au, pv = v - av;
		const double a = du * pu + dv * pv, cc = du * pv - dv * pu;
		if (a >= 0.0 && a <= seg[i].L2 && cc * cc <= seg[i].W2) { al = a; c = cc; return i; }
	}
	return n;
}

// u = ((ux*x + uy*y) + uz*z) + u0: the projection of rule F1, and the height of rule P2
SIMLOD_HD inline double profile_axis(const double (&ax)[4], double x, double y, double z) { return ((ax[0] * x + ax[1] * y) + ax[2] * z) + ax[3]; }

// rule P2 for a sample in segment i < n; in no segment (i == n: only a sample outside the contract in a COPIED node) station = offset = 0 and
// segment = SIMLOD_PROFILE_NO_SEGMENT
SIMLOD_HD inline SimlodProfileSample profile_record(const ProfileSegment* seg, uint32_t n, uint32_t i, double al, double c, double h) {
	SimlodProfileSample r;
	r.station = i < n ? (float)(seg[i].s0 + al * seg[i].inv) : 0.0f;
	r.offset = i < n ? (float)(c * seg[i].inv) : 0.0f;
	r.height = (float)h;
	r.segment = i < n ? i : SIMLOD_PROFILE_NO_SEGMENT;
	return r;
}

// rule P3: the class of the cube of (level, X, Y, Z), inflated by one level-20 cell (region-query rule 1), by the corridor.  The projected
// rectangle is footprint rule F2's; per segment al and c at its four corners.
SIMLOD_HD inline uint32_t classify_profile(const double (&mn)[3], double size, const double (&axU)[4], const double (&axV)[4], const ProfileSegment* seg,
                                           uint32_t n, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	const double s = ldexp(size, -(int)level), e = ldexp(size, -20);                         // (exact: powers of two; 20 = SIMLOD_MAX_DEPTH)
	const uint32_t A[3] = {X, Y, Z};
	double lo[3], hi[3];
	for (int k = 0; k < 3; k++) {
		lo[k] = (mn[k] + (double)A[k] * s) - e;
		hi[k] = (mn[k] + ((double)A[k] + 1.0) * s) + e;
	}
	const double* au = axU;
	const double* av = axV;
	const double Ulo = ((au[0] * (au[0] >= 0.0 ? lo[0] : hi[0]) + au[1] * (au[1] >= 0.0 ? lo[1] : hi[1])) + au[2] * (au[2] >= 0.0 ? lo[2] : hi[2])) + au[3];
	const double Uhi = ((au[0] * (au[0] >= 0.0 ? hi[0] : lo[0]) + au[1] * (au[1] >= 0.0 ? hi[1] : lo[1])) + au[2] * (au[2] >= 0.0 ? hi[2] : lo[2])) + au[3];
	const double Vlo = ((av[0] * (av[0] >= 0.0 ? lo[0] : hi[0]) + av[1] * (av[1] >= 0.0 ? lo[1] : hi[1])) + av[2] * (av[2] >= 0.0 ? lo[2] : hi[2])) + av[3];
	const double Vhi = ((av[0] * (av[0] >= 0.0 ? hi[0] : lo[0]) + av[1] * (av[1] >= 0.0 ? hi[1] : lo[1])) + av[2] * (av[2] >= 0.0 ? hi[2] : lo[2])) + av[3];
	bool near = false, covered = false;
	for (uint32_t i = 0; i < n; i++) {
		const double a_u = seg[i].au, a_v = seg[i].av, du = seg[i].du, dv = seg[i].dv, L2 = seg[i].L2, W2 = seg[i].W2;
		const double ul = du * (Ulo - a_u), uh = du * (Uhi - a_u), vl = dv * (Vlo - a_v), vh = dv * (Vhi - a_v);      // al = du*pu + dv*pv
		const double a00 = ul + vl, a01 = ul + vh, a10 = uh + vl, a11 = uh + vh;
		const double pl = du * (Vlo - a_v), ph = du * (Vhi - a_v), ql = dv * (Ulo - a_u), qh = dv * (Uhi - a_u);      // c = du*pv - dv*pu
		const double c00 = pl - ql, c01 = ph - ql, c10 = pl - qh, c11 = ph - qh;
		const double amin = fmin(fmin(a00, a01), fmin(a10, a11)), amax = fmax(fmax(a00, a01), fmax(a10, a11));
		const double cmin = fmin(fmin(c00, c01), fmin(c10, c11)), cmax = fmax(fmax(c00, c01), fmax(c10, c11));
		const bool far = amax < 0.0 || amin > L2 || (cmin > 0.0 && cmin * cmin > W2) || (cmax < 0.0 && cmax * cmax > W2);
		near = near || !far;
		covered = covered || (amin >= 0.0 && amax <= L2 && cmin * cmin <= W2 && cmax * cmax <= W2);
	}
	return !near ? PROFILE_NODE_OUTSIDE : covered ? PROFILE_NODE_COPIED : PROFILE_NODE_FILTERED;
}

}  // namespace simlod
