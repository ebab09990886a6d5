// lasso_rules.hpp — the lasso query's rules L1-L4 and L7 (include/simlod_hip.h, "lasso queries"): what a SimlodLasso must look like to be
// accepted, its rows and its edges widened to the fp64 block the kernels read, whether a projected point (U, V, W) is inside, and a node's class
// by the lasso.  No HIP in here: export_lasso.inc's kernels, the launchers (export.hip) and tests/host/lasso_rules_check.cpp (plain g++) read it
// here.  fp64 from the fp32 inputs, every sum in the order the header states, no fused multiply-add (the library is built with
// -ffp-contract=off; the host program likewise) and no division, so that the numpy mirror (simlod_amd/octree_io.py Lasso, classify_lasso,
// OctreeExport.crop(lasso=)) reproduces every decision bit for bit.
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

enum : uint32_t { LASSO_NODE_OUTSIDE = 0u, LASSO_NODE_FILTERED = 1u, LASSO_NODE_COPIED = 2u };   // (the numbers of export_common.inc's Q_*)

// the edge from a = P[i] to b = P[(i + 1) mod n]; du = b_u - a_u, dv = b_v - a_v (the layout of the footprint's FootEdge: one block, one copy)
struct LassoEdge { double au, av, du, dv; };
static_assert(sizeof(LassoEdge) == 32, "LassoEdge");

// rule L7, the lasso's own part
inline bool lasso_acceptable(const SimlodLasso& l) {
	if (l.numVertices < 3u || l.numVertices > SIMLOD_LASSO_MAX_VERTICES || l.reserved[0] != 0u || l.reserved[1] != 0u || l.reserved[2] != 0u) return false;
	for (int k = 0; k < 4; k++)
		if (!std::isfinite(l.rowU[k]) || !std::isfinite(l.rowV[k]) || !std::isfinite(l.rowW[k])) return false;
	for (uint32_t i = 0; i < l.numVertices; i++)
		if (!std::isfinite(l.vertices[i][0]) || !std::isfinite(l.vertices[i][1])) return false;
	return true;
}

// an acceptable lasso widened to fp64: rows[0..2] = rowU, rowV, rowW; edges[0 .. numVertices - 1]
inline void lasso_widen(const SimlodLasso& l, double (&rows)[3][4], LassoEdge* edges) {
	for (int k = 0; k < 4; k++) { rows[0][k] = (double)l.rowU[k]; rows[1][k] = (double)l.rowV[k]; rows[2][k] = (double)l.rowW[k]; }
	const uint32_t n = l.numVertices;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t j = i + 1u == n ? 0u : i + 1u;
		const double au = (double)l.vertices[i][0], av = (double)l.vertices[i][1];
		edges[i] = LassoEdge{au, av, (double)l.vertices[j][0] - au, (double)l.vertices[j][1] - av};
	}
}

// U = ((ux*x + uy*y) + uz*z) + u0
SIMLOD_HD inline double lasso_row(const double (&r)[4], double x, double y, double z) { return ((r[0] * x + r[1] * y) + r[2] * z) + r[3]; }

// Rule L1 at (U, V, W): W > 0 and the parity of the crossed edges.  sb = b_v*W is carried over as the next edge's sa.
SIMLOD_HD inline bool lasso_inside(const LassoEdge* edges, uint32_t n, double U, double V, double W) {
	if (!(W > 0.0)) return false;
	uint32_t odd = 0u;
	double sa = edges[0].av * W;
	for (uint32_t i = 0; i < n; i++) {
		const LassoEdge e = edges[i];
		const double sb = edges[i + 1u == n ? 0u : i + 1u].av * W;
		const double c = e.du * (V - sa) - e.dv * (U - e.au * W);
		odd ^= (uint32_t)(((sa > V) != (sb > V)) && ((c > 0.0) == (e.dv > 0.0)));
		sa = sb;
	}
	return odd != 0u;
}

// Rules L2-L4: the class of the cube of (level, X, Y, Z), inflated by one level-20 cell (region-query rule 1), by the lasso.  (U, V, W) at the
// eight corners (bit 0 of k: x, bit 1: y, bit 2: z, each choosing hi over lo); an edge is FAR when c has one strict sign at all eight, or when
// both ends' v lie above the point at all eight, or neither at any; a node with mixed signs of W or a NEAR edge is filtered, any other takes
// rule L1's verdict at corner 0.
SIMLOD_HD inline uint32_t classify_lasso(const double (&mn)[3], double size, const double (&rows)[3][4], const LassoEdge* edges, uint32_t n, uint32_t level,
                                         uint32_t X, uint32_t Y, uint32_t Z) {
	const double s = ldexp(size, -(int)level), e = ldexp(size, -20);                         // (exact: powers of two; 20 = SIMLOD_MAX_DEPTH)
	const uint32_t A[3] = {X, Y, Z};
	double lo[3], hi[3];
	for (int k = 0; k < 3; k++) {
		lo[k] = (mn[k] + (double)A[k] * s) - e;
		hi[k] = (mn[k] + ((double)A[k] + 1.0) * s) + e;
	}
	double U[8], V[8], W[8];
	bool front = true, behind = true;                                       // W_k > 0 at all eight; W_k <= 0 at all eight
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int k = 0; k < 8; k++) {
		const double x = (k & 1) ? hi[0] : lo[0], y = (k & 2) ? hi[1] : lo[1], z = (k & 4) ? hi[2] : lo[2];
		U[k] = lasso_row(rows[0], x, y, z);
		V[k] = lasso_row(rows[1], x, y, z);
		W[k] = lasso_row(rows[2], x, y, z);
		front = front && W[k] > 0.0;
		behind = behind && W[k] <= 0.0;
	}
	if (behind) return LASSO_NODE_OUTSIDE;
	if (!front) return LASSO_NODE_FILTERED;
	bool near = false;
	uint32_t odd = 0u;
	for (uint32_t i = 0; i < n; i++) {
		const LassoEdge ed = edges[i];
		const double bv = edges[i + 1u == n ? 0u : i + 1u].av;              // (sa and sb are multiplied out per edge: eight carried products per lane cost more registers than k_l_hier has)
		bool pos = true, neg = true, both = true, none = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
		for (int k = 0; k < 8; k++) {
			const double sa = ed.av * W[k], sb = bv * W[k];
			const double c = ed.du * (V[k] - sa) - ed.dv * (U[k] - ed.au * W[k]);
			const bool ua = sa > V[k], ub = sb > V[k];
			pos = pos && c > 0.0;
			neg = neg && c < 0.0;
			both = both && ua && ub;
			none = none && !ua && !ub;
			if (k == 0) odd ^= (uint32_t)((ua != ub) && ((c > 0.0) == (ed.dv > 0.0)));
		}
		near = near || !(pos || neg || both || none);                       // (not FAR)
	}
	return near ? LASSO_NODE_FILTERED : odd != 0u ? LASSO_NODE_COPIED : LASSO_NODE_OUTSIDE;
}

}  // namespace simlod
