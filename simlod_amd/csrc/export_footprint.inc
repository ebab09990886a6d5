// export_footprint.inc — part of export.hip: footprint queries.  FootEdge, FootGeom, FootArgs, stage_edges, Footprint (rule F1),
// classify_footprint (rules F2-F4), k_f_hier, k_f_count, k_f_write.
// ---- footprint query ------------------------------------------------------------------------------------------------------------------
// simlod_query_footprint (simlod_hip.h, "footprint queries"): the region query's five launches with an extruded polygon on top of the planes.
//   k_f_hier   k_q_hier with the class of a node combined from the planes (classify) and the polygon (classify_footprint).
//   k_q_dir, k_q_scan   as they are.
//   k_f_count, k_f_write   k_q_count's and k_q_write's bodies with rule F1 behind the planes' test.
// The polygon lies in the caller's scratch, widened to fp64 by the launcher: {a_u, a_v, du, dv} per edge.  Every kernel that needs it stages it
// in LDS once per workgroup; all lanes then read the same edge in the same iteration (a broadcast read).
// fp64 from the fp32 inputs, every sum in the order the header states, no fused multiply-add, no division: OctreeExport.crop(footprint=)
// reproduces every decision bit for bit.
struct FootEdge { double au, av, du, dv; };                                       // the edge from a = P[i] to b = P[(i + 1) mod n]; du = b_u - a_u, dv = b_v - a_v
static_assert(sizeof(FootEdge) == 32, "FootEdge");
constexpr uint64_t FOOT_BLOCK_BYTES = SIMLOD_FOOTPRINT_MAX_VERTICES * sizeof(FootEdge);   // 8 KB of the scratch buffer, in front of the items

struct FootGeom {
	double   axU[4], axV[4];
	uint64_t edges;                     // offset of FootEdge[n] in the scratch buffer
	uint32_t n, pad;
};
struct FootArgs {
	QueryArgs q;
	FootGeom  f;
};

__device__ __forceinline__ const QueryArgs& query_of(const FootArgs& fa) { return fa.q; }

// the polygon from the scratch buffer into LDS (any block size); the barrier is the caller's
__device__ __forceinline__ void stage_edges(const FootArgs& fa, FootEdge* sh) {
	const FootEdge* e = reinterpret_cast<const FootEdge*>(fa.q.x.scratch + fa.f.edges);
	for (uint32_t i = threadIdx.x; i < fa.f.n; i += blockDim.x) sh[i] = e[i];
}

// Rule F1 at (u, v): the parity of the crossed edges.  b_v is the next edge's a_v.
__device__ __forceinline__ bool foot_inside(const FootEdge* sh, uint32_t n, double u, double v) {
	uint32_t odd = 0u;
	double av = sh[0].av;
	for (uint32_t i = 0; i < n; i++) {
		const FootEdge e = sh[i];
		const double bv = sh[i + 1u == n ? 0u : i + 1u].av;
		const double c = e.du * (v - av) - e.dv * (u - e.au);
		odd ^= (uint32_t)(((av > v) != (bv > v)) && ((c > 0.0) == (e.dv > 0.0)));
		av = bv;
	}
	return odd != 0u;
}

// what k_f_count / k_f_write ask of a sample behind the planes: u = ((ux*x + uy*y) + uz*z) + u0, v likewise, then rule F1
struct Footprint {
	const FootGeom& f;
	const FootEdge* sh;
	__device__ __forceinline__ bool operator()(const u32x4& p) const {
		const double x = (double)__uint_as_float(p.x), y = (double)__uint_as_float(p.y), z = (double)__uint_as_float(p.z);
		const double u = ((f.axU[0] * x + f.axU[1] * y) + f.axU[2] * z) + f.axU[3];
		const double v = ((f.axV[0] * x + f.axV[1] * y) + f.axV[2] * z) + f.axV[3];
		return foot_inside(sh, f.n, u, v);
	}
};

// Rules F2-F4: the class of a node's inflated cube (region-query rule 1) by the polygon.  The projected rectangle [U_lo, U_hi] x [V_lo, V_hi]
// from the corners nearest and farthest along each axis; an edge is FAR when its v range misses the rectangle's or when c has one strict sign
// at all four corners; a node with a NEAR edge is filtered, any other takes rule F1's verdict at (U_lo, V_lo).
__device__ __forceinline__ uint32_t classify_footprint(const QueryGeom& g, const FootGeom& f, const FootEdge* sh, uint32_t level, uint32_t X, uint32_t Y,
                                                        uint32_t Z) {
	const double s = ldexp(g.size, -(int)level), e = ldexp(g.size, -SIMLOD_MAX_DEPTH);       // (exact: powers of two)
	const uint32_t A[3] = {X, Y, Z};
	double lo[3], hi[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		lo[k] = (g.min[k] + (double)A[k] * s) - e;
		hi[k] = (g.min[k] + ((double)A[k] + 1.0) * s) + e;
	}
	const double* au = f.axU;
	const double* av = f.axV;
	const double Ulo = ((au[0] * (au[0] >= 0.0 ? lo[0] : hi[0]) + au[1] * (au[1] >= 0.0 ? lo[1] : hi[1])) + au[2] * (au[2] >= 0.0 ? lo[2] : hi[2])) + au[3];
	const double Uhi = ((au[0] * (au[0] >= 0.0 ? hi[0] : lo[0]) + au[1] * (au[1] >= 0.0 ? hi[1] : lo[1])) + au[2] * (au[2] >= 0.0 ? hi[2] : lo[2])) + au[3];
	const double Vlo = ((av[0] * (av[0] >= 0.0 ? lo[0] : hi[0]) + av[1] * (av[1] >= 0.0 ? lo[1] : hi[1])) + av[2] * (av[2] >= 0.0 ? lo[2] : hi[2])) + av[3];
	const double Vhi = ((av[0] * (av[0] >= 0.0 ? hi[0] : lo[0]) + av[1] * (av[1] >= 0.0 ? hi[1] : lo[1])) + av[2] * (av[2] >= 0.0 ? hi[2] : lo[2])) + av[3];
	bool near = false;
	uint32_t odd = 0u;
	double a_v = sh[0].av;
	for (uint32_t i = 0; i < f.n; i++) {
		const FootEdge ed = sh[i];
		const double b_v = sh[i + 1u == f.n ? 0u : i + 1u].av;
		const double pl = ed.du * (Vlo - a_v), ph = ed.du * (Vhi - a_v), ql = ed.dv * (Ulo - ed.au), qh = ed.dv * (Uhi - ed.au);
		const double c00 = pl - ql, c01 = ph - ql, c10 = pl - qh, c11 = ph - qh;              // c(U_lo,V_lo), c(U_lo,V_hi), c(U_hi,V_lo), c(U_hi,V_hi)
		const bool far = fmax(a_v, b_v) < Vlo || fmin(a_v, b_v) > Vhi || (c00 > 0.0 && c01 > 0.0 && c10 > 0.0 && c11 > 0.0) ||
		                 (c00 < 0.0 && c01 < 0.0 && c10 < 0.0 && c11 < 0.0);
		near = near || !far;
		odd ^= (uint32_t)(((a_v > Vlo) != (b_v > Vlo)) && ((c00 > 0.0) == (ed.dv > 0.0)));
		a_v = b_v;
	}
	return near ? Q_FILTERED : odd != 0u ? Q_COPIED : Q_OUTSIDE;
}

__global__ __launch_bounds__(WG_TPB) void k_f_hier(FootArgs fa) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	const ExportArgs& a = fa.q.x;
	uint32_t* cls = reinterpret_cast<uint32_t*>(a.scratch + fa.q.cls);
	stage_edges(fa, sh_edges);
	__syncthreads();
	hier_walk<true>(a, [&](uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
		// outside by either; copied iff copied by both; else filtered
		const uint32_t p = classify(fa.q.g, level, X, Y, Z);
		if (p == Q_OUTSIDE) return (uint32_t)Q_OUTSIDE;
		const uint32_t c = classify_footprint(fa.q.g, fa.f, sh_edges, level, X, Y, Z);
		return c == Q_OUTSIDE ? (uint32_t)Q_OUTSIDE : (p == Q_COPIED && c == Q_COPIED) ? (uint32_t)Q_COPIED : (uint32_t)Q_FILTERED;
	}, cls);
	__syncthreads();
	query_totals(a, cls, sh_scan);
}

__global__ __launch_bounds__(LANE_TPB) void k_f_count(FootArgs fa) {
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	stage_edges(fa, sh_edges);
	__syncthreads();
	q_count<const FootArgs&>(fa, Footprint{fa.f, sh_edges});
}

__global__ __launch_bounds__(LANE_TPB) void k_f_write(FootArgs fa) {
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	stage_edges(fa, sh_edges);
	__syncthreads();
	q_write<const FootArgs&>(fa, Footprint{fa.f, sh_edges});
}
