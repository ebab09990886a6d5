// export_rays.inc — part of export.hip: ray queries over the pair pipeline (export_pairs.inc).  RayPart, RayArgs, RayD, ray_load, slab, sample_t,
// RayQuery, k_r_test, k_r_reduce.
// ---- ray query ------------------------------------------------------------------------------------------------------------------------
// simlod_query_rays (simlod_hip.h, "ray queries"): k_p_hier -> k_q_dir -> k_p_pairs<RayQuery, count> -> k_p_scan<RayQuery> ->
// k_p_pairs<RayQuery, fill> -> k_r_test -> k_r_reduce.  A count-only call also counts numHits in k_p_pairs (COUNT_TESTS_SAMPLES).
//   k_r_test    the hot path, node-major: one chunk per workgroup and turn, its four samples per lane kept in registers as fp64, then the
//               rays paired with the chunk's node in tiles of 64 from LDS; per ray a ballot, a wave arg-min of (t, ordinal) only where a lane
//               passed, the four waves combined through LDS, one 16-byte partial per (chunk, ray).  A chunk is read once however many rays
//               reach its node.
//   k_r_reduce  one wave per ray: the arg-min of (t, node, ordinal) over the ray's partials, the hit record (or the miss) written once.
// Nothing that is returned depends on the schedule: the counts are sums, and the hit is the minimum of a total order.
constexpr uint32_t RAY_TILE = SIMLOD_WAVE;                                        // k_r_test: rays per LDS tile

struct RayPart { double t; uint32_t node, ordinal; };                             // 16 B: the best sample of one (chunk, ray)
static_assert(sizeof(RayPart) == 16, "ray query records");

struct RayArgs {
	PairArgs           p;                // numQueries: the rays
	const SimlodRay*   rays;
	SimlodRayHit*      hits;
	SimlodRayCounts*   counts;
};

// a ray widened to fp64, and R of rule 3
struct RayD { double o[3], d[3], dd, tmin, tmax, rad, spr, R; };

// rule 1; `r` is complete either way
__device__ __forceinline__ bool ray_load(const SimlodRay* rays, uint32_t i, RayD& r) {
	const SimlodRay v = rays[i];
	const float f[10] = {v.origin[0], v.origin[1], v.origin[2], v.tMin, v.dir[0], v.dir[1], v.dir[2], v.tMax, v.radius, v.spread};
	bool ok = v.reserved[0] == 0u && v.reserved[1] == 0u;
#pragma unroll
	for (int k = 0; k < 10; k++) ok = ok && (__float_as_uint(f[k]) & 0x7f800000u) != 0x7f800000u;
	ok = ok && (v.dir[0] != 0.0f || v.dir[1] != 0.0f || v.dir[2] != 0.0f) && v.tMin >= 0.0f && v.tMin <= v.tMax && v.radius >= 0.0f && v.spread >= 0.0f;
#pragma unroll
	for (int k = 0; k < 3; k++) { r.o[k] = (double)v.origin[k]; r.d[k] = (double)v.dir[k]; }
	r.dd = (r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2];
	r.tmin = (double)v.tMin; r.tmax = (double)v.tMax; r.rad = (double)v.radius; r.spr = (double)v.spread;
	r.R = r.rad + r.spr * r.tmax;
	return ok;
}

// rule 3 for one node
__device__ __forceinline__ bool slab(const RayD& r, const PairArgs& a, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	const double s = ldexp(a.size, -(int)level), e = ldexp(a.size, -SIMLOD_MAX_DEPTH);
	const uint32_t A[3] = {X, Y, Z};
	double near = r.tmin, far = r.tmax;
	bool ok = true;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const double lo = (a.min[k] + (double)A[k] * s) - e, hi = (a.min[k] + ((double)A[k] + 1.0) * s) + e;
		const double L = lo - r.R, H = hi + r.R;
		if (r.d[k] == 0.0) ok = ok && !(r.o[k] < L || r.o[k] > H);
		else {
			const double t1 = (L - r.o[k]) / r.d[k], t2 = (H - r.o[k]) / r.d[k];
			near = fmax(near, fmin(t1, t2));
			far = fmin(far, fmax(t1, t2));
		}
	}
	return ok && near <= far;
}

// rule 2: the sample's parameter, or a negative number when it fails (a passing t is >= tMin >= 0; -0.0 passes and is not negative)
__device__ __forceinline__ double sample_t(const RayD& r, double x, double y, double z) {
	const double px = x - r.o[0], py = y - r.o[1], pz = z - r.o[2];
	const double t = ((r.d[0] * px + r.d[1] * py) + r.d[2] * pz) / r.dd;
	const double qx = px - t * r.d[0], qy = py - t * r.d[1], qz = pz - t * r.d[2];
	const double s2 = (qx * qx + qy * qy) + qz * qz, rr = r.rad + r.spr * t;
	return (t >= r.tmin && t <= r.tmax && s2 <= rr * rr) ? t : -1.0;
}

// what the pair pipeline asks of a query (export_pairs.inc)
struct RayQuery {
	using Args = RayArgs;
	using Wide = RayD;
	static constexpr bool COUNT_TESTS_SAMPLES = true;                              // a count-only call reports numHits
	static __device__ __forceinline__ bool load(const Args& a, uint32_t i, Wide& r) { return ray_load(a.rays, i, r); }
	static __device__ __forceinline__ bool probe(const Wide& r, const PairArgs& p, const SimlodExportNode& e) { return slab(r, p, e.level, e.X, e.Y, e.Z); }
	static __device__ __forceinline__ bool passes(const Wide& r, double x, double y, double z) { return sample_t(r, x, y, z) >= 0.0; }
	static __host__ __device__ __forceinline__ bool wants_results(const Args& a) { return a.hits != nullptr; }
	static __host__ __device__ __forceinline__ uint64_t part_bytes(const Args&) { return sizeof(RayPart); }
	static __device__ __forceinline__ void write_counts(const Args& a, const PairTotals& t) {
		SimlodRayCounts c;
		c.numNodes = t.numNodes; c.error = t.error; c.numHits = t.numHits; c.numInvalid = t.numInvalid;
		c.numPairs = t.numPairs; c.numCandidates = t.numCandidates;
		*a.counts = c;
	}
};

__global__ __launch_bounds__(LANE_TPB) void k_r_test(RayArgs a) {
	__shared__ double   sh_ray[11][RAY_TILE];                                      // o, d, dd, tMin, tMax, radius, spread of the tile's rays
	__shared__ uint64_t sh_part[RAY_TILE];
	__shared__ double   sh_t[PAIR_WAVES][RAY_TILE];
	__shared__ uint32_t sh_o[PAIR_WAVES][RAY_TILE];
	const ExportArgs& x = a.p.x;
	const Header* hdr = reinterpret_cast<const Header*>(x.scratch);
	const PairHeader* ph = reinterpret_cast<const PairHeader*>(x.scratch + 256u);
	if (ph->doResults == 0u || ph->numPairs == 0u) return;
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + a.p.at.cnt);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + a.p.at.nfirst);
	const Pair* pairs = reinterpret_cast<const Pair*>(x.scratch + ph->pairsOff);
	RayPart* parts = reinterpret_cast<RayPart*>(x.scratch + ph->partsOff);
	const uint64_t numItems = hdr->totalChunks;
	const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x / SIMLOD_WAVE;
	const double INF = __builtin_huge_val();
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const QItem it = items[i];
		const uint32_t c = cnt[it.node];                                           // (the same for the whole workgroup, as every branch on `it`)
		if (c == 0u) continue;
		double sx[4], sy[4], sz[4];
		test_chunk(it, sx, sy, sz);
		const uint64_t pf = nfirst[it.node];
		for (uint32_t j0 = 0; j0 < c; j0 += RAY_TILE) {
			const uint32_t nt = min(RAY_TILE, c - j0);
			__syncthreads();                                                       // (the tile before is done with)
			if (threadIdx.x < nt) {
				const Pair p = pairs[pf + j0 + threadIdx.x];
				RayD r;
				ray_load(a.rays, p.query, r);                                      // (valid: it formed a pair)
				const double v[11] = {r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], r.dd, r.tmin, r.tmax, r.rad, r.spr};
#pragma unroll
				for (int q = 0; q < 11; q++) sh_ray[q][threadIdx.x] = v[q];
				sh_part[threadIdx.x] = p.part;
			}
			__syncthreads();
			for (uint32_t q = 0; q < nt; q++) {
				RayD r;
				r.o[0] = sh_ray[0][q]; r.o[1] = sh_ray[1][q]; r.o[2] = sh_ray[2][q];
				r.d[0] = sh_ray[3][q]; r.d[1] = sh_ray[4][q]; r.d[2] = sh_ray[5][q];
				r.dd = sh_ray[6][q]; r.tmin = sh_ray[7][q]; r.tmax = sh_ray[8][q]; r.rad = sh_ray[9][q]; r.spr = sh_ray[10][q];
				double bt = INF;
				uint32_t bo = NONE;
#pragma unroll
				for (int j = 0; j < 4; j++) {
					const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
					const double t = sample_t(r, sx[j], sy[j], sz[j]);
					if (k < it.count && t >= 0.0 && t < bt) { bt = t; bo = k; }    // (k ascends with j: an equal t keeps the smaller ordinal)
				}
				if (__ballot(bo != NONE) != 0ull) { const Hit m = wave_hit_min<false>(bt, 0u, bo); bt = m.t; bo = m.ord; }
				if (lane == 0u) { sh_t[w][q] = bt; sh_o[w][q] = bo; }
			}
			__syncthreads();
			if (threadIdx.x < nt) {
				double bt = sh_t[0][threadIdx.x];
				uint32_t bo = sh_o[0][threadIdx.x];
#pragma unroll
				for (uint32_t ww = 1; ww < PAIR_WAVES; ww++) {
					const double ot = sh_t[ww][threadIdx.x];
					const uint32_t oo = sh_o[ww][threadIdx.x];
					if (hit_less(ot, 0u, oo, bt, 0u, bo)) { bt = ot; bo = oo; }
				}
				RayPart p;
				p.t = bt; p.node = bo != NONE ? it.node : NONE; p.ordinal = bo != NONE ? it.k * SIMLOD_POINTS_PER_CHUNK + bo : NONE;
				parts[sh_part[threadIdx.x] + it.k] = p;
			}
		}
	}
}
static_assert(RAY_TILE <= LANE_TPB && PAIR_WAVES == 4, "k_r_test: a lane per ray of the tile, four waves");

__global__ __launch_bounds__(LANE_TPB) void k_r_reduce(RayArgs a) {
	const ExportArgs& x = a.p.x;
	const PairHeader* ph = reinterpret_cast<const PairHeader*>(x.scratch + 256u);
	const uint32_t w = threadIdx.x / SIMLOD_WAVE, lane = (uint32_t)lane_id();
	const uint32_t ray = blockIdx.x * PAIR_WAVES + w;
	if (ray >= a.p.numQueries || ph->doResults == 0u) return;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(x.scratch + x.lay.first);
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	const uint64_t* rayFirst = reinterpret_cast<const uint64_t*>(x.scratch + a.p.at.qFirst);
	const RayPart* parts = reinterpret_cast<const RayPart*>(x.scratch + ph->partsOff);
	double bt = __builtin_huge_val();
	uint32_t bn = NONE, bo = NONE;
	const uint64_t end = rayFirst[ray + 1u];
	for (uint64_t p = rayFirst[ray] + lane; p < end; p += SIMLOD_WAVE) {
		const RayPart v = parts[p];
		if (v.node != NONE && hit_less(v.t, v.node, v.ordinal, bt, bn, bo)) { bt = v.t; bn = v.node; bo = v.ordinal; }
	}
	if (__ballot(bn != NONE) != 0ull) { const Hit m = wave_hit_min<true>(bt, bn, bo); bt = m.t; bn = m.node; bo = m.ord; }
	if (lane != 0u) return;
	SimlodRayHit h;
	h.t = bt; h.node = bn; h.ordinal = bo;
	h.sample.x = 0.0f; h.sample.y = 0.0f; h.sample.z = 0.0f; h.sample.color = 0u;
	if (bn != NONE) {
		const QItem it = items[first[bn] + bo / SIMLOD_POINTS_PER_CHUNK];
		h.sample = reinterpret_cast<const SimlodPoint*>(it.src)[bo % SIMLOD_POINTS_PER_CHUNK];
		atomicAdd(&a.counts->numHits, 1u);
	}
	a.hits[ray] = h;
}
