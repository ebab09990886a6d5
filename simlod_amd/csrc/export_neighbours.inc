// export_neighbours.inc — part of export.hip: neighbour queries over the pair pipeline (export_pairs.inc).  NbEntry, nb_part_bytes, NbArgs, SphereD,
// sphere_load, sphere_cube, sphere_d2, NbQuery, nb_less, k_n_test, k_n_reduce.
// ---- neighbour query ------------------------------------------------------------------------------------------------------------------
// simlod_query_neighbours (simlod_hip.h, "neighbour queries"): k_p_hier -> k_q_dir -> k_p_pairs<NbQuery, count> -> k_p_scan<NbQuery> ->
// k_p_pairs<NbQuery, fill> -> k_n_test -> k_n_reduce.  The count pass reads no sample.
//   k_n_test    the hot path, node-major: one chunk per workgroup and turn, its four samples per lane kept in registers as fp64, then the
//               queries paired with the chunk's node in tiles of NB_TILE from LDS; per query the lane's four d2 once, a ballot popcount into the
//               count, then selection rounds — the wave arg-min by (d2, ordinal) of the candidates above the previous winner — until no lane has a
//               candidate left or k are found; each wave leaves its sorted list in LDS and one lane per query merges the four into the
//               (chunk, query) partial: k entries and a count.  A chunk is read once however many queries reach its node.
//   k_n_reduce  one wave per query: up to k rounds of arg-min by (d2, node, ordinal) over the entries of the query's partials above the last
//               winner, the partial counts summed into within, the k records (the found ones, then miss records) written once.
// The only global atomics are integer counts and slot numbers inside a node's range of pairs.  The order in which pairs land in a node's range
// depends on the schedule; nothing that is returned does: the counts are sums of integers, each partial is written by one lane at an address
// fixed by (query, node, chunk), and the neighbours are a prefix of one total order in which no two samples are equal.
constexpr uint32_t NB_MAX_K = SIMLOD_NEIGHBOURS_MAX_K;
#ifndef NB_TILE_N
#define NB_TILE_N 32                                                              // (make variant DEFS="-DNB_TILE_N=64": the other tile DESIGN §11 measures)
#endif
constexpr uint32_t NB_TILE = NB_TILE_N;                                           // k_n_test: queries per LDS tile

struct NbEntry { double d2; uint32_t node, ordinal; };                            // 16 B: one entry of a partial; node NONE: none
static_assert(sizeof(NbEntry) == 16, "neighbour query records");
// a partial: NbEntry[k] (sorted, the unused ones NONE), then {uint32_t count, 0, 0, 0}: 16 * (k + 1) bytes
__host__ __device__ __forceinline__ uint64_t nb_part_bytes(uint32_t k) { return 16ull * (k + 1u); }

struct NbArgs {
	PairArgs              p;             // numQueries: the spheres
	const SimlodSphere*   queries;
	SimlodNeighbour*      neighbours;
	uint32_t*             within;
	SimlodNeighbourCounts* counts;
	uint32_t              k, pad;
};

// a query widened to fp64
struct SphereD { double c[3], rr; };

// rule 1; `s` is complete either way
__device__ __forceinline__ bool sphere_load(const SimlodSphere* queries, uint32_t i, SphereD& s) {
	const SimlodSphere v = queries[i];
	const float f[4] = {v.center[0], v.center[1], v.center[2], v.radius};
	bool ok = v.radius >= 0.0f;
#pragma unroll
	for (int k = 0; k < 4; k++) ok = ok && (__float_as_uint(f[k]) & 0x7f800000u) != 0x7f800000u;
#pragma unroll
	for (int k = 0; k < 3; k++) s.c[k] = (double)v.center[k];
	const double r = (double)v.radius;
	s.rr = r * r;
	return ok;
}

// rule 3 for one node
__device__ __forceinline__ bool sphere_cube(const SphereD& q, const PairArgs& a, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	const double s = ldexp(a.size, -(int)level), e = ldexp(a.size, -SIMLOD_MAX_DEPTH);
	const uint32_t A[3] = {X, Y, Z};
	double ex[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const double lo = (a.min[k] + (double)A[k] * s) - e, hi = (a.min[k] + ((double)A[k] + 1.0) * s) + e;
		ex[k] = fmax(fmax(lo - q.c[k], 0.0), q.c[k] - hi);
	}
	const double g2 = (ex[0] * ex[0] + ex[1] * ex[1]) + ex[2] * ex[2];
	return g2 <= q.rr;
}

// rule 2
__device__ __forceinline__ double sphere_d2(const SphereD& q, double x, double y, double z) {
	const double px = x - q.c[0], py = y - q.c[1], pz = z - q.c[2];
	return (px * px + py * py) + pz * pz;
}

// what the pair pipeline asks of a query (export_pairs.inc)
struct NbQuery {
	using Args = NbArgs;
	using Wide = SphereD;
	static constexpr bool COUNT_TESTS_SAMPLES = false;                             // numFound / numWithin are 0 in a count-only call
	static __device__ __forceinline__ bool load(const Args& n, uint32_t i, Wide& q) { return sphere_load(n.queries, i, q); }
	static __device__ __forceinline__ bool probe(const Wide& q, const PairArgs& p, const SimlodExportNode& e) { return sphere_cube(q, p, e.level, e.X, e.Y, e.Z); }
	static __host__ __device__ __forceinline__ bool wants_results(const Args& n) { return n.neighbours != nullptr; }
	static __host__ __device__ __forceinline__ uint64_t part_bytes(const Args& n) { return nb_part_bytes(n.k); }
	static __device__ __forceinline__ void write_counts(const Args& n, const PairTotals& t) {
		SimlodNeighbourCounts c;
		c.numNodes = t.numNodes; c.error = t.error; c.numInvalid = t.numInvalid; c.k = n.k;
		c.numPairs = t.numPairs; c.numCandidates = t.numCandidates; c.numFound = 0u; c.numWithin = 0u;    // (k_n_reduce adds the last two)
		*n.counts = c;
	}
};

// the order of the entries of one chunk: (d2, ordinal)
__device__ __forceinline__ bool nb_less(double d, uint32_t o, double bd, uint32_t bo) { return d < bd || (d == bd && o < bo); }

__global__ __launch_bounds__(LANE_TPB) void k_n_test(NbArgs n) {
	__shared__ double   sh_q[4][NB_TILE];                                          // cx, cy, cz, rr of the tile's queries
	__shared__ uint64_t sh_part[NB_TILE];
	__shared__ double   sh_d[PAIR_WAVES][NB_TILE][NB_MAX_K];                       // per wave and query: its sorted list ...
	__shared__ uint32_t sh_o[PAIR_WAVES][NB_TILE][NB_MAX_K];
	__shared__ uint32_t sh_n[PAIR_WAVES][NB_TILE];                                 // ... its length ...
	__shared__ uint32_t sh_c[PAIR_WAVES][NB_TILE];                                 // ... and how many of the wave's samples passed
	static_assert(sizeof(sh_q) + sizeof(sh_part) + sizeof(sh_d) + sizeof(sh_o) + sizeof(sh_n) + sizeof(sh_c) <= 64u * 1024u, "k_n_test: static LDS (a tile of 32: 26 KB, of 64: 53 KB)");
	const ExportArgs& x = n.p.x;
	const Header* hdr = reinterpret_cast<const Header*>(x.scratch);
	const PairHeader* ph = reinterpret_cast<const PairHeader*>(x.scratch + 256u);
	if (ph->doResults == 0u || ph->numPairs == 0u) return;
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + n.p.at.cnt);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + n.p.at.nfirst);
	const Pair* pairs = reinterpret_cast<const Pair*>(x.scratch + ph->pairsOff);
	uint8_t* parts = x.scratch + ph->partsOff;
	const uint64_t numItems = hdr->totalChunks;
	const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x / SIMLOD_WAVE;
	const uint32_t K = min(n.k, NB_MAX_K);                                         // (the launcher refuses more: every LDS index below is < NB_MAX_K)
	const uint64_t pb = nb_part_bytes(n.k);
	const double INF = __builtin_huge_val();
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const QItem it = items[i];
		const uint32_t c = cnt[it.node];                                           // (the same for the whole workgroup, as every branch on `it`)
		if (c == 0u) continue;
		double sx[4], sy[4], sz[4];
		test_chunk(it, sx, sy, sz);
		const uint64_t pf = nfirst[it.node];
		for (uint32_t j0 = 0; j0 < c; j0 += NB_TILE) {
			const uint32_t nt = min(NB_TILE, c - j0);
			__syncthreads();                                                       // (the tile before is done with)
			if (threadIdx.x < nt) {
				const Pair p = pairs[pf + j0 + threadIdx.x];
				SphereD q;
				sphere_load(n.queries, p.query, q);                                // (valid: it formed a pair)
				sh_q[0][threadIdx.x] = q.c[0]; sh_q[1][threadIdx.x] = q.c[1]; sh_q[2][threadIdx.x] = q.c[2]; sh_q[3][threadIdx.x] = q.rr;
				sh_part[threadIdx.x] = p.part;
			}
			__syncthreads();
			for (uint32_t qi = 0; qi < nt; qi++) {                                 // (qi < nt <= NB_TILE)
				SphereD q;
				q.c[0] = sh_q[0][qi]; q.c[1] = sh_q[1][qi]; q.c[2] = sh_q[2][qi]; q.rr = sh_q[3][qi];
				double d[4];
				uint32_t passed = 0;
#pragma unroll
				for (int j = 0; j < 4; j++) {
					const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
					const double d2 = sphere_d2(q, sx[j], sy[j], sz[j]);
					const bool ok = k < it.count && d2 <= q.rr;
					d[j] = ok ? d2 : INF;                                          // (a passing d2 is finite: rr is)
					passed += (uint32_t)__popcll(__ballot(ok));
				}
				// selection rounds: the wave's minimum by (d2, ordinal) among the candidates above the last winner
				double ld = -1.0;                                                  // (below every d2)
				uint32_t lo = 0u, found = 0u;
				while (found < K) {
					double bd = INF;
					uint32_t bo = NONE;
#pragma unroll
					for (int j = 0; j < 4; j++) {
						const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
						if (d[j] != INF && nb_less(ld, lo, d[j], k) && nb_less(d[j], k, bd, bo)) { bd = d[j]; bo = k; }
					}
					if (__ballot(bo != NONE) == 0ull) break;
					const Hit m = wave_hit_min<false>(bd, 0u, bo);
					if (lane == 0u) { sh_d[w][qi][found] = m.t; sh_o[w][qi][found] = m.ord; }   // (found < K <= NB_MAX_K)
					ld = m.t; lo = m.ord;
					found++;
				}
				if (lane == 0u) { sh_n[w][qi] = found; sh_c[w][qi] = passed; }
			}
			__syncthreads();
			if (threadIdx.x < nt) {
				// the four-way merge of the waves' lists into the (chunk, query) partial
				const uint32_t t = threadIdx.x;
				uint8_t* out = parts + (sh_part[t] + it.k) * pb;
				uint32_t h[PAIR_WAVES] = {0u, 0u, 0u, 0u}, len[PAIR_WAVES], total = 0u;
#pragma unroll
				for (uint32_t ww = 0; ww < PAIR_WAVES; ww++) { len[ww] = min(sh_n[ww][t], K); total += sh_c[ww][t]; }
				for (uint32_t r = 0; r < n.k; r++) {
					double bd = INF;
					uint32_t bo = NONE, bw = PAIR_WAVES;
#pragma unroll
					for (uint32_t ww = 0; ww < PAIR_WAVES; ww++) {
						if (h[ww] < len[ww]) {                                     // (h < len <= K <= NB_MAX_K)
							const double od = sh_d[ww][t][h[ww]];
							const uint32_t oo = sh_o[ww][t][h[ww]];
							if (bw == PAIR_WAVES || nb_less(od, oo, bd, bo)) { bd = od; bo = oo; bw = ww; }
						}
					}
#pragma unroll
					for (uint32_t ww = 0; ww < PAIR_WAVES; ww++) h[ww] += ww == bw ? 1u : 0u;
					NbEntry e;
					e.d2 = bd; e.node = bw != PAIR_WAVES ? it.node : NONE; e.ordinal = bw != PAIR_WAVES ? it.k * SIMLOD_POINTS_PER_CHUNK + bo : NONE;
					reinterpret_cast<NbEntry*>(out)[r] = e;
				}
				uint4 tail;
				tail.x = total; tail.y = 0u; tail.z = 0u; tail.w = 0u;
				*reinterpret_cast<uint4*>(out + 16ull * n.k) = tail;
			}
		}
	}
}
static_assert(NB_TILE <= LANE_TPB && PAIR_WAVES == 4 && NB_MAX_K == 16, "k_n_test: a lane per query of the tile, four waves, lists of at most 16");

__global__ __launch_bounds__(LANE_TPB) void k_n_reduce(NbArgs n) {
	const ExportArgs& x = n.p.x;
	const PairHeader* ph = reinterpret_cast<const PairHeader*>(x.scratch + 256u);
	const uint32_t w = threadIdx.x / SIMLOD_WAVE, lane = (uint32_t)lane_id();
	const uint32_t qi = blockIdx.x * PAIR_WAVES + w;
	if (qi >= n.p.numQueries || ph->doResults == 0u) return;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(x.scratch + x.lay.first);
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	const uint64_t* qFirst = reinterpret_cast<const uint64_t*>(x.scratch + n.p.at.qFirst);
	const uint8_t* parts = x.scratch + ph->partsOff;
	const uint64_t pb = nb_part_bytes(n.k);
	const uint64_t p0 = qFirst[qi], np = qFirst[qi + 1u] - p0;
	const uint8_t* mine = parts + p0 * pb;
	// within: the partial counts
	uint64_t total = 0;
	for (uint64_t p = lane; p < np; p += SIMLOD_WAVE) total += *reinterpret_cast<const uint32_t*>(mine + p * pb + 16ull * n.k);
#pragma unroll
	for (int o = SIMLOD_WAVE / 2; o > 0; o >>= 1) total += __shfl_xor(total, o, SIMLOD_WAVE);
	SimlodNeighbour* out = n.neighbours + (uint64_t)qi * n.k;
	const uint64_t numEntries = np * n.k;
	double ld = -1.0;                                                              // the last winner (below every entry)
	uint32_t ln = 0u, lo = 0u, found = 0u;
	while (found < n.k) {
		double bd = __builtin_huge_val();
		uint32_t bn = NONE, bo = NONE;
		for (uint64_t e = lane; e < numEntries; e += SIMLOD_WAVE) {
			const NbEntry v = *reinterpret_cast<const NbEntry*>(mine + (e / n.k) * pb + 16ull * (e % n.k));
			if (v.node != NONE && hit_less(ld, ln, lo, v.d2, v.node, v.ordinal) && (bn == NONE || hit_less(v.d2, v.node, v.ordinal, bd, bn, bo))) { bd = v.d2; bn = v.node; bo = v.ordinal; }
		}
		if (__ballot(bn != NONE) == 0ull) break;
		const Hit m = wave_hit_min<true>(bd, bn, bo);
		if (lane == 0u) {
			SimlodNeighbour r;
			r.d2 = m.t; r.node = m.node; r.ordinal = m.ord;
			const QItem it = items[first[m.node] + m.ord / SIMLOD_POINTS_PER_CHUNK];
			r.sample = reinterpret_cast<const SimlodPoint*>(it.src)[m.ord % SIMLOD_POINTS_PER_CHUNK];
			out[found] = r;
		}
		ld = m.t; ln = m.node; lo = m.ord;
		found++;
	}
	if (lane != 0u) return;
	SimlodNeighbour miss;
	miss.d2 = __builtin_huge_val(); miss.node = NONE; miss.ordinal = NONE;
	miss.sample.x = 0.0f; miss.sample.y = 0.0f; miss.sample.z = 0.0f; miss.sample.color = 0u;
	for (uint32_t r = found; r < n.k; r++) out[r] = miss;
	if (n.within != nullptr) n.within[qi] = (uint32_t)total;
	if (total != 0u) {
		atomicAdd((unsigned long long*)&n.counts->numFound, (unsigned long long)found);
		atomicAdd((unsigned long long*)&n.counts->numWithin, (unsigned long long)total);
	}
}
