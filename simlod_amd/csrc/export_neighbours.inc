// export_neighbours.inc — part of export.hip: neighbour queries.  NbArgs, SphereD, sphere_load, sphere_cube, NbEntry, nb_less, k_n_pairs, k_n_scan,
// k_n_test, k_n_reduce.  (After export_rays.inc: the layout, the pair records, wave_descend and wave_hit_min are the ray query's.)
// ---- neighbour query ------------------------------------------------------------------------------------------------------------------
// simlod_query_neighbours (simlod_hip.h, "neighbour queries"): seven launches on the caller's stream, four for a count-only call.
//   k_r_hier    the ray query's kernel as it is (the walk, the scans, the cleared counts), over RayLayout(cap, numQueries).
//   k_q_dir     the region query's directory kernel as it is: one item per chunk of every selected node.
//   k_n_pairs   one WAVE per query: wave_descend (export_rays.inc) with the sphere-cube probe of rule 3.
//               <count>: queries per node (an atomic count: the sum is the same in any order), chunks per query, numPairs, numCandidates,
//               numInvalid.  No sample is read.
//               <fill>: the same descent writes each pair {query, the query's first partial for this node} into its node's range.
//   k_n_scan    ONE workgroup: queries per node -> each node's range of pairs; chunks per query -> each query's range of partials; the
//               capacity check; SimlodNeighbourCounts.
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

struct NbEntry { double d2; uint32_t node, ordinal; };                            // 16 B: one entry of a partial (RayPart's shape); node NONE: none
static_assert(sizeof(NbEntry) == 16 && sizeof(RayPart) == sizeof(NbEntry), "neighbour query records");
// a partial: NbEntry[k] (sorted, the unused ones NONE), then {uint32_t count, 0, 0, 0}: 16 * (k + 1) bytes
__host__ __device__ __forceinline__ uint64_t nb_part_bytes(uint32_t k) { return 16ull * (k + 1u); }

struct NbArgs {
	RayArgs               r;             // the ray query's view: r.x, the box, numRays = numQueries, scratchBytes, the offsets (r.rays / r.hits unused)
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
__device__ __forceinline__ bool sphere_cube(const SphereD& q, const RayArgs& a, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
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

template <int FILL>
__global__ __launch_bounds__(LANE_TPB) void k_n_pairs(NbArgs n) {
	__shared__ uint32_t sh_fc[RAY_WAVES][RAY_LEVELS][SIMLOD_WAVE];                 // pending nodes per level: their firstChild ...
	__shared__ uint8_t  sh_mk[RAY_WAVES][RAY_LEVELS][SIMLOD_WAVE];                 // ... and childMask
	const RayArgs& a = n.r;
	const ExportArgs& x = a.x;
	const Header* hdr = reinterpret_cast<const Header*>(x.scratch);
	RayHeader* rh = reinterpret_cast<RayHeader*>(x.scratch + 256u);
	const uint32_t w = threadIdx.x / SIMLOD_WAVE, lane = (uint32_t)lane_id();
	const uint32_t qi = blockIdx.x * RAY_WAVES + w;
	if (qi >= a.numRays || hdr->error != 0u || (FILL && rh->doHits == 0u)) return;      // (the same for the whole wave, as every exit below)
	const uint32_t numListed = hdr->numListed;
	uint32_t* cnt = reinterpret_cast<uint32_t*>(x.scratch + a.at.cnt);
	uint32_t* fill = reinterpret_cast<uint32_t*>(x.scratch + a.at.fill);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + a.at.nfirst);
	uint32_t* qParts = reinterpret_cast<uint32_t*>(x.scratch + a.at.rayParts);
	const uint64_t* qFirst = reinterpret_cast<const uint64_t*>(x.scratch + a.at.rayFirst);
	SphereD q;
	const bool valid = sphere_load(n.queries, qi, q);
	if (!valid) {
		if (!FILL && lane == 0u) { atomicAdd(&rh->numInvalid, 1u); qParts[qi] = 0u; }
		return;
	}
	uint32_t nPairs = 0, nParts = 0;                                               // this lane's share (count)
	uint64_t nCand = 0;
	uint64_t run = FILL ? qFirst[qi] : 0u;                                         // (fill) the query's next free partial
	RayPair* pairs = reinterpret_cast<RayPair*>(x.scratch + rh->pairsOff);

	// what a turn does with its pairs: isPair per lane, `node` its table index, `ns` its samples
	auto on_pairs = [&](bool isPair, uint32_t node, uint32_t ns) {
		if (__ballot(isPair) == 0ull) return;
		if (FILL) {
			const uint32_t nch = isPair ? ceil_chunks(ns) : 0u;
			const uint32_t incl = wave_incl_scan(nch);
			if (isPair) {
				const uint64_t slot = nfirst[node] + atomicAdd(&fill[node], 1u);
				RayPair p;
				p.part = run + (incl - nch); p.ray = qi; p.pad = 0u;
				pairs[slot] = p;
			}
			run += __shfl(incl, SIMLOD_WAVE - 1, SIMLOD_WAVE);
			return;
		}
		if (isPair) { atomicAdd(&cnt[node], 1u); nPairs++; nParts += ceil_chunks(ns); nCand += ns; }
	};
	wave_descend(x, numListed, sh_fc[w], sh_mk[w], lane, [&](const SimlodExportNode& e) { return sphere_cube(q, a, e.level, e.X, e.Y, e.Z); }, on_pairs);
	if (FILL) return;
#pragma unroll
	for (int o = SIMLOD_WAVE / 2; o > 0; o >>= 1) {
		nPairs += __shfl_xor(nPairs, o, SIMLOD_WAVE);
		nParts += __shfl_xor(nParts, o, SIMLOD_WAVE);
		nCand += __shfl_xor(nCand, o, SIMLOD_WAVE);
	}
	if (lane == 0u) {
		qParts[qi] = nParts;
		if (nPairs != 0u) { atomicAdd((unsigned long long*)&rh->numPairs, (unsigned long long)nPairs); atomicAdd((unsigned long long*)&rh->numCand, (unsigned long long)nCand); }
	}
}

__global__ __launch_bounds__(WG_TPB) void k_n_scan(NbArgs n) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const RayArgs& a = n.r;
	const ExportArgs& x = a.x;
	Header* hdr = reinterpret_cast<Header*>(x.scratch);
	RayHeader* rh = reinterpret_cast<RayHeader*>(x.scratch + 256u);
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + a.at.cnt);
	uint64_t* nfirst = reinterpret_cast<uint64_t*>(x.scratch + a.at.nfirst);
	const uint32_t* qParts = reinterpret_cast<const uint32_t*>(x.scratch + a.at.rayParts);
	uint64_t* qFirst = reinterpret_cast<uint64_t*>(x.scratch + a.at.rayFirst);
	const uint32_t nn = hdr->numListed;
	uint32_t err = hdr->error;
	uint64_t pairs = 0, parts = 0;
	if (err == 0u) {
		for (uint32_t base = 0; base < nn; base += WG_TPB) {
			const uint32_t t = base + threadIdx.x;
			uint64_t tot;
			const uint64_t off = block_scan<uint64_t>(t < nn ? cnt[t] : 0u, tot, sh_scan);
			if (t < nn) nfirst[t] = pairs + off;
			pairs += tot;
		}
		// four queries per lane and turn
		for (uint32_t base = 0; base < a.numRays; base += 4u * WG_TPB) {
			const uint32_t i = base + 4u * threadIdx.x;
			uint32_t v[4];
#pragma unroll
			for (uint32_t j = 0; j < 4u; j++) v[j] = i + j < a.numRays ? qParts[i + j] : 0u;
			uint64_t tot;
			uint64_t off = parts + block_scan<uint64_t>((uint64_t)v[0] + v[1] + v[2] + v[3], tot, sh_scan);
#pragma unroll
			for (uint32_t j = 0; j < 4u; j++) {
				if (i + j < a.numRays) qFirst[i + j] = off;
				off += v[j];
			}
			parts += tot;
		}
	}
	if (threadIdx.x == 0) {
		nfirst[nn] = pairs;
		qFirst[a.numRays] = parts;
		// what a call with results needs behind the items: per pair its record and one partial, one partial more per further thousand candidates
		const uint64_t numCand = rh->numCand;
		const uint64_t pairsOff = x.lay.items + hdr->totalChunks * sizeof(QItem);
		const uint64_t need = pairsOff + pairs * (sizeof(RayPair) + nb_part_bytes(n.k)) + (numCand / SIMLOD_POINTS_PER_CHUNK) * nb_part_bytes(n.k);
		if (n.neighbours != nullptr && err == 0u && need > a.scratchBytes) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		hdr->error = err;
		rh->numPairs = pairs; rh->numParts = parts;
		rh->pairsOff = pairsOff; rh->partsOff = pairsOff + pairs * sizeof(RayPair);
		rh->doHits = n.neighbours != nullptr && err == 0u ? 1u : 0u;
		SimlodNeighbourCounts c;
		c.numNodes = nn; c.error = err; c.numInvalid = rh->numInvalid; c.k = n.k;
		c.numPairs = pairs; c.numCandidates = numCand; c.numFound = 0u; c.numWithin = 0u;    // (k_n_reduce adds the last two)
		*n.counts = c;
	}
}

// the order of the entries of one chunk: (d2, ordinal)
__device__ __forceinline__ bool nb_less(double d, uint32_t o, double bd, uint32_t bo) { return d < bd || (d == bd && o < bo); }

__global__ __launch_bounds__(LANE_TPB) void k_n_test(NbArgs n) {
	__shared__ double   sh_q[4][NB_TILE];                                          // cx, cy, cz, rr of the tile's queries
	__shared__ uint64_t sh_part[NB_TILE];
	__shared__ double   sh_d[RAY_WAVES][NB_TILE][NB_MAX_K];                        // per wave and query: its sorted list ...
	__shared__ uint32_t sh_o[RAY_WAVES][NB_TILE][NB_MAX_K];
	__shared__ uint32_t sh_n[RAY_WAVES][NB_TILE];                                  // ... its length ...
	__shared__ uint32_t sh_c[RAY_WAVES][NB_TILE];                                  // ... and how many of the wave's samples passed
	static_assert(sizeof(sh_q) + sizeof(sh_part) + sizeof(sh_d) + sizeof(sh_o) + sizeof(sh_n) + sizeof(sh_c) <= 64u * 1024u, "k_n_test: static LDS (a tile of 32: 26 KB, of 64: 53 KB)");
	const RayArgs& a = n.r;
	const ExportArgs& x = a.x;
	const Header* hdr = reinterpret_cast<const Header*>(x.scratch);
	const RayHeader* rh = reinterpret_cast<const RayHeader*>(x.scratch + 256u);
	if (rh->doHits == 0u || rh->numPairs == 0u) return;
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + a.at.cnt);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + a.at.nfirst);
	const RayPair* pairs = reinterpret_cast<const RayPair*>(x.scratch + rh->pairsOff);
	uint8_t* parts = x.scratch + rh->partsOff;
	const uint64_t numItems = hdr->totalChunks;
	const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x / SIMLOD_WAVE;
	const uint32_t K = min(n.k, NB_MAX_K);                                         // (the launcher refuses more: every LDS index below is < NB_MAX_K)
	const uint64_t pb = nb_part_bytes(n.k);
	const double INF = __builtin_huge_val();
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const QItem it = items[i];
		const uint32_t c = cnt[it.node];                                           // (the same for the whole workgroup, as every branch on `it`)
		if (c == 0u) continue;
		u32x4 v[4];
		load_chunk4<false, true>(reinterpret_cast<const u32x4*>(it.src), it.count, v);
		double sx[4], sy[4], sz[4];
#pragma unroll
		for (int j = 0; j < 4; j++) { sx[j] = (double)__uint_as_float(v[j].x); sy[j] = (double)__uint_as_float(v[j].y); sz[j] = (double)__uint_as_float(v[j].z); }
		const uint64_t pf = nfirst[it.node];
		for (uint32_t j0 = 0; j0 < c; j0 += NB_TILE) {
			const uint32_t nt = min(NB_TILE, c - j0);
			__syncthreads();                                                       // (the tile before is done with)
			if (threadIdx.x < nt) {
				const RayPair p = pairs[pf + j0 + threadIdx.x];
				SphereD q;
				sphere_load(n.queries, p.ray, q);                                  // (valid: it formed a pair)
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
				uint32_t h[RAY_WAVES] = {0u, 0u, 0u, 0u}, len[RAY_WAVES], total = 0u;
#pragma unroll
				for (uint32_t ww = 0; ww < RAY_WAVES; ww++) { len[ww] = min(sh_n[ww][t], K); total += sh_c[ww][t]; }
				for (uint32_t r = 0; r < n.k; r++) {
					double bd = INF;
					uint32_t bo = NONE, bw = RAY_WAVES;
#pragma unroll
					for (uint32_t ww = 0; ww < RAY_WAVES; ww++) {
						if (h[ww] < len[ww]) {                                     // (h < len <= K <= NB_MAX_K)
							const double od = sh_d[ww][t][h[ww]];
							const uint32_t oo = sh_o[ww][t][h[ww]];
							if (bw == RAY_WAVES || nb_less(od, oo, bd, bo)) { bd = od; bo = oo; bw = ww; }
						}
					}
#pragma unroll
					for (uint32_t ww = 0; ww < RAY_WAVES; ww++) h[ww] += ww == bw ? 1u : 0u;
					NbEntry e;
					e.d2 = bd; e.node = bw != RAY_WAVES ? it.node : NONE; e.ordinal = bw != RAY_WAVES ? it.k * SIMLOD_POINTS_PER_CHUNK + bo : NONE;
					reinterpret_cast<NbEntry*>(out)[r] = e;
				}
				uint4 tail;
				tail.x = total; tail.y = 0u; tail.z = 0u; tail.w = 0u;
				*reinterpret_cast<uint4*>(out + 16ull * n.k) = tail;
			}
		}
	}
}
static_assert(NB_TILE <= LANE_TPB && RAY_WAVES == 4 && NB_MAX_K == 16, "k_n_test: a lane per query of the tile, four waves, lists of at most 16");

__global__ __launch_bounds__(LANE_TPB) void k_n_reduce(NbArgs n) {
	const RayArgs& a = n.r;
	const ExportArgs& x = a.x;
	const RayHeader* rh = reinterpret_cast<const RayHeader*>(x.scratch + 256u);
	const uint32_t w = threadIdx.x / SIMLOD_WAVE, lane = (uint32_t)lane_id();
	const uint32_t qi = blockIdx.x * RAY_WAVES + w;
	if (qi >= a.numRays || rh->doHits == 0u) return;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(x.scratch + x.lay.first);
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	const uint64_t* qFirst = reinterpret_cast<const uint64_t*>(x.scratch + a.at.rayFirst);
	const uint8_t* parts = x.scratch + rh->partsOff;
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
