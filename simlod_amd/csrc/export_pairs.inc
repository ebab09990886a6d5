// export_pairs.inc — part of export.hip: the pair pipeline under the ray and the neighbour query.  The pair records, PairLayout, PairArgs,
// k_p_hier, hit_less, wave_hit_min, wave_descend, k_p_pairs, k_p_scan, pair_need, test_chunk.
// ---- pair queries ---------------------------------------------------------------------------------------------------------------------
// A pair query (simlod_query_rays, simlod_query_neighbours) pairs each record of a batch with the selected nodes it can reach, tests the
// samples of every pair and reduces per record: seven launches on the caller's stream, four for a count-only call.
//   k_p_hier    ONE workgroup: k_x_hier's walk (the table is the export's, into the caller's array or into scratch), then k_x_scan's scans:
//               firstSample, the node's first chunk item, the item capacity.
//   k_q_dir     the region query's directory kernel as it is (every entry tagged as copied): one item per chunk of every selected node.
//   k_p_pairs   one WAVE per query, the table descended depth first with a bucket of pending nodes per level: a turn takes up to eight nodes of
//               the deepest level that has any and probes their 64 children, one lane each (rule 3), so a bucket never holds more than 64.
//               <count>: queries per node (an atomic count: the sum is the same in any order), chunks per query, numPairs, numCandidates,
//               numInvalid; where the query says so (Q::COUNT_TESTS_SAMPLES) a count-only call also counts numHits, query-major, stopping
//               at a query's first passing sample.
//               <fill>: the same descent writes each pair {query, the query's first partial for this node} into its node's range.
//   k_p_scan    ONE workgroup: queries per node -> each node's range of pairs; chunks per query -> each query's range of partials; the
//               capacity check; the query's counts record.
//   the query's test kernel (node-major: a chunk is read once however many queries reach its node) and its reduce kernel (one wave per query).
// The pipeline exists once.  A query Q supplies: Q::Args (a PairArgs `p` first, then its own pointers), Q::Wide (a record widened to fp64),
// Q::load (rule 1), Q::probe (rule 3), Q::wants_results, Q::part_bytes (the size of one (chunk, query) partial), Q::write_counts,
// COUNT_TESTS_SAMPLES with Q::passes (rule 2), and its test and reduce kernels.
// The order in which pairs land in a node's range depends on the schedule; nothing that is returned does.
constexpr uint32_t PAIR_WAVES = LANE_TPB / SIMLOD_WAVE;                           // k_p_pairs / the reduce kernels: queries per workgroup
constexpr uint32_t PAIR_LEVELS = SIMLOD_MAX_DEPTH;                                // buckets: a node at level 20 has no children

struct PairHeader {                      // at byte 256 of the scratch buffer
	uint64_t numPairs, numCand, numParts, pairsOff, partsOff;
	uint32_t numInvalid, numHits, doResults, pad;
};
struct Pair { uint64_t part; uint32_t query, pad; };                              // 16 B: a query paired with a node, and its first partial for that node
static_assert(sizeof(Pair) == 16 && sizeof(PairHeader) <= 256, "pair query records");

// scratch: Header | PairHeader | map | par | first | cls | tab (the table when the caller wants none) | cnt | fill | nfirst u64[cap + 1] |
// qParts u32[numQueries] | qFirst u64[numQueries + 1] | items QItem[chunks] | pairs Pair[numPairs] | partials [<= numCandidates / 1000 + numPairs]
struct PairOffsets { uint64_t cls, cnt, fill, nfirst, qParts, qFirst; };          // what the pair kernels find beside the walk's arrays
struct PairLayout {
	Layout      x;                      // map / par / first / items; itemCap and bytes once the buffer is known (take_rest)
	uint64_t    tab;
	PairOffsets at;
	__host__ __device__ PairLayout(uint32_t cap, uint32_t numQueries) {
		const uint64_t q = align256(4ull * cap);
		x.map = 512u; x.par = x.map + q; x.first = x.par + q; at.cls = x.first + align256(4ull * cap + 4u); tab = at.cls + q;
		at.cnt = tab + align256(sizeof(SimlodExportNode) * (uint64_t)cap); at.fill = at.cnt + q; at.nfirst = at.fill + q;
		at.qParts = at.nfirst + align256(8ull * cap + 8u); at.qFirst = at.qParts + align256(4ull * numQueries);
		x.items = at.qFirst + align256(8ull * numQueries + 8u);
	}
};

// what a call needs up to the end of its partials (`partBytes` each): per pair its record and one partial, one partial more per further
// thousand candidates.  The scratch bounds and k_p_scan's capacity check are this one formula.
__host__ __device__ inline uint64_t pair_need(uint64_t pairsOff, uint64_t numPairs, uint64_t numCand, uint64_t partBytes) {
	return pairsOff + numPairs * (sizeof(Pair) + partBytes) + (numCand / SIMLOD_POINTS_PER_CHUNK) * partBytes;
}

struct PairArgs {
	ExportArgs  x;                      // (x.table: the caller's table or `tab`; x.lay: map / par / first / items / itemCap)
	double      min[3], size;
	uint32_t    numQueries, pad;
	uint64_t    scratchBytes;
	PairOffsets at;
};

__global__ __launch_bounds__(WG_TPB) void k_p_hier(PairArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const ExportArgs& x = a.x;
	hier_walk<false>(x, NoRegion(), nullptr);
	__syncthreads();
	Header* hdr = reinterpret_cast<Header*>(x.scratch);
	uint32_t* cls = reinterpret_cast<uint32_t*>(x.scratch + a.at.cls);
	uint32_t* cnt = reinterpret_cast<uint32_t*>(x.scratch + a.at.cnt);
	uint32_t* fill = reinterpret_cast<uint32_t*>(x.scratch + a.at.fill);
	const TableScan s = scan_table(x, sh_scan, [&](uint32_t t) { cls[t] = Q_COPIED; cnt[t] = 0u; fill[t] = 0u; });
	if (threadIdx.x == 0) {
		hdr->error = s.err;
		hdr->totalChunks = (s.err & SIMLOD_EXPORT_ERR_CAPACITY) ? 0u : s.items;  // the items k_q_dir writes
		PairHeader ph{};
		*reinterpret_cast<PairHeader*>(x.scratch + 256u) = ph;
	}
}

// the total order of the results: (key, node, ordinal), the key being t (ray query, rule 4) or d2 (neighbour query)
__device__ __forceinline__ bool hit_less(double t, uint32_t node, uint32_t ord, double bt, uint32_t bnode, uint32_t bord) {
	return t < bt || (t == bt && (node < bnode || (node == bnode && ord < bord)));
}

// The wave's minimum in that order, in every lane (call it where some lane has a candidate).  BY_NODE: a lane whose node is NONE has none;
// else every lane passes the same node and (t, ordinal) decides.
struct Hit { double t; uint32_t node, ord; };
template <bool BY_NODE>
__device__ __forceinline__ Hit wave_hit_min(double bt, uint32_t bn, uint32_t bo) {
#pragma unroll
	for (int o = SIMLOD_WAVE / 2; o > 0; o >>= 1) {
		const double ot = __shfl_xor(bt, o, SIMLOD_WAVE);
		const uint32_t on = BY_NODE ? __shfl_xor(bn, o, SIMLOD_WAVE) : bn, oo = __shfl_xor(bo, o, SIMLOD_WAVE);
		if ((!BY_NODE || on != NONE) && hit_less(ot, on, oo, bt, bn, bo)) { bt = ot; bn = on; bo = oo; }
	}
	return Hit{bt, bn, bo};
}

// One WAVE descends the table depth first with a bucket of pending nodes per level (fc / mk: this wave's buckets in LDS): a turn takes up to
// eight nodes of the deepest level that has any and probes their 64 children, one lane each, so a bucket never holds more than 64.
// probe(entry): does the node pass (rule 3 of the query); on_pairs(isPair per lane, table index, samples) once per turn for the selected
// entries with samples among those that passed.
template <class Probe, class OnPairs>
__device__ __forceinline__ void wave_descend(const ExportArgs& x, uint32_t numListed, uint32_t (&fc)[PAIR_LEVELS][SIMLOD_WAVE], uint8_t (&mk)[PAIR_LEVELS][SIMLOD_WAVE],
                                             uint32_t lane, Probe probe, OnPairs on_pairs) {
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t myCnt = 0;                                                            // lane L: the nodes pending at level L
	int cur = -1;                                                                  // the deepest level that may have any
	{
		const SimlodExportNode e = x.table[0];
		if (probe(e)) {
			if (e.childMask != 0u) {
				if (lane == 0u) { fc[0][0] = e.firstChild; mk[0][0] = e.childMask; myCnt = 1u; }
				cur = 0;
			}
			on_pairs(lane == 0u && e.numSamples != 0u && (e.flags & SIMLOD_EXPORT_FLAG_SELECTED) != 0u, 0u, e.numSamples);
		}
	}
	while (cur >= 0) {
		const uint32_t c = __shfl(myCnt, cur, SIMLOD_WAVE);
		if (c == 0u) { cur--; continue; }
		const uint32_t take = min(c, 8u), base = c - take;
		if ((int)lane == cur) myCnt = base;
		__builtin_amdgcn_wave_barrier();                                           // (the buckets go from lane to lane through LDS, inside one wave)
		const uint32_t e = lane >> 3, k = lane & 7u;
		bool has = false;
		uint32_t ci = 0;
		if (e < take) {
			const uint32_t f = fc[cur][base + e], m = mk[cur][base + e];
			ci = f + (uint32_t)__popc(m & ((1u << k) - 1u));
			has = ((m >> k) & 1u) != 0u && ci < numListed;
		}
		SimlodExportNode ce{};
		bool pass = false;
		if (has) { ce = x.table[ci]; pass = probe(ce); }
		const bool push = pass && ce.childMask != 0u && cur + 1 < (int)PAIR_LEVELS;
		const uint64_t pb = __ballot(push);
		__builtin_amdgcn_wave_barrier();
		if (pb != 0ull) {
			// (level cur + 1 was empty: cur is the deepest level with anything pending, so a bucket holds at most these 64)
			if (push) { const uint32_t pos = (uint32_t)__popcll(pb & below); fc[cur + 1][pos] = ce.firstChild; mk[cur + 1][pos] = ce.childMask; }
			if ((int)lane == cur + 1) myCnt = (uint32_t)__popcll(pb);
			cur++;
		}
		__builtin_amdgcn_wave_barrier();
		on_pairs(pass && ce.numSamples != 0u && (ce.flags & SIMLOD_EXPORT_FLAG_SELECTED) != 0u, ci, ce.numSamples);
	}
}

template <class Q, int FILL>
__global__ __launch_bounds__(LANE_TPB) void k_p_pairs(typename Q::Args a) {
	__shared__ uint32_t sh_fc[PAIR_WAVES][PAIR_LEVELS][SIMLOD_WAVE];               // pending nodes per level: their firstChild ...
	__shared__ uint8_t  sh_mk[PAIR_WAVES][PAIR_LEVELS][SIMLOD_WAVE];               // ... and childMask
	const PairArgs& p = a.p;
	const ExportArgs& x = p.x;
	const Header* hdr = reinterpret_cast<const Header*>(x.scratch);
	PairHeader* ph = reinterpret_cast<PairHeader*>(x.scratch + 256u);
	const uint32_t w = threadIdx.x / SIMLOD_WAVE, lane = (uint32_t)lane_id();
	const uint32_t qi = blockIdx.x * PAIR_WAVES + w;
	if (qi >= p.numQueries || hdr->error != 0u || (FILL && ph->doResults == 0u)) return;   // (the same for the whole wave, as every exit below)
	const uint32_t numListed = hdr->numListed;
	uint32_t* cnt = reinterpret_cast<uint32_t*>(x.scratch + p.at.cnt);
	uint32_t* fill = reinterpret_cast<uint32_t*>(x.scratch + p.at.fill);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + p.at.nfirst);
	uint32_t* qParts = reinterpret_cast<uint32_t*>(x.scratch + p.at.qParts);
	const uint64_t* qFirst = reinterpret_cast<const uint64_t*>(x.scratch + p.at.qFirst);
	typename Q::Wide q;
	const bool valid = Q::load(a, qi, q);
	if (!valid) {
		if (!FILL && lane == 0u) { atomicAdd(&ph->numInvalid, 1u); qParts[qi] = 0u; }
		return;
	}
	uint32_t nPairs = 0, nParts = 0;                                               // this lane's share (count)
	uint64_t nCand = 0;
	bool found = false;                                                            // (COUNT_TESTS_SAMPLES alone: a count-only call found a passing sample)
	uint64_t run = FILL ? qFirst[qi] : 0u;                                         // (fill) the query's next free partial
	Pair* pairs = reinterpret_cast<Pair*>(x.scratch + ph->pairsOff);

	// what a turn does with its pairs: isPair per lane, `node` its table index, `ns` its samples
	auto on_pairs = [&](bool isPair, uint32_t node, uint32_t ns) {
		const uint64_t pm = __ballot(isPair);
		if (pm == 0ull) return;
		if (FILL) {
			const uint32_t nch = isPair ? ceil_chunks(ns) : 0u;
			const uint32_t incl = wave_incl_scan(nch);
			if (isPair) {
				const uint64_t slot = nfirst[node] + atomicAdd(&fill[node], 1u);
				Pair pr;
				pr.part = run + (incl - nch); pr.query = qi; pr.pad = 0u;
				pairs[slot] = pr;
			}
			run += __shfl(incl, SIMLOD_WAVE - 1, SIMLOD_WAVE);
			return;
		}
		if (isPair) { atomicAdd(&cnt[node], 1u); nPairs++; nParts += ceil_chunks(ns); nCand += ns; }
		if constexpr (Q::COUNT_TESTS_SAMPLES) {
			if (Q::wants_results(a) || found) return;
			// count only: is there any passing sample?  The wave takes the turn's pairs one after the other and leaves at the first.
			const uint32_t* first = reinterpret_cast<const uint32_t*>(x.scratch + x.lay.first);
			const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
			for (uint64_t m = pm; m != 0ull && !found; m &= m - 1ull) {
				const int b = __ffsll((long long)m) - 1;
				const uint32_t nd = __shfl(node, b, SIMLOD_WAVE), nch = ceil_chunks(__shfl(ns, b, SIMLOD_WAVE)), f = first[nd];
				for (uint32_t k = 0; k < nch && !found; k++) {
					const QItem it = items[f + k];
					const SimlodPoint* s = reinterpret_cast<const SimlodPoint*>(it.src);
					for (uint32_t j0 = 0; j0 < it.count && !found; j0 += SIMLOD_WAVE) {
						const uint32_t j = j0 + lane;
						bool pass = false;
						if (j < it.count) { const SimlodPoint v = s[j]; pass = Q::passes(q, (double)v.x, (double)v.y, (double)v.z); }
						found = __ballot(pass) != 0ull;
					}
				}
			}
		}
	};

	wave_descend(x, numListed, sh_fc[w], sh_mk[w], lane, [&](const SimlodExportNode& e) { return Q::probe(q, p, e); }, on_pairs);
	if (FILL) return;
#pragma unroll
	for (int o = SIMLOD_WAVE / 2; o > 0; o >>= 1) {
		nPairs += __shfl_xor(nPairs, o, SIMLOD_WAVE);
		nParts += __shfl_xor(nParts, o, SIMLOD_WAVE);
		nCand += __shfl_xor(nCand, o, SIMLOD_WAVE);
	}
	if (lane == 0u) {
		qParts[qi] = nParts;
		if (nPairs != 0u) { atomicAdd((unsigned long long*)&ph->numPairs, (unsigned long long)nPairs); atomicAdd((unsigned long long*)&ph->numCand, (unsigned long long)nCand); }
		if constexpr (Q::COUNT_TESTS_SAMPLES) {
			if (found) atomicAdd(&ph->numHits, 1u);
		}
	}
}

// what k_p_scan hands to Q::write_counts
struct PairTotals { uint32_t numNodes, error, numHits, numInvalid; uint64_t numPairs, numCandidates; };

template <class Q>
__global__ __launch_bounds__(WG_TPB) void k_p_scan(typename Q::Args a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const PairArgs& p = a.p;
	const ExportArgs& x = p.x;
	Header* hdr = reinterpret_cast<Header*>(x.scratch);
	PairHeader* ph = reinterpret_cast<PairHeader*>(x.scratch + 256u);
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + p.at.cnt);
	uint64_t* nfirst = reinterpret_cast<uint64_t*>(x.scratch + p.at.nfirst);
	const uint32_t* qParts = reinterpret_cast<const uint32_t*>(x.scratch + p.at.qParts);
	uint64_t* qFirst = reinterpret_cast<uint64_t*>(x.scratch + p.at.qFirst);
	const uint32_t n = hdr->numListed;
	uint32_t err = hdr->error;
	uint64_t pairs = 0, parts = 0;
	if (err == 0u) {
		for (uint32_t base = 0; base < n; base += WG_TPB) {
			const uint32_t t = base + threadIdx.x;
			uint64_t tot;
			const uint64_t off = block_scan<uint64_t>(t < n ? cnt[t] : 0u, tot, sh_scan);
			if (t < n) nfirst[t] = pairs + off;
			pairs += tot;
		}
		// four queries per lane and turn
		for (uint32_t base = 0; base < p.numQueries; base += 4u * WG_TPB) {
			const uint32_t i = base + 4u * threadIdx.x;
			uint32_t v[4];
#pragma unroll
			for (uint32_t j = 0; j < 4u; j++) v[j] = i + j < p.numQueries ? qParts[i + j] : 0u;
			uint64_t tot;
			uint64_t off = parts + block_scan<uint64_t>((uint64_t)v[0] + v[1] + v[2] + v[3], tot, sh_scan);
#pragma unroll
			for (uint32_t j = 0; j < 4u; j++) {
				if (i + j < p.numQueries) qFirst[i + j] = off;
				off += v[j];
			}
			parts += tot;
		}
	}
	if (threadIdx.x == 0) {
		nfirst[n] = pairs;
		qFirst[p.numQueries] = parts;
		const uint64_t numCand = ph->numCand;
		const uint64_t pairsOff = x.lay.items + hdr->totalChunks * sizeof(QItem);
		const bool results = Q::wants_results(a);
		if (results && err == 0u && pair_need(pairsOff, pairs, numCand, Q::part_bytes(a)) > p.scratchBytes) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		hdr->error = err;
		ph->numPairs = pairs; ph->numParts = parts;
		ph->pairsOff = pairsOff; ph->partsOff = pairsOff + pairs * sizeof(Pair);
		ph->doResults = results && err == 0u ? 1u : 0u;
		Q::write_counts(a, PairTotals{n, err, ph->numHits, ph->numInvalid, pairs, numCand});
	}
}

// The test kernels, per chunk item: the lane's four samples k = lane + 256 j of the chunk widened to fp64 (the places behind it.count hold zeros).
__device__ __forceinline__ void test_chunk(const QItem& it, double (&sx)[4], double (&sy)[4], double (&sz)[4]) {
	u32x4 v[4];
	load_chunk4<false, true>(reinterpret_cast<const u32x4*>(it.src), it.count, v);
#pragma unroll
	for (int j = 0; j < 4; j++) { sx[j] = (double)__uint_as_float(v[j].x); sy[j] = (double)__uint_as_float(v[j].y); sz[j] = (double)__uint_as_float(v[j].z); }
}
