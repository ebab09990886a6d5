// export_rays.inc — part of export.hip: ray queries.  The ray records, RayLayout, RayArgs, k_r_hier, RayD, ray_load, slab, sample_t, hit_less,
// wave_hit_min, wave_descend, k_r_pairs, k_r_scan, k_r_test, k_r_reduce.
// ---- ray query ------------------------------------------------------------------------------------------------------------------------
// simlod_query_rays (simlod_hip.h, "ray queries"): seven launches on the caller's stream, four for a count-only call.
//   k_r_hier    ONE workgroup: k_x_hier's walk (the table is the export's, into the caller's array or into scratch), then k_x_scan's scans:
//               firstSample, the node's first chunk item, the item capacity.
//   k_q_dir     the region query's directory kernel as it is (every entry tagged as copied): one item per chunk of every selected node.
//   k_r_pairs   one WAVE per ray, the table descended depth first with a bucket of pending nodes per level: a turn takes up to eight nodes of
//               the deepest level that has any and tests their 64 children, one lane each (rule 3), so a bucket never holds more than 64.
//               <count>: rays per node (an atomic count: the sum is the same in any order), chunks per ray, numPairs, numCandidates, numInvalid;
//               in a count-only call also numHits, ray-major, stopping at a ray's first passing sample.
//               <fill>: the same descent writes each pair {ray, the ray's first partial for this node} into its node's range.
//   k_r_scan    ONE workgroup: rays per node -> each node's range of pairs; chunks per ray -> each ray's range of partials; the capacity
//               check; SimlodRayCounts.
//   k_r_test    the hot path, node-major: one chunk per workgroup and turn, its four samples per lane kept in registers as fp64, then the
//               rays paired with the chunk's node in tiles of 64 from LDS; per ray a ballot, a wave arg-min of (t, ordinal) only where a lane
//               passed, the four waves combined through LDS, one 16-byte partial per (chunk, ray).  A chunk is read once however many rays
//               reach its node.
//   k_r_reduce  one wave per ray: the arg-min of (t, node, ordinal) over the ray's partials, the hit record (or the miss) written once.
// The order in which pairs land in a node's range depends on the schedule; nothing that is returned does: the counts are sums, and the hit is
// the minimum of a total order.
constexpr uint32_t RAY_WAVES = LANE_TPB / SIMLOD_WAVE;                            // k_r_pairs / k_r_reduce: rays per workgroup
constexpr uint32_t RAY_LEVELS = SIMLOD_MAX_DEPTH;                                 // buckets: a node at level 20 has no children
constexpr uint32_t RAY_TILE = SIMLOD_WAVE;                                        // k_r_test: rays per LDS tile

struct RayHeader {                       // at byte 256 of the scratch buffer
	uint64_t numPairs, numCand, numParts, pairsOff, partsOff;
	uint32_t numInvalid, numHits, doHits, pad;
};
struct RayPair { uint64_t part; uint32_t ray, pad; };                             // 16 B: a ray paired with a node, and its first partial for that node
struct RayPart { double t; uint32_t node, ordinal; };                             // 16 B: the best sample of one (chunk, ray)
static_assert(sizeof(RayPair) == 16 && sizeof(RayPart) == 16 && sizeof(RayHeader) <= 256, "ray query records");

// scratch: Header | RayHeader | map | par | first | cls | tab (the table when the caller wants none) | cnt | fill | nfirst u64[cap + 1] |
// rayParts u32[numRays] | rayFirst u64[numRays + 1] | items QItem[chunks] | pairs RayPair[numPairs] | partials RayPart[<= numCandidates / 1000 + numPairs]
struct RayOffsets { uint64_t cls, cnt, fill, nfirst, rayParts, rayFirst; };       // what the ray kernels find beside the walk's arrays
struct RayLayout {
	Layout     x;                       // map / par / first / items; itemCap and bytes once the buffer is known (take_rest)
	uint64_t   tab;
	RayOffsets at;
	__host__ __device__ RayLayout(uint32_t cap, uint32_t numRays) {
		const uint64_t q = align256(4ull * cap);
		x.map = 512u; x.par = x.map + q; x.first = x.par + q; at.cls = x.first + align256(4ull * cap + 4u); tab = at.cls + q;
		at.cnt = tab + align256(sizeof(SimlodExportNode) * (uint64_t)cap); at.fill = at.cnt + q; at.nfirst = at.fill + q;
		at.rayParts = at.nfirst + align256(8ull * cap + 8u); at.rayFirst = at.rayParts + align256(4ull * numRays);
		x.items = at.rayFirst + align256(8ull * numRays + 8u);
	}
};

struct RayArgs {
	ExportArgs         x;                // (x.table: the caller's table or `tab`; x.lay: map / par / first / items / itemCap)
	double             min[3], size;
	const SimlodRay*   rays;
	uint32_t           numRays, pad;
	SimlodRayHit*      hits;
	SimlodRayCounts*   counts;
	uint64_t           scratchBytes;
	RayOffsets         at;
};

__global__ __launch_bounds__(WG_TPB) void k_r_hier(RayArgs a) {
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
		RayHeader rh{};
		*reinterpret_cast<RayHeader*>(x.scratch + 256u) = rh;
	}
}

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
__device__ __forceinline__ bool slab(const RayD& r, const RayArgs& a, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
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

// the total order of rule 4
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
// probe(entry): does the node pass (rule 3 of the ray query, rule 3 of the neighbour query); on_pairs(isPair per lane, table index, samples)
// once per turn for the selected entries with samples among those that passed.  Shared by k_r_pairs and k_n_pairs.
template <class Probe, class OnPairs>
__device__ __forceinline__ void wave_descend(const ExportArgs& x, uint32_t numListed, uint32_t (&fc)[RAY_LEVELS][SIMLOD_WAVE], uint8_t (&mk)[RAY_LEVELS][SIMLOD_WAVE],
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
		const bool push = pass && ce.childMask != 0u && cur + 1 < (int)RAY_LEVELS;
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

template <int FILL>
__global__ __launch_bounds__(LANE_TPB) void k_r_pairs(RayArgs a) {
	__shared__ uint32_t sh_fc[RAY_WAVES][RAY_LEVELS][SIMLOD_WAVE];                 // pending nodes per level: their firstChild ...
	__shared__ uint8_t  sh_mk[RAY_WAVES][RAY_LEVELS][SIMLOD_WAVE];                 // ... and childMask
	const ExportArgs& x = a.x;
	const Header* hdr = reinterpret_cast<const Header*>(x.scratch);
	RayHeader* rh = reinterpret_cast<RayHeader*>(x.scratch + 256u);
	const uint32_t w = threadIdx.x / SIMLOD_WAVE, lane = (uint32_t)lane_id();
	const uint32_t ray = blockIdx.x * RAY_WAVES + w;
	if (ray >= a.numRays || hdr->error != 0u || (FILL && rh->doHits == 0u)) return;     // (the same for the whole wave, as every exit below)
	const uint32_t numListed = hdr->numListed;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(x.scratch + x.lay.first);
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	uint32_t* cnt = reinterpret_cast<uint32_t*>(x.scratch + a.at.cnt);
	uint32_t* fill = reinterpret_cast<uint32_t*>(x.scratch + a.at.fill);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + a.at.nfirst);
	uint32_t* rayParts = reinterpret_cast<uint32_t*>(x.scratch + a.at.rayParts);
	const uint64_t* rayFirst = reinterpret_cast<const uint64_t*>(x.scratch + a.at.rayFirst);
	RayD r;
	const bool valid = ray_load(a.rays, ray, r);
	if (!valid) {
		if (!FILL && lane == 0u) { atomicAdd(&rh->numInvalid, 1u); rayParts[ray] = 0u; }
		return;
	}
	const bool countHits = !FILL && a.hits == nullptr;
	uint32_t nPairs = 0, nParts = 0;                                               // this lane's share (count)
	uint64_t nCand = 0;
	bool found = false;
	uint64_t run = FILL ? rayFirst[ray] : 0u;                                      // (fill) the ray's next free partial
	RayPair* pairs = reinterpret_cast<RayPair*>(x.scratch + rh->pairsOff);

	// what a turn does with its pairs: isPair per lane, `node` its table index, `ns` its samples
	auto on_pairs = [&](bool isPair, uint32_t node, uint32_t ns) {
		const uint64_t pm = __ballot(isPair);
		if (pm == 0ull) return;
		if (FILL) {
			const uint32_t nch = isPair ? ceil_chunks(ns) : 0u;
			const uint32_t incl = wave_incl_scan(nch);
			if (isPair) {
				const uint64_t slot = nfirst[node] + atomicAdd(&fill[node], 1u);
				RayPair p;
				p.part = run + (incl - nch); p.ray = ray; p.pad = 0u;
				pairs[slot] = p;
			}
			run += __shfl(incl, SIMLOD_WAVE - 1, SIMLOD_WAVE);
			return;
		}
		if (isPair) { atomicAdd(&cnt[node], 1u); nPairs++; nParts += ceil_chunks(ns); nCand += ns; }
		if (!countHits || found) return;
		// count only: is there any passing sample?  The wave takes the turn's pairs one after the other and leaves at the first.
		for (uint64_t m = pm; m != 0ull && !found; m &= m - 1ull) {
			const int b = __ffsll((long long)m) - 1;
			const uint32_t nd = __shfl(node, b, SIMLOD_WAVE), nch = ceil_chunks(__shfl(ns, b, SIMLOD_WAVE)), f = first[nd];
			for (uint32_t k = 0; k < nch && !found; k++) {
				const QItem it = items[f + k];
				const SimlodPoint* s = reinterpret_cast<const SimlodPoint*>(it.src);
				for (uint32_t j0 = 0; j0 < it.count && !found; j0 += SIMLOD_WAVE) {
					const uint32_t j = j0 + lane;
					bool pass = false;
					if (j < it.count) { const SimlodPoint v = s[j]; pass = sample_t(r, (double)v.x, (double)v.y, (double)v.z) >= 0.0; }
					found = __ballot(pass) != 0ull;
				}
			}
		}
	};

	wave_descend(x, numListed, sh_fc[w], sh_mk[w], lane, [&](const SimlodExportNode& e) { return slab(r, a, e.level, e.X, e.Y, e.Z); }, on_pairs);
	if (FILL) return;
#pragma unroll
	for (int o = SIMLOD_WAVE / 2; o > 0; o >>= 1) {
		nPairs += __shfl_xor(nPairs, o, SIMLOD_WAVE);
		nParts += __shfl_xor(nParts, o, SIMLOD_WAVE);
		nCand += __shfl_xor(nCand, o, SIMLOD_WAVE);
	}
	if (lane == 0u) {
		rayParts[ray] = nParts;
		if (nPairs != 0u) { atomicAdd((unsigned long long*)&rh->numPairs, (unsigned long long)nPairs); atomicAdd((unsigned long long*)&rh->numCand, (unsigned long long)nCand); }
		if (found) atomicAdd(&rh->numHits, 1u);
	}
}

__global__ __launch_bounds__(WG_TPB) void k_r_scan(RayArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const ExportArgs& x = a.x;
	Header* hdr = reinterpret_cast<Header*>(x.scratch);
	RayHeader* rh = reinterpret_cast<RayHeader*>(x.scratch + 256u);
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + a.at.cnt);
	uint64_t* nfirst = reinterpret_cast<uint64_t*>(x.scratch + a.at.nfirst);
	const uint32_t* rayParts = reinterpret_cast<const uint32_t*>(x.scratch + a.at.rayParts);
	uint64_t* rayFirst = reinterpret_cast<uint64_t*>(x.scratch + a.at.rayFirst);
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
		// four rays per lane and turn
		for (uint32_t base = 0; base < a.numRays; base += 4u * WG_TPB) {
			const uint32_t i = base + 4u * threadIdx.x;
			uint32_t v[4];
#pragma unroll
			for (uint32_t j = 0; j < 4u; j++) v[j] = i + j < a.numRays ? rayParts[i + j] : 0u;
			uint64_t tot;
			uint64_t off = parts + block_scan<uint64_t>((uint64_t)v[0] + v[1] + v[2] + v[3], tot, sh_scan);
#pragma unroll
			for (uint32_t j = 0; j < 4u; j++) {
				if (i + j < a.numRays) rayFirst[i + j] = off;
				off += v[j];
			}
			parts += tot;
		}
	}
	if (threadIdx.x == 0) {
		nfirst[n] = pairs;
		rayFirst[a.numRays] = parts;
		// what a call with hits needs behind the items: 32 bytes per pair (its record and one partial) and 16 per further thousand candidates
		const uint64_t numCand = rh->numCand;
		const uint64_t pairsOff = x.lay.items + hdr->totalChunks * sizeof(QItem);
		const uint64_t need = pairsOff + pairs * (sizeof(RayPair) + sizeof(RayPart)) + (numCand / SIMLOD_POINTS_PER_CHUNK) * sizeof(RayPart);
		if (a.hits != nullptr && err == 0u && need > a.scratchBytes) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		hdr->error = err;
		rh->numPairs = pairs; rh->numParts = parts;
		rh->pairsOff = pairsOff; rh->partsOff = pairsOff + pairs * sizeof(RayPair);
		rh->doHits = a.hits != nullptr && err == 0u ? 1u : 0u;
		SimlodRayCounts c;
		c.numNodes = n; c.error = err; c.numHits = rh->numHits; c.numInvalid = rh->numInvalid;
		c.numPairs = pairs; c.numCandidates = numCand;
		*a.counts = c;
	}
}

__global__ __launch_bounds__(LANE_TPB) void k_r_test(RayArgs a) {
	__shared__ double   sh_ray[11][RAY_TILE];                                      // o, d, dd, tMin, tMax, radius, spread of the tile's rays
	__shared__ uint64_t sh_part[RAY_TILE];
	__shared__ double   sh_t[RAY_WAVES][RAY_TILE];
	__shared__ uint32_t sh_o[RAY_WAVES][RAY_TILE];
	const ExportArgs& x = a.x;
	const Header* hdr = reinterpret_cast<const Header*>(x.scratch);
	const RayHeader* rh = reinterpret_cast<const RayHeader*>(x.scratch + 256u);
	if (rh->doHits == 0u || rh->numPairs == 0u) return;
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + a.at.cnt);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + a.at.nfirst);
	const RayPair* pairs = reinterpret_cast<const RayPair*>(x.scratch + rh->pairsOff);
	RayPart* parts = reinterpret_cast<RayPart*>(x.scratch + rh->partsOff);
	const uint64_t numItems = hdr->totalChunks;
	const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x / SIMLOD_WAVE;
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
		for (uint32_t j0 = 0; j0 < c; j0 += RAY_TILE) {
			const uint32_t nt = min(RAY_TILE, c - j0);
			__syncthreads();                                                       // (the tile before is done with)
			if (threadIdx.x < nt) {
				const RayPair p = pairs[pf + j0 + threadIdx.x];
				RayD r;
				ray_load(a.rays, p.ray, r);                                        // (valid: it formed a pair)
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
				for (uint32_t ww = 1; ww < RAY_WAVES; ww++) {
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
static_assert(RAY_TILE <= LANE_TPB && RAY_WAVES == 4, "k_r_test: a lane per ray of the tile, four waves");

__global__ __launch_bounds__(LANE_TPB) void k_r_reduce(RayArgs a) {
	const ExportArgs& x = a.x;
	const RayHeader* rh = reinterpret_cast<const RayHeader*>(x.scratch + 256u);
	const uint32_t w = threadIdx.x / SIMLOD_WAVE, lane = (uint32_t)lane_id();
	const uint32_t ray = blockIdx.x * RAY_WAVES + w;
	if (ray >= a.numRays || rh->doHits == 0u) return;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(x.scratch + x.lay.first);
	const QItem* items = reinterpret_cast<const QItem*>(x.scratch + x.lay.items);
	const uint64_t* rayFirst = reinterpret_cast<const uint64_t*>(x.scratch + a.at.rayFirst);
	const RayPart* parts = reinterpret_cast<const RayPart*>(x.scratch + rh->partsOff);
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
