// export_region.inc — part of export.hip: region queries.  QueryGeom, classify, QItem, QueryLayout, QueryArgs, query_totals, k_q_hier, k_q_dir,
// passes, q_count, k_q_count, k_q_scan, q_write, k_q_write.
// ---- region query ---------------------------------------------------------------------------------------------------------------------
// simlod_query_region (simlod_hip.h, "region queries"): five launches on the caller's stream.
//   k_q_hier   ONE workgroup: k_x_hier's walk with the classification (children outside the region are not listed; every listed entry gets its
//              class), then the scan of the chunks per node (-> the node's first item) and the totals before the test.
//   k_q_dir    one wave per table entry: k_x_dir's chunk addresses as items {source, count, node, chunk ordinal, class}; the chunk table's
//              slots are looked up by a lane each.
//   k_q_count  the filtered items: one chunk per workgroup and turn, the four 16-byte loads of a lane in flight before the test, ballots ->
//              one plain store of the item's count.  Leaves at once when no node is filtered.
//   k_q_scan   ONE workgroup: per filtered node the exclusive scan of its items' counts (-> each item's offset in the node), numSamples,
//              firstSample, the capacity check, SimlodQueryCounts.
//   k_q_write  copied items through copy_chunk (k_copy's body); filtered items read again, tested again and compacted IN ORDER: sample
//              k = lane + 256 j of the chunk belongs to segment (j, wave); the 16 segment counts go through LDS, inside a segment the ballot's
//              bits below the lane give the rank.  16-byte stores.

// ---- region queries: the classification of a node against the region (simlod_hip.h, "region queries", rules 1 and 4) ----------------------
// fp64 from the fp32 inputs, every sum in the order the header states (the library is built with -ffp-contract=off: no fused multiply-add),
// so that the numpy mirror (simlod_amd/octree_io.py OctreeExport.crop) reproduces every decision bit for bit.
struct QueryGeom {
	double   min[3], size;
	uint32_t numPlanes, pad;
	double   pl[SIMLOD_REGION_MAX_PLANES][4];
};

__device__ __forceinline__ uint32_t classify(const QueryGeom& g, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	const double s = ldexp(g.size, -(int)level), e = ldexp(g.size, -SIMLOD_MAX_DEPTH);       // (exact: powers of two)
	const uint32_t A[3] = {X, Y, Z};
	double lo[3], hi[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		lo[k] = (g.min[k] + (double)A[k] * s) - e;
		hi[k] = (g.min[k] + ((double)A[k] + 1.0) * s) + e;
	}
	bool inside = true;
	for (uint32_t p = 0; p < g.numPlanes; p++) {
		const double nx = g.pl[p][0], ny = g.pl[p][1], nz = g.pl[p][2], d = g.pl[p][3];
		const double dmax = ((nx * (nx >= 0.0 ? hi[0] : lo[0]) + ny * (ny >= 0.0 ? hi[1] : lo[1])) + nz * (nz >= 0.0 ? hi[2] : lo[2])) + d;
		if (dmax < 0.0) return Q_OUTSIDE;
		const double dmin = ((nx * (nx >= 0.0 ? lo[0] : hi[0]) + ny * (ny >= 0.0 ? lo[1] : hi[1])) + nz * (nz >= 0.0 ? lo[2] : hi[2])) + d;
		inside = inside && dmin >= 0.0;
	}
	return inside ? Q_COPIED : Q_FILTERED;
}

struct QItem { uint64_t src; uint32_t count, node, k, tag, pass, off; };          // 32 B, in the place of the export's CopyItems
static_assert(sizeof(QItem) == 32, "QItem");
// scratch: Layout's header | map | par | first, then cls u32[cap] (the class of each table entry), then the items up to the buffer's end
struct QueryLayout {
	Layout   x;                         // map / par / first / items; itemCap and bytes once the buffer is known (take_rest)
	uint64_t cls;
	__host__ __device__ explicit QueryLayout(uint32_t cap) {
		const uint64_t q = align256(4ull * cap);
		x.map = 256u; x.par = x.map + q; x.first = x.par + q; cls = x.first + align256(4ull * cap + 4u); x.items = cls + q;
	}
};

struct QueryArgs {
	ExportArgs         x;               // (x.counts unused; x.lay: map / par / first / items / itemCap as the query lays them out)
	QueryGeom          g;
	uint64_t           cls;             // offset of cls[] in the scratch buffer
	SimlodQueryCounts* counts;
};

// The scans behind a query's walk (ONE workgroup; k_q_hier, k_f_hier): the chunks per node (-> the node's first item) and the totals before the
// test.  `sh_scan`: WG_WAVES words.
__device__ __forceinline__ void query_totals(const ExportArgs& a, const uint32_t* cls, uint64_t* sh_scan) {
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(a.scratch + a.lay.first);
	const uint32_t n = hdr->numListed;
	// (not scan_table: the samples are only totalled here — firstSample is k_q_scan's, after the test — and the chunks share their scan with
	// the two node counts, so a turn has two scans; scan_table's two and a third for the counts would be a turn of another kernel)
	uint64_t cand = 0, items = 0, nFiltered = 0, nCopied = 0;
	for (uint32_t base = 0; base < n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		const uint64_t ns = t < n ? a.table[t].numSamples : 0u;
		const uint32_t c = t < n ? cls[t] : Q_OUTSIDE;
		// one scan for the three small counts, unpacked turn by turn: chunks in bits 0-39, filtered nodes (<= 1 024 a turn) in bits 40-51,
		// copied nodes from bit 52
		const uint64_t packed = (uint64_t)ceil_chunks(ns) | (ns != 0u && c == Q_FILTERED ? 1ull << 40 : 0ull) | (ns != 0u && c == Q_COPIED ? 1ull << 52 : 0ull);
		uint64_t totS, totP;
		block_scan<uint64_t>(ns, totS, sh_scan);
		const uint64_t offI = block_scan<uint64_t>(packed, totP, sh_scan) & 0xffffffffffull;
		if (t < n) first[t] = (uint32_t)(items + offI);
		cand += totS; items += totP & 0xffffffffffull; nFiltered += (totP >> 40) & 0xfffull; nCopied += totP >> 52;
	}
	if (threadIdx.x == 0) {
		uint32_t err = hdr->error;
		if (items > a.lay.itemCap) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		first[n] = (uint32_t)items;
		hdr->error = err;
		hdr->totalChunks = (err & SIMLOD_EXPORT_ERR_CAPACITY) ? 0u : items;      // the items k_q_dir writes
		hdr->counts[0] = (uint32_t)nFiltered; hdr->counts[1] = (uint32_t)nCopied;
		hdr->counts[2] = (uint32_t)cand; hdr->counts[3] = (uint32_t)(cand >> 32);
	}
}

__global__ __launch_bounds__(WG_TPB) void k_q_hier(QueryArgs q) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const ExportArgs& a = q.x;
	uint32_t* cls = reinterpret_cast<uint32_t*>(a.scratch + q.cls);
	hier_walk<true>(a, [&](uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) { return classify(q.g, level, X, Y, Z); }, cls);
	__syncthreads();
	query_totals(a, cls, sh_scan);
}

// One WAVE per table entry: while the builder's table is valid lane k looks chunk k up (a row holds at most 50, LEAF_ROW_SLOTS), all at once;
// what the rows do not give (a dropped table, the chunks behind a row's last slot) lane 0 follows by `next`, as k_x_dir does.
__global__ __launch_bounds__(LANE_TPB) void k_q_dir(QueryArgs q) {
	const ExportArgs& a = q.x;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	const uint32_t* map = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.map);
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.first);
	const uint32_t* cls = reinterpret_cast<const uint32_t*>(a.scratch + q.cls);
	QItem* items = reinterpret_cast<QItem*>(a.scratch + a.lay.items);
	const uint32_t t = blockIdx.x * (LANE_TPB / SIMLOD_WAVE) + threadIdx.x / SIMLOD_WAVE;
	const uint32_t lane = (uint32_t)lane_id();
	if (t >= hdr->numListed || hdr->totalChunks == 0u) return;             // (everything up to the lookups is the same for the whole wave)
	const SimlodExportNode& e = a.table[t];
	const uint32_t ns = e.numSamples;
	if (ns == 0u) return;
	const uint32_t src = map[t], tag = cls[t];
	const SimlodNode* n = a.nodes + src;
	const bool leaf = (e.flags & SIMLOD_EXPORT_FLAG_LEAF) != 0u;
	const SimlodChunk* head = leaf ? n->points : n->voxelChunks;
	const bool rows = leaf_rows_valid(a, src, head, leaf);
	const uint32_t nch = ceil_chunks(ns), f = first[t];
	auto put = [&](uint32_t k, const SimlodChunk* c) {
		QItem it;
		it.src = reinterpret_cast<uint64_t>(c->points);
		it.count = min(ns - k * SIMLOD_POINTS_PER_CHUNK, SIMLOD_POINTS_PER_CHUNK);
		it.node = t; it.k = k; it.tag = tag; it.pass = it.count; it.off = 0u;
		items[f + k] = it;
	};
	uint32_t good = 0;                       // chunks the rows gave: 0 .. good - 1
	bool shortList = false;
	if (rows) {
		const uint32_t kr = min(min(nch, a.ltSlots), (uint32_t)SIMLOD_WAVE);
		const SimlodChunk* c = lane == 0u ? head : lane < kr ? leaf_row_get(a.lt, a.ltPers, src, lane) : nullptr;
		const uint64_t missing = __ballot(lane < kr && c == nullptr);
		good = missing != 0ull ? (uint32_t)__ffsll((long long)missing) - 1u : kr;
		if (lane < good) put(lane, c);
		shortList = good < kr;
	}
	if (lane != 0u) return;
	uint32_t k = good;
	const SimlodChunk* c = good == 0u ? nullptr : good == 1u ? head : leaf_row_get(a.lt, a.ltPers, src, good - 1u);   // the chunk in front of chunk k
	for (; k < nch && !shortList; k++) {
		c = k == 0u ? head : c->next;
		if (c == nullptr) { shortList = true; break; }
		put(k, c);
	}
	if (shortList) {
		atomicOr(&hdr->error, SIMLOD_EXPORT_ERR_SHORT_LIST);
		for (; k < nch; k++) items[f + k] = QItem{0, 0, t, k, Q_OUTSIDE, 0, 0};
	}
}
static_assert(LEAF_ROW_SLOTS <= SIMLOD_WAVE, "k_q_dir: a row's slots fit one wave");

// rule 3: ((nx*x + ny*y) + nz*z) + d >= 0 for every plane, the fp32 coordinates widened to fp64 (a NaN fails)
__device__ __forceinline__ bool passes(const QueryGeom& g, const u32x4& v) {
	const double x = (double)__uint_as_float(v.x), y = (double)__uint_as_float(v.y), z = (double)__uint_as_float(v.z);
	bool ok = true;
	for (uint32_t p = 0; p < g.numPlanes; p++) ok = ok && ((g.pl[p][0] * x + g.pl[p][1] * y) + g.pl[p][2] * z) + g.pl[p][3] >= 0.0;
	return ok;
}

// The bodies of k_q_count and k_q_write take their kernel's argument block WHOLE, as `Args` says — `const QueryArgs&`, `const QueryArgs` or
// `const FootArgs&`, whichever leaves the kernel as it was (DESIGN §11: q_write by value keeps k_q_write's code, q_count by reference keeps
// k_q_count's registers; a member of a larger block handed on by value would be copied, and the planes' dynamic index puts such a copy into
// scratch memory).  query_of(args): the QueryArgs in it.
__device__ __forceinline__ const QueryArgs& query_of(const QueryArgs& q) { return q; }
// (the plane-only query: no footprint to ask — k_f_count / k_f_write, export_footprint.inc, bring theirs)
struct NoFootprint { __device__ __forceinline__ bool operator()(const u32x4&) const { return true; } };

// k_q_count's body; extra(v): what a sample has to pass on top of the planes (rule F1 of a footprint query).  INVERT (the inverse selections,
// export_inverse.inc; here and in q_write, e_paint and s_partial): a sample is taken iff it FAILS the planes' and extra's test, rule I1 — a
// compile-time choice between two expressions, so that the instances without it are the code they were.
template <typename Args, bool INVERT = false, typename Extra>
__device__ __forceinline__ void q_count(Args args, Extra extra) {
	const QueryArgs& q = query_of(args);
	__shared__ uint32_t sh_cnt[2][LANE_TPB / SIMLOD_WAVE];
	const Header* hdr = reinterpret_cast<const Header*>(q.x.scratch);
	if (hdr->counts[0] == 0u) return;                                      // no filtered node
	QItem* items = reinterpret_cast<QItem*>(q.x.scratch + q.x.lay.items);
	const uint64_t numItems = hdr->totalChunks;
	const int lane = lane_id(), w = (int)(threadIdx.x / SIMLOD_WAVE);
	uint32_t turn = 0;
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		if (items[i].tag != Q_FILTERED) continue;                          // (the same for the whole workgroup)
		const u32x4* s = reinterpret_cast<const u32x4*>(items[i].src);
		const uint32_t cnt = items[i].count;
		u32x4 v[4];
		load_chunk4<false, true>(s, cnt, v);
		uint32_t c = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			if (INVERT) c += (uint32_t)__popcll(__ballot(k < cnt && !(passes(q.g, v[j]) && extra(v[j]))));
			else c += (uint32_t)__popcll(__ballot(k < cnt && passes(q.g, v[j]) && extra(v[j])));
		}
		if (lane == 0) sh_cnt[turn][w] = c;
		__syncthreads();                    // (two buffers: the next turn's writes cannot overtake this turn's read)
		if (threadIdx.x == 0) items[i].pass = sh_cnt[turn][0] + sh_cnt[turn][1] + sh_cnt[turn][2] + sh_cnt[turn][3];
		turn ^= 1u;
	}
}
__global__ __launch_bounds__(LANE_TPB) void k_q_count(QueryArgs q) { q_count<const QueryArgs&>(q, NoFootprint()); }
static_assert(LANE_TPB / SIMLOD_WAVE == 4, "k_q_count / k_q_write: four waves");

__global__ __launch_bounds__(WG_TPB) void k_q_scan(QueryArgs q) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const ExportArgs& a = q.x;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.first);
	const uint32_t* cls = reinterpret_cast<const uint32_t*>(a.scratch + q.cls);
	QItem* items = reinterpret_cast<QItem*>(a.scratch + a.lay.items);
	const uint32_t n = hdr->numListed;
	const uint64_t numItems = hdr->totalChunks;
	uint64_t samples = 0;
	for (uint32_t base = 0; base < n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		uint64_t ns = t < n ? a.table[t].numSamples : 0u;
		if (t < n && ns != 0u && cls[t] == Q_FILTERED && numItems != 0u) {
			// eight counts in flight per turn: a lane walks its node's items alone, and a leaf has up to fifty
			uint32_t run = 0;
			const uint32_t f1 = first[t + 1u];
			for (uint32_t i = first[t]; i < f1; i += 8u) {
				uint32_t pass[8];
#pragma unroll
				for (uint32_t j = 0; j < 8u; j++) pass[j] = i + j < f1 ? items[i + j].pass : 0u;
#pragma unroll
				for (uint32_t j = 0; j < 8u; j++) {
					if (i + j < f1) items[i + j].off = run;
					run += pass[j];
				}
			}
			ns = run;
		}
		uint64_t totS;
		const uint64_t offS = block_scan<uint64_t>(ns, totS, sh_scan);
		if (t < n) { a.table[t].numSamples = (uint32_t)ns; a.table[t].firstSample = samples + offS; }
		samples += totS;
	}
	if (threadIdx.x == 0) {
		uint32_t err = hdr->error;
		if (a.samples != nullptr && samples > a.sampleCap) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		hdr->numItems = (a.samples == nullptr || (err & SIMLOD_EXPORT_ERR_CAPACITY)) ? 0u : numItems;   // count only / too small: nothing is written
		SimlodQueryCounts c;
		c.numNodes = n; c.error = err; c.numSamples = samples;
		c.numCandidates = (uint64_t)hdr->counts[2] | ((uint64_t)hdr->counts[3] << 32);
		c.numFilteredNodes = hdr->counts[0]; c.numCopiedNodes = hdr->counts[1];
		*q.counts = c;
	}
}

// k_q_write's body; extra(v) and INVERT as in q_count
template <typename Args, bool INVERT = false, typename Extra>
__device__ __forceinline__ void q_write(Args args, Extra extra) {
	const QueryArgs& q = query_of(args);
	__shared__ uint32_t sh_seg[2][16];
	const ExportArgs& a = q.x;
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const QItem* items = reinterpret_cast<const QItem*>(a.scratch + a.lay.items);
	const uint64_t numItems = hdr->numItems;
	const int lane = lane_id(), w = (int)(threadIdx.x / SIMLOD_WAVE);
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t turn = 0;
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const QItem it = items[i];
		if (it.count == 0u) continue;                                       // (the same for the whole workgroup, as every branch on `it`)
		const u32x4* s = reinterpret_cast<const u32x4*>(it.src);
		u32x4* d = reinterpret_cast<u32x4*>(a.samples + a.table[it.node].firstSample);
		if (it.tag == Q_COPIED) { copy_chunk(s, d + (uint64_t)it.k * SIMLOD_POINTS_PER_CHUNK, it.count); continue; }
		if (it.tag != Q_FILTERED || it.pass == 0u) continue;
		u32x4 v[4];
		load_chunk4<true, true>(s, it.count, v);
		uint64_t b[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			if (INVERT) b[j] = __ballot(k < it.count && !(passes(q.g, v[j]) && extra(v[j])));
			else b[j] = __ballot(k < it.count && passes(q.g, v[j]) && extra(v[j]));
			if (lane == 0) sh_seg[turn][j * 4 + w] = (uint32_t)__popcll(b[j]);
		}
		__syncthreads();                    // (two buffers, as in k_q_count)
		uint32_t before = it.off;           // samples of the node that pass before segment (j, w)
		d += before;
		uint32_t run = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) {
#pragma unroll
			for (int ww = 0; ww < 4; ww++) {
				if (ww == w && ((b[j] >> lane) & 1ull)) __builtin_nontemporal_store(v[j], d + run + (uint32_t)__popcll(b[j] & below));
				run += sh_seg[turn][j * 4 + ww];
			}
		}
		turn ^= 1u;
	}
}
__global__ __launch_bounds__(LANE_TPB) void k_q_write(QueryArgs q) { q_write<const QueryArgs>(q, NoFootprint()); }
