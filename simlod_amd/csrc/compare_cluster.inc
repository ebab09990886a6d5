// compare_cluster.inc — cluster queries (include/simlod_hip.h, "cluster queries"; rules K3, K7-K9 and the union-find in cluster_rules.hpp),
// included by compare.hip inside its anonymous namespace: the kernels that follow the compare queries' grid build (k_c_init .. k_c_decide,
// launched as they are by launch_grid with b = a) when the call is simlod_cluster_samples.  Every dependency between them is a kernel
// boundary; every one returns at once unless `run` (rules C6, C7).
//   k_k_core     one lane per sample (grid-stride): the 27 lookups, rule C2's test over each cell's records -> within[i]; parent[i] = i,
//                size[i] = 0, attach[i] = MISS.
//   k_k_link     the hot path.  One lane per valid sample, over its neighbourhood once.  A core unites itself with every core j < i that
//                passes rule C2 — each link taken once, from its higher end; within[j] is k_k_core's, a plain load — and carries the root it
//                reached on to the next neighbour, so that in a crowded cell a pair costs two loads and a compare.  A sample that is no core
//                keeps the minimum (d2, j) over the cores that pass (rule K5) as attach[i].  EVERY access to `parent` in this launch is an
//                agent-scope relaxed atomic (AgentParent), as k_c_insert reads its keys: a plain load may be served from this CU's L1 or
//                from a stale line of this XCD's L2 and never see another workgroup's link.  No lane waits for another; cluster_rules.hpp
//                has the argument for termination and for the root, and the bound of every loop.
//   k_k_sizes    root[i] = the root above i (core) or above attach[i] (border), MISS otherwise, into attach's word; `parent` is final by
//                now, so plain loads; integer atomic adds on size[root], ONE per wave and run of equal roots (ballot, popcount): a giant
//                component does not send an add per sample to one word.
//   k_k_roots    each workgroup takes ONE contiguous span of indices and counts the roots in it whose cluster is kept, and the others.
//   k_k_ids      each workgroup adds up the counts of the spans before its own and scans its span, 256 indices a turn: the kept roots'
//                numbers in ascending order of root (rule K8).  sizeHist in LDS, the largest cluster as one 64-bit maximum.  No look-back:
//                nothing here waits for another workgroup.
//   k_k_write    one lane per sample: the record (one 16-byte store), the colour, and the counts of rule K9 kept in registers.
//   k_k_final    ONE workgroup: the partial records added up into the summary.
// The only global atomics are the compare-and-swap on `parent` and the add on `size`; the summary's fields are plain stores into one
// partial record per workgroup (ClusPart, each kernel its own fields).

struct ClusPart {                      // one per workgroup; each kernel writes its own fields
	uint64_t error;                    // k_k_link, k_k_sizes: a loop reached its bound
	uint64_t kept, dissolved;          // k_k_roots
	uint64_t largest;                  // k_k_ids: cluster_largest_key
	uint64_t core, border, noise, within;   // k_k_write
	uint32_t hist[36];                 // k_k_ids: CLUSTER_SIZE_BINS rounded up to whole 16 bytes
};
static_assert(sizeof(ClusPart) == 208 && CLUSTER_SIZE_BINS <= 36u, "cluster scratch records");

// the scratch buffer behind the compare layout of (numA, numA): offsets in bytes, each a multiple of 16
struct ClusLayout {
	uint64_t within, parent, attach, size, id, parts, bytes;
	explicit ClusLayout(uint64_t numA) {
		const uint64_t words = (numA * sizeof(uint32_t) + 15u) / 16u * 16u;
		within = CmpLayout(numA).bytes;
		parent = within + words;
		attach = parent + words;
		size = attach + words;
		id = size + words;
		parts = id + words;
		bytes = parts + (uint64_t)CMP_MAX_PARTS * sizeof(ClusPart);
	}
};

struct ClusArgs {
	CmpArgs  c;
	uint64_t within, parent, attach, size, id, parts;
	uint64_t span;                     // k_k_roots, k_k_ids: indices per workgroup, a multiple of CMP_TPB
	uint32_t minNeighbours, minClusterSize;
	SimlodClusterRecord* records;
};
struct ClusWriteArgs {
	ClusArgs k;
	uint32_t table[256];
};
static_assert(sizeof(ClusWriteArgs) <= 4096, "k_k_write: the kernel arguments");

__device__ __forceinline__ uint32_t* words_of(const ClusArgs& k, uint64_t at) { return reinterpret_cast<uint32_t*>(k.c.scratch + at); }
__device__ __forceinline__ ClusPart* kparts_of(const ClusArgs& k) { return reinterpret_cast<ClusPart*>(k.c.scratch + k.parts); }

// cluster_rules.hpp's memory policy while links are being made: agent-scope relaxed atomics
struct AgentParent {
	uint32_t* p;
	__device__ __forceinline__ uint32_t load(uint32_t i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	__device__ __forceinline__ uint32_t cas(uint32_t i, uint32_t expected, uint32_t desired) { return atomicCAS(p + i, expected, desired); }
};
// and once they are final (cluster_root only: it stores nothing)
struct FinalParent {
	const uint32_t* p;
	__device__ __forceinline__ uint32_t load(uint32_t i) { return p[i]; }
};

__global__ __launch_bounds__(CMP_TPB) void k_k_core(ClusArgs k) {
	const CmpArgs& c = k.c;
	if (header_of(c)->run == 0u) return;
	const CmpSlot* tab = table_of(c);
	const u32x4* cells = reinterpret_cast<const u32x4*>(c.scratch + c.cells);
	uint32_t* within = words_of(k, k.within);
	uint32_t* parent = words_of(k, k.parent);
	uint32_t* attach = words_of(k, k.attach);
	uint32_t* size = words_of(k, k.size);
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numA; i += (uint64_t)gridDim.x * CMP_TPB) {
		const u32x4 s = c.a[i];
		uint32_t w = 0u;
		if (compare_valid(s.x, s.y, s.z)) {
			uint32_t cell[3];
			cells_of(c, s, cell);
			const double cx = (double)__uint_as_float(s.x), cy = (double)__uint_as_float(s.y), cz = (double)__uint_as_float(s.z);
			for_neighbour_cells(c, tab, cell, [&](uint32_t start, uint32_t count) {
				const uint64_t end = (uint64_t)start + count;                   // (at most numA: k_c_fill's argument)
				for (uint64_t j = start; j < end; j++) {
					const u32x4 v = cells[j];
					if (compare_d2((double)__uint_as_float(v.x), (double)__uint_as_float(v.y), (double)__uint_as_float(v.z), cx, cy, cz) <= c.rr) w++;
				}
			});
		}
		within[i] = w;
		parent[i] = (uint32_t)i;
		size[i] = 0u;
		attach[i] = CLUSTER_MISS;
	}
}

__global__ __launch_bounds__(CMP_TPB) void k_k_link(ClusArgs k) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = k.c;
	if (header_of(c)->run == 0u) return;
	const CmpSlot* tab = table_of(c);
	const u32x4* cells = reinterpret_cast<const u32x4*>(c.scratch + c.cells);
	const uint32_t* within = words_of(k, k.within);
	uint32_t* attach = words_of(k, k.attach);
	AgentParent m{words_of(k, k.parent)};
	const uint64_t budget = cluster_link_budget(c.numA);
	uint64_t error = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numA; i += (uint64_t)gridDim.x * CMP_TPB) {
		const u32x4 s = c.a[i];
		if (!compare_valid(s.x, s.y, s.z)) continue;
		uint32_t cell[3];
		cells_of(c, s, cell);
		const double cx = (double)__uint_as_float(s.x), cy = (double)__uint_as_float(s.y), cz = (double)__uint_as_float(s.z);
		if (cluster_is_core(within[i], k.minNeighbours)) {                      // rule K4: every link from its higher end
			uint32_t at = (uint32_t)i;                                          // i, or the last root found above it
			for_neighbour_cells(c, tab, cell, [&](uint32_t start, uint32_t count) {
				const uint64_t end = (uint64_t)start + count;
				for (uint64_t j = start; j < end; j++) {
					const u32x4 v = cells[j];
					if (v.w >= (uint32_t)i || at == CLUSTER_MISS) continue;
					if (!(compare_d2((double)__uint_as_float(v.x), (double)__uint_as_float(v.y), (double)__uint_as_float(v.z), cx, cy, cz) <= c.rr)) continue;
					if (!cluster_is_core(within[v.w], k.minNeighbours)) continue;
					at = cluster_link(m, at, v.w, budget);
				}
			});
			if (at == CLUSTER_MISS) error = 1u;
		} else {                                                                // rule K5: the first core in (d2, index)
			double best = __longlong_as_double((long long)COMPARE_MISS_D2_BITS);
			uint32_t to = CLUSTER_MISS;
			for_neighbour_cells(c, tab, cell, [&](uint32_t start, uint32_t count) {
				const uint64_t end = (uint64_t)start + count;
				for (uint64_t j = start; j < end; j++) {
					const u32x4 v = cells[j];
					const double d2 = compare_d2((double)__uint_as_float(v.x), (double)__uint_as_float(v.y), (double)__uint_as_float(v.z), cx, cy, cz);
					if (d2 <= c.rr && (d2 < best || (d2 == best && v.w < to)) && cluster_is_core(within[v.w], k.minNeighbours)) { best = d2; to = v.w; }
				}
			});
			attach[i] = to;
		}
	}
	error = block_reduce<true>(error, sh);
	if (threadIdx.x == 0u) kparts_of(k)[blockIdx.x].error = error;
}

__global__ __launch_bounds__(CMP_TPB) void k_k_sizes(ClusArgs k) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = k.c;
	if (header_of(c)->run == 0u) return;
	const uint32_t* within = words_of(k, k.within);
	uint32_t* root = words_of(k, k.attach);                                    // (lane i reads attach[i] and then writes root[i]: the same word)
	uint32_t* size = words_of(k, k.size);
	FinalParent m{words_of(k, k.parent)};
	const int lane = lane_id();
	uint64_t error = 0u;
	uint32_t pendRoot = CLUSTER_MISS, pendCount = 0u;                           // the wave's add not made yet (the same in every lane)
	// (the bound is the same for the whole workgroup: every lane of a wave reaches the ballots)
	for (uint64_t base = (uint64_t)blockIdx.x * CMP_TPB; base < c.numA; base += (uint64_t)gridDim.x * CMP_TPB) {
		const uint64_t i = base + threadIdx.x;
		uint32_t r = CLUSTER_MISS;
		if (i < c.numA) {
			const u32x4 s = c.a[i];
			if (compare_valid(s.x, s.y, s.z)) {
				const uint32_t from = cluster_is_core(within[i], k.minNeighbours) ? (uint32_t)i : root[i];
				if (from != CLUSTER_MISS) {
					uint64_t budget = c.numA;
					r = cluster_root(m, from, budget);
					if (r == CLUSTER_MISS) error = 1u;
				}
			}
			root[i] = r;
		}
		// ONE add per wave and distinct root, and none while the root stays what it was a turn ago: a component of millions of samples would
		// otherwise send millions of adds to one word (measured: 408 ms of a 530 ms call on 36 M samples, DESIGN §11).  Integer sums: any
		// grouping gives the same size.  At most one turn per lane.
		unsigned long long left = __ballot(r != CLUSTER_MISS);
		for (uint32_t turn = 0; turn < SIMLOD_WAVE && left != 0ull; turn++) {
			const uint32_t r0 = (uint32_t)__shfl((int)r, __ffsll(left) - 1, SIMLOD_WAVE);
			const unsigned long long same = __ballot(r == r0);                  // (r0 is a root: every such lane is in `left`)
			const uint32_t n = (uint32_t)__popcll(same);
			if (r0 == pendRoot) {
				pendCount += n;
			} else {
				if (pendCount != 0u && lane == 0) atomicAdd(&size[pendRoot], pendCount);   // (pendRoot < numA: an index `parent` held)
				pendRoot = r0;
				pendCount = n;
			}
			left &= ~same;
		}
	}
	if (pendCount != 0u && lane == 0) atomicAdd(&size[pendRoot], pendCount);
	error = block_reduce<true>(error, sh);
	if (threadIdx.x == 0u && error != 0u) kparts_of(k)[blockIdx.x].error = error;   // (k_k_link's grid: its word exists and is written)
}

// i is the root of a cluster (the cluster's lowest core: its own root), and whether that cluster is kept (rule K7)
__device__ __forceinline__ bool is_root(const uint32_t* root, uint64_t i) { return root[i] == (uint32_t)i; }

__global__ __launch_bounds__(CMP_TPB) void k_k_roots(ClusArgs k) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = k.c;
	if (header_of(c)->run == 0u) return;
	const uint32_t* root = words_of(k, k.attach);
	const uint32_t* size = words_of(k, k.size);
	const uint64_t first = (uint64_t)blockIdx.x * k.span, end = std::min<uint64_t>(first + k.span, c.numA);
	uint64_t kept = 0u, dissolved = 0u;
	for (uint64_t i = first + threadIdx.x; i < end; i += CMP_TPB) {
		if (!is_root(root, i)) continue;
		if (cluster_is_kept(size[i], k.minClusterSize)) kept++; else dissolved++;
	}
	kept = block_reduce<false>(kept, sh);
	dissolved = block_reduce<false>(dissolved, sh);
	if (threadIdx.x == 0u) { ClusPart* part = kparts_of(k) + blockIdx.x; part->kept = kept; part->dissolved = dissolved; }
}

__global__ __launch_bounds__(CMP_TPB) void k_k_ids(ClusArgs k) {
	__shared__ uint64_t sh[CMP_WAVES];
	__shared__ uint32_t sh_wave[CMP_WAVES];
	__shared__ uint32_t sh_hist[36];
	const CmpArgs& c = k.c;
	if (header_of(c)->run == 0u) return;
	const uint32_t* root = words_of(k, k.attach);
	const uint32_t* size = words_of(k, k.size);
	uint32_t* id = words_of(k, k.id);
	const ClusPart* parts = kparts_of(k);
	const int lane = lane_id();
	const uint32_t w = threadIdx.x / SIMLOD_WAVE;
	if (threadIdx.x < 36u) sh_hist[threadIdx.x] = 0u;
	uint64_t before = 0u;
	for (uint32_t p = threadIdx.x; p < blockIdx.x; p += CMP_TPB) before += parts[p].kept;
	uint32_t base = (uint32_t)block_reduce<false>(before, sh);                  // (its barriers: sh_hist is zero for everyone)
	const uint64_t first = (uint64_t)blockIdx.x * k.span, end = std::min<uint64_t>(first + k.span, c.numA);
	uint64_t largest = 0u;
	// (the bounds are the same for the whole workgroup: every lane reaches the barriers)
	for (uint64_t at = first; at < end; at += CMP_TPB) {
		const uint64_t i = at + threadIdx.x;
		uint32_t sz = 0u;
		bool kept = false;
		if (i < end && is_root(root, i)) { sz = size[i]; kept = cluster_is_kept(sz, k.minClusterSize); }
		uint32_t incl = kept ? 1u : 0u;
#pragma unroll
		for (int o = 1; o < SIMLOD_WAVE; o <<= 1) {
			const uint32_t t = (uint32_t)__shfl_up((int)incl, o, SIMLOD_WAVE);
			if (lane >= o) incl += t;
		}
		if (lane == SIMLOD_WAVE - 1) sh_wave[w] = incl;
		__syncthreads();
		uint32_t mine = base + incl - 1u, total = 0u;
		for (uint32_t q = 0; q < CMP_WAVES; q++) { if (q < w) mine += sh_wave[q]; total += sh_wave[q]; }
		if (kept) {
			id[i] = mine;                                                      // rule K8
			atomicAdd(&sh_hist[cluster_size_bin(sz)], 1u);
			const uint64_t key = cluster_largest_key(sz, mine);
			largest = key > largest ? key : largest;
		}
		base += total;
		__syncthreads();                                                       // (sh_wave is written again)
	}
	largest = block_reduce<true>(largest, sh);                                  // (its barriers: the histogram's atomics are done as well)
	ClusPart* part = kparts_of(k) + blockIdx.x;
	if (threadIdx.x == 0u) part->largest = largest;
	if (threadIdx.x < 36u) part->hist[threadIdx.x] = sh_hist[threadIdx.x];
}

__global__ __launch_bounds__(CMP_TPB) void k_k_write(ClusWriteArgs t) {
	__shared__ uint32_t sh_table[256];
	__shared__ uint64_t sh[CMP_WAVES];
	const ClusArgs& k = t.k;
	const CmpArgs& c = k.c;
	if (header_of(c)->run == 0u) return;
	for (uint32_t i = threadIdx.x; i < 256u; i += CMP_TPB) sh_table[i] = t.table[i];
	__syncthreads();
	const uint32_t* within = words_of(k, k.within);
	const uint32_t* root = words_of(k, k.attach);
	const uint32_t* size = words_of(k, k.size);
	const uint32_t* id = words_of(k, k.id);
	uint64_t core = 0u, border = 0u, noise = 0u, withinSum = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * CMP_TPB + threadIdx.x; i < c.numA; i += (uint64_t)gridDim.x * CMP_TPB) {
		const uint32_t wi = within[i], r = root[i];
		uint32_t cluster = CLUSTER_NOISE, sz = 0u;
		if (r != CLUSTER_MISS) {
			sz = size[r];
			if (cluster_is_kept(sz, k.minClusterSize)) cluster = id[r];        // (r is a kept root: k_k_ids wrote its number)
		}
		*reinterpret_cast<u32x4*>(k.records + i) = u32x4{cluster, r, sz, wi};   // rule K9
		if (c.colors != nullptr) c.colors[i] = cluster != CLUSTER_NOISE ? sh_table[cluster_colour_index(cluster)] : c.missColor;
		withinSum += wi;
		// (an invalid sample has within = 0 and no root: minNeighbours >= 1 keeps it from counting as a core)
		if (cluster == CLUSTER_NOISE) noise++; else if (cluster_is_core(wi, k.minNeighbours)) core++; else border++;
	}
	core = block_reduce<false>(core, sh);
	border = block_reduce<false>(border, sh);
	noise = block_reduce<false>(noise, sh);
	withinSum = block_reduce<false>(withinSum, sh);
	if (threadIdx.x == 0u) { ClusPart* part = kparts_of(k) + blockIdx.x; part->core = core; part->border = border; part->noise = noise; part->within = withinSum; }
}

__global__ __launch_bounds__(CMP_TPB) void k_k_final(ClusArgs k) {
	__shared__ uint64_t sh[CMP_WAVES];
	const CmpArgs& c = k.c;
	if (header_of(c)->run == 0u) return;
	const ClusPart* parts = kparts_of(k);
	SimlodClusterSummary* out = reinterpret_cast<SimlodClusterSummary*>(c.summary);
	if (threadIdx.x < CLUSTER_SIZE_BINS) {                                      // one lane per bin
		uint64_t h = 0u;
		for (uint32_t p = 0; p < c.gridA; p++) h += parts[p].hist[threadIdx.x];
		out->sizeHist[threadIdx.x] = h;
	}
	uint64_t error = 0u, kept = 0u, dissolved = 0u, largest = 0u, core = 0u, border = 0u, noise = 0u, within = 0u;
	for (uint32_t p = threadIdx.x; p < c.gridA; p += CMP_TPB) {
		error |= parts[p].error; kept += parts[p].kept; dissolved += parts[p].dissolved;
		largest = parts[p].largest > largest ? parts[p].largest : largest;
		core += parts[p].core; border += parts[p].border; noise += parts[p].noise; within += parts[p].within;
	}
	error = block_reduce<true>(error, sh);
	kept = block_reduce<false>(kept, sh);
	dissolved = block_reduce<false>(dissolved, sh);
	largest = block_reduce<true>(largest, sh);
	core = block_reduce<false>(core, sh);
	border = block_reduce<false>(border, sh);
	noise = block_reduce<false>(noise, sh);
	within = block_reduce<false>(within, sh);
	if (threadIdx.x == 0u) {
		out->error = error != 0u ? SIMLOD_CLUSTER_ERR_INTERNAL : 0u;            // (the budget's bit is clear: the pass ran)
		out->numClusters = (uint32_t)kept;
		out->numDissolved = dissolved;
		out->numCore = core; out->numBorder = border; out->numNoise = noise; out->numWithin = within;
		out->largestSize = (uint32_t)(largest >> 32);
		out->largestCluster = kept != 0u ? 0xffffffffu - (uint32_t)largest : 0u;
	}
}

uint64_t cluster_bytes(uint64_t numA) { return compare_count_acceptable(numA) ? ClusLayout(numA).bytes : 0u; }

// simlod_cluster_samples: the compare call's checks with b = a and the same six launches, then the seven above.
int launch_cluster_impl(const SimlodUniforms* u, const SimlodPoint* a, uint64_t numA, const SimlodClusterParams* params, void* scratch, uint64_t scratchBytes,
                        SimlodClusterRecord* records, uint32_t* colors, SimlodClusterSummary* summary, hipStream_t stream) {
	if (params == nullptr || !cluster_acceptable(*params)) return (int)hipErrorInvalidValue;
	ClusWriteArgs t{};
	ClusArgs& k = t.k;
	CmpArgs& c = k.c;
	const CmpCall call{params->radius, params->noiseColor, params->maxCandidates, params->maxWorkgroups};
	// (the summary has SimlodCompareSummary's size and its leading fields: k_c_decide writes it as it is and zeroes the rest)
	if (!compare_prepare(u, a, numA, a, numA, call, scratch, scratchBytes, records, colors, reinterpret_cast<SimlodCompareSummary*>(summary), c))
		return (int)hipErrorInvalidValue;
	const ClusLayout lay(numA);
	if (scratchBytes < lay.bytes) return (int)hipErrorInvalidValue;
	k.within = lay.within; k.parent = lay.parent; k.attach = lay.attach; k.size = lay.size; k.id = lay.id; k.parts = lay.parts;
	k.span = ((numA + c.gridA - 1u) / c.gridA + CMP_TPB - 1u) / CMP_TPB * CMP_TPB;  // gridA spans cover numA
	k.minNeighbours = params->minNeighbours; k.minClusterSize = params->minClusterSize;
	k.records = records;
	for (uint32_t i = 0; i < 256u; i++) t.table[i] = params->table[i];
	launch_grid(c, stream);
	if (records != nullptr) {
		SIMLOD_LAUNCH(k_k_core, dim3(c.gridA), dim3(CMP_TPB), stream, k);
		SIMLOD_LAUNCH(k_k_link, dim3(c.gridA), dim3(CMP_TPB), stream, k);
		SIMLOD_LAUNCH(k_k_sizes, dim3(c.gridA), dim3(CMP_TPB), stream, k);
		SIMLOD_LAUNCH(k_k_roots, dim3(c.gridA), dim3(CMP_TPB), stream, k);
		SIMLOD_LAUNCH(k_k_ids, dim3(c.gridA), dim3(CMP_TPB), stream, k);
		SIMLOD_LAUNCH(k_k_write, dim3(c.gridA), dim3(CMP_TPB), stream, t);
		SIMLOD_LAUNCH(k_k_final, dim3(1), dim3(CMP_TPB), stream, k);
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}
