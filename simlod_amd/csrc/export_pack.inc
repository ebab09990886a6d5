// export_pack.inc — part of export.hip: packed samples.  PackItem, PackLayout, PackArgs, k_pk_scan, k_pk_dir, pack_reduce, k_pk_pack, k_pk_unpack.
// ---- packed samples -------------------------------------------------------------------------------------------------------------------------
// simlod_pack_samples / simlod_unpack_samples (simlod_hip.h, "packed samples"; the rules in pack_rules.hpp): three launches on the caller's stream.
//   k_pk_scan    ONE workgroup: per table entry the range of rule K5 and its checks (rule K7), the exclusive scan of the pieces per entry
//                (-> first[]), the item capacity check, the counts record (numSamples, error; the rest zero).
//   k_pk_dir     one lane per table entry: the node's frame (rules K1, K2, K4 — the one fp64 division per node is here) and its pieces of at most
//                1 000 samples as PackItems, so that the hot kernel never touches the table.
//   k_pk_pack /  the hot path: one piece per 256-lane workgroup and turn (grid-stride).  A lane's four loads (16 bytes each; 8 for unpack) are
//   k_pk_unpack  issued before the arithmetic, non-temporal as k_copy's; per sample three fp64 subtract-multiply pairs and, for voxels, the fp32
//                verify; 8-byte (16-byte) non-temporal stores.  The three counters stay in registers over a workgroup's turns, are summed per
//                wave by shuffles and per workgroup in LDS, and leave the CU as at most three atomics per workgroup.

// 64 B; kind: bit 0 the leaf bit, bits 8-15 the level (ns and the fp32 node size follow from it exactly)
struct PackItem { uint64_t first; uint32_t count, kind; double nmin[3]; double k; float fmin[3]; uint32_t pad; };
static_assert(sizeof(PackItem) == 64, "PackItem");

// scratch: Header (error, numListed, numItems) | first u32[numNodes + 1] | items PackItem[...] up to the buffer's end
struct PackLayout {
	uint64_t first, items;
	__host__ __device__ explicit PackLayout(uint32_t n) { first = 256; items = first + align256(4ull * n + 4u); }
};
__host__ __device__ inline uint64_t pack_item_bound(uint32_t n, uint64_t sampleBound) { return sampleBound / SIMLOD_POINTS_PER_CHUNK + n + 1u; }

struct PackArgs {
	const SimlodExportNode* table;
	const SimlodDeltaEntry* entries;     // or nullptr
	uint32_t                n, pad;
	uint64_t                sampleCap;
	uint8_t*                scratch;
	uint64_t                first, items, itemCap;
	PackBox                 box;
	const void*             in;          // pack: SimlodPoint[sampleCap]; unpack: uint64_t[sampleCap]
	void*                   out;         // pack: uint64_t[sampleCap]; unpack: SimlodPoint[sampleCap]
	SimlodPackCounts*       counts;
};

__global__ __launch_bounds__(WG_TPB) void k_pk_scan(PackArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ uint32_t sh_err;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(a.scratch + a.first);
	if (threadIdx.x == 0) sh_err = 0u;                                      // (the scans' barriers lie between this and the lanes' bits)
	uint64_t samples = 0u, items = 0u;
	uint32_t bad = 0u;
	for (uint32_t base = 0; base < a.n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		uint64_t f = 0u;
		uint32_t cnt = 0u, err = 0u;
		if (t < a.n && !pack_entry_range(a.table[t], a.entries != nullptr ? a.entries + t : nullptr, a.sampleCap, f, cnt, err)) cnt = 0u;
		bad |= err;
		uint64_t totS, totI;
		block_scan<uint64_t>(cnt, totS, sh_scan);
		const uint64_t offI = block_scan<uint64_t>(ceil_chunks(cnt), totI, sh_scan);
		if (t < a.n) first[t] = (uint32_t)(items + offI);
		samples += totS; items += totI;
	}
	__syncthreads();                                                        // (n == 0 cannot be: the launcher refuses it)
	if (bad != 0u) atomicOr(&sh_err, bad);
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t err = sh_err;
		const bool over = items > a.itemCap;
		if (over) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		first[a.n] = (uint32_t)items;
		hdr->error = err; hdr->numListed = a.n;
		hdr->numItems = over ? 0u : items;
		SimlodPackCounts c;
		c.numSamples = over ? 0u : samples; c.numClamped = 0u; c.numInexact = 0u; c.numAlpha = 0u; c.error = err; c.reserved = 0u;
		*a.counts = c;
	}
}

__global__ __launch_bounds__(LANE_TPB) void k_pk_dir(PackArgs a) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.scratch + a.first);
	PackItem* items = reinterpret_cast<PackItem*>(a.scratch + a.items);
	const uint32_t t = blockIdx.x * LANE_TPB + threadIdx.x;
	if (t >= a.n || hdr->numItems == 0u) return;
	const SimlodExportNode& e = a.table[t];
	uint64_t f;
	uint32_t cnt, err;
	if (!pack_entry_range(e, a.entries != nullptr ? a.entries + t : nullptr, a.sampleCap, f, cnt, err)) return;
	const bool leaf = (e.flags & SIMLOD_EXPORT_FLAG_LEAF) != 0u;
	const PackFrame fr = pack_frame(a.box, e.level, e.X, e.Y, e.Z, leaf);
	PackItem it;
	it.kind = (leaf ? 1u : 0u) | e.level << 8; it.k = fr.k; it.pad = 0u;
	for (int k = 0; k < 3; k++) { it.nmin[k] = fr.nmin[k]; it.fmin[k] = fr.fmin[k]; }
	uint32_t at = first[t];
	for (uint32_t o = 0; o < cnt; o += SIMLOD_POINTS_PER_CHUNK) {
		it.first = f + o; it.count = min(cnt - o, (uint32_t)SIMLOD_POINTS_PER_CHUNK);
		items[at++] = it;
	}
}

__device__ __forceinline__ PackFrame pack_item_frame(const PackItem& it) {
	PackFrame f;
	for (int k = 0; k < 3; k++) { f.nmin[k] = it.nmin[k]; f.fmin[k] = it.fmin[k]; }
	f.k = it.k;
	return f;
}

// the sum of v over the workgroup's lanes into *dst: shuffles inside a wave, LDS between the waves, one atomic (if anything) per workgroup
__device__ __forceinline__ void pack_reduce(uint32_t v, uint32_t* lds, uint64_t* dst) {
#pragma unroll
	for (int o = SIMLOD_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, (unsigned)o, SIMLOD_WAVE);
	if (lane_id() == 0 && v != 0u) atomicAdd(lds, v);
	__syncthreads();
	if (threadIdx.x == 0 && *lds != 0u) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)*lds);
}

__global__ __launch_bounds__(LANE_TPB) void k_pk_pack(PackArgs a) {
	__shared__ uint32_t sh_sum[3];
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const PackItem* items = reinterpret_cast<const PackItem*>(a.scratch + a.items);
	const u32x4* samples = reinterpret_cast<const u32x4*>(a.in);
	uint64_t* packed = reinterpret_cast<uint64_t*>(a.out);
	const uint64_t numItems = hdr->numItems;
	if (threadIdx.x < 3u) sh_sum[threadIdx.x] = 0u;
	uint32_t clamped = 0u, inexact = 0u, alpha = 0u;                        // (a lane sees fewer than 2^32 samples: four per turn)
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const PackItem it = items[i];
		u32x4 v[4];
		load_chunk4<true, true>(samples + it.first, it.count, v);
		const PackFrame f = pack_item_frame(it);
		const bool leaf = (it.kind & 1u) != 0u;
		const float fns = a.box.sizef / pack_exp2(it.kind >> 8);
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			if (k < it.count) {
				uint32_t what;
				const uint64_t w = pack_sample(f, fns, leaf, __uint_as_float(v[j].x), __uint_as_float(v[j].y), __uint_as_float(v[j].z), v[j].w, what);
				__builtin_nontemporal_store(w, packed + it.first + k);
				clamped += what & PACK_CLAMPED ? 1u : 0u; inexact += what & PACK_INEXACT ? 1u : 0u; alpha += what & PACK_ALPHA ? 1u : 0u;
			}
		}
	}
	__syncthreads();                                                        // (sh_sum is zero for every wave)
	pack_reduce(clamped, &sh_sum[0], &a.counts->numClamped);
	pack_reduce(inexact, &sh_sum[1], &a.counts->numInexact);
	pack_reduce(alpha, &sh_sum[2], &a.counts->numAlpha);
}

__global__ __launch_bounds__(LANE_TPB) void k_pk_unpack(PackArgs a) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const PackItem* items = reinterpret_cast<const PackItem*>(a.scratch + a.items);
	const uint64_t* packed = reinterpret_cast<const uint64_t*>(a.in);
	u32x4* samples = reinterpret_cast<u32x4*>(a.out);
	const uint64_t numItems = hdr->numItems;
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const PackItem it = items[i];
		uint64_t w[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			w[j] = k < it.count ? __builtin_nontemporal_load(packed + it.first + k) : 0ull;
		}
		const PackFrame f = pack_item_frame(it);
		const bool leaf = (it.kind & 1u) != 0u;
		const double ns = pack_node_size(a.box.size, it.kind >> 8);
		const float fns = a.box.sizef / pack_exp2(it.kind >> 8);
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			if (k < it.count) {
				const SimlodPoint p = unpack_sample(f, ns, fns, leaf, w[j]);
				const u32x4 o = {__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), p.color};
				__builtin_nontemporal_store(o, samples + it.first + k);
			}
		}
	}
}
