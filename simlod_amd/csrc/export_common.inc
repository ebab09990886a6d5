// export_common.inc — part of export.hip (inside namespace simlod { namespace {): what every call family shares.  The constants, the scratch
// header and Layout, the wave and workgroup scans, ExportArgs, the classes of a table entry, the chunk table's stamp check, the scans behind a
// walk, the four-in-flight chunk loads, k_copy.
constexpr uint32_t WG_TPB = 1024;                                                  // the single-workgroup passes
constexpr uint32_t WG_WAVES = WG_TPB / SIMLOD_WAVE;
constexpr uint32_t LANE_TPB = 256;                                                 // one lane per node / the copy
constexpr uint64_t CHUNK_STRIDE = SIMLOD_ALLOC_ROUND(sizeof(SimlodChunk));         // 16 032: what AllocatorGlobal::alloc advances per chunk
constexpr uint64_t CHUNK_BASE = 16;                                                // first allocation behind the allocator header
constexpr uint64_t GRID_STRIDE = SIMLOD_ALLOC_ROUND(sizeof(SimlodOccupancyGrid));  // 262 160: what the builder's grid allocations advance
constexpr uint32_t NONE = SIMLOD_EXPORT_NONE;

struct CopyItem { uint64_t src, dst; uint32_t count, pad0; uint64_t pad1; };       // 32 B; count == 0: nothing
static_assert(sizeof(CopyItem) == 32, "CopyItem");

// scratch: header | map u32[cap] (export: table index -> node index) | par u32[cap] (export: parent table index) | first u32[cap + 1]
// (first copy item of each table entry) | items CopyItem[itemCap]
struct Header {
	uint32_t error, numListed, ok, pad;
	uint64_t numItems;
	uint64_t totalChunks;
	uint32_t counts[8];                  // import: inner, leaves, nonempty leaves, points, voxels, point chunks, voxel chunks
	// buildable import: the table entries of each level below 20 ([lvFirst, lvEnd): breadth-first order keeps a level together; level 20 has
	// no inner nodes), the grids (one per inner node and the root, in table order, from gridBase on), a grid that disagrees with the table,
	// the voxels rebuilt for a root that is a leaf
	uint32_t lvFirst[SIMLOD_MAX_DEPTH], lvEnd[SIMLOD_MAX_DEPTH];
	uint32_t numGrids, gridBad, rootVoxels, pad1;
	uint64_t gridBase, rootVoxBase;
};
static_assert(sizeof(Header) <= 256, "Header");
__host__ __device__ inline uint64_t align256(uint64_t v) { return (v + 255u) & ~255ull; }
struct Layout {
	uint64_t map = 0, par = 0, first = 0, items = 0, itemCap = 0, bytes = 0;
	Layout() = default;
	__host__ __device__ Layout(uint32_t cap, uint64_t sampleCap) {
		map = 256; par = map + align256(4ull * cap); first = par + align256(4ull * cap); items = first + align256(4ull * cap + 4u);
		itemCap = sampleCap / SIMLOD_POINTS_PER_CHUNK + cap + 1u;     // sum over nodes of ceil(n_i / 1000) <= N / 1000 + nodes
		bytes = items + itemCap * sizeof(CopyItem);
	}
	// a query's items (32 bytes each, as CopyItems) take what a buffer of `scratchBytes` has from `items` on: its caller sizes it by a bound of its own
	void take_rest(uint64_t scratchBytes) { itemCap = std::min<uint64_t>((scratchBytes - items) / sizeof(CopyItem), 0xffffffffull); bytes = scratchBytes; }
};

// inclusive scan over the wave
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T x) {
	const int lane = lane_id();
#pragma unroll
	for (int o = 1; o < SIMLOD_WAVE; o <<= 1) {
		const T y = __shfl_up(x, (unsigned)o, SIMLOD_WAVE);
		if (lane >= o) x += y;
	}
	return x;
}

// exclusive scan over the workgroup (WG_TPB lanes); every lane gets the total.  `lds`: WG_WAVES words, reused by the next call after a barrier.
template <typename T>
__device__ __forceinline__ T block_scan(T v, T& total, T* lds) {
	const T x = wave_incl_scan(v);
	const int lane = lane_id(), w = (int)(threadIdx.x / SIMLOD_WAVE);
	if (lane == SIMLOD_WAVE - 1) lds[w] = x;
	__syncthreads();
	T before = 0, all = 0;
	for (int k = 0; k < (int)WG_WAVES; k++) { const T s = lds[k]; before += k < w ? s : (T)0; all += s; }
	__syncthreads();
	total = all;
	return before + x - v;
}

__device__ __forceinline__ uint32_t ceil_chunks(uint64_t n) { return (uint32_t)((n + SIMLOD_POINTS_PER_CHUNK - 1u) / SIMLOD_POINTS_PER_CHUNK); }

struct ExportArgs {
	const SimlodNode*  nodes;
	const SimlodStats* stats;
	uint32_t           maxLevel, select, cap;
	uint8_t*           scratch;
	SimlodExportNode*  table;
	SimlodPoint*       samples;
	uint64_t           sampleCap;
	SimlodExportCounts* counts;
	Layout             lay;
	// the builder's chunk table of `nodes` (LeafTableRef), or table == nullptr
	const uint8_t*     lt;
	const uint8_t*     ltPers;
	const uint32_t*    ltMagic;
	const uint32_t*    ltBatch;
	const uint64_t*    ltNodes;
	const uint64_t*    ltSig;
	uint32_t           ltMagicValue, ltSlots, ltRows;
};

// the class of a table entry against a query's region (cls[] in the scratch buffer; the pair queries tag every entry as copied).  Q_EMPTIED
// (the inverse selections only, export_inverse.inc): listed, contributes nothing — what an outside root is, for any node
enum : uint32_t { Q_OUTSIDE = 0u, Q_FILTERED = 1u, Q_COPIED = 2u, Q_EMPTIED = 3u };

// Does the builder's chunk table describe node `src` of this octree as it is now (render.hip visible_nodes: the same four stamp words), and
// does its row start at the list's head?  `leaf`: the list is the node's points.  Never the voxel row of the ROOT: the builder keeps no such
// row (construct_voxelize.inc vox_chunk_publish), but k_begin's rebuild_side_tables fills row 0 from the root's voxel list as it is THEN — it
// starts at the head from then on, and the slots behind what the list held at the rebuild are whatever was there.
__device__ __forceinline__ bool leaf_rows_valid(const ExportArgs& a, uint32_t src, const SimlodChunk* head, bool leaf) {
	bool rows = false;
	if (a.lt != nullptr && src < a.ltRows && (src != 0u || leaf)) {
		rows = *a.ltMagic == a.ltMagicValue && *a.ltBatch == a.stats->batchletIndex && *a.ltNodes == (uint64_t)a.nodes && *a.ltSig == table_signature(a.stats);
		rows = rows && leaf_row_get(a.lt, a.ltPers, src, 0u) == head;
	}
	return rows;
}

// The scans behind a walk (ONE workgroup; k_x_scan, k_p_hier): numSamples -> firstSample, the chunks per node -> first[] (the node's first
// item), first[n], the item capacity check.  per(t): what the kernel writes per entry on top.  `err` (lane 0 only): the header's error word
// with the check applied.  (`a` by value: k_x_scan then reads its arguments where it did before the routine was shared, and keeps its registers.)
struct TableScan { uint32_t n, err; uint64_t samples, items; };
template <typename F>
__device__ __forceinline__ TableScan scan_table(const ExportArgs a, uint64_t* sh_scan, F per) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(a.scratch + a.lay.first);
	TableScan s{hdr->numListed, 0u, 0u, 0u};
	for (uint32_t base = 0; base < s.n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		const uint64_t ns = t < s.n ? a.table[t].numSamples : 0u;
		uint64_t totS, totI;
		const uint64_t offS = block_scan<uint64_t>(ns, totS, sh_scan);
		const uint64_t offI = block_scan<uint64_t>(ceil_chunks(ns), totI, sh_scan);
		if (t < s.n) { a.table[t].firstSample = s.samples + offS; first[t] = (uint32_t)(s.items + offI); per(t); }
		s.samples += totS; s.items += totI;
	}
	if (threadIdx.x == 0) {
		s.err = hdr->error | (s.items > a.lay.itemCap ? SIMLOD_EXPORT_ERR_CAPACITY : 0u);
		first[s.n] = (uint32_t)s.items;
	}
	return s;
}

// Four 16-byte loads of a lane in flight: the samples k = lane + 256 j < cnt of the chunk at `s`; the other v[j] become zero (ZERO) or stay
// as they are.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <bool NONTEMPORAL, bool ZERO>
__device__ __forceinline__ void load_chunk4(const u32x4* s, uint32_t cnt, u32x4 (&v)[4]) {
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
		if (ZERO) v[j] = k < cnt ? (NONTEMPORAL ? __builtin_nontemporal_load(s + k) : s[k]) : u32x4{0u, 0u, 0u, 0u};
		else if (k < cnt) v[j] = NONTEMPORAL ? __builtin_nontemporal_load(s + k) : s[k];
	}
}
__device__ __forceinline__ void copy_chunk(const u32x4* s, u32x4* d, uint32_t cnt) {
	u32x4 v[4];
	load_chunk4<true, false>(s, cnt, v);
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
		if (k < cnt) __builtin_nontemporal_store(v[j], d + k);
	}
}
// the hot path: one chunk (<= 1 000 samples of 16 bytes) per workgroup and turn, four 16-byte loads per lane in flight before the stores
__global__ __launch_bounds__(LANE_TPB) void k_copy(const uint8_t* scratch, uint64_t itemsOff) {
	const Header* hdr = reinterpret_cast<const Header*>(scratch);
	const CopyItem* items = reinterpret_cast<const CopyItem*>(scratch + itemsOff);
	const uint64_t numItems = hdr->numItems;
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const CopyItem it = items[i];
		copy_chunk(reinterpret_cast<const u32x4*>(it.src), reinterpret_cast<u32x4*>(it.dst), it.count);
	}
}
static_assert(4u * LANE_TPB >= SIMLOD_POINTS_PER_CHUNK, "k_copy: one chunk per workgroup and turn");
