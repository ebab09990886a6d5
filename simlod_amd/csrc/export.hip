// export.hip — octree export / import (include/simlod_hip.h, "octree export / import"; no counterpart in the reference).
//
// Export: four launches on the caller's stream.
//   k_x_hier   ONE workgroup: the breadth-first walk, level by level (at most 21 levels, none past maxLevel).  Per level one lane per node:
//              the node's child mask from its non-null children, a workgroup exclusive scan of the popcounts gives the children's table
//              indices, the lane writes its table entry (everything but firstSample) and its children's source indices.  Config 2 has
//              4 425 nodes: five rounds of 1 024 lanes in all; no grid-wide barrier.
//   k_x_scan   ONE workgroup: exclusive scans of numSamples (-> firstSample) and of the chunks per node (-> the node's first copy item);
//              the capacity check of the samples; SimlodExportCounts.
//   k_x_dir    one lane per table entry: the node's chunk addresses — the first <= 50 from the builder's chunk table while that is valid
//              (the stamp check r_visible does, render.hip), the rest (or all) by `next` — as copy items {source, destination, count}.
//   k_copy     the hot path: one workgroup per chunk at a time (grid-stride), 16-byte loads and stores, four per lane in flight.
// Import: k_i_validate (ONE workgroup: every check, the scans, the Stats counts) -> k_i_nodes (one lane per node: Node record, the chunk
// headers of its list, its copy items) -> k_copy (the same kernel, samples -> chunks) -> k_i_finish (allocator header, Stats).
// The buildable import (simlod_import_octree_buildable): the same four kernels — the validation with the buildability checks, the Node records
// with grid pointers — and, between k_copy and k_i_finish, the occupancy grids rebuilt from the samples: k_i_gleaf, k_i_gdown per level,
// k_i_groot (below); k_i_finish then also writes the builder's counters as k_reset does.
// Region query (simlod_query_region): k_q_hier -> k_q_dir -> k_q_count -> k_q_scan -> k_q_write, described at "region query" below.
// Ray query (simlod_query_rays): k_r_hier -> k_q_dir -> k_r_pairs<count> -> k_r_scan -> k_r_pairs<fill> -> k_r_test -> k_r_reduce, at "ray query" below.
// Everything in between lives in the caller's scratch buffer (export_min_bytes), never in kernel_construct's momentary buffer: the builder's
// recycle stack and the chunk table export reads are there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "simlod_device.hpp"
#include "simlod_hip.h"
#include "simlod_internal.hpp"

namespace simlod {
namespace {

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
};

// exclusive scan over the workgroup (WG_TPB lanes); every lane gets the total.  `lds`: WG_WAVES words, reused by the next call after a barrier.
template <typename T>
__device__ __forceinline__ T block_scan(T v, T& total, T* lds) {
	const int lane = lane_id(), w = (int)(threadIdx.x / SIMLOD_WAVE);
	T x = v;
#pragma unroll
	for (int o = 1; o < SIMLOD_WAVE; o <<= 1) {
		const T y = __shfl_up(x, (unsigned)o, SIMLOD_WAVE);
		if (lane >= o) x += y;
	}
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

// ---- region queries: the classification of a node against the region (simlod_hip.h, "region queries", rules 1 and 4) ----------------------
// fp64 from the fp32 inputs, every sum in the order the header states (the library is built with -ffp-contract=off: no fused multiply-add),
// so that the numpy mirror (simlod_amd/octree_io.py OctreeExport.crop) reproduces every decision bit for bit.
struct QueryGeom {
	double   min[3], size;
	uint32_t numPlanes, pad;
	double   pl[SIMLOD_REGION_MAX_PLANES][4];
};
enum : uint32_t { Q_OUTSIDE = 0u, Q_FILTERED = 1u, Q_COPIED = 2u };

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

// The breadth-first walk of k_x_hier and, QUERY, of k_q_hier: there a child that lies outside the region is not listed (it counts as cut off
// for the node-count check), and cls[t] gets the class of every listed entry; numSamples then holds the samples BEFORE the test.
template <bool QUERY>
__device__ __forceinline__ void hier_walk(const ExportArgs& a, const QueryGeom* g, uint32_t* cls) {
	__shared__ uint32_t sh_scan[WG_WAVES];
	__shared__ uint32_t sh_err, sh_trunc;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* map = reinterpret_cast<uint32_t*>(a.scratch + a.lay.map);
	uint32_t* par = reinterpret_cast<uint32_t*>(a.scratch + a.lay.par);
	const uint32_t numNodes = a.stats->numNodes;
	const uint32_t maxLevel = min(a.maxLevel, (uint32_t)SIMLOD_MAX_DEPTH);
	if (threadIdx.x == 0) {
		sh_err = numNodes == 0u ? SIMLOD_EXPORT_ERR_NODE_COUNT : a.cap == 0u ? SIMLOD_EXPORT_ERR_CAPACITY : 0u;
		sh_trunc = 0u;
		if (sh_err == 0u) { map[0] = 0u; par[0] = NONE; }
	}
	__syncthreads();
	uint32_t lo = 0u, hi = sh_err == 0u ? 1u : 0u;
	for (uint32_t L = 0; L <= maxLevel && lo < hi; L++) {
		uint32_t next = hi;
		for (uint32_t base = lo; base < hi; base += WG_TPB) {
			const uint32_t t = base + threadIdx.x;
			const bool act = t < hi;
			const uint32_t src = act ? map[t] : 0u;
			const SimlodNode* n = a.nodes + src;
			uint32_t child[8], mask = 0u;
			bool srcLeaf = true;
			if (act) {
#pragma unroll
				for (int k = 0; k < 8; k++) {
					const SimlodNode* c = n->children[k];
					child[k] = 0u;
					if (c == nullptr) continue;
					srcLeaf = false;
					const uint64_t idx = (uint64_t)(c - a.nodes);
					if (c < a.nodes || idx >= numNodes) { atomicOr(&sh_err, SIMLOD_EXPORT_ERR_NODE_COUNT); continue; }
					child[k] = (uint32_t)idx;
					if (L >= maxLevel) continue;
					// (the child's cube follows from its parent's: no load of the child's record, which would put eight dependent loads in a row)
					if (QUERY && classify(*g, n->level + 1u, 2u * n->X + ((k >> 2) & 1), 2u * n->Y + ((k >> 1) & 1), 2u * n->Z + (k & 1)) == Q_OUTSIDE) {
						atomicOr(&sh_trunc, 1u);
						continue;
					}
					mask |= 1u << k;
				}
				if (!srcLeaf && L >= maxLevel) atomicOr(&sh_trunc, 1u);
			}
			uint32_t total;
			const uint32_t off = block_scan<uint32_t>((uint32_t)__popc(mask), total, sh_scan);
			const uint32_t fc = next + off;
			if (act) {
				uint32_t r = 0;
				for (int k = 0; k < 8; k++) {
					if (!(mask & (1u << k))) continue;
					if (fc + r < a.cap) { map[fc + r] = child[k]; par[fc + r] = t; }
					else atomicOr(&sh_err, SIMLOD_EXPORT_ERR_CAPACITY);
					r++;
				}
				const uint32_t parent = par[t];
				bool sel = true;
				if (a.select == SIMLOD_EXPORT_CUT) sel = srcLeaf || L == maxLevel;
				else if (a.select == SIMLOD_EXPORT_VISIBLE) {
					// render.cu:905-935 as r_visible decides it (render.hip visible_nodes): drawn = visible && (large ? leaf : parent large)
					const bool parentLarge = parent != NONE && a.nodes[map[parent]].isLarge != 0;
					sel = n->visible != 0 && (n->isLarge != 0 ? srcLeaf : parentLarge);
				}
				SimlodExportNode e;
				e.level = n->level; e.X = n->X; e.Y = n->Y; e.Z = n->Z;
				e.parent = parent;
				e.firstChild = mask != 0u ? fc : NONE;
				e.childMask = (uint8_t)mask;
				e.flags = (uint8_t)((srcLeaf ? SIMLOD_EXPORT_FLAG_LEAF : 0u) | (sel ? SIMLOD_EXPORT_FLAG_SELECTED : 0u));
				e.reserved = 0;
				e.numSamples = sel ? (srcLeaf ? n->numPoints : n->numVoxels) : 0u;
				e.firstSample = 0;
				if (QUERY) {
					const uint32_t c = classify(*g, e.level, e.X, e.Y, e.Z);              // (only the root can be outside here)
					if (c == Q_OUTSIDE) e.numSamples = 0u;
					cls[t] = c;
				}
				a.table[t] = e;
			}
			next += total;
		}
		__syncthreads();                         // (the children's map entries, written by other lanes, are read next level)
		lo = hi;
		hi = min(next, a.cap);
		if (sh_err & SIMLOD_EXPORT_ERR_CAPACITY) break;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t err = sh_err;
		const uint32_t listed = (err & SIMLOD_EXPORT_ERR_CAPACITY) ? lo : hi;        // entries written
		// every node is reached exactly once from the root: all of them when nothing was cut off, no more than all of them otherwise
		if (sh_trunc == 0u ? listed != numNodes : listed > numNodes) err |= SIMLOD_EXPORT_ERR_NODE_COUNT;
		hdr->error = err;
		hdr->numListed = listed;
	}
}

__global__ __launch_bounds__(WG_TPB) void k_x_hier(ExportArgs a) { hier_walk<false>(a, nullptr, nullptr); }

__global__ __launch_bounds__(WG_TPB) void k_x_scan(ExportArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(a.scratch + a.lay.first);
	const uint32_t n = hdr->numListed;
	uint64_t samples = 0, items = 0;
	for (uint32_t base = 0; base < n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		const uint64_t ns = t < n ? a.table[t].numSamples : 0u;
		uint64_t totS, totI;
		const uint64_t offS = block_scan<uint64_t>(ns, totS, sh_scan);
		const uint64_t offI = block_scan<uint64_t>(ceil_chunks(ns), totI, sh_scan);
		if (t < n) { a.table[t].firstSample = samples + offS; first[t] = (uint32_t)(items + offI); }
		samples += totS; items += totI;
	}
	if (threadIdx.x == 0) {
		uint32_t err = hdr->error;
		if (samples > a.sampleCap || items > a.lay.itemCap) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		first[n] = (uint32_t)items;
		hdr->numItems = (err & SIMLOD_EXPORT_ERR_CAPACITY) ? 0u : items;       // a sample array that is too small gets nothing
		SimlodExportCounts c;
		c.numNodes = n; c.error = err; c.numSamples = samples;
		*a.counts = c;
	}
}

__global__ __launch_bounds__(LANE_TPB) void k_x_dir(ExportArgs a) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const uint32_t* map = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.map);
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.first);
	CopyItem* items = reinterpret_cast<CopyItem*>(a.scratch + a.lay.items);
	const uint32_t t = blockIdx.x * LANE_TPB + threadIdx.x;
	if (t >= hdr->numListed || hdr->numItems == 0u) return;
	const SimlodExportNode& e = a.table[t];
	const uint32_t ns = e.numSamples;
	if (ns == 0u) return;
	const uint32_t src = map[t];
	const SimlodNode* n = a.nodes + src;
	const SimlodChunk* c = (e.flags & SIMLOD_EXPORT_FLAG_LEAF) ? n->points : n->voxelChunks;
	// the builder's table describes this octree as it is now (render.hip visible_nodes: the same four stamp words) and its row starts at the list's head
	bool rows = false;
	if (a.lt != nullptr && src < a.ltRows) {
		rows = *a.ltMagic == a.ltMagicValue && *a.ltBatch == a.stats->batchletIndex && *a.ltNodes == (uint64_t)a.nodes && *a.ltSig == table_signature(a.stats);
		rows = rows && leaf_row_get(a.lt, a.ltPers, src, 0u) == c;
	}
	const uint32_t nch = ceil_chunks(ns), f = first[t];
	const uint64_t dst0 = reinterpret_cast<uint64_t>(a.samples + e.firstSample);
	uint32_t k = 0;
	for (; k < nch; k++) {
		if (k > 0u) c = rows && k < a.ltSlots ? leaf_row_get(a.lt, a.ltPers, src, k) : c->next;
		if (c == nullptr) { atomicOr(&a.counts->error, SIMLOD_EXPORT_ERR_SHORT_LIST); break; }
		CopyItem it;
		it.src = reinterpret_cast<uint64_t>(c->points);
		it.dst = dst0 + (uint64_t)k * SIMLOD_POINTS_PER_CHUNK * sizeof(SimlodPoint);
		it.count = min(ns - k * SIMLOD_POINTS_PER_CHUNK, SIMLOD_POINTS_PER_CHUNK);
		it.pad0 = 0; it.pad1 = 0;
		items[f + k] = it;
	}
	for (; k < nch; k++) items[f + k] = CopyItem{0, 0, 0, 0, 0};
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void copy_chunk(const u32x4* s, u32x4* d, uint32_t cnt) {
	u32x4 v[4];
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
		if (k < cnt) v[j] = __builtin_nontemporal_load(s + k);
	}
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
struct QItem { uint64_t src; uint32_t count, node, k, tag, pass, off; };          // 32 B, in the place of the export's CopyItems
static_assert(sizeof(QItem) == 32, "QItem");
// scratch: Layout's header | map | par | first, then cls u32[cap] (the class of each table entry), then the items up to the buffer's end
__host__ __device__ inline uint64_t query_fixed_bytes(uint32_t cap) { return 256u + 3u * align256(4ull * cap) + align256(4ull * cap + 4u); }

struct QueryArgs {
	ExportArgs         x;               // (x.counts unused; x.lay: map / par / first / items / itemCap as the query lays them out)
	QueryGeom          g;
	uint64_t           cls;             // offset of cls[] in the scratch buffer
	SimlodQueryCounts* counts;
};

__global__ __launch_bounds__(WG_TPB) void k_q_hier(QueryArgs q) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const ExportArgs& a = q.x;
	uint32_t* cls = reinterpret_cast<uint32_t*>(a.scratch + q.cls);
	hier_walk<true>(a, &q.g, cls);
	__syncthreads();
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(a.scratch + a.lay.first);
	const uint32_t n = hdr->numListed;
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
	const SimlodChunk* head = (e.flags & SIMLOD_EXPORT_FLAG_LEAF) ? n->points : n->voxelChunks;
	// the builder's table while its stamp matches, as k_x_dir reads it
	bool rows = false;
	if (a.lt != nullptr && src < a.ltRows) {
		rows = *a.ltMagic == a.ltMagicValue && *a.ltBatch == a.stats->batchletIndex && *a.ltNodes == (uint64_t)a.nodes && *a.ltSig == table_signature(a.stats);
		rows = rows && leaf_row_get(a.lt, a.ltPers, src, 0u) == head;
	}
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

__global__ __launch_bounds__(LANE_TPB) void k_q_count(QueryArgs q) {
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
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			v[j] = k < cnt ? s[k] : u32x4{0u, 0u, 0u, 0u};
		}
		uint32_t c = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			c += (uint32_t)__popcll(__ballot(k < cnt && passes(q.g, v[j])));
		}
		if (lane == 0) sh_cnt[turn][w] = c;
		__syncthreads();                    // (two buffers: the next turn's writes cannot overtake this turn's read)
		if (threadIdx.x == 0) items[i].pass = sh_cnt[turn][0] + sh_cnt[turn][1] + sh_cnt[turn][2] + sh_cnt[turn][3];
		turn ^= 1u;
	}
}
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

__global__ __launch_bounds__(LANE_TPB) void k_q_write(QueryArgs q) {
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
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			v[j] = k < it.count ? __builtin_nontemporal_load(s + k) : u32x4{0u, 0u, 0u, 0u};
		}
		uint64_t b[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			b[j] = __ballot(k < it.count && passes(q.g, v[j]));
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
struct RayLayout {
	uint64_t map, par, first, cls, tab, cnt, fill, nfirst, rayParts, rayFirst, items;
	__host__ __device__ RayLayout(uint32_t cap, uint32_t numRays) {
		const uint64_t q = align256(4ull * cap);
		map = 512u; par = map + q; first = par + q; cls = first + align256(4ull * cap + 4u); tab = cls + q;
		cnt = tab + align256(sizeof(SimlodExportNode) * (uint64_t)cap); fill = cnt + q; nfirst = fill + q;
		rayParts = nfirst + align256(8ull * cap + 8u); rayFirst = rayParts + align256(4ull * numRays);
		items = rayFirst + align256(8ull * numRays + 8u);
	}
};

struct RayArgs {
	ExportArgs         x;                // (x.table: the caller's table or `tab`; x.lay: map / par / first / items / itemCap)
	double             min[3], size;
	const SimlodRay*   rays;
	uint32_t           numRays, pad;
	SimlodRayHit*      hits;
	SimlodRayCounts*   counts;
	uint64_t           scratchBytes, cls, cnt, fill, nfirst, rayParts, rayFirst;
};

__global__ __launch_bounds__(WG_TPB) void k_r_hier(RayArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	const ExportArgs& x = a.x;
	hier_walk<false>(x, nullptr, nullptr);
	__syncthreads();
	Header* hdr = reinterpret_cast<Header*>(x.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(x.scratch + x.lay.first);
	uint32_t* cls = reinterpret_cast<uint32_t*>(x.scratch + a.cls);
	uint32_t* cnt = reinterpret_cast<uint32_t*>(x.scratch + a.cnt);
	uint32_t* fill = reinterpret_cast<uint32_t*>(x.scratch + a.fill);
	const uint32_t n = hdr->numListed;
	uint64_t samples = 0, items = 0;
	for (uint32_t base = 0; base < n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		const uint64_t ns = t < n ? x.table[t].numSamples : 0u;
		uint64_t totS, totI;
		const uint64_t offS = block_scan<uint64_t>(ns, totS, sh_scan);
		const uint64_t offI = block_scan<uint64_t>(ceil_chunks(ns), totI, sh_scan);
		if (t < n) { x.table[t].firstSample = samples + offS; first[t] = (uint32_t)(items + offI); cls[t] = Q_COPIED; cnt[t] = 0u; fill[t] = 0u; }
		samples += totS; items += totI;
	}
	if (threadIdx.x == 0) {
		uint32_t err = hdr->error;
		if (items > x.lay.itemCap) err |= SIMLOD_EXPORT_ERR_CAPACITY;
		first[n] = (uint32_t)items;
		hdr->error = err;
		hdr->totalChunks = (err & SIMLOD_EXPORT_ERR_CAPACITY) ? 0u : items;      // the items k_q_dir writes
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
	uint32_t* cnt = reinterpret_cast<uint32_t*>(x.scratch + a.cnt);
	uint32_t* fill = reinterpret_cast<uint32_t*>(x.scratch + a.fill);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + a.nfirst);
	uint32_t* rayParts = reinterpret_cast<uint32_t*>(x.scratch + a.rayParts);
	const uint64_t* rayFirst = reinterpret_cast<const uint64_t*>(x.scratch + a.rayFirst);
	RayD r;
	const bool valid = ray_load(a.rays, ray, r);
	if (!valid) {
		if (!FILL && lane == 0u) { atomicAdd(&rh->numInvalid, 1u); rayParts[ray] = 0u; }
		return;
	}
	const bool countHits = !FILL && a.hits == nullptr;
	const uint64_t below = (1ull << lane) - 1ull;
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
			uint32_t incl = nch;
#pragma unroll
			for (int o = 1; o < SIMLOD_WAVE; o <<= 1) {
				const uint32_t y = __shfl_up(incl, (unsigned)o, SIMLOD_WAVE);
				if ((int)lane >= o) incl += y;
			}
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

	uint32_t myCnt = 0;                                                            // lane L: the nodes pending at level L
	int cur = -1;                                                                  // the deepest level that may have any
	{
		const SimlodExportNode e = x.table[0];
		if (slab(r, a, e.level, e.X, e.Y, e.Z)) {
			if (e.childMask != 0u) {
				if (lane == 0u) { sh_fc[w][0][0] = e.firstChild; sh_mk[w][0][0] = e.childMask; myCnt = 1u; }
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
			const uint32_t fc = sh_fc[w][cur][base + e], mk = sh_mk[w][cur][base + e];
			ci = fc + (uint32_t)__popc(mk & ((1u << k) - 1u));
			has = ((mk >> k) & 1u) != 0u && ci < numListed;
		}
		SimlodExportNode ce{};
		bool pass = false;
		if (has) { ce = x.table[ci]; pass = slab(r, a, ce.level, ce.X, ce.Y, ce.Z); }
		const bool push = pass && ce.childMask != 0u && cur + 1 < (int)RAY_LEVELS;
		const uint64_t pb = __ballot(push);
		__builtin_amdgcn_wave_barrier();
		if (pb != 0ull) {
			// (level cur + 1 was empty: cur is the deepest level with anything pending, so a bucket holds at most these 64)
			if (push) { const uint32_t pos = (uint32_t)__popcll(pb & below); sh_fc[w][cur + 1][pos] = ce.firstChild; sh_mk[w][cur + 1][pos] = ce.childMask; }
			if ((int)lane == cur + 1) myCnt = (uint32_t)__popcll(pb);
			cur++;
		}
		__builtin_amdgcn_wave_barrier();
		on_pairs(pass && ce.numSamples != 0u && (ce.flags & SIMLOD_EXPORT_FLAG_SELECTED) != 0u, ci, ce.numSamples);
	}
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
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + a.cnt);
	uint64_t* nfirst = reinterpret_cast<uint64_t*>(x.scratch + a.nfirst);
	const uint32_t* rayParts = reinterpret_cast<const uint32_t*>(x.scratch + a.rayParts);
	uint64_t* rayFirst = reinterpret_cast<uint64_t*>(x.scratch + a.rayFirst);
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
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(x.scratch + a.cnt);
	const uint64_t* nfirst = reinterpret_cast<const uint64_t*>(x.scratch + a.nfirst);
	const RayPair* pairs = reinterpret_cast<const RayPair*>(x.scratch + rh->pairsOff);
	RayPart* parts = reinterpret_cast<RayPart*>(x.scratch + rh->partsOff);
	const uint64_t numItems = hdr->totalChunks;
	const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x / SIMLOD_WAVE;
	const double INF = __builtin_huge_val();
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const QItem it = items[i];
		const uint32_t c = cnt[it.node];                                           // (the same for the whole workgroup, as every branch on `it`)
		if (c == 0u) continue;
		const u32x4* s = reinterpret_cast<const u32x4*>(it.src);
		double sx[4], sy[4], sz[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			const u32x4 v = k < it.count ? s[k] : u32x4{0u, 0u, 0u, 0u};
			sx[j] = (double)__uint_as_float(v.x); sy[j] = (double)__uint_as_float(v.y); sz[j] = (double)__uint_as_float(v.z);
		}
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
				if (__ballot(bo != NONE) != 0ull) {
#pragma unroll
					for (int o = SIMLOD_WAVE / 2; o > 0; o >>= 1) {
						const double ot = __shfl_xor(bt, o, SIMLOD_WAVE);
						const uint32_t oo = __shfl_xor(bo, o, SIMLOD_WAVE);
						if (hit_less(ot, 0u, oo, bt, 0u, bo)) { bt = ot; bo = oo; }
					}
				}
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
	const uint64_t* rayFirst = reinterpret_cast<const uint64_t*>(x.scratch + a.rayFirst);
	const RayPart* parts = reinterpret_cast<const RayPart*>(x.scratch + rh->partsOff);
	double bt = __builtin_huge_val();
	uint32_t bn = NONE, bo = NONE;
	const uint64_t end = rayFirst[ray + 1u];
	for (uint64_t p = rayFirst[ray] + lane; p < end; p += SIMLOD_WAVE) {
		const RayPart v = parts[p];
		if (v.node != NONE && hit_less(v.t, v.node, v.ordinal, bt, bn, bo)) { bt = v.t; bn = v.node; bo = v.ordinal; }
	}
	if (__ballot(bn != NONE) != 0ull) {
#pragma unroll
		for (int o = SIMLOD_WAVE / 2; o > 0; o >>= 1) {
			const double ot = __shfl_xor(bt, o, SIMLOD_WAVE);
			const uint32_t on = __shfl_xor(bn, o, SIMLOD_WAVE), oo = __shfl_xor(bo, o, SIMLOD_WAVE);
			if (on != NONE && hit_less(ot, on, oo, bt, bn, bo)) { bt = ot; bn = on; bo = oo; }
		}
	}
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

// ---- import -------------------------------------------------------------------------------------------------------------------------
struct ImportArgs {
	const SimlodExportNode* table;
	uint32_t                n;
	const SimlodPoint*      samples;
	uint64_t                numSamples;
	uint8_t*                scratch;
	Layout                  lay;
	uint8_t*                pers;
	uint64_t                persCap;
	SimlodNode*             nodes;
	SimlodStats*            stats;
	// the buildable import (launch_import_buildable): the box as the builder derives it (construct.hip), and what k_reset also writes
	uint32_t                buildable;
	float                   minx, miny, minz, size;
	uint32_t*               numBatchesUploaded;
	uint32_t*               batchSizes;
	uint32_t*               feedback;
	uint32_t                feedbackSeq, frameCounter;
};

__device__ __forceinline__ uint32_t octant_of(const SimlodExportNode& e) { return ((e.X & 1u) << 2) | ((e.Y & 1u) << 1) | (e.Z & 1u); }

__global__ __launch_bounds__(WG_TPB) void k_i_validate(ImportArgs a) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ uint32_t sh_bad;
	__shared__ uint32_t sh_cnt[7];
	__shared__ uint32_t sh_lvFirst[SIMLOD_MAX_DEPTH], sh_lvEnd[SIMLOD_MAX_DEPTH];
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	uint32_t* first = reinterpret_cast<uint32_t*>(a.scratch + a.lay.first);
	uint32_t* gridOf = reinterpret_cast<uint32_t*>(a.scratch + a.lay.map);     // buildable: table index -> grid ordinal (NONE: a leaf below the root)
	if (threadIdx.x < 7) sh_cnt[threadIdx.x] = 0u;
	if (threadIdx.x < (uint32_t)SIMLOD_MAX_DEPTH) { sh_lvFirst[threadIdx.x] = NONE; sh_lvEnd[threadIdx.x] = 0u; }
	if (threadIdx.x == 0) sh_bad = 0u;
	__syncthreads();
	uint64_t samples = 0, chunks = 0, children = 1, grids = 0;        // (the root is nobody's child)
	for (uint32_t base = 0; base < a.n; base += WG_TPB) {
		const uint32_t t = base + threadIdx.x;
		const bool act = t < a.n;
		SimlodExportNode e{};
		bool bad = false;
		if (act) {
			e = a.table[t];
			bad |= e.level > (uint32_t)SIMLOD_MAX_DEPTH || e.reserved != 0 || (e.flags & ~(SIMLOD_EXPORT_FLAG_LEAF | SIMLOD_EXPORT_FLAG_SELECTED)) != 0;
			if (t == 0u) bad |= e.parent != NONE || e.level != 0u || e.X != 0u || e.Y != 0u || e.Z != 0u;
			else if (e.parent >= t) bad = true;
			else {
				// level and coordinates follow from the parent, and the parent lists this entry where its octant says
				const SimlodExportNode p = a.table[e.parent];
				const uint32_t k = octant_of(e);
				bad |= e.level != p.level + 1u || (e.X >> 1) != p.X || (e.Y >> 1) != p.Y || (e.Z >> 1) != p.Z;
				bad |= !(p.childMask & (1u << k)) || p.firstChild == NONE || t != p.firstChild + (uint32_t)__popc(p.childMask & ((1u << k) - 1u));
			}
			if (e.childMask == 0u) bad |= e.firstChild != NONE;
			else bad |= e.firstChild == NONE || e.firstChild <= t || (uint64_t)e.firstChild + (uint32_t)__popc(e.childMask) > a.n || e.level >= (uint32_t)SIMLOD_MAX_DEPTH;
			if (a.buildable) {
				// a full export of an octree the builder made: every sample present, the leaf flag as the children say, eight children or none
				bad |= (e.flags & SIMLOD_EXPORT_FLAG_SELECTED) == 0u || ((e.flags & SIMLOD_EXPORT_FLAG_LEAF) != 0u) != (e.childMask == 0u);
				bad |= e.childMask != 0u && e.childMask != 0xffu;
				if (e.level < (uint32_t)SIMLOD_MAX_DEPTH) { atomicMin(&sh_lvFirst[e.level], t); atomicMax(&sh_lvEnd[e.level], t + 1u); }
			}
		}
		const uint64_t kids = (uint64_t)__popc(e.childMask), ns = act ? e.numSamples : 0u, nch = act ? ceil_chunks(ns) : 0u;
		const bool hasGrid = act && a.buildable != 0u && (t == 0u || e.childMask != 0u);
		uint64_t totK, totS, totC, totG;
		const uint64_t offK = block_scan<uint64_t>(kids, totK, sh_scan);
		const uint64_t offS = block_scan<uint64_t>(ns, totS, sh_scan);
		const uint64_t offC = block_scan<uint64_t>(nch, totC, sh_scan);
		const uint64_t offG = block_scan<uint64_t>(hasGrid ? 1u : 0u, totG, sh_scan);
		if (act && a.buildable) gridOf[t] = hasGrid ? (uint32_t)(grids + offG) : NONE;
		if (act) {
			// breadth-first order: an entry's children come right after the children of the entries before it
			if (e.childMask != 0u) bad |= (uint64_t)e.firstChild != children + offK;
			bad |= e.firstSample != samples + offS;
			if (samples + offS + ns <= a.numSamples && chunks + offC < a.lay.itemCap) first[t] = (uint32_t)(chunks + offC);
			const bool leaf = e.childMask == 0u;
			const uint32_t c[7] = {leaf ? 0u : 1u, leaf ? 1u : 0u, leaf && ns > 0u ? 1u : 0u, leaf ? (uint32_t)ns : 0u, leaf ? 0u : (uint32_t)ns,
			                       leaf ? (uint32_t)nch : 0u, leaf ? 0u : (uint32_t)nch};
			for (int q = 0; q < 7; q++) if (c[q] != 0u) atomicAdd(&sh_cnt[q], c[q]);
		}
		if (bad) atomicOr(&sh_bad, 1u);
		children += totK; samples += totS; chunks += totC; grids += totG;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		bool bad = sh_bad != 0u || a.n == 0u || children != a.n || samples != a.numSamples || chunks > a.lay.itemCap;
		// persistent layout: the chunks, then (buildable) the grids, then the voxel list of a root that is still a leaf (<= one voxel per point)
		uint64_t end = CHUNK_BASE + chunks * CHUNK_STRIDE;
		hdr->gridBase = end;
		if (a.buildable) {
			end += grids * GRID_STRIDE;
			hdr->rootVoxBase = end;
			if (a.n != 0u && a.table[0].childMask == 0u) end += (uint64_t)ceil_chunks(a.table[0].numSamples) * CHUNK_STRIDE;
		}
		bad |= end > a.persCap;
		hdr->ok = bad ? 0u : 1u;
		hdr->numItems = bad ? 0u : chunks;
		hdr->totalChunks = chunks;
		hdr->numGrids = (uint32_t)grids; hdr->gridBad = 0u; hdr->rootVoxels = 0u;
		for (int l = 0; l < SIMLOD_MAX_DEPTH; l++) { hdr->lvFirst[l] = sh_lvFirst[l]; hdr->lvEnd[l] = sh_lvEnd[l]; }
		for (int q = 0; q < 7; q++) hdr->counts[q] = sh_cnt[q];
		if (bad) a.stats->dbg |= SIMLOD_ERR_IMPORT;
		else first[a.n] = (uint32_t)chunks;
	}
}

__global__ __launch_bounds__(LANE_TPB) void k_i_nodes(ImportArgs a) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const uint32_t t = blockIdx.x * LANE_TPB + threadIdx.x;
	if (t >= a.n || hdr->ok == 0u) return;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.first);
	CopyItem* items = reinterpret_cast<CopyItem*>(a.scratch + a.lay.items);
	const SimlodExportNode e = a.table[t];
	const bool leaf = e.childMask == 0u;
	const uint32_t ns = e.numSamples, nch = ceil_chunks(ns), f = first[t];
	SimlodChunk* head = ns != 0u ? reinterpret_cast<SimlodChunk*>(a.pers + CHUNK_BASE + (uint64_t)f * CHUNK_STRIDE) : nullptr;
	SimlodNode nd;
	uint32_t r = 0;
	for (int k = 0; k < 8; k++) nd.children[k] = (e.childMask & (1u << k)) ? a.nodes + e.firstChild + r++ : nullptr;
	nd.counter = leaf ? ns : 0u;
	nd.numPoints = leaf ? ns : 0u;
	nd.level = e.level; nd.X = e.X; nd.Y = e.Y; nd.Z = e.Z;
	nd.countIteration = 0u; nd.countFlag = 0u;
	// 'r' and one digit per level below the root, the octant the path takes there (construct_expand.inc: the builder's names)
	for (int k = 0; k < 20; k++) nd.name[k] = 0;
	nd.name[0] = 'r';
	for (uint32_t l = 1; l <= e.level && l < 20u; l++) {
		const uint32_t s = e.level - l;
		nd.name[l] = (uint8_t)('0' + ((((e.X >> s) & 1u) << 2) | (((e.Y >> s) & 1u) << 1) | ((e.Z >> s) & 1u)));
	}
	nd.visible = 0; nd.isFiltered = 0; nd.isLeaf = 0; nd.isLarge = 0;
	nd.grid = nullptr;
	if (a.buildable) {
		const uint32_t g = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.map)[t];
		if (g != NONE) nd.grid = reinterpret_cast<SimlodOccupancyGrid*>(a.pers + hdr->gridBase + (uint64_t)g * GRID_STRIDE);
	}
	nd.points = leaf ? head : nullptr;
	nd.voxelChunks = leaf ? nullptr : head;
	nd.numVoxels = leaf ? 0u : ns;
	nd.numVoxelsStored = nd.numVoxels;
	a.nodes[t] = nd;
	// the list: consecutive chunks, `next` as the builder leaves it (the last one NULL), the head's size / padding_0 the tail's address
	// (construct_begin.inc tail_of), the other chunks' 0
	const uint64_t src0 = reinterpret_cast<uint64_t>(a.samples + e.firstSample);
	for (uint32_t k = 0; k < nch; k++) {
		SimlodChunk* c = reinterpret_cast<SimlodChunk*>(a.pers + CHUNK_BASE + (uint64_t)(f + k) * CHUNK_STRIDE);
		c->next = k + 1u < nch ? reinterpret_cast<SimlodChunk*>(reinterpret_cast<uint8_t*>(c) + CHUNK_STRIDE) : nullptr;
		*reinterpret_cast<uint64_t*>(&c->size) = k == 0u ? reinterpret_cast<uint64_t>(a.pers + CHUNK_BASE + (uint64_t)(f + nch - 1u) * CHUNK_STRIDE) : 0ull;
		CopyItem it;
		it.src = src0 + (uint64_t)k * SIMLOD_POINTS_PER_CHUNK * sizeof(SimlodPoint);
		it.dst = reinterpret_cast<uint64_t>(c->points);
		it.count = min(ns - k * SIMLOD_POINTS_PER_CHUNK, SIMLOD_POINTS_PER_CHUNK);
		it.pad0 = 0; it.pad1 = 0;
		items[f + k] = it;
	}
}

__global__ void k_i_finish(ImportArgs a) {
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	// buildable: what the next kernel_construct launch is sized by (simlod_hip.cpp launch_plan), as k_reset reports it — nothing ingested, nothing uploaded
	if (a.buildable && a.feedback != nullptr) {
		a.feedback[0] = 0u; a.feedback[1] = 0u; a.feedback[2] = 1u;
		__hip_atomic_store(a.feedback + 3, a.feedbackSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
	if (hdr->ok == 0u) return;
	const uint32_t rootVoxChunks = ceil_chunks(hdr->rootVoxels);
	SimlodAllocatorGlobal* alloc = reinterpret_cast<SimlodAllocatorGlobal*>(a.pers);
	alloc->buffer = a.pers;
	alloc->offset = a.buildable ? hdr->rootVoxBase + (uint64_t)rootVoxChunks * CHUNK_STRIDE : CHUNK_BASE + hdr->totalChunks * CHUNK_STRIDE;
	SimlodStats s{};
	s.numNodes = a.n;
	s.numInner = hdr->counts[0]; s.numLeaves = hdr->counts[1]; s.numNonemptyLeaves = hdr->counts[2];
	// (the voxels of a root that is still a leaf are not counted: the builder's Stats count the lists of inner nodes only)
	s.numPoints = hdr->counts[3]; s.numVoxels = hdr->counts[4];
	s.numChunksPoints = hdr->counts[5]; s.numChunksVoxels = hdr->counts[6];
	s.allocatedBytes_persistent = alloc->offset;
	if (a.buildable) {
		// the builder's counters start as after a reset (batchletIndex, numPointsProcessed: 0), with an empty recycle stack: numAllocatedChunks is the
		// stack pointer a split returns its leaf's chunks below (voxels.cu:346-357), so it counts the point chunks in use, and chunkPoolSize (its
		// high-water mark) equals it — 0 would send the first split's chunks below the stack's bottom (SIMLOD_ERR_CHUNK_QUEUE_OVERFLOW)
		s.numAllocatedChunks = hdr->counts[5]; s.chunkPoolSize = hdr->counts[5];
		s.frameID = a.frameCounter;
		s.dbg = hdr->gridBad != 0u ? SIMLOD_ERR_IMPORT_GRID : 0u;
		*a.numBatchesUploaded = 0u;
		for (uint32_t k = 0; k < SIMLOD_BATCH_STREAM_SIZE; k++) a.batchSizes[k] = 0u;
	}
	*a.stats = s;
}

// ---- the buildable import's occupancy grids ------------------------------------------------------------------------------------------
// The grid of a node is the set of its level's cells of every point below it (every point samples every node on its path that has a grid,
// voxels.cu:449-469; a node that splits re-samples all its points, :362-381; the root's grid is cleared and re-sampled at its split).  A child
// covers one 64^3 octant of its parent's 128^3 grid (8 192 words): the node grid is the fp32 quotient of quantize(F_FULL) scaled by an exact
// power of two, so the bit below which a point files at level L + 1 is the top bit of its cell at level L — the max face included (2^28 on an
// axis: cell 0, node coordinate 0).  So every word of a parent's grid is written by exactly one of its eight children, with plain stores:
//   k_i_gleaf   a leaf's octant from its points, built in LDS (one workgroup per table entry; inner entries leave at once)
//   k_i_gdown   per level, deepest first: an inner node's finished grid, 2x2x2 cells -> one, into its octant of the parent's grid; its popcount
//               against its voxel count on the way (one workgroup per node)
//   k_i_groot   the root: the popcount check of an inner root; a root that is still a leaf gets its grid and its voxel list from its points
constexpr uint32_t G_TPB = 256;
constexpr uint32_t OCT_WORDS = SIMLOD_GRID_NUM_WORDS / 8u;                        // 8 192 words: one octant of a grid, two words per row of 64 cells
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t* grid_of(const ImportArgs& a, const Header* hdr, uint32_t t) {
	const uint32_t g = reinterpret_cast<const uint32_t*>(a.scratch + a.lay.map)[t];
	return reinterpret_cast<uint32_t*>(a.pers + hdr->gridBase + (uint64_t)g * GRID_STRIDE);
}
// word w of an octant (w = xw | ly << 1 | lz << 7) -> its word in the grid whose octant (ox, oy, oz) it is (cell = x + 128 y + 128^2 z)
__device__ __forceinline__ uint32_t octant_word(uint32_t w, uint32_t ox, uint32_t oy, uint32_t oz) {
	return ox * 2u + (w & 1u) + 4u * (oy * 64u + ((w >> 1) & 63u)) + 512u * (oz * 64u + (w >> 7));
}
// bit i (< 16) = bit 2i | bit 2i + 1 of v: 32 cells of a row -> the 16 cells of the level above
__device__ __forceinline__ uint32_t squeeze(uint32_t v) {
	v = (v | (v >> 1)) & 0x55555555u;
	v = (v | (v >> 1)) & 0x33333333u;
	v = (v | (v >> 2)) & 0x0f0f0f0fu;
	v = (v | (v >> 4)) & 0x00ff00ffu;
	return (v | (v >> 8)) & 0x0000ffffu;
}

__global__ __launch_bounds__(G_TPB) void k_i_gleaf(ImportArgs a) {
	__shared__ uint32_t oct[OCT_WORDS];
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const uint32_t t = blockIdx.x;
	if (hdr->ok == 0u || t == 0u || t >= a.n) return;
	const SimlodExportNode e = a.table[t];
	if (e.childMask != 0u) return;
	for (uint32_t w = threadIdx.x; w < OCT_WORDS; w += G_TPB) oct[w] = 0u;
	__syncthreads();
	// the cell in the PARENT's grid (level e.level - 1): grid_cell() of construct_voxelize.inc, the builder's quantisation (k_voxelize)
	const uint32_t shf = (uint32_t)(SIMLOD_MAX_DEPTH + 2) - e.level;
	const uint32_t ox = e.X & 1u, oy = e.Y & 1u, oz = e.Z & 1u;
	const float4* pts = reinterpret_cast<const float4*>(a.samples + e.firstSample);
	const uint32_t n = e.numSamples;
	for (uint32_t i0 = 0; i0 < n; i0 += 4u * G_TPB) {
		float4 p[4];
#pragma unroll
		for (uint32_t j = 0; j < 4u; j++) {
			const uint32_t i = i0 + j * G_TPB + threadIdx.x;
			p[j] = i < n ? pts[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		}
#pragma unroll
		for (uint32_t j = 0; j < 4u; j++) {
			if (i0 + j * G_TPB + threadIdx.x >= n) continue;
			const uint32_t cx = (quantize(F_FULL, p[j].x, a.minx, a.size) >> shf) & 127u;
			const uint32_t cy = (quantize(F_FULL, p[j].y, a.miny, a.size) >> shf) & 127u;
			const uint32_t cz = (quantize(F_FULL, p[j].z, a.minz, a.size) >> shf) & 127u;
			// (a cell outside the leaf's octant is not the builder's either: dropped, and the parent's popcount check reports the octree)
			if ((cx >> 6) != ox || (cy >> 6) != oy || (cz >> 6) != oz) continue;
			const uint32_t lx = cx & 63u;
			atomicOr(&oct[(lx >> 5) | ((cy & 63u) << 1) | ((cz & 63u) << 7)], 1u << (lx & 31u));
		}
	}
	__syncthreads();
	uint32_t* parent = grid_of(a, hdr, e.parent);
	for (uint32_t k = threadIdx.x; k < OCT_WORDS / 2u; k += G_TPB) {
		u32x2 v;
		v.x = oct[2u * k]; v.y = oct[2u * k + 1u];
		*reinterpret_cast<u32x2*>(parent + octant_word(2u * k, ox, oy, oz)) = v;
	}
}

__global__ __launch_bounds__(G_TPB) void k_i_gdown(ImportArgs a, uint32_t level) {
	__shared__ uint32_t sh_pop;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	if (hdr->ok == 0u) return;
	const uint32_t lo = hdr->lvFirst[level], hi = min(hdr->lvEnd[level], a.n);
	for (uint32_t t = lo + blockIdx.x; t < hi; t += gridDim.x) {
		const SimlodExportNode e = a.table[t];
		if (e.childMask == 0u) continue;                                   // (the same for the whole workgroup)
		const uint32_t* child = grid_of(a, hdr, t);
		uint32_t* parent = grid_of(a, hdr, e.parent);
		const uint32_t ox = e.X & 1u, oy = e.Y & 1u, oz = e.Z & 1u;
		if (threadIdx.x == 0) sh_pop = 0u;
		__syncthreads();
		uint32_t pop = 0;
		// output word w: cells xw * 32 .. + 31 of row (ly, lz) of the octant <- child words 2 xw, 2 xw + 1 of rows (2 ly + {0, 1}, 2 lz + {0, 1});
		// four outputs per lane and turn, their 16 loads in flight together
		for (uint32_t w0 = 0; w0 < OCT_WORDS; w0 += 4u * G_TPB) {
			u32x2 r[4][4];
#pragma unroll
			for (uint32_t j = 0; j < 4u; j++) {
				const uint32_t w = w0 + j * G_TPB + threadIdx.x, xw = w & 1u, ly = (w >> 1) & 63u, lz = w >> 7;
#pragma unroll
				for (uint32_t q = 0; q < 4u; q++)
					r[j][q] = *reinterpret_cast<const u32x2*>(child + 2u * xw + 4u * (2u * ly + (q & 1u)) + 512u * (2u * lz + (q >> 1)));
			}
#pragma unroll
			for (uint32_t j = 0; j < 4u; j++) {
				const uint32_t w = w0 + j * G_TPB + threadIdx.x;
				const uint32_t lo32 = r[j][0].x | r[j][1].x | r[j][2].x | r[j][3].x, hi32 = r[j][0].y | r[j][1].y | r[j][2].y | r[j][3].y;
#pragma unroll
				for (uint32_t q = 0; q < 4u; q++) pop += (uint32_t)__popc(r[j][q].x) + (uint32_t)__popc(r[j][q].y);
				parent[octant_word(w, ox, oy, oz)] = squeeze(lo32) | (squeeze(hi32) << 16);
			}
		}
		atomicAdd(&sh_pop, pop);
		__syncthreads();
		// a non-root inner node: one voxel per occupied cell (oracle_check_invariants rule 12)
		if (threadIdx.x == 0 && sh_pop != e.numSamples) atomicOr(&hdr->gridBad, 1u);
		__syncthreads();
	}
}
static_assert(OCT_WORDS % (4u * G_TPB) == 0u, "k_i_gdown: whole turns");

// The root.  Inner: its grid is complete (k_i_gdown of level 1); it may hold duplicate voxels (its grid was cleared when it split), so its
// popcount is at most its voxel count.  A leaf: its grid in 16 slabs of 8 z-layers (4 096 words) built in LDS from its points, and its voxel
// list, which the export does not carry: one voxel per occupied cell in ascending cell order (slot = cells before it), at the cell centre
// (voxel_centre, the builder's formula), coloured by the cell's lowest-index point (atomicMin of the point index into the slot's colour word,
// then the index replaced by that point's colour).  One workgroup: a root that is a leaf holds a few ten thousand points.
constexpr uint32_t R_TPB = WG_TPB, SLAB_WORDS = 4096u, SLABS = SIMLOD_GRID_NUM_WORDS / SLAB_WORDS;
static_assert(SLAB_WORDS == 4u * R_TPB, "k_i_groot: four words per lane and slab");

__device__ __forceinline__ SimlodPoint* root_voxel(const ImportArgs& a, const Header* hdr, uint32_t rank) {
	SimlodChunk* c = reinterpret_cast<SimlodChunk*>(a.pers + hdr->rootVoxBase + (uint64_t)(rank / SIMLOD_POINTS_PER_CHUNK) * CHUNK_STRIDE);
	return &c->points[rank % SIMLOD_POINTS_PER_CHUNK];
}

__global__ __launch_bounds__(R_TPB) void k_i_groot(ImportArgs a) {
	__shared__ uint32_t occ[SLAB_WORDS], pre[SLAB_WORDS];
	__shared__ uint32_t sh_scan[WG_WAVES];
	__shared__ uint32_t sh_pop;
	Header* hdr = reinterpret_cast<Header*>(a.scratch);
	if (hdr->ok == 0u) return;
	const SimlodExportNode r = a.table[0];
	uint32_t* grid = grid_of(a, hdr, 0u);
	if (r.childMask != 0u) {
		if (threadIdx.x == 0) sh_pop = 0u;
		__syncthreads();
		uint32_t pop = 0;
		const uint4* g4 = reinterpret_cast<const uint4*>(grid);
		for (uint32_t w = threadIdx.x; w < SIMLOD_GRID_NUM_WORDS / 4u; w += R_TPB) {
			const uint4 v = g4[w];
			pop += (uint32_t)(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w));
		}
		atomicAdd(&sh_pop, pop);
		__syncthreads();
		if (threadIdx.x == 0 && sh_pop > r.numSamples) atomicOr(&hdr->gridBad, 1u);
		return;
	}
	const uint32_t n = r.numSamples;
	const float4* pts = reinterpret_cast<const float4*>(a.samples + r.firstSample);
	const uint32_t* colors = reinterpret_cast<const uint32_t*>(pts) + 3;             // SimlodPoint.color: the fourth word
	uint32_t base = 0;                                                                 // voxels of the slabs before
	for (uint32_t s = 0; s < SLABS; s++) {
		for (uint32_t w = threadIdx.x; w < SLAB_WORDS; w += R_TPB) occ[w] = 0u;
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < n; i += R_TPB) {
			const float4 p = pts[i];
			const uint32_t cell = ((quantize(F_FULL, p.x, a.minx, a.size) >> 21) & 127u) + ((quantize(F_FULL, p.y, a.miny, a.size) >> 21) & 127u) * 128u +
			                      ((quantize(F_FULL, p.z, a.minz, a.size) >> 21) & 127u) * 16384u;
			if ((cell >> 5) / SLAB_WORDS == s) atomicOr(&occ[(cell >> 5) % SLAB_WORDS], 1u << (cell & 31u));
		}
		__syncthreads();
		const uint32_t w0 = 4u * threadIdx.x;
		const uint4 mine = make_uint4(occ[w0], occ[w0 + 1u], occ[w0 + 2u], occ[w0 + 3u]);
		reinterpret_cast<uint4*>(grid)[(s * SLAB_WORDS + w0) / 4u] = mine;
		const uint32_t c0 = (uint32_t)__popc(mine.x), c1 = (uint32_t)__popc(mine.y), c2 = (uint32_t)__popc(mine.z), c3 = (uint32_t)__popc(mine.w);
		uint32_t total;
		const uint32_t off = base + block_scan<uint32_t>(c0 + c1 + c2 + c3, total, sh_scan);
		pre[w0] = off; pre[w0 + 1u] = off + c0; pre[w0 + 2u] = off + c0 + c1; pre[w0 + 3u] = off + c0 + c1 + c2;
		// the slab's voxels at their cell centres, colour word = "no point yet"
		const uint32_t words[4] = {mine.x, mine.y, mine.z, mine.w};
		for (uint32_t k = 0; k < 4u; k++) {
			uint32_t bits = words[k], rank = pre[w0 + k];
			while (bits != 0u) {
				const uint32_t b = (uint32_t)__ffs((int)bits) - 1u;
				bits &= bits - 1u;
				const uint32_t cell = (s * SLAB_WORDS + w0 + k) * 32u + b;
				const float4 v = voxel_centre(a.size, a.minx, a.miny, a.minz, 0, 0u, 0u, 0u, cell & 127u, (cell >> 7) & 127u, cell >> 14, 0.0f);
				SimlodPoint* o = root_voxel(a, hdr, rank++);
				o->x = v.x; o->y = v.y; o->z = v.z; o->color = 0xffffffffu;
			}
		}
		__threadfence();
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < n; i += R_TPB) {
			const float4 p = pts[i];
			const uint32_t cell = ((quantize(F_FULL, p.x, a.minx, a.size) >> 21) & 127u) + ((quantize(F_FULL, p.y, a.miny, a.size) >> 21) & 127u) * 128u +
			                      ((quantize(F_FULL, p.z, a.minz, a.size) >> 21) & 127u) * 16384u;
			if ((cell >> 5) / SLAB_WORDS != s) continue;
			const uint32_t w = (cell >> 5) % SLAB_WORDS, below = occ[w] & ((1u << (cell & 31u)) - 1u);
			atomicMin(&root_voxel(a, hdr, pre[w] + (uint32_t)__popc(below))->color, i);
		}
		__threadfence();
		__syncthreads();
		for (uint32_t k = base + threadIdx.x; k < base + total; k += R_TPB) {
			SimlodPoint* o = root_voxel(a, hdr, k);
			const uint32_t idx = __hip_atomic_load(&o->color, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			o->color = idx < n ? colors[4u * (uint64_t)idx] : 0u;          // (every occupied cell has a point: idx < n)
		}
		base += total;
		__syncthreads();                          // (occ and pre are the next slab's)
	}
	// the list: consecutive chunks, `next` as the builder leaves it, the head's spare word the tail's address (k_i_nodes)
	const uint32_t nch = ceil_chunks(base);
	for (uint32_t k = threadIdx.x; k < nch; k += R_TPB) {
		SimlodChunk* c = reinterpret_cast<SimlodChunk*>(a.pers + hdr->rootVoxBase + (uint64_t)k * CHUNK_STRIDE);
		c->next = k + 1u < nch ? reinterpret_cast<SimlodChunk*>(reinterpret_cast<uint8_t*>(c) + CHUNK_STRIDE) : nullptr;
		*reinterpret_cast<uint64_t*>(&c->size) = k == 0u ? reinterpret_cast<uint64_t>(a.pers + hdr->rootVoxBase + (uint64_t)(nch - 1u) * CHUNK_STRIDE) : 0ull;
	}
	if (threadIdx.x == 0) {
		SimlodNode* root = a.nodes;
		root->numVoxels = base; root->numVoxelsStored = base;
		root->voxelChunks = base != 0u ? reinterpret_cast<SimlodChunk*>(a.pers + hdr->rootVoxBase) : nullptr;
		hdr->rootVoxels = base;
	}
}

uint32_t copy_grid(uint64_t itemCap) {
	const uint64_t g = (uint64_t)device_info().numCUs * 8u;                 // 8 workgroups of 256 lanes per CU
	return (uint32_t)(itemCap < g ? (itemCap == 0u ? 1u : itemCap) : g);
}

}  // namespace

uint64_t export_min_bytes(uint32_t nodeCapacity, uint64_t sampleCapacity) { return Layout(nodeCapacity, sampleCapacity).bytes; }

int launch_export(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                  SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity, SimlodExportCounts* counts, hipStream_t stream) {
	if (nodes == nullptr || stats == nullptr || scratch == nullptr || table == nullptr || counts == nullptr || (samples == nullptr && sampleCapacity != 0u))
		return (int)hipErrorInvalidValue;
	if (select > SIMLOD_EXPORT_VISIBLE || scratchBytes < export_min_bytes(tableCapacity, sampleCapacity)) return (int)hipErrorInvalidValue;
	if (select == SIMLOD_EXPORT_VISIBLE && !array_state(ctx, nodes).rendered) return (int)hipErrorInvalidValue;
	ExportArgs a{};
	a.nodes = nodes; a.stats = stats; a.maxLevel = maxLevel; a.select = select; a.cap = tableCapacity;
	a.scratch = reinterpret_cast<uint8_t*>(scratch); a.table = table; a.samples = samples; a.sampleCap = sampleCapacity; a.counts = counts;
	a.lay = Layout(tableCapacity, sampleCapacity);
	LeafTableRef lt;
	if (find_leaf_table(ctx, nodes, lt) && lt.slots <= LEAF_ROW_SLOTS) {
		a.lt = lt.table; a.ltPers = lt.pers; a.ltMagic = lt.magic; a.ltBatch = lt.batch; a.ltNodes = lt.tableNodes; a.ltSig = lt.sig;
		a.ltMagicValue = lt.magicValue; a.ltSlots = lt.slots; a.ltRows = lt.rows;
	}
	SIMLOD_LAUNCH(k_x_hier, dim3(1), dim3(WG_TPB), stream, a);
	SIMLOD_LAUNCH(k_x_scan, dim3(1), dim3(WG_TPB), stream, a);
	if (tableCapacity != 0u) SIMLOD_LAUNCH(k_x_dir, dim3((tableCapacity + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, a);
	SIMLOD_LAUNCH(k_copy, dim3(copy_grid(a.lay.itemCap)), dim3(LANE_TPB), stream, (const uint8_t*)a.scratch, a.lay.items);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t query_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound) {
	return query_fixed_bytes(nodeCapacity) + (sampleBound / SIMLOD_POINTS_PER_CHUNK + nodeCapacity + 1u) * sizeof(QItem);
}

int launch_query(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRegion* region, uint32_t maxLevel,
                 uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples,
                 uint64_t sampleCapacity, SimlodQueryCounts* counts, hipStream_t stream) {
	if (nodes == nullptr || stats == nullptr || u == nullptr || region == nullptr || scratch == nullptr || table == nullptr || counts == nullptr)
		return (int)hipErrorInvalidValue;
	if (region->numPlanes > SIMLOD_REGION_MAX_PLANES || region->reserved[0] != 0u || region->reserved[1] != 0u || region->reserved[2] != 0u)
		return (int)hipErrorInvalidValue;
	if ((select != SIMLOD_EXPORT_ALL && select != SIMLOD_EXPORT_CUT) || scratchBytes < query_min_bytes(tableCapacity, 0u)) return (int)hipErrorInvalidValue;
	QueryArgs q{};
	for (uint32_t p = 0; p < region->numPlanes; p++)
		for (int k = 0; k < 4; k++) {
			if (!std::isfinite(region->planes[p][k])) return (int)hipErrorInvalidValue;
			q.g.pl[p][k] = (double)region->planes[p][k];
		}
	q.g.numPlanes = region->numPlanes;
	// the box as kernel_construct derives it (construct.hip launch_construct, voxels.cu:860-863)
	const float bx = u->boxMax.x - u->boxMin.x, by = u->boxMax.y - u->boxMin.y, bz = u->boxMax.z - u->boxMin.z;
	q.g.size = (double)fmaxf(fmaxf(bx, by), bz);
	q.g.min[0] = (double)u->boxMin.x; q.g.min[1] = (double)u->boxMin.y; q.g.min[2] = (double)u->boxMin.z;
	ExportArgs& a = q.x;
	a.nodes = nodes; a.stats = stats; a.maxLevel = maxLevel; a.select = select; a.cap = tableCapacity;
	a.scratch = reinterpret_cast<uint8_t*>(scratch); a.table = table; a.samples = samples; a.sampleCap = sampleCapacity;
	const uint64_t quarter = align256(4ull * tableCapacity);
	a.lay.map = 256u; a.lay.par = a.lay.map + quarter; a.lay.first = a.lay.par + quarter;
	q.cls = a.lay.first + align256(4ull * tableCapacity + 4u);
	a.lay.items = q.cls + quarter;
	a.lay.itemCap = std::min<uint64_t>((scratchBytes - a.lay.items) / sizeof(QItem), 0xffffffffull);
	a.lay.bytes = a.lay.items + a.lay.itemCap * sizeof(QItem);
	q.counts = counts;
	LeafTableRef lt;
	if (find_leaf_table(ctx, nodes, lt) && lt.slots <= LEAF_ROW_SLOTS) {
		a.lt = lt.table; a.ltPers = lt.pers; a.ltMagic = lt.magic; a.ltBatch = lt.batch; a.ltNodes = lt.tableNodes; a.ltSig = lt.sig;
		a.ltMagicValue = lt.magicValue; a.ltSlots = lt.slots; a.ltRows = lt.rows;
	}
	const uint32_t grid = copy_grid(a.lay.itemCap);
	SIMLOD_LAUNCH(k_q_hier, dim3(1), dim3(WG_TPB), stream, q);
	constexpr uint32_t perWg = LANE_TPB / SIMLOD_WAVE;                        // k_q_dir: one wave per table entry
	if (tableCapacity != 0u) SIMLOD_LAUNCH(k_q_dir, dim3((tableCapacity + perWg - 1u) / perWg), dim3(LANE_TPB), stream, q);
	SIMLOD_LAUNCH(k_q_count, dim3(grid), dim3(LANE_TPB), stream, q);
	SIMLOD_LAUNCH(k_q_scan, dim3(1), dim3(WG_TPB), stream, q);
	if (samples != nullptr) SIMLOD_LAUNCH(k_q_write, dim3(grid), dim3(LANE_TPB), stream, q);
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

uint64_t rays_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound, uint32_t numRays, uint64_t numPairs, uint64_t numCandidates) {
	return RayLayout(nodeCapacity, numRays).items + (sampleBound / SIMLOD_POINTS_PER_CHUNK + nodeCapacity + 1u) * sizeof(QItem) +
	       numPairs * (sizeof(RayPair) + sizeof(RayPart)) + (numCandidates / SIMLOD_POINTS_PER_CHUNK) * sizeof(RayPart);
}

int launch_rays(Context& ctx, const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* u, const SimlodRay* rays, uint32_t numRays,
                uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity,
                SimlodRayHit* hits, SimlodRayCounts* counts, hipStream_t stream) {
	if (nodes == nullptr || stats == nullptr || u == nullptr || rays == nullptr || scratch == nullptr || counts == nullptr) return (int)hipErrorInvalidValue;
	if (numRays == 0u || numRays > SIMLOD_RAYS_MAX || select > SIMLOD_EXPORT_VISIBLE) return (int)hipErrorInvalidValue;
	if (scratchBytes < rays_min_bytes(tableCapacity, 0u, numRays, 0u, 0u)) return (int)hipErrorInvalidValue;
	if (select == SIMLOD_EXPORT_VISIBLE && !array_state(ctx, nodes).rendered) return (int)hipErrorInvalidValue;
	const RayLayout rl(tableCapacity, numRays);
	RayArgs r{};
	ExportArgs& a = r.x;
	a.nodes = nodes; a.stats = stats; a.maxLevel = maxLevel; a.select = select; a.cap = tableCapacity;
	a.scratch = reinterpret_cast<uint8_t*>(scratch);
	a.table = table != nullptr ? table : reinterpret_cast<SimlodExportNode*>(a.scratch + rl.tab);
	a.lay.map = rl.map; a.lay.par = rl.par; a.lay.first = rl.first; a.lay.items = rl.items;
	a.lay.itemCap = std::min<uint64_t>((scratchBytes - rl.items) / sizeof(QItem), 0xffffffffull);
	a.lay.bytes = scratchBytes;
	// the box as kernel_construct derives it (construct.hip launch_construct, voxels.cu:860-863)
	const float bx = u->boxMax.x - u->boxMin.x, by = u->boxMax.y - u->boxMin.y, bz = u->boxMax.z - u->boxMin.z;
	r.size = (double)fmaxf(fmaxf(bx, by), bz);
	r.min[0] = (double)u->boxMin.x; r.min[1] = (double)u->boxMin.y; r.min[2] = (double)u->boxMin.z;
	r.rays = rays; r.numRays = numRays; r.hits = hits; r.counts = counts; r.scratchBytes = scratchBytes;
	r.cls = rl.cls; r.cnt = rl.cnt; r.fill = rl.fill; r.nfirst = rl.nfirst; r.rayParts = rl.rayParts; r.rayFirst = rl.rayFirst;
	LeafTableRef lt;
	if (find_leaf_table(ctx, nodes, lt) && lt.slots <= LEAF_ROW_SLOTS) {
		a.lt = lt.table; a.ltPers = lt.pers; a.ltMagic = lt.magic; a.ltBatch = lt.batch; a.ltNodes = lt.tableNodes; a.ltSig = lt.sig;
		a.ltMagicValue = lt.magicValue; a.ltSlots = lt.slots; a.ltRows = lt.rows;
	}
	QueryArgs q{};                                                              // k_q_dir's view of the same buffers
	q.x = a; q.cls = rl.cls;
	const uint32_t rayGrid = (numRays + RAY_WAVES - 1u) / RAY_WAVES;
	SIMLOD_LAUNCH(k_r_hier, dim3(1), dim3(WG_TPB), stream, r);
	constexpr uint32_t perWg = LANE_TPB / SIMLOD_WAVE;                          // k_q_dir: one wave per table entry
	if (tableCapacity != 0u) SIMLOD_LAUNCH(k_q_dir, dim3((tableCapacity + perWg - 1u) / perWg), dim3(LANE_TPB), stream, q);
	SIMLOD_LAUNCH(k_r_pairs<0>, dim3(rayGrid), dim3(LANE_TPB), stream, r);
	SIMLOD_LAUNCH(k_r_scan, dim3(1), dim3(WG_TPB), stream, r);
	if (hits != nullptr) {
		SIMLOD_LAUNCH(k_r_pairs<1>, dim3(rayGrid), dim3(LANE_TPB), stream, r);
		SIMLOD_LAUNCH(k_r_test, dim3(copy_grid(a.lay.itemCap)), dim3(LANE_TPB), stream, r);
		SIMLOD_LAUNCH(k_r_reduce, dim3(rayGrid), dim3(LANE_TPB), stream, r);
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

int launch_import(Context& ctx, const SimlodExportNode* table, uint32_t numNodes, const SimlodPoint* samples, uint64_t numSamples, void* scratch,
                  uint64_t scratchBytes, uint8_t* pers, uint64_t persCapacity, SimlodNode* nodes, SimlodStats* stats, hipStream_t stream) {
	if (table == nullptr || scratch == nullptr || pers == nullptr || nodes == nullptr || stats == nullptr || (samples == nullptr && numSamples != 0u))
		return (int)hipErrorInvalidValue;
	if (numNodes == 0u || numNodes > ctx.nodeCapacity.load() || scratchBytes < export_min_bytes(numNodes, numSamples)) return (int)hipErrorInvalidValue;
	ImportArgs a{};
	a.table = table; a.n = numNodes; a.samples = samples; a.numSamples = numSamples; a.scratch = reinterpret_cast<uint8_t*>(scratch);
	a.lay = Layout(numNodes, numSamples); a.pers = pers; a.persCap = persCapacity; a.nodes = nodes; a.stats = stats;
	SIMLOD_LAUNCH(k_i_validate, dim3(1), dim3(WG_TPB), stream, a);
	SIMLOD_LAUNCH(k_i_nodes, dim3((numNodes + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, a);
	SIMLOD_LAUNCH(k_copy, dim3(copy_grid(a.lay.itemCap)), dim3(LANE_TPB), stream, (const uint8_t*)a.scratch, a.lay.items);
	SIMLOD_LAUNCH(k_i_finish, dim3(1), dim3(1), stream, a);
	if (profile_enabled()) profile_close(stream);
	const int rc = (int)hipGetLastError();
	if (rc != 0) return rc;
	// the builder's side tables and its chunk table describe the octree that was there (simlod_octree_image_replaced)
	forget_leaf_table(ctx, nodes);
	ctx.sideTablesStale.store(true);
	array_event(ctx, nodes, ARRAY_IMPORTED);
	return 0;
}

int launch_import_buildable(Context& ctx, const SimlodUniforms* u, const SimlodExportNode* table, uint32_t numNodes, const SimlodPoint* samples,
                            uint64_t numSamples, void* scratch, uint64_t scratchBytes, uint8_t* pers, SimlodNode* nodes, SimlodStats* stats,
                            uint32_t* numBatchesUploaded, uint32_t* batchSizes, hipStream_t stream) {
	if (u == nullptr || table == nullptr || scratch == nullptr || pers == nullptr || nodes == nullptr || stats == nullptr || numBatchesUploaded == nullptr ||
	    batchSizes == nullptr || (samples == nullptr && numSamples != 0u))
		return (int)hipErrorInvalidValue;
	if (numNodes == 0u || numNodes > ctx.nodeCapacity.load() || scratchBytes < export_min_bytes(numNodes, numSamples)) return (int)hipErrorInvalidValue;
	ImportArgs a{};
	a.table = table; a.n = numNodes; a.samples = samples; a.numSamples = numSamples; a.scratch = reinterpret_cast<uint8_t*>(scratch);
	a.lay = Layout(numNodes, numSamples); a.pers = pers; a.persCap = u->persistentBufferCapacity; a.nodes = nodes; a.stats = stats;
	a.buildable = 1u;
	// the box as kernel_construct derives it (construct.hip launch_construct, voxels.cu:860-863)
	const float bx = u->boxMax.x - u->boxMin.x, by = u->boxMax.y - u->boxMin.y, bz = u->boxMax.z - u->boxMin.z;
	a.size = fmaxf(fmaxf(bx, by), bz);
	a.minx = u->boxMin.x; a.miny = u->boxMin.y; a.minz = u->boxMin.z;
	a.numBatchesUploaded = numBatchesUploaded; a.batchSizes = batchSizes; a.frameCounter = (uint32_t)u->frameCounter;
	// what launch_reset forgets of this node array's launches and upload counter (the counter is zeroed by k_i_finish, in stream order)
	forget_launch_history(ctx, stats, numBatchesUploaded, &a.feedback, &a.feedbackSeq);
	SIMLOD_LAUNCH(k_i_validate, dim3(1), dim3(WG_TPB), stream, a);
	SIMLOD_LAUNCH(k_i_nodes, dim3((numNodes + LANE_TPB - 1u) / LANE_TPB), dim3(LANE_TPB), stream, a);
	SIMLOD_LAUNCH(k_copy, dim3(copy_grid(a.lay.itemCap)), dim3(LANE_TPB), stream, (const uint8_t*)a.scratch, a.lay.items);
	SIMLOD_LAUNCH(k_i_gleaf, dim3(numNodes), dim3(G_TPB), stream, a);
	// inner nodes lie at levels 0 .. numInner - 1 at most (and below 20): one launch per level that can have any, deepest first
	const uint32_t numInner = (numNodes - 1u) / 8u;
	const uint32_t deepest = std::min<uint32_t>((uint32_t)SIMLOD_MAX_DEPTH - 1u, numInner > 0u ? numInner - 1u : 0u);
	const uint32_t wgs = std::min<uint32_t>(numNodes, device_info().numCUs * 4u);
	for (uint32_t level = deepest; level >= 1u; level--) SIMLOD_LAUNCH(k_i_gdown, dim3(wgs), dim3(G_TPB), stream, a, level);
	SIMLOD_LAUNCH(k_i_groot, dim3(1), dim3(R_TPB), stream, a);
	SIMLOD_LAUNCH(k_i_finish, dim3(1), dim3(1), stream, a);
	if (profile_enabled()) profile_close(stream);
	const int rc = (int)hipGetLastError();
	if (rc != 0) return rc;
	forget_leaf_table(ctx, nodes);
	ctx.sideTablesStale.store(true);
	array_event(ctx, nodes, ARRAY_IMPORTED_BUILDABLE);
	return 0;
}

}  // namespace simlod
