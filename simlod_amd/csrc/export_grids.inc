// export_grids.inc — part of export.hip: the buildable import's occupancy grids.  grid_of, octant_word, squeeze, k_i_gleaf, k_i_gdown,
// root_voxel, root_cell, k_i_groot.
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
// the cell of the root's grid a point files in (cell = x + 128 y + 128^2 z)
__device__ __forceinline__ uint32_t root_cell(const ImportArgs& a, const float4& p) {
	return ((quantize(F_FULL, p.x, a.minx, a.size) >> 21) & 127u) + ((quantize(F_FULL, p.y, a.miny, a.size) >> 21) & 127u) * 128u +
	       ((quantize(F_FULL, p.z, a.minz, a.size) >> 21) & 127u) * 16384u;
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
			const uint32_t cell = root_cell(a, p);
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
			const uint32_t cell = root_cell(a, p);
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
	for (uint32_t k = threadIdx.x; k < nch; k += R_TPB) link_chunk_list(a.pers, hdr->rootVoxBase, 0u, nch, k);
	if (threadIdx.x == 0) {
		SimlodNode* root = a.nodes;
		root->numVoxels = base; root->numVoxelsStored = base;
		root->voxelChunks = base != 0u ? reinterpret_cast<SimlodChunk*>(a.pers + hdr->rootVoxBase) : nullptr;
		hdr->rootVoxels = base;
	}
}
