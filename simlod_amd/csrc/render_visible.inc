// render_visible.inc — visibility, draw items and the chunk directory: the frustum planes, node_geometry, visible_nodes and the r_visible kernel.
// math.cuh:154-201: six planes from the rows of the matrix, normalised; a box is outside when its corner farthest along a plane's
// normal is behind the plane.  The planes are the same for every node: plane i is normalised ONCE per workgroup (24 correctly rounded
// divisions and 6 square roots that every lane used to repeat), into LDS.
__device__ __forceinline__ void frustum_plane(const SimlodMat4& m, int i, float out[4]) {
	const simlod_float4* R = m.rows;
	const float m0 = R[0].x, m1 = R[1].x, m2 = R[2].x, m3 = R[3].x;
	const float m4 = R[0].y, m5 = R[1].y, m6 = R[2].y, m7 = R[3].y;
	const float m8 = R[0].z, m9 = R[1].z, m10 = R[2].z, m11 = R[3].z;
	const float m12 = R[0].w, m13 = R[1].w, m14 = R[2].w, m15 = R[3].w;
	const float P[6][4] = {
		{m3 - m0, m7 - m4, m11 - m8, m15 - m12}, {m3 + m0, m7 + m4, m11 + m8, m15 + m12},
		{m3 + m1, m7 + m5, m11 + m9, m15 + m13}, {m3 - m1, m7 - m5, m11 - m9, m15 - m13},
		{m3 - m2, m7 - m6, m11 - m10, m15 - m14}, {m3 + m2, m7 + m6, m11 + m10, m15 + m14}};
	const float x = P[i][0], y = P[i][1], z = P[i][2], w = P[i][3];
	float d2 = x * x; d2 = d2 + y * y; d2 = d2 + z * z;
	const float len = sqrtf(d2);
	out[0] = x / len; out[1] = y / len; out[2] = z / len; out[3] = w / len;
}

__device__ __forceinline__ bool intersects_frustum(const float (*planes)[4], const float mn[3], const float mx[3]) {
	bool inside = true;
#pragma unroll
	for (int i = 0; i < 6; i++) {
		const float nx = planes[i][0], ny = planes[i][1], nz = planes[i][2], c = planes[i][3];
		const float vx = nx > 0.0f ? mx[0] : mn[0];
		const float vy = ny > 0.0f ? mx[1] : mn[1];
		const float vz = nz > 0.0f ? mx[2] : mn[2];
		float d = nx * vx; d = d + ny * vy; d = d + nz * vz; d = d + c;
		if (d < 0.0f) inside = false;
	}
	return inside;
}

// render.cu:760-861: a node's box is inside when it meets the frustum, large when its screen box spans more than 2 x minNodeSize pixels.
// Pure geometry of (level, X, Y, Z): a node can evaluate its PARENT's `large` — (level - 1, X/2, Y/2, Z/2) — without reading it.
template <bool FRUSTUM>
__device__ __forceinline__ void node_geometry(const RenderArgs& a, const float (*planes)[4], uint32_t level, uint32_t X, uint32_t Y, uint32_t Z, bool& inside, bool& large) {
	const float nodeSize = a.cubeSize / exp2_int(level);
	const float cmin[3] = {a.minx, a.miny, a.minz};
	const uint32_t XYZ[3] = {X, Y, Z};
	float mn[3], mx[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		mn[k] = cmin[k] + ((float)XYZ[k] + 0.0f) * nodeSize;
		mx[k] = cmin[k] + ((float)XYZ[k] + 1.0f) * nodeSize;
	}
	float sx[8], sy[8];
#pragma unroll
	for (int k = 0; k < 8; k++) {   // p000, p001, p010, p011, p100, p101, p110, p111 (render.cu:783-790)
		const float x = (k & 4) ? mx[0] : mn[0], y = (k & 2) ? mx[1] : mn[1], z = (k & 1) ? mx[2] : mn[2];
		const float cx = dot_row(a.transformUpdate.rows[0], x, y, z);
		const float cy = dot_row(a.transformUpdate.rows[1], x, y, z);
		const float cw = dot_row(a.transformUpdate.rows[3], x, y, z);
		sx[k] = ((cx / cw) * 0.5f + 0.5f) * a.width;
		sy[k] = ((cy / cw) * 0.5f + 0.5f) * a.height;
	}
	const float minx = fminf(fminf(fminf(sx[0], sx[1]), fminf(sx[2], sx[3])), fminf(fminf(sx[4], sx[5]), fminf(sx[6], sx[7])));
	const float maxx = fmaxf(fmaxf(fmaxf(sx[0], sx[1]), fmaxf(sx[2], sx[3])), fmaxf(fmaxf(sx[4], sx[5]), fmaxf(sx[6], sx[7])));
	const float miny = fminf(fminf(fminf(sy[0], sy[1]), fminf(sy[2], sy[3])), fminf(fminf(sy[4], sy[5]), fminf(sy[6], sy[7])));
	const float maxy = fmaxf(fmaxf(fmaxf(sy[0], sy[1]), fmaxf(sy[2], sy[3])), fmaxf(fmaxf(sy[4], sy[5]), fmaxf(sy[6], sy[7])));
	const float dx = maxx - minx, dy = maxy - miny;
	inside = FRUSTUM ? intersects_frustum(planes, mn, mx) : false;
	const double lim = 2.0 * (double)a.minNodeSize;
	large = (double)dx > lim || (double)dy > lim;                                           // render.cu:860-861
}

// ---- visibility, draw items and the frame's chunk directory: ONE launch, one lane per node -------------------------------------------------
// The reference flags every node (render.cu:760-861), then lets every LARGE node emit its small visible children, and itself when it is
// a visible leaf (render.cu:746-756, 906-933), then gives one workgroup a whole node and lets it chase the chunk list while it draws
// (render.cu:106-159, 179-207).  Here a node decides about ITSELF: drawn when visible and either small under a large parent — the
// parent's `large` is geometry of (level - 1, X/2, Y/2, Z/2), computed right here with the parent's own arithmetic — or a large leaf.
// No lane waits for another's flags, so flags, emission and draw items are one kernel whose critical path is four memory round trips
// (node fields; one reservation per wave; the chunk-table row; stores) instead of three kernels with twelve.
// Draw items: a lane writes its node's chunk addresses into the frame's directory — copied from the builder's chunk table when that is
// valid, else by walking the list (the only serial pointer chase left in a frame) — and cuts the list into items of <= 64 chunks.
// `clip` (render_common.inc: NoClip, Clip): a node the frame's clip empties counts as holding nothing — not visible, in the node array either.
template <typename POLICY>
__device__ __forceinline__ void visible_nodes(const RenderArgs& a, const float (&planes)[6][4], const uint32_t numNodes, SimlodNode* staged, const uint32_t readyEarly, const POLICY& clip) {
	const uint32_t i = blockIdx.x * TPB + threadIdx.x;
	const bool active = i < numNodes;
	// the workgroup's 256 nodes were staged in LDS with coalesced loads (r_visible): a lane reading ITS 152-byte node from memory touched a
	// cache line per lane and field — a thousand line requests per wave, 5 us of the kernel's 19
	SimlodNode* n = staged + (active ? threadIdx.x : 0u);
	SimlodNode* nGlobal = a.nodes + (active ? i : 0u);
	// The builder keeps, per node, the addresses of the first chunks of its list (construct_*.hip, leaf chunk table: a leaf's row lists
	// its point chunks, an inner node's its voxel chunks) and stamps the table with the octree it describes (k_finish).  When that stamp
	// matches THIS octree as it is now, and the node's row starts at the list's head, the row IS the list.
	// (all words of the stamp in flight together: tested one after the other, each waited for the one before — five round trips)
	bool tableValid = false;
	const SimlodChunk* rowHead = nullptr;                    // first entry of this node's row of the table: in flight with the node's fields
	if (a.leafTable != nullptr) {
		const uint32_t magic = *a.leafTableMagic, batch = *a.leafTableBatch, batchNow = a.stats->batchletIndex;
		const uint64_t tableNodes = *a.leafTableNodes, sig = *a.leafTableSig, sigNow = table_signature(a.stats);
		if (a.leafTableSlots <= 64u && a.leafTableRows != 0u) rowHead = leaf_row_get(a.leafTable, a.leafTablePers, active && i < a.leafTableRows ? i : 0u, 0u);
		tableValid = (magic == a.leafTableMagicValue) & (batch == batchNow) & (tableNodes == (uint64_t)a.nodes) & (sig == sigNow);
	}
	const uint32_t level = n->level, X = n->X, Y = n->Y, Z = n->Z;
	const uint32_t counts[2] = {n->numPoints, n->numVoxels};
	const SimlodChunk* heads[2] = {n->points, n->voxelChunks};
	bool leaf = true;
#pragma unroll
	for (int k = 0; k < 8; k++) leaf = leaf && n->children[k] == nullptr;
	bool inside, large, unused, parentLarge = false;
	node_geometry<true>(a, planes, level, X, Y, Z, inside, large);
	bool visible = inside && (counts[0] > 0u || counts[1] > 0u);
	if constexpr (POLICY::ON) visible = visible && !clip.empties(level, X, Y, Z);
	if (active) { n->visible = visible ? 1 : 0; n->isLarge = large ? 1 : 0; nGlobal->visible = visible ? 1 : 0; nGlobal->isLarge = large ? 1 : 0; }      // (the staged copy goes to the visible list)
	if (active && visible && !large && level > 0u) node_geometry<false>(a, planes, level - 1u, X >> 1, Y >> 1, Z >> 1, unused, parentLarge);   // only who needs it
	const bool emit = active && visible && (large ? leaf : parentLarge);
	R_PROBE_MAX(2);
	if (__ballot(emit) == 0ull) return;

	// one reservation per wave and counter (returning device-scope atomics on one word retire at ~11 ns each, and a lane waits ~2.5 us
	// for each one it depends on): visible-list slots, directory entries, draw items
	const bool draws = emit && a.showPoints;
	// the LDS tile of the node's draw items: its screen box when that fits a tile; else a tile in the MIDDLE of the box (the corners of a
	// cube's screen box are empty, the terrain runs through its middle) — samples that fall outside take the global path.  A node that
	// reaches behind the camera has no box and no tile.
	int tileX = -1, tileY = -1;
	uint32_t tileW = TILE, tileH = TILE;
	bool noTile = draws, sorts = false;
	if (draws && a.useTiles) {
		const float nodeSize = a.cubeSize / exp2_int(level);
		float mnx = 3.0e38f, mny = 3.0e38f, mxx = -3.0e38f, mxy = -3.0e38f;
		bool front = true;
		for (int k = 0; k < 8; k++) {
			const float x = a.minx + ((float)X + ((k & 4) ? 1.0f : 0.0f)) * nodeSize, y = a.miny + ((float)Y + ((k & 2) ? 1.0f : 0.0f)) * nodeSize;
			const float z = a.minz + ((float)Z + ((k & 1) ? 1.0f : 0.0f)) * nodeSize;
			const float cw = dot_row(a.transform.rows[3], x, y, z);
			if (!(cw > 0.0f)) { front = false; break; }
			// (the hardware's approximate reciprocal: where the tile lies decides how fast a frame is drawn, not what it shows; the correctly
			// rounded divisions of eight corners were a microsecond of this kernel)
			const float rw = __builtin_amdgcn_rcpf(cw);
			const float sx = ((dot_row(a.transform.rows[0], x, y, z) * rw) * 0.5f + 0.5f) * a.width, sy = ((dot_row(a.transform.rows[1], x, y, z) * rw) * 0.5f + 0.5f) * a.height;
			mnx = fminf(mnx, sx); mny = fminf(mny, sy); mxx = fmaxf(mxx, sx); mxy = fmaxf(mxy, sy);
		}
		if (front && mnx > -1.0e6f && mny > -1.0e6f && mnx < 1.0e6f && mny < 1.0e6f) {
			// the part of the box that is on the screen
			const int x0 = max((int)mnx - 1, 0), y0 = max((int)mny - 1, 0);
			const int x1 = min((int)fminf(mxx, 1.0e6f) + a.pointSize + 2, a.W + 1), y1 = min((int)fminf(mxy, 1.0e6f) + a.pointSize + 2, a.H + 1);
			const int bw = max(x1 - x0, 1), bh = max(y1 - y0, 1);
			// the tile takes the box's shape: TILE x TILE words, as wide or as high as the box asks for (a node seen at a grazing angle — the
			// terrain towards the horizon of a close-up — is a strip of 1000 x 40 pixels: under a square tile most of its samples went outside)
			if (bh <= bw) { tileH = (uint32_t)min(bh, TILE); tileW = (uint32_t)min(bw, TILE * TILE / (int)tileH); }
			else { tileW = (uint32_t)min(bw, TILE); tileH = (uint32_t)min(bh, TILE * TILE / (int)tileW); }
			tileX = x0 + (bw - (int)tileW) / 2; tileY = y0 + (bh - (int)tileH) / 2;
			noTile = false;
			sorts = a.binsPossible && (uint32_t)bw * (uint32_t)bh > a.binMinArea;                 // much larger than a tile: its samples are sorted into the screen bins
		} else sorts = a.binsPossible != 0u;                                                      // reaches behind the camera: no box, no tile — sorted
		if (sorts && a.useBins) { tileX = TILE_BINNED; noTile = false; }
	}
	// (launch_render leaves the bins out of a frame — two kernels — when the buffer's previous frame had nothing to sort: this frame tells the next)
	const uint32_t waveSorts = (uint32_t)__popcll(__ballot(sorts));
	R_PROBE_MAX(9);
	// ... and their size: up to ITEM_CHUNKS chunks; an eighth of that for a node without a tile: every sample of such an item is a scattered
	// global atomic, 64 memory transactions per wave instruction — a 32 000-sample item of that kind took ~100 us, the frame's makespan in the
	// close-up preset; short ones spread over the CUs (and have no tile to clear or flush)
	const uint32_t perItem = noTile ? ITEM_CHUNKS / 8u : tileX == TILE_BINNED ? BIN_ITEM_CHUNKS : ITEM_CHUNKS;
	const uint32_t weight = tileX == TILE_BINNED ? 2u : 1u;                                 // a sorting item takes what a tile item of twice its samples takes: it queues with those
	uint32_t numChunks[2], pieces[2];
#pragma unroll
	for (int l = 0; l < 2; l++) {
		const bool have = draws && counts[l] != 0u && heads[l] != nullptr;
		numChunks[l] = have ? (counts[l] + SIMLOD_POINTS_PER_CHUNK - 1) / SIMLOD_POINTS_PER_CHUNK : 0u;
		pieces[l] = (numChunks[l] + perItem - 1) / perItem;
	}
	const uint32_t myChunks = numChunks[0] + numChunks[1];
	// A node has one list worth drawing (a leaf its points, an inner node its voxels): that one may come from the builder's chunk table
	const int rowList = numChunks[0] != 0u ? 0 : 1;
	// (a draw item that reads its chunks straight from the row names the row — 256-byte aligned — with bit 0 set and its first slot in bits 1..7: item_chunk)
	const uint8_t* const slots = tableValid && draws && a.leafTableSlots <= 64u && i < a.leafTableRows ? a.leafTable + (uint64_t)i * LEAF_ROW_BYTES : nullptr;
	const uint32_t fromTable = slots != nullptr ? min(numChunks[rowList], a.leafTableSlots) : 0u;
	uint32_t myClass[ITEM_CLASSES] = {0u, 0u, 0u, 0u};                                   // a list's pieces: full ones (class 0), then the rest
#pragma unroll
	for (int l = 0; l < 2; l++) {
		if (pieces[l] == 0u) continue;
		const uint32_t fullClass = item_class(perItem * weight), lastClass = item_class((numChunks[l] - (pieces[l] - 1u) * perItem) * weight);
#pragma unroll
		for (int cl = 0; cl < ITEM_CLASSES; cl++) myClass[cl] += (fullClass == (uint32_t)cl ? pieces[l] - 1u : 0u) + (lastClass == (uint32_t)cl ? 1u : 0u);
	}
	const unsigned long long emitters = __ballot(emit);
	const uint32_t slotsBefore = __builtin_amdgcn_mbcnt_hi((uint32_t)(emitters >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)emitters, 0u)), waveSlots = (uint32_t)__popcll(emitters);
	uint32_t waveChunks;
	const uint32_t chunksBefore = wave_prefix_u32(myChunks, waveChunks);
	uint32_t classBase[ITEM_CLASSES], waveClass[ITEM_CLASSES];
#pragma unroll
	for (int cl = 0; cl < ITEM_CLASSES; cl++) classBase[cl] = wave_prefix_u32(myClass[cl], waveClass[cl]);
	const bool isLeafDraw = emit && counts[0] > 0u, isInnerDraw = emit && counts[0] == 0u && counts[1] > 0u;   // render.cu:748-754
	const uint32_t wLeaves = (uint32_t)__popcll(__ballot(isLeafDraw)), wInner = (uint32_t)__popcll(__ballot(isInnerDraw));
	const uint32_t wPts = wave_sum_u32(isLeafDraw ? counts[0] : 0u), wVox = wave_sum_u32(isInnerDraw ? counts[1] : 0u);
	uint32_t* work = work_words(a.mom, a.lay);
	uint32_t slot = 0, dirBase = 0, waveBase[ITEM_CLASSES] = {0u, 0u, 0u, 0u};
	R_PROBE_MAX(10);
	if (lane_id() == 0) {
		if (readyEarly != a.launchSeq) { wait_frame_ready(a); R_PROBE_MAX(11); }            // (read while the nodes were on their way: by then thread 0 had long published)
		R_PROBE_MAX(8);
		slot = atomicAdd(counter_at(a.mom, C_VISIBLE), waveSlots);
		if (waveSorts != 0u) atomicAdd(work + W_SORTING_NODES, waveSorts);
		if (waveChunks != 0u) {
			dirBase = atomicAdd(work + W_DIR_ENTRIES, waveChunks);
#pragma unroll
			for (int cl = 0; cl < ITEM_CLASSES; cl++) if (waveClass[cl] != 0u) waveBase[cl] = atomicAdd(work + W_ITEMS0 + cl, waveClass[cl]);
		}
		if (wLeaves) { atomicAdd(counter_at(a.mom, C_LEAVES), wLeaves); atomicAdd(counter_at(a.mom, C_POINTS), wPts); }
		if (wInner) { atomicAdd(counter_at(a.mom, C_INNER), wInner); atomicAdd(counter_at(a.mom, C_VOXELS), wVox); }
	}
	slot = __shfl(slot, 0) + slotsBefore; dirBase = __shfl(dirBase, 0) + chunksBefore;
	if (slot != 0xffffffffu) R_PROBE_MAX(3);
#pragma unroll
	for (int cl = 0; cl < ITEM_CLASSES; cl++) classBase[cl] += __shfl(waveBase[cl], 0);      // this lane's next free slot in class cl
	DrawItem* items = reinterpret_cast<DrawItem*>(a.mom + a.lay.items);
	const SimlodChunk** dir = reinterpret_cast<const SimlodChunk**>(a.mom + a.lay.dir);
	// A list that fits a row of the builder's chunk table (<= 50 chunks: every leaf below its limit, most inner nodes) is not copied at
	// all: its draw item points INTO the row, once the row is seen to start with the list's head (r_draw ends the item at a gap, should
	// a row ever have one).  Measured: copying the rows into the frame's directory — per lane, or by whole waves — was 10 us of this
	// kernel's 28 (the visible nodes are neighbours in the node array: a few waves had all the copying to do).
	const bool rowDirect = fromTable != 0u && numChunks[rowList] <= a.leafTableSlots && rowHead == heads[rowList];
	uint32_t throughTable = 0;
	if (emit) {
		const bool listed = slot < SIMLOD_MAX_VISIBLE_NODES;
		if (!listed) atomicOr(&a.stats->dbg, SIMLOD_ERR_VISIBLE_OVERFLOW);
		else {
			const ulonglong1* src = reinterpret_cast<const ulonglong1*>(n);
			ulonglong1* dst = reinterpret_cast<ulonglong1*>(reinterpret_cast<SimlodNode*>(a.mom + FrameLayout::visible) + slot);
#pragma unroll
			for (int w = 0; w < (int)(sizeof(SimlodNode) / 8); w++) dst[w] = src[w];
		}
		for (int l = 0; l < 2; l++, dirBase += numChunks[l - 1]) {
			if (numChunks[l] == 0u) continue;
			const bool fits = listed && dirBase + numChunks[l] <= MAX_DIR_CHUNKS;
			if (!fits) atomicOr(&a.stats->dbg, SIMLOD_ERR_VISIBLE_OVERFLOW);                // its items are reserved: they stay, empty
			uint32_t k = 0;
			if (fits) {
				const SimlodChunk* chunk = heads[l];
				if (l == rowList && rowDirect) { k = numChunks[l]; chunk = nullptr; throughTable++; }   // nothing to copy
				for (; k < numChunks[l] && chunk != nullptr; k++) { dir[dirBase + k] = chunk; chunk = chunk->next; }
			}
			const uint32_t have = min(counts[l], k * SIMLOD_POINTS_PER_CHUNK);      // a list shorter than its counter says: draw what is there
			for (uint32_t p = 0; p < pieces[l]; p++) {
				const uint32_t firstSample = p * perItem * SIMLOD_POINTS_PER_CHUNK;
				const uint32_t cl = p + 1u < pieces[l] ? item_class(perItem * weight) : item_class((numChunks[l] - p * perItem) * weight);
				uint32_t at = 0;
#pragma unroll
				for (int q = 0; q < ITEM_CLASSES; q++) if (cl == (uint32_t)q) at = classBase[q]++;
				if (at >= a.itemCap) { atomicOr(&a.stats->dbg, SIMLOD_ERR_VISIBLE_OVERFLOW); continue; }
				DrawItem it;
				it.chunks = l == rowList && rowDirect ? reinterpret_cast<const SimlodChunk* const*>((uint64_t)slots | 1ull | (uint64_t)(p * perItem) << 1) : dir + dirBase + p * perItem;
				it.samples = have > firstSample ? min(have - firstSample, perItem * SIMLOD_POINTS_PER_CHUNK) : 0u;
				it.visibleIdx = slot; it.tileX = tileX; it.tileY = tileY; it.tileWH = tileW | (tileH << 16); it.took = 0u;
				items[(uint64_t)cl * a.itemCap + at] = it;
			}
		}
	}
	R_PROBE_MAX(4);
	const uint32_t waveTable = wave_sum_u32(throughTable);
	if (lane_id() == 0 && waveTable != 0u) atomicAdd(counter_at(a.mom, C_TABLE_LISTS), waveTable);
}

// One definition for both kinds of frame: r_visible(a) — no clip, the kernel as it was before there were clips — and r_visible(a, k) with the
// frame's clip as a second argument (RenderArgs goes to every kernel of the frame: the clip stays out of it), its planes staged in LDS.
template <typename... CLIP>
__global__ __launch_bounds__(TPB) void r_visible(RenderArgs a, CLIP... k) {
	ClipStore<sizeof...(CLIP) != 0> sh_clip;
	const auto clip = sh_clip.policy(k...);
	R_PROBE_MIN(0);
	if (blockIdx.x == 0 && threadIdx.x == 0) clear_counters(a);
	const uint32_t numNodes = min(a.stats->numNodes, a.nodeCapacity);
	if (numNodes != 0xffffffffu) R_PROBE_MAX(1);
	if (blockIdx.x * TPB < numNodes) {                                                 // whole workgroups: the lanes of a wave reserve together
		__shared__ float planes[6][4];
		__shared__ unsigned long long staged[TPB * sizeof(SimlodNode) / 8];
		static_assert(sizeof(SimlodNode) % 8 == 0, "nodes are staged as 8-byte words");
		const uint32_t words = min((uint32_t)TPB, numNodes - blockIdx.x * TPB) * (uint32_t)(sizeof(SimlodNode) / 8);
		const unsigned long long* src = reinterpret_cast<const unsigned long long*>(a.nodes + (uint64_t)blockIdx.x * TPB);
		constexpr uint32_t PER_THREAD = sizeof(SimlodNode) / 8;                     // all of a thread's loads in flight, then the stores
		unsigned long long held[PER_THREAD];
#pragma unroll
		for (uint32_t q = 0; q < PER_THREAD; q++) { const uint32_t w = q * TPB + threadIdx.x; held[q] = w < words ? src[w] : 0ull; }
#pragma unroll
		for (uint32_t q = 0; q < PER_THREAD; q++) staged[q * TPB + threadIdx.x] = held[q];
		const uint32_t readyEarly = __hip_atomic_load(frame_ready_word(a.mom, a.lay), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (threadIdx.x < 6) frustum_plane(a.transformUpdate, (int)threadIdx.x, planes[threadIdx.x]);
		__syncthreads();
		visible_nodes(a, planes, numNodes, reinterpret_cast<SimlodNode*>(staged), readyEarly, clip);
		R_PROBE_MAX(5);
	}
	clear_frame(a);
	R_PROBE_MAX(6); R_PROBE_MIN(7);
}
