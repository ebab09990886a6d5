// export_paint.inc — part of export.hip: paint regions.  PaintOp, PaintArgs, FootPaintArgs, paint_colour, e_paint, k_e_paint, k_ef_paint.
// ---- paint regions ----------------------------------------------------------------------------------------------------------------------
// simlod_paint_region (simlod_hip.h, "paint regions"): the footprint query's count-only call — k_q_hier / k_f_hier -> k_q_dir -> k_q_count /
// k_f_count -> k_q_scan — and then, where that query has k_q_write / k_f_write:
//   k_e_paint    the items once more, one chunk per workgroup and turn.  A copied chunk in SET mode without `previous` is stored to without a
//                load.  Every other chunk is read as k_q_write reads it (four 16-byte loads of a lane in flight), a filtered one tested again,
//                and each lane stores the colour of the samples IT read: no two lanes write the same word, so no atomic.  The rank of a sample
//                in the query's order — previous[j], colors[j] — comes from the item's offset, the 16 segment counts in LDS and the ballot's
//                bits below the lane, as in q_write; without either array there is no LDS traffic and no barrier.
//   k_ef_paint   the same body with rule F1 behind the planes' test, the polygon staged in LDS as k_f_write stages it.
// k_q_scan zeroes hdr->numItems for a count-only call: the items are hdr->totalChunks.  Rule E5's check is made here, by every workgroup, from
// what k_q_scan left in the counts record; workgroup 0 adds the error bit.
// The rules themselves (E1-E3) in paint_rules.hpp.
// A sample that was loaded is stored whole, 16 bytes: lanes next to each other then fill whole lines, where 4-byte stores 16 bytes apart leave
// every line a quarter written (DESIGN §11 has both timings; -DPAINT_STORE_RECORD=0 builds the other).  The chunk that is not loaded has only
// its colour words to store.
#ifndef PAINT_STORE_RECORD
#define PAINT_STORE_RECORD 1
#endif
#ifndef PAINT_LOAD_NT
#define PAINT_LOAD_NT 1                // the loads are non-temporal, as k_q_write's (0: plain loads, measured too)
#endif
#ifndef PAINT_STORE_NT
#define PAINT_STORE_NT 0               // the 16-byte stores are plain (1: non-temporal, as k_q_write's; measured too, and no faster in place)
#endif

struct PaintOp {
	uint32_t        mode, color, strength, pad;
	float           z0, scale;
	uint64_t        table;              // offset of the ramp's 256 words in the scratch buffer
	const uint32_t* colors;             // ARRAY, else nullptr
	uint32_t*       previous;           // or nullptr
	uint64_t        colorCap;
	uint32_t        checkCap, pad1;     // rule E5: an array was given
};
struct PaintArgs     { QueryArgs q; PaintOp p; };
struct FootPaintArgs { FootArgs  f; PaintOp p; };
__device__ __forceinline__ const QueryArgs& query_of(const PaintArgs& pa) { return pa.q; }
__device__ __forceinline__ const QueryArgs& query_of(const FootPaintArgs& pa) { return pa.f.q; }

// rules E1-E4: the new colour word of sample j of the query's order
__device__ __forceinline__ uint32_t paint_colour(const PaintOp& p, const uint32_t* ramp, const u32x4& v, uint64_t j) {
	switch (p.mode) {
		case SIMLOD_PAINT_SET:   return p.color;
		case SIMLOD_PAINT_BLEND: return paint_blend(v.w, p.color, p.strength);
		case SIMLOD_PAINT_RAMP:  return ramp[paint_ramp_index(__uint_as_float(v.z), p.z0, p.scale)];
		default:                 return p.colors[j];
	}
}

// the body of the paint kernels; extra(v) and INVERT as in q_count
template <typename Args, bool INVERT = false, typename Extra>
__device__ __forceinline__ void e_paint(const Args& args, Extra extra) {
	const QueryArgs& q = query_of(args);
	const PaintOp& p = args.p;
	__shared__ uint32_t sh_seg[2][16];
	const ExportArgs& a = q.x;
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const QItem* items = reinterpret_cast<const QItem*>(a.scratch + a.lay.items);
	const uint32_t* ramp = reinterpret_cast<const uint32_t*>(a.scratch + p.table);
	// rule E5 (the same for every workgroup)
	const uint32_t err = q.counts->error;
	const bool over = p.checkCap != 0u && q.counts->numSamples > p.colorCap;
	if (err != 0u || over) {
		if (over && blockIdx.x == 0u && threadIdx.x == 0u) q.counts->error = err | SIMLOD_EXPORT_ERR_CAPACITY;
		return;
	}
	const uint64_t numItems = hdr->totalChunks;
	const bool ranked = p.colors != nullptr || p.previous != nullptr;
	const int lane = lane_id(), w = (int)(threadIdx.x / SIMLOD_WAVE);
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t turn = 0;
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const QItem it = items[i];
		if (it.count == 0u) continue;                                       // (the same for the whole workgroup, as every branch on `it`)
		const bool copied = it.tag == Q_COPIED;
		if (!copied && (it.tag != Q_FILTERED || it.pass == 0u)) continue;
		u32x4* s = reinterpret_cast<u32x4*>(it.src);
		if (copied && p.mode == SIMLOD_PAINT_SET && p.previous == nullptr) {
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
				if (k < it.count) reinterpret_cast<uint32_t*>(s + k)[3] = p.color;
			}
			continue;
		}
		u32x4 v[4];
		load_chunk4<PAINT_LOAD_NT != 0, true>(s, it.count, v);
		bool     on[4];
		uint32_t rank[4];                                                   // of the lane's sample j within the item (ranked only)
		if (copied) {
#pragma unroll
			for (int j = 0; j < 4; j++) {
				rank[j] = threadIdx.x + (uint32_t)j * LANE_TPB;
				on[j] = rank[j] < it.count;
			}
		} else {
			uint64_t b[4];
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
				if (INVERT) b[j] = __ballot(k < it.count && !(passes(q.g, v[j]) && extra(v[j])));
				else b[j] = __ballot(k < it.count && passes(q.g, v[j]) && extra(v[j]));
				on[j] = ((b[j] >> lane) & 1ull) != 0ull;
				rank[j] = 0u;
			}
			if (ranked) {
#pragma unroll
				for (int j = 0; j < 4; j++)
					if (lane == 0) sh_seg[turn][j * 4 + w] = (uint32_t)__popcll(b[j]);
				__syncthreads();                // (two buffers, as in k_q_count)
				uint32_t run = 0;
#pragma unroll
				for (int j = 0; j < 4; j++) {
#pragma unroll
					for (int ww = 0; ww < 4; ww++) {
						if (ww == w) rank[j] = run + (uint32_t)__popcll(b[j] & below);
						run += sh_seg[turn][j * 4 + ww];
					}
				}
				turn ^= 1u;
			}
		}
		// sample 0 of the item in the query's order: a copied chunk lies at its ordinal, a filtered one behind what passed before it
		const uint64_t j0 = ranked ? a.table[it.node].firstSample + (copied ? (uint64_t)it.k * SIMLOD_POINTS_PER_CHUNK : (uint64_t)it.off) : 0u;
#pragma unroll
		for (int j = 0; j < 4; j++) {
			if (!on[j]) continue;
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			const uint64_t at = j0 + rank[j];
			if (p.previous != nullptr) p.previous[at] = v[j].w;
			const uint32_t c = paint_colour(p, ramp, v[j], at);
#if PAINT_STORE_RECORD
			v[j].w = c;
#if PAINT_STORE_NT
			__builtin_nontemporal_store(v[j], s + k);
#else
			s[k] = v[j];
#endif
#else
			reinterpret_cast<uint32_t*>(s + k)[3] = c;
#endif
		}
	}
}

__global__ __launch_bounds__(LANE_TPB) void k_e_paint(PaintArgs pa) { e_paint<PaintArgs>(pa, NoFootprint()); }

__global__ __launch_bounds__(LANE_TPB) void k_ef_paint(FootPaintArgs pa) {
	__shared__ FootEdge sh_edges[SIMLOD_FOOTPRINT_MAX_VERTICES];
	stage_edges(pa.f, sh_edges);
	__syncthreads();
	e_paint<FootPaintArgs>(pa, Footprint{pa.f.f, sh_edges});
}
