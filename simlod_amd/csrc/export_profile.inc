// export_profile.inc — part of export.hip: profile queries.  ProfGeom, ProfArgs, stage_segments, sample_uv, Profile (rule P1), k_pr_hier, k_pr_count,
// locate_record, k_pr_write.  The rules themselves: profile_rules.hpp.
// ---- profile query --------------------------------------------------------------------------------------------------------------------
// simlod_query_profile (simlod_hip.h, "profile queries"): the region query's five launches with a corridor along a polyline on top of the planes,
// and a derived record per returned sample.  (k_pr_*: k_p_* are the pair queries' kernels, export_pairs.inc.)
//   k_pr_hier   k_q_hier with the class of a node combined from the planes (classify) and the corridor (classify_profile, rule P3).
//   k_q_dir, k_q_scan   as they are.
//   k_pr_count  k_q_count's body with rule P1 behind the planes' test.
//   k_pr_write  a body of its own beside q_write: a sample and its SimlodProfileSample go to the same index of `samples` and `records`.  COPIED
//               items keep their place (firstSample + 1000 k + j) but every lane still looks its samples' segments up — a node one segment
//               covers may hold samples an earlier segment owns; FILTERED items are compacted in order as q_write does.
// The segments lie in the caller's scratch, computed by the launcher (rule P0: the square root and the division are the host's).  Every kernel
// stages them in LDS once per workgroup; all lanes then read the same segment in the same iteration (a broadcast read, no bank conflict).
static_assert(PROFILE_NODE_OUTSIDE == Q_OUTSIDE && PROFILE_NODE_FILTERED == Q_FILTERED && PROFILE_NODE_COPIED == Q_COPIED, "profile_rules.hpp: the classes");

struct ProfGeom {
	double   axU[4], axV[4], axH[4];
	uint64_t segs;                      // offset of ProfileSegment[n] in the scratch buffer
	uint32_t n, pad;                    // segments
};
struct ProfArgs {
	QueryArgs            q;
	ProfGeom             f;
	SimlodProfileSample* records;       // or nullptr: samples only
};

__device__ __forceinline__ const QueryArgs& query_of(const ProfArgs& pa) { return pa.q; }

// the segments from the scratch buffer into LDS (any block size); the barrier is the caller's
__device__ __forceinline__ void stage_segments(const ProfArgs& pa, ProfileSegment* sh) {
	const ProfileSegment* s = reinterpret_cast<const ProfileSegment*>(pa.q.x.scratch + pa.f.segs);
	for (uint32_t i = threadIdx.x; i < pa.f.n; i += blockDim.x) sh[i] = s[i];
}

// what k_pr_count asks of a sample behind the planes: (u, v) as footprint rule F1, then rule P1
struct Profile {
	const ProfGeom&       f;
	const ProfileSegment* sh;
	__device__ __forceinline__ bool operator()(const u32x4& p) const {
		const double x = (double)__uint_as_float(p.x), y = (double)__uint_as_float(p.y), z = (double)__uint_as_float(p.z);
		double al, c;
		return profile_locate(sh, f.n, profile_axis(f.axU, x, y, z), profile_axis(f.axV, x, y, z), al, c) < f.n;
	}
};

__global__ __launch_bounds__(WG_TPB) void k_pr_hier(ProfArgs pa) {
	__shared__ uint64_t sh_scan[WG_WAVES];
	__shared__ ProfileSegment sh_segs[PROFILE_MAX_SEGMENTS];
	const ExportArgs& a = pa.q.x;
	uint32_t* cls = reinterpret_cast<uint32_t*>(a.scratch + pa.q.cls);
	stage_segments(pa, sh_segs);
	__syncthreads();
	hier_walk<true>(a, [&](uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
		// outside by either; copied iff copied by both; else filtered
		const uint32_t p = classify(pa.q.g, level, X, Y, Z);
		if (p == Q_OUTSIDE) return (uint32_t)Q_OUTSIDE;
		const uint32_t c = classify_profile(pa.q.g.min, pa.q.g.size, pa.f.axU, pa.f.axV, sh_segs, pa.f.n, level, X, Y, Z);
		return c == Q_OUTSIDE ? (uint32_t)Q_OUTSIDE : (p == Q_COPIED && c == Q_COPIED) ? (uint32_t)Q_COPIED : (uint32_t)Q_FILTERED;
	}, cls);
	__syncthreads();
	query_totals(a, cls, sh_scan);
}

__global__ __launch_bounds__(LANE_TPB) void k_pr_count(ProfArgs pa) {
	__shared__ ProfileSegment sh_segs[PROFILE_MAX_SEGMENTS];
	stage_segments(pa, sh_segs);
	__syncthreads();
	q_count<const ProfArgs&>(pa, Profile{pa.f, sh_segs});
}

// rules P1 and P2 for one sample: its lowest segment (< f.n: it is in one) and its record as the 16 bytes that are stored
__device__ __forceinline__ uint32_t locate_record(const ProfGeom& f, const ProfileSegment* sh, const u32x4& p, u32x4& rec) {
	const double x = (double)__uint_as_float(p.x), y = (double)__uint_as_float(p.y), z = (double)__uint_as_float(p.z);
	double al = 0.0, c = 0.0;
	const uint32_t i = profile_locate(sh, f.n, profile_axis(f.axU, x, y, z), profile_axis(f.axV, x, y, z), al, c);
	const SimlodProfileSample r = profile_record(sh, f.n, i, al, c, profile_axis(f.axH, x, y, z));
	rec = u32x4{__float_as_uint(r.station), __float_as_uint(r.offset), __float_as_uint(r.height), r.segment};
	return i;
}

__global__ __launch_bounds__(LANE_TPB) void k_pr_write(ProfArgs pa) {
	__shared__ ProfileSegment sh_segs[PROFILE_MAX_SEGMENTS];
	__shared__ uint32_t sh_seg[2][16];
	stage_segments(pa, sh_segs);
	__syncthreads();
	const QueryArgs& q = pa.q;
	const ExportArgs& a = q.x;
	const Header* hdr = reinterpret_cast<const Header*>(a.scratch);
	const QItem* items = reinterpret_cast<const QItem*>(a.scratch + a.lay.items);
	const uint64_t numItems = hdr->numItems;                                // (0 for a count-only call and after a capacity error: nothing is written)
	const int lane = lane_id(), w = (int)(threadIdx.x / SIMLOD_WAVE);
	const uint64_t below = (1ull << lane) - 1ull;
	const bool withRecords = pa.records != nullptr;
	uint32_t turn = 0;
	for (uint64_t i = blockIdx.x; i < numItems; i += gridDim.x) {
		const QItem it = items[i];
		if (it.count == 0u) continue;                                       // (the same for the whole workgroup, as every branch on `it`)
		const u32x4* s = reinterpret_cast<const u32x4*>(it.src);
		const uint64_t base = a.table[it.node].firstSample;
		u32x4* d = reinterpret_cast<u32x4*>(a.samples + base);
		u32x4* r = withRecords ? reinterpret_cast<u32x4*>(pa.records + base) : nullptr;
		u32x4 v[4], rec[4];
		if (it.tag == Q_COPIED) {
			load_chunk4<true, false>(s, it.count, v);
			const uint64_t at = (uint64_t)it.k * SIMLOD_POINTS_PER_CHUNK;
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
				if (k < it.count) {
					__builtin_nontemporal_store(v[j], d + at + k);
					if (withRecords) {
						locate_record(pa.f, sh_segs, v[j], rec[j]);
						__builtin_nontemporal_store(rec[j], r + at + k);
					}
				}
			}
			continue;
		}
		if (it.tag != Q_FILTERED || it.pass == 0u) continue;
		load_chunk4<true, true>(s, it.count, v);
		uint64_t b[4];
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t k = threadIdx.x + (uint32_t)j * LANE_TPB;
			b[j] = __ballot(k < it.count && passes(q.g, v[j]) && locate_record(pa.f, sh_segs, v[j], rec[j]) < pa.f.n);
			if (lane == 0) sh_seg[turn][j * 4 + w] = (uint32_t)__popcll(b[j]);
		}
		__syncthreads();                    // (two buffers, as in k_q_count)
		d += it.off;                        // samples of the node that pass before this item
		r += it.off;
		uint32_t run = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) {
#pragma unroll
			for (int ww = 0; ww < 4; ww++) {
				if (ww == w && ((b[j] >> lane) & 1ull)) {
					const uint32_t at = run + (uint32_t)__popcll(b[j] & below);
					__builtin_nontemporal_store(v[j], d + at);
					if (withRecords) __builtin_nontemporal_store(rec[j], r + at);
				}
				run += sh_seg[turn][j * 4 + ww];
			}
		}
		turn ^= 1u;
	}
}
