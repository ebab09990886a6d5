// octree_state.hpp — what libsimlod_hip.so keeps for ONE octree between launches (one record per node array, in its context's registry), and how a
// kernel_construct launch is sized from it.  No HIP in here: the registry takes its page-locked words from an allocator the caller brings, the sizing is
// a function of plain numbers — tests/host/octree_state_check.cpp runs both on a machine without a GPU.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <mutex>
#include <vector>
#ifndef SIMLOD_MAX_BATCHES_PER_LAUNCH
#define SIMLOD_MAX_BATCHES_PER_LAUNCH 20u     // include/simlod_abi.h (voxels.cu:883), for a program that includes this header alone
#endif

namespace simlod {
struct LeafTableRef {
	const void*               nodes;
	const void*               block;       // start of the buffer the table lives in (the construct kernel's momentary buffer)
	const uint8_t*            table;       // rows of LEAF_ROW_BYTES (leaf_row_get)
	const uint8_t*            pers;        // the persistent buffer the rows' offsets refer to
	const uint32_t*           magic;
	const uint32_t*           batch;
	const uint64_t*           tableNodes;
	const uint64_t*           sig;         // table_signature() of the Stats the table was stamped for
	uint32_t                  magicValue, slots;
	uint32_t                  rows;        // rows the table has (the node capacity of the launch that registered it)
};
struct LaunchHistory {      // seen (page-locked, written by the launches' last kernels and by k_reset): [0] batchletIndex, [1] the upload counter, [2] fit for exact groups, [3] sequence number of the launch that wrote them
	volatile uint32_t* seen; uint32_t prevIndex, prevUploaded, arrivals; bool havePrev;
	uint32_t seq, resetSeq; bool resetKnown;      // launches (and resets) of this octree so far | the latest reset's number | ... and it ran through this library (index 0 from there on)
	uint32_t enq[32];                             // batches launch #seq was sized for
};
static constexpr uint32_t NOTHING_SEEN = 0xffffffffu;
struct LaunchPlan { uint32_t batches; bool mayGroup; uint32_t* feedback; uint32_t seq; bool sideTablesStale; };   // batches this launch can find (0: none — an idle frame) | exact groups allowed | where its last kernel reports, and as which launch | it rebuilds the side tables
enum ArrayEvent : int { ARRAY_RESET, ARRAY_CONSTRUCT, ARRAY_RENDERED, ARRAY_IMPORTED, ARRAY_IMPORTED_BUILDABLE };   // (buildable: grids and builder state, as after a reset)
using WordsAlloc = volatile uint32_t* (*)();      // 64 page-locked bytes for a launch's or a frame's feedback words, or nullptr (simlod_hip.cpp: hipHostMalloc)
// The words of a new registry entry: those of the entry that made room for it, else fresh ones.  The oldest entry's page-locked words are handed on,
// never freed while the context lives: a copy enqueued by an earlier launch may still be on its way into them (what arrives late is at worst a stale
// hint for the new owner: one launch with too many or too few groups, one frame that sorts or does not)
inline volatile uint32_t* words_for_newcomer(volatile uint32_t* handedOn, WordsAlloc alloc) { return handedOn != nullptr ? handedOn : alloc(); }

// One node array as the library knows it.  `nodes` is the key: two arrays may share a context, and each has its own record.
struct OctreeState {
	const void*   nodes;
	LeafTableRef  table; bool haveTable;         // builder -> rasteriser, export: where the octree's leaf chunk table lives (simlod_internal.hpp leaf_row_get), after a launch whose layout fits
	// a kernel_render ran on it since its last reset, construct or import (SIMLOD_EXPORT_VISIBLE reads the visible / isLarge bytes that frame wrote) | it holds an
	// imported octree (no grids, no builder state: kernel_construct and the colour filter refuse it until the next reset)
	bool          rendered, imported;
	bool          sideTablesStale;               // simlod_octree_image_replaced / a reset / an import: the next kernel_construct rebuilds its side tables whatever the stamp in the buffer says (an uploaded image with the same counters as the one it replaces: ADVICE r5)
	LaunchHistory history;                       // (history.seen == nullptr: no page-locked memory — launches are not sized)
	void on(ArrayEvent e) {
		switch (e) {
		case ARRAY_RESET: rendered = false; imported = false; break;
		case ARRAY_CONSTRUCT: rendered = false; break;
		case ARRAY_RENDERED: rendered = true; break;
		case ARRAY_IMPORTED: rendered = false; imported = true; break;
		case ARRAY_IMPORTED_BUILDABLE: rendered = false; imported = false; break;
		}
	}
	void image_replaced() { haveTable = false; sideTablesStale = true; }      // the octree in the buffers is not the one the builder's side tables and its chunk table describe
	bool take_stale() { const bool stale = sideTablesStale; sideTablesStale = false; return stale; }
};

// ---- the registry of a context (Context::octrees, under Context::octreesLock): 64 records, the oldest makes room ----------------------------------
static constexpr size_t OCTREES_KEPT = 64;
inline OctreeState* find_octree(std::vector<OctreeState>& octrees, const void* nodes) {
	for (OctreeState& o : octrees) if (o.nodes == nodes) return &o;
	return nullptr;
}
inline volatile uint32_t* evict_oldest_octree(std::vector<OctreeState>& octrees) {      // -> its feedback words, for the record that takes its place
	volatile uint32_t* seen = octrees.front().history.seen; octrees.erase(octrees.begin()); return seen;
}
// A record made anew starts STALE: every octree's life in this library begins with a reset, an import or simlod_octree_image_replaced, which say so anyway;
// what is left is a launch for an array the context has never seen or has evicted, and there rebuilding the side tables from the node array is the safe answer.
inline OctreeState& octree_of(std::vector<OctreeState>& octrees, const void* nodes, WordsAlloc alloc) {
	if (OctreeState* known = find_octree(octrees, nodes)) return *known;
	volatile uint32_t* seen = words_for_newcomer(octrees.size() >= OCTREES_KEPT ? evict_oldest_octree(octrees) : nullptr, alloc);
	if (seen != nullptr) { seen[0] = NOTHING_SEEN; seen[1] = NOTHING_SEEN; seen[2] = 1u; seen[3] = 0u; }
	OctreeState o{};
	o.nodes = nodes; o.sideTablesStale = true; o.history.seen = seen;
	octrees.push_back(o);
	return octrees.back();
}

// ---- launch sizing: how many batches a kernel_construct launch can find (simlod_hip.cpp launch_plan) ----------------------------------------------
// The reference's kernel loops over whatever has been uploaded when it starts (voxels.cu:870-885); here every group of batches is a handful of kernel
// launches the HOST enqueues before it can read that number (the upload counter lives on the device).  Kernels of a group without a batch leave at
// once, but its event hops stand in line behind the real work (~45 us per empty group).  What the host can know:
//   * the upload counter itself: the reference's uploader publishes it with cuMemsetD32Async(cptr_numBatchesUploaded, n, 1, stream_upload)
//     (main_progressive_octree.cpp:1047-1050) — shim/cuda.h passes every such write on (simlod_upload_counter_written), the Python mirror does the same;
//   * Stats.batchletIndex as the latest launch whose end the host has seen left it (k_finish stores it, the upload counter, whether the octree is
//     fit for exact groups, and the launch's sequence number into page-locked memory: no synchronisation), and how many batches the launches
//     enqueued since then were sized for.
// pending = uploaded - index - (what those launches will take).  A host that does not say (no shim, no hint): the counter the latest report saw + the
// uploader's pace, and never less than one group — a host that uploads, launches once and waits must not wait for ever.
// The launch is numbered ++h.seq.  seen: the four words of h.seen, read once | hinted: simlod_context_hint_pending_batches for this launch, else < 0 |
// hostKnown, uploadedHost: the host has said what it wrote to the upload counter, and what (simlod_upload_counter_written; a reset: zero)
// limit: the most this launch may take — the context's batch limit L (<= 20); a CHAIN of n launches (simlod_launch_construct_chain) is sized as ONE launch
// with limit n x L, and counts as one in enq[].
inline LaunchPlan size_launch(LaunchHistory* h, const uint32_t seen[4], int hinted, uint32_t limit, bool hostKnown, uint32_t uploadedHost) {
	LaunchPlan plan{SIMLOD_MAX_BATCHES_PER_LAUNCH, true, nullptr, 0u, false};
	const uint32_t seq = ++h->seq;
	plan.feedback = const_cast<uint32_t*>(h->seen); plan.seq = seq;
	const uint32_t index = seen[0], uploadedSeen = seen[1], reportSeq = seen[3];
	// a launch of this octree, or its reset, has ended and said so.  (A report from BEFORE the latest reset — a launch that was still running when the host
	// enqueued the reset writes its words after forget_launch_history cleared them — describes an octree that is gone: ignored; k_reset's own report follows it)
	const bool reported = index != NOTHING_SEEN && uploadedSeen != NOTHING_SEEN && (int32_t)(reportSeq - h->resetSeq) >= 0;
	plan.mayGroup = !reported || seen[2] != 0u;
	// what the launches enqueued behind the reporting one (or behind the reset, while nothing has reported) were sized for
	const uint32_t since = reported ? reportSeq : h->resetSeq;
	uint32_t inflight = 0;
	if (seq - since > 32u) inflight = NOTHING_SEEN;
	else for (uint32_t q = since + 1u; q != seq; q++) inflight += h->enq[q % 32u];
	const bool knowsStart = reported || h->resetKnown;                                  // index is known: the report's, or zero (a reset is in the stream ahead of this launch)
	const uint32_t indexNow = reported ? index : 0u;
	uint32_t want;
	if (hinted >= 0) want = (uint32_t)hinted;
	else if (knowsStart && inflight != NOTHING_SEEN && hostKnown && !(reported && uploadedSeen > uploadedHost)) {
		// (... unless a launch has SEEN more on the device than the host has told: a host that does not pass its counter writes on — the only value this
		// library knows is the zero of its own reset.  Such a host gets the prediction below)
		const uint32_t pending = uploadedHost > indexNow ? uploadedHost - indexNow : 0u;
		want = pending > inflight ? pending - inflight : 0u;
		// (a launch may take less than it was sized for — the memory guard, the time budget —: while the launches in flight have not reported, they
		// cannot be counted on to have taken everything, and this one enqueues one group: a frame loop must not stand still with batches pending)
		if (want == 0u && pending != 0u) want = 1u;
		// ... and nothing at all is enqueued only on the word of a host that has been HEARD since the reset or whose launches have reported: "zero uploaded"
		// right after a reset is also what a host that tells nothing looks like (it uploads, launches once and waits)
		if (want == 0u && !reported) want = 1u;
	} else if (!reported) want = std::max<uint32_t>(SIMLOD_MAX_BATCHES_PER_LAUNCH, limit);   // nothing is known: everything (a chain: its cap)
	else {
		// the host says nothing: what the latest report saw pending + what was uploaded between the last two reports (the uploader's pace per launch)
		const uint32_t pending = uploadedSeen > index ? uploadedSeen - index : 0u;
		if (!h->havePrev) h->arrivals = SIMLOD_MAX_BATCHES_PER_LAUNCH;                  // (one report says nothing about the pace)
		else if (index != h->prevIndex || uploadedSeen != h->prevUploaded)
			h->arrivals = uploadedSeen >= h->prevUploaded && index >= h->prevIndex ? uploadedSeen - h->prevUploaded : SIMLOD_MAX_BATCHES_PER_LAUNCH;   // (counters that went back: reset by other means)
		else if (pending == 0u) h->arrivals = 0u;                                       // the same numbers again and nothing pending: the loader is idle or done
		h->prevIndex = index; h->prevUploaded = uploadedSeen; h->havePrev = true;
		want = std::max<uint32_t>(1u, pending + h->arrivals);                           // (never nothing: such a host may upload, launch once and wait)
	}
	plan.batches = std::min<uint32_t>(want, limit);
	h->enq[seq % 32u] = plan.batches;
	return plan;
}
// ---- chained launches (simlod_launch_construct_chain): one k_begin, the groups of every segment, one tail ----------------------------------------
// A SEGMENT is what one of the chain's launches would have taken: L batches, counted from the chain's first.  Groups never straddle a segment
// boundary (voxel colours depend on the grouping: the chain's groups are those of the launch-by-launch run), so a launch sized for `batches`
// enqueues ceil(L / take) groups per whole segment and ceil(rest / take) for the last.
inline uint32_t chain_groups(uint32_t batches, uint32_t L, uint32_t take) {
	if (L == 0u || take == 0u) return 0u;
	return batches / L * ((L + take - 1u) / take) + (batches % L + take - 1u) / take;
}
// Group ordinals index tables of SIMLOD_MAX_BATCHES_PER_LAUNCH entries (events, Ctl.tagOf / voxT / segStart): the segments ONE device launch can hold.
// A chain of more is cut by the entry point into several device launches.
inline uint32_t chain_segments_per_launch(uint32_t L, uint32_t take) {
	const uint32_t perSegment = chain_groups(L, L, take);
	return perSegment == 0u ? 1u : std::max<uint32_t>(1u, SIMLOD_MAX_BATCHES_PER_LAUNCH / perSegment);
}
// the device launches of a chain of `launches`: how many segments device launch #k takes (k = 0, 1, ...; 0 when the chain has ended before it)
inline uint32_t chain_cut(uint32_t launches, uint32_t L, uint32_t take, uint32_t k) {
	const uint32_t per = chain_segments_per_launch(L, take);
	return (uint64_t)k * per >= launches ? 0u : std::min<uint32_t>(per, launches - k * per);
}
// A chain goes launch by launch, one plain launch per segment, when it would go batch by batch (take == 1) or finds at most one group: nothing to overlap at a seam
inline bool chain_goes_plain(uint32_t batches, uint32_t L, uint32_t take) { return take <= 1u || chain_groups(batches, L, take) <= 1u; }
// ... and the plan of a chain that goes plain becomes the plan of its first launch (the others are sized when they are enqueued)
inline void shrink_planned(LaunchHistory* h, LaunchPlan* plan, uint32_t L) {
	plan->batches = std::min<uint32_t>(plan->batches, L);
	if (h != nullptr && plan->feedback != nullptr) h->enq[plan->seq % 32u] = plan->batches;
}

// A reset through this library (the reset is numbered ++h.seq, the return value): nothing ingested, nothing uploaded, as k_reset will report in stream order
inline uint32_t forget_history(LaunchHistory* h) {
	h->seen[0] = NOTHING_SEEN; h->seen[1] = NOTHING_SEEN; h->seen[2] = 1u;
	h->havePrev = false;
	h->resetSeq = ++h->seq; h->resetKnown = true;
	h->enq[h->seq % 32u] = 0u;
	return h->seq;
}
}  // namespace simlod
