// octree_state_check.cpp — simlod_amd/csrc/octree_state.hpp on the host, alone: the launch sizing row by row, and the registry of per-octree records.
// A program of its own (tests/test_octree_state.py builds it with the address and undefined-behaviour sanitizers and runs it); exit status 0 = every check held.
#include "octree_state.hpp"

#include <cstdio>
#include <cstring>

using namespace simlod;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                  \
	do {                                                                                  \
		if (!(cond)) { g_failed++; std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
	} while (0)

static constexpr uint32_t NS = NOTHING_SEEN;

// ---- a fake page-locked allocator -------------------------------------------------------------------------------------------------------
static uint32_t g_pool[80][16];
static int g_allocs = 0;
static volatile uint32_t* fake_words() { return g_allocs < 80 ? g_pool[g_allocs++] : nullptr; }

// ---- sizing -----------------------------------------------------------------------------------------------------------------------------
struct Octree {      // one history with its own feedback words, as octree_of makes it
	std::vector<OctreeState> reg;
	LaunchHistory* h;
	Octree() { h = &octree_of(reg, this, fake_words).history; }
	Octree(const Octree& o) : reg(o.reg) {          // (a copy continues with words of its own)
		h = &reg[0].history;
		volatile uint32_t* mine = fake_words();
		for (int k = 0; k < 4; k++) mine[k] = o.h->seen[k];
		h->seen = mine;
	}
	void report(uint32_t index, uint32_t uploaded, uint32_t fit, uint32_t seq) { h->seen[0] = index; h->seen[1] = uploaded; h->seen[2] = fit; h->seen[3] = seq; }
	// one launch: hinted < 0: no hint; told < 0: the host has said nothing about its upload counter
	uint32_t launch(const char* row, int hinted, int told, uint32_t limit = SIMLOD_MAX_BATCHES_PER_LAUNCH) {
		const uint32_t seen[4] = {h->seen[0], h->seen[1], h->seen[2], h->seen[3]};
		const bool reported = seen[0] != NS && seen[1] != NS && (int32_t)(seen[3] - h->resetSeq) >= 0;
		const uint32_t before = h->seq;
		const LaunchPlan s = size_launch(h, seen, hinted, limit, told >= 0, told >= 0 ? (uint32_t)told : 0u);
		CHECK(s.feedback == h->seen && s.seq == h->seq && !s.sideTablesStale, "row %s: the launch reports into the history's words, under its number", row);
		CHECK(s.mayGroup == (!reported || seen[2] != 0u), "row %s: mayGroup %d, reported %d, seen[2] %u", row, (int)s.mayGroup, (int)reported, seen[2]);
		CHECK(h->seq == before + 1u && h->enq[h->seq % 32u] == s.batches, "row %s: the launch is numbered and remembered", row);
		return s.batches;
	}
	uint32_t reset() { return forget_history(h); }
};

#define ROW(name, got, want) do { const uint32_t g_ = (got); CHECK(g_ == (want), "row %s: %u batches, expected %u", name, g_, (uint32_t)(want)); } while (0)

static Octree after_reset_reported(uint32_t fit = 1u) {      // reset through the library, k_reset has reported: seen = 0, 0, fit, resetSeq
	Octree o;
	const uint32_t seq = o.reset();
	o.report(0u, 0u, fit, seq);
	return o;
}

static void check_sizing() {
	static_assert(SIMLOD_MAX_BATCHES_PER_LAUNCH == 20u, "the table is worked out for 20");
	{   // 1, 1b: a hint wins in any state — a new history, after a reset, with reports; cut by the limit
		Octree a; ROW("1 new", a.launch("1 new", 7, -1), 7u);
		Octree b; b.reset(); ROW("1 reset", b.launch("1 reset", 7, 0), 7u);
		Octree c = after_reset_reported(0u); c.report(3u, 6u, 0u, c.h->seq); ROW("1 reported", c.launch("1 reported", 7, 9), 7u);
		Octree d = after_reset_reported(); ROW("1b", d.launch("1b", 7, 5, 4u), 4u);
	}
	{   // 2: a history made by a launch (no reset through the library), nothing reported: everything, whatever the host has told
		Octree a; ROW("2 silent", a.launch("2 silent", -1, -1), 20u);
		Octree b; ROW("2 told", b.launch("2 told", -1, 5), 20u);
		Octree c; ROW("2 limit", c.launch("2 limit", -1, -1, 3u), 3u);
	}
	{   // 3, 4: reset through the library, k_reset not yet reported (seen = NS, NS, 1, 0)
		Octree a; a.reset();
		CHECK(a.h->seen[0] == NS && a.h->seen[1] == NS && a.h->seen[2] == 1u && a.h->seen[3] == 0u && a.h->resetKnown && a.h->resetSeq == 1u && a.h->seq == 1u, "forget_history");
		ROW("3", a.launch("3", -1, 5), 5u);
		Octree b; b.reset(); ROW("4", b.launch("4", -1, 0), 1u);
	}
	{   // 5: reset, k_reset reported, the host's value is the reset's zero: NOTHING is enqueued.  This is the known finding (a host that tells
		// nothing, uploads, launches once and waits gets a launch of zero groups once k_reset's own report has made `reported` true) — pinned as the code
		// has it, not fixed here
		Octree a = after_reset_reported(); ROW("5", a.launch("5", -1, 0), 0u);
	}
	{   // 6, 7: as 5, then one launch sized 5 in flight
		Octree a = after_reset_reported(0u);
		ROW("6 (the launch in flight)", a.launch("6-", -1, 5), 5u);
		Octree b = a;
		ROW("6", a.launch("6", -1, 8), 3u);
		ROW("7", b.launch("7", -1, 5), 1u);
	}
	{   // 8: a silent host (the library knows only its own reset's zero), the launches' reports alone
		Octree a = after_reset_reported();
		a.report(3u, 6u, 1u, a.h->seq); ROW("8a", a.launch("8a", -1, 0), 20u);
		a.report(6u, 9u, 1u, a.h->seq); ROW("8b", a.launch("8b", -1, 0), 6u);
		a.report(9u, 9u, 0u, a.h->seq); ROW("8c", a.launch("8c", -1, 0), 1u);
		a.report(9u, 9u, 0u, a.h->seq); ROW("8d", a.launch("8d", -1, 0), 1u);
	}
	{   // 9: a report whose sequence number is older than the latest reset is no report
		Octree a = after_reset_reported();
		a.launch("9-", -1, 3); a.launch("9-", -1, 6);           // launches 2 and 3
		a.reset();                                            // reset 4
		Octree none = a;
		a.report(3u, 6u, 0u, 2u);                             // launch 2 was still running: its words arrive behind the reset's clearing
		CHECK(none.h->seen[0] == NS && none.h->seq == a.h->seq, "row 9: the twin has no report");
		ROW("9 told", a.launch("9 told", -1, 5), none.launch("9 told twin", -1, 5));
		Octree b = after_reset_reported();
		b.launch("9-", -1, 3); b.reset(); b.report(1u, 3u, 0u, 1u);
		ROW("9 zero", b.launch("9 zero", -1, 0), 1u);         // (as row 4)
	}
	{   // 10: more than 32 launches since the report: what they were sized for is no longer known — not the told branch
		Octree a = after_reset_reported();                    // the report is number 1
		for (int k = 0; k < 31; k++) a.launch("10-", 0, 5);   // launches 2 .. 32, each hinted to nothing
		Octree edge = a;
		ROW("10 edge", edge.launch("10 edge", -1, 5), 5u);    // launch 33: 32 since the report, all of them known: told, 5 - 0
		a.launch("10-", 0, 5);                                // launch 33
		ROW("10", a.launch("10", -1, 5), 20u);                // launch 34: the prediction (nothing pending in the report, pace unknown: everything)
	}
}

// ---- registry ---------------------------------------------------------------------------------------------------------------------------
static void check_registry() {
	std::vector<OctreeState> reg;
	int arrays[70];
	const int allocsBefore = g_allocs;
	OctreeState& a0 = octree_of(reg, &arrays[0], fake_words);
	CHECK(a0.sideTablesStale && !a0.haveTable && !a0.rendered && !a0.imported && a0.nodes == &arrays[0], "a fresh record is stale and empty");
	CHECK(a0.history.seen != nullptr && a0.history.seen[0] == NS && a0.history.seen[1] == NS && a0.history.seen[2] == 1u && a0.history.seen[3] == 0u && a0.history.seq == 0u && !a0.history.resetKnown, "a fresh record's words say nothing");
	CHECK(a0.take_stale() && !a0.sideTablesStale && !a0.take_stale(), "taking the flag clears it");
	octree_of(reg, &arrays[1], fake_words).take_stale();
	OctreeState *A = find_octree(reg, &arrays[0]), *B = find_octree(reg, &arrays[1]);
	CHECK(A != nullptr && B != nullptr && A != B && reg.size() == 2 && g_allocs == allocsBefore + 2, "two records, two allocations");
	A->haveTable = true; B->haveTable = true;
	A->image_replaced();
	CHECK(A->sideTablesStale && !A->haveTable && !B->sideTablesStale && B->haveTable, "marking A does not show on B");
	CHECK(!B->take_stale() && A->sideTablesStale, "taking B's flag leaves A's");
	CHECK(A->take_stale() && !A->take_stale(), "A's flag is there once");
	CHECK(&octree_of(reg, &arrays[0], fake_words) == A && reg.size() == 2 && g_allocs == allocsBefore + 2, "a known array is found, not made again");

	// the parent's array_event switch, written out: {event, rendered before, imported before} -> {rendered, imported}
	static const struct { ArrayEvent e; bool r, i; } want[5] = {{ARRAY_RESET, false, false}, {ARRAY_CONSTRUCT, false, false /* imported: kept */}, {ARRAY_RENDERED, true, false /* kept */},
	                                                          {ARRAY_IMPORTED, false, true}, {ARRAY_IMPORTED_BUILDABLE, false, false}};
	for (int k = 0; k < 5; k++)
		for (int before = 0; before < 4; before++) {
			OctreeState s{};
			s.rendered = (before & 1) != 0; s.imported = (before & 2) != 0; s.sideTablesStale = true; s.haveTable = true;
			s.on(want[k].e);
			const bool keepsImported = want[k].e == ARRAY_CONSTRUCT || want[k].e == ARRAY_RENDERED;
			CHECK(s.rendered == want[k].r && s.imported == (keepsImported ? (before & 2) != 0 : want[k].i), "event %d from state %d: rendered %d imported %d", k, before, (int)s.rendered, (int)s.imported);
			CHECK(s.sideTablesStale && s.haveTable, "an array event touches nothing else");
		}

	// lookups of an unknown array change nothing
	const OctreeState snapshot = *A;
	CHECK(find_octree(reg, &arrays[69]) == nullptr && reg.size() == 2 && g_allocs == allocsBefore + 2 && std::memcmp(&snapshot, A, sizeof snapshot) == 0, "an unknown array is not found and nothing moves");

	// 64 records; the 65th array evicts the first, and gets its feedback words
	for (int k = 2; k < 64; k++) octree_of(reg, &arrays[k], fake_words);
	CHECK(reg.size() == OCTREES_KEPT && g_allocs == allocsBefore + 64 && find_octree(reg, &arrays[0]) != nullptr, "64 records are kept");
	volatile uint32_t* firstWords = find_octree(reg, &arrays[0])->history.seen;
	volatile uint32_t* secondWords = find_octree(reg, &arrays[1])->history.seen;
	firstWords[0] = 7u; firstWords[1] = 9u; firstWords[2] = 0u; firstWords[3] = 5u;          // (what a launch of the first array reported)
	OctreeState& late = octree_of(reg, &arrays[64], fake_words);
	CHECK(reg.size() == OCTREES_KEPT && find_octree(reg, &arrays[0]) == nullptr && find_octree(reg, &arrays[1]) != nullptr, "the 65th array evicts the first");
	CHECK(late.history.seen == firstWords && g_allocs == allocsBefore + 64, "the evicted record's words are handed on: nothing allocated, nothing to free");
	CHECK(firstWords[0] == NS && firstWords[1] == NS && firstWords[2] == 1u && firstWords[3] == 0u && late.sideTablesStale && late.history.seq == 0u, "the newcomer starts as any fresh record");
	OctreeState& back = octree_of(reg, &arrays[0], fake_words);                               // the first array again: it evicts the second
	CHECK(back.history.seen == secondWords && back.sideTablesStale && find_octree(reg, &arrays[1]) == nullptr && g_allocs == allocsBefore + 64, "an evicted array comes back stale, with the next oldest's words");
	int distinct = 0;
	for (const OctreeState& o : reg) for (int k = 0; k < 64; k++) if (o.history.seen == g_pool[allocsBefore + k]) distinct++;
	CHECK(distinct == 64, "every allocation is still owned by exactly one record");

	// the helper frame_feedback shares: hand on, else allocate; an allocator that has nothing left
	uint32_t w[16];
	CHECK(words_for_newcomer(w, fake_words) == w && g_allocs == allocsBefore + 64, "words_for_newcomer hands on");
	g_allocs = 80;
	std::vector<OctreeState> dry;
	OctreeState& none = octree_of(dry, &arrays[3], fake_words);
	CHECK(none.history.seen == nullptr && none.sideTablesStale && dry.size() == 1, "no page-locked memory: a record without words");
}

int main() {
	check_registry();
	g_allocs = 0;
	check_sizing();
	if (g_failed == 0) std::printf("octree_state_check: ok\n");
	return g_failed == 0 ? 0 : 1;
}
