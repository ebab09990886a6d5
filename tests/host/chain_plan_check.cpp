// chain_plan_check.cpp — the host side of chained construct launches (simlod_amd/csrc/octree_state.hpp: size_launch with a chain's limit, chain_groups,
// chain_segments_per_launch, chain_cut, chain_goes_plain, shrink_planned), alone on the host.  A program of its own (tests/test_chain_plan.py builds it with the
// address and undefined-behaviour sanitizers and runs it); exit status 0 = every check held.  Every row is worked by hand in tests/test_chain_plan.py.
#include "octree_state.hpp"

#include <cstdio>

using namespace simlod;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                  \
	do {                                                                                  \
		if (!(cond)) { g_failed++; std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
	} while (0)
#define ROW(name, got, want) do { const uint32_t g_ = (got); CHECK(g_ == (uint32_t)(want), "row %s: %u, expected %u", name, g_, (uint32_t)(want)); } while (0)

static constexpr uint32_t NS = NOTHING_SEEN;
static uint32_t g_pool[32][16];
static int g_allocs = 0;
static volatile uint32_t* fake_words() { return g_allocs < 32 ? g_pool[g_allocs++] : nullptr; }

struct Octree {
	std::vector<OctreeState> reg;
	LaunchHistory* h;
	Octree() { h = &octree_of(reg, this, fake_words).history; }
	void report(uint32_t index, uint32_t uploaded, uint32_t fit, uint32_t seq) { h->seen[0] = index; h->seen[1] = uploaded; h->seen[2] = fit; h->seen[3] = seq; }
	// a chain of `launches` with batch limit L: sized as ONE launch with limit launches x L
	LaunchPlan chain(int hinted, int told, uint32_t launches, uint32_t L = SIMLOD_MAX_BATCHES_PER_LAUNCH) {
		const uint32_t seen[4] = {h->seen[0], h->seen[1], h->seen[2], h->seen[3]};
		const uint32_t before = h->seq;
		const LaunchPlan s = size_launch(h, seen, hinted, launches * L, told >= 0, told >= 0 ? (uint32_t)told : 0u);
		CHECK(h->seq == before + 1u && h->enq[h->seq % 32u] == s.batches, "a chain is ONE launch in the history, sized for its total");
		return s;
	}
};

static void check_sizing() {
	static_assert(SIMLOD_MAX_BATCHES_PER_LAUNCH == 20u, "the rows are worked out for 20");
	{   // S1: told counter.  Reset through the library (not yet reported), the host has published 36: a chain of 2 is sized 36, a chain of 3 too (cap 60)
		Octree a; forget_history(a.h); ROW("S1 chain of 2", a.chain(-1, 36, 2).batches, 36u);
		Octree b; forget_history(b.h); ROW("S1 chain of 3", b.chain(-1, 36, 3).batches, 36u);
		// ... and 50 published against a chain of 2: its cap, 40; the launch behind it finds the 10 that are left (50 - 0 - 40 in flight)
		Octree c; forget_history(c.h); ROW("S1 cap", c.chain(-1, 50, 2).batches, 40u);
		ROW("S1 behind the chain", c.chain(-1, 50, 1).batches, 10u);
	}
	{   // S2: the hint may name up to launches x L: 36 for a chain of 2; 50 is cut to 40; with L = 7, a chain of 3 takes a hint of 20 whole and 25 cut to 21
		Octree a; ROW("S2 36", a.chain(36, -1, 2).batches, 36u);
		Octree b; ROW("S2 50", b.chain(50, -1, 2).batches, 40u);
		Octree c; ROW("S2 L7 20", c.chain(20, -1, 3, 7u).batches, 20u);
		Octree d; ROW("S2 L7 25", d.chain(25, -1, 3, 7u).batches, 21u);
	}
	{   // S3: reports only (a host that tells nothing).  Reset reported (0, 0), then a launch reported index 20 of 50 seen: pending 30, one report says nothing
		// about the pace (arrivals = 20): want 50 — a chain of 2 is cut to 40, a chain of 3 gets 50
		Octree a; const uint32_t r = forget_history(a.h); a.report(0u, 0u, 1u, r);
		a.h->seq += 1u; a.h->enq[a.h->seq % 32u] = 20u; a.report(20u, 50u, 1u, a.h->seq);
		Octree b; const uint32_t rb = forget_history(b.h); b.report(0u, 0u, 1u, rb);
		b.h->seq += 1u; b.h->enq[b.h->seq % 32u] = 20u; b.report(20u, 50u, 1u, b.h->seq);
		ROW("S3 chain of 2", a.chain(-1, -1, 2).batches, 40u);
		ROW("S3 chain of 3", b.chain(-1, -1, 3).batches, 50u);
	}
	{   // S4: a silent host after a reset, nothing reported (seen = NS): nothing is known, the chain is sized for its cap — 40, 60; L = 7, three launches: 21
		Octree a; forget_history(a.h); CHECK(a.h->seen[0] == NS, "forget_history"); ROW("S4 2", a.chain(-1, -1, 2).batches, 40u);
		Octree b; forget_history(b.h); ROW("S4 3", b.chain(-1, -1, 3).batches, 60u);
		Octree c; forget_history(c.h); ROW("S4 L7", c.chain(-1, -1, 3, 7u).batches, 21u);
		Octree d; ROW("S4 one launch stays 20", d.chain(-1, -1, 1).batches, 20u);
	}
	{   // S5: a chain that goes plain becomes the plan of its first launch: 36 sized, take 1 -> 20, and the history remembers 20
		Octree a; forget_history(a.h);
		LaunchPlan p = a.chain(-1, 36, 2);
		CHECK(chain_goes_plain(p.batches, 20u, 1u), "take == 1 goes plain");
		shrink_planned(a.h, &p, 20u);
		CHECK(p.batches == 20u && a.h->enq[a.h->seq % 32u] == 20u, "shrink_planned: %u, %u", p.batches, a.h->enq[a.h->seq % 32u]);
		ROW("S5 the launch behind it", a.chain(-1, 36, 1).batches, 16u);
	}
}

static void check_groups() {
	// (pending, L, take) -> groups, the sum over segments of ceil(segment / take)
	ROW("G 21", chain_groups(21u, 20u, 5u), 5u);         // 5,5,5,5 | 1
	ROW("G 36", chain_groups(36u, 20u, 5u), 8u);         // 5,5,5,5 | 5,5,5,1
	ROW("G 41", chain_groups(41u, 20u, 5u), 9u);         // 4 | 4 | 1
	ROW("G 50", chain_groups(50u, 20u, 5u), 10u);        // 4 | 4 | 5,5
	ROW("G 20", chain_groups(20u, 20u, 5u), 4u);
	ROW("G L7", chain_groups(20u, 7u, 5u), 6u);          // 5,2 | 5,2 | 5,1
	ROW("G take 2", chain_groups(50u, 20u, 2u), 25u);    // 10 | 10 | 5
	ROW("G 12 of 3", chain_groups(12u, 20u, 5u), 3u);    // 5,5,2
	ROW("G none", chain_groups(0u, 20u, 5u), 0u);
	ROW("G coalesced 36 by 10", chain_groups(36u, 20u, 10u), 4u);   // 10,10 | 10,6
	ROW("G coalesced 36 by 3", chain_groups(36u, 20u, 3u), 13u);    // 7 | 3,3,3,3,3,1
	ROW("G one launch", chain_groups(13u, 20u, 5u), 3u);             // ceil(13 / 5), as before chains
	ROW("G take 1", chain_groups(36u, 20u, 1u), 36u);
	// plain: batch by batch, or at most one group
	CHECK(chain_goes_plain(36u, 20u, 1u) && chain_goes_plain(5u, 20u, 5u) && chain_goes_plain(0u, 20u, 5u) && !chain_goes_plain(6u, 20u, 5u) && !chain_goes_plain(36u, 20u, 5u), "chain_goes_plain");
}

static void check_cut() {
	// segments a device launch holds: floor(20 / groups per whole segment), at least one
	ROW("C 5", chain_segments_per_launch(20u, 5u), 5u);      // 4 groups per segment
	ROW("C 2", chain_segments_per_launch(20u, 2u), 2u);      // 10
	ROW("C 3", chain_segments_per_launch(20u, 3u), 2u);      // 7
	ROW("C 12", chain_segments_per_launch(20u, 12u), 10u);   // 2
	ROW("C 20", chain_segments_per_launch(20u, 20u), 20u);   // 1
	ROW("C 1", chain_segments_per_launch(20u, 1u), 1u);      // 20
	ROW("C L7", chain_segments_per_launch(7u, 5u), 10u);     // 2
	// SIMLOD_EXACT_GROUP=2, 50 batches, a chain of 3: device launches of 2 and 1 segments — 20 and 5 groups
	ROW("C cut 0", chain_cut(3u, 20u, 2u, 0u), 2u);
	ROW("C cut 1", chain_cut(3u, 20u, 2u, 1u), 1u);
	ROW("C cut 2", chain_cut(3u, 20u, 2u, 2u), 0u);
	ROW("C cut groups 0", chain_groups(40u, 20u, 2u), 20u);
	ROW("C cut groups 1", chain_groups(10u, 20u, 2u), 5u);
	// groups of five: a chain of 3 is one device launch; a chain of 7 is 5 + 2
	ROW("C five 0", chain_cut(3u, 20u, 5u, 0u), 3u);
	ROW("C five 1", chain_cut(3u, 20u, 5u, 1u), 0u);
	ROW("C seven 0", chain_cut(7u, 20u, 5u, 0u), 5u);
	ROW("C seven 1", chain_cut(7u, 20u, 5u, 1u), 2u);
	// no cut ever numbers a group beyond the tables
	for (uint32_t L = 1u; L <= 20u; L++)
		for (uint32_t take = 1u; take <= 20u; take++)
			CHECK(chain_groups(chain_segments_per_launch(L, take) * L, L, take) <= SIMLOD_MAX_BATCHES_PER_LAUNCH, "L %u take %u", L, take);
}

int main() {
	check_sizing();
	check_groups();
	check_cut();
	if (g_failed == 0) std::printf("chain_plan_check: ok\n");
	return g_failed == 0 ? 0 : 1;
}
