// cluster_rules.hpp — the cluster queries' rules K3, K7-K9 and their refusals (include/simlod_hip.h, "cluster queries"): what a
// SimlodClusterParams record must be to be accepted, the core test, the record's constants, the bin of a size, the colour index, and the
// lock-free union-find that finds rule K4's components.  No HIP in here, and nothing of the library's other headers but the ABI's structs and
// compare_rules.hpp, whose validity, cell, h, key and d2 ARE rule K1's and are not restated: compare_cluster.inc's kernels and launcher and
// tests/host/cluster_rules_check.cpp (plain g++) read it here.
//
// The union-find works on an array `parent` of 32-bit indices through a small memory policy M with two members,
//   uint32_t load(uint32_t i)                                   parent[i], an atomic load
//   uint32_t cas(uint32_t i, uint32_t expected, uint32_t desired)   compare-and-swap on parent[i]; the value found there
// which the kernels instantiate with agent-scope relaxed atomics and the host check with std::atomic.  The invariant is parent[i] <= i, and a
// parent only ever DEcreases: cluster_link hangs the HIGHER of two roots under the lower, path splitting stores an ancestor.  So every chain
// is strictly descending and ends; the lowest index of a component can never get a parent and is its one root when every link is done
// (rule K4's root, whatever the schedule: rule K10).  No step waits for another thread.  A compare-and-swap that fails means that the root it
// aimed at got a lower parent meanwhile — progress somewhere else —, and the caller goes on from where it stands.  The count of one link in
// an array of n: the two indices it holds only ever move DOWN a chain, one place or more per step of a find, so the finds of one link take
// at most 2 * (n - 1) steps together; a failed compare-and-swap leaves its root with a lower parent, so the find that follows it takes at
// least one step, and there are no more failures than steps: at most 4 * (n - 1) steps and failures in all.  `budget` counts both and starts
// at 4 * n (cluster_link_budget), a number known at launch, so it is never spent; a loop that found it spent would give up with CLUSTER_MISS
// (rule K10's SIMLOD_CLUSTER_ERR_INTERNAL), it never spins.
#pragma once
#include <stdint.h>
#include <cmath>
#include "simlod_hip.h"
#include "compare_rules.hpp"

namespace simlod {

constexpr uint32_t CLUSTER_NOISE = SIMLOD_CLUSTER_NOISE;                      // rule K9: `cluster` of noise and of dissolved samples
constexpr uint32_t CLUSTER_MISS = SIMLOD_CLUSTER_MISS;                        // rule K9: `root` of true noise; no index (numA <= 2^32 - 2)
constexpr uint32_t CLUSTER_SIZE_BINS = SIMLOD_CLUSTER_SIZE_BINS;              // rule K9: floor(log2(size)) of sizes below 2^32, and one to spare

// the refusals of the record itself: the radius (rule C1), minNeighbours (rule K3), minClusterSize (rule K7), the reserved word
inline bool cluster_acceptable(const SimlodClusterParams& p) {
	return std::isfinite(p.radius) && p.radius >= 0.0f && p.minNeighbours >= 1u && p.minClusterSize >= 1u && p.reserved == 0u;
}

// rule K3
SIMLOD_HD inline bool cluster_is_core(uint32_t within, uint32_t minNeighbours) { return within >= minNeighbours; }
// rule K7
SIMLOD_HD inline bool cluster_is_kept(uint32_t size, uint32_t minClusterSize) { return size >= minClusterSize; }
// rule K9: floor(log2(size)) for size >= 1 (0 for size 0, which no cluster has)
SIMLOD_HD inline uint32_t cluster_size_bin(uint32_t size) {
	uint32_t b = 0u;
	while (size > 1u) { size >>= 1; b++; }
	return b;
}
// rule K9: the table entry of a kept cluster
SIMLOD_HD inline uint32_t cluster_colour_index(uint32_t cluster) { return cluster & 255u; }
// rule K9: largestSize and largestCluster as ONE number whose maximum is the largest size and, among equals, the lowest cluster number
SIMLOD_HD inline uint64_t cluster_largest_key(uint32_t size, uint32_t cluster) { return (uint64_t)size << 32 | (uint64_t)(0xffffffffu - cluster); }

// the find steps and failed compare-and-swaps one cluster_link may take in an array of n indices: more than the 4 * (n - 1) it can need
SIMLOD_HD inline uint64_t cluster_link_budget(uint64_t n) { return 4u * n; }

// The root above x: parent followed to its fixed point, every node passed given its grandparent on the way (path splitting: the stored value
// is an ancestor and lower than the one it replaces; a compare-and-swap, so that a lower value another thread stored meanwhile stays).
template <typename M>
SIMLOD_HD inline uint32_t cluster_find(M& m, uint32_t x, uint64_t& budget) {
	uint32_t p = m.load(x);
	while (p != x) {
		if (budget == 0u) return CLUSTER_MISS;
		budget--;
		const uint32_t g = m.load(p);
		if (g != p) m.cas(x, p, g);
		x = p;
		p = g;
	}
	return x;
}

// The same without a store, for a `parent` that no longer changes.
template <typename M>
SIMLOD_HD inline uint32_t cluster_root(M& m, uint32_t x, uint64_t& budget) {
	uint32_t p = m.load(x);
	while (p != x) {
		if (budget == 0u) return CLUSTER_MISS;
		budget--;
		x = p;
		p = m.load(x);
	}
	return x;
}

// a and b into one component -> a root both were under when it returned (the lower of their two roots), to go on from; CLUSTER_MISS: the
// budget is spent.  The short way out first: in a crowded cell nearly every pair is under one root already.
template <typename M>
SIMLOD_HD inline uint32_t cluster_link(M& m, uint32_t a, uint32_t b, uint64_t budget) {
	for (;;) {
		a = cluster_find(m, a, budget);
		b = cluster_find(m, b, budget);
		if (a == CLUSTER_MISS || b == CLUSTER_MISS) return CLUSTER_MISS;
		if (a == b) return a;
		if (a < b) { const uint32_t t = a; a = b; b = t; }
		if (m.cas(a, a, b) == a) return b;                                      // the higher root under the lower
		if (budget == 0u) return CLUSTER_MISS;                                  // (a got a lower parent meanwhile: on from a and b themselves)
		budget--;
	}
}

}  // namespace simlod
