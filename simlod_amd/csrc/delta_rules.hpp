// delta_rules.hpp — the view delta's rules D2-D5 (include/simlod_hip.h, "view deltas"): the order of a table's entries as a key, the search of a
// key in a held table, the state of an entry against the held entry of its key, and what the two calls refuse in their own arguments.  No HIP in
// here: export_delta.inc's kernels, the launchers (export.hip) and tests/host/delta_rules_check.cpp (plain g++) read it here.
#pragma once
#include <stdint.h>
#include "simlod_hip.h"
#if defined(__HIPCC__)
#define SIMLOD_HD __host__ __device__
#else
#define SIMLOD_HD
#endif

namespace simlod {

// Every table is breadth-first with children in octant order (octant k: bit 2 from X, bit 1 from Y, bit 0 from Z), so its entries ascend by
// (level, Morton(X, Y, Z)) — a pair: a level-20 Morton code has 60 bits.  Bit i of a coordinate goes to bit 3 i (+ 2 for X, + 1 for Y).
SIMLOD_HD inline uint64_t delta_spread3(uint32_t v) {
	uint64_t x = v & 0x1fffffu;                                              // 21 bits: a coordinate is below 2^20, the bit above is kept apart
	x = (x | x << 32) & 0x001f00000000ffffull;
	x = (x | x << 16) & 0x001f0000ff0000ffull;
	x = (x | x << 8) & 0x100f00f00f00f00full;
	x = (x | x << 4) & 0x10c30c30c30c30c3ull;
	x = (x | x << 2) & 0x1249249249249249ull;
	return x;
}
struct DeltaKey { uint32_t level; uint64_t morton; };
SIMLOD_HD inline DeltaKey delta_key(uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	return DeltaKey{level, delta_spread3(X) << 2 | delta_spread3(Y) << 1 | delta_spread3(Z)};
}
SIMLOD_HD inline bool delta_key_less(const DeltaKey& a, const DeltaKey& b) { return a.level != b.level ? a.level < b.level : a.morton < b.morton; }

// rule D2: the index h < numHeld with held[h].(level, X, Y, Z) equal to the four words given, else SIMLOD_EXPORT_NONE.  A binary search for the
// first entry whose key is not below the wanted one — a probe loads the four key words of one entry, and which entry follows from the probe
// before it alone —, then the four words at the index found are compared.  Nothing outside held[0, numHeld) is read, whatever it holds; in a
// table that is not in key order an entry may be missed, never mistaken.
SIMLOD_HD inline uint32_t delta_find(const SimlodExportNode* held, uint32_t numHeld, uint32_t level, uint32_t X, uint32_t Y, uint32_t Z) {
	const DeltaKey want = delta_key(level, X, Y, Z);
	uint32_t lo = 0u, hi = numHeld;                                           // every entry in front of lo is below `want`, none from hi on
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		const SimlodExportNode& e = held[mid];
		if (delta_key_less(delta_key(e.level, e.X, e.Y, e.Z), want)) lo = mid + 1u; else hi = mid;
	}
	if (lo >= numHeld) return SIMLOD_EXPORT_NONE;
	const SimlodExportNode& e = held[lo];
	return e.level == level && e.X == X && e.Y == Y && e.Z == Z ? lo : SIMLOD_EXPORT_NONE;
}

// rules D3-D5: the state of a table entry (its flags and count n) against the held entry of its key (`found`; its flags and count), and the
// leading samples the receiver holds already.
SIMLOD_HD inline uint32_t delta_state(uint32_t flags, uint32_t n, bool found, uint32_t heldFlags, uint32_t heldSamples, uint32_t deltaFlags, uint32_t& numKept) {
	numKept = 0u;
	if (!(flags & SIMLOD_EXPORT_FLAG_SELECTED)) return SIMLOD_DELTA_NONE;
	const uint32_t hs = found && (heldFlags & SIMLOD_EXPORT_FLAG_SELECTED) ? heldSamples : 0u;
	const bool kind = found && ((flags ^ heldFlags) & SIMLOD_EXPORT_FLAG_LEAF) == 0u;
	if (kind && hs == n && n > 0u) { numKept = n; return SIMLOD_DELTA_KEPT; }
	if ((deltaFlags & SIMLOD_DELTA_TAILS) && kind && hs > 0u && hs < n) { numKept = hs; return SIMLOD_DELTA_GROWN; }
	return SIMLOD_DELTA_ADDED;
}

// What simlod_query_view_delta refuses in its own arguments (on top of what simlod_query_view refuses).
inline bool delta_acceptable(uint32_t deltaFlags, const void* held, uint32_t numHeld, const void* dropped, uint32_t droppedCapacity) {
	if ((deltaFlags & ~SIMLOD_DELTA_TAILS) != 0u) return false;
	if (held == nullptr && numHeld != 0u) return false;
	if (dropped == nullptr && droppedCapacity != 0u) return false;
	return true;
}

}  // namespace simlod
