// delta_rules_check.cpp — simlod_amd/csrc/delta_rules.hpp on the host (tests/test_delta_rules.py builds this with g++ and the address and
// undefined-behaviour sanitizers).
//   delta_rules_check <cases.bin> <out.bin>
// cases.bin: u32 numHeld, numNodes, numStates, numCalls; numHeld x SimlodExportNode (the held table, in an allocation of exactly that size);
//            numNodes x (u32 level, X, Y, Z); numStates x (u32 flags, n, found, heldFlags, heldSamples, deltaFlags);
//            numCalls x (u32 deltaFlags, held is null, numHeld, dropped is null, droppedCapacity).
// out.bin:   per node u32 delta_find's index, the low and the high word of its Morton code; per state u32 state, numKept; per call u32 accepted.
// Before anything else: delta_spread3 against a loop over the bits, and delta_key_less against the order of the coordinates' bits.
#include <cstdio>
#include <cstring>
#include <vector>

#include "delta_rules.hpp"

using namespace simlod;

static uint64_t spread_slow(uint32_t v) {
	uint64_t x = 0;
	for (int i = 0; i < 21; i++) x |= (uint64_t)((v >> i) & 1u) << (3 * i);
	return x;
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	uint32_t s = 12345u;
	for (int i = 0; i < 200000; i++) {
		s = s * 1664525u + 1013904223u;
		const uint32_t v = i < 21 ? 1u << i : i == 21 ? 0x1fffffu : (s >> 8) & 0x1fffffu;
		if (delta_spread3(v) != spread_slow(v)) { std::fprintf(stderr, "spread3(%#x)\n", v); return 1; }
	}
	// the first octant digit that differs, from the top, decides — X before Y before Z
	for (uint32_t bit = 0; bit < 20; bit++) {
		const DeltaKey lo = delta_key(20, 0, 0, (1u << bit) | ((1u << bit) - 1u)), y = delta_key(20, 0, 1u << bit, 0), x = delta_key(20, 1u << bit, 0, 0);
		if (!delta_key_less(lo, y) || !delta_key_less(y, x) || delta_key_less(x, lo) || delta_key_less(x, x)) { std::fprintf(stderr, "order at bit %u\n", bit); return 1; }
	}
	if (!delta_key_less(delta_key(19, 0x7ffff, 0x7ffff, 0x7ffff), delta_key(20, 0, 0, 0))) { std::fprintf(stderr, "levels\n"); return 1; }
	FILE* f = std::fopen(argv[1], "rb");
	if (f == nullptr) return 2;
	uint32_t head[4];
	if (std::fread(head, 4, 4, f) != 4) return 2;
	std::vector<SimlodExportNode> held(head[0]);                             // (exactly numHeld entries: a read past them is the sanitizer's to find)
	if (head[0] != 0u && std::fread(held.data(), sizeof(SimlodExportNode), head[0], f) != head[0]) return 2;
	std::vector<uint32_t> nodes(4u * head[1]), states(6u * head[2]), calls(5u * head[3]);
	if (head[1] != 0u && std::fread(nodes.data(), 16, head[1], f) != head[1]) return 2;
	if (head[2] != 0u && std::fread(states.data(), 24, head[2], f) != head[2]) return 2;
	if (head[3] != 0u && std::fread(calls.data(), 20, head[3], f) != head[3]) return 2;
	std::fclose(f);
	std::vector<uint32_t> out;
	for (uint32_t i = 0; i < head[1]; i++) {
		const uint32_t* k = &nodes[4 * i];
		out.push_back(delta_find(head[0] != 0u ? held.data() : nullptr, head[0], k[0], k[1], k[2], k[3]));
		const DeltaKey key = delta_key(k[0], k[1], k[2], k[3]);
		out.push_back((uint32_t)key.morton);
		out.push_back((uint32_t)(key.morton >> 32));
	}
	for (uint32_t i = 0; i < head[2]; i++) {
		const uint32_t* c = &states[6 * i];
		uint32_t kept = 0xdeadbeefu;
		out.push_back(delta_state(c[0], c[1], c[2] != 0u, c[3], c[4], c[5], kept));
		out.push_back(kept);
	}
	static const uint32_t word = 0u;
	for (uint32_t i = 0; i < head[3]; i++) {
		const uint32_t* c = &calls[5 * i];
		out.push_back(delta_acceptable(c[0], c[1] != 0u ? nullptr : &word, c[2], c[3] != 0u ? nullptr : &word, c[4]) ? 1u : 0u);
	}
	f = std::fopen(argv[2], "wb");
	if (f == nullptr || std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
	std::fclose(f);
	return 0;
}
