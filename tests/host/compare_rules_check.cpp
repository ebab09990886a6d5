// compare_rules_check.cpp — simlod_amd/csrc/compare_rules.hpp on the host, alone: which SimlodCompareParams records, boxes and counts a call
// accepts, rule C4's h and inv, a sample's validity and its cell's 60-bit key, a key's home slot, the table's capacity, and rule C5's threshold
// index.  A program of its own (tests/test_compare_rules.py builds it with the address and undefined-behaviour sanitizers, runs it and compares
// every line it prints with tests/compare_ref.py).
//   input:  u32 numParams, u32 numValues, u32 numD2, u32 numKeys, u32 numCounts, u32 pad, f32 boxMin, f32 size, numParams x SimlodCompareParams,
//           numValues x u32 (the bits of an fp32 coordinate), numD2 x f64, numKeys x u64, numCounts x u64
//   output: per record "p <index> <accepted>"; one line "g <bits of h> <bits of inv> <box accepted>" from the first record's radius; per value
//           "v <bits> <cell>"; per three consecutive values "k <valid> <key>"; per d2 "i <bits> <index>" against the first record's thresholds;
//           per key "h <key> <home at 2 slots> <at 2^15> <at 2^33>"; per count "s <count> <accepted> <slots> <log2>"; integers in hexadecimal
#include "compare_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

static uint64_t bits_of(double d) {
	uint64_t b;
	std::memcpy(&b, &d, 8);
	return b;
}

int main(int argc, char** argv) {
	if (argc != 2) { std::printf("usage: compare_rules_check <cases>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t head[6];
	float box[2];
	if (std::fread(head, 4, 6, in) != 6 || std::fread(box, 4, 2, in) != 2) { std::printf("short header\n"); return 2; }
	const uint32_t np = head[0], nv = head[1], nd = head[2], nk = head[3], nc = head[4];
	if (np == 0) { std::printf("no record\n"); return 2; }
	std::vector<SimlodCompareParams> params(np);
	std::vector<uint32_t> values(nv);
	std::vector<double> d2(nd);
	std::vector<uint64_t> keys(nk), counts(nc);
	auto read = [&](void* to, size_t bytes, size_t count) { return count == 0 || std::fread(to, bytes, count, in) == count; };   // (an empty vector has no data())
	if (!read(params.data(), sizeof(SimlodCompareParams), np) || !read(values.data(), 4, nv) || !read(d2.data(), 8, nd) || !read(keys.data(), 8, nk) ||
	    !read(counts.data(), 8, nc)) { std::printf("short body\n"); return 2; }
	std::fclose(in);
	for (uint32_t i = 0; i < np; i++) std::printf("p %x %x\n", i, compare_acceptable(params[i]) ? 1u : 0u);
	const float mn[3] = {box[0], box[0], box[0]};
	const double h = compare_h(params[0].radius, box[1]), inv = compare_inv(params[0].radius, box[1]);
	std::printf("g %llx %llx %x\n", (unsigned long long)bits_of(h), (unsigned long long)bits_of(inv), compare_box_acceptable(mn, box[1]) ? 1u : 0u);
	auto cell = [&](uint32_t b) {
		float x;
		std::memcpy(&x, &b, 4);
		return summary_cell20(x, (double)box[0], inv);
	};
	for (uint32_t i = 0; i < nv; i++) std::printf("v %x %x\n", values[i], cell(values[i]));
	for (uint32_t i = 0; i + 2 < nv; i++) {
		const bool valid = compare_valid(values[i], values[i + 1], values[i + 2]);
		const uint64_t key = valid ? compare_key(cell(values[i]), cell(values[i + 1]), cell(values[i + 2])) : 0u;
		std::printf("k %x %llx\n", valid ? 1u : 0u, (unsigned long long)key);
	}
	for (uint32_t i = 0; i < nd; i++) std::printf("i %llx %x\n", (unsigned long long)bits_of(d2[i]), compare_index(params[0].thresholds2, d2[i]));
	for (uint32_t i = 0; i < nk; i++)
		std::printf("h %llx %llx %llx %llx\n", (unsigned long long)keys[i], (unsigned long long)compare_home(keys[i], 1u),
		            (unsigned long long)compare_home(keys[i], 15u), (unsigned long long)compare_home(keys[i], 33u));
	for (uint32_t i = 0; i < nc; i++) {
		const bool ok = compare_count_acceptable(counts[i]);
		const uint64_t slots = ok ? compare_table_slots(counts[i]) : 0u;
		std::printf("s %llx %x %llx %x\n", (unsigned long long)counts[i], ok ? 1u : 0u, (unsigned long long)slots, ok ? compare_log2(slots) : 0u);
	}
	return 0;
}
