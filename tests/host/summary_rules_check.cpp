// summary_rules_check.cpp — simlod_amd/csrc/summary_rules.hpp on the host, alone: which SimlodSummaryParams records a call accepts (rule S8), the
// key of rule S1, the cell of rule S2 and, through paint_rules.hpp, the index of rule S3.  A program of its own (tests/test_summary_rules.py
// builds it with the address and undefined-behaviour sanitizers, runs it and compares every line it prints with tests/summary_ref.py).
//   input:  u32 numParams, u32 numValues, f32 boxMin, f32 size, f32 z0, f32 scale, numParams x SimlodSummaryParams, numValues x u32 (the bits
//           of an fp32 coordinate)
//   output: per record a line "p <index> <accepted>", per value a line "v <bits> <key> <unkey(key)> <is_nan> <is_finite> <cell> <index>", all
//           integers in hexadecimal; the cell from boxMin and summary_inv(size), the index from z0 and scale
#include "summary_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

int main(int argc, char** argv) {
	if (argc != 2) { std::printf("usage: summary_rules_check <cases>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t head[2];
	float box[4];
	if (std::fread(head, 4, 2, in) != 2 || std::fread(box, 4, 4, in) != 4) { std::printf("short header\n"); return 2; }
	const uint32_t np = head[0], nv = head[1];
	std::vector<SimlodSummaryParams> params(np);
	std::vector<uint32_t> values(nv);
	auto read = [&](void* to, size_t bytes, size_t count) { return count == 0 || std::fread(to, bytes, count, in) == count; };   // (an empty vector has no data())
	if (!read(params.data(), sizeof(SimlodSummaryParams), np) || !read(values.data(), 4, nv)) { std::printf("short body\n"); return 2; }
	std::fclose(in);
	for (uint32_t i = 0; i < np; i++) std::printf("p %x %x\n", i, summary_acceptable(params[i]) ? 1u : 0u);
	const double inv = summary_inv(box[1]);
	for (uint32_t i = 0; i < nv; i++) {
		const uint32_t b = values[i];
		float x;
		std::memcpy(&x, &b, 4);
		const uint32_t k = summary_key(b);
		std::printf("v %x %x %x %x %x %x %x\n", b, k, summary_unkey(k), summary_is_nan(b) ? 1u : 0u, summary_is_finite(b) ? 1u : 0u,
		            summary_cell20(x, (double)box[0], inv), paint_ramp_index(x, box[2], box[3]));
	}
	return 0;
}
