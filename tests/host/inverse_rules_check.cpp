// inverse_rules_check.cpp — simlod_amd/csrc/inverse_rules.hpp on the host, alone: the class map of rule I2, the sample rule I1 and rule I9's own
// refusal.  A program of its own (tests/test_inverse_rules.py builds it with the address and undefined-behaviour sanitizers and runs it on a file
// of positive classes; the test compares what it writes with the numpy class map of tests/inverse_ref.py).
//   input:  u32 numNodes, numNodes x u32 positive class (0 outside, 1 filtered, 2 copied)
//   output: numNodes x u8 inverse class, then u8 inverse_passes(false), u8 inverse_passes(true), then four u8: inverse_polygons_acceptable for
//           (no polygon), (footprint), (lasso), (both)
#include "inverse_rules.hpp"

#include <cstdio>
#include <vector>

using namespace simlod;

int main(int argc, char** argv) {
	if (argc != 3) { std::printf("usage: inverse_rules_check <classes> <out>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t n = 0;
	if (std::fread(&n, 4, 1, in) != 1) { std::printf("short header\n"); return 2; }
	std::vector<uint32_t> positive(n);
	if (std::fread(positive.data(), 4, n, in) != n) { std::printf("short body\n"); return 2; }
	std::fclose(in);
	std::vector<uint8_t> out;
	for (uint32_t c : positive) out.push_back((uint8_t)inverse_class(c));
	out.push_back(inverse_passes(false) ? 1 : 0);
	out.push_back(inverse_passes(true) ? 1 : 0);
	const int fp = 0, lasso = 0;                                              // (any two objects: only the pointers are looked at)
	out.push_back(inverse_polygons_acceptable(nullptr, nullptr) ? 1 : 0);
	out.push_back(inverse_polygons_acceptable(&fp, nullptr) ? 1 : 0);
	out.push_back(inverse_polygons_acceptable(nullptr, &lasso) ? 1 : 0);
	out.push_back(inverse_polygons_acceptable(&fp, &lasso) ? 1 : 0);
	FILE* o = std::fopen(argv[2], "wb");
	if (o == nullptr || std::fwrite(out.data(), 1, out.size(), o) != out.size()) { std::printf("cannot write %s\n", argv[2]); return 2; }
	std::fclose(o);
	return 0;
}
