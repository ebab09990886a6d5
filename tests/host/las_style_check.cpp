// las_style_check.cpp — simlod_amd/csrc/las_style_rules.hpp on the host, alone: what simlod_decode_las_styled accepts and where it looks for the
// attribute.  A program of its own (tests/test_las_style.py builds it with the address and undefined-behaviour sanitizers and runs it on a file of cases).
//   input:  u32 numCases, numCases x { SimlodLasStyle, u32 bytesPerPoint, u32 format }
//   output: per case u32 { accepted, kind, offset, bytes, shift, mask, sign, milli-mul } — zeros behind `accepted` for a case that is refused
//   stdout: the layout of SimlodLasStyle as this compiler sees it
#include "las_style_rules.hpp"

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

int main(int argc, char** argv) {
	if (argc != 3) { std::printf("usage: las_style_check <cases> <out>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t count = 0;
	if (std::fread(&count, 4, 1, in) != 1) { std::printf("short header\n"); return 2; }
	std::vector<uint32_t> out;
	for (uint32_t i = 0; i < count; i++) {
		SimlodLasStyle s;
		uint32_t tail[2];
		if (std::fread(&s, sizeof(s), 1, in) != 1 || std::fread(tail, 4, 2, in) != 2) { std::printf("short body\n"); return 2; }
		LasField f{};
		const bool ok = las_style_acceptable(s, tail[0], tail[1], f);
		if (!ok) f = LasField{};
		const uint32_t row[8] = {ok ? 1u : 0u, f.kind, f.offset, f.bytes, f.shift, f.mask, f.sign, (uint32_t)(f.mul * 1000.0 + 0.5)};
		out.insert(out.end(), row, row + 8);
	}
	std::fclose(in);
	FILE* o = std::fopen(argv[2], "wb");
	if (o == nullptr || std::fwrite(out.data(), 4, out.size(), o) != out.size()) { std::printf("cannot write %s\n", argv[2]); return 2; }
	std::fclose(o);
	std::printf("sizeof %zu attribute %zu reserved %zu lo %zu hi %zu lut %zu count %d\n", sizeof(SimlodLasStyle), offsetof(SimlodLasStyle, attribute),
	            offsetof(SimlodLasStyle, reserved), offsetof(SimlodLasStyle, lo), offsetof(SimlodLasStyle, hi), offsetof(SimlodLasStyle, lut), (int)SIMLOD_LAS_ATTRIBUTE_COUNT);
	return 0;
}
