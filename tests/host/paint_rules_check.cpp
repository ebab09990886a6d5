// paint_rules_check.cpp — simlod_amd/csrc/paint_rules.hpp on the host, alone: which SimlodPaint records a call accepts (rule E9) and the colour
// word a sample gets (rules E1-E3).  A program of its own (tests/test_paint_rules.py builds it with the address and undefined-behaviour
// sanitizers and compares what it writes with tests/paint_ref.py and octree_io.Paint, byte for byte).  It forms a colour the way
// export_paint.inc's paint_colour does: by the record's mode, from the sample's colour word and the fp32 z.
//   input:  u32 numRecords, u32 numSamples, numRecords x SimlodPaint, numRecords x u32 haveColors, numSamples x {f32 z, u32 color}
//   output: per record u8 accepted, then — zeros when refused or for an ARRAY record — numSamples x u32 colour, numSamples x u32 ramp index
#include "paint_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

struct Sample { float z; uint32_t color; };

int main(int argc, char** argv) {
	if (argc != 3) { std::printf("usage: paint_rules_check <cases> <out>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t head[2];
	if (std::fread(head, 4, 2, in) != 2) { std::printf("short header\n"); return 2; }
	const uint32_t nr = head[0], ns = head[1];
	std::vector<SimlodPaint> records(nr);
	std::vector<uint32_t> have(nr);
	std::vector<Sample> samples(ns);
	auto read = [&](void* to, size_t bytes, size_t count) { return count == 0 || std::fread(to, bytes, count, in) == count; };   // (an empty vector has no data())
	if (!read(records.data(), sizeof(SimlodPaint), nr) || !read(have.data(), 4, nr) || !read(samples.data(), sizeof(Sample), ns)) {
		std::printf("short body\n");
		return 2;
	}
	std::fclose(in);
	FILE* o = std::fopen(argv[2], "wb");
	if (o == nullptr) { std::printf("cannot write %s\n", argv[2]); return 2; }
	auto write = [&](const void* from, size_t bytes, size_t count) { return count == 0 || std::fwrite(from, bytes, count, o) == count; };
	std::vector<uint32_t> colour(ns), index(ns);
	for (uint32_t r = 0; r < nr; r++) {
		const SimlodPaint& p = records[r];
		const uint8_t ok = paint_acceptable(p, have[r] != 0u) ? 1 : 0;
		if (ns != 0u) { std::memset(colour.data(), 0, ns * 4u); std::memset(index.data(), 0, ns * 4u); }
		if (ok != 0 && p.mode != SIMLOD_PAINT_ARRAY) {
			for (uint32_t i = 0; i < ns; i++) {
				if (p.mode == SIMLOD_PAINT_RAMP) index[i] = paint_ramp_index(samples[i].z, p.z0, p.scale);
				colour[i] = p.mode == SIMLOD_PAINT_SET ? p.color : p.mode == SIMLOD_PAINT_BLEND ? paint_blend(samples[i].color, p.color, p.strength) : p.table[index[i]];
			}
		}
		if (!write(&ok, 1, 1) || !write(colour.data(), 4, ns) || !write(index.data(), 4, ns)) { std::printf("cannot write %s\n", argv[2]); return 2; }
	}
	std::fclose(o);
	return 0;
}
