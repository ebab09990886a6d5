// surface_rules_check.cpp — simlod_amd/csrc/surface_rules.hpp on the host, alone: which SimlodSurfaceParams records a call accepts, rule N2's
// invq and quantised offset, rule N3's widening D, rule N4's factor, and rules N3-N8 from a sample's nine sums to its normal, its two
// variation numbers and its colour index.  A program of its own (tests/test_surface_rules.py builds it with the address and
// undefined-behaviour sanitizers, runs it and compares every line it prints with tests/surface_ref.py).
//   input:  u32 numParams, u32 numOffsets, u32 numSums, u32 numMatrices, u32 numSamples, u32 pad, f32 radius, f32 size,
//           numParams x SimlodSurfaceParams, numOffsets x f64, numSums x i64, numMatrices x 6 f64, numSamples x Sample (below)
//   output: per record "p <index> <accepted>"; one line "g <bits of invq>"; per offset "q <bits> <q as u32>"; per sum "d <sum> <bits of D>";
//           per matrix "f <bits of f> <m != 0>"; per sample "e <index> <estimated> <bits of v0 v1 v2> <bits of lambdaNum lambdaDen vv>
//           <bits of the fp32 normal x3> <bits of num den> <index>" (zeros after <estimated> when degenerate), the index against the
//           thresholds of the record the sample names; integers in hexadecimal
#include "surface_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

struct Sample {
	int64_t  S[SURFACE_SUMS];
	double   c[3];
	uint32_t within, params;           // params: which record's orientation, light, colourBy and thresholds
};
static_assert(sizeof(Sample) == 104, "Sample");

static uint32_t bits32(float f) {
	uint32_t b;
	std::memcpy(&b, &f, 4);
	return b;
}

int main(int argc, char** argv) {
	if (argc != 2) { std::printf("usage: surface_rules_check <cases>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t head[6];
	float box[2];
	if (std::fread(head, 4, 6, in) != 6 || std::fread(box, 4, 2, in) != 2) { std::printf("short header\n"); return 2; }
	const uint32_t np = head[0], no = head[1], ns = head[2], nm = head[3], ne = head[4];
	if (np == 0) { std::printf("no record\n"); return 2; }
	std::vector<SimlodSurfaceParams> params(np);
	std::vector<double> offsets(no), matrices((size_t)nm * 6u);
	std::vector<int64_t> sums(ns);
	std::vector<Sample> samples(ne);
	auto read = [&](void* to, size_t bytes, size_t count) { return count == 0 || std::fread(to, bytes, count, in) == count; };   // (an empty vector has no data())
	if (!read(params.data(), sizeof(SimlodSurfaceParams), np) || !read(offsets.data(), 8, no) || !read(sums.data(), 8, ns) ||
	    !read(matrices.data(), 48, nm) || !read(samples.data(), sizeof(Sample), ne)) { std::printf("short body\n"); return 2; }
	std::fclose(in);
	for (uint32_t i = 0; i < np; i++) std::printf("p %x %x\n", i, surface_acceptable(params[i]) ? 1u : 0u);
	const double invq = surface_invq(box[0], box[1]);
	std::printf("g %llx\n", (unsigned long long)surface_bits(invq));
	for (uint32_t i = 0; i < no; i++) std::printf("q %llx %x\n", (unsigned long long)surface_bits(offsets[i]), (uint32_t)surface_q(offsets[i], invq));
	for (uint32_t i = 0; i < ns; i++) std::printf("d %llx %llx\n", (unsigned long long)sums[i], (unsigned long long)surface_bits(surface_D(sums[i])));
	for (uint32_t i = 0; i < nm; i++) {
		double s[SYM_ENTRIES], f;
		for (int k = 0; k < SYM_ENTRIES; k++) s[k] = matrices[(size_t)i * 6u + k];
		const bool ok = surface_factor(s, f);
		std::printf("f %llx %x\n", (unsigned long long)surface_bits(f), ok ? 1u : 0u);
	}
	for (uint32_t i = 0; i < ne; i++) {
		const Sample& s = samples[i];
		if (s.params >= np) { std::printf("sample %u names record %u\n", i, s.params); return 2; }
		const SimlodSurfaceParams& p = params[s.params];
		const double orient[3] = {(double)p.orient[0], (double)p.orient[1], (double)p.orient[2]};
		const double light[3] = {(double)p.light[0], (double)p.light[1], (double)p.light[2]};
		SurfaceEstimate e;
		if (!surface_estimate(s.S, s.within, s.c, orient, p.orientMode, e)) {
			std::printf("e %x 0 0 0 0 0 0 0 0 0 0 0 0 0\n", i);
			continue;
		}
		double num, den;
		surface_colour_terms(e, p.colourBy, light, num, den);
		std::printf("e %x 1 %llx %llx %llx %llx %llx %llx %x %x %x %llx %llx %x\n", i, (unsigned long long)surface_bits(e.v[0]),
		            (unsigned long long)surface_bits(e.v[1]), (unsigned long long)surface_bits(e.v[2]), (unsigned long long)surface_bits(e.lambdaNum),
		            (unsigned long long)surface_bits(e.lambdaDen), (unsigned long long)surface_bits(e.vv), bits32((float)e.v[0]), bits32((float)e.v[1]),
		            bits32((float)e.v[2]), (unsigned long long)surface_bits(num), (unsigned long long)surface_bits(den), surface_index(p.thresholds, num, den));
	}
	return 0;
}
