// align_rules_check.cpp — simlod_amd/csrc/align_rules.hpp on the host, alone: which SimlodAlignParams records a call accepts, rule A1's
// posed centre and its validity, rule A2's cell of a double, rule A4's invQ, inside test and Q, rule A5's lo/hi split and squared residual,
// and rule A7's stamp and its comparison.  A program of its own (tests/test_align_rules.py builds it with the address and
// undefined-behaviour sanitizers, runs it and compares every line it prints with tests/align_ref.py).
//   input:  u32 numParams, u32 numPoints, u32 numCoords, u32 numProducts, u32 numPairs, u32 numStamps, f32 gridRadius, f32 size, f64 min[3],
//           f64 pose[12], u64 b, u64 numB, numParams x SimlodAlignParams, numPoints x 3 f32, numCoords x f64, numProducts x u64,
//           numPairs x 6 u32 (Q of c' x3, Q of s x3), numStamps x 2 AlignStamp (have, want)
//   output: per record "p <index> <accepted>"; one line "g <bits of inv> <bits of invQ>"; per point "c <index> <valid> <bits of c' x3>
//           <cell x3>" (cells 0 when invalid); per coordinate, on axis 0, "q <bits> <cell> <inside> <Q>"; per product "l <lo> <hi>"; per
//           pair "e <E>"; one line "t <magic> <filled> <b> <numB> <inv> <min x3>" for the stamp of the header's values, filled; per stamp
//           pair "s <index> <serves>"; integers in hexadecimal
#include "align_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

typedef unsigned long long ull;

int main(int argc, char** argv) {
	if (argc != 2) { std::printf("usage: align_rules_check <cases>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t head[6];
	float box[2];
	double mn[3], pose[12];
	uint64_t grid[2];
	if (std::fread(head, 4, 6, in) != 6 || std::fread(box, 4, 2, in) != 2 || std::fread(mn, 8, 3, in) != 3 || std::fread(pose, 8, 12, in) != 12 ||
	    std::fread(grid, 8, 2, in) != 2) { std::printf("short header\n"); return 2; }
	const uint32_t np = head[0], nc = head[1], nq = head[2], nl = head[3], ne = head[4], ns = head[5];
	std::vector<SimlodAlignParams> params(np);
	std::vector<float> points((size_t)nc * 3u);
	std::vector<double> coords(nq);
	std::vector<uint64_t> products(nl);
	std::vector<uint32_t> pairs((size_t)ne * 6u);
	std::vector<AlignStamp> stamps((size_t)ns * 2u);
	auto read = [&](void* to, size_t bytes, size_t count) { return count == 0 || std::fread(to, bytes, count, in) == count; };   // (an empty vector has no data())
	if (!read(params.data(), sizeof(SimlodAlignParams), np) || !read(points.data(), 12, nc) || !read(coords.data(), 8, nq) || !read(products.data(), 8, nl) ||
	    !read(pairs.data(), 24, ne) || !read(stamps.data(), 2 * sizeof(AlignStamp), ns)) { std::printf("short body\n"); return 2; }
	std::fclose(in);
	for (uint32_t i = 0; i < np; i++) std::printf("p %x %x\n", i, align_acceptable(params[i]) ? 1u : 0u);
	const double inv = compare_inv(box[0], box[1]), invq = align_invq(box[1]);
	std::printf("g %llx %llx\n", (ull)align_bits(inv), (ull)align_bits(invq));
	for (uint32_t i = 0; i < nc; i++) {
		uint32_t bits[3];
		std::memcpy(bits, &points[(size_t)i * 3u], 12);
		double cp[3] = {0.0, 0.0, 0.0};
		const bool valid = compare_valid(bits[0], bits[1], bits[2]) &&
		                   align_pose(pose, (double)points[(size_t)i * 3u], (double)points[(size_t)i * 3u + 1u], (double)points[(size_t)i * 3u + 2u], cp);
		if (!valid) { std::printf("c %x 0 0 0 0 0 0 0\n", i); continue; }
		std::printf("c %x 1 %llx %llx %llx %x %x %x\n", i, (ull)align_bits(cp[0]), (ull)align_bits(cp[1]), (ull)align_bits(cp[2]), align_cell20(cp[0], mn[0], inv),
		            align_cell20(cp[1], mn[1], inv), align_cell20(cp[2], mn[2], inv));
	}
	for (uint32_t i = 0; i < nq; i++) {
		uint32_t q;
		const bool inside = align_q(coords[i], mn[0], invq, q);
		std::printf("q %llx %x %x %x\n", (ull)align_bits(coords[i]), align_cell20(coords[i], mn[0], inv), inside ? 1u : 0u, q);
	}
	for (uint32_t i = 0; i < nl; i++) std::printf("l %llx %llx\n", (ull)align_lo(products[i]), (ull)align_hi(products[i]));
	for (uint32_t i = 0; i < ne; i++) {
		const uint32_t qa[3] = {pairs[(size_t)i * 6u], pairs[(size_t)i * 6u + 1u], pairs[(size_t)i * 6u + 2u]};
		const uint32_t qb[3] = {pairs[(size_t)i * 6u + 3u], pairs[(size_t)i * 6u + 4u], pairs[(size_t)i * 6u + 5u]};
		std::printf("e %llx\n", (ull)align_sq(qa, qb));
	}
	const AlignStamp t = align_stamp(reinterpret_cast<const void*>((uintptr_t)grid[0]), grid[1], inv, mn, true);
	std::printf("t %x %x %llx %llx %llx %llx %llx %llx\n", t.magic, t.filled, (ull)t.b, (ull)t.numB, (ull)t.inv, (ull)t.min[0], (ull)t.min[1], (ull)t.min[2]);
	for (uint32_t i = 0; i < ns; i++) std::printf("s %x %x\n", i, align_stamp_serves(stamps[(size_t)i * 2u], stamps[(size_t)i * 2u + 1u]) ? 1u : 0u);
	return 0;
}
