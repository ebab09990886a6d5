// pack_rules_check.cpp — simlod_amd/csrc/pack_rules.hpp on the host, alone: the box a call accepts, the ranges of rule K5, the records of rules
// K0-K4 and what they decode to (rule K8), with the counts of rule K6.  A program of its own (tests/test_pack_rules.py builds it with the address
// and undefined-behaviour sanitizers and runs it on a hand-made table; the test compares what it writes with octree_io.pack_samples /
// unpack_samples byte for byte).  It walks the table the way export_pack.inc's kernels do: entry by entry, pack_entry_range, pack_frame, then
// pack_sample / unpack_sample per sample.
//   input:  u32 numNodes, u32 hasEntries, u64 numSamples, f32 boxMin[3], f32 boxMax[3], numNodes x SimlodExportNode,
//           hasEntries ? numNodes x SimlodDeltaEntry, numSamples x SimlodPoint
//   output: u8 accepted (the box; numNodes != 0), then — zeros when refused — numSamples x u64 packed (zero where no range covers), SimlodPackCounts of
//           the pack, numSamples x SimlodPoint unpacked from those records (zero where no range covers), SimlodPackCounts of the unpack
#include "pack_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

int main(int argc, char** argv) {
	if (argc != 3) { std::printf("usage: pack_rules_check <cases> <out>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t head[2];
	uint64_t numSamples;
	float box[6];
	if (std::fread(head, 4, 2, in) != 2 || std::fread(&numSamples, 8, 1, in) != 1 || std::fread(box, 4, 6, in) != 6) { std::printf("short header\n"); return 2; }
	const uint32_t n = head[0];
	std::vector<SimlodExportNode> table(n);
	std::vector<SimlodDeltaEntry> entries(head[1] != 0u ? n : 0u);
	std::vector<SimlodPoint> samples(numSamples);
	auto read = [&](void* to, size_t bytes, size_t count) { return count == 0 || std::fread(to, bytes, count, in) == count; };   // (an empty vector has no data())
	if (!read(table.data(), sizeof(SimlodExportNode), n) || !read(entries.data(), sizeof(SimlodDeltaEntry), entries.size()) ||
	    !read(samples.data(), sizeof(SimlodPoint), samples.size())) {
		std::printf("short body\n");
		return 2;
	}
	std::fclose(in);
	std::vector<uint64_t> packed(numSamples, 0ull);
	std::vector<SimlodPoint> back(numSamples);
	if (!back.empty()) std::memset(back.data(), 0, back.size() * sizeof(SimlodPoint));
	SimlodPackCounts pc, uc;
	std::memset(&pc, 0, sizeof pc);
	std::memset(&uc, 0, sizeof uc);
	PackBox b;
	const float mn[3] = {box[0], box[1], box[2]}, mx[3] = {box[3], box[4], box[5]};
	const bool ok = n != 0u && pack_box(mn, mx, b);
	if (ok) {
		for (uint32_t t = 0; t < n; t++) {
			const SimlodExportNode& e = table[t];
			uint64_t first;
			uint32_t cnt, err;
			const bool on = pack_entry_range(e, entries.empty() ? nullptr : &entries[t], numSamples, first, cnt, err);
			pc.error |= err; uc.error |= err;
			if (!on) continue;
			const bool leaf = (e.flags & SIMLOD_EXPORT_FLAG_LEAF) != 0u;
			const PackFrame f = pack_frame(b, e.level, e.X, e.Y, e.Z, leaf);
			const double ns = pack_node_size(b.size, e.level);
			const float fns = b.sizef / pack_exp2(e.level);
			for (uint64_t i = first; i < first + cnt; i++) {
				uint32_t what;
				const SimlodPoint& p = samples[i];
				packed[i] = pack_sample(f, fns, leaf, p.x, p.y, p.z, p.color, what);
				pc.numClamped += what & PACK_CLAMPED ? 1u : 0u; pc.numInexact += what & PACK_INEXACT ? 1u : 0u; pc.numAlpha += what & PACK_ALPHA ? 1u : 0u;
				back[i] = unpack_sample(f, ns, fns, leaf, packed[i] | 1ull << 63);      // (bit 63 is ignored)
			}
			pc.numSamples += cnt; uc.numSamples += cnt;
		}
	}
	FILE* o = std::fopen(argv[2], "wb");
	const uint8_t accepted = ok ? 1 : 0;
	auto write = [&](const void* from, size_t bytes, size_t count) { return count == 0 || std::fwrite(from, bytes, count, o) == count; };
	if (o == nullptr || !write(&accepted, 1, 1) || !write(packed.data(), 8, packed.size()) || !write(&pc, sizeof pc, 1) ||
	    !write(back.data(), sizeof(SimlodPoint), back.size()) || !write(&uc, sizeof uc, 1)) {
		std::printf("cannot write %s\n", argv[2]);
		return 2;
	}
	std::fclose(o);
	return 0;
}
