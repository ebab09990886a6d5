// profile_rules_check.cpp — simlod_amd/csrc/profile_rules.hpp on the host, alone: what the profile query accepts, the segment block of rule P0 and a
// node's class by the corridor (rule P3).  A program of its own (tests/test_profile_rules.py builds it with the address and undefined-behaviour
// sanitizers and runs it on a file of cases; the test compares what it writes with octree_io.Profile.segments and octree_io.classify_profile).
//   input:  u32 numProfiles, u32 numNodes, f32 boxMin[3], f32 boxMax[3], numProfiles x SimlodProfile, numNodes x u32 {level, X, Y, Z}
//   output: per profile: u8 accepted, 63 x 64 bytes of segments (zeros behind the last one), then per node u8 class (PROFILE_NODE_*) — zeros for a
//           profile that is refused
#include "profile_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

int main(int argc, char** argv) {
	if (argc != 3) { std::printf("usage: profile_rules_check <cases> <out>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t counts[2];
	float box[6];
	if (std::fread(counts, 4, 2, in) != 2 || std::fread(box, 4, 6, in) != 6) { std::printf("short header\n"); return 2; }
	std::vector<SimlodProfile> profiles(counts[0]);
	std::vector<uint32_t> nodes(4 * (size_t)counts[1]);
	if (std::fread(profiles.data(), sizeof(SimlodProfile), profiles.size(), in) != profiles.size() || std::fread(nodes.data(), 16, counts[1], in) != counts[1]) {
		std::printf("short body\n");
		return 2;
	}
	std::fclose(in);
	// the box as every launcher derives it (simlod_internal.hpp octree_box): the largest fp32 extent, from the minimum corner
	const float size = fmaxf(fmaxf(box[3] - box[0], box[4] - box[1]), box[5] - box[2]);
	const double mn[3] = {(double)box[0], (double)box[1], (double)box[2]};
	std::vector<uint8_t> out;
	for (const SimlodProfile& p : profiles) {
		ProfileSegment seg[PROFILE_MAX_SEGMENTS];
		std::memset(seg, 0, sizeof seg);
		bool ok = profile_acceptable(p);
		if (ok && !profile_segments(p, seg)) { ok = false; std::memset(seg, 0, sizeof seg); }
		out.push_back(ok ? 1 : 0);
		const uint8_t* bytes = reinterpret_cast<const uint8_t*>(seg);
		out.insert(out.end(), bytes, bytes + sizeof seg);
		double axU[4], axV[4];
		for (int k = 0; k < 4; k++) { axU[k] = (double)p.axisU[k]; axV[k] = (double)p.axisV[k]; }
		for (uint32_t i = 0; i < counts[1]; i++)
			out.push_back((uint8_t)(ok ? classify_profile(mn, (double)size, axU, axV, seg, p.numVertices - 1u, nodes[4 * i], nodes[4 * i + 1], nodes[4 * i + 2], nodes[4 * i + 3]) : 0u));
	}
	FILE* o = std::fopen(argv[2], "wb");
	if (o == nullptr || std::fwrite(out.data(), 1, out.size(), o) != out.size()) { std::printf("cannot write %s\n", argv[2]); return 2; }
	std::fclose(o);
	return 0;
}
