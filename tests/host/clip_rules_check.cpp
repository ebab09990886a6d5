// clip_rules_check.cpp — simlod_amd/csrc/clip_rules.hpp on the host, alone: what the clip setter accepts, and the class and the action of a node under a clip.
// A program of its own (tests/test_clip_rules.py builds it with the address and undefined-behaviour sanitizers and runs it on a file of cases; the test
// compares what it writes with octree_io.classify_nodes).
//   input:  u32 numClips, u32 numNodes, f32 boxMin[3], f32 boxMax[3], numClips x SimlodClip, numNodes x u32 {level, X, Y, Z}
//   output: per clip: u8 accepted, then per node u8 class (CLIP_NODE_*) and u8 action (CLIP_ACT_*) — zeros for a clip that is refused
#include "clip_rules.hpp"

#include <cstdio>
#include <vector>

using namespace simlod;

int main(int argc, char** argv) {
	if (argc != 3) { std::printf("usage: clip_rules_check <cases> <out>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t counts[2];
	float box[6];
	if (std::fread(counts, 4, 2, in) != 2 || std::fread(box, 4, 6, in) != 6) { std::printf("short header\n"); return 2; }
	std::vector<SimlodClip> clips(counts[0]);
	std::vector<uint32_t> nodes(4 * (size_t)counts[1]);
	if (std::fread(clips.data(), sizeof(SimlodClip), clips.size(), in) != clips.size() || std::fread(nodes.data(), 16, counts[1], in) != counts[1]) {
		std::printf("short body\n");
		return 2;
	}
	std::fclose(in);
	// the box as every launcher derives it (simlod_internal.hpp octree_box): the largest fp32 extent, from the minimum corner
	const float size = fmaxf(fmaxf(box[3] - box[0], box[4] - box[1]), box[5] - box[2]);
	std::vector<uint8_t> out;
	for (const SimlodClip& c : clips) {
		const bool ok = clip_acceptable(c);
		out.push_back(ok ? 1 : 0);
		const ClipArgs k = ok ? clip_args(c, size, box[0], box[1], box[2]) : ClipArgs{};
		for (uint32_t i = 0; i < counts[1]; i++) {
			const uint32_t cls = ok ? classify_node(k.min, k.size, k.numPlanes, k.pl, nodes[4 * i], nodes[4 * i + 1], nodes[4 * i + 2], nodes[4 * i + 3]) : 0u;
			out.push_back((uint8_t)cls);
			out.push_back((uint8_t)(ok ? clip_action(k.mode, cls) : 0u));
		}
	}
	FILE* o = std::fopen(argv[2], "wb");
	if (o == nullptr || std::fwrite(out.data(), 1, out.size(), o) != out.size()) { std::printf("cannot write %s\n", argv[2]); return 2; }
	std::fclose(o);
	return 0;
}
