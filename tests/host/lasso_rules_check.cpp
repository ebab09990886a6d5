// lasso_rules_check.cpp — simlod_amd/csrc/lasso_rules.hpp on the host, alone: what the lasso query accepts (rule L7), the rows and the edge block
// widened to fp64, and a node's class by the lasso (rules L2-L4).  A program of its own (tests/test_lasso_rules.py builds it with the address and
// undefined-behaviour sanitizers and runs it on a file of cases; the test compares what it writes with octree_io.Lasso.edges and
// octree_io.classify_lasso).
//   input:  u32 numLassos, u32 numNodes, f32 boxMin[3], f32 boxMax[3], numLassos x SimlodLasso, numNodes x u32 {level, X, Y, Z}
//   output: per lasso: u8 accepted, 12 x f64 rows (U, V, W), 256 x 32 bytes of edges (zeros behind the last one), then per node u8 class
//           (LASSO_NODE_*) — zeros for a lasso that is refused
#include "lasso_rules.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace simlod;

int main(int argc, char** argv) {
	if (argc != 3) { std::printf("usage: lasso_rules_check <cases> <out>\n"); return 2; }
	FILE* in = std::fopen(argv[1], "rb");
	if (in == nullptr) { std::printf("cannot read %s\n", argv[1]); return 2; }
	uint32_t counts[2];
	float box[6];
	if (std::fread(counts, 4, 2, in) != 2 || std::fread(box, 4, 6, in) != 6) { std::printf("short header\n"); return 2; }
	std::vector<SimlodLasso> lassos(counts[0]);
	std::vector<uint32_t> nodes(4 * (size_t)counts[1]);
	if (std::fread(lassos.data(), sizeof(SimlodLasso), lassos.size(), in) != lassos.size() || std::fread(nodes.data(), 16, counts[1], in) != counts[1]) {
		std::printf("short body\n");
		return 2;
	}
	std::fclose(in);
	// the box as every launcher derives it (simlod_internal.hpp octree_box): the largest fp32 extent, from the minimum corner
	const float size = fmaxf(fmaxf(box[3] - box[0], box[4] - box[1]), box[5] - box[2]);
	const double mn[3] = {(double)box[0], (double)box[1], (double)box[2]};
	std::vector<uint8_t> out;
	std::vector<LassoEdge> edges(SIMLOD_LASSO_MAX_VERTICES);
	for (const SimlodLasso& l : lassos) {
		double rows[3][4];
		std::memset(rows, 0, sizeof rows);
		std::memset(edges.data(), 0, edges.size() * sizeof(LassoEdge));
		const bool ok = lasso_acceptable(l);
		if (ok) lasso_widen(l, rows, edges.data());
		out.push_back(ok ? 1 : 0);
		const uint8_t* rb = reinterpret_cast<const uint8_t*>(rows);
		out.insert(out.end(), rb, rb + sizeof rows);
		const uint8_t* eb = reinterpret_cast<const uint8_t*>(edges.data());
		out.insert(out.end(), eb, eb + edges.size() * sizeof(LassoEdge));
		for (uint32_t i = 0; i < counts[1]; i++)
			out.push_back((uint8_t)(ok ? classify_lasso(mn, (double)size, rows, edges.data(), l.numVertices, nodes[4 * i], nodes[4 * i + 1], nodes[4 * i + 2], nodes[4 * i + 3]) : 0u));
	}
	FILE* o = std::fopen(argv[2], "wb");
	if (o == nullptr || std::fwrite(out.data(), 1, out.size(), o) != out.size()) { std::printf("cannot write %s\n", argv[2]); return 2; }
	std::fclose(o);
	return 0;
}
