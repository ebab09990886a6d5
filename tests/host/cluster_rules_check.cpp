// cluster_rules_check.cpp — simlod_amd/csrc/cluster_rules.hpp on the host, driven by tests/test_cluster_rules.py: the refusals, the core test,
// the size bin and the colour index printed line by line for the values in the input file, and cluster_find / cluster_link / cluster_root
// with a std::atomic memory policy on the link lists of the file: serially in several orders and from eight threads, the final root array
// against the per-component minimum the file carries.  A program of its own (plain g++, any sanitizer), nothing of HIP.
//   input: u32 numRecords, numCore, numSizes, numClusters, numLists, 0; the SimlodClusterParams records; (within, minNeighbours) pairs; sizes;
//          cluster numbers; per list u32 n, numLinks, then n expected roots, then numLinks (i, j) pairs.
//   argv[2]: "serial" (default), "threads", or "both".
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "cluster_rules.hpp"

using namespace simlod;

struct AtomicParent {                  // cluster_rules.hpp's memory policy on the host
	std::atomic<uint32_t>* p;
	uint32_t load(uint32_t i) { return p[i].load(std::memory_order_relaxed); }
	uint32_t cas(uint32_t i, uint32_t expected, uint32_t desired) {
		p[i].compare_exchange_strong(expected, desired, std::memory_order_relaxed);
		return expected;                                                       // (the value found: compare_exchange stores it there on failure)
	}
};

static bool read_all(FILE* f, void* to, size_t bytes) { return bytes == 0 || fread(to, 1, bytes, f) == bytes; }

// every link of `links` taken in the order `order` by `threads` threads (thread t takes the entries t, t + threads, ...) -> the number of
// links that gave up, then whether the roots equal `want`
static void run(const std::vector<uint32_t>& links, const std::vector<uint32_t>& order, uint32_t n, const std::vector<uint32_t>& want, unsigned threads,
                const char* what, unsigned list) {
	std::vector<std::atomic<uint32_t>> parent(n);
	for (uint32_t i = 0; i < n; i++) parent[i].store(i, std::memory_order_relaxed);
	std::atomic<uint32_t> failed{0};
	auto work = [&](unsigned t) {
		AtomicParent m{parent.data()};
		for (size_t k = t; k < order.size(); k += threads) {
			const uint32_t e = order[k];
			if (cluster_link(m, links[2u * e], links[2u * e + 1u], cluster_link_budget(n)) == CLUSTER_MISS) failed.fetch_add(1u);
		}
	};
	if (threads == 1u) {
		work(0u);
	} else {
		std::vector<std::thread> pool;
		for (unsigned t = 0; t < threads; t++) pool.emplace_back(work, t);
		for (auto& th : pool) th.join();
	}
	AtomicParent m{parent.data()};
	bool same = true, descending = true;
	for (uint32_t i = 0; i < n; i++) {
		uint64_t budget = n;
		if (cluster_root(m, i, budget) != want[i]) same = false;
		if (m.load(i) > i) descending = false;
	}
	printf("u %x %s %x %x %x\n", list, what, failed.load(), (unsigned)same, (unsigned)descending);
}

int main(int argc, char** argv) {
	if (argc < 2) return 2;
	const std::string mode = argc > 2 ? argv[2] : "serial";
	FILE* f = fopen(argv[1], "rb");
	if (f == nullptr) return 2;
	uint32_t head[6];
	if (!read_all(f, head, sizeof head)) return 3;
	std::vector<SimlodClusterParams> records(head[0]);
	std::vector<uint32_t> core(2u * head[1]), sizes(head[2]), clusters(head[3]);
	if (!read_all(f, records.data(), records.size() * sizeof(SimlodClusterParams)) || !read_all(f, core.data(), core.size() * 4u) ||
	    !read_all(f, sizes.data(), sizes.size() * 4u) || !read_all(f, clusters.data(), clusters.size() * 4u))
		return 3;
	if (mode != "threads") {
		for (size_t i = 0; i < records.size(); i++) printf("p %zx %x\n", i, (unsigned)cluster_acceptable(records[i]));
		for (size_t i = 0; i < head[1]; i++) printf("c %x %x %x\n", core[2u * i], core[2u * i + 1u], (unsigned)cluster_is_core(core[2u * i], core[2u * i + 1u]));
		for (uint32_t s : sizes) printf("b %x %x %x\n", s, cluster_size_bin(s), (unsigned)cluster_is_kept(s, 5u));
		for (uint32_t c : clusters) printf("i %x %x\n", c, cluster_colour_index(c));
		printf("k %llx %llx\n", (unsigned long long)cluster_largest_key(7u, 0u), (unsigned long long)cluster_largest_key(7u, 3u));
	}
	for (unsigned list = 0; list < head[4]; list++) {
		uint32_t nl[2];
		if (!read_all(f, nl, sizeof nl)) return 3;
		std::vector<uint32_t> want(nl[0]), links(2u * (size_t)nl[1]);
		if (!read_all(f, want.data(), want.size() * 4u) || !read_all(f, links.data(), links.size() * 4u)) return 3;
		std::vector<uint32_t> order(nl[1]);
		for (uint32_t e = 0; e < nl[1]; e++) order[e] = e;
		if (mode != "threads") {
			run(links, order, nl[0], want, 1u, "forward", list);
			std::vector<uint32_t> back(order.rbegin(), order.rend());
			run(links, back, nl[0], want, 1u, "reverse", list);
			uint64_t state = 0x9e3779b97f4a7c15ull;                            // three shuffles by a fixed generator
			for (int round = 0; round < 3; round++) {
				std::vector<uint32_t> mixed(order);
				for (size_t k = mixed.size(); k > 1u; k--) {
					state = state * 6364136223846793005ull + 1442695040888963407ull;
					std::swap(mixed[k - 1u], mixed[(size_t)((state >> 33) % k)]);
				}
				run(links, mixed, nl[0], want, 1u, "shuffled", list);
			}
		}
		if (mode != "serial") {
			for (int round = 0; round < 3; round++) run(links, order, nl[0], want, 8u, "threads", list);
		}
	}
	fclose(f);
	return 0;
}
