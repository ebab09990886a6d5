// render_layout_check.cpp — simlod_amd/csrc/render_layout.hpp on the host, alone: the regions of kernel_render's buffer in order and without overlap at nine
// frame sizes, the offsets as literal numbers at six of them, the pool's capacity rule, the index enums.
// A program of its own (tests/test_render_layout.py builds it with the address and undefined-behaviour sanitizers and runs it); exit status 0 = every check held.
#include "render_layout.hpp"

#include <cstdio>
#include <vector>

using namespace simlod;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                  \
	do {                                                                                  \
		if (!(cond)) { g_failed++; std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
	} while (0)
#define ULL(v) ((unsigned long long)(v))

struct Size { uint32_t w, h; };
static const Size SIZES[] = {{1, 1}, {3, 3}, {128, 96}, {129, 97}, {1920, 1080}, {1921, 1081}, {2560, 1440}, {3840, 2160}, {4096, 2160}};

// ---- the regions: in the stated order, none overlapping, aligned, `bytes` = the end of the last one + the tail -----------------------------------
static void check_regions(uint32_t w, uint32_t h) {
	const FrameLayout l(w, h);
	const uint64_t px = (uint64_t)w * h, tiles = l.binTiles;
	struct Region { const char* name; uint64_t start, size; };
	const Region R[] = {
		{"visible", l.visible, (uint64_t)VISIBLE_NODES * NODE_BYTES}, {"counters", l.counters, (uint64_t)C_COUNT * COUNTER_STRIDE}, {"lines", l.lines, 32},
		{"vertices", l.vertices, 16ull * LINE_VERTEX_CAP}, {"framebuffer", l.framebuffer, px * 8}, {"work", l.work, WORK_BYTES},
		{"items", l.items, (uint64_t)MAX_DRAW_ITEMS * ITEM_CLASSES * DRAW_ITEM_BYTES}, {"depth", l.depth, px * 4}, {"colour", l.colour, px * 8}, {"sums", l.sums, px * 16},
		{"dir", l.dir, (uint64_t)MAX_DIR_CHUNKS * 8}, {"binSegs", l.binSegs, tiles * BIN_SEG_CAP * BIN_SEG_BYTES}, {"binSegCount", l.binSegCount, tiles * 4},
		{"binStats", l.binStats, tiles * BIN_SEG_BYTES}, {"binPool", l.binPool, tiles != 0 ? (uint64_t)BIN_POOL_ENTRIES * 16 : 0},
	};
	const int n = (int)(sizeof(R) / sizeof(R[0]));
	for (int i = 0; i < n; i++) {
		if (i + 1 < n) CHECK(R[i].start + R[i].size <= R[i + 1].start, "%ux%u: %s [%llu, +%llu) runs into %s at %llu", w, h, R[i].name, ULL(R[i].start), ULL(R[i].size), R[i + 1].name, ULL(R[i + 1].start));
		// (no region leaves more than one rounding step unused in front of the next: nothing else hides in between)
		if (i + 1 < n) CHECK(R[i + 1].start - (R[i].start + R[i].size) < 16, "%ux%u: a gap behind %s", w, h, R[i].name);
		// The pool alone starts on a multiple of 8, not of 16, when the frame has an odd number of bins: binStats in front of it holds 8 bytes per bin, and
		// the sum the layout had before this header rounded nothing there (1 x 1 and 3 x 3 have one bin; 1 x 1: 66 402 536).  Positions are as they were.
		const bool pool = i == n - 1;
		CHECK(R[i].start % (pool ? 8 : 16) == 0, "%ux%u: %s starts at %llu", w, h, R[i].name, ULL(R[i].start));
		if (pool) CHECK(R[i].start % 16 == (tiles % 2 == 0 ? 0u : 8u), "%ux%u: binPool at %llu with %llu bins", w, h, ULL(R[i].start), ULL(tiles));
	}
	CHECK(l.bytes == R[n - 1].start + R[n - 1].size + TAIL_BYTES, "%ux%u: bytes %llu", w, h, ULL(l.bytes));
	CHECK(l.probe >= l.vertices && l.probe + 12ull * 8192 * 8 <= l.framebuffer, "the probe words lie inside the vertex array");
	CHECK(l.binTilesX == (w >> BIN_SHIFT) + 1u, "%ux%u: binTilesX %u", w, h, l.binTilesX);
	const uint64_t all = (uint64_t)l.binTilesX * ((h >> BIN_SHIFT) + 1u);
	CHECK(l.binTiles == (all <= BIN_MAX_TILES ? all : 0), "%ux%u: binTiles %u of %llu", w, h, l.binTiles, ULL(all));
	// a buffer of exactly `bytes` holds the whole pool wherever there are bins
	if (l.binTiles != 0) CHECK(l.pool_entries(l.bytes, (int)BIN_POOL_ENTRIES) == BIN_POOL_ENTRIES, "%ux%u: %u entries in a buffer of `bytes`", w, h, l.pool_entries(l.bytes, (int)BIN_POOL_ENTRIES));
}

// ---- the offsets as numbers: what the three pieces of arithmetic this header replaced gave (render_buffer_bytes, render_plane_offsets, launch_render) ----
struct Row { uint32_t w, h; uint64_t work, depth, colour, sums, dir; uint32_t binTiles; uint64_t binPool, bytes; };
static const Row TABLE[] = {
	{1, 1, 31200160ull, 50400416ull, 50400432ull, 50400448ull, 50400464ull, 1, 66402536ull, 114402792ull},
	{129, 97, 31300256ull, 50500512ull, 50550576ull, 50650688ull, 50850896ull, 20, 66892096ull, 114892352ull},
	{1920, 1080, 47788944ull, 66989200ull, 75283600ull, 91872400ull, 125050000ull, 2074, 145322448ull, 193322704ull},
	{1921, 1081, 47812960ull, 67013216ull, 75319632ull, 91932448ull, 125158064ull, 2074, 145430512ull, 193430768ull},
	{2560, 1440, 60691344ull, 79891600ull, 94637200ull, 124128400ull, 183110800ull, 3726, 206786368ull, 254786624ull},
	{3840, 2160, 97555344ull, 116755600ull, 149933200ull, 216288400ull, 348998800ull, 8228, 381948480ull, 429948736ull},
	{4096, 2160, 101979024ull, 121179280ull, 156568720ull, 227347600ull, 368905360ull, 0 /* 8772 > 8704 */, 384905360ull /* = binSegs */, 384905616ull},
};
static void check_table() {
	for (const Row& r : TABLE) {
		const FrameLayout l(r.w, r.h);
		CHECK(l.work == r.work && l.items == r.work + 256, "%ux%u: work %llu items %llu", r.w, r.h, ULL(l.work), ULL(l.items));
		CHECK(l.depth == r.depth && l.colour == r.colour && l.sums == r.sums && l.dir == r.dir, "%ux%u: depth %llu colour %llu sums %llu dir %llu", r.w, r.h, ULL(l.depth), ULL(l.colour), ULL(l.sums), ULL(l.dir));
		CHECK(l.binTiles == r.binTiles && l.binPool == r.binPool && l.bytes == r.bytes, "%ux%u: binTiles %u binPool %llu bytes %llu", r.w, r.h, l.binTiles, ULL(l.binPool), ULL(l.bytes));
		if (r.binTiles == 0) CHECK(l.binPool == l.binSegs && l.binSegCount == l.binSegs && l.binStats == l.binSegs, "%ux%u: no bins, no tables", r.w, r.h);
	}
	CHECK(FrameLayout::visible == 0 && FrameLayout::counters == 100000ull * 152, "counters at %llu", ULL(FrameLayout::counters));
	CHECK(FrameLayout::lines == FrameLayout::counters + (uint64_t)C_COUNT * 16, "lines at %llu", ULL(FrameLayout::lines));
	CHECK(FrameLayout::vertices == FrameLayout::lines + 32, "vertices at %llu", ULL(FrameLayout::vertices));
	CHECK(FrameLayout::framebuffer == FrameLayout::vertices + 16ull * LINE_VERTEX_CAP && FrameLayout::framebuffer == 31200144ull, "framebuffer at %llu", ULL(FrameLayout::framebuffer));
	CHECK(FrameLayout::probe == FrameLayout::vertices + 8000000ull, "probe at %llu", ULL(FrameLayout::probe));
}

// ---- the pool: min(knob clamped to [0, BIN_POOL_ENTRIES], what the buffer has between binPool and its tail) ----------------------------------------
static void check_pool() {
	const uint64_t host = 200000000ull;                  // what the reference host allocates whatever its window's size
	const FrameLayout hd(1920, 1080), qhd(2560, 1440), uhd(3840, 2160);
	CHECK((host - hd.binPool - 256) / 16 == 3417331ull, "room at 1920x1080: %llu", ULL((host - hd.binPool - 256) / 16));
	CHECK(hd.pool_entries(host, (int)BIN_POOL_ENTRIES) == BIN_POOL_ENTRIES && BIN_POOL_ENTRIES == 3000000u, "1920x1080 in the host's buffer: %u", hd.pool_entries(host, (int)BIN_POOL_ENTRIES));
	CHECK(hd.pool_entries(host, 2000000000) == BIN_POOL_ENTRIES, "the knob is clamped: %u", hd.pool_entries(host, 2000000000));
	CHECK(qhd.pool_entries(host, (int)BIN_POOL_ENTRIES) == 0 && uhd.pool_entries(host, (int)BIN_POOL_ENTRIES) == 0, "2560x1440: %u, 3840x2160: %u", qhd.pool_entries(host, (int)BIN_POOL_ENTRIES), uhd.pool_entries(host, (int)BIN_POOL_ENTRIES));
	CHECK(hd.pool_entries(host, 20000) == 20000 && hd.pool_entries(hd.bytes, 20000) == 20000, "the tests' knob: %u", hd.pool_entries(host, 20000));
	CHECK(hd.pool_entries(host, -1) == 0 && hd.pool_entries(host, -2147483647 - 1) == 0 && hd.pool_entries(host, 0) == 0, "a negative knob: %u", hd.pool_entries(host, -1));
	for (const Size& s : SIZES) {
		const FrameLayout l(s.w, s.h);
		CHECK(l.pool_entries(l.binPool + 255, (int)BIN_POOL_ENTRIES) == 0 && l.pool_entries(l.binPool + 256, (int)BIN_POOL_ENTRIES) == 0 && l.pool_entries(0, (int)BIN_POOL_ENTRIES) == 0, "%ux%u: a buffer that ends before the pool", s.w, s.h);
		CHECK(l.pool_entries(l.binPool + 256 + 16 * 7 + 15, (int)BIN_POOL_ENTRIES) == 7, "%ux%u: whole entries only", s.w, s.h);
	}
}

// ---- the index enums: the numbers tools/raster_items.py and the runtime document ------------------------------------------------------------------
static void check_indices() {
	CHECK(W_CURSOR0 == 0 && W_DIR_ENTRIES == 4 && W_ITEMS0 == 8 && W_ITEMS0 + ITEM_CLASSES - 1 == 11 && W_POOL_TAKEN == 12 && W_BINNED == 13 && W_SORTING_NODES == 14 && W_READY == 15, "work words");
	CHECK(W_COUNT > W_SORTING_NODES && W_READY >= W_COUNT && W_READY < 64, "W_COUNT %d W_READY %d", (int)W_COUNT, (int)W_READY);
	CHECK(C_VISIBLE == 0 && C_POINTS == 1 && C_VOXELS == 2 && C_INNER == 3 && C_LEAVES == 4 && C_TABLE_LISTS == 5 && C_OUTSIDE_TILES == 6 && C_COUNT == 7, "counters");
	// the accessors, on a buffer that reaches as far as the work area
	const FrameLayout l(129, 97);
	std::vector<uint8_t> buffer(l.items);
	uint8_t* const mom = buffer.data();
	CHECK(reinterpret_cast<uint8_t*>(counter_at(mom, C_OUTSIDE_TILES)) == mom + FrameLayout::counters + 6 * 16, "counter_at");
	CHECK(reinterpret_cast<uint8_t*>(work_words(mom, l)) == mom + l.work && frame_ready_word(mom, l) == work_words(mom, l) + W_READY, "work_words, frame_ready_word");
	*frame_ready_word(mom, l) = 7u;
	for (int k = 0; k < W_COUNT; k++) work_words(mom, l)[k] = 0u;
	CHECK(*frame_ready_word(mom, l) == 7u, "zeroing the work words leaves the frame-ready word alone");
}

int main() {
	for (const Size& s : SIZES) check_regions(s.w, s.h);
	check_table();
	check_pool();
	check_indices();
	if (g_failed != 0) { std::printf("%d checks failed\n", g_failed); return 1; }
	std::printf("render_layout.hpp: all checks held\n");
	return 0;
}
