// render_layout.hpp — the byte layout of kernel_render's momentary buffer, stated ONCE: the capacities that size its regions, the indices of its
// counters and work words, where every region starts for a width x height frame, the address helpers the kernels share.  No HIP in here: the kernels
// (render_*.inc), the launcher (render.hip), the C ABI (simlod_render_frame_layout) and tests/host/render_layout_check.cpp (plain g++) read it here.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define SIMLOD_HD __host__ __device__
#else
#define SIMLOD_HD
#endif

namespace simlod {
// ---- capacities -------------------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t VISIBLE_NODES = 100000, NODE_BYTES = 152;   // SIMLOD_MAX_VISIBLE_NODES records of sizeof(SimlodNode): the visible-node array (render.hip asserts both against simlod_abi.h)
static constexpr uint32_t MAX_DRAW_ITEMS = 150000;          // per size class: 100 000 visible nodes, one list each, + slices of long lists
static constexpr int      ITEM_CLASSES = 4;                 // draw items are queued by size, biggest first (render_common.inc)
static constexpr uint32_t DRAW_ITEM_BYTES = 32, BIN_SEG_BYTES = 8;   // sizeof(DrawItem), sizeof(BinSeg) (render.hip asserts both)
static constexpr uint32_t MAX_DIR_CHUNKS = 2000000;         // chunk directory of a frame: 2 G visible samples
static constexpr uint32_t BIN_SHIFT = 5, BIN = 1u << BIN_SHIFT;   // a bin = 32 x 32 pixels: 2074 of them at 1920 x 1080 — the terrain towards the horizon of a close-up is a strip of three hundred
static constexpr uint32_t BIN_POOL_MIN = 65536;             // a buffer that has room for fewer pool entries than this behind its planes draws without bins
static constexpr uint32_t BIN_POOL_ENTRIES = 3000000;       // 48 MB of entries per frame and pass: the buffer stays inside the host's 200 MB at 1920 x 1080 (main_progressive_octree.cpp:555) (what does not fit: device-scope atomics, as before)
static constexpr uint32_t BIN_SEG_CAP = 256;                // segments (item x bin) a bin can list
static constexpr uint32_t BIN_MAX_TILES = 8704;             // (3840 x 2160 pixels: 8228) the per-bin counters of a sorting workgroup live in its LDS; larger frames do not sort
static constexpr uint32_t LINE_VERTEX_CAP = 1000000u;       // render.cu:1119
static constexpr uint32_t COUNTER_STRIDE = 16, WORK_BYTES = 256, TAIL_BYTES = 256;   // Allocator::alloc rounds every block up to 16 bytes | the work area | what the buffer keeps free behind its last region
// ---- named indices ----------------------------------------------------------------------------------------------------------------------------
// the frame's counters, COUNTER_STRIDE bytes apart.  [5]: lists r_visible read through the builder's chunk table; [6]: samples the first draw pass sent
// down the global-atomic path (outside their item's LDS tile, or no tile)
enum { C_VISIBLE = 0, C_POINTS = 1, C_VOXELS = 2, C_INNER = 3, C_LEAVES = 4, C_TABLE_LISTS = 5, C_OUTSIDE_TILES = 6, C_COUNT = 7 };
// the work area's 32-bit words: the draw cursors of the three draw modes (W_CURSOR0 + MODE) | chunk directory entries in use | draw items per size
// class (W_ITEMS0 + class) | entries taken from the bin pool | samples that were binned (first draw pass) | nodes that sort or would.  W_COUNT covers
// every word a frame zeroes (clear_counters); W_READY lies OUTSIDE that range on purpose (frame_ready_word below).
enum { W_CURSOR0 = 0, W_DIR_ENTRIES = 4, W_ITEMS0 = 8, W_POOL_TAKEN = 12, W_BINNED = 13, W_SORTING_NODES = 14, W_COUNT = 15, W_READY = W_COUNT };
static_assert(W_ITEMS0 + ITEM_CLASSES <= W_POOL_TAKEN && W_READY >= W_COUNT && (W_READY + 1) * 4 <= (int)WORK_BYTES, "the work words fit the work area; W_READY is not zeroed");
SIMLOD_HD constexpr uint64_t align16(uint64_t v) { return (v + 15) / 16 * 16; }
// ---- where everything lies for a frame of width x height --------------------------------------------------------------------------------------
// In this order, none overlapping: visible | counters | lines | vertices | framebuffer | work | items | depth | colour | sums | dir | binSegs |
// binSegCount | binStats | binPool | the tail.  Up to the framebuffer it is the momentary layout of render.cu:1108-1123, and those offsets are
// compile-time constants (the kernels fold them into immediates); `probe` is no region of its own: a -DVAR_PROBE build keeps its clock words in the
// second half of the vertex array.  Every start is a multiple of 16 except binPool's, which is one of 8 (binStats holds 8 bytes per bin).
struct FrameLayout {
	static constexpr uint64_t visible = 0;                                                             // VISIBLE_NODES node records
	static constexpr uint64_t counters = (uint64_t)VISIBLE_NODES * NODE_BYTES;                        // C_COUNT x 16 B
	static constexpr uint64_t lines = counters + (uint64_t)C_COUNT * COUNTER_STRIDE;                  // 32 B header: word 0 = vertices in use
	static constexpr uint64_t vertices = lines + 32;                                                   // 1 M x 16 B
	static constexpr uint64_t probe = vertices + 8000000ull;
	static constexpr uint64_t framebuffer = vertices + 16ull * LINE_VERTEX_CAP;                       // uint64 per pixel: depth bits << 32 | colour
	uint64_t work = 0, items = 0;          // the work words | ITEM_CLASSES arrays of MAX_DRAW_ITEMS draw items
	uint64_t depth = 0, colour = 0, sums = 0;   // HQS: uint32 depth per pixel | packed colour sums, uint64 per pixel | {R, G, B, count}, 4 x uint32 per pixel
	uint64_t dir = 0;                      // the frame's chunk directory: MAX_DIR_CHUNKS addresses
	// per bin: its segment list, its segment counter, {entries, time} of its latest r_overflow (tools/raster_bins.py); the pool comes last: it takes what the buffer has left
	uint64_t binSegs = 0, binSegCount = 0, binStats = 0, binPool = 0;
	uint64_t bytes = 0;                    // the full layout: the whole pool and the tail
	uint32_t binTilesX = 0, binTiles = 0;  // bins per row (pixel columns 0..W: render.cu:91-92 clamps to W, not W - 1), bins in all — 0: more than BIN_MAX_TILES, the frame has no bins
	FrameLayout() = default;
	SIMLOD_HD FrameLayout(uint32_t width, uint32_t height) {
		const uint64_t px = (uint64_t)width * height;
		binTilesX = (width >> BIN_SHIFT) + 1u;
		const uint64_t tiles = (uint64_t)binTilesX * ((height >> BIN_SHIFT) + 1u);
		binTiles = tiles <= BIN_MAX_TILES ? (uint32_t)tiles : 0u;
		work = framebuffer + align16(px * 8);
		items = work + WORK_BYTES;
		depth = items + (uint64_t)MAX_DRAW_ITEMS * ITEM_CLASSES * DRAW_ITEM_BYTES;
		colour = depth + align16(px * 4);
		sums = colour + align16(px * 8);
		dir = sums + px * 16;
		binSegs = dir + (uint64_t)MAX_DIR_CHUNKS * 8;
		binSegCount = binSegs + (uint64_t)binTiles * BIN_SEG_CAP * BIN_SEG_BYTES;
		binStats = binSegCount + align16((uint64_t)binTiles * 4);
		binPool = binStats + (uint64_t)binTiles * BIN_SEG_BYTES;
		bytes = binPool + (binTiles != 0u ? (uint64_t)BIN_POOL_ENTRIES * 16 : 0u) + TAIL_BYTES;
	}
	// 16-byte entries the pool may take in a buffer of bufferBytes: what lies between binPool and the tail, at most min(the knob, BIN_POOL_ENTRIES) (SIMLOD_DEBUG_BIN_POOL: a pool that runs out)
	SIMLOD_HD uint32_t pool_entries(uint64_t bufferBytes, int knobEntries) const {
		const uint64_t knob = knobEntries < 0 ? 0u : (uint64_t)knobEntries < BIN_POOL_ENTRIES ? (uint64_t)knobEntries : BIN_POOL_ENTRIES;
		const uint64_t room = bufferBytes > binPool + TAIL_BYTES ? (bufferBytes - binPool - TAIL_BYTES) / 16 : 0;
		return (uint32_t)(knob < room ? knob : room);
	}
};
// ---- accessors --------------------------------------------------------------------------------------------------------------------------------
SIMLOD_HD inline uint32_t* counter_at(uint8_t* mom, int k) { return reinterpret_cast<uint32_t*>(mom + FrameLayout::counters + COUNTER_STRIDE * k); }
SIMLOD_HD inline uint32_t* work_words(uint8_t* mom, const FrameLayout& lay) { return reinterpret_cast<uint32_t*>(mom + lay.work); }
// Thread 0 of r_visible publishes the launch's sequence number here once the frame's counters are zero, and the waves wait for it: the word must never
// read as the value a stale buffer holds, so no frame zeroes it (W_READY >= W_COUNT) — zeroing would make 0 such a value for an instant.
SIMLOD_HD inline uint32_t* frame_ready_word(uint8_t* mom, const FrameLayout& lay) { return work_words(mom, lay) + W_READY; }
}  // namespace simlod
