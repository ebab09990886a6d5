// render.hip — software point/voxel rasteriser for MI355X (gfx950): the `kernel_render` entry point, and the
// one-thread `kernel` of reset.cu.
//
// Replaces modules/progressive_octree/render.cu:1084-1355 (one persistent cooperative CUDA kernel, ~25 grid.sync())
// behind the same argument list, reading the same Node/Chunk image and leaving the same uint64 framebuffer
// (depth bits << 32 | colour) at the same offset of the momentary buffer.  The only cross-workgroup traffic inside a launch
// is device-scope atomics (visible-node list, work queue, framebuffer).
//
// A frame is a chain of ordinary launches on the caller's stream (simlod_launch_render_part runs it in four parts for multi-GPU frames), in this order:
//   RENDER_FIRST    r_visible: always — counters and planes cleared, visible nodes, draw items, chunk directory;  r_draw<MIN64> (plain frames: the only
//                   draw pass) or r_draw<DEPTH> (HQS: the depth pass);  r_overflow<same mode> when the frame sorts into the screen bins (useBins: the
//                   buffer has room for the pool and its previous frame had nodes to sort);  plain frames with Uniforms.showBoundingBox: the lines
//   RENDER_COLOR    HQS: r_draw<COLOR>, r_overflow<COLOR> when the frame sorts;  in a frame that runs in parts r_unpack (the sums ranks all-reduce)
//   RENDER_RESOLVE  HQS: r_resolve, then the lines (r_lines_emit, r_lines_raster) — unless the resolve is fused into r_output: a whole frame without
//                   debug lines that has a colour buffer (SIMLOD_RASTER_FUSED_RESOLVE)
//   RENDER_OUTPUT   r_output<fused>: always — Stats, EDL, the RGBA8 image
// A frame whose context has a clip (simlod_context_set_clip) runs r_visible and r_draw<mode> WITH the clip as a second kernel argument: the same
// definitions under the Clip policy (render_common.inc).  Every other kernel of the frame is the same.
//
// Arithmetic contract: projection = four fp32 dot products evaluated left to right, IEEE divide,
// pixel coordinate in fp64 exactly as `int x = (ndc.x * 0.5 + 0.5) * width` does (render.cu:66-67), no FMA
// contraction anywhere (this file is compiled with -ffp-contract=off), so the pre-EDL framebuffer is bit-identical
// to the CPU oracle's for the same octree image.
// One translation unit: the layout of the momentary buffer is render_layout.hpp, the device code lies in render_*.inc, k_reset and the
// host side — launch_reset, launch_render — here.
#include "simlod_device.hpp"
#include "simlod_hip.h"
#include "simlod_internal.hpp"
#include "render_layout.hpp"
#include "clip_rules.hpp"
#include <atomic>
#include <chrono>

namespace simlod {

// The device code, pass by pass (textual parts of THIS translation unit; each names what it holds in its first line):
#include "render_common.inc"    // RenderArgs, DrawItem, BinSeg, tile and bin constants, probe macros, dot_row, DPP wave sums, the clears, wait_frame_ready, the clip policies
#include "render_visible.inc"   // frustum_plane, node_geometry, visible_nodes, r_visible
#include "render_draw.inc"      // DrawCtx, the hot table, draw_sample / draw_wave / draw_staged / draw_item, tile_clear / tile_flush, r_draw
#include "render_bins.inc"      // bin_item (r_draw calls it: declared in render_draw.inc), r_overflow
#include "render_lines.inc"     // the debug lines: r_lines_emit, r_lines_raster
#include "render_output.inc"    // r_resolve, r_unpack, resolved_depth_bits, r_output
static_assert(VISIBLE_NODES == SIMLOD_MAX_VISIBLE_NODES && sizeof(SimlodNode) == NODE_BYTES, "render_layout.hpp sizes the visible-node array: SIMLOD_MAX_VISIBLE_NODES whole node records");
static_assert(sizeof(DrawItem) == DRAW_ITEM_BYTES, "tools/raster_items.py reads draw items as 32-byte records");
static_assert(sizeof(BinSeg) == BIN_SEG_BYTES, "render_layout.hpp sizes the bin tables by 8-byte segments");

// ---- reset.cu:20-86 -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_reset(uint8_t* pers, SimlodNode* nodes, SimlodStats* stats, uint32_t* numBatchesUploaded,
                                               uint32_t* batchSizes, uint32_t frameCounter, uint32_t* feedback, uint32_t resetSeq) {
	// The allocator starts at offset 16 and the root's occupancy grid is its first allocation (reset.cu:42-67), so the
	// grid sits at pers + 16: every workgroup can clear its share without waiting for thread 0.
	uint4* grid = reinterpret_cast<uint4*>(pers + 16);
	for (uint32_t w = blockIdx.x * TPB + threadIdx.x; w < SIMLOD_GRID_NUM_WORDS / 4; w += gridDim.x * TPB) grid[w] = make_uint4(0, 0, 0, 0);
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	SimlodAllocatorGlobal* alloc = reinterpret_cast<SimlodAllocatorGlobal*>(pers);
	alloc->buffer = pers;
	alloc->offset = 16 + SIMLOD_ALLOC_ROUND(sizeof(SimlodOccupancyGrid));
	SimlodStats s{};
	s.numNodes = 1;
	s.frameID = frameCounter;
	*stats = s;
	SimlodNode* root = nodes;
	for (int k = 0; k < 8; k++) root->children[k] = nullptr;
	root->isFiltered = 0;
	root->counter = 0; root->numPoints = 0; root->level = 0;
	root->X = 0; root->Y = 0; root->Z = 0;
	root->countIteration = 0;
	for (int k = 0; k < 20; k++) root->name[k] = 0;
	root->name[0] = 'r';
	root->numVoxels = 0; root->numVoxelsStored = 0;
	root->voxelChunks = nullptr;
	root->points = nullptr;     // not in reset.cu: a list surviving the allocator restart would alias new allocations
	root->grid = reinterpret_cast<SimlodOccupancyGrid*>(pers + 16);
	*numBatchesUploaded = 0;
	for (uint32_t k = 0; k < SIMLOD_BATCH_STREAM_SIZE; k++) batchSizes[k] = 0;
	// what the next kernel_construct launches size themselves by (simlod_hip.cpp launch_plan; page-locked): nothing ingested, nothing uploaded, as of this reset
	if (feedback != nullptr) { feedback[0] = 0u; feedback[1] = 0u; feedback[2] = 1u; __hip_atomic_store(feedback + 3, resetSeq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
int launch_reset(Context& ctx, const SimlodUniforms* u, uint8_t* pers, SimlodNode* nodes, SimlodStats* stats, uint32_t* numBatchesUploaded,
                 uint32_t* batchSizes, hipStream_t stream) {
	octree_image_replaced(ctx, nodes);
	uint32_t* words = nullptr; uint32_t seq = 0;
	forget_launch_history(ctx, nodes, numBatchesUploaded, &words, &seq);
	SIMLOD_LAUNCH(k_reset, dim3(64), dim3(TPB), stream, pers, nodes, stats, numBatchesUploaded, batchSizes, (uint32_t)u->frameCounter, words, seq);
	return (int)hipGetLastError();
}

// parts: RENDER_* bits, as in the table at the top of this file
int launch_render(Context& ctx, uint32_t* buffer, const SimlodUniforms* u, SimlodNode* nodes, uint32_t* colorbuffer, SimlodStats* stats,
                  uint64_t* frameStart, hipStream_t stream, uint32_t parts) {
	RenderArgs a{};
	a.mom = reinterpret_cast<uint8_t*>(buffer); a.nodes = nodes; a.stats = stats; a.colorbuffer = colorbuffer; a.frameStart = frameStart;
	a.transform = u->transform; a.transformUpdate = u->transform_updateBound;
	a.width = u->width; a.height = u->height;
	a.W = (int)u->width; a.H = (int)u->height;
	if (a.W <= 0 || a.H <= 0) return (int)hipErrorInvalidValue;
	a.numPixels = (uint32_t)a.W * (uint32_t)a.H;
	octree_box(u, a.cubeSize, a.minx, a.miny, a.minz);                   // render.cu:1135-1137
	a.minNodeSize = u->minNodeSize;
	a.pointSize = u->pointSize;
	a.nodeCapacity = ctx.nodeCapacity.load();
	a.frameCounter = (uint32_t)u->frameCounter;
	a.showPoints = u->showPoints; a.colorByNode = u->colorByNode; a.colorByLOD = u->colorByLOD; a.hqs = u->useHighQualityShading;
	a.lay = FrameLayout((uint32_t)a.W, (uint32_t)a.H);
	LeafTableRef lt;
	if (ctx.tune(KNOB_RASTER_LEAF_TABLE, 1) && find_leaf_table(ctx, nodes, lt)) {
		a.leafTable = lt.table; a.leafTablePers = lt.pers; a.leafTableMagic = lt.magic; a.leafTableBatch = lt.batch; a.leafTableNodes = lt.tableNodes; a.leafTableSig = lt.sig;
		a.leafTableMagicValue = lt.magicValue; a.leafTableSlots = lt.slots; a.leafTableRows = lt.rows;
	}
	a.itemCap = MAX_DRAW_ITEMS;
	a.useTiles = (uint32_t)ctx.tune(KNOB_RASTER_LDS_TILES, 1);
	// SIMLOD_RASTER_SCREEN_BINS: 0 = off, else the screen-box area from which a node sorts, in units of 1024 pixels (default: two tiles)
	const int binKnob = ctx.tune(KNOB_RASTER_SCREEN_BINS, 32);
	a.binsPossible = a.useTiles != 0u && a.lay.binTiles != 0u && binKnob > 0 && a.pointSize == 1 ? 1u : 0u;
	a.binMinArea = (uint32_t)max(binKnob, 0) * 1024u;
	// ... and a frame sorts when the buffer's previous frame had nodes to sort (a frame that has none pays 4-5 us for two idle kernels; one that
	// has some and does not sort them draws them the slow way, with the same result)
	bool possible = a.binsPossible != 0u, bins = false;
	uint64_t bufferBytes = 0;
	a.binFeedback = a.lay.binTiles != 0u ? frame_feedback(ctx, buffer, parts, possible, bins, bufferBytes) : nullptr;      // (parts after the first: what the first part decided)
	a.binsPossible = possible ? 1u : 0u;
	a.useBins = bins ? 1u : 0u;
	if (a.binsPossible) {
		// The reference host allocates 200 000 000 bytes for this buffer whatever the window's size (main_progressive_octree.cpp:555), and the planes and
		// bin tables in front of the pool grow with the frame: 1920 x 1080 leaves room for the whole pool (3 417 331 entries' worth), 2560 x 1440 and 4K
		// for none of it (at 2560 x 1440 the pool would start at byte 206 786 368: such a frame draws without bins).  The pool is what the ALLOCATION
		// behind `buffer` has left (asked once per buffer); samples that find it full take the atomics, as before the bins.
		a.binPoolCap = a.lay.pool_entries(bufferBytes, ctx.tune(KNOB_DEBUG_BIN_POOL, (int)BIN_POOL_ENTRIES));      // (the knob: tests, a pool that runs out)
		if (a.lay.pool_entries(bufferBytes, (int)BIN_POOL_ENTRIES) < BIN_POOL_MIN) { a.binsPossible = 0; a.useBins = 0; frame_feedback_no_bins(ctx, buffer); }
	}
	// (what thread 0 of r_visible publishes once the frame's counters are zero: never the value a stale or poisoned buffer holds)
	static std::atomic<uint32_t> launchSeq{(uint32_t)std::chrono::steady_clock::now().time_since_epoch().count() | 1u};
	a.launchSeq = launchSeq.fetch_add(2u);

	const DeviceInfo& dev = device_info();
	const uint32_t gridPixels = dev.numCUs * 8;
	const uint32_t gridNodes = (a.nodeCapacity + TPB - 1) / TPB;
	// one draw workgroup per CU: its 128 x 128-pixel tile takes 64-128 KB of the CU's 160 KB of LDS.  The depth pass too, though two of
	// its 64 KB tiles would fit: the draw loop is ALU-bound, two workgroups per CU each run at half speed, and the last big items then
	// finish later (HQS frame 0.227 ms against 0.231 ms).
	const uint32_t gridDraw = dev.numCUs * (uint32_t)ctx.tune(KNOB_DRAW_MULT, 1);
	const bool whole = parts == RENDER_ALL;
	// the context's clip, as it is now: copied once, widened on the host, handed to the kernels by value (frames already enqueued keep theirs).
	// colorByNode / colorByLOD win over HIGHLIGHT: such a frame is the unclipped one.
	const SimlodClip clip = clip_of(ctx);
	const bool clipped = clip.mode != SIMLOD_CLIP_OFF && !(clip.mode == SIMLOD_CLIP_HIGHLIGHT && (a.colorByNode || a.colorByLOD));
	const ClipArgs k = clipped ? clip_args(clip, a.cubeSize, a.minx, a.miny, a.minz) : ClipArgs{};
	auto lines = [&]() {
		if (!u->showBoundingBox) return;
		SIMLOD_LAUNCH(r_lines_emit, dim3((SIMLOD_MAX_VISIBLE_NODES + TPB - 1) / TPB), dim3(TPB), stream, a, u->transformInv_updateBound);
		SIMLOD_LAUNCH(r_lines_raster, dim3((LINE_VERTEX_CAP / 2 + TPB - 1) / TPB), dim3(TPB), stream, a);
	};
	if (parts & RENDER_FIRST) {
		if (clipped) SIMLOD_LAUNCH(r_visible, dim3(gridNodes), dim3(TPB), stream, a, k);
		else SIMLOD_LAUNCH(r_visible, dim3(gridNodes), dim3(TPB), stream, a);
		if (a.hqs) {
			if (clipped) SIMLOD_LAUNCH(r_draw<MODE_DEPTH>, dim3(gridDraw), dim3(DTPB), stream, a, k);
			else SIMLOD_LAUNCH(r_draw<MODE_DEPTH>, dim3(gridDraw), dim3(DTPB), stream, a);
			if (a.useBins) SIMLOD_LAUNCH(r_overflow<MODE_DEPTH>, dim3(a.lay.binTiles), dim3(OTPB), stream, a);
		} else {
			if (clipped) SIMLOD_LAUNCH(r_draw<MODE_MIN64>, dim3(gridDraw), dim3(DTPB), stream, a, k);
			else SIMLOD_LAUNCH(r_draw<MODE_MIN64>, dim3(gridDraw), dim3(DTPB), stream, a);
			if (a.useBins) SIMLOD_LAUNCH(r_overflow<MODE_MIN64>, dim3(a.lay.binTiles), dim3(OTPB), stream, a);
			lines();
		}
	}
	if (a.hqs && (parts & RENDER_COLOR)) {
		if (clipped) SIMLOD_LAUNCH(r_draw<MODE_COLOR>, dim3(gridDraw), dim3(DTPB), stream, a, k);
		else SIMLOD_LAUNCH(r_draw<MODE_COLOR>, dim3(gridDraw), dim3(DTPB), stream, a);
		if (a.useBins) SIMLOD_LAUNCH(r_overflow<MODE_COLOR>, dim3(a.lay.binTiles), dim3(OTPB), stream, a);
		if (!whole) SIMLOD_LAUNCH(r_unpack, dim3(gridPixels), dim3(TPB), stream, a);     // ranks all-reduce(SUM) the {R,G,B,count} plane
	}
	// whole HQS frames without debug lines resolve inside r_output
	const bool fused = a.hqs && whole && !u->showBoundingBox && colorbuffer != nullptr && ctx.tune(KNOB_RASTER_FUSED_RESOLVE, 1) != 0;
	if (a.hqs && (parts & RENDER_RESOLVE) && !fused) {
		SIMLOD_LAUNCH(r_resolve, dim3(gridPixels), dim3(TPB), stream, a);
		lines();
	}
	if (parts & RENDER_OUTPUT) {
		const dim3 gridOutput((uint32_t)(a.W + OUT_TW - 1) / OUT_TW, (uint32_t)(a.H + OUT_TH - 1) / OUT_TH);
		if (fused) SIMLOD_LAUNCH(r_output<true>, gridOutput, dim3(TPB), stream, a);
		else SIMLOD_LAUNCH(r_output<false>, gridOutput, dim3(TPB), stream, a);
	}
	if (profile_enabled()) profile_close(stream);
	return (int)hipGetLastError();
}

}  // namespace simlod
