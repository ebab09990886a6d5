/* simlod_hip.h — C ABI of libsimlod_hip.so, the MI355X (gfx950) implementation of SimLOD's two hot paths.
 *
 * Drop-in boundary.  The reference host reaches its device code through exactly one surface:
 *
 *     CudaModularProgram({.modules = {...cu paths}, .kernels = {names}})      include/CudaModularProgram.h:166-190
 *     program->kernels["name"]  -> CUfunction                                 include/CudaModularProgram.h:241-256
 *     cuLaunchCooperativeKernel(fn, gx,gy,gz, bx,by,bz, smem, stream, void** args)
 *                                         modules/progressive_octree/main_progressive_octree.cpp:351, :396, :507
 *
 * with three programs / kernels:
 *     reset  : {reset.cu, utils.cu}                    -> "kernel"             main_progressive_octree.cpp:620-626
 *     update : {progressive_octree_voxels.cu, utils.cu} -> "kernel_construct"  main_progressive_octree.cpp:603-610
 *     render : {render.cu, utils.cu}                   -> "kernel_render"      main_progressive_octree.cpp:612-618
 *
 * This header exports that surface 1:1 (simlod_program_* / simlod_launch_cooperative, same argument arrays as
 * the reference builds at main_progressive_octree.cpp:337-345, :374-382, :499-507) plus typed entry points for
 * hosts that prefer not to build void* arrays.  All pointers are DEVICE pointers unless stated otherwise; all
 * structs are the ones of simlod_abi.h.  Every function returns 0 on success or a hipError_t value; launches are
 * asynchronous on `stream` (a hipStream_t passed as void*; NULL = the null stream), like the reference's.
 *
 * Device-side conditions the reference reports by printf or by silently dropping data are
 * reported in Stats.dbg (a field the reference never writes) as a bit mask of SIMLOD_ERR_*.
 */
#ifndef SIMLOD_HIP_H
#define SIMLOD_HIP_H

#include "simlod_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Stats.dbg bits */
#define SIMLOD_ERR_MOMENTARY_TOO_SMALL 0x001u /* Uniforms.momentaryBufferCapacity cannot hold the scratch layout   */
#define SIMLOD_ERR_SPILLED_OVERFLOW    0x002u /* spill space exhausted: some splits were DEFERRED to a later batch (no point lost) */
#define SIMLOD_ERR_SPILLING_OVERFLOW   0x004u /* more leaves cross the limit at once than one split round holds (65 536; voxels.cu:847: 100 000): the rest is deferred */
#define SIMLOD_ERR_NODES_EXHAUSTED     0x008u /* node array full (main_progressive_octree.cpp:552: 263 157 nodes): leaves stop splitting */
#define SIMLOD_ERR_DIRECTORY_FULL      0x010u /* FATAL: directory of the chunks allocated in a batch full (sticky until reset) */
#define SIMLOD_ERR_NULL_CHUNK          0x020u /* insert into a leaf without storage (voxels.cu:599-604)             */
#define SIMLOD_ERR_BARRIER_TIMEOUT     0x040u /* FATAL: in-kernel grid barrier of the split cascade gave up (sticky until reset) */
#define SIMLOD_ERR_CHUNK_QUEUE_OVERFLOW 0x080u /* > 1 000 000 recycled chunks (voxels.cu:856)                        */
#define SIMLOD_ERR_VISIBLE_OVERFLOW    0x100u /* > 100 000 visible nodes (render.cu:1108)                           */
#define SIMLOD_ERR_ACCOUNTING          0x200u /* exact mode, launches of several batches: the per-batch chunk accounting of a group did not end at the chunk count the octree has (Stats.allocatedBytes_persistent / chunkPoolSize may differ from the reference's; the octree itself is sound) */

/* ---- per-octree contexts --------------------------------------------------------------------------------------------------------
 * The reference host keeps ONE octree per process and its launch signatures carry no handle (main_progressive_octree.cpp:337-345,
 * :374-382, :499-507).  What this library keeps between launches — ingest mode, node capacity, batch limit, tuning knobs, its second
 * stream and events, the table registry that links kernel_construct to kernel_render, the launch feedback — lives in a context; a
 * launch finds its context through the NODE ARRAY it is given.  Node arrays that were never attached share the default context, which
 * is what the simlod_set_* calls below configure: a host with one octree never needs these functions.  A host with several octrees
 * (one per tile, per data set, per thread) makes a context per octree and attaches the octree's node array to it.
 *
 * Tuning knobs (SIMLOD_OVERLAP_TAIL, SIMLOD_EXPAND_WGS, SIMLOD_GRID_MULT, SIMLOD_COUNT_TPB, SIMLOD_VOXELIZE_WGS, SIMLOD_ADAPTIVE_GROUPS,
 * SIMLOD_RASTER_LEAF_TABLE, SIMLOD_RASTER_LDS_TILES, SIMLOD_DRAW_MULT, SIMLOD_RASTER_FUSED_RESOLVE, SIMLOD_DEBUG_FORCE_BARRIER_TIMEOUT,
 * SIMLOD_DEBUG_VOXELIZE_CLOCK, SIMLOD_DEBUG_BUDGET_US, SIMLOD_GROUP_BATCHES, SIMLOD_DEBUG_PHASE_WG, SIMLOD_EVENT_SYSTEM_FENCE — 1: the
 * events between the builder's two streams keep the system-scope fence HIP gives an event by default —, SIMLOD_RASTER_SCREEN_BINS — 0:
 * no screen bins; n: nodes whose screen box exceeds n x 1024 pixels sort their samples into the bins (default 32) —,
 * SIMLOD_DEBUG_BIN_POOL — entries of the bin pool, for tests —, SIMLOD_EXACT_GROUP — batches an EXACT-mode group may have (default 5, at most 12;
 * 1: one batch per group as before round 6; the momentary buffer's size decides how many fit) —, SIMLOD_DEBUG_IRREGULAR_CHILDREN — 1: every inner node's child word
 * sends k_count's descent through Node.children (the path of an image whose children are not eight consecutive nodes; for tests)) are read from the environment ONCE, when a context is made (the default
 * context: at its first use); simlod_context_set_knob overrides one by name (set = 0: back to the built-in default),
 * simlod_context_reload_env reads the environment again.  ctx == NULL means the default context everywhere. */
typedef struct SimlodContext SimlodContext;
int simlod_context_create(SimlodContext** out);
int simlod_context_destroy(SimlodContext* ctx);                               /* synchronises the device, detaches the context's node arrays; no launch with one of them may be in progress on another thread */
int simlod_context_attach(SimlodContext* ctx, const SimlodNode* nodes);       /* launches given `nodes` run in ctx from now on (NULL: default again) */
int simlod_context_set_node_capacity(SimlodContext* ctx, uint32_t numNodes);
int simlod_context_set_ingest_mode(SimlodContext* ctx, uint32_t mode);
int simlod_context_set_construct_batch_limit(SimlodContext* ctx, uint32_t maxBatches);
/* "That many ring batches are pending right now" (uploaded and not ingested, not counting what launches already enqueued will take): for the NEXT
 * kernel_construct launch of the context only — it enqueues kernels for that many batches (0: none, an idle frame), whatever the library would have
 * guessed.  The hint is consumed by the context's next launch, whichever octree that launch is for (a launch uses at most its batch limit of it, a chain —
 * simlod_launch_construct_chain — up to launches x that).  Optional: hosts whose upload-counter writes reach simlod_upload_counter_written (shim/cuda.h does that for the reference's) need not call it. */
int simlod_context_hint_pending_batches(SimlodContext* ctx, uint32_t pending);
/* The host has enqueued a write of `value` to the 4-byte upload counter at `numBatchesUploaded` (main_progressive_octree.cpp:1047-1050:
 * cuMemsetD32Async(cptr_numBatchesUploaded, batchStreamUploadIndex + 1, 1, stream_upload)).  kernel_construct reads the counter on the device when it
 * runs (voxels.cu:870-885); the library, which has to enqueue a group of kernels per batch BEFORE that, sizes its launches by what it is told here and by
 * what its earlier launches reported.  Addresses that no reset / construct launch has been given as `numBatchesUploaded` are ignored (the shims forward
 * every 4-byte memset).  Without it the library predicts from its launches' own reports alone: at least one group per launch, a burst picked up a launch late. */
int simlod_upload_counter_written(const void* numBatchesUploaded, uint32_t value);
/* Multi-GPU jobs (no counterpart in the reference, which is single-GPU: main_progressive_octree.cpp:274, CudaModularProgram.h:215).  Ranks own
 * level-3 cells of ONE global cube; the nodes of levels 0-2 exist on every rank.  The single-GPU octree of the whole data set splits such a
 * node when the GLOBAL count under it crosses 50 000 (progressive_octree_voxels.cu:209-217); a rank that looked at its own count would keep it
 * as a leaf and kernel_render would draw its points where one GPU draws the node's voxels (render.cu:918-932).  So the host names the upper
 * nodes whose global count exceeds the limit — 73 bits: bit 0 the root; bit 1 + c the level-1 node with cell code c = x << 2 | y << 1 | z;
 * bit 9 + c the level-2 node, c = its level-1 octant << 3 | the octant below (lo: bits 0..63, hi: bits 64..72) — and kernel_construct splits
 * such a node as soon as it exists, whatever it holds: in the first batch ingested after the call, or, when no batch is pending, by a batch
 * of ZERO points (publish batchSizes[slot] = 0 and bump numBatchesUploaded).  A named node's parent must be named too (hipErrorInvalidValue).
 * Mask 0 (the default): the reference's rule alone — every Node and Stats field is the reference's.  simlod_amd/distributed.py trunk_mask
 * derives the mask from the all-reduced histogram over the 512 level-3 cells; with it the composed frame of N ranks
 * (simlod_render_frame_composed) has the single-GPU frame's depth at every pixel. */
int simlod_context_set_trunk_mask(SimlodContext* ctx, uint64_t lo, uint64_t hi);
int simlod_context_set_knob(SimlodContext* ctx, const char* name, int value, int set);
int simlod_context_reload_env(SimlodContext* ctx);
uint64_t simlod_context_construct_buffer_min_bytes(SimlodContext* ctx);

/* Number of Node records the host's node buffer holds (default 263 157 = 40 000 000 / 152,
 * main_progressive_octree.cpp:552).  Default context; set before the first reset if the host allocates differently. */
int simlod_set_node_capacity(uint32_t numNodes);

/* Ingest granularity of kernel_construct.  0 (default) = EXACT: one ring batch at a time, as progressive_octree_voxels.cu:883-949 does
 * — every Node and Stats field after every batch is the reference's.  1 = COALESCED: all pending batches of a launch (<= 20, as many
 * as the momentary buffer holds) are ingested as one batch.  Topology, per-node sample multisets, occupancy bitsets, voxel positions
 * and counts do not depend on the granularity; the allocator / chunk-pool accounting (Stats.allocatedBytes_persistent,
 * numAllocatedChunks, chunkPoolSize) does: fewer intermediate chunks are ever allocated.  Default context.
 * Voxel colours: the reference colours a voxel from a point of the first batch that hit its cell.  EXACT mode voxelizes a launch's batches in
 * groups (SIMLOD_EXACT_GROUP, default 5): a voxel's colour comes from a point of the GROUP that holds that batch (or from a stored point an
 * earlier batch brought); SIMLOD_EXACT_GROUP=1 gives the reference's outcome set.  COALESCED mode: from the launch that holds that batch. */
int simlod_set_ingest_mode(uint32_t mode);

/* Optional host hint: no more than `maxBatches` (1..20, default 20) ring batches are pending when kernel_construct is launched, so
 * no more than that many per-batch kernel groups need to be enqueued (the reference host knows its upload counter,
 * main_progressive_octree.cpp:1012-1050).  A launch never ingests more than this many batches.  Default context. */
int simlod_set_construct_batch_limit(uint32_t maxBatches);

/* kernel_render reads the chunk lists of visible nodes through a table kernel_construct keeps in ITS momentary buffer (one row of chunk
 * addresses per node), for as long as a stamp in that buffer says the table describes the octree in `nodes` as it is now: same node
 * array, same Stats.batchletIndex / numNodes / numPoints / numVoxels / allocatedBytes_persistent as after the last kernel_construct.
 * kernel_reset drops the association.  A host that writes an octree image into `nodes` / the persistent buffer by other means
 * (memcpy of a saved image) calls this afterwards; kernel_render then walks the `next` pointers, as the reference does
 * (render.cu:106-159), until kernel_construct has run again. */
int simlod_octree_image_replaced(const SimlodNode* nodes);

/* Byte offset of the uint64 framebuffer inside kernel_render's momentary `buffer` (identical to where the
 * reference's bump allocator places it, render.cu:1108-1123) and the size of that buffer's full layout: planes, draw items, chunk directory
 * and, last, the screen bins (a 48 MB pool of 16-byte entries + per-bin tables) that frames with very large nodes sort their samples into.
 * 1920 x 1080: 193.5 MB — inside the 200 000 000 bytes the reference host allocates whatever its window's size (main_progressive_octree.cpp:555).
 * Larger frames need more for the full layout (1920 x 1200: 202 MB, 2560 x 1440: 255 MB); a buffer that is smaller is still fine as long as it
 * holds everything in front of the bin pool (2560 x 1440: 206.8 MB): kernel_render asks the runtime how large the ALLOCATION behind `buffer` is
 * (hipMemGetAddressRange) and sizes the pool by what is left — with less than 1 MB left it draws without bins (same frame, the samples of
 * screen-filling nodes take device-scope atomics).  A host that carves `buffer` out of a larger allocation of its own must therefore give it
 * simlod_render_buffer_bytes(width, height): what lies behind `buffer` inside that allocation is taken for the pool. */
uint64_t simlod_render_framebuffer_offset(void);
uint64_t simlod_render_buffer_bytes(uint32_t width, uint32_t height);
/* Minimum size of kernel_construct's momentary `buffer` (the host allocates 300 MB, main_progressive_octree.cpp:554). */
uint64_t simlod_construct_buffer_min_bytes(void);

/* ---- typed launches -------------------------------------------------------------------------------------- */
/* reset.cu:20-29  `kernel` */
int simlod_launch_reset(const SimlodUniforms* uniforms /*host*/, uint8_t* buffer_octree, SimlodNode* nodes,
                        SimlodStats* stats, void* cudaprint, uint32_t* numBatchesUploaded, uint32_t* batchSizes,
                        void* stream);

/* progressive_octree_voxels.cu:804-816  `kernel_construct` */
int simlod_launch_construct(const SimlodUniforms* uniforms /*host*/, SimlodPoint* points, uint32_t* buffer,
                            uint8_t* buffer_persistent, SimlodNode* nodes, SimlodStats* stats,
                            uint64_t* frameStartTimestamp, void* cudaprint, uint32_t* numBatchesUploaded_volatile,
                            uint32_t* batchSizes, void* stream);

/* A CHAIN of kernel_construct launches: one call that stands for `launches` (>= 1) consecutive simlod_launch_construct calls with NOTHING between
 * them on the stream — a host that drains a burst of uploaded batches and looks at the octree only afterwards.  Between two such launches the
 * builder's two-stream pipeline would drain (the last group's back half, the tail kernels, the next launch's k_begin, its first group's front half,
 * one after the other); inside a chain that seam is an ordinary group boundary.  Contract:
 *   - the effect is that of `launches` consecutive simlod_launch_construct calls with nothing between them; the octree, Stats and the launch report
 *     are those of the LAST of them.  No intermediate state is observable — whatever the caller enqueues next on `stream` sees the complete octree
 *     and complete Stats, as after simlod_launch_construct;
 *   - launches == 1 IS simlod_launch_construct: the same code path, the same kernels in the same order;
 *   - the upload counter is read ONCE, by the chain's k_begin: batches published while the chain runs are taken by the next launch, as with a
 *     launch today (consecutive launches would each have looked);
 *   - a SEGMENT is what one of those launches would have taken: L = min(the context's construct batch limit, 20) batches, counted from the chain's
 *     first batch.  Groups of batches (SIMLOD_EXACT_GROUP, coalesced mode) never straddle a segment boundary: 36 batches in groups of five are
 *     ingested as 5,5,5,5 | 5,5,5,1, the groups — and so the voxel colours — of the two-launch run.  The 10 ms time budget is per segment;
 *   - the chain is sized as ONE launch for up to launches x L batches (told counter, hint, reports, prediction; the cap when nothing is known), and
 *     simlod_context_hint_pending_batches may name up to launches x L for it;
 *   - a chain that would go batch by batch (exact mode near the memory guard, a forced time budget, SIMLOD_EXACT_GROUP=1) or that finds at most
 *     one group is issued as plain launches, one per segment, exactly as today; a chain whose groups exceed what one device launch can number
 *     (20) is cut into several device launches inside the call;
 *   - a chain may STOP earlier than the launches it stands for would: once a segment stops (time budget, memory guard), the segments behind it take
 *     nothing, and the memory guard treats the first group of a later segment like any group inside a launch (conservatively, while the voxel half
 *     of the group before may still allocate).  The host launches again, as it does after any launch that left batches pending; that launch's first
 *     group is decided exactly, and the end state is the reference's.
 * A host that renders, reads Stats or uploads by Stats between launches keeps calling simlod_launch_construct. */
int simlod_launch_construct_chain(const SimlodUniforms* uniforms /*host*/, SimlodPoint* points, uint32_t* buffer,
                                  uint8_t* buffer_persistent, SimlodNode* nodes, SimlodStats* stats,
                                  uint64_t* frameStartTimestamp, void* cudaprint, uint32_t* numBatchesUploaded_volatile,
                                  uint32_t* batchSizes, uint32_t launches, void* stream);

/* render.cu:1084-1093  `kernel_render`; `colorbuffer` stands for the GL surface: a linear width*height RGBA8 image */
int simlod_launch_render(uint32_t* buffer, const SimlodUniforms* uniforms /*host*/, SimlodNode* nodes,
                         uint32_t* colorbuffer, SimlodStats* stats, uint64_t* frameStartTimestamp, void* cudaprint,
                         void* stream);

/* colorfilter.cu:163-169  `kernel` of the colour-filter module (its host call is commented out in the reference,
 * main_progressive_octree.cpp:430-462): every voxel of every inner node becomes the average colour of the child samples in its cell,
 * bottom-up, ten levels of inner nodes per call.  `buffer` is the momentary buffer (Uniforms.momentaryBufferCapacity bytes, at least
 * simlod_colorfilter_buffer_min_bytes()); `numNodes` is a DEVICE pointer to the node count, or NULL for Stats.numNodes.  Voxel
 * positions, counts and list structure stay as they are; Node.isFiltered is set on every node that was processed. */
int simlod_launch_colorfilter(const SimlodUniforms* uniforms /*host*/, uint32_t* buffer, SimlodNode* nodes, uint32_t* numNodes,
                              SimlodStats* stats, void* stream);
uint64_t simlod_colorfilter_buffer_min_bytes(void);

/* kernel_render in four parts, for frames composed across GPUs (the reference is single-GPU).  Every rank calls the
 * parts in order on its own octree and reduces the named plane of the render buffer over all ranks in between:
 *   part 0  clear, visibility, first pass — plain: the 64-bit atomicMin pass and the debug lines; HQS: the depth pass
 *           HQS: all-reduce(MIN, 32-bit) of the depth plane   [simlod_render_depth_plane_offset, width*height uint32]
 *   part 1  HQS only: colour pass, sums folded into the sum planes
 *           HQS: all-reduce(SUM, 32-bit) of the sum planes     [simlod_render_sum_planes_offset, width*height x {R,G,B,count} uint32]
 *   part 2  HQS only: resolve (render.cu:607-632), then the debug lines
 *           all-reduce(MIN, 64-bit) of the framebuffer          [simlod_render_framebuffer_offset, width*height uint64; the stored
 *           words never have the sign bit set, so a signed MIN will do] — for HQS only needed when showBoundingBox is set
 *   part 3  Stats, EDL, RGBA8 output
 * With one rank and no reductions the four parts produce exactly the frame of simlod_launch_render. */
int simlod_launch_render_part(uint32_t part, uint32_t* buffer, const SimlodUniforms* uniforms /*host*/, SimlodNode* nodes,
                              uint32_t* colorbuffer, SimlodStats* stats, uint64_t* frameStartTimestamp, void* cudaprint,
                              void* stream);
uint64_t simlod_render_depth_plane_offset(uint32_t width, uint32_t height);
uint64_t simlod_render_sum_planes_offset(uint32_t width, uint32_t height);
/* The whole layout of kernel_render's `buffer` for a width x height frame (simlod_amd/csrc/render_layout.hpp states it; this is its image for
 * hosts and tools): byte offsets of every region in buffer order, `bytes` = simlod_render_buffer_bytes(width, height), and the few sizes a reader
 * of the regions needs.  `framebuffer`, `depth` and `sums` are what the three offset queries above return.  The frame's counters are 32-bit words
 * `counterStride` bytes apart from `counters` on; `work` holds 32-bit words (their indices: the W_* enum of render_layout.hpp, abi.py WORK_WORDS);
 * `items` holds `itemClasses` arrays of `maxDrawItems` records of `drawItemBytes`; `binSegs` lists per bin 256 segments of `binSegBytes`, `binStats`
 * one such record per bin, `binPool` 16-byte entries up to the buffer's tail.  binTiles == 0: a frame too large for the bins; `probe`: the clock
 * words of a -DVAR_PROBE build, inside the vertex array.  hipErrorInvalidValue for out == NULL or a zero width or height. */
typedef struct SimlodFrameLayout {
	uint64_t visible, counters, lines, vertices, probe, framebuffer;
	uint64_t work, items, depth, colour, sums, dir;
	uint64_t binSegs, binSegCount, binStats, binPool;
	uint64_t bytes, binTiles, binTilesX;
	uint64_t counterStride, drawItemBytes, binSegBytes, maxDrawItems, itemClasses;
} SimlodFrameLayout;
SIMLOD_STATIC_ASSERT(sizeof(SimlodFrameLayout) == 192, "SimlodFrameLayout: 24 x uint64");
int simlod_render_frame_layout(uint32_t width, uint32_t height, SimlodFrameLayout* out);

/* The four parts and the reductions between them in ONE call, for hosts that are not Python (simlod_amd/distributed.py render_frame is the
 * same sequence over torch.distributed).  `reduce` is called on the launch stream's timeline, between the parts, with the plane to reduce
 * IN PLACE over all ranks: `data` (device memory inside `buffer`), `count` elements of `elemBytes` bytes, `op`; it returns 0 or an error
 * code, which ends the frame.  Plane and order, per frame:
 *     HQS:   SIMLOD_PLANE_DEPTH (uint32, MIN) after part 0;  SIMLOD_PLANE_SUMS (uint32 x 4 per pixel, SUM) after part 1;
 *            SIMLOD_PLANE_FRAMEBUFFER (uint64, MIN) after part 2 only when Uniforms.showBoundingBox is set
 *     plain: SIMLOD_PLANE_FRAMEBUFFER (uint64, MIN) after part 0
 * reduce == NULL: no reduction — the frame of simlod_launch_render.  The all-gather of the visible-node records (the first Stats.numVisibleNodes
 * records of `buffer`, 152 bytes each) is the host's own business: nothing in the frame depends on it. */
#define SIMLOD_PLANE_DEPTH       0u
#define SIMLOD_PLANE_SUMS        1u
#define SIMLOD_PLANE_FRAMEBUFFER 2u
#define SIMLOD_REDUCE_MIN        0u
#define SIMLOD_REDUCE_SUM        1u
typedef int (*SimlodReduceFn)(void* user, uint32_t plane, void* data, uint64_t count, uint32_t elemBytes, uint32_t op, void* stream);
int simlod_render_frame_composed(uint32_t* buffer, const SimlodUniforms* uniforms /*host*/, SimlodNode* nodes, uint32_t* colorbuffer,
                                 SimlodStats* stats, uint64_t* frameStartTimestamp, void* cudaprint, void* stream,
                                 SimlodReduceFn reduce, void* user);
/* ... with the reductions as ncclAllReduce calls on `ncclComm` (an ncclComm_t of RCCL: one rank per GPU over xGMI), enqueued on `stream`.
 * RCCL is looked up when this is first called — the copy already loaded in the process (the one that made `ncclComm`: a PyTorch process has its own
 * torch/lib/librccl.so), else dlopen("librccl.so"); the library itself does not link against it.  hipErrorNotSupported if there is none, or if
 * ncclGetVersion names a release outside 2.10 .. 2.x: the call passes ncclDataType_t / ncclRedOp_t by their 2.x numbers (ncclUint32 = 3,
 * ncclUint64 = 5, ncclSum = 0, ncclMin = 3).  simlod_rccl_version(): the NCCL_VERSION_CODE found (0: none). */
int simlod_render_frame_rccl(uint32_t* buffer, const SimlodUniforms* uniforms /*host*/, SimlodNode* nodes, uint32_t* colorbuffer,
                             SimlodStats* stats, uint64_t* frameStartTimestamp, void* cudaprint, void* stream, void* ncclComm);
int simlod_rccl_version(void);

/* ---- CudaModularProgram-shaped surface ------------------------------------------------------------------- */
typedef struct SimlodProgram SimlodProgram;
typedef struct SimlodFunction SimlodFunction;

/* Mirrors CudaModularProgram's constructor: module paths are matched by file name (reset.cu,
 * progressive_octree_voxels.cu, render.cu, utils.cu); the device code is precompiled for gfx950, nothing is
 * compiled at run time (colorfilter.cu -> `kernel` is known as well).  Unknown kernel names make the call fail with hipErrorNotFound. */
int simlod_program_create(SimlodProgram** out, const char* const* modules, int numModules,
                          const char* const* kernels, int numKernels);
void simlod_program_destroy(SimlodProgram* program);
/* program->kernels[name]; NULL when absent */
SimlodFunction* simlod_program_kernel(SimlodProgram* program, const char* name);
/* cuOccupancyMaxActiveBlocksPerMultiprocessor stand-in used by main_progressive_octree.cpp:494-496 */
int simlod_function_max_active_blocks(SimlodFunction* fn, int blockSize, int* numBlocks);
/* cuLaunchCooperativeKernel stand-in.  `args` holds pointers to the kernel arguments in declaration order, the
 * Uniforms struct by value (i.e. args[k] points at a host Uniforms).  The requested geometry is accepted and
 * ignored: the implementation sizes its own launches for the 256 CUs / 8 XCDs of the device. */
int simlod_launch_cooperative(SimlodFunction* fn, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned by,
                              unsigned bz, unsigned sharedMemBytes, void* stream, void** args);

/* ---- measurement aid (not part of the reference surface) ------------------------------------------------------
 * When enabled, every internal kernel launch is bracketed by HIP events recorded on the launch stream, so that
 * bench.py can attribute device time to the kernels rocprofv3 lists.  Off by default (zero overhead). */
typedef struct SimlodProfileEntry {
	char     name[48];     /* internal kernel name, e.g. "k_insert", "r_draw<MODE_MIN64>" */
	uint32_t launches;
	uint32_t pad;
	double   total_ms;
} SimlodProfileEntry;
int simlod_profile_enable(int on);             /* 0 off | 1 every kernel (the builder's two streams become one) | 2 k_voxelize only, on its own stream: the builder's pipeline as in production */
int simlod_profile_collect(SimlodProfileEntry* out, int capacity, int* count);

/* ---- loader side -------------------------------------------------------------------------------
 * Replaces the parse loop of loadLasNative (modules/progressive_octree/LasLoader.cpp:169-227, called by the loader threads at
 * main_progressive_octree.cpp:866-870): `records` = numPoints raw LAS point records of bytesPerPoint bytes each, in DEVICE
 * memory (16-byte aligned), exactly the bytes the reference reads from offsetToPointData + bytesPerPoint * firstPoint;
 * `format` = LasHeader.format (RGB is taken for 2, 3, 5 and 7, as in the reference); scale = LasHeader.scale;
 * offset[k] = LasHeader.offset[k] + translation[k] (the sum the reference forms at LasLoader.cpp:197-199, translation = -boxMin).
 * out = numPoints Points, e.g. a slot of the batch ring.  Positions and r,g,b are bit-identical to the reference's; alpha,
 * which the reference leaves uninitialised, is 255.  Returns 0 or a hipError_t (invalid value: bytesPerPoint outside [12, 255],
 * RGB beyond the record, misaligned pointers). */
int simlod_decode_las(const void* records, uint64_t numPoints, uint32_t bytesPerPoint, uint32_t format,
                      const double scale[3], const double offset[3], SimlodPoint* out, void* stream);

/* ---- styled decode: colour by attribute (no counterpart in the reference, whose loader takes RGB or nothing) -------------------------
 * simlod_decode_las with the colour taken from one attribute of the record through a 256-entry table.  Positions are simlod_decode_las's.
 *
 * The colour of a scalar attribute with value v (fp64):
 *     inv = 256.0 / (hi - lo)            formed once, on the host
 *     t   = (v - lo) * inv               fp64 subtract, then fp64 multiply, never contracted
 *     idx = t >= 0 ? (t < 256 ? (uint32)t : 255) : 0          (a NaN gives 0)
 *     colour = 0xff000000 | (lut[idx] & 0xffffff)
 * With lo = 0, hi = 256 a byte attribute indexes the table with itself.  v and its place in the record (ASPRS LAS 1.4 R15, tables 7-17):
 *     attribute           formats 0-5                             formats 6-10
 *     intensity           u16 @ 12                                u16 @ 12
 *     return number       byte 14, bits 0-2                       byte 14, bits 0-3
 *     number of returns   byte 14, bits 3-5                       byte 14, bits 4-7
 *     classification      byte 15, bits 0-4 (flags masked off)    u8 @ 16
 *     user data           u8 @ 17                                 u8 @ 17
 *     scan angle (deg)    i8 @ 16                                 i16 @ 18, times 0.006 (one fp64 multiply)
 *     point source id     u16 @ 18                                u16 @ 20
 *     GPS time            f64 @ 20 (formats 1, 3, 4, 5 only)      f64 @ 22
 *     elevation           (double)Z * scale[2] + offset[2]        the same
 * Elevation is the fp64 value the position's z is rounded from: it is in the frame `offset` translates into.
 * SIMLOD_LAS_RGB takes the RGB triple (c > 255 ? c / 256 : c per channel) of every format that has one — 2, 3, 5 at 20, 28, 28 and 7, 8, 10 at
 * 30 — and leaves the others black; lo, hi and lut are ignored.  For formats 2, 3, 5, 7 that is simlod_decode_las's output, byte for byte.
 * style == NULL is simlod_decode_las itself.  hipErrorInvalidValue, nothing launched or written: whatever simlod_decode_las refuses, format > 10,
 * an unknown attribute, reserved != 0, lo or hi not finite or hi <= lo, an attribute the format lacks, a field that ends beyond bytesPerPoint.
 * Asynchronous on `stream`; no allocation, synchronisation or copy of its own: the style travels in the kernel's arguments. */
enum { SIMLOD_LAS_RGB = 0, SIMLOD_LAS_INTENSITY, SIMLOD_LAS_CLASSIFICATION, SIMLOD_LAS_RETURN_NUMBER,
       SIMLOD_LAS_NUMBER_OF_RETURNS, SIMLOD_LAS_USER_DATA, SIMLOD_LAS_POINT_SOURCE_ID, SIMLOD_LAS_SCAN_ANGLE,
       SIMLOD_LAS_GPS_TIME, SIMLOD_LAS_ELEVATION, SIMLOD_LAS_ATTRIBUTE_COUNT };
typedef struct SimlodLasStyle {      /* host memory; read completely before the call returns */
	uint32_t attribute;              /* SIMLOD_LAS_* */
	uint32_t reserved;               /* 0 */
	double   lo, hi;                 /* the window mapped onto the table; finite, hi > lo (ignored for RGB) */
	uint32_t lut[256];               /* 0x00BBGGRR; the top byte is ignored, the alpha written is always 255 */
} SimlodLasStyle;
SIMLOD_STATIC_ASSERT(sizeof(SimlodLasStyle) == 1048, "LasStyle");
SIMLOD_STATIC_ASSERT(offsetof(SimlodLasStyle, lo) == 8, "LasStyle.lo");
SIMLOD_STATIC_ASSERT(offsetof(SimlodLasStyle, hi) == 16, "LasStyle.hi");
SIMLOD_STATIC_ASSERT(offsetof(SimlodLasStyle, lut) == 24, "LasStyle.lut");
int simlod_decode_las_styled(const void* records, uint64_t numPoints, uint32_t bytesPerPoint, uint32_t format,
                             const double scale[3], const double offset[3], const SimlodLasStyle* style,
                             SimlodPoint* out, void* stream);

/* ---- workload generator (BASELINE config 4; no counterpart in the reference) ------------------------------------------------------------
 * Points firstIndex .. firstIndex + numPoints - 1 of a procedurally generated, tiled terrain, written to `out` (device memory): the
 * stream is tile after tile (`pointsPerTile` points each, tiles laid out row-major with `tilesX` tiles per row, each tileExtent[0] x
 * tileExtent[1] metres, heights within [0, tileExtent[2])), inside a tile swath by swath like an airborne LAS scan.  One continuous
 * surface over all tiles; a pure function of (seed, index), so every rank of a multi-GPU job can generate any part of the stream. */
int simlod_generate_terrain(SimlodPoint* out, uint64_t numPoints, uint64_t firstIndex, uint64_t pointsPerTile, uint32_t seed,
                            uint32_t tilesX, const float tileExtent[3], void* stream);
/* The same stream with flight lines: inside a tile the points come in strips of `swathWidth` metres (along x), each strip row by row —
 * what an airborne scanner with a finite swath writes (BASELINE config 3's stand-in file; simlod_amd/synthetic.terrain_scan is the host
 * twin).  swathWidth <= 0 or >= the tile's width: one strip, i.e. simlod_generate_terrain. */
int simlod_generate_terrain_scan(SimlodPoint* out, uint64_t numPoints, uint64_t firstIndex, uint64_t pointsPerTile, uint32_t seed,
                                 uint32_t tilesX, const float tileExtent[3], float swathWidth, void* stream);

/* ---- octree export / import (no counterpart in the reference) --------------------------------------------------------------
 * A pointer-free, self-describing form of the octree, for saving it, handing a LOD cut to other code, and rendering it in another process.
 *
 * The table lists nodes breadth-first from the root (entry 0): within a level in their parents' order, children in octant order
 * (k = x << 2 | y << 1 | z).  It does not depend on where the builder put each node, so two builds of one input give one table.  The
 * samples of a node follow its chunk list (chunk 0 first); sample order inside the list and voxel colours are as scheduling-dependent as
 * the image itself.  A node's samples are its points if it is a leaf of the SOURCE octree, else its voxels: the lists kernel_render draws. */
typedef struct SimlodExportNode {
	uint32_t level, X, Y, Z;      /* as Node                                                                                     */
	uint32_t parent;              /* table index; 0xffffffff for the root                                                        */
	uint32_t firstChild;          /* table index of the first LISTED child (listed children are consecutive, in octant order); 0xffffffff: none */
	uint8_t  childMask;           /* bit k: the child in octant k is listed                                                      */
	uint8_t  flags;               /* SIMLOD_EXPORT_FLAG_*                                                                        */
	uint16_t reserved;            /* 0                                                                                           */
	uint32_t numSamples;          /* samples of this node in the sample array (0 if not selected)                                */
	uint64_t firstSample;         /* exclusive scan of numSamples in table order                                                 */
} SimlodExportNode;
typedef struct SimlodExportCounts {   /* written by the device */
	uint32_t numNodes;            /* table entries written                                                                       */
	uint32_t error;               /* SIMLOD_EXPORT_ERR_* bits; nonzero: the table / samples are incomplete                      */
	uint64_t numSamples;          /* samples written                                                                             */
} SimlodExportCounts;
SIMLOD_STATIC_ASSERT(sizeof(SimlodExportNode) == 40, "ExportNode");
SIMLOD_STATIC_ASSERT(offsetof(SimlodExportNode, parent) == 16, "ExportNode.parent");
SIMLOD_STATIC_ASSERT(offsetof(SimlodExportNode, firstChild) == 20, "ExportNode.firstChild");
SIMLOD_STATIC_ASSERT(offsetof(SimlodExportNode, childMask) == 24, "ExportNode.childMask");
SIMLOD_STATIC_ASSERT(offsetof(SimlodExportNode, flags) == 25, "ExportNode.flags");
SIMLOD_STATIC_ASSERT(offsetof(SimlodExportNode, reserved) == 26, "ExportNode.reserved");
SIMLOD_STATIC_ASSERT(offsetof(SimlodExportNode, numSamples) == 28, "ExportNode.numSamples");
SIMLOD_STATIC_ASSERT(offsetof(SimlodExportNode, firstSample) == 32, "ExportNode.firstSample");
SIMLOD_STATIC_ASSERT(sizeof(SimlodExportCounts) == 16, "ExportCounts");
SIMLOD_STATIC_ASSERT(offsetof(SimlodExportCounts, numSamples) == 8, "ExportCounts.numSamples");

#define SIMLOD_EXPORT_NONE         0xffffffffu
#define SIMLOD_EXPORT_FLAG_LEAF    0x01u   /* a leaf of the source octree: its samples are points, else voxels */
#define SIMLOD_EXPORT_FLAG_SELECTED 0x02u  /* the node's samples are in the sample array */
/* `select` */
#define SIMLOD_EXPORT_ALL          0u      /* every listed node */
#define SIMLOD_EXPORT_CUT          1u      /* the leaves of the truncated table: source leaves with level <= maxLevel and inner nodes at maxLevel */
#define SIMLOD_EXPORT_VISIBLE      2u      /* the nodes the last kernel_render on this node array drew (render.cu:905-935, from Node.visible / isLarge) */
/* SimlodExportCounts.error bits */
#define SIMLOD_EXPORT_ERR_CAPACITY   0x1u  /* tableCapacity or sampleCapacity too small: nothing was written beyond either */
#define SIMLOD_EXPORT_ERR_NODE_COUNT 0x2u  /* the nodes reached from the root are not Stats.numNodes (or a child pointer leaves the node array) */
#define SIMLOD_EXPORT_ERR_SHORT_LIST 0x4u  /* a chunk list ends before its count */
/* Stats.dbg bit of simlod_import_octree: the table failed validation; nothing was written but this bit */
#define SIMLOD_ERR_IMPORT 0x400u

/* Bytes of the `scratch` buffer export and import need for tables of up to nodeCapacity entries and up to sampleCapacity samples. */
uint64_t simlod_export_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleCapacity);

/* Writes the table (nodes with level <= maxLevel; 20 or more: every node) and the selected samples of the octree in `nodes` / Stats.
 * Stats.numNodes and Stats.numPoints + Stats.numVoxels bound every selection: size `table` and `samples` from them.  The real counts go to
 * `counts` (device).  SIMLOD_EXPORT_VISIBLE without a kernel_render on `nodes` since its last reset, construct or import: hipErrorInvalidValue,
 * nothing enqueued.  While the builder's chunk table for `nodes` is valid the first chunks of each list come from it; the rest by `next`. */
int simlod_export_octree(const SimlodNode* nodes, const SimlodStats* stats, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                         SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity, SimlodExportCounts* counts,
                         void* stream);

/* Writes a renderable octree from a table (e.g. a loaded file): fresh chunks from byte 16 of `persistent` (the allocator header at byte 0
 * made consistent), Node records (children from firstChild / childMask, level, X/Y/Z, name, counts, list heads, grid = NULL; a table node
 * without listed children becomes a leaf and its samples its points) and the Stats counts (numNodes, numInner, numLeaves, numNonemptyLeaves,
 * numPoints, numVoxels, numChunksPoints, numChunksVoxels, allocatedBytes_persistent; the other fields 0).  numNodes above the context's node
 * capacity, or 0: hipErrorInvalidValue, nothing enqueued.  A validation kernel runs first (levels and coordinates against the parent,
 * breadth-first order, child and sample ranges, the scan, the persistent bytes the chunks need against persistentCapacity): if anything
 * fails it sets SIMLOD_ERR_IMPORT in Stats.dbg and nothing else is written.  The builder's chunk table for `nodes` is dropped, as
 * simlod_octree_image_replaced does.  An imported octree is for rendering: until kernel_reset runs on `nodes`, kernel_construct and the colour
 * filter return hipErrorInvalidValue for it and enqueue nothing. */
int simlod_import_octree(const SimlodExportNode* table, uint32_t numNodes, const SimlodPoint* samples, uint64_t numSamples, void* scratch,
                         uint64_t scratchBytes, uint8_t* persistent, uint64_t persistentCapacity, SimlodNode* nodes, SimlodStats* stats, void* stream);

/* Stats.dbg bit of simlod_import_octree_buildable: a rebuilt occupancy grid disagrees with the table (a non-root inner node's popcount is
 * not its numSamples, or the root's exceeds its numSamples) — the uniforms' box is not the one the octree was built with.  FATAL: sticky
 * until kernel_reset; kernel_construct launches do nothing while it is set.  The octree still renders. */
#define SIMLOD_ERR_IMPORT_GRID 0x800u

/* The "buildable" import: everything simlod_import_octree writes, plus what kernel_construct needs to go on ingesting into the octree —
 * the occupancy grid of every inner node and of the root, rebuilt from the samples (the grid of a node is the set of its level's cells of
 * every point below it: the leaves' samples), and a builder state as after a reset (batchletIndex, numPointsProcessed 0; the recycle stack
 * empty: numAllocatedChunks = chunkPoolSize = the point chunks in use).  `uniforms` give the box (boxMin / boxMax, which must be the box the octree was
 * built with), persistentBufferCapacity and frameCounter.  The upload counter and batchSizes are zeroed in stream order, as kernel_reset
 * does, and the next kernel_construct launch is sized as after a reset.
 * Only full exports qualify: besides simlod_import_octree's checks the validation kernel requires every entry SELECTED, FLAG_LEAF set
 * exactly when childMask == 0, childMask 0 or 0xff, and the chunks, the grids (SIMLOD_ALLOC_ROUND(sizeof(SimlodOccupancyGrid)) each) and,
 * for a root that is still a leaf, room for its voxel list (one chunk per 1 000 of its points) within persistentBufferCapacity; a failure
 * sets SIMLOD_ERR_IMPORT and writes nothing else.  A root that is still a leaf gets its voxels back (the export carries its points only):
 * one per occupied cell of its grid, in ascending cell order, at the cell centre, coloured by the cell's lowest-index point.
 * The scratch bound is simlod_export_buffer_min_bytes(numNodes, numSamples). */
int simlod_import_octree_buildable(const SimlodUniforms* uniforms, const SimlodExportNode* table, uint32_t numNodes, const SimlodPoint* samples,
                                   uint64_t numSamples, void* scratch, uint64_t scratchBytes, uint8_t* persistent, SimlodNode* nodes,
                                   SimlodStats* stats, uint32_t* numBatchesUploaded, uint32_t* batchSizes, void* stream);

/* ---- region queries: the samples inside a convex region at a chosen level of detail ---------------------------------------------------
 * simlod_query_region writes what simlod_export_octree writes — a breadth-first table and a sample array — restricted to the intersection of
 * up to 16 half-spaces.  The result is an ordinary table: it validates, saves, and imports render-only (a crop).  The source is only read.
 *
 * The box is the builder's: min = uniforms.boxMin, size = the largest extent (fmaxf of the fp32 differences boxMax - boxMin).  All geometry is
 * fp64 computed from the fp32 inputs without fused multiply-add, every sum in the order written here.
 *  1. Listed nodes.  Entry 0 is the root.  A node below it is listed iff its parent is listed, its level is <= maxLevel and it is not OUTSIDE.
 *     With s = size / 2^level, e = size * 2^-20, lo_a = (min_a + A * s) - e and hi_a = (min_a + (A + 1) * s) + e for the node's coordinate A on
 *     axis a, a node is outside iff D_max = ((nx*fx + ny*fy) + nz*fz) + d < 0 for some plane, f_a = n_a >= 0 ? hi_a : lo_a (the corner farthest
 *     along the normal).  The inflation by e (one level-20 cell) covers the fp32 rounding of the builder's quantisation, which can file a point
 *     up to about size * 2^-22 beyond the exact face of its node.  childMask / firstChild / parent describe the listed nodes only.
 *  2. Selected nodes among the listed: SIMLOD_EXPORT_ALL every one, SIMLOD_EXPORT_CUT the source leaves and the nodes at maxLevel.  FLAG_LEAF
 *     keeps its meaning (a leaf of the source octree).  A root that is outside is listed and contributes no samples.
 *  3. A selected node that is not outside contributes those of its samples with ((nx*x + ny*y) + nz*z) + d >= 0 for every plane (a NaN fails),
 *     in chunk-list order with the failing ones removed.  numSamples / firstSample are the counts after filtering and their scan.
 *  4. Such a node is COPIED without a per-sample test iff D_min >= 0 for every plane (the nearest corner of the same inflated cube:
 *     f_a = n_a >= 0 ? lo_a : hi_a); else it is FILTERED.  For finite samples in the half-open box min <= p < min + size neither the culling nor
 *     the shortcut changes the result.  OUTSIDE THE CONTRACT: samples outside that box, on its max faces, or with non-finite coordinates.  The
 *     builder does not keep them in the node whose cube holds them (a point with x == min + size is stored under nodes with X = 0); such a sample
 *     is returned iff the node it is stored in is copied, or is filtered and the sample passes the test.
 *  5. samples == NULL: count only — the table and the counts are complete and nothing else is written (sampleCapacity is ignored).  Otherwise
 *     a tableCapacity or sampleCapacity that is too small sets SIMLOD_EXPORT_ERR_CAPACITY and nothing is written beyond either.  Stats.numNodes
 *     and Stats.numPoints + Stats.numVoxels bound every result.
 *  6. With zero planes the result equals simlod_export_octree(maxLevel, select) byte for byte and every node with samples is copied. */
#define SIMLOD_REGION_MAX_PLANES 16u
typedef struct SimlodRegion {          /* host memory, read before the call returns */
	uint32_t numPlanes;                /* 0..16; 0: the whole space */
	uint32_t reserved[3];              /* 0 */
	float    planes[SIMLOD_REGION_MAX_PLANES][4];   /* (nx, ny, nz, d): a point is inside iff nx*x + ny*y + nz*z + d >= 0 for every plane */
} SimlodRegion;
typedef struct SimlodQueryCounts {     /* written by the device */
	uint32_t numNodes;                 /* table entries written                                                                  */
	uint32_t error;                    /* SIMLOD_EXPORT_ERR_* bits                                                               */
	uint64_t numSamples;               /* samples that passed (= written, unless count-only or a capacity error)                 */
	uint64_t numCandidates;            /* samples of the selected, listed nodes that are not outside, before the test            */
	uint32_t numFilteredNodes;         /* such nodes (with at least one sample) whose samples were tested one by one             */
	uint32_t numCopiedNodes;           /* such nodes (with at least one sample) that were copied without a test                  */
} SimlodQueryCounts;
SIMLOD_STATIC_ASSERT(sizeof(SimlodRegion) == 272, "Region");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRegion, planes) == 16, "Region.planes");
SIMLOD_STATIC_ASSERT(sizeof(SimlodQueryCounts) == 32, "QueryCounts");
SIMLOD_STATIC_ASSERT(offsetof(SimlodQueryCounts, numSamples) == 8, "QueryCounts.numSamples");
SIMLOD_STATIC_ASSERT(offsetof(SimlodQueryCounts, numCandidates) == 16, "QueryCounts.numCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodQueryCounts, numFilteredNodes) == 24, "QueryCounts.numFilteredNodes");
SIMLOD_STATIC_ASSERT(offsetof(SimlodQueryCounts, numCopiedNodes) == 28, "QueryCounts.numCopiedNodes");

/* Bytes of the `scratch` buffer a query needs for a table of up to nodeCapacity entries whose selected nodes hold up to sampleBound samples
 * BEFORE the test (Stats.numPoints + Stats.numVoxels always suffices): one 32-byte item per 1 000-sample chunk.  A buffer that holds the
 * table's part but too few items makes the query report SIMLOD_EXPORT_ERR_CAPACITY. */
uint64_t simlod_query_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound);

/* The region query (rules above).  Asynchronous on `stream`; everything in between lives in `scratch`.  hipErrorInvalidValue with nothing
 * enqueued: a null pointer other than `samples`, numPlanes > 16, a non-finite coefficient, nonzero `reserved`, `select` other than
 * SIMLOD_EXPORT_ALL / SIMLOD_EXPORT_CUT, scratchBytes below simlod_query_buffer_min_bytes(tableCapacity, 0).  While the builder's chunk table
 * for `nodes` is valid the first chunks of each list come from it, the rest by `next` (as simlod_export_octree). */
int simlod_query_region(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                        uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity,
                        SimlodPoint* samples, uint64_t sampleCapacity, SimlodQueryCounts* counts, void* stream);

/* ---- clip regions: a frame that shows the inside of a region, cuts it away, or highlights it ---------------------------------------------
 * A clip is a SimlodRegion, a mode and a colour, kept by the context and honoured by every frame entry point (simlod_launch_render,
 * simlod_launch_render_part, simlod_render_frame_composed, simlod_render_frame_rccl).  Nothing is copied: the frame's own kernels decide per
 * node and per sample.  It is read when a frame (or a part of one) is enqueued and travels as a kernel argument, so frames already enqueued
 * keep theirs.  The setter does no device work.
 *
 * The box and all arithmetic are the region section's: min = uniforms.boxMin, size = the largest fp32 extent; fp64 from the fp32 inputs, no
 * fused multiply-add, every sum in the order written there.
 *  C1. A sample PASSES iff it passes region rule 3: ((nx*x + ny*y) + nz*z) + d >= 0 for every plane (a NaN fails).
 *  C2. A node's class is OUTSIDE, COPIED or FILTERED exactly as region rules 1 and 4 say (the cube inflated by one level-20 cell), for
 *      each node on its own from (level, X, Y, Z) — not through its parent.
 *  C3. A clipped frame is the frame kernel_render draws, with the same uniforms, of the same octree image after this edit:
 *          mode                        OUTSIDE node   COPIED node                        FILTERED node
 *          SIMLOD_CLIP_INSIDE          emptied        as it is                           failing samples removed
 *          SIMLOD_CLIP_OUTSIDE         as it is       emptied                            passing samples removed
 *          SIMLOD_CLIP_HIGHLIGHT       as it is       every sample's colour := color     passing samples' colour := color
 *      EMPTIED: numPoints = numVoxels = 0.  By render.cu:760-861 such a node is not visible: not listed, not drawn, no bounding-box lines,
 *      not counted in Stats; Node.visible is written as 0 in the node array too, so SIMLOD_EXPORT_VISIBLE follows the clip.  Other nodes
 *      decide as before (emission depends on the node's own flags and its parent's geometry only).
 *      REMOVED: the sample draws nothing.  The node's counts stay: numVisiblePoints / numVisibleVoxels count whole nodes, as the reference
 *      does for samples off screen.  Points and voxels are samples alike.
 *  C4. Uniforms.colorByNode / colorByLOD win over HIGHLIGHT: with either set a HIGHLIGHT frame is the unclipped frame.
 *  C5. Zero planes: every node with samples is COPIED — INSIDE is the unclipped frame, OUTSIDE a clear frame without a visible node.
 *  C6. The clip is geometry of the world: it applies whether or not transform_updateBound differs from transform.
 *  OUTSIDE THE CONTRACT, as in region rule 4: samples outside the half-open box, on its max faces, or non-finite. */
#define SIMLOD_CLIP_OFF       0u
#define SIMLOD_CLIP_INSIDE    1u
#define SIMLOD_CLIP_OUTSIDE   2u       /* cut-away */
#define SIMLOD_CLIP_HIGHLIGHT 3u
typedef struct SimlodClip {            /* host memory, read before the call returns */
	uint32_t     mode;                 /* SIMLOD_CLIP_* */
	uint32_t     color;                /* HIGHLIGHT: the colour word (as Point.color) */
	uint32_t     reserved[2];          /* 0 */
	SimlodRegion region;
} SimlodClip;
SIMLOD_STATIC_ASSERT(sizeof(SimlodClip) == 288, "Clip");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClip, region) == 16, "Clip.region");
/* Sets the clip of `ctx` (NULL: the default context) for the frames enqueued from now on; clip == NULL or mode SIMLOD_CLIP_OFF: no clip.
 * hipErrorInvalidValue, the context's clip left as it was: a mode above 3, numPlanes > 16, a non-finite coefficient, nonzero `reserved` in
 * either struct. */
int simlod_context_set_clip(SimlodContext* ctx, const SimlodClip* clip);
int simlod_set_clip(const SimlodClip* clip);   /* the default context */

/* ---- footprint queries: the samples inside an extruded polygon at a chosen level of detail ------------------------------------------------
 * simlod_query_footprint is simlod_query_region plus a footprint: a polygon of up to 256 vertices in a plane the points are mapped into by an
 * affine map, extruded along the map's null direction (a parcel, a building outline, a lasso drawn in an orthographic view).  The polygon need
 * not be convex.  Everything the region section says stays in force: the box, the inflated cube lo_a / hi_a of rule 1, the listing and
 * selection rules, rule 5's count-only calls and capacities, SimlodQueryCounts, SIMLOD_EXPORT_REGION, the chunk-table / `next` sources.  The
 * footprint composes with the region's half-spaces (polygon, height band and frustum in one call), and the result is an ordinary table.
 * An affine map covers plan-view outlines and any orthographic view; a polygon on the screen of a perspective camera (u = x_clip / w) is a
 * lasso: see "lasso queries" below.
 *
 * All new geometry is fp64 computed from the fp32 inputs without fused multiply-add, every sum in the order written here; there is no division.
 *  F1. Sample rule.  u = ((ux*x + uy*y) + uz*z) + u0 and v likewise from axisU / axisV.  For each edge i from a = P[i] to b = P[(i+1) mod n]:
 *      du = b_u - a_u, dv = b_v - a_v, c = du*(v - a_v) - dv*(u - a_u); the edge is crossed iff (a_v > v) != (b_v > v) and (c > 0) == (dv > 0).
 *      The sample passes the footprint iff the number of crossed edges is odd (the even-odd rule: self-intersecting polygons are defined; a
 *      polygon of zero area passes nothing off its own line; a NaN coordinate passes nothing).  A sample exactly on an edge's line (c == 0)
 *      crosses that edge iff it runs towards smaller v: a rectangle (lo, lo), (lo, hi), (hi, hi), (hi, lo) passes lo <= u <= hi, lo <= v < hi.
 *      A sample passes the query iff it passes F1 and region rule 3.
 *  F2. Projected rectangle of a node.  U_lo = ((ux*fx + uy*fy) + uz*fz) + u0 with f_a = u_a >= 0 ? lo_a : hi_a; U_hi from the opposite corner;
 *      V_lo, V_hi likewise (the corner selection of region rules 1 and 4).  fp64 rounding is monotone, so the computed (u, v) of every sample
 *      inside the inflated cube lies in the rectangle, in floating point and not only in exact arithmetic.
 *  F3. Far edges.  Edge i is FAR from a node iff max(a_v, b_v) < V_lo, or min(a_v, b_v) > V_hi, or c(U_lo,V_lo), c(U_lo,V_hi), c(U_hi,V_lo),
 *      c(U_hi,V_hi) are all > 0 or all < 0 (c is monotone in u and in v: the sign then holds for every sample of the node).  Any other edge
 *      is NEAR.
 *  F4. Node class by the footprint.  A node with a NEAR edge is FILTERED.  A node without one takes rule F1's verdict at (U_lo, V_lo): COPIED
 *      if that point passes, else OUTSIDE.  The final class: OUTSIDE if outside by the planes or by the footprint, COPIED iff copied by both,
 *      else FILTERED.  Each node is classified on its own; outside nodes are not listed, copied nodes contribute every sample without a test.
 *  F5. For finite samples in the half-open box F3 / F4 change nothing against F1 applied to every sample — provided no corner value lies within
 *      fp64 rounding of zero with the wrong exact sign (an edge's line grazing a node's corner).  The host mirror asserts this per query.
 *  F6. footprint == NULL gives exactly simlod_query_region, byte for byte.  `region` is required and may have zero planes.
 *  F7. hipErrorInvalidValue with nothing enqueued: everything simlod_query_region refuses, numVertices outside 3..256, a non-finite vertex or
 *      axis coefficient, nonzero `reserved`, scratchBytes below simlod_footprint_buffer_min_bytes(tableCapacity, 0). */
#define SIMLOD_FOOTPRINT_MAX_VERTICES 256u
typedef struct SimlodFootprint {       /* host memory, read before the call returns */
	uint32_t numVertices;              /* 3..256; the polygon closes from the last vertex to the first */
	uint32_t reserved[3];              /* 0 */
	float    axisU[4], axisV[4];       /* u = ((ux*x + uy*y) + uz*z) + u0, v likewise: an affine map of the point into the polygon's plane */
	float    vertices[SIMLOD_FOOTPRINT_MAX_VERTICES][2];   /* (u, v) */
} SimlodFootprint;
SIMLOD_STATIC_ASSERT(sizeof(SimlodFootprint) == 2096, "Footprint");
SIMLOD_STATIC_ASSERT(offsetof(SimlodFootprint, axisU) == 16, "Footprint.axisU");
SIMLOD_STATIC_ASSERT(offsetof(SimlodFootprint, axisV) == 32, "Footprint.axisV");
SIMLOD_STATIC_ASSERT(offsetof(SimlodFootprint, vertices) == 48, "Footprint.vertices");

/* simlod_query_buffer_min_bytes plus a fixed block for the polygon widened to fp64 (8 KB). */
uint64_t simlod_footprint_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound);

/* The footprint query (rules above; arguments as simlod_query_region's).  Asynchronous on `stream` once `footprint` has been read. */
int simlod_query_footprint(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                           const SimlodFootprint* footprint, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                           SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity,
                           SimlodQueryCounts* counts, void* stream);

/* ---- profile queries: the samples in a corridor along a polyline, each with its station, offset and height ---------------------------------
 * simlod_query_profile is simlod_query_region plus a profile: a polyline of up to 64 vertices in a plane the points are mapped into by an affine
 * map (as a footprint's), and a half-width.  The result is the samples within the half-width of a segment, at the chosen level of detail, and
 * for each of them a SimlodProfileSample: the segment it belongs to, its distance along the polyline, its signed distance from the segment's
 * line and its height — a road's, a river bank's or a power line's cross-section.  Everything the region section says stays in force: the box,
 * the inflated cube lo_a / hi_a of rule 1, the listing and selection rules, rule 5's count-only calls and capacities, SimlodQueryCounts,
 * SIMLOD_EXPORT_REGION, the chunk-table / `next` sources.  The profile composes with the region's half-spaces (a height band, say), and the
 * table and `samples` are an ordinary export table; records[k] belongs to samples[k].
 * THE CORRIDOR is the union of one rectangle per segment, with square ends (as Potree's height profile).  On the outside of a bend the wedge
 * between two rectangles belongs to no segment: a sample there is not returned.  On the inside the rectangles overlap: the lower segment owns.
 *
 * All new geometry is fp64 computed from the fp32 inputs without fused multiply-add, every sum in the order written here.  The device neither
 * divides nor takes a square root.
 *  P0. Segments.  Segment i runs from a = P[i] to b = P[i+1]: du = b_u - a_u, dv = b_v - a_v, L2 = du*du + dv*dv, W2 = (w*w)*L2 with
 *      w = halfWidth.  The launcher computes, on the host, len = sqrt(L2), inv = 1.0/len, s0_0 = 0 and s0_(i+1) = s0_i + len_i, and places
 *      {a_u, a_v, du, dv, L2, W2, inv, s0} (64 bytes per segment) in a block of the scratch buffer.  A segment with L2 == 0 is refused.
 *  P1. Sample rule.  u and v as footprint rule F1.  For segment i: pu = u - a_u, pv = v - a_v, al = du*pu + dv*pv, c = du*pv - dv*pu.  The sample
 *      is IN segment i iff al >= 0 && al <= L2 && c*c <= W2 (a NaN fails).  It passes iff it passes region rule 3 and is in some segment; ITS
 *      segment is the lowest such i.
 *  P2. Record.  station = (float)(s0_i + al*inv_i), offset = (float)(c*inv_i) (positive to the left of the direction of travel),
 *      height = (float)(((hx*x + hy*y) + hz*z) + h0) from axisH, segment = i.
 *  P3. Node class by the profile.  With the projected rectangle [U_lo, U_hi] x [V_lo, V_hi] of footprint rule F2: per segment al and c at the
 *      four corners (U_lo,V_lo), (U_lo,V_hi), (U_hi,V_lo), (U_hi,V_hi), as al = du*(U - a_u) + dv*(V - a_v) and c = du*(V - a_v) - dv*(U - a_u),
 *      and their minima and maxima al_min, al_max, c_min, c_max.  The segment is FAR iff al_max < 0 || al_min > L2 ||
 *      (c_min > 0 && c_min*c_min > W2) || (c_max < 0 && c_max*c_max > W2).  It COVERS the node iff al_min >= 0 && al_max <= L2 &&
 *      c_min*c_min <= W2 && c_max*c_max <= W2.  The node is OUTSIDE iff every segment is FAR, COPIED iff some segment covers it, else FILTERED.
 *      The final class combines with the planes' as footprint rule F4 does: OUTSIDE if outside by either, COPIED iff copied by both, else
 *      FILTERED.  A COPIED node's samples all pass without a test and are not counted one by one; each still gets its record, with the lowest
 *      segment it is in (which need not be the one that covers the node).
 *  P4. al and c as computed are monotone in u and in v (every product and every sum is), so they take their extremes at the corners in floating
 *      point too: for finite samples in the half-open box P3 changes nothing against P1 applied to every sample, without a grazing exception.
 *      The host mirror asserts this per query.  A sample OUTSIDE that contract in a COPIED node is returned as every sample of such a node is;
 *      if it is in no segment its record has station = offset = 0 and segment = SIMLOD_PROFILE_NO_SEGMENT.
 *  P5. profile == NULL gives exactly simlod_query_region, byte for byte, and `records` is not written.  records == NULL with samples != NULL
 *      gives the crop by the corridor without records.  records != NULL with samples == NULL is refused.  `records` has room for
 *      sampleCapacity records and is 16-byte aligned.
 *  P6. hipErrorInvalidValue with nothing enqueued: everything simlod_query_region refuses, numVertices outside 2..64, halfWidth not finite or
 *      <= 0, a non-finite vertex or axis coefficient, a segment of length zero, nonzero `reserved`, records without samples, scratchBytes below
 *      simlod_profile_buffer_min_bytes(tableCapacity, 0).  Neither capacity error writes anything past the capacity. */
#define SIMLOD_PROFILE_MAX_VERTICES 64u
#define SIMLOD_PROFILE_NO_SEGMENT   0xffffffffu
typedef struct SimlodProfile {         /* host memory, read before the call returns */
	uint32_t numVertices;              /* 2..64: numVertices - 1 segments */
	float    halfWidth;                /* > 0, finite: the corridor reaches this far to either side of a segment */
	uint32_t reserved[2];              /* 0 */
	float    axisU[4], axisV[4];       /* the plan coordinates, as SimlodFootprint's */
	float    axisH[4];                 /* the reported height h = ((hx*x + hy*y) + hz*z) + h0 */
	float    vertices[SIMLOD_PROFILE_MAX_VERTICES][2];   /* (u, v) */
} SimlodProfile;
typedef struct SimlodProfileSample {   /* written by the device, one per returned sample, same index as the sample */
	float    station;                  /* distance along the polyline from vertex 0 */
	float    offset;                   /* signed distance from the segment's line, positive to the left of the direction of travel */
	float    height;
	uint32_t segment;
} SimlodProfileSample;
SIMLOD_STATIC_ASSERT(sizeof(SimlodProfile) == 576, "Profile");
SIMLOD_STATIC_ASSERT(offsetof(SimlodProfile, halfWidth) == 4, "Profile.halfWidth");
SIMLOD_STATIC_ASSERT(offsetof(SimlodProfile, axisU) == 16, "Profile.axisU");
SIMLOD_STATIC_ASSERT(offsetof(SimlodProfile, axisV) == 32, "Profile.axisV");
SIMLOD_STATIC_ASSERT(offsetof(SimlodProfile, axisH) == 48, "Profile.axisH");
SIMLOD_STATIC_ASSERT(offsetof(SimlodProfile, vertices) == 64, "Profile.vertices");
SIMLOD_STATIC_ASSERT(sizeof(SimlodProfileSample) == 16, "ProfileSample");
SIMLOD_STATIC_ASSERT(offsetof(SimlodProfileSample, height) == 8, "ProfileSample.height");
SIMLOD_STATIC_ASSERT(offsetof(SimlodProfileSample, segment) == 12, "ProfileSample.segment");

/* simlod_query_buffer_min_bytes plus a fixed block for the segments (4 KB). */
uint64_t simlod_profile_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound);

/* The profile query (rules above; arguments as simlod_query_footprint's, plus `records`).  Asynchronous on `stream` once `profile` has been read. */
int simlod_query_profile(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                         const SimlodProfile* profile, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                         SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity,
                         SimlodProfileSample* records, SimlodQueryCounts* counts, void* stream);

/* ---- paint regions: recolour the samples inside a region in place, with undo ------------------------------------------------------------------
 * simlod_paint_region writes a colour into the octree itself, for the samples a footprint query selects: "select, then mark".  What
 * SIMLOD_CLIP_HIGHLIGHT shows for one region and one frame becomes part of the octree: every later frame, export, query, packed result and
 * saved file carries it.  It is the one call besides ingest and import that writes the octree, and it writes colour words only.
 *
 * Everything the region and the footprint section say stays in force: the box, the classes of a node, rules 3 and F1 per sample, the
 * chunk-table / `next` sources.
 *  E0. Target set and order.  The painted samples are exactly the samples, in the order, that simlod_query_footprint(region, footprint,
 *      maxLevel = 20, SIMLOD_EXPORT_ALL) returns on the same octree (footprint == NULL: simlod_query_region): every level, points and voxels
 *      alike; a COPIED node is painted whole without a test, a FILTERED node sample by sample.  `table` and `counts` come back as that query's
 *      count-only call writes them; counts.numSamples is the number painted.  Sample j of that order is "sample j" below.
 *  E1. SIMLOD_PAINT_SET.  The whole colour word becomes `color`.
 *  E2. SIMLOD_PAINT_BLEND.  For each of the bytes 0..2: c' = (c*(256 - a) + t*a + 128) >> 8 in integers, c the sample's byte, t that byte of
 *      `color`, a = strength in 1..255.  Byte 3 is kept.
 *  E3. SIMLOD_PAINT_RAMP.  t = ((double)z - (double)z0) * (double)scale from the sample's fp32 z, without fused multiply-add; i = 255 if
 *      t >= 255, (uint32_t)t if t > 0, else 0 (a NaN gives 0); the whole colour word becomes table[i].  `scale` is finite and > 0.
 *  E4. SIMLOD_PAINT_ARRAY and `previous`.  Sample j gets colors[j].  In every mode, with previous != NULL, the colour word sample j had before
 *      the call goes to previous[j] (each sample is read before it is written, and by nothing else).  The set and the order depend on positions
 *      only, and paint never changes a position: `previous` of one call, passed as `colors` to an ARRAY call with the same region and
 *      footprint, restores the octree byte for byte.  `colors` and `previous` are DEVICE memory of colorCapacity words each and do not overlap.
 *  E5. All or nothing.  When counts.numSamples > colorCapacity while `colors` or `previous` is given, SIMLOD_EXPORT_ERR_CAPACITY is set in
 *      counts.error; then, and with any other error bit of the query (a tableCapacity or scratch buffer too small: SIMLOD_EXPORT_ERR_CAPACITY;
 *      a broken list), no colour and no word of `previous` is written.  colorCapacity is ignored when both arrays are NULL.
 *  E6. Nothing else changes: positions and sample order, chunk headers, Node records, Stats, the occupancy grids, the allocator header and the
 *      frame state stay as they are, and the builder's chunk table stays valid (no simlod_octree_image_replaced).  An imported octree,
 *      render-only or buildable, is painted like a built one.
 *  E7. Later ingest.  A painted point keeps its colour through leaf splits (a split moves the 16 bytes).  A voxel created later takes its colour
 *      from its points, as before, painted or not; a painted voxel keeps its colour.  simlod_launch_colorfilter, run afterwards, averages
 *      whatever colours it finds: no claim is made about its result.
 *  E8. Not carried.  A receiver's held cut does not learn of a paint: simlod_query_view_delta compares counts, so a painted node that is KEPT is
 *      not sent again.  The multi-GPU layer has no paint call; each rank may paint its own octree.
 *  E9. hipErrorInvalidValue with nothing enqueued: everything simlod_query_footprint refuses (with simlod_paint_buffer_min_bytes(tableCapacity, 0)
 *      as the scratch bound), paint == NULL, a mode above 3, nonzero `reserved` / `reserved2`, BLEND with strength outside 1..255, RAMP with z0 or
 *      scale not finite or scale <= 0, ARRAY with colors == NULL.  Fields a mode does not use are ignored.
 * ORDERING.  Asynchronous on `stream` once `region`, `footprint` and `paint` have been read.  The call writes the octree: no frame, query,
 * export or construct launch on the same `nodes` may overlap it. */
#define SIMLOD_PAINT_SET    0u         /* colour word := color (what SIMLOD_CLIP_HIGHLIGHT shows, made permanent) */
#define SIMLOD_PAINT_BLEND  1u         /* bytes 0..2: c' = (c*(256-a) + t*a + 128) >> 8, t = that byte of color, a = strength in 1..255; byte 3 kept */
#define SIMLOD_PAINT_RAMP   2u         /* colour word := table[i], i from the sample's z (rule E3) */
#define SIMLOD_PAINT_ARRAY  3u         /* colour word := colors[index of the sample in query order] (undo, or colours computed elsewhere) */
typedef struct SimlodPaint {           /* host memory, read before the call returns */
	uint32_t mode;                     /* SIMLOD_PAINT_* */
	uint32_t color;                    /* SET, BLEND: the colour word (as Point.color) */
	uint32_t strength;                 /* BLEND: 1..255 */
	uint32_t reserved;                 /* 0 */
	float    z0, scale;                /* RAMP: t = (z - z0) * scale */
	uint32_t reserved2[2];             /* 0 */
	uint32_t table[256];               /* RAMP: the colour words */
} SimlodPaint;
SIMLOD_STATIC_ASSERT(sizeof(SimlodPaint) == 1056, "Paint");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPaint, color) == 4, "Paint.color");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPaint, strength) == 8, "Paint.strength");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPaint, z0) == 16, "Paint.z0");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPaint, scale) == 20, "Paint.scale");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPaint, table) == 32, "Paint.table");

/* simlod_footprint_buffer_min_bytes plus a fixed block for the ramp's table (1 KB), with or without a footprint. */
uint64_t simlod_paint_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound);

/* The paint call (rules above).  `nodes`, `stats`, `uniforms`, `region`, `footprint`, `scratch`, `table` and `counts` as simlod_query_footprint's. */
int simlod_paint_region(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                        const SimlodFootprint* footprint /*or NULL*/, const SimlodPaint* paint, void* scratch, uint64_t scratchBytes,
                        SimlodExportNode* table, uint32_t tableCapacity, const uint32_t* colors /*ARRAY only*/, uint32_t* previous /*or NULL*/,
                        uint64_t colorCapacity, SimlodQueryCounts* counts, void* stream);

/* ---- summary queries: a selection's extent, histograms and moments in place ------------------------------------------------------------------
 * simlod_query_summary says something ABOUT the samples a footprint query selects without copying them out: how many there are, the box they
 * span, the sums a centroid and a covariance come from, the histogram of their heights in the bins a RAMP paint would use, and the histograms
 * of the four bytes of their colour words.  It is a read-only reduction: each selected sample is read once, one fixed-size record is written,
 * and every field of it is an integer count, an integer sum or a minimum / maximum under a total order — exact, and independent of the order
 * in which the samples are visited.
 *
 * Everything the region and the footprint section say stays in force: the box, the classes of a node, rules 3 and F1 per sample, the
 * chunk-table / `next` sources.
 *  S0. Set.  The summarised samples are exactly the samples that simlod_query_footprint(region, footprint, maxLevel, select) returns on the same
 *      octree (footprint == NULL: simlod_query_region).  Unlike paint, maxLevel and select are the caller's: the summary of one level-of-detail
 *      cut is the meaningful one.  `table` and `counts` come back as that query's count-only call writes them, byte for byte.  A COPIED node
 *      contributes every sample without a test, a FILTERED node the samples that pass.
 *  S1. Extent.  Per axis, over the samples whose coordinate on that axis is not a NaN: the minimum and the maximum under the total order of the
 *      key k(bits) = bits ^ ((bits >> 31) ? 0xffffffff : 0x80000000) of the coordinate's 32 bits, compared as unsigned integers.  Under that key
 *      -0 < +0 and the infinities take part, so the result does not depend on the order of visiting.  With no such sample min = +inf and
 *      max = -inf.
 *  S2. Moments.  Per axis a, t = ((double)x_a - (double)boxMin_a) * inv with inv = 1048576.0 / (double)size, `size` the box size of the region
 *      section; inv is one IEEE division made by the launcher on the host.  The device does not divide and uses no fused multiply-add.
 *      c20 = 1048575 if t >= 1048575.0, (uint32_t)t if t > 0.0, else 0 (a NaN gives 0); c16 = c20 >> 4.  sum[a] is the sum of c20_a; sum2 holds
 *      the sums of the six products c16_a * c16_b in the order xx, yy, zz, xy, xz, yz.  All sums are 64-bit unsigned integers: a term of `sum`
 *      is below 2^20 and a term of `sum2` below 2^32, so no sum can overflow while numSamples < 2^32; neither can a histogram's 32-bit
 *      partial count.  numSamples is bounded by Stats.numPoints + Stats.numVoxels; past 2^32 selected samples (64 GB of them) the sums and
 *      the histograms may wrap, and no error bit says so.
 *  S3. histZ.  histZ[i] counts the samples with i = rule E3's index of their z under params.z0 and params.scale: exactly the number of samples
 *      a SIMLOD_PAINT_RAMP paint of the same selection (at maxLevel = 20, SIMLOD_EXPORT_ALL) would give table[i].
 *  S4. histC.  histC[k][(color >> 8k) & 255] counts, for k = 0..3, byte k of the colour word.
 *  S5. All or nothing.  With any error bit in counts.error (a tableCapacity or scratch buffer too small: SIMLOD_EXPORT_ERR_CAPACITY; a broken
 *      list) `summary` is not written at all.
 *  S6. Nothing is written but `scratch`, `table`, `counts` and `summary`: the octree, its frame state and the builder's chunk table are
 *      untouched.  Any octree the footprint query accepts is accepted: built, imported (render-only or buildable), shifted, deep.
 *  S7. Grid independence.  The record does not depend on params.maxWorkgroups.
 *  S8. hipErrorInvalidValue with nothing enqueued: everything simlod_query_footprint refuses (with simlod_summary_buffer_min_bytes(tableCapacity, 0)
 *      as the scratch bound), params == NULL, summary == NULL, z0 or scale not finite, scale <= 0, nonzero `reserved`, `summary` not 8-byte
 *      aligned.
 * numNonFinite counts the samples with a NaN or an infinity in x, y or z.  Asynchronous on `stream` once `region`, `footprint` and `params`
 * have been read; `summary` is DEVICE memory. */
typedef struct SimlodSummaryParams {   /* host memory, read before the call returns */
	float    z0, scale;                /* the z histogram's bins: rule E3's index of (z, z0, scale) */
	uint32_t maxWorkgroups;            /* 0: the library's choice; else the reduction launches at most this many workgroups */
	uint32_t reserved;                 /* 0 */
} SimlodSummaryParams;
typedef struct SimlodSummary {         /* written by the device */
	uint64_t numSamples;               /* == counts.numSamples */
	uint64_t numNonFinite;             /* samples with a NaN or an infinity in x, y or z */
	float    min[3], max[3];           /* rule S1 */
	uint64_t sum[3];                   /* rule S2: sum of c20 per axis */
	uint64_t sum2[6];                  /* rule S2: sum of c16_a * c16_b for xx, yy, zz, xy, xz, yz */
	uint64_t histZ[256];               /* rule S3 */
	uint64_t histC[4][256];            /* rule S4: byte k of the colour word */
} SimlodSummary;
SIMLOD_STATIC_ASSERT(sizeof(SimlodSummaryParams) == 16, "SummaryParams");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummaryParams, scale) == 4, "SummaryParams.scale");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummaryParams, maxWorkgroups) == 8, "SummaryParams.maxWorkgroups");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummaryParams, reserved) == 12, "SummaryParams.reserved");
SIMLOD_STATIC_ASSERT(sizeof(SimlodSummary) == 10352, "Summary");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummary, numNonFinite) == 8, "Summary.numNonFinite");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummary, min) == 16, "Summary.min");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummary, max) == 28, "Summary.max");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummary, sum) == 40, "Summary.sum");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummary, sum2) == 64, "Summary.sum2");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummary, histZ) == 112, "Summary.histZ");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSummary, histC) == 2160, "Summary.histC");

/* simlod_footprint_buffer_min_bytes plus the partial records of the largest grid the library ever chooses (about 5 MB), with or without a
 * footprint; params.maxWorkgroups only lowers the grid. */
uint64_t simlod_summary_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound);

/* The summary query (rules above).  `nodes`, `stats`, `uniforms`, `region`, `footprint`, `maxLevel`, `select`, `scratch`, `table` and `counts`
 * as simlod_query_footprint's. */
int simlod_query_summary(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                         const SimlodFootprint* footprint /*or NULL*/, const SimlodSummaryParams* params, uint32_t maxLevel, uint32_t select,
                         void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, SimlodSummary* summary /*device*/,
                         SimlodQueryCounts* counts, void* stream);

/* ---- lasso queries: select, paint and summarise by a polygon on the screen of a perspective camera ---------------------------------------------
 * simlod_query_lasso is simlod_query_region plus a lasso: a polygon of up to 256 vertices on a screen the points are mapped onto by a PROJECTIVE
 * map — three rows U, V, W of a 4 x 4 matrix, the screen position being (U/W, V/W) where W > 0 (in front of the eye).  It is the selection a user
 * draws with the mouse in a 3-D view; simlod_paint_lasso and simlod_query_summary_lasso are "select, then mark" and "what is this selection" for
 * it.  The polygon need not be convex.  Everything the region section says stays in force: the box, the inflated cube lo_a / hi_a of rule 1, the
 * listing and selection rules, rule 5's count-only calls and capacities, SimlodQueryCounts, SIMLOD_EXPORT_REGION, the chunk-table / `next`
 * sources.  The lasso composes with the region's half-spaces (a frustum, a height slab), and the result is an ordinary table.
 * NOT COVERED: a lasso on profile queries, clip regions, view queries and deltas; a lasso and a footprint in one call.
 *
 * All new geometry is fp64 computed from the fp32 inputs without fused multiply-add, every sum in the order written here; there is NO DIVISION:
 * the even-odd rule on the screen is multiplied through by W > 0.
 *  L1. Sample rule.  U = ((ux*x + uy*y) + uz*z) + u0 from rowU, V and W likewise from rowV / rowW.  The sample fails unless W > 0 (a NaN fails).
 *      For each edge i from a = P[i] to b = P[(i+1) mod n]: du = b_u - a_u, dv = b_v - a_v, sa = a_v*W, sb = b_v*W,
 *      c = du*(V - sa) - dv*(U - a_u*W); the edge is crossed iff (sa > V) != (sb > V) and (c > 0) == (dv > 0).  The sample passes the lasso iff the
 *      number of crossed edges is odd (the even-odd rule, as footprint rule F1: self-intersecting polygons are defined, a polygon of zero area
 *      passes nothing off its own line).  Edge i's sb and edge i+1's sa are the same product, so the rule is watertight at vertices.  A sample
 *      passes the query iff it passes L1 and region rule 3.
 *  L2. Corners.  The eight corners of a node's inflated cube are numbered k = 0..7 with bit 0 for x, bit 1 for y and bit 2 for z, each choosing
 *      hi_a over lo_a; (U_k, V_k, W_k) by L1's formulas at corner k.  fp64 rounding is monotone and the eight corners include the extreme one of
 *      every row, so a node with W_k <= 0 at all eight holds no passing sample and a node with W_k > 0 at all eight has W > 0 at every sample, in
 *      floating point and not only in exact arithmetic.
 *  L3. Far edges, for a node with W_k > 0 at all eight corners.  Edge i is FAR iff c by L1's formula at (U_k, V_k, W_k) is > 0 at all eight
 *      corners or < 0 at all eight, or sa > V and sb > V at all eight, or neither sa > V nor sb > V at any of the eight (each of these quantities
 *      is affine in (x, y, z): its sign on the cube is its sign at the corners).  Any other edge is NEAR.
 *  L4. Node class by the lasso.  OUTSIDE if W_k <= 0 at all eight corners.  FILTERED if the signs of W are mixed or there is a NEAR edge.
 *      Otherwise L1's verdict at corner 0: COPIED if it passes, else OUTSIDE.  The final class combines with the planes' exactly as rule F4 does:
 *      OUTSIDE if outside by either, COPIED iff copied by both, else FILTERED.
 *  L5. For finite samples in the half-open box L2-L4 change nothing against L1 applied to every sample — provided no corner value lies within
 *      fp64 rounding of zero with the wrong exact sign (an edge's plane through the eye grazing a node's corner).  The host mirror asserts this
 *      per query.
 *  L6. lasso == NULL gives exactly simlod_query_region / the footprint-less simlod_paint_region / the footprint-less simlod_query_summary, byte
 *      for byte.  `region` is required and may have zero planes.
 *  L7. hipErrorInvalidValue with nothing enqueued: everything simlod_query_region refuses, numVertices outside 3..256, a non-finite vertex or
 *      row coefficient, nonzero `reserved`, scratchBytes below the call's own minimum (simlod_lasso_buffer_min_bytes(tableCapacity, 0),
 *      simlod_paint_buffer_min_bytes, simlod_summary_buffer_min_bytes).  A row W of zeros is legal and selects nothing; a vertex behind
 *      numVertices is not looked at.
 * For a camera with the row-major world-view-projection matrix M (Uniforms.transform) and a width x height screen whose pixel (i, j) covers ndc
 * [2i/width - 1, 2(i+1)/width - 1]: rowU = width/2 * (M[0] + M[3]), rowV = height/2 * (M[1] + M[3]), rowW = M[3], vertices in pixels. */
#define SIMLOD_LASSO_MAX_VERTICES 256u
typedef struct SimlodLasso {           /* host memory, read before the call returns */
	uint32_t numVertices;              /* 3..256; the polygon closes from the last vertex to the first */
	uint32_t reserved[3];              /* 0 */
	float    rowU[4], rowV[4], rowW[4];   /* U = ((ux*x + uy*y) + uz*z) + u0, V and W likewise: screen position (U/W, V/W) where W > 0 */
	float    vertices[SIMLOD_LASSO_MAX_VERTICES][2];   /* (u, v) on that screen */
} SimlodLasso;
SIMLOD_STATIC_ASSERT(sizeof(SimlodLasso) == 2112, "Lasso");
SIMLOD_STATIC_ASSERT(offsetof(SimlodLasso, rowU) == 16, "Lasso.rowU");
SIMLOD_STATIC_ASSERT(offsetof(SimlodLasso, rowV) == 32, "Lasso.rowV");
SIMLOD_STATIC_ASSERT(offsetof(SimlodLasso, rowW) == 48, "Lasso.rowW");
SIMLOD_STATIC_ASSERT(offsetof(SimlodLasso, vertices) == 64, "Lasso.vertices");

/* simlod_footprint_buffer_min_bytes' value: simlod_query_buffer_min_bytes plus the fixed block for the polygon widened to fp64 (8 KB). */
uint64_t simlod_lasso_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound);

/* The lasso query (rules above; arguments as simlod_query_footprint's).  Asynchronous on `stream` once `lasso` has been read. */
int simlod_query_lasso(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                       const SimlodLasso* lasso /*or NULL*/, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                       SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples, uint64_t sampleCapacity, SimlodQueryCounts* counts,
                       void* stream);

/* simlod_paint_region with a lasso in the footprint's place: rules E0-E9 with "the samples simlod_query_lasso(region, lasso, maxLevel = 20,
 * SIMLOD_EXPORT_ALL) returns" as the target set and order.  The scratch minimum is simlod_paint_buffer_min_bytes. */
int simlod_paint_lasso(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                       const SimlodLasso* lasso /*or NULL*/, const SimlodPaint* paint, void* scratch, uint64_t scratchBytes,
                       SimlodExportNode* table, uint32_t tableCapacity, const uint32_t* colors /*ARRAY only*/, uint32_t* previous /*or NULL*/,
                       uint64_t colorCapacity, SimlodQueryCounts* counts, void* stream);

/* simlod_query_summary with a lasso in the footprint's place: rules S0-S8 with "the samples simlod_query_lasso(region, lasso, maxLevel, select)
 * returns" as the set.  The scratch minimum is simlod_summary_buffer_min_bytes. */
int simlod_query_summary_lasso(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                               const SimlodLasso* lasso /*or NULL*/, const SimlodSummaryParams* params, uint32_t maxLevel, uint32_t select,
                               void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity,
                               SimlodSummary* summary /*device*/, SimlodQueryCounts* counts, void* stream);

/* ---- inverse selections: all but a region, a footprint or a lasso ------------------------------------------------------------------------------
 * simlod_query_inverse, simlod_paint_inverse and simlod_query_summary_inverse are the three verbs of a selection — copy it out, recolour it in
 * place, describe it — for the samples the selection does NOT hold: "everything except this tripod, this car, this parcel".  The complement of a
 * convex region is not convex and that of a lasso is no lasso, so no other call expresses it.  SIMLOD_CLIP_OUTSIDE draws that frame; these calls
 * turn it into data, and importing the query's result (simlod_import_octree) makes it permanent: the selection is erased.
 * POSITIVE below is the existing query with the same arguments: simlod_query_footprint if `footprint` is given, simlod_query_lasso if `lasso` is
 * given, else simlod_query_region.  Everything the region section says about the box, the inflated cube, SimlodQueryCounts and
 * SIMLOD_EXPORT_REGION stays in force.  The flag is the entry point: no `reserved` word of SimlodRegion, SimlodFootprint or SimlodLasso means
 * anything new, and a nonzero one is refused as before.
 * NOT COVERED: inverse profile queries; an inverse clip mode (SIMLOD_CLIP_OUTSIDE exists); inverse on rays, neighbours, views or deltas; a
 * BUILDABLE import of an inverse result — the voxels are filtered by their own position, so a rebuilt grid's popcount no longer equals the voxel
 * count and SIMLOD_ERR_IMPORT_GRID would be right to fire (re-deriving the voxels from the surviving points is a later step).
 *
 *  I1. Sample rule.  A sample passes the inverse iff it does not pass POSITIVE's sample rule: region rule 3 and, where given, F1 or L1.  A NaN
 *      coordinate fails the positive rule, so it passes the inverse.  No new arithmetic: the fp64 operations, their order and the absence of
 *      fused multiply-add are POSITIVE's, bit for bit.
 *  I2. Node classes.  Each node gets POSITIVE's final class (rules 1 and 4, F4, L4) from its own (level, X, Y, Z); then OUTSIDE becomes COPIED
 *      (every sample, no test), COPIED becomes EMPTIED (contributes nothing; its samples are not read) and FILTERED stays FILTERED, by I1.
 *  I3. Listing.  Nothing is culled: the table is simlod_export_octree(maxLevel, select)'s in every field except numSamples and firstSample — the
 *      same entries, order, parent, firstChild, childMask and flags.  An EMPTIED node is listed with numSamples 0.  So the result imports with
 *      the source's tree shape: inner nodes stay inner and their samples stay voxels; a node whose children all vanished does not become a leaf
 *      that draws its voxels as points.
 *  I4. Counts.  numCandidates: the samples of the selected nodes that are not EMPTIED.  numCopiedNodes / numFilteredNodes: such nodes with at
 *      least one sample, by the mapped class.  numSamples: the samples after the test.
 *  I5. Rule 5 (count-only calls, capacities), the chunk-table / `next` sources and the error bits are the region query's.
 *  I6. Partition.  For one set of arguments a node's POSITIVE samples and its inverse samples are disjoint and together are the node's samples, in
 *      chunk-list order.  Sample by sample, whatever the coordinates, as long as POSITIVE lists the node (both calls give the node the same
 *      class, so this covers samples outside the contract too); for a node POSITIVE does not list it holds for the samples of the contract
 *      (F5 / L5).
 *  I7. Degenerate selections.  Zero planes and no polygon: every node is EMPTIED and numSamples is 0.  A selection that selects nothing: the
 *      result equals simlod_export_octree(maxLevel, select) byte for byte.
 *  I8. simlod_paint_inverse follows rules E0-E9 with "the samples simlod_query_inverse(..., 20, SIMLOD_EXPORT_ALL) returns, in that order" as the
 *      target set; `previous` followed by an ARRAY paint with the same arguments is the undo.  simlod_query_summary_inverse follows rules S0-S8
 *      with simlod_query_inverse(..., maxLevel, select) as the set.
 *  I9. hipErrorInvalidValue with nothing enqueued: everything POSITIVE refuses; `footprint` and `lasso` both non-NULL; scratchBytes below the
 *      call's own minimum (simlod_inverse_buffer_min_bytes(tableCapacity, 0), simlod_paint_buffer_min_bytes, simlod_summary_buffer_min_bytes) —
 *      the same with or without a polygon.
 *  I10. For a selection of planes only, the inverse at maxLevel 20 / SIMLOD_EXPORT_ALL holds, per node, exactly the samples that clip rule C3's
 *      SIMLOD_CLIP_OUTSIDE edit keeps, in order. */

/* simlod_footprint_buffer_min_bytes' value, whether a polygon is given or not. */
uint64_t simlod_inverse_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound);

/* The inverse query (rules above; arguments as simlod_query_footprint's and simlod_query_lasso's, at most one of the two polygons).  Asynchronous
 * on `stream` once the polygon has been read. */
int simlod_query_inverse(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                         const SimlodFootprint* footprint /*or NULL*/, const SimlodLasso* lasso /*or NULL*/, uint32_t maxLevel, uint32_t select,
                         void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples /*or NULL*/,
                         uint64_t sampleCapacity, SimlodQueryCounts* counts, void* stream);

/* simlod_paint_region on the inverse selection (rule I8).  The scratch minimum is simlod_paint_buffer_min_bytes. */
int simlod_paint_inverse(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                         const SimlodFootprint* footprint /*or NULL*/, const SimlodLasso* lasso /*or NULL*/, const SimlodPaint* paint, void* scratch,
                         uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, const uint32_t* colors /*ARRAY only*/,
                         uint32_t* previous /*or NULL*/, uint64_t colorCapacity, SimlodQueryCounts* counts, void* stream);

/* simlod_query_summary on the inverse selection (rule I8).  The scratch minimum is simlod_summary_buffer_min_bytes. */
int simlod_query_summary_inverse(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRegion* region,
                                 const SimlodFootprint* footprint /*or NULL*/, const SimlodLasso* lasso /*or NULL*/,
                                 const SimlodSummaryParams* params, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                                 SimlodExportNode* table, uint32_t tableCapacity, SimlodSummary* summary /*device*/, SimlodQueryCounts* counts,
                                 void* stream);

/* ---- ray queries: the first sample in a cone along each ray of a batch ----------------------------------------------------------------------
 * simlod_query_rays answers "what does this ray hit" for up to 2^20 rays at once: per ray the sample with the smallest parameter t that lies
 * within radius + spread * t of the ray, among the samples of the nodes simlod_export_octree(maxLevel, select) selects.  The source is only read.
 *
 * The box is the builder's, as for region queries (min = uniforms.boxMin, size = the largest fp32 extent).  All geometry is fp64 computed from the
 * fp32 inputs without fused multiply-add, every sum in the order written here; divisions are IEEE divisions.  s, e, lo_a, hi_a of a node are
 * those of region-query rule 1 (the cube inflated by one level-20 cell).
 *  0. The table.  The nodes considered are exactly the entries of simlod_export_octree(maxLevel, select) on the same octree, select ALL, CUT or
 *     VISIBLE (VISIBLE is refused as the export refuses it when no frame ran).  SimlodRayHit.node is an index into THAT table and `ordinal` an
 *     index into that node's sample range: export.samples[export.nodes[node].firstSample + ordinal] is the hit's sample.  With table != NULL the
 *     call also writes that table, byte for byte the export's (it is never pruned per ray); tableCapacity bounds the walk either way.
 *  1. Valid rays.  A ray is valid iff every float is finite, dir != 0, 0 <= tMin <= tMax, radius >= 0, spread >= 0 and reserved == 0.  An
 *     invalid ray misses, is counted in numInvalid and forms no pair (checked on the device: rays may come from a kernel).
 *  2. The sample test.  With p = sample - origin (per component), dd = (dx*dx + dy*dy) + dz*dz, t = ((dx*px + dy*py) + dz*pz) / dd,
 *     q_a = p_a - t*d_a, s2 = (qx*qx + qy*qy) + qz*qz and rr = radius + spread*t the sample passes iff t >= tMin && t <= tMax && s2 <= rr*rr
 *     (a NaN fails).
 *  3. Pairs.  A valid ray and a selected table entry with numSamples > 0 form a PAIR iff the entry and all its listed ancestors pass the slab
 *     test: R = radius + spread*tMax; per axis a, L = lo_a - R and H = hi_a + R; if d_a == 0 the axis fails iff o_a < L || o_a > H and otherwise
 *     contributes nothing; else t1 = (L - o_a)/d_a, t2 = (H - o_a)/d_a, n_a = fmin(t1, t2), f_a = fmax(t1, t2); the node passes iff no axis fails
 *     and max(tMin, n_x, n_y, n_z) <= min(tMax, f_x, f_y, f_z) over the contributing axes.  numPairs is the number of pairs, numCandidates the
 *     sum of numSamples over the pairs; both are defined by this rule alone, whatever work the kernels skip.
 *  4. The hit of a valid ray is, among the samples of its pairs that pass rule 2, the one with the smallest t; equal t: the smallest node,
 *     then the smallest ordinal.  No passing sample: a miss (t = +infinity, node = ordinal = 0xffffffff, a zero sample).  The result is a pure
 *     function of the octree image and the rays.  For finite samples in the half-open box the culling of rule 3 never changes it: a passing
 *     sample lies within R of the ray's point at its t, which therefore lies in the node's cube widened by R, and in every ancestor's (what e
 *     leaves over the builder's quantisation slack, about size * 2^-21, is many orders above the fp64 rounding of the slab test, about
 *     size * 2^-50).  OUTSIDE THE CONTRACT, as in region-query rule 4: samples outside that box or on its max faces; such a sample is a
 *     candidate iff the node it is stored in forms a pair.
 *  5. hits == NULL: count only — the counts (and the table, if asked for) are complete, nothing else is written, and
 *     simlod_rays_buffer_min_bytes(cap, bound, numRays, 0, 0) of scratch suffices (numHits then comes from a ray-major pass that stops at a
 *     ray's first passing sample: it reads a chunk once per ray that reaches it, so a host that wants the hits anyway asks for them).
 *     With hits, scratch sized from the counts of a count-only call always suffices; a buffer that holds the walk but not the pairs sets
 *     SIMLOD_EXPORT_ERR_CAPACITY and then NO hit record is written; a walk error (ERR_NODE_COUNT, ERR_SHORT_LIST, the table capacity) likewise. */
typedef struct SimlodRay {             /* DEVICE memory */
	float    origin[3]; float tMin;    /* world coordinates (the uniforms' box)                                 */
	float    dir[3];    float tMax;    /* any non-zero direction; t is in units of |dir|                        */
	float    radius;    float spread;  /* cone radius at parameter t: radius + spread * t                       */
	uint32_t reserved[2];              /* 0                                                                     */
} SimlodRay;
typedef struct SimlodRayHit {          /* DEVICE memory, one per ray, in ray order */
	double      t;                     /* parameter of the hit; miss: +infinity                                 */
	uint32_t    node;                  /* table index of the node that holds it; miss: 0xffffffff               */
	uint32_t    ordinal;               /* index among that node's samples in chunk-list order; miss: 0xffffffff */
	SimlodPoint sample;                /* the 16 bytes of the sample; miss: zeros                               */
} SimlodRayHit;
typedef struct SimlodRayCounts {       /* written by the device */
	uint32_t numNodes;                 /* table entries                                                         */
	uint32_t error;                    /* SIMLOD_EXPORT_ERR_* bits                                              */
	uint32_t numHits;                  /* rays with a hit                                                        */
	uint32_t numInvalid;               /* rays that fail rule 1                                                 */
	uint64_t numPairs;                 /* rule 3                                                                */
	uint64_t numCandidates;            /* rule 3                                                                */
} SimlodRayCounts;
SIMLOD_STATIC_ASSERT(sizeof(SimlodRay) == 48, "Ray");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRay, tMin) == 12, "Ray.tMin");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRay, dir) == 16, "Ray.dir");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRay, tMax) == 28, "Ray.tMax");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRay, radius) == 32, "Ray.radius");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRay, spread) == 36, "Ray.spread");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRay, reserved) == 40, "Ray.reserved");
SIMLOD_STATIC_ASSERT(sizeof(SimlodRayHit) == 32, "RayHit");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRayHit, node) == 8, "RayHit.node");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRayHit, ordinal) == 12, "RayHit.ordinal");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRayHit, sample) == 16, "RayHit.sample");
SIMLOD_STATIC_ASSERT(sizeof(SimlodRayCounts) == 32, "RayCounts");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRayCounts, numHits) == 8, "RayCounts.numHits");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRayCounts, numInvalid) == 12, "RayCounts.numInvalid");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRayCounts, numPairs) == 16, "RayCounts.numPairs");
SIMLOD_STATIC_ASSERT(offsetof(SimlodRayCounts, numCandidates) == 24, "RayCounts.numCandidates");
#define SIMLOD_RAYS_MAX (1u << 20)

/* Bytes of the `scratch` buffer a ray query needs: a table of up to nodeCapacity entries whose selected nodes hold up to sampleBound samples
 * (Stats.numPoints + Stats.numVoxels always suffices), numRays rays, and — for a call with hits — the numPairs and numCandidates a count-only
 * call reported (0, 0: enough for a count-only call).  The sum of a part that depends on nodeCapacity and numRays only, 32 bytes per chunk
 * item for sampleBound / 1000 + nodeCapacity + 1 items, 32 bytes per pair (its record and one partial result) and 16 bytes per further thousand
 * candidates.  What a call with hits really needs is the same sum with the chunks the table's selected nodes have (ceil(numSamples / 1000)
 * each) in the place of that item bound: one byte less sets SIMLOD_EXPORT_ERR_CAPACITY. */
uint64_t simlod_rays_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound, uint32_t numRays, uint64_t numPairs, uint64_t numCandidates);

/* The ray query (rules above).  Asynchronous on `stream`; everything in between lives in `scratch`.  hipErrorInvalidValue with nothing
 * enqueued: a null pointer other than `table` / `hits`, numRays == 0 or > SIMLOD_RAYS_MAX, `select` other than ALL / CUT / VISIBLE (VISIBLE
 * without a frame), scratchBytes below simlod_rays_buffer_min_bytes(tableCapacity, 0, numRays, 0, 0).  A scratch buffer too small for the
 * chunk items or the pairs sets SIMLOD_EXPORT_ERR_CAPACITY on the device.  While the builder's chunk table for `nodes` is valid the first
 * chunks of each list come from it, the rest by `next` (as simlod_export_octree). */
int simlod_query_rays(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodRay* rays, uint32_t numRays,
                      uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity,
                      SimlodRayHit* hits, SimlodRayCounts* counts, void* stream);

/* ---- neighbour queries: the k nearest samples within a radius of each position of a batch ------------------------------------------------------
 * simlod_query_neighbours answers "which samples lie around this position" for up to 2^20 positions at once: per query the k <= 16 samples
 * nearest to `center` among those within `radius` of it, among the samples of the nodes simlod_export_octree(maxLevel, select) selects, and how
 * many samples lie within the radius at all.  The source is only read.
 *
 * The box is the builder's, as for region queries (min = uniforms.boxMin, size = the largest fp32 extent).  All geometry is fp64 computed from the
 * fp32 inputs without fused multiply-add, every sum in the order written here.  s, e, lo_a, hi_a of a node are those of region-query rule 1 (the
 * cube inflated by one level-20 cell).  c_a is the centre, r the radius, rr = r*r.
 *  0. The table.  Exactly as ray-query rule 0: the nodes considered are the entries of simlod_export_octree(maxLevel, select) on the same octree,
 *     select ALL, CUT or VISIBLE (VISIBLE is refused as the export refuses it when no frame ran).  SimlodNeighbour.node is an index into THAT
 *     table and `ordinal` an index into that node's sample range: export.samples[export.nodes[node].firstSample + ordinal] is the neighbour's
 *     sample.  With table != NULL the call also writes that table, byte for byte the export's; tableCapacity bounds the walk either way.
 *  1. Valid queries.  A query is valid iff its four floats are finite and radius >= 0 (radius 0 is valid).  An invalid query forms no pair, is
 *     counted in numInvalid, and gets k miss records and within = 0 (checked on the device: queries may come from a kernel).
 *  2. The sample test.  With p_a = s_a - c_a per component of the sample s, d2 = (px*px + py*py) + pz*pz; the sample passes iff d2 <= rr (a NaN
 *     fails).
 *  3. Pairs.  A valid query and a selected table entry with numSamples > 0 form a PAIR iff the entry and all its listed ancestors pass the
 *     sphere-cube test: ex_a = max(lo_a - c_a, 0, c_a - hi_a), g2 = (ex_x*ex_x + ex_y*ex_y) + ex_z*ex_z; the node passes iff g2 <= rr.  numPairs
 *     is the number of pairs, numCandidates the sum of numSamples over the pairs; both are defined by this rule alone, whatever work the kernels
 *     skip.  For finite samples in the half-open box the culling never changes a result: such a sample lies in its node's exact cube and in
 *     every ancestor's up to the builder's quantisation slack (about size * 2^-22), so per axis |p_a| exceeds ex_a by at least what e leaves
 *     over that slack (about size * 2^-21, many orders above the fp64 rounding of the differences, about size * 2^-52) wherever ex_a > 0, and
 *     |p_a| >= 0 = ex_a elsewhere; squares of non-negative numbers and sums taken in the same order are monotone under IEEE rounding, so
 *     g2 <= d2, and d2 <= rr implies g2 <= rr for the node and each of its ancestors.  OUTSIDE THE CONTRACT, as in region-query rule 4 and for
 *     rays: samples outside that box, on its max faces or with non-finite coordinates; such a sample is a candidate iff the node it is stored
 *     in forms a pair.
 *  4. The result.  neighbours[q*k .. q*k + k) holds the first k of query q's passing samples (those of its pairs that pass rule 2) in the total
 *     order (d2, node, ordinal), ascending; the places behind them hold the miss record (d2 = +infinity, node = ordinal = 0xffffffff, a zero
 *     sample).  within[q] is the number of passing samples among the query's pairs, however large.  numFound is the sum over the queries of
 *     min(k, within), numWithin the sum of within.  Everything returned is the prefix of one total order or a sum: a pure function of the
 *     octree image and the queries.  A query centred on a sample finds that sample at d2 = 0: callers who want the OTHER points ask for k + 1.
 *  5. neighbours == NULL: count only, and then `within` must be NULL too — the counts (and the table, if asked for) are complete except that
 *     numFound = numWithin = 0; no sample is tested, nothing else is written, and simlod_neighbours_buffer_min_bytes(cap, bound, n, k, 0, 0) of
 *     scratch suffices.  With results, scratch sized from the numPairs and numCandidates of a count-only call always suffices; a buffer that
 *     holds the walk but not the pairs sets SIMLOD_EXPORT_ERR_CAPACITY and then NO neighbour or within record is written; a walk error
 *     (ERR_NODE_COUNT, ERR_SHORT_LIST, the table capacity) likewise. */
typedef struct SimlodSphere {          /* DEVICE memory */
	float    center[3];                /* world coordinates (the uniforms' box)                                 */
	float    radius;                   /* >= 0                                                                  */
} SimlodSphere;
typedef struct SimlodNeighbour {       /* DEVICE memory, k per query, in query order (SimlodRayHit's shape) */
	double      d2;                    /* squared distance (rule 2); miss: +infinity                            */
	uint32_t    node;                  /* table index of the node that holds it; miss: 0xffffffff               */
	uint32_t    ordinal;               /* index among that node's samples in chunk-list order; miss: 0xffffffff */
	SimlodPoint sample;                /* the 16 bytes of the sample; miss: zeros                               */
} SimlodNeighbour;
typedef struct SimlodNeighbourCounts { /* written by the device */
	uint32_t numNodes;                 /* table entries                                                         */
	uint32_t error;                    /* SIMLOD_EXPORT_ERR_* bits                                              */
	uint32_t numInvalid;               /* queries that fail rule 1                                              */
	uint32_t k;                        /* the call's k                                                          */
	uint64_t numPairs;                 /* rule 3                                                                */
	uint64_t numCandidates;            /* rule 3                                                                */
	uint64_t numFound;                 /* neighbour records that are not the miss record (rule 4)               */
	uint64_t numWithin;                /* the sum of within (rule 4)                                            */
} SimlodNeighbourCounts;
SIMLOD_STATIC_ASSERT(sizeof(SimlodSphere) == 16, "Sphere");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSphere, radius) == 12, "Sphere.radius");
SIMLOD_STATIC_ASSERT(sizeof(SimlodNeighbour) == 32, "Neighbour");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbour, node) == 8, "Neighbour.node");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbour, ordinal) == 12, "Neighbour.ordinal");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbour, sample) == 16, "Neighbour.sample");
SIMLOD_STATIC_ASSERT(sizeof(SimlodNeighbourCounts) == 48, "NeighbourCounts");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbourCounts, numInvalid) == 8, "NeighbourCounts.numInvalid");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbourCounts, k) == 12, "NeighbourCounts.k");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbourCounts, numPairs) == 16, "NeighbourCounts.numPairs");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbourCounts, numCandidates) == 24, "NeighbourCounts.numCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbourCounts, numFound) == 32, "NeighbourCounts.numFound");
SIMLOD_STATIC_ASSERT(offsetof(SimlodNeighbourCounts, numWithin) == 40, "NeighbourCounts.numWithin");
#define SIMLOD_NEIGHBOURS_MAX (1u << 20)
#define SIMLOD_NEIGHBOURS_MAX_K 16u

/* Bytes of the `scratch` buffer a neighbour query needs: a table of up to nodeCapacity entries whose selected nodes hold up to sampleBound
 * samples (Stats.numPoints + Stats.numVoxels always suffices), numQueries queries, and — for a call with results — the numPairs and
 * numCandidates a count-only call reported (0, 0: enough for a count-only call).  The sum of a part that depends on nodeCapacity and numQueries
 * only (the ray query's for as many rays), 32 bytes per chunk item for sampleBound / 1000 + nodeCapacity + 1 items, 16 + 16 * (k + 1) bytes per
 * pair (its record and one partial result: k entries and a count) and 16 * (k + 1) bytes per further thousand candidates.  What a call with
 * results really needs is the same sum with the chunks the table's selected nodes have (ceil(numSamples / 1000) each) in the place of that
 * item bound: one byte less sets SIMLOD_EXPORT_ERR_CAPACITY. */
uint64_t simlod_neighbours_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound, uint32_t numQueries, uint32_t k, uint64_t numPairs,
                                            uint64_t numCandidates);

/* The neighbour query (rules above).  Asynchronous on `stream`; everything in between lives in `scratch`.  hipErrorInvalidValue with nothing
 * enqueued and nothing touched: a null pointer other than `table` / `neighbours` / `within`, within != NULL while neighbours == NULL,
 * numQueries == 0 or > SIMLOD_NEIGHBOURS_MAX, k == 0 or > SIMLOD_NEIGHBOURS_MAX_K, `select` other than ALL / CUT / VISIBLE (VISIBLE without a
 * frame), scratchBytes below simlod_neighbours_buffer_min_bytes(tableCapacity, 0, numQueries, k, 0, 0).  `within` may be NULL in a call with
 * neighbours.  A scratch buffer too small for the chunk items or the pairs sets SIMLOD_EXPORT_ERR_CAPACITY on the device.  While the builder's
 * chunk table for `nodes` is valid the first chunks of each list come from it, the rest by `next` (as simlod_export_octree). */
int simlod_query_neighbours(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodSphere* queries,
                            uint32_t numQueries, uint32_t k, uint32_t maxLevel, uint32_t select, void* scratch, uint64_t scratchBytes,
                            SimlodExportNode* table, uint32_t tableCapacity, SimlodNeighbour* neighbours, uint32_t* within,
                            SimlodNeighbourCounts* counts, void* stream);

/* ---- view queries: the level-of-detail cut a camera needs, within a sample budget --------------------------------------------------------------
 * simlod_query_view writes what simlod_export_octree(maxLevel, SIMLOD_EXPORT_VISIBLE) writes after a frame — without a frame: no render buffer,
 * nothing written to the source, and with a ladder of what coarser cuts would cost, from which a sample budget chooses one.
 *
 * The camera is `uniforms`: width, height, transform_updateBound, minNodeSize, boxMin, boxMax, as simlod_launch_render takes them (cube size = the
 * largest fp32 extent, min = boxMin).  All geometry is the fp32 arithmetic of kernel_render's visibility pass (render.cu:760-861), without fused
 * multiply-add, divisions and square roots correctly rounded:
 *   planes   row vectors r_j = (M[j].x, M[j].y, M[j].z, M[j].w) of M = transform_updateBound; the six planes r3 - r0, r3 + r0, r3 + r1, r3 - r1,
 *            r3 - r2, r3 + r2, each divided by len = sqrtf((x*x + y*y) + z*z) of its first three components.
 *   cube     s = size / 2^level; mn_a = min_a + ((float)A + 0.0f) * s, mx_a = min_a + ((float)A + 1.0f) * s for the node's coordinate A on axis a.
 *   inside   for every plane (nx, ny, nz, c): v_a = n_a > 0 ? mx_a : mn_a; d = (((nx*vx) + ny*vy) + nz*vz) + c; inside iff no plane has d < 0.
 *   extents  the corners p000, p001, p010, p011, p100, p101, p110, p111 (bit 2 of the corner number picks mx on x, bit 1 on y, bit 0 on z);
 *            dot(r, p) = (((r.x*p.x) + r.y*p.y) + r.z*p.z) + r.w*1.0f; sx = ((dot(r0, p) / dot(r3, p)) * 0.5f + 0.5f) * width, sy likewise from r1
 *            and height; min and max over the corners as the trees fminf(fminf(fminf(s0, s1), fminf(s2, s3)), fminf(fminf(s4, s5), fminf(s6, s7)))
 *            and fmaxf likewise (fminf / fmaxf drop a NaN); dx = maxx - minx, dy = maxy - miny.
 *  V1. Listed nodes: exactly as simlod_export_octree — breadth-first, every node with level <= maxLevel; FLAG_LEAF as there.
 *  V2. inside(n) as above, or true under SIMLOD_VIEW_NO_CULL.  has(n): the node's sample count (numPoints of a source leaf, else numVoxels) > 0.
 *      visible(n) = inside && has.  numInside counts the listed nodes that are visible.
 *  V3. large_b(n) iff (double)dx > L_b || (double)dy > L_b with L_b = 2.0 * (double)minNodeSize * 2^b (exact; a NaN extent is never large).
 *      R(n) = the number of b in 0..20 with large_b(n).  P(root) = 21 under SIMLOD_VIEW_DRAW_SMALL_ROOT, else 0; P(n) = R(parent of n) otherwise.
 *  V4. drawn_b(n) iff visible(n) && (b < R(n) ? leaf(n) : b < P(n)) — render.cu:905-935 with minNodeSize * 2^b.
 *  V5. S(b) = the sum of the sample counts of the listed nodes drawn at b, for every b in 0..20: samplesAt, whatever minBias / maxBias say.
 *  V6. bias = the smallest b in [minBias, maxBias] with S(b) <= sampleBudget (S need not be monotone: the finest cut that fits wins).  If none
 *      fits: SIMLOD_EXPORT_ERR_BUDGET, bias = maxBias, the table is complete for maxBias, numSamples = S(maxBias), and no sample is written.
 *      S may be 0: once the root is not large nothing is drawn, as in a frame (SIMLOD_VIEW_DRAW_SMALL_ROOT draws it then).
 *  V7. SELECTED, numSamples and firstSample follow drawn_bias; numSelected counts the selected nodes.  Samples in chunk-list order, as the export
 *      writes them.  samples == NULL: count only — the table and the counts are complete, nothing else is written (sampleCapacity is ignored).
 *      Capacity errors as simlod_export_octree; a scratch buffer too small for the chunk items sets SIMLOD_EXPORT_ERR_CAPACITY.
 *  V8. With flags == 0 and no budget the table and the samples equal, byte for byte, simlod_export_octree(maxLevel, SIMLOD_EXPORT_VISIBLE) after a
 *      simlod_launch_render (no clip set) with the same uniforms except minNodeSize * 2^bias.
 *  V9. The source is only read: Node.visible / isLarge keep the last frame's values. */
typedef struct SimlodView {            /* host memory, read before the call returns */
	uint32_t flags;                    /* SIMLOD_VIEW_* */
	uint32_t minBias, maxBias;         /* 0 <= minBias <= maxBias <= 20 */
	uint32_t reserved;                 /* 0 */
	uint64_t sampleBudget;             /* 0xffffffffffffffff: none */
} SimlodView;
#define SIMLOD_VIEW_MAX_BIAS        20u
#define SIMLOD_VIEW_NO_CULL         0x1u   /* every node counts as inside the frustum */
#define SIMLOD_VIEW_DRAW_SMALL_ROOT 0x2u   /* the root counts as having a large parent */
#define SIMLOD_EXPORT_ERR_BUDGET    0x8u   /* SimlodViewCounts.error: no bias in [minBias, maxBias] fits sampleBudget */
typedef struct SimlodViewCounts {      /* written by the device */
	uint32_t numNodes;                 /* table entries written                                                                  */
	uint32_t error;                    /* SIMLOD_EXPORT_ERR_* bits                                                               */
	uint64_t numSamples;               /* S(bias) (= written, unless count-only or an error)                                     */
	uint32_t bias;                     /* the chosen bias                                                                        */
	uint32_t numSelected;              /* listed nodes drawn at `bias`                                                           */
	uint32_t numInside;                /* listed nodes that are visible (V2)                                                     */
	uint32_t reserved;                 /* 0                                                                                      */
	uint64_t samplesAt[SIMLOD_VIEW_MAX_BIAS + 1u];   /* S(b) for b = 0..20                                                       */
} SimlodViewCounts;
SIMLOD_STATIC_ASSERT(sizeof(SimlodView) == 24, "View");
SIMLOD_STATIC_ASSERT(offsetof(SimlodView, minBias) == 4, "View.minBias");
SIMLOD_STATIC_ASSERT(offsetof(SimlodView, maxBias) == 8, "View.maxBias");
SIMLOD_STATIC_ASSERT(offsetof(SimlodView, sampleBudget) == 16, "View.sampleBudget");
SIMLOD_STATIC_ASSERT(sizeof(SimlodViewCounts) == 200, "ViewCounts");
SIMLOD_STATIC_ASSERT(offsetof(SimlodViewCounts, numSamples) == 8, "ViewCounts.numSamples");
SIMLOD_STATIC_ASSERT(offsetof(SimlodViewCounts, bias) == 16, "ViewCounts.bias");
SIMLOD_STATIC_ASSERT(offsetof(SimlodViewCounts, numSelected) == 20, "ViewCounts.numSelected");
SIMLOD_STATIC_ASSERT(offsetof(SimlodViewCounts, numInside) == 24, "ViewCounts.numInside");
SIMLOD_STATIC_ASSERT(offsetof(SimlodViewCounts, samplesAt) == 32, "ViewCounts.samplesAt");

/* The view query (rules above).  Asynchronous on `stream`; everything in between lives in `scratch`, whose chunk items (32 bytes per 1 000-sample
 * chunk of the result) take what the buffer has behind simlod_export_buffer_min_bytes(tableCapacity, 0): size it by
 * simlod_export_buffer_min_bytes(tableCapacity, samples of the result).  hipErrorInvalidValue with nothing enqueued: a null pointer other than
 * `samples`, unknown flag bits, nonzero `reserved`, minBias > maxBias, maxBias > 20, a non-finite minNodeSize, width, height or entry of
 * transform_updateBound, scratchBytes below simlod_export_buffer_min_bytes(tableCapacity, 0).  While the builder's chunk table for `nodes` is
 * valid the first chunks of each list come from it, the rest by `next` (as simlod_export_octree). */
int simlod_query_view(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodView* view, uint32_t maxLevel,
                      void* scratch, uint64_t scratchBytes, SimlodExportNode* table, uint32_t tableCapacity, SimlodPoint* samples,
                      uint64_t sampleCapacity, SimlodViewCounts* counts, void* stream);

/* ---- view deltas: what a camera move adds to the cut a receiver holds ------------------------------------------------------------------------
 * simlod_query_view_delta answers simlod_query_view's question for a receiver that still holds the result of an earlier call: it writes the
 * new cut's table, per entry what the receiver has of it already, the samples it lacks, and the held entries it may drop.
 * simlod_merge_view_delta puts a held sample array and a delta together into the new cut's sample array.
 *
 * A table's entries ascend by (level, Morton(X, Y, Z)) — breadth-first, children in octant order —, so an entry's counterpart in another table
 * is found by key, without walking that table.
 *  D1. `table` and `counts.view` are byte for byte what simlod_query_view writes for the same nodes / uniforms / view / maxLevel: the chosen
 *      bias, the ladder, SIMLOD_EXPORT_ERR_BUDGET.  On a budget error no sample is written and every entry has state NONE (numKept = numDelta =
 *      0).  The table is an ordinary table: it validates, and it is the `held` of the next call.
 *  D2. entries[t].held = the index h < numHeld with held[h].(level, X, Y, Z) == table[t].(level, X, Y, Z), else SIMLOD_EXPORT_NONE.  `held`
 *      must be a table this library wrote (any export, query or merge; of an older, a cropped or a truncated octree).  For any other content
 *      the result is unspecified, but nothing outside held[0, numHeld) is read and nothing outside the outputs is written.  held == NULL
 *      requires numHeld == 0.
 *  D3. An entry that is not SELECTED has state NONE.  For a SELECTED entry with n = numSamples: hs = held[h].numSamples where the held entry is
 *      SELECTED, 0 otherwise or without h; the kind agrees when FLAG_LEAF is equal on both sides.  KEPT iff the kinds agree and hs == n and
 *      n > 0: numKept = n.
 *  D4. GROWN iff SIMLOD_DELTA_TAILS is set, the kinds agree and 0 < hs < n: numKept = hs, and the node contributes the samples [hs, n) of its
 *      chunk list.  This rests on an invariant of kernel_construct: while a node keeps its kind its list is only appended to — stored samples
 *      are neither moved nor rewritten.  The caller must not set the flag across a reset, an import or a colour-filter launch.  hs > n: ADDED.
 *  D5. Every other SELECTED entry is ADDED (one with n == 0 too), numKept = 0.  numDelta = numSamples - numKept, firstDelta the exclusive scan
 *      of numDelta in table order; `delta` holds numDelta samples per entry at firstDelta, inside a node in chunk-list order.
 *  D6. `dropped` lists, in ascending order, the held indices h with held[h] SELECTED, held[h].numSamples > 0 and no KEPT or GROWN entry whose
 *      `held` is h.  numDropped is exact whatever droppedCapacity is; more than droppedCapacity of them set SIMLOD_EXPORT_ERR_CAPACITY
 *      (dropped == NULL: the list is only counted), and nothing is written beyond the capacity.  The same holds for deltaCapacity
 *      (delta == NULL: count only — table, entries, dropped and counts are complete, no sample is written) and tableCapacity.
 *  D7. With numHeld == 0 every selected entry is ADDED, firstDelta == firstSample, and `delta` equals simlod_query_view's samples byte for byte.
 *  D8. The source octree and `held` are only read.  Rule V9 carries over.
 *  D9. simlod_merge_view_delta: the samples [firstSample, firstSample + numKept + numDelta) of each entry whose state is not NONE are
 *      heldSamples[held[h].firstSample .. + numKept) followed by delta[firstDelta .. + numDelta).  After a delta on an unchanged octree the
 *      result equals simlod_query_view's sample array byte for byte; after growth exactly when the invariant of D4 holds.  `counts` as the
 *      export writes them (numNodes, error, numSamples = the samples assembled); an entry that reaches beyond sampleCapacity sets
 *      SIMLOD_EXPORT_ERR_CAPACITY and nothing is written; a KEPT or GROWN entry whose `held` is not below numHeld sets
 *      SIMLOD_EXPORT_ERR_SHORT_LIST and is left out. */
typedef struct SimlodDeltaEntry {      /* one per entry of `table`, same index; written by the device */
	uint32_t held;                     /* index of the held-table entry with this entry's (level, X, Y, Z); SIMLOD_EXPORT_NONE: none */
	uint32_t state;                    /* SIMLOD_DELTA_*                                                                          */
	uint32_t numKept;                  /* leading samples of the node that the receiver holds already                            */
	uint32_t numDelta;                 /* table[t].numSamples - numKept: this node's samples in the delta array                  */
	uint64_t firstDelta;               /* exclusive scan of numDelta in table order                                              */
} SimlodDeltaEntry;
#define SIMLOD_DELTA_NONE  0u
#define SIMLOD_DELTA_KEPT  1u
#define SIMLOD_DELTA_GROWN 2u
#define SIMLOD_DELTA_ADDED 3u
#define SIMLOD_DELTA_TAILS 0x1u        /* deltaFlags: allow GROWN (rule D4) */
typedef struct SimlodDeltaCounts {     /* written by the device */
	SimlodViewCounts view;             /* exactly what simlod_query_view reports for the same arguments (error: with the delta's own bits) */
	uint64_t numDeltaSamples;          /* the sum of numDelta (= written, unless count-only or an error)                         */
	uint64_t numKeptSamples;           /* the sum of numKept                                                                     */
	uint32_t numKept, numGrown, numAdded;   /* entries in each state                                                             */
	uint32_t numDropped;               /* rule D6                                                                                */
} SimlodDeltaCounts;
SIMLOD_STATIC_ASSERT(sizeof(SimlodDeltaEntry) == 24, "DeltaEntry");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaEntry, state) == 4, "DeltaEntry.state");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaEntry, numKept) == 8, "DeltaEntry.numKept");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaEntry, numDelta) == 12, "DeltaEntry.numDelta");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaEntry, firstDelta) == 16, "DeltaEntry.firstDelta");
SIMLOD_STATIC_ASSERT(sizeof(SimlodDeltaCounts) == 232, "DeltaCounts");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaCounts, numDeltaSamples) == 200, "DeltaCounts.numDeltaSamples");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaCounts, numKeptSamples) == 208, "DeltaCounts.numKeptSamples");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaCounts, numKept) == 216, "DeltaCounts.numKept");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaCounts, numGrown) == 220, "DeltaCounts.numGrown");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaCounts, numAdded) == 224, "DeltaCounts.numAdded");
SIMLOD_STATIC_ASSERT(offsetof(SimlodDeltaCounts, numDropped) == 228, "DeltaCounts.numDropped");

/* Bytes of the `scratch` buffer the two calls below need for tables of up to nodeCapacity entries, results of up to sampleBound samples and
 * a held table of numHeld entries. */
uint64_t simlod_view_delta_buffer_min_bytes(uint32_t nodeCapacity, uint64_t sampleBound, uint32_t numHeld);

/* The view delta (rules above).  Asynchronous on `stream`; `entries` has room for tableCapacity records.  The copy items (32 bytes per piece of
 * at most 1 000 samples) take what `scratch` has behind simlod_view_delta_buffer_min_bytes(tableCapacity, 0, numHeld): size it by
 * simlod_view_delta_buffer_min_bytes(tableCapacity, samples of the delta, numHeld); too few set SIMLOD_EXPORT_ERR_CAPACITY.
 * hipErrorInvalidValue with nothing enqueued: everything simlod_query_view refuses, unknown deltaFlags, held == NULL with numHeld != 0,
 * dropped == NULL with droppedCapacity != 0, a null pointer other than `delta`, `held` and `dropped`, scratchBytes below
 * simlod_view_delta_buffer_min_bytes(tableCapacity, 0, numHeld). */
int simlod_query_view_delta(const SimlodNode* nodes, const SimlodStats* stats, const SimlodUniforms* uniforms, const SimlodView* view, uint32_t maxLevel,
                            const SimlodExportNode* held, uint32_t numHeld, uint32_t deltaFlags, void* scratch, uint64_t scratchBytes,
                            SimlodExportNode* table, uint32_t tableCapacity, SimlodDeltaEntry* entries, SimlodPoint* delta, uint64_t deltaCapacity,
                            uint32_t* dropped, uint32_t droppedCapacity, SimlodDeltaCounts* counts, void* stream);

/* The merge (rule D9) of the arrays a receiver has: the held table and its samples, and the table, entries and delta of a
 * simlod_query_view_delta call against that held table; numNodes entries.  All device memory; asynchronous on `stream`.  The scratch bound is
 * simlod_view_delta_buffer_min_bytes(numNodes, samples of the result, numHeld), refused below (numNodes, 0, numHeld) as above.
 * hipErrorInvalidValue with nothing enqueued: a null pointer other than `held` (with numHeld == 0), `heldSamples`, `delta` and `samples` (with
 * sampleCapacity == 0); a scratch buffer below the bound. */
int simlod_merge_view_delta(const SimlodExportNode* held, uint32_t numHeld, const SimlodPoint* heldSamples, const SimlodExportNode* table,
                            const SimlodDeltaEntry* entries, uint32_t numNodes, const SimlodPoint* delta, void* scratch, uint64_t scratchBytes,
                            SimlodPoint* samples, uint64_t sampleCapacity, SimlodExportCounts* counts, void* stream);

/* ---- packed samples: 8-byte records for export, query and delta results -------------------------------------------------------------------------
 * Every way out of the octree ends in 16-byte SimlodPoint records.  simlod_pack_samples turns the samples of any table + samples pair this library
 * wrote — an export, a region / footprint / profile / view query, a view delta — into 8-byte records, simlod_unpack_samples turns them back.
 * A voxel is a cell of its node's 128^3 grid and comes back bit for bit; a point is stored relative to its leaf's cube with 13 bits per axis.
 *
 * Box: min = uniforms.boxMin, size = the largest fp32 extent, as in the region queries.  All fp64 arithmetic works from the fp32 inputs, without
 * contraction, in the order written.
 *  K0. A packed sample is one little-endian uint64_t: bits 0-23 the low 24 bits of the colour word, bits 24-36 qx, bits 37-49 qy, bits 50-62 qz,
 *      bit 63 zero.  Alpha is not carried: unpack writes 0xff000000 | rgb.
 *  K1. Per node, in fp64: ns = size * 2^-level (exact); nmin_a = (double)min_a + (double)A * ns for the node's coordinate A on axis a.
 *  K2. Points (the entry has SIMLOD_EXPORT_FLAG_LEAF): k = 8192.0 / ns, formed once per node; t = ((double)p_a - nmin_a) * k;
 *      q_a = t >= 0 ? (t < 8192 ? (uint32)t : 8191) : 0 (a NaN gives 0).  The sample is CLAMPED iff some axis fails t >= 0 && t < 8192.
 *  K3. Point decode: p'_a = (float)(nmin_a + ((double)q_a + 0.5) * (ns / 8192.0)).
 *  K4. Voxels (no SIMLOD_EXPORT_FLAG_LEAF): K2 with 128 in the place of 8192, so the fields hold values below 128 (CLAMPED likewise).  Decode is
 *      the builder's fp32 sequence for a cell centre, operation by operation: nodeSize = size / 2^level, nmin_a = ((float)A + 0.0f) * nodeSize +
 *      min_a, p'_a = nmin_a + (nodeSize * ((float)q_a + 0.5f)) / 128.0f.  A voxel is INEXACT iff a decoded coordinate differs in bits from the
 *      original; it is packed all the same.  On octrees the builder made no voxel is.
 *  K5. Which samples.  entries == NULL: per table entry with SIMLOD_EXPORT_FLAG_SELECTED the range [firstSample, firstSample + numSamples).
 *      With `entries` (SimlodDeltaEntry, same index as the table): per entry with state != SIMLOD_DELTA_NONE the range [firstDelta, firstDelta +
 *      numDelta) of the delta array.  packed[i] belongs to samples[i]: same index, same ranges; indices no range covers are not written.
 *  K6. SimlodPackCounts: numSamples packed or unpacked, numClamped, numInexact, numAlpha (samples whose top colour byte is not 0xff), error.
 *      Unpack reports numSamples and error only; the rest is 0.
 *  K7. An entry whose range reaches beyond sampleCapacity sets SIMLOD_EXPORT_ERR_CAPACITY and writes nothing (every other entry is complete, and
 *      numSamples counts those).  Too few scratch items for the pieces of all ranges set SIMLOD_EXPORT_ERR_CAPACITY too; then nothing at all is
 *      written and numSamples is 0.  An entry with level > 20 sets SIMLOD_EXPORT_ERR_NODE_COUNT and is skipped.  The table must be one this
 *      library wrote; for other content the result is unspecified, but nothing outside the given arrays is read or written.
 *  K8. Unpack masks every field to its width (13 bits; 7 for voxels) and ignores bit 63.  For a voxel node with numInexact == 0 and numAlpha == 0,
 *      unpack(pack(samples)) is the sample array byte for byte.  For a point that was not clamped |p'_a - p_a| <= ns / 16384 + ulp32(p'_a) / 2 +
 *      ns * 2^-40 (the last term covers the two fp64 roundings of K2).
 *  K9. Pack and unpack only read their inputs; they need no octree, no context and no Stats. */
#define SIMLOD_PACK_COLOR_BITS 24u
#define SIMLOD_PACK_POINT_BITS 13u     /* per axis, points */
#define SIMLOD_PACK_VOXEL_BITS 7u      /* per axis, voxels: the low bits of the same fields */
#define SIMLOD_PACK_SHIFT_X    24u
#define SIMLOD_PACK_SHIFT_Y    37u
#define SIMLOD_PACK_SHIFT_Z    50u
typedef struct SimlodPackCounts {      /* written by the device */
	uint64_t numSamples;               /* samples packed / unpacked                                                              */
	uint64_t numClamped;               /* rule K2 / K4                                                                           */
	uint64_t numInexact;               /* rule K4                                                                                */
	uint64_t numAlpha;                 /* samples whose top colour byte is not 0xff                                              */
	uint32_t error;                    /* SIMLOD_EXPORT_ERR_* bits (rule K7)                                                     */
	uint32_t reserved;                 /* 0                                                                                      */
} SimlodPackCounts;
SIMLOD_STATIC_ASSERT(sizeof(SimlodPackCounts) == 40, "PackCounts");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPackCounts, numSamples) == 0, "PackCounts.numSamples");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPackCounts, numClamped) == 8, "PackCounts.numClamped");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPackCounts, numInexact) == 16, "PackCounts.numInexact");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPackCounts, numAlpha) == 24, "PackCounts.numAlpha");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPackCounts, error) == 32, "PackCounts.error");
SIMLOD_STATIC_ASSERT(offsetof(SimlodPackCounts, reserved) == 36, "PackCounts.reserved");

/* Bytes of the `scratch` buffer the two calls below need for a table of numNodes entries whose ranges hold up to sampleBound samples: a header,
 * a word per entry and 64 bytes per piece of at most 1 000 samples. */
uint64_t simlod_pack_buffer_min_bytes(uint32_t numNodes, uint64_t sampleBound);

/* Pack (rules above) and unpack.  All pointers other than `uniforms` are device memory; asynchronous on `stream`; nothing is allocated,
 * synchronised or copied.  `samples` / `packed` have sampleCapacity records.  hipErrorInvalidValue with nothing enqueued: a null pointer other
 * than `entries`, numNodes == 0, a box that is not finite or has no extent, scratchBytes below simlod_pack_buffer_min_bytes(numNodes, 0). */
int simlod_pack_samples(const SimlodUniforms* uniforms /*host*/, const SimlodExportNode* table, const SimlodDeltaEntry* entries /*or NULL*/,
                        uint32_t numNodes, const SimlodPoint* samples, uint64_t sampleCapacity, void* scratch, uint64_t scratchBytes,
                        uint64_t* packed, SimlodPackCounts* counts, void* stream);
int simlod_unpack_samples(const SimlodUniforms* uniforms /*host*/, const SimlodExportNode* table, const SimlodDeltaEntry* entries /*or NULL*/,
                          uint32_t numNodes, const uint64_t* packed, uint64_t sampleCapacity, void* scratch, uint64_t scratchBytes,
                          SimlodPoint* samples, SimlodPackCounts* counts, void* stream);

/* ---- compare queries: each sample's distance to the nearest sample of another cloud -----------------------------------------------------------
 * simlod_compare_samples relates TWO sample arrays: for every sample of `a` the nearest sample of `b` within a radius, how many samples of `b`
 * lie within that radius, a colour looked up from the squared distance, and one summary record with the histogram of those distances.  With
 * b == a the same call gives the local density (`within`).  `a` and `b` are flat device arrays of the 16-byte sample — the `samples` of any
 * export, query, view or unpack result —; the call knows nothing of octrees.  Both arrays are only read.  The search runs on a hash grid over `b`
 * whose cell is as large as the radius asks for; what the grid lets the kernels skip never changes a result (rule C4).
 *
 * All fp64 arithmetic works from the fp32 inputs, without fused multiply-add, every sum in the order written here.  Each field is defined by
 * its rule alone, whatever work the kernels skip.
 *  C1. Valid samples.  A sample is valid iff its x, y and z are finite.  An invalid sample of `b` is never a neighbour and is counted in
 *      numInvalidB.  An invalid sample of `a` gets the miss record and missColor, lands in hist[256] and is counted in numInvalidA.  The radius
 *      must be finite and >= 0; radius 0 is valid and matches coincident samples only.
 *  C2. The sample test (neighbour-query rule 2).  With p_a = s_a - c_a per component of the sample s of `b` and the sample c of `a`,
 *      d2 = (px*px + py*py) + pz*pz and rr = (double)r * (double)r; the sample passes iff d2 <= rr.
 *  C3. The result.  Over the valid samples of `b` that pass for a valid a[i]: within[i] is their number, nearest[i] the first of them in the
 *      total order (d2, index in `b`), d2[i] that sample's d2.  With none passing the record is the MISS record: d2 = +infinity,
 *      nearest = 0xffffffff, within = 0.  A sample compared with its own cloud finds itself at d2 = 0; of duplicates the lowest index wins.
 *  C4. The grid.  h = max((double)r * (1 + 2^-10), (double)size * 2^-20) with `size` the largest fp32 extent of the uniforms' box and
 *      min = boxMin (a size that is not finite or not > 0, or a boxMin that is not finite, is refused); inv = 1.0 / h, one IEEE division made
 *      by the launcher on the host.  A valid sample's cell is, per axis, summary rule S2's c20 with this inv in the place of that rule's:
 *      t = ((double)x - (double)min) * inv, cell = 1048575 if t >= 1048575.0, (uint32_t)t if t > 0.0, else 0.  Coordinates outside the box
 *      clamp to the edge cells, so `b` need not share `a`'s box.  numCells is the number of distinct cells that hold a valid sample of `b`,
 *      maxCellPopulation the largest number of valid samples of `b` in one cell, numCandidates the sum, over the valid samples of `a`, of the
 *      populations of the up to 27 cells at per-axis offsets -1, 0, +1 from the sample's cell; an offset that leaves [0, 2^20) is skipped, not
 *      clamped.  Only those cells are searched, and for finite samples that never changes rule C3: two samples with d2 <= rr differ by at most
 *      r * (1 + 2^-52) on each axis (a square is monotone under IEEE rounding and the sums only add non-negative terms), so their t differ by
 *      less than r * (1 + 2^-52) / (r * (1 + 2^-10)) < 1 - 2^-11 plus the rounding of the two products, at most 2^-31 each inside the clamp
 *      range (t < 2^20, 53-bit significands); truncation then puts them into the same cell or into adjacent ones, and the clamp, being
 *      monotone, never moves two cells further apart.  With h at its floor size * 2^-20 the radius is smaller still and the same holds.
 *  C5. Colours and histogram.  For a matched sample i = the number of entries of thresholds2 that are <= d2 (0 .. 255; the 255 entries are
 *      ascending — each >= the one before — and finite; a binary search, no square root is taken anywhere): colors[j] = table[i] and hist[i]
 *      counts it.  An unmatched or invalid sample of `a` gets missColor and hist[256].
 *  C6. The budget.  With maxCandidates != 0 and numCandidates > maxCandidates no sample is tested: error = SIMLOD_COMPARE_ERR_BUDGET, no
 *      record and no colour is written, numMatched = numWithin = 0, maxD2 = 0 and hist is all zero; the other fields are complete.  (A radius
 *      that puts all of `b` into a few cells would otherwise launch numA x numB tests.)
 *  C7. Count only.  records == NULL (then colors must be NULL too): the grid is built and error, numCells, maxCellPopulation, numCandidates,
 *      numInvalidA and numInvalidB are written as above; no distance is computed, numMatched = numWithin = 0, maxD2 = 0, hist all zero.
 *  C8. Determinism.  Everything returned is a sum of integers, a maximum, or the minimum of a total order: a pure function of the two arrays
 *      and the parameters, independent of the schedule, of maxWorkgroups and of where the hash table puts a cell.  Two calls give the same
 *      bytes.
 * Nothing is written but `scratch`, `records`, `colors` and `summary`.  `a` and `b` may be the same array. */
#define SIMLOD_COMPARE_ERR_BUDGET 0x1u
#define SIMLOD_COMPARE_MISS       0xffffffffu
typedef struct SimlodCompareRecord {   /* DEVICE memory, one per sample of `a`, same index */
	double   d2;                       /* rule C3; miss: +infinity                                              */
	uint32_t nearest;                  /* index into `b`; miss: 0xffffffff                                      */
	uint32_t within;                   /* valid samples of `b` that pass rule C2                                */
} SimlodCompareRecord;
typedef struct SimlodCompareParams {   /* host memory; read completely before the call returns */
	float    radius;                   /* finite, >= 0                                                          */
	uint32_t missColor;                /* rule C5                                                               */
	uint64_t maxCandidates;            /* rule C6; 0: no limit                                                  */
	double   thresholds2[255];         /* rule C5: squared distances, ascending, finite                         */
	uint32_t table[256];               /* rule C5                                                               */
	uint32_t maxWorkgroups;            /* 0: the library's choice; else no kernel launches more workgroups      */
	uint32_t reserved;                 /* 0                                                                     */
} SimlodCompareParams;
typedef struct SimlodCompareSummary {  /* written by the device */
	uint32_t error;                    /* SIMLOD_COMPARE_ERR_* bits                                             */
	uint32_t numCells;                 /* rule C4                                                               */
	uint32_t maxCellPopulation;        /* rule C4                                                               */
	uint32_t numInvalidA;              /* rule C1                                                               */
	uint32_t numInvalidB;              /* rule C1                                                               */
	uint32_t numMatched;               /* samples of `a` with within > 0                                        */
	uint64_t numWithin;                /* the sum of within                                                     */
	uint64_t numCandidates;            /* rule C4                                                               */
	double   maxD2;                    /* the largest matched d2; 0 when none matched                           */
	uint64_t hist[257];                /* rule C5; [256]: unmatched and invalid samples of `a`                  */
} SimlodCompareSummary;
SIMLOD_STATIC_ASSERT(sizeof(SimlodCompareRecord) == 16, "CompareRecord");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareRecord, nearest) == 8, "CompareRecord.nearest");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareRecord, within) == 12, "CompareRecord.within");
SIMLOD_STATIC_ASSERT(sizeof(SimlodCompareParams) == 3088, "CompareParams");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareParams, missColor) == 4, "CompareParams.missColor");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareParams, maxCandidates) == 8, "CompareParams.maxCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareParams, thresholds2) == 16, "CompareParams.thresholds2");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareParams, table) == 2056, "CompareParams.table");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareParams, maxWorkgroups) == 3080, "CompareParams.maxWorkgroups");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareParams, reserved) == 3084, "CompareParams.reserved");
SIMLOD_STATIC_ASSERT(sizeof(SimlodCompareSummary) == 2104, "CompareSummary");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, numCells) == 4, "CompareSummary.numCells");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, maxCellPopulation) == 8, "CompareSummary.maxCellPopulation");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, numInvalidA) == 12, "CompareSummary.numInvalidA");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, numInvalidB) == 16, "CompareSummary.numInvalidB");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, numMatched) == 20, "CompareSummary.numMatched");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, numWithin) == 24, "CompareSummary.numWithin");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, numCandidates) == 32, "CompareSummary.numCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, maxD2) == 40, "CompareSummary.maxD2");
SIMLOD_STATIC_ASSERT(offsetof(SimlodCompareSummary, hist) == 48, "CompareSummary.hist");

/* Bytes of the `scratch` buffer a compare call needs; it depends on the two counts only (in fact on numB): a header, the hash table (16 bytes
 * per slot), 12 bytes and one 16-byte grid record per sample of `b`, and the partial records of the largest grid the library ever chooses.
 * There is no capacity error on the device.  0 for counts the call refuses. */
uint64_t simlod_compare_buffer_min_bytes(uint64_t numA, uint64_t numB);
/* The hash table's capacity: the smallest power of two >= 2 * numB (0 for a numB the call refuses). */
uint64_t simlod_compare_table_slots(uint64_t numB);

/* The compare query (rules above).  Asynchronous on `stream` once `uniforms` and `params` have been read.  hipErrorInvalidValue with nothing
 * enqueued and nothing touched: a null pointer other than `records` / `colors`; colors != NULL while records == NULL; numA or numB equal to 0
 * or >= 2^32 - 1; a radius that is not finite or < 0; a box whose boxMin is not finite or whose size is not finite or not > 0; thresholds2 not
 * ascending or not finite; a nonzero `reserved`; scratchBytes below simlod_compare_buffer_min_bytes(numA, numB) (one byte less is refused, the
 * exact size is accepted); `a`, `b`, `scratch` or `records` not 16-byte aligned, `colors` not 4-byte aligned, `summary` not 8-byte aligned. */
int simlod_compare_samples(const SimlodUniforms* uniforms /*host*/, const SimlodPoint* a, uint64_t numA, const SimlodPoint* b, uint64_t numB,
                           const SimlodCompareParams* params /*host*/, void* scratch, uint64_t scratchBytes,
                           SimlodCompareRecord* records /*or NULL: count only*/, uint32_t* colors /*or NULL*/,
                           SimlodCompareSummary* summary, void* stream);

/* ---- surface queries: each sample's normal and roughness from its neighbours --------------------------------------------------------------------
 * simlod_surface_samples fits a least-squares plane through the samples of `b` within a radius of every sample of `a` (b == a is the usual
 * case): the plane's unnormalised normal, the two numbers whose quotient is the surface variation l1 / (l1 + l2 + l3) of the neighbourhood's
 * covariance (eigenvalues l1 <= l2 <= l3; 0 on a plane, 1/3 for an isotropic blob), `within`, and a colour from a 256-entry table indexed by
 * a hillshade (the Lambert term against a light direction) or by the variation.  It runs on the compare queries' hash grid over `b`, built
 * by the same kernels in the same scratch layout; the arrays, the box and the grid's fields of the summary mean what they mean there.
 *
 * No division and no square root run on the device: every device operation is an fp64 add, subtract, multiply or compare, an integer
 * operation, a conversion, or an exact scaling by a power of two, without fused multiply-add, every sum in the order written here.  fp64
 * SUBNORMALS ARE NOT FLUSHED, on the device or in the host mirror: rule N4 multiplies small entries by a power of two that may leave them
 * subnormal and relies on IEEE gradual underflow giving the same bits on both sides.  A symmetric 3x3 matrix is its six entries xx, xy, xz,
 * yy, yz, zz.
 *  N1. Neighbourhood.  Rules C1, C2 and C4 hold with this record's radius: the valid samples, the test d2 <= rr, and the grid — h, inv, the
 *      up to 27 cells, numCells, maxCellPopulation, numCandidates and numInvalidB are the compare query's, and so are its refusals.
 *  N2. Quantised offsets.  invq = 16384.0 / h, one IEEE division made by the launcher on the host.  For a sample s of `b` that passes for
 *      the sample c of `a`, per axis q = (int32_t)(p * invq) with p = (double)s - (double)c as in rule C2, truncated towards zero.
 *      |p| <= r * (1 + 2^-52) < h (rule C4's argument), so |q| <= 16384.
 *  N3. Sums.  Per sample of `a` nine signed 64-bit sums over the passing samples: Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz of q and of the
 *      products of two q (each <= 2^28: an int32; with fewer than 2^32 neighbours every sum stays below 2^60).  They are integers: they
 *      depend neither on the order of visiting nor on where the hash table put a cell.  D(S) = (double)(int32_t)(S >> 32) * 4294967296.0 +
 *      (double)(uint32_t)S — an arithmetic shift, an exact product and one rounded add —, n = (double)within, and for the six entries
 *      M_uv = n * D(S_uv) - D(S_u) * D(S_v): n^2 times the covariance of the quantised offsets, with no division.
 *  N4. The scaling P of a symmetric matrix.  m = the largest |x| of its six entries, e = the 11 exponent bits of m, f = the double whose
 *      bits are (uint64_t)(2046 - e) << 52, i.e. 2^(1023 - e); every entry is multiplied by f — exact for the largest, which lands in
 *      [1, 2) (in [2^-51, 2) when m itself is subnormal), IEEE-rounded for an entry that becomes subnormal.  m == 0 makes the sample
 *      degenerate (rule N9).
 *  N5. The normal.  M <- P(M); t = (Mxx + Myy) + Mzz; B = t*I - M (diagonal entries t - M_uu, the others -M_uv, a change of sign): the
 *      eigenvector of M's smallest eigenvalue is B's dominant one.  Eight times B <- P(B*B), each entry (Bi0*B0j + Bi1*B1j) + Bi2*B2j for
 *      i <= j, the matrix kept symmetric.  j* = the FIRST index of the largest diagonal entry of the result, v = its column j*.  Eight
 *      squarings raise the eigenvalue ratio to the 256th power: with g = (l2 - l1) / (l2 + l3) >= 1/8 the other eigenvectors' share of v is
 *      at most (7/8)^256 = 1.4e-15.
 *  N6. Orientation.  orientMode SIMLOD_SURFACE_ORIENT_DIRECTION: o = `orient`, widened; SIMLOD_SURFACE_ORIENT_POSITION (a sensor's
 *      position): o = (double)orient - (double)c per axis.  s = (vx*ox + vy*oy) + vz*oz; s < 0 negates v, s == 0 keeps it (so a zero
 *      `orient` direction never flips).  normal[k] = (float)v[k], rounded to nearest.
 *  N7. Variation.  w = M*v, w_i = (Mi0*v0 + Mi1*v1) + Mi2*v2 with the scaled M and the oriented v; lambdaNum = (v0*w0 + v1*w1) + v2*w2,
 *      vv = (v0*v0 + v1*v1) + v2*v2, lambdaDen = vv * t.  Both go into the record; the host divides.
 *  N8. Colour index.  colourBy SIMLOD_SURFACE_SHADE: a = (vx*Lx + vy*Ly) + vz*Lz with L = `light`, widened (finite, not all zero),
 *      num = a * fabs(a), den = vv * ((Lx*Lx + Ly*Ly) + Lz*Lz): the thresholds are signed squared cosines in [-1, 1].
 *      SIMLOD_SURFACE_VARIATION: num = lambdaNum, den = lambdaDen: the thresholds are variations in [0, 1].  The index (0 .. 255) is the
 *      number of the 255 thresholds (finite, ascending: each >= the one before) with thresholds[i] * den <= num, found by binary search —
 *      den >= 0 and IEEE rounding is monotone, so the products ascend with the thresholds.  colors[i] = table[index]; hist[index] counts it.
 *  N9. Degenerate and invalid samples.  A valid sample of `a` is degenerate when within < 3 or rule N4 finds m == 0, for M or for any of
 *      the eight B: normal 0, lambdaNum = lambdaDen = 0, its true `within`, missColor, hist[256], counted in numDegenerate.  An invalid
 *      sample of `a` gets the same record with within = 0 and is counted in numInvalidA, not in numDegenerate.  Every other sample is
 *      counted in numEstimated; numWithin is the sum of every record's `within`.
 * N10. Budget, count only, determinism.  Rules C6 and C7 hold with SIMLOD_SURFACE_ERR_BUDGET (numEstimated = numDegenerate = numWithin = 0
 *      and hist all zero where no sample is tested).  Rule C8 holds and is stronger here: no index of `b` enters a record, so a record does
 *      not depend on the order of `b` at all.
 * Nothing is written but `scratch`, `records`, `colors` and `summary`.  `a` and `b` may be the same array. */
#define SIMLOD_SURFACE_ERR_BUDGET       0x1u
#define SIMLOD_SURFACE_SHADE            0u
#define SIMLOD_SURFACE_VARIATION        1u
#define SIMLOD_SURFACE_ORIENT_DIRECTION 0u
#define SIMLOD_SURFACE_ORIENT_POSITION  1u
typedef struct SimlodSurfaceRecord {   /* DEVICE memory, one per sample of `a`, same index */
	float    normal[3];                /* rules N5, N6: unnormalised; degenerate or invalid: 0                  */
	uint32_t within;                   /* valid samples of `b` that pass rule C2                                */
	double   lambdaNum;                /* rule N7                                                               */
	double   lambdaDen;                /* rule N7; variation = lambdaNum / lambdaDen                            */
} SimlodSurfaceRecord;
typedef struct SimlodSurfaceParams {   /* host memory; read completely before the call returns */
	float    radius;                   /* finite, >= 0                                                          */
	uint32_t missColor;                /* rule N9                                                               */
	uint64_t maxCandidates;            /* rule C6; 0: no limit                                                  */
	double   thresholds[255];          /* rule N8: ascending, finite                                            */
	uint32_t table[256];               /* rule N8                                                               */
	float    light[3];                 /* rule N8: finite; not all zero with SIMLOD_SURFACE_SHADE               */
	float    orient[3];                /* rule N6: finite                                                       */
	uint32_t colourBy;                 /* SIMLOD_SURFACE_SHADE or SIMLOD_SURFACE_VARIATION                      */
	uint32_t orientMode;               /* SIMLOD_SURFACE_ORIENT_DIRECTION or SIMLOD_SURFACE_ORIENT_POSITION     */
	uint32_t maxWorkgroups;            /* 0: the library's choice; else no kernel launches more workgroups      */
	uint32_t reserved;                 /* 0                                                                     */
} SimlodSurfaceParams;
typedef struct SimlodSurfaceSummary {  /* written by the device; SimlodCompareSummary's layout, field for field */
	uint32_t error;                    /* SIMLOD_SURFACE_ERR_* bits                                             */
	uint32_t numCells;                 /* rule C4                                                               */
	uint32_t maxCellPopulation;        /* rule C4                                                               */
	uint32_t numInvalidA;              /* rule C1                                                               */
	uint32_t numInvalidB;              /* rule C1                                                               */
	uint32_t numEstimated;             /* samples of `a` with a normal                                          */
	uint64_t numWithin;                /* the sum of within                                                     */
	uint64_t numCandidates;            /* rule C4                                                               */
	uint64_t numDegenerate;            /* rule N9                                                               */
	uint64_t hist[257];                /* rule N8; [256]: degenerate and invalid samples of `a`                 */
} SimlodSurfaceSummary;
SIMLOD_STATIC_ASSERT(sizeof(SimlodSurfaceRecord) == 32, "SurfaceRecord");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceRecord, within) == 12, "SurfaceRecord.within");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceRecord, lambdaNum) == 16, "SurfaceRecord.lambdaNum");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceRecord, lambdaDen) == 24, "SurfaceRecord.lambdaDen");
SIMLOD_STATIC_ASSERT(sizeof(SimlodSurfaceParams) == 3120, "SurfaceParams");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, missColor) == 4, "SurfaceParams.missColor");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, maxCandidates) == 8, "SurfaceParams.maxCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, thresholds) == 16, "SurfaceParams.thresholds");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, table) == 2056, "SurfaceParams.table");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, light) == 3080, "SurfaceParams.light");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, orient) == 3092, "SurfaceParams.orient");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, colourBy) == 3104, "SurfaceParams.colourBy");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, orientMode) == 3108, "SurfaceParams.orientMode");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, maxWorkgroups) == 3112, "SurfaceParams.maxWorkgroups");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceParams, reserved) == 3116, "SurfaceParams.reserved");
SIMLOD_STATIC_ASSERT(sizeof(SimlodSurfaceSummary) == sizeof(SimlodCompareSummary), "SurfaceSummary");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, numCells) == 4, "SurfaceSummary.numCells");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, maxCellPopulation) == 8, "SurfaceSummary.maxCellPopulation");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, numInvalidA) == 12, "SurfaceSummary.numInvalidA");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, numInvalidB) == 16, "SurfaceSummary.numInvalidB");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, numEstimated) == offsetof(SimlodCompareSummary, numMatched), "SurfaceSummary.numEstimated");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, numWithin) == 24, "SurfaceSummary.numWithin");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, numCandidates) == 32, "SurfaceSummary.numCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, numDegenerate) == offsetof(SimlodCompareSummary, maxD2), "SurfaceSummary.numDegenerate");
SIMLOD_STATIC_ASSERT(offsetof(SimlodSurfaceSummary, hist) == 48, "SurfaceSummary.hist");

/* Bytes of the `scratch` buffer a surface call needs: simlod_compare_buffer_min_bytes(numA, numB), the layout is the compare call's. */
uint64_t simlod_surface_buffer_min_bytes(uint64_t numA, uint64_t numB);

/* The surface query (rules above).  Asynchronous on `stream` once `uniforms` and `params` have been read.  hipErrorInvalidValue with nothing
 * enqueued and nothing touched: everything simlod_compare_samples refuses (null pointers, colors without records, the counts, the radius, the
 * box, thresholds not ascending or not finite, `reserved`, scratchBytes one byte short, the alignments — `records` at 16 bytes); a colourBy
 * or an orientMode out of range; a `light` or an `orient` that is not finite; a zero `light` with SIMLOD_SURFACE_SHADE. */
int simlod_surface_samples(const SimlodUniforms* uniforms /*host*/, const SimlodPoint* a, uint64_t numA, const SimlodPoint* b, uint64_t numB,
                           const SimlodSurfaceParams* params /*host*/, void* scratch, uint64_t scratchBytes,
                           SimlodSurfaceRecord* records /*or NULL: count only*/, uint32_t* colors /*or NULL*/,
                           SimlodSurfaceSummary* summary, void* stream);

/* ---- cluster queries: each sample's connected component within a radius ------------------------------------------------------------------------
 * simlod_cluster_samples relates ONE sample array to itself: the samples that can be reached from one another in steps of at most a radius
 * form a cluster.  With minNeighbours > 1 only samples with that many samples around them carry a step (the density rule of DBSCAN), so a
 * thin bridge of stray samples joins nothing.  Per sample it returns the cluster's number, its root (the lowest index of its cores), its size
 * and `within`, a colour from a 256-entry table indexed by the cluster's number, and one summary record.  It runs on the compare queries' hash
 * grid over `a`, built by the same kernels; the array, the box and the grid's fields of the summary mean what they mean there.  Every number
 * returned is an integer.
 *  K1. Valid samples, the test, the grid.  Rules C1, C2 and C4 hold with this record's radius and b = a: the valid samples, the test
 *      d2 <= rr, and the grid — h, inv, the up to 27 cells, numCells, maxCellPopulation, numCandidates, and the compare query's refusals.
 *  K2. Budget and count only.  Rules C6 and C7 hold with SIMLOD_CLUSTER_ERR_BUDGET: where no sample is tested every field of the summary
 *      past numCandidates is zero and no record and no colour is written.
 *  K3. Core.  within[i] is the number of valid samples j of `a`, i itself included, with d2 <= rr (rule C2).  A valid sample is a CORE iff
 *      within[i] >= minNeighbours.  minNeighbours must be >= 1; 1 makes every valid sample a core, which is plain Euclidean clustering
 *      (single linkage at the radius).  Rule C2's d2 is symmetric bit for bit: s - c and c - s are exact negations of each other, their
 *      squares are equal and the sums are taken in the same order, so "i is within r of j" does not depend on which of the two asks.
 *  K4. Components.  Two cores are linked iff their d2 <= rr.  A cluster is a connected component of the cores under these links; its
 *      `root` is the lowest index in `a` of its cores.
 *  K5. Border and noise.  A valid sample that is no core, with at least one core passing rule C2, is a BORDER sample of the cluster of the
 *      first such core in the total order (d2, index) — rule C3's order.  It links nothing: two clusters that share a border sample stay
 *      two.  With no core passing the sample is noise.  An invalid sample is noise with within = 0.
 *  K6. Sizes.  A cluster's size is the number of its cores plus the number of its border samples.
 *  K7. Small clusters.  A cluster whose size is below minClusterSize (>= 1; 1 keeps all) is DISSOLVED: its members keep `root` and `size`
 *      and get cluster = SIMLOD_CLUSTER_NOISE, so root != SIMLOD_CLUSTER_MISS tells a dissolved sample from true noise.
 *  K8. Numbers.  The kept clusters are numbered 0 .. numClusters - 1 in ascending order of `root`.
 *  K9. Record, colour, summary.  A member of a cluster: {cluster, root, size, within}; true noise: {SIMLOD_CLUSTER_NOISE,
 *      SIMLOD_CLUSTER_MISS, 0, within}.  colors[i] = table[cluster & 255] for a sample of a kept cluster, noiseColor for every other.
 *      numClusters: the kept clusters; numDissolved: the dissolved ones; numCore and numBorder: the cores and the border samples of the
 *      KEPT clusters; numNoise: every other sample — true noise, the members of dissolved clusters and the invalid samples —, so that
 *      numCore + numBorder + numNoise = numA; numWithin: the sum of within; largestSize: the largest size of a kept cluster (0 with none),
 *      largestCluster: the lowest number among the clusters of that size (0 with none); sizeHist[k]: the kept clusters with
 *      floor(log2(size)) = k.  numInvalidB repeats numInvalidA: the grid is over `a` itself.
 * K10. Determinism.  Rule C8 holds: every field is a sum of integers, a maximum, or the minimum of a total order — a root is the minimum of
 *      a set of indices, a number the rank of a root —: a pure function of the array and the parameters, independent of the schedule, of
 *      maxWorkgroups and of where the hash table puts a cell.  Two calls give the same bytes.  The union-find that finds the components
 *      bounds every loop by a number known at launch; should a bound ever be reached the call stops there and sets
 *      SIMLOD_CLUSTER_ERR_INTERNAL, with records that mean nothing.  No input is known that does it.
 * Nothing is written but `scratch`, `records`, `colors` and `summary`. */
#define SIMLOD_CLUSTER_ERR_BUDGET   0x1u
#define SIMLOD_CLUSTER_ERR_INTERNAL 0x2u
#define SIMLOD_CLUSTER_NOISE        0xffffffffu
#define SIMLOD_CLUSTER_MISS         0xffffffffu
#define SIMLOD_CLUSTER_SIZE_BINS    33
typedef struct SimlodClusterRecord {   /* DEVICE memory, one per sample of `a`, same index */
	uint32_t cluster;                  /* rule K8; SIMLOD_CLUSTER_NOISE: noise or dissolved                     */
	uint32_t root;                     /* rule K4; SIMLOD_CLUSTER_MISS: true noise                              */
	uint32_t size;                     /* rule K6; 0: true noise                                                */
	uint32_t within;                   /* rule K3                                                               */
} SimlodClusterRecord;
typedef struct SimlodClusterParams {   /* host memory; read completely before the call returns */
	float    radius;                   /* finite, >= 0                                                          */
	uint32_t minNeighbours;            /* rule K3; >= 1                                                         */
	uint32_t minClusterSize;           /* rule K7; >= 1                                                         */
	uint32_t noiseColor;               /* rule K9                                                               */
	uint64_t maxCandidates;            /* rule C6; 0: no limit                                                  */
	uint32_t table[256];               /* rule K9                                                               */
	uint32_t maxWorkgroups;            /* 0: the library's choice; else no kernel launches more workgroups      */
	uint32_t reserved;                 /* 0                                                                     */
} SimlodClusterParams;
typedef struct SimlodClusterSummary {  /* written by the device; SimlodCompareSummary's size, its leading fields at their offsets */
	uint32_t error;                    /* SIMLOD_CLUSTER_ERR_* bits                                             */
	uint32_t numCells;                 /* rule C4                                                               */
	uint32_t maxCellPopulation;        /* rule C4                                                               */
	uint32_t numInvalidA;              /* rule C1                                                               */
	uint32_t numInvalidB;              /* = numInvalidA                                                         */
	uint32_t numClusters;              /* rule K8                                                               */
	uint64_t numWithin;                /* the sum of within                                                     */
	uint64_t numCandidates;            /* rule C4                                                               */
	uint64_t numCore;                  /* rule K9                                                               */
	uint64_t numBorder;                /* rule K9                                                               */
	uint64_t numNoise;                 /* rule K9                                                               */
	uint64_t numDissolved;             /* rule K7: clusters, not samples                                        */
	uint32_t largestSize;              /* rule K9                                                               */
	uint32_t largestCluster;           /* rule K9                                                               */
	uint64_t sizeHist[SIMLOD_CLUSTER_SIZE_BINS];   /* rule K9                                                   */
	uint64_t zero[220];                /* 0                                                                     */
} SimlodClusterSummary;
SIMLOD_STATIC_ASSERT(sizeof(SimlodClusterRecord) == 16, "ClusterRecord");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterRecord, within) == 12, "ClusterRecord.within");
SIMLOD_STATIC_ASSERT(sizeof(SimlodClusterParams) == 1056, "ClusterParams");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterParams, maxCandidates) == 16, "ClusterParams.maxCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterParams, table) == 24, "ClusterParams.table");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterParams, maxWorkgroups) == 1048, "ClusterParams.maxWorkgroups");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterParams, reserved) == 1052, "ClusterParams.reserved");
SIMLOD_STATIC_ASSERT(sizeof(SimlodClusterSummary) == sizeof(SimlodCompareSummary), "ClusterSummary");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, error) == offsetof(SimlodCompareSummary, error), "ClusterSummary.error");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, numCells) == offsetof(SimlodCompareSummary, numCells), "ClusterSummary.numCells");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, maxCellPopulation) == offsetof(SimlodCompareSummary, maxCellPopulation), "ClusterSummary.maxCellPopulation");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, numInvalidA) == offsetof(SimlodCompareSummary, numInvalidA), "ClusterSummary.numInvalidA");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, numInvalidB) == offsetof(SimlodCompareSummary, numInvalidB), "ClusterSummary.numInvalidB");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, numClusters) == offsetof(SimlodCompareSummary, numMatched), "ClusterSummary.numClusters");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, numWithin) == offsetof(SimlodCompareSummary, numWithin), "ClusterSummary.numWithin");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, numCandidates) == offsetof(SimlodCompareSummary, numCandidates), "ClusterSummary.numCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, numCore) == offsetof(SimlodCompareSummary, maxD2), "ClusterSummary.numCore");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, numBorder) == offsetof(SimlodCompareSummary, hist), "ClusterSummary.numBorder");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, largestSize) == 72, "ClusterSummary.largestSize");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, sizeHist) == 80, "ClusterSummary.sizeHist");
SIMLOD_STATIC_ASSERT(offsetof(SimlodClusterSummary, zero) == 344, "ClusterSummary.zero");

/* Bytes of the `scratch` buffer a cluster call needs, a pure function of numA: simlod_compare_buffer_min_bytes(numA, numA), five 32-bit words
 * per sample (within, parent, attach / root, size, number; each array rounded up to 16 bytes) and the partial records of the largest grid.
 * 0 for a count the call refuses. */
uint64_t simlod_cluster_buffer_min_bytes(uint64_t numA);

/* The cluster query (rules above).  Asynchronous on `stream` once `uniforms` and `params` have been read.  hipErrorInvalidValue with nothing
 * enqueued and nothing touched: everything simlod_compare_samples refuses of its arguments with b = a (null pointers, colors without
 * records, the count, the radius, the box, `reserved`, the alignments — `records` at 16 bytes); minNeighbours == 0; minClusterSize == 0;
 * scratchBytes below simlod_cluster_buffer_min_bytes(numA) (one byte less is refused, the exact size is accepted). */
int simlod_cluster_samples(const SimlodUniforms* uniforms /*host*/, const SimlodPoint* a, uint64_t numA,
                           const SimlodClusterParams* params /*host*/, void* scratch, uint64_t scratchBytes,
                           SimlodClusterRecord* records /*or NULL: count only*/, uint32_t* colors /*or NULL*/,
                           SimlodClusterSummary* summary, void* stream);

/* ---- align queries: the rigid motion that fits one cloud onto another -------------------------------------------------------------------------
 * simlod_align_samples is one step of a registration by ICP (iterative closest point): every sample of `a` is moved by a pose, its nearest
 * sample of `b` within a radius is found as the compare query finds it, and over the matched pairs the call returns the exact integer sums
 * a least-squares rigid fit needs — the two centroids, the nine cross moments and the squared residual.  The host solves the 3x3 problem
 * (simlod_amd/octree_io.py align_solve) and calls again with the updated pose.  `b` does not move between steps, so the hash grid over it
 * is built by the first call and REUSED by the later ones (rule A7), which launch the test pass alone.  The arrays, the box, the scratch
 * layout and the grid's fields of the summary mean what they mean for the compare query; the scratch buffer is that query's with one more
 * array of partial records behind it.
 *
 * All fp64 arithmetic runs without fused multiply-add, every sum in the order written here.  Each field is defined by its rule alone,
 * whatever work the kernels skip.
 *  A1. Pose.  `pose` is a 3x4 matrix T, row-major; all 12 entries must be finite or the call is refused.  For a sample c of `a`, widened
 *      to fp64: c'_k = ((T_k0*cx + T_k1*cy) + T_k2*cz) + T_k3.  A sample of `a` is valid iff its x, y and z are finite AND all three c'_k
 *      are finite (a product can overflow); an invalid one gets the miss record and counts in numInvalidA.  Rule C1 holds unchanged for `b`.
 *  A2. The grid.  Rule C4 holds with gridRadius in the place of the radius: h = max((double)gridRadius * (1 + 2^-10), (double)size * 2^-20),
 *      inv = 1.0 / h.  gridRadius must be finite and >= radius, or the call is refused: one grid serves every smaller radius, so an ICP may
 *      tighten its radius between steps without a new build.  The cell of c' is, per axis, C4's clamp applied to t = (c'_k - min_k) * inv:
 *      1048575 if t >= 1048575.0, (uint32_t)t if t > 0.0, else 0.  The up to 27 cells around it are searched, and that never changes rule
 *      A3: here p = s - c' is a ROUNDED subtraction, but d2 <= rr still bounds |p_k| by r * (1 + 2^-52) (C4's argument), the true
 *      difference is p_k * (1 + e) with |e| <= 2^-53, so |s_k - c'_k| < r * (1 + 2^-51); with r <= gridRadius the two t differ by less than
 *      (1 + 2^-51) / (1 + 2^-10) < 1 - 2^-11 plus the roundings of the two subtractions from min and of the two products, each at most
 *      2^-31 inside the clamp range: less than 1, so truncation puts them into the same cell or into adjacent ones, and the clamp never
 *      moves two cells further apart.  The factor 1 + 2^-10 covers it; with h at its floor the radius is smaller still.
 *  A3. Test and result.  p = (double)s - c' per component, d2 = (px*px + py*py) + pz*pz; a sample of `b` passes iff
 *      d2 <= (double)radius * (double)radius.  within, nearest and d2 follow rule C3 in the order (d2, index in `b`).  The record is
 *      SimlodCompareRecord and the miss record is the compare query's.
 *  A4. Quantisation.  invQ = 16777216.0 / (double)size, one IEEE division made by the launcher on the host.  For a double x on axis k:
 *      t = (x - min_k) * invQ; x is INSIDE iff t >= 0.0 && t < 16777216.0, and then Q = (uint32_t)t (24 bits).  A matched pair
 *      (c', s = b[nearest]) is SUMMED iff all six coordinates are inside; a matched pair that is not summed counts in numOutside.
 *  A5. Sums over the summed pairs.  numSummed is their number; sumA[k] = sum of Q(c'_k), sumB[k] = sum of Q(s_k).  For the product
 *      P = Q(c'_k) * Q(s_l) < 2^48: crossLo[3k+l] = sum of (P & 0xffffffff), crossHi[3k+l] = sum of (P >> 32).  With
 *      e_k = (int64)Q(s_k) - (int64)Q(c'_k) and E = (e_x*e_x + e_y*e_y) + e_z*e_z < 2^50: sqLo = sum of (E & 0xffffffff),
 *      sqHi = sum of (E >> 32).  With fewer than 2^32 pairs no word overflows: every term is below 2^32.  The host reads hi * 2^32 + lo
 *      as an integer of any size.
 *  A6. Budget, count only.  Rule C6 holds with SIMLOD_ALIGN_ERR_BUDGET: no sample is tested, no record is written, and every field after
 *      numCandidates is zero.  SIMLOD_ALIGN_COUNT_ONLY gives the grid's fields only, as rule C7 does.  records == NULL WITHOUT that flag
 *      is a full call that writes no records: the ICP's normal case.
 *  A7. Grid reuse.  A call without SIMLOD_ALIGN_REUSE_GRID builds the grid with the compare query's kernels and then writes a STAMP into
 *      the unused words of the scratch buffer's header: a magic number, the pointer `b`, numB, the bits of inv and of min[3], whether the
 *      grid records were filled (a count-only build fills none), and the grid's totals numCells, maxCellPopulation and numInvalidB.  A
 *      call WITH the flag builds nothing; every kernel it launches compares the stamp with its own arguments before its first read of the
 *      table.  On a mismatch — another `b` or numB, another box or gridRadius, a scratch buffer no build call stamped, a full call on a
 *      grid a count-only build left unfilled — nothing of the table or the grid records is read, no record is written,
 *      error = SIMLOD_ALIGN_ERR_GRID and every other field of the summary is zero.  The grid's totals of a reuse call come from the
 *      stamp, so maxWorkgroups may differ between the calls.  The caller must not have changed `b` or the scratch buffer between the
 *      build call and the reuse call: the stamp names the array, it does not hash it.  Every other call of this header that takes a
 *      scratch buffer neither writes a stamp nor honours one (the compare, surface and cluster calls clear it).
 *  A8. Refusals: below, at the call.
 *  A9. Determinism.  Rule C8 holds; a reuse call returns the bytes a build call with the same arguments returns.
 * A10. Identity.  With the identity pose and gridRadius == radius the records and the summary's fields up to maxD2 are those of
 *      simlod_compare_samples, byte for byte: ((1*x + 0*y) + 0*z) + 0 == x for finite x, y and z — the product by 1 is exact, a zero
 *      product adds nothing — so c' is the widened sample and every later operation is the compare query's.
 * Nothing is written but `scratch`, `records` and `summary`.  `a` and `b` may be the same array. */
#define SIMLOD_ALIGN_ERR_BUDGET  0x1u
#define SIMLOD_ALIGN_ERR_GRID    0x2u
#define SIMLOD_ALIGN_COUNT_ONLY  0x1u      /* flags: rule A6 */
#define SIMLOD_ALIGN_REUSE_GRID  0x2u      /* flags: rule A7 */
typedef struct SimlodAlignParams {     /* host memory; read completely before the call returns */
	float    radius;                   /* finite, >= 0                                                          */
	float    gridRadius;               /* rule A2: finite, >= radius                                            */
	uint64_t maxCandidates;            /* rule C6; 0: no limit                                                  */
	double   pose[12];                 /* rule A1: 3x4, row-major, finite                                       */
	uint32_t flags;                    /* SIMLOD_ALIGN_COUNT_ONLY | SIMLOD_ALIGN_REUSE_GRID                     */
	uint32_t maxWorkgroups;            /* 0: the library's choice; else no kernel launches more workgroups      */
	uint32_t reserved;                 /* 0                                                                     */
} SimlodAlignParams;
typedef struct SimlodAlignSummary {    /* written by the device; SimlodCompareSummary's leading fields at their offsets */
	uint32_t error;                    /* SIMLOD_ALIGN_ERR_* bits                                               */
	uint32_t numCells;                 /* rule C4                                                               */
	uint32_t maxCellPopulation;        /* rule C4                                                               */
	uint32_t numInvalidA;              /* rule A1                                                               */
	uint32_t numInvalidB;              /* rule C1                                                               */
	uint32_t numMatched;               /* samples of `a` with within > 0                                        */
	uint64_t numWithin;                /* the sum of within                                                     */
	uint64_t numCandidates;            /* rule C4                                                               */
	double   maxD2;                    /* the largest matched d2; 0 when none matched                           */
	uint64_t numSummed;                /* rule A5                                                               */
	uint64_t numOutside;               /* rule A4                                                               */
	uint64_t sumA[3];                  /* rule A5                                                               */
	uint64_t sumB[3];                  /* rule A5                                                               */
	uint64_t crossLo[9];               /* rule A5: [3k + l], k the axis of c', l the axis of s                  */
	uint64_t crossHi[9];               /* rule A5                                                               */
	uint64_t sqLo;                     /* rule A5                                                               */
	uint64_t sqHi;                     /* rule A5                                                               */
} SimlodAlignSummary;
SIMLOD_STATIC_ASSERT(sizeof(SimlodAlignParams) == 128, "AlignParams");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignParams, gridRadius) == 4, "AlignParams.gridRadius");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignParams, maxCandidates) == 8, "AlignParams.maxCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignParams, pose) == 16, "AlignParams.pose");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignParams, flags) == 112, "AlignParams.flags");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignParams, maxWorkgroups) == 116, "AlignParams.maxWorkgroups");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignParams, reserved) == 120, "AlignParams.reserved");
SIMLOD_STATIC_ASSERT(sizeof(SimlodAlignSummary) == 272, "AlignSummary");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, error) == offsetof(SimlodCompareSummary, error), "AlignSummary.error");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, numCells) == offsetof(SimlodCompareSummary, numCells), "AlignSummary.numCells");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, maxCellPopulation) == offsetof(SimlodCompareSummary, maxCellPopulation), "AlignSummary.maxCellPopulation");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, numInvalidA) == offsetof(SimlodCompareSummary, numInvalidA), "AlignSummary.numInvalidA");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, numInvalidB) == offsetof(SimlodCompareSummary, numInvalidB), "AlignSummary.numInvalidB");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, numMatched) == offsetof(SimlodCompareSummary, numMatched), "AlignSummary.numMatched");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, numWithin) == offsetof(SimlodCompareSummary, numWithin), "AlignSummary.numWithin");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, numCandidates) == offsetof(SimlodCompareSummary, numCandidates), "AlignSummary.numCandidates");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, maxD2) == offsetof(SimlodCompareSummary, maxD2), "AlignSummary.maxD2");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, numSummed) == 48, "AlignSummary.numSummed");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, numOutside) == 56, "AlignSummary.numOutside");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, sumA) == 64, "AlignSummary.sumA");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, sumB) == 88, "AlignSummary.sumB");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, crossLo) == 112, "AlignSummary.crossLo");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, crossHi) == 184, "AlignSummary.crossHi");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, sqLo) == 256, "AlignSummary.sqLo");
SIMLOD_STATIC_ASSERT(offsetof(SimlodAlignSummary, sqHi) == 264, "AlignSummary.sqHi");

/* Bytes of the `scratch` buffer an align call needs: simlod_compare_buffer_min_bytes(numA, numB) and, behind that layout, the test pass's
 * partial records of the largest grid the library ever chooses.  0 for counts the call refuses. */
uint64_t simlod_align_buffer_min_bytes(uint64_t numA, uint64_t numB);

/* The align query (rules above).  Asynchronous on `stream` once `uniforms` and `params` have been read.  hipErrorInvalidValue with nothing
 * enqueued and nothing touched (rule A8): everything simlod_compare_samples refuses of the arguments both calls have (null pointers other
 * than `records`, the counts, the radius, the box, the alignments — `records` at 16 bytes, `summary` at 8); a `pose` with an entry that is
 * not finite; a gridRadius that is not finite or < radius; unknown bits in `flags`; a nonzero `reserved`; scratchBytes below
 * simlod_align_buffer_min_bytes(numA, numB) (one byte less is refused, the exact size is accepted). */
int simlod_align_samples(const SimlodUniforms* uniforms /*host*/, const SimlodPoint* a, uint64_t numA, const SimlodPoint* b, uint64_t numB,
                         const SimlodAlignParams* params /*host*/, void* scratch, uint64_t scratchBytes,
                         SimlodCompareRecord* records /*or NULL: sums only*/, SimlodAlignSummary* summary, void* stream);

/* Version / build info string (static storage). */
const char* simlod_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* SIMLOD_HIP_H */
