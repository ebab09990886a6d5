"""numpy mirrors of include/simlod_abi.h (the SimLOD Node/Chunk/Point/Uniforms/Stats layout).

Reference definitions: modules/progressive_octree/structures.cuh:21-143 and
modules/progressive_octree/HostDeviceInterface.h:6-71.  Sizes and offsets are asserted at import time
against the numbers pinned in include/simlod_abi.h.
"""
import numpy as np

MAX_POINTS_PER_NODE = 50_000
POINTS_PER_CHUNK = 1000
GRID_SIZE = 128
GRID_NUM_WORDS = GRID_SIZE ** 3 // 32
MAX_DEPTH = 20
BATCH_STREAM_SIZE = 50
MAX_BATCH_SIZE = 1_000_000
MAX_BATCHES_PER_LAUNCH = 20
MAX_VISIBLE_NODES = 100_000
CLEAR_PIXEL = (0x7F800000 << 32) | 0x00332211
NODE_BYTES_PER_SLOT_HOST = 200          # main_progressive_octree.cpp:552 sizes the node array as 200 000 x 200 B
CHUNK_BYTES = 16016
GRID_BYTES = 262144

point_dtype = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("color", "<u4")])

node_dtype = np.dtype({
    "names": ["children", "counter", "numPoints", "level", "X", "Y", "Z", "countIteration", "countFlag",
              "name", "visible", "isFiltered", "isLeaf", "isLarge", "grid", "points", "voxelChunks",
              "numVoxels", "numVoxelsStored"],
    "formats": [("<u8", 8), "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4",
                ("u1", 20), "u1", "u1", "u1", "u1", "<u8", "<u8", "<u8", "<u4", "<u4"],
    "offsets": [0, 64, 68, 72, 76, 80, 84, 88, 92, 96, 116, 117, 118, 119, 120, 128, 136, 144, 148],
    "itemsize": 152,
})

mat4_dtype = np.dtype(("<f4", (4, 4)))   # rows[i] = matrix row i

uniforms_dtype = np.dtype({
    "names": ["width", "height", "time", "fovy_rad", "world", "view", "proj", "transform",
              "transform_updateBound", "transformInv_updateBound", "persistentBufferCapacity",
              "momentaryBufferCapacity", "frameCounter", "boxMin", "boxMax", "showBoundingBox", "showPoints",
              "colorByNode", "colorByLOD", "colorWhite", "doUpdateVisibility", "doProgressive", "LOD",
              "useHighQualityShading", "minNodeSize", "pointSize", "updateStats", "enableEDL", "edlStrength"],
    "formats": ["<f4", "<f4", "<f4", "<f4", mat4_dtype, mat4_dtype, mat4_dtype, mat4_dtype, mat4_dtype, mat4_dtype,
                "<u8", "<u8", "<u8", ("<f4", 3), ("<f4", 3), "u1", "u1", "u1", "u1", "u1", "u1", "u1", "<f4",
                "u1", "<f4", "<i4", "u1", "u1", "<f4"],
    "offsets": [0, 4, 8, 12, 16, 80, 144, 208, 272, 336, 400, 408, 416, 424, 436, 448, 449, 450, 451, 452, 453,
                454, 456, 460, 464, 468, 472, 473, 476],
    "itemsize": 480,
})

stats_dtype = np.dtype({
    "names": ["frameID", "numNodes", "numInner", "numLeaves", "numNonemptyLeaves", "numPoints", "numVoxels",
              "allocatedBytes_momentary", "allocatedBytes_persistent", "numVisibleNodes", "numVisibleInner",
              "numVisibleLeaves", "numVisiblePoints", "numVisibleVoxels", "numChunksPoints", "numChunksVoxels",
              "batchletIndex", "numPointsProcessed", "numAllocatedChunks", "chunkPoolSize", "dbg",
              "memCapacityReached"],
    "formats": ["<u4"] * 7 + ["<u8", "<u8"] + ["<u4"] * 8 + ["<u8", "<u8", "<u8", "<u4", "u1"],
    "offsets": [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72, 76, 80, 88, 96, 104, 108],
    "itemsize": 112,
})

assert point_dtype.itemsize == 16 and node_dtype.itemsize == 152
assert uniforms_dtype.itemsize == 480 and stats_dtype.itemsize == 112


def alloc_round(size: int) -> int:
    """AllocatorGlobal::alloc rounding, utils.h.cu:190."""
    return 16 * ((size + 16) // 16)


def make_uniforms(width, height, transform, box_size, *, transform_update_bound=None,
                  persistent_capacity=0, momentary_capacity=0, frame_counter=0, point_size=1,
                  min_node_size=64.0, hqs=False, show_points=True, color_by_node=False, color_by_lod=False,
                  show_bounding_box=False, fovy_deg=60.0, box_min=(0.0, 0.0, 0.0)):
    """Fill a Uniforms record the way getUniforms() does (main_progressive_octree.cpp:283-331).

    `transform` is the ROW-MAJOR 4x4 world-view-projection matrix (rows[i] = row i, i.e. what the host
    obtains after glm::transpose).  The reference host always sends boxMin = 0 and boxMax = the bounding-box size (:312-313);
    `box_min` places the box elsewhere: boxMin = float32(box_min), boxMax = float32(boxMin + float32(box_size)), the sum formed in
    fp32 as a host that keeps fp32 coordinates would form it (so boxMax - boxMin need not give box_size back).
    """
    u = np.zeros((), dtype=uniforms_dtype)
    t = np.asarray(transform, dtype=np.float32).reshape(4, 4)
    tu = t if transform_update_bound is None else np.asarray(transform_update_bound, np.float32).reshape(4, 4)
    ident = np.eye(4, dtype=np.float32)
    u["width"], u["height"] = float(width), float(height)
    u["fovy_rad"] = np.float32(3.1415) * np.float32(fovy_deg) / np.float32(180.0)
    u["world"], u["view"], u["proj"] = ident, ident, ident
    u["transform"], u["transform_updateBound"] = t, tu
    with np.errstate(all="ignore"):
        try:
            u["transformInv_updateBound"] = np.linalg.inv(tu.astype(np.float64)).astype(np.float32)
        except np.linalg.LinAlgError:
            u["transformInv_updateBound"] = ident
    u["persistentBufferCapacity"] = persistent_capacity
    u["momentaryBufferCapacity"] = momentary_capacity
    u["frameCounter"] = frame_counter
    mn = np.asarray(box_min, dtype=np.float32).reshape(3)
    u["boxMin"] = mn
    u["boxMax"] = mn + np.asarray(box_size, dtype=np.float32).reshape(3)
    u["showBoundingBox"] = show_bounding_box
    u["showPoints"] = show_points
    u["colorByNode"], u["colorByLOD"] = color_by_node, color_by_lod
    u["doUpdateVisibility"] = 1
    u["LOD"] = 0.2
    u["useHighQualityShading"] = hqs
    u["minNodeSize"] = min_node_size
    u["pointSize"] = point_size
    u["enableEDL"] = 1
    u["edlStrength"] = 0.8
    return u


# ---- octree export / import (include/simlod_hip.h, "octree export / import") ---------------------------------------------------------
EXPORT_ALL, EXPORT_CUT, EXPORT_VISIBLE = 0, 1, 2
EXPORT_SELECT = {"all": EXPORT_ALL, "cut": EXPORT_CUT, "visible": EXPORT_VISIBLE}
EXPORT_REGION = 3                       # the `select` an OctreeExport carries that came from a region query (never passed to the device)
EXPORT_NONE = 0xFFFFFFFF
EXPORT_FLAG_LEAF, EXPORT_FLAG_SELECTED = 0x1, 0x2
EXPORT_ERR_CAPACITY, EXPORT_ERR_NODE_COUNT, EXPORT_ERR_SHORT_LIST = 0x1, 0x2, 0x4
SIMLOD_ERR_IMPORT = 0x400
SIMLOD_ERR_IMPORT_GRID = 0x800          # simlod_import_octree_buildable: a rebuilt grid disagrees with the table (wrong box); sticky until a reset

export_node_dtype = np.dtype({
    "names": ["level", "X", "Y", "Z", "parent", "firstChild", "childMask", "flags", "reserved", "numSamples", "firstSample"],
    "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "u1", "u1", "<u2", "<u4", "<u8"],
    "offsets": [0, 4, 8, 12, 16, 20, 24, 25, 26, 28, 32],
    "itemsize": 40,
})
export_counts_dtype = np.dtype({"names": ["numNodes", "error", "numSamples"], "formats": ["<u4", "<u4", "<u8"], "offsets": [0, 4, 8], "itemsize": 16})
assert export_node_dtype.itemsize == 40 and export_counts_dtype.itemsize == 16

# ---- region queries (include/simlod_hip.h, "region queries") ----------------------------------------------------------------------------
REGION_MAX_PLANES = 16
region_dtype = np.dtype({"names": ["numPlanes", "reserved", "planes"], "formats": ["<u4", ("<u4", 3), ("<f4", (REGION_MAX_PLANES, 4))],
                         "offsets": [0, 4, 16], "itemsize": 272})
query_counts_dtype = np.dtype({"names": ["numNodes", "error", "numSamples", "numCandidates", "numFilteredNodes", "numCopiedNodes"],
                               "formats": ["<u4", "<u4", "<u8", "<u8", "<u4", "<u4"], "offsets": [0, 4, 8, 16, 24, 28], "itemsize": 32})
assert region_dtype.itemsize == 272 and query_counts_dtype.itemsize == 32

# ---- view queries (include/simlod_hip.h, "view queries") --------------------------------------------------------------------------------
VIEW_MAX_BIAS = 20
VIEW_NO_CULL, VIEW_DRAW_SMALL_ROOT = 0x1, 0x2
VIEW_NO_BUDGET = 0xFFFFFFFFFFFFFFFF
EXPORT_ERR_BUDGET = 0x8
view_dtype = np.dtype({"names": ["flags", "minBias", "maxBias", "reserved", "sampleBudget"], "formats": ["<u4", "<u4", "<u4", "<u4", "<u8"],
                       "offsets": [0, 4, 8, 12, 16], "itemsize": 24})
view_counts_dtype = np.dtype({"names": ["numNodes", "error", "numSamples", "bias", "numSelected", "numInside", "reserved", "samplesAt"],
                              "formats": ["<u4", "<u4", "<u8", "<u4", "<u4", "<u4", "<u4", ("<u8", VIEW_MAX_BIAS + 1)],
                              "offsets": [0, 4, 8, 16, 20, 24, 28, 32], "itemsize": 200})
assert view_dtype.itemsize == 24 and view_counts_dtype.itemsize == 200


def view_record(bias=0, max_bias=VIEW_MAX_BIAS, budget=None, cull=True, draw_small_root=False):
    """The SimlodView record of a view query: the biases [bias, max_bias], the sample budget (None: none) and the two flags."""
    v = np.zeros(1, dtype=view_dtype)
    v["flags"] = (0 if cull else VIEW_NO_CULL) | (VIEW_DRAW_SMALL_ROOT if draw_small_root else 0)
    v["minBias"], v["maxBias"] = int(bias), int(max_bias)
    v["sampleBudget"] = VIEW_NO_BUDGET if budget is None else int(budget)
    return v


# ---- view deltas (include/simlod_hip.h, "view deltas") -----------------------------------------------------------------------------------
DELTA_NONE, DELTA_KEPT, DELTA_GROWN, DELTA_ADDED = 0, 1, 2, 3
DELTA_TAILS = 0x1
delta_entry_dtype = np.dtype({"names": ["held", "state", "numKept", "numDelta", "firstDelta"], "formats": ["<u4", "<u4", "<u4", "<u4", "<u8"],
                              "offsets": [0, 4, 8, 12, 16], "itemsize": 24})
delta_counts_dtype = np.dtype({"names": ["view", "numDeltaSamples", "numKeptSamples", "numKept", "numGrown", "numAdded", "numDropped"],
                               "formats": [view_counts_dtype, "<u8", "<u8", "<u4", "<u4", "<u4", "<u4"],
                               "offsets": [0, 200, 208, 216, 220, 224, 228], "itemsize": 232})
assert delta_entry_dtype.itemsize == 24 and delta_counts_dtype.itemsize == 232

# ---- packed samples (include/simlod_hip.h, "packed samples") ------------------------------------------------------------------------------
PACK_COLOR_BITS, PACK_POINT_BITS, PACK_VOXEL_BITS = 24, 13, 7               # rule K0: bits 0-23 rgb, then 13 bits per axis; voxels use the low 7
PACK_SHIFT_X, PACK_SHIFT_Y, PACK_SHIFT_Z = 24, 37, 50
PACK_ITEM_BYTES = 64                                                       # of the scratch buffer per piece of at most 1 000 samples
pack_counts_dtype = np.dtype({"names": ["numSamples", "numClamped", "numInexact", "numAlpha", "error", "reserved"],
                              "formats": ["<u8", "<u8", "<u8", "<u8", "<u4", "<u4"], "offsets": [0, 8, 16, 24, 32, 36], "itemsize": 40})
assert pack_counts_dtype.itemsize == 40


# ---- clip regions (include/simlod_hip.h, "clip regions") --------------------------------------------------------------------------------
CLIP_OFF, CLIP_INSIDE, CLIP_OUTSIDE, CLIP_HIGHLIGHT = 0, 1, 2, 3
CLIP_MODES = {"off": CLIP_OFF, "inside": CLIP_INSIDE, "outside": CLIP_OUTSIDE, "highlight": CLIP_HIGHLIGHT}
clip_dtype = np.dtype({"names": ["mode", "color", "reserved", "region"], "formats": ["<u4", "<u4", ("<u4", 2), region_dtype], "offsets": [0, 4, 8, 16], "itemsize": 288})
assert clip_dtype.itemsize == 288 and clip_dtype.fields["region"][1] == 16

# ---- footprint queries (include/simlod_hip.h, "footprint queries") ----------------------------------------------------------------------
FOOTPRINT_MAX_VERTICES = 256
footprint_dtype = np.dtype({"names": ["numVertices", "reserved", "axisU", "axisV", "vertices"],
                            "formats": ["<u4", ("<u4", 3), ("<f4", 4), ("<f4", 4), ("<f4", (FOOTPRINT_MAX_VERTICES, 2))],
                            "offsets": [0, 4, 16, 32, 48], "itemsize": 2096})
assert footprint_dtype.itemsize == 2096

# ---- paint regions (include/simlod_hip.h, "paint regions") -------------------------------------------------------------------------------
PAINT_SET, PAINT_BLEND, PAINT_RAMP, PAINT_ARRAY = 0, 1, 2, 3
PAINT_MODES = {"set": PAINT_SET, "blend": PAINT_BLEND, "ramp": PAINT_RAMP, "array": PAINT_ARRAY}
paint_dtype = np.dtype({"names": ["mode", "color", "strength", "reserved", "z0", "scale", "reserved2", "table"],
                        "formats": ["<u4", "<u4", "<u4", "<u4", "<f4", "<f4", ("<u4", 2), ("<u4", 256)],
                        "offsets": [0, 4, 8, 12, 16, 20, 24, 32], "itemsize": 1056})
assert paint_dtype.itemsize == 1056

# ---- summary queries (include/simlod_hip.h, "summary queries") ---------------------------------------------------------------------------
SUMMARY_CELLS = 1 << 20                                                     # rule S2: cells per axis; the products use the top 16 bits
SUMMARY_MOMENTS = ("xx", "yy", "zz", "xy", "xz", "yz")                      # the order of SimlodSummary.sum2
summary_params_dtype = np.dtype({"names": ["z0", "scale", "maxWorkgroups", "reserved"], "formats": ["<f4", "<f4", "<u4", "<u4"],
                                 "offsets": [0, 4, 8, 12], "itemsize": 16})
summary_dtype = np.dtype({"names": ["numSamples", "numNonFinite", "min", "max", "sum", "sum2", "histZ", "histC"],
                          "formats": ["<u8", "<u8", ("<f4", 3), ("<f4", 3), ("<u8", 3), ("<u8", 6), ("<u8", 256), ("<u8", (4, 256))],
                          "offsets": [0, 8, 16, 28, 40, 64, 112, 2160], "itemsize": 10352})
assert summary_params_dtype.itemsize == 16 and summary_dtype.itemsize == 10352

# ---- compare queries (include/simlod_hip.h, "compare queries") ---------------------------------------------------------------------------
COMPARE_ERR_BUDGET = 0x1
COMPARE_MISS = 0xFFFFFFFF                                                   # `nearest` of the miss record; its d2 is +infinity
COMPARE_MAX_COUNT = (1 << 32) - 2                                           # numA, numB: 1 .. 2^32 - 2
COMPARE_HASH_MUL = 0x9E3779B97F4A7C15                                       # compare_rules.hpp compare_home
compare_record_dtype = np.dtype({"names": ["d2", "nearest", "within"], "formats": ["<f8", "<u4", "<u4"], "offsets": [0, 8, 12], "itemsize": 16})
compare_params_dtype = np.dtype({"names": ["radius", "missColor", "maxCandidates", "thresholds2", "table", "maxWorkgroups", "reserved"],
                                 "formats": ["<f4", "<u4", "<u8", ("<f8", 255), ("<u4", 256), "<u4", "<u4"],
                                 "offsets": [0, 4, 8, 16, 2056, 3080, 3084], "itemsize": 3088})
compare_summary_dtype = np.dtype({"names": ["error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numMatched", "numWithin",
                                            "numCandidates", "maxD2", "hist"],
                                  "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<f8", ("<u8", 257)],
                                  "offsets": [0, 4, 8, 12, 16, 20, 24, 32, 40, 48], "itemsize": 2104})
assert compare_record_dtype.itemsize == 16 and compare_params_dtype.itemsize == 3088 and compare_summary_dtype.itemsize == 2104

# ---- surface queries (include/simlod_hip.h, "surface queries") ---------------------------------------------------------------------------
SURFACE_ERR_BUDGET = 0x1
SURFACE_SHADE, SURFACE_VARIATION = 0, 1                                     # colourBy
SURFACE_ORIENT_DIRECTION, SURFACE_ORIENT_POSITION = 0, 1                    # orientMode
SURFACE_ORIENT_MODES = {"direction": SURFACE_ORIENT_DIRECTION, "position": SURFACE_ORIENT_POSITION}
SURFACE_MIN_WITHIN = 3                                                      # rule N9: fewer neighbours span no plane
SURFACE_Q_SCALE = 16384.0                                                   # rule N2: invq = 16384 / h
SURFACE_SQUARINGS = 8                                                       # rule N5
surface_record_dtype = np.dtype({"names": ["normal", "within", "lambdaNum", "lambdaDen"], "formats": [("<f4", 3), "<u4", "<f8", "<f8"],
                                 "offsets": [0, 12, 16, 24], "itemsize": 32})
surface_params_dtype = np.dtype({"names": ["radius", "missColor", "maxCandidates", "thresholds", "table", "light", "orient", "colourBy", "orientMode",
                                           "maxWorkgroups", "reserved"],
                                 "formats": ["<f4", "<u4", "<u8", ("<f8", 255), ("<u4", 256), ("<f4", 3), ("<f4", 3), "<u4", "<u4", "<u4", "<u4"],
                                 "offsets": [0, 4, 8, 16, 2056, 3080, 3092, 3104, 3108, 3112, 3116], "itemsize": 3120})
surface_summary_dtype = np.dtype({"names": ["error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numEstimated", "numWithin",
                                            "numCandidates", "numDegenerate", "hist"],
                                  "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<u8", ("<u8", 257)],
                                  "offsets": [0, 4, 8, 12, 16, 20, 24, 32, 40, 48], "itemsize": 2104})
assert surface_record_dtype.itemsize == 32 and surface_params_dtype.itemsize == 3120 and surface_summary_dtype.itemsize == 2104

# ---- cluster queries (include/simlod_hip.h, "cluster queries") ---------------------------------------------------------------------------
CLUSTER_ERR_BUDGET, CLUSTER_ERR_INTERNAL = 0x1, 0x2
CLUSTER_NOISE = 0xFFFFFFFF                                                  # `cluster` of noise and of dissolved samples
CLUSTER_MISS = 0xFFFFFFFF                                                   # `root` of true noise
CLUSTER_SIZE_BINS = 33                                                      # sizeHist: floor(log2(size))
cluster_record_dtype = np.dtype({"names": ["cluster", "root", "size", "within"], "formats": ["<u4", "<u4", "<u4", "<u4"], "offsets": [0, 4, 8, 12],
                                 "itemsize": 16})
cluster_params_dtype = np.dtype({"names": ["radius", "minNeighbours", "minClusterSize", "noiseColor", "maxCandidates", "table", "maxWorkgroups", "reserved"],
                                 "formats": ["<f4", "<u4", "<u4", "<u4", "<u8", ("<u4", 256), "<u4", "<u4"],
                                 "offsets": [0, 4, 8, 12, 16, 24, 1048, 1052], "itemsize": 1056})
cluster_summary_dtype = np.dtype({"names": ["error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numClusters", "numWithin",
                                            "numCandidates", "numCore", "numBorder", "numNoise", "numDissolved", "largestSize", "largestCluster",
                                            "sizeHist", "zero"],
                                  "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<u4", "<u4",
                                              ("<u8", CLUSTER_SIZE_BINS), ("<u8", 220)],
                                  "offsets": [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 76, 80, 344], "itemsize": 2104})
assert cluster_record_dtype.itemsize == 16 and cluster_params_dtype.itemsize == 1056 and cluster_summary_dtype.itemsize == compare_summary_dtype.itemsize

# ---- align queries (include/simlod_hip.h, "align queries") -------------------------------------------------------------------------------
ALIGN_ERR_BUDGET, ALIGN_ERR_GRID = 0x1, 0x2
ALIGN_COUNT_ONLY, ALIGN_REUSE_GRID = 0x1, 0x2                               # flags
ALIGN_Q_SCALE = 16777216.0                                                  # rule A4: invQ = 2^24 / size
align_params_dtype = np.dtype({"names": ["radius", "gridRadius", "maxCandidates", "pose", "flags", "maxWorkgroups", "reserved"],
                               "formats": ["<f4", "<f4", "<u8", ("<f8", 12), "<u4", "<u4", "<u4"],
                               "offsets": [0, 4, 8, 16, 112, 116, 120], "itemsize": 128})
align_summary_dtype = np.dtype({"names": ["error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numMatched", "numWithin",
                                          "numCandidates", "maxD2", "numSummed", "numOutside", "sumA", "sumB", "crossLo", "crossHi", "sqLo", "sqHi"],
                                "formats": ["<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<f8", "<u8", "<u8", ("<u8", 3), ("<u8", 3),
                                            ("<u8", 9), ("<u8", 9), "<u8", "<u8"],
                                "offsets": [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 88, 112, 184, 256, 264], "itemsize": 272})
assert align_params_dtype.itemsize == 128 and align_summary_dtype.itemsize == 272


def align_prototypes(L):
    """The ctypes prototypes of the two align entry points on the loaded library L (runtime.lib() calls it)."""
    import ctypes
    u64, vp = ctypes.c_uint64, ctypes.c_void_p
    L.simlod_align_buffer_min_bytes.restype = u64
    L.simlod_align_buffer_min_bytes.argtypes = [u64, u64]
    L.simlod_align_samples.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp]


# ---- lasso queries (include/simlod_hip.h, "lasso queries") -------------------------------------------------------------------------------
LASSO_MAX_VERTICES = 256
lasso_dtype = np.dtype({"names": ["numVertices", "reserved", "rowU", "rowV", "rowW", "vertices"],
                        "formats": ["<u4", ("<u4", 3), ("<f4", 4), ("<f4", 4), ("<f4", 4), ("<f4", (LASSO_MAX_VERTICES, 2))],
                        "offsets": [0, 4, 16, 32, 48, 64], "itemsize": 2112})
assert lasso_dtype.itemsize == 2112

# ---- profile queries (include/simlod_hip.h, "profile queries") --------------------------------------------------------------------------
PROFILE_MAX_VERTICES = 64
PROFILE_NO_SEGMENT = 0xFFFFFFFF
profile_dtype = np.dtype({"names": ["numVertices", "halfWidth", "reserved", "axisU", "axisV", "axisH", "vertices"],
                          "formats": ["<u4", "<f4", ("<u4", 2), ("<f4", 4), ("<f4", 4), ("<f4", 4), ("<f4", (PROFILE_MAX_VERTICES, 2))],
                          "offsets": [0, 4, 8, 16, 32, 48, 64], "itemsize": 576})
profile_sample_dtype = np.dtype({"names": ["station", "offset", "height", "segment"], "formats": ["<f4", "<f4", "<f4", "<u4"],
                                 "offsets": [0, 4, 8, 12], "itemsize": 16})
# the fp64 block of rule P0, one row per segment, as the launcher places it in the scratch buffer
profile_segment_dtype = np.dtype({"names": ["au", "av", "du", "dv", "L2", "W2", "inv", "s0"], "formats": ["<f8"] * 8})
assert profile_dtype.itemsize == 576 and profile_sample_dtype.itemsize == 16 and profile_segment_dtype.itemsize == 64

# ---- ray queries (include/simlod_hip.h, "ray queries") -----------------------------------------------------------------------------------
RAYS_MAX = 1 << 20
ray_dtype = np.dtype({"names": ["origin", "tMin", "dir", "tMax", "radius", "spread", "reserved"],
                      "formats": [("<f4", 3), "<f4", ("<f4", 3), "<f4", "<f4", "<f4", ("<u4", 2)], "offsets": [0, 12, 16, 28, 32, 36, 40], "itemsize": 48})
ray_hit_dtype = np.dtype({"names": ["t", "node", "ordinal", "sample"], "formats": ["<f8", "<u4", "<u4", point_dtype], "offsets": [0, 8, 12, 16], "itemsize": 32})
ray_counts_dtype = np.dtype({"names": ["numNodes", "error", "numHits", "numInvalid", "numPairs", "numCandidates"],
                             "formats": ["<u4", "<u4", "<u4", "<u4", "<u8", "<u8"], "offsets": [0, 4, 8, 12, 16, 24], "itemsize": 32})
assert ray_dtype.itemsize == 48 and ray_hit_dtype.itemsize == 32 and ray_counts_dtype.itemsize == 32

# ---- neighbour queries (include/simlod_hip.h, "neighbour queries") -----------------------------------------------------------------------
NEIGHBOURS_MAX = 1 << 20
NEIGHBOURS_MAX_K = 16
sphere_dtype = np.dtype({"names": ["center", "radius"], "formats": [("<f4", 3), "<f4"], "offsets": [0, 12], "itemsize": 16})
neighbour_dtype = np.dtype({"names": ["d2", "node", "ordinal", "sample"], "formats": ["<f8", "<u4", "<u4", point_dtype], "offsets": [0, 8, 12, 16], "itemsize": 32})
neighbour_counts_dtype = np.dtype({"names": ["numNodes", "error", "numInvalid", "k", "numPairs", "numCandidates", "numFound", "numWithin"],
                                   "formats": ["<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<u8", "<u8"], "offsets": [0, 4, 8, 12, 16, 24, 32, 40], "itemsize": 48})
assert sphere_dtype.itemsize == 16 and neighbour_dtype.itemsize == 32 and neighbour_counts_dtype.itemsize == 48

# ---- styled LAS decode (include/simlod_hip.h, "styled decode") ---------------------------------------------------------------------------
(LAS_RGB, LAS_INTENSITY, LAS_CLASSIFICATION, LAS_RETURN_NUMBER, LAS_NUMBER_OF_RETURNS, LAS_USER_DATA, LAS_POINT_SOURCE_ID, LAS_SCAN_ANGLE,
 LAS_GPS_TIME, LAS_ELEVATION, LAS_ATTRIBUTE_COUNT) = range(11)
LAS_ATTRIBUTES = {"rgb": LAS_RGB, "intensity": LAS_INTENSITY, "classification": LAS_CLASSIFICATION, "return_number": LAS_RETURN_NUMBER,
                  "number_of_returns": LAS_NUMBER_OF_RETURNS, "user_data": LAS_USER_DATA, "point_source_id": LAS_POINT_SOURCE_ID,
                  "scan_angle": LAS_SCAN_ANGLE, "gps_time": LAS_GPS_TIME, "elevation": LAS_ELEVATION}
las_style_dtype = np.dtype({"names": ["attribute", "reserved", "lo", "hi", "lut"], "formats": ["<u4", "<u4", "<f8", "<f8", ("<u4", 256)],
                            "offsets": [0, 4, 8, 16, 24], "itemsize": 1048})
assert las_style_dtype.itemsize == 1048

# ---- kernel_render's buffer (include/simlod_hip.h simlod_render_frame_layout; simlod_amd/csrc/render_layout.hpp states the layout) -------
frame_layout_dtype = np.dtype([(n, "<u8") for n in (
    "visible", "counters", "lines", "vertices", "probe", "framebuffer", "work", "items", "depth", "colour", "sums", "dir",
    "binSegs", "binSegCount", "binStats", "binPool", "bytes", "binTiles", "binTilesX",
    "counterStride", "drawItemBytes", "binSegBytes", "maxDrawItems", "itemClasses")])
assert frame_layout_dtype.itemsize == 192
# the frame's counters (enum C_*) and the 32-bit words of its work area (enum W_*), by the enums' names
COUNTERS = {"C_VISIBLE": 0, "C_POINTS": 1, "C_VOXELS": 2, "C_INNER": 3, "C_LEAVES": 4, "C_TABLE_LISTS": 5, "C_OUTSIDE_TILES": 6, "C_COUNT": 7}
WORK_WORDS = {"W_CURSOR0": 0, "W_DIR_ENTRIES": 4, "W_ITEMS0": 8, "W_POOL_TAKEN": 12, "W_BINNED": 13, "W_SORTING_NODES": 14, "W_COUNT": 15, "W_READY": 15}
# a draw item (render_common.inc DrawItem), as the raster tools read it
draw_item_dtype = np.dtype([("chunks", "<u8"), ("samples", "<u4"), ("visibleIdx", "<u4"), ("tileX", "<i4"), ("tileY", "<i4"), ("tileW", "<u2"), ("tileH", "<u2"), ("took", "<u4")])
assert draw_item_dtype.itemsize == 32
