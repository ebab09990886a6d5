"""Test-side restatement of simlod_import_octree_buildable (include/simlod_hip.h) on a table, its samples and the uniforms: the occupancy
grids it rebuilds and the voxel list of a root that is still a leaf.  The rule: the grid of the root and of every inner node is the set of that
node's level-cells of all points below it (its subtree's leaves' samples), the cell of a point being the builder's (quantize(F_FULL), the
level shift of grid_cell / voxel_of).  test_resume_io.py pins this rule to the oracle's images; the GPU tests pin the device to this."""
import numpy as np

from simlod_amd import abi

GRID_BITS = 21                      # 128^3 cells


def box_of(uniforms):
    """(boxMin as float32[3], size) as kernel_construct derives them: the largest extent, fp32 (voxels.cu:860-863)."""
    u = np.asarray(uniforms).reshape(-1)[0]
    mn = np.asarray(u["boxMin"], np.float32)
    mx = np.asarray(u["boxMax"], np.float32)
    ext = [np.float32(mx[k] - mn[k]) for k in range(3)]
    return mn, np.float32(max(max(ext[0], ext[1]), ext[2]))


def quantize_full(samples, mn, size):
    """The 28-bit coordinates of quantize(F_FULL, p, min, size): fp32 scale * (p - min) / size, truncated; v_cvt_u32_f32 saturates (NaN and
    negatives: 0)."""
    out = []
    with np.errstate(all="ignore"):
        for k, a in enumerate("xyz"):
            v = np.float32(268435456.0) * (samples[a].astype(np.float32) - mn[k])
            v = (v / size).astype(np.float64)
            q = np.clip(np.floor(v), 0.0, 4294967295.0)
            q[np.isnan(v)] = 0.0
            out.append(q.astype(np.uint32))
    return out


def cells_at(level, pX, pY, pZ):
    """grid_cell(level, ...) of construct_voxelize.inc: x + 128 y + 128^2 z of the level's 128^3 grid."""
    s = (abi.MAX_DEPTH + 1 - np.asarray(level, dtype=np.int64)).astype(np.uint32)
    return (((pX >> s) & 127) + ((pY >> s) & 127) * 128 + ((pZ >> s) & 127) * 16384).astype(np.int64)


def _leaf_points(t):
    """Sample index -> the table entry it belongs to, for the leaves' samples only (an inner entry's samples are voxels)."""
    owner = np.repeat(np.arange(len(t), dtype=np.int64), t["numSamples"].astype(np.int64))
    idx = np.nonzero(t["childMask"][owner] == 0)[0]
    return idx, owner[idx]


def rebuild_grids(table, samples, uniforms):
    """{table index: uint32[65536]} for the root and every inner node."""
    t = np.asarray(table).view(abi.export_node_dtype)
    s = np.asarray(samples).view(abi.point_dtype)
    mn, size = box_of(uniforms)
    idx, cur = _leaf_points(t)
    pX, pY, pZ = (q[idx] for q in quantize_full(s, mn, size))
    has = t["childMask"] != 0
    has[0] = True
    parent = t["parent"].astype(np.int64)
    level = t["level"].astype(np.int64)
    keys = []
    while len(cur):
        g = has[cur]
        keys.append((cur[g] << GRID_BITS) | cells_at(level[cur[g]], pX[g], pY[g], pZ[g]))
        up = cur != 0
        cur, pX, pY, pZ = parent[cur[up]], pX[up], pY[up], pZ[up]
    keys = np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    node = keys >> GRID_BITS
    cells = keys & ((1 << GRID_BITS) - 1)
    out = {}
    for i in np.nonzero(has)[0]:
        lo, hi = np.searchsorted(node, [i, i + 1])
        c = cells[lo:hi]
        # the cells of a node are unique: the sum of their bits per word is their OR (exact in float64)
        w = np.bincount(c >> 5, weights=(np.ones(len(c), np.uint64) << (c & 31).astype(np.uint64)).astype(np.float64), minlength=abi.GRID_NUM_WORDS)
        out[int(i)] = w.astype(np.uint64).astype(np.uint32)
    return out


def root_leaf_voxels(table, samples, uniforms):
    """The voxel list the import gives a root that is still a leaf: one voxel per occupied cell of its grid in ascending cell order, at the cell
    centre by the builder's fp32 formula (voxel_centre, voxels.cu:103-114), coloured by the lowest-index point of the cell.  -> (cells, voxels)."""
    t = np.asarray(table).view(abi.export_node_dtype)
    assert t[0]["childMask"] == 0, "the root has children"
    s = np.asarray(samples).view(abi.point_dtype)
    f, n = int(t[0]["firstSample"]), int(t[0]["numSamples"])
    pts = s[f: f + n]
    mn, size = box_of(uniforms)
    cells = cells_at(0, *quantize_full(pts, mn, size))
    uc, first = np.unique(cells, return_index=True)
    vox = np.zeros(len(uc), dtype=abi.point_dtype)
    node_size = np.float32(size / np.float32(1.0))
    for a, c in zip("xyz", (uc & 127, (uc >> 7) & 127, uc >> 14)):
        k = "xyz".index(a)
        nmin = np.float32(np.float32(np.float32(0.0) + np.float32(0.0)) * node_size) + mn[k]
        vox[a] = np.float32(nmin) + (node_size * (c.astype(np.float32) + np.float32(0.5))) / np.float32(128.0)
    vox["color"] = pts["color"][first]
    return uc, vox


def grid_of_image(nodes, i, persistent):
    """The occupancy grid of node i of a HOST-addressed image whose persistent buffer is the numpy array `persistent`."""
    off = int(nodes[i]["grid"]) - persistent.ctypes.data
    assert 0 <= off <= persistent.size - abi.GRID_BYTES, "grid outside the persistent buffer"
    return persistent[off: off + abi.GRID_BYTES].view(np.uint32)
