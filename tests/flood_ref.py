"""Numpy models for the flood tests (tests/test_gpu_flood_edges.py): which nodes of an octree lie in a cell, how many input points lie in a node, and
what a root cascade keeps when the node array cannot take all of it.

grant_model() is written from the CONTRACT in the comments of simlod_amd/csrc/construct_expand.inc ("no room in the node array for the whole cascade: as
many of its splits as still fit, children first"; "as many as still fit, the first in local-node order, the others stay too full") and DESIGN §4.2, not from
the kernel's code: one slot (the root's, in an empty octree) settles three levels from the counts of the 512 level-3 cells alone."""
import numpy as np

LIMIT = 50_000                      # MAX_POINTS_PER_NODE: a node that holds more splits


def octant(o):
    """Octant number -> (x, y, z) bits.  The bit order is x, y, z: where a node's coordinates are formed, X = 2 X + (o >> 2 & 1), Y = 2 Y + (o >> 1 & 1),
    Z = 2 Z + (o & 1)."""
    return (o >> 2) & 1, (o >> 1) & 1, o & 1


def cell_counts(points, box, level):
    """Input points per cell of the 2^level grid: int64[2^level, 2^level, 2^level] indexed [X, Y, Z] (the builder's quantization: the fp32 quotient
    2^20 * p / size, truncated, its top `level` bits)."""
    size = np.float32(max(box))
    side = 1 << level
    idx = [((np.float32(2 ** 20) * points[a] / size).astype(np.uint32) >> np.uint32(20 - level)).astype(np.int64) for a in "xyz"]
    assert all(int(i.max()) < side for i in idx)
    return np.bincount((idx[0] * side + idx[1]) * side + idx[2], minlength=side ** 3).reshape(side, side, side)


def points_per_node(points, box, level, X, Y, Z):
    """Input points in each of the nodes (level[i]; X[i], Y[i], Z[i])."""
    out = np.zeros(len(level), dtype=np.int64)
    for l in np.unique(level):
        sel = level == l
        if l == 0:
            out[sel] = len(points)
        else:
            c = cell_counts(points, box, int(l))
            out[sel] = c[X[sel].astype(np.int64), Y[sel].astype(np.int64), Z[sel].astype(np.int64)]
    return out


def inside(dump, level, cell):
    """Mask of the dump's nodes at or below `level` that lie in cell (X, Y, Z) of that level."""
    lvl = dump["level"].astype(np.int64)
    sh = np.maximum(lvl - level, 0)
    m = lvl >= level
    for f, c in zip("XYZ", cell):
        m &= (dump[f].astype(np.int64) >> sh) == c
    return m


def inner_per_level(dump, mask=None):
    """{level: inner nodes} of a dump (of the nodes under `mask`)."""
    inner = dump["isLeaf"] == 0
    if mask is not None:
        inner = inner & mask
    lv, n = np.unique(dump["level"][inner], return_counts=True)
    return {int(a): int(b) for a, b in zip(lv, n)}


def inner_set(dump):
    inner = dump["isLeaf"] == 0
    return {(int(l), int(x), int(y), int(z)) for l, x, y, z in zip(dump["level"][inner], dump["X"][inner], dump["Y"][inner], dump["Z"][inner])}


def grant_model(counts3, max_nodes=None):
    """One ingest of `counts3` (cell_counts at level 3) into an empty octree whose node array holds `max_nodes` nodes (None: no limit).

    The root's slot holds 1 + 8 nodes: the root and its children.  From the counts alone the children over the limit split, and the grandchildren over the
    limit under them: every split takes eight nodes, and all of them are asked for at once.  Where they do not all fit, (capacity - in use) / 8 splits are
    granted: the children by octant, then the grandchildren of the children that do split, by (child, octant).  Then every level-3 node that exists and is
    over the limit asks for eight nodes (a slot of the next round), all at once; where they do not fit, (capacity - in use) / 8 are granted, to the first in
    local-node order (child, grandchild, octant).  Nothing of this input splits below level 3 (asserted by the caller from the counts).

    -> dict(num_nodes, inner: set of (level, X, Y, Z), want_splits, kept_splits, want_slots, kept_slots)"""
    c3 = np.asarray(counts3, dtype=np.int64)
    assert c3.shape == (8, 8, 8)
    c2 = c3.reshape(4, 2, 4, 2, 4, 2).sum(axis=(1, 3, 5))
    c1 = c2.reshape(2, 2, 2, 2, 2, 2).sum(axis=(1, 3, 5))
    assert c3.sum() > LIMIT, "the root splits"
    cap = np.iinfo(np.int64).max if max_nodes is None else int(max_nodes)
    used = 1 + 8
    assert used <= cap
    inner = {(0, 0, 0, 0)}
    # the cascade's wants, in the order a partial grant serves them
    children = [j for j in range(8) if c1[octant(j)] > LIMIT]
    at2 = lambda j, k: tuple(2 * a + b for a, b in zip(octant(j), octant(k)))
    grand = [(j, k) for j in children for k in range(8) if c2[at2(j, k)] > LIMIT]
    want = len(children) + len(grand)
    granted = want if used + 8 * want <= cap else min(want, (cap - used) // 8)
    kept1 = children[:granted]
    kept2 = [(j, k) for j, k in grand if j in kept1][:granted - len(kept1)]
    used += 8 * granted
    inner |= {(1,) + octant(j) for j in kept1} | {(2,) + at2(j, k) for j, k in kept2}
    # the level-3 nodes that exist (their parent split) and are still over the limit: local-node order = (child, grandchild, octant)
    at3 = lambda j, k, m: tuple(2 * a + b for a, b in zip(at2(j, k), octant(m)))
    slots = [(j, k, m) for j, k in kept2 for m in range(8) if c3[at3(j, k, m)] > LIMIT]
    fit = len(slots) if used + 8 * len(slots) <= cap else min(len(slots), (cap - used) // 8)
    used += 8 * fit
    inner |= {(3,) + at3(*s) for s in slots[:fit]}
    return dict(num_nodes=used, inner=inner, want_splits=want, kept_splits=len(kept1) + len(kept2), want_slots=len(slots), kept_slots=fit)
