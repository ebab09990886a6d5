"""The mirror of a clipped frame (include/simlod_hip.h, "clip regions", rule C3): the oracle's own rasteriser, unchanged, on an EDITED copy of a
host-addressed octree image.  Emptied nodes get numPoints = numVoxels = 0; a removed sample is relocated to NaN coordinates (the oracle then
draws nothing for it and the node's counts stay — tests/test_clip_rules.py keeps the guard that an all-NaN octree draws 0 pixels); a highlighted
sample gets the clip's colour word.  Node classes come from octree_io.classify_nodes, the per-sample test from region_ref.brute_mask."""
import numpy as np

import oracle
from region_ref import brute_mask
from simlod_amd import abi
from simlod_amd.octree_io import classify_nodes

CHUNK_BYTES, CHUNK_NEXT = 16016, 16008            # a chunk: 1 000 samples of 16 bytes, a size word, `next`
OUTSIDE, FILTERED, COPIED = 0, 1, 2
LISTS = (("points", "numPoints"), ("voxelChunks", "numVoxels"))


def copy_image(nodes, pers, nn, used=None):
    """A private copy of a HOST-addressed image (the first `used` bytes of its persistent buffer: all that is allocated), its pointers rebased to the copies."""
    n2, p2 = nodes[:nn].copy(), pers[:used].copy()
    oracle.rebase_image(n2, nn, p2, nodes.ctypes.data, pers.ctypes.data)
    return n2, p2


def chunk_views(pers, head, count):
    """The samples of a chunk list as writable abi.point_dtype views into `pers`, chunk by chunk (oracle.gather_samples' walk)."""
    base = pers.ctypes.data
    left, p = int(count), int(head)
    while left > 0 and p != 0:
        off = p - base
        assert 0 <= off and off + CHUNK_BYTES <= pers.size, "a chunk outside the image's persistent buffer"
        n = min(left, abi.POINTS_PER_CHUNK)
        yield pers[off: off + 16 * n].view(abi.point_dtype)
        left -= n
        p = int(pers[off + CHUNK_NEXT: off + CHUNK_NEXT + 8].view(np.uint64)[0])


def node_classes(nodes, nn, region, u):
    """OUTSIDE / FILTERED / COPIED per node record (rules 1 and 4), each from its own (level, X, Y, Z)."""
    uu = np.ascontiguousarray(u).reshape(1)
    outside, inside = classify_nodes(region.planes.astype(np.float64), nodes[:nn], np.asarray(uu["boxMin"][0].tolist()[:3], np.float32),
                                     np.asarray(uu["boxMax"][0].tolist()[:3], np.float32))
    return np.where(outside, OUTSIDE, np.where(inside, COPIED, FILTERED))


class ClippedImage:
    """nodes / pers / nn: the edited image (host-addressed).  cls: the class of every node; emptied: the nodes the clip emptied; tested: per
    FILTERED node with samples, [(samples before the edit, in chunk order, passing mask)] for its point list and its voxel list."""

    def __init__(self, nodes, pers, nn, cls, emptied, tested):
        self.nodes, self.pers, self.nn, self.cls, self.emptied, self.tested = nodes, pers, nn, cls, emptied, tested


def clip_image(nodes, pers, nn, clip, u, used=None):
    """The table of rule C3 applied to a copy of the image."""
    n2, p2 = copy_image(nodes, pers, nn, used)
    cls = node_classes(n2, nn, clip.region, u)
    has = (n2["numPoints"][:nn] > 0) | (n2["numVoxels"][:nn] > 0)
    mode = abi.CLIP_MODES[clip.mode]
    emptied = np.zeros(nn, bool)
    if mode == abi.CLIP_INSIDE:
        emptied = has & (cls == OUTSIDE)
    elif mode == abi.CLIP_OUTSIDE:
        emptied = has & (cls == COPIED)
    tested = {}
    if mode != abi.CLIP_OFF:
        touch = has & ~emptied & ((cls == FILTERED) | ((mode == abi.CLIP_HIGHLIGHT) & (cls == COPIED)))
        for i in np.nonzero(touch)[0]:
            for head, count in LISTS:
                for v in chunk_views(p2, n2[head][i], n2[count][i]):
                    if cls[i] == COPIED:                                   # (HIGHLIGHT)
                        v["color"] = clip.color
                        continue
                    before = v.copy()
                    with np.errstate(invalid="ignore"):
                        ok = brute_mask(clip.region, before)
                    tested.setdefault(int(i), []).append((before, ok))
                    if mode == abi.CLIP_HIGHLIGHT:
                        v["color"][ok] = clip.color
                    else:
                        gone = ~ok if mode == abi.CLIP_INSIDE else ok
                        for a in "xyz":
                            v[a][gone] = np.nan
        n2["numPoints"][:nn][emptied] = 0
        n2["numVoxels"][:nn][emptied] = 0
    return ClippedImage(n2, p2, nn, cls, emptied, tested)


def kept_samples(img, i):
    """The samples of node i the edited image still holds (finite ones), in chunk order: point list, then voxel list."""
    parts = [v[np.isfinite(v["x"])] for head, count in LISTS for v in chunk_views(img.pers, img.nodes[head][i], img.nodes[count][i])]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=abi.point_dtype)


def all_samples_to_nan(nodes, pers, nn, used=None):
    """A copy of the image with EVERY sample relocated to NaN, counts untouched."""
    n2, p2 = copy_image(nodes, pers, nn, used)
    for i in range(nn):
        for head, count in LISTS:
            for v in chunk_views(p2, n2[head][i], n2[count][i]):
                for a in "xyz":
                    v[a] = np.nan
    return n2, p2
