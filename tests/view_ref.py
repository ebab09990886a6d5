"""Shared by the view-query tests (tests/test_view_io.py, test_view_rules.py, test_gpu_view.py): the cameras, uniforms whose minNodeSize is
scaled by a bias, the oracle's frame as a set of node keys, the 3 M-point terrain, and the guards that keep a comparison from passing on
nothing."""
import numpy as np

import cases
import oracle
from simlod_amd import abi, camera, synthetic
from util import node_keys

WIDTH, HEIGHT = 1920, 1080
MIN_NODE_SIZE = 64.0
CAMERAS = ["bird", "closer", "inside", "grazing", "away"]
TERRAIN_BOX = (600.0, 400.0, 40.0)
_BUILT = {}


def transform_of(which, box, offset=(0.0, 0.0, 0.0), width=WIDTH, height=HEIGHT):
    """The named camera of cases.camera_pose for a box of size `box` at `offset`.  `grazing` skims the synthetic terrain: on another box it
    is simply one more camera low inside the box."""
    return camera.lookat_transform(*cases.camera_pose(which, box, offset), width, height)


def uniforms_of(box, T, bias=0, box_min=(0.0, 0.0, 0.0), width=WIDTH, height=HEIGHT, frozen=None, show_points=True, **kw):
    """Uniforms of a frame with minNodeSize = 64 * 2^bias (exact in fp32): what rule V8 renders to compare a view query at `bias` with."""
    return abi.make_uniforms(width, height, T, box, transform_update_bound=frozen, min_node_size=MIN_NODE_SIZE * 2.0 ** bias, box_min=box_min,
                             show_points=show_points, **kw)


def terrain_3m_batches():
    """synthetic.terrain(3 000 000, seed 3) in batches of 1 M: 409 nodes, four levels below the root."""
    pts, box = synthetic.terrain(3_000_000, seed=3, box=TERRAIN_BOX, tile=50.0)
    return [pts[i:i + 1_000_000] for i in range(0, len(pts), 1_000_000)], box


def terrain_3m():
    """-> (full export, box, HostOctree) of the oracle-built 3 M terrain, once per session."""
    if "t3m" not in _BUILT:
        from region_ref import host_octree
        batches, box = terrain_3m_batches()
        ex, _, _, ho = host_octree(batches=batches, box=box)
        _BUILT["t3m"] = (ex, box, ho)
    return _BUILT["t3m"]


def oracle_visible(ho, u):
    """The oracle's frame of `u` on its own octree -> (sorted keys of the visible-node records, the samples they hold)."""
    ho.render(u)
    vis = ho.visible
    leaf = vis["numPoints"] > 0                                   # render.cu:748-754: a drawn node with points is drawn as a leaf
    return np.sort(node_keys(vis)), int(np.where(leaf, vis["numPoints"], vis["numVoxels"]).astype(np.int64).sum())


def selected_keys(ex):
    t = ex.nodes
    return np.sort(node_keys(t[(t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0]))


def ladder_of(full, u, **kw):
    """The mirror's ladder S(0..20) and counts record for the camera of `u`."""
    _, c = full.view(u, return_counts=True, **kw)
    return [int(v) for v in c["samplesAt"]], c


def first_zero(ladder):
    return next(b for b, s in enumerate(ladder) if s == 0)


def assert_closer_ladder(ladder):
    """The `closer` ladder of the 3 M terrain: at least four distinct non-zero rungs, and it ends at zero — the budget cases need both."""
    assert len({s for s in ladder if s > 0}) >= 4, ladder
    assert ladder[-1] == 0 and ladder[0] > ladder[1] > ladder[2] > 0, ladder


def assert_not_monotone(ladder):
    """-> the first b with S(b) < S(b + 1) (rule V6: S need not be monotone)."""
    ups = [b for b in range(len(ladder) - 1) if ladder[b] < ladder[b + 1]]
    assert ups, ladder
    return ups[0]


def complete_tree(depth=4, seed=7):
    """A complete 8-ary tree down to `depth` in the unit box as a full export, made by hand: (8^(depth+1) - 1) / 7 entries in breadth-first
    order, one to three samples per entry at the node's centre.  Level 4 lists 4 096 entries: several turns of a 1 024-lane walk, and the
    parents of one turn's entries lie in another's."""
    rs = np.random.RandomState(seed)
    levels = [np.zeros((1, 3), np.int64)]
    for _ in range(depth):
        p = levels[-1]
        k = np.arange(8)
        oct_ = np.stack([(k >> 2) & 1, (k >> 1) & 1, k & 1], axis=1)                  # octant k: bit 2 -> X, bit 1 -> Y, bit 0 -> Z
        levels.append((2 * p[:, None, :] + oct_[None, :, :]).reshape(-1, 3))
    n = sum(len(l) for l in levels)
    t = np.zeros(n, dtype=abi.export_node_dtype)
    first = np.cumsum([0] + [len(l) for l in levels])
    for L, xyz in enumerate(levels):
        a = slice(first[L], first[L + 1])
        i = np.arange(len(xyz))
        t["level"][a], t["X"][a], t["Y"][a], t["Z"][a] = L, xyz[:, 0], xyz[:, 1], xyz[:, 2]
        t["parent"][a] = abi.EXPORT_NONE if L == 0 else first[L - 1] + i // 8
        inner = L < depth
        t["firstChild"][a] = first[L + 1] + 8 * i if inner else abi.EXPORT_NONE
        t["childMask"][a] = 0xFF if inner else 0
        t["flags"][a] = abi.EXPORT_FLAG_SELECTED | (0 if inner else abi.EXPORT_FLAG_LEAF)
    t["numSamples"] = rs.randint(1, 4, size=n)
    ns = t["numSamples"].astype(np.int64)
    t["firstSample"] = np.concatenate([[0], np.cumsum(ns)[:-1]])
    s = np.zeros(int(ns.sum()), dtype=abi.point_dtype)
    owner = np.repeat(np.arange(n), ns)
    size = np.ldexp(1.0, -t["level"].astype(np.int64))
    for a, A in zip("xyz", "XYZ"):
        s[a] = ((t[A] + 0.5) * size)[owner]
    s["color"] = rs.randint(0, 1 << 24, size=len(s))
    from simlod_amd.octree_io import OctreeExport
    return OctreeExport(t, s, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
