"""The batch-aware voxel colour check (tests/util.py: tag_colors, first_hit_batches, assert_voxel_winners) on the port oracle's own octrees.

BASELINE.md §3: a voxel's colour is the colour of a point of the FIRST batch that hit its cell.  With tagged inputs (colour = point index) the
oracle's image must meet that rule exactly, and the checker must reject an image in which a voxel was recoloured to a point of a later batch,
to a point outside its cell, or — deep in the tree, where the old membership check gave up — to the point of the neighbouring cell."""
import ctypes

import numpy as np
import pytest

import oracle
from cases import CASES, batches_of, case, uniforms_for
from simlod_amd import abi, camera, synthetic
from util import (STATS_BUILD_FIELDS, assert_stats_equal, assert_voxel_winners, batch_of_points, first_hit_batches, replay_first_hits,
                  tag_colors, voxel_colors_are_member)

_CACHE = {}


def _tight(b):
    return b


def _terrain_2m():
    pts, box = synthetic.terrain(2_000_000, seed=21, box=(1500.0, 1000.0, 100.0), tile=125.0)
    T = camera.lookat_transform((1.8 * box[0], -1.2 * box[1], 1.4 * max(box)), (0.5 * box[0], 0.5 * box[1], 0.3 * box[2]), 256, 256)
    return pts, box, 250_000, T


def _deep_cluster():
    """60 000 points in one level-16 cell near the origin of the unit cube (+ 2 000 spread over the cube): the root's split cascades down to
    level 16, whose 128^3 grid has cells of 2^-23 — positions there still resolve neighbouring cells, so the cell check can be seen to bite."""
    rs = np.random.RandomState(4)
    side, corner = np.float32(2.0 ** -16), np.float32(3 * 2.0 ** -10)
    v = corner + rs.random_sample((60_000, 3)).astype(np.float32) * side
    v = np.minimum(v, np.nextafter(corner + side, np.float32(0)))
    w = np.minimum(rs.random_sample((2_000, 3)).astype(np.float32), np.float32(0.999999))
    xyz = np.concatenate([w[:1_000], v, w[1_000:]])
    pts = np.zeros(len(xyz), dtype=abi.point_dtype)
    pts["x"], pts["y"], pts["z"] = xyz.T
    box = (1.0, 1.0, 1.0)
    return pts, box, 31_000, camera.lookat_transform((1.8, -1.2, 1.4), (0.5, 0.5, 0.3), 256, 256)


def _run(name):
    """(tagged points, batches, uniforms, HostOctree after the batch-by-batch replay, first-hit table), cached per input."""
    if name not in _CACHE:
        if name == "terrain_2m":
            pts, box, batch, T = _terrain_2m()
        elif name == "deep_cluster":
            pts, box, batch, T = _deep_cluster()
        else:
            pts, box, batch, T = case(name)
        tagged = tag_colors(pts)
        batches = batches_of(name, tagged, batch)
        u = uniforms_for(box, T)
        ref, fh = replay_first_hits(u, batches)
        _CACHE[name] = (tagged, batches, u, ref, fh)
    return _CACHE[name]


def _check(name, bound=_tight):
    tagged, batches, u, ref, fh = _run(name)
    nn = int(ref.stats["numNodes"][0])
    return assert_voxel_winners(ref.nodes, nn, tagged, batch_of_points(batches), fh, bound, u)


def _voxel_color_address(ref, node_index, slot):
    """Host address of the colour word of voxel `slot` of a node of the oracle's image (chunks of 1 000 samples, `next` at byte 16 008)."""
    chunk = int(ref.nodes["voxelChunks"][node_index])
    for _ in range(slot // abi.POINTS_PER_CHUNK):
        chunk = ctypes.c_uint64.from_address(chunk + 16 * abi.POINTS_PER_CHUNK + 8).value
    return chunk + 16 * (slot % abi.POINTS_PER_CHUNK) + 12


class _Recoloured:
    """Recolour one voxel of a cached oracle image for the duration of a `with` block."""

    def __init__(self, ref, node_index, slot, color):
        self.word = ctypes.c_uint32.from_address(_voxel_color_address(ref, node_index, slot))
        self.color = color

    def __enter__(self):
        self.old, self.word.value = self.word.value, self.color

    def __exit__(self, *exc):
        self.word.value = self.old


def _node_voxels(ref, i):
    nd = ref.nodes[i]
    return oracle.gather_samples(int(nd["voxelChunks"]), int(nd["numVoxelsStored"]))


def _cells_of_all(u, tagged, nd):
    return oracle.voxel_cells(u, tagged, int(nd["level"]), int(nd["X"]), int(nd["Y"]), int(nd["Z"]))[0]


# ---- the oracle's own image meets the reference's rule -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES + ["terrain_2m"])
def test_oracle_voxels_are_coloured_by_the_first_batch_that_hit_their_cell(built_libs, name):
    tagged, batches, u, ref, fh = _run(name)
    nn = int(ref.stats["numNodes"][0])
    assert _check(name) == int(ref.nodes["numVoxelsStored"][:nn].sum()) == len(fh) > 0
    if len(batches) > 1:                   # (hotspot_150k is one batch)
        assert len(np.unique(fh["batch"])) > 1, "a single batch made every voxel: the check would have nothing to tell apart"
    # tagging changes no construction decision: the batch-by-batch replay of the tagged points is the untagged octree, counters and all
    pts, box, batch, T = _terrain_2m() if name == "terrain_2m" else case(name)
    plain = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=abi.BATCH_STREAM_SIZE)
    plain.reset(u)
    for b in batches_of(name, pts, batch):
        plain.upload(b)
        plain.construct(u)
    assert_stats_equal(ref.stats[0], plain.stats[0], STATS_BUILD_FIELDS, name)
    a, b = ref.dump(), plain.dump()
    for f in oracle.dump_dtype.names:
        if f not in ("pointsSum", "pointsXor"):
            assert np.array_equal(a[f], b[f]), f


def test_first_hit_batches_is_the_replays_table(built_libs):
    tagged, batches, u, ref, fh = _run("uniform_3x40k")
    assert np.array_equal(first_hit_batches(u, batches), fh)


def test_duplicate_root_voxels_of_a_root_that_split_are_paired(built_libs):
    """ragged_tiny: the root samples itself while it is a leaf, and the batch that splits it (the 50 001st point) clears its grid and samples
    everything again — the root holds two voxels in many cells, made by different batches; both are paired with the oracle's."""
    tagged, batches, u, ref, fh = _run("ragged_tiny")
    root = fh[fh["level"] == 0]
    grp = np.stack([root[f] for f in ("cell", "x", "y", "z")], axis=1)
    _, first, counts = np.unique(grp, axis=0, return_index=True, return_counts=True)
    assert counts.max() == 2 and (counts == 2).sum() > 1000
    dup = np.isin(np.arange(len(root)), first[counts == 2])
    split_batch = 4                        # batches: 1, 7, 0, 49 992, then the point that crosses 50 000
    assert (root["batch"][dup] < split_batch).all()
    assert (root["batch"][np.isin(np.arange(len(root)), first[counts == 2] + 1)] == split_batch).all()
    assert _check("ragged_tiny") == len(fh)


# ---- the checker fails where it must ----------------------------------------------------------------------------------------------------
def test_a_voxel_recoloured_to_a_later_batch_of_its_cell_fails(built_libs):
    tagged, batches, u, ref, fh = _run("terrain_4x100k")
    bop = batch_of_points(batches)
    nn = int(ref.stats["numNodes"][0])
    for i in np.argsort(ref.nodes["level"][:nn], kind="stable"):
        nd = ref.nodes[i]
        if int(nd["numVoxelsStored"]) == 0 or int(nd["level"]) == 0:       # (below the root a cell holds one voxel)
            continue
        vox, cells = _node_voxels(ref, i), _cells_of_all(u, tagged, nd)
        win_cells = cells[vox["color"].astype(np.int64)]
        mine = fh[(fh["level"] == nd["level"]) & (fh["key"] == (int(nd["X"]) << 40 | int(nd["Y"]) << 20 | int(nd["Z"])))]
        bstar = mine["batch"][np.searchsorted(mine["cell"], win_cells)].astype(np.int64)
        latest = np.full(128 ** 3, -1, np.int64)
        inside = cells != 0xFFFFFFFF
        np.maximum.at(latest, cells[inside].astype(np.int64), np.arange(len(tagged))[inside])
        # a voxel whose cell a point of a batch after its first-hit batch hit as well
        cand = np.nonzero(bop[latest[win_cells]].astype(np.int64) > bstar)[0]
        if len(cand):
            s = int(cand[0])
            q = int(latest[win_cells[s]])
            break
    else:
        pytest.fail("no cell hit by two batches")
    with _Recoloured(ref, i, s, q):
        with pytest.raises(AssertionError, match="later batch than the bound allows"):
            _check("terrain_4x100k")
        # (the membership check accepts it: the point does lie in the cell)
        assert voxel_colors_are_member(ref.nodes, nn, tagged, tuple(np.ravel(u["boxMax"]))) == len(fh)
    _check("terrain_4x100k")


def test_a_voxel_recoloured_to_a_point_outside_its_cell_fails(built_libs):
    tagged, batches, u, ref, fh = _run("uniform_3x40k")
    nn = int(ref.stats["numNodes"][0])
    i = int(np.nonzero(ref.nodes["numVoxelsStored"][:nn] > 1)[0][-1])
    vox = _node_voxels(ref, i)
    with _Recoloured(ref, i, 0, int(vox["color"][1])):       # the winner of another voxel of the same node
        with pytest.raises(AssertionError, match="outside the voxel's cell"):
            _check("uniform_3x40k")
    assert _check("uniform_3x40k") == len(fh)


def test_a_deep_voxel_recoloured_to_its_neighbour_cells_point_fails(built_libs):
    tagged, batches, u, ref, fh = _run("deep_cluster")
    nn = int(ref.stats["numNodes"][0])
    levels = ref.nodes["level"][:nn].astype(np.int64)
    levels[ref.nodes["numVoxelsStored"][:nn] == 0] = -1
    i = int(np.argmax(levels))
    nd = ref.nodes[i]
    assert int(nd["level"]) == 16
    vox, cells = _node_voxels(ref, i), _cells_of_all(u, tagged, nd)
    owner = np.full(128 ** 3, -1, np.int64)
    inside = cells != 0xFFFFFFFF
    owner[cells[inside].astype(np.int64)] = np.arange(len(tagged))[inside]
    wc = cells[vox["color"].astype(np.int64)].astype(np.int64)
    nb = np.where(wc % 128 < 127, wc + 1, wc - 1)              # the x-neighbour inside the node's grid
    s = int(np.nonzero(owner[nb] >= 0)[0][0])
    with _Recoloured(ref, i, s, int(owner[nb[s]])):
        with pytest.raises(AssertionError, match="outside the voxel's cell"):
            _check("deep_cluster")
    assert _check("deep_cluster") == len(fh)
