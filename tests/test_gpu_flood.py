"""A root cascade that floods k_expand's widened build paths, against the port oracle the way tests/test_gpu_groups.py compares: every Node field,
every build counter of Stats.

ONE exact group of four batches (3 x 1 M + 990 000 points) goes into an empty octree:
  * 72 level-3 cells hold 55 000 uniform points each — still too full after the three levels the root's slot settles: 72 slots of the next round out of
    ONE slot (more than a wave of them: one reservation, one counted grid allocation, their histograms zeroed by the whole workgroup);
  * 100 further level-3 cells hold 300 points each — more than 64 fresh leaves in the root's slot (their chunks: several waves of alloc_points in one turn);
  * two dense and two or three sparse cells share a level-2 cell (36 of them, so that every sparse cell's parent splits); the octant (1, 1, 1) of the root
    stays empty: a new leaf at level 1, two levels and more above the top table's — with the 500 level-3 leaves around it the whole-workgroup fill of
    the top table has entries of every size.
The preconditions are asserted from the ORACLE's octree before anything is compared, so the test cannot pass without the paths having run.  The same
case runs with the trunk mask of a multi-GPU job whose other ranks fill the rest of the box (every node of levels 0-2 named: the empty octant splits twice
by the mask alone and all 512 level-3 nodes exist)."""
import numpy as np
import pytest

import oracle
from simlod_amd import abi
from test_gpu_groups import GROUP_MOMENTARY, GROUP_PERSISTENT, _cam, _compare, _drive
from test_gpu_parity import _device
from cases import H, W

DENSE_CELLS, DENSE_POINTS = 72, 55_000
SPARSE_CELLS, SPARSE_POINTS = 100, 300
CONCENTRATED_POINTS = 52_000
BATCH = 1_000_000
G = 4
ALL_TRUNK_NODES = ((1 << 64) - 1, (1 << 9) - 1)      # simlod_context_set_trunk_mask: bit 0 the root, 1 + c the level-1 nodes, 9 + c the level-2 nodes
_CASE = {}


def flood_case(dense=DENSE_CELLS, sparse=SPARSE_CELLS, concentrated=0, seed=23):
    """-> (points, box, batches, level-3 cells (x, y, z) that are dense, ... that are sparse).  `dense` / `sparse`: how many of each, spread evenly over the 36
    level-2 cells (at least one dense cell in each: every sparse cell's parent splits).  `concentrated`: in that many of the first dense cells CONCENTRATED_POINTS
    of the cell's points lie in its level-6 subcell (3, 3, 3), at the same fractional offsets — the cell's cascade goes three levels further down."""
    key = (dense, sparse, concentrated, seed)
    if key in _CASE:
        return _CASE[key]
    ndense, nsparse_all = dense, sparse
    rs = np.random.RandomState(seed)
    l2 = [(x, y, z) for x in range(4) for y in range(4) for z in range(4) if not (x >= 2 and y >= 2 and z >= 2)]      # (the level-2 cells outside octant (1, 1, 1))
    assert len(l2) == 56
    l2 = [l2[i] for i in rs.permutation(56)[:36]]
    dense, sparse = [], []
    for i, (x, y, z) in enumerate(l2):
        kids = rs.permutation(8)
        nd = ndense // 36 + (1 if i < ndense % 36 else 0)                  # (the default: 2)
        nsparse = nsparse_all // 36 + (1 if i < nsparse_all % 36 else 0)      # (the default: 3 if i < 28 else 2)
        assert nd >= 1 and nd + nsparse <= 8
        for k in kids[:nd]:
            dense.append((2 * x + (k >> 2 & 1), 2 * y + (k >> 1 & 1), 2 * z + (k & 1)))
        for k in kids[nd:nd + nsparse]:
            sparse.append((2 * x + (k >> 2 & 1), 2 * y + (k >> 1 & 1), 2 * z + (k & 1)))
    assert len(dense) == ndense and len(sparse) == nsparse_all and len(set(dense + sparse)) == ndense + nsparse_all
    cells = np.concatenate([np.repeat(np.asarray(dense, dtype=np.float32), DENSE_POINTS, axis=0), np.repeat(np.asarray(sparse, dtype=np.float32), SPARSE_POINTS, axis=0)])
    n = len(cells)
    assert n == ndense * DENSE_POINTS + nsparse_all * SPARSE_POINTS and (G - 1) * BATCH < n <= G * BATCH
    assert key != (DENSE_CELLS, SPARSE_CELLS, 0, 23) or n == 3_990_000
    v = (rs.random_sample((n, 3)) * 0.998 + 0.001).astype(np.float32)      # (strictly inside its cell: no sample on a cell's face)
    p = (cells + v) * np.float32(0.125)
    assert concentrated <= ndense
    for d in range(concentrated):                     # (the dense cells' points come first, cell by cell)
        s = slice(d * DENSE_POINTS, d * DENSE_POINTS + CONCENTRATED_POINTS)
        p[s] = (cells[s] + (np.float32(3.0) + v[s]) * np.float32(0.125)) * np.float32(0.125)
    c = np.floor(v * np.float32(255.0)).astype(np.uint32)
    pts = np.empty(n, dtype=abi.point_dtype)
    pts["x"], pts["y"], pts["z"] = p[:, 0], p[:, 1], p[:, 2]
    pts["color"] = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | np.uint32(255 << 24)
    pts = pts[rs.permutation(n)]                      # every batch of the group holds a quarter of every cell
    batches = [pts[i:i + BATCH] for i in range(0, n, BATCH)]
    assert len(batches) == G
    _CASE[key] = (pts, np.array([1, 1, 1], dtype=np.float32), batches, dense, sparse)
    return _CASE[key]


def _oracle(u, batches, mask):
    ref = oracle.HostOctree("port", persistent_bytes=GROUP_PERSISTENT)
    ref.reset(u)
    if mask is not None:
        ref.set_trunk_mask(*mask)
    for b in batches:
        ref.upload(b)
        ref.construct(u)
    assert ref.last_error() == 0 and int(ref.stats["batchletIndex"][0]) == len(batches)
    return ref


def assert_flood_preconditions(dump, dense, sparse, masked):
    """What the oracle's octree must look like for the device's ingest of the group to have taken the widened paths."""
    lvl, leaf, pts = dump["level"], dump["isLeaf"] != 0, dump["numPoints"]
    cell = lambda i: (int(dump["X"][i]), int(dump["Y"][i]), int(dump["Z"][i]))
    # the root's slot settles levels 1-3; an inner node at level 3 was still too full after them: a slot of the next round — exactly the dense cells
    inner3 = {cell(i) for i in np.nonzero((lvl == 3) & ~leaf)[0]}
    assert inner3 == set(dense) and len(inner3) == DENSE_CELLS > 64
    assert not np.any((lvl >= 4) & ~leaf), "the cascade ends with the second round"
    # the fresh leaves of the root's slot: the nodes of levels 1-3 that hold samples and stay leaves — the sparse cells
    fresh = {cell(i) for i in np.nonzero((lvl >= 1) & (lvl <= 3) & leaf & (pts > 0))[0]}
    assert fresh == set(sparse) and len(fresh) == SPARSE_CELLS > 64
    assert np.all(pts[(lvl == 3) & leaf & (pts > 0)] == SPARSE_POINTS)
    # new leaves two levels and more above the top table's level: the entries of the whole-workgroup fill
    if masked:
        assert int(((lvl == 3)).sum()) == 512 and int((lvl <= 2).sum()) == 73 and not np.any((lvl <= 2) & leaf)
    else:
        assert any(cell(i) == (1, 1, 1) for i in np.nonzero((lvl == 1) & leaf & (pts == 0))[0]), "the empty octant: a leaf at level 1 (4096 cells of the top table)"
        assert int(((lvl == 3) & leaf).sum()) > 64


def test_flood_case_yields_the_layout_in_the_oracle(built_libs):
    """CPU: the case really has the counts its arithmetic promises — with and without the mask."""
    pts, box, batches, dense, sparse = flood_case()
    u = abi.make_uniforms(W, H, _cam(box), box, persistent_capacity=GROUP_PERSISTENT, momentary_capacity=GROUP_MOMENTARY)
    for mask in (None, ALL_TRUNK_NODES):
        assert_flood_preconditions(_oracle(u, batches, mask).dump(), dense, sparse, mask is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "trunk_mask"])
def test_one_group_floods_the_root_cascade_and_builds_the_oracles_octree(built_libs, masked):
    pts, box, batches, dense, sparse = flood_case()
    mask = ALL_TRUNK_NODES if masked else None
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", G)
        u = dev.uniforms(W, H, _cam(box), box)
        ref = _oracle(u, batches, mask)
        assert_flood_preconditions(ref.dump(), dense, sparse, masked)
        if masked:
            dev.set_trunk_mask(*mask)                  # (the mask belongs to the context: the reset in _drive leaves it)
        ends, taken, sizes = _drive(dev, u, batches, G)
        assert ends == [G] and taken == [G] and sizes == [G] and dev.groups_ingested() == 1, f"one launch, one group of {G}: {ends} {taken} {sizes}"
        nodes, pers, nn = _compare(dev, f"flood masked={masked}", ref)
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()
