"""Ancestor paths across the end of a node's row (construct_state.inc: a row holds a node's first PATH_DIRECT ancestors; a deeper node continues in
the row of its PATH_DIRECT-th ancestor), against the port oracle the way tests/test_gpu_groups.py and tests/test_gpu_flood_edges.py compare: the
whole dump, the build fields of Stats, the structural invariants.

Four seeded batches into ONE cell of level `cell_level` at the origin of a unit box (every point strictly inside its cell of level cell_level + 2):
  A   60 000 points: the root's chain of splits ends in eight leaves at level cell_level + 1 — with cell_level + 1 == PATH_DIRECT their rows are
      exactly full: no terminator, no continuation;
  B  400 000 more: every one of those leaves crosses 50 000 and splits — 64 leaves at level cell_level + 2, whose paths need the continuation, written
      by k_expand for slots whose own node sits on the boundary (batch by batch) or across a cascade that straddles it (one group);
  C  100 000 more, about 1 500 per leaf: k_voxelize's piece path reads those paths;
  D    2 000 more, about 30 per leaf: the small-item path does.
The library does not export its PATH_DIRECT, so the levels are chosen for the two row lengths the project considers: cell_level 11 puts the boundary
where the default build has it (PATH_DIRECT = 12: leaves at 12, then 13), cell_level 9 where a build with PATH_DIRECT = 10 has it (leaves at 10, then
11; the default build reads both whole from the row).  Each case is driven three ways: batch by batch, as one exact group of four, and batch by batch
with the side tables thrown away between B and C, so that k_begin's rebuild writes the continued rows the later batches read.
The preconditions come from the input's arithmetic and from the ORACLE's own dumps, before anything is compared.  All comparisons are equalities."""
import numpy as np
import pytest

import oracle
from cases import H, W
from simlod_amd import abi
from test_gpu_groups import GROUP_MOMENTARY, GROUP_PERSISTENT, _cam, _compare, _drive
from test_gpu_parity import _device

SIZES = (60_000, 400_000, 100_000, 2_000)      # A, B, C, D
LIMIT = 50_000                                 # a leaf splits when it holds more (voxels.cu:209-217)
VOX_SMALL = 512                                # construct_expand.inc: a leaf with fewer new samples goes the wave-per-leaf way
CELL_LEVELS = [11, 9]
OFF_ORIGIN_MARGIN = 1.0 / 64.0                 # of a cell of level cell_level + 2, off the origin: far more than the fp32 rounding of a coordinate there
_CASES, _REFS = {}, {}


def deep_case(cell_level, scale=1.0, cell=None):
    """-> (box, [A, B, C, D], per batch the 64 counts of the cells of level cell_level + 2, index x << 4 | y << 2 | z)
    `scale` (a power of two) is the size of the box; `cell` the cell of level cell_level the points go into, (0, 0, 0) by default.  Off the
    origin a coordinate is formed in fp64 and rounded to fp32, so the margin that keeps a point strictly inside its cell is wider there."""
    key = (cell_level, float(scale), None if cell is None else tuple(int(c) for c in cell))
    if key not in _CASES:
        rs = np.random.RandomState(100 + cell_level)
        assert np.frexp(float(scale))[0] == 0.5, "the box size is a power of two"
        size = np.float32(float(scale) * 2.0 ** -(cell_level + 2))                 # of a cell of level cell_level + 2
        batches, counts = [], []
        for n in SIZES:
            sub = rs.randint(0, 4, size=(n, 3))
            r = rs.random_sample((n, 3))
            if cell is None:
                v = (r * 0.998 + 0.001).astype(np.float32)                         # strictly inside the cell: no sample on a face
                p = (sub.astype(np.float32) + v) * size                            # (a power of two: exact)
                want = sub
            else:
                assert all(0 <= int(c) < 1 << cell_level for c in cell)
                v = r * (1.0 - 2.0 * OFF_ORIGIN_MARGIN) + OFF_ORIGIN_MARGIN
                want = sub + 4 * np.asarray(cell, dtype=np.int64)
                p = ((want.astype(np.float64) + v) * np.float64(size)).astype(np.float32)
                v = v.astype(np.float32)
            assert np.array_equal(np.floor(p.astype(np.float64) / np.float64(size)).astype(np.int64), want)
            c = np.floor(v * np.float32(255.0)).astype(np.uint32)
            pts = np.empty(n, dtype=abi.point_dtype)
            pts["x"], pts["y"], pts["z"] = p[:, 0], p[:, 1], p[:, 2]
            pts["color"] = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | np.uint32(255 << 24)
            batches.append(pts)
            counts.append(np.bincount(sub[:, 0] << 4 | sub[:, 1] << 2 | sub[:, 2], minlength=64))
        _CASES[key] = (np.array([scale, scale, scale], dtype=np.float32), batches, counts)
    return _CASES[key]


def _upper(counts64):
    """counts of the 64 cells -> of the eight cells one level up"""
    i = np.arange(64)
    return np.bincount((i >> 5 & 1) << 2 | (i >> 3 & 1) << 1 | (i >> 1 & 1), weights=counts64, minlength=8).astype(np.int64)


def assert_input_arithmetic(counts):
    a, b, c, d = counts
    assert np.all(_upper(a) > 0) and np.all(_upper(a) <= LIMIT) and int(a.sum()) == SIZES[0] > LIMIT, "A: the cell splits, its eight children do not"
    assert np.all(_upper(a + b) > LIMIT) and np.all(a + b <= LIMIT), "B: every child splits, no grandchild does"
    assert np.all(c >= VOX_SMALL), "C: every leaf gets a piece"
    assert np.all(d > 0) and np.all(d < VOX_SMALL), "D: every leaf gets a small item"
    assert np.all(a + b + c + d <= LIMIT), "nothing splits after B"


class _Reference:
    def __init__(self, ref, after):
        self.stats, self._dump, self.after = ref.stats.copy(), ref.dump(), after

    def dump(self):
        return self._dump


def _uniforms(box):
    return abi.make_uniforms(W, H, _cam(box), box, persistent_capacity=GROUP_PERSISTENT, momentary_capacity=GROUP_MOMENTARY)


def _reference(cell_level, u, batches):
    """The port oracle after the four batches, one at a time, and its dump after each of them — once per case."""
    if cell_level not in _REFS:
        ref = oracle.HostOctree("port", persistent_bytes=GROUP_PERSISTENT)
        ref.reset(u)
        after = []
        for b in batches:
            ref.upload(b)
            ref.construct(u)
            after.append(ref.dump())
        assert ref.last_error() == 0 and int(ref.stats["batchletIndex"][0]) == len(batches)
        _REFS[cell_level] = _Reference(ref, after)
    return _REFS[cell_level]


def _leaves(dump):
    """non-empty leaves per level"""
    sel = (dump["isLeaf"] != 0) & (dump["numPoints"] > 0)
    return {int(l): int((sel & (dump["level"] == l)).sum()) for l in np.unique(dump["level"][sel])}


def assert_oracle_preconditions(ref, cell_level, counts):
    """From the oracle's own dumps: where the non-empty leaves are after A and from B on, how many, and what each holds."""
    assert_input_arithmetic(counts)
    edge = cell_level + 1
    assert _leaves(ref.after[0]) == {edge: 8}, "after A: eight non-empty leaves, all at the level whose paths fill a row exactly"
    assert int(ref.after[0]["level"].max()) == edge and len(ref.after[0]) == 1 + 8 * edge, "a chain of splits from the root to the cell"
    total = np.zeros(64, dtype=np.int64)
    for k, dump in enumerate(ref.after):
        total += counts[k]
        if k == 0:
            continue
        assert _leaves(dump) == {edge + 1: 64}, "from B on: 64 non-empty leaves one level further down, none left above"
        assert len(dump) == 1 + 8 * edge + 64 and int(((dump["level"] == edge) & (dump["isLeaf"] == 0)).sum()) == 8
        sel = (dump["level"] == edge + 1) & (dump["isLeaf"] != 0)
        assert np.all(dump["X"][sel] < 4) and np.all(dump["Y"][sel] < 4) and np.all(dump["Z"][sel] < 4)
        got = np.zeros(64, dtype=np.int64)
        got[dump["X"][sel].astype(np.int64) << 4 | dump["Y"][sel].astype(np.int64) << 2 | dump["Z"][sel].astype(np.int64)] = dump["numPoints"][sel]
        assert np.array_equal(got, total), f"after batch {k}: the leaves hold the input's counts"


@pytest.mark.parametrize("cell_level", CELL_LEVELS)
def test_deep_case_yields_its_leaves_in_the_oracle(built_libs, cell_level):
    """CPU: the input has the counts its arithmetic promises, and the oracle's octree has its leaves on both sides of the boundary."""
    box, batches, counts = deep_case(cell_level)
    assert_oracle_preconditions(_reference(cell_level, _uniforms(box), batches), cell_level, counts)


def _finish(dev, ref, name):
    nodes, pers, nn = _compare(dev, name, ref)
    oracle.check_invariants(nodes, nn)


@pytest.mark.gpu
@pytest.mark.parametrize("cell_level", CELL_LEVELS)
def test_batch_by_batch_across_the_end_of_a_path_row_builds_the_oracles_octree(built_libs, cell_level):
    box, batches, counts = deep_case(cell_level)
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", 1)
        u = dev.uniforms(W, H, _cam(box), box)
        ref = _reference(cell_level, u, batches)
        assert_oracle_preconditions(ref, cell_level, counts)
        ends, taken, sizes = _drive(dev, u, batches, 1)
        assert ends == [1, 2, 3, 4] and taken == [1, 1, 1, 1] and dev.groups_ingested() == 4, f"four launches of one batch: {ends} {taken} {sizes}"
        _finish(dev, ref, f"deep paths, cell level {cell_level}, batch by batch")
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cell_level", CELL_LEVELS)
def test_one_group_of_four_across_the_end_of_a_path_row_builds_the_oracles_octree(built_libs, cell_level):
    box, batches, counts = deep_case(cell_level)
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", 4)
        u = dev.uniforms(W, H, _cam(box), box)
        ref = _reference(cell_level, u, batches)
        assert_oracle_preconditions(ref, cell_level, counts)
        ends, taken, sizes = _drive(dev, u, batches, 4)
        assert ends == [4] and taken == [4] and sizes == [4] and dev.groups_ingested() == 1, f"one launch, one group of four: {ends} {taken} {sizes}"
        _finish(dev, ref, f"deep paths, cell level {cell_level}, one group")
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cell_level", CELL_LEVELS)
def test_rebuilt_side_tables_continue_the_paths_the_later_batches_read(built_libs, cell_level):
    import torch
    box, batches, counts = deep_case(cell_level)
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", 1)
        u = dev.uniforms(W, H, _cam(box), box)
        ref = _reference(cell_level, u, batches)
        assert_oracle_preconditions(ref, cell_level, counts)
        ends, taken, sizes = _drive(dev, u, batches[:2], 1)
        assert ends == [1, 2], f"A and B: {ends} {taken} {sizes}"
        # the side tables as k_expand left them are gone — everything in the momentary buffer but the recycle stack of released chunks (bytes 4096 ..
        # 4096 + 8 000 000, which has to survive between launches: tests/test_gpu_parity.py) — and the library is told so, as after an import
        # (tests/test_gpu_resume.py: simlod_import_octree_buildable ends the same way): the next launch's k_begin rebuilds every row from the node array
        torch.cuda.synchronize()
        dev.momentary[:4096].fill_(0xA5)
        dev.momentary[4096 + 8_000_000:].fill_(0xA5)
        assert dev.L.simlod_octree_image_replaced(dev._p(dev.nodes)) == 0
        dev.groups_ingested(zero=True)
        for k, b in enumerate(batches[2:]):
            dev.upload(b)
            dev.construct(u)
            assert dev.processed() == 3 + k
        assert dev.groups_ingested() == 2
        _finish(dev, ref, f"deep paths, cell level {cell_level}, rebuilt side tables")
    finally:
        dev.close()
