"""k_expand's widened build phase at its edges (tests/test_gpu_flood.py has its middle: 72 next-round slots and 100 fresh leaves out of the root's slot of an
empty octree).  Every case goes into the port oracle and into the device as ONE exact group of four batches and is compared the way tests/test_gpu_groups.py
compares: every Node field, every build counter of Stats, the structural invariants.  Each GPU test has a CPU twin that asserts, from the oracle's octree
alone, the preconditions that prove the path ran; the GPU test asserts them again before it compares.

  A  the counts at the wave boundaries: 64 / 65 next-round slots (block_exclusive's records of one and two waves) with 64 / 65 fresh leaves (one and two
     waves of alloc_points), and 72 slots with 129 fresh leaves (three waves);
  B  the same flood into a level-2 leaf that already holds 15 734 points: a slot with stored points that move, below the top table's level, whose moved
     points make 237 fresh leaves (four waves) — the allocator and chunk-pool counters must be those of batch-by-batch ingestion;
  C  the default flood in coalesced mode: the same kernels without per-batch accounting (its CPU twin is test_flood_case_yields_the_layout_in_the_oracle:
     same input, same oracle);
  D  a third round: five of the 72 dense cells hold 52 000 of their points in one level-6 cell — the instance (1, MAX) waits for the decisions of 72 slots
     spread over the workgroups and runs its in-kernel histogram pass over histograms the whole-workgroup zeroing prepared;
  E  512 fresh leaves out of the root's slot: eight waves of alloc_points, more than 1 024 new chunks (phase 2 loops), 512 top-table entries;
  F  partial grants: the default flood into node arrays of 169, 360, 593 and 598 nodes.  The oracle knows no node limit: the expectation is
     flood_ref.grant_model, written from the documented rule.
All comparisons are equalities."""
import numpy as np
import pytest

import oracle
from cases import H, W
from flood_ref import cell_counts, grant_model, inner_per_level, inner_set, inside, points_per_node
from simlod_amd import abi, synthetic
from test_gpu_flood import BATCH, DENSE_POINTS, G, SPARSE_POINTS, flood_case
from test_gpu_groups import GROUP_MOMENTARY, GROUP_PERSISTENT, _cam, _compare, _drive
from test_gpu_parity import GRANULARITY_FREE_FIELDS, GRANULARITY_FREE_STATS, _device
from util import host_image_of, points_multiset_hash, voxel_colors_are_member

SIMLOD_ERR_NODES_EXHAUSTED = 0x8          # include/simlod_hip.h
BOUNDARIES = [(64, 64), (65, 65), (72, 129)]
STORED_CELL = (1, 2, 0)                   # B: the level-2 leaf the flood goes into
CAPACITIES = {169: (169, 20, 0), 360: (353, 43, 0), 593: (593, 43, 30), 598: (593, 43, 30)}      # max_nodes -> Stats.numNodes, splits kept of 43, slots kept of 72
_REFS = {}
_BUILD_UNIFORMS = ["boxMin", "boxMax", "persistentBufferCapacity"]      # what the oracle's build reads of the uniforms besides the batches


class _Reference:
    """What a comparison needs of an oracle run (the oracle's 16 GB of address space go back)."""

    def __init__(self, ref):
        self.stats, self._dump = ref.stats.copy(), ref.dump()

    def dump(self):
        return self._dump


def _uniforms(box):
    return abi.make_uniforms(W, H, _cam(box), box, persistent_capacity=GROUP_PERSISTENT, momentary_capacity=GROUP_MOMENTARY)


def _reference(name, u, batches):
    """The port oracle after `batches`, one at a time — once per case -> (reference, dump after the first batch)."""
    if name not in _REFS:
        ref = oracle.HostOctree("port", persistent_bytes=GROUP_PERSISTENT)
        ref.reset(u)
        first = None
        for b in batches:
            ref.upload(b)
            ref.construct(u)
            if first is None:
                first = ref.dump()
        assert ref.last_error() == 0 and int(ref.stats["batchletIndex"][0]) == len(batches)
        _REFS[name] = (_Reference(ref), first, [np.array(u[f], copy=True) for f in _BUILD_UNIFORMS])
    r, first, u0 = _REFS[name]
    assert all(np.array_equal(a, u[f]) for a, f in zip(u0, _BUILD_UNIFORMS)), "one case, one box and one capacity"
    return r, first


def _cells(dump, sel):
    return {(int(dump["X"][i]), int(dump["Y"][i]), int(dump["Z"][i])) for i in np.nonzero(sel)[0]}


def _group_of_four(dev, u, batches, name, ref):
    """One launch, one group of four, then the full comparison."""
    ends, taken, sizes = _drive(dev, u, batches, G)
    assert ends == [G] and taken == [G] and sizes == [G] and dev.groups_ingested() == 1, f"one launch, one group of {G}: {ends} {taken} {sizes}"
    nodes, pers, nn = _compare(dev, name, ref)
    oracle.check_invariants(nodes, nn)


# ---- A: the counts at the wave boundaries --------------------------------------------------------------------------------------------------
def assert_boundary_preconditions(dump, dense, sparse):
    lvl, leaf, pts = dump["level"], dump["isLeaf"] != 0, dump["numPoints"]
    assert _cells(dump, (lvl == 3) & ~leaf) == set(dense), "the inner nodes at level 3 — the slots of the next round — are the dense cells"
    assert _cells(dump, (lvl == 3) & leaf & (pts > 0)) == set(sparse) and not np.any((lvl >= 1) & (lvl <= 2) & leaf & (pts > 0)), \
        "the non-empty leaves of levels 1-3 — the fresh leaves of the root's slot — are the sparse cells"
    assert int(((lvl >= 1) & (lvl <= 3) & leaf & (pts > 0)).sum()) == len(sparse)
    assert not np.any((lvl >= 4) & ~leaf), "no inner node below level 3"
    assert np.all(pts[(lvl == 3) & leaf & (pts > 0)] == SPARSE_POINTS)


@pytest.mark.parametrize("dense,sparse", BOUNDARIES)
def test_boundary_cases_yield_their_counts_in_the_oracle(built_libs, dense, sparse):
    pts, box, batches, dcells, scells = flood_case(dense, sparse)
    assert len(dcells) == dense and len(scells) == sparse and len(batches) == G
    ref, _ = _reference(f"boundary {dense} {sparse}", _uniforms(box), batches)
    assert_boundary_preconditions(ref.dump(), dcells, scells)


@pytest.mark.gpu
@pytest.mark.parametrize("dense,sparse", BOUNDARIES)
def test_slots_and_fresh_leaves_at_the_wave_boundaries_build_the_oracles_octree(built_libs, dense, sparse):
    pts, box, batches, dcells, scells = flood_case(dense, sparse)
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", G)
        u = dev.uniforms(W, H, _cam(box), box)
        ref, _ = _reference(f"boundary {dense} {sparse}", u, batches)
        assert_boundary_preconditions(ref.dump(), dcells, scells)
        _group_of_four(dev, u, batches, f"boundary {dense} slots, {sparse} fresh leaves", ref)
    finally:
        dev.close()


# ---- B: the flood into a leaf that holds points -----------------------------------------------------------------------------------------------
def stored_leaf_case():
    """-> (box, [the uniform batch, then the default flood scaled into level-2 cell STORED_CELL])"""
    pts, box, batches, dense, sparse = flood_case()
    first, ubox = synthetic.uniform_cube(1_000_000, seed=5)
    assert np.array_equal(np.asarray(ubox, dtype=np.float32), box)
    moved = np.array(pts, copy=True)
    for a, c in zip("xyz", STORED_CELL):
        moved[a] = pts[a] * np.float32(0.25) + np.float32(0.25) * np.float32(c)
    return box, [first] + [moved[i:i + BATCH] for i in range(0, len(moved), BATCH)]


def assert_stored_leaf_preconditions(first, dump):
    # after the uniform batch: the root and 8 + 64 nodes, every level-2 node a leaf, ours with 15 734 points
    assert len(first) == 73 and int(((first["level"] == 2) & (first["isLeaf"] != 0)).sum()) == 64
    mine = inside(first, 2, STORED_CELL)
    assert int(mine.sum()) == 1 and int(first["numPoints"][mine][0]) == 15_734 and int(first["isLeaf"][mine][0]) == 1
    # after the group: the cascade below that leaf, and nothing else
    assert len(dump) == 1_001
    cell = inside(dump, 2, STORED_CELL)
    assert int(cell.sum()) == 1 + 8 * (1 + 7 + 36 + 72)
    assert inner_per_level(dump, cell) == {2: 1, 3: 7, 4: 36, 5: 72}, "the slot's own node, 7 children and 36 grandchildren split, 72 slots of the next round, none below"
    assert inner_per_level(dump, ~cell) == {0: 1, 1: 8}
    lvl, leaf, pts = dump["level"], dump["isLeaf"] != 0, dump["numPoints"]
    fresh = [int((cell & (lvl == l) & leaf & (pts > 0)).sum()) for l in (3, 4, 5)]
    assert fresh == [1, 20, 216] and sum(fresh) == 237 > 3 * 64, "the stored points that moved make every leaf of the cascade a fresh one: four waves"


def test_stored_leaf_case_yields_its_counts_in_the_oracle(built_libs):
    box, batches = stored_leaf_case()
    ref, first = _reference("stored leaf", _uniforms(box), batches)
    assert_stored_leaf_preconditions(first, ref.dump())


@pytest.mark.gpu
def test_flood_into_a_leaf_that_holds_points_builds_the_oracles_octree_and_counters(built_libs):
    box, batches = stored_leaf_case()
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", G)
        u = dev.uniforms(W, H, _cam(box), box)
        ref, first = _reference("stored leaf", u, batches)
        assert_stored_leaf_preconditions(first, ref.dump())
        ends, taken, sizes = _drive(dev, u, batches[:1], 1)                  # the uniform batch: a launch of its own
        assert ends == [1] and taken == [1]
        dev.set_batch_limit(G)
        for b in batches[1:]:
            dev.upload(b)
        dev.construct(u)
        assert dev.processed() == 1 + G and dev.group_size() == G and dev.groups_ingested() == 2, "one batch, then one group of four"
        nodes, pers, nn = _compare(dev, "flood into a stored leaf", ref)      # (STATS_BUILD_FIELDS: numAllocatedChunks and chunkPoolSize as batch by batch)
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


# ---- C: the default flood, coalesced -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_coalesced_flood_builds_the_same_octree_content(built_libs):
    from test_gpu_flood import assert_flood_preconditions
    pts, box, batches, dense, sparse = flood_case()
    dev = _device(coalesce=True, persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        u = dev.uniforms(W, H, _cam(box), box)
        ref, _ = _reference("flood", u, batches)
        assert_flood_preconditions(ref.dump(), dense, sparse, False)
        ends, taken, sizes = _drive(dev, u, batches, G)
        assert ends == [G] and taken == [G], f"one launch for the four batches: {ends} {taken}"
        nodes, pers, nn = _compare(dev, "coalesced flood", ref, GRANULARITY_FREE_FIELDS, GRANULARITY_FREE_STATS)
        oracle.check_invariants(nodes, nn)
        assert voxel_colors_are_member(nodes, nn, pts, box) == int(nodes["numVoxelsStored"][:nn].sum()) > 0
    finally:
        dev.close()


# ---- D: a third round ---------------------------------------------------------------------------------------------------------------------------
def assert_third_round_preconditions(dump, dense):
    assert len(dump) == 1_049
    assert inner_per_level(dump) == {0: 1, 1: 7, 2: 36, 3: 72, 4: 5, 5: 5, 6: 5}, "round 0 ends at level 3, round 1 at level 6, round 2 splits the five level-6 nodes"
    # the five inner nodes at level 6 lie in five DIFFERENT dense cells — slots of round 1 —: round 2 ran out of five slots
    lvl, leaf = dump["level"], dump["isLeaf"] != 0
    six = _cells(dump, (lvl == 6) & ~leaf)
    assert six == {(8 * x + 3, 8 * y + 3, 8 * z + 3) for x, y, z in dense[:5]} and len({(x >> 3, y >> 3, z >> 3) for x, y, z in six}) == 5


def test_third_round_case_yields_its_counts_in_the_oracle(built_libs):
    pts, box, batches, dense, sparse = flood_case(concentrated=5)
    ref, _ = _reference("third round", _uniforms(box), batches)
    assert_third_round_preconditions(ref.dump(), dense)


@pytest.mark.gpu
def test_a_third_round_behind_the_flood_builds_the_oracles_octree(built_libs):
    pts, box, batches, dense, sparse = flood_case(concentrated=5)
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", G)
        u = dev.uniforms(W, H, _cam(box), box)
        ref, _ = _reference("third round", u, batches)
        assert_third_round_preconditions(ref.dump(), dense)
        _group_of_four(dev, u, batches, "third round", ref)
    finally:
        dev.close()


# ---- E: 512 fresh leaves ------------------------------------------------------------------------------------------------------------------------
def full_cube_case():
    pts, box = synthetic.uniform_cube(3_990_000, seed=31)
    return np.asarray(box, dtype=np.float32), [pts[i:i + BATCH] for i in range(0, len(pts), BATCH)]


def assert_full_cube_preconditions(dump):
    lvl, leaf, pts = dump["level"], dump["isLeaf"] != 0, dump["numPoints"]
    assert len(dump) == 585 and int(((lvl == 2) & ~leaf).sum()) == 64 and inner_per_level(dump) == {0: 1, 1: 8, 2: 64}
    fresh = (lvl == 3) & leaf & (pts > 0)
    assert int(fresh.sum()) == 512 == 8 * 64, "eight waves of alloc_points, 512 entries of the top table"
    assert int(((pts[fresh].astype(np.int64) + 999) // 1000).sum()) > 1024, "more new chunks than the workgroup has threads"


def test_full_cube_case_yields_its_counts_in_the_oracle(built_libs):
    box, batches = full_cube_case()
    assert len(batches) == G
    ref, _ = _reference("full cube", _uniforms(box), batches)
    assert_full_cube_preconditions(ref.dump())


@pytest.mark.gpu
def test_512_fresh_leaves_out_of_the_roots_slot_build_the_oracles_octree(built_libs):
    box, batches = full_cube_case()
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", G)
        u = dev.uniforms(W, H, _cam(box), box)
        ref, _ = _reference("full cube", u, batches)
        assert_full_cube_preconditions(ref.dump())
        _group_of_four(dev, u, batches, "512 fresh leaves", ref)
    finally:
        dev.close()


# ---- F: partial grants --------------------------------------------------------------------------------------------------------------------------
def test_grant_model_equals_the_oracle_without_a_limit_and_cuts_where_the_rule_says(built_libs):
    """CPU: the model's octree with no node limit is the oracle's (so its counts, orders of magnitude and cells are the input's), and at the four
    capacities it grants what the arithmetic of the rule gives."""
    pts, box, batches, dense, sparse = flood_case()
    c3 = cell_counts(pts, box, 3)
    assert {tuple(int(v) for v in c) for c in np.argwhere(c3 == DENSE_POINTS)} == set(dense) and {tuple(int(v) for v in c) for c in np.argwhere(c3 == SPARSE_POINTS)} == set(sparse)
    assert int(cell_counts(pts, box, 4).max()) <= 50_000, "nothing splits below level 3: the model's three levels are the whole octree"
    ref, _ = _reference("flood", _uniforms(box), batches)
    free = grant_model(c3)
    assert (free["want_splits"], free["kept_splits"], free["want_slots"], free["kept_slots"]) == (7 + 36, 43, 72, 72)
    assert free["inner"] == inner_set(ref.dump()) and free["num_nodes"] == len(ref.dump()) == 1 + 8 * (1 + 43 + 72)
    for cap, (num_nodes, splits, slots) in CAPACITIES.items():
        m = grant_model(c3, cap)
        assert (m["num_nodes"], m["kept_splits"], m["kept_slots"]) == (num_nodes, splits, slots), cap
        assert m["want_splits"] == 43 and m["inner"] < free["inner"] and len(m["inner"]) == 1 + splits + slots
        assert m["want_slots"] == (72 if splits == 43 else 2 * (splits - 7)), "two dense cells under every grandchild that splits"
    # 169: the seven children, then the first 13 grandchildren by (child, octant) — not any 13
    m = grant_model(c3, 169)
    assert sum(1 for n in m["inner"] if n[0] == 1) == 7 and sum(1 for n in m["inner"] if n[0] == 2) == 13
    two = sorted(((x >> 1) << 2 | (y >> 1) << 1 | (z >> 1), (x & 1) << 2 | (y & 1) << 1 | (z & 1)) for l, x, y, z in free["inner"] if l == 2)
    assert {(2, 2 * (j >> 2 & 1) + (k >> 2 & 1), 2 * (j >> 1 & 1) + (k >> 1 & 1), 2 * (j & 1) + (k & 1)) for j, k in two[:13]} == {n for n in m["inner"] if n[0] == 2}


@pytest.mark.gpu
@pytest.mark.parametrize("max_nodes", sorted(CAPACITIES))
def test_a_full_node_array_grants_the_first_splits_in_order_and_keeps_every_point(built_libs, max_nodes):
    pts, box, batches, dense, sparse = flood_case()
    want = grant_model(cell_counts(pts, box, 3), max_nodes)
    assert (want["num_nodes"], want["kept_splits"], want["kept_slots"]) == CAPACITIES[max_nodes] and want["want_splits"] == 43
    n = len(pts)
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY, max_nodes=max_nodes)      # (the capacity belongs to the octree's context: the library's default stays)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", G)
        u = dev.uniforms(W, H, _cam(box), box)
        ends, taken, sizes = _drive(dev, u, batches, G)
        assert ends == [G] and taken == [G] and sizes == [G] and dev.groups_ingested() == 1, f"one launch, one group of {G}: {ends} {taken} {sizes}"
        ds = dev.read_stats()
        print(f"max_nodes={max_nodes}: Stats.numNodes={int(ds['numNodes'])} dbg={int(ds['dbg']):#x} numPoints={int(ds['numPoints'])}")
        assert int(ds["numNodes"]) == want["num_nodes"]
        assert int(ds["dbg"]) == SIMLOD_ERR_NODES_EXHAUSTED
        assert int(ds["numPoints"]) == int(ds["numPointsProcessed"]) == n == 3_990_000
        nodes, pers, nn = host_image_of(dev)
        assert nn == want["num_nodes"]
        d = oracle.dump_image(nodes, nn)
        got = inner_set(d)
        assert got == want["inner"], f"inner nodes: {len(got)} for {len(want['inner'])}; not granted by the rule: {sorted(got - want['inner'])[:8]}, missing: {sorted(want['inner'] - got)[:8]}"
        leaf = d["isLeaf"] != 0
        assert np.array_equal(d["numPoints"][leaf].astype(np.int64), points_per_node(pts, box, d["level"][leaf], d["X"][leaf], d["Y"][leaf], d["Z"][leaf]))
        assert int(d["numPoints"][leaf].max()) > 50_000, "the splits that were not granted: leaves over the limit"
        tot = oracle.check_invariants(nodes, nn, allow_overfull=True)
        assert tot["points"] == n
        hs, hx = points_multiset_hash(pts)
        with np.errstate(over="ignore"):
            assert hs == np.uint64(d["pointsSum"].sum()) and hx == np.bitwise_xor.reduce(d["pointsXor"])
        assert voxel_colors_are_member(nodes, nn, pts, box) == int(nodes["numVoxelsStored"][:nn].sum()) > 0
        dev.render(u)                                                 # and the octree is still drawable
        assert int((dev.framebuffer(W, H) != abi.CLEAR_PIXEL).sum()) > 1000
    finally:
        dev.close()
