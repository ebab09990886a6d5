"""Chained construct launches (simlod_launch_construct_chain, DeviceOctree.construct_chain / drain with chain=True): one call that stands for
several back-to-back launches, with the launch boundary turned into an ordinary group boundary of the builder's pipeline.

Every case: the chained octree is the port oracle's (fed batch by batch: the whole dump, the build fields of Stats, the structural invariants) AND the
same device's launch-by-launch run (chain=False: dump and Stats equal), and the number of groups ingested is the launch-by-launch count — the groups,
and with them the voxel colours' outcome set, do not change.  Batches are 30 000 points, so leaves cross 50 000 within two batches and splits and
cascades straddle every seam; 300 MB momentary buffer, default knobs unless the case says otherwise."""
import numpy as np
import pytest

import oracle
from cases import H, W
from simlod_amd import abi, synthetic
from test_gpu_groups import GROUP_PERSISTENT, _cam, _compare
from test_gpu_parity import GRANULARITY_FREE_FIELDS, GRANULARITY_FREE_STATS, _device
from util import STATS_BUILD_FIELDS, assert_dumps_equal, assert_frame_equals_oracle, assert_stats_equal, host_image_of

pytestmark = pytest.mark.gpu

MOMENTARY = 300_000_000
BATCH = 30_000
MAXB = 50
_INPUTS, _REFS = {}, {}


def _points(kind):
    """50 batches of each input, made once; a case takes a prefix."""
    if kind not in _INPUTS:
        n = MAXB * BATCH
        pts, box = synthetic.uniform_cube(n, seed=77) if kind == "uniform" else synthetic.terrain(n, seed=7)
        _INPUTS[kind] = (pts, box)
    return _INPUTS[kind]


def _batches(kind, num):
    pts, box = _points(kind)
    return [pts[i * BATCH:(i + 1) * BATCH] for i in range(num)], box


def _late_root_batches():
    """20 batches of 2 000 points — 40 000: the root is still a leaf when the first segment ends — then five of 30 000: the root splits in the first
    group behind the seam, in that group's second batch (k_rootpre has the batch in front of it to sample into the root's grid)."""
    pts, box = _points("uniform")
    out = [pts[i * 2000:(i + 1) * 2000] for i in range(20)]
    base = 20 * 2000
    out += [pts[base + i * BATCH: base + (i + 1) * BATCH] for i in range(5)]
    return out, box


def _oracle(key, u, batches, persistent=GROUP_PERSISTENT, mask=None):
    """The port oracle fed batch by batch — once per input, shared and left unchanged."""
    if key not in _REFS:
        ref = oracle.HostOctree("port", persistent_bytes=persistent, ring_slots=abi.BATCH_STREAM_SIZE)
        ref.reset(u)
        if mask is not None:
            ref.set_trunk_mask(*mask)
        for b in batches:
            ref.upload(b)
            ref.construct(u)
        if not batches:
            ref.construct(u)                 # (an idle launch)
        assert ref.last_error() == 0
        _REFS[key] = ref
    return _REFS[key]


def _run(batches, box, *, chain, knobs=None, limit=None, coalesce=False, mask=None, how="drain", persistent=GROUP_PERSISTENT):
    """Reset, upload everything, ingest.  how: "drain" or ("chain", n): ONE construct_chain(n) — with chain=False the n plain launches it stands for.
    -> (device, uniforms, Stats, dump, groups ingested)"""
    dev = _device(persistent_bytes=persistent, momentary_bytes=MOMENTARY, coalesce=coalesce, chain=chain)
    for k, v in (knobs or {}).items():
        dev.tune(k, v)
    u = dev.uniforms(W, H, _cam(box), box)
    dev.reset(u)
    if mask is not None:
        dev.set_trunk_mask(*mask)
    dev.groups_ingested(zero=True)
    if limit is not None:
        dev.set_batch_limit(limit)
    for b in batches:
        dev.upload(b)
    if how == "drain":
        dev.drain(u)
    elif chain:
        dev.construct_chain(u, how[1])
    else:
        for _ in range(how[1]):
            dev.construct(u)
    dev.processed()
    return dev, u


def _both(batches, box, **kw):
    """The chained run and the launch-by-launch run of the same device code: equal dumps, equal Stats, equal group counts.  -> the chained device, u, groups"""
    plain, u = _run(batches, box, chain=False, **kw)
    try:
        ps, pg = plain.read_stats(), plain.groups_ingested()
        pn, ppers, pnn = host_image_of(plain)
        pd = oracle.dump_image(pn, pnn)
    finally:
        plain.close()
    dev, u = _run(batches, box, chain=True, **kw)
    ds = dev.read_stats()
    assert int(ds["dbg"]) == 0 and int(ps["dbg"]) == 0
    nodes, pers, nn = host_image_of(dev)
    assert_dumps_equal(oracle.dump_image(nodes, nn), pd, "chained against launch by launch")
    assert_stats_equal(ds, ps, STATS_BUILD_FIELDS, "chained against launch by launch")
    groups = dev.groups_ingested()
    assert groups == pg, f"{groups} groups chained, {pg} launch by launch"
    return dev, u, groups


def _groups_of(segments, take=5):
    return sum(-(-s // take) for s in segments)


@pytest.mark.parametrize("kind", ["uniform", "terrain"])
@pytest.mark.parametrize("num,segments", [(21, (20, 1)), (36, (20, 16)), (41, (20, 20, 1)), (50, (20, 20, 10))])
def test_chained_drain_builds_the_oracles_octree_in_the_groups_of_the_launches(built_libs, kind, num, segments):
    batches, box = _batches(kind, num)
    dev, u, groups = _both(batches, box)
    try:
        assert dev.processed() == num and dev.group_size() == 5
        assert groups == _groups_of(segments), f"{num} batches: the groups of launches of {segments}"
        ref = _oracle((kind, num), u, batches)
        nodes, pers, nn = _compare(dev, f"{kind} {num} chained", ref)
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


def test_a_chain_of_one_is_the_plain_launch(built_libs):
    batches, box = _batches("uniform", 20)
    dev, u, groups = _both(batches, box, how=("chain", 1))
    try:
        assert dev.processed() == 20 and groups == 4
        nodes, pers, nn = _compare(dev, "chain of one", _oracle(("uniform", 20), u, batches))
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


def test_segments_follow_the_contexts_batch_limit(built_libs):
    """Limit 7, 20 batches: segments of 7, 7, 6 in groups 5,2 | 5,2 | 5,1."""
    batches, box = _batches("terrain", 20)
    dev, u, groups = _both(batches, box, limit=7)
    try:
        assert dev.processed() == 20 and groups == 6
        nodes, pers, nn = _compare(dev, "limit 7", _oracle(("terrain", 20), u, batches))
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


def test_a_chain_with_more_groups_than_ordinals_is_cut_inside_the_call(built_libs):
    """SIMLOD_EXACT_GROUP=2, 50 batches: 10 | 10 | 5 groups — 25, more than the 20 ordinals of one device launch: ONE construct_chain(3) call takes them all."""
    batches, box = _batches("uniform", 50)
    dev, u, groups = _both(batches, box, knobs={"SIMLOD_EXACT_GROUP": 2}, how=("chain", 3))
    try:
        assert dev.processed() == 50 and groups == 25 and dev.group_size() == 2
        nodes, pers, nn = _compare(dev, "groups of two, cut", _oracle(("uniform", 50), u, batches))
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


def test_later_segments_that_find_nothing_leave_the_stats_of_one_launch(built_libs):
    batches, box = _batches("terrain", 12)
    dev, u, groups = _both(batches, box, how=("chain", 3))
    try:
        assert dev.processed() == 12 and groups == 3
        nodes, pers, nn = _compare(dev, "chain of 3, 12 uploaded", _oracle(("terrain", 12), u, batches))
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


def test_a_chain_with_nothing_uploaded_is_an_idle_launch(built_libs):
    _, box = _batches("uniform", 1)
    dev, u, groups = _both([], box, how=("chain", 3))
    try:
        assert dev.processed() == 0 and groups == 0
        _compare(dev, "idle chain", _oracle(("uniform", 0), u, []))
    finally:
        dev.close()


def test_coalesced_chain_builds_the_same_octree_content(built_libs):
    """Coalesced mode, 36 batches: content counts as in test_coalesced_ingest_builds_the_same_octree_content (what does not depend on the granularity).
    With 30 000-point batches the root is still a leaf after the group's first batch and has sampled itself when the second splits it
    (voxels.cu:371-382, 449-463): the root's voxel count holds only if coalesced groups replay that too (k_rootpre, from the batches' sizes)."""
    batches, box = _batches("terrain", 36)
    dev, u, groups = _both(batches, box, coalesce=True)
    try:
        assert dev.processed() == 36 and groups < 36
        nodes, pers, nn = _compare(dev, "coalesced chain", _oracle(("terrain", 36), u, batches), GRANULARITY_FREE_FIELDS, GRANULARITY_FREE_STATS)
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


def test_chain_with_the_trunk_mask_set(built_libs):
    """The root and its eight children split whatever they hold (multi-GPU trunk): forced splits in the first group, cascades across the seam."""
    mask = (0x1FF, 0)
    batches, box = _batches("terrain", 36)
    dev, u, groups = _both(batches, box, mask=mask)
    try:
        assert dev.processed() == 36 and groups == 8
        nodes, pers, nn = _compare(dev, "trunk mask", _oracle(("terrain", 36, mask), u, batches, mask=mask))
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


def test_the_root_splits_in_the_first_group_and_in_the_first_group_behind_a_seam(built_libs):
    """30 000-point batches: the root crosses 50 000 in the second batch of the first group (every drain case above; asserted here on 21 batches).  The
    second input keeps the root a leaf through the whole first segment and splits it in the first group behind the seam (k_rootpre)."""
    late, box = _late_root_batches()
    dev, u, groups = _both(late, box)
    try:
        assert dev.processed() == 25 and groups == 5
        early = _oracle(("uniform", 2), u, _batches("uniform", 2)[0])
        assert int(early.stats["numNodes"][0]) > 1, "30 000-point batches: the root splits in the first group"
        before_seam = _oracle("late root, first segment", u, late[:20])
        assert int(before_seam.stats["numNodes"][0]) == 1, "the root is still a leaf when the first segment ends"
        behind_seam = _oracle("late root, 22 batches", u, late[:22])
        assert int(behind_seam.stats["numNodes"][0]) > 1, "... and has split by the second batch behind the seam"
        nodes, pers, nn = _compare(dev, "root splits behind the seam", _oracle("late root", u, late))
        oracle.check_invariants(nodes, nn)
    finally:
        dev.close()


def test_memory_guard_inside_the_second_segment_drained_to_the_end(built_libs):
    """The persistent capacity is chosen on the CPU: the oracle, fed the 36 batches with a large buffer, gives the allocator offset after every batch; the
    reference's guard (voxels.cu:896-912) refuses batch b when offset(b - 1) + 200 MB >= capacity, so capacity = offset after batch 27 + 200 MB trips
    it in front of batch 28 — inside the second segment — provided the offset before batch 27 lies below it (asserted).  A capacity that small is
    below what exact groups need at all (construct.hip: SIMLOD_MEM_SAFETY_MARGIN + a worst-case group of two batches), so this chain goes batch by
    batch — plain launches inside the entry point; drain() takes it to the end either way and every counter is the oracle's."""
    batches, box = _batches("terrain", 36)
    margin = 200_000_000
    probe = oracle.HostOctree("port", persistent_bytes=GROUP_PERSISTENT, ring_slots=abi.BATCH_STREAM_SIZE)
    offsets = []
    u = abi.make_uniforms(W, H, _cam(box), box, persistent_capacity=GROUP_PERSISTENT, momentary_capacity=MOMENTARY)
    probe.reset(u)
    for b in batches:
        probe.upload(b)
        probe.construct(u)
        offsets.append(int(probe.stats["allocatedBytes_persistent"][0]))
    cap = offsets[27] + margin
    assert offsets[26] + margin < cap, "the allocator grows in batch 28"
    ucap = np.array(u, copy=True)
    ucap["persistentBufferCapacity"] = cap
    ref = oracle.HostOctree("port", persistent_bytes=cap, ring_slots=abi.BATCH_STREAM_SIZE)
    ref.reset(ucap)
    for b in batches:
        ref.upload(b)
        ref.construct(ucap)
    stop = int(ref.stats["batchletIndex"][0])
    assert 20 < stop < 36 and int(ref.stats["memCapacityReached"][0]) == 1, f"the reference stops at {stop}"
    from simlod_amd.runtime import SimlodError
    dev = _device(persistent_bytes=cap + 4096, momentary_bytes=MOMENTARY, chain=True)
    try:
        dev.persistent[cap:].fill_(0x3C)
        dev.persistent_bytes = cap
        ud = dev.uniforms(W, H, _cam(box), box)
        assert int(ud["persistentBufferCapacity"]) == cap
        dev.reset(ud)
        for b in batches:
            dev.upload(b)
        with pytest.raises(SimlodError, match="memCapacityReached=1"):
            dev.drain(ud)                                           # to the end: until launches make no progress any more
        ds = dev.read_stats()
        assert int(ds["dbg"]) == 0 and int(ds["memCapacityReached"]) == 1 and int(ds["batchletIndex"]) == stop
        assert_stats_equal(ds, ref.stats[0], STATS_BUILD_FIELDS, "memory guard")
        nodes, pers, nn = host_image_of(dev)
        assert_dumps_equal(oracle.dump_image(nodes, nn), ref.dump(), "memory guard")
        assert bool((dev.persistent[cap:] == 0x3C).all())
    finally:
        dev.close()


def test_two_chained_ingests_leave_identical_counters(built_libs):
    batches, box = _batches("terrain", 36)
    seen = []
    for _ in range(2):
        dev, u = _run(batches, box, chain=True)
        try:
            ds = dev.read_stats()
            nodes, pers, nn = host_image_of(dev)
            seen.append((ds, oracle.dump_image(nodes, nn), dev.groups_ingested()))
        finally:
            dev.close()
    assert_stats_equal(seen[0][0], seen[1][0], STATS_BUILD_FIELDS, "two chained ingests")
    assert_dumps_equal(seen[0][1], seen[1][1], "two chained ingests")
    assert seen[0][2] == seen[1][2] == 8


def test_a_render_right_after_a_chain_sees_the_complete_octree(built_libs):
    """The tail really closes the chain: a frame enqueued behind it, with no synchronisation in between, is the oracle's frame of the final image."""
    batches, box = _batches("uniform", 36)
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=MOMENTARY, chain=True)
    try:
        u = dev.uniforms(W, H, _cam(box), box)
        dev.reset(u)
        for b in batches:
            dev.upload(b)
        dev.construct_chain(u, 2)
        dev.render(u)
        assert dev.processed() == 36
        nodes, pers, nn = host_image_of(dev)
        assert_frame_equals_oracle(dev, nodes, nn, u, "render behind a chain", 1000)
    finally:
        dev.close()
