"""Exact mode in groups of batches: every group size, the default drain, coalesced mode and the memory guard, against the port
oracle — every Node and Stats field, and which batch coloured each voxel (tests/util.py assert_voxel_winners on tagged inputs).

The reference colours a voxel from the FIRST batch that hit its cell.  A group voxelizes its batches together: any sample of the
group may win a cell, so with groups the bound is "no later than the last batch of the group (of the launch) that first hit the cell";
SIMLOD_EXACT_GROUP=1 must meet the reference's rule exactly.  The group counter (Ctl.expandNs[4], DeviceOctree.groups_ingested) proves the
groups were really taken."""
import numpy as np
import pytest

import oracle
from cases import H, W, batches_of, case
from simlod_amd import abi, camera, synthetic
from test_gpu_parity import GRANULARITY_FREE_FIELDS, GRANULARITY_FREE_STATS, _device, _ingest
from util import (STATS_BUILD_FIELDS, assert_dumps_equal, assert_stats_equal, assert_voxel_winners, batch_of_points, host_image_of, late_voxels,
                  replay_first_hits, tag_colors)

pytestmark = pytest.mark.gpu

GROUP_PERSISTENT = 16 << 30          # far from the memory guard for any group: prepare_batch never cuts a group of 12 batches of 1 M points
GROUP_MOMENTARY = 1_000_000_000      # holds the layout of groups of 12 (ACCT_MAX_GROUP)
SCENARIOS = ["ragged_tiny", "uniform_3x40k", "terrain_4x100k", "terrain_6m", "hotspot_3m"]
_CACHE = {}


def _cam(box):
    return camera.lookat_transform((1.8 * box[0], -1.2 * box[1], 1.4 * max(box)), (0.5 * box[0], 0.5 * box[1], 0.3 * box[2]), W, H)


def _input(name):
    """-> (points, box, batches of the TAGGED points)"""
    if name == "terrain_6m":
        pts, box = synthetic.terrain(6_000_000, seed=7)
        batch = 1_000_000
    elif name == "hotspot_3m":
        pts, box = synthetic.hotspot(3_000_000, seed=11)
        batch = 400_000
    elif name == "terrain_36m":
        pts, box = synthetic.terrain(36_000_000, seed=7)
        batch = abi.MAX_BATCH_SIZE
    elif name == "config5_20m":
        pts, box = synthetic.hotspot(20_000_000, seed=11)
        batch = abi.MAX_BATCH_SIZE
    elif name.startswith("coalesced_"):
        kind, n, batch = {"coalesced_terrain_1m": ("terrain", 7_300_000, abi.MAX_BATCH_SIZE), "coalesced_terrain_300k": ("terrain", 7_300_000, 300_000),
                          "coalesced_hotspot": ("hotspot", 5_000_000, abi.MAX_BATCH_SIZE)}[name]
        pts, box = (synthetic.terrain(n, seed=9, box=(3000.0, 2000.0, 200.0), tile=125.0) if kind == "terrain" else
                    synthetic.hotspot(n, seed=13, level=4, cell=(5, 9, 6)))
    else:
        pts, box, batch, _ = case(name)
    return pts, box, batches_of(name, tag_colors(pts), batch)


def _inputs(name):
    """(box, tagged points, batches) — once per input (the full-size inputs empty the cache before and after)."""
    if name not in _CACHE:
        pts, box, batches = _input(name)
        _CACHE[name] = dict(box=box, batches=batches, tagged=np.concatenate(batches))
    c = _CACHE[name]
    return c["box"], c["tagged"], c["batches"]


def _reference(name, u):
    """(tagged points, batches, port oracle after them, first-hit table) — the oracle's run does not depend on the group size."""
    box, tagged, batches = _inputs(name)
    c = _CACHE[name]
    if "ref" not in c:
        c["ref"], c["fh"] = replay_first_hits(u, batches)
        assert int(c["ref"].stats["batchletIndex"][0]) == len(batches), "the oracle's memory guard tripped"
    return tagged, batches, c["ref"], c["fh"]


def _launch_bound(ends):
    """bound(b*) = the last batch of the launch that ingested b* (`ends`: Stats.batchletIndex after each launch)."""
    e = np.asarray(ends, dtype=np.int64)
    return lambda b: e[np.searchsorted(e, b, side="right")] - 1


def _drive(dev, u, batches, per_launch):
    """Reset, then upload `per_launch` batches at a time and launch once for them (set_batch_limit: the launch takes all of them).  Returns
    (Stats.batchletIndex after each launch, batches per launch, Ctl.groupMax of each launch).  Stops when a launch takes nothing."""
    dev.reset(u)
    dev.groups_ingested(zero=True)
    dev.set_batch_limit(per_launch)
    ends, taken, sizes = [], [], []
    done = 0
    for i in range(0, len(batches), per_launch):
        for b in batches[i:i + per_launch]:
            dev.upload(b)
        while done < min(i + per_launch, len(batches)):
            dev.construct(u)
            now = dev.processed()
            if now == done:
                return ends, taken, sizes
            ends.append(now); taken.append(now - done); sizes.append(dev.group_size())
            done = now
    return ends, taken, sizes


def _compare(dev, name, ref, fields=None, stats=None):
    ds = dev.read_stats()
    assert int(ds["dbg"]) == 0, f"{name}: Stats.dbg={int(ds['dbg']):#x}"
    assert_stats_equal(ds, ref.stats[0], stats or STATS_BUILD_FIELDS, name)
    nodes, pers, nn = host_image_of(dev)
    got, want = oracle.dump_image(nodes, nn), ref.dump()
    if fields is None:
        assert_dumps_equal(got, want, name)
    else:
        assert len(got) == len(want)
        for f in fields:
            assert np.array_equal(got[f], want[f]), f"{name}: {f}"
    return nodes, pers, nn             # (the nodes point into `pers`: keep it alive while they are read)


# ---- every group size --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("G", [1, 2, 5, 12])
def test_exact_groups_of_every_size_build_the_oracles_octree_and_colour_from_the_group(built_libs, G, name):
    box = _inputs(name)[0]
    dev = _device(persistent_bytes=GROUP_PERSISTENT, momentary_bytes=GROUP_MOMENTARY)
    try:
        dev.tune("SIMLOD_EXACT_GROUP", G)
        u = dev.uniforms(W, H, _cam(box), box)
        tagged, batches, ref, fh = _reference(name, u)
        ends, taken, sizes = _drive(dev, u, batches, G)
        assert ends and ends[-1] == len(batches), f"ingest stopped at {ends}"
        groups = dev.groups_ingested()
        nodes, pers, nn = _compare(dev, f"{name} G={G}", ref)
        bop = batch_of_points(batches)
        if G == 1:
            assert groups == len(batches)
            checked = assert_voxel_winners(nodes, nn, tagged, bop, fh, lambda b: b, u)
        else:
            # the layout held groups of G, and they were taken: one group per launch (nothing cut)
            assert all(s == G for s, t in zip(sizes, taken) if t > 1), f"Ctl.groupMax per launch {sizes} (batches {taken})"
            assert groups == sum(-(-t // G) for t in taken) < len(batches), f"{groups} groups for launches of {taken} batches"
            checked = assert_voxel_winners(nodes, nn, tagged, bop, fh, _launch_bound(ends), u)
            late, total = late_voxels(nodes, nn, tagged, bop, fh, u)
            print(f"{name} G={G}: {late} of {total} voxels ({100.0 * late / total:.3f} %) coloured from a later batch of the group than the first hit")
        assert checked == int(nodes["numVoxelsStored"][:nn].sum()) > 0
    finally:
        dev.close()


# ---- the default drain: whatever the group boundaries, a voxel's colour comes from at most SIMLOD_EXACT_GROUP - 1 batches after its first hit ----
@pytest.mark.parametrize("name", SCENARIOS)
def test_default_drain_colours_within_a_group_of_the_first_hit(built_libs, name):
    box = _inputs(name)[0]
    dev = _device(persistent_bytes=GROUP_PERSISTENT)
    try:
        u = dev.uniforms(W, H, _cam(box), box)
        tagged, batches, ref, fh = _reference(name, u)
        dev.groups_ingested(zero=True)
        _ingest(dev, u, batches)
        nodes, pers, nn = _compare(dev, f"{name} default", ref)
        assert dev.groups_ingested() <= len(batches)
        assert assert_voxel_winners(nodes, nn, tagged, batch_of_points(batches), fh, lambda b: b + 5 - 1, u) == int(nodes["numVoxelsStored"][:nn].sum())
    finally:
        dev.close()


# ---- coalesced mode: a launch's batches are one batch — a voxel's colour comes from the launch that first hit its cell ------------------------
@pytest.mark.parametrize("name", ["coalesced_terrain_1m", "coalesced_terrain_300k", "coalesced_hotspot"])
def test_coalesced_ingest_colours_from_the_launch_of_the_first_hit(built_libs, name):
    box = _inputs(name)[0]
    dev = _device(ring_slots=abi.BATCH_STREAM_SIZE, coalesce=True, momentary_bytes=400_000_000)
    try:
        u = dev.uniforms(W, H, _cam(box), box)
        tagged, batches, ref, fh = _reference(name, u)
        ends, taken, _ = _drive(dev, u, batches, abi.MAX_BATCHES_PER_LAUNCH)
        assert ends[-1] == len(batches) and max(taken) > 1
        nodes, pers, nn = _compare(dev, name, ref, GRANULARITY_FREE_FIELDS, GRANULARITY_FREE_STATS)
        assert assert_voxel_winners(nodes, nn, tagged, batch_of_points(batches), fh, _launch_bound(ends), u) == int(nodes["numVoxelsStored"][:nn].sum())
    finally:
        dev.close()


# ---- the memory guard while groups are on -------------------------------------------------------------------------------------------------
def _group_slack_bytes(samples, num_nodes):
    """construct_state.inc group_slack_bytes (SLOT_CAP_GRIDS = 256)."""
    chunk, grid = abi.alloc_round(abi.CHUNK_BYTES), abi.alloc_round(abi.GRID_BYTES)
    return (2 * (samples * abi.MAX_DEPTH // abi.POINTS_PER_CHUNK + num_nodes + 1) + samples // abi.POINTS_PER_CHUNK + 4096) * chunk + 256 * grid


@pytest.mark.slow
def test_memory_guard_trips_like_the_reference_while_exact_groups_are_on(built_libs):
    """A persistent capacity just above the one at which construct.hip allows groups at all (SIMLOD_MEM_SAFETY_MARGIN + group_slack_bytes(2 M, 0)):
    the first launch takes a group of two batches, prepare_batch cuts the groups after it to one batch as the worst-case slack outgrows the
    distance to the guard, and the guard trips at the reference's batch — same Stats, same octree, nothing written behind the capacity, colours
    from the launch of the first hit.  (The input is the terrain, whose allocator grows ~25 MB per 1 M-point batch; a uniform cube would reach
    the reference's own limit of 3 M moved points per batch — 512 leaves crossing 50 000 together, at 25 M points — before the guard.)"""
    import torch
    G, per_launch, step = 2, 4, abi.MAX_BATCH_SIZE
    margin = 200_000_000                                          # SIMLOD_MEM_SAFETY_MARGIN, voxels.cu:898
    cap = margin + _group_slack_bytes(2 * step, 0) + 150_000_000
    assert 1_700_000_000 < cap < 1_900_000_000
    pts, box = synthetic.terrain(80_000_000, seed=17)
    tagged_all = tag_colors(pts)
    del pts
    all_batches = [tagged_all[i:i + step] for i in range(0, len(tagged_all), step)]
    dev = _device(ring_slots=abi.BATCH_STREAM_SIZE, persistent_bytes=cap + 4096)
    try:
        dev.persistent[cap:].fill_(0x3C)                          # canary behind the capacity the uniforms announce
        dev.tune("SIMLOD_EXACT_GROUP", G)
        u = dev.uniforms(W, H, _cam(box), box)
        u["persistentBufferCapacity"] = cap
        dev.persistent_bytes = cap
        dev.reset(u)
        dev.groups_ingested(zero=True)
        dev.set_batch_limit(per_launch)
        ends, taken, per_launch_groups = [], [], []
        done, uploaded = 0, 0
        while True:
            if done == uploaded:
                if uploaded == len(all_batches):
                    break
                for b in all_batches[uploaded:uploaded + per_launch]:
                    dev.upload(b)
                uploaded = min(uploaded + per_launch, len(all_batches))
            before = dev.groups_ingested()
            dev.construct(u)                                      # (near the guard a launch may take fewer batches: launch again)
            now = dev.processed()
            if now == done:
                break
            ends.append(now); taken.append(now - done); per_launch_groups.append(dev.groups_ingested() - before)
            done = now
        for _ in range(3):                                        # the frame loop keeps launching; nothing may move any more
            dev.construct(u)
        torch.cuda.synchronize()
        ds = dev.read_stats()
        assert int(ds["memCapacityReached"]) == 1 and int(ds["batchletIndex"]) == done < uploaded, (done, uploaded, taken)
        ref, fh = replay_first_hits(u, all_batches[:uploaded], persistent_bytes=cap)
        assert int(ref.stats["memCapacityReached"][0]) == 1
        assert_stats_equal(ds, ref.stats[0], STATS_BUILD_FIELDS, "memory guard, groups")
        nodes, pers, nn = host_image_of(dev)
        assert_dumps_equal(oracle.dump_image(nodes, nn), ref.dump(), "memory guard, groups")
        assert int(ds["allocatedBytes_persistent"]) <= cap and bool((dev.persistent[cap:] == 0x3C).all())
        # groups before the guard (a launch with fewer groups than batches), and cuts to one batch (more groups than launches of G would have)
        groups = sum(per_launch_groups)
        assert any(g < t for g, t in zip(per_launch_groups, taken)), f"no grouped launch: groups {per_launch_groups} for batches {taken}"
        assert sum(-(-t // G) for t in taken) < groups < done, f"groups {per_launch_groups} for batches {taken}"
        tagged = np.concatenate(all_batches[:uploaded])
        assert assert_voxel_winners(nodes, nn, tagged, batch_of_points(all_batches[:uploaded]), fh, _launch_bound(ends), u) == int(nodes["numVoxelsStored"][:nn].sum())
    finally:
        dev.close()


# ---- full size ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.slow
@pytest.mark.parametrize("name", ["terrain_36m", "config5_20m"])
def test_full_size_colours_within_a_group_of_the_first_hit(built_libs, name):
    _CACHE.clear()
    box = _inputs(name)[0]
    dev = _device(persistent_bytes=GROUP_PERSISTENT, ring_slots=abi.BATCH_STREAM_SIZE)
    try:
        u = dev.uniforms(W, H, _cam(box), box)
        tagged, batches, ref, fh = _reference(name, u)
        _ingest(dev, u, batches)
        nodes, pers, nn = _compare(dev, name, ref)
        assert assert_voxel_winners(nodes, nn, tagged, batch_of_points(batches), fh, lambda b: b + 5 - 1, u) == int(nodes["numVoxelsStored"][:nn].sum())
    finally:
        dev.close()
        _CACHE.clear()
