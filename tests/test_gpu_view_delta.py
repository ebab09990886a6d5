"""GPU tier: simlod_query_view_delta and simlod_merge_view_delta (include/simlod_hip.h, "view deltas") through the C ABI with poisoned buffers —
counts, table, entries, delta, dropped and the bytes behind each against the host mirror OctreeExport.view_delta, and the device merge against
a raw simlod_query_view of the same camera: camera pairs, offsets in the middle of a chunk, octrees that grow between two cuts, a level of
4 096 entries, octrees 13 and 20 deep, capacities, refusals, a budget error, rule D8, and held tables that are garbage."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import deep_ref
import delta_ref as dr
import view_ref as vr
from simlod_amd import abi, camera
from simlod_amd.octree_io import OctreeExport
from test_gpu_view import Raw as ViewRaw, _box_of, _uniforms
from util import _build, _device, _ingest

pytestmark = pytest.mark.gpu
W, H = vr.WIDTH, vr.HEIGHT
POISON = 0xA5


def _mk(dev, n):
    return torch.full((max(int(n), 16),), POISON, dtype=torch.uint8, device=dev.device)


class RawDelta:
    """One simlod_query_view_delta call with every buffer poisoned: rc, the counts record, and the buffers as the call left them.  `held`: an
    OctreeExport, None, or the bytes of a held table (a uint8 array of whole 40-byte records)."""

    def __init__(self, dev, u, held, view=None, max_level=20, *, tails=False, flags=None, table_cap=None, delta_cap=None, dropped_cap=None, count_only=False,
                 scratch_bytes=None, null=(), num_held=None):
        st = dev.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        hb = None if held is None else held if isinstance(held, np.ndarray) else held.nodes.view(np.uint8).reshape(-1)
        self.num_held = (0 if hb is None else len(hb) // 40) if num_held is None else num_held
        self.held_t = None if hb is None else torch.from_numpy(np.ascontiguousarray(hb)).to(dev.device)
        self.held_before = None if hb is None else self.held_t.clone()
        self.table_cap = nn if table_cap is None else table_cap
        self.delta_cap = bound if delta_cap is None else delta_cap
        self.dropped_cap = max(self.num_held, 0) if dropped_cap is None else dropped_cap
        L = dev.L
        need = int(L.simlod_view_delta_buffer_min_bytes(self.table_cap, bound, self.num_held)) if scratch_bytes is None else scratch_bytes
        self.scratch, self.table, self.entries = _mk(dev, need), _mk(dev, (self.table_cap + 4) * 40), _mk(dev, (self.table_cap + 4) * 24)
        self.delta, self.dropped = _mk(dev, (self.delta_cap + 1000) * 16), _mk(dev, (self.dropped_cap + 64) * 4)
        self.counts_t = _mk(dev, abi.delta_counts_dtype.itemsize + 56)
        uu, up = dev._u(u)
        v = abi.view_record() if view is None else view
        ptr = {k: (None if k in null or t is None else dev._p(t)) for k, t in (("nodes", dev.nodes), ("stats", dev.stats), ("scratch", self.scratch), ("table", self.table),
                                                                                ("entries", self.entries), ("counts", self.counts_t), ("held", self.held_t),
                                                                                ("dropped", self.dropped), ("delta", None if count_only else self.delta))}
        self.rc = L.simlod_query_view_delta(ptr["nodes"], ptr["stats"], None if "uniforms" in null else up, None if "view" in null else ctypes.c_void_p(v.ctypes.data),
                                            max_level, ptr["held"], self.num_held, (abi.DELTA_TAILS if tails else 0) if flags is None else flags, ptr["scratch"],
                                            ctypes.c_uint64(need), ptr["table"], self.table_cap, ptr["entries"], ptr["delta"], ctypes.c_uint64(self.delta_cap),
                                            ptr["dropped"], self.dropped_cap, ptr["counts"], dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:232].view(abi.delta_counts_dtype)[0]

    def bytes_of(self, which, n):
        t, size = {"table": (self.table, 40), "entries": (self.entries, 24), "delta": (self.delta, 16), "dropped": (self.dropped, 4)}[which]
        return t[: int(n) * size].cpu().numpy().tobytes()

    def poison_behind(self, nodes, samples, dropped):
        return (bool((self.table[nodes * 40:] == POISON).all()) and bool((self.entries[nodes * 24:] == POISON).all()) and
                bool((self.delta[samples * 16:] == POISON).all()) and bool((self.dropped[dropped * 4:] == POISON).all()) and
                bool((self.counts_t[232:] == POISON).all()))

    def untouched(self):
        return self.poison_behind(0, 0, 0) and bool((self.counts_t == POISON).all()) and bool((self.scratch == POISON).all())

    def held_unchanged(self):
        return self.held_t is None or bool((self.held_t == self.held_before).all())


class RawMerge:
    """One simlod_merge_view_delta call on the buffers a RawDelta left, with the held samples given (an array of abi.point_dtype, or None)."""

    def __init__(self, dev, raw, held_samples, sample_cap=None):
        n = int(raw.counts["view"]["numNodes"])
        total = int(raw.counts["numDeltaSamples"]) + int(raw.counts["numKeptSamples"])
        self.sample_cap = total if sample_cap is None else sample_cap
        hs = None if held_samples is None or len(held_samples) == 0 else torch.from_numpy(np.ascontiguousarray(held_samples).view(np.uint8).reshape(-1)).to(dev.device)
        need = int(dev.L.simlod_view_delta_buffer_min_bytes(n, total, raw.num_held))
        scratch, self.samples, self.counts_t = _mk(dev, need), _mk(dev, (self.sample_cap + 1000) * 16), _mk(dev, 16 + 48)
        opt = lambda t: None if t is None else dev._p(t)
        self.rc = dev.L.simlod_merge_view_delta(opt(raw.held_t), raw.num_held, opt(hs), dev._p(raw.table), dev._p(raw.entries), n, dev._p(raw.delta), dev._p(scratch),
                                                ctypes.c_uint64(need), dev._p(self.samples), ctypes.c_uint64(self.sample_cap), dev._p(self.counts_t), dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:16].view(abi.export_counts_dtype)[0]

    def sample_bytes(self, n):
        return self.samples[: int(n) * 16].cpu().numpy().tobytes()

    def poison_behind(self, samples):
        return bool((self.samples[samples * 16:] == POISON).all()) and bool((self.counts_t[16:] == POISON).all())


def _assert_delta(raw, mirror, what):
    assert raw.rc == 0, what
    assert raw.counts.tobytes() == mirror.counts.tobytes(), f"{what}: counts {raw.counts} against the mirror's {mirror.counts}"
    n, ns, nd = mirror.num_nodes, mirror.num_samples, len(mirror.dropped)
    assert raw.bytes_of("table", n) == mirror.nodes.tobytes(), f"{what}: the table differs"
    assert raw.bytes_of("entries", n) == mirror.entries.tobytes(), f"{what}: the entries differ"
    assert raw.bytes_of("delta", ns) == mirror.samples.tobytes(), f"{what}: the delta samples differ"
    assert raw.bytes_of("dropped", nd) == mirror.dropped.tobytes(), f"{what}: the dropped list differs"
    assert raw.poison_behind(n, ns, nd), f"{what}: written past the result"
    assert raw.held_unchanged(), f"{what}: the held table changed"


def _assert_merge(dev, raw, held, u, view, what, max_level=20):
    """The device merge of `raw` and the held samples against a raw simlod_query_view of the same camera."""
    fresh = ViewRaw(dev, u, view, max_level)
    assert fresh.rc == 0 and int(fresh.counts["error"]) == 0, what
    assert raw.counts["view"].tobytes() == fresh.counts.tobytes() and raw.bytes_of("table", int(fresh.counts["numNodes"])) == fresh.table_bytes(), f"{what}: rule D1"
    merged = RawMerge(dev, raw, None if held is None else held.samples)
    ns = int(fresh.counts["numSamples"])
    assert merged.rc == 0 and (int(merged.counts["numNodes"]), int(merged.counts["error"]), int(merged.counts["numSamples"])) == (int(fresh.counts["numNodes"]), 0, ns), what
    assert merged.sample_bytes(ns) == fresh.sample_bytes(), f"{what}: the merge is not the fresh view"
    assert merged.poison_behind(ns), f"{what}: the merge wrote past its result"
    return fresh


def _host(raw_view, base, max_level=20):
    """A raw simlod_query_view result as an OctreeExport on the host: what a receiver holds."""
    nn, ns = int(raw_view.counts["numNodes"]), int(raw_view.counts["numSamples"])
    return OctreeExport(np.frombuffer(raw_view.table_bytes(nn), np.uint8).copy(), np.frombuffer(raw_view.sample_bytes(ns), np.uint8).copy(), base["boxMin"], base["boxMax"],
                        max_level, abi.EXPORT_VISIBLE)


def _check_pair(dev, base, full, old, new, what, tails=False, held=None):
    """One camera pair: the held cut from the mirror (which test_gpu_view pins to the device), the raw delta against the mirror, the merge
    against a fresh view.  -> the mirror's delta"""
    box, mn = _box_of(base)
    cam = lambda c: _uniforms(dev, base, vr.transform_of(c, box, mn))
    if held is None:
        held = full.view(cam(old[0]), **old[1]) if old is not None else None
    u = cam(new[0])
    view = abi.view_record(new[1].get("bias", 0))
    mirror = full.view_delta(u, held, tails=tails, **new[1])
    raw = RawDelta(dev, u, held, view, tails=tails)
    _assert_delta(raw, mirror, what)
    _assert_merge(dev, raw, held, u, view, what)
    return mirror


@pytest.fixture(scope="module")
def terrain3m(built_libs):
    batches, box = vr.terrain_3m_batches()
    dev = _device()
    u = dev.uniforms(W, H, vr.transform_of("bird", box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    return dev, u, box, dev.export_octree(u)


ALL_PAIRS = dr.PAIRS + [("closer -> closer", ("closer", {}), ("closer", {})), ("nothing -> closer", None, ("closer", {"bias": 1}))]


def _static_pairs(dev, u, full, source):
    for what, old, new in ALL_PAIRS:
        m = _check_pair(dev, u, full, old, new, f"{what} ({source})")
        kept, grown, added, dropped = dr.states(m)
        if what in dr.MIXED:
            assert kept > 0 and added > 0 and dropped > 0 and grown == 0, what
        elif what == "closer -> away":
            assert (kept, added) == (0, 0) and dropped > 0
        elif what == "closer -> closer":
            assert kept > 0 and (added, dropped, m.num_samples) == (0, 0, 0)
        else:                                                                        # rule D7
            assert kept == 0 and added > 0 and dropped == 0 and np.array_equal(m.entries["firstDelta"], m.nodes["firstSample"])


def _mid_chunk(dev, u, box, full, source):
    """The held table of the same camera with numSamples lowered to 1, 999, 1 000, 1 001 and n - 1 on five nodes: under SIMLOD_DELTA_TAILS the delta
    is exactly samples[hs:] of those nodes — copies that begin in the middle of a chunk, at a chunk's end, at its start —, without it they come whole."""
    uc = _uniforms(dev, u, vr.transform_of("closer", box))
    fresh = full.view(uc)
    held, idx = dr.lowered(fresh)
    m = _check_pair(dev, u, full, None, ("closer", {}), f"lowered, tails ({source})", tails=True, held=held)
    hs, n = held.nodes["numSamples"][idx].astype(np.int64), fresh.nodes["numSamples"][idx].astype(np.int64)
    want = np.concatenate([fresh.samples[int(a) + int(k): int(a) + int(c)] for a, k, c in zip(fresh.nodes["firstSample"][idx], hs, n)])
    assert m.samples.tobytes() == want.tobytes() and dr.states(m)[1:] == (5, 0, 0)
    w = _check_pair(dev, u, full, None, ("closer", {}), f"lowered, whole ({source})", tails=False, held=held)
    assert dr.states(w)[1:] == (0, 5, 5) and w.num_samples == int(n.sum())


# ---- 1. camera pairs and offsets inside a chunk --------------------------------------------------------------------------------------------------
def test_pairs_on_the_3m_terrain(terrain3m):
    dev, u, box, full = terrain3m
    _static_pairs(dev, u, full, "as built")


def test_offsets_in_the_middle_of_a_chunk(terrain3m):
    dev, u, box, full = terrain3m
    _mid_chunk(dev, u, box, full, "as built")


def test_pairs_and_offsets_when_every_list_is_walked(terrain3m):
    dev, u, box, full = terrain3m
    dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))            # the builder's chunk table no longer counts
    _static_pairs(dev, u, full, "walk")
    _mid_chunk(dev, u, box, full, "walk")


def test_pairs_on_the_shifted_terrain(built_libs):
    dev, u, _, _ = _build("terrain_4x100k", cases.GEOREF)
    full = dev.export_octree(u)
    seen = np.zeros(4, np.int64)
    for what, old, new in ALL_PAIRS:
        seen += dr.states(_check_pair(dev, u, full, old, new, f"georef {what}"))
    assert (seen[[0, 2, 3]] > 0).all(), seen


def test_python_entry_points(terrain3m):
    dev, u, box, full = terrain3m
    ub, uc = (_uniforms(dev, u, vr.transform_of(c, box)) for c in ("bird", "closer"))
    held = dev.query_view(ub)
    mirror = full.view_delta(uc, full.view(ub))
    delta, c = dev.query_view_delta(uc, held, return_counts=True)
    assert c.tobytes() == mirror.counts.tobytes() == dev.count_view_delta(uc, held).tobytes()
    assert delta.device.type == "cuda" and all(getattr(delta, f).tobytes() == getattr(mirror, f).tobytes() for f in ("nodes", "entries", "samples", "dropped"))
    merged = dev.merge_view_delta(held, delta)
    fresh = dev.query_view(uc)
    assert merged.select == abi.EXPORT_VISIBLE and merged.nodes.tobytes() == fresh.nodes.tobytes() and merged.samples.tobytes() == fresh.samples.tobytes()
    merged.validate()
    first = dev.query_view_delta(ub, None)
    assert dev.merge_view_delta(None, first).samples.tobytes() == held.samples.tobytes()


# ---- 2. octrees that grow between two cuts: this decides rule D4 -----------------------------------------------------------------------------------
def _grow(dev, u, uc, batches, held_after, bias, what):
    """Ingest `held_after` batches, take the held cut on the device, ingest the rest; the delta with and without tails against the mirror, the
    merge against a fresh view.  -> the mirror's delta with tails"""
    dev.reset(u)
    _ingest(dev, u, batches[:held_after])
    view = abi.view_record(bias)
    held = _host(ViewRaw(dev, uc, view), u)
    assert held.num_samples > 0
    _ingest(dev, u, batches[held_after:])
    full = dev.export_octree(u)
    out = None
    for tails in (True, False):
        mirror = full.view_delta(uc, held, bias=bias, tails=tails)
        raw = RawDelta(dev, uc, held, view, tails=tails)
        _assert_delta(raw, mirror, f"{what}, tails {tails}")
        _assert_merge(dev, raw, held, uc, view, f"{what}, tails {tails}")
        out = out or mirror
    return out, held


def test_growth_of_the_uniform_cube(built_libs):
    batches, box = dr.cube_batches()
    dev = _device()
    u = dev.uniforms(W, H, vr.transform_of("closer", box), box)
    m, held = _grow(dev, u, _uniforms(dev, u, vr.transform_of("closer", box)), batches, dr.CUBE_HELD_AFTER, dr.CUBE_BIAS, "uniform cube")
    kept, grown, added, dropped = dr.states(m)
    changed = dr.kind_changed(m, held)
    assert grown > 0 and added > 0 and dropped > 0 and len(changed) >= 1 and (m.entries["state"][changed] == abi.DELTA_ADDED).all()
    assert 0 < int(m.counts["numKeptSamples"]) and (m.entries["numKept"][m.entries["state"] == abi.DELTA_GROWN] % 1000 != 0).any()


def test_growth_of_the_3m_terrain(built_libs, held_after=1):
    """The held cut after one batch of a million, the new one after all three."""
    batches, box = vr.terrain_3m_batches()
    dev = _device()
    u = dev.uniforms(W, H, vr.transform_of("bird", box), box)
    m, _ = _grow(dev, u, _uniforms(dev, u, vr.transform_of("closer", box)), batches, held_after, 0, f"3 M terrain after {held_after}")
    assert dr.states(m)[1] > 0 and int(m.counts["numKeptSamples"]) > 0


# ---- 3. width: several workgroups in the match, several turns in the compaction ------------------------------------------------------------------------
def test_levels_of_more_than_1024_entries(built_libs):
    tree = vr.complete_tree(4)
    assert tree.num_nodes == 4681 and int((tree.nodes["level"] == 4).sum()) == 4096
    dev = _device()
    dev.import_octree(tree)
    box = (1.0, 1.0, 1.0)
    base = dev.uniforms(W, H, vr.transform_of("inside", box), box)
    full = dev.export_octree(base)
    for old, new in ((("closer", {}), ("closer", {"bias": 1})), (("closer", {"bias": 1}), ("bird", {}))):
        m = _check_pair(dev, base, full, old, new, f"complete tree {old} -> {new}")
        kept, grown, added, dropped = dr.states(m)
        assert kept > 0 and added > 0 and dropped > 0
        d = m.dropped
        assert len(np.unique(d // 1024)) >= 3, "the dropped entries must come from several turns of the compaction"
        assert len(np.unique(np.nonzero(m.entries["held"] != abi.EXPORT_NONE)[0] // 256)) >= 10, "matches in many workgroups"


# ---- 4. depth: level-13 and level-20 keys ----------------------------------------------------------------------------------------------------------------
def _deep_device(name):
    d = deep_ref.built(name)
    dev = _device()
    u = dev.uniforms(W, H, vr.transform_of("bird", d.box), d.box)
    dev.reset(u)
    _ingest(dev, u, d.batches)
    return d, dev, u, dev.export_octree(u)


def _deep_pair(dev, u, full, T, min_node_size, what):
    uc = _uniforms(dev, u, T)
    uc["minNodeSize"] = min_node_size
    held = full.view(uc, bias=2)
    mirror = full.view_delta(uc, held)
    raw = RawDelta(dev, uc, held)
    _assert_delta(raw, mirror, what)
    _assert_merge(dev, raw, held, uc, abi.view_record(), what)
    return mirror


def test_depth_13(built_libs):
    d, dev, u, full = _deep_device("d13x")
    m = _deep_pair(dev, u, full, deep_ref.close_cam(d, W, H), vr.MIN_NODE_SIZE, "d13x close-up against bias 2")
    deep = m.nodes["level"] == deep_ref.LEAF_LEVEL
    assert int((m.entries["state"][deep] == abi.DELTA_KEPT).sum()) >= 8 and int((m.entries["state"][deep] == abi.DELTA_ADDED).sum()) >= 1
    assert len(m.dropped) >= 1


def test_depth_20(built_libs):
    """Level-20 nodes are a millionth of the box wide: a minNodeSize of 2^-11 pixels makes the one with points large at bias 0 and small at bias 2,
    2^-12 keeps it at both."""
    d, dev, u, full = _deep_device("d20")
    p = np.asarray(deep_ref.POINT, dtype=np.float64)
    T = camera.lookat_transform(tuple(p + np.asarray((0.9, -0.7, 0.8))), tuple(p), W, H)
    states = {}
    for k in (11, 12):
        m = _deep_pair(dev, u, full, T, 2.0 ** -k, f"d20 minNodeSize 2^-{k}")
        deep = m.nodes["level"] == 20
        assert int(deep.sum()) == 8 and (m.entries["held"][deep] != abi.EXPORT_NONE).all(), "the level-20 keys must match"
        assert len(set(m.entries["held"][deep].tolist())) == 8
        states[k] = sorted(set(m.entries["state"][deep].tolist()) - {abi.DELTA_NONE})
    assert states == {11: [abi.DELTA_ADDED], 12: [abi.DELTA_KEPT]}, states


# ---- 5. capacities, count only, refusals, a budget error, rule D8 -----------------------------------------------------------------------------------
def test_capacities_and_count_only(terrain3m):
    dev, u, box, full = terrain3m
    ub, uc = (_uniforms(dev, u, vr.transform_of(c, box)) for c in ("bird", "closer"))
    held = full.view(ub)
    mirror = full.view_delta(uc, held)
    nn, ns, nd = mirror.num_nodes, mirror.num_samples, len(mirror.dropped)
    assert nn > 1 and ns > 0 and nd > 1
    nodes_before, stats_before = dev.nodes.clone(), dev.stats.clone()
    # exact capacities: the full result
    exact = RawDelta(dev, uc, held, table_cap=nn, delta_cap=ns, dropped_cap=nd, scratch_bytes=int(dev.L.simlod_view_delta_buffer_min_bytes(nn, ns, held.num_nodes)))
    _assert_delta(exact, mirror, "exact capacities")
    # count only: table, entries, dropped and counts are complete, no sample is written; no more scratch than the bound without samples
    cnt = RawDelta(dev, uc, held, count_only=True, scratch_bytes=int(dev.L.simlod_view_delta_buffer_min_bytes(nn, 0, held.num_nodes)))
    assert cnt.rc == 0 and cnt.counts.tobytes() == mirror.counts.tobytes()
    assert all(cnt.bytes_of(w, k) == exact.bytes_of(w, k) for w, k in (("table", nn), ("entries", nn), ("dropped", nd))) and cnt.poison_behind(nn, 0, nd)
    # ... and without a dropped list: it is counted
    bare = RawDelta(dev, uc, held, count_only=True, null=("dropped",), dropped_cap=0)
    assert bare.rc == 0 and bare.counts.tobytes() == mirror.counts.tobytes() and bare.poison_behind(nn, 0, 0)
    want = mirror.counts.copy()
    want["view"]["error"] = abi.EXPORT_ERR_CAPACITY
    # one delta sample short: the error bit, exact counts, no sample written
    short = RawDelta(dev, uc, held, delta_cap=ns - 1)
    assert short.rc == 0 and short.counts.tobytes() == want.tobytes() and short.poison_behind(nn, 0, nd)
    assert short.bytes_of("entries", nn) == mirror.entries.tobytes() and short.bytes_of("dropped", nd) == mirror.dropped.tobytes()
    # one dropped index short: the error bit, exact counts, nothing behind the capacity; the delta is complete
    few = RawDelta(dev, uc, held, dropped_cap=nd - 1)
    assert few.rc == 0 and few.counts.tobytes() == want.tobytes() and few.poison_behind(nn, ns, nd - 1)
    assert few.bytes_of("dropped", nd - 1) == mirror.dropped[:-1].tobytes() and few.bytes_of("delta", ns) == mirror.samples.tobytes()
    # one table entry short: the error bit, nothing behind the capacity, no sample
    small = RawDelta(dev, uc, held, table_cap=nn - 1)
    assert small.rc == 0 and int(small.counts["view"]["error"]) & abi.EXPORT_ERR_CAPACITY and int(small.counts["view"]["numNodes"]) <= nn - 1
    assert small.poison_behind(nn - 1, 0, held.num_nodes)
    # a scratch buffer with room for the tables' part but not for the delta's items: the device says so
    assert mirror_items(mirror) > 2 * nn + 1
    lean = RawDelta(dev, uc, held, scratch_bytes=int(dev.L.simlod_view_delta_buffer_min_bytes(nn, 0, held.num_nodes)))
    assert lean.rc == 0 and lean.counts.tobytes() == want.tobytes() and lean.poison_behind(nn, 0, nd)
    # the merge: one sample short
    m = RawMerge(dev, exact, held.samples, sample_cap=ns + int(mirror.counts["numKeptSamples"]) - 1)
    assert m.rc == 0 and int(m.counts["error"]) == abi.EXPORT_ERR_CAPACITY and int(m.counts["numSamples"]) == ns + int(mirror.counts["numKeptSamples"]) and m.poison_behind(0)
    # rule D8
    assert bool((dev.nodes == nodes_before).all()) and bool((dev.stats == stats_before).all())


def mirror_items(mirror):
    """The copy pieces of a delta: per entry the chunks its samples [numKept, n) touch."""
    e = mirror.entries
    k, d = e["numKept"].astype(np.int64), e["numDelta"].astype(np.int64)
    return int(np.where(d > 0, (k + d + 999) // 1000 - k // 1000, 0).sum())


def test_budget_error(terrain3m):
    dev, u, box, full = terrain3m
    uc = _uniforms(dev, u, vr.transform_of("closer", box))
    held = full.view(uc, bias=2)
    view = abi.view_record(0, 0, 1)
    mirror = full.view_delta(uc, held, max_bias=0, budget=1)
    raw = RawDelta(dev, uc, held, view)
    _assert_delta(raw, mirror, "no bias fits")
    assert int(raw.counts["view"]["error"]) == abi.EXPORT_ERR_BUDGET and int(raw.counts["numDeltaSamples"]) == 0 and int(raw.counts["numDropped"]) > 0
    assert not mirror.entries["state"].any()
    m = RawMerge(dev, raw, held.samples)
    assert m.rc == 0 and int(m.counts["error"]) == 0 and int(m.counts["numSamples"]) == 0 and m.poison_behind(0)


def test_invalid_arguments_enqueue_nothing(built_libs):
    dev, u, _, box = _build("uniform_3x40k")
    nn = int(dev.read_stats()["numNodes"])
    ok = _uniforms(dev, u, vr.transform_of("bird", box))
    held = dev.export_octree(u).view(_uniforms(dev, u, vr.transform_of("closer", box)))

    def refused(uu=ok, **kw):
        raw = RawDelta(dev, uu, held, **kw)
        assert raw.rc == 1, kw                                                          # hipErrorInvalidValue
        assert raw.untouched(), kw

    for null in ("nodes", "stats", "uniforms", "view", "scratch", "table", "entries", "counts", "held", "dropped"):
        refused(null=(null,))
    for flags in (2, 3, 1 << 31):
        refused(flags=flags)
    for field, value in (("flags", 4), ("reserved", 1), ("minBias", 3), ("maxBias", 21)):
        v = abi.view_record(0, 2)
        v[field] = value
        refused(view=v)
    for field, value in (("minNodeSize", np.nan), ("width", np.inf)):
        w = np.array(ok, copy=True)
        w[field] = value
        refused(uu=w)
    refused(scratch_bytes=int(dev.L.simlod_view_delta_buffer_min_bytes(nn, 0, held.num_nodes)) - 1)
    # what may be null: the delta (count only), the held table with numHeld 0, the dropped list with capacity 0
    assert RawDelta(dev, ok, held, count_only=True).rc == 0
    assert RawDelta(dev, ok, None).rc == 0
    assert RawDelta(dev, ok, held, null=("dropped",), dropped_cap=0).rc == 0


# ---- 6. held tables that are garbage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "shuffled", "swapped"])
def test_garbage_held_tables(terrain3m, kind):
    """Rule D2 promises little for a held table this library did not write — the call returns, reads nothing outside the table, writes nothing
    outside its outputs — and one thing follows by construction: what it does not find it sends, so the merge of its own result is the view."""
    dev, u, box, full = terrain3m
    ub, uc = (_uniforms(dev, u, vr.transform_of(c, box)) for c in ("bird", "closer"))
    held = full.view(ub)
    rs = np.random.RandomState(23)
    if kind == "random":
        hb = rs.randint(0, 256, size=held.num_nodes * 40).astype(np.uint8)
        garbage = OctreeExport(hb, np.zeros(0, abi.point_dtype), held.box_min, held.box_max)
    elif kind == "shuffled":
        garbage = OctreeExport(held.nodes[rs.permutation(held.num_nodes)].copy(), held.samples, held.box_min, held.box_max)
        hb = garbage.nodes.view(np.uint8).reshape(-1)
    else:
        t = held.nodes.copy()                                                  # ten pairs of entries change places: some keys are still found
        for _ in range(10):
            i, j = rs.randint(0, len(t), 2)
            t[[i, j]] = t[[j, i]]
        hb = t.view(np.uint8).reshape(-1)
        garbage = OctreeExport(hb, held.samples, held.box_min, held.box_max)
    mirror = full.view_delta(uc, garbage)
    raw = RawDelta(dev, uc, hb)
    _assert_delta(raw, mirror, f"{kind} held table")
    fresh = ViewRaw(dev, uc)
    if kind == "random":
        assert int(raw.counts["numKept"]) == 0 and int(raw.counts["numDeltaSamples"]) == int(fresh.counts["numSamples"])
    elif kind == "swapped":
        assert 0 < int(raw.counts["numKept"]) < int(full.view_delta(uc, held).counts["numKept"])
    merged = RawMerge(dev, raw, garbage.samples)
    ns = int(fresh.counts["numSamples"])
    assert merged.rc == 0 and int(merged.counts["error"]) == 0 and int(merged.counts["numSamples"]) == ns
    assert merged.sample_bytes(ns) == fresh.sample_bytes() and merged.poison_behind(ns)
