"""CPU tier of the view deltas (include/simlod_hip.h, "view deltas"): the numpy mirror OctreeExport.view_delta / ViewDelta.apply on oracle-built
octrees — camera pairs on the 3 M terrain, an octree that grows between two cuts, rule D7, the ABI, and the refusals, which precede device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import delta_ref as dr
import view_ref as vr
from simlod_amd import abi
from simlod_amd.octree_io import ViewDelta, delta_between

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def terrain(built_libs):
    return vr.terrain_3m()


def _u(box, cam):
    return vr.uniforms_of(box, vr.transform_of(cam, box))


@pytest.mark.parametrize("what,old,new", dr.PAIRS, ids=[p[0] for p in dr.PAIRS])
def test_delta_and_merge_give_the_fresh_view(terrain, what, old, new):
    full, box, _ = terrain
    held = full.view(_u(box, old[0]), **old[1])
    fresh, vc = full.view(_u(box, new[0]), return_counts=True, **new[1])
    delta = full.view_delta(_u(box, new[0]), held, **new[1])
    assert isinstance(delta, ViewDelta) and delta.counts["view"].tobytes() == vc.tobytes()
    dr.assert_delta_consistent(delta, held, fresh)
    kept, grown, added, dropped = dr.states(delta)
    assert grown == 0
    if what in dr.MIXED:
        assert kept > 0 and added > 0 and dropped > 0, (kept, added, dropped)
        assert 0 < delta.num_samples < fresh.num_samples
    else:                                                     # the camera that looks away: the new cut is empty, everything held goes
        sel = (held.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
        assert (kept, added) == (0, 0) and fresh.num_samples == 0
        assert np.array_equal(delta.dropped, np.nonzero(sel & (held.nodes["numSamples"] > 0))[0]) and dropped > 0
    # a KEPT entry's samples are the held entry's, and the dropped entries are exactly the held ones no entry kept
    e = delta.entries
    k = np.nonzero(e["state"] == abi.DELTA_KEPT)[0]
    hk = e["held"][k]
    assert all(np.array_equal(held.nodes[f][hk], delta.nodes[f][k]) for f in ("level", "X", "Y", "Z", "numSamples"))
    hsel = np.nonzero(((held.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0) & (held.nodes["numSamples"] > 0))[0]
    assert np.array_equal(np.sort(np.concatenate([hk, delta.dropped])), hsel)


def test_the_same_camera_sends_nothing(terrain):
    full, box, _ = terrain
    for cam in ("bird", "closer", "inside"):
        held = full.view(_u(box, cam))
        delta = full.view_delta(_u(box, cam), held)
        c = delta.counts
        assert int(c["numDeltaSamples"]) == 0 and int(c["numDropped"]) == 0 and int(c["numAdded"]) == 0 and delta.num_samples == 0
        assert int(c["numKept"]) == int(c["view"]["numSelected"]) > 0 and int(c["numKeptSamples"]) == held.num_samples
        dr.assert_delta_consistent(delta, held, held)


def test_nothing_held_is_the_view(terrain):
    """Rule D7."""
    full, box, _ = terrain
    u = _u(box, "closer")
    fresh = full.view(u, bias=1)
    for held in (None, full.view(_u(box, "away"))):
        delta = full.view_delta(u, held, bias=1)
        e, tb = delta.entries, delta.nodes
        sel = (tb["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
        assert (e["state"][sel] == abi.DELTA_ADDED).all() and np.array_equal(e["firstDelta"], tb["firstSample"]) and len(delta.dropped) == 0
        assert delta.samples.tobytes() == fresh.samples.tobytes() and delta.num_samples > 0
        if held is None:
            assert (e["held"] == abi.EXPORT_NONE).all()
        dr.assert_delta_consistent(delta, held, fresh)


def test_budget_error_sends_nothing(terrain):
    """Rule D1: no bias fits -> the table of maxBias, every entry NONE, no sample; what is held is dropped by rule D6."""
    full, box, _ = terrain
    u = _u(box, "closer")
    held = full.view(u, bias=2)
    fresh, vc = full.view(u, max_bias=0, budget=1, return_counts=True)
    delta = full.view_delta(u, held, max_bias=0, budget=1)
    assert int(vc["error"]) == abi.EXPORT_ERR_BUDGET and delta.counts["view"].tobytes() == vc.tobytes()
    assert delta.nodes.tobytes() == fresh.nodes.tobytes() and int(fresh.nodes["numSamples"].astype(np.int64).sum()) > 0
    e = delta.entries
    assert not e["state"].any() and not e["numKept"].any() and not e["numDelta"].any() and delta.num_samples == 0
    assert (e["held"] != abi.EXPORT_NONE).sum() > 0 and len(delta.dropped) == int(((held.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0).sum())
    assert delta.apply(held).num_samples == 0


@pytest.mark.parametrize("tails", [True, False])
def test_growth_between_two_cuts(built_libs, tails):
    """The uniform cube after four and after eight batches under `closer` at bias 2: nodes that grew keep their head under SIMLOD_DELTA_TAILS —
    on the oracle's octree the held samples are a prefix of the new list, so the merge gives the fresh view — and come whole without it."""
    before, after, box = dr.grown_cube()
    u = _u(box, "closer")
    held = before.view(u, bias=dr.CUBE_BIAS)
    fresh = after.view(u, bias=dr.CUBE_BIAS)
    delta = after.view_delta(u, held, bias=dr.CUBE_BIAS, tails=tails)
    dr.assert_delta_consistent(delta, held, fresh)
    kept, grown, added, dropped = dr.states(delta)
    changed = dr.kind_changed(delta, held)
    assert len(changed) >= 1 and (delta.entries["state"][changed] == abi.DELTA_ADDED).all()
    assert added > 0 and dropped > 0
    with_tails = after.view_delta(u, held, bias=dr.CUBE_BIAS, tails=True)
    g = with_tails.entries["state"] == abi.DELTA_GROWN
    assert g.sum() > 0
    if tails:
        assert grown == int(g.sum()) and 0 < int(delta.counts["numKeptSamples"]) and delta.num_samples < fresh.num_samples
        e = delta.entries
        assert (e["numKept"][g] == held.nodes["numSamples"][e["held"][g]]).all() and (e["numDelta"][g] > 0).all()
    else:
        assert grown == 0 and (delta.entries["state"][g] == abi.DELTA_ADDED).all() and not delta.entries["numKept"][g].any()
        assert dropped == dr.states(with_tails)[3] + int(g.sum())


def test_lowered_counts_send_the_tails(terrain):
    """A receiver that holds only the head of five nodes (1, 999, 1 000, 1 001 and n - 1 samples): with tails those nodes send samples[hs:] and
    nothing else is sent; without, they come whole."""
    full, box, _ = terrain
    u = _u(box, "closer")
    fresh = full.view(u)
    held, idx = dr.lowered(fresh)
    hs = held.nodes["numSamples"][idx].astype(np.int64)
    n = fresh.nodes["numSamples"][idx].astype(np.int64)
    assert hs.tolist()[:4] == [1, 999, 1000, 1001] and hs[4] == n[4] - 1 and (n > 2000).all()
    delta = full.view_delta(u, held, tails=True)
    dr.assert_delta_consistent(delta, held, fresh)
    assert dr.states(delta) == (int(fresh.nodes["numSamples"].astype(bool).sum()) - 5, 5, 0, 0)
    want = np.concatenate([fresh.samples[int(a) + int(k): int(a) + int(m)] for a, k, m in zip(fresh.nodes["firstSample"][idx], hs, n)])
    assert delta.samples.tobytes() == want.tobytes()
    whole = full.view_delta(u, held, tails=False)
    dr.assert_delta_consistent(whole, held, fresh)
    assert dr.states(whole) == (dr.states(delta)[0], 0, 5, 5) and whole.num_samples == int(n.sum()) and whole.dropped.tolist() == idx.tolist()


def test_delta_between_two_cuts_needs_no_octree(terrain):
    """The rules D2-D6 take two tables: a cropped or truncated held table is as good as any."""
    full, box, _ = terrain
    u = _u(box, "closer")
    fresh = full.view(u)
    held = full.view(_u(box, "inside"), max_level=3)
    assert held.num_nodes < fresh.num_nodes
    delta = delta_between(fresh, held)
    dr.assert_delta_consistent(delta, held, fresh)
    assert int(delta.counts["numKept"]) > 0 and int(delta.counts["numAdded"]) > 0


def test_abi_matches_the_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodDeltaEntry\) == (\d+)", src).group(1)) == abi.delta_entry_dtype.itemsize == 24
    assert int(re.search(r"sizeof\(SimlodDeltaCounts\) == (\d+)", src).group(1)) == abi.delta_counts_dtype.itemsize == 232
    for struct, dtype in (("SimlodDeltaEntry", abi.delta_entry_dtype), ("SimlodDeltaCounts", abi.delta_counts_dtype)):
        found = re.findall(rf"offsetof\({struct}, (\w+)\) == (\d+)", src)
        assert len(found) >= 4
        for field, off in found:
            assert dtype.fields[field][1] == int(off), (struct, field)
    assert abi.delta_entry_dtype.names == ("held", "state", "numKept", "numDelta", "firstDelta")
    assert abi.delta_counts_dtype.fields["view"][0] == abi.view_counts_dtype and abi.delta_counts_dtype.fields["view"][1] == 0
    for name, value in (("SIMLOD_DELTA_NONE", abi.DELTA_NONE), ("SIMLOD_DELTA_KEPT", abi.DELTA_KEPT), ("SIMLOD_DELTA_GROWN", abi.DELTA_GROWN),
                        ("SIMLOD_DELTA_ADDED", abi.DELTA_ADDED), ("SIMLOD_DELTA_TAILS", abi.DELTA_TAILS)):
        assert int(re.search(rf"#define {name}\s+(0x[0-9a-f]+|\d+)u", src).group(1), 0) == value, name


def test_library_refuses_before_device_work(built_libs):
    """Every refusal of the two calls precedes device work: hipErrorInvalidValue (1) without a GPU, the buffers untouched."""
    from simlod_amd import runtime
    L = runtime.lib()
    for sym in ("simlod_view_delta_buffer_min_bytes", "simlod_query_view_delta", "simlod_merge_view_delta"):
        assert sym in runtime.EXPORTED_SYMBOLS and hasattr(L, sym)
    box = (1.0, 1.0, 1.0)
    u = np.ascontiguousarray(vr.uniforms_of(box, vr.transform_of("bird", box))).reshape(1)
    cap, nh = 8, 5
    need = int(L.simlod_view_delta_buffer_min_bytes(cap, 0, nh))
    assert need > int(L.simlod_export_buffer_min_bytes(cap, 0)) and int(L.simlod_view_delta_buffer_min_bytes(cap, 5000, nh)) == need + 5 * 32
    assert int(L.simlod_view_delta_buffer_min_bytes(cap, 0, 0)) < need
    bufs = {k: np.full(n, 0xA5, np.uint8) for k, n in (("nodes", 152 * cap), ("stats", abi.stats_dtype.itemsize), ("held", 40 * nh), ("scratch", need), ("table", 40 * cap),
                                                       ("entries", 24 * cap), ("delta", 16 * 8), ("dropped", 4 * nh), ("counts", 232), ("held_samples", 16 * 8),
                                                       ("samples", 16 * 8), ("xcounts", 16))}
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(view=None, uu=u, scratch_bytes=need, null=(), flags=0, num_held=nh, dropped_cap=nh):
        g = {k: (None if k in null else b) for k, b in bufs.items()}
        v = abi.view_record() if view is None else view
        return L.simlod_query_view_delta(p(g["nodes"]), p(g["stats"]), p(uu), None if "view" in null else p(v), 20, p(g["held"]), num_held, flags, p(g["scratch"]),
                                         ctypes.c_uint64(scratch_bytes), p(g["table"]), cap, p(g["entries"]), p(g["delta"]), ctypes.c_uint64(8), p(g["dropped"]),
                                         dropped_cap, p(g["counts"]), None)

    for k in ("nodes", "stats", "scratch", "table", "entries", "counts", "view", "held", "dropped"):
        assert call(null=(k,)) == 1, k
    assert call(uu=None) == 1
    assert call(scratch_bytes=need - 1) == 1
    for flags in (2, 3, 0x80000000):
        assert call(flags=flags) == 1, flags
    for field, value in (("flags", 4), ("reserved", 1), ("minBias", 21), ("maxBias", 21)):
        v = abi.view_record()
        v[field] = value
        assert call(view=v) == 1, field
    for field in ("minNodeSize", "width", "height"):
        w = u.copy()
        w[field] = np.nan
        assert call(uu=w) == 1, field
    w = u.copy()
    w["transform_updateBound"][0, 3, 2] = -np.inf
    assert call(uu=w) == 1

    def merge(null=(), scratch_bytes=need, num_held=nh, sample_cap=8):
        g = {k: (None if k in null else b) for k, b in bufs.items()}
        return L.simlod_merge_view_delta(p(g["held"]), num_held, p(g["held_samples"]), p(g["table"]), p(g["entries"]), cap, p(g["delta"]), p(g["scratch"]),
                                         ctypes.c_uint64(scratch_bytes), p(g["samples"]), ctypes.c_uint64(sample_cap), p(g["xcounts"]), None)

    for k in ("held", "table", "entries", "scratch", "samples", "xcounts"):
        assert merge(null=(k,)) == 1, k
    assert merge(scratch_bytes=need - 1) == 1
    assert all((b == 0xA5).all() for b in bufs.values())
