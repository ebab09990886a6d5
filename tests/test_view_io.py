"""CPU tier of the view queries (include/simlod_hip.h, "view queries"): the numpy mirror OctreeExport.view against the oracle's frames on
oracle-built octrees (rule V8 with the oracle in the rasteriser's place), the budget rule, the two flags, and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import cases
import deep_ref
import region_ref
import view_ref
from simlod_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIASES = range(9)
TREES = ["terrain_4x100k", "terrain_3m", "d13x", "d20", "georef"]


def _tree(name):
    """-> (full export, box, box_min, HostOctree)"""
    if name == "terrain_3m":
        ex, box, ho = view_ref.terrain_3m()
        return ex, box, (0.0, 0.0, 0.0), ho
    if name in ("d13x", "d20"):
        d = deep_ref.built(name)
        return d.export, d.box, (0.0, 0.0, 0.0), d.ho
    mn = cases.GEOREF if name == "georef" else (0.0, 0.0, 0.0)
    ex, _, box, ho = region_ref.host_octree("terrain_4x100k", box_min=mn)
    return ex, box, tuple(float(np.float32(v)) for v in mn), ho


@pytest.fixture(scope="module")
def terrain(built_libs):
    return view_ref.terrain_3m()


@pytest.mark.parametrize("name", TREES)
def test_mirror_selects_what_the_oracle_draws(built_libs, name):
    """Five cameras at 1920 x 1080, minNodeSize 64, bias 0..8: the keys of the mirror's selected entries equal the keys of the oracle's visible
    records after a frame with minNodeSize 64 * 2^b, and S(b) the samples those records hold.  (The oracle takes min / max where the device
    and the mirror take fminf / fmaxf: they differ only where a corner has w == 0, which none of these cameras produces — the device follows
    r_visible there.)"""
    full, box, mn, ho = _tree(name)
    drawn = 0
    for cam in view_ref.CAMERAS:
        # (the shifted terrain's bird camera is the one the box-origin tests use)
        T = cases.shifted_cam(box, mn, view_ref.WIDTH, view_ref.HEIGHT) if (name, cam) == ("georef", "bird") else view_ref.transform_of(cam, box, mn)
        u0 = view_ref.uniforms_of(box, T, box_min=mn)
        ladder, c0 = view_ref.ladder_of(full, u0)
        for b in BIASES:
            keys, held = view_ref.oracle_visible(ho, view_ref.uniforms_of(box, T, b, box_min=mn, show_points=False))
            ex, c = full.view(u0, bias=b, max_bias=b, return_counts=True)
            assert np.array_equal(view_ref.selected_keys(ex), keys), f"{name} {cam} bias {b}: {int(c['numSelected'])} selected, the oracle draws {len(keys)}"
            assert ladder[b] == held == int(c["numSamples"]) == ex.num_samples, f"{name} {cam} bias {b}"
            assert int(c["bias"]) == b and int(c["numSelected"]) == len(keys) and int(c["error"]) == 0 and int(c["numInside"]) == int(c0["numInside"])
            ex.validate()
            drawn += len(keys)
        if cam == "away":
            assert not any(ladder), "the camera that looks away selects nothing"
    assert drawn > 0


def test_ladders_of_the_3m_terrain(terrain):
    """What the budget cases below and on the device rely on: `closer` has at least four distinct non-zero rungs, `inside` is not monotone."""
    full, box, _ = terrain
    closer, _ = view_ref.ladder_of(full, view_ref.uniforms_of(box, view_ref.transform_of("closer", box)))
    view_ref.assert_closer_ladder(closer)
    inside, _ = view_ref.ladder_of(full, view_ref.uniforms_of(box, view_ref.transform_of("inside", box)))
    view_ref.assert_not_monotone(inside)


def test_budget_rule_on_the_mirror(terrain):
    full, box, _ = terrain
    u = view_ref.uniforms_of(box, view_ref.transform_of("closer", box))
    S, _ = view_ref.ladder_of(full, u)
    view_ref.assert_closer_ladder(S)

    def chosen(**kw):
        ex, c = full.view(u, return_counts=True, **kw)
        return int(c["bias"]), int(c["error"]), int(c["numSamples"]), ex

    assert chosen(budget=S[1])[:3] == (1, 0, S[1])
    assert chosen(budget=S[1] - 1)[:3] == (2, 0, S[2])
    assert chosen(budget=0)[:3] == (view_ref.first_zero(S), 0, 0)
    assert chosen(bias=2)[:3] == (2, 0, S[2])
    bias, err, ns, ex = chosen(max_bias=6, budget=S[6] - 1)
    assert (bias, err, ns) == (6, abi.EXPORT_ERR_BUDGET, S[6]) and ex.num_samples == 0
    assert int(ex.nodes["numSamples"].astype(np.int64).sum()) == S[6], "the table is complete for maxBias"
    with pytest.raises(ValueError):
        full.view(u, max_bias=6, budget=S[6] - 1)
    ui = view_ref.uniforms_of(box, view_ref.transform_of("inside", box))
    Si, _ = view_ref.ladder_of(full, ui)
    up = view_ref.assert_not_monotone(Si)
    # a budget between S(up) and S(up + 1), everything finer too large: the finest cut that fits wins, not the coarsest
    assert all(s > Si[up] for s in Si[:up])
    _, c = full.view(ui, budget=(Si[up] + Si[up + 1]) // 2, return_counts=True)
    assert int(c["bias"]) == up and int(c["numSamples"]) == Si[up]


def test_flags_on_the_mirror(terrain):
    full, box, _ = terrain
    for cam in view_ref.CAMERAS:
        u = view_ref.uniforms_of(box, view_ref.transform_of(cam, box))
        for b in (0, 2, 5):
            culled, all_ = (set(view_ref.selected_keys(full.view(u, bias=b, max_bias=b, cull=c)).tolist()) for c in (True, False))
            assert culled <= all_, f"{cam} bias {b}"
        if cam == "away":
            assert not culled and len(set(view_ref.selected_keys(full.view(u, cull=False)).tolist())) > 0
    u = view_ref.uniforms_of(box, view_ref.transform_of("closer", box))
    S, _ = view_ref.ladder_of(full, u)
    z = view_ref.first_zero(S)
    ex, c = full.view(u, bias=z, max_bias=z, draw_small_root=True, return_counts=True)
    root = int(full.nodes["numSamples"][0])
    assert view_ref.selected_keys(ex).tolist() == [0] and ex.num_samples == root == int(c["numSamples"]) and root > 0
    assert np.array_equal(ex.samples.view(np.uint8), full.samples[:root].view(np.uint8))
    for b in range(z):
        plain, small = (full.view(u, bias=b, max_bias=b, draw_small_root=f) for f in (False, True))
        assert np.array_equal(plain.nodes, small.nodes) and np.array_equal(plain.samples, small.samples), b


def test_view_needs_a_full_export(terrain):
    full, box, _ = terrain
    u = view_ref.uniforms_of(box, view_ref.transform_of("closer", box))
    with pytest.raises(ValueError):
        full.view(u, bias=1).view(u)
    with pytest.raises(ValueError):
        full.view(u, bias=3, max_bias=2)
    with pytest.raises(ValueError):
        full.view(u, max_bias=21)
    # max_level truncates the table as simlod_export_octree does, and the selection with it
    ex = full.view(u, max_level=1)
    assert ex.num_nodes == int((full.nodes["level"] <= 1).sum()) and ex.max_level == 1 and not ex.nodes["childMask"][ex.nodes["level"] == 1].any()


def test_abi_matches_the_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodView\) == (\d+)", src).group(1)) == abi.view_dtype.itemsize == 24
    assert int(re.search(r"sizeof\(SimlodViewCounts\) == (\d+)", src).group(1)) == abi.view_counts_dtype.itemsize == 200
    for struct, dtype in (("SimlodView", abi.view_dtype), ("SimlodViewCounts", abi.view_counts_dtype)):
        found = re.findall(rf"offsetof\({struct}, (\w+)\) == (\d+)", src)
        assert len(found) >= 3
        for field, off in found:
            assert dtype.fields[field][1] == int(off), (struct, field)
    assert abi.view_dtype.names == ("flags", "minBias", "maxBias", "reserved", "sampleBudget")
    assert abi.view_counts_dtype.names[:3] == abi.export_counts_dtype.names and abi.view_counts_dtype["samplesAt"].shape == (21,)
    for name, value in (("SIMLOD_VIEW_MAX_BIAS", abi.VIEW_MAX_BIAS), ("SIMLOD_VIEW_NO_CULL", abi.VIEW_NO_CULL),
                        ("SIMLOD_VIEW_DRAW_SMALL_ROOT", abi.VIEW_DRAW_SMALL_ROOT), ("SIMLOD_EXPORT_ERR_BUDGET", abi.EXPORT_ERR_BUDGET)):
        assert int(re.search(rf"#define {name}\s+(0x[0-9a-f]+|\d+)u", src).group(1), 0) == value, name
    assert abi.EXPORT_ERR_BUDGET not in (abi.EXPORT_ERR_CAPACITY, abi.EXPORT_ERR_NODE_COUNT, abi.EXPORT_ERR_SHORT_LIST)
    v = abi.view_record(2, 7, 1000, cull=False, draw_small_root=True)[0]
    assert (int(v["flags"]), int(v["minBias"]), int(v["maxBias"]), int(v["reserved"]), int(v["sampleBudget"])) == (3, 2, 7, 0, 1000)
    assert int(abi.view_record()["sampleBudget"][0]) == 0xFFFFFFFFFFFFFFFF


def test_library_exports_the_view_call_and_refuses_before_device_work(built_libs):
    """Every refusal of simlod_query_view precedes device work: hipErrorInvalidValue (1) without a GPU, the buffers untouched."""
    from simlod_amd import runtime
    L = runtime.lib()
    assert "simlod_query_view" in runtime.EXPORTED_SYMBOLS and hasattr(L, "simlod_query_view")
    box = (1.0, 1.0, 1.0)
    u = np.ascontiguousarray(view_ref.uniforms_of(box, view_ref.transform_of("bird", box))).reshape(1)
    cap = 8
    need = int(L.simlod_export_buffer_min_bytes(cap, 0))
    bufs = {k: np.full(n, 0xA5, np.uint8) for k, n in (("nodes", 152 * cap), ("stats", abi.stats_dtype.itemsize), ("scratch", need), ("table", 40 * cap),
                                                       ("samples", 16 * 8), ("counts", 200))}
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(view=None, uu=u, scratch_bytes=need, null=None):
        g = {k: (None if k == null else b) for k, b in bufs.items()}
        v = abi.view_record() if view is None else view
        return L.simlod_query_view(p(g["nodes"]), p(g["stats"]), p(uu), None if null == "view" else p(v), 20, p(g["scratch"]), ctypes.c_uint64(scratch_bytes),
                                   p(g["table"]), cap, p(g["samples"]), ctypes.c_uint64(8), p(g["counts"]), None)

    for k in ("nodes", "stats", "scratch", "table", "counts", "view"):
        assert call(null=k) == 1, k
    assert call(uu=None) == 1
    assert call(scratch_bytes=need - 1) == 1
    for field, value in (("flags", 4), ("flags", 0x80000000), ("reserved", 1), ("minBias", 21), ("maxBias", 21)):
        v = abi.view_record()
        v[field] = value
        assert call(view=v) == 1, field
    v = abi.view_record(5, 4)
    assert call(view=v) == 1
    for field in ("minNodeSize", "width", "height"):
        for value in (np.nan, np.inf):
            w = u.copy()
            w[field] = value
            assert call(uu=w) == 1, field
    w = u.copy()
    w["transform_updateBound"][0, 3, 2] = -np.inf
    assert call(uu=w) == 1
    assert all((b == 0xA5).all() for b in bufs.values())
