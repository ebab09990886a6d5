"""GPU tier: a frozen visibility camera (Uniforms.transform_updateBound != Uniforms.transform).  The reference separates the camera that
CHOOSES the nodes (frustum test, `large`, the LOD cut: render.cu:792-861, 1025-1053 — frozen when its GUI's "Update Visibility" is off) from
the camera that DRAWS them; the frustum's debug lines exist to look at the frozen frustum from elsewhere.  render.hip keeps the two matrices
apart on purpose, and the frozen case is where the rasteriser's fast paths meet inputs they were not tuned on: a coarse cut drawn large
(boxes of many tiles, screen bins), visible nodes wholly off the live screen (an empty tile box), nodes behind the live camera only.

One frozen camera (the suite's bird camera) chooses, the live cameras of tests/cases.py draw; `narrow` and `grazing_back` choose with another
camera (cases.frozen_pair).  Every frame: bit-identical to the oracle's on the same downloaded image, render Stats equal, RGBA8 within 1, the
buffer's next three frames identical.  Guards, from the oracle alone: the frame differs from the oracle's (live, live) and (frozen, frozen)
frames and draws more than the suite's floor of 2000 pixels; `away` is all clear by construction and is guarded by its Stats instead."""
import numpy as np
import pytest

import cases
from simlod_amd import abi, synthetic
from test_gpu_parity import _device, _ingest
from util import assert_frame_equals_oracle, host_image_of, node_keys, oracle_frame

pytestmark = pytest.mark.gpu
SIZES = {"uniform": (384, 256), "terrain": (1000, 562)}
FLOOR = 2000
_BUILT = {}


def _octree(kind, **knobs):
    """(device, box, host image) of uniform 1 M / terrain 1.5 M (the octrees of the render edge cases), built once; with knobs, a device of its own."""
    key = (kind,) + tuple(sorted(knobs.items()))
    if key not in _BUILT:
        for k in [k for k in _BUILT if k[0] != kind]:
            del _BUILT[k]
        if kind == "uniform":
            pts, box = synthetic.uniform_cube(1_000_000, seed=77)
        else:
            pts, box = synthetic.terrain(1_500_000, seed=3, box=(600.0, 400.0, 40.0), tile=50.0)
        dev = _device(ring_slots=2)
        for k, v in knobs.items():
            dev.tune(k, v)
        Wd, Hd = SIZES[kind]
        u = dev.uniforms(Wd, Hd, np.eye(4, dtype=np.float32), box)
        _ingest(dev, u, [pts[i:i + 1_000_000] for i in range(0, len(pts), 1_000_000)])
        assert int(dev.read_stats()["dbg"]) == 0
        _BUILT[key] = (dev, box) + host_image_of(dev)
    return _BUILT[key]


def _uniforms(dev, kind, case, box, *, hqs=False, boxes=False, point_size=1, min_node_size=64.0, live=None, frozen=None):
    Wd, Hd = SIZES[kind]
    Tl, Tf = cases.frozen_pair(case, box, Wd, Hd)
    return dev.uniforms(Wd, Hd, Tl if live is None else live, box, transform_update_bound=Tf if frozen is None else frozen, hqs=hqs,
                        show_bounding_box=boxes, point_size=point_size, min_node_size=min_node_size), Tl, Tf


def _check(kind, case, what, knobs=None, **kw):
    dev, box, nodes, pers, nn = _octree(kind, **(knobs or {}))
    Wd, Hd = SIZES[kind]
    u, Tl, Tf = _uniforms(dev, kind, case, box, **kw)
    assert not np.array_equal(u["transform"], u["transform_updateBound"])
    dev.render(u)
    fb_dev, col_dev, st, vis = assert_frame_equals_oracle(dev, nodes, nn, u, what, None)
    binned = dev.samples_binned(Wd, Hd)
    for _ in range(3):                      # the buffer's next frames (bin feedback: from the third on the first frame's finding decides)
        dev.render(u)
        assert np.array_equal(dev.framebuffer(Wd, Hd), fb_dev) and np.array_equal(dev.color(Wd, Hd), col_dev), f"{what}: a later frame differs"
        binned = max(binned, dev.samples_binned(Wd, Hd))        # (whether a frame sorts into the bins follows what the buffer's earlier frames found)
    # guards against vacuity, from the oracle alone
    fb_ll, _, st_ll, _ = oracle_frame(nodes, nn, _uniforms(dev, kind, case, box, **dict(kw, frozen=Tl))[0])
    fb_ff, _, st_ff, _ = oracle_frame(nodes, nn, _uniforms(dev, kind, case, box, **dict(kw, live=Tf))[0])
    nonbg = int((fb_dev != abi.CLEAR_PIXEL).sum())
    print(f"{what}: {int(st['numVisibleNodes'])} visible nodes (live camera alone {int(st_ll['numVisibleNodes'])}), {nonbg} pixels drawn, "
          f"{int((fb_dev != fb_ll).sum())} differ from (live, live), {int((fb_dev != fb_ff).sum())} from (frozen, frozen), {binned} samples binned")
    assert int(st["numVisibleNodes"]) == int(st_ff["numVisibleNodes"]) > 0, "the frozen camera chooses"
    assert not np.array_equal(fb_dev, fb_ff)
    if case == "away":
        assert int(st_ll["numVisibleNodes"]) == 0 and (kw.get("boxes") or nonbg == 0)
    elif case == "grazing_back" and not kw.get("boxes"):
        # (nearly the unfrozen cut by construction: the five nodes it adds lie off the live screen, so the guard is on Stats, as for `away`)
        assert int(st["numVisibleNodes"]) != int(st_ll["numVisibleNodes"]) and nonbg > FLOOR
    else:
        assert not np.array_equal(fb_dev, fb_ll) and nonbg > FLOOR
    return binned, st, vis


CASES = [(kind, case) for kind in ("uniform", "terrain") for case in cases.LIVE_CAMERAS + ["grazing_back"] if kind == "terrain" or "grazing" not in case]


@pytest.mark.parametrize("boxes", [False, True], ids=["points", "boxes"])
@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("kind,case", CASES)
def test_frozen_camera_frames_bit_exact(built_libs, kind, case, hqs, boxes):
    _check(kind, case, f"{kind} {case} hqs={int(hqs)} boxes={int(boxes)}", hqs=hqs, boxes=boxes)


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("kind", ["uniform", "terrain"])
@pytest.mark.parametrize("case", ["closer", "panned"])
def test_frozen_camera_point_size_2(built_libs, kind, case, hqs):
    _check(kind, case, f"{kind} {case} pointSize 2 hqs={int(hqs)}", hqs=hqs, point_size=2)


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("kind", ["uniform", "terrain"])
@pytest.mark.parametrize("case", ["closer", "narrow"])
def test_frozen_camera_fine_cut(built_libs, kind, case, hqs):
    """minNodeSize 16: the cut is every nonempty node of these octrees (64 and 54), not a dozen.  Both cameras then choose the same nodes, so
    the frames are drawn with the lines on: the frozen frustum's lines are what differs from the (live, live) frame."""
    _, st, _ = _check(kind, case, f"{kind} {case} minNodeSize 16 hqs={int(hqs)}", hqs=hqs, min_node_size=16.0, boxes=True)
    assert int(st["numVisibleNodes"]) >= 50


@pytest.mark.parametrize("knob", ["no_bins", "small_pool"])
@pytest.mark.parametrize("case", ["grazing", "grazing_back"])
def test_frozen_camera_grazing_without_bins_and_with_a_small_pool(built_libs, case, knob):
    knobs = {"SIMLOD_RASTER_SCREEN_BINS": 0} if knob == "no_bins" else {"SIMLOD_DEBUG_BIN_POOL": 20_000}
    binned, _, _ = _check("terrain", case, f"terrain {case} {knob}", knobs=knobs, hqs=True)
    assert binned == 0 if knob == "no_bins" else 0 < binned <= 20_000, binned


def test_a_frozen_case_reaches_the_screen_bins(built_libs):
    """The screen bins (render.hip r_overflow) must be reached with the two matrices apart.  The bird camera's dozen coarse nodes drawn by the
    skimming camera do reach them (tens of thousands of samples); `grazing_back` is kept beside it: the grazing camera draws what the same camera moved
    30 m back chose — nearly the unfrozen cut, but every node's `large` / frustum decision and its tile box come from different matrices."""
    binned_bird, _, _ = _check("terrain", "grazing", "terrain grazing hqs (bins)", hqs=True)
    binned_back, _, _ = _check("terrain", "grazing_back", "terrain grazing_back hqs (bins)", hqs=True)
    print(f"samples binned: frozen bird camera {binned_bird}, frozen grazing_back camera {binned_back}")
    assert max(binned_bird, binned_back) > 0, (binned_bird, binned_back)


def test_a_frozen_frame_in_parts_equals_the_whole_frame(built_libs):
    """The frame's parts (simlod_render_frame_composed with reductions that change nothing: one rank) under a frozen camera, closer / HQS."""
    for kind in ("uniform", "terrain"):
        dev, box, nodes, pers, nn = _octree(kind)
        Wd, Hd = SIZES[kind]
        u, _, _ = _uniforms(dev, kind, "closer", box, hqs=True)
        dev.render(u)
        fb, col = dev.framebuffer(Wd, Hd), dev.color(Wd, Hd)
        assert int((fb != abi.CLEAR_PIXEL).sum()) > FLOOR
        dev.render_buffer.fill_(0xA5)
        calls = []
        dev.render_composed(u, reduce=lambda plane, *a: calls.append(plane) or 0)
        assert calls == [0, 1]
        assert np.array_equal(dev.framebuffer(Wd, Hd), fb) and np.array_equal(dev.color(Wd, Hd), col)


@pytest.mark.parametrize("case", ["panned", "closer", "away", "narrow"])
def test_export_visible_after_a_frozen_frame_lists_the_frozen_cameras_nodes(built_libs, case):
    dev, box, nodes, pers, nn = _octree("terrain")
    u, Tl, Tf = _uniforms(dev, "terrain", case, box)
    dev.render(u)
    ex = dev.export_octree(u, select="visible")
    sel = ex.nodes[(ex.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0]
    _, _, st, vis = oracle_frame(nodes, nn, u)
    _, _, _, vis_ff = oracle_frame(nodes, nn, _uniforms(dev, "terrain", case, box, live=Tf)[0])
    _, _, _, vis_ll = oracle_frame(nodes, nn, _uniforms(dev, "terrain", case, box, frozen=Tl)[0])
    assert len(vis) > 0 and np.array_equal(np.sort(node_keys(sel)), np.sort(node_keys(vis)))
    assert np.array_equal(np.sort(node_keys(vis)), np.sort(node_keys(vis_ff))), "the visible set is the frozen camera's"
    assert not np.array_equal(np.sort(node_keys(vis)), np.sort(node_keys(vis_ll))), "and not the live camera's"
    assert int(ex.nodes["numSamples"].sum()) == int(st["numVisiblePoints"]) + int(st["numVisibleVoxels"])
