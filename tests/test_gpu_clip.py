"""GPU tier: clip regions (include/simlod_hip.h, "clip regions") — DeviceOctree.set_clip, then the ordinary frame calls — against the mirror of
tests/clip_ref.py: the oracle's own rasteriser on the downloaded image edited by rule C3's table.  Every clipped frame: dbg == 0, render Stats
equal, pre-EDL framebuffer bit-identical, RGBA8 within 1, the buffer's next three frames identical; and, from the oracle alone, the frame differs
from the unclipped oracle frame and draws more than 2000 pixels unless the case says otherwise.

The octrees are the two of tests/test_gpu_frozen_camera.py (uniform 1 M at 384 x 256, terrain 1.5 M at 1000 x 562), built once; a mirror is made
once per (octree, region, mode) and shared by every camera and shading mode that looks at it."""
import ctypes

import numpy as np
import pytest

import cases
import clip_ref
import region_ref
import util
from simlod_amd import abi, camera
from simlod_amd.octree_io import Clip
from test_gpu_frozen_camera import SIZES, _octree
from util import assert_frame_equals_oracle, node_keys, oracle_frame

pytestmark = pytest.mark.gpu
FLOOR = 2000
COLOUR = 0x00FF20E0                     # the highlight colour word: no sample of the synthetic inputs carries it
MODES = ["inside", "outside", "highlight"]
_MIRRORS, _UNCLIPPED = {}, {}


def _uniforms(dev, kind, case, box, *, frozen=False, live=None, **kw):
    Wd, Hd = SIZES[kind]
    if frozen:
        Tl, Tf = cases.frozen_pair(case, box, Wd, Hd)
        kw["transform_update_bound"] = Tf
    else:
        Tl = camera.lookat_transform(*cases.camera_pose(case, box), Wd, Hd)
    return dev.uniforms(Wd, Hd, Tl if live is None else live, box, **kw)


def _forget_other_octrees(cache, tag):
    """`tag` names a built octree (its kind first, then its knobs); _octree keeps the builds of one kind at a time, and so do the caches."""
    for k in [k for k in cache if k[0][0] != tag[0] and {k[0][0], tag[0]} == {"uniform", "terrain"}]:
        del cache[k]


def _mirror(tag, region_kind, mode, nodes, pers, nn, clip, u):
    """The edited image of (octree, region, mode): made once.  Only the box of `u` goes into it."""
    key = (tag, region_kind, mode)
    if key not in _MIRRORS:
        _forget_other_octrees(_MIRRORS, tag)
        _MIRRORS[key] = clip_ref.clip_image(nodes, pers, nn, clip, u)
    return _MIRRORS[key]


def _unclipped(tag, nodes, nn, u):
    """The oracle's frame of the unedited image of octree `tag` under `u`: made once."""
    key = (tag, np.ascontiguousarray(u).tobytes())
    if key not in _UNCLIPPED:
        _forget_other_octrees(_UNCLIPPED, tag)
        _UNCLIPPED[key] = oracle_frame(nodes, nn, u)
    return _UNCLIPPED[key]


def _tag(kind, knobs=None):
    return (kind,) + tuple(sorted((knobs or {}).items()))


def _clipped_frame(dev, tag, nodes, pers, nn, u, clip, region_kind, what, floor=FLOOR, differs=True, render=None):
    """One clipped frame and everything every clipped-frame check asserts.  -> (mirror, device fb, oracle Stats, oracle visible records)"""
    Wd, Hd = int(u["width"]), int(u["height"])
    img = _mirror(tag, region_kind, clip.mode, nodes, pers, nn, clip, u)
    render = render or dev.render
    dev.set_clip(clip)
    try:
        render(u)
        fb_dev, col_dev, st, vis = assert_frame_equals_oracle(dev, img.nodes, nn, u, what, floor)
        for _ in range(3):
            render(u)
            assert np.array_equal(dev.framebuffer(Wd, Hd), fb_dev) and np.array_equal(dev.color(Wd, Hd), col_dev), f"{what}: a later frame differs"
        assert int(dev.read_stats()["dbg"]) == 0
    finally:
        dev.set_clip(None)
    fb_un, _, st_un, _ = _unclipped(tag, nodes, nn, u)
    nonbg = int((fb_dev != abi.CLEAR_PIXEL).sum())
    print(f"{what}: {int(st['numVisibleNodes'])} visible nodes (unclipped {int(st_un['numVisibleNodes'])}), {int(img.emptied.sum())} emptied, {nonbg} pixels drawn, "
          f"{int((fb_dev != fb_un).sum())} differ from the unclipped frame")
    if differs:
        assert not np.array_equal(fb_dev, fb_un), f"{what}: the clip must change the frame"
    return img, fb_dev, st, vis


def _check(kind, case, region_kind, mode, what, knobs=None, floor=FLOOR, differs=True, parts=False, **kw):
    dev, box, nodes, pers, nn = _octree(kind, **(knobs or {}))
    u = _uniforms(dev, kind, case, box, **kw)
    clip = Clip(region_ref.region(region_kind, box), mode, COLOUR)
    render = (lambda uu: dev.render_composed(uu, reduce=lambda plane, *a: 0)) if parts else None
    return (dev, u, clip) + _clipped_frame(dev, _tag(kind, knobs), nodes, pers, nn, u, clip, region_kind, what, floor, differs, render)


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
FRAMES = [(kind, case, region_kind, mode, hqs) for kind, case in (("uniform", "closer"), ("terrain", "closer"), ("terrain", "grazing"))
          for region_kind in ("oblique", "box") for mode in MODES for hqs in (False, True)]


@pytest.mark.parametrize("kind,case,region_kind,mode,hqs", FRAMES, ids=[f"{k}-{c}-{r}-{m}-{'hqs' if h else 'plain'}" for k, c, r, m, h in FRAMES])
def test_clipped_frames_bit_exact(built_libs, kind, case, region_kind, mode, hqs):
    dev, u, clip, img, fb, st, vis = _check(kind, case, region_kind, mode, f"{kind} {case} {region_kind} {mode} hqs={int(hqs)}", hqs=hqs)
    if region_kind == "oblique":
        # the UNCLIPPED visible list holds a node of each class: every row of rule C3's table is at work in these frames
        _, _, nodes, pers, nn = _octree(kind)
        vis_un = _unclipped(_tag(kind), nodes, nn, u)[3]
        cls = clip_ref.node_classes(vis_un, len(vis_un), clip.region, u)
        counts = [int((cls == c).sum()) for c in (clip_ref.OUTSIDE, clip_ref.COPIED, clip_ref.FILTERED)]
        print(f"unclipped visible list: {counts[0]} outside / {counts[1]} copied / {counts[2]} filtered of {len(vis_un)}")
        assert min(counts) >= 1, counts


# ---- degenerate regions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("region_kind,mode", [("none", "inside"), ("miss", "outside")])
def test_a_clip_that_removes_nothing_is_the_unclipped_frame(built_libs, region_kind, mode, hqs):
    dev, u, clip, img, fb, st, vis = _check("terrain", "closer", region_kind, mode, f"terrain closer {region_kind} {mode} hqs={int(hqs)}", differs=False, hqs=hqs)
    _, _, nodes, pers, nn = _octree("terrain")
    fb_un, _, st_un, _ = _unclipped(_tag("terrain"), nodes, nn, u)
    assert np.array_equal(fb, fb_un) and not img.emptied.any() and not img.tested
    util.assert_stats_equal(st, st_un, util.STATS_RENDER_FIELDS)


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("region_kind,mode", [("none", "outside"), ("miss", "inside")])
def test_a_clip_that_removes_everything_is_a_clear_frame(built_libs, region_kind, mode, hqs):
    dev, u, clip, img, fb, st, vis = _check("terrain", "closer", region_kind, mode, f"terrain closer {region_kind} {mode} hqs={int(hqs)}", floor=None, hqs=hqs)
    assert (fb == abi.CLEAR_PIXEL).all() and int(st["numVisibleNodes"]) == 0 and len(vis) == 0


@pytest.mark.parametrize("override", ["color_by_node", "color_by_lod"])
@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
def test_colour_overrides_win_over_highlight(built_libs, override, hqs):
    """Rule C4: with colorByNode or colorByLOD set, a HIGHLIGHT frame is the unclipped frame."""
    dev, box, nodes, pers, nn = _octree("terrain")
    u = _uniforms(dev, "terrain", "closer", box, hqs=hqs, **{override: True})
    dev.set_clip(Clip(region_ref.region("oblique", box), "highlight", COLOUR))
    try:
        dev.render(u)
        fb, _, _, _ = assert_frame_equals_oracle(dev, nodes, nn, u, f"highlight under {override}", FLOOR)
    finally:
        dev.set_clip(None)
    assert not np.array_equal(fb, _unclipped(_tag("terrain"), nodes, nn, _uniforms(dev, "terrain", "closer", box, hqs=hqs))[0]), "the override must show"


def test_off_again(built_libs):
    """After set_clip(None), and after a clip of mode "off", the frame is the oracle's on the unedited image."""
    dev, box, nodes, pers, nn = _octree("terrain")
    u = _uniforms(dev, "terrain", "closer", box)
    region = region_ref.region("oblique", box)
    for off in (None, Clip(region, "off", COLOUR)):
        dev.set_clip(Clip(region, "inside"))
        dev.render(u)
        clipped = dev.framebuffer(*SIZES["terrain"])
        dev.set_clip(off)
        dev.render(u)
        fb, _, _, _ = assert_frame_equals_oracle(dev, nodes, nn, u, f"off again ({'None' if off is None else 'mode off'})", FLOOR)
        assert not np.array_equal(fb, clipped)
    dev.set_clip(None)


# ---- every draw path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_clip_in_the_screen_bins(built_libs, mode):
    """terrain grazing, HQS: the frame sorts samples into the screen bins (bin_item tests a sample before it becomes a bin entry)."""
    dev, u, clip, *_ = _check("terrain", "grazing", "oblique", mode, f"terrain grazing oblique {mode} (bins)", hqs=True)
    dev.set_clip(clip)
    try:
        binned = 0
        for _ in range(3):                      # (whether a frame sorts follows what the buffer's earlier frames found)
            dev.render(u)
            binned = max(binned, dev.samples_binned(*SIZES["terrain"]))
    finally:
        dev.set_clip(None)
    assert binned > 0


@pytest.mark.parametrize("knob", ["no_bins", "small_pool"])
@pytest.mark.parametrize("mode", ["inside", "highlight"])
def test_clip_without_bins_and_with_a_small_pool(built_libs, mode, knob):
    knobs = {"SIMLOD_RASTER_SCREEN_BINS": 0} if knob == "no_bins" else {"SIMLOD_DEBUG_BIN_POOL": 20_000}
    dev, u, clip, *_ = _check("terrain", "grazing", "oblique", mode, f"terrain grazing oblique {mode} {knob}", knobs=knobs, hqs=True)
    dev.set_clip(clip)
    try:
        binned = 0
        for _ in range(3):
            dev.render(u)
            binned = max(binned, dev.samples_binned(*SIZES["terrain"]))
    finally:
        dev.set_clip(None)
    assert binned == 0 if knob == "no_bins" else 0 < binned <= 20_000, binned


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("mode", MODES)
def test_clip_with_point_size_2(built_libs, mode, hqs):
    """pointSize 2: every sample goes through draw_sample."""
    _check("terrain", "closer", "oblique", mode, f"terrain closer oblique {mode} pointSize 2 hqs={int(hqs)}", hqs=hqs, point_size=2)


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("mode", MODES)
def test_clip_from_inside_the_box(built_libs, mode, hqs):
    """The `inside` camera: nodes reach behind the camera and their items have no tile (with the screen bins off: every sample of such an item
    takes the global path).  The region is the box: the camera stands inside it and looks out through its x = 70 % face, so every mode changes
    the frame (the oblique half-space holds everything this camera sees)."""
    dev, u, clip, *_ = _check("terrain", "inside", "box", mode, f"terrain inside box {mode} hqs={int(hqs)}", knobs={"SIMLOD_RASTER_SCREEN_BINS": 0}, hqs=hqs)
    dev.set_clip(clip)
    try:
        dev.render(u)
        items = dev.draw_items(*SIZES["terrain"])
    finally:
        dev.set_clip(None)
    assert int(((items["tileX"] == -1) & (items["samples"] > 0)).sum()) > 0, "no item without a tile"


def _far_back(box, factor):
    """The `closer` camera's line of sight, `factor` times as far from its target."""
    eye, target = (np.asarray(v) for v in cases.camera_pose("closer", box))
    return tuple(target + factor * (eye - target)), tuple(target)


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("mode", MODES)
def test_clip_on_tiles_of_a_few_pixels(built_libs, mode, hqs):
    """draw_wave runs for items whose tile holds at most 64 pixels — a node at most 4 pixels across, with the tile's margin: the `closer` camera
    chooses its 48 nodes and a camera 20 times as far back on the same line of sight draws them.  Such a frame is small by construction (the
    CPU oracle draws 246 pixels unclipped, 133 / 130 inside / outside the oblique half): the floor is 100 pixels here."""
    dev, box, nodes, pers, nn = _octree("terrain")
    Wd, Hd = SIZES["terrain"]
    chooser = camera.lookat_transform(*cases.camera_pose("closer", box), Wd, Hd)
    live = camera.lookat_transform(*_far_back(box, 20.0), Wd, Hd)
    dev, u, clip, *_ = _check("terrain", "closer", "oblique", mode, f"terrain far back oblique {mode} hqs={int(hqs)}", floor=100, live=live,
                              transform_update_bound=chooser, hqs=hqs)
    dev.set_clip(clip)
    try:
        dev.render(u)
        items = dev.draw_items(Wd, Hd)
    finally:
        dev.set_clip(None)
    area = items["tileW"].astype(np.int64) * items["tileH"].astype(np.int64)
    small = (items["tileX"] >= 0) & (area <= 64) & (items["samples"] > 0)
    print(f"{int(small.sum())} of {len(items)} items have a tile of at most 64 pixels")
    assert int(small.sum()) > 0


# ---- edges of the frame ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("mode", ["inside", "outside"])
def test_bounding_boxes_only_for_nodes_the_clip_left_visible(built_libs, mode, hqs):
    dev, u, clip, img, fb, st, vis = _check("terrain", "closer", "oblique", mode, f"terrain closer oblique {mode} boxes hqs={int(hqs)}", hqs=hqs, show_bounding_box=True)
    _, _, nodes, pers, nn = _octree("terrain")
    assert int(st["numVisibleNodes"]) < int(_unclipped(_tag("terrain"), nodes, nn, u)[2]["numVisibleNodes"])


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("mode", MODES)
def test_clip_under_a_frozen_camera(built_libs, mode, hqs):
    dev, u, *_ = _check("terrain", "closer", "oblique", mode, f"terrain closer (frozen) oblique {mode} hqs={int(hqs)}", frozen=True, hqs=hqs)
    assert not np.array_equal(u["transform"], u["transform_updateBound"])


@pytest.mark.parametrize("mode", MODES)
def test_clip_in_a_box_off_the_origin(built_libs, mode):
    """terrain_4x100k at cases.GEOREF, the region placed relative to boxMin."""
    if "georef" not in _GEOREF:
        dev, u, pts, box = util._build("terrain_4x100k", cases.GEOREF)
        _GEOREF["georef"] = (dev, u, box) + util.host_image_of(dev)
    dev, u, box, nodes, pers, nn = _GEOREF["georef"]
    box_min = np.asarray(u["boxMin"].tolist(), np.float64).reshape(3)
    clip = Clip(region_ref.region("oblique", box, box_min), mode, COLOUR)
    img, *_ = _clipped_frame(dev, _tag("georef"), nodes, pers, nn, u, clip, "oblique", f"terrain_4x100k georef oblique {mode}")
    assert img.tested and (mode == "highlight" or img.emptied.any()), "the region must filter some nodes of this octree and empty others"


_GEOREF = {}


@pytest.mark.parametrize("mode", MODES)
def test_a_clipped_frame_in_parts_equals_the_whole_frame(built_libs, mode):
    """render_composed with a reduce that changes nothing (one rank): every part reads the context's clip."""
    _check("terrain", "closer", "oblique", mode, f"terrain closer oblique {mode} in parts", parts=True, hqs=True)


# ---- composition -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["inside", "outside"])
def test_export_visible_follows_the_clip(built_libs, mode):
    dev, u, clip, img, fb, st, vis = _check("terrain", "closer", "oblique", mode, f"terrain closer oblique {mode} (export)")
    dev.set_clip(clip)
    try:
        dev.render(u)
        ex = dev.export_octree(u, select="visible")
    finally:
        dev.set_clip(None)
    sel = ex.nodes[(ex.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0]
    _, _, nodes, pers, nn = _octree("terrain")
    vis_un = _unclipped(_tag("terrain"), nodes, nn, u)[3]
    assert 0 < len(vis) < len(vis_un) and np.array_equal(np.sort(node_keys(sel)), np.sort(node_keys(vis)))


def test_a_clip_on_one_context_leaves_another_octrees_frame_unclipped(built_libs):
    dev, box, nodes, pers, nn = _octree("terrain")
    other, u2, _, box2 = util._build("uniform_3x40k")
    nodes2, pers2, nn2 = util.host_image_of(other)
    dev.set_clip(Clip(region_ref.region("oblique", box), "inside"))
    try:
        other.render(u2)
        assert_frame_equals_oracle(other, nodes2, nn2, u2, "the other octree's frame", FLOOR)
        # ... and the other way round: the other octree's clip is not this one's
        dev.set_clip(None)
        other.set_clip(Clip(region_ref.region("oblique", box2), "outside"))
        u = _uniforms(dev, "terrain", "closer", box)
        dev.render(u)
        assert_frame_equals_oracle(dev, nodes, nn, u, "this octree's frame", FLOOR)
        other.render(u2)
        img = clip_ref.clip_image(nodes2, pers2, nn2, Clip(region_ref.region("oblique", box2), "outside"), u2)
        fb, _, _, _ = assert_frame_equals_oracle(other, img.nodes, nn2, u2, "the other octree's clipped frame", FLOOR)
        assert not np.array_equal(fb, oracle_frame(nodes2, nn2, u2)[0])
    finally:
        dev.set_clip(None)
        other.set_clip(None)
        other.close()


def test_bad_arguments_leave_the_clip_as_it_was(built_libs):
    """A mode above 3, 17 planes, a non-finite coefficient, a nonzero reserved word in either struct: hipErrorInvalidValue, and the next frame is
    the one the context's clip asked for before the call."""
    dev, box, nodes, pers, nn = _octree("terrain")
    u = _uniforms(dev, "terrain", "closer", box)
    clip = Clip(region_ref.region("oblique", box), "inside")
    img = _mirror(_tag("terrain"), "oblique", "inside", nodes, pers, nn, clip, u)
    good = clip.record()
    dev.set_clip(clip)
    try:
        for edit in ("mode", "planes", "nan", "inf", "clip_reserved", "region_reserved"):
            r = good.copy()
            if edit == "mode":
                r["mode"] = 4
            elif edit == "planes":
                r["region"]["numPlanes"] = 17
            elif edit == "nan":
                r["region"]["planes"][0, 0, 1] = np.nan
            elif edit == "inf":
                r["region"]["planes"][0, 0, 3] = -np.inf
            elif edit == "clip_reserved":
                r["reserved"][0, 1] = 1
            else:
                r["region"]["reserved"][0, 0] = 1
            assert dev.L.simlod_context_set_clip(dev.ctx, ctypes.c_void_p(r.ctypes.data)) == 1, edit
            dev.render(u)
            assert_frame_equals_oracle(dev, img.nodes, nn, u, f"after a refused clip ({edit})", FLOOR)
    finally:
        dev.set_clip(None)
