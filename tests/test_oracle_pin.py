"""Pins the C restatement (oracle/simlod_oracle.c) against the reference ITSELF: oracle/_ref = the reference's own
reset.cu / progressive_octree_voxels.cu / render.cu compiled in place as single-thread host code (oracle/Makefile).
A serial run has one legal outcome, so the two must agree on every byte that is not an address: node records, chunk
contents at identical allocator offsets, occupancy grids, Stats, pre-EDL framebuffers.

Every scenario is one `record_*` function, run on a back-end: tests/golden/make_golden_pin.py runs them on the reference
(kind="ref") into tests/golden/oracle_pin.npz; the tests run them on the restatement and compare with that fixture, so
they need neither the reference nor oracle/_ref.  Framebuffers are kept as SHA-256 digests."""
import hashlib
import os

import numpy as np
import pytest

import oracle
import cases
from cases import CASES, batches_of, case, uniforms_for
from util import STATS_BUILD_FIELDS, STATS_RENDER_FIELDS, assert_dumps_equal, assert_stats_equal

NODE_VALUE_FIELDS = ["counter", "numPoints", "level", "X", "Y", "Z", "countIteration", "name", "numVoxels", "numVoxelsStored"]
GOLDEN_PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_pin.npz")
EDGE_VARIANTS = ["odd_size_hqs", "odd_size_plain_boxes", "tiny_frame", "inside_the_cloud_hqs", "inside_the_cloud_plain", "fine_lod_hqs", "boxes_only"]


def _digest(fb):
    return np.frombuffer(hashlib.sha256(fb.tobytes()).digest(), dtype=np.uint8)


def golden(scenario):
    """The reference's record of one scenario (keys "<scenario>__<what>" in tests/golden/oracle_pin.npz)."""
    g = np.load(GOLDEN_PIN)
    return {k.split("__", 1)[1]: g[k] for k in g.files if k.split("__", 1)[0] == scenario}


OFFSET_BOXES = [(name, off) for name in CASES for off in ("dyadic", "inexact")] + [("terrain_4x100k", "georef")]
FROZEN_CASES = [(name, live) for name in ("uniform_3x40k", "terrain_4x100k") for live in cases.LIVE_CAMERAS if not (live == "grazing" and name != "terrain_4x100k")]


def _run(kind, name, offset=None):
    """Build a case on a back-end; with `offset` (a name of cases.offset_of) the points, the box and the camera are moved by it."""
    pts, box, batch, T = case(name)
    if offset is not None:
        off = cases.offset_of(offset, box)
        pts, box_min, box, batch = cases.shifted(name, off)
        u = uniforms_for(box, cases.shifted_cam(box, off), box_min=box_min)
        return _build(kind, name, pts, batch, u), u
    u = uniforms_for(box, T)
    return _build(kind, name, pts, batch, u), box, T


def _build(kind, name, pts, batch, u):
    o = oracle.HostOctree(kind, persistent_bytes=1 << 30, ring_slots=8)
    o.reset(u)
    for b in batches_of(name, pts, batch):
        o.upload(b)
    while int(o.stats["batchletIndex"][0]) < int(o.num_uploaded[0]):
        o.construct(u)
    return o


def _with(u, **fields):
    v = np.array(u, copy=True)
    for k, val in fields.items():
        v[k] = val
    return v


def record_build(kind, name, offset=None):
    if offset is None:
        o, box, T = _run(kind, name)
        frame_uniforms = lambda hqs: uniforms_for(box, T, hqs=hqs)
    else:
        o, u0 = _run(kind, name, offset)
        frame_uniforms = lambda hqs: _with(u0, useHighQualityShading=int(hqs))
    n = int(o.stats["numNodes"][0])
    rec = {"stats": o.stats.copy(), "dump": o.dump()}                # the dump: every stored point, voxel position and grid bit
    for f in NODE_VALUE_FIELDS:
        rec[f"node_{f}"] = o.nodes[f][:n].copy()
    # same allocation order -> same offsets inside the persistent buffer for grids and chunk lists
    for f in ("grid", "points", "voxelChunks"):
        rec[f"offset_{f}"] = np.where(o.nodes[f][:n] != 0, o.nodes[f][:n] - np.uint64(o.persistent.ctypes.data), 0)
    rec["children"] = np.where(o.nodes["children"][:n] != 0, o.nodes["children"][:n] - np.uint64(o.nodes.ctypes.data), 0)
    for hqs in (False, True):
        fb, _ = o.render(frame_uniforms(hqs))
        rec[f"fb_{int(hqs)}"], rec[f"render_stats_{int(hqs)}"], rec[f"visible_{int(hqs)}"] = _digest(fb), o.stats.copy(), o.visible["name"].copy()
        if offset is not None and not hqs:
            from simlod_amd import abi
            rec["nonbg"] = np.array([int((fb != abi.CLEAR_PIXEL).sum())])
    return o, rec


def record_offset_box(kind, name, offset):
    """record_build with the case's points, box and camera moved by a named offset (cases.offset_of): boxMin != 0."""
    return record_build(kind, name, offset)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_reference_build(built_libs, name):
    _check_build(name, *record_build("port", name), golden(f"build_{name}"))


@pytest.mark.parametrize("name,offset", OFFSET_BOXES)
def test_restatement_equals_reference_build_in_a_box_off_the_origin(built_libs, name, offset):
    """The build and the two frames with boxMin != 0 (the reference's kernels honour it; its host never sends it).  Guards: the fixture's
    frame draws something, and the same points in the box [0, boxMax] give another octree — so a `min` that is dropped somewhere shows."""
    port, got = record_offset_box("port", name, offset)
    want = golden(f"offset_{offset}_{name}")
    _check_build(f"{name}/{offset}", port, got, want)
    assert int(want["nonbg"][0])  > 200                   # (the hotspot is one level-3 cell: some 350 pixels)
    assert np.array_equal(want["nonbg"], got["nonbg"])
    _, u = _run("port", name, offset)
    if offset == "inexact":
        assert cases.size_differs(u), "the inexact offset must make (boxMin + size) - boxMin differ from size"
    pts = cases.shifted(name, cases.offset_of(offset, case(name)[1]))[0]
    ignoring = _build("port", name, pts, case(name)[2], cases.origin_box_uniforms(u)).dump()
    assert len(ignoring) != len(got["dump"]) or any(not np.array_equal(ignoring[f], got["dump"][f]) for f in ("key", "numPoints", "gridHash", "voxelPosSum"))


def _check_build(name, port, got, want):
    assert port.last_error() == 0
    assert_stats_equal(got["stats"][0], want["stats"][0], STATS_BUILD_FIELDS, name)
    for f in NODE_VALUE_FIELDS:
        assert np.array_equal(want[f"node_{f}"], got[f"node_{f}"]), f"Node.{f}"
    for f in ("grid", "points", "voxelChunks"):
        assert np.array_equal(want[f"offset_{f}"], got[f"offset_{f}"]), f"Node.{f} offsets"
    assert np.array_equal(want["children"], got["children"]), "children indices"
    assert_dumps_equal(got["dump"], want["dump"], name)
    for hqs in (0, 1):
        assert np.array_equal(want[f"fb_{hqs}"], got[f"fb_{hqs}"]), f"{name}: pre-EDL framebuffer differs (hqs={hqs})"
        assert_stats_equal(got[f"render_stats_{hqs}"][0], want[f"render_stats_{hqs}"][0], STATS_RENDER_FIELDS, name)
        va, vb = want[f"visible_{hqs}"], got[f"visible_{hqs}"]
        assert len(va) == len(vb) and np.array_equal(va, vb), "visible-node list order"


_FROZEN_BUILT = {}


def record_frozen_camera(kind, name, live):
    """Frames of a case whose nodes are chosen by one camera (transform_updateBound: frustum test, `large`, render.cu:792-861, 1025-1053) and
    drawn by another (transform), plain / HQS x node boxes off / on.  minNodeSize is 64 on the terrain, where the two cameras then cut its 33
    nodes at different depths, and 16 on uniform_3x40k, whose 9 nodes leave nothing to cut: there the cameras differ in the frustum test
    only.  Also, for the tests' guards: the non-background pixels of the frame, in how many pixels it differs from the (live, live) and the
    (frozen, frozen) frame, and numVisibleNodes of (live, live)."""
    if (kind, name) not in _FROZEN_BUILT:
        _FROZEN_BUILT.clear()
        _FROZEN_BUILT[(kind, name)] = _run(kind, name)
    from simlod_amd import abi
    o, box, _ = _FROZEN_BUILT[(kind, name)]
    Tl, Tf = cases.frozen_pair(live, box, cases.W, cases.H)
    rec = {}
    for hqs in (0, 1):
        for boxes in (0, 1):
            mk = lambda t, tu: abi.make_uniforms(cases.W, cases.H, t, box, transform_update_bound=tu, persistent_capacity=1 << 30, momentary_capacity=300_000_000,
                                                 hqs=bool(hqs), min_node_size=64.0 if "terrain" in name else 16.0, show_bounding_box=bool(boxes))
            fb = o.render(mk(Tl, Tf))[0]
            st, vis = o.stats.copy(), o.visible["name"].copy()
            fb_ll = o.render(mk(Tl, Tl))[0]
            n_ll = int(o.stats["numVisibleNodes"][0])
            fb_ff = o.render(mk(Tf, Tf))[0]
            k = f"{hqs}{boxes}"
            rec[f"fb_{k}"], rec[f"stats_{k}"], rec[f"visible_{k}"] = _digest(fb), st, vis
            rec[f"guard_{k}"] = np.array([int((fb != abi.CLEAR_PIXEL).sum()), int((fb != fb_ll).sum()), int((fb != fb_ff).sum()), n_ll])
    return rec


@pytest.mark.parametrize("name,live", FROZEN_CASES)
def test_frozen_visibility_camera_matches_reference(built_libs, name, live):
    """transform_updateBound != transform: the restatement against the reference's own render.cu.  Guards, from the fixture alone: the frame
    differs from the frame of (frozen, frozen) and — on the terrain — of (live, live); `away` draws nothing but still lists the frozen
    camera's nodes, where (live, live) lists none; on uniform_3x40k (every node drawn by either camera) the cameras with another frustum
    list another number of nodes than (live, live) does."""
    got, want = record_frozen_camera("port", name, live), golden(f"frozen_{name}_{live}")
    for k in ("00", "01", "10", "11"):
        assert np.array_equal(want[f"fb_{k}"], got[f"fb_{k}"]), f"{name}/{live}: pre-EDL framebuffer differs (hqs, boxes = {k})"
        assert_stats_equal(got[f"stats_{k}"][0], want[f"stats_{k}"][0], STATS_RENDER_FIELDS, f"{name}/{live}/{k}")
        assert np.array_equal(want[f"visible_{k}"], got[f"visible_{k}"]), "visible-node list order"
        assert np.array_equal(want[f"guard_{k}"], got[f"guard_{k}"])
        nonbg, d_live, d_frozen, n_live = (int(v) for v in want[f"guard_{k}"])
        assert d_frozen > 0
        if live == "away":                                              # (its debug lines lie behind the live camera; (live, live) sees its own frustum)
            assert (nonbg == 0 or k[1] == "1") and n_live == 0 and int(want[f"stats_{k}"]["numVisibleNodes"][0]) > 0
        elif "terrain" in name or k[1] == "1":                          # (with the lines on, the frozen frustum itself is on screen)
            assert d_live > 0 and nonbg > 500, (nonbg, d_live)
        else:
            assert nonbg > 500 and (live not in ("inside",) or n_live != int(want[f"stats_{k}"]["numVisibleNodes"][0]))


def record_modes(kind):
    """Frames of uniform_3x40k in the point-size, debug-line and colour modes, in this order; -> (frames, digests)."""
    o, box, T = _run(kind, "uniform_3x40k")
    frames = []
    for ps in (2, 3):
        frames.append((("point_size", ps), o.render(uniforms_for(box, T, point_size=ps))[0]))
    for hqs in (0, 1):                      # debug lines: node boxes + frustum, rasterization.cuh:90-183
        u = uniforms_for(box, T, hqs=bool(hqs))
        u["showBoundingBox"] = 1
        frames.append((("showBoundingBox", hqs), o.render(u)[0]))
    for field in ("colorByNode", "colorByLOD"):
        u = uniforms_for(box, T)
        u[field] = 1
        for hqs in (0, 1):
            u["useHighQualityShading"] = hqs
            frames.append(((field, hqs), o.render(u)[0]))
    return frames, {"fb": np.stack([_digest(fb) for _, fb in frames])}


def test_point_size_and_color_modes_match_reference(built_libs):
    frames, got = record_modes("port")
    want = golden("modes")["fb"]
    assert len(want) == len(frames)
    for (what, fb), a, b in zip(frames, want, got["fb"]):
        assert np.array_equal(a, b), what
        if what[0] == "showBoundingBox":
            assert int(((fb & np.uint64(0xffffffff)) == np.uint64(0xff00)).sum()) > 500


def record_hazards(kind):
    from simlod_amd import camera, synthetic
    rs = np.random.RandomState(4)
    base, box = synthetic.uniform_cube(20_000, seed=9)
    same = np.repeat(base[:1], 70_000)
    same["x"], same["y"], same["z"] = np.float32(0.3), np.float32(0.6), np.float32(0.2)
    corners = np.repeat(base[:1], 4_000)
    for k in "xyz":
        corners[k] = rs.choice(np.array([0.0, 1.0], dtype=np.float32), 4_000)
    pts = np.concatenate([base[:10_000], same, corners, base[10_000:]])
    T = camera.lookat_transform((1.8, -1.2, 1.4), (0.5, 0.5, 0.3), 256, 256)
    u = uniforms_for(box, T)
    o = oracle.HostOctree(kind, persistent_bytes=1 << 30, ring_slots=4)
    o.reset(u)
    o.add_points(u, pts, 50_000)
    rec = {"stats": o.stats.copy(), "dump": o.dump()}
    rec["fb"] = _digest(o.render(u)[0])
    return o, rec


def test_hazard_regimes_match_reference(built_libs):
    """Where the reference is lossy the restatement must be lossy in the same way (the HIP path documents where it is not):
    20 split rounds down to level 20 with 70 000 identical points (the reference does not count after its 20th split, allocates no
    chunks for the level-20 leaf, increments its numPoints and drops the points, voxels.cu:394-412, 599-604 — the restatement
    reports that as NULL_CHUNK), and points exactly on the box faces (coordinate == boxMax quantises to 2^20, wraps into the low
    child, voxels.cu:148-179)."""
    from simlod_amd import abi
    port, got = record_hazards("port")
    want = golden("hazards")
    assert port.last_error() == 5                                   # ORACLE_ERR_NULL_CHUNK
    assert_stats_equal(got["stats"][0], want["stats"][0], STATS_BUILD_FIELDS, "hazards")
    assert int(want["stats"]["numNodes"][0]) == 1 + 8 * 20 and int(want["dump"]["level"].max()) == abi.MAX_DEPTH
    assert_dumps_equal(got["dump"], want["dump"], "hazards")
    assert np.array_equal(want["fb"], got["fb"])


def record_edge_case(kind, variant):
    from simlod_amd import abi, camera, synthetic
    Wd, Hd = (250, 131) if "odd_size" in variant else (40, 23) if variant == "tiny_frame" else (384, 256)
    pts, box = synthetic.uniform_cube(300_000, seed=77)
    if "inside" in variant:
        eye, target = (0.52, 0.48, 0.5), (0.9, 0.6, 0.45)
    else:
        eye, target = (1.8, -1.2, 1.4), (0.5, 0.5, 0.3)
    T = camera.lookat_transform(eye, target, Wd, Hd)
    u = abi.make_uniforms(Wd, Hd, T, box, persistent_capacity=1 << 30, momentary_capacity=300_000_000, hqs="hqs" in variant)
    u["showBoundingBox"] = 1 if "boxes" in variant else 0
    u["showPoints"] = 0 if variant == "boxes_only" else 1
    if variant == "fine_lod_hqs" or "odd_size" in variant:
        u["minNodeSize"] = 8.0
    if variant == "tiny_frame":
        u["minNodeSize"] = 2.0
    o = oracle.HostOctree(kind, persistent_bytes=1 << 30, ring_slots=4)
    o.reset(u)
    o.add_points(u, pts, 100_000)
    fb = o.render(u)[0]
    return fb, {"fb": _digest(fb), "stats": o.stats.copy(), "visible": o.visible["name"].copy(), "nonbg": np.array([int((fb != abi.CLEAR_PIXEL).sum())])}


@pytest.mark.parametrize("variant", EDGE_VARIANTS)
def test_render_edge_cases_match_reference(built_libs, variant):
    """The render edge cases of the GPU suite (tests/test_gpu_parity.py: frame sizes off the 16-pixel grid, camera inside the cloud,
    fine LOD threshold, lines without points), restatement against the reference's own render.cu on a reference-built octree."""
    _, got = record_edge_case("port", variant)
    want = golden(f"edge_{variant}")
    assert np.array_equal(want["fb"], got["fb"]), variant
    assert_stats_equal(got["stats"][0], want["stats"][0], STATS_RENDER_FIELDS, variant)
    assert np.array_equal(want["visible"], got["visible"])
    assert int(want["nonbg"][0]) > 50


def test_edl_restatement_matches_the_reference_edl_block():
    """EDL (render.cu:1255-1325) pinned to the reference itself: tests/golden/edl_uniform_3x40k.npz was minted by running the
    reference's own render.cu with its EDL pass enabled, one in-tile thread per call (tests/golden/make_golden_edl.py).  The
    restatement's EDL'd RGBA8 image must agree within 1 per channel (log2 / exp come from different libms) on every full 16x16 tile.
    The last row is left out: there the reference reads the depth of pixel W*H — one past the framebuffer (render.cu:1303)."""
    import os
    from cases import H, W, batches_of, case, uniforms_for
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "edl_uniform_3x40k.npz"))
    pts, box, batch, T = case("uniform_3x40k")
    u = uniforms_for(box, T)
    o = oracle.HostOctree("port", persistent_bytes=1 << 28, ring_slots=8)
    o.reset(u)
    for b in batches_of("uniform_3x40k", pts, batch):
        o.upload(b)
    while int(o.stats["batchletIndex"][0]) < int(o.num_uploaded[0]):
        o.construct(u)
    rows = np.arange(W * H) // W
    cmp = rows < H - 1
    for mode, hqs in (("plain", False), ("hqs", True)):
        fb, col = o.render(uniforms_for(box, T, hqs=hqs), edl=True)
        want = G[f"color_{mode}"]
        d = np.abs(col.view(np.uint8).astype(np.int16) - want.view(np.uint8).astype(np.int16)).reshape(-1, 4).max(axis=1)
        assert int(d[cmp].max()) <= 1, f"{mode}: {int((d[cmp] > 1).sum())} pixels differ by more than 1 from the reference's EDL output"
        assert int((want & 0xffffff != (fb & 0xffffff).astype(np.uint32)).sum()) > 1000, "the fixture must actually be shaded"
