"""GPU tier: an octree whose box does not start at the origin (Uniforms.boxMin != 0).  The reference's kernels honour boxMin everywhere, its
host always sends 0; this library is an ABI for other hosts, and every kernel family reads boxMin: the builder's quantisation and voxel
centres, the node boxes of the frame, the debug lines, the colour filter, the grid rebuild of the buildable import, the plane geometry of
region queries, the projected node rectangles of footprint queries.  Here the whole chain runs on shifted inputs (tests/cases.py: dyadic, inexact, georef) against the oracle on the same inputs /
the same downloaded image, by the comparisons of the suites for the origin box.  Every case that builds on small inputs also shows that it
can tell "honours boxMin" from "ignores it": the oracle, given the same points in the box [0, boxMax], builds another octree."""
import numpy as np
import pytest

import cases
import footprint_ref as fr
import oracle
import region_ref as rr
import test_gpu_footprint as on_footprints
from export_ref import export_host
from simlod_amd import abi, camera, synthetic
from simlod_amd.octree_io import OctreeExport, Region
from test_gpu_export import _assert_export, _variants
from test_gpu_groups import _drive
from test_gpu_parity import GRANULARITY_FREE_FIELDS, GRANULARITY_FREE_STATS, _device, _ingest
from test_gpu_region import COUNT_FIELDS, Raw, _assert_matches
from test_gpu_resume import RESUME_FIELDS, _assert_fields, _assert_stats, _check_import, _continuous, _feed
from util import (STATS_BUILD_FIELDS, assert_dumps_equal, assert_frame_equals_oracle, assert_stats_equal, assert_voxel_winners, batch_of_points,
                  host_image_of, points_multiset_hash, replay_first_hits, tag_colors)

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
SMALL = [(name, off) for name in cases.CASES for off in ("dyadic", "inexact")] + [("terrain_4x100k", "georef")]
TERRAIN_BOX = (600.0, 400.0, 40.0)
_ORACLES = {}


def _box_min(offset):
    return tuple(float(np.float32(v)) for v in offset)


def _oracle_build(key, u, batches):
    """The port oracle's build of `batches`, once per input."""
    if key not in _ORACLES:
        _ORACLES.clear()                    # (one at a time: an oracle holds a gigabyte)
        ref = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=abi.BATCH_STREAM_SIZE)
        ref.reset(u)
        for b in batches:
            ref.upload(b)
            ref.construct(u)
        assert ref.last_error() == 0 and int(ref.stats["batchletIndex"][0]) == len(batches)
        _ORACLES[key] = ref
    return _ORACLES[key]


def _differs(a, b):
    return len(a) != len(b) or any(not np.array_equal(a[f], b[f]) for f in ("key", "numPoints", "gridHash", "voxelPosSum"))


# ---- build -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", SMALL)
def test_construct_in_a_box_off_the_origin_matches_oracle(built_libs, name, offset):
    off = cases.offset_of(offset, cases.case(name)[1])
    pts, box_min, box, batch = cases.shifted(name, off)
    batches = cases.batches_of(name, pts, batch)
    dev = _device(ring_slots=8)
    u = dev.uniforms(W, H, cases.shifted_cam(box, off), box, box_min=box_min)
    assert tuple(u["boxMin"].tolist()) == box_min and (pts["x"] >= u["boxMin"][0]).all() and (pts["x"] <= u["boxMax"][0]).all()
    if offset == "inexact":
        assert cases.size_differs(u), "the inexact offset must make (boxMin + size) - boxMin differ from size"
    _ingest(dev, u, batches)
    ref = _oracle_build((name, offset), u, batches)
    ds = dev.read_stats()
    assert int(ds["dbg"]) == 0, f"device error bits {int(ds['dbg']):#x}"
    assert_stats_equal(ds, ref.stats[0], STATS_BUILD_FIELDS, f"{name}@{offset}")
    nodes, pers, nn = host_image_of(dev)
    assert_dumps_equal(oracle.dump_image(nodes, nn), ref.dump(), f"{name}@{offset}")
    oracle.check_invariants(nodes, nn)
    # guard: the same points in the box [0, boxMax] are another octree
    ign = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=abi.BATCH_STREAM_SIZE)
    v = cases.origin_box_uniforms(u)
    ign.reset(v)
    for b in batches:
        ign.upload(b)
        ign.construct(v)
    assert _differs(ign.dump(), ref.dump())


def _big_input(kind, offset):
    if kind == "terrain":
        pts, box = synthetic.terrain(3_000_000, seed=3, box=TERRAIN_BOX, tile=50.0)
        batch = 1_000_000
    else:
        pts, box = synthetic.hotspot(1_200_000, seed=11, level=4, cell=(5, 9, 6))
        batch = 400_000
    off = cases.offset_of(offset, box)
    pts = cases.shift_points(pts, off)
    return pts, box, off, [pts[i:i + batch] for i in range(0, len(pts), batch)]


@pytest.mark.parametrize("mode", ["default", "exact_group_1", "coalesced"])
@pytest.mark.parametrize("kind,offset", [("terrain", "inexact"), ("terrain", "georef"), ("hotspot", "inexact")])
def test_multi_batch_ingest_in_a_box_off_the_origin(built_libs, kind, offset, mode):
    """Sizes at which the multi-batch paths run, in the three ingest modes: default exact groups and SIMLOD_EXACT_GROUP=1 give every Node and
    Stats field of the oracle, coalesced mode the content that does not depend on the batch granularity."""
    pts, box, off, batches = _big_input(kind, offset)
    dev = _device(ring_slots=abi.BATCH_STREAM_SIZE, coalesce=mode == "coalesced", **({"momentary_bytes": 400_000_000} if mode == "coalesced" else {}))
    if mode == "exact_group_1":
        dev.tune("SIMLOD_EXACT_GROUP", 1)
    Wd, Hd = 640, 360
    if kind == "hotspot":                   # the close camera of the suite's hotspot frames: the level-4 cell fills the frame
        c = (np.array([5, 9, 6], dtype=np.float64) + 0.5) / 16.0
        eye, target = c + 0.09 * np.array([1.4, -1.1, 0.9]) + np.asarray(off), c + np.asarray(off)
    else:
        eye, target = cases.camera_pose("bird", box, off)
    u = dev.uniforms(Wd, Hd, camera.lookat_transform(tuple(eye), tuple(target), Wd, Hd), box, box_min=_box_min(off))
    dev.reset(u)
    for b in batches:                       # all pending at once: a launch takes them as groups (or, coalesced, as one batch)
        dev.upload(b)
    dev.drain(u)
    ref = _oracle_build((kind, offset), u, batches)
    ds = dev.read_stats()
    assert int(ds["dbg"]) == 0, f"device error bits {int(ds['dbg']):#x}"
    nodes, pers, nn = host_image_of(dev)
    got, want = oracle.dump_image(nodes, nn), ref.dump()
    assert int(want["level"].max()) >= 3
    if mode == "coalesced":
        assert_stats_equal(ds, ref.stats[0], GRANULARITY_FREE_STATS, kind)
        assert len(got) == len(want)
        for f in GRANULARITY_FREE_FIELDS:
            assert np.array_equal(got[f], want[f]), f
    else:
        assert_stats_equal(ds, ref.stats[0], STATS_BUILD_FIELDS, kind)
        assert_dumps_equal(got, want, f"{kind}@{offset} {mode}")
    oracle.check_invariants(nodes, nn)
    u["useHighQualityShading"] = 1
    dev.render(u)
    assert_frame_equals_oracle(dev, nodes, nn, u, f"{kind}@{offset} {mode}", 2000)


def test_voxel_winners_in_a_box_off_the_origin(built_libs):
    """Which point coloured each voxel (tagged colours, util.assert_voxel_winners): the cell arithmetic of the check goes through
    oracle.voxel_cells(uniforms, ...) and gets the shifted uniforms — with the origin box every winner would lie outside its voxel's node."""
    name, off = "terrain_4x100k", cases.GEOREF
    pts, box_min, box, batch = cases.shifted(name, off)
    batches = cases.batches_of(name, tag_colors(pts), batch)
    tagged = np.concatenate(batches)
    dev = _device(ring_slots=8)
    dev.tune("SIMLOD_EXACT_GROUP", 1)
    u = dev.uniforms(W, H, cases.shifted_cam(box, off), box, box_min=box_min)
    ref, fh = replay_first_hits(u, batches)
    ends, taken, sizes = _drive(dev, u, batches, 1)
    assert ends and ends[-1] == len(batches)
    ds = dev.read_stats()
    assert int(ds["dbg"]) == 0
    assert_stats_equal(ds, ref.stats[0], STATS_BUILD_FIELDS, name)
    nodes, pers, nn = host_image_of(dev)
    assert_dumps_equal(oracle.dump_image(nodes, nn), ref.dump(), name)
    checked = assert_voxel_winners(nodes, nn, tagged, batch_of_points(batches), fh, lambda b: b, u)
    assert checked == int(nodes["numVoxelsStored"][:nn].sum()) > 0
    with pytest.raises(AssertionError, match="outside the voxel's"):
        assert_voxel_winners(nodes, nn, tagged, batch_of_points(batches), fh, lambda b: b, cases.origin_box_uniforms(u))


# ---- render ------------------------------------------------------------------------------------------------------------------------------------
_BUILT = {}


def _render_octree(kind, offset):
    """(device, uniforms' box arguments, host image) of a device-built shifted octree, once per (kind, offset)."""
    if (kind, offset) not in _BUILT:
        _BUILT.clear()
        if kind == "uniform":
            pts, box = synthetic.uniform_cube(1_000_000, seed=1234)
        else:
            pts, box = synthetic.terrain(1_500_000, seed=3, box=TERRAIN_BOX, tile=50.0)
        off = cases.offset_of(offset, box)
        pts = cases.shift_points(pts, off)
        dev = _device(ring_slots=2)
        u = dev.uniforms(W, H, cases.shifted_cam(box, off), box, box_min=_box_min(off))
        _ingest(dev, u, [pts[i:i + 1_000_000] for i in range(0, len(pts), 1_000_000)])
        assert int(dev.read_stats()["dbg"]) == 0
        _BUILT[(kind, offset)] = (dev, box, off) + host_image_of(dev)
    return _BUILT[(kind, offset)]


@pytest.mark.parametrize("variant", ["plain", "hqs", "hqs_ps2", "plain_boxes", "by_node"])
@pytest.mark.parametrize("kind,offset", [("uniform", "inexact"), ("uniform", "dyadic"), ("terrain", "georef"), ("terrain", "inexact")])
def test_render_in_a_box_off_the_origin_bit_exact(built_libs, kind, offset, variant):
    """The suite's camera translated by the offset: pre-EDL frame bit-identical to the oracle's on the downloaded image, render Stats equal,
    RGBA8 within 1.  The node boxes (min + X * nodeSize) decide visibility and the lines; the guard frame shows that boxMin matters to both."""
    dev, box, off, nodes, pers, nn = _render_octree(kind, offset)
    Wd, Hd = (512, 512) if kind == "uniform" else (640, 360)
    eye, target = cases.camera_pose("bird", box, off)
    u = dev.uniforms(Wd, Hd, camera.lookat_transform(eye, target, Wd, Hd), box, box_min=_box_min(off), hqs="hqs" in variant,
                     point_size=2 if "ps2" in variant else 1, color_by_node="by_node" in variant, show_bounding_box="boxes" in variant)
    dev.render(u)
    fb_dev, _, st, _ = assert_frame_equals_oracle(dev, nodes, nn, u, f"{kind}@{offset} {variant}", 10_000 if kind == "uniform" else 2000)   # (the suite's floors: 512^2 cube / edge cases)
    dev.render(u)                           # a frame is a pure function of (image, uniforms)
    assert np.array_equal(dev.framebuffer(Wd, Hd), fb_dev)
    from util import oracle_frame
    fb_ign, _, st_ign, _ = oracle_frame(nodes, nn, cases.origin_box_uniforms(u))
    assert not np.array_equal(fb_ign, fb_dev), "with boxMin ignored the oracle draws another frame: the case can tell"


@pytest.mark.parametrize("offset,variant", [("inexact", "grazing_hqs"), ("inexact", "grazing_plain"), ("dyadic", "grazing_hqs"), ("georef", "inside_hqs"),
                                            ("georef", "inside_plain_boxes"), ("inexact", "inside_hqs"), ("inexact", "inside_plain_boxes")])
def test_render_edge_cameras_on_the_shifted_terrain(built_libs, offset, variant):
    """The skimming camera (leaves much larger on screen than an LDS tile: the screen bins) and a camera inside the cloud (w <= 0), both
    translated by the offset.  (No skimming camera at the georef offset: an fp32 world-view-projection matrix with translations of 4e6 cannot
    place an eye 6 m above the ground — the oracle finds no node visible there.)"""
    dev, box, off, nodes, pers, nn = _render_octree("terrain", offset)
    Wd, Hd = (1000, 562) if "grazing" in variant else (384, 256)
    eye, target = cases.camera_pose("grazing" if "grazing" in variant else "inside", box, off)
    u = dev.uniforms(Wd, Hd, camera.lookat_transform(eye, target, Wd, Hd), box, box_min=_box_min(off), hqs="hqs" in variant, show_bounding_box="boxes" in variant)
    dev.render(u)
    fb_dev, col_dev, _, _ = assert_frame_equals_oracle(dev, nodes, nn, u, f"terrain@{offset} {variant}", 2000)
    if "grazing" in variant:
        binned = dev.samples_binned(Wd, Hd)
        for _ in range(3):                  # the buffer's next frames: whether a frame sorts into the bins follows what the frames before it found
            dev.render(u)                   # (this buffer's earlier frames, of other cameras, found no node for them)
            assert np.array_equal(dev.framebuffer(Wd, Hd), fb_dev) and np.array_equal(dev.color(Wd, Hd), col_dev)
            binned = max(binned, dev.samples_binned(Wd, Hd))
        assert binned > 0, binned


# ---- colour filter -----------------------------------------------------------------------------------------------------------------------------
def _rows(v):
    return np.sort(np.ascontiguousarray(v).view(np.dtype((np.void, 16))).reshape(-1))


def _filter_octants(nodes, i, u):
    """colorfilter.cu:58-161, 312-357 restated in numpy for node i of a HOST-addressed image: per child octant, in octant order, the voxels the
    filter makes of the child's samples (its points and its voxels) — one per first-hit cell of the 64^3 sample grid, at the cell centre, with the
    average colour.  The filter finds the cell from 2^24 * (p - boxMin) / octreeSize with octreeSize = (boxMin + cubeSize) - boxMin PER AXIS (:75-79),
    the builder from ... / cubeSize: where the two differ in fp32 a node can have more or fewer first hits than voxels."""
    f32 = np.float32
    mn, mx = np.asarray(u["boxMin"], f32).reshape(3), np.asarray(u["boxMax"], f32).reshape(3)
    cube = (mx - mn).max()
    osz = (mn + cube) - mn
    nd = nodes[i]
    L = int(nd["level"])
    node_size = cube / f32(2.0 ** L)
    node_min = np.array([nd["X"], nd["Y"], nd["Z"]], dtype=f32) * node_size + mn
    out = []
    for k in range(8):
        ptr = int(nd["children"][k])
        if ptr == 0:
            continue
        ch = nodes[(ptr - nodes.ctypes.data) // abi.node_dtype.itemsize]
        smp = np.concatenate([oracle.gather_samples(int(ch["points"]), int(ch["numPoints"])) if ch["numPoints"] else np.zeros(0, abi.point_dtype),
                              oracle.gather_samples(int(ch["voxelChunks"]), int(ch["numVoxels"])) if ch["numVoxels"] else np.zeros(0, abi.point_dtype)])
        c = [((((f32(16777216.0) * (smp[a] - mn[j])) / osz[j]).astype(np.int64).astype(np.uint32) >> np.uint32(17 - L)) % np.uint32(64)).astype(f32) for j, a in enumerate("xyz")]
        vi = np.minimum((c[0] + c[1] * f32(64.0) + c[2] * f32(4096.0)).astype(np.int64), 64 ** 3 - 1)
        cells, inv, cnt = np.unique(vi, return_inverse=True, return_counts=True)
        assert cnt.max(initial=0) < 1024, "a cell's 10-bit count overflows: undefined in the reference"
        col = smp["color"].astype(np.int64)
        avg = [(np.bincount(inv, weights=(col >> sh) & 255, minlength=len(cells)).astype(np.int64) // cnt) & 255 for sh in (0, 8, 16)]
        v = np.zeros(len(cells), dtype=abi.point_dtype)
        p = [((k >> 2) & 1) * 64 + cells % 64, ((k >> 1) & 1) * 64 + (cells % 4096) // 64, (k & 1) * 64 + cells // 4096]
        for j, a in enumerate("xyz"):
            v[a] = node_min[j] + (node_size * (p[j].astype(f32) + f32(0.5))) / f32(128.0)
        v["color"] = (avg[0] | (avg[1] << 8) | (avg[2] << 16)).astype(np.uint32)
        out.append(v)
    return out


def _assert_filtered_like_the_restatement(nodes, nn, before, u, what):
    """Every inner node of a filtered image against _filter_octants of ITS OWN children (a node is filtered after them): octant by octant the
    node's voxel slots hold that octant's voxels — all of them as a multiset where they fit, else distinct ones of them (which ones is the
    order of first hits: serial in the reference, scheduling dependent on the device); slots behind the last first hit keep the voxel the
    builder put there.  -> {node index: True where first hits == voxels for the node and every inner node below it}."""
    clean = {}
    order = np.argsort(-nodes["level"][:nn].astype(np.int64), kind="stable")
    for i in (int(k) for k in order):
        nd = nodes[i]
        kids = [int(pk) for pk in nd["children"] if pk]
        if not kids:
            continue
        nv = int(nd["numVoxelsStored"])
        assert nv == int(nd["numVoxels"])
        got = oracle.gather_samples(int(nd["voxelChunks"]), nv) if nv else np.zeros(0, abi.point_dtype)
        at = 0
        for v in _filter_octants(nodes, i, u):
            seg = got[at: min(at + len(v), nv)]
            if at + len(v) <= nv:
                assert np.array_equal(_rows(seg), _rows(v)), f"{what}: node {i} (level {int(nd['level'])}): an octant's voxels are not the restatement's"
            else:
                r = _rows(seg)
                assert len(np.unique(r)) == len(r) and np.isin(r, _rows(v)).all(), f"{what}: node {i} (level {int(nd['level'])}): voxels outside the octant's first hits"
            at += len(v)
        if at < nv:
            assert got[at:].tobytes() == before[i][at:].tobytes(), f"{what}: node {i}: a voxel behind the last first hit was touched"
        clean[i] = at == nv and all(clean.get((pk - nodes.ctypes.data) // abi.node_dtype.itemsize, True) for pk in kids)
    return clean


@pytest.mark.parametrize("offset", ["inexact", "dyadic"])
@pytest.mark.parametrize("kind,n", [("uniform", 1_000_000), ("terrain", 3_000_000)])
def test_colorfilter_in_a_box_off_the_origin_equals_the_reference_kernel(built_libs, kind, n, offset):
    """simlod_launch_colorfilter against colorfilter.cu itself (oracle/_ref/libref_filter.so) on the same shifted image.

    dyadic offset: octreeSize == cubeSize, the filter finds the builder's cells, and per inner node the voxels and averaged colours are the
    reference kernel's as multisets, as at the origin.

    inexact offsets: octreeSize = (boxMin + cubeSize) - boxMin differs from cubeSize on the y axis (asserted), the filter's cells are not
    the builder's, and most nodes get a few more or fewer first hits than they have voxels (observed: uniform 1 M, the eight level-1 nodes
    121 258 for 121 259 voxels ... 121 770 for 121 769, the root 794 836 for 794 833).  The reference only reports that (colorfilter.cu:387-395) and
    writes the surplus voxels past the node's list; which first hits fall behind the list is their order — serial there, scheduling dependent
    here, where they are dropped — so the two images cannot be compared as whole multisets.  Compared instead, on both images: every inner node
    against the numpy restatement of the reference's arithmetic applied to the node's own children (_assert_filtered_like_the_restatement), and
    device against reference kernel as multisets on every node where first hits == voxels at and below the node."""
    if not oracle.have_ref_filter():
        pytest.skip("oracle/_ref/libref_filter.so was not built (no reference checkout where the snapshot was made)")
    pts, box = synthetic.uniform_cube(n, seed=41) if kind == "uniform" else synthetic.terrain(n, seed=6, box=TERRAIN_BOX, tile=50.0)
    off = cases.offset_of(offset, box)
    pts = cases.shift_points(pts, off)
    dev = _device(ring_slots=4)
    u = dev.uniforms(W, H, cases.shifted_cam(box, off), box, box_min=_box_min(off))
    assert cases.size_differs(u) == (offset == "inexact")
    _ingest(dev, u, [pts[i:i + abi.MAX_BATCH_SIZE] for i in range(0, n, abi.MAX_BATCH_SIZE)])
    nodes_0, pers_0, nn = host_image_of(dev)                      # the image as built ...
    before = {i: oracle.gather_samples(int(nodes_0[i]["voxelChunks"]), int(nodes_0[i]["numVoxelsStored"])) for i in range(nn) if nodes_0[i]["numVoxelsStored"]}
    nodes_a, pers_a, _ = host_image_of(dev)
    oracle.ref_colorfilter(nodes_a, nn, u)                        # ... filtered by the reference's own kernel on the host
    dev.colorfilter(u)                                            # ... and by the HIP kernels on the device
    nodes_b, pers_b, nn_b = host_image_of(dev)
    assert nn == nn_b and int(dev.read_stats()["dbg"]) == 0
    assert np.array_equal(nodes_a["isFiltered"][:nn], nodes_b["isFiltered"][:nn])
    assert np.array_equal(nodes_a["numVoxelsStored"][:nn], nodes_b["numVoxelsStored"][:nn]) and np.array_equal(nodes_a["numPoints"][:nn], nodes_b["numPoints"][:nn])
    clean_a = _assert_filtered_like_the_restatement(nodes_a, nn, before, u, "reference kernel")
    clean_b = _assert_filtered_like_the_restatement(nodes_b, nn, before, u, "device")
    assert len(clean_b) >= (1 if kind == "uniform" else 20)
    same = changed = 0
    for i in clean_b:
        if not (clean_a[i] and clean_b[i]):
            continue
        nv = int(nodes_a[i]["numVoxelsStored"])
        va, vb = oracle.gather_samples(int(nodes_a[i]["voxelChunks"]), nv), oracle.gather_samples(int(nodes_b[i]["voxelChunks"]), nv)
        assert np.array_equal(_rows(va), _rows(vb)), f"node {i} (level {int(nodes_a[i]['level'])}): filtered voxels differ from the reference kernel's"
        same += 1
        changed += int(not np.array_equal(np.sort(before[i]["color"]), np.sort(vb["color"])))
    print(f"{kind}@{offset}: {len(clean_b)} inner nodes, {same} with first hits == voxels at and below them (reference kernel: {sum(clean_a.values())})")
    if offset == "dyadic":
        assert same == len(clean_b) and changed > 0, "octreeSize == cubeSize: every node is the reference kernel's, and colours were rewritten"
    else:
        assert sum(clean_b.values()) < len(clean_b), "the inexact offset must move some cell of the filter off the builder's"
    d = oracle.dump_image(nodes_b, nn)
    hs, hx = points_multiset_hash(pts)
    with np.errstate(over="ignore"):
        assert hs == np.uint64(d["pointsSum"].sum()) and hx == np.bitwise_xor.reduce(d["pointsXor"]), "the filter must not touch the points"
    dev.render(u)                                                 # and the octree is still drawable
    assert int((dev.framebuffer(W, H) != abi.CLEAR_PIXEL).sum()) > 1000


# ---- export / import / resume ------------------------------------------------------------------------------------------------------------------
def _resume_input(name):
    """-> (points, box, offset, batches, cut): the first `cut` batches are built before the export"""
    if name == "terrain_georef":
        pts, box = synthetic.terrain(1_500_000, seed=3, box=TERRAIN_BOX, tile=50.0)
        off, batch, cut = cases.GEOREF, 250_000, 3
    elif name == "hotspot_inexact":
        pts, box = synthetic.hotspot(1_200_000, seed=32, level=1, cell=(1, 0, 0))
        off, batch, cut = cases.INEXACT_UNIT, 200_000, 2
    elif name == "root_leaf_inexact":       # the root is a leaf at the export (its voxels are rebuilt at the cell centres) and splits after the resume
        pts, box = synthetic.terrain(90_000, seed=33, box=(300.0, 200.0, 20.0), tile=50.0)
        off, batch, cut = cases.INEXACT_TERRAIN, 15_000, 2
    else:
        raise KeyError(name)
    pts = cases.shift_points(pts, off)
    return pts, box, off, [pts[i:i + batch] for i in range(0, len(pts), batch)], cut


@pytest.mark.parametrize("name", ["terrain_georef", "hotspot_inexact", "root_leaf_inexact"])
def test_export_import_and_resume_in_a_box_off_the_origin(built_libs, tmp_path, name):
    from simlod_amd.runtime import SimlodError
    pts, box, off, batches, cut = _resume_input(name)
    src = _device(persistent_bytes=2 << 30)
    u = src.uniforms(W, H, cases.shifted_cam(box, off), box, box_min=_box_min(off))
    src.reset(u)
    _feed(src, u, batches[:cut])
    assert int(src.read_stats()["dbg"]) == 0
    # the export is the host restatement's of the same image, and carries the box
    nodes, pers, nn = host_image_of(src)
    t, s = export_host(nodes, nn)
    ex = src.export_octree(u)
    _assert_export(ex, t, s, name)
    assert ex.box_min == _box_min(off) and ex.box_max == tuple(np.asarray(u["boxMax"], np.float32).tolist())
    ex.save(tmp_path / "shifted.simlodx")
    ld = OctreeExport.load(tmp_path / "shifted.simlodx")
    assert ld.is_buildable and ld.box_min == ex.box_min and ld.box_max == ex.box_max
    # a plain import into a fresh object draws the source's frames bit for bit (and they are the oracle's)
    view = _device(persistent_bytes=2 << 30)
    view.import_octree(ld)
    for vname, v in _variants(u):
        src.render(v)
        fb_s, _, _, _ = assert_frame_equals_oracle(src, nodes, nn, v, f"{name} {vname}", 1000)
        view.render(v)
        # (a root that is still a leaf draws its voxels too, which the export does not carry: that frame is compared after the buildable
        # import below, which makes them anew)
        if ex.nodes[0]["childMask"] != 0:
            assert np.array_equal(view.framebuffer(W, H), fb_s) and np.array_equal(view.color(W, H), src.color(W, H)), f"{name} {vname}: the imported octree draws another frame"
    del view
    # the same export with the origin box of the same size: the realistic mistake, refused by the rebuilt grids
    if ex.nodes[0]["childMask"] != 0:
        wrong = src.uniforms(W, H, cases.shifted_cam(box, off), box)
        assert np.array_equal(np.asarray(wrong["boxMax"]) - np.asarray(wrong["boxMin"]), np.asarray(box, np.float32))
        with pytest.raises(SimlodError, match="SIMLOD_ERR_IMPORT_GRID"):        # (an export that names the wrong box itself passes the host's check)
            _device(persistent_bytes=2 << 30).import_octree(OctreeExport(ex.nodes, ex.samples, wrong["boxMin"], wrong["boxMax"]), buildable=True, uniforms=wrong)
    with pytest.raises(SimlodError, match="is not the export's"):
        _device(persistent_bytes=2 << 30).import_octree(ld, buildable=True, uniforms=src.uniforms(W, H, cases.shifted_cam(box, off), box))
    # buildable import with the right box: the grids are resume_ref's, then the remaining batches give the continuous build node for node
    dst = _device(persistent_bytes=2 << 30)
    dst.nodes.fill_(0xA5)
    uu = dst.uniforms(W, H, u["transform"], box, box_min=_box_min(off))
    assert uu["boxMin"].tobytes() == u["boxMin"].tobytes() and uu["boxMax"].tobytes() == u["boxMax"].tobytes()
    dst.import_octree(ld, buildable=True, uniforms=uu)
    _check_import(src, dst, ex, uu, name)
    del src
    _feed(dst, uu, batches[cut:])
    ref = _continuous(uu, batches)
    nodes, pers, n = host_image_of(dst)
    _assert_fields(oracle.dump_image(nodes, n), ref.dump(), RESUME_FIELDS, f"{name} (resume vs continuous)")
    oracle.check_invariants(nodes, n)
    st = dst.read_stats()
    _assert_stats(st, ref.stats[0], name)
    assert int(st["dbg"]) == 0 and int(st["batchletIndex"]) == len(batches) - cut


# ---- region queries ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", [("uniform_3x40k", "inexact"), ("terrain_4x100k", "georef"), ("hotspot_150k", "dyadic"), ("terrain_4x100k", "inexact")])
def test_query_region_in_a_box_off_the_origin(built_libs, name, offset):
    """simlod_query_region on shifted octrees: byte-equal to the host mirror OctreeExport.crop (one level cut and full depth), multiset-equal to
    the brute-force filter of the input, the count-only call consistent.  Regions are placed relative to the shifted box."""
    off = cases.offset_of(offset, cases.case(name)[1])
    pts, box_min, box, batch = cases.shifted(name, off)
    dev = _device(persistent_bytes=2 << 30)
    u = dev.uniforms(W, H, cases.shifted_cam(box, off), box, box_min=box_min)
    dev.reset(u)
    _feed(dev, u, cases.batches_of(name, pts, batch))
    assert int(dev.read_stats()["dbg"]) == 0
    full = dev.export_octree(u)
    assert full.box_min == box_min
    for kind in ("oblique", "slab", "box", "miss"):
        r = rr.region(kind, box, box_min)
        inside = rr.brute_mask(r, pts)
        if kind == "miss":
            assert not inside.any()
        else:
            assert inside.any() and (not inside.all() or "hotspot" in name), "the region must cut the cloud"
        for sel, ml in (("cut", 20), ("cut", 2), ("all", 20)):
            mirror, cnt = full.crop(r, ml, sel, return_counts=True)
            _assert_matches(Raw(dev, u, r, ml, sel), mirror, cnt, f"{name}@{offset} {kind} {sel}@{ml}")
        ex, c = dev.query_region(u, r, return_counts=True)
        mirror, cnt = full.crop(r, 20, "cut", return_counts=True)
        assert ex.nodes.tobytes() == mirror.nodes.tobytes() and ex.samples.tobytes() == mirror.samples.tobytes()
        rr.assert_same_multiset(ex.samples, pts[inside], f"{name}@{offset} {kind}")
        cc = dev.count_region(u, r)
        assert [int(cc[f]) for f in COUNT_FIELDS] == [int(c[f]) for f in COUNT_FIELDS] == [int(cnt[f]) for f in COUNT_FIELDS]
        # the same region against the origin box is another answer (or none): the query reads boxMin
        if kind in ("oblique", "box"):
            ign = dev.count_region(cases.origin_box_uniforms(u), r)
            assert [int(ign[f]) for f in COUNT_FIELDS] != [int(c[f]) for f in COUNT_FIELDS]


# ---- footprint queries -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", fr.SHIFTED)
def test_query_footprint_in_a_box_off_the_origin(built_libs, name, offset):
    """simlod_query_footprint on shifted octrees, the footprints placed relative to the shifted box: byte-equal to the host mirror
    OctreeExport.crop(footprint=) at full depth, one level cut and with the inner nodes' voxels, from the builder's chunk table and from walked
    lists; multiset-equal to the input filtered by footprint_ref.contains_exact; the count-only call consistent.  At the georef offset one
    fp32 step in y is 0.25 m, and the node rectangles (boxMin + X * size) - e and the fp64 edge products are six orders larger than at the
    origin."""
    off = cases.offset_of(offset, cases.case(name)[1])
    pts, box_min, box, batch = cases.shifted(name, off)
    dev = _device(persistent_bytes=2 << 30)
    u = dev.uniforms(W, H, cases.shifted_cam(box, off), box, box_min=box_min)
    dev.reset(u)
    _feed(dev, u, cases.batches_of(name, pts, batch))
    assert int(dev.read_stats()["dbg"]) == 0
    full = dev.export_octree(u)
    assert full.box_min == box_min
    prints = {kind: fr.footprint(kind, box, box_min) for kind in fr.SHIFTED_KINDS + (["star128"] if name in fr.SHIFTED_STAR128 else [])}
    slab = rr.region("slab", box, box_min)
    modes = (("cut", 20), ("cut", 2), ("all", 20))
    crops = {(kind, sel, ml): full.crop(Region(), ml, sel, return_counts=True, footprint=f) for kind, f in prints.items() for sel, ml in modes}
    crops["star7+slab", "cut", 20] = full.crop(slab, 20, "cut", return_counts=True, footprint=prints["star7"])
    for source in ("chunk table", "walk"):
        for (kind, sel, ml), (mirror, cnt) in crops.items():
            f, r = (prints["star7"], slab) if kind == "star7+slab" else (prints[kind], None)
            on_footprints._assert_matches(on_footprints.Raw(dev, u, f, r, ml, sel), mirror, cnt, f"{name}@{offset} {kind} {sel}@{ml} ({source})")
        dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))        # the builder's chunk table no longer counts: every list is walked
    for kind, f in prints.items():
        exact = fr.contains_exact(f, pts)
        if kind == "miss":
            assert not exact.any()
        else:
            assert exact.any() and not exact.all(), "the footprint must cut the cloud"
        mirror, cnt = crops[kind, "cut", 20]
        ex, c = dev.query_region(u, Region(), return_counts=True, footprint=f)
        assert ex.nodes.tobytes() == mirror.nodes.tobytes() and ex.samples.tobytes() == mirror.samples.tobytes()
        rr.assert_same_multiset(ex.samples, pts[exact], f"{name}@{offset} {kind}")
        cc = dev.count_region(u, Region(), footprint=f)
        assert [int(cc[k]) for k in COUNT_FIELDS] == [int(c[k]) for k in COUNT_FIELDS] == [int(cnt[k]) for k in COUNT_FIELDS]
        # the same footprint against the origin box is another answer (or none): the query reads boxMin
        if kind in ("star7", "rect"):
            ign = dev.count_region(cases.origin_box_uniforms(u), Region(), footprint=f)
            assert [int(ign[k]) for k in COUNT_FIELDS] != [int(c[k]) for k in COUNT_FIELDS]
    both = fr.contains_exact(prints["star7"], pts) & rr.brute_mask(slab, pts)
    assert both.any()
    rr.assert_same_multiset(crops["star7+slab", "cut", 20][0].samples, pts[both], f"{name}@{offset} star7 and slab")
