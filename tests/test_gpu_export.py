"""GPU tier: simlod_export_octree / simlod_import_octree (include/simlod_hip.h, "octree export / import") against the host restatement of
tests/export_ref.py, byte for byte, and the round trip export -> (file ->) import -> frame against the source octree's frame and the oracle's."""
import ctypes

import numpy as np
import pytest

import cases
import oracle
from export_ref import export_host, keys_of
from simlod_amd import abi, camera, synthetic
from util import STATS_BUILD_FIELDS, assert_dumps_equal, assert_stats_equal, host_image_of, points_multiset_hash

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
STATS_IMPORT_FIELDS = ["numNodes", "numInner", "numLeaves", "numNonemptyLeaves", "numPoints", "numVoxels", "numChunksPoints", "numChunksVoxels"]
CHUNK_STRIDE = abi.alloc_round(abi.CHUNK_BYTES)


def _device(**kw):
    from simlod_amd.runtime import DeviceOctree
    kw.setdefault("persistent_bytes", 2 << 30)
    kw.setdefault("max_pixels", 1920 * 1080)
    dev = DeviceOctree("cuda:0", **kw)
    # nothing may trust bytes it did not write (tests/test_gpu_parity.py _device)
    dev.momentary.fill_(0xA5); dev.render_buffer.fill_(0xA5); dev.persistent.fill_(0xA5)
    return dev


def _build(name, dev=None):
    pts, box, batch, T = cases.case(name)
    dev = dev or _device()
    u = dev.uniforms(W, H, T, box)
    dev.reset(u)
    for b in cases.batches_of(name, pts, batch):
        if dev.uploaded_host - dev.processed() >= dev.ring_slots:
            dev.drain(u)
        dev.upload(b)
    dev.drain(u)
    assert int(dev.read_stats()["dbg"]) == 0
    return dev, u, pts


def _host_export(dev, max_level=20, select=abi.EXPORT_ALL):
    nodes, pers, n = host_image_of(dev)
    t, s = export_host(nodes, n, max_level, select)
    del pers
    return t, s


def _assert_export(ex, t, s, what=""):
    assert ex.num_nodes == len(t) and ex.num_samples == len(s), (what, ex.num_nodes, len(t), ex.num_samples, len(s))
    got = ex.nodes
    if got.tobytes() != t.tobytes():
        bad = np.nonzero(got.view(np.uint8).reshape(-1, 40) != t.view(np.uint8).reshape(-1, 40))[0]
        raise AssertionError(f"{what}: table differs at {len(np.unique(bad))} entries, first {bad[0]}: {got[bad[0]]} != {t[bad[0]]}")
    if ex.samples.tobytes() != s.tobytes():
        bad = np.nonzero(ex.samples.view(np.uint8).reshape(-1, 16) != s.view(np.uint8).reshape(-1, 16))[0]
        raise AssertionError(f"{what}: samples differ at {len(np.unique(bad))} samples, first {bad[0]}")


def _oracle_render(nodes, nn, u):
    fb = np.zeros(W * H, dtype=np.uint64)
    col = np.zeros(W * H, dtype=np.uint32)
    vis = np.zeros(abi.MAX_VISIBLE_NODES, dtype=abi.node_dtype)
    stats = np.zeros(1, dtype=abi.stats_dtype)
    stats["numNodes"] = nn
    uu = np.ascontiguousarray(u).reshape(1)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    oracle.port_lib().oracle_render(None, p(uu), p(nodes), p(stats), p(fb), p(col), p(vis), 1)
    return fb, col


def _variants(u):
    out = []
    for name, kw in (("plain", {}), ("hqs", {"useHighQualityShading": 1}), ("by_node", {"colorByNode": 1}), ("ps2", {"pointSize": 2})):
        v = np.array(u, copy=True)
        for k, val in kw.items():
            v[k] = val
        out.append((name, v))
    return out


@pytest.mark.parametrize("name", cases.CASES)
def test_export_all_matches_host(built_libs, name):
    dev, u, pts = _build(name)
    t, s = _host_export(dev)
    _assert_export(dev.export_octree(u), t, s, f"{name} (chunk table)")
    dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))        # the builder's chunk table no longer counts: every list is walked
    _assert_export(dev.export_octree(u), t, s, f"{name} (walk)")
    st = dev.read_stats()
    assert len(s) == int(st["numPoints"]) + int(st["numVoxels"]) and len(t) == int(st["numNodes"])


def test_lists_longer_than_a_chunk_table_row(built_libs):
    """The voxel lists of a dense cube's upper nodes hold more than 50 chunks, a row of the builder's chunk table: k_x_dir takes what the row
    gives and follows `next` behind it, and the result is the host walk's, as it is with the table dropped."""
    pts, box = synthetic.uniform_cube(600_000, seed=9)
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    for i in range(0, len(pts), 200_000):
        if dev.uploaded_host - dev.processed() >= dev.ring_slots:
            dev.drain(u)
        dev.upload(pts[i:i + 200_000])
    dev.drain(u)
    assert int(dev.read_stats()["dbg"]) == 0
    t, s = _host_export(dev)
    assert int(t["numSamples"].max()) > 50 * abi.POINTS_PER_CHUNK
    _assert_export(dev.export_octree(u), t, s, "dense cube (chunk table)")
    dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))
    _assert_export(dev.export_octree(u), t, s, "dense cube (walk)")


def test_export_cut_levels(built_libs):
    dev, u, pts = _build("hotspot_150k")
    deepest = int(_host_export(dev)[0]["level"].max())
    assert deepest >= 3
    for ml in (0, 2, deepest, 20):
        t, s = _host_export(dev, ml, abi.EXPORT_CUT)
        ex = dev.export_octree(u, max_level=ml, select="cut")
        _assert_export(ex, t, s, f"cut@{ml}")
        assert ex.nodes["level"].max() == min(ml, deepest)
        assert (ex.nodes["childMask"][ex.nodes["level"] == ml] == 0).all()
        ex.validate()
    assert len(s) == int(dev.read_stats()["numPoints"]) == len(pts)
    assert points_multiset_hash(ex.samples) == points_multiset_hash(pts)


@pytest.mark.parametrize("hqs", [False, True])
def test_export_visible(built_libs, hqs):
    from simlod_amd.runtime import SimlodError
    dev, u, pts = _build("terrain_4x100k")
    with pytest.raises(SimlodError, match="hipError 1"):
        dev.export_octree(u, select="visible")                     # no frame since the last construct
    u["useHighQualityShading"] = int(hqs)
    dev.render(u)
    st = dev.read_stats()
    ex = dev.export_octree(u, select="visible")
    sel = ex.nodes[(ex.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0]
    buf, _ = dev.visible_records()
    nv = int(st["numVisibleNodes"])
    vis = buf[: nv * abi.node_dtype.itemsize].cpu().numpy().view(abi.node_dtype)
    vkeys = (vis["level"].astype(np.uint64) << np.uint64(60)) | (vis["X"].astype(np.uint64) << np.uint64(40)) | (vis["Y"].astype(np.uint64) << np.uint64(20)) | vis["Z"].astype(np.uint64)
    assert nv > 0 and np.array_equal(np.sort(keys_of(sel)), np.sort(vkeys))
    assert int(ex.nodes["numSamples"].sum()) == int(st["numVisiblePoints"]) + int(st["numVisibleVoxels"])
    t, s = _host_export(dev, 20, abi.EXPORT_VISIBLE)
    _assert_export(ex, t, s, "visible")


def _frames_equal(src, dst, u, what, floor=1000):
    nodes, pers, nn = host_image_of(src)
    for name, v in _variants(u):
        src.render(v)
        fb_s, col_s = src.framebuffer(W, H), src.color(W, H)
        dst.render(v)
        fb_d, col_d = dst.framebuffer(W, H), dst.color(W, H)
        assert int((fb_s != abi.CLEAR_PIXEL).sum()) > floor, (what, name)
        assert np.array_equal(fb_d, fb_s), f"{what} {name}: {int((fb_d != fb_s).sum())} pixels differ from the source frame"
        assert np.array_equal(col_d, col_s), f"{what} {name}: colour plane differs from the source frame"
        fb_o, col_o = _oracle_render(nodes, nn, v)
        assert np.array_equal(fb_d, fb_o), f"{what} {name}: {int((fb_d != fb_o).sum())} pixels differ from the oracle's frame"
        assert int(np.abs(col_d.view(np.uint8).astype(np.int16) - col_o.view(np.uint8).astype(np.int16)).max()) <= 1
    del pers


@pytest.mark.parametrize("name", ["uniform_3x40k", "terrain_4x100k"])
def test_roundtrip_frames(built_libs, name):
    src, u, pts = _build(name)
    ex = src.export_octree(u)
    dst = _device()
    dst.nodes.fill_(0xA5)
    dst.import_octree(ex)
    assert_stats_equal(dst.read_stats(), src.read_stats(), STATS_IMPORT_FIELDS, name)
    _frames_equal(src, dst, u, name)
    re = dst.export_octree(u)
    assert re.nodes.tobytes() == ex.nodes.tobytes() and re.samples.tobytes() == ex.samples.tobytes()


def test_roundtrip_through_file(built_libs, tmp_path):
    from simlod_amd.octree_io import OctreeExport
    src, u, pts = _build("uniform_3x40k")
    ex = src.export_octree(u)
    ex.save(tmp_path / "uniform.simlodx")
    ld = OctreeExport.load(tmp_path / "uniform.simlodx")
    assert ld.device.type == "cpu" and ld.box_max == tuple(np.asarray(u["boxMax"], np.float32).tolist())
    dst = _device()
    dst.import_octree(ld)
    uu = dst.uniforms(W, H, u["transform"], ld.box_max)
    _frames_equal(src, dst, uu, "file")
    re = dst.export_octree(uu)
    assert re.nodes.tobytes() == ex.nodes.tobytes() and re.samples.tobytes() == ex.samples.tobytes()


def test_truncated_roundtrip(built_libs):
    src, u, pts = _build("hotspot_150k")
    ex = src.export_octree(u, max_level=2, select="cut")
    dst = _device()
    dst.import_octree(ex)
    re = dst.export_octree(u, select="cut")
    a, b = ex.nodes.copy(), re.nodes.copy()
    cut = (a["level"] == 2) & ((a["flags"] & abi.EXPORT_FLAG_LEAF) == 0)
    assert cut.any() and (b["flags"][cut] & abi.EXPORT_FLAG_LEAF).all()
    a["flags"][cut] |= abi.EXPORT_FLAG_LEAF
    assert a.tobytes() == b.tobytes() and re.samples.tobytes() == ex.samples.tobytes()
    assert int(dst.read_stats()["numLeaves"]) == int(((a["childMask"]) == 0).sum())


def test_import_validation_on_device(built_libs):
    from simlod_amd.runtime import SimlodError
    src, u, pts = _build("terrain_4x100k")
    ex = src.export_octree(u)
    chunks = int(((ex.nodes["numSamples"].astype(np.int64) + 999) // 1000).sum())
    need = 16 + chunks * CHUNK_STRIDE
    # one chunk short: the validation kernel refuses, nothing but Stats.dbg changes
    dst = _device(persistent_bytes=need - CHUNK_STRIDE)
    dst.nodes.fill_(0xA5)
    dst.import_octree(ex, check=False)
    st = dst.read_stats()
    assert int(st["dbg"]) & abi.SIMLOD_ERR_IMPORT
    assert int(st["numNodes"]) == 0
    assert bool((dst.nodes == 0xA5).all()) and bool((dst.persistent == 0xA5).all())
    with pytest.raises(SimlodError, match="SIMLOD_ERR_IMPORT"):
        dst.import_octree(ex)
    # exactly enough: accepted
    ok = _device(persistent_bytes=need)
    ok.import_octree(ex)
    assert int(ok.read_stats()["allocatedBytes_persistent"]) == need
    # more nodes than the node array holds: refused on the host, nothing enqueued
    small = _device(max_nodes=ex.num_nodes - 1)
    small.nodes.fill_(0xA5)
    with pytest.raises(SimlodError, match="hipError 1"):
        small.import_octree(ex)
    assert bool((small.nodes == 0xA5).all()) and bool((small.persistent == 0xA5).all()) and int(small.read_stats()["dbg"]) == 0


def test_construct_refused_on_imported(built_libs):
    from simlod_amd.runtime import SimlodError
    name = "uniform_3x40k"
    src, u, pts = _build(name)
    ex = src.export_octree(u)
    dst = _device()
    dst.import_octree(ex)
    with pytest.raises(SimlodError, match="hipError 1"):
        dst.construct(u)
    with pytest.raises(SimlodError, match="hipError 1"):
        dst.colorfilter(u)
    re = dst.export_octree(u)
    assert re.nodes.tobytes() == ex.nodes.tobytes() and re.samples.tobytes() == ex.samples.tobytes()
    # after a reset the array is the builder's again
    _build(name, dst)
    _, box, batch, _ = cases.case(name)
    ref = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=8)
    ref.reset(u)
    ref.add_points(u, pts, batch)
    nodes, pers, n = host_image_of(dst)
    assert_dumps_equal(oracle.dump_image(nodes, n), ref.dump(), name)
    assert_stats_equal(dst.read_stats(), ref.stats[0], STATS_BUILD_FIELDS, name)


def test_two_contexts_export_by_node_array(built_libs):
    a, ua, _ = _build("uniform_3x40k")
    b, ub, _ = _build("terrain_4x100k")
    assert a.ctx.value != b.ctx.value
    t, s = _host_export(a)
    _assert_export(a.export_octree(ua), t, s, "A")
    t, s = _host_export(b)
    _assert_export(b.export_octree(ub), t, s, "B")


@pytest.mark.slow
def test_config2_export_roundtrip(built_libs):
    import torch
    n_points = 36_000_000
    tile = (6000.0, 4000.0, 400.0)
    box = np.array(tile, dtype=np.float32)
    Wd, Hd = 1920, 1080
    src = _device(persistent_bytes=4 << 30)
    gen = torch.empty(n_points * 16, dtype=torch.uint8, device=src.device)
    src.generate_terrain(gen, 0, n_points, 7, 1, tile)
    T = camera.world_view_proj(camera.orbit_view(-0.207, -0.797, 3866.886, (box[0] / 2, box[1] / 2, 0.35 * box[2])), camera.perspective(aspect=Wd / Hd))
    u = src.uniforms(Wd, Hd, T, box, hqs=True)
    src.reset(u)
    src.stream(u, gen, n_points)
    st = src.read_stats()
    ex = src.export_octree(u)
    assert ex.num_nodes == int(st["numNodes"]) and ex.num_samples == int(st["numPoints"]) + int(st["numVoxels"])
    cut = src.export_octree(u, select="cut")
    assert cut.num_samples == n_points == int(st["numPoints"])
    h_in = points_multiset_hash(gen.cpu().numpy().view(abi.point_dtype))
    del gen
    assert points_multiset_hash(cut.samples) == h_in
    del cut
    dst = _device(persistent_bytes=2 << 30)
    dst.import_octree(ex)
    assert_stats_equal(dst.read_stats(), st, STATS_IMPORT_FIELDS, "config 2")
    for hqs in (1, 0):
        u["useHighQualityShading"] = hqs
        src.render(u)
        dst.render(u)
        assert np.array_equal(dst.framebuffer(Wd, Hd), src.framebuffer(Wd, Hd)) and np.array_equal(dst.color(Wd, Hd), src.color(Wd, Hd))
