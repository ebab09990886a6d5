"""GPU tier: simlod_import_octree_buildable (include/simlod_hip.h) — build a prefix of the batches, export it (through a file), import it
buildable into a fresh poisoned object, ingest the remaining batches, and compare with the oracle's CONTINUOUS build of all batches; the import
itself against the source octree and tests/resume_ref.py; the refusals."""
import ctypes

import numpy as np
import pytest

import oracle
from export_ref import entry_index
from resume_ref import rebuild_grids, root_leaf_voxels
from simlod_amd import abi, camera, synthetic
from test_gpu_export import _device, _frames_equal
from util import EXACT_FIELDS, host_image_of, voxel_colors_are_member

import cases

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
# node by node: everything but the history of inner nodes (counter: the arrivals when the node split) and countIteration
RESUME_FIELDS = [f for f in EXACT_FIELDS if f not in ("counter", "countIteration")]
RESUME_STATS = ["numNodes", "numInner", "numLeaves", "numNonemptyLeaves", "numPoints", "numVoxels", "numChunksPoints", "numChunksVoxels", "memCapacityReached"]
CHUNK_STRIDE = abi.alloc_round(abi.CHUNK_BYTES)
GRID_STRIDE = abi.alloc_round(abi.GRID_BYTES)


def _input(name):
    """-> (points, box, batches, cut): the first `cut` batches are built before the export"""
    if name == "terrain_4m":
        pts, box = synthetic.terrain(4_000_000, seed=31, box=(2000.0, 1200.0, 80.0), tile=50.0)
        return pts, box, [pts[i:i + 500_000] for i in range(0, len(pts), 500_000)], 4
    if name == "hotspot_3m":
        pts, box = synthetic.hotspot(3_000_000, seed=32, level=1, cell=(1, 0, 0))
        return pts, box, [pts[i:i + 400_000] for i in range(0, len(pts), 400_000)], 3
    if name == "terrain_90k":               # the root is a leaf at the export and splits after the resume
        pts, box = synthetic.terrain(90_000, seed=33, box=(300.0, 200.0, 20.0), tile=50.0)
        return pts, box, [pts[i:i + 15_000] for i in range(0, len(pts), 15_000)], 2
    if name in ("ragged_before", "ragged_after"):   # cut before / after the batch that splits the root
        pts, box, _, _ = cases.case("ragged_tiny")
        return pts, box, cases.batches_of("ragged_tiny", pts, None), 4 if name == "ragged_before" else 5
    raise KeyError(name)


def _feed(dev, u, batches):
    for b in batches:
        if dev.uploaded_host - dev.processed() >= dev.ring_slots:
            dev.drain(u)
        dev.upload(b)
    dev.drain(u)


def _continuous(u, batches):
    ref = oracle.HostOctree("port", persistent_bytes=2 << 30, ring_slots=abi.BATCH_STREAM_SIZE)
    ref.reset(u)
    for b in batches:
        ref.upload(b)
        ref.construct(u)
        assert ref.last_error() == 0
    return ref


def _assert_fields(a, b, fields, what):
    assert len(a) == len(b), f"{what}: node count {len(a)} != {len(b)}"
    for f in fields:
        if not np.array_equal(a[f], b[f]):
            i = int(np.nonzero(np.any(np.atleast_2d((a[f] != b[f]).reshape(len(a), -1)), axis=1))[0][0])
            raise AssertionError(f"{what}: field {f} differs; first: level={a['level'][i]} XYZ=({a['X'][i]},{a['Y'][i]},{a['Z'][i]}) {a[f][i]} != {b[f][i]}")


def _assert_stats(a, b, what):
    for f in RESUME_STATS:
        assert int(a[f]) == int(b[f]), f"{what}: Stats.{f} {int(a[f])} != {int(b[f])}"


def _export_through_file(src, u, tmp_path):
    from simlod_amd.octree_io import OctreeExport
    ex = src.export_octree(u)
    ex.save(tmp_path / "prefix.simlodx")
    ld = OctreeExport.load(tmp_path / "prefix.simlodx")
    assert ld.is_buildable
    return ex, ld


def _import(dst, ld, u):
    dst.nodes.fill_(0xA5)
    uu = dst.uniforms(W, H, u["transform"], ld.box_max)
    dst.import_octree(ld, buildable=True, uniforms=uu)
    return uu


def _check_import(src, dst, ex, u, what, floor=1000):
    """Right after the buildable import: the source's dump (grids included), resume_ref's grids byte for byte, the same export, the same frames
    (more than `floor` pixels drawn)."""
    nodes_s, pers_s, ns = host_image_of(src)
    nodes_d, pers_d, nd = host_image_of(dst)
    _assert_fields(oracle.dump_image(nodes_d, nd), oracle.dump_image(nodes_s, ns), RESUME_FIELDS, f"{what} (import vs source)")
    oracle.check_invariants(nodes_d, nd)
    grids = rebuild_grids(ex.nodes, ex.samples, u)
    where = entry_index(ex.nodes)
    have = np.nonzero(nodes_d["grid"][:nd] != 0)[0]
    assert len(have) == len(grids)
    for i in have:
        n = nodes_d[i]
        key = (int(n["level"]), int(n["X"]), int(n["Y"]), int(n["Z"]))
        off = int(n["grid"]) - pers_d.ctypes.data
        assert np.array_equal(pers_d[off: off + abi.GRID_BYTES].view(np.uint32), grids[where[key]]), f"{what}: grid of node {i} differs from resume_ref's"
    if ex.nodes[0]["childMask"] == 0:
        _, vox = root_leaf_voxels(ex.nodes, ex.samples, u)
        got = oracle.gather_samples(int(nodes_d[0]["voxelChunks"]), int(nodes_d[0]["numVoxelsStored"]))
        assert got.tobytes() == vox.tobytes(), f"{what}: the root's rebuilt voxels differ from resume_ref's"
    assert_st = dst.read_stats()
    # the builder's state: nothing ingested yet, an empty recycle stack (its pointer at the point chunks in use)
    assert int(assert_st["dbg"]) == 0 and int(assert_st["batchletIndex"]) == 0 and int(assert_st["numPointsProcessed"]) == 0
    assert int(assert_st["numAllocatedChunks"]) == int(assert_st["chunkPoolSize"]) == int(assert_st["numChunksPoints"])
    _assert_stats(assert_st, src.read_stats(), what)
    re = dst.export_octree(u)
    assert re.nodes.tobytes() == ex.nodes.tobytes() and re.samples.tobytes() == ex.samples.tobytes(), f"{what}: the re-export differs"
    if ex.nodes[0]["childMask"] != 0:
        _frames_equal(src, dst, u, what, floor)
    else:
        # a root that is still a leaf draws its voxels too, and the source coloured those by whichever point got there first (scheduling
        # dependent): positions, hence depths, are bit-equal
        src.render(u)
        dst.render(u)
        fs, fd = src.framebuffer(W, H), dst.framebuffer(W, H)
        assert int((fs != abi.CLEAR_PIXEL).sum()) > 1000 and np.array_equal(fd >> np.uint64(32), fs >> np.uint64(32)), f"{what}: depth differs"


def _resume(name, tmp_path, dst=None, check_import=True, **kw):
    pts, box, batches, cut = _input(name)
    return _resume_batches(name, box, batches, cut, tmp_path, dst=dst, check_import=check_import, pts=pts, **kw)


def _resume_batches(name, box, batches, cut, tmp_path, dst=None, check_import=True, pts=None, feed=_feed, src=None, **kw):
    """Build batches[:cut] (on `src`: a fresh exact-mode device by default), export through a file, import buildable into `dst` (a fresh device by
    default), feed batches[cut:] with `feed`, and compare with the oracle's continuous build of all batches.  -> (dst, its uniforms, the export)"""
    T = cases._cam(box)
    src = src or _device()
    u = src.uniforms(W, H, T, box)
    src.reset(u)
    _feed(src, u, batches[:cut])
    assert int(src.read_stats()["dbg"]) == 0
    ex, ld = _export_through_file(src, u, tmp_path)
    dst = dst or _device(**kw)
    uu = _import(dst, ld, u)
    if check_import:
        _check_import(src, dst, ex, uu, name)
    del src
    feed(dst, uu, batches[cut:])
    ref = _continuous(uu, batches)
    nodes, pers, n = host_image_of(dst)
    _assert_fields(oracle.dump_image(nodes, n), ref.dump(), RESUME_FIELDS, f"{name} (resume vs continuous)")
    oracle.check_invariants(nodes, n)
    st = dst.read_stats()
    _assert_stats(st, ref.stats[0], name)
    assert int(st["dbg"]) == 0 and int(st["batchletIndex"]) == len(batches) - cut
    assert int(st["numPointsProcessed"]) == sum(len(b) for b in batches[cut:])
    if pts is not None and len(pts) <= 100_000:
        assert voxel_colors_are_member(nodes, n, pts, box) > 0
    return dst, uu, ex


@pytest.mark.parametrize("name", ["terrain_4m", "hotspot_3m", "terrain_90k", "ragged_before", "ragged_after"])
def test_resume_equals_continuous(built_libs, tmp_path, name):
    _resume(name, tmp_path, check_import=name != "terrain_4m")


def test_resume_over_a_longer_history(built_libs, tmp_path):
    # the object built a different octree with MORE batches than the resumed session runs: its tag words must not look current
    dst = _device()
    pts, box = synthetic.uniform_cube(300_000, seed=34)
    u = dst.uniforms(W, H, cases._cam(box), box)
    dst.reset(u)
    _feed(dst, u, [pts[i:i + 5_000] for i in range(0, len(pts), 5_000)])
    assert int(dst.read_stats()["batchletIndex"]) == 60
    _resume("terrain_90k", tmp_path, dst=dst, check_import=False)


@pytest.mark.parametrize("mode", ["exact_group_1", "exact_default", "coalesced"])
def test_resume_modes(built_libs, tmp_path, mode):
    dst = _device(coalesce=mode == "coalesced")
    if mode == "exact_group_1":
        dst.tune("SIMLOD_EXACT_GROUP", 1)
    _resume("hotspot_3m", tmp_path, dst=dst, check_import=False)


def test_first_launch_is_sized_like_after_a_reset(built_libs, tmp_path):
    pts, box, batches, cut = _input("terrain_90k")
    src = _device()
    u = src.uniforms(W, H, cases._cam(box), box)
    src.reset(u)
    _feed(src, u, batches[:cut])
    _, ld = _export_through_file(src, u, tmp_path)
    dst = _device()
    uu = _import(dst, ld, u)
    for b in batches[cut:cut + 3]:
        dst.upload(b)
    dst.construct(uu)                          # ONCE: sized from the host's counter writes, as after a reset
    assert dst.processed() > 0


def _raw_import(dst, ex, u):
    """simlod_import_octree_buildable without the host-side checks of import_octree."""
    table, samples = ex.table_tensor.to(dst.device), ex.samples_tensor.to(dst.device)
    scratch = dst._export_scratch(int(dst.L.simlod_export_buffer_min_bytes(ex.num_nodes, ex.num_samples)))
    uu, up = dst._u(u)
    rc = dst.L.simlod_import_octree_buildable(up, dst._p(table), ex.num_nodes, dst._p(samples), ctypes.c_uint64(ex.num_samples), dst._p(scratch),
                                              ctypes.c_uint64(scratch.numel()), dst._p(dst.persistent), dst._p(dst.nodes), dst._p(dst.stats),
                                              dst._p(dst.num_uploaded), dst._p(dst.batch_sizes), dst._stream())
    assert rc == 0
    dst.uploaded_host = dst.processed_host = 0
    return int(dst.read_stats()["dbg"])


def _untouched(dev):
    return bool((dev.nodes == 0xA5).all()) and bool((dev.persistent == 0xA5).all())


def test_refusals(built_libs, tmp_path):
    from simlod_amd.octree_io import OctreeExport
    from simlod_amd.runtime import SimlodError
    pts, box, batches, cut = _input("hotspot_3m")
    src = _device()
    u = src.uniforms(W, H, cases._cam(box), box)
    src.reset(u)
    _feed(src, u, batches[:cut])
    ex = src.export_octree(u)
    # truncated or cut: refused on the host, nothing enqueued
    dst = _device()
    dst.nodes.fill_(0xA5)
    for bad in (src.export_octree(u, max_level=2, select="cut"), src.export_octree(u, select="cut")):
        with pytest.raises(SimlodError):
            dst.import_octree(bad, buildable=True, uniforms=u)
    with pytest.raises(SimlodError):
        dst.import_octree(ex, buildable=True)                    # no uniforms
    assert _untouched(dst) and int(dst.read_stats()["dbg"]) == 0
    # a flipped leaf flag past the host: SIMLOD_ERR_IMPORT, nothing else written
    t = ex.nodes.copy()
    t["flags"][int(np.nonzero(t["childMask"] == 0)[0][0])] &= ~np.uint8(abi.EXPORT_FLAG_LEAF)
    assert _raw_import(dst, OctreeExport(t, ex.samples, ex.box_min, ex.box_max), u) & abi.SIMLOD_ERR_IMPORT
    assert _untouched(dst)
    # persistent capacity: chunks + grids exactly fit, one byte less does not
    chunks = int(((ex.nodes["numSamples"].astype(np.int64) + 999) // 1000).sum())
    grids = 1 + int((ex.nodes["childMask"][1:] != 0).sum())
    need = 16 + chunks * CHUNK_STRIDE + grids * GRID_STRIDE
    small = np.array(u, copy=True)
    small["persistentBufferCapacity"] = need - 1
    assert _raw_import(dst, ex, small) & abi.SIMLOD_ERR_IMPORT
    assert _untouched(dst)
    small["persistentBufferCapacity"] = need
    assert _raw_import(dst, ex, small) == 0 and int(dst.read_stats()["allocatedBytes_persistent"]) == need
    # a wrong box past the host: SIMLOD_ERR_IMPORT_GRID; construct() then ingests nothing, the octree still renders
    wrong = np.array(u, copy=True)
    wrong["boxMax"] = np.asarray(u["boxMax"], np.float32) * np.float32(2.0)
    bad = _device()
    assert _raw_import(bad, ex, wrong) & abi.SIMLOD_ERR_IMPORT_GRID
    with pytest.raises(SimlodError, match="SIMLOD_ERR_IMPORT_GRID"):        # (an export that names the wrong box itself passes the host's check)
        _device().import_octree(OctreeExport(ex.nodes, ex.samples, (0, 0, 0), wrong["boxMax"]), buildable=True, uniforms=wrong)
    bad.upload(batches[cut])
    bad.construct(wrong)
    st = bad.read_stats()
    assert int(st["batchletIndex"]) == 0 and int(st["numPoints"]) == int(src.read_stats()["numPoints"])
    assert int(st["dbg"]) & abi.SIMLOD_ERR_IMPORT_GRID
    bad.render(u)
    assert int((bad.framebuffer(W, H) != abi.CLEAR_PIXEL).sum()) > 100


def test_colorfilter_on_a_buildable_import(built_libs, tmp_path):
    pts, box, batches, cut = _input("terrain_90k")
    src = _device()
    u = src.uniforms(W, H, cases._cam(box), box)
    src.reset(u)
    _feed(src, u, batches[:4])
    ex_before, ld = _export_through_file(src, u, tmp_path)
    dst = _device()
    uu = _import(dst, ld, u)
    src.colorfilter(u)
    dst.colorfilter(uu)
    a, b = src.export_octree(u), dst.export_octree(uu)
    assert a.nodes.tobytes() == b.nodes.tobytes()
    # the filter writes a node's voxels in the order their cells were first hit (scheduling dependent): the same samples per node, byte for byte
    owner = np.repeat(np.arange(a.num_nodes), a.nodes["numSamples"].astype(np.int64))

    def per_node(ex):
        w = ex.samples.view(np.uint32).reshape(-1, 4)
        return w[np.lexsort([w[:, 3], w[:, 2], w[:, 1], w[:, 0], owner])]
    assert np.array_equal(per_node(a), per_node(b))
    assert a.samples.tobytes() != ex_before.samples.tobytes()             # (the filter did change colours)


@pytest.mark.slow
def test_config2_resume(built_libs):
    import torch
    n_points, half = 36_000_000, 18_000_000
    tile = (6000.0, 4000.0, 400.0)
    box = np.array(tile, dtype=np.float32)
    Wd, Hd = 1920, 1080
    full = _device(persistent_bytes=4 << 30)
    gen = torch.empty(n_points * 16, dtype=torch.uint8, device=full.device)
    full.generate_terrain(gen, 0, n_points, 7, 1, tile)
    T = camera.world_view_proj(camera.orbit_view(-0.207, -0.797, 3866.886, (box[0] / 2, box[1] / 2, 0.35 * box[2])), camera.perspective(aspect=Wd / Hd))
    u = full.uniforms(Wd, Hd, T, box, hqs=True)
    full.reset(u)
    full.stream(u, gen, n_points)
    nodes_f, pers_f, nf = host_image_of(full)
    dump_f, st_f = oracle.dump_image(nodes_f, nf), full.read_stats()
    del nodes_f, pers_f, full
    part = _device(persistent_bytes=4 << 30)
    part.reset(u)
    part.stream(u, gen[: half * 16], half)
    ex = part.export_octree(u)
    del part
    dst = _device(persistent_bytes=4 << 30)
    dst.import_octree(ex, buildable=True, uniforms=u)
    del ex
    dst.stream(u, gen[half * 16:], n_points - half)
    nodes, pers, n = host_image_of(dst)
    _assert_fields(oracle.dump_image(nodes, n), dump_f, RESUME_FIELDS, "config 2 (resume vs continuous)")
    oracle.check_invariants(nodes, n)
    st = dst.read_stats()
    _assert_stats(st, st_f, "config 2")
    assert int(st["dbg"]) == 0
