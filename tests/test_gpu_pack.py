"""GPU tier: simlod_pack_samples and simlod_unpack_samples (include/simlod_hip.h, "packed samples") — the device against the numpy mirror
octree_io.pack_samples / unpack_samples on the device's own exports and query results, byte for byte: packed words, unpacked samples, counts.
A hand-made table on the kernels' piece and wave boundaries through the C ABI with poisoned buffers, capacities, exports of three octrees, octrees
13 and 20 deep, a region query's result, a view delta and its merge; the calls leave their inputs alone."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import deep_ref
import pack_ref as kr
import region_ref as rr
import view_ref as vr
from simlod_amd import abi, camera
from simlod_amd.octree_io import OctreeExport, PackedExport, PackedViewDelta, ViewDelta, pack_samples, unpack_samples
from util import _build, _device, _ingest

pytestmark = pytest.mark.gpu
POISON = 0xA5
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
EXTRA = 64                                    # records behind the capacity that must keep their poison


@pytest.fixture(scope="module")
def small(built_libs):
    """A device object for its library handle, scratch buffer and stream: the calls need no octree (rule K9)."""
    return _device(persistent_bytes=64 << 20, max_pixels=64 * 64)


class RawPack:
    """One simlod_pack_samples (or, unpack, simlod_unpack_samples) call through the C ABI with the output, the counts and the scratch buffer
    poisoned.  src: the samples (abi.point_dtype) or the packed words (uint64)."""

    def __init__(self, dev, unpack, table, src, box_min, box_max, entries=None, capacity=None, scratch_bytes=None):
        L = dev.L
        n = len(src) if capacity is None else capacity
        nn = len(table)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev.device)
        self.table, self.src = up(table), up(src)
        self.entries = None if entries is None else up(entries)
        self.before = [t.clone() for t in (self.table, self.src)] + ([] if entries is None else [self.entries.clone()])
        self.out_size = 16 if unpack else 8
        self.out = torch.full(((len(src) + EXTRA) * self.out_size,), POISON, dtype=torch.uint8, device=dev.device)
        self.counts_t = torch.full((40 + 24,), POISON, dtype=torch.uint8, device=dev.device)
        need = int(L.simlod_pack_buffer_min_bytes(nn, len(src))) if scratch_bytes is None else scratch_bytes
        self.scratch = torch.full((need + 256,), POISON, dtype=torch.uint8, device=dev.device)
        u = np.zeros(1, dtype=abi.uniforms_dtype)
        u["boxMin"], u["boxMax"] = box_min, box_max
        call = L.simlod_unpack_samples if unpack else L.simlod_pack_samples
        self.rc = call(ctypes.c_void_p(u.ctypes.data), dev._p(self.table), None if entries is None else dev._p(self.entries), nn, dev._p(self.src), ctypes.c_uint64(n),
                       dev._p(self.scratch), ctypes.c_uint64(need), dev._p(self.out), dev._p(self.counts_t), dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:40].view(abi.pack_counts_dtype)[0]
        self.result = self.out.cpu().numpy()[: len(src) * self.out_size].view(abi.point_dtype if unpack else np.uint64)
        self.behind_ok = bool((self.out[len(src) * self.out_size:] == POISON).all()) and bool((self.counts_t[40:] == POISON).all()) and \
            bool((self.scratch[need:] == POISON).all())

    def inputs_unchanged(self):
        now = [self.table, self.src] + ([] if self.entries is None else [self.entries])
        return all(bool((a == b).all()) for a, b in zip(now, self.before))


def _poison(n, unpack):
    return np.full(n * (16 if unpack else 8), POISON, np.uint8).view(abi.point_dtype if unpack else np.uint64)


def _assert_raw_is_mirror(dev, table, samples, mn, mx, entries=None, what=""):
    """pack then unpack through the C ABI against the mirror: words, samples, both counts records, poison where nothing belongs, inputs unchanged.
    -> (packed, pack counts, unpacked)"""
    raw = RawPack(dev, False, table, samples, mn, mx, entries)
    want, wc = pack_samples(table, samples, mn, mx, entries, out=_poison(len(samples), False))
    assert raw.rc == 0 and raw.counts.tobytes() == wc.tobytes(), f"{what}: counts {raw.counts}, the mirror has {wc}"
    assert raw.result.tobytes() == want.tobytes(), f"{what}: {int((raw.result != want).sum())} packed words differ"
    assert raw.behind_ok and raw.inputs_unchanged(), what
    back = RawPack(dev, True, table, raw.result, mn, mx, entries)
    wback, wuc = unpack_samples(table, want, mn, mx, entries, out=_poison(len(samples), True))
    assert back.rc == 0 and back.counts.tobytes() == wuc.tobytes() and back.result.tobytes() == wback.tobytes(), f"{what}: the unpacked samples differ"
    assert back.behind_ok and back.inputs_unchanged(), what
    return raw.result, raw.counts, back.result


# ---- 1. the hand table: no octree ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["origin", "georef"])
def test_hand_table_pack_then_unpack(small, where):
    mn = np.zeros(3, np.float32) if where == "origin" else np.asarray(cases.GEOREF, np.float32)
    mx = (mn + np.asarray((1, 1, 1) if where == "origin" else (600, 400, 40), np.float32)).astype(np.float32)
    table = kr.the_hand_table()
    samples, trouble = kr.hand_samples(table, mn, mx)
    packed, c, back = _assert_raw_is_mirror(small, table, samples, mn, mx, what=f"hand table {where}")
    assert int(c["numSamples"]) == len(samples) and int(c["numAlpha"]) == 2 and int(c["numInexact"]) >= 1 and int(c["numClamped"]) >= 5 and int(c["error"]) == 0
    if where == "origin":
        assert int(c["numInexact"]) == 1
        vox = kr.voxel_mask(table, len(samples))
        vox[[trouble["off centre"], trouble["alpha 0"]]] = False
        assert back[vox].tobytes() == samples[vox].tobytes()


def test_hand_table_sample_capacity_one_short(small):
    """Rule K7: the last entry reaches one sample beyond sampleCapacity — SIMLOD_EXPORT_ERR_CAPACITY, its outputs keep their poison, every other
    entry is complete."""
    mn, mx = (0, 0, 0), (1, 1, 1)
    table = kr.the_hand_table()
    samples, _ = kr.hand_samples(table, mn, mx)
    n, last = len(samples), int(table["numSamples"][-1])
    assert last > 1 and int(table["firstSample"][-1]) + last == n
    raw = RawPack(small, False, table, samples, mn, mx, capacity=n - 1)
    want, wc = pack_samples(table, samples[:-1], mn, mx, out=_poison(n - 1, False))
    assert raw.rc == 0 and int(raw.counts["error"]) == abi.EXPORT_ERR_CAPACITY and raw.counts.tobytes() == wc.tobytes()
    assert int(raw.counts["numSamples"]) == n - last
    assert raw.result[: n - 1].tobytes() == want.tobytes() and (raw.result[n - last:] == POISON64).all() and not (raw.result[: n - last] == POISON64).any()
    assert raw.behind_ok and raw.inputs_unchanged()
    full = pack_samples(table, samples, mn, mx)[0]
    back = RawPack(small, True, table, full, mn, mx, capacity=n - 1)
    wback, wuc = unpack_samples(table, full[:-1], mn, mx, out=_poison(n - 1, True))
    assert back.rc == 0 and int(back.counts["error"]) == abi.EXPORT_ERR_CAPACITY and back.counts.tobytes() == wuc.tobytes()
    assert back.result[: n - 1].tobytes() == wback.tobytes() and (back.result[n - last:].view(np.uint8) == POISON).all()
    assert back.behind_ok and back.inputs_unchanged()


def test_hand_table_scratch_one_item_short(small):
    """Rule K7: a scratch buffer with room for one piece fewer than the ranges have — SIMLOD_EXPORT_ERR_CAPACITY and nothing is written; with room
    for exactly the pieces the call is complete."""
    mn, mx = (0, 0, 0), (1, 1, 1)
    table = kr.the_hand_table()
    samples, _ = kr.hand_samples(table, mn, mx)
    L = small.L
    floor = int(L.simlod_pack_buffer_min_bytes(len(table), 0))
    pieces = kr.num_pieces(table)
    exact = floor + (pieces - (len(table) + 1)) * abi.PACK_ITEM_BYTES
    assert exact - abi.PACK_ITEM_BYTES >= floor and exact <= int(L.simlod_pack_buffer_min_bytes(len(table), len(samples)))
    want, wc = pack_samples(table, samples, mn, mx)
    for unpack, src in ((False, samples), (True, want)):
        short = RawPack(small, unpack, table, src, mn, mx, scratch_bytes=exact - abi.PACK_ITEM_BYTES)
        assert short.rc == 0 and int(short.counts["error"]) == abi.EXPORT_ERR_CAPACITY and int(short.counts["numSamples"]) == 0
        assert (short.result.view(np.uint8) == POISON).all() and short.behind_ok and short.inputs_unchanged()
        fits = RawPack(small, unpack, table, src, mn, mx, scratch_bytes=exact)
        assert fits.rc == 0 and int(fits.counts["error"]) == 0 and int(fits.counts["numSamples"]) == len(samples) and fits.behind_ok
        assert fits.result.tobytes() == (unpack_samples(table, want, mn, mx)[0] if unpack else want).tobytes()
        if not unpack:
            assert fits.counts.tobytes() == wc.tobytes()
        refused = RawPack(small, unpack, table, src, mn, mx, scratch_bytes=floor - 1)
        assert refused.rc == 1 and (refused.out == POISON).all() and (refused.counts_t == POISON).all() and (refused.scratch == POISON).all()


# ---- 2. the device's own exports ----------------------------------------------------------------------------------------------------------------------
def _assert_export(dev, ex, what):
    """DeviceOctree.pack / unpack on `ex` against the mirror on the same arrays -> (PackedExport, counts, the unpacked OctreeExport)"""
    table_before, samples_before = ex.table_tensor.clone(), ex.samples_tensor.clone()
    px, c = dev.pack(ex, return_counts=True)
    mirror, mc = ex.pack(return_counts=True)
    assert isinstance(px, PackedExport) and px.device.type == "cuda" and c.tobytes() == mc.tobytes(), f"{what}: counts {c}, the mirror has {mc}"
    assert px.packed.tobytes() == mirror.packed.tobytes() and px.nodes.tobytes() == ex.nodes.tobytes(), what
    assert int(c["numInexact"]) == 0 and int(c["numAlpha"]) == 0 and int(c["numSamples"]) == ex.num_samples > 0
    back, uc = dev.unpack(px, return_counts=True)
    mback, muc = mirror.unpack(return_counts=True)
    assert isinstance(back, OctreeExport) and back.samples.tobytes() == mback.samples.tobytes() and uc.tobytes() == muc.tobytes(), what
    assert (back.select, back.max_level, back.box_min, back.box_max) == (ex.select, ex.max_level, ex.box_min, ex.box_max)
    assert bool((ex.table_tensor == table_before).all()) and bool((ex.samples_tensor == samples_before).all()), f"{what}: the call changed its inputs"
    vox = kr.voxel_mask(ex.nodes, ex.num_samples)
    assert back.samples[vox].tobytes() == ex.samples[vox].tobytes(), what
    kr.assert_points_within_bound(ex.nodes, ex.samples, back.samples, ex.box_min, ex.box_max, what=what)
    return px, c, back


@pytest.mark.parametrize("name,offset,cut", [("uniform_3x40k", None, False), ("hotspot_150k", None, True), ("terrain_4x100k", cases.GEOREF, False)],
                         ids=["uniform_3x40k", "hotspot_150k-cut2", "terrain_4x100k@georef"])
def test_exports(built_libs, name, offset, cut):
    dev, u, _, _ = _build(name, offset)
    ex = dev.export_octree(u, 2, "cut") if cut else dev.export_octree(u)
    px, c, back = _assert_export(dev, ex, name)
    if cut:
        assert not (ex.nodes["flags"][ex.nodes["numSamples"] > 0] & abi.EXPORT_FLAG_LEAF).any()
        assert back.samples.tobytes() == ex.samples.tobytes() and ex.num_samples > 0
    else:
        vox = kr.voxel_mask(ex.nodes, ex.num_samples)
        assert vox.any() and not vox.all()
    # the raw call with poison behind every output says the same
    _assert_raw_is_mirror(dev, ex.nodes, ex.samples, ex.box_min, ex.box_max, what=f"{name} raw")


@pytest.mark.parametrize("name", ["d13", "d20"])
def test_deep_octrees(built_libs, name):
    """Voxels of level-12 and level-19 inner nodes, and the level-20 leaf of identical points."""
    d = deep_ref.built(name)
    dev = _device()
    u = dev.uniforms(cases.W, cases.H, np.eye(4, dtype=np.float32), d.box)
    dev.reset(u)
    _ingest(dev, u, d.batches)
    ex = dev.export_octree(u)
    _assert_export(dev, ex, name)
    t = ex.nodes
    inner = (t["flags"] & abi.EXPORT_FLAG_LEAF) == 0
    deepest = 12 if name == "d13" else 19
    assert int(t["numSamples"][inner & (t["level"] == deepest)].astype(np.int64).sum()) > 0, f"no voxels at level {deepest}"
    if name == "d20":
        assert int(t["numSamples"][~inner & (t["level"] == 20)].astype(np.int64).sum()) > 1000


# ---- 3. a query's result and a view delta ----------------------------------------------------------------------------------------------------------
def test_region_query_result(built_libs):
    dev, u, _, box = _build("uniform_3x40k")
    ex = dev.query_region(u, rr.region("oblique", box), select="cut")
    assert 0 < ex.num_samples and ex.select == abi.EXPORT_REGION
    px, c, _ = _assert_export(dev, ex, "region oblique")
    assert px.select == abi.EXPORT_REGION


def test_view_delta_and_its_merge(built_libs):
    """The bird camera against a held cut from `closer` on the terrain: the packed delta equals the mirror's, and the merge of the unpacked delta
    equals the merge of the delta itself on voxel entries, within rule K8's bound on leaf entries.  The octree has 33 nodes on three levels, and
    with the same octree on both sides the bird's coarser cut adds voxel entries only; so the held cut is taken after two of the four batches:
    leaves that split since then come as voxel entries, and a new leaf comes as points."""
    pts, box, batch, T = cases.case("terrain_4x100k")
    batches = cases.batches_of("terrain_4x100k", pts, batch)
    dev = _device()
    u = dev.uniforms(cases.W, cases.H, T, box)
    ub, uc = (dev.uniforms(cases.W, cases.H, camera.lookat_transform(*cases.camera_pose(c, box), cases.W, cases.H), box, min_node_size=vr.MIN_NODE_SIZE)
              for c in ("bird", "closer"))
    dev.reset(u)
    _ingest(dev, u, batches[:2])
    held = dev.query_view(uc)
    _ingest(dev, u, batches[2:])
    delta = dev.query_view_delta(ub, held)
    e, t = delta.entries, delta.nodes
    added = (e["state"] == abi.DELTA_ADDED) & (e["numDelta"] > 0)
    leaf = (t["flags"] & abi.EXPORT_FLAG_LEAF) != 0
    assert (added & leaf).any() and (added & ~leaf).any(), "the delta must add a voxel entry and a leaf entry"
    before = [x.clone() for x in (delta.table_tensor, delta.entries_tensor, delta.samples_tensor)]
    pd, c = dev.pack(delta, return_counts=True)
    mirror, mc = delta.pack(return_counts=True)
    assert isinstance(pd, PackedViewDelta) and pd.packed.tobytes() == mirror.packed.tobytes() and c.tobytes() == mc.tobytes()
    assert int(c["numSamples"]) == delta.num_samples == int(delta.counts["numDeltaSamples"]) and int(c["numInexact"]) == 0 and int(c["numAlpha"]) == 0
    assert all(bool((a == b).all()) for a, b in zip(before, (delta.table_tensor, delta.entries_tensor, delta.samples_tensor)))
    back = dev.unpack(pd)
    assert isinstance(back, ViewDelta) and back.samples.tobytes() == mirror.unpack().samples.tobytes()
    assert back.entries.tobytes() == e.tobytes() and back.dropped.tobytes() == delta.dropped.tobytes()
    exact = dev.merge_view_delta(held, delta)
    lossy = dev.merge_view_delta(held, back)
    assert lossy.nodes.tobytes() == exact.nodes.tobytes() and lossy.num_samples == exact.num_samples
    vox = kr.voxel_mask(exact.nodes, exact.num_samples)
    assert vox.any() and lossy.samples[vox].tobytes() == exact.samples[vox].tobytes()
    n, worst = kr.assert_points_within_bound(exact.nodes, exact.samples, lossy.samples, exact.box_min, exact.box_max, what="merged leaf entries")
    assert n > 0 and (lossy.samples[~vox]["color"] == exact.samples[~vox]["color"]).all()
    assert lossy.samples.tobytes() != exact.samples.tobytes()                   # (points are 13 bits per axis: the leaf entries did change)
