"""GPU tier: simlod_query_summary (include/simlod_hip.h, "summary queries") through the C ABI against the host mirror OctreeExport.summarize on
the device's own export, byte for byte: every region and footprint of the paint test with the chunk table and without it, at both selections;
grid independence; the one-bin histograms; the cross-check with a RAMP paint; that nothing but the outputs is written; the empty and the
single-sample selection; capacities and refused arguments; imported, shifted, deep and grown octrees; the Python entry point and the
summarise-summarise-paint workflow.  Every octree here is built by the test that summarises it."""
import ctypes
import types

import numpy as np
import pytest
import torch

import cases
import deep_ref as dr
import footprint_ref as fr
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Paint, Region
from test_gpu_paint import COMBOS, _classes, _image
from util import _build, _device, _ingest

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
COUNT_FIELDS = list(abi.query_counts_dtype.names)
SLACK = 64                                    # table entries behind tableCapacity, bytes behind the summary record
NBYTES = abi.summary_dtype.itemsize


def _bins(box, box_min=(0, 0, 0)):
    return np.float32(float(box_min[2]) + 0.1 * float(box[2])), np.float32(256.0 / (0.7 * float(box[2])))


class Raw:
    """One simlod_query_summary call with every buffer poisoned: rc, the counts record and the buffers as the call left them."""

    def __init__(self, dev, u, region=None, footprint=None, *, ml=20, sel="all", z0=0.0, scale=1.0, max_wg=0, table_cap=None, scratch_bytes=None,
                 params_record=None, region_record=None, foot_record=None, null=(), misalign=0):
        st = dev.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        self.table_cap = nn if table_cap is None else table_cap
        L = dev.L
        need = int(L.simlod_summary_buffer_min_bytes(self.table_cap, bound)) if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        self.scratch, self.table, self.counts_t = mk(need), mk((self.table_cap + SLACK) * 40), mk(abi.query_counts_dtype.itemsize)
        self.out_t = mk(NBYTES + SLACK)
        uu, up = dev._u(u)
        r = (Region() if region is None else region).record() if region_record is None else region_record
        f = foot_record if foot_record is not None else None if footprint is None else footprint.record()
        p = params_record
        if p is None:
            p = np.zeros(1, dtype=abi.summary_params_dtype)
            p["z0"], p["scale"], p["maxWorkgroups"] = z0, scale, max_wg
        ptr = lambda name, a: None if name in null or a is None else ctypes.c_void_p(a.ctypes.data)
        dp = lambda name, t: None if name in null or t is None else dev._p(t)
        out = None if "summary" in null else ctypes.c_void_p(self.out_t.data_ptr() + misalign)
        self.rc = L.simlod_query_summary(dp("nodes", dev.nodes), dp("stats", dev.stats), None if "uniforms" in null else up, ptr("region", r), ptr("footprint", f),
                                         ptr("params", p), ml, abi.EXPORT_SELECT[sel] if isinstance(sel, str) else sel, dp("scratch", self.scratch),
                                         ctypes.c_uint64(need), dp("table", self.table), self.table_cap, out, dp("counts", self.counts_t), dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]

    def table_bytes(self, n):
        return self.table[: n * 40].cpu().numpy().tobytes()

    def summary_bytes(self):
        return self.out_t[:NBYTES].cpu().numpy().tobytes()

    def record(self):
        return self.out_t[:NBYTES].cpu().numpy().view(abi.summary_dtype)[0]

    def no_summary(self):
        return bool((self.out_t == 0xA5).all())

    def untouched(self):
        """Nothing but the scratch buffer was written."""
        return bool((self.counts_t == 0xA5).all()) and bool((self.table == 0xA5).all()) and self.no_summary()


def _count_only(dev, u, region, footprint, ml, sel):
    """The table and the counts of the count-only simlod_query_footprint(region, footprint, ml, sel) call."""
    st = dev.read_stats()
    table = dev._table(int(st["numNodes"]))
    c = dev._query(u, Region() if region is None else region, ml, abi.EXPORT_SELECT[sel], table, None, 0, int(st["numPoints"]) + int(st["numVoxels"]), footprint)
    return table[: int(c["numNodes"]) * 40].cpu().numpy().tobytes(), c


def _compare(dev, u, state, region, footprint, ml, sel, z0, scale, what, **kw):
    """One call against the mirror on `state` (the octree's full export on the host) and against the count-only query -> the mirror's Summary."""
    want, cnt = state.summarize(region, ml, sel, footprint=footprint, z0=z0, scale=scale, return_counts=True)
    wtable = state.crop(Region() if region is None else region, ml, sel, footprint=footprint).nodes
    qtable, qc = _count_only(dev, u, region, footprint, ml, sel)
    raw = Raw(dev, u, region, footprint, ml=ml, sel=sel, z0=z0, scale=scale, **kw)
    assert raw.rc == 0, what
    assert {f: int(raw.counts[f]) for f in COUNT_FIELDS} == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    n = int(cnt["numNodes"])
    assert raw.counts.tobytes() == qc.tobytes() and raw.table_bytes(n) == qtable == wtable.tobytes(), f"{what}: not the count-only query's table"
    assert bool((raw.table[n * 40:] == 0xA5).all()), f"{what}: the table was written past numNodes"
    assert bool((raw.out_t[NBYTES:] == 0xA5).all()), f"{what}: written past the record"
    got = raw.record()
    for f in abi.summary_dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), f"{what}: {f} differs: {got[f]} != {want[f]}"
    assert raw.summary_bytes() == want.tobytes(), what
    return want


@pytest.mark.parametrize("source", ["chunk table", "walk"])
@pytest.mark.parametrize("name", ["hotspot_150k", "ragged_tiny"])
def test_summary_matches_mirror(built_libs, name, source):
    """Every combination of the paint test's COMBOS at ALL@20 and at CUT at a middle level: the record, the counts and the table are the
    mirror's and the count-only query's.  source "walk": the builder's chunk table is dropped first."""
    dev, u, pts, box = _build(name)
    if source == "walk":
        dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))
    state = dev.export_octree(u).to("cpu")
    z0, scale = _bins(box)
    mid = max(1, int(state.nodes["level"].max()) // 2)
    seen = np.zeros(4, np.int64)
    total = 0
    for rk, fk in COMBOS:
        r, f = rr.region(rk, box), None if fk is None else fr.footprint(fk, box)
        cl = _classes(state, r, f)
        seen += cl
        if name == "hotspot_150k" and (rk, fk) in (("box", None), ("none", "rect")):
            assert min(cl) >= 1, f"{rk} {fk}: (filtered, copied, short filtered chunks, full filtered chunks) = {cl}"
        for sel, ml in (("all", 20), ("cut", mid)):
            total += _compare(dev, u, state, r, f, ml, sel, z0, scale, f"{name} {rk} {fk} {sel}@{ml} ({source})").num_samples
    assert (seen[[0, 1, 3]] >= 1).all() and (seen[2] >= 1 or name != "hotspot_150k"), seen
    assert total > 0


def test_grid_independence(built_libs):
    """Rule S7: 1, 3 and the library's number of workgroups write the same bytes (with 1 and 3 every workgroup takes many turns)."""
    dev, u, pts, box = _build("hotspot_150k")
    state = dev.export_octree(u).to("cpu")
    z0, scale = _bins(box)
    for r, f in ((Region(), None), (rr.region("slab", box), fr.footprint("star7", box))):
        want = state.summarize(r, 20, "all", footprint=f, z0=z0, scale=scale)
        assert want.num_samples > 20_000
        for wg in (1, 3, 0):
            raw = Raw(dev, u, r, f, z0=z0, scale=scale, max_wg=wg)
            assert raw.rc == 0 and int(raw.counts["error"]) == 0 and raw.summary_bytes() == want.tobytes(), wg


def test_one_colour_one_height_band(built_libs):
    """The path where every lane of a wave names the same bin: after a SET paint of the whole box each histC[k] has one bin that holds every
    sample, and with bins that put every z at the top so has histZ."""
    dev, u, pts, box = _build("hotspot_150k")
    colour = 0x11C0FFEE
    dev.paint_region(u, Region(), Paint.set(colour))
    torch.cuda.synchronize()
    state = dev.export_octree(u).to("cpu")
    n = state.num_samples
    z0, scale = np.float32(-1000.0), np.float32(1000.0)
    want = _compare(dev, u, state, Region(), None, 20, "all", z0, scale, "one colour")
    got = Raw(dev, u, Region(), None, z0=z0, scale=scale).record()
    assert int(got["numSamples"]) == n == want.num_samples
    for k in range(4):
        assert int(got["histC"][k][(colour >> (8 * k)) & 255]) == n and int(got["histC"][k].sum()) == n
    assert int(got["histZ"][255]) == n and int(got["histZ"].sum()) == n
    # ... and through filtered chunks, where the lanes that pass are some of a wave's
    f = fr.footprint("star7", box)
    _compare(dev, u, state, rr.region("slab", box), f, 20, "all", *_bins(box), "one colour, star7")


def test_histz_is_what_a_ramp_paint_paints(built_libs):
    """Rule S3 on the device alone: summarise a footprint selection, paint it RAMP with table[i] = i | 0xff000000 in the same bins, summarise
    again: byte 0 of the colours now has the first call's z histogram and byte 3 is 255 everywhere."""
    dev, u, pts, box = _build("hotspot_150k")
    r, f = rr.region("slab", box), fr.footprint("star7", box)
    z0, scale = dev.summarize_region(u, r, 20, "all", footprint=f).ramp_range()        # the bins that spread this selection's heights
    first = dev.summarize_region(u, r, 20, "all", footprint=f, z0=z0, scale=scale)
    n = first.num_samples
    assert n > 1000 and int(first["histZ"][0]) >= 1 and int(first["histZ"][255]) >= 1 and int((first["histZ"] > 0).sum()) > 2
    c = dev.paint_region(u, r, Paint.ramp_from(first, np.arange(256, dtype=np.uint32) | np.uint32(0xFF000000)), footprint=f)
    assert int(c["numSamples"]) == n
    torch.cuda.synchronize()
    second = dev.summarize_region(u, r, 20, "all", footprint=f, z0=z0, scale=scale)
    assert second["histC"][0].tolist() == first["histZ"].tolist() and int(second["histC"][3][255]) == n == second.num_samples
    assert int(second["histC"][1][0]) == n == int(second["histC"][2][0])
    assert second["histZ"].tolist() == first["histZ"].tolist() and second["sum"].tolist() == first["sum"].tolist()


def test_nothing_else_is_written(built_libs):
    """Rule S6: the Node array, Stats and every allocated byte of the persistent buffer are what they were, the builder's chunk table still
    serves the export, and a frame drawn after the call is the frame drawn before it."""
    dev, u, pts, box = _build("uniform_3x40k")
    dev.render(u)
    before_fb = dev.framebuffer(W, H).copy()
    torch.cuda.synchronize()
    image = _image(dev)
    before = dev.export_octree(u).to("cpu")
    z0, scale = _bins(box)
    for r, f, sel, ml in ((rr.region("oblique", box), None, "all", 20), (rr.region("slab", box), fr.footprint("star7", box), "cut", 2)):
        raw = Raw(dev, u, r, f, ml=ml, sel=sel, z0=z0, scale=scale)
        assert raw.rc == 0 and int(raw.counts["error"]) == 0 and 0 < int(raw.counts["numSamples"]) < before.num_samples
    assert _image(dev) == image
    after = dev.export_octree(u)
    assert after.nodes.tobytes() == before.nodes.tobytes() and after.samples.tobytes() == before.samples.tobytes()
    dev.render(u)
    diff = np.nonzero(dev.framebuffer(W, H) != before_fb)[0]
    assert len(diff) == 0, f"{len(diff)} pixels differ, first {diff[:5]}"


def test_empty_and_single_sample(built_libs):
    dev, u, pts, box = _build("uniform_3x40k")
    state = dev.export_octree(u).to("cpu")
    z0, scale = _bins(box)
    want = _compare(dev, u, state, rr.region("miss", box), None, 20, "all", z0, scale, "empty")
    assert want.num_samples == 0 and (want["min"] == np.inf).all() and (want["max"] == -np.inf).all() and not want["histC"].any()
    # a box of one ulp to either side of a leaf point that no other sample shares its position with
    smp = state.samples
    leaf = np.repeat((state.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0, state.nodes["numSamples"].astype(np.int64))
    w = np.stack([smp[a].view(np.uint32) for a in "xyz"], axis=1)
    _, first, count = np.unique(w, axis=0, return_index=True, return_counts=True)
    i = int(next(j for j in first[count == 1] if leaf[j] and all(float(smp[a][j]) > 0 for a in "xyz")))
    p = [np.float32(smp[a][i]) for a in "xyz"]
    tiny = Region.from_box([float(np.nextafter(v, np.float32(-np.inf))) for v in p], [float(np.nextafter(v, np.float32(np.inf))) for v in p])
    one = _compare(dev, u, state, tiny, None, 20, "all", z0, scale, "one sample")
    assert 1 <= one.num_samples <= 3
    leaves = _compare(dev, u, state, tiny, None, 20, "cut", z0, scale, "one sample, leaves only")
    assert leaves.num_samples == 1 and leaves["min"].tobytes() == leaves["max"].tobytes() == np.array(p, np.float32).tobytes()
    assert int(leaves["histZ"].max()) == 1 and [int(h.max()) for h in leaves["histC"]] == [1] * 4


def test_all_or_nothing_and_refusals(built_libs):
    dev, u, pts, box = _build("uniform_3x40k")
    r, f = rr.region("box", box), fr.footprint("star7", box)
    nn = int(dev.read_stats()["numNodes"])
    z0, scale = _bins(box)
    ok = Raw(dev, u, r, f, z0=z0, scale=scale)
    assert ok.rc == 0 and int(ok.counts["error"]) == 0 and int(ok.counts["numSamples"]) > 1000 and not ok.no_summary()
    # rule S5: a table or a scratch buffer too small
    raw = Raw(dev, u, r, f, z0=z0, scale=scale, table_cap=nn - 1)
    assert raw.rc == 0 and int(raw.counts["error"]) & abi.EXPORT_ERR_CAPACITY and raw.no_summary()
    assert bool((raw.table[(nn - 1) * 40:] == 0xA5).all())
    raw = Raw(dev, u, r, f, z0=z0, scale=scale, scratch_bytes=int(dev.L.simlod_summary_buffer_min_bytes(nn, 0)))
    assert raw.rc == 0 and int(raw.counts["error"]) & abi.EXPORT_ERR_CAPACITY and raw.no_summary()

    # rule S8
    def refused(**kw):
        kw.setdefault("z0", z0); kw.setdefault("scale", scale)
        raw = Raw(dev, u, kw.pop("region", r), kw.pop("footprint", f), **kw)
        assert raw.rc == 1, kw                                                          # hipErrorInvalidValue
        assert raw.untouched() and bool((raw.scratch == 0xA5).all()), kw

    for bad_z0, bad_scale in ((0.0, 0.0), (0.0, -2.0), (0.0, np.nan), (0.0, np.inf), (np.nan, 1.0), (-np.inf, 1.0), (np.inf, 1.0)):
        refused(z0=bad_z0, scale=bad_scale)
    rec = np.zeros(1, dtype=abi.summary_params_dtype); rec["scale"], rec["reserved"] = 1.0, 1
    refused(params_record=rec)
    refused(null=("params",))
    refused(null=("summary",))
    refused(misalign=4)
    refused(scratch_bytes=int(dev.L.simlod_summary_buffer_min_bytes(nn, 0)) - 1)
    # everything simlod_query_footprint refuses
    refused(sel=abi.EXPORT_VISIBLE)
    refused(sel=7)
    for nv in (2, 257):
        rec = f.record(); rec["numVertices"] = nv
        refused(foot_record=rec)
    rec = f.record(); rec["vertices"][0, 1, 0] = np.nan
    refused(foot_record=rec)
    rec = f.record(); rec["reserved"][0, 1] = 1
    refused(foot_record=rec)
    rec = r.record(); rec["numPlanes"] = 17
    refused(region_record=rec)
    rec = r.record(); rec["planes"][0, 0, 3] = np.inf
    refused(region_record=rec)
    for name in ("region", "stats", "uniforms", "scratch", "table", "counts", "nodes"):
        refused(null=(name,))
    # maxWorkgroups is any number
    big = Raw(dev, u, r, f, z0=z0, scale=scale, max_wg=0xFFFFFFFF)
    assert big.rc == 0 and big.summary_bytes() == ok.summary_bytes()


def _one_call(dev, u, region, footprint, what, sel="all", ml=20, box_min=(0, 0, 0)):
    state = dev.export_octree(u).to("cpu")
    box = np.asarray(state.box_max, np.float64) - np.asarray(state.box_min, np.float64)
    want = _compare(dev, u, state, region, footprint, ml, sel, *_bins(box, state.box_min), what)
    assert 0 < want.num_samples < state.num_samples, what
    return state, want


@pytest.mark.parametrize("buildable", [False, True], ids=["render-only", "buildable"])
def test_summarise_an_imported_octree(built_libs, buildable):
    src, u, pts, box = _build("ragged_tiny")
    ex = src.export_octree(u)
    dst = _device()
    dst.nodes.fill_(0xA5)
    if buildable:
        dst.import_octree(ex, buildable=True, uniforms=u)
    else:
        dst.import_octree(ex)
    assert int(dst.read_stats()["dbg"]) == 0
    _one_call(dst, u, rr.region("slab", box), fr.footprint("star7", box), f"imported (buildable={buildable})")
    _one_call(dst, u, rr.region("oblique", box), None, f"imported (buildable={buildable}), cut", sel="cut", ml=1)


def test_summarise_in_a_box_off_the_origin(built_libs):
    name, offset = "terrain_4x100k", "georef"
    dev, u, pts, box = _build(name, cases.offset_of(offset, cases.case(name)[1]))
    box_min = dev.export_octree(u).box_min
    assert box_min != (0.0, 0.0, 0.0)
    state, want = _one_call(dev, u, rr.region("slab", box, box_min), fr.footprint("star7", box, box_min), f"{name}@{offset}")
    # the cells are counted from the box's corner, not from the origin
    size = float((np.asarray(state.box_max, np.float32) - np.asarray(state.box_min, np.float32)).max())
    ctr = want.centroid(state.box_min, size)
    lo, hi = want.extent()
    assert (ctr >= lo.astype(np.float64) - 1.0).all() and (ctr <= hi.astype(np.float64) + 1.0).all()


def test_summarise_a_13_deep_octree(built_libs):
    box, batches, counts, origin = dr.d13_input("d13")
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    d = types.SimpleNamespace(name="d13", size=float(max(box)), origin=np.asarray(origin, np.float64))
    state, _ = _one_call(dev, u, dr.d13_regions(d)["slab"], dr.d13_footprints(d)["star7"], "d13 slab star7")
    assert int(state.nodes["level"].max()) == dr.LEAF_LEVEL
    cl = _classes(state, dr.d13_regions(d)["cell12"], None)
    assert cl[0] >= 1 and cl[1] >= 1, cl
    _one_call(dev, u, dr.d13_regions(d)["cell12"], None, "d13 cell12")
    _one_call(dev, u, dr.d13_regions(d)["cell12"], None, "d13 cell12 cut@12", sel="cut", ml=12)


def test_summarise_a_20_deep_octree(built_libs):
    box, batches, fourth, same = dr.d20_input()
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    full = dev.export_octree(u).to("cpu")
    e, k = dr.deep_entry(full)
    assert int(full.nodes["level"][e]) == abi.MAX_DEPTH and k > 0
    region, keeps = dr.d20_regions(full)["cell20"]
    _one_call(dev, u, region, None, "d20 cell20")
    f, keeps = dr.d20_footprints()["lo_x=x"]
    _one_call(dev, u, Region(), f, "d20 lo_x=x")


def test_summarise_after_further_ingest(built_libs):
    """An octree summarised, grown by batches that split leaves, and summarised again: both times the mirror's record on the export of the
    moment, through the builder's chunk table as the ingest left it."""
    name = "terrain_4x100k"
    pts, box, batch, T = cases.case(name)
    dev = _device()
    u = dev.uniforms(W, H, T, box)
    dev.reset(u)
    batches = cases.batches_of(name, pts, batch)
    _ingest(dev, u, batches[:2])
    st = dev.read_stats()
    r, f = rr.region("slab", box), fr.footprint("star7", box)
    _, early = _one_call(dev, u, r, f, "two batches")
    _ingest(dev, u, batches[2:])
    st2 = dev.read_stats()
    assert int(st2["numLeaves"]) > int(st["numLeaves"]) and int(st2["numPoints"]) == len(pts), "the later batches split no leaf"
    _, late = _one_call(dev, u, r, f, "all batches")
    assert late.num_samples > early.num_samples


def test_python_entry_point_and_workflow(built_libs):
    """DeviceOctree.summarize_region returns the mirror's Summary; summarise (any bins) -> ramp_range -> summarise -> Paint.ramp_from ->
    paint_region leaves an octree whose export is the mirror's after the same three mirror calls."""
    dev, u, pts, box = _build("uniform_3x40k")
    state = dev.export_octree(u).to("cpu")
    r, f = rr.region("slab", box), fr.footprint("star7", box)
    first = dev.summarize_region(u, r, footprint=f, max_level=20, select="all")
    wfirst = state.summarize(r, 20, "all", footprint=f)
    assert first == wfirst and 0 < first.num_samples < state.num_samples
    z0, scale = first.ramp_range()
    assert (z0, scale) == wfirst.ramp_range()
    second = dev.summarize_region(u, r, footprint=f, max_level=20, select="all", z0=z0, scale=scale)
    wsecond = state.summarize(r, 20, "all", footprint=f, z0=z0, scale=scale)
    assert second == wsecond and int(second["histZ"][0]) >= 1 and int(second["histZ"][255]) >= 1
    palette = (np.arange(16, dtype=np.uint32) * np.uint32(0x00101010)) | np.uint32(0xFF000000)
    for equalize in (False, True):
        paint = Paint.ramp_from(second, palette, equalize=equalize)
        c = dev.paint_region(u, r, paint, footprint=f)
        state, wc = state.paint(r, Paint.ramp_from(wsecond, palette, equalize=equalize), footprint=f)
        assert int(c["numSamples"]) == int(wc["numSamples"]) == second.num_samples
        torch.cuda.synchronize()
        got = dev.export_octree(u)
        assert got.nodes.tobytes() == state.nodes.tobytes() and got.samples.tobytes() == state.samples.tobytes(), equalize
    # the defaults: the cut at the deepest level, no footprint, bins (0, 1); and a smaller grid
    assert dev.summarize_region(u, r) == state.summarize(r, None, "cut")
    assert dev.summarize_region(u, r, max_level=2, max_workgroups=2) == state.summarize(r, 2, "cut")
    with pytest.raises(ValueError):
        state.summarize(r, z0=0.0, scale=-1.0)
