"""GPU tier: simlod_query_inverse, simlod_paint_inverse and simlod_query_summary_inverse (include/simlod_hip.h, "inverse selections") through the
C ABI against the host mirrors OctreeExport.crop / paint / summarize(invert=True), byte for byte; against the positive calls (partition,
degenerate selections, summaries that add up); in-place behaviour (undo, the no-load path); count-only calls, capacities, refused arguments;
DeviceOctree.erase_region against the frame SIMLOD_CLIP_OUTSIDE draws; imported, shifted and deep octrees.  Every buffer a call may write is
poisoned first."""
import ctypes
import types

import numpy as np
import pytest
import torch

import cases
import deep_ref as dr
import footprint_ref as fr
import inverse_ref as ir
import lasso_ref as lr
import paint_ref as pf
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Clip, Lasso, Paint, Region
from util import _build, _device, _ingest

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
MODES = ir.MODES
COUNT_FIELDS = list(abi.query_counts_dtype.names)
NBYTES = abi.summary_dtype.itemsize
POISON = 0xA5A5A5A5
SLACK = 64


def _mk(dev, n):
    return torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)


def _sizes(dev):
    st = dev.read_stats()
    return int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])


def _ptr(rec):
    return None if rec is None else ctypes.c_void_p(rec.ctypes.data)


def _polygons(fp, lasso, fp_record, lasso_record):
    f = fp_record if fp_record is not None else None if fp is None else fp.record()
    l = lasso_record if lasso_record is not None else None if lasso is None else lasso.record()
    return f, l


class Raw:
    """One simlod_query_inverse call (entry="positive": the existing query with the same arguments) with every buffer poisoned: rc, the counts
    record, and the buffers as the call left them."""

    def __init__(self, dev, u, sel3, max_level=20, select="cut", *, table_cap=None, sample_cap=None, count_only=False, scratch_bytes=None,
                 fp_record=None, lasso_record=None, region_record=None, null_region=False, entry="inverse"):
        region, fp, lasso = sel3
        nn, bound = _sizes(dev)
        self.table_cap = nn if table_cap is None else table_cap
        self.sample_cap = bound if sample_cap is None else sample_cap
        L = dev.L
        need = int(L.simlod_inverse_buffer_min_bytes(self.table_cap, bound)) if scratch_bytes is None else scratch_bytes
        self.scratch, self.table, self.samples = _mk(dev, need), _mk(dev, (self.table_cap + 4) * 40), _mk(dev, (self.sample_cap + 1000) * 16)
        self.counts_t = _mk(dev, abi.query_counts_dtype.itemsize)
        uu, up = dev._u(u)
        r = (Region() if region is None else region).record() if region_record is None else region_record
        f, l = _polygons(fp, lasso, fp_record, lasso_record)
        head = (dev._p(dev.nodes), dev._p(dev.stats), up, None if null_region else _ptr(r))
        tail = (max_level, abi.EXPORT_SELECT[select] if isinstance(select, str) else select, dev._p(self.scratch), ctypes.c_uint64(need),
                dev._p(self.table), self.table_cap, None if count_only else dev._p(self.samples), ctypes.c_uint64(self.sample_cap),
                dev._p(self.counts_t), dev._stream())
        if entry == "inverse":
            self.rc = L.simlod_query_inverse(*head, _ptr(f), _ptr(l), *tail)
        elif f is not None:
            self.rc = L.simlod_query_footprint(*head, _ptr(f), *tail)
        elif l is not None:
            self.rc = L.simlod_query_lasso(*head, _ptr(l), *tail)
        else:
            self.rc = L.simlod_query_region(*head, *tail)
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]

    def table_bytes(self, n=None):
        n = int(self.counts["numNodes"]) if n is None else n
        return self.table[: n * 40].cpu().numpy().tobytes()

    def nodes(self):
        return self.table[: int(self.counts["numNodes"]) * 40].cpu().numpy().view(abi.export_node_dtype)

    def points(self):
        return self.samples[: int(self.counts["numSamples"]) * 16].cpu().numpy().view(abi.point_dtype)

    def sample_bytes(self, n=None):
        n = int(self.counts["numSamples"]) if n is None else n
        return self.samples[: n * 16].cpu().numpy().tobytes()

    def poison_behind(self, nodes, samples):
        return bool((self.table[nodes * 40:] == 0xA5).all()) and bool((self.samples[samples * 16:] == 0xA5).all())

    def untouched(self):
        return bool((self.counts_t == 0xA5).all()) and self.poison_behind(0, 0) and bool((self.scratch == 0xA5).all())


class RawPaint:
    """One simlod_paint_inverse call with every buffer poisoned.  previous=False: a null pointer."""

    def __init__(self, dev, u, paint, sel3, *, colors=None, color_cap=None, scratch_bytes=None, fp_record=None, lasso_record=None, previous=True):
        region, fp, lasso = sel3
        nn, bound = _sizes(dev)
        L = dev.L
        need = int(L.simlod_paint_buffer_min_bytes(nn, bound)) if scratch_bytes is None else scratch_bytes
        self.scratch, self.table, self.counts_t = _mk(dev, need), _mk(dev, (nn + SLACK) * 40), _mk(dev, abi.query_counts_dtype.itemsize)
        self.cap = (bound if colors is None else len(colors)) if color_cap is None else color_cap
        self.prev_t = _mk(dev, (self.cap + SLACK) * 4)
        self.col_t = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint32).view(np.uint8)).to(dev.device)
        uu, up = dev._u(u)
        r, p = (Region() if region is None else region).record(), paint.record()
        f, l = _polygons(fp, lasso, fp_record, lasso_record)
        self.rc = L.simlod_paint_inverse(dev._p(dev.nodes), dev._p(dev.stats), up, _ptr(r), _ptr(f), _ptr(l), _ptr(p), dev._p(self.scratch), ctypes.c_uint64(need),
                                         dev._p(self.table), nn, None if self.col_t is None else dev._p(self.col_t), dev._p(self.prev_t) if previous else None,
                                         ctypes.c_uint64(self.cap if (previous or colors is not None) else 0), dev._p(self.counts_t), dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]

    def previous(self, n=None):
        w = self.prev_t.cpu().numpy().view(np.uint32)
        return w if n is None else w[:n]

    def untouched(self):
        return bool((self.counts_t == 0xA5).all()) and bool((self.table == 0xA5).all()) and bool((self.prev_t == 0xA5).all()) and bool((self.scratch == 0xA5).all())


class RawSummary:
    """One simlod_query_summary_inverse call with every buffer poisoned."""

    def __init__(self, dev, u, sel3, *, ml=20, sel="all", z0=0.0, scale=1.0, max_wg=0, scratch_bytes=None, fp_record=None, lasso_record=None):
        region, fp, lasso = sel3
        nn, bound = _sizes(dev)
        L = dev.L
        need = int(L.simlod_summary_buffer_min_bytes(nn, bound)) if scratch_bytes is None else scratch_bytes
        self.scratch, self.table, self.counts_t = _mk(dev, need), _mk(dev, (nn + SLACK) * 40), _mk(dev, abi.query_counts_dtype.itemsize)
        self.out_t = _mk(dev, NBYTES + SLACK)
        uu, up = dev._u(u)
        r = (Region() if region is None else region).record()
        f, l = _polygons(fp, lasso, fp_record, lasso_record)
        p = np.zeros(1, dtype=abi.summary_params_dtype)
        p["z0"], p["scale"], p["maxWorkgroups"] = z0, scale, max_wg
        self.rc = L.simlod_query_summary_inverse(dev._p(dev.nodes), dev._p(dev.stats), up, _ptr(r), _ptr(f), _ptr(l), _ptr(p), ml, abi.EXPORT_SELECT[sel],
                                                 dev._p(self.scratch), ctypes.c_uint64(need), dev._p(self.table), nn, dev._p(self.out_t), dev._p(self.counts_t),
                                                 dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]

    def summary_bytes(self):
        return self.out_t[:NBYTES].cpu().numpy().tobytes()

    def untouched(self):
        return bool((self.counts_t == 0xA5).all()) and bool((self.table == 0xA5).all()) and bool((self.out_t == 0xA5).all()) and bool((self.scratch == 0xA5).all())


def _assert_matches(raw, mirror, cnt, what):
    assert raw.rc == 0, what
    got = {f: int(raw.counts[f]) for f in COUNT_FIELDS}
    assert got == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    assert raw.table_bytes() == mirror.nodes.tobytes(), f"{what}: the table differs"
    assert raw.sample_bytes() == mirror.samples.tobytes(), f"{what}: the samples differ"
    assert raw.poison_behind(mirror.num_nodes, mirror.num_samples), f"{what}: written past the result"


def _mirror(full, sel3, ml, sel):
    region, fp, lasso = sel3
    return full.crop(region, ml, sel, return_counts=True, footprint=fp, lasso=lasso, invert=True)


def _paint_and_compare(dev, u, state, paint, sel3, rs, what, previous=True):
    """One simlod_paint_inverse call against the mirror on `state` -> (the mirror's export after the call, the previous colours)."""
    region, fp, lasso = sel3
    n = len(state.crop(region, 20, "all", footprint=fp, lasso=lasso, invert=True, return_index=True)[1])
    colors = rs.randint(0, 1 << 32, n + 5, dtype=np.uint64).astype(np.uint32) if paint.mode == abi.PAINT_ARRAY else None
    want, cnt, prev = state.paint(region, paint, footprint=fp, lasso=lasso, colors=colors, return_previous=True, invert=True)
    raw = RawPaint(dev, u, paint, sel3, colors=colors, previous=previous)
    assert raw.rc == 0, what
    assert {f: int(raw.counts[f]) for f in COUNT_FIELDS} == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    assert int(cnt["numSamples"]) == n
    assert bool((raw.table[int(cnt["numNodes"]) * 40:] == 0xA5).all()), f"{what}: the table was written past numNodes"
    if previous:
        assert np.array_equal(raw.previous(n), prev), f"{what}: previous differs"
        assert (raw.previous()[n:] == POISON).all(), f"{what}: previous was written past numSamples"
    else:
        assert (raw.previous() == POISON).all(), f"{what}: previous was written without being given"
    got = dev.export_octree(u)
    assert got.nodes.tobytes() == want.nodes.tobytes(), f"{what}: the table of the export moved"
    assert got.samples.tobytes() == want.samples.tobytes(), f"{what}: {int((got.samples['color'] != want.samples['color']).sum())} colours differ from the mirror's"
    return want, prev


def _summary_and_compare(dev, u, state, sel3, ml, sel, z0, scale, what, **kw):
    region, fp, lasso = sel3
    want, cnt = state.summarize(region, ml, sel, footprint=fp, lasso=lasso, z0=z0, scale=scale, return_counts=True, invert=True)
    raw = RawSummary(dev, u, sel3, ml=ml, sel=sel, z0=z0, scale=scale, **kw)
    assert raw.rc == 0, what
    assert {f: int(raw.counts[f]) for f in COUNT_FIELDS} == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    n = int(cnt["numNodes"])
    assert raw.table[: n * 40].cpu().numpy().tobytes() == _mirror(state, sel3, ml, sel)[0].nodes.tobytes(), what
    assert bool((raw.table[n * 40:] == 0xA5).all()) and bool((raw.out_t[NBYTES:] == 0xA5).all()), f"{what}: written past the result"
    assert len(want.tobytes()) == NBYTES and raw.summary_bytes() == want.tobytes(), what
    return want


def _bins(box, box_min=(0, 0, 0)):
    return np.float32(float(box_min[2]) + 0.1 * float(box[2])), np.float32(256.0 / (0.7 * float(box[2])))


_BUILT = {}


def _case(name):
    """The case's octree on the device and its full export on the host, once per module.  Nothing may paint it without undoing."""
    if name not in _BUILT:
        dev, u, pts, box = _build(name)
        _BUILT[name] = (dev, u, pts, box, dev.export_octree(u).to("cpu"))
    return _BUILT[name]


@pytest.mark.parametrize("family", ir.FAMILIES)
@pytest.mark.parametrize("name", cases.CASES)
def test_inverse_matches_mirror(built_libs, name, family):
    """Per case x selection of the family x MODES, the chunks read from the builder's chunk table: table, samples, counts, nothing behind the
    result."""
    dev, u, pts, box, full = _case(name)
    for kind in ir.names_for(family, name):
        sel3 = ir.selection(family, kind, box)
        for sel, ml in MODES:
            mirror, cnt = _mirror(full, sel3, ml, sel)
            _assert_matches(Raw(dev, u, sel3, ml, sel), mirror, cnt, f"{name} {family} {kind} {sel}@{ml}")


WALK_KINDS = {"planes": ("oblique", "box"), "footprint": ("rect", "star7"), "lasso": ("half", "rect_fp", "bowtie")}


@pytest.mark.parametrize("name", cases.CASES)
def test_inverse_by_the_walk_paint_summary_and_python_entry_points(built_libs, name):
    """After simlod_octree_image_replaced every chunk list is walked by `next`: query, summary and the four paints (undone afterwards) against
    the mirrors; then the Python entry points, and invert=False through Python against the old entry points' bytes."""
    dev, u, pts, box = _build(name)
    full = dev.export_octree(u).to("cpu")
    dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))
    z0, scale = _bins(box)
    rs = np.random.RandomState(29)
    for family in ir.FAMILIES:
        for kind in WALK_KINDS[family]:
            sel3 = ir.selection(family, kind, box)
            for sel, ml in MODES:
                mirror, cnt = _mirror(full, sel3, ml, sel)
                _assert_matches(Raw(dev, u, sel3, ml, sel), mirror, cnt, f"{name} {family} {kind} {sel}@{ml} (walk)")
                _summary_and_compare(dev, u, full, sel3, ml, sel, z0, scale, f"{name} {family} {kind} summary {sel}@{ml} (walk)")
        sel3 = ir.selection(family, WALK_KINDS[family][0], box)
        state, undo = full, []
        for mode in ("set", "blend", "ramp", "array"):
            state, prev = _paint_and_compare(dev, u, state, pf.paints(box)[mode], sel3, rs, f"{name} {family} {mode} (walk)")
            undo.append(prev)
        assert state.samples.tobytes() != full.samples.tobytes()
        for prev in reversed(undo):
            raw = RawPaint(dev, u, Paint.array(), sel3, colors=prev)
            assert raw.rc == 0 and int(raw.counts["error"]) == 0
        back = dev.export_octree(u)
        assert back.nodes.tobytes() == full.nodes.tobytes() and back.samples.tobytes() == full.samples.tobytes(), f"{name} {family}: undo"
    # the Python entry points
    region, fp, lasso = ir.selection("lasso", "half", box)
    mirror, cnt = full.crop(region, 20, "cut", return_counts=True, lasso=lasso, invert=True)
    ex, c = dev.query_region(u, region, return_counts=True, lasso=lasso, invert=True)
    assert ex.select == abi.EXPORT_REGION and ex.nodes.tobytes() == mirror.nodes.tobytes() and ex.samples.tobytes() == mirror.samples.tobytes()
    cc = dev.count_region(u, region, lasso=lasso, invert=True)
    assert [int(cc[k]) for k in COUNT_FIELDS] == [int(c[k]) for k in COUNT_FIELDS] == [int(cnt[k]) for k in COUNT_FIELDS]
    s = dev.summarize_region(u, region, 20, "all", lasso=lasso, z0=z0, scale=scale, invert=True)
    assert s.tobytes() == full.summarize(region, 20, "all", lasso=lasso, z0=z0, scale=scale, invert=True).tobytes()
    c, prev = dev.paint_region(u, rr.region("box", box), Paint.set(0x00C0FFEE), return_previous=True, invert=True)
    want, wc = full.paint(rr.region("box", box), Paint.set(0x00C0FFEE), invert=True)
    assert int(c["numSamples"]) == int(wc["numSamples"]) and dev.export_octree(u).samples.tobytes() == want.samples.tobytes()
    dev.paint_region(u, rr.region("box", box), Paint.array(), colors=prev, invert=True)
    assert dev.export_octree(u).samples.tobytes() == full.samples.tobytes()
    with pytest.raises(ValueError):
        dev.count_region(u, Region(), lasso=lasso, footprint=fr.footprint("rect", box), invert=True)
    # invert=False is the old entry point, byte for byte
    for family in ir.FAMILIES:
        sel3 = region, fp, lasso = ir.selection(family, WALK_KINDS[family][0], box)
        ex, c = dev.query_region(u, region, 20, "all", return_counts=True, footprint=fp, lasso=lasso, invert=False)
        old = Raw(dev, u, sel3, 20, "all", entry="positive")
        assert old.rc == 0 and ex.nodes.tobytes() == old.table_bytes() and ex.samples.tobytes() == old.sample_bytes() and c.tobytes() == old.counts.tobytes()


@pytest.mark.parametrize("name", ["terrain_4x100k", "hotspot_150k", "ragged_tiny"])
def test_positive_and_inverse_partition_every_node(built_libs, name):
    """I6 and I7 on the device, against export_octree; the summaries of the two halves add up to the export's."""
    dev, u, pts, box, full = _case(name)
    z0, scale = _bins(box)
    for family, kind in (("planes", "oblique"), ("planes", "box"), ("footprint", "rect"), ("lasso", "half"), ("lasso", "rect_fp")):
        sel3 = ir.selection(family, kind, box)
        for sel, ml in MODES:
            export = dev.export_octree(u, max_level=ml, select=sel)
            pos, inv = Raw(dev, u, sel3, ml, sel, entry="positive"), Raw(dev, u, sel3, ml, sel)
            assert pos.rc == inv.rc == 0 and int(pos.counts["error"]) == int(inv.counts["error"]) == 0
            assert int(pos.counts["numSamples"]) + int(inv.counts["numSamples"]) == export.num_samples, (name, family, kind, sel, ml)
            pn, pp, nn_, ip = pos.nodes(), pos.points(), inv.nodes(), inv.points()
            where = {(int(e["level"]), int(e["X"]), int(e["Y"]), int(e["Z"])): t for t, e in enumerate(pn)}
            assert len(nn_) == export.num_nodes
            for t, e in enumerate(export.nodes):
                a = int(nn_["firstSample"][t])
                parts = [ip[a: a + int(nn_["numSamples"][t])]]
                k = where.get((int(e["level"]), int(e["X"]), int(e["Y"]), int(e["Z"])))
                if k is not None:
                    b = int(pn["firstSample"][k])
                    parts.append(pp[b: b + int(pn["numSamples"][k])])
                both = np.concatenate(parts)
                if len(both) != int(e["numSamples"]) or len(both):
                    c = int(e["firstSample"])
                    rr.assert_same_multiset(both, export.samples[c: c + int(e["numSamples"])], f"{name} {family} {kind} {sel}@{ml}: node {t}")
            # the summaries add up
            a = dev.summarize_region(u, sel3[0], ml, sel, footprint=sel3[1], lasso=sel3[2], z0=z0, scale=scale)
            b = dev.summarize_region(u, sel3[0], ml, sel, footprint=sel3[1], lasso=sel3[2], z0=z0, scale=scale, invert=True)
            whole = dev.summarize_region(u, Region(), ml, sel, z0=z0, scale=scale)
            assert a.num_samples + b.num_samples == whole.num_samples == export.num_samples
            assert np.array_equal(a["histC"] + b["histC"], whole["histC"]), (name, family, kind, sel, ml)
    for sel, ml in MODES:
        export = dev.export_octree(u, max_level=ml, select=sel)
        none = Raw(dev, u, (Region(), None, None), ml, sel)
        assert none.rc == 0 and [int(none.counts[k]) for k in COUNT_FIELDS] == [export.num_nodes, 0, 0, 0, 0, 0]
        t = none.nodes()
        assert not t["numSamples"].any() and not t["firstSample"].any() and none.poison_behind(export.num_nodes, 0)
        for f in ("level", "X", "Y", "Z", "parent", "firstChild", "childMask", "flags"):
            assert np.array_equal(t[f], export.nodes[f]), f
        for family in ir.FAMILIES:
            miss = Raw(dev, u, ir.selection(family, "miss", box), ml, sel)
            assert miss.rc == 0 and int(miss.counts["error"]) == 0 and int(miss.counts["numFilteredNodes"]) == 0
            assert miss.table_bytes() == export.nodes.tobytes() and miss.sample_bytes() == export.samples.tobytes(), (name, family, sel, ml)
            assert miss.poison_behind(export.num_nodes, export.num_samples)


def test_set_without_previous_stores_without_loading(built_libs):
    """SET without `previous`: a COPIED chunk of the inverse (a node the positive query culls) takes the path that stores without a load.  The
    result still equals the mirror, `previous` stays poisoned, and an ARRAY paint of the colours the mirror remembers is the undo."""
    dev, u, pts, box, full = _case("terrain_4x100k")
    rs = np.random.RandomState(3)
    for family, kind in (("planes", "oblique"), ("lasso", "half"), ("footprint", "rect")):
        sel3 = ir.selection(family, kind, box)
        cnt = _mirror(full, sel3, 20, "all")[1]
        assert int(cnt["numCopiedNodes"]) > 0 and int(cnt["numFilteredNodes"]) > 0
        _, _, prev = full.paint(sel3[0], Paint.set(0x11223344), footprint=sel3[1], lasso=sel3[2], return_previous=True, invert=True)
        _paint_and_compare(dev, u, full, Paint.set(0x11223344), sel3, rs, f"{family} {kind}: SET without previous", previous=False)
        raw = RawPaint(dev, u, Paint.array(), sel3, colors=prev)
        assert raw.rc == 0 and int(raw.counts["error"]) == 0
        back = dev.export_octree(u)
        assert back.nodes.tobytes() == full.nodes.tobytes() and back.samples.tobytes() == full.samples.tobytes(), f"{family} {kind}: undo"


def test_count_only_capacities_and_refusals(built_libs):
    dev, u, pts, box, full = _case("uniform_3x40k")
    ok = ir.selection("lasso", "star7", box)
    foot = fr.footprint("rect", box)
    ref = Raw(dev, u, ok)
    nn, ns = int(ref.counts["numNodes"]), int(ref.counts["numSamples"])
    all_nodes = _sizes(dev)[0]
    assert ref.rc == 0 and int(ref.counts["error"]) == 0 and nn == all_nodes and ns > 0
    cnt = Raw(dev, u, ok, count_only=True)
    assert cnt.rc == 0 and cnt.counts.tobytes() == ref.counts.tobytes() and cnt.table_bytes() == ref.table_bytes() and cnt.poison_behind(nn, 0)
    exact = Raw(dev, u, ok, table_cap=nn, sample_cap=ns)
    assert exact.rc == 0 and exact.counts.tobytes() == ref.counts.tobytes()
    assert exact.table_bytes() == ref.table_bytes() and exact.sample_bytes() == ref.sample_bytes() and exact.poison_behind(nn, ns)
    short = Raw(dev, u, ok, table_cap=nn, sample_cap=ns - 1)
    assert short.rc == 0 and int(short.counts["error"]) == abi.EXPORT_ERR_CAPACITY and int(short.counts["numSamples"]) == ns and short.poison_behind(nn, 0)
    small = Raw(dev, u, ok, table_cap=nn - 1, sample_cap=ns)
    assert small.rc == 0 and int(small.counts["error"]) & abi.EXPORT_ERR_CAPACITY and int(small.counts["numNodes"]) <= nn - 1 and small.poison_behind(nn - 1, 0)
    # a scratch buffer with room for the table's part and the polygon but not for the items: the device says so
    need0 = int(dev.L.simlod_inverse_buffer_min_bytes(all_nodes, 0))
    for sel3 in (ok, ir.selection("planes", "oblique", box)):
        items = Raw(dev, u, sel3, scratch_bytes=need0)
        assert items.rc == 0 and int(items.counts["error"]) & abi.EXPORT_ERR_CAPACITY and items.poison_behind(all_nodes, 0)

    image = dev.export_octree(u).samples.tobytes()

    def refused(sel3=ok, **kw):
        raw = Raw(dev, u, sel3, **kw)
        assert raw.rc == 1 and raw.untouched(), kw                                      # hipErrorInvalidValue
        pkw = {k: v for k, v in kw.items() if k in ("fp_record", "lasso_record", "scratch_bytes")}
        if pkw or not kw:
            if "scratch_bytes" in pkw:
                pkw["scratch_bytes"] = int(dev.L.simlod_paint_buffer_min_bytes(all_nodes, 0)) - 1
            p = RawPaint(dev, u, Paint.set(3), sel3, **pkw)
            assert p.rc == 1 and p.untouched(), kw
            if "scratch_bytes" in pkw:
                pkw["scratch_bytes"] = int(dev.L.simlod_summary_buffer_min_bytes(all_nodes, 0)) - 1
            s = RawSummary(dev, u, sel3, **pkw)
            assert s.rc == 1 and s.untouched(), kw

    # a footprint and a lasso together
    refused((Region(), foot, ok[2]))
    # the call's own scratch minimum, with a polygon and without one
    refused(scratch_bytes=need0 - 1)
    refused(ir.selection("planes", "oblique", box), scratch_bytes=need0 - 1)
    # everything the lasso query refuses of the lasso, and the footprint query of the footprint
    for n in (0, 2, 257, 0xFFFFFFFF):
        rec = ok[2].record(); rec["numVertices"] = n
        refused(lasso_record=rec)
        rec = foot.record(); rec["numVertices"] = n
        refused((Region(), foot, None), fp_record=rec)
    for field, at, v in (("vertices", (0, 3, 1), np.nan), ("rowU", (0, 2), np.inf), ("rowW", (0, 0), np.nan)):
        rec = ok[2].record(); rec[field][at] = v
        refused(lasso_record=rec)
    for field, at, v in (("vertices", (0, 1, 0), np.nan), ("axisU", (0, 1), np.inf), ("axisV", (0, 3), np.nan)):
        rec = foot.record(); rec[field][at] = v
        refused((Region(), foot, None), fp_record=rec)
    for k in range(3):
        rec = ok[2].record(); rec["reserved"][0, k] = 1
        refused(lasso_record=rec)
        rec = foot.record(); rec["reserved"][0, k] = 1
        refused((Region(), foot, None), fp_record=rec)
    # everything simlod_query_region refuses
    planes = rr.region("oblique", box)
    rec = planes.record(); rec["numPlanes"] = 17
    refused(region_record=rec)
    rec = planes.record(); rec["planes"][0, 0, 3] = np.nan
    refused(region_record=rec)
    for k in range(3):
        rec = planes.record(); rec["reserved"][0, k] = 1
        refused(region_record=rec)
    refused(null_region=True)
    refused(select=abi.EXPORT_VISIBLE)
    refused(select=abi.EXPORT_REGION)
    assert dev.export_octree(u).samples.tobytes() == image


# ---- erase -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("terrain_4x100k", "oblique"), ("hotspot_150k", "box")])
def test_erase_makes_clip_outside_permanent(built_libs, name, kind):
    """The frame with SIMLOD_CLIP_OUTSIDE set — rule C3: "the frame of the octree image after this edit" — and the frame of the octree after
    erase_region without a clip: the 64-bit framebuffers are equal word for word, plain and HQS.  Then the counts, the export against the mirror's
    inverse, and a second erase."""
    dev, u0, pts, box = _build(name)
    full = dev.export_octree(u0).to("cpu")
    assert full.nodes["childMask"][0] != 0, "the root must be an inner node: a leaf root carries a voxel list the export does not"
    region = rr.region(kind, box)
    T = cases.case(name)[3]
    us = [dev.uniforms(W, H, T, box, hqs=hqs, show_bounding_box=False) for hqs in (False, True)]
    clipped = []
    dev.set_clip(Clip(region, "outside"))
    try:
        for u in us:
            dev.render(u)
            clipped.append(dev.framebuffer(W, H).copy())
    finally:
        dev.set_clip(None)
    dev.render(us[0])
    unclipped = dev.framebuffer(W, H).copy()
    assert not np.array_equal(unclipped, clipped[0]), "the clip must change the frame"
    c = dev.erase_region(us[0], region)
    mirror, cnt = full.crop(region, 20, "all", return_counts=True, invert=True)
    assert [int(c[k]) for k in COUNT_FIELDS] == [int(cnt[k]) for k in COUNT_FIELDS]
    st = dev.read_stats()
    assert int(st["dbg"]) == 0 and int(st["numPoints"]) + int(st["numVoxels"]) == int(c["numSamples"]) and int(st["numNodes"]) == full.num_nodes
    for u, want in zip(us, clipped):
        dev.render(u)
        got = dev.framebuffer(W, H)
        assert int(dev.read_stats()["dbg"]) == 0
        diff = np.nonzero(got != want)[0]
        assert len(diff) == 0, f"{name} {kind} hqs={int(u['useHighQualityShading'])}: {len(diff)} pixels differ from the clipped frame, first {diff[:5]}"
        assert int((got != abi.CLEAR_PIXEL).sum()) > 100
    after = dev.export_octree(us[0]).to("cpu")
    assert after.nodes.tobytes() == mirror.nodes.tobytes() and after.samples.tobytes() == mirror.samples.tobytes()
    # erase once more, with another selection: the mirror of the octree as it is now
    region2, fp2, lasso2 = ir.selection("lasso", "half", box)
    c2 = dev.erase_region(us[0], region2, lasso=lasso2)
    mirror2, cnt2 = after.crop(region2, 20, "all", return_counts=True, lasso=lasso2, invert=True)
    # (on the hotspot the first erase has already taken what the left half of the screen shows: the second may remove nothing more)
    assert [int(c2[k]) for k in COUNT_FIELDS] == [int(cnt2[k]) for k in COUNT_FIELDS] and 0 < int(c2["numSamples"]) <= int(c["numSamples"])
    assert name != "terrain_4x100k" or int(c2["numSamples"]) < int(c["numSamples"])
    twice = dev.export_octree(us[0])
    assert twice.nodes.tobytes() == mirror2.nodes.tobytes() and twice.samples.tobytes() == mirror2.samples.tobytes()
    dev.render(us[0])
    assert int(dev.read_stats()["dbg"]) == 0 and int((dev.framebuffer(W, H) != abi.CLEAR_PIXEL).sum()) > 100
    with pytest.raises(Exception):
        dev.construct(us[0])                    # render-only until a reset


# ---- other octrees -----------------------------------------------------------------------------------------------------------------------
def _one_of_each(dev, u, sel3, what):
    """Query, summary and paint once on the octree of `dev` against the mirror of ITS export."""
    state = dev.export_octree(u).to("cpu")
    box = np.asarray(state.box_max, np.float64) - np.asarray(state.box_min, np.float64)
    mirror, cnt = _mirror(state, sel3, 20, "cut")
    _assert_matches(Raw(dev, u, sel3, 20, "cut"), mirror, cnt, f"{what}: query")
    mirror, cnt = _mirror(state, sel3, 20, "all")
    _assert_matches(Raw(dev, u, sel3, 20, "all"), mirror, cnt, f"{what}: query, all")
    z0, scale = _bins(box, state.box_min)
    _summary_and_compare(dev, u, state, sel3, 20, "cut", z0, scale, f"{what}: summary")
    state, prev = _paint_and_compare(dev, u, state, pf.paints(box, state.box_min)["ramp"], sel3, np.random.RandomState(23), f"{what}: paint")
    assert 0 < len(prev) < state.num_samples, f"{what}: {len(prev)} of {state.num_samples} samples"
    return state


@pytest.mark.parametrize("buildable", [False, True], ids=["render-only", "buildable"])
def test_inverse_on_an_imported_octree(built_libs, buildable):
    src, u, pts, box, full = _case("terrain_4x100k")
    dst = _device()
    dst.nodes.fill_(0xA5)
    if buildable:
        dst.import_octree(full.to("cuda:0"), buildable=True, uniforms=u)
    else:
        dst.import_octree(full.to("cuda:0"))
    assert int(dst.read_stats()["dbg"]) == 0
    for family, kind in (("planes", "oblique"), ("footprint", "rect"), ("lasso", "half")):
        _one_of_each(dst, u, ir.selection(family, kind, box), f"imported (buildable={buildable}) {family} {kind}")
    assert src.export_octree(u).samples.tobytes() == full.samples.tobytes()             # the source was not painted


@pytest.mark.parametrize("name,offset", fr.SHIFTED)
def test_inverse_in_a_box_off_the_origin(built_libs, name, offset):
    off = cases.offset_of(offset, cases.case(name)[1])
    dev, u, pts, box = _build(name, off)
    box_min = dev.export_octree(u).box_min
    assert box_min != (0.0, 0.0, 0.0)
    # (the box, not the slab: the hotspot lies inside the slab whole, and its inverse there is empty)
    for family, kind in (("planes", "box"), ("footprint", "star7"), ("lasso", "half")):
        _one_of_each(dev, u, ir.selection(family, kind, box, box_min), f"{name}@{offset} {family} {kind}")


def test_inverse_on_a_13_deep_octree(built_libs):
    box, batches, counts, origin = dr.d13_input("d13")
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    d = types.SimpleNamespace(name="d13", size=float(max(box)), origin=np.asarray(origin, np.float64))
    full = dev.export_octree(u).to("cpu")
    assert int(full.nodes["level"].max()) == dr.LEAF_LEVEL
    _one_of_each(dev, u, (dr.d13_regions(d)["cell12"], None, None), "d13 cell12 region")
    _one_of_each(dev, u, (Region(), dr.d13_footprints(d)["cell12"], None), "d13 cell12 footprint")
    _one_of_each(dev, u, (Region(), None, Lasso.from_pixels(dr.close_cam(d), W, H, lr.pixels("star7"))), "d13 star7")


def test_inverse_on_a_20_deep_octree(built_libs):
    box, batches, fourth, same = dr.d20_input()
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    full = dev.export_octree(u).to("cpu")
    e, k = dr.deep_entry(full)
    assert int(full.nodes["level"][e]) == abi.MAX_DEPTH and k > 0
    _one_of_each(dev, u, (dr.d20_regions(full)["x>=below"][0], None, None), "d20 x>=below")
    f, keeps = dr.d20_footprints()["lo_x=x"]
    _one_of_each(dev, u, (Region(), f, None), "d20 lo_x=x")
    _one_of_each(dev, u, (Region(), None, Lasso.from_footprint(f)), "d20 lo_x=x as a lasso")
