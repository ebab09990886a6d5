"""GPU tier: simlod_query_lasso, simlod_paint_lasso and simlod_query_summary_lasso (include/simlod_hip.h, "lasso queries") through the C ABI
against the host mirrors OctreeExport.crop / paint / summarize(lasso=), byte for byte, and against a brute-force filter of the input points;
the null lasso against the region query; the lasso of a footprint against the footprint query; count-only calls, capacities, refused
arguments; imported, shifted and deep octrees.  Every buffer a call may write is poisoned first."""
import ctypes
import types

import numpy as np
import pytest
import torch

import cases
import deep_ref as dr
import footprint_ref as fr
import lasso_ref as lr
import paint_ref as pf
import region_ref as rr
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import Lasso, Paint, Region, classify_lasso, classify_nodes
from util import _build, _device, _ingest, assert_frame_equals_oracle, host_image_of

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
MODES = lr.MODES
COUNT_FIELDS = list(abi.query_counts_dtype.names)
NBYTES = abi.summary_dtype.itemsize
POISON = 0xA5A5A5A5
SLACK = 64


def _mk(dev, n):
    return torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)


def _sizes(dev):
    st = dev.read_stats()
    return int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])


class Raw:
    """One simlod_query_lasso call (entry="region": simlod_query_region; "footprint": simlod_query_footprint with `lasso` a Footprint) with
    every buffer poisoned: rc, the counts record, and the buffers as the call left them.  lasso None: a null pointer."""

    def __init__(self, dev, u, lasso, region=None, max_level=20, select="cut", *, table_cap=None, sample_cap=None, count_only=False,
                 scratch_bytes=None, record=None, region_record=None, null_region=False, entry="lasso"):
        nn, bound = _sizes(dev)
        self.table_cap = nn if table_cap is None else table_cap
        self.sample_cap = bound if sample_cap is None else sample_cap
        L = dev.L
        need = int(L.simlod_lasso_buffer_min_bytes(self.table_cap, bound)) if scratch_bytes is None else scratch_bytes
        self.scratch, self.table, self.samples = _mk(dev, need), _mk(dev, (self.table_cap + 4) * 40), _mk(dev, (self.sample_cap + 1000) * 16)
        self.counts_t = _mk(dev, abi.query_counts_dtype.itemsize)
        uu, up = dev._u(u)
        r = (Region() if region is None else region).record() if region_record is None else region_record
        f = record if record is not None else None if lasso is None else lasso.record()
        head = (dev._p(dev.nodes), dev._p(dev.stats), up, None if null_region else ctypes.c_void_p(r.ctypes.data))
        tail = (max_level, abi.EXPORT_SELECT[select] if isinstance(select, str) else select, dev._p(self.scratch), ctypes.c_uint64(need),
                dev._p(self.table), self.table_cap, None if count_only else dev._p(self.samples), ctypes.c_uint64(self.sample_cap),
                dev._p(self.counts_t), dev._stream())
        if entry == "region":
            self.rc = L.simlod_query_region(*head, *tail)
        else:
            call = L.simlod_query_lasso if entry == "lasso" else L.simlod_query_footprint
            self.rc = call(*head, None if f is None else ctypes.c_void_p(f.ctypes.data), *tail)
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]

    def table_bytes(self, n=None):
        n = int(self.counts["numNodes"]) if n is None else n
        return self.table[: n * 40].cpu().numpy().tobytes()

    def sample_bytes(self, n=None):
        n = int(self.counts["numSamples"]) if n is None else n
        return self.samples[: n * 16].cpu().numpy().tobytes()

    def poison_behind(self, nodes, samples):
        return bool((self.table[nodes * 40:] == 0xA5).all()) and bool((self.samples[samples * 16:] == 0xA5).all())


class RawPaint:
    """One simlod_paint_lasso call with every buffer poisoned."""

    def __init__(self, dev, u, paint, region, lasso, *, colors=None, color_cap=None, scratch_bytes=None, record=None):
        nn, bound = _sizes(dev)
        L = dev.L
        need = int(L.simlod_paint_buffer_min_bytes(nn, bound)) if scratch_bytes is None else scratch_bytes
        self.scratch, self.table, self.counts_t = _mk(dev, need), _mk(dev, (nn + SLACK) * 40), _mk(dev, abi.query_counts_dtype.itemsize)
        self.cap = (bound if colors is None else len(colors)) if color_cap is None else color_cap
        self.prev_t = _mk(dev, (self.cap + SLACK) * 4)
        self.col_t = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint32).view(np.uint8)).to(dev.device)
        uu, up = dev._u(u)
        r, p = (Region() if region is None else region).record(), paint.record()
        f = record if record is not None else None if lasso is None else lasso.record()
        self.rc = L.simlod_paint_lasso(dev._p(dev.nodes), dev._p(dev.stats), up, ctypes.c_void_p(r.ctypes.data), None if f is None else ctypes.c_void_p(f.ctypes.data),
                                       ctypes.c_void_p(p.ctypes.data), dev._p(self.scratch), ctypes.c_uint64(need), dev._p(self.table), nn,
                                       None if self.col_t is None else dev._p(self.col_t), dev._p(self.prev_t), ctypes.c_uint64(self.cap), dev._p(self.counts_t),
                                       dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]

    def previous(self, n=None):
        w = self.prev_t.cpu().numpy().view(np.uint32)
        return w if n is None else w[:n]

    def untouched(self):
        return bool((self.counts_t == 0xA5).all()) and bool((self.table == 0xA5).all()) and bool((self.prev_t == 0xA5).all()) and bool((self.scratch == 0xA5).all())


class RawSummary:
    """One simlod_query_summary_lasso call with every buffer poisoned."""

    def __init__(self, dev, u, region, lasso, *, ml=20, sel="all", z0=0.0, scale=1.0, max_wg=0, scratch_bytes=None, record=None):
        nn, bound = _sizes(dev)
        L = dev.L
        need = int(L.simlod_summary_buffer_min_bytes(nn, bound)) if scratch_bytes is None else scratch_bytes
        self.scratch, self.table, self.counts_t = _mk(dev, need), _mk(dev, (nn + SLACK) * 40), _mk(dev, abi.query_counts_dtype.itemsize)
        self.out_t = _mk(dev, NBYTES + SLACK)
        uu, up = dev._u(u)
        r = (Region() if region is None else region).record()
        f = record if record is not None else None if lasso is None else lasso.record()
        p = np.zeros(1, dtype=abi.summary_params_dtype)
        p["z0"], p["scale"], p["maxWorkgroups"] = z0, scale, max_wg
        self.rc = L.simlod_query_summary_lasso(dev._p(dev.nodes), dev._p(dev.stats), up, ctypes.c_void_p(r.ctypes.data),
                                               None if f is None else ctypes.c_void_p(f.ctypes.data), ctypes.c_void_p(p.ctypes.data), ml, abi.EXPORT_SELECT[sel],
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


_BUILT = {}


def _case(name):
    """The case's octree on the device, its full export on the host and the mirror's crops so far, once per module."""
    if name not in _BUILT:
        dev, u, pts, box = _build(name)
        _BUILT[name] = (dev, u, pts, box, dev.export_octree(u).to("cpu"))
    return _BUILT[name]


@pytest.mark.parametrize("cam", lr.CAMERAS)
@pytest.mark.parametrize("name", cases.CASES)
def test_lasso_matches_mirror(built_libs, name, cam):
    """Per case x camera x lasso x MODES, the chunks read from the builder's chunk table: table, samples, counts, nothing behind the result.
    tri has 3 vertices, star128 has 256."""
    dev, u, pts, box, full = _case(name)
    T = lr.transform(cam, box)
    for kind in lr.names_for(name):
        l = lr.lasso(kind, T)
        for sel, ml in MODES:
            mirror, cnt = full.crop(Region(), ml, sel, return_counts=True, lasso=l)
            _assert_matches(Raw(dev, u, l, None, ml, sel), mirror, cnt, f"{name} {cam} {kind} {sel}@{ml}")
            if cam == "away":
                assert mirror.num_nodes == 1 and mirror.num_samples == 0


@pytest.mark.parametrize("name", cases.CASES)
def test_lasso_matches_mirror_by_the_walk_and_python_entry_points(built_libs, name):
    """After simlod_octree_image_replaced every chunk list is walked by `next`; then the Python entry points: a count-only call, exact buffers."""
    dev, u, pts, box = _build(name)
    full = dev.export_octree(u).to("cpu")
    dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))
    T = lr.transform("bird", box)
    for kind in ("star7", "tri", "bowtie"):
        l = lr.lasso(kind, T)
        for sel, ml in MODES:
            mirror, cnt = full.crop(Region(), ml, sel, return_counts=True, lasso=l)
            _assert_matches(Raw(dev, u, l, None, ml, sel), mirror, cnt, f"{name} {kind} {sel}@{ml} (walk)")
    l = lr.lasso("star7", lr.transform("closer", box))
    mirror, cnt = full.crop(Region(), 20, "cut", return_counts=True, lasso=l)
    ex, c = dev.query_region(u, Region(), return_counts=True, lasso=l)
    assert ex.select == abi.EXPORT_REGION and ex.nodes.tobytes() == mirror.nodes.tobytes() and ex.samples.tobytes() == mirror.samples.tobytes()
    cc = dev.count_region(u, Region(), lasso=l)
    assert [int(cc[k]) for k in COUNT_FIELDS] == [int(c[k]) for k in COUNT_FIELDS] == [int(cnt[k]) for k in COUNT_FIELDS]
    inb = lr.inbox(pts, full.box_min, full.box_max)
    got = ex.samples
    rr.assert_same_multiset(got[lr.inbox(got, full.box_min, full.box_max)], pts[l.contains(pts) & inb], name)
    with pytest.raises(ValueError):
        dev.count_region(u, Region(), lasso=l, footprint=fr.footprint("rect", box))
    with pytest.raises(ValueError):
        dev.paint_region(u, Region(), Paint.set(1), lasso=l, footprint=fr.footprint("rect", box))
    with pytest.raises(ValueError):
        dev.summarize_region(u, Region(), lasso=l, footprint=fr.footprint("rect", box))


def test_null_lasso_is_the_region_query_and_a_footprints_lasso_is_the_footprint_query(built_libs):
    dev, u, pts, box, full = _case("terrain_4x100k")
    for kind in ("oblique", "box", "none"):
        for sel, ml in MODES:
            r = rr.region(kind, box)
            a, b = Raw(dev, u, None, r, ml, sel), Raw(dev, u, None, r, ml, sel, entry="region")
            assert a.rc == b.rc == 0 and a.counts.tobytes() == b.counts.tobytes(), (kind, sel, ml)
            n, s = int(a.counts["numNodes"]), int(a.counts["numSamples"])
            assert a.table_bytes() == b.table_bytes() and a.sample_bytes() == b.sample_bytes() and a.poison_behind(n, s), (kind, sel, ml)
    # the null lasso asks for the region query's scratch bytes only
    nn, bound = _sizes(dev)
    need = int(dev.L.simlod_query_buffer_min_bytes(nn, bound))
    assert Raw(dev, u, None, rr.region("oblique", box), scratch_bytes=need).counts.tobytes() == Raw(dev, u, None, rr.region("oblique", box)).counts.tobytes()
    # Lasso.from_footprint: the footprint query's samples, in its order
    for kind in ("star7", "oblique", "rect", "bowtie"):
        f = fr.footprint(kind, box)
        for sel, ml in MODES:
            a, b = Raw(dev, u, Lasso.from_footprint(f), None, ml, sel), Raw(dev, u, f, None, ml, sel, entry="footprint")
            assert a.rc == b.rc == 0 and int(a.counts["numSamples"]) == int(b.counts["numSamples"]) > 0, (kind, sel, ml)
            assert a.sample_bytes() == b.sample_bytes(), (kind, sel, ml)
    # the cover lasso under the bird camera is the export
    cover = lr.lasso("cover", lr.transform("bird", box))
    for sel, ml in MODES:
        raw = Raw(dev, u, cover, None, ml, sel)
        ex = dev.export_octree(u, max_level=ml, select=sel)
        assert raw.rc == 0 and int(raw.counts["error"]) == 0 and int(raw.counts["numFilteredNodes"]) == 0
        assert raw.table_bytes() == ex.nodes.tobytes() and raw.sample_bytes() == ex.samples.tobytes(), (sel, ml)


def test_lasso_inside_the_frustum_and_a_height_slab(built_libs):
    dev, u, pts, box, full = _case("terrain_4x100k")
    T = lr.transform("closer", box)
    l = lr.lasso("star7", T)
    slab = Region.from_box((-1e6, -1e6, 0.35 * box[2]), (1e6, 1e6, 0.6 * box[2]))
    r = Region.from_planes(np.concatenate([Region.from_frustum(T).planes, slab.planes]))
    for sel, ml in MODES:
        mirror, cnt = full.crop(r, ml, sel, return_counts=True, lasso=l)
        _assert_matches(Raw(dev, u, l, r, ml, sel), mirror, cnt, f"frustum + slab + star7 {sel}@{ml}")
    mirror = full.crop(r, 20, "cut", lasso=l)
    both = l.contains(pts) & rr.brute_mask(r, pts)
    assert 0 < both.sum() < min(int(l.contains(pts).sum()), int(rr.brute_mask(r, pts).sum()))
    rr.assert_same_multiset(mirror.samples, pts[both], "frustum + slab + star7")


def test_count_only_capacities_and_refusals(built_libs):
    dev, u, pts, box, full = _case("uniform_3x40k")
    ok = lr.lasso("star7", lr.transform("bird", box))
    ref = Raw(dev, u, ok)
    nn, ns = int(ref.counts["numNodes"]), int(ref.counts["numSamples"])
    assert ref.rc == 0 and int(ref.counts["error"]) == 0 and nn > 1 and ns > 0
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
    all_nodes = _sizes(dev)[0]
    items = Raw(dev, u, ok, scratch_bytes=int(dev.L.simlod_lasso_buffer_min_bytes(all_nodes, 0)))
    assert items.rc == 0 and int(items.counts["error"]) & abi.EXPORT_ERR_CAPACITY and items.poison_behind(all_nodes, 0)

    def bad_records():
        for n in (0, 2, 257, 0xFFFFFFFF):
            rec = ok.record(); rec["numVertices"] = n
            yield rec
        for field, at, v in (("vertices", (0, 3, 1), np.nan), ("vertices", (0, 0, 0), -np.inf), ("rowU", (0, 2), np.inf), ("rowV", (0, 3), np.nan),
                             ("rowW", (0, 0), np.nan), ("rowW", (0, 3), np.inf)):
            rec = ok.record(); rec[field][at] = v
            yield rec
        for k in range(3):
            rec = ok.record(); rec["reserved"][0, k] = 1
            yield rec

    def refused(**kw):
        raw = Raw(dev, u, kw.pop("lasso", ok), **kw)
        assert raw.rc == 1, kw                                                          # hipErrorInvalidValue
        assert bool((raw.counts_t == 0xA5).all()) and raw.poison_behind(0, 0) and bool((raw.scratch == 0xA5).all()), kw

    image = dev.export_octree(u).samples.tobytes()
    for rec in bad_records():
        refused(record=rec)
        p = RawPaint(dev, u, Paint.set(3), None, ok, record=rec)
        assert p.rc == 1 and p.untouched()
        s = RawSummary(dev, u, None, ok, record=rec)
        assert s.rc == 1 and s.untouched()
    refused(scratch_bytes=int(dev.L.simlod_lasso_buffer_min_bytes(all_nodes, 0)) - 1)
    p = RawPaint(dev, u, Paint.set(3), None, ok, scratch_bytes=int(dev.L.simlod_paint_buffer_min_bytes(all_nodes, 0)) - 1)
    assert p.rc == 1 and p.untouched()
    s = RawSummary(dev, u, None, ok, scratch_bytes=int(dev.L.simlod_summary_buffer_min_bytes(all_nodes, 0)) - 1)
    assert s.rc == 1 and s.untouched()
    assert dev.export_octree(u).samples.tobytes() == image
    # everything simlod_query_region refuses
    planes = rr.region("oblique", box)
    rec = planes.record(); rec["numPlanes"] = 17
    refused(region_record=rec)
    rec = planes.record(); rec["planes"][0, 0, 3] = np.nan
    refused(region_record=rec)
    rec = planes.record(); rec["reserved"][0, 2] = 1
    refused(region_record=rec)
    refused(null_region=True)
    refused(select=abi.EXPORT_VISIBLE)
    refused(select=abi.EXPORT_REGION)
    # a vertex beyond numVertices is not looked at; a row W of zeros is legal and selects nothing
    rec = ok.record(); rec["vertices"][0, len(ok), 0] = np.nan
    assert Raw(dev, u, ok, record=rec).counts.tobytes() == ref.counts.tobytes()
    rec = ok.record(); rec["rowW"][0] = 0.0
    zero = Raw(dev, u, ok, record=rec)
    assert zero.rc == 0 and [int(zero.counts[k]) for k in COUNT_FIELDS] == [1, 0, 0, 0, 0, 0]


def _paint_and_compare(dev, u, state, paint, region, lasso, rs, what):
    """One simlod_paint_lasso call against the mirror on `state` -> the mirror's export after the call."""
    n = len(state.crop(region, 20, "all", lasso=lasso, return_index=True)[1])
    colors = rs.randint(0, 1 << 32, n + 5, dtype=np.uint64).astype(np.uint32) if paint.mode == abi.PAINT_ARRAY else None
    want, cnt, prev = state.paint(region, paint, lasso=lasso, colors=colors, return_previous=True)
    raw = RawPaint(dev, u, paint, region, lasso, colors=colors)
    assert raw.rc == 0, what
    assert {f: int(raw.counts[f]) for f in COUNT_FIELDS} == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    assert int(cnt["numSamples"]) == n
    assert bool((raw.table[int(cnt["numNodes"]) * 40:] == 0xA5).all()), f"{what}: the table was written past numNodes"
    assert np.array_equal(raw.previous(n), prev), f"{what}: previous differs"
    assert (raw.previous()[n:] == POISON).all(), f"{what}: previous was written past numSamples"
    got = dev.export_octree(u)
    assert got.nodes.tobytes() == want.nodes.tobytes(), f"{what}: the table of the export moved"
    assert got.samples.tobytes() == want.samples.tobytes(), f"{what}: {int((got.samples['color'] != want.samples['color']).sum())} colours differ from the mirror's"
    return want, prev


def _summary_and_compare(dev, u, state, region, lasso, ml, sel, z0, scale, what, **kw):
    want, cnt = state.summarize(region, ml, sel, lasso=lasso, z0=z0, scale=scale, return_counts=True)
    raw = RawSummary(dev, u, region, lasso, ml=ml, sel=sel, z0=z0, scale=scale, **kw)
    assert raw.rc == 0, what
    assert {f: int(raw.counts[f]) for f in COUNT_FIELDS} == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    n = int(cnt["numNodes"])
    assert raw.table[: n * 40].cpu().numpy().tobytes() == state.crop(Region() if region is None else region, ml, sel, lasso=lasso).nodes.tobytes(), what
    assert bool((raw.table[n * 40:] == 0xA5).all()) and bool((raw.out_t[NBYTES:] == 0xA5).all()), f"{what}: written past the result"
    assert raw.summary_bytes() == want.tobytes(), what
    return want


def _bins(box, box_min=(0, 0, 0)):
    return np.float32(float(box_min[2]) + 0.1 * float(box[2])), np.float32(256.0 / (0.7 * float(box[2])))


@pytest.mark.parametrize("name", ["hotspot_150k", "ragged_tiny"])
def test_paint_and_summary_match_mirror(built_libs, name):
    """SET / BLEND / RAMP / ARRAY one after the other with the mirror following; `previous` comes back and its ARRAY paint restores the octree;
    the frame rendered afterwards is the oracle's frame of that image; the summary of every MODE; grid independence; histC verifies a SET."""
    dev, u, pts, box = _build(name)
    start = dev.export_octree(u).to("cpu")
    rs = np.random.RandomState(17)
    T = lr.transform("bird", box)
    for kind, region in (("star7", Region()), ("bowtie", rr.region("slab", box))):
        l = lr.lasso(kind, T)
        state = start
        undo = []
        for mode in ("set", "blend", "ramp", "array"):
            state, prev = _paint_and_compare(dev, u, state, pf.paints(box)[mode], region, l, rs, f"{name} {kind} {mode}")
            undo.append(prev)
        assert state.samples.tobytes() != start.samples.tobytes()
        # the frame of the painted octree is the oracle's frame of the same image
        dev.render(u)
        nodes, pers, n = host_image_of(dev)
        assert_frame_equals_oracle(dev, nodes, n, u, f"{name} {kind}: the painted frame", 100)
        for prev in reversed(undo):
            raw = RawPaint(dev, u, Paint.array(), region, l, colors=prev)
            assert raw.rc == 0 and int(raw.counts["error"]) == 0
        back = dev.export_octree(u)
        assert back.nodes.tobytes() == start.nodes.tobytes() and back.samples.tobytes() == start.samples.tobytes(), f"{name} {kind}: undo"
        z0, scale = _bins(box)
        for sel, ml in MODES:
            want = _summary_and_compare(dev, u, start, region, l, ml, sel, z0, scale, f"{name} {kind} summary {sel}@{ml}")
        for wg in (1, 3, 64):
            _summary_and_compare(dev, u, start, region, l, 20, "cut", z0, scale, f"{name} {kind} summary, {wg} workgroups", max_wg=wg)
    # histC of a SET paint verifies that paint
    l = lr.lasso("star7", T)
    colour = 0x7B2D9E41
    c = dev.paint_region(u, Region(), Paint.set(colour), lasso=l)
    s = dev.summarize_region(u, Region(), 20, "all", lasso=l)
    n = int(c["numSamples"])
    assert n > 0 and s.num_samples == n and all(int(s["histC"][k][(colour >> (8 * k)) & 255]) == n for k in range(4))
    want, cnt = start.paint(Region(), Paint.set(colour), lasso=l)
    assert dev.export_octree(u).samples.tobytes() == want.samples.tobytes() and int(cnt["numSamples"]) == n


def _one_of_each(dev, u, lasso, region, what):
    """Query, paint and summary once on the octree of `dev` against the mirror of ITS export."""
    state = dev.export_octree(u).to("cpu")
    box = np.asarray(state.box_max, np.float64) - np.asarray(state.box_min, np.float64)
    mirror, cnt = state.crop(region, 20, "cut", return_counts=True, lasso=lasso)
    _assert_matches(Raw(dev, u, lasso, region, 20, "cut"), mirror, cnt, f"{what}: query")
    z0, scale = _bins(box, state.box_min)
    _summary_and_compare(dev, u, state, region, lasso, 20, "cut", z0, scale, f"{what}: summary")
    state, prev = _paint_and_compare(dev, u, state, pf.paints(box, state.box_min)["ramp"], region, lasso, np.random.RandomState(23), f"{what}: paint")
    n = len(prev)
    assert 0 < n < state.num_samples, f"{what}: {n} of {state.num_samples} samples"
    return state


@pytest.mark.parametrize("buildable", [False, True], ids=["render-only", "buildable"])
def test_lasso_on_an_imported_octree(built_libs, buildable):
    src, u, pts, box, full = _case("terrain_4x100k")
    dst = _device()
    dst.nodes.fill_(0xA5)
    if buildable:
        dst.import_octree(full.to("cuda:0"), buildable=True, uniforms=u)
    else:
        dst.import_octree(full.to("cuda:0"))
    assert int(dst.read_stats()["dbg"]) == 0
    _one_of_each(dst, u, lr.lasso("star7", lr.transform("closer", box)), rr.region("slab", box), f"imported (buildable={buildable})")
    assert src.export_octree(u).samples.tobytes() == full.samples.tobytes()             # the source was not painted


def test_lasso_in_a_box_off_the_origin(built_libs):
    name, offset = "terrain_4x100k", "georef"
    off = cases.offset_of(offset, cases.case(name)[1])
    dev, u, pts, box = _build(name, off)
    box_min = dev.export_octree(u).box_min
    assert box_min != (0.0, 0.0, 0.0)
    l = lr.lasso("star7", lr.transform("closer", box, off))
    state = _one_of_each(dev, u, l, rr.region("slab", box, box_min), f"{name}@{offset}")
    # the brute-force filter of the contract's input points
    got = state.crop(Region(), 20, "cut", lasso=l).samples
    inb = lr.inbox(pts, state.box_min, state.box_max)
    g, w = got[lr.inbox(got, state.box_min, state.box_max)], pts[l.contains(pts) & inb]
    assert len(g) == len(w) and np.array_equal(rr.sorted_samples(g)[:, 0], rr.sorted_samples(w)[:, 0])      # (positions: the colours were painted)


def test_lasso_on_a_13_deep_octree(built_libs):
    box, batches, counts, origin = dr.d13_input("d13")
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    d = types.SimpleNamespace(name="d13", size=float(max(box)), origin=np.asarray(origin, np.float64))
    full = dev.export_octree(u).to("cpu")
    assert int(full.nodes["level"].max()) == dr.LEAF_LEVEL
    l = Lasso.from_pixels(dr.close_cam(d), W, H, lr.pixels("star7"))
    outside, copied = classify_lasso(l, full.nodes, full.box_min, full.box_max)
    deep = (full.nodes["level"] == dr.LEAF_LEVEL) & (full.nodes["numSamples"] != 0)
    assert (deep & ~outside & ~copied).any(), "no filtered node at level 13"
    _one_of_each(dev, u, l, Region(), "d13 star7")


def test_lasso_on_a_20_deep_octree(built_libs):
    box, batches, fourth, same = dr.d20_input()
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    full = dev.export_octree(u).to("cpu")
    e, k = dr.deep_entry(full)
    assert int(full.nodes["level"][e]) == abi.MAX_DEPTH and k > 0
    f, keeps = dr.d20_footprints()["lo_x=x"]
    _one_of_each(dev, u, Lasso.from_footprint(f), Region(), "d20 lo_x=x as a lasso")
    _one_of_each(dev, u, lr.lasso("star7", lr.transform("closer", box)), Region(), "d20 star7")


@pytest.fixture(scope="module")
def terrain3m(built_libs):
    t = fr.TERRAIN_3M
    pts, box = synthetic.terrain(t["n"], seed=t["seed"], box=t["box"], tile=t["tile"])
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, [pts[i:i + 1_000_000] for i in range(0, len(pts), 1_000_000)])
    return dev, u, pts, box, dev.export_octree(u).to("cpu")


def test_terrain_lasso_is_not_vacuous(terrain3m):
    """The 3 M-point terrain under the `closer` camera with a lasso around the screen centre: copied and filtered nodes, a pruned table, some
    but not all candidates; the device equals the mirror byte for byte and the input's brute-force filter as a multiset."""
    dev, u, pts, box, full = terrain3m
    l = Lasso.from_pixels(lr.transform("closer", box), W, H, fr.star(128, 128, 90, 45, 7))
    mirror, cnt = full.crop(Region(), 20, "cut", return_counts=True, lasso=l)
    print({k: int(cnt[k]) for k in COUNT_FIELDS}, "of", full.num_nodes, "nodes")
    assert int(cnt["numCopiedNodes"]) > 0 and int(cnt["numFilteredNodes"]) > 0 and int(cnt["numNodes"]) < full.num_nodes
    assert 0 < int(cnt["numSamples"]) < int(cnt["numCandidates"])
    raw = Raw(dev, u, l, None, 20, "cut")
    _assert_matches(raw, mirror, cnt, "3 M terrain, star")
    inb = lr.inbox(pts, full.box_min, full.box_max)
    got = mirror.samples
    rr.assert_same_multiset(got[lr.inbox(got, full.box_min, full.box_max)], pts[l.contains(pts) & inb], "3 M terrain, star")
    mirror, cnt = full.crop(Region(), 20, "all", return_counts=True, lasso=l)
    _assert_matches(Raw(dev, u, l, None, 20, "all"), mirror, cnt, "3 M terrain, star, all")
