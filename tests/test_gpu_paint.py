"""GPU tier: simlod_paint_region (include/simlod_hip.h, "paint regions") through the C ABI against the host mirror OctreeExport.paint on the
device's own export, byte for byte: every mode, region and footprint with the chunk table and without it; undo; what a paint leaves alone; a
painted octree's frame against the SIMLOD_CLIP_HIGHLIGHT frame; capacities and refused arguments; later ingest; imported, shifted and deep
octrees.  Every octree here is built by the test that paints it."""
import ctypes
import types

import numpy as np
import pytest
import torch

import cases
import deep_ref as dr
import footprint_ref as fr
import paint_ref as pf
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Clip, Paint, Region, classify_footprint, classify_nodes
from util import _build, _device, _ingest

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
COUNT_FIELDS = list(abi.query_counts_dtype.names)
MODES = ["set", "blend", "ramp", "array"]
# every region kind without a footprint; a convex (rect) and a non-convex (star7) footprint alone; the non-convex one with planes
COMBOS = [(k, None) for k in rr.REGION_NAMES] + [("none", "rect"), ("none", "star7"), ("slab", "star7")]
POISON = 0xA5A5A5A5
SLACK = 64                                    # words of `previous` behind colorCapacity, table entries behind tableCapacity


class Raw:
    """One simlod_paint_region call with every buffer poisoned: rc, the counts record and the buffers as the call left them.  colors: uint32
    words (numpy) or None; previous=False: a null pointer; color_cap: colorCapacity (default: what the arrays hold)."""

    def __init__(self, dev, u, paint, region=None, footprint=None, *, colors=None, previous=True, color_cap=None, table_cap=None, scratch_bytes=None,
                 record=None, region_record=None, foot_record=None, null=()):
        st = dev.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        self.table_cap = nn if table_cap is None else table_cap
        L = dev.L
        need = int(L.simlod_paint_buffer_min_bytes(self.table_cap, bound)) if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        self.scratch, self.table, self.counts_t = mk(need), mk((self.table_cap + SLACK) * 40), mk(abi.query_counts_dtype.itemsize)
        self.cap = (bound if colors is None else len(colors)) if color_cap is None else color_cap
        self.prev_t = mk((self.cap + SLACK) * 4) if previous else None
        self.col_t = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint32).view(np.uint8)).to(dev.device)
        uu, up = dev._u(u)
        r = (Region() if region is None else region).record() if region_record is None else region_record
        f = foot_record if foot_record is not None else None if footprint is None else footprint.record()
        p = paint.record() if record is None else record
        ptr = lambda name, a: None if name in null or a is None else ctypes.c_void_p(a.ctypes.data)
        dp = lambda name, t: None if name in null or t is None else dev._p(t)
        self.rc = L.simlod_paint_region(dp("nodes", dev.nodes), dp("stats", dev.stats), None if "uniforms" in null else up, ptr("region", r), ptr("footprint", f),
                                        ptr("paint", p), dp("scratch", self.scratch), ctypes.c_uint64(need), dp("table", self.table), self.table_cap,
                                        dp("colors", self.col_t), dp("previous", self.prev_t), ctypes.c_uint64(self.cap), dp("counts", self.counts_t), dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]

    def table_bytes(self, n):
        return self.table[: n * 40].cpu().numpy().tobytes()

    def previous(self, n=None):
        w = self.prev_t.cpu().numpy().view(np.uint32)
        return w if n is None else w[:n]

    def untouched(self):
        """Nothing but the scratch buffer was written."""
        return bool((self.counts_t == 0xA5).all()) and bool((self.table == 0xA5).all()) and (self.prev_t is None or bool((self.prev_t == 0xA5).all()))


def _count_only(dev, u, region, footprint):
    """The table and the counts of the count-only simlod_query_footprint(region, footprint, 20, ALL) call."""
    nn = int(dev.read_stats()["numNodes"])
    table = dev._table(nn)
    c = dev._query(u, Region() if region is None else region, 20, abi.EXPORT_ALL, table, None, 0, int(dev.read_stats()["numPoints"]) + int(dev.read_stats()["numVoxels"]), footprint)
    return table[: int(c["numNodes"]) * 40].cpu().numpy().tobytes(), c


def _classes(full, region, footprint):
    """What the mirror's classification makes of the nodes the query lists: (filtered nodes, copied nodes, filtered chunks with fewer than 64
    samples, filtered chunks with exactly 1 000 samples), each with samples."""
    crop = full.crop(region, 20, "all", footprint=footprint)
    key = lambda a: list(zip(a["level"].tolist(), a["X"].tolist(), a["Y"].tolist(), a["Z"].tolist()))
    src = {k: i for i, k in enumerate(key(full.nodes))}
    t = full.nodes[np.array([src[k] for k in key(crop.nodes)])]
    out, ins = classify_nodes(region.planes.astype(np.float64), t, full.box_min, full.box_max)
    if footprint is not None:
        near, corner = classify_footprint(footprint, t, full.box_min, full.box_max)
        out, ins = out | (~near & ~corner), ins & ~near & corner
    ns = t["numSamples"].astype(np.int64)
    filtered, copied = ~out & ~ins & (ns > 0), ins & (ns > 0)
    tail = ns % abi.POINTS_PER_CHUNK
    return int(filtered.sum()), int(copied.sum()), int((filtered & (tail > 0) & (tail < 64)).sum()), int((filtered & (ns >= abi.POINTS_PER_CHUNK)).sum())


def _image(dev):
    """(the Node array, Stats, the persistent buffer as far as it is allocated) as bytes"""
    st = dev.read_stats()
    return (dev.nodes[: int(st["numNodes"]) * abi.node_dtype.itemsize].cpu().numpy().tobytes(), dev.stats.cpu().numpy().tobytes(),
            dev.persistent[: int(st["allocatedBytes_persistent"])].cpu().numpy().tobytes())


def _same_positions(a, b):
    return a.nodes.tobytes() == b.nodes.tobytes() and all(a.samples[k].tobytes() == b.samples[k].tobytes() for k in ("x", "y", "z"))


def _paint_and_compare(dev, u, state, paint, region, footprint, rs, what, check_table=True):
    """One call against the mirror on `state` (the octree's export as the mirror has it) -> the mirror's export after the call."""
    n = len(state.crop(region, 20, "all", footprint=footprint, return_index=True)[1])
    colors = rs.randint(0, 1 << 32, n + 5, dtype=np.uint64).astype(np.uint32) if paint.mode == abi.PAINT_ARRAY else None
    want, cnt, prev = state.paint(region, paint, footprint=footprint, colors=colors, return_previous=True)
    if check_table:
        qtable, qc = _count_only(dev, u, region, footprint)
    raw = Raw(dev, u, paint, region, footprint, colors=colors)
    assert raw.rc == 0, what
    assert {f: int(raw.counts[f]) for f in COUNT_FIELDS} == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    assert int(cnt["numSamples"]) == n
    if check_table:
        assert raw.counts.tobytes() == qc.tobytes() and raw.table_bytes(int(qc["numNodes"])) == qtable, f"{what}: not the count-only query's table"
    assert bool((raw.table[int(cnt["numNodes"]) * 40:] == 0xA5).all()), f"{what}: the table was written past numNodes"
    assert np.array_equal(raw.previous(n), prev), f"{what}: previous differs"
    assert (raw.previous()[n:] == POISON).all(), f"{what}: previous was written past numSamples"
    got = dev.export_octree(u)
    assert got.nodes.tobytes() == want.nodes.tobytes(), f"{what}: the table of the export moved"
    assert got.samples.tobytes() == want.samples.tobytes(), f"{what}: {int((got.samples['color'] != want.samples['color']).sum())} colours differ from the mirror's"
    return want


@pytest.mark.parametrize("source", ["chunk table", "walk"])
@pytest.mark.parametrize("name", ["hotspot_150k", "ragged_tiny"])
def test_paint_matches_mirror(built_libs, name, source):
    """Every mode x every combination of COMBOS, one call after the other on one octree, the mirror following on the host: after each call the
    full export, the call's table and counts and `previous` are the mirror's.  source "walk": the builder's chunk table is dropped first."""
    dev, u, pts, box = _build(name)
    if source == "walk":
        dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))
    state = dev.export_octree(u).to("cpu")
    rs = np.random.RandomState(17)
    seen = np.zeros(4, np.int64)
    for rk, fk in COMBOS:
        r, f = rr.region(rk, box), None if fk is None else fr.footprint(fk, box)
        cl = _classes(state, r, f)
        seen += cl
        if name == "hotspot_150k" and (rk, fk) in (("box", None), ("none", "rect")):
            assert min(cl) >= 1, f"{rk} {fk}: (filtered, copied, short filtered chunks, full filtered chunks) = {cl}"
        for mode in MODES:
            state = _paint_and_compare(dev, u, state, pf.paints(box)[mode], r, f, rs, f"{name} {rk} {fk} {mode} ({source})", check_table=mode == "set")
    assert (seen[[0, 1, 3]] >= 1).all() and (seen[2] >= 1 or name != "hotspot_150k"), seen


def test_python_entry_point_and_undo(built_libs):
    """DeviceOctree.paint_region: SET with return_previous, then ARRAY with those colours — the export, the Node array, Stats and every
    allocated byte of the persistent buffer are what they were before the first call."""
    dev, u, pts, box = _build("uniform_3x40k")
    before, image = dev.export_octree(u).to("cpu"), _image(dev)
    r, f = rr.region("slab", box), fr.footprint("star7", box)
    want, cnt, wprev = before.paint(r, Paint.set(0x01C0FFEE), footprint=f, return_previous=True)
    c, prev = dev.paint_region(u, r, Paint.set(0x01C0FFEE), footprint=f, return_previous=True)
    assert [int(c[k]) for k in COUNT_FIELDS] == [int(cnt[k]) for k in COUNT_FIELDS] and 0 < int(c["numSamples"]) < before.num_samples
    assert np.array_equal(prev.cpu().numpy().view(np.uint32), wprev)
    after = dev.export_octree(u)
    assert after.samples.tobytes() == want.samples.tobytes() != before.samples.tobytes() and after.nodes.tobytes() == before.nodes.tobytes()
    nodes, stats, pers = _image(dev)
    assert nodes == image[0] and stats == image[1] and pers != image[2]
    c2 = dev.paint_region(u, r, Paint.array(), footprint=f, colors=prev)
    assert [int(c2[k]) for k in COUNT_FIELDS] == [int(c[k]) for k in COUNT_FIELDS]
    back = dev.export_octree(u)
    assert back.nodes.tobytes() == before.nodes.tobytes() and back.samples.tobytes() == before.samples.tobytes()
    assert _image(dev) == image
    # colours as numpy words, and without previous
    dev.paint_region(u, r, Paint.array(), footprint=f, colors=np.full(int(c["numSamples"]), 0x01C0FFEE, np.uint32))
    assert dev.export_octree(u).samples.tobytes() == want.samples.tobytes()
    with pytest.raises(ValueError):
        dev.paint_region(u, r, Paint.array(), footprint=f)


def test_only_colours_move(built_libs):
    dev, u, pts, box = _build("terrain_4x100k")
    before, image = dev.export_octree(u).to("cpu"), _image(dev)
    r = rr.region("oblique", box)
    dev.paint_region(u, r, Paint.blend(0x00FF2010, 200))
    after = dev.export_octree(u)
    nodes, stats, pers = _image(dev)
    assert nodes == image[0] and stats == image[1]
    assert _same_positions(after, before)
    changed = after.samples["color"] != before.samples["color"]
    assert 0 < int(changed.sum()) < before.num_samples
    assert (after.samples["color"] >> 24 == before.samples["color"] >> 24).all()             # byte 3 is kept
    assert after.samples.tobytes() == before.paint(r, Paint.blend(0x00FF2010, 200))[0].samples.tobytes()
    # of the persistent buffer only colour words differ: the fourth word of a 16-byte record
    a, b = np.frombuffer(pers, np.uint32), np.frombuffer(image[2], np.uint32)
    at = np.nonzero(a != b)[0]
    assert len(at) == int(changed.sum()) and (at % 4 == 3).all()


def test_painted_frame_is_the_highlight_frame(built_libs):
    """Rule C3: the HIGHLIGHT frame of the unpainted octree is the unclipped frame of the SET-painted one, pre-EDL framebuffer bit for bit."""
    dev, u, pts, box = _build("uniform_3x40k")
    r, colour = rr.region("oblique", box), 0xFF00C8FA
    dev.render(u)
    plain = dev.framebuffer(W, H).copy()
    dev.set_clip(Clip(r, "highlight", colour))
    try:
        dev.render(u)
        lit = dev.framebuffer(W, H).copy()
    finally:
        dev.set_clip(None)
    assert int((lit != plain).sum()) > 100, "the highlight changes nothing: the comparison would pass on anything"
    torch.cuda.synchronize()
    dev.paint_region(u, r, Paint.set(colour))
    dev.render(u)
    painted = dev.framebuffer(W, H).copy()
    diff = np.nonzero(painted != lit)[0]
    assert len(diff) == 0, f"{len(diff)} pixels differ, first {diff[:5]}"


def test_all_or_nothing_and_refusals(built_libs):
    dev, u, pts, box = _build("uniform_3x40k")
    before = dev.export_octree(u).to("cpu")
    r, f = rr.region("box", box), fr.footprint("star7", box)
    nn = int(dev.read_stats()["numNodes"])
    n = int(before.crop(r, 20, "all", return_counts=True, footprint=f)[1]["numSamples"])
    assert n > 1000

    def unchanged():
        ex = dev.export_octree(u)
        return ex.nodes.tobytes() == before.nodes.tobytes() and ex.samples.tobytes() == before.samples.tobytes()

    # rule E5: one word short, with previous, with colors, with both
    for kw in (dict(), dict(colors=np.zeros(n - 1, np.uint32), previous=False), dict(colors=np.zeros(n - 1, np.uint32))):
        mode = Paint.array() if "colors" in kw else Paint.set(3)
        raw = Raw(dev, u, mode, r, f, color_cap=n - 1, **kw)
        assert raw.rc == 0 and int(raw.counts["error"]) == abi.EXPORT_ERR_CAPACITY and int(raw.counts["numSamples"]) == n, kw
        assert (raw.prev_t is None or bool((raw.prev_t == 0xA5).all())) and unchanged(), kw
    # ... a table or a scratch buffer too small
    raw = Raw(dev, u, Paint.set(3), r, f, table_cap=nn - 1)
    assert raw.rc == 0 and int(raw.counts["error"]) & abi.EXPORT_ERR_CAPACITY and bool((raw.prev_t == 0xA5).all()) and unchanged()
    assert bool((raw.table[(nn - 1) * 40:] == 0xA5).all())
    raw = Raw(dev, u, Paint.set(3), r, f, scratch_bytes=int(dev.L.simlod_paint_buffer_min_bytes(nn, 0)))
    assert raw.rc == 0 and int(raw.counts["error"]) & abi.EXPORT_ERR_CAPACITY and bool((raw.prev_t == 0xA5).all()) and unchanged()
    # colorCapacity is ignored without arrays
    raw = Raw(dev, u, Paint.set(before.samples["color"][0]), rr.region("miss", box), None, previous=False, color_cap=0)
    assert raw.rc == 0 and int(raw.counts["error"]) == 0 and int(raw.counts["numSamples"]) == 0 and unchanged()

    # rule E9
    def refused(paint=Paint.set(3), **kw):
        raw = Raw(dev, u, paint, kw.pop("region", r), kw.pop("footprint", f), **kw)
        assert raw.rc == 1, kw                                                          # hipErrorInvalidValue
        assert raw.untouched() and bool((raw.scratch == 0xA5).all()), kw

    for mode in (4, 0xFFFFFFFF):
        rec = Paint.set(3).record(); rec["mode"] = mode
        refused(record=rec)
    for field, k in (("reserved", None), ("reserved2", 0), ("reserved2", 1)):
        rec = Paint.ramp(0, 1, pf.ramp_table()).record()
        if k is None:
            rec[field] = 1
        else:
            rec[field][0, k] = 1
        refused(record=rec)
    for s in (0, 256):
        rec = Paint.blend(3, 5).record(); rec["strength"] = s
        refused(record=rec)
    for z0, scale in ((0.0, 0.0), (0.0, -2.0), (0.0, np.nan), (0.0, np.inf), (np.nan, 1.0), (-np.inf, 1.0)):
        rec = Paint.ramp(0, 1, pf.ramp_table()).record(); rec["z0"], rec["scale"] = z0, scale
        refused(record=rec)
    refused(Paint.array())                                                              # ARRAY without colors
    refused(null=("paint",))
    refused(scratch_bytes=int(dev.L.simlod_paint_buffer_min_bytes(nn, 0)) - 1)
    # everything simlod_query_footprint refuses
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
    assert unchanged()
    # fields a mode does not use are ignored
    rec = Paint.set(before.samples["color"][0]).record(); rec["strength"], rec["scale"] = 999, np.nan
    assert Raw(dev, u, None, rr.region("miss", box), record=rec).rc == 0 and unchanged()


def test_painted_points_keep_their_colour_through_later_ingest(built_libs):
    """Rule E7: everything painted with a colour no input carries, then batches that split leaves: in the final export the leaf points with
    that colour number exactly the points ingested before the paint."""
    name, colour = "terrain_4x100k", 0x7E57C0DE
    pts, box, batch, T = cases.case(name)
    assert not (pts["color"] == colour).any()
    dev = _device()
    u = dev.uniforms(W, H, T, box)
    dev.reset(u)
    batches = cases.batches_of(name, pts, batch)
    _ingest(dev, u, batches[:2])
    early = sum(len(b) for b in batches[:2])
    st = dev.read_stats()
    assert int(st["numPoints"]) == early
    torch.cuda.synchronize()
    c = dev.paint_region(u, Region(), Paint.set(colour))
    assert int(c["numSamples"]) == int(st["numPoints"]) + int(st["numVoxels"]) and int(c["numFilteredNodes"]) == 0
    mid = dev.export_octree(u)
    assert (mid.samples["color"] == colour).all()
    _ingest(dev, u, batches[2:])
    st2 = dev.read_stats()
    assert int(st2["numLeaves"]) > int(st["numLeaves"]) and int(st2["numPoints"]) == len(pts), "the later batches split no leaf"
    ex = dev.export_octree(u)
    leaf = np.repeat((ex.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0, ex.nodes["numSamples"].astype(np.int64))
    assert int(leaf.sum()) == len(pts)
    assert int((ex.samples["color"][leaf] == colour).sum()) == early
    # the painted points are the early points: the same positions
    def positions(p):
        w = np.stack([p[a].view(np.uint32) for a in ("x", "y", "z")], axis=1)
        return w[np.lexsort(w.T)]
    assert np.array_equal(positions(ex.samples[leaf & (ex.samples["color"] == colour)]), positions(np.concatenate(batches[:2])))


def _one_call(dev, u, region, footprint, what, modes=("ramp", "blend")):
    state = dev.export_octree(u).to("cpu")
    box = np.asarray(state.box_max, np.float64) - np.asarray(state.box_min, np.float64)
    rs = np.random.RandomState(23)
    n = 0
    for mode in modes:
        state = _paint_and_compare(dev, u, state, pf.paints(box, state.box_min)[mode], region, footprint, rs, f"{what} {mode}")
        n = int(state.crop(region, 20, "all", return_counts=True, footprint=footprint)[1]["numSamples"])
    assert 0 < n < state.num_samples, what
    return state


@pytest.mark.parametrize("buildable", [False, True], ids=["render-only", "buildable"])
def test_paint_an_imported_octree(built_libs, buildable):
    src, u, pts, box = _build("terrain_4x100k")
    ex = src.export_octree(u)
    dst = _device()
    dst.nodes.fill_(0xA5)
    if buildable:
        dst.import_octree(ex, buildable=True, uniforms=u)
    else:
        dst.import_octree(ex)
    assert int(dst.read_stats()["dbg"]) == 0
    _one_call(dst, u, rr.region("slab", box), fr.footprint("star7", box), f"imported (buildable={buildable})")
    # the source was not painted
    assert src.export_octree(u).samples.tobytes() == ex.samples.tobytes()


def test_paint_in_a_box_off_the_origin(built_libs):
    name, offset = "terrain_4x100k", "georef"
    dev, u, pts, box = _build(name, cases.offset_of(offset, cases.case(name)[1]))
    box_min = dev.export_octree(u).box_min
    assert box_min != (0.0, 0.0, 0.0)
    _one_call(dev, u, rr.region("slab", box, box_min), fr.footprint("star7", box, box_min), f"{name}@{offset}", modes=("ramp", "array"))


def test_paint_a_13_deep_octree(built_libs):
    box, batches, counts, origin = dr.d13_input("d13")
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    d = types.SimpleNamespace(name="d13", size=float(max(box)), origin=np.asarray(origin, np.float64))
    full = dev.export_octree(u)
    assert int(full.nodes["level"].max()) == dr.LEAF_LEVEL
    state = _one_call(dev, u, dr.d13_regions(d)["slab"], dr.d13_footprints(d)["star7"], "d13 slab star7", modes=("set", "array"))
    cl = _classes(state, dr.d13_regions(d)["cell12"], None)
    assert cl[0] >= 1 and cl[1] >= 1, cl
    _one_call(dev, u, dr.d13_regions(d)["cell12"], None, "d13 cell12", modes=("blend",))


def test_paint_a_20_deep_octree(built_libs):
    box, batches, fourth, same = dr.d20_input()
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    full = dev.export_octree(u).to("cpu")
    e, k = dr.deep_entry(full)
    assert int(full.nodes["level"][e]) == abi.MAX_DEPTH and k > 0
    region, keeps = dr.d20_regions(full)["cell20"]
    state = _one_call(dev, u, region, None, "d20 cell20", modes=("set",))
    first = int(state.nodes["firstSample"][e])
    assert (state.samples["color"][first: first + k] == pf.paints(box)["set"].color).all()
    f, keeps = dr.d20_footprints()["lo_x=x"]
    _one_call(dev, u, Region(), f, "d20 lo_x=x", modes=("ramp",))
