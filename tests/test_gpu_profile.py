"""GPU tier: simlod_query_profile (include/simlod_hip.h, "profile queries") through the C ABI against the host mirror OctreeExport.profile —
counts, table, samples and records byte for byte, nothing written behind them — and against Profile.locate on the input points; null records,
the null profile against simlod_query_region; count-only calls, capacities, refused arguments; a box off the origin, a 20-deep octree, an
imported octree, and the Python entry points."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import deep_ref as dr
import profile_ref as pr
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Profile, Region
from test_profile_rules import _bad_records
from util import _build, _device, _ingest

pytestmark = pytest.mark.gpu
MODES = [("cut", 20), ("all", 20), ("cut", 2)]
COUNT_FIELDS = list(abi.query_counts_dtype.names)


class Raw:
    """One simlod_query_profile call (entry="region": simlod_query_region) with every buffer poisoned: rc, the counts record, and the buffers as
    the call left them.  profile None: a null pointer."""

    def __init__(self, dev, u, profile, region=None, max_level=20, select="cut", *, table_cap=None, sample_cap=None, count_only=False,
                 scratch_bytes=None, record=None, region_record=None, null_region=False, null_records=False, entry="profile"):
        st = dev.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        self.table_cap = nn if table_cap is None else table_cap
        self.sample_cap = bound if sample_cap is None else sample_cap
        L = dev.L
        need = int(L.simlod_profile_buffer_min_bytes(self.table_cap, bound)) if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        self.scratch, self.table, self.samples, self.records = mk(need), mk((self.table_cap + 4) * 40), mk((self.sample_cap + 1000) * 16), mk((self.sample_cap + 1000) * 16)
        self.counts_t = mk(abi.query_counts_dtype.itemsize)
        uu, up = dev._u(u)
        r = (Region() if region is None else region).record() if region_record is None else region_record
        f = record if record is not None else None if profile is None else profile.record()
        head = (dev._p(dev.nodes), dev._p(dev.stats), up, None if null_region else ctypes.c_void_p(r.ctypes.data))
        mid = (max_level, abi.EXPORT_SELECT[select] if isinstance(select, str) else select, dev._p(self.scratch), ctypes.c_uint64(need),
               dev._p(self.table), self.table_cap, None if count_only else dev._p(self.samples), ctypes.c_uint64(self.sample_cap))
        tail = (dev._p(self.counts_t), dev._stream())
        if entry == "region":
            self.rc = L.simlod_query_region(*head, *mid, *tail)
        else:
            self.rc = L.simlod_query_profile(*head, None if f is None else ctypes.c_void_p(f.ctypes.data), *mid, None if null_records else dev._p(self.records), *tail)
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]

    def table_bytes(self, n=None):
        n = int(self.counts["numNodes"]) if n is None else n
        return self.table[: n * 40].cpu().numpy().tobytes()

    def sample_bytes(self, n=None):
        n = int(self.counts["numSamples"]) if n is None else n
        return self.samples[: n * 16].cpu().numpy().tobytes()

    def record_bytes(self, n=None):
        n = int(self.counts["numSamples"]) if n is None else n
        return self.records[: n * 16].cpu().numpy().tobytes()

    def poison_behind(self, nodes, samples, records=None):
        records = samples if records is None else records
        return bool((self.table[nodes * 40:] == 0xA5).all()) and bool((self.samples[samples * 16:] == 0xA5).all()) and bool((self.records[records * 16:] == 0xA5).all())


def _assert_matches(raw, mirror, rec, cnt, what):
    assert raw.rc == 0, what
    got = {f: int(raw.counts[f]) for f in COUNT_FIELDS}
    assert got == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    assert raw.table_bytes() == mirror.nodes.tobytes(), f"{what}: the table differs"
    assert raw.sample_bytes() == mirror.samples.tobytes(), f"{what}: the samples differ"
    assert raw.record_bytes() == rec.tobytes(), f"{what}: the records differ"
    assert raw.poison_behind(mirror.num_nodes, mirror.num_samples), f"{what}: written past the result"


@pytest.mark.parametrize("name", cases.CASES)
def test_profile_matches_mirror(built_libs, name):
    dev, u, pts, box = _build(name)
    full = dev.export_octree(u)
    profiles = {kind: pr.profile(kind, box) for kind in pr.PROFILE_NAMES}
    want = {(kind, sel, ml): full.profile(f, None, ml, sel, return_counts=True) for kind, f in profiles.items() for sel, ml in MODES}
    for source in ("chunk table", "walk"):
        for (kind, sel, ml), (mirror, rec, cnt) in want.items():
            _assert_matches(Raw(dev, u, profiles[kind], None, ml, sel), mirror, rec, cnt, f"{name} {kind} {sel}@{ml} ({source})")
        dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))        # the builder's chunk table no longer counts: every list is walked
    # the Python entry points: a count-only call, then exact buffers
    f = profiles["zigzag"]
    mirror, rec, cnt = want["zigzag", "cut", 20]
    ex, records, c = dev.query_profile(u, f, return_counts=True)
    assert ex.select == abi.EXPORT_REGION and ex.nodes.tobytes() == mirror.nodes.tobytes() and ex.samples.tobytes() == mirror.samples.tobytes()
    assert records.cpu().numpy().tobytes() == rec.tobytes()
    cc = dev.count_profile(u, f)
    assert [int(cc[k]) for k in COUNT_FIELDS] == [int(c[k]) for k in COUNT_FIELDS] == [int(cnt[k]) for k in COUNT_FIELDS]
    # a leaf-level cut holds every input point once: the result is Profile.locate on the input, as a multiset of (sample, record)
    seg, station, offset, h = f.locate(pts)
    rr.assert_same_multiset(ex.samples, pts[seg >= 0], name)
    got = np.concatenate([ex.samples.view(np.uint32).reshape(-1, 4), records.cpu().numpy().view(np.uint32).reshape(-1, 4)], axis=1)
    ref = np.concatenate([pts[seg >= 0].view(np.uint32).reshape(-1, 4), f.records(pts[seg >= 0]).view(np.uint32).reshape(-1, 4)], axis=1)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    assert np.array_equal(order(got), order(ref)), f"{name}: (sample, record) pairs differ from Profile.locate on the input"


@pytest.fixture(scope="module")
def terrain(built_libs):
    dev, u, pts, box = _build("terrain_4x100k")
    return dev, u, pts, box, dev.export_octree(u)


def test_region_composes_and_null_arguments(terrain):
    dev, u, pts, box, full = terrain
    f = pr.profile("zigzag", box)
    band = Region.from_planes([[0, 0, 1, -12.0], [0, 0, -1, 25.0]])
    for sel, ml in MODES:
        mirror, rec, cnt = full.profile(f, band, ml, sel, return_counts=True)
        assert 0 < mirror.num_samples < full.profile(f, None, ml, sel)[0].num_samples
        a = Raw(dev, u, f, band, ml, sel)
        _assert_matches(a, mirror, rec, cnt, f"zigzag and a height band {sel}@{ml}")
        # records == NULL: the same samples, the records buffer untouched
        b = Raw(dev, u, f, band, ml, sel, null_records=True)
        assert b.rc == 0 and b.counts.tobytes() == a.counts.tobytes() and b.table_bytes() == a.table_bytes() and b.sample_bytes() == a.sample_bytes()
        assert b.poison_behind(mirror.num_nodes, mirror.num_samples, 0), (sel, ml)
    # profile == NULL: simlod_query_region byte for byte, with its scratch bytes, and the records are not written
    for kind in ("oblique", "box", "none"):
        for sel, ml in MODES:
            r = rr.region(kind, box)
            a, b = Raw(dev, u, None, r, ml, sel), Raw(dev, u, None, r, ml, sel, entry="region")
            assert a.rc == b.rc == 0 and a.counts.tobytes() == b.counts.tobytes(), (kind, sel, ml)
            n, s = int(a.counts["numNodes"]), int(a.counts["numSamples"])
            assert a.table_bytes() == b.table_bytes() and a.sample_bytes() == b.sample_bytes() and a.poison_behind(n, s, 0), (kind, sel, ml)
    st = dev.read_stats()
    need = int(dev.L.simlod_query_buffer_min_bytes(int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])))
    assert Raw(dev, u, None, rr.region("oblique", box), scratch_bytes=need).counts.tobytes() == Raw(dev, u, None, rr.region("oblique", box)).counts.tobytes()
    # cover is the plain export, every record in segment 0
    cover = pr.profile("cover", box)
    for sel, ml in MODES:
        raw = Raw(dev, u, cover, None, ml, sel)
        ex = dev.export_octree(u, max_level=ml, select=sel)
        assert raw.rc == 0 and int(raw.counts["error"]) == 0 and int(raw.counts["numFilteredNodes"]) == 0
        assert raw.table_bytes() == ex.nodes.tobytes() and raw.sample_bytes() == ex.samples.tobytes(), (sel, ml)
        assert raw.record_bytes() == cover.records(ex.samples).tobytes() and raw.poison_behind(ex.num_nodes, ex.num_samples)


def test_count_only_and_capacities(terrain):
    dev, u, pts, box, full = terrain
    f = pr.profile("hairpin", box)
    ref = Raw(dev, u, f)
    nn, ns = int(ref.counts["numNodes"]), int(ref.counts["numSamples"])
    assert ref.rc == 0 and int(ref.counts["error"]) == 0 and nn > 1 and ns > 0
    assert int(ref.counts["numCopiedNodes"]) > 0 and int(ref.counts["numFilteredNodes"]) > 0
    cnt = Raw(dev, u, f, count_only=True, null_records=True)
    assert cnt.rc == 0 and cnt.counts.tobytes() == ref.counts.tobytes()
    assert cnt.table_bytes() == ref.table_bytes() and cnt.poison_behind(nn, 0)          # the table is complete, no sample and no record was written
    # exact capacities: the full result
    exact = Raw(dev, u, f, table_cap=nn, sample_cap=ns)
    assert exact.rc == 0 and exact.counts.tobytes() == ref.counts.tobytes()
    assert exact.table_bytes() == ref.table_bytes() and exact.sample_bytes() == ref.sample_bytes() and exact.record_bytes() == ref.record_bytes()
    assert exact.poison_behind(nn, ns)
    # one sample short: the error bit, the counts still say what is needed, no sample and no record is written
    short = Raw(dev, u, f, table_cap=nn, sample_cap=ns - 1)
    assert short.rc == 0 and int(short.counts["error"]) == abi.EXPORT_ERR_CAPACITY and int(short.counts["numSamples"]) == ns
    assert short.poison_behind(nn, 0)
    # one table entry short: the error bit, nothing behind the capacity
    small = Raw(dev, u, f, table_cap=nn - 1, sample_cap=ns)
    assert small.rc == 0 and int(small.counts["error"]) & abi.EXPORT_ERR_CAPACITY and int(small.counts["numNodes"]) <= nn - 1
    assert small.poison_behind(nn - 1, 0)
    # a scratch buffer with room for the table's part and the segments but not for the items: the device says so
    raw = Raw(dev, u, f, table_cap=nn, scratch_bytes=int(dev.L.simlod_profile_buffer_min_bytes(nn, 0)))
    assert raw.rc == 0 and int(raw.counts["error"]) & abi.EXPORT_ERR_CAPACITY and raw.poison_behind(nn, 0)
    assert int(dev.count_profile(u, f)["numSamples"]) == ns


def test_invalid_arguments_enqueue_nothing(built_libs):
    dev, u, pts, box = _build("uniform_3x40k")
    ok = pr.profile("zigzag", box)
    nn = int(dev.read_stats()["numNodes"])

    def refused(**kw):
        raw = Raw(dev, u, kw.pop("profile", ok), **kw)
        assert raw.rc == 1, kw                                                          # hipErrorInvalidValue
        assert bool((raw.counts_t == 0xA5).all()) and raw.poison_behind(0, 0) and bool((raw.scratch == 0xA5).all()), kw

    # the profile's own (rule P6): the records of tests/test_profile_rules.py
    for edit, rec in _bad_records()[1]:
        refused(record=rec)
    refused(count_only=True)                                                             # records without samples
    refused(scratch_bytes=int(dev.L.simlod_profile_buffer_min_bytes(nn, 0)) - 1)
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
    # a vertex beyond numVertices is not looked at
    rec = ok.record(); rec["vertices"][0, len(ok), 0] = np.nan
    assert Raw(dev, u, ok, record=rec).rc == 0


def test_profile_in_a_box_off_the_origin(built_libs):
    """terrain_4x100k at cases.GEOREF, where one fp32 step is 1/32 m in x and 1/2 m in y: input points lie ON the lines of an axis-aligned corridor."""
    dev, u, pts, box = _build("terrain_4x100k", cases.GEOREF)
    box_min = tuple(float(np.float32(v)) for v in cases.GEOREF)
    full = dev.export_octree(u)
    on_lines = Profile.from_xy([(box_min[0] + 100.0, box_min[1] + 200.0), (box_min[0] + 500.0, box_min[1] + 200.0)], 50.0)
    seg, decided = pr.locate_exact(on_lines, pts, return_decided=True)
    assert int(decided.sum()) >= 10 and np.array_equal(seg, on_lines.locate(pts)[0])
    for kind, f in [("on the lines", on_lines)] + [(k, pr.profile(k, box, box_min)) for k in ("zigzag", "oblique", "narrow")]:
        for sel, ml in (("cut", 20), ("all", 20)):
            mirror, rec, cnt = full.profile(f, None, ml, sel, return_counts=True)
            assert mirror.num_samples > 0
            _assert_matches(Raw(dev, u, f, None, ml, sel), mirror, rec, cnt, f"georef {kind} {sel}@{ml}")
    got = Raw(dev, u, on_lines)
    rr.assert_same_multiset(got.samples[: int(got.counts["numSamples"]) * 16].cpu().numpy().view(abi.point_dtype), pts[seg >= 0], "georef, on the lines")


def _d20_profiles():
    """Corridors through the 70 000 identical points of deep_ref's D20 at POINT, narrow against the box: the nodes of the chain of splits that are
    smaller than the corridor are COPIED (a level-18 node, 2^-18 wide and holding the point, lies within 2^-17 of a line through the point; so do
    the nodes below it).  The last corridor ends AT the point (al == L2 for all 70 000): every node of the chain reaches past the end and is
    filtered."""
    x, y = dr.POINT[0], dr.POINT[1]
    return {"w-10": Profile.from_xy([(x - 0.25, y - 0.125), (x + 0.25, y + 0.125)], 2.0 ** -10),
            "w-17 bend": Profile.from_xy([(x - 0.125, y), (x + 2.0 ** -16, y), (x + 2.0 ** -16, y + 0.25)], 2.0 ** -17),
            "ends at the point": Profile.from_xy([(0.125, y), (x, y)], 2.0 ** -12)}


def test_profile_on_a_20_deep_octree(built_libs):
    d = dr.built("d20")
    dev = _device()
    u = dev.uniforms(cases.W, cases.H, cases._cam(d.box), d.box)
    dev.reset(u)
    _ingest(dev, u, d.batches)
    full = dev.export_octree(u)
    assert int(full.nodes["level"].max()) == abi.MAX_DEPTH
    for kind, f in _d20_profiles().items():
        for sel, ml in (("cut", 20), ("all", 20), ("cut", 12)):
            mirror, rec, cnt = full.profile(f, None, ml, sel, return_counts=True)
            if sel == "all":
                deep = mirror.nodes["level"][np.repeat(np.arange(mirror.num_nodes), mirror.nodes["numSamples"].astype(np.int64))]
                assert int(cnt["numFilteredNodes"]) >= 3 and (deep == abi.MAX_DEPTH).sum() >= 70_000, (kind, cnt)
                assert int(cnt["numCopiedNodes"]) >= 3 or kind == "ends at the point", (kind, cnt)
            _assert_matches(Raw(dev, u, f, None, ml, sel), mirror, rec, cnt, f"d20 {kind} {sel}@{ml}")


def test_profile_on_an_imported_octree(built_libs):
    src, u, pts, box = _build("terrain_4x100k")
    f = pr.profile("single", box)
    crop, records = src.query_profile(u, f, select="all")
    crop.validate()
    assert 1 < crop.num_nodes < int(src.read_stats()["numNodes"]) and crop.num_samples > 0
    dst = _device()
    dst.nodes.fill_(0xA5)
    dst.import_octree(crop)
    back = dst.export_octree(u)
    assert back.samples.tobytes() == crop.samples.tobytes()
    for kind, sel, ml in (("hairpin", "cut", 20), ("oblique", "all", 20), ("narrow", "all", 20), ("zigzag", "cut", 2)):
        g = pr.profile(kind, box)
        mirror, rec, mc = back.profile(g, None, ml, sel, return_counts=True)
        assert mirror.num_samples > 0
        _assert_matches(Raw(dst, u, g, None, ml, sel), mirror, rec, mc, f"imported crop, {kind} {sel}@{ml}")
