"""GPU tier: simlod_query_footprint (include/simlod_hip.h, "footprint queries") through the C ABI against the host mirror
OctreeExport.crop(footprint=), byte for byte, and against a brute-force filter of the input points; the null footprint against
simlod_query_region; count-only calls, capacities, refused arguments, and the result as an octree."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import footprint_ref as fr
import oracle
import region_ref as rr
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import Region
from util import STATS_BUILD_FIELDS, _build, _device, _ingest, assert_dumps_equal, assert_stats_equal, host_image_of

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
MODES = [("cut", 20), ("all", 20), ("cut", 2)]
COUNT_FIELDS = list(abi.query_counts_dtype.names)
SLAB_3M = [[0.6, 0.8, 0.1, -342.0 + 120.0], [-0.6, -0.8, -0.1, 342.0 + 120.0]]


class Raw:
    """One simlod_query_footprint call (entry="region": simlod_query_region) with every buffer poisoned: rc, the counts record, and the
    buffers as the call left them.  footprint None: a null pointer."""

    def __init__(self, dev, u, footprint, region=None, max_level=20, select="cut", *, table_cap=None, sample_cap=None, count_only=False,
                 scratch_bytes=None, record=None, region_record=None, null_region=False, entry="footprint"):
        st = dev.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        self.table_cap = nn if table_cap is None else table_cap
        self.sample_cap = bound if sample_cap is None else sample_cap
        L = dev.L
        need = int(L.simlod_footprint_buffer_min_bytes(self.table_cap, bound)) if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        self.scratch, self.table, self.samples = mk(need), mk((self.table_cap + 4) * 40), mk((self.sample_cap + 1000) * 16)
        self.counts_t = mk(abi.query_counts_dtype.itemsize)
        uu, up = dev._u(u)
        r = (Region() if region is None else region).record() if region_record is None else region_record
        f = record if record is not None else None if footprint is None else footprint.record()
        head = (dev._p(dev.nodes), dev._p(dev.stats), up, None if null_region else ctypes.c_void_p(r.ctypes.data))
        tail = (max_level, abi.EXPORT_SELECT[select] if isinstance(select, str) else select, dev._p(self.scratch), ctypes.c_uint64(need),
                dev._p(self.table), self.table_cap, None if count_only else dev._p(self.samples), ctypes.c_uint64(self.sample_cap),
                dev._p(self.counts_t), dev._stream())
        if entry == "region":
            self.rc = L.simlod_query_region(*head, *tail)
        else:
            self.rc = L.simlod_query_footprint(*head, None if f is None else ctypes.c_void_p(f.ctypes.data), *tail)
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


def _assert_matches(raw, mirror, cnt, what):
    assert raw.rc == 0, what
    got = {f: int(raw.counts[f]) for f in COUNT_FIELDS}
    assert got == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    assert raw.table_bytes() == mirror.nodes.tobytes(), f"{what}: the table differs"
    assert raw.sample_bytes() == mirror.samples.tobytes(), f"{what}: the samples differ"
    assert raw.poison_behind(mirror.num_nodes, mirror.num_samples), f"{what}: written past the result"


@pytest.mark.parametrize("name", cases.CASES)
def test_footprint_matches_mirror(built_libs, name):
    dev, u, pts, box = _build(name)
    full = dev.export_octree(u)
    prints = {kind: fr.footprint(kind, box) for kind in fr.names_for(name)}
    crops = {}
    for kind, f in prints.items():
        for sel, ml in MODES:
            crops[kind, sel, ml] = full.crop(Region(), ml, sel, return_counts=True, footprint=f)
    for source in ("chunk table", "walk"):
        for (kind, sel, ml), (mirror, cnt) in crops.items():
            _assert_matches(Raw(dev, u, prints[kind], None, ml, sel), mirror, cnt, f"{name} {kind} {sel}@{ml} ({source})")
        dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))        # the builder's chunk table no longer counts: every list is walked
    # the Python entry points: a count-only call, then exact buffers
    f = prints["star7"]
    mirror, cnt = crops["star7", "cut", 20]
    ex, c = dev.query_region(u, Region(), return_counts=True, footprint=f)
    assert ex.select == abi.EXPORT_REGION and ex.nodes.tobytes() == mirror.nodes.tobytes() and ex.samples.tobytes() == mirror.samples.tobytes()
    cc = dev.count_region(u, Region(), footprint=f)
    assert [int(cc[k]) for k in COUNT_FIELDS] == [int(c[k]) for k in COUNT_FIELDS] == [int(cnt[k]) for k in COUNT_FIELDS]
    rr.assert_same_multiset(ex.samples, pts[f.contains(pts)], name)


@pytest.fixture(scope="module")
def terrain3m(built_libs):
    t = fr.TERRAIN_3M
    pts, box = synthetic.terrain(t["n"], seed=t["seed"], box=t["box"], tile=t["tile"])
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, [pts[i:i + 1_000_000] for i in range(0, len(pts), 1_000_000)])
    return dev, u, pts, box, dev.export_octree(u)


@pytest.mark.parametrize("kind", ["star", "triangle"])
def test_terrain_footprints_are_not_vacuous(terrain3m, kind):
    dev, u, pts, box, full = terrain3m
    f = fr.terrain3m_footprints()[kind]
    st = dev.read_stats()
    raw = Raw(dev, u, f, None, 20, "cut")
    c = raw.counts
    assert raw.rc == 0 and int(c["error"]) == 0
    print(kind, {k: int(c[k]) for k in COUNT_FIELDS}, "of", int(st["numNodes"]), "nodes")
    assert int(c["numCopiedNodes"]) > 0 and int(c["numFilteredNodes"]) > 0 and int(c["numNodes"]) < int(st["numNodes"])
    assert 0 < int(c["numSamples"]) < int(c["numCandidates"])
    got = raw.samples[: int(c["numSamples"]) * 16].cpu().numpy().view(abi.point_dtype)
    rr.assert_same_multiset(got, pts[f.contains(pts)], f"3 M terrain, {kind}")
    mirror, cnt = full.crop(Region(), 20, "cut", return_counts=True, footprint=f)
    _assert_matches(raw, mirror, cnt, f"3 M terrain, {kind}")
    mirror, cnt = full.crop(Region(), 20, "all", return_counts=True, footprint=f)
    _assert_matches(Raw(dev, u, f, None, 20, "all"), mirror, cnt, f"3 M terrain, {kind}, all")


def test_terrain_star7_and_slab(terrain3m):
    dev, u, pts, box, full = terrain3m
    f, r = fr.footprint("star7", box), Region.from_planes(SLAB_3M)
    mirror, cnt = full.crop(r, 20, "cut", return_counts=True, footprint=f)
    raw = Raw(dev, u, f, r, 20, "cut")
    _assert_matches(raw, mirror, cnt, "3 M terrain, star7 and slab")
    both = f.contains(pts) & rr.brute_mask(r, pts)
    assert 0 < both.sum() < min(int(f.contains(pts).sum()), int(rr.brute_mask(r, pts).sum()))
    rr.assert_same_multiset(mirror.samples, pts[both], "3 M terrain, star7 and slab")


def test_null_footprint_is_the_region_query_and_cover_is_the_export(built_libs):
    dev, u, pts, box = _build("terrain_4x100k")
    for kind in ("oblique", "box", "none"):
        for sel, ml in MODES:
            r = rr.region(kind, box)
            a, b = Raw(dev, u, None, r, ml, sel), Raw(dev, u, None, r, ml, sel, entry="region")
            assert a.rc == b.rc == 0 and a.counts.tobytes() == b.counts.tobytes(), (kind, sel, ml)
            n, s = int(a.counts["numNodes"]), int(a.counts["numSamples"])
            assert a.table_bytes() == b.table_bytes() and a.sample_bytes() == b.sample_bytes() and a.poison_behind(n, s), (kind, sel, ml)
    # the null footprint asks for the region query's scratch bytes only
    st = dev.read_stats()
    need = int(dev.L.simlod_query_buffer_min_bytes(int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])))
    assert Raw(dev, u, None, rr.region("oblique", box), scratch_bytes=need).counts.tobytes() == Raw(dev, u, None, rr.region("oblique", box)).counts.tobytes()
    cover = fr.footprint("cover", box)
    for sel, ml in MODES:
        raw = Raw(dev, u, cover, None, ml, sel)
        ex = dev.export_octree(u, max_level=ml, select=sel)
        assert raw.rc == 0 and int(raw.counts["error"]) == 0 and int(raw.counts["numFilteredNodes"]) == 0
        assert raw.table_bytes() == ex.nodes.tobytes() and raw.sample_bytes() == ex.samples.tobytes(), (sel, ml)
        assert int(raw.counts["numCopiedNodes"]) == int((ex.nodes["numSamples"] != 0).sum())


def test_lists_longer_than_a_chunk_table_row(built_libs):
    """The voxel lists of a dense cube's upper nodes hold more than 50 chunks, a row of the builder's chunk table: the directory takes what
    the table gives and follows `next` behind it."""
    pts, box = synthetic.uniform_cube(600_000, seed=9)
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, [pts[i:i + 200_000] for i in range(0, len(pts), 200_000)])
    full = dev.export_octree(u)
    assert int(full.nodes["numSamples"].max()) > 50 * abi.POINTS_PER_CHUNK
    f = fr.footprint("star7", box)
    mirror, cnt = full.crop(Region(), 20, "all", return_counts=True, footprint=f)
    assert int(mirror.nodes["numSamples"].max()) > 0 and int(cnt["numFilteredNodes"]) > 0
    _assert_matches(Raw(dev, u, f, None, 20, "all"), mirror, cnt, "dense cube, star7, chunk table")
    dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))
    _assert_matches(Raw(dev, u, f, None, 20, "all"), mirror, cnt, "dense cube, star7, walk")


def test_count_only_and_capacities(terrain3m):
    dev, u, pts, box, full = terrain3m
    f = fr.terrain3m_footprints()["star"]
    ref = Raw(dev, u, f)
    nn, ns = int(ref.counts["numNodes"]), int(ref.counts["numSamples"])
    assert ref.rc == 0 and int(ref.counts["error"]) == 0 and nn > 1 and ns > 0
    cnt = Raw(dev, u, f, count_only=True)
    assert cnt.rc == 0 and cnt.counts.tobytes() == ref.counts.tobytes()
    assert cnt.table_bytes() == ref.table_bytes() and cnt.poison_behind(nn, 0)          # the table is complete, no sample was written
    # exact capacities: the full result
    exact = Raw(dev, u, f, table_cap=nn, sample_cap=ns)
    assert exact.rc == 0 and exact.counts.tobytes() == ref.counts.tobytes()
    assert exact.table_bytes() == ref.table_bytes() and exact.sample_bytes() == ref.sample_bytes() and exact.poison_behind(nn, ns)
    # one sample short: the error bit, the counts still say what is needed, no sample is written
    short = Raw(dev, u, f, table_cap=nn, sample_cap=ns - 1)
    assert short.rc == 0 and int(short.counts["error"]) == abi.EXPORT_ERR_CAPACITY and int(short.counts["numSamples"]) == ns
    assert short.poison_behind(nn, 0)
    # one table entry short: the error bit, nothing behind the capacity
    small = Raw(dev, u, f, table_cap=nn - 1, sample_cap=ns)
    assert small.rc == 0 and int(small.counts["error"]) & abi.EXPORT_ERR_CAPACITY and int(small.counts["numNodes"]) <= nn - 1
    assert small.poison_behind(nn - 1, 0)
    assert int(dev.count_region(u, Region(), footprint=f)["numSamples"]) == ns


def test_invalid_arguments_enqueue_nothing(built_libs):
    dev, u, pts, box = _build("uniform_3x40k")
    ok = fr.footprint("star7", box)
    nn = int(dev.read_stats()["numNodes"])

    def refused(**kw):
        raw = Raw(dev, u, kw.pop("footprint", ok), **kw)
        assert raw.rc == 1, kw                                                          # hipErrorInvalidValue
        assert bool((raw.counts_t == 0xA5).all()) and raw.poison_behind(0, 0) and bool((raw.scratch == 0xA5).all()), kw

    # the footprint's own
    for n in (0, 2, 257, 0xFFFFFFFF):
        rec = ok.record(); rec["numVertices"] = n
        refused(record=rec)
    rec = ok.record(); rec["vertices"][0, 3, 1] = np.nan
    refused(record=rec)
    rec = ok.record(); rec["vertices"][0, 0, 0] = -np.inf
    refused(record=rec)
    rec = ok.record(); rec["axisU"][0, 2] = np.inf
    refused(record=rec)
    rec = ok.record(); rec["axisV"][0, 3] = np.nan
    refused(record=rec)
    for k in range(3):
        rec = ok.record(); rec["reserved"][0, k] = 1
        refused(record=rec)
    refused(scratch_bytes=int(dev.L.simlod_footprint_buffer_min_bytes(nn, 0)) - 1)
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
    # a scratch buffer with room for the table's part and the polygon but not for the items: the device says so
    raw = Raw(dev, u, ok, scratch_bytes=int(dev.L.simlod_footprint_buffer_min_bytes(nn, 0)))
    assert raw.rc == 0 and int(raw.counts["error"]) & abi.EXPORT_ERR_CAPACITY and raw.poison_behind(nn, 0)


def test_query_leaves_its_source_alone(built_libs):
    name = "terrain_4x100k"
    pts, box, batch, T = cases.case(name)
    dev = _device()
    u = dev.uniforms(W, H, T, box)
    dev.reset(u)
    batches = cases.batches_of(name, pts, batch)
    _ingest(dev, u, batches[:2])
    before = dev.export_octree(u)
    for kind in ("star7", "oblique", "rect", "cover", "miss", "bowtie"):
        dev.query_region(u, Region(), select="all", footprint=fr.footprint(kind, box))
        dev.count_region(u, rr.region("slab", box), max_level=1, footprint=fr.footprint(kind, box))
    after = dev.export_octree(u)
    assert before.nodes.tobytes() == after.nodes.tobytes() and before.samples.tobytes() == after.samples.tobytes()
    _ingest(dev, u, batches[2:])
    ref = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=8)
    ref.reset(u)
    ref.add_points(u, pts, batch)
    nodes, pers, n = host_image_of(dev)
    assert_dumps_equal(oracle.dump_image(nodes, n), ref.dump(), name)
    assert_stats_equal(dev.read_stats(), ref.stats[0], STATS_BUILD_FIELDS, name)


def test_footprint_crop_is_an_octree(built_libs):
    src, u, pts, box = _build("terrain_4x100k")
    f = fr.footprint("star7", box)
    crop, cnt = src.query_region(u, Region(), select="all", return_counts=True, footprint=f)
    crop.validate()
    assert 1 < crop.num_nodes < int(src.read_stats()["numNodes"]) and crop.num_samples > 0
    dst = _device()
    dst.nodes.fill_(0xA5)
    dst.import_octree(crop)
    st = dst.read_stats()
    assert int(st["dbg"]) == 0 and int(st["numNodes"]) == crop.num_nodes and int(st["numPoints"]) + int(st["numVoxels"]) == crop.num_samples
    # its full export is the crop again; an entry that lost all its children is a leaf of the NEW octree
    back = dst.export_octree(u)
    want = crop.nodes.copy()
    want["flags"][want["childMask"] == 0] |= abi.EXPORT_FLAG_LEAF
    assert back.nodes.tobytes() == want.tobytes() and back.samples.tobytes() == crop.samples.tobytes()
    # it renders
    dst.render(u)
    assert int((dst.framebuffer(W, H) != abi.CLEAR_PIXEL).sum()) > 100
    # and a footprint query ON the imported octree equals the mirror of ITS export
    for kind, sel, ml in (("bowtie", "cut", 20), ("oblique", "all", 20), ("rect", "cut", 2)):
        g = fr.footprint(kind, box)
        mirror, mc = back.crop(Region(), ml, sel, return_counts=True, footprint=g)
        _assert_matches(Raw(dst, u, g, None, ml, sel), mirror, mc, f"imported crop, {kind} {sel}@{ml}")
