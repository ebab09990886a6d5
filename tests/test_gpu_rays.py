"""GPU tier: simlod_query_rays (include/simlod_hip.h, "ray queries") through the C ABI against the host mirror OctreeExport.cast on the
device's own export, byte for byte, and against a brute force over the input points; count-only calls, capacities, refused arguments,
the limit of 2^20 rays, long chunk lists, imported octrees and a box off the origin."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import oracle
import rays_ref as yr
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import Rays
from util import STATS_BUILD_FIELDS, _build, _chunks, _device, _ingest, assert_dumps_equal, assert_stats_equal, host_image_of

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
MODES = [("cut", 20), ("all", 20), ("cut", 2)]
COUNT_FIELDS = list(abi.ray_counts_dtype.names)
NONE = abi.EXPORT_NONE


class Raw:
    """One simlod_query_rays call with every buffer poisoned: rc, the counts record, and the buffers as the call left them.  Without
    scratch_bytes a call with hits is sized from the counts of a count-only call of its own, as a host would do it."""

    def __init__(self, dev, u, rays, max_level=20, select="cut", *, table_cap=None, count_only=False, want_table=True, scratch_bytes=None,
                 num_rays=None, null=()):
        st = dev.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        self.table_cap = nn if table_cap is None else table_cap
        L = dev.L
        rec = np.ascontiguousarray(rays.record() if isinstance(rays, Rays) else rays)
        self.n = len(rec) if num_rays is None else num_rays
        sel = abi.EXPORT_SELECT[select] if isinstance(select, str) else select
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        d_rays = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev.device) if len(rec) else mk(48)
        uu, up = dev._u(u)

        def call(scratch, need, table, hits, counts):
            a = {"nodes": dev._p(dev.nodes), "stats": dev._p(dev.stats), "uniforms": up, "rays": dev._p(d_rays), "scratch": dev._p(scratch), "counts": dev._p(counts)}
            for k in null:
                a[k] = None
            rc = L.simlod_query_rays(a["nodes"], a["stats"], a["uniforms"], a["rays"], self.n, max_level, sel, a["scratch"], ctypes.c_uint64(need),
                                     None if table is None else dev._p(table), self.table_cap, None if hits is None else dev._p(hits), a["counts"], dev._stream())
            torch.cuda.synchronize()
            return rc

        if scratch_bytes is None:
            need = int(L.simlod_rays_buffer_min_bytes(self.table_cap, bound, self.n, 0, 0))
            if not count_only:
                c0 = mk(32)
                rc = call(mk(need), need, None, None, c0)
                assert rc == 0, rc
                c0 = c0.cpu().numpy()[:32].view(abi.ray_counts_dtype)[0]
                need = int(L.simlod_rays_buffer_min_bytes(self.table_cap, bound, self.n, int(c0["numPairs"]), int(c0["numCandidates"])))
        else:
            need = scratch_bytes
        self.need = need
        self.scratch, self.counts_t = mk(need), mk(32)
        self.table = mk((self.table_cap + 4) * 40) if want_table else None
        self.hits_t = mk((self.n + 4) * 32)
        self.rc = call(self.scratch, need, self.table, None if count_only else self.hits_t, self.counts_t)
        self.counts = self.counts_t.cpu().numpy()[:32].view(abi.ray_counts_dtype)[0]

    def hits(self):
        return self.hits_t[: self.n * 32].cpu().numpy().view(abi.ray_hit_dtype)

    def table_bytes(self, n=None):
        n = int(self.counts["numNodes"]) if n is None else n
        return self.table[: n * 40].cpu().numpy().tobytes()

    def poison_behind(self, nodes, hits):
        return (self.table is None or bool((self.table[nodes * 40:] == 0xA5).all())) and bool((self.hits_t[hits * 32:] == 0xA5).all())

    def untouched(self):
        return bool((self.counts_t == 0xA5).all()) and self.poison_behind(0, 0) and bool((self.scratch == 0xA5).all())


def _assert_matches(raw, hits, cnt, what, table=None):
    assert raw.rc == 0, what
    got = {f: int(raw.counts[f]) for f in COUNT_FIELDS}
    assert got == {f: int(cnt[f]) for f in COUNT_FIELDS}, what
    dh = raw.hits()
    if dh.tobytes() != hits.tobytes():
        bad = np.nonzero(dh != hits)[0]
        raise AssertionError(f"{what}: {len(bad)} hits differ, first ray {bad[0]}: device {dh[bad[0]]} mirror {hits[bad[0]]}")
    if table is not None:
        assert raw.table_bytes() == table.nodes.tobytes(), f"{what}: the table differs"
    assert raw.poison_behind(int(cnt["numNodes"]), len(hits)), f"{what}: written past the result"


@pytest.mark.parametrize("name", cases.CASES)
def test_rays_match_mirror(built_libs, name):
    dev, u, pts, box = _build(name)
    full = dev.export_octree(u)
    sets = yr.ray_sets(name, pts, box)
    want, tables = {}, {}
    for sel, ml in MODES:
        tables[sel, ml] = dev.export_octree(u, max_level=ml, select=sel)
        assert tables[sel, ml].nodes.tobytes() == full.truncated(ml, sel).nodes.tobytes()
        for key, (rays, needs_misses, cone) in sets.items():
            hits, cnt, passing = full.cast(rays, ml, sel, return_counts=True, return_passing=True)
            if (sel, ml) == ("cut", 20):
                share = yr.assert_not_vacuous(hits, needs_misses, f"{name} {key}", passing, cone)
                print(name, key, f"hit share {share:.2f}", {f: int(cnt[f]) for f in COUNT_FIELDS})
            yr.assert_hits_index_export(hits, tables[sel, ml], f"{name} {key} {sel}@{ml}")
            want[key, sel, ml] = (hits, cnt)
    for source in ("chunk table", "walk"):
        for (key, sel, ml), (hits, cnt) in want.items():
            raw = Raw(dev, u, sets[key][0], ml, sel)
            _assert_matches(raw, hits, cnt, f"{name} {key} {sel}@{ml} ({source})", tables[sel, ml])
        dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))        # the builder's chunk table no longer counts: every list is walked
    # the Python entry points: a count-only call, then exact scratch; host rays and device rays
    key = next(iter(sets))
    rays = sets[key][0]
    hits, cnt = want[key, "cut", 20]
    got, c = dev.cast_rays(u, rays, return_counts=True)
    assert got.dtype == abi.ray_hit_dtype and got.tobytes() == hits.tobytes()
    cc = dev.count_rays(u, rays)
    assert [int(cc[f]) for f in COUNT_FIELDS] == [int(c[f]) for f in COUNT_FIELDS] == [int(cnt[f]) for f in COUNT_FIELDS]
    d_rays = torch.from_numpy(rays.record().view(np.uint8).reshape(-1)).to(dev.device)
    d_hits = dev.cast_rays(u, d_rays)
    assert isinstance(d_hits, torch.Tensor) and d_hits.device == d_rays.device and d_hits.cpu().numpy().tobytes() == hits.tobytes()
    yr.assert_hits_are_brute(got, rays, pts, name)


def test_visible_selection(built_libs):
    dev, u, pts, box = _build("terrain_4x100k")
    rays = yr.cones(pts, box, 0.002)
    before = Raw(dev, u, rays, 20, "visible", count_only=True)
    assert before.rc == 1 and before.untouched()                              # no frame yet: refused as the export refuses it
    dev.render(u)
    ex = dev.export_octree(u, select="visible")
    hits, cnt, passing = ex.cast_selected(rays, return_counts=True, return_passing=True)
    yr.assert_not_vacuous(hits, False, "visible", passing, True)
    yr.assert_hits_index_export(hits, ex, "visible")
    _assert_matches(Raw(dev, u, rays, 20, "visible"), hits, cnt, "visible", ex)
    assert dev.cast_rays(u, rays, select="visible").tobytes() == hits.tobytes()


@pytest.fixture(scope="module")
def terrain3m(built_libs):
    pts, box = synthetic.terrain(3_000_000, seed=3, box=(600.0, 400.0, 40.0), tile=50.0)
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, [pts[i:i + 1_000_000] for i in range(0, len(pts), 1_000_000)])
    return dev, u, pts, box, dev.export_octree(u)


def _rays_3m(box, pts):
    """2 048 vertical rays of radius 0.1, 2 048 of radius 0.5, 1 024 pixel cones of the fixture's camera through pixels the terrain covers
    (it fills about 7 % of this camera's frame)."""
    thin, wide = yr.vertical(None, box, 0.1, n=2048, seed=5), yr.vertical(None, box, 0.5, n=2048, seed=6)
    covered = yr.covered_pixels(cases._cam(box), W, H, pts)
    px = covered[np.sort(np.random.RandomState(7).choice(len(covered), 1024, replace=False))]
    cones = Rays.from_pixels(cases._cam(box), W, H, px, pixel_radius=0.5, t_max=3000.0)
    return thin, wide, cones


def test_terrain_3m(terrain3m):
    dev, u, pts, box, full = terrain3m
    thin, wide, cones = _rays_3m(box, pts)
    rays = Rays.from_records(np.concatenate([thin.record(), wide.record(), cones.record()]))
    hits, cnt, passing = full.cast(rays, 20, "cut", return_counts=True, return_passing=True)
    yr.assert_not_vacuous(hits[:2048], True, "3 M terrain, vertical r0.1")
    yr.assert_not_vacuous(hits[2048:4096], False, "3 M terrain, vertical r0.5")
    yr.assert_not_vacuous(hits[4096:], False, "3 M terrain, pixel cones", passing[4096:], True)
    raw = Raw(dev, u, rays)
    print({f: int(raw.counts[f]) for f in COUNT_FIELDS}, "scratch", raw.need)
    _assert_matches(raw, hits, cnt, "3 M terrain", dev.export_octree(u, select="cut"))
    pick = np.sort(np.random.RandomState(8).choice(len(rays), 256, replace=False))
    sub = Rays.from_records(rays.record()[pick])
    yr.assert_hits_are_brute(raw.hits()[pick], sub, pts, "3 M terrain, 256 rays against the raw points")


def test_one_ray_and_the_limit(terrain3m):
    dev, u, pts, box, full = terrain3m
    thin, wide, cones = _rays_3m(box, pts)
    one = Rays.from_records(cones.record()[:1])
    hits, cnt = full.cast(one, return_counts=True)
    _assert_matches(Raw(dev, u, one), hits, cnt, "one ray")
    # 2^20 rays: the 4 096 vertical ones at every 256th position, all others above the box pointing up (valid, no pair)
    n = abi.RAYS_MAX
    rec = np.zeros(n, dtype=abi.ray_dtype)
    rec["origin"] = (300.0, 200.0, box[2] + 50.0)
    rec["dir"] = (0.0, 0.0, 1.0)
    rec["tMax"] = 10.0
    rec[::256] = np.concatenate([thin.record(), wide.record()])
    many = Rays.from_records(rec)
    hits, cnt = full.cast(many, return_counts=True)
    assert int(cnt["numInvalid"]) == 0 and (hits["node"][::256] != NONE).mean() > 0.25 and (np.delete(hits["node"], np.s_[::256]) == NONE).all()
    raw = Raw(dev, u, many, want_table=False)
    _assert_matches(raw, hits, cnt, "2^20 rays")
    over = Raw(dev, u, rec[:16], num_rays=n + 1, count_only=True)
    assert over.rc == 1 and over.untouched()


def test_count_only_and_capacities(terrain3m):
    dev, u, pts, box, full = terrain3m
    thin, wide, cones = _rays_3m(box, pts)
    rays = Rays.from_records(np.concatenate([wide.record()[:512], cones.record()[:128]]))
    hits, cnt = full.cast(rays, return_counts=True)
    ref = Raw(dev, u, rays)
    _assert_matches(ref, hits, cnt, "reference")
    nn = int(cnt["numNodes"])
    only = Raw(dev, u, rays, count_only=True)
    assert only.rc == 0 and only.counts.tobytes() == ref.counts.tobytes()                       # complete, numHits included
    assert only.table_bytes() == ref.table_bytes() and only.poison_behind(nn, 0)               # the table is complete, no hit was written
    assert Raw(dev, u, rays, count_only=True, want_table=False).counts.tobytes() == ref.counts.tobytes()
    # the exact need (simlod_hip.h): the chunks of the table's nodes in the place of the item bound
    cut = dev.export_octree(u, select="cut")
    L = dev.L
    P, C = int(cnt["numPairs"]), int(cnt["numCandidates"])
    exact = int(L.simlod_rays_buffer_min_bytes(nn, 0, len(rays), P, C)) - 32 * (nn + 1) + 32 * _chunks(cut)
    assert exact >= int(L.simlod_rays_buffer_min_bytes(nn, 0, len(rays), 0, 0)) and P > 0
    ok = Raw(dev, u, rays, scratch_bytes=exact)
    _assert_matches(ok, hits, cnt, "exact scratch")
    # room for one pair fewer: the error bit, the counts still say what is needed, NO hit record is written
    short = Raw(dev, u, rays, scratch_bytes=exact - 32)
    assert short.rc == 0 and int(short.counts["error"]) == abi.EXPORT_ERR_CAPACITY and short.poison_behind(nn, 0)
    assert int(short.counts["numPairs"]) == P and int(short.counts["numCandidates"]) == C
    # a count-only buffer given to a call with hits: the same
    small = Raw(dev, u, rays, scratch_bytes=only.need)
    assert small.rc == 0 and int(small.counts["error"]) == abi.EXPORT_ERR_CAPACITY and small.poison_behind(nn, 0)
    # one table entry short: the walk's error, no hit, nothing behind the capacity
    tiny = Raw(dev, u, rays, table_cap=nn - 1)
    assert tiny.rc == 0 and int(tiny.counts["error"]) & abi.EXPORT_ERR_CAPACITY and int(tiny.counts["numNodes"]) <= nn - 1 and tiny.poison_behind(nn - 1, 0)


def test_lists_longer_than_a_chunk_table_row(built_libs):
    """The root of a dense cube holds far more than 50 chunks of voxels, a row of the builder's chunk table: with the table cut at level 0
    every hit lies in that list, most of them behind its 50th chunk."""
    pts, box = synthetic.uniform_cube(600_000, seed=9)
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, [pts[i:i + 200_000] for i in range(0, len(pts), 200_000)])
    full = dev.export_octree(u)
    assert int(full.nodes["numSamples"][0]) > 100 * abi.POINTS_PER_CHUNK
    rays = yr.random_rays(pts, box, 0.01)
    for sel, ml in (("cut", 0), ("all", 20)):
        hits, cnt = full.cast(rays, ml, sel, return_counts=True)
        hit = hits["node"] != NONE
        if ml == 0:
            assert hit.mean() > 0.5 and (hits["ordinal"][hit] >= 50 * abi.POINTS_PER_CHUNK).sum() >= 16
        _assert_matches(Raw(dev, u, rays, ml, sel), hits, cnt, f"dense cube {sel}@{ml}, chunk table")
    dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))
    hits, cnt = full.cast(rays, 0, "cut", return_counts=True)
    _assert_matches(Raw(dev, u, rays, 0, "cut"), hits, cnt, "dense cube cut@0, walk")


def test_invalid_arguments_enqueue_nothing(built_libs):
    dev, u, pts, box = _build("uniform_3x40k")
    rays = yr.random_rays(pts, box, 0.02)
    nn = int(dev.read_stats()["numNodes"])

    def refused(**kw):
        kw.setdefault("count_only", False)
        kw.setdefault("scratch_bytes", int(dev.L.simlod_rays_buffer_min_bytes(nn, 1_000_000, len(rays), 1000, 1_000_000)))
        raw = Raw(dev, u, kw.pop("rays", rays), **kw)
        assert raw.rc == 1, kw                                                          # hipErrorInvalidValue
        assert raw.untouched(), kw

    for k in ("nodes", "stats", "uniforms", "rays", "scratch", "counts"):
        refused(null=(k,))
    refused(num_rays=0)
    refused(num_rays=abi.RAYS_MAX + 1)
    refused(select=abi.EXPORT_REGION)
    refused(select=abi.EXPORT_VISIBLE)                                                  # no frame ran
    refused(scratch_bytes=int(dev.L.simlod_rays_buffer_min_bytes(nn, 0, len(rays), 0, 0)) - 1)
    # table and hits may be null
    ok = Raw(dev, u, rays, count_only=True, want_table=False)
    assert ok.rc == 0 and int(ok.counts["error"]) == 0 and int(ok.counts["numHits"]) > 0
    # a scratch buffer with room for the table's part but not for the chunk items: the device says so
    raw = Raw(dev, u, rays, scratch_bytes=int(dev.L.simlod_rays_buffer_min_bytes(nn, 0, len(rays), 0, 0)))
    assert raw.rc == 0 and int(raw.counts["error"]) & abi.EXPORT_ERR_CAPACITY and raw.poison_behind(nn, 0)


def test_degenerate_rays_on_the_device(built_libs):
    dev, u, pts, box = _build("terrain_4x100k")
    full = dev.export_octree(u)
    good = yr.vertical(pts, box, 0.5, n=64).record()
    bad = []
    for k, v in (("dir", [[0, 0, 0]]), ("origin", [[np.nan, 1, 1]]), ("dir", [[0, np.inf, -1]]), ("tMax", np.inf), ("tMin", np.nan), ("tMin", 70.0),
                 ("tMin", -1.0), ("radius", -0.5), ("spread", -1e-3), ("spread", np.nan), ("reserved", [[0, 1]])):
        r = good[:1].copy()
        r[k] = v
        bad.append(r)
    # axis-parallel rays: along +x inside the footprint, outside it, and along -z at the root's widened face and one ulp beyond
    e = np.ldexp(np.float64(max(box)), -20)
    face = np.float32(-(e + 0.5))
    z = float(np.median(pts["z"]))
    axis = Rays([[-5.0, 200.0, z], [-5.0, 900.0, z], [300.0, 200.0, z]], (1.0, 0.0, 0.0), 0.0, 700.0, 0.5, 0.0).record()
    edge = Rays([[float(face), 100.0, 50.0], [float(np.nextafter(face, np.float32(-1e9))), 100.0, 50.0]], (0.0, 0.0, -1.0), 0.0, 60.0, 0.5, 0.0).record()
    rays = Rays.from_records(np.concatenate([good[:32]] + bad + [axis, edge, good[32:]]))
    hits, cnt = full.cast(rays, return_counts=True)
    assert int(cnt["numInvalid"]) == len(bad) and int(cnt["numHits"]) >= 16
    _assert_matches(Raw(dev, u, rays), hits, cnt, "degenerate and axis-parallel rays")
    only_bad = Rays.from_records(np.concatenate(bad))
    hits, cnt = full.cast(only_bad, return_counts=True)
    _assert_matches(Raw(dev, u, only_bad), hits, cnt, "invalid rays only")


def test_imported_octrees_and_a_shifted_box(built_libs):
    off = cases.GEOREF
    src, u, pts, box = _build("terrain_4x100k", off)
    full = src.export_octree(u)
    base_pts, base_box, _, _ = cases.case("terrain_4x100k")
    sets = {k: yr.shift_rays(v[0], off) for k, v in yr.ray_sets("terrain_4x100k", base_pts, base_box).items() if k != "vertical r0.25"}
    want = {}
    for key, rays in sets.items():
        for sel, ml in MODES:
            want[key, sel, ml] = full.cast(rays, ml, sel, return_counts=True)
        yr.assert_not_vacuous(want[key, "cut", 20][0], False, f"georef {key}")
    for (key, sel, ml), (hits, cnt) in want.items():
        _assert_matches(Raw(src, u, sets[key], ml, sel), hits, cnt, f"georef {key} {sel}@{ml}")
    yr.assert_hits_are_brute(want["vertical r0.5", "cut", 20][0], sets["vertical r0.5"], pts, "georef")
    for buildable in (False, True):
        dst = _device()
        dst.nodes.fill_(0xA5)
        if buildable:
            dst.import_octree(full, buildable=True, uniforms=u)
        else:
            dst.import_octree(full)
        back = dst.export_octree(u)
        assert back.nodes.tobytes() == full.nodes.tobytes() and back.samples.tobytes() == full.samples.tobytes()
        for (key, sel, ml), (hits, cnt) in want.items():
            _assert_matches(Raw(dst, u, sets[key], ml, sel), hits, cnt, f"imported (buildable={buildable}) {key} {sel}@{ml}")


def test_rays_leave_their_source_alone(built_libs):
    name = "terrain_4x100k"
    pts, box, batch, T = cases.case(name)
    dev = _device()
    u = dev.uniforms(W, H, T, box)
    dev.reset(u)
    batches = cases.batches_of(name, pts, batch)
    _ingest(dev, u, batches[:2])
    before = dev.export_octree(u)
    for key, (rays, _, _) in yr.ray_sets(name, pts, box).items():
        dev.cast_rays(u, rays, select="all")
        dev.count_rays(u, rays, max_level=1)
    after = dev.export_octree(u)
    assert before.nodes.tobytes() == after.nodes.tobytes() and before.samples.tobytes() == after.samples.tobytes()
    _ingest(dev, u, batches[2:])
    ref = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=8)
    ref.reset(u)
    ref.add_points(u, pts, batch)
    nodes, pers, n = host_image_of(dev)
    assert_dumps_equal(oracle.dump_image(nodes, n), ref.dump(), name)
    assert_stats_equal(dev.read_stats(), ref.stats[0], STATS_BUILD_FIELDS, name)
