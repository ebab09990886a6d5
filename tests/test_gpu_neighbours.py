"""GPU tier: simlod_query_neighbours (include/simlod_hip.h, "neighbour queries") through the C ABI against the host mirror
OctreeExport.neighbours on the device's own export, byte for byte, and against a brute force over the input points; exact ties, more
queries on one node than a tile holds, count-only calls, capacities, refused arguments, degenerate queries, the limit of 2^20 queries,
imported octrees and a box off the origin; the ray and the neighbour query in turn on one octree's cached scratch."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import neighbours_ref as nr
import oracle
import rays_ref as yr
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import Spheres
from util import STATS_BUILD_FIELDS, _build, _chunks, _device, _ingest, assert_dumps_equal, assert_stats_equal, host_image_of

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
MODES = [("cut", 20), ("all", 20), ("cut", 2)]
COUNT_FIELDS = list(abi.neighbour_counts_dtype.names)
NONE = abi.EXPORT_NONE
NB, CB = abi.neighbour_dtype.itemsize, abi.neighbour_counts_dtype.itemsize


def _build_points(pts, box, batch):
    dev = _device()
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    _ingest(dev, u, [pts[i:i + batch] for i in range(0, len(pts), batch)])
    return dev, u


class Raw:
    """One simlod_query_neighbours call with every buffer poisoned: rc, the counts record, and the buffers as the call left them.  Without
    scratch_bytes a call with results is sized from the counts of a count-only call of its own, as a host would do it."""

    def __init__(self, dev, u, spheres, k, max_level=20, select="cut", *, table_cap=None, count_only=False, want_table=True, want_within=True,
                 scratch_bytes=None, num_queries=None, null=()):
        st = dev.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        self.table_cap = nn if table_cap is None else table_cap
        L = dev.L
        rec = np.ascontiguousarray(spheres.record() if isinstance(spheres, Spheres) else spheres)
        self.n = len(rec) if num_queries is None else num_queries
        self.k = k
        sel = abi.EXPORT_SELECT[select] if isinstance(select, str) else select
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        d_q = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev.device) if len(rec) else mk(16)
        uu, up = dev._u(u)

        def call(scratch, need, table, out, within, counts):
            a = {"nodes": dev._p(dev.nodes), "stats": dev._p(dev.stats), "uniforms": up, "queries": dev._p(d_q), "scratch": dev._p(scratch), "counts": dev._p(counts)}
            for key in null:
                a[key] = None
            rc = L.simlod_query_neighbours(a["nodes"], a["stats"], a["uniforms"], a["queries"], self.n, k, max_level, sel, a["scratch"], ctypes.c_uint64(need),
                                           None if table is None else dev._p(table), self.table_cap, None if out is None else dev._p(out),
                                           None if within is None else dev._p(within), a["counts"], dev._stream())
            torch.cuda.synchronize()
            return rc

        if scratch_bytes is None:
            need = int(L.simlod_neighbours_buffer_min_bytes(self.table_cap, bound, self.n, k, 0, 0))
            if not count_only:
                c0 = mk(CB)
                rc = call(mk(need), need, None, None, None, c0)
                assert rc == 0, rc
                c0 = c0.cpu().numpy()[:CB].view(abi.neighbour_counts_dtype)[0]
                need = int(L.simlod_neighbours_buffer_min_bytes(self.table_cap, bound, self.n, k, int(c0["numPairs"]), int(c0["numCandidates"])))
        else:
            need = scratch_bytes
        self.need = need
        self.scratch, self.counts_t = mk(need), mk(CB)
        self.table = mk((self.table_cap + 4) * 40) if want_table else None
        rows = min(self.n, len(rec)) if num_queries is not None else self.n
        self.out_t = mk((rows * min(k, 16) + 4) * NB)
        self.within_t = mk((rows + 4) * 4)
        self.rc = call(self.scratch, need, self.table, None if count_only else self.out_t, self.within_t if want_within and not count_only else None, self.counts_t)
        self.counts = self.counts_t.cpu().numpy()[:CB].view(abi.neighbour_counts_dtype)[0]

    def neighbours(self):
        return self.out_t[: self.n * self.k * NB].cpu().numpy().view(abi.neighbour_dtype).reshape(self.n, self.k)

    def within(self):
        return self.within_t[: self.n * 4].cpu().numpy().view(np.uint32).astype(np.int64)

    def table_bytes(self, n=None):
        n = int(self.counts["numNodes"]) if n is None else n
        return self.table[: n * 40].cpu().numpy().tobytes()

    def poison_behind(self, nodes, queries, within=None):
        within = queries if within is None else within
        return ((self.table is None or bool((self.table[nodes * 40:] == 0xA5).all())) and bool((self.out_t[queries * self.k * NB:] == 0xA5).all())
                and bool((self.within_t[within * 4:] == 0xA5).all()))

    def untouched(self):
        return bool((self.counts_t == 0xA5).all()) and self.poison_behind(0, 0) and bool((self.scratch == 0xA5).all())


def _assert_matches(raw, want, what, table=None):
    nb, within, cnt = want
    assert raw.rc == 0, what
    got = {f: int(raw.counts[f]) for f in COUNT_FIELDS}
    assert got == {f: int(cnt[f]) for f in COUNT_FIELDS}, (what, got)
    dn = raw.neighbours()
    if dn.tobytes() != nb.tobytes():
        bad = np.nonzero((dn != nb).any(1))[0]
        raise AssertionError(f"{what}: {len(bad)} queries differ, first {bad[0]}: device {dn[bad[0]]} mirror {nb[bad[0]]}")
    assert np.array_equal(raw.within(), within), f"{what}: within differs at {np.nonzero(raw.within() != within)[0][:8]}"
    if table is not None:
        assert raw.table_bytes() == table.nodes.tobytes(), f"{what}: the table differs"
    assert raw.poison_behind(int(cnt["numNodes"]), len(nb)), f"{what}: written past the result"


def _knn_brute(pts, centers, k):
    x, y, z = (pts[a].astype(np.float64) for a in "xyz")
    out = np.zeros((len(centers), k))
    for i, c in enumerate(centers.astype(np.float64)):
        px, py, pz = x - c[0], y - c[1], z - c[2]
        out[i] = np.sort((px * px + py * py) + pz * pz)[:k]
    return out


@pytest.mark.parametrize("name", cases.CASES)
def test_neighbours_match_mirror(built_libs, name):
    dev, u, pts, box = _build(name)
    full = dev.export_octree(u)
    sets = nr.query_sets(pts, box)
    want, tables = {}, {}
    for sel, ml in MODES:
        tables[sel, ml] = dev.export_octree(u, max_level=ml, select=sel)
        for key, k in (("thin", 8), ("wide", 8), ("wide", 1), ("wide", 16)):
            res = full.neighbours(sets[key], k, ml, sel, return_counts=True)
            if (sel, ml, k) == ("cut", 20, 8):
                print(name, key, nr.assert_not_vacuous(key, res[1], f"{name} {key}"), {f: int(res[2][f]) for f in COUNT_FIELDS})
            nr.assert_found_index_export(res[0], tables[sel, ml], f"{name} {key} k={k} {sel}@{ml}")
            nr.assert_misses_behind(res[0], res[1], k, f"{name} {key} k={k} {sel}@{ml}")
            want[key, k, sel, ml] = res
    for source in ("chunk table", "walk"):
        for (key, k, sel, ml), res in want.items():
            _assert_matches(Raw(dev, u, sets[key], k, ml, sel), res, f"{name} {key} k={k} {sel}@{ml} ({source})", tables[sel, ml])
        dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))        # the builder's chunk table no longer counts: every list is walked
    # the Python entry points: a count-only call, then exact scratch; host queries and device queries
    for key in ("wide", "thin"):
        nb, within, cnt = want[key, 8, "cut", 20]
        got, gw, c = dev.find_neighbours(u, sets[key], 8, return_counts=True)
        assert got.dtype == abi.neighbour_dtype and got.shape == (nr.N_QUERIES, 8) and got.tobytes() == nb.tobytes() and np.array_equal(gw, within)
        assert [int(c[f]) for f in COUNT_FIELDS] == [int(cnt[f]) for f in COUNT_FIELDS]
        cc = dev.count_neighbours(u, sets[key], 8)
        assert [int(cc[f]) for f in COUNT_FIELDS[:6]] == [int(cnt[f]) for f in COUNT_FIELDS[:6]] and int(cc["numFound"]) == 0 and int(cc["numWithin"]) == 0
        nr.assert_found_are_brute(got, gw, sets[key], pts, 8, f"{name} {key}")
    d_q = torch.from_numpy(sets["wide"].record().view(np.uint8).reshape(-1)).to(dev.device)
    d_nb, d_w = dev.find_neighbours(u, d_q, 8)
    assert isinstance(d_nb, torch.Tensor) and d_nb.device == d_q.device and d_nb.cpu().numpy().tobytes() == want["wide", 8, "cut", 20][0].tobytes()
    assert isinstance(d_w, torch.Tensor) and np.array_equal(d_w.cpu().numpy().astype(np.int64), want["wide", 8, "cut", 20][1])
    # k_nearest from a quarter of the thin radius: some positions need at least two doublings
    p = pts[nr._chosen(pts)]
    r0 = 0.25 * nr.radii(pts, box)[1]
    _, w2 = nr.brute(Spheres.from_points(p, 2.0 * np.float32(r0)), pts, 8)
    assert (w2 < 8).sum() >= 8, "no position needs a second doubling"
    knn, kw = dev.k_nearest(u, p, 8, r0)
    centers = np.stack([p["x"], p["y"], p["z"]], axis=1)
    assert (kw >= 8).all() and np.array_equal(np.ascontiguousarray(knn["d2"]).view(np.uint64), _knn_brute(pts, centers, 8).view(np.uint64))


@pytest.fixture(scope="module")
def lattice_dev(built_libs):
    pts, box = nr.lattice()
    dev, u = _build_points(pts, box, nr.LATTICE_BATCH)
    return dev, u, pts, box, dev.export_octree(u)


def test_lattice_ties(lattice_dev):
    dev, u, pts, box, full = lattice_dev
    assert int(full.nodes["childMask"][0]) != 0, "the root has not split"
    q = nr.lattice_queries()
    for sel in ("cut", "all"):
        ex = full.truncated(20, sel)
        res = full.neighbours(q, nr.LATTICE_K, 20, sel, return_counts=True)
        want = nr.exhaustive(ex, q, nr.LATTICE_K)
        assert res[0].tobytes() == want[0].tobytes() and np.array_equal(res[1], want[1]), sel
        if sel == "cut":
            nr.assert_lattice_ties(res[0], res[1], ex, q, "lattice cut")
        _assert_matches(Raw(dev, u, q, nr.LATTICE_K, 20, sel), res, f"lattice {sel}", ex)


def test_more_queries_than_a_tile_and_long_lists(built_libs):
    """The root of a dense cube holds far more than 100 chunks of voxels; with the table cut at level 0 all 200 queries pair with it: several
    full tiles and a partial one, lists behind the 50th chunk (a row of the builder's chunk table), k = 16."""
    pts, box = synthetic.uniform_cube(600_000, seed=9)
    dev, u = _build_points(pts, box, 200_000)
    full = dev.export_octree(u)
    assert int(full.nodes["numSamples"][0]) > 100 * abi.POINTS_PER_CHUNK
    rs = np.random.RandomState(12)
    q = Spheres(0.1 + 0.8 * rs.rand(200, 3), 0.03 + 0.02 * rs.rand(200))
    res = full.neighbours(q, 16, 0, "cut", return_counts=True)
    nb, within, cnt = res
    assert int(cnt["numPairs"]) == 200 and np.median(within) >= 64, np.median(within)
    chunks = np.unique(nb["ordinal"][nb["node"] != NONE] // abi.POINTS_PER_CHUNK)
    assert len(chunks) >= 100 and (chunks >= 50).sum() >= 50, len(chunks)
    _assert_matches(Raw(dev, u, q, 16, 0, "cut"), res, "dense cube cut@0, chunk table")
    dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))
    _assert_matches(Raw(dev, u, q, 16, 0, "cut"), res, "dense cube cut@0, walk")


@pytest.fixture(scope="module")
def terrain(built_libs):
    dev, u, pts, box = _build("terrain_4x100k")
    return dev, u, pts, box, dev.export_octree(u)


def test_count_only_and_capacities(terrain):
    dev, u, pts, box, full = terrain
    q, k = nr.wide(pts, box), 8
    res = full.neighbours(q, k, return_counts=True)
    nb, within, cnt = res
    ref = Raw(dev, u, q, k)
    _assert_matches(ref, res, "reference")
    nn = int(cnt["numNodes"])
    only = Raw(dev, u, q, k, count_only=True)
    assert only.rc == 0 and int(only.counts["numFound"]) == 0 and int(only.counts["numWithin"]) == 0
    assert all(int(only.counts[f]) == int(ref.counts[f]) for f in COUNT_FIELDS[:6])
    assert only.table_bytes() == ref.table_bytes() and only.poison_behind(nn, 0)               # the table is complete, no record was written
    assert all(int(Raw(dev, u, q, k, count_only=True, want_table=False).counts[f]) == int(only.counts[f]) for f in COUNT_FIELDS)
    # `within` may be null in a call with neighbours
    _assert_nw = Raw(dev, u, q, k, want_within=False)
    assert _assert_nw.rc == 0 and _assert_nw.neighbours().tobytes() == nb.tobytes() and _assert_nw.poison_behind(nn, len(q), 0)
    # the exact need (simlod_hip.h): the chunks of the table's nodes in the place of the item bound
    cut = dev.export_octree(u, select="cut")
    L = dev.L
    P, C = int(cnt["numPairs"]), int(cnt["numCandidates"])
    exact = int(L.simlod_neighbours_buffer_min_bytes(nn, 0, len(q), k, P, C)) - 32 * (nn + 1) + 32 * _chunks(cut)
    assert exact >= int(L.simlod_neighbours_buffer_min_bytes(nn, 0, len(q), k, 0, 0)) and P > 0
    _assert_matches(Raw(dev, u, q, k, scratch_bytes=exact), res, "exact scratch")
    # room for one pair fewer: the error bit, the counts still say what is needed, NO record is written
    short = Raw(dev, u, q, k, scratch_bytes=exact - (16 + 16 * (k + 1)))
    assert short.rc == 0 and int(short.counts["error"]) == abi.EXPORT_ERR_CAPACITY and short.poison_behind(nn, 0)
    assert int(short.counts["numPairs"]) == P and int(short.counts["numCandidates"]) == C
    byte = Raw(dev, u, q, k, scratch_bytes=exact - 1)
    assert byte.rc == 0 and int(byte.counts["error"]) == abi.EXPORT_ERR_CAPACITY and byte.poison_behind(nn, 0)
    # a count-only buffer given to a call with results: the same
    small = Raw(dev, u, q, k, scratch_bytes=only.need)
    assert small.rc == 0 and int(small.counts["error"]) == abi.EXPORT_ERR_CAPACITY and small.poison_behind(nn, 0)
    # one table entry short: the walk's error, no record, nothing behind the capacity
    tiny = Raw(dev, u, q, k, table_cap=nn - 1)
    assert tiny.rc == 0 and int(tiny.counts["error"]) & abi.EXPORT_ERR_CAPACITY and int(tiny.counts["numNodes"]) <= nn - 1 and tiny.poison_behind(nn - 1, 0)


def test_invalid_arguments_enqueue_nothing(terrain):
    dev, u, pts, box, full = terrain
    q = nr.wide(pts, box)
    nn = int(dev.read_stats()["numNodes"])
    L = dev.L

    def refused(k=8, **kw):
        kw.setdefault("count_only", False)
        kw.setdefault("scratch_bytes", int(L.simlod_neighbours_buffer_min_bytes(nn, 1_000_000, len(q), 16, 1000, 10_000_000)))
        raw = Raw(dev, u, q, k, **kw)
        assert raw.rc == 1, (k, kw)                                                     # hipErrorInvalidValue
        assert raw.untouched(), (k, kw)

    for key in ("nodes", "stats", "uniforms", "queries", "scratch", "counts"):
        refused(null=(key,))
    # within without neighbours
    mk = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev.device)
    d_q = torch.from_numpy(q.record().view(np.uint8).reshape(-1)).to(dev.device)
    need = int(L.simlod_neighbours_buffer_min_bytes(nn, 1_000_000, len(q), 8, 0, 0))
    scratch, wt, ct = mk(need), mk(len(q) * 4), mk(CB)
    rc = L.simlod_query_neighbours(dev._p(dev.nodes), dev._p(dev.stats), dev._u(u)[1], dev._p(d_q), len(q), 8, 20, abi.EXPORT_CUT, dev._p(scratch),
                                   ctypes.c_uint64(need), None, nn, None, dev._p(wt), dev._p(ct), dev._stream())
    torch.cuda.synchronize()
    assert rc == 1 and bool((scratch == 0xA5).all()) and bool((wt == 0xA5).all()) and bool((ct == 0xA5).all())
    refused(num_queries=0)
    refused(num_queries=abi.NEIGHBOURS_MAX + 1)
    refused(k=0)
    refused(k=abi.NEIGHBOURS_MAX_K + 1)
    refused(select=abi.EXPORT_REGION)
    refused(scratch_bytes=int(L.simlod_neighbours_buffer_min_bytes(nn, 0, len(q), 8, 0, 0)) - 1)
    fresh, u2, _, _ = _build("ragged_tiny")
    raw = Raw(fresh, u2, q, 8, select=abi.EXPORT_VISIBLE, count_only=True)              # no frame ran
    assert raw.rc == 1 and raw.untouched()
    # table, neighbours and within may be null
    ok = Raw(dev, u, q, 8, count_only=True, want_table=False)
    assert ok.rc == 0 and int(ok.counts["error"]) == 0 and int(ok.counts["numPairs"]) > 0
    # a scratch buffer with room for the table's part but not for the chunk items: the device says so
    raw = Raw(dev, u, q, 8, scratch_bytes=int(L.simlod_neighbours_buffer_min_bytes(nn, 0, len(q), 8, 0, 0)))
    assert raw.rc == 0 and int(raw.counts["error"]) & abi.EXPORT_ERR_CAPACITY and raw.poison_behind(nn, 0)


def test_degenerate_queries_on_the_device(terrain):
    # radius 0 exactly on duplicated points: 500 points twice, the second time under another colour (as the ray query's tie test)
    pts, box, batch, _ = cases.case("uniform_3x40k")
    dup = pts[np.random.RandomState(7).choice(len(pts), 500, replace=False)].copy()
    dup["color"] ^= 0x00FFFFFF
    dev, u = _build_points(np.concatenate([pts, dup]), box, 40_000)
    full = dev.export_octree(u)
    q, bad, odd = nr.degenerate_batch(nr.wide(pts, box), box, extra=[Spheres.from_points(dup[:8], 0.0).record()])
    nbad = bad.stop - bad.start
    for k in (2, 8):
        res = full.neighbours(q, k, return_counts=True)
        nb, within, cnt = res
        assert int(cnt["numInvalid"]) == nbad and (within[bad] == 0).all() and (within[odd:odd + 8] == 2).all() and within[odd + 8] == 0
        assert within[odd + 9] > 0 and within[odd + 10] == full.truncated(20, "cut").num_samples
        _assert_matches(Raw(dev, u, q, k), res, f"degenerate queries k={k}")
    only_bad = Spheres.from_records(q.record()[bad])
    res = full.neighbours(only_bad, 8, return_counts=True)
    assert int(res[2]["numPairs"]) == 0 and int(res[2]["numInvalid"]) == nbad
    _assert_matches(Raw(dev, u, only_bad, 8), res, "invalid queries only")
    # rule 3 at its edge, and the whole box of ragged_tiny
    dev, u, pts, box, full = terrain
    res = full.neighbours(nr.edge_queries(box), 8, return_counts=True)
    _assert_matches(Raw(dev, u, nr.edge_queries(box), 8), res, "edge queries")
    tiny, u2, tp, tb = _build("ragged_tiny")
    whole = Spheres([[0.5, 0.5, 0.5]], 2.0)
    res = tiny.export_octree(u2).neighbours(whole, 16, return_counts=True)
    assert int(res[1][0]) == len(tp)
    _assert_matches(Raw(tiny, u2, whole, 16), res, "the whole box")


def test_visible_selection(built_libs):
    dev, u, pts, box = _build("terrain_4x100k")
    q = nr.wide(pts, box)
    before = Raw(dev, u, q, 8, 20, "visible", count_only=True)
    assert before.rc == 1 and before.untouched()                              # no frame yet: refused as the export refuses it
    dev.render(u)
    ex = dev.export_octree(u, select="visible")
    res = ex.neighbours_selected(q, 8, return_counts=True)
    assert (res[1] > 0).mean() >= 0.25
    nr.assert_found_index_export(res[0], ex, "visible")
    _assert_matches(Raw(dev, u, q, 8, 20, "visible"), res, "visible", ex)
    got, gw = dev.find_neighbours(u, q, 8, select="visible")
    assert got.tobytes() == res[0].tobytes() and np.array_equal(gw, res[1])


def test_the_limit_of_queries(terrain):
    """2^20 queries at k = 1: 4 096 real ones at every 256th place, all others far above the box with a small radius (valid, no pair)."""
    dev, u, pts, box, full = terrain
    n = abi.NEIGHBOURS_MAX
    rec = np.zeros(n, dtype=abi.sphere_dtype)
    rec["center"] = (300.0, 200.0, 50.0 * max(box))
    rec["radius"] = 0.5
    real = pts[np.sort(np.random.RandomState(45).choice(len(pts), 4096, replace=False))]
    rec[::256] = Spheres.from_points(real, nr.radii(pts, box)[1]).record()
    many = Spheres.from_records(rec)
    res = full.neighbours(many, 1, return_counts=True)
    nb, within, cnt = res
    assert int(cnt["numInvalid"]) == 0 and (within[::256] >= 1).all() and (nb["d2"][::256, 0] == 0).all() and (np.delete(within, np.s_[::256]) == 0).all()
    _assert_matches(Raw(dev, u, many, 1, want_table=False), res, "2^20 queries")
    over = Raw(dev, u, rec[:16], 1, num_queries=n + 1, count_only=True)
    assert over.rc == 1 and over.untouched()


def test_imported_octrees_and_a_shifted_box(built_libs):
    off = cases.GEOREF
    src, u, pts, box = _build("terrain_4x100k", off)
    full = src.export_octree(u)
    base_pts, base_box, _, _ = cases.case("terrain_4x100k")
    sets = {key: nr.shift_spheres(s, off) for key, s in nr.query_sets(base_pts, base_box).items()}
    want = {}
    for key, q in sets.items():
        for sel, ml in MODES:
            want[key, sel, ml] = full.neighbours(q, 8, ml, sel, return_counts=True)
    assert (want["wide", "cut", 20][1] > 8).mean() >= 0.25
    for (key, sel, ml), res in want.items():
        _assert_matches(Raw(src, u, sets[key], 8, ml, sel), res, f"georef {key} {sel}@{ml}")
    nr.assert_found_are_brute(*want["wide", "cut", 20][:2], sets["wide"], pts, 8, "georef")
    for buildable in (False, True):
        dst = _device()
        dst.nodes.fill_(0xA5)
        if buildable:
            dst.import_octree(full, buildable=True, uniforms=u)
        else:
            dst.import_octree(full)
        back = dst.export_octree(u)
        assert back.nodes.tobytes() == full.nodes.tobytes() and back.samples.tobytes() == full.samples.tobytes()
        for (key, sel, ml), res in want.items():
            _assert_matches(Raw(dst, u, sets[key], 8, ml, sel), res, f"imported (buildable={buildable}) {key} {sel}@{ml}")


def test_queries_leave_their_source_alone(built_libs):
    name = "terrain_4x100k"
    pts, box, batch, T = cases.case(name)
    dev = _device()
    u = dev.uniforms(W, H, T, box)
    dev.reset(u)
    batches = cases.batches_of(name, pts, batch)
    _ingest(dev, u, batches[:2])
    before = dev.export_octree(u)
    for key, q in nr.query_sets(pts, box).items():
        dev.find_neighbours(u, q, 8, select="all")
        dev.count_neighbours(u, q, 16, max_level=1)
    after = dev.export_octree(u)
    assert before.nodes.tobytes() == after.nodes.tobytes() and before.samples.tobytes() == after.samples.tobytes()
    _ingest(dev, u, batches[2:])
    ref = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=8)
    ref.reset(u)
    ref.add_points(u, pts, batch)
    nodes, pers, n = host_image_of(dev)
    assert_dumps_equal(oracle.dump_image(nodes, n), ref.dump(), name)
    assert_stats_equal(dev.read_stats(), ref.stats[0], STATS_BUILD_FIELDS, name)


def test_queries_alternate_on_one_scratch(built_libs):
    """The ray and the neighbour query share the pair kernels, the scratch layout and, through DeviceOctree, one cached scratch tensor: calls
    of both in turn (CUT @ 20) return what each returns alone, and no call sees what the one before left in the buffer."""
    name = "uniform_3x40k"
    dev, u, pts, box = _build(name)
    full = dev.export_octree(u)
    rays = yr.ray_sets(name, pts, box)["vertical r0.003"][0]
    q, k = nr.wide(pts, box), 8
    hits, rc = full.cast(rays, return_counts=True)
    nb, within, nc = full.neighbours(q, k, return_counts=True)
    assert int(rc["numHits"]) > 0 and int(rc["numPairs"]) > 0 and int(nc["numPairs"]) > 0 and int(nc["numWithin"]) > 0
    first = dev.cast_rays(u, rays)
    got, gw = dev.find_neighbours(u, q, k)
    again = dev.cast_rays(u, rays)
    crays = dev.count_rays(u, rays)
    cnb = dev.count_neighbours(u, q, k)
    assert first.tobytes() == hits.tobytes() and again.tobytes() == first.tobytes()
    assert got.tobytes() == nb.tobytes() and np.array_equal(gw, within)
    assert {f: int(crays[f]) for f in abi.ray_counts_dtype.names} == {f: int(rc[f]) for f in abi.ray_counts_dtype.names}
    same = [f for f in COUNT_FIELDS if f not in ("numFound", "numWithin")]
    assert {f: int(cnb[f]) for f in same} == {f: int(nc[f]) for f in same}
    assert int(cnb["numFound"]) == 0 and int(cnb["numWithin"]) == 0
