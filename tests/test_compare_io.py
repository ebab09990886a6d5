"""CPU tier of the compare queries (include/simlod_hip.h, "compare queries"): the numpy mirror octree_io.compare_samples against the per-sample
brute force of tests/compare_ref.py — records, colours and the summary record byte for byte — on the inputs the GPU tier runs; the budget and
the count-only form; the numpy mirror of the header's hash; and the Compare class."""
import numpy as np
import pytest

import compare_ref as cr
from simlod_amd import abi
from simlod_amd.octree_io import Compare, OctreeExport, compare_cells, compare_h, compare_home, compare_samples, compare_table_slots

PALETTE = [0xFF0000FF, 0xFF00FFFF, 0xFF00FF00, 0xFFFF0000]


def _compare(radius, **kw):
    """A ramp whose bins are narrower than the radius, so that several bins, bin 255 and the miss colour all occur."""
    return Compare.linear(0.75 * radius if radius > 0 else 1.0, PALETTE, radius=radius, miss_color=0xFF123456, **kw)


def _size(mn, mx):
    return float((np.asarray(mx, np.float32) - np.asarray(mn, np.float32)).max())


def _same(got, want, what):
    for g, w, name in zip(got, want, ("records", "colours", "summary")):
        assert (g is None) == (w is None), f"{what}: {name}"
        if g is not None and g.tobytes() != w.tobytes():
            if name == "summary":
                bad = [(f, g[f], w[f]) for f in g.dtype.names if np.asarray(g[f]).tobytes() != np.asarray(w[f]).tobytes()]
            else:
                assert len(g) == len(w), f"{what}: {len(g)} {name}, {len(w)} wanted"
                rows = lambda v: np.ascontiguousarray(v).view(np.uint8).reshape(len(v), -1)
                bad = [(int(i), g[i], w[i]) for i in np.flatnonzero((rows(g) != rows(w)).any(axis=1))[:5]]
            raise AssertionError(f"{what}: {name} differ: {bad}")


@pytest.mark.parametrize("name", cr.CASES)
def test_mirror_equals_the_brute_force(name):
    a, b, mn, mx, radius = cr.case(name)
    a = a[: cr.EXACT_A_LIMIT.get(name, len(a))]
    cmp = _compare(radius)
    want = cr.compare_exact(a, b, mn, _size(mn, mx), radius, cmp.thresholds2, cmp.table, cmp.miss_color)
    got = compare_samples(a, b, (mn, mx), cmp)
    _same(got, want, name)
    s = got[2]
    assert int(s["hist"].sum()) == len(a) and int(s["hist"][:256].sum()) == int(s["numMatched"])
    # the count-only form: the same grid fields, nothing else
    c = compare_samples(a, b, (mn, mx), cmp, count_only=True)
    assert c[0] is None and c[1] is None
    for f in ("error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numCandidates"):
        assert int(c[2][f]) == int(s[f]), f
    assert int(c[2]["numMatched"]) == int(c[2]["numWithin"]) == 0 and float(c[2]["maxD2"]) == 0.0 and not c[2]["hist"].any()
    _same(c, cr.compare_exact(a, b, mn, _size(mn, mx), radius, cmp.thresholds2, cmp.table, cmp.miss_color, count_only=True), name + " count only")


def test_what_the_cases_cover():
    """The cases hold what their names promise — ties, d2 == rr, a hot cell, distinct cells, invalid samples, the floor of h."""
    got = {}
    for name in cr.CASES:
        a, b, mn, mx, radius = cr.case(name)
        got[name] = (a, b, radius) + compare_samples(a, b, (mn, mx), _compare(radius))
    rec = got["lattice"][3]
    inner = rec["within"] == 7                                              # itself and six neighbours at exactly the radius
    assert inner.sum() == 4 ** 3 and (rec["d2"] == 0.0).all() and (rec["nearest"] == np.arange(len(rec))).all()
    rec = got["lattice_ulp"][3]
    assert (rec["d2"] > 0).all() and len(set(rec["within"].tolist())) > 3    # the ulp decides which of the six still pass
    assert int(got["one_matched"][5]["numMatched"]) == 1 and int(got["one_unmatched"][5]["hist"][256]) == 1
    assert float(got["one_coincident_r0"][3]["d2"][0]) == 0.0 and int(got["one_coincident_r0"][3]["within"][0]) == 1
    s = got["hot_cell"][5]
    assert int(s["numCells"]) == 1 and int(s["maxCellPopulation"]) == 3000 and 0 < int(s["numMatched"]) < 1100
    s = got["distinct_cells"][5]
    assert int(s["numCells"]) == 20000 and int(s["maxCellPopulation"]) == 1
    s = got["invalid"][5]
    assert int(s["numInvalidA"]) == 6 and int(s["numInvalidB"]) == 6 and int(s["hist"][256]) >= 6
    rec = got["invalid"][3]
    assert rec["within"][22] >= 1 and rec["within"][23] >= 1 and rec["d2"][22] == 0.0   # the samples at +-1e30 match in the edge cells
    s = got["b_outside"][5]
    assert 0 < int(s["numMatched"]) <= 30                                   # only a's samples near the face reach b
    rec = got["r0_duplicates"][3]
    assert (rec["within"][:40] >= 2).any() and (rec["within"][40:] == 0).all() and (rec["nearest"][:40] < 80).all()
    a, b, radius = got["h_floor"][:3]
    assert compare_h(radius, 4.0) == 4.0 * 2.0 ** -20 and 0 < int(got["h_floor"][5]["numMatched"]) < 100
    rec = got["cell_faces"][3]
    assert (rec["within"] >= 1).all()                                       # b at distance r: found across every face


def test_worked_example_of_the_integration_guide():
    """INTEGRATION §8, "Comparing two clouds": box [0, 4)^3, r = 0.5, one sample of a and three of b."""
    a, b = cr.points([[1.0, 1.0, 1.0]]), cr.points([[1.5, 1.0, 1.0], [1.0, 1.5, 1.0], [1.6, 1.0, 1.0]])
    cmp = Compare.linear(0.5, PALETTE)
    assert compare_h(0.5, 4.0) == 0.50048828125 and cmp.thresholds2[254] == 0.25
    rec, col, s = compare_samples(a, b, ((0, 0, 0), (4, 4, 4)), cmp)
    assert (float(rec["d2"][0]), int(rec["nearest"][0]), int(rec["within"][0])) == (0.25, 0, 2) and int(col[0]) == int(cmp.table[255])
    assert (int(s["numCells"]), int(s["numCandidates"]), int(s["hist"][255]), float(s["maxD2"])) == (3, 2, 1, 0.25)
    _same((rec, col, s), cr.compare_exact(a, b, (0, 0, 0), 4.0, 0.5, cmp.thresholds2, cmp.table, 0), "worked example")


def test_budget():
    a, b, mn, mx, radius = cr.case("hot_cell")
    a = a[:200]
    n = int(compare_samples(a, b, (mn, mx), _compare(radius), count_only=True)[2]["numCandidates"])
    assert n > 0
    for budget, runs in ((n + 1, True), (n, True), (n - 1, False)):
        rec, col, s = compare_samples(a, b, (mn, mx), _compare(radius, max_candidates=budget))
        assert (rec is not None) == runs and int(s["error"]) == (0 if runs else abi.COMPARE_ERR_BUDGET) and int(s["numCandidates"]) == n
        want = cr.compare_exact(a[:20], b, mn, _size(mn, mx), radius, _compare(radius).thresholds2, _compare(radius).table, 0xFF123456,
                                max_candidates=budget)
        assert (want[0] is None) == (compare_samples(a[:20], b, (mn, mx), _compare(radius, max_candidates=budget))[0] is None)


def test_hash_mirror_and_table_slots():
    for n, want in ((1, 2), (2, 4), (3, 8), (4, 8), (5, 16), (1 << 20, 1 << 21), ((1 << 20) + 1, 1 << 22), (abi.COMPARE_MAX_COUNT, 1 << 33)):
        assert compare_table_slots(n) == cr.table_slots(n) == want
    rs = np.random.RandomState(3)
    keys = rs.randint(0, 1 << 60, 500, dtype=np.uint64)
    for slots in (2, 8, 1 << 15, 1 << 33):
        home = compare_home(keys, slots)
        assert home.tolist() == [cr.home_of(int(k), slots) for k in keys] and int(home.max()) < slots
    a, b, mn, mx, radius = cr.case("invalid")
    inv = 1.0 / compare_h(radius, _size(mn, mx))
    valid, keys = compare_cells(b, np.asarray(mn, np.float64), np.float64(inv))
    xyz = cr._xyz(b)
    for j, p in enumerate(xyz):
        assert bool(valid[j]) == cr.is_valid(*p)
        if valid[j]:
            assert int(keys[j]) == cr.key_of(cr.cell_of(p, [float(np.float32(v)) for v in mn], inv))


def test_compare_class():
    c = Compare.linear(2.0, PALETTE, radius=1.5, miss_color=7, max_candidates=99, max_workgroups=3)
    assert c.thresholds2[0] == (2.0 / 255.0) ** 2 and c.thresholds2[254] == 4.0 and float(c.radius) == 1.5
    assert c.table[0] == PALETTE[0] and c.table[255] == PALETTE[3] and len(set(c.table.tolist())) == 4
    r = c.record()
    assert r.dtype == abi.compare_params_dtype and int(r["reserved"][0]) == 0 and int(r["maxCandidates"][0]) == 99 and int(r["maxWorkgroups"][0]) == 3
    assert Compare.from_record(r) == c and Compare.from_record(r).record().tobytes() == r.tobytes()
    assert int(c.record(max_candidates=5)["maxCandidates"][0]) == 5 and int(Compare.linear(1.0, PALETTE).record()["maxCandidates"][0]) == 0
    assert c.index([0.0, c.thresholds2[0], np.nextafter(c.thresholds2[0], 0.0), 4.0, 100.0]).tolist() == [0, 1, 0, 255, 255]
    assert [cr.index_of(c.thresholds2.tolist(), v) for v in (0.0, c.thresholds2[0], 4.0)] == [0, 1, 255]
    s = np.zeros((), dtype=abi.compare_summary_dtype)
    s["maxD2"] = 9.0
    f = Compare.from_summary(s, PALETTE, radius=5.0)
    assert f.thresholds2[254] == 9.0 and float(f.radius) == 5.0
    assert Compare.from_summary(np.zeros((), dtype=abi.compare_summary_dtype), PALETTE, radius=5.0).thresholds2[254] == 25.0
    for bad in (dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(radius=1e39)):
        with pytest.raises(ValueError):
            Compare.linear(1.0, PALETTE, **bad)
    t = c.thresholds2.copy()
    t[10] = t[9] / 2
    with pytest.raises(ValueError):
        Compare(1.0, t, c.table)
    with pytest.raises(ValueError):
        Compare(1.0, c.thresholds2[:-1], c.table)
    with pytest.raises(ValueError):
        Compare.linear(0.0, PALETTE)


def test_export_compare():
    """OctreeExport.compare: two exports' samples through compare_samples, in the first one's box."""
    a, b, mn, mx, radius = cr.case("lattice_ulp")
    table = np.zeros(1, dtype=abi.export_node_dtype)
    ea, eb = OctreeExport(table, a, mn, mx), OctreeExport(table, b, mn, mx)
    got = ea.compare(eb, _compare(radius))
    _same(got, compare_samples(a, b, (mn, mx), _compare(radius)), "export")
