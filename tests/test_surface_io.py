"""CPU tier of the surface queries (include/simlod_hip.h, "surface queries"): the host mirror octree_io.surface_samples against
tests/surface_ref.py's one-sample-at-a-time restatement of rules N1-N10, byte for byte, on every case and for both colourBy values; what each
case is there to show; independence of b's order; the budget; count only; the Surface class, its classmethods and every refusal;
unit_normals and variation; INTEGRATION's worked example; and the rule's accuracy against numpy.linalg.eigh."""
import numpy as np
import pytest

import compare_ref as cr
import surface_ref as sf
from simlod_amd import abi
from simlod_amd.octree_io import Compare, Surface, compare_samples, surface_normals64, surface_samples, surface_unit_normals, surface_variation

SUBNORMAL = 2.2250738585072014e-308
PALETTE = [0xFF0000FF, 0xFF00FFFF, 0xFF00FF00, 0xFFFF0000]


def _size(mn, mx):
    return float((np.asarray(mx, np.float32) - np.asarray(mn, np.float32)).max())


def _both(name, colour_by, variant=0, trace=None, **kw):
    """(the case, the mirror's result, the reference's) for one variant of a case; a big case on the part of a the brute force can take."""
    a, b, mn, mx, radius, _ = sf.case(name)
    a = a[: sf.EXACT_A_LIMIT.get(name)]
    rec = sf.case_params(name, colour_by, **kw)[variant]
    got = surface_samples(a, b, (mn, mx), Surface.from_record(rec))
    want = sf.surface_exact(a, b, np.asarray(mn, np.float32), _size(mn, mx), rec, trace=trace)
    return (a, b, mn, mx, radius, rec), got, want


def _same(got, want, what):
    assert got[2].tobytes() == want[2].tobytes(), (what, got[2], want[2])
    if want[0] is None:
        assert got[0] is None and got[1] is None, what
        return
    bad = np.flatnonzero((got[0].view(np.uint8).reshape(-1, 32) != want[0].view(np.uint8).reshape(-1, 32)).any(axis=1))
    assert len(bad) == 0, (what, [(int(i), got[0][i], want[0][i]) for i in bad[:4]])
    assert got[1].tobytes() == want[1].tobytes(), what


@pytest.mark.parametrize("colour_by", [sf.SHADE, sf.VARIATION])
@pytest.mark.parametrize("name", sf.CASES)
def test_mirror_equals_the_reference(name, colour_by):
    for variant in range(len(sf.case(name)[5])):
        (a, b, mn, mx, radius, rec), got, want = _both(name, colour_by, variant)
        _same(got, want, (name, colour_by, variant))
        s = got[2]
        assert int(s["numEstimated"]) + int(s["numDegenerate"]) + int(s["numInvalidA"]) == len(a) == int(s["hist"].sum())
        assert int(s["hist"][256]) == int(s["numDegenerate"]) + int(s["numInvalidA"]) and int(s["numWithin"]) == int(got[0]["within"].sum())
    if name in sf.EXACT_A_LIMIT:                                            # the whole of a: its first records are the part's
        a, b, mn, mx, radius, _ = sf.case(name)
        full = surface_samples(a, b, (mn, mx), Surface.from_record(sf.case_params(name, colour_by)[0]))
        assert full[0][: len(got[0])].tobytes() == got[0].tobytes() and full[1][: len(got[1])].tobytes() == got[1].tobytes()


def test_what_the_small_cases_show():
    _, got, _ = _both("three_points", sf.SHADE)
    assert (got[0]["within"] == 3).all() and int(got[2]["numEstimated"]) == 3 and (got[0]["lambdaDen"] > 0).all()
    for name, n in (("two_points", 2), ("coincident", 5)):
        _, got, _ = _both(name, sf.VARIATION)
        assert int(got[2]["numDegenerate"]) == n == int(got[2]["hist"][256]) and (got[0]["within"] == n).all() and (got[1] == sf.MISS_COLOR).all()
        assert not got[0]["normal"].any() and not got[0]["lambdaNum"].any() and not got[0]["lambdaDen"].any()
    _, got, _ = _both("collinear", sf.SHADE)                               # rank 1: v is still defined, and perpendicular to the line
    assert int(got[2]["numEstimated"]) == 7
    assert (np.abs(surface_unit_normals(got[0]) @ (np.array([1 / 64.0, 1 / 32.0, -1 / 128.0]) * 64 / np.sqrt(5.25))) < 1e-3).all()
    (a, *_), got, _ = _both("r0", sf.SHADE)
    assert int(got[2]["numDegenerate"]) == len(a) and int(got[2]["numEstimated"]) == 0 and (got[0]["within"][:30] >= 1).all()
    (a, *_), got, _ = _both("invalid", sf.SHADE)
    assert int(got[2]["numInvalidA"]) == 6 and int(got[2]["numInvalidB"]) == 6 and (got[0]["within"][:6] == 0).all() and (got[1][:6] == sf.MISS_COLOR).all()
    _, got, _ = _both("b_outside", sf.SHADE)
    assert 0 < int(got[2]["numEstimated"]) and 0 < int(got[2]["numDegenerate"])


def test_plane_grid_normals_are_the_planes():
    """The lattice's offsets stay on the plane z = x - 0.5 after quantisation (pz == px exactly), so every interior normal is the plane's to
    1e-12 in the sine, oriented towards +z."""
    (a, *_), got, _ = _both("plane_grid", sf.SHADE)
    n = surface_unit_normals(got[0]).reshape(7, 7, 3)[1:6, 1:6].reshape(-1, 3)
    want = np.array(sf.PLANE_NORMAL) / np.sqrt(2.0)
    sine = np.sqrt((np.cross(n, want) ** 2).sum(axis=1))
    assert len(n) == 25 and sine.max() <= 1e-12 and (n @ want > 0).all(), sine.max()
    assert (got[0]["within"].reshape(7, 7)[1:6, 1:6] == 5).all() and (surface_variation(got[0]).reshape(7, 7)[1:6, 1:6] <= 1e-30).all()


def test_line_tiny_passes_through_subnormals():
    trace = []
    _, got, want = _both("line_tiny", sf.SHADE, trace=trace)
    _same(got, want, "line_tiny")
    small = [x for t in trace if t for m in t[2:] for x in m if x != 0.0 and abs(x) < SUBNORMAL]
    assert len(small) >= 30 and int(got[2]["numEstimated"]) == 100


def test_cell_faces_and_wide_sums_reach_what_they_are_for():
    a, b, mn, mx, radius, _ = sf.case("cell_faces")
    inv = cr.inv_of(float(np.float32(radius)), 4.0)
    pa, pb = cr._xyz(a), cr._xyz(b)
    rr = float(np.float32(radius)) ** 2
    near = [s for s in pb if cr.d2_of(s, pa[0]) <= rr]
    c0 = cr.cell_of(pa[0], mn, inv)
    offs = {tuple(np.subtract(cr.cell_of(s, mn, inv), c0)) for s in near}
    assert len(near) >= 27 and len(offs) == 27                              # the mid-cell centre has a neighbour in each of its 27 cells
    cells = {cr.cell_of(p, mn, inv)[k] for p in pa[1:] for k in range(3)}
    assert {1, 2, 6, 7} <= cells and cells & {8, 9}                         # the face centres fall on both sides; the corner at cell 9's
    a, b, mn, mx, radius, _ = sf.case("wide_sums")
    pa, pb = cr._xyz(a), cr._xyz(b)
    S, within = sf.sums_of(pa[0], pb, range(len(pb)), radius * radius, sf.invq_of(radius, 4.0))
    assert within > 100 and min(S[3], S[6], S[8]) >= 1 << 32 and max(S[0], S[1], S[2]) < 0
    assert sf.widen(S[0]) == float(S[0]) and sf.widen(S[3]) == float(S[3])


def test_orientation():
    """orient_flip's variants on the flat patch (z constant: v = (+-0, +-0, v2)): a direction below flips, a direction or a sensor IN the plane
    gives s == 0 and keeps, a zero direction never flips, a sensor below flips and one above keeps."""
    flat = slice(0, 25)
    z = []
    for variant in range(6):
        _, got, want = _both("orient_flip", sf.SHADE, variant)
        _same(got, want, variant)
        n = got[0]["normal"][flat]
        assert not n[:, :2].any() and (n[:, 2] != 0).all()
        z.append(np.sign(n[:, 2]))
    assert (z[0] < 0).all() and (z[4] < 0).all()                            # flipped
    for k in (1, 2, 3, 5):                                                  # kept: the rule's own sign, that of column j*'s diagonal entry
        assert (z[k] > 0).all(), k
    # everywhere else a flip changes the sign of the whole normal and nothing else
    up, down = _both("orient_flip", sf.SHADE, 5)[1][0], _both("orient_flip", sf.SHADE, 4)[1][0]
    assert (np.abs(up["normal"]) == np.abs(down["normal"])).all() and up["lambdaNum"].tobytes() == down["lambdaNum"].tobytes()


def test_threshold_edges():
    """thresholds[i] * den == num exactly: light along the flat patch's normal meets the threshold 1 (index 255), against it the threshold
    -1 (index 1); a perfect plane's lambdaNum == 0 meets the threshold 0 (index 1)."""
    flat = slice(0, 25)
    (_, _, _, _, _, rec), got, want = _both("shade_edges", sf.SHADE, 0)
    _same(got, want, "along")
    assert float(rec["thresholds"][0][254]) == 1.0 and float(rec["thresholds"][0][0]) == -1.0
    assert (got[1][flat] == sf.TABLE[255]).all() and int(got[2]["hist"][255]) >= 25
    _, got, want = _both("shade_edges", sf.SHADE, 1)
    _same(got, want, "against")
    assert (got[1][flat] == sf.TABLE[1]).all()
    (_, _, _, _, _, rec), got, want = _both("variation_edges", sf.VARIATION)
    _same(got, want, "variation")
    assert float(rec["thresholds"][0][0]) == 0.0 and (got[0]["lambdaNum"][flat] == 0.0).all() and (got[0]["lambdaDen"][flat] > 0.0).all()
    assert (got[1][flat] == sf.TABLE[1]).all() and (surface_variation(got[0])[50:] > 0.01).all()


@pytest.mark.parametrize("name", ["hot_cell", "cell_faces", "wide_sums", "invalid"])
def test_records_do_not_depend_on_the_order_of_b(name):
    a, b, mn, mx, radius, _ = sf.case(name)
    s = Surface.from_record(sf.case_params(name, sf.VARIATION)[0])
    first = surface_samples(a, b, (mn, mx), s)
    again = surface_samples(a, b[np.random.RandomState(3).permutation(len(b))], (mn, mx), s)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))


def test_budget_and_count_only():
    a, b, mn, mx, radius, _ = sf.case("hot_cell")
    a = a[:40]
    size = _size(mn, mx)
    n = int(surface_samples(a, b, (mn, mx), Surface.from_record(sf.params(radius, sf.SHADE)), count_only=True)[2]["numCandidates"])
    assert n > 1
    for budget, runs in ((n + 1, True), (n, True), (n - 1, False)):
        rec = sf.params(radius, sf.SHADE, budget=budget)
        got = surface_samples(a, b, (mn, mx), Surface.from_record(rec))
        _same(got, sf.surface_exact(a, b, np.asarray(mn, np.float32), size, rec), budget)
        assert (got[0] is not None) == runs and int(got[2]["error"]) == (0 if runs else abi.SURFACE_ERR_BUDGET) and int(got[2]["numCandidates"]) == n
        c = surface_samples(a, b, (mn, mx), Surface.from_record(rec), count_only=True)
        _same(c, sf.surface_exact(a, b, np.asarray(mn, np.float32), size, rec, count_only=True), budget)
        assert c[0] is None and int(c[2]["numEstimated"]) == 0 and not c[2]["hist"].any() and int(c[2]["error"]) == int(got[2]["error"])
    # the grid's fields are the compare query's, field for field
    cmp = compare_samples(a, b, (mn, mx), Compare.linear(1.0, PALETTE, radius=radius), count_only=True)[2]
    for f in ("numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numCandidates"):
        assert int(cmp[f]) == int(c[2][f])


def test_surface_class():
    h = Surface.hillshade(0.5, (1.0, 1.0, 2.0), PALETTE, miss_color=7, max_candidates=9, max_workgroups=3)
    c = -1.0 + np.arange(1, 256) / 128.0
    assert h.thresholds.tobytes() == (c * np.abs(c)).tobytes() == np.array(sf.shade_thresholds()).tobytes() and h.colour_by == abi.SURFACE_SHADE
    assert -1.0 < h.thresholds[0] and h.thresholds[254] < 1.0 and h.thresholds[127] == 0.0
    assert h.orient.tolist() == [0.0, 0.0, 1.0] and h.orient_mode == abi.SURFACE_ORIENT_DIRECTION and h.table[0] == PALETTE[0] and h.table[255] == PALETTE[3]
    v = Surface.variation(0.5, 1.0 / 3.0, PALETTE, orient=(1.0, 2.0, 3.0), orient_mode="position")
    assert v.thresholds.tobytes() == np.array(sf.variation_thresholds()).tobytes() and v.colour_by == abi.SURFACE_VARIATION and v.thresholds[254] == 1.0 / 3.0
    assert v.orient_mode == abi.SURFACE_ORIENT_POSITION and v.max_candidates is None
    for s in (h, v):
        r = s.record()
        assert r.dtype == abi.surface_params_dtype and r.shape == (1,) and int(r["reserved"][0]) == 0 and sf.params_acceptable(r)
        assert Surface.from_record(r) == s and Surface.from_record(r).record().tobytes() == r.tobytes()
    assert h != v and h != Surface.hillshade(0.5, (1.0, 1.0, 2.0), PALETTE, miss_color=8, max_candidates=9, max_workgroups=3)
    assert int(h.record()["maxCandidates"][0]) == 9 and int(h.record(11)["maxCandidates"][0]) == 11 and int(v.record()["maxCandidates"][0]) == 0
    # index(): the binary search counts the thresholds with t * den <= num
    num, den = np.array([-5.0, -1.0, -0.5, 0.0, 0.3, 1.0, 4.0, 0.0]), np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0])
    assert h.index(num, den).tolist() == [sf.index_of(sf.shade_thresholds(), x, y) for x, y in zip(num, den)]
    t, tab = sf.shade_thresholds(), sf.TABLE
    bad_t = lambda i, x: [x if k == i else y for k, y in enumerate(t)]
    for what, make in (("radius < 0", lambda: Surface(-1.0, t, tab)), ("radius NaN", lambda: Surface(np.nan, t, tab)), ("radius inf", lambda: Surface(np.inf, t, tab)),
                       ("radius beyond float32", lambda: Surface(1e39, t, tab)), ("254 thresholds", lambda: Surface(1.0, t[:254], tab)),
                       ("255 table entries", lambda: Surface(1.0, t, tab[:255])), ("threshold NaN", lambda: Surface(1.0, bad_t(9, np.nan), tab)),
                       ("threshold inf", lambda: Surface(1.0, bad_t(254, np.inf), tab)), ("descending", lambda: Surface(1.0, bad_t(100, -2.0), tab)),
                       ("colour_by 2", lambda: Surface(1.0, t, tab, colour_by=2)), ("orient_mode 2", lambda: Surface(1.0, t, tab, orient_mode=2)),
                       ("orient_mode name", lambda: Surface(1.0, t, tab, orient_mode="sideways")), ("light NaN", lambda: Surface(1.0, t, tab, light=(0.0, np.nan, 1.0))),
                       ("light inf, unused", lambda: Surface(1.0, t, tab, colour_by=abi.SURFACE_VARIATION, light=(np.inf, 0.0, 1.0))),
                       ("orient inf", lambda: Surface(1.0, t, tab, orient=(0.0, 0.0, -np.inf))), ("orient beyond float32", lambda: Surface(1.0, t, tab, orient=(1e39, 0.0, 0.0))),
                       ("zero light", lambda: Surface(1.0, t, tab, light=(0.0, -0.0, 0.0))), ("two light values", lambda: Surface(1.0, t, tab, light=(0.0, 1.0))),
                       ("miss colour", lambda: Surface(1.0, t, tab, miss_color=1 << 32)), ("budget < 0", lambda: Surface(1.0, t, tab, max_candidates=-1)),
                       ("vmax 0", lambda: Surface.variation(1.0, 0.0, PALETTE)), ("no colour", lambda: Surface.hillshade(1.0, (0, 0, 1), [])),
                       ("reserved", lambda: Surface.from_record(sf.params(1.0, sf.SHADE, reserved=1)))):
        with pytest.raises(ValueError):
            make()
        assert what
    assert Surface(1.0, t, tab, colour_by=abi.SURFACE_VARIATION, light=(0.0, 0.0, 0.0)).light.tolist() == [0.0, 0.0, 0.0]   # a zero light is fine unused
    assert Surface(0.0, np.zeros(255), tab, orient=(0.0, 0.0, 0.0)).radius == 0.0
    # the class and the reference agree on which records are acceptable
    for kw, ok in ((dict(radius=-1.0), False), (dict(light=(0.0, 0.0, 0.0)), False), (dict(orient=(np.nan, 0.0, 0.0)), False), (dict(reserved=2), False),
                   (dict(thresholds=bad_t(3, 5.0)), False), (dict(orient_mode=sf.POSITION), True), (dict(radius=0.0), True)):
        kw = dict(dict(radius=1.0, colour_by=sf.SHADE), **kw)
        assert sf.params_acceptable(sf.params(**kw)) == ok, kw


def test_unit_normals_and_variation():
    _, got, _ = _both("invalid", sf.VARIATION)
    rec = got[0]
    n, v = surface_unit_normals(rec), surface_variation(rec)
    est = rec["lambdaDen"] != 0
    assert n.dtype == np.float64 and n.shape == (len(rec), 3) and v.dtype == np.float64 and 0 < est.sum() < len(rec)
    assert np.allclose((n[est] ** 2).sum(axis=1), 1.0, atol=1e-12) and not n[~est].any() and not v[~est].any()
    assert (v[est] == rec["lambdaNum"][est] / rec["lambdaDen"][est]).all() and (v >= -1e-15).all() and (v <= 1.0 / 3.0 + 1e-12).all()
    assert (n[est][:, 2] >= 0).all()                                        # orient = (0, 0, 1)


def test_integration_worked_example():
    """INTEGRATION §8, "surface queries": three points in a box of size 4, radius 0.5, the sample (1, 1, 1)."""
    a, b, mn, mx, radius, _ = sf.case("three_points")
    assert cr.h_of(radius, 4.0) == 0.50048828125 and sf.invq_of(radius, 4.0) == 32736.031219512195
    pa = cr._xyz(a)
    S, within = sf.sums_of(pa[0], pa, [0, 1, 2], radius * radius, sf.invq_of(radius, 4.0))
    assert (S, within) == ([8184, 8184, 2046, 66977856, 0, 0, 66977856, 16744464, 4186116], 3)
    M = sf.moments(S, within)
    assert M == [133955712.0, -66977856.0, -16744464.0, 133955712.0, 33488928.0, 8372232.0]
    f, ok = sf.factor_of(M)
    assert f == 2.0 ** -26 and ok and sf.scale(M)[0][0] == 1.9960956573486328
    v, lnum, lden, vv = sf.estimate(S, within, pa[0], [0.0, 0.0, 1.0], sf.DIRECTION)
    assert v == [2.156301243799136e-17, -0.3674784984962579, 1.4699139939850316] and v[1] / v[2] == -0.25
    assert (lnum, lden, vv) == (1.1969876444468319e-33, 9.451224836919279, 2.295687596570092)
    assert sf.colour_terms((v, lnum, lden, vv), sf.SHADE, [0.0, 0.0, 1.0]) == (2.1606471497130277, 2.295687596570092)
    got = surface_samples(a, b, (mn, mx), Surface.hillshade(radius, (0.0, 0.0, 1.0), sf.TABLE, miss_color=sf.MISS_COLOR))
    assert got[0]["normal"][0].tolist() == [float(np.float32(x)) for x in v] and got[0]["lambdaDen"][0] == lden and int(got[0]["within"][0]) == 3
    assert int(got[2]["hist"][252]) == 3 and (got[1] == sf.TABLE[252]).all() and int(got[2]["numWithin"]) == 9 == int(got[2]["numCandidates"])
    assert (Surface.variation(radius, 1.0 / 3.0, sf.TABLE).index(lnum, lden)) == 0


def test_normals_against_eigh():
    """The rule's accuracy against an independent reference: 1 728 random patches of 12 samples (flat, elongated, tilted at random), the
    mirror's normal in float64 — before the record rounds it to float32, which alone costs 6e-8 — against numpy.linalg.eigh's eigenvector of the smallest eigenvalue of the SAME M (from the exact integer sums).  For a
    patch with g = (l2 - l1) / (l2 + l3) >= 1/8 the sine of the angle is at most 1e-12: (7/8)^256 = 1.4e-15 for the method, times three
    orders of magnitude for the rounding of eight 3x3 squarings (the prototype's worst case was 1.5e-15)."""
    rs = np.random.RandomState(11)
    r, per = 0.05, 12
    g3 = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = 0.35 + g3 * 0.3
    pts = np.zeros((len(centres), per, 3))
    for i in range(len(centres)):
        rot = np.linalg.qr(rs.randn(3, 3))[0]
        scales = np.array([1.0, 0.4 + 0.6 * rs.rand(), 0.02 + 0.5 * rs.rand()])
        off = rs.rand(per, 3) * 2.0 - 1.0
        off /= np.maximum(1.0, np.sqrt((off ** 2).sum(axis=1)))[:, None]
        pts[i] = centres[i] + (off * scales * 0.9 * r) @ rot.T
        pts[i, 0] = centres[i]
    b = sf.points(pts.reshape(-1, 3))
    a = b[::per].copy()
    box, surface = ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0)), Surface.variation(r, 1.0 / 3.0, PALETTE, orient=(0.0, 0.0, 0.0))
    got = surface_samples(a, b, box, surface)
    rec, v64 = got[0], surface_normals64(a, b, box, surface)
    assert (v64.astype(np.float32) == rec["normal"]).all()                  # the records carry exactly these, rounded
    assert int(got[2]["numEstimated"]) == len(a) and (rec["within"] == per).all()
    invq, pb = sf.invq_of(float(np.float32(r)), 4.0), cr._xyz(b)
    rr = float(np.float32(r)) ** 2
    worst, checked = 0.0, 0
    for i in range(len(a)):
        S, n = sf.sums_of(pb[i * per], pb, range(i * per, (i + 1) * per), rr, invq)
        assert n == per
        M = np.array([[n * S[3] - S[0] * S[0], n * S[4] - S[0] * S[1], n * S[5] - S[0] * S[2]],
                      [n * S[4] - S[0] * S[1], n * S[6] - S[1] * S[1], n * S[7] - S[1] * S[2]],
                      [n * S[5] - S[0] * S[2], n * S[7] - S[1] * S[2], n * S[8] - S[2] * S[2]]], dtype=np.float64)   # exact: below 2^53
        lam, vec = np.linalg.eigh(M)
        if (lam[1] - lam[0]) / (lam[1] + lam[2]) < 0.125:
            continue
        checked += 1
        v = v64[i]
        sine = np.sqrt((np.cross(v, vec[:, 0]) ** 2).sum()) / np.sqrt((v ** 2).sum())
        worst = max(worst, sine)
        assert abs(float(rec["lambdaNum"][i]) / float(rec["lambdaDen"][i]) - lam[0] / lam.sum()) <= 1e-12
    print(f"patches with g >= 1/8: {checked} of {len(a)}; worst sine {worst:.3e}")
    assert checked >= 1000
    assert worst <= 1e-12, worst
