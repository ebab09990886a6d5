"""CPU tier: lasso queries (include/simlod_hip.h, "lasso queries") — the ABI struct, octree_io.Lasso, classify_lasso and the host mirrors
OctreeExport.crop / paint / summarize(lasso=) against a brute-force filter of the contract's input points, on octrees built by the oracle's
port, at the origin and in the shifted boxes of tests/test_gpu_box_origin.py; there the filter is lasso_ref.contains_exact as well, rule L1
with every comparison and every edge's side decided exactly."""
import os
import re

import numpy as np
import pytest

import cases
import footprint_ref as fr
import lasso_ref as lr
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Footprint, Lasso, Paint, Profile, Region, classify_lasso, classify_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = lr.MODES


def test_lasso_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodLasso\) == (\d+)", src).group(1)) == abi.lasso_dtype.itemsize == 2112
    offs = dict(re.findall(r"offsetof\(SimlodLasso, (\w+)\) == (\d+)", src))
    assert sorted(offs) == ["rowU", "rowV", "rowW", "vertices"]
    for f, o in offs.items():
        assert abi.lasso_dtype.fields[f][1] == int(o), f
    assert abi.lasso_dtype.fields["numVertices"][1] == 0 and abi.lasso_dtype.fields["reserved"][1] == 4
    assert int(re.search(r"#define SIMLOD_LASSO_MAX_VERTICES (\d+)u", src).group(1)) == abi.LASSO_MAX_VERTICES == 256
    r = Lasso([(1, 2), (3, 4), (5, 7)], (1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12)).record()
    assert r.dtype == abi.lasso_dtype and int(r["numVertices"][0]) == 3 and not r["reserved"].any()
    assert r["vertices"][0, :3].tolist() == [[1, 2], [3, 4], [5, 7]] and not r["vertices"][0, 3:].any()
    assert r["rowU"][0].tolist() == [1, 2, 3, 4] and r["rowV"][0].tolist() == [5, 6, 7, 8] and r["rowW"][0].tolist() == [9, 10, 11, 12]
    assert "NOT COVERED: perspective lassos" not in src


def test_lasso_symbols_exported(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_lasso_buffer_min_bytes", "simlod_query_lasso", "simlod_paint_lasso", "simlod_query_summary_lasso"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    for nn, bound in ((0, 0), (100, 0), (7000, 5_000_000)):
        assert L.simlod_lasso_buffer_min_bytes(nn, bound) == L.simlod_footprint_buffer_min_bytes(nn, bound)


def test_lasso_constructors():
    tri = [(0, 0), (1, 0), (0, 1)]
    rows = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 1))
    l = Lasso(tri, *rows)
    assert l.vertices.dtype == l.row_u.dtype == l.row_v.dtype == l.row_w.dtype == np.float32 and len(l) == 3
    assert len(Lasso(np.zeros((256, 2)), *rows)) == 256
    for bad in (tri[:2], np.zeros((257, 2)), [(0, 0), (1, np.nan), (0, 1)], [(0, 0), (1e39, 0), (0, 1)], [(0, 0), (np.inf, 0), (0, 1)]):
        with pytest.raises(ValueError):
            Lasso(bad, *rows)
    for k in range(3):
        for v in (np.nan, np.inf, 1e39):                # (1e39: infinite as float32)
            r = [list(x) for x in rows]
            r[k][2] = v
            with pytest.raises(ValueError):
                Lasso(tri, *r)
    Lasso(tri, rows[0], rows[1], (0, 0, 0, 0))          # a row W of zeros is legal
    # from_pixels / from_ndc: the rows the header states, computed in float64 and narrowed
    T = lr.transform("bird", (1.0, 1.0, 1.0))
    m = np.asarray(T, np.float64).reshape(4, 4)
    p = Lasso.from_pixels(T, 640, 480, tri)
    assert np.array_equal(p.row_u, (320.0 * (m[0] + m[3])).astype(np.float32)) and np.array_equal(p.row_v, (240.0 * (m[1] + m[3])).astype(np.float32))
    assert np.array_equal(p.row_w, m[3].astype(np.float32))
    n = Lasso.from_ndc(T, tri)
    assert np.array_equal(n.row_u, m[0].astype(np.float32)) and np.array_equal(n.row_v, m[1].astype(np.float32)) and np.array_equal(n.row_w, m[3].astype(np.float32))
    f = Footprint(tri, (1, 2, 3, 4), (5, 6, 7, 8))
    g = Lasso.from_footprint(f)
    assert np.array_equal(g.row_u, f.axis_u) and np.array_equal(g.row_v, f.axis_v) and g.row_w.tolist() == [0, 0, 0, 1] and np.array_equal(g.vertices, f.vertices)
    a_u, a_v, b_v, du, dv = g.edges()
    assert np.array_equal(g.edge_block(), np.stack([a_u, a_v, du, dv], axis=1)) and np.array_equal(b_v, np.roll(a_v, -1))


def _pts(xyz):
    p = np.zeros(len(xyz), dtype=abi.point_dtype)
    a = np.asarray(xyz, dtype=np.float32)
    p["x"], p["y"], p["z"] = a[:, 0], a[:, 1], a[:, 2]
    return p


def test_contains_is_the_even_odd_rule_in_front_of_the_eye():
    """Hand-made cases: the eye at the origin looking along +z (U = x, V = y, W = z: the screen position is (x/z, y/z))."""
    rows = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0))
    ell = Lasso([(0, 0), (4, 0), (4, 2), (2, 2), (2, 4), (0, 4)], *rows)                  # a concave L
    pts = _pts([(1, 1, 1), (3, 1, 1), (1, 3, 1), (3, 3, 1), (5, 1, 1), (2, 2, 2), (6, 6, 2), (6, 2, 2), (-1, 1, 1)])
    assert ell.contains(pts).tolist() == [True, True, True, False, False, True, False, True, False]
    # behind the eye the same screen position (x/z, y/z) does not count; nor does W == 0; nor a NaN
    assert ell.contains(_pts([(-1, -1, -1), (1, 1, -1), (1, 1, 0), (np.nan, 1, 1), (1, np.nan, 1), (1, 1, np.nan)])).tolist() == [False] * 6
    bow = Lasso([(0, 0), (4, 4), (0, 4), (4, 0)], *rows)                                  # two triangles meeting at (2, 2)
    assert bow.contains(_pts([(2, 1, 1), (2, 3, 1), (1, 2, 1), (3, 2, 1), (4, 2, 2), (4, 6, 2)])).tolist() == [True, True, False, False, True, True]
    flat = Lasso([(0, 0), (2, 2), (4, 4)], *rows)                                         # zero area: nothing off its own line
    assert not flat.contains(_pts([(1, 2, 1), (3, 1, 1), (2, 5, 1), (5, 5, 1), (-1, -1, 1)])).any()
    # a row W of zeros selects nothing
    assert not Lasso(ell.vertices, rows[0], rows[1], (0, 0, 0, 0)).contains(pts).any()
    # the rule is watertight at a vertex's height: points whose V equals a vertex's a_v * W exactly are in or out, never both ways
    v = ell.contains(_pts([(1, 2, 1), (3, 2, 1), (2, 4, 2), (6, 4, 2)]))
    assert v.tolist() == [True, False, True, False]


def test_convex_triangle_against_the_divided_screen_position():
    """An independent statement that divides: inside a convex triangle iff the three edge cross products of the screen position (U/W, V/W) have
    one sign — away from the edges, where fp64 rounding cannot matter."""
    box = (600.0, 400.0, 40.0)
    T = lr.transform("bird", box)
    tri = Lasso.from_pixels(T, lr.W, lr.H, [(96, 100), (165, 112), (118, 155)])          # (the named "tri" covers this box's whole picture)
    rs = np.random.RandomState(5)
    pts = _pts(rs.random_sample((20000, 3)) * np.asarray(box))
    U, V, Wc = tri.project(*(pts[a].astype(np.float64) for a in "xyz"))
    assert (Wc > 0).all()
    su, sv = U / Wc, V / Wc
    P = tri.vertices.astype(np.float64)
    cross = np.stack([(P[(i + 1) % 3, 0] - P[i, 0]) * (sv - P[i, 1]) - (P[(i + 1) % 3, 1] - P[i, 1]) * (su - P[i, 0]) for i in range(3)])
    length = np.array([np.hypot(*(P[(i + 1) % 3] - P[i])) for i in range(3)])[:, None]
    clear = (np.abs(cross) > 1e-6 * length).all(axis=0)                                     # more than a millionth of a pixel from every edge's line
    inside = (cross > 0).all(axis=0) | (cross < 0).all(axis=0)
    assert clear.sum() > 19000 and 1000 < inside[clear].sum() < clear.sum() - 1000
    assert np.array_equal(tri.contains(pts)[clear], inside[clear])
    # and from_pixels is the pixel convention of Rays.from_pixels: pixel i covers ndc [2i/W - 1, 2(i+1)/W - 1]
    m = np.asarray(T, np.float64).reshape(4, 4)
    h = np.stack([pts[a].astype(np.float64) for a in "xyz"] + [np.ones(len(pts))], axis=1) @ m.T
    assert np.allclose(su, 0.5 * lr.W * (h[:, 0] / h[:, 3] + 1.0), rtol=0, atol=1e-3) and np.allclose(sv, 0.5 * lr.H * (h[:, 1] / h[:, 3] + 1.0), rtol=0, atol=1e-3)
    ndc = Lasso.from_ndc(T, P / np.array([0.5 * lr.W, 0.5 * lr.H]) - 1.0)
    assert np.array_equal(ndc.contains(pts)[clear], inside[clear])


def test_classify_lasso_on_a_hand_made_table():
    """The eye at (0.5, 0.5, -1) of a unit box looking along +z: W = z + 1 - 1.25 puts the eye plane at z = 0.25."""
    rows = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, -0.25))
    # on the screen (x / (z - 0.25), y / (z - 0.25)); the square 0.1 .. 0.9 at z = 1.25 is the polygon 0.1 .. 0.9
    sq = Lasso([(0.1, 0.1), (0.1, 1.2), (1.2, 1.2), (1.2, 0.1)], *rows)
    t = np.zeros(5, dtype=abi.export_node_dtype)
    t["level"] = [3, 2, 3, 3, 2]
    t["X"], t["Y"], t["Z"] = [3, 1, 2, 7, 0], [3, 1, 2, 7, 0], [0, 0, 5, 5, 3]
    # z 0 .. 0.125: behind the eye plane; z 0 .. 0.25 (+ a cell): straddles it; level 3 at (0.25 .. 0.375, z 0.625 .. 0.75): screen 0.5 .. 1 inside;
    # level 3 at (0.875 .. 1, z 0.625 .. 0.75): screen 1.75 .. 2.7 outside; level 2 at (0 .. 0.25, z 0.75 .. 1): screen 0 .. 0.5, cut by the edge u = 0.1
    outside, copied = classify_lasso(sq, t, (0, 0, 0), (1, 1, 1))
    assert outside.tolist() == [True, False, False, True, False] and copied.tolist() == [False, False, True, False, False]
    # every sample of the copied node passes, none of the outside ones
    rs = np.random.RandomState(2)
    for i, want in ((0, False), (2, True), (3, False)):
        s = 2.0 ** -int(t["level"][i])
        lo = np.array([t["X"][i], t["Y"][i], t["Z"][i]]) * s
        assert (sq.contains(_pts(lo + rs.random_sample((500, 3)) * s)) == want).all(), i


def test_lasso_does_not_combine_with_a_footprint_or_a_profile():
    ex, pts, box, ho = rr.host_octree("ragged_tiny")
    l, f = lr.lasso("tri", lr.transform("bird", box)), fr.footprint("rect", box)
    p = Profile.from_xy([(0.1, 0.1), (0.9, 0.9)], 0.1)
    for call in (lambda: ex.crop(Region(), lasso=l, footprint=f), lambda: ex.crop(Region(), lasso=l, profile=p),
                 lambda: ex.paint(Region(), Paint.set(1), footprint=f, lasso=l), lambda: ex.summarize(Region(), footprint=f, lasso=l)):
        with pytest.raises(ValueError):
            call()


@pytest.fixture(scope="module", params=cases.CASES)
def built(request):
    name = request.param
    ex, pts, box, ho = rr.host_octree(name)
    return name, ex, pts, box, (0.0, 0.0, 0.0)


def _check(name, ex, pts, box, off, cam, kind, exact=False):
    """crop(lasso=) in the three MODES against the brute-force filter of the contract's input points, and what the cameras promise."""
    l = lr.lasso(kind, lr.transform(cam, box, off))
    inb = lr.inbox(pts, ex.box_min, ex.box_max)
    want = pts[l.contains(pts) & inb]
    if exact:
        verdict, decided = lr.contains_exact(l, pts[inb], return_decided=True)
        assert np.array_equal(verdict, l.contains(pts[inb])), f"{name} {cam} {kind}: rule L1 in fp64 differs from the exact rule at {int((verdict != l.contains(pts[inb])).sum())} samples"
    outside, copied = classify_lasso(l, ex.nodes, ex.box_min, ex.box_max)
    for sel, ml in MODES:
        crop, c = ex.crop(Region(), ml, sel, return_counts=True, lasso=l)               # (asserts rule L5 per node)
        crop.validate()
        if (sel, ml) == ("cut", 20):                     # the leaves' samples: the input points
            got = crop.samples
            rr.assert_same_multiset(got[lr.inbox(got, ex.box_min, ex.box_max)], want, f"{name} {cam} {kind}")
        if cam == "away":
            assert outside.all() and crop.num_nodes == 1 and crop.num_samples == 0 and int(c["numCopiedNodes"]) == int(c["numFilteredNodes"]) == 0
        assert int(c["numSamples"]) == crop.num_samples and int(c["numNodes"]) == crop.num_nodes
    if cam == "inside":
        # the eye is in the box: the root's corners lie on both sides of the eye plane
        mn, size = np.asarray(ex.box_min, np.float64), float(np.max(np.asarray(ex.box_max, np.float32) - np.asarray(ex.box_min, np.float32)))
        w = [l.project(*(mn + size * np.array([(k >> a) & 1 for a in range(3)])))[2] for k in range(8)]
        assert min(w) < 0 < max(w) and not outside[0] and not copied[0]
    if kind == "cover" and cam == "bird":
        assert not outside.any() and copied.all()
    return l


@pytest.mark.parametrize("cam", lr.CAMERAS)
def test_crop_with_a_lasso_is_the_brute_force_filter(built, cam):
    name, ex, pts, box, off = built
    for kind in lr.names_for(name):
        _check(name, ex, pts, box, off, cam, kind)


@pytest.mark.parametrize("name,offset", lr.SHIFTED)
def test_lassos_in_a_box_off_the_origin(name, offset):
    """The shifted pairs: the brute-force filter in fp64 AND rule L1 decided exactly (lasso_ref.contains_exact) on the contract's points."""
    pts0, box, batch, T = cases.case(name)
    off = cases.offset_of(offset, box)
    ex, pts, box, ho = rr.host_octree(name, box_min=off)
    for cam in lr.CAMERAS:
        for kind in lr.SHIFTED_KINDS + (["star128"] if name in fr.SHIFTED_STAR128 and cam == "bird" else []):
            _check(f"{name}+{offset}", ex, pts, box, off, cam, kind, exact=cam != "away")


def test_the_exact_path_is_not_dead():
    """contains_exact takes its Fraction path for points on an edge's plane through the eye, and decides them as the strict rule does."""
    rows = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0))
    sq = Lasso([(1, 1), (1, 3), (3, 3), (3, 1)], *rows)
    pts = _pts([(1, 2, 1), (3, 2, 1), (2, 1, 1), (2, 3, 1), (2, 2, 1), (6, 4, 2), (2, 4, 2), (0, 0, 1)])
    verdict, decided = lr.contains_exact(sq, pts, return_decided=True)
    assert decided[:4].all() and decided[5] and decided[6] and not decided[4]
    assert np.array_equal(verdict, sq.contains(pts))
    assert verdict.tolist() == [True, True, True, False, True, True, True, False]


def test_from_footprint_selects_what_the_footprint_selects(built):
    """Lasso.from_footprint(f).contains equals f.contains bit for bit, and crop(lasso=) returns crop(footprint=)'s samples in its order; the node
    classes may differ (eight corners against a rectangle), but no copied node of one is outside for the other."""
    name, ex, pts, box, off = built
    for kind in fr.names_for(name):
        f = fr.footprint(kind, box)
        l = Lasso.from_footprint(f)
        assert np.array_equal(l.contains(pts), f.contains(pts)), kind
        for sel, ml in MODES:
            a = ex.crop(Region(), ml, sel, footprint=f)
            b = ex.crop(Region(), ml, sel, lasso=l)
            assert a.samples.tobytes() == b.samples.tobytes(), (kind, sel, ml)
        lo, lc = classify_lasso(l, ex.nodes, ex.box_min, ex.box_max)
        from simlod_amd.octree_io import classify_footprint
        near, corner = classify_footprint(f, ex.nodes, ex.box_min, ex.box_max)
        fo, fc = ~near & ~corner, ~near & corner
        assert not (lc & fo).any() and not (fc & lo).any(), kind


def test_lasso_composes_with_planes_paint_and_summary(built):
    name, ex, pts, box, off = built
    T = lr.transform("bird", box)
    l = lr.lasso("star7", T)
    r = rr.region("slab", box)
    crop, c, index = ex.crop(r, 20, "all", return_counts=True, lasso=l, return_index=True)
    inb = lr.inbox(pts, ex.box_min, ex.box_max)
    leaves = ex.crop(r, 20, "cut", lasso=l).samples                                         # the leaves' samples: the input points
    rr.assert_same_multiset(leaves[lr.inbox(leaves, ex.box_min, ex.box_max)], pts[l.contains(pts) & rr.brute_mask(r, pts) & inb], name)
    # inside the camera's own frustum nothing changes for a lasso on its screen
    a = ex.crop(Region.from_frustum(T), 20, "cut", lasso=lr.lasso("rect", T))
    b = ex.crop(Region(), 20, "cut", lasso=lr.lasso("rect", T))
    rr.assert_same_multiset(a.samples, b.samples, name)
    # paint: exactly crop's samples change, and the ARRAY paint of `previous` restores the export
    painted, pc, previous = ex.paint(r, Paint.set(0x11223344), lasso=l, return_previous=True)
    assert pc.tobytes() == c.tobytes() and np.array_equal(previous, ex.samples["color"][index])
    changed = np.zeros(ex.num_samples, bool)
    changed[index] = True
    assert (painted.samples["color"][changed] == 0x11223344).all() and np.array_equal(painted.samples["color"][~changed], ex.samples["color"][~changed])
    back, _ = painted.paint(r, Paint.array(), lasso=l, colors=previous)
    assert back.samples.tobytes() == ex.samples.tobytes()
    # summary: the summary of crop's samples, and histC of the painted export verifies the paint
    cut, cc = ex.crop(r, 3, "cut", return_counts=True, lasso=l)
    s, sc = ex.summarize(r, 3, "cut", lasso=l, return_counts=True)
    assert s.num_samples == cut.num_samples and sc.tobytes() == cc.tobytes()
    sp = painted.summarize(r, 20, "all", lasso=l)
    assert int(sp["histC"][0][0x44]) == int(sp["histC"][1][0x33]) == int(sp["histC"][2][0x22]) == int(sp["histC"][3][0x11]) == len(index)


def test_every_class_occurs():
    """Not vacuous: over the cases, cameras and lassos each of OUTSIDE, COPIED and FILTERED occurs on nodes that hold samples, `inside` gives
    nodes whose corners lie on both sides of the eye plane, and tri and bowtie under the bird camera copy nodes of the terrain."""
    seen = {0: 0, 1: 0, 2: 0}
    copied_by = set()
    for name in ("uniform_3x40k", "terrain_4x100k", "hotspot_150k"):
        ex, pts, box, ho = rr.host_octree(name)
        holds = ex.nodes["numSamples"] != 0
        for cam in lr.CAMERAS:
            for kind in ("star7", "rect", "tri", "bowtie"):
                l = lr.lasso(kind, lr.transform(cam, box))
                outside, copied = classify_lasso(l, ex.nodes, ex.box_min, ex.box_max)
                cls = np.where(outside, 0, np.where(copied, 2, 1))[holds]
                for k in seen:
                    seen[k] += int((cls == k).sum())
                if (cls == 2).any():
                    copied_by.add((name, cam, kind))
    assert all(v > 0 for v in seen.values()), seen
    assert ("terrain_4x100k", "bird", "tri") in copied_by and ("terrain_4x100k", "bird", "bowtie") in copied_by, copied_by
