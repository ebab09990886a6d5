"""CPU tier: footprint queries (include/simlod_hip.h, "footprint queries") — the ABI struct, octree_io.Footprint, classify_footprint and the
host mirror OctreeExport.crop(footprint=) against a brute-force filter of the input points, on octrees built by the oracle's port, at the
origin and in the shifted boxes of tests/test_gpu_box_origin.py; there the filter is footprint_ref.contains_exact as well, rule F1 with every
edge's side decided exactly."""
import os
import re

import numpy as np
import pytest

import cases
import footprint_ref as fr
import region_ref as rr
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import Footprint, Region, classify_footprint, classify_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("cut", 20), ("all", 20), ("cut", 2)]


def test_footprint_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodFootprint\) == (\d+)", src).group(1)) == abi.footprint_dtype.itemsize == 2096
    offs = dict(re.findall(r"offsetof\(SimlodFootprint, (\w+)\) == (\d+)", src))
    assert sorted(offs) == ["axisU", "axisV", "vertices"]
    for f, o in offs.items():
        assert abi.footprint_dtype.fields[f][1] == int(o), f
    assert abi.footprint_dtype.fields["numVertices"][1] == 0 and abi.footprint_dtype.fields["reserved"][1] == 4
    assert int(re.search(r"#define SIMLOD_FOOTPRINT_MAX_VERTICES (\d+)u", src).group(1)) == abi.FOOTPRINT_MAX_VERTICES == 256
    r = Footprint([(1, 2), (3, 4), (5, 7)], (1, 2, 3, 4), (5, 6, 7, 8)).record()
    assert r.dtype == abi.footprint_dtype and int(r["numVertices"][0]) == 3 and not r["reserved"].any()
    assert r["vertices"][0, :3].tolist() == [[1, 2], [3, 4], [5, 7]] and not r["vertices"][0, 3:].any()
    assert r["axisU"][0].tolist() == [1, 2, 3, 4] and r["axisV"][0].tolist() == [5, 6, 7, 8]


def test_footprint_symbols_exported(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_footprint_buffer_min_bytes", "simlod_query_footprint"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    # the query's bytes plus a fixed block for the widened polygon
    block = L.simlod_footprint_buffer_min_bytes(100, 0) - L.simlod_query_buffer_min_bytes(100, 0)
    assert block >= 256 * 32
    assert L.simlod_footprint_buffer_min_bytes(7000, 5_000_000) - L.simlod_query_buffer_min_bytes(7000, 5_000_000) == block


def test_footprint_constructors():
    tri = [(0, 0), (1, 0), (0, 1)]
    f = Footprint(tri)
    assert f.vertices.dtype == f.axis_u.dtype == f.axis_v.dtype == np.float32
    assert f.axis_u.tolist() == [1, 0, 0, 0] and f.axis_v.tolist() == [0, 1, 0, 0]
    assert Footprint.from_xy(tri).vertices.tolist() == f.vertices.tolist()
    assert len(Footprint(np.zeros((256, 2)))) == 256
    for bad in (tri[:2], np.zeros((257, 2)), [(0, 0), (1, np.nan), (0, 1)], [(0, 0), (1e39, 0), (0, 1)], [(0, 0), (np.inf, 0), (0, 1)]):
        with pytest.raises(ValueError):
            Footprint(bad)
    with pytest.raises(ValueError):
        Footprint(tri, axis_u=(1, 0, np.nan, 0))
    with pytest.raises(ValueError):
        Footprint(tri, axis_v=(0, 1e39, 0, 0))           # infinite as float32
    r = Footprint.from_rect((1, 2), (3, 4))
    assert sorted(map(tuple, r.vertices.tolist())) == [(1, 2), (1, 4), (3, 2), (3, 4)]


def _pts(xyz):
    p = np.zeros(len(xyz), dtype=abi.point_dtype)
    a = np.asarray(xyz, dtype=np.float32)
    p["x"], p["y"], p["z"] = a[:, 0], a[:, 1], a[:, 2]
    return p


def test_contains_is_the_even_odd_rule():
    # a concave L, a bowtie that crosses itself, a polygon without area, a convex triangle against its edges' cross products
    L = Footprint.from_xy([(0, 0), (4, 0), (4, 1), (1, 1), (1, 4), (0, 4)])
    got = L.contains(_pts([(0.5, 0.5, 9), (3, 0.5, -9), (0.5, 3, 0), (3, 3, 0), (2, 2, 0), (-1, 0.5, 0), (5, 0.5, 0), (np.nan, 0.5, 0), (0.5, 0.5, np.nan)]))
    assert got.tolist() == [True, True, True, False, False, False, False, False, False]
    bow = Footprint.from_xy([(0, 0), (4, 4), (0, 4), (4, 0)])
    assert bow.contains(_pts([(2, 3, 0), (2, 1, 0), (1, 2, 0), (3, 2, 0)])).tolist() == [True, True, False, False]
    # zero area: nothing off the polygon's own line passes
    flat = Footprint.from_xy([(0, 0), (2, 2), (4, 4), (1, 1)])
    rs = np.random.RandomState(0)
    p = rs.rand(1000, 3) * 4
    assert (p[:, 0] != p[:, 1]).all() and not flat.contains(_pts(p)).any()
    # against the winding of a convex polygon: the sign of every edge's cross product, away from the edges
    tri = Footprint.from_xy([(0.5, 0.25), (3.5, 1.0), (1.0, 3.75)])
    p = rs.rand(20000, 3) * 4
    a = tri.vertices.astype(np.float64)
    b = np.roll(a, -1, axis=0)
    cr = (b[:, 0] - a[:, 0])[None] * (p[:, 1, None] - a[:, 1][None]) - (b[:, 1] - a[:, 1])[None] * (p[:, 0, None] - a[:, 0][None])
    far = (np.abs(cr) > 1e-3).all(axis=1)
    assert np.array_equal(tri.contains(_pts(p))[far], (cr > 0).all(axis=1)[far]) and 2000 < (cr > 0).all(axis=1).sum() < 8000
    # an oblique map: the same triangle seen through u = 2x + 1, v = z
    ob = Footprint(tri.vertices, (2, 0, 0, 1), (0, 0, 1, 0))
    q = p.copy()
    q[:, 0], q[:, 2] = (p[:, 0] - 1) / 2, p[:, 1]
    assert np.array_equal(ob.contains(_pts(q))[far], (cr > 0).all(axis=1)[far])


def test_classify_footprint_on_a_hand_made_table():
    # box [0, 8)^3; level-1 nodes are cubes of 4; the footprint x, y in [0.5, 3.5] lies in the nodes (0, 0, *).  Node (1, 0, 0) beside it is
    # NEAR all the same (rule F3 looks at an edge's v range and at its LINE: the horizontal edges' lines cut that node); node (0, 1, 0) above
    # it misses every edge's v range; the level-3 node (2, 2, 5) lies inside
    t = np.zeros(5, dtype=abi.export_node_dtype)
    t["level"] = [0, 1, 1, 1, 3]
    t["X"], t["Y"], t["Z"] = [0, 0, 1, 0, 2], [0, 0, 0, 1, 2], [0, 1, 0, 0, 5]
    near, corner = classify_footprint(Footprint.from_rect((0.5, 0.5), (3.5, 3.5)), t, (0, 0, 0), (8, 8, 8))
    assert near.tolist() == [True, True, True, False, False] and corner[3:].tolist() == [False, True]
    # a footprint around everything: no near edge anywhere, every corner inside
    near, corner = classify_footprint(Footprint.from_rect((-1, -1), (9, 9)), t, (0, 0, 0), (8, 8, 8))
    assert not near.any() and corner.all()
    # mixed signs in the axes: u = -x + 8 maps [0.5, 3.5) to (4.5, 7.5]
    near, corner = classify_footprint(Footprint([(4.5, 0.5), (4.5, 3.5), (7.5, 3.5), (7.5, 0.5)], (-1, 0, 0, 8)), t, (0, 0, 0), (8, 8, 8))
    assert near.tolist() == [True, True, True, False, False] and corner[3:].tolist() == [False, True]


@pytest.fixture(scope="module", params=cases.CASES)
def built(request):
    """-> (name, full export, points, box)"""
    name = request.param
    ex, pts, box, ho = rr.host_octree(name)
    return name, ex, pts, box


def test_crop_with_a_footprint_is_the_brute_force_filter(built):
    name, ex, pts, box = built
    for kind in fr.names_for(name):
        f = fr.footprint(kind, box)
        inside = f.contains(pts)
        if kind == "miss":
            assert not inside.any()
        elif kind == "cover":
            assert inside.all()
        else:
            assert 0 < inside.sum() and (inside.sum() < len(pts) or "hotspot" in name), (name, kind)
        for sel, ml in MODES:
            c, cnt = ex.crop(Region(), ml, sel, return_counts=True, footprint=f)
            c.validate()
            assert c.select == abi.EXPORT_REGION and c.max_level == ml
            assert int(cnt["numNodes"]) == c.num_nodes and int(cnt["numSamples"]) == c.num_samples <= int(cnt["numCandidates"])
            if (sel, ml) == ("cut", 20):
                rr.assert_same_multiset(c.samples, pts[inside], f"{name} {kind}")
            if kind == "cover":
                t = ex.truncated(ml, sel)
                assert c.nodes.tobytes() == t.nodes.tobytes() and c.samples.tobytes() == t.samples.tobytes(), (name, sel, ml)
                assert int(cnt["numFilteredNodes"]) == 0 and int(cnt["numCopiedNodes"]) == int((t.nodes["numSamples"] != 0).sum())
            if kind == "miss":
                assert [int(cnt[k]) for k in cnt.dtype.names] == [1, 0, 0, 0, 0, 0]
    # without a footprint nothing changed
    for kind in rr.REGION_NAMES:
        r = rr.region(kind, box)
        a, ca = ex.crop(r, 20, "cut", return_counts=True)
        b, cb = ex.crop(r, 20, "cut", return_counts=True, footprint=None)
        assert a.nodes.tobytes() == b.nodes.tobytes() and a.samples.tobytes() == b.samples.tobytes() and ca.tobytes() == cb.tobytes()


def test_crop_per_node_order_and_classes(built):
    """Per listed node: the source node's samples under the test, in order; the classes are classify_footprint's."""
    name, ex, pts, box = built
    f = fr.footprint("star7", box)
    c = ex.crop(Region(), 20, "all", footprint=f)
    near, corner = classify_footprint(f, ex.nodes, ex.box_min, ex.box_max)
    src = {(int(e["level"]), int(e["X"]), int(e["Y"]), int(e["Z"])): i for i, e in enumerate(ex.nodes)}
    listed = np.zeros(ex.num_nodes, bool)
    for e in c.nodes:
        i = src[(int(e["level"]), int(e["X"]), int(e["Y"]), int(e["Z"]))]
        listed[i] = True
        s = ex.nodes[i]
        seg = ex.samples[int(s["firstSample"]): int(s["firstSample"]) + int(s["numSamples"])]
        got = c.samples[int(e["firstSample"]): int(e["firstSample"]) + int(e["numSamples"])]
        want = seg[f.contains(seg)] if near[i] else seg if corner[i] else seg[:0]
        assert got.tobytes() == want.tobytes(), (name, e)
    # a node below the root is listed iff its parent is and it is not outside
    outside = ~near & ~corner
    par = ex.nodes["parent"].astype(np.int64)
    want = np.ones(ex.num_nodes, bool)
    for i in range(1, ex.num_nodes):
        want[i] = want[par[i]] and not outside[i]
    assert np.array_equal(listed, want)


def test_footprint_composes_with_planes(built):
    name, ex, pts, box = built
    f, r = fr.footprint("star7", box), rr.region("slab", box)
    c, cnt = ex.crop(r, 20, "cut", return_counts=True, footprint=f)
    c.validate()
    both = f.contains(pts) & rr.brute_mask(r, pts)
    assert 0 < both.sum() < min(f.contains(pts).sum(), rr.brute_mask(r, pts).sum()) or "hotspot" in name
    rr.assert_same_multiset(c.samples, pts[both], f"{name} star7 and slab")
    # the final class: outside by either, copied iff copied by both
    po, pi = classify_nodes(r.planes.astype(np.float64), c.nodes, ex.box_min, ex.box_max)
    near, corner = classify_footprint(f, c.nodes, ex.box_min, ex.box_max)
    assert not (po | (~near & ~corner))[1:].any()                       # nothing outside is listed below the root
    full = ex.crop(Region(), 20, "cut").nodes
    key = lambda a: list(zip(a["level"].tolist(), a["X"].tolist(), a["Y"].tolist(), a["Z"].tolist()))
    before = dict(zip(key(full), full["numSamples"].tolist()))
    copied = pi & ~near & corner
    kept = np.array([before[k] for k in key(c.nodes)])
    assert np.array_equal(c.nodes["numSamples"][copied], kept[copied])
    assert int(cnt["numCopiedNodes"]) == int((copied & (c.nodes["numSamples"] != 0)).sum())


def test_rect_footprint_against_the_box_region(built):
    name, ex, pts, box = built
    lo, hi = fr.rect_of(box)
    f, r = fr.footprint("rect", box), rr.region("box", box)
    # rule F1 drops points on the polygon's max edges in v, the planes keep them: no input point lies there
    assert not (pts["x"] == np.float32(hi[0])).any() and not (pts["y"] == np.float32(hi[1])).any()
    a = ex.crop(Region(), 20, "cut", footprint=f)
    b = ex.crop(r, 20, "cut")
    assert a.num_samples > 0 or "hotspot" in name
    rr.assert_same_multiset(a.samples, b.samples, f"{name} rect")
    rr.assert_same_multiset(a.samples, pts[rr.brute_mask(r, pts)], f"{name} rect, brute force")


# ---- a box off the origin: the inputs of tests/test_gpu_box_origin.py ----------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", fr.SHIFTED)
def test_footprints_in_a_box_off_the_origin(name, offset):
    """The oracle's octree of a shifted case: the crop is the brute-force filter by Footprint.contains and by contains_exact alike (they agree on
    every point), every footprint filters a node at the deepest level, and star7 composes with the slab."""
    off = cases.offset_of(offset, cases.case(name)[1])
    ex, pts, box, ho = rr.host_octree(name, box_min=off)
    box_min = ex.box_min
    assert box_min == tuple(float(np.float32(v)) for v in off)
    deepest = int(ex.nodes["level"].max())
    has = ex.truncated(20, "cut").nodes["numSamples"] > 0
    copied = {}
    for kind in fr.SHIFTED_KINDS:
        f = fr.footprint(kind, box, box_min)
        inside = f.contains(pts)
        exact, decided = fr.contains_exact(f, pts, return_decided=True)
        assert np.array_equal(inside, exact), f"{name}@{offset} {kind}: rule F1 in fp64 and the exact rule disagree on {int((inside != exact).sum())} points"
        c, cnt = ex.crop(Region(), 20, "cut", return_counts=True, footprint=f)
        c.validate()
        rr.assert_same_multiset(c.samples, pts[exact], f"{name}@{offset} {kind}")
        near, corner = classify_footprint(f, ex.nodes, ex.box_min, ex.box_max)
        print(name, offset, kind, {k: int(cnt[k]) for k in cnt.dtype.names}, f"{int(inside.sum())} inside, {int(decided.sum())} decided in Fractions")
        if kind == "miss":
            assert not inside.any() and [int(cnt[k]) for k in cnt.dtype.names] == [1, 0, 0, 0, 0, 0]
        else:
            assert 0 < inside.sum() < len(pts), (name, kind)
            assert (has & near & (ex.nodes["level"] == deepest)).any(), f"{name}@{offset} {kind}: no filtered node at level {deepest}"
            assert int(cnt["numFilteredNodes"]) >= 1 and int(cnt["numCopiedNodes"]) == int((has & ~near & corner).sum()), (name, kind)
            copied[kind] = int(cnt["numCopiedNodes"])
    # these octrees are two to four levels deep: only the hotspot's leaves are small enough to lie inside a footprint (the rectangle) whole.
    # tests/test_deep_io.py has footprints that copy nodes at level 13
    assert copied["rect"] >= 1 or name != "hotspot_150k", copied
    f, r = fr.footprint("star7", box, box_min), rr.region("slab", box, box_min)
    both = fr.contains_exact(f, pts) & rr.brute_mask(r, pts)
    assert 0 < both.sum() < min(f.contains(pts).sum(), rr.brute_mask(r, pts).sum()) or "hotspot" in name
    rr.assert_same_multiset(ex.crop(r, 20, "cut", footprint=f).samples, pts[both], f"{name}@{offset} star7 and slab")


def test_the_exact_path_is_not_dead():
    """At the georef offset one fp32 step is 1/32 m in x and 0.25 m in y: input points lie ON edges of the rectangle and the bowtie, where c is 0
    or too close for fp64, and Fractions decide them — the same way as the fp64 formula."""
    pts, box_min, box, _ = cases.shifted("terrain_4x100k", cases.GEOREF)
    for kind, n in (("rect", 31), ("bowtie", 28)):
        f = fr.footprint(kind, box, box_min)
        exact, decided = fr.contains_exact(f, pts, return_decided=True)
        assert np.array_equal(exact, f.contains(pts)), kind
        assert int(decided.sum()) == n, (kind, int(decided.sum()))
    # a point on a rectangle's edges by from_rect's convention: lo_x <= x <= hi_x, lo_y <= y < hi_y
    r = Footprint.from_rect((1, 2), (3, 4))
    on = _pts([(1, 3, 0), (3, 3, 0), (2, 2, 0), (2, 4, 0), (1, 2, 0), (3, 4, 0), (2, 3, 0), (0.5, 3, 0)])
    exact, decided = fr.contains_exact(r, on, return_decided=True)
    assert exact.tolist() == [True, True, True, False, True, False, True, False] and np.array_equal(exact, r.contains(on))
    assert decided.tolist() == [True, True, False, False, True, False, False, False]


@pytest.fixture(scope="module")
def terrain3m():
    t = fr.TERRAIN_3M
    pts, box = synthetic.terrain(t["n"], seed=t["seed"], box=t["box"], tile=t["tile"])
    ex, _, _, _ = rr.host_octree(pts=pts, box=box, batch=1_000_000)
    return ex, pts, box


@pytest.mark.parametrize("kind", ["star", "triangle"])
def test_terrain_footprints_are_not_vacuous(terrain3m, kind):
    ex, pts, box = terrain3m
    f = fr.terrain3m_footprints()[kind]
    c, cnt = ex.crop(Region(), 20, "cut", return_counts=True, footprint=f)
    c.validate()
    print(kind, {k: int(cnt[k]) for k in cnt.dtype.names}, "of", ex.num_nodes, "nodes")
    assert int(cnt["numCopiedNodes"]) > 0 and int(cnt["numFilteredNodes"]) > 0 and int(cnt["numNodes"]) < ex.num_nodes
    assert 0 < int(cnt["numSamples"]) < int(cnt["numCandidates"])
    inside = f.contains(pts)
    assert int(inside.sum()) == {"star": 516_959, "triangle": 1_003_291}[kind]
    rr.assert_same_multiset(c.samples, pts[inside], f"3 M terrain, {kind}")
