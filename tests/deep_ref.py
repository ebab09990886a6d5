"""Shared by tests/test_deep_io.py and tests/test_gpu_deep_octrees.py: octrees 13 and 20 levels deep, built by the port oracle, the query
sets, regions and footprints aimed at their deepest nodes, and the guards that keep a comparison on them from passing on nothing.

  D13   test_gpu_deep_paths.deep_case(11): four batches A to D, 562 000 points in the level-11 cell at the origin of a unit box; 161 nodes
        (the root, twelve times eight, 64 leaves at level 13);
  D13x  the same case in a box of 2^13, in the level-11 cell CELL_X far from the origin: a level-13 node is 1 wide, so a camera behind the
        0.1 near plane sees level-13 nodes larger than minNodeSize;
  D20   30 000 uniform points, 70 000 identical ones at fp32 (0.3, 0.6, 0.2), 30 000 uniform points, in batches of 50 000: a chain of twenty
        splits (eight nodes at every level 1 .. 20).  The device stores the identical points in the level-20 leaf; the reference counts them
        and stores none (voxels.cu:394-412, 599-604), so `completed_export` puts them into the oracle's export by hand.  D20R adds a fourth
        batch (5 000 more identical points, 5 000 uniform ones) for the resume."""
import numpy as np

import cases
import footprint_ref as fr
from export_ref import export_host
from region_ref import host_octree
from simlod_amd import abi, camera, synthetic
from simlod_amd.octree_io import Footprint, OctreeExport, Rays, Region, Spheres, classify_footprint, classify_nodes
from test_gpu_deep_paths import SIZES, assert_input_arithmetic, deep_case

CELL_LEVEL = 11
LEAF_LEVEL = CELL_LEVEL + 2
SCALE_X = 2.0 ** 13
CELL_X = (1434, 1229, 1536)                       # of level 11: coordinates at 0.70, 0.60, 0.75 of the box
POINT = tuple(float(np.float32(v)) for v in (0.3, 0.6, 0.2))
D20_BATCH = 50_000
NONE = abi.EXPORT_NONE
_BUILT = {}


class Deep:
    """One input and the oracle's octree of it."""

    def __init__(self, name, box, batches, origin=(0.0, 0.0, 0.0)):
        self.name, self.box, self.batches = name, box, batches
        self.size = float(max(box))
        self.origin = np.asarray(origin, dtype=np.float64)          # the low corner of the cell the points are in
        self.export, self.pts, _, self.ho = host_octree(batches=batches, box=box, export=name.startswith("d13"))
        self.u = cases.uniforms_for(box, np.eye(4, dtype=np.float32))
        self.nn = int(self.ho.stats["numNodes"][0])


def d13_input(which):
    """-> (box, batches, counts, low corner of the level-11 cell)"""
    if which == "d13":
        box, batches, counts = deep_case(CELL_LEVEL)
        return box, batches, counts, np.zeros(3)
    box, batches, counts = deep_case(CELL_LEVEL, scale=SCALE_X, cell=CELL_X)
    return box, batches, counts, np.asarray(CELL_X, dtype=np.float64) * (SCALE_X * 2.0 ** -CELL_LEVEL)


def d20_input():
    """-> (box, the three batches, the fourth batch, the identical points of all four batches)"""
    base, box = synthetic.uniform_cube(60_000, seed=9)
    same = np.repeat(base[:1], 75_000)
    same["x"], same["y"], same["z"] = (np.float32(v) for v in POINT)
    pts = np.concatenate([base[:30_000], same[:70_000], base[30_000:]])
    more, _ = synthetic.uniform_cube(5_000, seed=10)
    return box, [pts[i:i + D20_BATCH] for i in range(0, len(pts), D20_BATCH)], np.concatenate([same[70_000:], more]), same


def built(name):
    """'d13', 'd13x', 'd20' (three batches), 'd20r' (four) -> Deep, once per session."""
    if name not in _BUILT:
        if name in ("d13", "d13x"):
            box, batches, counts, origin = d13_input(name)
            d = Deep(name, box, batches, origin)
            d.counts = counts
        else:
            box, batches, fourth, same = d20_input()
            d = Deep(name, box, batches + [fourth] if name == "d20r" else batches)
            d.same = same
            d.k = leaf_count(d.ho)
            d.export = completed_export(d.ho, same[:d.k])
        _BUILT[name] = d
    return _BUILT[name]


def level_histogram(table):
    lv = np.asarray(table["level"]).astype(np.int64)
    return {int(l): int((lv == l).sum()) for l in np.unique(lv)}


def deep_leaf(ho):
    """The index of the one non-empty level-20 node of an oracle image."""
    nn = int(ho.stats["numNodes"][0])
    at = np.nonzero((ho.nodes["level"][:nn] == abi.MAX_DEPTH) & (ho.nodes["numPoints"][:nn] > 0))[0]
    assert len(at) == 1, f"{len(at)} non-empty nodes at level {abi.MAX_DEPTH}"
    return int(at[0])


def leaf_count(ho):
    """k: the points the ORACLE counts in its level-20 leaf (it stores none of them)."""
    return int(ho.nodes["numPoints"][deep_leaf(ho)])


def completed_export(ho, leaf_points, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0)):
    """The oracle's collision image as a full export: export_host cannot walk the level-20 leaf (a count without chunks), so the leaf is exported
    empty and `leaf_points` (k identical records, k the oracle's count) are put in at its entry."""
    i = deep_leaf(ho)
    nn = int(ho.stats["numNodes"][0])
    k = int(ho.nodes["numPoints"][i])
    leaf_points = np.ascontiguousarray(leaf_points).view(abi.point_dtype)
    assert len(leaf_points) == k and len(np.unique(leaf_points.view(np.dtype((np.void, 16))))) == 1, "k copies of one record"
    ho.nodes["numPoints"][i] = 0
    try:
        t, s = export_host(ho.nodes, nn)
    finally:
        ho.nodes["numPoints"][i] = k
    nd = ho.nodes[i]
    e = np.nonzero((t["level"] == abi.MAX_DEPTH) & (t["X"] == nd["X"]) & (t["Y"] == nd["Y"]) & (t["Z"] == nd["Z"]))[0]
    assert len(e) == 1 and int(t["numSamples"][e[0]]) == 0 and int(t["childMask"][e[0]]) == 0
    e = int(e[0])
    first = int(t["firstSample"][e])
    t["numSamples"][e] = k
    t["firstSample"] = np.concatenate([[0], np.cumsum(t["numSamples"].astype(np.uint64))[:-1]]).astype(np.uint64)
    s = np.concatenate([s[:first], leaf_points, s[first:]])
    return OctreeExport(t, s, box_min, box_max).validate(buildable=True)


def deep_entry(export):
    """The table entry of the one non-empty level-20 node of an export, and its sample count."""
    t = export.nodes
    at = np.nonzero((t["level"] == abi.MAX_DEPTH) & (t["numSamples"] > 0))[0]
    assert len(at) == 1, f"{len(at)} non-empty entries at level {abi.MAX_DEPTH}"
    return int(at[0]), int(t["numSamples"][at[0]])


def assert_d13_shape(export, what):
    assert level_histogram(export.nodes) == {0: 1, **{l: 8 for l in range(1, LEAF_LEVEL)}, LEAF_LEVEL: 64}, what
    t = export.nodes
    leaves = (t["level"] == LEAF_LEVEL) & (t["numSamples"] > 0)
    assert int(leaves.sum()) == 64 and int(t["numSamples"][leaves].sum()) == sum(SIZES), what


def assert_d20_shape(export, k, what):
    assert level_histogram(export.nodes) == {0: 1, **{l: 8 for l in range(1, abi.MAX_DEPTH + 1)}}, what
    e, n = deep_entry(export)
    assert n == k > 0, f"{what}: the level-20 entry holds {n} samples, the oracle counted {k}"
    f = int(export.nodes["firstSample"][e])
    s = export.samples[f: f + n]
    assert (s["x"] == np.float32(POINT[0])).all() and (s["y"] == np.float32(POINT[1])).all() and (s["z"] == np.float32(POINT[2])).all(), what
    return e


# ---- D13 / D13x: rays, spheres, regions, footprints ----------------------------------------------------------------------------------------
def _chosen(pts, n, seed):
    return pts[np.sort(np.random.RandomState(seed).choice(len(pts), n, replace=False))]


def _xyz(p):
    return np.stack([p["x"], p["y"], p["z"]], axis=1).astype(np.float64)


def d13_rays(d, n=64):
    """{name: (Rays, is a cone set)}: thin rays (radius 2^-22 of the box) from outside the box, each aimed at an input point, and cones from
    one eye outside the box at input points, a few point spacings wide where they arrive."""
    size = d.size
    tgt = _xyz(_chosen(d.pts, n, 51))
    rs = np.random.RandomState(52)
    v = rs.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    org = tgt - 2.0 * size * v                                     # 2 box sizes away: outside the box whatever the direction
    assert ((org < 0) | (org > size)).any(1).all()
    thin = Rays(org, tgt - org, 0.0, 2.0, np.ldexp(size, -22), 0.0)
    tgt = _xyz(_chosen(d.pts, n, 53))
    eye = np.array([1.8, -1.2, 1.4]) * size
    dv = tgt - eye
    dist = np.linalg.norm(dv, axis=1)
    cones = Rays(np.broadcast_to(eye, dv.shape), dv / dist[:, None], 0.0, 1.01 * dist, 0.0, 8e-6)
    return {"thin": (thin, False), "cones": (cones, True)}


SPHERE_K = 16


def d13_spheres(d):
    """{name: Spheres} centred at input points: radii 2^-17 (most queries find fewer than 16), 2^-15 (every query finds more) and 2^-12 of the
    box (half the level-11 cell: tens of thousands within, 16 queries only)."""
    return {"r-17": Spheres.from_points(_chosen(d.pts, 64, 54), np.ldexp(d.size, -17)),
            "r-15": Spheres.from_points(_chosen(d.pts, 96, 55), np.ldexp(d.size, -15)),
            "r-12": Spheres.from_points(_chosen(d.pts, 16, 56), np.ldexp(d.size, -12))}


def assert_spheres_not_vacuous(within_by_set, what):
    """Over all sets: within >= 16 for more than half of the queries, below 16 for at least one (the selection drops something, and runs short)."""
    w = np.concatenate([np.asarray(v) for v in within_by_set.values()])
    assert (w >= SPHERE_K).mean() > 0.5 and (w < SPHERE_K).any() and (w > 0).all(), f"{what}: within {np.sort(w)}"


def d13_regions(d):
    """{name: Region} for D13: the box of the level-12 cell (1, 0, 1), widened by two level-20 cells so that its eight level-13 nodes are
    copied whole and their neighbours filtered; a slab through the level-11 cell at an offset no fp32 holds exactly; the frustum of a camera
    half a cell size in front of the cell that sees a part of it."""
    c11 = np.ldexp(d.size, -CELL_LEVEL)
    c12, e = 0.5 * c11, np.ldexp(d.size, -abi.MAX_DEPTH)
    lo = d.origin + np.array([1.0, 0.0, 1.0]) * c12
    n = np.array([0.6, 0.8, 0.1])
    c = float(n @ (d.origin + np.array([0.37, 0.41, 0.53]) * c11))
    h = 0.3 * c11
    eye = d.origin + np.array([0.45, -0.4, 0.55]) * c11
    target = d.origin + np.array([0.6, 0.5, 0.3]) * c11
    T = camera.lookat_transform(tuple(eye), tuple(target), cases.W, cases.H)
    return {"cell12": Region.from_box(lo - 2.0 * e, lo + c12 + 2.0 * e), "slab": Region.from_planes([[*n, -c + h], [*(-n), c + h]]),
            "frustum": Region.from_frustum(T)}


def region_classes(export, region, level, max_level=20, select="cut"):
    """How many entries of level `level` with samples the region query filters sample by sample, and how many entries of any level it copies
    whole — from classify_nodes (rules 1 and 4 of the mirror) on the table the query walks."""
    t = export.truncated(max_level, select).nodes
    outside, inside = classify_nodes(np.asarray(region.planes, np.float32).astype(np.float64), t, export.box_min, export.box_max)
    has = ((t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0) & (t["numSamples"] > 0)
    return int((has & ~outside & ~inside & (t["level"] == level)).sum()), int((has & inside).sum())


def assert_region_not_vacuous(export, region, level, what):
    filtered, copied = region_classes(export, region, level)
    assert filtered >= 1 and copied >= 1, f"{what}: {filtered} filtered nodes at level {level}, {copied} copied nodes"
    return filtered, copied


CLOSE_OFFSET = (3.0, -2.5, 2.5)          # of the eye from the middle of D13x's level-11 cell, in level-13 node sizes


def close_cam(d, width=cases.W, height=cases.H):
    """A camera a few level-13 node sizes from D13x's cell: at the cases' camera the whole cloud is one pixel."""
    mid = d.origin + 0.5 * np.ldexp(d.size, -CELL_LEVEL)
    return camera.lookat_transform(tuple(mid + np.asarray(CLOSE_OFFSET) * np.ldexp(d.size, -LEAF_LEVEL)), tuple(mid), width, height)


def d13_footprints(d):
    """{name: Footprint} for D13 / D13x, in the level-11 cell the points fill: a seven-pointed star around its centre; the xy face of
    d13_regions' cell12 (the level-12 cell (1, 0, .), widened by two level-20 cells); footprint_ref's oblique triangle, a cell size across, at
    the cell's centre."""
    c11 = np.ldexp(d.size, -CELL_LEVEL)
    c12, e = 0.5 * c11, np.ldexp(d.size, -abi.MAX_DEPTH)
    mid = d.origin + 0.5 * c11
    lo = d.origin + np.array([1.0, 0.0, 1.0]) * c12
    uc = float(np.dot(fr.OBLIQUE_U[:3], mid) + fr.OBLIQUE_U[3])
    vc = float(np.dot(fr.OBLIQUE_V[:3], mid) + fr.OBLIQUE_V[3])
    out = {"star7": Footprint.from_xy(fr.star(mid[0], mid[1], 0.45 * c11, 0.15 * c11, 7)),
           "cell12": Footprint.from_rect((lo[0] - 2.0 * e, lo[1] - 2.0 * e), (lo[0] + c12 + 2.0 * e, lo[1] + c12 + 2.0 * e)),
           "oblique": Footprint([(uc - 0.35 * c11, vc - 0.25 * c11), (uc + 0.40 * c11, vc - 0.10 * c11), (uc - 0.05 * c11, vc + 0.35 * c11)], fr.OBLIQUE_U, fr.OBLIQUE_V)}
    for key, f in out.items():
        assert len(np.unique(f.vertices, axis=0)) == len(f), f"{d.name} {key}: two vertices are one fp32 point"
    return out


def footprint_classes(export, footprint, level, max_level=20, select="cut"):
    """region_classes for a footprint, from classify_footprint (rules F2-F4): how many entries of level `level` with samples have a NEAR edge
    and are filtered sample by sample, how many entries of any level are copied whole, and how many entries of that level are outside."""
    t = export.truncated(max_level, select).nodes
    near, corner = classify_footprint(footprint, t, export.box_min, export.box_max)
    has = ((t["flags"] & abi.EXPORT_FLAG_SELECTED) != 0) & (t["numSamples"] > 0)
    at = has & (t["level"] == level)
    return int((at & near).sum()), int((has & ~near & corner).sum()), int((at & ~near & ~corner).sum())


# Which of d13_footprints can copy a node whole.  The projected rectangle of a level-13 node is a quarter of the level-11 cell wide in plan
# view and 0.375 of it in the oblique axes' u; the star's inner radius is 0.15 of the cell and the triangle is 0.75 wide at its base, so
# neither holds a whole leaf, and a leaf is all that carries samples in a cut.  They are told from an empty answer by their outside leaves.
D13_COPIES = {"star7": False, "cell12": True, "oblique": False}


def assert_footprint_not_vacuous(export, footprint, level, what, copies=True):
    """At least one filtered node with samples at `level`, and at least one node copied whole — or, for a footprint too narrow to hold a
    node (copies=False), none copied and at least one node of that level outside."""
    filtered, copied, outside = footprint_classes(export, footprint, level)
    assert filtered >= 1 and (copied >= 1 if copies else copied == 0 and outside >= 1), \
        f"{what}: {filtered} filtered and {outside} outside nodes at level {level}, {copied} copied nodes"
    return filtered, copied


def assert_hits_at_level(hits, table, level, what, share=0.9):
    hit = hits["node"] != NONE
    at = float((table["level"][hits["node"][hit]] == level).mean())
    assert hit.any() and at >= share, f"{what}: only {at:.2f} of the hit nodes are at level {level}"
    return at


# ---- D20: everything through the one point ---------------------------------------------------------------------------------------------------
ULP = float(np.spacing(np.float32(0.6)))          # the largest of the point's three fp32 spacings
D20_DIRS = [(1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.5, -0.25, 1.0), (-0.5, 2.0, 0.5), (0.125, -0.125, -0.125)]


def d20_rays():
    """Per direction a ray of radius 0 and one of radius one fp32 ulp through the point, which sits at t = 0.25 exactly (origin = point -
    dir / 4 is formed in fp64 and must be an fp32: asserted), and last a ray along +x that passes the level-20 cell two cell widths away
    in y.  -> (Rays, index of the missing ray)"""
    p = np.array(POINT, dtype=np.float64)
    org, dirs, rad = [], [], []
    for dv in D20_DIRS:
        o = p - 0.25 * np.asarray(dv)
        assert np.array_equal(o.astype(np.float32).astype(np.float64), o), "the origin is not an fp32: choose another direction"
        for r in (0.0, ULP):
            org.append(o); dirs.append(dv); rad.append(r)
    cell = np.ldexp(1.0, -abi.MAX_DEPTH)
    org.append(p - np.array([0.25, 0.0, 0.0]) + np.array([0.0, 2.0 * cell + 0.25 * cell, 0.0]))
    dirs.append((1.0, 0.0, 0.0)); rad.append(0.0)
    rec = Rays(np.array(org), np.array(dirs), 0.0, 1.0, np.array(rad), 0.0)
    assert np.array_equal(rec.record()["origin"][:-1].astype(np.float64), np.array(org[:-1]))
    return rec, len(org) - 1


def d20_many_rays(n=320):
    """n rays of radius 0 through the point, from seeded dyadic directions: many rays share one level-20 node."""
    rs = np.random.RandomState(61)
    # eighths, kept where point - dir / 4 stays below the next power of two above the point's coordinate: the origin is then an fp32
    dv = np.stack([rs.randint(-6, 9, size=n), rs.randint(-8, 9, size=n), rs.randint(-1, 9, size=n)], axis=1).astype(np.float64) / 8.0
    dv[(dv == 0).all(1)] = (1.0, 0.0, 0.0)
    p = np.array(POINT, dtype=np.float64)
    org = p - 0.25 * dv
    assert np.array_equal(org.astype(np.float32).astype(np.float64), org)
    return Rays(org, dv, 0.0, 1.0, 0.0, 0.0)


D20_RADII = (0.0, 2.0 ** -22, 1e-3)


def d20_spheres():
    """One query at the point per radius of D20_RADII."""
    return Spheres(np.array([POINT] * len(D20_RADII), dtype=np.float64), np.array(D20_RADII))


def d20_many_spheres(n=320):
    """n queries at the point, radii 0 .. 2^-21 in turn."""
    return Spheres(np.array([POINT] * n, dtype=np.float64), np.ldexp(np.arange(n) % 3, -22))


def d20_regions(export):
    """{name: (Region, how many of the k identical points it keeps: 'all' or 'none')}: the half-spaces x >= the point's x one fp32 ulp to
    either side, and a box around the level-20 cell alone (inside its level-19 parent, half a level-20 cell beyond the cell's faces)."""
    x = np.float32(POINT[0])
    below, above = np.nextafter(x, np.float32(0.0)), np.nextafter(x, np.float32(1.0))
    e, _ = deep_entry(export)
    nd = export.nodes[e]
    cell = np.ldexp(1.0, -abi.MAX_DEPTH)
    lo = np.array([nd["X"], nd["Y"], nd["Z"]], dtype=np.float64) * cell
    return {"x>=below": (Region.from_planes([[1.0, 0.0, 0.0, -float(below)]]), "all"),
            "x>=above": (Region.from_planes([[1.0, 0.0, 0.0, -float(above)]]), "none"),
            "cell20": (Region.from_box(lo - 0.5 * cell, lo + 1.5 * cell), "all")}


FRACTION_DECIDED = ("lo_x=x", "hi_x=x")           # the point lies ON a vertical edge of these: c == 0 exactly, for all k identical points


def d20_footprints():
    """{name: (Footprint, how many of the k identical points it keeps: 'all' or 'none')}: plan-view rectangles whose corners are fp32 numbers
    (asserted: record() holds them unrounded).  `cell` is the level-20 cell of POINT with half a cell more on every side; the others have one
    side at the point's own x or y, or one fp32 step from it, and take a share of the uniform points too.  Footprint.from_rect's convention
    is lo_x <= x <= hi_x and lo_y <= y < hi_y."""
    x, y = np.float32(POINT[0]), np.float32(POINT[1])
    nxt = lambda v, to: float(np.nextafter(v, np.float32(to)))
    x, y, x_below, x_above, y_above = float(x), float(y), nxt(x, 0.0), nxt(x, 1.0), nxt(y, 1.0)
    cell = np.ldexp(1.0, -abi.MAX_DEPTH)
    cx, cy = np.floor(x / cell) * cell, np.floor(y / cell) * cell
    rects = {"cell": ((cx - 0.5 * cell, cy - 0.5 * cell), (cx + 1.5 * cell, cy + 1.5 * cell), "all"),
             "lo_x=x": ((x, 0.125), (0.5, 0.875), "all"),
             "lo_x=above": ((x_above, 0.125), (0.5, 0.875), "none"),
             "hi_x=x": ((0.125, 0.125), (x, 0.875), "all"),
             "hi_x=below": ((0.125, 0.125), (x_below, 0.875), "none"),
             "lo_y=y": ((0.125, y), (0.5, 0.75), "all"),
             "hi_y=y": ((0.125, 0.5), (0.5, y), "none"),
             "hi_y=above": ((0.125, 0.5), (0.5, y_above), "all")}
    out = {}
    for key, (lo, hi, keeps) in rects.items():
        f = Footprint.from_rect(lo, hi)
        want = np.array([(lo[0], lo[1]), (lo[0], hi[1]), (hi[0], hi[1]), (hi[0], lo[1])], dtype=np.float64)
        assert np.array_equal(f.record()["vertices"][0, :4].astype(np.float64), want), f"{key}: a corner is not an fp32 number"
        out[key] = (f, keeps)
    return out
