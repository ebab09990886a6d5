"""Shared by the footprint-query tests: the footprints they use, placed relative to a case's box, the two footprints of the 3 M-point
terrain, the shifted inputs of the box-offset tests, and `contains_exact`, rule F1 with every edge's side decided exactly."""
from fractions import Fraction

import numpy as np

from simlod_amd.octree_io import Footprint

FOOTPRINT_NAMES = ["star7", "star128", "oblique", "rect", "cover", "miss", "bowtie"]
SLOW_FOOTPRINTS = {"star128": ("ragged_tiny", "terrain_4x100k")}          # 256 edges: the numpy loop over them is the slow part
OBLIQUE_U, OBLIQUE_V = (0.8, 0.6, 0.1, -3.0), (-0.6, 0.8, 0.2, 5.0)
# footprints in a box off the origin (tests/test_gpu_box_origin.py, tests/test_footprint_io.py): the (case, offset) pairs of the region query's
# test there, the footprints every pair gets, and the pairs that get the 256-edge star too
SHIFTED = [("uniform_3x40k", "inexact"), ("terrain_4x100k", "georef"), ("hotspot_150k", "dyadic"), ("terrain_4x100k", "inexact")]
SHIFTED_KINDS = ["star7", "oblique", "rect", "bowtie", "miss"]
SHIFTED_STAR128 = ("uniform_3x40k", "hotspot_150k")
SURE = 2.0 ** -50


def contains_exact(footprint, points, return_decided=False):
    """Rule F1 with the EXACT sign of c = du * (v - a_v) - dv * (u - a_u) per edge, for the fp64 (u, v) of Footprint.project (the header's
    operation order, taken as data) and the fp64 edge values of Footprint.edges.

    Per point and edge p = du * (v - a_v), q = dv * (u - a_u) and c = p - q in fp64 carry five roundings of at most 2^-53 each (the two
    differences, the two products, the last difference): the error of c is below 2^-51 (|p| + |q|), so where |c| > 2^-50 (|p| + |q|) the
    fp64 sign is the exact one.  A point with an edge that crosses its v and is not decided that way is decided edge by edge in
    fractions.Fraction on the same fp64 values, once per distinct (u, v).
    -> a boolean per point; return_decided: and a boolean per point, whether Fractions decided it."""
    p = np.asarray(points)
    u, v = footprint.project(*(p[a].astype(np.float64) for a in ("x", "y", "z")))
    if not (np.isfinite(u).all() and np.isfinite(v).all()):
        raise ValueError("a projected coordinate is not finite: the exact rule has no side for it")
    edges = list(zip(*footprint.edges()))
    odd, hard = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for a_u, a_v, b_v, du, dv in edges:
        pp, qq = du * (v - a_v), dv * (u - a_u)
        c = pp - qq
        sure = np.abs(c) > SURE * (np.abs(pp) + np.abs(qq))
        crosses = (a_v > v) != (b_v > v)
        odd ^= crosses & sure & ((c > 0) == (dv > 0))
        hard |= crosses & ~sure
    if hard.any():
        uv, inverse = np.unique(np.stack([u[hard], v[hard]], axis=1), axis=0, return_inverse=True)
        verdict = np.zeros(len(uv), bool)
        for k, (uk, vk) in enumerate(uv):
            fu, fv = Fraction(float(uk)), Fraction(float(vk))
            for a_u, a_v, b_v, du, dv in edges:
                if (a_v > vk) != (b_v > vk):
                    c = Fraction(float(du)) * (fv - Fraction(float(a_v))) - Fraction(float(dv)) * (fu - Fraction(float(a_u)))
                    verdict[k] ^= (c > 0) == (dv > 0)
        odd[hard] = verdict[inverse.reshape(-1)]
    return (odd, hard) if return_decided else odd


def star(cx, cy, r0, r1, n):
    """2n vertices alternating radius r0 / r1 at the angles k * pi / n, rounded to float32."""
    k = np.arange(2 * n)
    r = np.where(k % 2 == 0, float(r0), float(r1))
    a = k * np.pi / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1).astype(np.float32)


def names_for(case):
    return [k for k in FOOTPRINT_NAMES if case in SLOW_FOOTPRINTS.get(k, (case,))]


def footprint(kind, box, box_min=(0, 0, 0)):
    """The test footprints for the box [box_min, box_min + box] (the octree's cube has the largest extent as its size)."""
    box = np.asarray(box, dtype=np.float64)
    mn = np.asarray(box_min, dtype=np.float64)
    size = float(box.max())
    cx, cy = mn[0] + box[0] / 2, mn[1] + box[1] / 2
    m = float(min(box[0], box[1]))
    if kind == "star7":
        return Footprint.from_xy(star(cx, cy, 0.45 * m, 0.15 * m, 7))
    if kind == "star128":
        return Footprint.from_xy(star(cx, cy, 0.45 * m, 0.15 * m, 128))
    if kind == "oblique":
        c = mn + box / 2
        uc = float(np.dot(OBLIQUE_U[:3], c) + OBLIQUE_U[3])
        vc = float(np.dot(OBLIQUE_V[:3], c) + OBLIQUE_V[3])
        return Footprint([(uc - 0.35 * m, vc - 0.25 * m), (uc + 0.40 * m, vc - 0.10 * m), (uc - 0.05 * m, vc + 0.35 * m)], OBLIQUE_U, OBLIQUE_V)
    if kind == "rect":                     # the rectangle of region_ref's "box" region
        return Footprint.from_rect(rect_of(box, mn)[0], rect_of(box, mn)[1])
    if kind == "cover":                    # 10 % larger than the xy projection of the octree's cube: every node lies inside
        return Footprint.from_rect((mn[0] - 0.1 * size, mn[1] - 0.1 * size), (mn[0] + 1.1 * size, mn[1] + 1.1 * size))
    if kind == "miss":                     # three box sizes away, in u and in v (rule F3 has a range test in v only: every edge is FAR by it)
        q = lambda fx, fy: (mn[0] + fx * size, mn[1] + fy * size)
        return Footprint.from_xy([q(3.0, 3.0), q(3.5, 3.0), q(3.2, 3.5)])
    if kind == "bowtie":                   # crossing order: two triangles that meet in the centre
        p = lambda fx, fy: (mn[0] + fx * box[0], mn[1] + fy * box[1])
        return Footprint.from_xy([p(0.2, 0.2), p(0.8, 0.8), p(0.2, 0.8), p(0.8, 0.2)])
    raise KeyError(kind)


def rect_of(box, mn=(0, 0, 0)):
    """(lo, hi) of the "rect" footprint: 30-70 % x 20-90 % of the xy extents."""
    box, mn = np.asarray(box, np.float64), np.asarray(mn, np.float64)
    return (mn[0] + 0.3 * box[0], mn[1] + 0.2 * box[1]), (mn[0] + 0.7 * box[0], mn[1] + 0.9 * box[1])


# the 3 M-point terrain of test_gpu_region.py (synthetic.terrain(3_000_000, seed=3, box=(600, 400, 40), tile=50))
TERRAIN_3M = dict(n=3_000_000, seed=3, box=(600.0, 400.0, 40.0), tile=50.0)


def terrain3m_footprints():
    return {"star": Footprint.from_xy(star(300, 200, 190, 70, 7)), "triangle": Footprint.from_xy([(50, 50), (550, 80), (250, 380)])}
