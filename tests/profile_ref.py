"""Shared by the profile-query tests: the profiles they use, placed relative to a case's box, and `locate_exact`, rule P1 with every
comparison decided exactly."""
from fractions import Fraction

import numpy as np

from footprint_ref import OBLIQUE_U, OBLIQUE_V
from simlod_amd.octree_io import Profile

PROFILE_NAMES = ["single", "zigzag", "hairpin", "wave64", "cover", "miss", "oblique", "narrow"]
OBLIQUE_H = (0.05, -0.1, 0.99, 2.5)
SURE = 2.0 ** -50
# Half-widths as fractions of the smaller plan extent.  The octrees of tests/cases.py are two to four levels deep: the leaves of terrain_4x100k
# are 150 m cubes in a 600 m x 400 m box, and a node is COPIED only when ONE segment's rectangle holds its whole plan square — a half-width of
# 75 m (|cos| + |sin|) for a segment at that angle, a segment at least as long.  So the corridors that must copy a node there
# (tests/test_profile_io.py test_profiles_are_not_vacuous) are a quarter of the box wide, and wave64's sinusoid runs far beyond the box so that its
# 63 segments are 200 m long each.  `narrow` is `single` at the 3 % a user would draw; tests/test_gpu_profile.py has narrow corridors that
# copy nodes on a 20-deep octree.
WIDTH = {"single": 0.30, "zigzag": 0.27, "hairpin": 0.22, "wave64": 0.22, "oblique": 0.05, "narrow": 0.03}


def profile(kind, box, box_min=(0, 0, 0)):
    """The test profiles for the box [box_min, box_min + box] (the octree's cube has the largest extent as its size)."""
    box = np.asarray(box, dtype=np.float64)
    mn = np.asarray(box_min, dtype=np.float64)
    size = float(box.max())
    m = float(min(box[0], box[1]))
    p = lambda fx, fy: (mn[0] + fx * box[0], mn[1] + fy * box[1])
    if kind in ("single", "narrow"):       # one diagonal segment
        return Profile.from_xy([p(0.08, 0.12), p(0.93, 0.86)], WIDTH[kind] * m)
    if kind == "zigzag":                   # five vertices: four bends of different angles
        return Profile.from_xy([p(0.05, 0.2), p(0.3, 0.8), p(0.5, 0.25), p(0.72, 0.85), p(0.95, 0.4)], WIDTH["zigzag"] * m)
    if kind == "hairpin":                  # out and back at a small angle: the two rectangles overlap over most of their length
        return Profile.from_xy([p(0.1, 0.54), p(0.9, 0.58), p(0.1, 0.62)], WIDTH["hairpin"] * m)
    if kind == "wave64":                   # 64 vertices on two periods of a sinusoid 21 box lengths long, the box in its middle
        t = np.linspace(0.0, 1.0, 64)
        return Profile.from_xy(np.stack([mn[0] + (0.5 + 21.0 * (t - 0.5) - 1.0 / 24.0) * box[0], mn[1] + (0.5625 + 0.1 * np.sin(4 * np.pi * t)) * box[1]], axis=1),
                               WIDTH["wave64"] * m)
    if kind == "cover":                    # one segment three cube sizes long through the cube's middle, wider than the cube: every node lies inside
        return Profile.from_xy([(mn[0] - size, mn[1] + 0.5 * size), (mn[0] + 2.0 * size, mn[1] + 0.5 * size)], 2.0 * size)
    if kind == "miss":                     # three box sizes away
        q = lambda fx, fy: (mn[0] + fx * size, mn[1] + fy * size)
        return Profile.from_xy([q(3.0, 3.0), q(3.5, 3.2), q(3.2, 3.6)], 0.05 * size)
    if kind == "oblique":                  # the footprints' oblique plane, and a height that is not z
        c = mn + box / 2
        uc = float(np.dot(OBLIQUE_U[:3], c) + OBLIQUE_U[3])
        vc = float(np.dot(OBLIQUE_V[:3], c) + OBLIQUE_V[3])
        return Profile([(uc - 0.4 * m, vc - 0.3 * m), (uc + 0.1 * m, vc + 0.05 * m), (uc + 0.45 * m, vc - 0.2 * m)], WIDTH["oblique"] * m, OBLIQUE_U, OBLIQUE_V, OBLIQUE_H)
    raise KeyError(kind)


def locate_exact(prof, points, return_decided=False):
    """Rule P1 with every comparison decided exactly, for the fp64 (u, v) of Profile.project (the header's operation order, taken as data), the
    fp64 a_u, a_v, du, dv of Profile.segments (exact differences of fp32 numbers) and the half-width: a point is in segment i iff
    0 <= al <= du^2 + dv^2 and c^2 <= w^2 (du^2 + dv^2) with al = du (u - a_u) + dv (v - a_v) and c = du (v - a_v) - dv (u - a_u) as real numbers.

    With p = du * (u - a_u), q = dv * (v - a_v): al = p + q in fp64 carries five roundings of at most 2^-53 each, so its error is below
    2^-51 (|p| + |q|); L2 carries three.  Where |al| > 2^-50 (|p| + |q|) and |al - L2| > 2^-50 (|p| + |q| + L2) the fp64 comparisons are the exact
    ones.  Likewise c = p' - q' has an error e_c < 2^-51 (|p'| + |q'|) and |c| <= |p'| + |q'|, so c*c is off by less than
    2 |c| e_c + e_c^2 + 2^-53 c^2 < 2^-49 (|p'| + |q'|)^2, and W2 = (w*w)*L2 by less than 2^-50 W2: where |c*c - W2| > 2^-48 ((|p'| + |q'|)^2 + W2) the
    fp64 comparison is the exact one.  A point with a comparison that is not clear for some segment is located in fractions.Fraction, every
    segment of it.
    -> the segment per point (int64, -1: none); return_decided: and a boolean per point, whether Fractions decided it."""
    pt = np.asarray(points)
    u, v = prof.project(*(pt[a].astype(np.float64) for a in ("x", "y", "z")))
    if not (np.isfinite(u).all() and np.isfinite(v).all()):
        raise ValueError("a projected coordinate is not finite: the exact rule has no verdict for it")
    segs = prof.segments()
    seg = np.full(len(pt), -1, np.int64)
    hard = np.zeros(len(pt), bool)
    for i, s in enumerate(segs):
        pu, pv = u - s["au"], v - s["av"]
        p, q = s["du"] * pu, s["dv"] * pv
        al = p + q
        pp, qq = s["du"] * pv, s["dv"] * pu
        c = pp - qq
        ma, mc = np.abs(p) + np.abs(q), np.abs(pp) + np.abs(qq)
        sure = (np.abs(al) > SURE * ma) & (np.abs(al - s["L2"]) > SURE * (ma + s["L2"])) & (np.abs(c * c - s["W2"]) > 4 * SURE * (mc * mc + s["W2"]))
        # a comparison that is clear and FAILS settles the segment whatever the others say
        out = ((al < 0) & (np.abs(al) > SURE * ma)) | ((al > s["L2"]) & (np.abs(al - s["L2"]) > SURE * (ma + s["L2"]))) | \
              ((c * c > s["W2"]) & (np.abs(c * c - s["W2"]) > 4 * SURE * (mc * mc + s["W2"])))
        inside = sure & (al >= 0) & (al <= s["L2"]) & (c * c <= s["W2"])
        hard |= (seg < 0) & ~out & ~inside
        seg[(seg < 0) & inside & ~hard] = i
    if hard.any():
        w = Fraction(float(prof.half_width))
        F = [tuple(Fraction(float(s[k])) for k in ("au", "av", "du", "dv")) for s in segs]
        for k in np.nonzero(hard)[0]:
            fu, fv = Fraction(float(u[k])), Fraction(float(v[k]))
            seg[k] = -1
            for i, (au, av, du, dv) in enumerate(F):
                al, c, L2 = du * (fu - au) + dv * (fv - av), du * (fv - av) - dv * (fu - au), du * du + dv * dv
                if 0 <= al <= L2 and c * c <= w * w * L2:
                    seg[k] = i
                    break
    return (seg, hard) if return_decided else seg
