"""Shared by the lasso-query tests: the lassos they use, in pixel coordinates of the 256 x 256 test screen, the cameras they go with, the mask of
the contract's samples (finite, in the half-open box), and `contains_exact`, rule L1 with every comparison and every edge's side decided
exactly."""
from fractions import Fraction

import numpy as np

import cases
import footprint_ref as fr
from simlod_amd import camera
from simlod_amd.octree_io import Lasso, _box_of

W, H = cases.W, cases.H
LASSO_NAMES = ["star7", "star128", "rect", "tri", "bowtie", "cover", "miss"]
SLOW_LASSOS = {"star128": ("ragged_tiny", "uniform_3x40k")}                # 256 edges: the numpy loop over them is the slow part
CAMERAS = ["bird", "closer", "inside", "away"]
MODES = [("cut", 20), ("all", 20), ("cut", 2)]
SHIFTED = fr.SHIFTED                                                        # the (case, offset) pairs of the box-offset tests
SHIFTED_KINDS = ["star7", "rect", "tri", "bowtie", "miss"]
SURE = 2.0 ** -50


def transform(which, box, offset=(0.0, 0.0, 0.0)):
    """The row-major world-view-projection matrix of the named camera of cases.camera_pose on the test screen."""
    return camera.lookat_transform(*cases.camera_pose(which, box, offset), W, H)


def pixels(kind):
    """The named polygons, in continuous pixel coordinates of the W x H screen."""
    if kind == "star7":
        return fr.star(128, 128, 110, 40, 7)
    if kind == "star128":
        return fr.star(128, 128, 110, 40, 128)
    if kind == "rect":                     # (96, 100) - (160, 150), in the orientation of Footprint.from_rect
        return np.array([(96, 100), (96, 150), (160, 150), (160, 100)], np.float32)
    if kind == "tri":
        return np.array([(40, 60), (220, 90), (110, 230)], np.float32)
    if kind == "half":                     # the left half of the screen (inverse_ref.half_screen; the builder states scale it onto the points' picture)
        return np.array([(0, 0), (W / 2, 0), (W / 2, H), (0, H)], np.float32)
    if kind == "bowtie":                   # crossing order: two triangles that meet in the centre
        return np.array([(50, 50), (200, 200), (50, 200), (200, 50)], np.float32)
    if kind == "cover":                    # 64 screens wide: larger than the picture of a box that lies in front of the camera
        return np.array([(-64 * W, -64 * H), (-64 * W, 65 * H), (65 * W, 65 * H), (65 * W, -64 * H)], np.float32)
    if kind == "miss":                     # three screens away, in u and in v
        return np.array([(3.0 * W, 3.0 * H), (3.5 * W, 3.0 * H), (3.2 * W, 3.5 * H)], np.float32)
    raise KeyError(kind)


def names_for(case):
    return [k for k in LASSO_NAMES if case in SLOW_LASSOS.get(k, (case,))]


def lasso(kind, T):
    """The named lasso on the test screen of the camera T."""
    return Lasso.from_pixels(T, W, H, pixels(kind))


def inbox(pts, box_min, box_max):
    """The samples of the contract: finite and in the half-open box of the region section (a NaN compares false)."""
    mn, size = _box_of(box_min, box_max)
    ok = np.ones(len(pts), bool)
    with np.errstate(invalid="ignore"):
        for k, a in enumerate("xyz"):
            c = pts[a].astype(np.float64)
            ok &= (c >= mn[k]) & (c < mn[k] + size)
    return ok


def contains_exact(lasso_, points, return_decided=False):
    """Rule L1 with the EXACT sign of c = du * (V - a_v * W) - dv * (U - a_u * W) per edge and the EXACT comparisons a_v * W > V, b_v * W > V, for
    the fp64 (U, V, W) of Lasso.project (the header's operation order, taken as data) and the fp64 edge values of Lasso.edges.

    In fp64 sa = a_v * W carries one rounding of at most 2^-53 |sa|, so where |sa - V| > 2^-50 |sa| the computed comparison is the exact one.
    p = du * (V - sa) carries that rounding times |du|, the difference's and the product's; q = dv * (U - a_u * W) likewise; c = p - q one more:
    the error of c is below 2^-51 (|p| + |q|) + 2^-53 (|du * sa| + |dv * a_u * W|), so where |c| > 2^-50 (|p| + |q| + |du * sa| + |dv * a_u * W|)
    the fp64 sign is the exact one.  A point with W > 0 and an edge not decided that way is decided edge by edge in fractions.Fraction on the
    same fp64 values, once per distinct (U, V, W).
    -> a boolean per point; return_decided: and a boolean per point, whether Fractions decided it."""
    p = np.asarray(points)
    U, V, Wc = lasso_.project(*(p[a].astype(np.float64) for a in ("x", "y", "z")))
    if not (np.isfinite(U).all() and np.isfinite(V).all() and np.isfinite(Wc).all()):
        raise ValueError("a projected coordinate is not finite: the exact rule has no side for it")
    edges = list(zip(*lasso_.edges()))
    front = Wc > 0
    odd, hard = np.zeros(len(p), bool), np.zeros(len(p), bool)
    for a_u, a_v, b_v, du, dv in edges:
        sa, sb, au_w = a_v * Wc, b_v * Wc, a_u * Wc
        cmp_sure = (np.abs(sa - V) > SURE * np.abs(sa)) & (np.abs(sb - V) > SURE * np.abs(sb))
        pp, qq = du * (V - sa), dv * (U - au_w)
        c = pp - qq
        c_sure = np.abs(c) > SURE * (np.abs(pp) + np.abs(qq) + np.abs(du * sa) + np.abs(dv * au_w))
        crosses = (sa > V) != (sb > V)
        odd ^= crosses & cmp_sure & c_sure & ((c > 0) == (dv > 0))
        hard |= ~cmp_sure | (crosses & ~c_sure)
    hard &= front
    if hard.any():
        uvw, inverse = np.unique(np.stack([U[hard], V[hard], Wc[hard]], axis=1), axis=0, return_inverse=True)
        verdict = np.zeros(len(uvw), bool)
        for k, (uk, vk, wk) in enumerate(uvw):
            fu, fv, fw = Fraction(float(uk)), Fraction(float(vk)), Fraction(float(wk))
            for a_u, a_v, b_v, du, dv in edges:
                fa, fb = Fraction(float(a_v)) * fw, Fraction(float(b_v)) * fw
                if (fa > fv) != (fb > fv):
                    c = Fraction(float(du)) * (fv - fa) - Fraction(float(dv)) * (fu - Fraction(float(a_u)) * fw)
                    verdict[k] ^= (c > 0) == (dv > 0)
        odd[hard] = verdict[inverse.reshape(-1)]
    odd &= front
    return (odd, hard) if return_decided else odd
