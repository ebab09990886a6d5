"""Shared by the surface tests: rules N1-N10 of "surface queries" (include/simlod_hip.h) restated one sample at a time in plain Python — a brute
force over ALL of b for every sample of a, with no grid; Python integers for rules N2 and N3, Python floats (IEEE fp64, one rounding per
operation, `a*a + b*b` fuses nothing, subnormals kept) for the rest, `struct` for rule N4's bits and for the rounding to fp32.  The
neighbourhood's rules (C1, C2, C4) and the grid's fields come from compare_ref, as rule N1 says.  Nothing here uses octree_io's vectorised
mirror or numpy arithmetic (numpy only hands over the fields and takes the result)."""
import math
import struct

import numpy as np

import compare_ref as cr
from simlod_amd import abi

SHADE, VARIATION = 0, 1
DIRECTION, POSITION = 0, 1
Q_SCALE = 16384.0
SQUARINGS = 8
MISS_COLOR = 0xFF123456
TABLE = (np.arange(256, dtype=np.uint32) * np.uint32(0x00010101)) | np.uint32(0xFF000000)

points, f32 = cr.points, cr.f32


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def params_acceptable(r):
    """The refusals of one abi.surface_params_dtype record: the compare record's, the two modes, light and orient finite, no zero light
    with SHADE."""
    r = np.asarray(r, dtype=abi.surface_params_dtype).reshape(-1)[0]
    if not cr.params_acceptable(float(r["radius"]), r["thresholds"].tolist(), int(r["reserved"])):
        return False
    if int(r["colourBy"]) > VARIATION or int(r["orientMode"]) > POSITION:
        return False
    light, orient = [float(v) for v in r["light"]], [float(v) for v in r["orient"]]
    if not all(math.isfinite(v) for v in light + orient):
        return False
    return not (int(r["colourBy"]) == SHADE and light == [0.0, 0.0, 0.0])


def invq_of(radius, size):
    """Rule N2: invq = 16384.0 / h."""
    return Q_SCALE / cr.h_of(radius, size)


def q_of(p, invq):
    """Rule N2: truncation towards zero."""
    return int(p * invq)


def widen(s):
    """Rule N3's D: the arithmetic shift, the exact product, one rounded add."""
    return float(s >> 32) * 4294967296.0 + float(s & 0xFFFFFFFF)


def factor_of(sym):
    """Rule N4: (f, m != 0) for the six entries of a symmetric matrix."""
    m = max(abs(x) for x in sym)
    e = (bits_of(m) >> 52) & 0x7FF
    return from_bits((2046 - e) << 52), m != 0.0


def scale(sym):
    f, ok = factor_of(sym)
    return [x * f for x in sym], ok


def moments(S, within):
    """Rule N3: the six entries xx, xy, xz, yy, yz, zz of M from the nine sums x, y, z, xx, xy, xz, yy, yz, zz."""
    n = float(within)
    dx, dy, dz = widen(S[0]), widen(S[1]), widen(S[2])
    return [n * widen(S[3]) - dx * dx, n * widen(S[4]) - dx * dy, n * widen(S[5]) - dx * dz,
            n * widen(S[6]) - dy * dy, n * widen(S[7]) - dy * dz, n * widen(S[8]) - dz * dz]


def square(B):
    xx, xy, xz, yy, yz, zz = B
    return [(xx * xx + xy * xy) + xz * xz, (xx * xy + xy * yy) + xz * yz, (xx * xz + xy * yz) + xz * zz,
            (xy * xy + yy * yy) + yz * yz, (xy * xz + yy * yz) + yz * zz, (xz * xz + yz * yz) + zz * zz]


def estimate(S, within, c, orient, orient_mode, trace=None):
    """Rules N3-N7 for one sample -> None (degenerate, rule N9) or (v, lambdaNum, lambdaDen, vv); trace: a list that receives M and every B."""
    if within < 3:
        return None
    M, ok = scale(moments(S, within))
    if not ok:
        return None
    t = (M[0] + M[3]) + M[5]
    B = [t - M[0], -M[1], -M[2], t - M[3], -M[4], t - M[5]]
    if trace is not None:
        trace += [M, B]
    for _ in range(SQUARINGS):
        B, nz = scale(square(B))
        ok = ok and nz
        if trace is not None:
            trace.append(B)
    if not ok:
        return None
    xx, xy, xz, yy, yz, zz = B
    v, best = [xx, xy, xz], xx
    if yy > best:
        v, best = [xy, yy, yz], yy
    if zz > best:
        v = [xz, yz, zz]
    o = list(orient) if orient_mode == DIRECTION else [orient[k] - c[k] for k in range(3)]
    if (v[0] * o[0] + v[1] * o[1]) + v[2] * o[2] < 0.0:
        v = [-x for x in v]
    w = [(M[0] * v[0] + M[1] * v[1]) + M[2] * v[2], (M[1] * v[0] + M[3] * v[1]) + M[4] * v[2], (M[2] * v[0] + M[4] * v[1]) + M[5] * v[2]]
    num = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]
    vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    return v, num, vv * t, vv


def colour_terms(est, colour_by, light):
    """Rule N8: (num, den)."""
    v, lnum, lden, vv = est
    if colour_by == SHADE:
        a = (v[0] * light[0] + v[1] * light[1]) + v[2] * light[2]
        return a * abs(a), vv * ((light[0] * light[0] + light[1] * light[1]) + light[2] * light[2])
    return lnum, lden


def index_of(thresholds, num, den):
    """Rule N8: the number of thresholds with t * den <= num, counted one by one."""
    return sum(1 for t in thresholds if t * den <= num)


def sums_of(p, pb, valid_b, rr, invq):
    """Rules C2, N2, N3 for the centre p over all of b -> (the nine sums, within)."""
    S, within = [0] * 9, 0
    for j in valid_b:
        d = [pb[j][k] - p[k] for k in range(3)]
        if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= rr:
            q = [q_of(d[k], invq) for k in range(3)]
            within += 1
            for k, v in enumerate((q[0], q[1], q[2], q[0] * q[0], q[0] * q[1], q[0] * q[2], q[1] * q[1], q[1] * q[2], q[2] * q[2])):
                S[k] += v
    return S, within


def surface_exact(a, b, box_min, size, record, count_only=False, trace=None):
    """simlod_surface_samples on `a` and `b` (abi.point_dtype) with the abi.surface_params_dtype `record`, one sample at a time -> (records
    as abi.surface_record_dtype, colours as uint32, the summary as an abi.surface_summary_dtype record); records and colours are None for a
    count-only call and when the budget is exceeded.  trace: a list that receives, per estimated or degenerate-by-N4 sample, its matrices."""
    r = np.asarray(record, dtype=abi.surface_params_dtype).reshape(-1)[0]
    radius, thresholds = float(r["radius"]), [float(v) for v in r["thresholds"]]
    light, orient = [float(v) for v in r["light"]], [float(v) for v in r["orient"]]
    colour_by, orient_mode, miss = int(r["colourBy"]), int(r["orientMode"]), int(r["missColor"])
    # the grid's fields and the budget: the compare query's (rule N1)
    _, _, grid = cr.compare_exact(a, b, box_min, size, radius, np.zeros(255), TABLE, 0, max_candidates=int(r["maxCandidates"]), count_only=True)
    out = np.zeros((), dtype=abi.surface_summary_dtype)
    for f in ("error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numCandidates"):
        out[f] = grid[f]
    if count_only or int(out["error"]) != 0:
        return None, None, out
    invq, rr = invq_of(radius, float(np.float32(size))), radius * radius
    pa, pb = cr._xyz(a), cr._xyz(b)
    valid_b = [j for j, s in enumerate(pb) if cr.is_valid(*s)]
    rec = np.zeros(len(pa), dtype=abi.surface_record_dtype)
    colours = np.zeros(len(pa), np.uint32)
    hist = [0] * 257
    estimated = degenerate = within_sum = 0
    for i, p in enumerate(pa):
        est, within = None, 0
        if cr.is_valid(*p):
            S, within = sums_of(p, pb, valid_b, rr, invq)
            tr = None if trace is None else []
            est = estimate(S, within, p, orient, orient_mode, tr)
            if trace is not None:
                trace.append(tr)
            if est is None:
                degenerate += 1
            else:
                estimated += 1
        k = 256
        if est is not None:
            k = index_of(thresholds, *colour_terms(est, colour_by, light))
            rec[i] = (tuple(f32(x) for x in est[0]), within, est[1], est[2])
        else:
            rec[i] = ((0.0, 0.0, 0.0), within, 0.0, 0.0)
        hist[k] += 1
        colours[i] = int(r["table"][k]) if k < 256 else miss
        within_sum += within
    out["numEstimated"], out["numDegenerate"], out["numWithin"], out["hist"] = estimated, degenerate, within_sum, hist
    return rec, colours, out


# ---- parameter records ---------------------------------------------------------------------------------------------------------------------
def shade_thresholds():
    """Surface.hillshade's: c * |c| with c = -1 + (i + 1) / 128."""
    return [c * abs(c) for c in (-1.0 + (i + 1) / 128.0 for i in range(255))]


def variation_thresholds(vmax=1.0 / 3.0):
    """Surface.variation's: (i + 1) * vmax / 255."""
    return [((i + 1) * vmax) / 255.0 for i in range(255)]


def params(radius, colour_by, thresholds=None, light=(0.0, 0.0, 1.0), orient=(0.0, 0.0, 1.0), orient_mode=DIRECTION, budget=0, wg=0, reserved=0):
    """One abi.surface_params_dtype record, filled in by hand."""
    r = np.zeros(1, dtype=abi.surface_params_dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        r["radius"], r["light"][0], r["orient"][0] = radius, light, orient
    r["missColor"], r["maxCandidates"], r["maxWorkgroups"], r["reserved"], r["colourBy"], r["orientMode"] = MISS_COLOR, budget, wg, reserved, colour_by, orient_mode
    r["thresholds"][0] = (shade_thresholds() if colour_by == SHADE else variation_thresholds()) if thresholds is None else thresholds
    r["table"][0] = TABLE
    return r


def case_params(name, colour_by, **kw):
    """The records a case is run with for one colourBy: one per variant the case names (orientation, light, thresholds)."""
    radius, variants = case(name)[4:6]
    out = []
    for v in variants:
        v = dict(v)
        t = v.pop("thresholds", {}).get(colour_by)
        out.append(params(radius, colour_by, thresholds=t, **v, **kw))
    return out


# ---- the inputs the io tier and the GPU tier share: name -> (a, b, box_min, box_max, radius, variants) ----------------------------------------
def _flat_patch(n, spacing, origin):
    """An n x n lattice in the plane z = origin[2], every coordinate exactly representable."""
    return [[origin[0] + i * spacing, origin[1] + j * spacing, origin[2]] for i in range(n) for j in range(n)]


PLANE_NORMAL = (-1.0, 0.0, 1.0)             # plane_grid's plane z = x - 0.5, oriented towards +z


def case(name):
    rs = np.random.RandomState(29)
    unit = ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    one = [{}]
    if name == "three_points":              # within == 3, not collinear: the smallest estimate
        p = points([[1.0, 1.0, 1.0], [1.25, 1.0, 1.0], [1.0, 1.25, 1.0625]])
        return p, p.copy(), *unit, 0.5, one
    if name == "two_points":
        p = points([[1.0, 1.0, 1.0], [1.25, 1.0, 1.125]])
        return p, p.copy(), *unit, 0.5, one
    if name == "coincident":                # five equal samples: M == 0
        p = points([[1.5, 2.5, 0.75]] * 5)
        return p, p.copy(), *unit, 0.5, one
    if name == "collinear":                 # rank-1 M: the rule still defines v
        p = points([[1.0 + k / 64.0, 1.0 + k / 32.0, 2.0 - k / 128.0] for k in range(7)])
        return p, p.copy(), *unit, 0.5, one
    if name == "plane_grid":                # 7 x 7 lattice on the plane z = x - 0.5 (pz == px exactly, so the quantised offsets stay on it)
        p = points([[1.0 + i / 8.0, 1.0 + j / 8.0, 0.5 + i / 8.0] for i in range(7) for j in range(7)])
        return p, p.copy(), *unit, 0.2, one
    if name == "line_tiny":
        # ten samples along x with a random jitter in y of 1e-4 r; and three lines whose jitter is symmetric (y0, y0 + j, y0 - j at every x,
        # j = m * 2^-16 about 1e-3 r): there Mxy == 0 exactly, B stays diagonal, and its small entry (Myy / t)^(2^k) passes through the
        # subnormals at the sixth squaring on its way to 0 (tests/test_surface_io.py looks for them in the reference's trace)
        r = 0.25
        x = 0.5 + np.arange(10) * (r / 12.0)
        groups = [np.stack([x, 0.5 + (rs.rand(10) - 0.5) * 2.0e-4 * r, np.full(10, 1.0)], -1)]
        for g, m in enumerate((16, 17, 18)):
            y0, j = 1.0 + 0.5 * g, m * 2.0 ** -16
            groups.append(np.array([[xi, y, 1.0] for xi in x for y in (y0, y0 + j, y0 - j)]))
        p = points(np.concatenate(groups))
        return p, p.copy(), *unit, r, one
    if name == "cell_faces":                # neighbours in all 27 cells of a mid-cell centre; centres an ulp either side of faces, and at a corner
        r = np.float32(0.3)
        h = cr.h_of(float(r), 4.0)
        mid = np.array([3.5 * h, 4.5 * h, 5.5 * h])
        ctr = [mid]
        for k in (2, 7):
            v = np.float32(k * h)
            for x in (float(cr._ulp(v, False)), float(v), float(cr._ulp(v, True))):
                ctr += [np.array([x, 1.0, 1.0]), np.array([2.0, x, 1.0]), np.array([2.0, 2.0, x])]
        ctr.append(np.array([float(np.float32(9 * h))] * 3))
        fb = [mid + np.array([dx, dy, dz]) * h * (0.55 + 0.02 * rs.rand(3)) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
        for c in ctr[1:]:
            fb.append(c)
            for k in range(3):
                for sgn in (-1.0, 1.0):
                    q = c + (rs.rand(3) - 0.5) * 0.2 * float(r)
                    q[k] = c[k] + sgn * 0.9 * float(r)
                    fb.append(q)
        return points(ctr), points(fb), *unit, float(r), one
    if name == "hot_cell":                  # 3 000 b samples in one cell, 300 a samples in and around it
        r = 0.25
        h = cr.h_of(float(np.float32(r)), 4.0)
        lo = 5 * h
        b = points(lo + rs.rand(3000, 3) * h * 0.98 + h * 0.01)
        a = points(lo + (rs.rand(300, 3) * 3.4 - 1.2) * h)
        return a, b, *unit, r, one
    if name == "wide_sums":                 # neighbours near +-r on every axis, more of them on the negative side: Sxx >= 2^32, Sx < 0
        r, c = 0.5, np.array([2.0, 2.0, 2.0])
        fb = [c]
        for k in range(3):
            for sgn, n in ((-1.0, 40), (1.0, 20)):
                q = c + (rs.rand(n, 3) - 0.5) * 0.04 * r
                q[:, k] = c[k] + sgn * r * (0.999 - 0.02 * rs.rand(n))
                fb += list(q)
        b = points(fb)
        return points(np.concatenate([[c], np.asarray(fb)[1::15]])), b, *unit, r, one
    if name == "invalid":                   # NaN and both infinities in a and in b, samples at +-1e30, a box off the origin
        mn, mx = (100.0, -50.0, 7.0), (104.0, -46.0, 11.0)
        base = np.array(mn) + rs.rand(260, 3) * np.array([4.0, 4.0, 1.0])
        a, b = points(base[:150]), points(base[60:])
        for k, v in enumerate([np.nan, np.inf, -np.inf] * 2):
            a["xyz"[k % 3]][k] = v
            b["zxy"[k % 3]][k + 3] = v
        a["x"][20], a["y"][21], b["x"][30], b["z"][31] = 1e30, -1e30, -1e30, 1e30
        a[22], a[23] = b[31], b[30]
        return a, b, mn, mx, 0.7, one
    if name == "b_outside":                 # b entirely outside a's box
        a = points(rs.rand(150, 3) * 4.0)
        b = points(rs.rand(400, 3) * np.array([1.0, 4.0, 4.0]) + np.array([4.2, 0.0, 0.0]))
        a["x"][:50] = np.float32(3.9)
        return a, b, *unit, 0.8, one
    if name == "r0":                        # radius 0: h at its floor, coincident samples only, everything degenerate
        base = rs.rand(60, 3) * 4.0
        b = points(np.concatenate([base, base[:30], base[:30], base[:10]]))
        return points(np.concatenate([base[::2], rs.rand(10, 3) * 4.0])), b, *unit, 0.0, one
    if name in ("orient_flip", "shade_edges", "variation_edges"):
        # a flat patch (z exactly constant: v = (0, 0, v2), lambdaNum == 0, s == 0 for an o in the plane), a tilted one and a rough blob
        flat = _flat_patch(5, 0.125, (1.0, 1.0, 1.5))
        tilt = [[2.5 + i / 8.0, 1.0 + j / 8.0, 1.0 + i / 16.0 + j / 32.0] for i in range(5) for j in range(5)]
        blob = (np.array([1.0, 3.0, 3.0]) + rs.rand(40, 3) * 0.3).tolist()
        p = points(flat + tilt + blob)
        if name == "orient_flip":
            variants = [dict(orient=(0.0, 0.0, -1.0)), dict(orient=(1.0, 0.5, 0.0)), dict(orient=(0.0, 0.0, 0.0)),
                        dict(orient=(3.0, 3.0, 1.5), orient_mode=POSITION), dict(orient=(1.25, 1.25, 0.5), orient_mode=POSITION),
                        dict(orient=(1.25, 1.25, 3.5), orient_mode=POSITION)]
        elif name == "shade_edges":         # thresholds -1 and 1 present; light exactly along and against the flat patch's normal
            t = [c * abs(c) for c in (-1.0 + i / 127.0 for i in range(255))]
            variants = [dict(light=(0.0, 0.0, 1.0), thresholds={SHADE: t}), dict(light=(0.0, 0.0, -2.0), thresholds={SHADE: t})]
        else:                               # threshold 0 present: a perfect plane's lambdaNum == 0 meets it
            variants = [dict(thresholds={VARIATION: [(i / 254.0) / 3.0 for i in range(255)]})]
        return p, p.copy(), *unit, 0.2, variants
    raise KeyError(name)


CASES = ["three_points", "two_points", "coincident", "collinear", "plane_grid", "line_tiny", "cell_faces", "hot_cell", "wide_sums", "invalid", "b_outside",
         "r0", "orient_flip", "shade_edges", "variation_edges"]
# the brute force takes numA * numB steps: the big case is checked on a part of a only
EXACT_A_LIMIT = {"hot_cell": 40}
