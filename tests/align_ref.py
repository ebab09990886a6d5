"""Shared by the align tests: rules A1-A6 of "align queries" (include/simlod_hip.h) restated one sample at a time in plain Python — the pose,
a brute force over ALL of b for every sample of a with no grid, the quantisation and the sums; Python floats (IEEE fp64, one rounding per
operation, `a*b + c*d` fuses nothing) where the header prescribes fp64 arithmetic, Python integers for everything else.  The grid's fields
(numCells, maxCellPopulation, numCandidates) come from a dictionary of cells.  Nothing here uses octree_io's vectorised mirror or numpy
arithmetic (numpy only hands over the fields and takes the result).  Also the stamp's comparison (rule A7), and the cases and the
registration scene the io tier and the GPU tier share."""
import math

import numpy as np

import compare_ref as cr
from simlod_amd import abi

MISS = cr.MISS
CELLS = cr.CELLS
Q_SCALE = 16777216.0
KNOWN_FLAGS = 0x3
STAMP_MAGIC = 0x414C4753
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def params(radius, grid_radius=None, pose=None, flags=0, budget=0, wg=0, reserved=0):
    """One abi.align_params_dtype record, field by field (no Align object: refused values must be expressible)."""
    r = np.zeros(1, dtype=abi.align_params_dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        r["radius"], r["gridRadius"] = radius, radius if grid_radius is None else grid_radius
    r["maxCandidates"], r["flags"], r["maxWorkgroups"], r["reserved"] = budget, flags, wg, reserved
    r["pose"][0] = IDENTITY if pose is None else np.asarray(pose, np.float64).reshape(-1)
    return r


def params_acceptable(rec):
    """Rule A8's refusals of the record: the radius, gridRadius, the pose, the flags, the reserved word."""
    r = np.asarray(rec, dtype=abi.align_params_dtype).reshape(-1)[0]
    radius, grid = float(r["radius"]), float(r["gridRadius"])
    if not math.isfinite(radius) or not radius >= 0.0 or not math.isfinite(grid) or not grid >= radius:
        return False
    if int(r["flags"]) & ~KNOWN_FLAGS or int(r["reserved"]) != 0:
        return False
    return all(math.isfinite(float(v)) for v in r["pose"])


def posed(T, c):
    """Rule A1: c'_k = ((T_k0*cx + T_k1*cy) + T_k2*cz) + T_k3 from the widened sample c -> (c', valid)."""
    out = []
    for k in range(3):
        out.append(((T[4 * k] * c[0] + T[4 * k + 1] * c[1]) + T[4 * k + 2] * c[2]) + T[4 * k + 3])
    return out, all(math.isfinite(v) for v in c) and all(math.isfinite(v) for v in out)


def cell_of(x, box_min, inv):
    """Rule A2 on one axis: C4's clamp applied to t = (x - min) * inv, x a double."""
    t = (x - box_min) * inv
    if t >= 1048575.0:
        return 1048575
    if t > 0.0:
        return int(t)
    return 0


def q_of(x, box_min, invq):
    """Rule A4 on one axis -> (inside, Q)."""
    t = (x - box_min) * invq
    inside = t >= 0.0 and t < Q_SCALE
    return inside, int(t) if inside else 0


def invq_of(size):
    return Q_SCALE / float(size)


def lo_hi(p):
    return p & 0xFFFFFFFF, p >> 32


def stamp(b, num_b, inv_bits, min_bits, filled, totals=(0, 0, 0), magic=STAMP_MAGIC):
    return {"magic": magic, "filled": filled, "b": b, "numB": num_b, "inv": inv_bits, "min": tuple(min_bits), "totals": tuple(totals)}


def stamp_serves(have, want):
    """Rule A7: the stamp found serves the call — the same array, count, inv and corner, and filled if the call reads the grid records."""
    same = have["magic"] == STAMP_MAGIC and all(have[k] == want[k] for k in ("b", "numB", "inv", "min"))
    return same and (have["filled"] == 1 or (have["filled"] == 0 and want["filled"] == 0))


def align_exact(a, b, box_min, size, radius, grid_radius, pose, max_candidates=0, count_only=False):
    """simlod_align_samples on `a` and `b` (abi.point_dtype), one sample at a time -> (records as abi.compare_record_dtype, the summary as an
    abi.align_summary_dtype record); the records are None for a count-only call and when the budget is exceeded.  box_min: three fp32
    values, size: the fp32 box size, radius and grid_radius: fp32 values, pose: 12 doubles."""
    mn = [float(np.float32(v)) for v in box_min]
    r, g = float(np.float32(radius)), float(np.float32(grid_radius))
    inv = cr.inv_of(g, float(np.float32(size)))
    invq = invq_of(float(np.float32(size)))
    rr = r * r
    T = [float(v) for v in np.asarray(pose, np.float64).reshape(-1)]
    pa, pb = cr._xyz(a), cr._xyz(b)
    out = np.zeros((), dtype=abi.align_summary_dtype)
    cells, valid_b = {}, []
    for j, s in enumerate(pb):
        if cr.is_valid(*s):
            valid_b.append(j)
            c = tuple(cell_of(s[k], mn[k], inv) for k in range(3))
            cells[c] = cells.get(c, 0) + 1
    out["numInvalidB"] = len(pb) - len(valid_b)
    out["numCells"], out["maxCellPopulation"] = len(cells), max(cells.values()) if cells else 0
    centres, candidates, invalid_a = [], 0, 0
    for p in pa:
        cp, ok = posed(T, p)
        centres.append(cp if ok else None)
        if not ok:
            invalid_a += 1
            continue
        c = [cell_of(cp[k], mn[k], inv) for k in range(3)]
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    n = (c[0] + dx, c[1] + dy, c[2] + dz)
                    if min(n) >= 0 and max(n) < CELLS:
                        candidates += cells.get(n, 0)
    out["numInvalidA"], out["numCandidates"] = invalid_a, candidates
    if max_candidates != 0 and candidates > max_candidates:
        out["error"] = abi.ALIGN_ERR_BUDGET
    if count_only or int(out["error"]) != 0:
        return None, out
    rec = np.zeros(len(pa), dtype=abi.compare_record_dtype)
    matched = within_sum = summed = outside = 0
    max_d2 = 0.0
    sum_a, sum_b = [0, 0, 0], [0, 0, 0]
    cross_lo, cross_hi, sq_lo, sq_hi = [0] * 9, [0] * 9, 0, 0
    for i, cp in enumerate(centres):
        best, nearest, within = math.inf, MISS, 0
        if cp is not None:
            for j in valid_b:                                               # (ascending: of equal d2 the lowest index stays)
                d2 = cr.d2_of(pb[j], cp)
                if d2 <= rr:
                    within += 1
                    if d2 < best:
                        best, nearest = d2, j
        rec[i] = (best, nearest, within)
        if not within:
            continue
        matched += 1
        within_sum += within
        max_d2 = max(max_d2, best)
        qa = [q_of(cp[k], mn[k], invq) for k in range(3)]
        qb = [q_of(pb[nearest][k], mn[k], invq) for k in range(3)]
        if not all(v[0] for v in qa + qb):
            outside += 1
            continue
        summed += 1
        for k in range(3):
            sum_a[k] += qa[k][1]
            sum_b[k] += qb[k][1]
            for l in range(3):
                lo, hi = lo_hi(qa[k][1] * qb[l][1])
                cross_lo[3 * k + l] += lo
                cross_hi[3 * k + l] += hi
        e = [qb[k][1] - qa[k][1] for k in range(3)]
        lo, hi = lo_hi((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        sq_lo += lo
        sq_hi += hi
    out["numMatched"], out["numWithin"], out["maxD2"] = matched, within_sum, max_d2
    out["numSummed"], out["numOutside"], out["sumA"], out["sumB"] = summed, outside, sum_a, sum_b
    out["crossLo"], out["crossHi"], out["sqLo"], out["sqHi"] = cross_lo, cross_hi, sq_lo, sq_hi
    return rec, out


# ---- poses ------------------------------------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    """Rodrigues' rotation matrix about `axis` (normalised here), float64."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def motion(axis, degrees, through, shift):
    """The 3x4 pose: a rotation about `axis` through the point `through`, then a shift."""
    R, c = rotation(axis, degrees), np.asarray(through, np.float64)
    return np.hstack([R, (c - R @ c + np.asarray(shift, np.float64)).reshape(3, 1)])


def inverse(pose):
    R, t = pose[:, :3], pose[:, 3]
    return np.hstack([R.T, (-R.T @ t).reshape(3, 1)])


def moved(points, pose):
    """abi.point_dtype samples moved by a pose in float64 and rounded to fp32 (how a test makes the cloud a pose will bring back)."""
    xyz = np.stack([points["x"], points["y"], points["z"]], -1).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        out = cr.points(xyz @ pose[:, :3].T + pose[:, 3])
    out["color"] = points["color"]
    return out


# ---- the cases: name -> (a, b, box_min, box_max, radius, grid_radius, pose as a 3x4 array) ----------------------------------------------------
GENERAL = motion((0.3, -0.2, 1.0), 7.0, (2.0, 2.0, 2.0), (0.11, -0.07, 0.05))
ROT90 = np.array([[0.0, -1.0, 0.0, 2.5], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])     # the lattice of spacing 0.5 onto itself, exactly
EDGE_TX = 8.0 - 2.0 ** -49                                                   # 8 + EDGE_TX is one fp64 step below 16


def _under(name, pose, take_a=None, take_b=None):
    """A compare case with its `a` moved by the inverse of `pose` (rounded to fp32), so that the pose brings it back to where it was, nearly."""
    a, b, mn, mx, radius = cr.case(name)
    a, b = a[:take_a], b[:take_b]
    return moved(a, inverse(pose)), b, mn, mx, radius, radius, pose


def case(name):
    rs = np.random.RandomState(29)
    unit = ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    if name == "identity":
        b = cr.points(rs.rand(300, 3) * 4.0)
        a = cr.points(np.stack([b["x"], b["y"], b["z"]], -1)[::2].astype(np.float64) + (rs.rand(150, 3) - 0.5) * 0.2)
        return a, b, *unit, 0.3, 0.3, eye
    if name == "rot90_lattice":             # exact arithmetic: c' is a lattice point, d2 == rr passes, six equidistant neighbours tie
        p = cr.points(cr.lattice())
        return p, p.copy(), *unit, 0.5, 0.5, ROT90
    if name == "general":
        b = cr.points(0.5 + rs.rand(300, 3) * 3.0)
        a = moved(cr.points(np.stack([b["x"], b["y"], b["z"]], -1)[:200].astype(np.float64) + (rs.rand(200, 3) - 0.5) * 0.1), inverse(GENERAL))
        return a, b, *unit, 0.25, 0.25, GENERAL
    if name == "small_radius":              # radius < gridRadius: the grid is coarser than the test needs
        a, b, mn, mx, _, _, pose = case("general")
        return a, b, mn, mx, 0.1, 0.4, pose
    if name == "radius_0":                  # coincident samples only, under an exact pose; the grid at gridRadius
        p = cr.points(cr.lattice())
        return p, p.copy(), *unit, 0.0, 0.5, ROT90
    if name == "overflow":                  # 1e308 * 1e38 overflows: those samples of a are invalid; 1e308 * 0 is 0
        b = cr.points(np.concatenate([rs.rand(120, 2) * 4.0, np.zeros((120, 1))], -1))
        a = cr.points(np.concatenate([rs.rand(80, 2) * 4.0, np.zeros((80, 1))], -1))
        a["z"][::7] = np.float32(1e38)
        a["z"][3] = np.float32(-1e38)
        pose = eye.copy()
        pose[0, 2] = 1e308
        return a, b, *unit, 0.4, 0.4, pose
    if name == "edges":                     # Q at its edges: c' at min (inside), at min + size (outside) and one fp64 step below it (inside)
        big = ((0.0, 0.0, 0.0), (16.0, 16.0, 16.0))
        under16 = float(np.nextafter(np.float32(16.0), np.float32(0.0)))
        a = cr.points([[8.0, 0.0, 5.0], [8.0, 16.0, 5.0], [8.0, 3.0, 5.0], [2.0, 3.0, 5.0], [8.0, 3.0, 0.0], [8.0, 3.0, 16.0], [8.0, 7.0, 7.0]])
        b = cr.points([[16.0, 0.0, 5.0], [under16, 0.0, 5.0], [under16, 16.0, 5.0], [under16, under16, 5.0], [16.0, 3.0, 5.0], [15.9, 3.0, 5.0],
                       [10.0, 3.0, 5.0], [under16, 3.0, 0.0], [under16, 3.0, -0.01], [under16, 3.0, 16.0], [under16, 3.0, under16], [15.99, 7.0, 7.0]])
        pose = eye.copy()
        pose[0, 3] = EDGE_TX
        return a, b, *big, 0.05, 0.05, pose
    if name == "outside_pairs":             # c' outside with s inside, and the reverse: both count in numOutside
        a = cr.points([[4.2, 1.0, 1.0], [3.8, 2.0, 1.0], [1.0, -0.2, 1.0], [1.0, 0.2, 2.0], [2.0, 2.0, 2.0], [2.0, 2.0, 4.3]])
        b = cr.points([[3.8, 1.0, 1.0], [4.2, 2.0, 1.0], [1.0, 0.2, 1.0], [1.0, -0.2, 2.0], [2.1, 2.0, 2.0], [2.0, 2.0, 4.4]])
        return a, b, *unit, 0.5, 0.5, eye
    if name == "hot_cell":
        return _under("hot_cell", motion((0.0, 0.0, 1.0), 2.0, (1.3, 1.3, 1.3), (0.01, 0.0, -0.01)), 120, 300)
    if name == "cell_faces":                # a pure shift by a power of two: a - 0.25 and (a - 0.25) + 0.25 are exact, c' stays ON the faces
        pose = eye.copy()
        pose[0, 3] = 0.25
        return _under("cell_faces", pose)
    if name == "invalid":
        return _under("invalid", motion((1.0, 1.0, 0.0), 1.0, (102.0, -48.0, 9.0), (0.02, 0.01, 0.0)))
    if name == "b_outside":
        return _under("b_outside", motion((0.0, 1.0, 0.2), 3.0, (2.0, 2.0, 2.0), (0.0, 0.05, 0.0)))
    if name == "two_pairs":                 # fewer than 3 pairs: sums, but nothing to solve
        return cr.points([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [3.5, 3.5, 3.5]]), cr.points([[1.1, 1.0, 1.0], [2.0, 1.1, 1.0]]), *unit, 0.3, 0.3, eye
    raise KeyError(name)


CASES = ["identity", "rot90_lattice", "general", "small_radius", "radius_0", "overflow", "edges", "outside_pairs", "hot_cell", "cell_faces", "invalid",
         "b_outside", "two_pairs"]


def exact(name, max_candidates=0, count_only=False):
    a, b, mn, mx, radius, grid, pose = case(name)
    size = float((np.asarray(mx, np.float32) - np.asarray(mn, np.float32)).max())
    return align_exact(a, b, mn, size, radius, grid, pose, max_candidates, count_only)


# ---- the registration scene: B a smooth height field, A every third sample moved away -------------------------------------------------------
SCENE_BOX = ((0.0, 0.0, 0.0), (16.0, 16.0, 16.0))
SCENE_RADIUS = 0.25
SCENE_STEPS = 12
SCENE_BOUND = 4e-6                                                           # four fp32 steps at 8 (9.5e-7 each): the rounding of A itself


def scene():
    """-> (a, b, original): b 6 000 samples of a height field with coordinates in [1, 9]; original = b[::3]; a = original moved by the
    inverse of a rotation of 3 degrees about (0.2, -0.1, 1) through (5, 5, 2) plus (0.08, -0.05, 0.04), rounded to fp32."""
    rs = np.random.RandomState(5)
    xy = 1.0 + rs.rand(6000, 2) * 8.0
    z = 5.0 + 2.0 * np.sin(1.1 * xy[:, 0]) * np.cos(0.9 * xy[:, 1]) + 1.0 * np.sin(0.5 * xy[:, 0] + 0.8 * xy[:, 1])   # relief in every direction: nothing slides
    b = cr.points(np.concatenate([xy, z.reshape(-1, 1)], -1))
    assert 1.0 <= min(b["x"].min(), b["y"].min(), b["z"].min()) and max(b["x"].max(), b["y"].max(), b["z"].max()) <= 9.0
    original = b[::3].copy()
    truth = motion((0.2, -0.1, 1.0), 3.0, (5.0, 5.0, 2.0), (0.08, -0.05, 0.04))
    return moved(original, inverse(truth)), b, original
