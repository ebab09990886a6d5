"""Shared by the compare tests: rules C1-C5 of "compare queries" (include/simlod_hip.h) restated one sample at a time in plain Python — a brute
force over ALL of b for every sample of a, with no grid; Python floats (IEEE fp64, one rounding per operation, `a*a + b*b` fuses nothing) where
the header prescribes fp64 arithmetic, integers for everything else.  The grid's fields (numCells, maxCellPopulation, numCandidates) come from
a dictionary of cells.  Nothing here uses octree_io's vectorised mirror or numpy arithmetic (numpy only hands over the fields and takes the
result), and the cell is summary_ref's restatement of rule S2, as rule C4 says."""
import math
import struct

import numpy as np

import summary_ref as sr
from simlod_amd import abi

MISS = 0xFFFFFFFF
HASH_MUL = 0x9E3779B97F4A7C15
CELLS = 1 << 20
MAX_COUNT = (1 << 32) - 2


def f32(x):
    """x rounded to fp32, as a Python float (an overflow becomes an infinity)."""
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def params_acceptable(radius, thresholds2, reserved=0):
    """The refusals of the record: a radius (as fp32) that is not finite or < 0, thresholds that are not 255 finite ascending values, a
    nonzero reserved word."""
    r = f32(radius) if not math.isnan(radius) else radius
    if not math.isfinite(r) or not r >= 0.0 or reserved != 0:
        return False
    t = [float(v) for v in thresholds2]
    return len(t) == 255 and all(math.isfinite(v) for v in t) and all(t[i] >= t[i - 1] for i in range(1, 255))


def h_of(radius, size):
    """Rule C4: h = max((double)r * (1 + 2^-10), (double)size * 2^-20)."""
    return max(float(radius) * (1.0 + 2.0 ** -10), float(size) * 2.0 ** -20)


def inv_of(radius, size):
    return 1.0 / h_of(radius, size)


def is_valid(x, y, z):
    """Rule C1."""
    return math.isfinite(x) and math.isfinite(y) and math.isfinite(z)


def cell_of(p, box_min, inv):
    """Rule C4: the three 20-bit cells of a valid sample."""
    return tuple(sr.cell20(p[k], box_min[k], inv) for k in range(3))


def key_of(cell):
    return cell[0] | cell[1] << 20 | cell[2] << 40


def table_slots(num_b):
    """simlod_compare_table_slots: the smallest power of two >= 2 * numB; 0 for a count the call refuses."""
    if not 0 < num_b <= MAX_COUNT:
        return 0
    s = 2
    while s < 2 * num_b:
        s *= 2
    return s


def home_of(key, slots):
    """The slot a key's probing starts at: the top log2(slots) bits of the key's product with the odd constant, modulo 2^64."""
    log2 = slots.bit_length() - 1
    return ((key * HASH_MUL) & 0xFFFFFFFFFFFFFFFF) >> (64 - log2)


def index_of(thresholds2, d2):
    """Rule C5: the number of entries that are <= d2 (counted one by one, no search)."""
    return sum(1 for t in thresholds2 if t <= d2)


def d2_of(s, c):
    """Rule C2: p = s - c per component, d2 = (px*px + py*py) + pz*pz."""
    px, py, pz = s[0] - c[0], s[1] - c[1], s[2] - c[2]
    return (px * px + py * py) + pz * pz


def _xyz(points):
    p = np.asarray(points, dtype=abi.point_dtype).reshape(-1)
    return list(zip(p["x"].astype(np.float64).tolist(), p["y"].astype(np.float64).tolist(), p["z"].astype(np.float64).tolist()))


def compare_exact(a, b, box_min, size, radius, thresholds2, table, miss_color, max_candidates=0, count_only=False):
    """simlod_compare_samples on `a` and `b` (abi.point_dtype), one sample at a time -> (records as abi.compare_record_dtype, colours as
    uint32, the summary as an abi.compare_summary_dtype record); records and colours are None for a count-only call and when the budget is
    exceeded.  box_min: three fp32 values, size: the fp32 box size, radius: an fp32 value."""
    mn = [float(np.float32(v)) for v in box_min]
    r = float(np.float32(radius))
    inv = inv_of(r, float(np.float32(size)))
    rr = r * r
    t2 = [float(v) for v in thresholds2]
    pa, pb = _xyz(a), _xyz(b)
    out = np.zeros((), dtype=abi.compare_summary_dtype)
    cells = {}
    valid_b = []
    for j, s in enumerate(pb):
        if is_valid(*s):
            valid_b.append(j)
            c = cell_of(s, mn, inv)
            cells[c] = cells.get(c, 0) + 1
    out["numInvalidB"] = len(pb) - len(valid_b)
    out["numCells"], out["maxCellPopulation"] = len(cells), max(cells.values()) if cells else 0
    candidates = invalid_a = 0
    for p in pa:
        if not is_valid(*p):
            invalid_a += 1
            continue
        c = cell_of(p, mn, inv)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    n = (c[0] + dx, c[1] + dy, c[2] + dz)
                    if min(n) >= 0 and max(n) < CELLS:
                        candidates += cells.get(n, 0)
    out["numInvalidA"], out["numCandidates"] = invalid_a, candidates
    if max_candidates != 0 and candidates > max_candidates:
        out["error"] = abi.COMPARE_ERR_BUDGET
    if count_only or int(out["error"]) != 0:
        return None, None, out
    rec = np.zeros(len(pa), dtype=abi.compare_record_dtype)
    colours = np.zeros(len(pa), np.uint32)
    hist = [0] * 257
    matched = within_sum = 0
    max_d2 = 0.0
    for i, p in enumerate(pa):
        best, nearest, within = math.inf, MISS, 0
        if is_valid(*p):
            for j in valid_b:                                               # (ascending: of equal d2 the lowest index stays)
                d2 = d2_of(pb[j], p)
                if d2 <= rr:
                    within += 1
                    if d2 < best:
                        best, nearest = d2, j
        rec[i] = (best, nearest, within)
        k = index_of(t2, best) if within else 256
        hist[k] += 1
        colours[i] = int(table[k]) if within else miss_color
        if within:
            matched += 1
            within_sum += within
            max_d2 = max(max_d2, best)
    out["numMatched"], out["numWithin"], out["maxD2"], out["hist"] = matched, within_sum, max_d2, hist
    return rec, colours, out


def points(xyz, color=None):
    """An abi.point_dtype array from an (n, 3) array of coordinates (rounded to fp32) and colours (default: the index)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    p = np.zeros(len(xyz), dtype=abi.point_dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["color"] = np.arange(len(xyz), dtype=np.uint32) if color is None else color
    return p


# ---- the inputs the io tier and the GPU tier share: name -> (a, b, box_min, box_max, radius) -------------------------------------------------
def _ulp(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


def lattice(n=6, spacing=0.5):
    g = np.arange(n) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def case(name):
    rs = np.random.RandomState(17)
    unit = ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    if name == "one_matched":
        return points([[1.0, 1.0, 1.0]]), points([[1.25, 1.0, 1.0]]), *unit, 0.5
    if name == "one_unmatched":
        return points([[1.0, 1.0, 1.0]]), points([[3.0, 1.0, 1.0]]), *unit, 0.5
    if name == "one_coincident_r0":
        return points([[1.0, 2.0, 3.0]]), points([[1.0, 2.0, 3.0]]), *unit, 0.0
    if name == "lattice":                   # exactly representable: d2 == rr passes, six equidistant neighbours tie
        p = points(lattice())
        return p, p.copy(), *unit, 0.5
    if name == "lattice_ulp":               # every a coordinate one fp32 ulp up or down
        b = points(lattice())
        a = b.copy()
        for k, ax in enumerate("xyz"):
            up = rs.randint(0, 2, len(a)).astype(bool)
            a[ax] = np.where(up, np.nextafter(b[ax], np.float32(np.inf)), np.nextafter(b[ax], np.float32(-np.inf)))
        return a, b, *unit, 0.5
    if name == "cell_faces":                # a at min + k*h (fp32) and its ulp neighbours, b at distance r on the far side of the face
        r = np.float32(0.3)
        h = h_of(float(r), 4.0)
        xs = []
        for k in (1, 2, 5, 9):
            v = np.float32(k * h)
            xs += [float(_ulp(v, False)), float(v), float(_ulp(v, True))]
        a = points([[x, 1.0, 1.0] for x in xs] + [[1.0, x, 1.0] for x in xs] + [[1.0, 1.0, x] for x in xs])
        fb = []
        for p in a:
            for k, ax in enumerate("xyz"):
                for sgn in (-1.0, 1.0):
                    q = [float(p["x"]), float(p["y"]), float(p["z"])]
                    q[k] = float(np.float32(q[k] + sgn * float(r)))
                    fb.append(q)
        return a, points(fb), *unit, float(r)
    if name == "hot_cell":                  # 3 000 b samples in one cell, 1 100 a samples around it
        r = 0.25
        h = h_of(float(np.float32(r)), 4.0)
        lo = 5 * h
        b = points(lo + rs.rand(3000, 3) * h * 0.98 + h * 0.01)
        a = points(lo + (rs.rand(1100, 3) * 3.4 - 1.2) * h)
        return a, b, *unit, r
    if name == "distinct_cells":            # 20 000 b samples in 20 000 distinct cells
        r = 0.01
        h = h_of(float(np.float32(r)), 4.0)
        idx = rs.permutation(60 * 60 * 60)[:20000]
        c = np.stack([idx % 60, idx // 60 % 60, idx // 3600], -1)
        b = points((c + 0.25 + 0.5 * rs.rand(20000, 3)) * h)
        a = points((rs.rand(300, 3) * 60) * h)
        return a, b, *unit, r
    if name == "invalid":                   # NaN and both infinities in a and in b, samples at +-1e30, a box off the origin
        mn, mx = (100.0, -50.0, 7.0), (104.0, -46.0, 11.0)
        base = np.array(mn) + rs.rand(200, 3) * 4.0
        a, b = points(base[:120]), points(base[60:])
        bad = [np.nan, np.inf, -np.inf]
        for k, v in enumerate(bad * 2):
            a["xyz"[k % 3]][k] = v
            b["zxy"[k % 3]][k + 3] = v
        a["x"][20], a["y"][21], b["x"][30], b["z"][31] = 1e30, -1e30, -1e30, 1e30
        a[22], a[23] = b[31], b[30]             # (coincident with the far samples: matched in the clamped edge cells)
        return a, b, mn, mx, 0.6
    if name == "b_outside":                 # b entirely outside a's box
        a = points(rs.rand(150, 3) * 4.0)
        b = points(rs.rand(150, 3) * 4.0 + np.array([4.5, 0.0, 0.0]))
        a["x"][:30] = np.float32(3.9)
        return a, b, *unit, 0.8
    if name == "r0_duplicates":             # radius 0: coincident samples only; of duplicates the lowest index wins
        base = rs.rand(80, 3) * 4.0
        b = points(np.concatenate([base, base[:40], base[:10]]))
        a = points(np.concatenate([base[::2], rs.rand(20, 3) * 4.0]))
        return a, b, *unit, 0.0
    if name == "h_floor":                   # a radius so small that h sits at size * 2^-20
        base = rs.rand(100, 3) * 4.0
        b = points(base)
        a = points(base + rs.randint(-1, 2, (100, 3)) * 1e-7)
        return a, b, *unit, 1e-7
    raise KeyError(name)


CASES = ["one_matched", "one_unmatched", "one_coincident_r0", "lattice", "lattice_ulp", "cell_faces", "hot_cell", "distinct_cells", "invalid", "b_outside",
         "r0_duplicates", "h_floor"]
# the brute force takes numA * numB steps: the two big cases are checked on a part of a only
EXACT_A_LIMIT = {"hot_cell": 120, "distinct_cells": 40}
