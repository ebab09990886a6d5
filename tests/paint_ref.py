"""Shared by the paint tests: rules E0-E4 of "paint regions" (include/simlod_hip.h) restated one sample at a time in plain Python — integers for the
colours, Python floats (IEEE fp64, one rounding per operation, no fused multiply-add) where the header prescribes fp64 arithmetic, and
fractions.Fraction where a rounding is to be checked.  Nothing here uses octree_io's vectorised mirror, and nothing classifies a node: by region
rule 4 and footprint rule F5 the samples a query returns are, for samples of the contract, those that pass the per-sample test, in the order
of the full export."""
from fractions import Fraction

import numpy as np

from simlod_amd import abi

SET, BLEND, RAMP, ARRAY = 0, 1, 2, 3


def blend_byte(c, t, a):
    """Rule E2 for one byte, in integers."""
    return (c * (256 - a) + t * a + 128) >> 8


def blend_byte_rounded(c, t, a):
    """The same byte as a rounding: c + (t - c) * a / 256 rounded to the nearest integer, a tie upwards."""
    x = Fraction(c * (256 - a) + t * a, 256) + Fraction(1, 2)
    return x.numerator // x.denominator


def blend(word, color, a):
    out = word & 0xFF000000
    for sh in (0, 8, 16):
        out |= blend_byte((word >> sh) & 0xFF, (color >> sh) & 0xFF, a) << sh
    return out


def ramp_index_of_t(t):
    """Rule E3's index of the fp64 value t."""
    if t >= 255.0:
        return 255
    if t > 0.0:
        return int(t)
    return 0                                  # (a NaN fails both comparisons)


def ramp_t(z, z0, scale):
    """t of rule E3 from three fp32 values given as Python floats: two fp64 operations."""
    return (float(z) - float(z0)) * float(scale)


def ramp_index(z, z0, scale):
    return ramp_index_of_t(ramp_t(z, z0, scale))


def new_colour(mode, word, z, color=0, strength=0, z0=0.0, scale=0.0, table=None, from_array=None):
    if mode == SET:
        return color
    if mode == BLEND:
        return blend(word, color, strength)
    if mode == RAMP:
        return int(table[ramp_index(z, z0, scale)])
    return int(from_array)


def targets(samples, planes, footprint=None):
    """Rule E0 by the per-sample tests alone: the indices of the samples (abi.point_dtype, in the full export's order) that pass region rule 3
    for every plane and, with a footprint, rule F1 — each sample on its own, in Python floats in the header's operation order."""
    pl = [tuple(float(v) for v in np.asarray(p, np.float32)) for p in np.asarray(planes, np.float32).reshape(-1, 4)]
    xs, ys, zs = (samples[a].astype(np.float64).tolist() for a in ("x", "y", "z"))
    edges = None
    if footprint is not None:
        au, av = [float(v) for v in footprint.axis_u], [float(v) for v in footprint.axis_v]
        vs = [(float(a), float(b)) for a, b in footprint.vertices]
        n = len(vs)
        edges = [(vs[i][0], vs[i][1], vs[(i + 1) % n][1], vs[(i + 1) % n][0] - vs[i][0], vs[(i + 1) % n][1] - vs[i][1]) for i in range(n)]
    out = []
    for j, (x, y, z) in enumerate(zip(xs, ys, zs)):
        ok = True
        for nx, ny, nz, d in pl:
            if not ((nx * x + ny * y) + nz * z) + d >= 0.0:
                ok = False
                break
        if ok and edges is not None:
            u = ((au[0] * x + au[1] * y) + au[2] * z) + au[3]
            v = ((av[0] * x + av[1] * y) + av[2] * z) + av[3]
            odd = False
            for a_u, a_v, b_v, du, dv in edges:
                if (a_v > v) != (b_v > v):
                    c = du * (v - a_v) - dv * (u - a_u)
                    if (c > 0.0) == (dv > 0.0):
                        odd = not odd
            ok = odd
        if ok:
            out.append(j)
    return out


def paint(samples, idx, rec, colors=None):
    """Rules E1-E4 on the target samples `idx` (from `targets`) of `samples` with the SimlodPaint record `rec` (abi.paint_dtype):
    -> (the colour column after the call as a uint32 array, the previous colours of the targets in order as a list)."""
    r = np.asarray(rec).reshape(-1)[0]
    mode, color, strength = int(r["mode"]), int(r["color"]), int(r["strength"])
    z0, scale, table = float(r["z0"]), float(r["scale"]), [int(v) for v in r["table"]]
    col = [int(v) for v in samples["color"]]
    zs = samples["z"].astype(np.float64).tolist()
    previous = []
    for j, i in enumerate(idx):
        previous.append(col[i])
        col[i] = new_colour(mode, col[i], zs[i], color, strength, z0, scale, table, None if colors is None else colors[j])
    return np.asarray(col, dtype=np.uint32), previous


def in_contract(samples, box_min, box_max):
    """Are all samples finite and in the half-open box (region rule 4)?  Only then is `targets` the query's result."""
    mn = np.asarray(box_min, np.float32)
    size = np.float64((np.asarray(box_max, np.float32) - mn).max())
    ok = np.ones(len(samples), bool)
    for k, a in enumerate(("x", "y", "z")):
        v = samples[a].astype(np.float64)
        ok &= np.isfinite(v) & (v >= np.float64(mn[k])) & (v < np.float64(mn[k]) + size)
    return bool(ok.all())


def ramp_table(seed=5):
    """A 256-word table without repeats and without the words the golden inputs carry in their high byte."""
    rs = np.random.RandomState(seed)
    return (rs.permutation(1 << 16)[:256].astype(np.uint32) << np.uint32(8)) | np.uint32(0x5A000000) | np.arange(256, dtype=np.uint32)



def paints(box, box_min=(0, 0, 0)):
    """The paints the tests use, by name, for a box: one per mode (ARRAY takes its colours from the caller)."""
    from simlod_amd.octree_io import Paint
    z0 = float(box_min[2]) + 0.1 * float(box[2])
    z1 = float(box_min[2]) + 0.8 * float(box[2])
    return {"set": Paint.set(0xFF00C8FA), "blend": Paint.blend(0x0010F020, 77), "ramp": Paint.ramp(z0, z1, ramp_table()), "array": Paint.array()}


assert (SET, BLEND, RAMP, ARRAY) == (abi.PAINT_SET, abi.PAINT_BLEND, abi.PAINT_RAMP, abi.PAINT_ARRAY)
