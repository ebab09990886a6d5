"""Shared by the summary tests: rules S1-S4 of "summary queries" (include/simlod_hip.h) restated one sample at a time in plain Python — integers
for the keys, the cells, the sums and the counts, `struct` for the bits of a float, Python floats (IEEE fp64, one rounding per operation, no
fused multiply-add) where the header prescribes fp64 arithmetic.  Nothing here uses octree_io's vectorised mirror or numpy arithmetic (numpy
only hands over the fields), and rule S3's index is written out from the header's text of rule E3, not imported."""
import struct

import numpy as np

from simlod_amd import abi

KEY_POS_INF, KEY_NEG_INF = 0xFF800000, 0x007FFFFF          # the keys of +inf and -inf: the extent of no sample
MOMENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # xx, yy, zz, xy, xz, yz


def bits_of(x):
    """The 32 bits of the fp32 value x (a Python float that is one)."""
    return struct.unpack("<I", struct.pack("<f", x))[0]


def float_of(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def key(bits):
    """Rule S1: k(bits) = bits ^ ((bits >> 31) ? 0xffffffff : 0x80000000)."""
    return bits ^ (0xFFFFFFFF if bits >> 31 else 0x80000000)


def unkey(k):
    return k ^ (0x80000000 if k >> 31 else 0xFFFFFFFF)


def is_nan(bits):
    return (bits & 0x7FFFFFFF) > 0x7F800000


def is_finite(bits):
    return (bits & 0x7F800000) != 0x7F800000


def inv_of(size):
    """Rule S2: inv = 1048576.0 / (double)size, one IEEE division."""
    return 1048576.0 / float(size)


def cell20(x, box_min, inv):
    """Rule S2: t = ((double)x - (double)boxMin) * inv; 1048575 if t >= 1048575.0, (uint32_t)t if t > 0.0, else 0 (a NaN gives 0)."""
    t = (float(x) - float(box_min)) * float(inv)
    if t >= 1048575.0:
        return 1048575
    if t > 0.0:
        return int(t)
    return 0


def z_index(z, z0, scale):
    """Rule E3 as the header words it: t = ((double)z - (double)z0) * (double)scale; i = 255 if t >= 255, (uint32_t)t if t > 0, else 0."""
    t = (float(z) - float(z0)) * float(scale)
    if t >= 255.0:
        return 255
    if t > 0.0:
        return int(t)
    return 0


def summarize_exact(samples, box_min, size, z0, scale):
    """SimlodSummary of `samples` (abi.point_dtype) as a record of abi.summary_dtype, one sample at a time.  box_min: three fp32 values,
    size: the fp32 box size, z0 / scale: fp32 values."""
    mn = [float(np.float32(v)) for v in box_min]
    inv = inv_of(float(np.float32(size)))
    z0, scale = float(np.float32(z0)), float(np.float32(scale))
    words = np.ascontiguousarray(samples).view(np.uint32).reshape(-1, 4).tolist()
    kmin, kmax = [KEY_POS_INF] * 3, [KEY_NEG_INF] * 3
    s1, s2 = [0] * 3, [0] * 6
    non_finite = 0
    hz, hc = [0] * 256, [[0] * 256 for _ in range(4)]
    for w in words:
        c16 = []
        finite = True
        for a in range(3):
            b = w[a]
            finite = finite and is_finite(b)
            if not is_nan(b):
                k = key(b)
                kmin[a], kmax[a] = min(kmin[a], k), max(kmax[a], k)
            c = cell20(float_of(b), mn[a], inv)
            s1[a] += c
            c16.append(c >> 4)
        for j, (a, b) in enumerate(MOMENTS):
            s2[j] += c16[a] * c16[b]
        non_finite += 0 if finite else 1
        hz[z_index(float_of(w[2]), z0, scale)] += 1
        for k in range(4):
            hc[k][(w[3] >> (8 * k)) & 255] += 1
    rec = np.zeros((), dtype=abi.summary_dtype)
    rec["numSamples"], rec["numNonFinite"] = len(words), non_finite
    rec["min"] = np.array([unkey(k) for k in kmin], np.uint32).view(np.float32)
    rec["max"] = np.array([unkey(k) for k in kmax], np.uint32).view(np.float32)
    rec["sum"], rec["sum2"], rec["histZ"], rec["histC"] = s1, s2, hz, hc
    return rec
