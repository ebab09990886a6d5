"""What the packed-sample tests share (include/simlod_hip.h, "packed samples"): rules K1-K4 and K8 restated one record at a time with Python
floats (IEEE double) and numpy.float32 scalars — independent of octree_io's vectorised mirror —, hand-made tables whose entries sit on the piece
and wave boundaries of the kernels, and the samples that go with them, trouble included."""
import math
import struct

import numpy as np

from simlod_amd import abi

COUNTS = (0, 1, 255, 256, 999, 1000, 1001, 2049)        # per entry: nothing, one lane, a wave boundary, a piece boundary, three pieces
F32 = np.float32


def bits(f):
    return struct.unpack("<I", struct.pack("<f", float(f)))[0]


def box_of(box_min, box_max):
    mn = [F32(v) for v in box_min]
    size = max(F32(b) - a for a, b in zip(mn, box_max))
    return mn, F32(size)


def exp2f(level):
    return F32(struct.unpack("<f", struct.pack("<I", (127 + level) << 23))[0])


def voxel_centre(mn, size, level, A, c):
    """simlod_device.hpp voxel_centre for one axis, operation by operation in fp32"""
    node = F32(size / exp2f(level))
    nmin = F32(F32(F32(A) + F32(0.0)) * node) + mn
    return F32(nmin + F32(F32(node * F32(F32(c) + F32(0.5))) / F32(128.0)))


def frame(mn, size, level, A):
    ns = math.ldexp(float(size), -level)                       # rule K1
    return ns, [float(mn[a]) + float(A[a]) * ns for a in range(3)]


def quantize(t, lim):
    if t >= 0.0:
        return int(t) if t < lim else lim - 1
    return 0                                                    # negative or a NaN


def pack_one(mn, size, entry, p):
    """One record by rules K0, K2, K4 -> (word, clamped, inexact, alpha)"""
    level, A = int(entry["level"]), (int(entry["X"]), int(entry["Y"]), int(entry["Z"]))
    leaf = bool(entry["flags"] & abi.EXPORT_FLAG_LEAF)
    lim = 8192 if leaf else 128
    ns, nmin = frame(mn, size, level, A)
    k = float(lim) / ns
    word, clamped, inexact = int(p["color"]) & 0xFFFFFF, False, False
    for a, (name, shift) in enumerate((("x", 24), ("y", 37), ("z", 50))):
        t = (float(p[name]) - nmin[a]) * k
        clamped |= not (t >= 0.0 and t < lim)
        q = quantize(t, lim)
        word |= q << shift
        if not leaf:
            inexact |= bits(voxel_centre(mn[a], size, level, A[a], q)) != bits(p[name])
    return word, clamped, inexact, (int(p["color"]) >> 24) != 0xFF


def unpack_one(mn, size, entry, word):
    """One sample by rules K3, K4, K8 -> (x, y, z as float32, colour)"""
    level, A = int(entry["level"]), (int(entry["X"]), int(entry["Y"]), int(entry["Z"]))
    leaf = bool(entry["flags"] & abi.EXPORT_FLAG_LEAF)
    ns, nmin = frame(mn, size, level, A)
    out = []
    for a, shift in enumerate((24, 37, 50)):
        q = (word >> shift) & (0x1FFF if leaf else 0x7F)
        out.append(F32(nmin[a] + (float(q) + 0.5) * (ns / 8192.0)) if leaf else voxel_centre(mn[a], size, level, A[a], q))
    return out[0], out[1], out[2], 0xFF000000 | (word & 0xFFFFFF)


def ranges(table, entries=None):
    """rule K5: (t, first, n) per touched entry"""
    out = []
    for t in range(len(table)):
        if entries is None:
            if table["flags"][t] & abi.EXPORT_FLAG_SELECTED and table["numSamples"][t]:
                out.append((t, int(table["firstSample"][t]), int(table["numSamples"][t])))
        elif entries["state"][t] != abi.DELTA_NONE and entries["numDelta"][t]:
            out.append((t, int(entries["firstDelta"][t]), int(entries["numDelta"][t])))
    return out


def pack_ref(table, samples, box_min, box_max, entries=None, pick=None):
    """Record by record: {sample index: (word, clamped, inexact, alpha)} for the covered indices (`pick`: only those)."""
    mn, size = box_of(box_min, box_max)
    out = {}
    for t, first, n in ranges(table, entries):
        for i in range(first, first + n):
            if pick is None or i in pick:
                out[i] = pack_one(mn, size, table[t], samples[i])
    return out


def unpack_ref(table, packed, box_min, box_max, entries=None, pick=None):
    mn, size = box_of(box_min, box_max)
    out = {}
    for t, first, n in ranges(table, entries):
        for i in range(first, first + n):
            if pick is None or i in pick:
                out[i] = unpack_one(mn, size, table[t], int(packed[i]))
    return out


def entry_of_sample(table, entries=None):
    """(index of the table entry per covered sample index) as a dict of ranges -> arrays: idx (sample indices), ent (their entries)"""
    r = ranges(table, entries)
    idx = np.concatenate([np.arange(f, f + n) for _, f, n in r]) if r else np.zeros(0, np.int64)
    ent = np.concatenate([np.full(n, t) for t, _, n in r]) if r else np.zeros(0, np.int64)
    return idx, ent


# ---- hand-made tables ------------------------------------------------------------------------------------------------------------------------
def hand_table(counts, levels, leaf_flags):
    """A valid breadth-first table (octree_io.validate_table passes) with one SELECTED entry per (count, level, leaf flag), in the order given
    (levels ascending; at most one at level 0 and eight per level).  Per level the requested entries are siblings, children of the first entry
    of the level above; a level nobody asked for has one entry that is not selected, so the chain reaches the deepest level."""
    assert list(levels) == sorted(levels) and len(counts) == len(levels) == len(leaf_flags)
    rows = []                                  # (level, X, Y, Z, parent, count or None, leaf)
    parent = abi.EXPORT_NONE
    px = (0, 0, 0)
    for level in range(max(levels) + 1):
        want = [(c, f) for c, lv, f in zip(counts, levels, leaf_flags) if lv == level] or [(None, False)]
        assert len(want) <= (8 if level else 1)
        start = min((3 * level + 1) % 8, 8 - len(want)) if level else 0
        first_row = len(rows)
        for j, (c, f) in enumerate(want):
            o = start + j
            xyz = (px[0] * 2 + (o >> 2 & 1), px[1] * 2 + (o >> 1 & 1), px[2] * 2 + (o & 1)) if level else (0, 0, 0)
            rows.append((level, xyz, parent, c, f, o))
        parent, px = first_row, rows[first_row][1]
    t = np.zeros(len(rows), dtype=abi.export_node_dtype)
    t["firstChild"] = abi.EXPORT_NONE
    for i, (level, xyz, par, c, f, o) in enumerate(rows):
        t["level"][i], (t["X"][i], t["Y"][i], t["Z"][i]), t["parent"][i] = level, xyz, par
        t["flags"][i] = (abi.EXPORT_FLAG_LEAF if f else 0) | (abi.EXPORT_FLAG_SELECTED if c is not None else 0)
        t["numSamples"][i] = c or 0
        if par != abi.EXPORT_NONE:
            t["childMask"][par] |= 1 << o
            t["firstChild"][par] = min(int(t["firstChild"][par]), i)
    ns = t["numSamples"].astype(np.uint64)
    t["firstSample"] = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.uint64)
    return t


# the suite's hand table: leaf and voxel entries at levels 0, 1, 7, 13, 19 and 20, every count of COUNTS as a leaf and as a voxel entry
HAND_SPEC = [(1001, 0, False),
             (0, 1, True), (1, 1, False), (255, 1, True), (2049, 1, False), (2049, 1, True), (2049, 1, False), (2049, 1, True), (2049, 1, True),
             (256, 7, False), (999, 7, True), (1000, 7, False), (1001, 7, True), (2049, 7, True), (2049, 7, False), (2049, 7, True), (2049, 7, False),
             (0, 13, False), (1, 13, True), (255, 13, False), (256, 13, True), (1000, 13, True),
             (999, 19, False), (2049, 19, False), (1000, 19, True), (256, 19, True),
             (1001, 20, True), (255, 20, True), (1, 20, True), (2049, 20, True)]


def num_pieces(table, entries=None):
    """the pieces of at most 1 000 samples the ranges fall into: the scratch items a call needs"""
    return sum((n + 999) // 1000 for _, _, n in ranges(table, entries))


def the_hand_table():
    c, lv, f = zip(*HAND_SPEC)
    return hand_table(c, lv, f)


TROUBLE = ("nan", "+inf", "-inf", "max face", "below min", "off centre", "alpha 0", "alpha 7f")


def hand_samples(table, box_min, box_max, seed=17):
    """Samples for a hand table in the box: seeded points inside each leaf entry's cube (as fp32 allows), true voxel_centre positions for the
    voxel entries, alpha 0xff — then the trouble of TROUBLE, one sample each, put into the entries that are big enough:
    -> (samples, {trouble: sample index})."""
    mn, size = box_of(box_min, box_max)
    rs = np.random.RandomState(seed)
    smp = np.zeros(int(table["numSamples"].astype(np.int64).sum()), dtype=abi.point_dtype)
    where = {}
    leaves, voxels = [], []
    for t, first, n in ranges(table):
        e = table[t]
        level, A = int(e["level"]), (int(e["X"]), int(e["Y"]), int(e["Z"]))
        ns, nmin = frame(mn, size, level, A)
        s = smp[first: first + n]
        s["color"] = 0xFF000000 | rs.randint(0, 1 << 24, n).astype(np.uint32)
        if e["flags"] & abi.EXPORT_FLAG_LEAF:
            for a, name in enumerate("xyz"):
                s[name] = (nmin[a] + rs.random_sample(n) * ns).astype(np.float32)
            leaves.append((t, first, n))
        else:
            cells = rs.randint(0, 128, (n, 3))
            for a, name in enumerate("xyz"):
                s[name] = [voxel_centre(mn[a], size, level, A[a], int(c)) for c in cells[:, a]]
            voxels.append((t, first, n))
    big_leaf = max(leaves, key=lambda r: (r[2], -int(table["level"][r[0]])))       # the shallowest of the largest: fp32 resolves its cube
    t, first, n = big_leaf
    ns, nmin = frame(mn, size, int(table["level"][t]), (int(table["X"][t]), int(table["Y"][t]), int(table["Z"][t])))
    for j, what in enumerate(TROUBLE[:5]):
        i = first + 3 + 7 * j
        where[what] = i
        if what == "nan":
            smp["y"][i] = np.nan
        elif what == "+inf":
            smp["x"][i] = np.inf
        elif what == "-inf":
            smp["z"][i] = -np.inf
        elif what == "max face":
            smp["x"][i] = F32(nmin[0] + ns)
        else:
            smp["y"][i] = np.nextafter(F32(nmin[1]), F32(-np.inf))
    t, first, n = max(voxels, key=lambda r: (r[2], -int(table["level"][r[0]])))
    i = first + 5
    where["off centre"] = i
    smp["z"][i] = np.nextafter(smp["z"][i], F32(np.inf))
    where["alpha 0"], where["alpha 7f"] = first + 9, leaves[0][1]
    smp["color"][where["alpha 0"]] &= 0x00FFFFFF
    smp["color"][where["alpha 7f"]] = (smp["color"][where["alpha 7f"]] & 0x00FFFFFF) | 0x7F000000
    return smp, where


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def assert_points_within_bound(table, before, after, box_min, box_max, clamped_ok=None, entries=None, what=""):
    """Rule K8 for every leaf entry's unclamped points: |p' - p| <= ns / 16384 + ulp32(p') / 2 + ns * 2^-40 per axis.  Unclamped is decided here,
    from rule K2 in float64 per sample (vectorised per entry).  Returns (points checked, the worst ratio to the bound)."""
    mn, size = box_of(box_min, box_max)
    checked, worst = 0, 0.0
    for t, first, n in ranges(table, entries):
        e = table[t]
        if not e["flags"] & abi.EXPORT_FLAG_LEAF:
            continue
        ns, nmin = frame(mn, size, int(e["level"]), (int(e["X"]), int(e["Y"]), int(e["Z"])))
        k = 8192.0 / ns
        b, a = before[first: first + n], after[first: first + n]
        with np.errstate(invalid="ignore", over="ignore"):
            tt = np.stack([(b[nm].astype(np.float64) - nmin[ax]) * k for ax, nm in enumerate("xyz")])
            ok = ((tt >= 0) & (tt < 8192)).all(axis=0)
            for ax, nm in enumerate("xyz"):
                err = np.abs(a[nm].astype(np.float64) - b[nm].astype(np.float64))[ok]
                bound = ns / 16384.0 + ulp32(a[nm][ok]) / 2 + ns * 2.0 ** -40
                assert (err <= bound).all(), f"{what}: entry {t} axis {nm}: {int((err > bound).sum())} points beyond rule K8's bound"
                if len(err):
                    worst = max(worst, float((err / bound).max()))
        checked += int(ok.sum())
    return checked, worst


def voxel_mask(table, num_samples, entries=None):
    """True for the sample indices that belong to voxel entries"""
    m = np.zeros(num_samples, bool)
    for t, first, n in ranges(table, entries):
        if not table["flags"][t] & abi.EXPORT_FLAG_LEAF:
            m[first: first + n] = True
    return m
