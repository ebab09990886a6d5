"""CPU tier of the align queries' shared rules (include/simlod_hip.h, "align queries"): simlod_amd/csrc/align_rules.hpp — which
SimlodAlignParams records a call accepts, rule A1's posed centre and validity, rule A2's cell of a double, rule A4's invQ, inside test and Q,
rule A5's lo/hi split and squared residual, rule A7's stamp and its comparison — checked on the host by a program of its own
(tests/host/align_rules_check.cpp, built by plain g++ with the address and undefined-behaviour sanitizers, run as a host binary with nothing
preloaded) against tests/align_ref.py, line by line; and hand tables."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import align_ref as ar
import compare_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAMP = np.dtype({"names": ["magic", "filled", "b", "numB", "inv", "min", "totals"], "formats": ["<u4", "<u4", "<u8", "<u8", "<u8", ("<u8", 3), ("<u8", 3)],
                  "offsets": [0, 4, 8, 16, 24, 32, 56], "itemsize": 80})


def _d64(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_hand_tables():
    """Rules A1, A2, A4, A5 and A7 by hand."""
    assert ar.posed(ar.IDENTITY, (1.5, -2.0, 3.0)) == ([1.5, -2.0, 3.0], True)                      # rule A10: the identity changes nothing
    assert ar.posed([0.0, -1.0, 0.0, 2.5, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0], (0.5, 1.0, 2.0)) == ([1.5, 0.5, 2.0], True)
    over = list(ar.IDENTITY)
    over[2] = 1e308
    assert ar.posed(over, (1.0, 1.0, 0.0)) == ([1.0, 1.0, 0.0], True) and not ar.posed(over, (1.0, 1.0, 1e38))[1]   # a product overflows
    assert not ar.posed(ar.IDENTITY, (math.nan, 0.0, 0.0))[1] and not ar.posed(ar.IDENTITY, (0.0, math.inf, 0.0))[1]
    invq = ar.invq_of(16.0)
    assert invq == 2.0 ** 20
    assert ar.q_of(0.0, 0.0, invq) == (True, 0) and ar.q_of(-0.0, 0.0, invq) == (True, 0) and ar.q_of(-5e-324, 0.0, invq) == (False, 0)
    assert ar.q_of(16.0, 0.0, invq) == (False, 0) and ar.q_of(float(np.nextafter(16.0, 0.0)), 0.0, invq) == (True, (1 << 24) - 1)
    assert ar.q_of(2.0 ** -20, 0.0, invq) == (True, 1) and ar.q_of(float(np.nextafter(2.0 ** -20, 0.0)), 0.0, invq) == (True, 0)
    assert ar.q_of(math.nan, 0.0, invq) == (False, 0) and ar.q_of(math.inf, 0.0, invq) == (False, 0)
    assert [ar.lo_hi(p) for p in (0, (1 << 32) - 1, 1 << 32, (1 << 48) - 1)] == [(0, 0), (0xFFFFFFFF, 0), (0, 1), (0xFFFFFFFF, 0xFFFF)]
    assert ar.cell_of(-1.0, 0.0, 4.0) == 0 and ar.cell_of(0.3, 0.0, 4.0) == 1 and ar.cell_of(1e30, 0.0, 4.0) == 1048575 and ar.cell_of(math.nan, 0.0, 4.0) == 0
    want = ar.stamp(0x7000, 10, 5, (1, 2, 3), 1)
    assert ar.stamp_serves(dict(want, totals=(7, 8, 9)), want) and ar.stamp_serves(want, dict(want, filled=0))
    assert not ar.stamp_serves(dict(want, filled=0), want) and ar.stamp_serves(dict(want, filled=0), dict(want, filled=0))
    for change in (dict(magic=0xA5A5A5A5), dict(b=0x7010), dict(numB=11), dict(inv=6), dict(min=(1, 2, 4)), dict(filled=0xA5A5A5A5)):
        assert not ar.stamp_serves(dict(want, **change), want), change


def _records():
    """(accepted records, refused records and what is wrong with each)"""
    bad_pose = lambda k, v: [v if i == k else x for i, x in enumerate(ar.IDENTITY)]
    good = [ar.params(0.5), ar.params(0.0, 0.0), ar.params(-0.0, 0.0), ar.params(0.0, 3.0e38), ar.params(0.25, 0.25, flags=3, budget=(1 << 64) - 1, wg=0xFFFFFFFF),
            ar.params(1.0, 2.0, pose=bad_pose(3, -1.7e308), flags=1), ar.params(1.0, 1.0, pose=np.zeros(12), flags=2)]
    bad = [(ar.params(-1.0, 1.0), "radius < 0"), (ar.params(np.nan, 1.0), "radius NaN"), (ar.params(np.inf, np.inf), "radius inf"),
           (ar.params(1.0, np.nextafter(np.float32(1.0), np.float32(0.0))), "gridRadius < radius"), (ar.params(1.0, np.nan), "gridRadius NaN"),
           (ar.params(1.0, np.inf), "gridRadius inf"), (ar.params(1.0, reserved=1), "reserved"), (ar.params(1.0, flags=4), "flag 4"),
           (ar.params(1.0, flags=0x80000001), "flag 2^31"), (ar.params(1.0, pose=bad_pose(0, np.nan)), "pose NaN"),
           (ar.params(1.0, pose=bad_pose(11, np.inf)), "pose inf"), (ar.params(1.0, pose=bad_pose(6, -np.inf)), "pose -inf")]
    return good, bad


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("align_rules") / "align_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "align_rules_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("scene", ["general", "edges", "overflow", "invalid"])
def test_header_agrees_with_the_reference(checker, tmp_path, scene):
    """Every line the host program prints equals align_ref's: the records accepted and refused; inv and invQ; c', its validity and its
    cells for every sample of a case under the case's pose; the cell, the inside test and Q of doubles at and around the box's two ends
    and whole steps of Q; the lo/hi split at 0, 2^32 - 1, 2^32, 2^48 - 1 and random products; E of random pairs and of the extremes; the
    stamp of a build call and which stamps serve which calls."""
    good, bad = _records()
    records = good + [r for r, _ in bad]
    a, b, mn, mx, radius, grid, pose = ar.case(scene)
    mn = [float(np.float32(v)) for v in mn]
    size = float((np.asarray(mx, np.float32) - np.asarray(mn, np.float32)).max())
    g32 = float(np.float32(grid))
    inv, invq = cr.inv_of(g32, size), ar.invq_of(size)
    T = [float(v) for v in pose.reshape(-1)]
    rs = np.random.RandomState(11)
    pts = np.stack([a["x"], a["y"], a["z"]], -1).astype(np.float32)
    pts = np.concatenate([pts, np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 3e38, 3e38], [-3e38, 1.0, 2.0]], np.float32)])
    lo, hi = mn[0], mn[0] + size
    coords = [lo, hi, -0.0, 0.0, math.nan, math.inf, -math.inf, 1e300, -1e300, 5e-324, -5e-324]
    for v in (lo, hi, lo + 1.0 / invq, lo + 2.0 / invq, lo + 12345.0 / invq, lo + 1.0 / inv, lo + 7.0 / inv, lo + 1048575.0 / inv):
        coords += [float(np.nextafter(v, -np.inf)), v, float(np.nextafter(v, np.inf))]
    coords += (lo + (rs.rand(300) * 1.2 - 0.1) * size).tolist()
    products = [0, (1 << 32) - 1, 1 << 32, (1 << 48) - 1, (1 << 32) + 1, ((1 << 24) - 1) ** 2, 1, 0xFFFFFFFF00000000 >> 16]
    products += [int(x) * int(y) for x, y in rs.randint(0, 1 << 24, (200, 2))]
    top = (1 << 24) - 1
    pairs = [[0, 0, 0, 0, 0, 0], [top, top, top, 0, 0, 0], [0, 0, 0, top, top, top], [top, 0, top, 0, top, 0], [5, 6, 7, 5, 6, 7], [1, 0, 0, 0, 0, 0]]
    pairs += rs.randint(0, 1 << 24, (200, 6)).tolist()
    b_ptr, num_b = 0x7F00DEAD0000, len(b)
    want = ar.stamp(b_ptr, num_b, _d64(inv), [_d64(v) for v in mn], 1)
    stamps = [(dict(want, totals=(3, 4, 5)), want), (want, dict(want, filled=0)), (dict(want, filled=0), want), (dict(want, filled=0), dict(want, filled=0)),
              (dict(want, magic=0xA5A5A5A5), want), (dict(want, magic=0), want), (dict(want, b=b_ptr + 16), want), (dict(want, numB=num_b + 1), want),
              (dict(want, inv=_d64(inv) + 1), want), (dict(want, filled=0xA5A5A5A5), want), (dict(want, filled=2), dict(want, filled=0))]
    for k in range(3):
        m = list(want["min"])
        m[k] ^= 1 << 63
        stamps.append((dict(want, min=tuple(m)), want))
    poisoned = dict(magic=0xA5A5A5A5, filled=0xA5A5A5A5, b=0xA5A5A5A5A5A5A5A5, numB=0xA5A5A5A5A5A5A5A5, inv=0xA5A5A5A5A5A5A5A5, min=(0xA5A5A5A5A5A5A5A5,) * 3, totals=(0, 0, 0))
    stamps.append((poisoned, want))
    stamp_records = np.zeros((len(stamps), 2), dtype=STAMP)
    for i, pair in enumerate(stamps):
        for j, s in enumerate(pair):
            stamp_records[i, j] = (s["magic"], s["filled"], s["b"], s["numB"], s["inv"], s["min"], s["totals"])
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(records), len(pts), len(coords), len(products), len(pairs), len(stamps)], "<u4").tobytes())
        f.write(np.array([g32, size], "<f4").tobytes())
        f.write(np.array(mn + T, "<f8").tobytes())
        f.write(np.array([b_ptr, num_b], "<u8").tobytes())
        f.write(b"".join(r.tobytes() for r in records))                   # (128 bytes each, the trailing padding included)
        f.write(pts.astype("<f4").tobytes())
        f.write(np.array(coords, "<f8").tobytes())
        f.write(np.array(products, "<u8").tobytes())
        f.write(np.array(pairs, "<u4").tobytes())
        f.write(stamp_records.tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.split("\n")
    assert lines.pop() == ""
    lines_want = []
    for i, r in enumerate(records):
        ok = ar.params_acceptable(r)
        assert ok == (i < len(good)), (["ok"] * len(good) + [w for _, w in bad])[i]
        lines_want.append(f"p {i:x} {int(ok):x}")
    lines_want.append(f"g {_d64(inv):x} {_d64(invq):x}")
    n_valid = 0
    for i, p in enumerate(pts.astype(np.float64).tolist()):
        cp, ok = ar.posed(T, p)
        n_valid += ok
        cells = [ar.cell_of(cp[k], mn[k], inv) for k in range(3)] if ok else [0, 0, 0]
        lines_want.append(f"c {i:x} 1 " + " ".join(f"{_d64(v):x}" for v in cp) + " " + " ".join(f"{c:x}" for c in cells) if ok else f"c {i:x} 0 0 0 0 0 0 0")
    qs = set()
    for x in coords:
        inside, q = ar.q_of(x, mn[0], invq)
        qs.add(q if inside else -1)
        lines_want.append(f"q {_d64(x):x} {ar.cell_of(x, mn[0], inv):x} {int(inside):x} {q:x}")
    lines_want += ["l {:x} {:x}".format(*ar.lo_hi(p)) for p in products]
    for qa in pairs:
        e = [qa[3 + k] - qa[k] for k in range(3)]
        lines_want.append(f"e {(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]:x}")
    lines_want.append(f"t {ar.STAMP_MAGIC:x} 1 {b_ptr:x} {num_b:x} {_d64(inv):x} " + " ".join(f"{v:x}" for v in want["min"]))
    lines_want += [f"s {i:x} {int(ar.stamp_serves(have, w)):x}" for i, (have, w) in enumerate(stamps)]
    assert len(lines) == len(lines_want)
    assert lines == lines_want, [(x, y) for x, y in zip(lines, lines_want) if x != y][:5]
    assert [ar.stamp_serves(h, w) for h, w in stamps[:4]] == [True, True, False, True] and not any(ar.stamp_serves(h, w) for h, w in stamps[4:])
    assert n_valid >= len(a) // 2 and len(pts) - n_valid >= 3 and qs >= {-1, 0, 1, 2, 12345, (1 << 24) - 1}
