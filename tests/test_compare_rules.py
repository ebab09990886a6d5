"""CPU tier of the compare queries' shared rules (include/simlod_hip.h, "compare queries"): simlod_amd/csrc/compare_rules.hpp — which
SimlodCompareParams records, boxes and counts a call accepts, rule C4's h, inv, cell and key, the key's home slot, the table's capacity and rule
C5's threshold index — checked on the host by a program of its own (tests/host/compare_rules_check.cpp, built by plain g++ with the address and
undefined-behaviour sanitizers, run as a host binary with nothing preloaded) against tests/compare_ref.py, line by line; and hand tables."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import compare_ref as cr
import summary_ref as sr
from simlod_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def _bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def _ulps(x):
    x = F32(x)
    return [_bits(np.nextafter(x, F32(-np.inf))), _bits(x), _bits(np.nextafter(x, F32(np.inf)))]


def _d64(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_hand_tables():
    """Rule C4 by hand: h at radius 0 and below the floor is size * 2^-20, above it r * (1 + 2^-10); FLT_MAX stays finite in fp64."""
    assert cr.h_of(0.0, 64.0) == 64.0 / 1048576.0 and cr.h_of(float(F32(1e-7)), 4.0) == 4.0 / 1048576.0
    assert cr.h_of(0.5, 4.0) == 0.5 + 0.5 / 1024.0 and cr.inv_of(0.5, 4.0) == 1.0 / (0.5 + 0.5 / 1024.0)
    assert np.isfinite(cr.h_of(FLT_MAX, 4.0)) and cr.inv_of(FLT_MAX, 4.0) > 0.0
    # in a box [100, 164) at the floor the cell is summary rule S2's: inv = 16384
    inv = cr.inv_of(0.0, 64.0)
    assert inv == 16384.0 and cr.cell_of((100.0, 164.0, 132.0), (100.0,) * 3, inv) == (0, 1048575, 524288)
    assert cr.cell_of((-1e30, 1e30, 99.0), (100.0,) * 3, inv) == (0, 1048575, 0)      # outside the box: the edge cells
    assert cr.key_of((1, 2, 3)) == 1 | 2 << 20 | 3 << 40 and cr.key_of((1048575,) * 3) == (1 << 60) - 1
    assert [cr.table_slots(n) for n in (0, 1, 2, 3, 1 << 31, (1 << 32) - 2, (1 << 32) - 1)] == [0, 2, 4, 8, 1 << 32, 1 << 33, 0]
    assert cr.home_of(0, 1 << 15) == 0 and all(cr.home_of(k, 2) in (0, 1) for k in range(50))
    t = [float(i) for i in range(1, 256)]
    assert [cr.index_of(t, v) for v in (0.0, 0.999, 1.0, 1.5, 255.0, 1e300, float("inf"))] == [0, 0, 1, 1, 255, 255, 255]


def _params():
    """(accepted records, refused records and what is wrong with each)"""
    lin = ((np.arange(1, 256) * 2.0) / 255.0) ** 2

    def rec(radius, t2=lin, reserved=0, budget=0, wg=0):
        r = np.zeros(1, dtype=abi.compare_params_dtype)
        with np.errstate(over="ignore"):
            r["radius"], r["reserved"], r["maxCandidates"], r["maxWorkgroups"], r["missColor"] = radius, reserved, budget, wg, 0xFF00FF00
        r["thresholds2"][0] = t2
        r["table"][0] = np.arange(256, dtype=np.uint32) * 0x01010101
        return r

    def with_t(i, v):
        t = lin.copy()
        t[i] = v
        return t
    good = [rec(0.5), rec(0.0), rec(-0.0), rec(FLT_MAX, budget=(1 << 64) - 1, wg=0xFFFFFFFF), rec(1e-45), rec(1.0, np.zeros(255)), rec(1.0, np.full(255, 7.5)),
            rec(1.0, with_t(0, -3.0)), rec(1.0, with_t(254, 1e300))]
    bad = [(rec(-1.0), "radius < 0"), (rec(np.nan), "radius NaN"), (rec(np.inf), "radius inf"), (rec(-np.inf), "radius -inf"), (rec(1.0, reserved=1), "reserved 1"),
           (rec(1.0, reserved=0x80000000), "reserved high bit"), (rec(1.0, with_t(100, np.nan)), "threshold NaN"), (rec(1.0, with_t(254, np.inf)), "threshold inf"),
           (rec(1.0, with_t(0, -np.inf)), "threshold -inf"), (rec(1.0, with_t(10, lin[8])), "descending"), (rec(1.0, with_t(254, 0.0)), "last descending")]
    return good, bad


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("compare_rules") / "compare_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "compare_rules_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("box_min,size,radius", [(0.0, 4.0, 0.5), (100.0, 64.0, 0.0), (-417.25, 1000.0, 1e-7), (0.0, 4.0, FLT_MAX), (3.3, 37.5, 2.167)])
def test_header_agrees_with_the_reference(checker, tmp_path, box_min, size, radius):
    """Every line the host program prints equals compare_ref's: the records accepted and refused, h and inv, the cell of the fixed edge values
    (signed zeros, denormals, the box's faces and the cell faces min + k*h with their fp32 neighbours, coordinates far outside the box, the
    non-finite values) and of random ones, the keys of their triples, the threshold index at each threshold and its two fp64 neighbours, the
    home slots and the table's capacity."""
    good, bad = _params()
    good[0]["radius"] = radius
    records = good + [r for r, _ in bad]
    mn, sz, r32 = float(F32(box_min)), float(F32(size)), float(F32(radius))
    h = cr.h_of(r32, sz)
    rs = np.random.RandomState(5)
    values = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
              0x7F800001, 0x7F7FFFFF, 0xFF7FFFFF, _bits(mn - 1e30), _bits(mn + 1e30), _bits(1e30), _bits(-1e30), _bits(mn - 0.5 * sz), _bits(mn + 3.0 * sz)]
    values += _ulps(mn) + _ulps(mn + sz)
    values += rs.randint(0, 1 << 32, 600, dtype=np.uint64).tolist()
    values += np.array(mn + sz * (rs.rand(600) * 1.2 - 0.1), F32).view(np.uint32).tolist()
    with np.errstate(over="ignore"):                                        # (at FLT_MAX the cell faces lie beyond fp32)
        for k in (1, 2, 3, 7, 100, 1048574, 1048575, 1048576):
            if np.isfinite(F32(mn + k * h)):
                values += _ulps(mn + k * h)
        values += np.array(mn + h * (rs.rand(300) * 40.0 - 2.0), F32).view(np.uint32).tolist()
    t2 = [float(v) for v in good[0]["thresholds2"][0]]
    d2 = [0.0, 5e-324, 1e300, float("inf"), float(np.nextafter(t2[0], 0.0))]
    for t in t2:
        d2 += [float(np.nextafter(t, -np.inf)), t, float(np.nextafter(t, np.inf))]
    keys = [0, 1, (1 << 60) - 1, 1 << 59] + rs.randint(0, 1 << 60, 300, dtype=np.uint64).tolist()
    counts = [0, 1, 2, 3, 4, 5, 1000, 1 << 20, (1 << 20) + 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, 1 << 40]
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(records), len(values), len(d2), len(keys), len(counts), 0], "<u4").tobytes())
        f.write(np.array([box_min, size], "<f4").tobytes())
        f.write(np.concatenate(records).tobytes())
        f.write(np.array(values, "<u4").tobytes())
        f.write(np.array(d2, "<f8").tobytes())
        f.write(np.array(keys, "<u8").tobytes())
        f.write(np.array(counts, "<u8").tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.split("\n")
    assert lines.pop() == ""
    inv = cr.inv_of(r32, sz)
    cells = [sr.cell20(sr.float_of(b), mn, inv) for b in values]
    want = []
    for i, r in enumerate(records):
        ok = cr.params_acceptable(float(r["radius"][0]), r["thresholds2"][0].tolist(), int(r["reserved"][0]))
        assert ok == (i < len(good)), (["ok"] * len(good) + [w for _, w in bad])[i]
        want.append(f"p {i:x} {int(ok):x}")
    want.append(f"g {_d64(h):x} {_d64(inv):x} 1")
    want += [f"v {b:x} {c:x}" for b, c in zip(values, cells)]
    for i in range(len(values) - 2):
        valid = cr.is_valid(*(sr.float_of(b) for b in values[i:i + 3]))
        want.append(f"k {int(valid):x} {cr.key_of(tuple(cells[i:i + 3])) if valid else 0:x}")
    want += [f"i {_d64(v):x} {cr.index_of(t2, v):x}" for v in d2]
    want += [f"h {k:x} {cr.home_of(k, 2):x} {cr.home_of(k, 1 << 15):x} {cr.home_of(k, 1 << 33):x}" for k in keys]
    for n in counts:
        s = cr.table_slots(n)
        want.append(f"s {n:x} {int(s != 0):x} {s:x} {s.bit_length() - 1 if s else 0:x}")
    assert len(lines) == len(want)
    assert lines == want, [(a, b) for a, b in zip(lines, want) if a != b][:5]
    assert {0, 1048575} <= set(cells)
    if radius == 0.5:
        assert {1, 2, 3, 7} <= set(cells)                                   # the cell faces and their neighbours fall on both sides
