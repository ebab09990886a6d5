"""CPU tier of the summary queries' shared rules (include/simlod_hip.h, "summary queries"): simlod_amd/csrc/summary_rules.hpp — which
SimlodSummaryParams records a call accepts (rule S8), the key of rule S1, the cell of rule S2 and the index of rule S3 — checked on the host by a
program of its own (tests/host/summary_rules_check.cpp, built by plain g++ with the address and undefined-behaviour sanitizers, run as a host
binary with nothing preloaded) against tests/summary_ref.py, line by line; and the hand tables of the key's order and the cell's edges."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import summary_ref as sr
from simlod_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def _ulps(x):
    """x as fp32 and its two neighbours, as bits."""
    x = F32(x)
    return [_bits(np.nextafter(x, F32(-np.inf))), _bits(x), _bits(np.nextafter(x, F32(np.inf)))]


def edge_values(box_min, size):
    """The fixed list: signed zeros, denormals, infinities, NaNs of both signs, the box's faces and their neighbours, the coordinates that put t
    on 255 and on 1048575 (exact for a power-of-two size) and their neighbours, a coordinate below the box."""
    mn, size = float(F32(box_min)), float(F32(size))
    v = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F800000, 0xFF800000,
         0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF]
    v += _ulps(mn) + _ulps(mn + size)
    v += _ulps(mn + 255.0 * size / 1048576.0) + _ulps(mn + 1048575.0 * size / 1048576.0) + _ulps(mn + size / 1048576.0)
    v += [_bits(mn - 0.5 * size), _bits(mn - 1e30), _bits(mn + 0.5 * size), _bits(mn + 3.0 * size)]
    return v


def test_key_is_a_total_order():
    """Rule S1 by hand: -inf < -1 < -denormal < -0 < +0 < denormal < 1 < +inf, the NaNs outside, and unkey undoes key."""
    order = [0xFFC00000, 0xFF800001, 0xFF800000, _bits(-1.0), 0x80000001, 0x80000000, 0x00000000, 0x00000001, _bits(1.0), 0x7F800000, 0x7F800001, 0x7FC00000]
    keys = [sr.key(b) for b in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert sr.key(0x7F800000) == sr.KEY_POS_INF and sr.key(0xFF800000) == sr.KEY_NEG_INF
    assert [sr.unkey(k) for k in keys] == order
    # every key that is no NaN's lies between the keys of the infinities, every NaN's outside
    for b in order:
        assert sr.is_nan(b) == (not sr.KEY_NEG_INF <= sr.key(b) <= sr.KEY_POS_INF), hex(b)
    assert [sr.is_finite(b) for b in (0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0, 0x80000001)] == [False, False, False, True, True, True]


def test_cell_hand_table():
    """Rule S2 in a box [100, 164): inv = 16384 and every t below is exact."""
    inv = sr.inv_of(64.0)
    assert inv == 16384.0
    below = float(np.nextafter(F32(100.0), F32(0.0)))
    want = {100.0: 0, below: 0, 50.0: 0, 100.0 + 1.0 / 16384.0: 1, 100.0 + 255.0 / 16384.0: 255, 164.0: 1048575, 100.0 + 1048575.0 / 16384.0: 1048575,
            100.0 + 1048574.0 / 16384.0: 1048574, 132.0: 524288, float("inf"): 1048575, float("-inf"): 0, float("nan"): 0, 1e30: 1048575}
    for x, c in want.items():
        assert sr.cell20(x, 100.0, inv) == c, x
    # just below the max face (164 - 2^-16): t = 1048575.75, the last cell; one 20-bit cell below it, t = 1048574.75, the one before
    assert sr.cell20(float(np.nextafter(F32(164.0), F32(0.0))), 100.0, inv) == 1048575
    assert sr.cell20(164.0 - 2.0 ** -14 - 2.0 ** -16, 100.0, inv) == 1048574
    # rule S3's index is rule E3's: the same formula with 255 in the place of 1048575
    assert [sr.z_index(z, 100.0, 16384.0) for z in (100.0, below, 100.0 + 255.0 / 16384.0, 100.0 + 254.5 / 16384.0, float("nan"), float("inf"))] == [0, 0, 255, 254, 0, 255]


def _params():
    """(accepted records, refused records and what is wrong with each)"""
    def rec(z0, scale, wg=0, reserved=0):
        r = np.zeros(1, dtype=abi.summary_params_dtype)
        with np.errstate(over="ignore"):
            r["z0"], r["scale"], r["maxWorkgroups"], r["reserved"] = z0, scale, wg, reserved
        return r
    good = [rec(0.0, 1.0), rec(-5.0, 1e-30, 7), rec(1e30, 3e38, 0xFFFFFFFF), rec(-0.0, 1e-45, 1)]
    bad = [(rec(0.0, 0.0), "scale 0"), (rec(0.0, -0.0), "scale -0"), (rec(0.0, -1.0), "scale < 0"), (rec(0.0, np.nan), "scale NaN"), (rec(0.0, np.inf), "scale inf"),
           (rec(np.nan, 1.0), "z0 NaN"), (rec(np.inf, 1.0), "z0 inf"), (rec(-np.inf, 1.0), "z0 -inf"), (rec(0.0, 1.0, 0, 1), "reserved 1"),
           (rec(0.0, 1.0, 3, 0x80000000), "reserved high bit")]
    return good, bad


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("summary_rules") / "summary_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "summary_rules_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("box_min,size,z0,scale", [(100.0, 64.0, 100.0, 16384.0), (0.0, 37.5, -3.25, 7.3), (-417.25, 1000.0, 12.0, 0.001)])
def test_header_agrees_with_the_reference(checker, tmp_path, box_min, size, z0, scale):
    """Every line the host program prints — the fixed edge values and 2 000 random bit patterns — equals summary_ref's, and
    summary_acceptable accepts and refuses what rule S8 lists."""
    good, bad = _params()
    rs = np.random.RandomState(5)
    values = edge_values(box_min, size) + rs.randint(0, 1 << 32, 1000, dtype=np.uint64).tolist()
    values += np.array(box_min + size * (rs.rand(1000) * 1.2 - 0.1), F32).view(np.uint32).tolist()
    records = good + [r for r, _ in bad]
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(records), len(values)], "<u4").tobytes())
        f.write(np.array([box_min, size, z0, scale], "<f4").tobytes())
        f.write(np.concatenate(records).tobytes())
        f.write(np.array(values, "<u4").tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.split("\n")
    assert lines.pop() == "" and len(lines) == len(records) + len(values)
    want = [f"p {i:x} {1 if i < len(good) else 0:x}" for i in range(len(records))]
    assert lines[: len(records)] == want, [(a, b, (["ok"] * len(good) + [w for _, w in bad])[i]) for i, (a, b) in enumerate(zip(lines, want)) if a != b]
    mn, sz, z0f, scf = (float(F32(v)) for v in (box_min, size, z0, scale))
    inv = sr.inv_of(sz)
    cells, indices = set(), set()
    for b, line in zip(values, lines[len(records):]):
        k = sr.key(b)
        x = sr.float_of(b)
        c, i = sr.cell20(x, mn, inv), sr.z_index(x, z0f, scf)
        assert line == f"v {b:x} {k:x} {b:x} {int(sr.is_nan(b)):x} {int(sr.is_finite(b)):x} {c:x} {i:x}", hex(b)
        assert sr.unkey(k) == b
        cells.add(c); indices.add(i)
    assert {0, 1048575} <= cells and {0, 255} <= indices
    if size == 64.0:
        assert {1, 254, 255, 1048574} <= cells and {254, 255} <= indices          # (an ulp at 100 is an eighth of a cell)
