"""CPU tier of the surface queries' shared rules (include/simlod_hip.h, "surface queries"): simlod_amd/csrc/surface_rules.hpp — which
SimlodSurfaceParams records a call accepts, rule N2's invq and truncation, rule N3's D, rule N4's factor and rules N3-N8 from nine sums to the
normal, the variation's two numbers and the colour index — checked on the host by a program of its own (tests/host/surface_rules_check.cpp,
built by plain g++ with the address and undefined-behaviour sanitizers, run as a host binary with nothing preloaded) against
tests/surface_ref.py, line by line; and hand tables."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import compare_ref as cr
import surface_ref as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = np.dtype({"names": ["S", "c", "within", "params"], "formats": [("<i8", 9), ("<f8", 3), "<u4", "<u4"], "offsets": [0, 72, 96, 100], "itemsize": 104})
SMALL_CASES = ["three_points", "two_points", "coincident", "collinear", "plane_grid", "line_tiny", "wide_sums", "cell_faces", "orient_flip", "shade_edges",
               "variation_edges"]


def _d64(x):
    return sf.bits_of(x)


def _f32bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_hand_tables():
    """Rules N2-N4 by hand."""
    assert sf.invq_of(0.5, 4.0) == 16384.0 / (0.5 + 0.5 / 1024.0) and sf.invq_of(0.0, 64.0) == 16384.0 * 16384.0
    invq = sf.invq_of(0.5, 4.0)
    assert [sf.q_of(p, invq) for p in (0.0, -0.0, 0.25, -0.25, 0.5, -0.5, 1e-9, -1e-9)] == [0, 0, 8184, -8184, 16368, -16368, 0, 0]   # towards zero
    assert abs(sf.q_of(0.5 * (1 + 2.0 ** -52), invq)) <= 16384
    assert [sf.widen(s) for s in (0, 1, -1, 1 << 32, -(1 << 32), (1 << 32) + 5, -(1 << 32) - 5)] == [0.0, 1.0, -1.0, 2.0 ** 32, -2.0 ** 32, 2.0 ** 32 + 5, -2.0 ** 32 - 5]
    assert sf.widen((1 << 60) - 1) == 2.0 ** 60 and sf.widen(-(1 << 60) + 1) == -2.0 ** 60 and sf.widen((1 << 53) + 1) == 2.0 ** 53   # one rounded add
    assert sf.factor_of([3.0, 0, 0, -1.0, 0, 0]) == (0.5, True) and sf.factor_of([0.0, 0, 0, 0, -0.75, 0]) == (2.0, True)
    assert sf.factor_of([0.0, -0.0, 0, 0, 0, 0]) == (2.0 ** 1023, False) and sf.factor_of([5e-324, 0, 0, 0, 0, 0]) == (2.0 ** 1023, True)
    assert sf.scale([2.0 ** 100, 2.0 ** -974, 0, 0, 0, 0])[0][:2] == [1.0, 5e-324]          # the small entry ends as the smallest subnormal
    assert sf.scale([1.0, -1.9999, 0, 0, 0, 2.0 ** -1074])[0] == [1.0, -1.9999, 0, 0, 0, 2.0 ** -1074]


def _records():
    """(accepted records, refused records and what is wrong with each)"""
    t = np.array(sf.shade_thresholds())

    def with_t(i, v):
        u = t.copy()
        u[i] = v
        return u
    good = [sf.params(0.5, sf.SHADE), sf.params(0.0, sf.VARIATION, light=(0.0, 0.0, 0.0)), sf.params(-0.0, sf.SHADE, orient=(0.0, 0.0, 0.0)),
            sf.params(3.0e38, sf.VARIATION, orient_mode=sf.POSITION, budget=(1 << 64) - 1, wg=0xFFFFFFFF), sf.params(1.0, sf.SHADE, thresholds=np.zeros(255)),
            sf.params(1.0, sf.SHADE, thresholds=with_t(0, -7.0)), sf.params(1.0, sf.SHADE, light=(0.0, -1e-45, 0.0), orient=(-3.0e38, 1.0, 2.0)),
            sf.params(1.0, sf.VARIATION, thresholds=with_t(254, 1e300))]
    bad = [(sf.params(-1.0, sf.SHADE), "radius < 0"), (sf.params(np.nan, sf.SHADE), "radius NaN"), (sf.params(np.inf, sf.SHADE), "radius inf"),
           (sf.params(1.0, sf.SHADE, reserved=1), "reserved"), (sf.params(1.0, 2), "colourBy 2"), (sf.params(1.0, 0xFFFFFFFF), "colourBy -1"),
           (sf.params(1.0, sf.SHADE, orient_mode=2), "orientMode 2"), (sf.params(1.0, sf.SHADE, light=(np.nan, 0.0, 1.0)), "light NaN"),
           (sf.params(1.0, sf.VARIATION, light=(0.0, np.inf, 1.0)), "light inf, unused"), (sf.params(1.0, sf.SHADE, orient=(0.0, 0.0, -np.inf)), "orient -inf"),
           (sf.params(1.0, sf.VARIATION, orient=(np.nan, 0.0, 0.0), orient_mode=sf.POSITION), "orient NaN"),
           (sf.params(1.0, sf.SHADE, light=(0.0, -0.0, 0.0)), "zero light"), (sf.params(1.0, sf.SHADE, thresholds=with_t(100, np.nan)), "threshold NaN"),
           (sf.params(1.0, sf.SHADE, thresholds=with_t(254, np.inf)), "threshold inf"), (sf.params(1.0, sf.SHADE, thresholds=with_t(10, t[8])), "descending"),
           (sf.params(1.0, sf.SHADE, thresholds=with_t(254, -1.0)), "last descending")]
    return good, bad


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("surface_rules") / "surface_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "surface_rules_check.cpp"), "-o", exe])
    return exe


def test_header_agrees_with_the_reference(checker, tmp_path):
    """Every line the host program prints equals surface_ref's: the records accepted and refused; invq; the truncation of offsets of both
    signs around whole steps; D at 0, +-1, +-2^32, +-(2^60 - 1) and at random sums; P's factor for matrices led by normal numbers,
    subnormals and zeros; and rules N3-N8 — v, lambdaNum, lambdaDen, vv, the fp32 normal, num, den and the index — from the sums of every
    sample of the small cases, under each of the case's orientations and lights and both colourBy values."""
    good, bad = _records()
    records = good + [r for r, _ in bad]
    radius, size = 0.2, 4.0
    invq = sf.invq_of(float(np.float32(radius)), size)
    rs = np.random.RandomState(7)
    offsets = [0.0, -0.0, 5e-324, -5e-324, 1.0 / invq, -1.0 / invq, float(np.float32(radius)), -float(np.float32(radius))]
    for k in (1, 2, 3, 100, 8191, 16383):
        for v in (k / invq, -k / invq):
            offsets += [float(np.nextafter(v, -np.inf)), v, float(np.nextafter(v, np.inf))]
    offsets += ((rs.rand(300) * 2 - 1) * float(np.float32(radius))).tolist()
    sums = [0, 1, -1, 1 << 32, -(1 << 32), (1 << 32) - 1, -(1 << 32) + 1, (1 << 32) + 1, -(1 << 32) - 1, (1 << 60) - 1, -(1 << 60) + 1, 1 << 31, -(1 << 31),
            (1 << 53) + 1, -(1 << 53) - 1, (1 << 59) + (1 << 5) + 1, 0x7FFFFFFF, 0xFFFFFFFF, -0xFFFFFFFF]
    sums += [int(v) for v in rs.randint(-(1 << 60), 1 << 60, 200, dtype=np.int64)] + [int(v) for v in rs.randint(-(1 << 34), 1 << 34, 100, dtype=np.int64)]
    matrices = [[3.0, 0, 0, -1.0, 0, 0], [0.0, -0.0, 0, 0, 0, 0], [5e-324, 0, 0, 0, 0, 0], [0, 0, -1e-310, 0, 2e-310, 0], [1.0, -1.9999, 0, 0, 0, 2.0 ** -1074],
                [2.0 ** 100, 2.0 ** -974, 0, 0, 0, 0], [0, 0, 0, 0, 0, -2.0 ** 124], [1e308, -1.7e308, 0, 0, 0, 0]]
    matrices += (rs.randn(100, 6) * 10.0 ** rs.randint(-300, 300, (100, 1))).tolist()
    # the samples: every sample of the small cases, with each record the case is run with
    samples, want_e = [], []
    for name in SMALL_CASES:
        a, b, mn, mx, r, _ = sf.case(name)
        pa, pb = cr._xyz(a), cr._xyz(b)
        valid_b = [j for j, s in enumerate(pb) if cr.is_valid(*s)]
        r32 = float(np.float32(r))
        cinvq = sf.invq_of(r32, 4.0)
        per = [sf.sums_of(p, pb, valid_b, r32 * r32, cinvq) for p in pa]
        for colour_by in (sf.SHADE, sf.VARIATION):
            for rec in sf.case_params(name, colour_by):
                records.append(rec)
                light, orient = [float(v) for v in rec["light"][0]], [float(v) for v in rec["orient"][0]]
                for p, (S, within) in zip(pa, per):
                    samples.append((S, p, within, len(records) - 1))
                    e = sf.estimate(S, within, p, orient, int(rec["orientMode"][0]))
                    i = len(samples) - 1
                    if e is None:
                        want_e.append(f"e {i:x} 0 0 0 0 0 0 0 0 0 0 0 0 0")
                        continue
                    num, den = sf.colour_terms(e, colour_by, light)
                    words = [_d64(x) for x in e[0]] + [_d64(e[1]), _d64(e[2]), _d64(e[3])] + [_f32bits(x) for x in e[0]] + [_d64(num), _d64(den)]
                    want_e.append(f"e {i:x} 1 " + " ".join(f"{w:x}" for w in words) + f" {sf.index_of(rec['thresholds'][0].tolist(), num, den):x}")
    sample_records = np.zeros(len(samples), dtype=SAMPLE)
    for i, (S, p, within, which) in enumerate(samples):
        sample_records[i] = (S, p, within, which)
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(records), len(offsets), len(sums), len(matrices), len(samples), 0], "<u4").tobytes())
        f.write(np.array([radius, size], "<f4").tobytes())
        f.write(np.concatenate(records).tobytes())
        f.write(np.array(offsets, "<f8").tobytes())
        f.write(np.array(sums, "<i8").tobytes())
        f.write(np.array(matrices, "<f8").tobytes())
        f.write(sample_records.tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.split("\n")
    assert lines.pop() == ""
    want = []
    for i, r in enumerate(records):
        ok = sf.params_acceptable(r)
        if i < len(good) + len(bad):
            assert ok == (i < len(good)), (["ok"] * len(good) + [w for _, w in bad])[i]
        want.append(f"p {i:x} {int(ok):x}")
    want.append(f"g {_d64(invq):x}")
    want += [f"q {_d64(p):x} {sf.q_of(p, invq) & 0xFFFFFFFF:x}" for p in offsets]
    want += [f"d {s & 0xFFFFFFFFFFFFFFFF:x} {_d64(sf.widen(s)):x}" for s in sums]
    for m in matrices:
        f, ok = sf.factor_of([float(x) for x in m])
        want.append(f"f {_d64(f):x} {int(ok):x}")
    want += want_e
    assert len(lines) == len(want)
    assert lines == want, [(a, b) for a, b in zip(lines, want) if a != b][:5]
    estimated = sum(1 for w in want_e if w.split()[2] == "1")
    assert estimated >= 500 and len(want_e) - estimated >= 14 and all(sf.params_acceptable(r) for r in records[len(good) + len(bad):])
    assert {sf.q_of(p, invq) for p in offsets} >= {0, 1, -1, 2, -2, 16383, -16383}
