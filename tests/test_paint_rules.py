"""CPU tier of the paint regions' shared rules (include/simlod_hip.h, "paint regions"): simlod_amd/csrc/paint_rules.hpp — which SimlodPaint records
a call accepts (rule E9) and the colour word a sample gets (rules E1-E3) — checked on the host by a program of its own
(tests/host/paint_rules_check.cpp, built by plain g++ with the address and undefined-behaviour sanitizers, run as a host binary with nothing
preloaded) against tests/paint_ref.py, one sample at a time in Python integers and floats, and against octree_io.Paint.apply; and the hand
tables of rules E2 and E3."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import paint_ref as pf
from simlod_amd import abi
from simlod_amd.octree_io import Paint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_blend_hand_table():
    """Rule E2, bytes 0 and 255 against strength 1, 128 and 255: (c*(256 - a) + t*a + 128) >> 8."""
    want = {  # (c, t, a): c'
        (0, 0, 1): 0, (0, 0, 128): 0, (0, 0, 255): 0,
        (0, 255, 1): 1, (0, 255, 128): 128, (0, 255, 255): 254,            # (255 + 128) >> 8, (32640 + 128) >> 8, (65025 + 128) >> 8
        (255, 0, 1): 254, (255, 0, 128): 128, (255, 0, 255): 1,            # (65025 + 128) >> 8, (32640 + 128) >> 8, (255 + 128) >> 8
        (255, 255, 1): 255, (255, 255, 128): 255, (255, 255, 255): 255,    # (65280 + 128) >> 8
    }
    for (c, t, a), out in want.items():
        assert pf.blend_byte(c, t, a) == out == pf.blend_byte_rounded(c, t, a), (c, t, a)
        word = 0xAB000000 | c | (c << 8) | (c << 16)
        got = int(Paint.blend(t | (t << 8) | (t << 16) | 0x77000000, a).apply(np.array([word], np.uint32), np.zeros(1, F32))[0])
        assert got == (0xAB000000 | out | (out << 8) | (out << 16)) == pf.blend(word, t | (t << 8) | (t << 16), a), (c, t, a)
    # every byte pair at every strength: the integer formula is the rounding, and a byte never leaves 0..255 nor passes its target
    for a in (1, 2, 77, 128, 254, 255):
        for c in range(0, 256, 5):
            for t in range(0, 256, 3):
                out = pf.blend_byte(c, t, a)
                assert out == pf.blend_byte_rounded(c, t, a) and min(c, t) <= out <= max(c, t)
    # the bytes are independent and byte 3 is kept
    assert pf.blend(0x12FF0080, 0xEE00FF80, 128) == 0x12808080


def test_ramp_hand_table():
    """Rule E3: t at exactly 0, just below 1, exactly 255, negative, NaN, and z equal to z0."""
    below_one = float(np.nextafter(1.0, 0.0))
    assert [pf.ramp_index_of_t(t) for t in (0.0, -0.0, below_one, 1.0, 254.99999999, 255.0, 255.5, 256.0, 1e300, np.inf, -1e-300, -3.5, -np.inf, np.nan)] == \
        [0, 0, 0, 1, 254, 255, 255, 255, 255, 255, 0, 0, 0, 0]
    # through z, z0 and scale as the record holds them (fp32): z0 = 2, scale = 0.5 -> t = (z - 2) / 2, every value exact
    p = Paint(abi.PAINT_RAMP, z0=2.0, scale=0.5, table=np.arange(256) + 1000)
    z = np.array([2.0, 4.0 - 2.0 ** -21, 4.0, 512.0, 511.99997, 513.0, 1e30, 1.0, -1e30, np.nan, np.inf, -np.inf], F32)
    want = [0, 0, 1, 255, 254, 255, 255, 0, 0, 0, 255, 0]
    assert float(z[1]) < 4.0 and float(z[4]) < 512.0
    assert [pf.ramp_index(float(v), 2.0, 0.5) for v in z] == want
    assert p.ramp_index(z).tolist() == want
    assert p.apply(np.zeros(len(z), np.uint32), z).tolist() == [1000 + i for i in want]
    # Paint.ramp(z0, z1, table): 256 equal bins over [z0, z1), the ends held outside
    q = Paint.ramp(10.0, 74.0, np.arange(256))
    assert float(q.scale) == 4.0 and float(q.z0) == 10.0
    assert q.ramp_index(np.array([9.0, 10.0, 10.24, 10.25, 73.74, 73.75, 74.0, 80.0], F32)).tolist() == [0, 0, 0, 1, 254, 255, 255, 255]


def _records():
    """(accepted records with haveColors, refused records with haveColors and what is wrong with each)"""
    tab = pf.ramp_table()
    good = [(Paint.set(0x01020304).record(), 0), (Paint.set(0xFFFFFFFF).record(), 1), (Paint.blend(0x00FF7F01, 1).record(), 0),
            (Paint.blend(0xFF0080FF, 128).record(), 0), (Paint.blend(0x10203040, 255).record(), 1), (Paint.ramp(-3.0, 9.5, tab).record(), 0),
            (Paint(abi.PAINT_RAMP, z0=0.0, scale=1e-30, table=tab).record(), 0), (Paint(abi.PAINT_RAMP, z0=-1e30, scale=3e38, table=tab).record(), 0),
            (Paint.array().record(), 1)]
    # fields a mode does not use are ignored
    r = Paint.set(7).record(); r["strength"], r["scale"], r["z0"] = 999, np.nan, np.inf
    good.append((r, 0))
    r = Paint.blend(7, 9).record(); r["scale"] = -1.0
    good.append((r, 0))
    bad = []
    for mode in (4, 5, 0xFFFFFFFF):
        r = Paint.set(1).record(); r["mode"] = mode
        bad.append((r, 1, f"mode {mode}"))
    for base in (Paint.set(1), Paint.blend(1, 2), Paint.ramp(0, 1, tab), Paint.array()):
        for field, k in (("reserved", None), ("reserved2", 0), ("reserved2", 1)):
            r = base.record()
            if k is None:
                r[field] = 1
            else:
                r[field][0, k] = 0x80000000
            bad.append((r, 1, f"mode {base.mode} {field}"))
    for s in (0, 256, 0xFFFFFFFF):
        r = Paint.blend(1, 2).record(); r["strength"] = s
        bad.append((r, 0, f"strength {s}"))
    for z0, scale in ((0.0, 0.0), (0.0, -1.0), (0.0, np.nan), (0.0, np.inf), (np.nan, 1.0), (np.inf, 1.0), (-np.inf, 1.0), (0.0, -0.0)):
        r = Paint.ramp(0, 1, tab).record(); r["z0"], r["scale"] = z0, scale
        bad.append((r, 0, f"ramp z0 {z0} scale {scale}"))
    bad.append((Paint.array().record(), 0, "ARRAY without colors"))
    return good, bad


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("paint_rules") / "paint_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "paint_rules_check.cpp"), "-o", exe])
    return exe


def test_header_paints_as_the_reference_does(checker, tmp_path):
    """4 000 samples — random words and heights, heights that put t on and next to the integers 0, 1, 255 and 256, NaN and infinities — under
    every accepted record: the colour and the ramp index equal paint_ref's per sample and Paint.apply's; every record rule E9 refuses is
    refused; the Python constructors refuse what the header refuses."""
    rs = np.random.RandomState(11)
    good, bad = _records()
    n = 4000
    z = (rs.rand(n) * 40.0 - 10.0).astype(F32)
    z[:8] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e38, -1e38, 1e-45]
    k = 8
    for rec, _ in good:
        if int(rec["mode"][0]) != abi.PAINT_RAMP:
            continue
        z0, sc = float(rec["z0"][0]), float(rec["scale"][0])
        for ti in (0.0, 1.0, 2.0, 254.0, 255.0, 256.0):
            with np.errstate(over="ignore", invalid="ignore"):
                c = F32(z0 + ti / sc)
                z[k: k + 3] = [np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))]
            k += 3
    col = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    col[:4] = [0, 0xFFFFFFFF, 0xFF000000, 0x00FFFFFF]
    smp = np.zeros(n, dtype=[("z", "<f4"), ("color", "<u4")])
    smp["z"], smp["color"] = z, col
    records = [r for r, _ in good] + [r for r, _, _ in bad]
    have = np.array([h for _, h in good] + [h for _, h, _ in bad], "<u4")
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(records), n], "<u4").tobytes())
        f.write(np.concatenate(records).tobytes())
        f.write(have.tobytes())
        f.write(smp.tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(len(records), 1 + 8 * n)
    zl = [float(v) for v in z]
    seen_idx = set()
    for j, (rec, _) in enumerate(good):
        r = rec[0]
        mode = int(r["mode"])
        assert got[j, 0] == 1, f"record {j} (mode {mode}) refused"
        colour, index = got[j, 1: 1 + 4 * n].view("<u4"), got[j, 1 + 4 * n:].view("<u4")
        if mode == abi.PAINT_ARRAY:
            assert not colour.any() and not index.any()
            continue
        table = [int(v) for v in r["table"]]
        want = [pf.new_colour(mode, int(c), zz, int(r["color"]), int(r["strength"]), float(r["z0"]), float(r["scale"]), table) for c, zz in zip(col, zl)]
        assert colour.tolist() == want, f"record {j} (mode {mode}): the header and the reference differ"
        if mode == abi.PAINT_RAMP:
            assert index.tolist() == [pf.ramp_index(zz, float(r["z0"]), float(r["scale"])) for zz in zl]
            seen_idx |= set(index.tolist())
        else:
            assert not index.any()
        p = Paint(mode, int(r["color"]), int(r["strength"]) if mode == abi.PAINT_BLEND else 0, r["z0"] if mode == abi.PAINT_RAMP else 0.0,
                  r["scale"] if mode == abi.PAINT_RAMP else 0.0, r["table"])
        assert p.apply(col, z).tolist() == want, f"record {j} (mode {mode}): Paint.apply and the reference differ"
    assert {0, 1, 2, 253, 254, 255} <= seen_idx
    for j, (_, _, what) in enumerate(bad):
        assert not got[len(good) + j].any(), f"a record with {what} was accepted"
    for kw in (dict(mode=4), dict(mode="blend", strength=0), dict(mode="blend", strength=256), dict(mode="ramp", scale=0.0), dict(mode="ramp", scale=-1.0),
               dict(mode="ramp", scale=np.nan), dict(mode="ramp", scale=1e39), dict(mode="ramp", z0=np.inf, scale=1.0), dict(mode="set", color=1 << 32),
               dict(mode="ramp", scale=1.0, table=np.zeros(255))):
        with pytest.raises(ValueError):
            Paint(**kw)
    with pytest.raises(ValueError):
        Paint.ramp(3.0, 3.0, np.zeros(256))
