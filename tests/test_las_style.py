"""CPU tier of the styled LAS decode (include/simlod_hip.h, "styled decode"): lasio.decode_records, the numpy mirror of simlod_decode_las_styled,
against tests/las_style_ref.py (a per-record restatement of the spec's field table) for every attribute of every format, on random records and on
planted edge values; against oracle.decode_las_port where the two overlap; lasio.Style; the layout of SimlodLasStyle and what the call refuses
(simlod_amd/csrc/las_style_rules.hpp by a host program of its own under the sanitizers, and the C entry itself with no points)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import las_style_ref as ref
import oracle
from simlod_amd import abi, lasio
from simlod_amd.lasio import Style

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE, OFFSET = (1e-3, 2.5e-3, 1e-2), (-694000.123, 3915000.456, -3.0)
WINDOWS = {"intensity": (0.0, 65536.0), "classification": (0.0, 256.0), "return_number": (1.0, 6.0), "number_of_returns": (0.0, 16.0),
           "user_data": (16.0, 200.0), "point_source_id": (1000.0, 50000.0), "scan_angle": (-90.0, 90.0), "gps_time": (-1e9, 3e9),
           "elevation": (-10.0, 60.0)}


def _lut(seed=3):
    return np.random.RandomState(seed).randint(0, 2 ** 32, size=256, dtype=np.uint64).astype(np.uint32)      # (top bytes set: they must be ignored)


def _records(n, fmt, bpp=None, seed=0, **attributes):
    rs = np.random.RandomState(seed + 17 * fmt)
    xyz = rs.randint(-2 ** 31, 2 ** 31 - 1, size=(n, 3), dtype=np.int64).astype(np.int32)
    xyz[:, 2] = rs.randint(-2000, 8000, size=n)                                   # heights that fall inside and outside the elevation window
    rgb = rs.randint(0, 65536, size=(n, 3)).astype(np.uint16)
    return lasio.las_records(xyz, rgb, fmt, bytes_per_point=bpp, seed=seed + 1, attributes=attributes or None)


def _assert_mirror_is_ref(rec, bpp, fmt, style, what):
    got = lasio.decode_records(rec, bpp, fmt, SCALE, OFFSET, style)
    x, y, z, colour = ref.decode(rec, bpp, fmt, SCALE, OFFSET, style.attribute, style.lo, style.hi, style.lut)
    for name, want in (("x", x), ("y", y), ("z", z)):
        assert np.array_equal(got[name].view(np.uint32), want.view(np.uint32)), (what, name)
    bad = np.nonzero(got["color"] != colour)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} colours differ, first at record {bad[:1]}"
    return got


@pytest.mark.parametrize("fmt", range(11))
@pytest.mark.parametrize("attribute", ref.NAMES[1:])
def test_mirror_equals_the_per_record_reference(attribute, fmt):
    """Random records: GPS times are random bit patterns (NaNs, infinities and denormals among them), flag bits are set above the class."""
    a = abi.LAS_ATTRIBUTES[attribute]
    assert ref.NAMES[a] == attribute
    rec = _records(700, fmt, seed=a)
    if attribute == "gps_time" and fmt in (0, 2):
        assert not ref.has(a, fmt)
        with pytest.raises(ValueError):
            lasio.decode_records(rec, rec.shape[1], fmt, SCALE, OFFSET, Style(a, *WINDOWS[attribute], _lut()))
        return
    if attribute == "gps_time":                                                   # every class of double is there, whatever the seed
        special = np.array([0x7ff8000000000001, 0xfff0000000000000, 0x7ff0000000000000, 1, 0x8000000000000001, 0, 0x8000000000000000], dtype="<u8").view("<f8")
        rec = _records(700, fmt, seed=a, gps_time=np.resize(special, 700))
        rec[7:, :] = _records(700, fmt, seed=a)[7:, :]
    got = _assert_mirror_is_ref(rec, rec.shape[1], fmt, Style(a, *WINDOWS[attribute], _lut()), (attribute, fmt))
    assert np.all(got["color"] >> 24 == 255) and len(np.unique(got["color"])) > 1


@pytest.mark.parametrize("fmt", [0, 1, 3, 6, 8, 10])
def test_planted_edge_values(fmt):
    lut = _lut(5)
    at = lambda got, k: int(got["color"][k]) & 0xffffff
    entry = lambda k: int(lut[k]) & 0xffffff
    # intensity 0 and 65535 over the full window, and a window whose ends are hit exactly: v == lo, the largest double below hi, v == hi
    rec = _records(8, fmt, intensity=np.array([0, 65535, 100, 355, 356, 99, 228, 227]))
    got = _assert_mirror_is_ref(rec, rec.shape[1], fmt, Style(abi.LAS_INTENSITY, 0.0, 65536.0, lut), "intensity, full window")
    assert at(got, 0) == entry(0) and at(got, 1) == entry(255)
    got = _assert_mirror_is_ref(rec, rec.shape[1], fmt, Style(abi.LAS_INTENSITY, 100.0, 356.0, lut), "intensity, 100..356")
    assert [at(got, k) for k in range(2, 8)] == [entry(k) for k in (0, 255, 255, 0, 128, 127)]
    got = _assert_mirror_is_ref(rec, rec.shape[1], fmt, Style(abi.LAS_INTENSITY, 0.0, float(np.nextafter(355.0, 400.0)), lut), "hi just above a value")
    assert at(got, 3) == entry(255) and at(got, 4) == entry(255) and at(got, 2) < 1 << 24
    if fmt not in (0, 2):
        hi = 1000.0
        rec = _records(4, fmt, gps_time=np.array([0.0, float(np.nextafter(hi, 0.0)), hi, -0.0]))
        got = _assert_mirror_is_ref(rec, rec.shape[1], fmt, Style(abi.LAS_GPS_TIME, 0.0, hi, lut), "gps time at the window's ends")
        assert [at(got, k) for k in range(4)] == [entry(0), entry(255), entry(255), entry(0)]
    # scan angles: -128 is the 8-bit field's lowest value, -30000 steps of 0.006 degrees are -180 degrees
    angles = np.array([-128, 127, 0, -1]) if fmt <= 5 else np.array([-30000, 30000, 0, -1])
    rec = _records(4, fmt, scan_angle=angles)
    lo, hi = (-128.0, 128.0) if fmt <= 5 else (-30000 * 0.006, 30000 * 0.006 + 1.0)
    got = _assert_mirror_is_ref(rec, rec.shape[1], fmt, Style(abi.LAS_SCAN_ANGLE, lo, hi, lut), "scan angle")
    assert at(got, 0) == entry(0) and (fmt > 5 or at(got, 1) == entry(255))
    # class byte 0xff: 31 with the flag bits masked off (formats 0-5), 255 where the class has a byte of its own
    rec = _records(3, fmt)
    rec[:, 15 if fmt <= 5 else 16] = 0xff
    got = _assert_mirror_is_ref(rec, rec.shape[1], fmt, Style(abi.LAS_CLASSIFICATION, 0.0, 256.0, lut), "class 0xff")
    assert at(got, 0) == entry(31 if fmt <= 5 else 255)
    # an elevation window in which several t are integers exactly: heights k / 4 over [0, 64) give t = k
    rec = _records(300, fmt)
    rec[:, 8:12] = np.ascontiguousarray((np.arange(300) - 20).astype("<i4")).view(np.uint8).reshape(300, 4)
    got = lasio.decode_records(rec, rec.shape[1], fmt, (1.0, 1.0, 0.25), (0.0, 0.0, 0.0), Style(abi.LAS_ELEVATION, 0.0, 64.0, lut))
    x, y, z, colour = ref.decode(rec, rec.shape[1], fmt, (1.0, 1.0, 0.25), (0.0, 0.0, 0.0), abi.LAS_ELEVATION, 0.0, 64.0, lut)
    assert np.array_equal(got["color"], colour) and np.array_equal(got["z"], z)
    assert [at(got, k) for k in (0, 20, 21, 275, 276, 299)] == [entry(k) for k in (0, 0, 1, 255, 255, 255)]


@pytest.mark.parametrize("fmt,bpp", [(1, 28), (2, 26), (3, 34), (7, 37), (5, 63), (0, 20), (8, 38), (10, 67)])
def test_no_style_and_rgb_style_against_the_oracles_decode(built_libs, fmt, bpp):
    rec = _records(900, fmt, bpp)
    port = oracle.decode_las_port(rec, bpp, fmt, SCALE, OFFSET)
    if fmt in (1, 2, 3, 7):
        assert np.array_equal(lasio.decode_records(rec, bpp, fmt, SCALE, OFFSET).view(np.uint8), port.view(np.uint8))
    got = lasio.decode_records(rec, bpp, fmt, SCALE, OFFSET, Style.rgb())
    x, y, z, colour = ref.decode(rec, bpp, fmt, SCALE, OFFSET, ref.RGB, 0.0, 1.0, None)
    assert np.array_equal(got["color"], colour) and np.array_equal(got["z"], z)
    if fmt in (2, 3, 5, 7):
        assert np.array_equal(got.view(np.uint8), port.view(np.uint8))
    elif fmt in (8, 10):                                                          # the triple is read although the reference's list stops at 7
        c = np.ascontiguousarray(rec[:, 30:36]).view("<u2").reshape(-1, 3).astype(np.uint32)
        c = np.where(c > 255, c // 256, c)
        assert np.array_equal(got["color"], 0xff000000 | c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)) and np.all(port["color"] == 0xff000000)
    else:
        assert np.all(got["color"] == 0xff000000)


def test_las_records_default_output_is_unchanged():
    rs = np.random.RandomState(2)
    xyz, rgb = rs.randint(-1000, 1000, size=(50, 3)).astype(np.int32), rs.randint(0, 65536, size=(50, 3)).astype(np.uint16)
    for fmt in (1, 3, 6, 8):
        want = np.random.RandomState(9).randint(0, 256, size=(50, lasio.FORMAT_BYTES[fmt]), dtype=np.uint8)
        want[:, 0:12] = xyz.view(np.uint8).reshape(50, 12)
        if fmt in (3, 8):
            want[:, {3: 28, 8: 30}[fmt]:{3: 34, 8: 36}[fmt]] = rgb.view(np.uint8).reshape(50, 6)
        assert np.array_equal(lasio.las_records(xyz, rgb, fmt, seed=9), want)
        planted = lasio.las_records(xyz, rgb, fmt, seed=9, attributes={"return_number": np.full(50, 5)})
        assert np.array_equal(planted[:, 14] & (0x7 if fmt <= 5 else 0xf), np.full(50, 5))
        assert np.array_equal(np.delete(planted, 14, axis=1), np.delete(want, 14, axis=1))
        assert np.array_equal(planted[:, 14] >> (3 if fmt <= 5 else 4), want[:, 14] >> (3 if fmt <= 5 else 4))


def test_style_constructors():
    for s in (Style.intensity(), Style.classification(), Style.elevation(10.0, 90.0), Style.of("scan_angle", -30, 30, "heat"), Style.rgb()):
        assert s.lut.dtype == np.uint32 and s.lut.shape == (256,) and np.all(s.lut >> 24 == 0)
        r = s.record()
        assert r.dtype == abi.las_style_dtype and int(r["reserved"][0]) == 0 and np.array_equal(r["lut"][0], s.lut)
        assert (int(r["attribute"][0]), float(r["lo"][0]), float(r["hi"][0])) == (s.attribute, s.lo, s.hi)
    c = Style.classification()
    assert (c.attribute, c.lo, c.hi) == (abi.LAS_CLASSIFICATION, 0.0, 256.0)
    assert len({int(c.lut[k]) for k in (2, 3, 4, 5, 6, 9)}) == 6 and int(c.lut[200]) == int(c.lut[77])      # six classes apart, one fallback
    assert int(Style.classification({6: (1, 2, 3)}).lut[6]) == 0x030201
    i = Style.intensity()
    assert (i.attribute, i.lo, i.hi) == (abi.LAS_INTENSITY, 0.0, 65536.0) and int(i.lut[0]) == 0 and int(i.lut[255]) == 0xffffff
    for name, stops in lasio.RAMPS.items():
        lut = Style.of("intensity", 0, 1, name).lut
        assert int(lut[0]) == stops[0][0] | stops[0][1] << 8 | stops[0][2] << 16 and int(lut[255]) == stops[-1][0] | stops[-1][1] << 8 | stops[-1][2] << 16
        ch = np.stack([lut & 255, (lut >> 8) & 255, (lut >> 16) & 255]).astype(np.int64)
        assert any(np.all(np.diff(ch[k][:32]) >= 0) and np.all(np.diff(ch[k][-32:]) >= 0) and ch[k][-1] > ch[k][0] for k in range(3)), name
    assert Style.elevation(10.0, 90.0).in_frame((5.0, 6.0, -7.5)).lo == 2.5 and Style.elevation(10.0, 90.0).in_frame((5.0, 6.0, -7.5)).hi == 82.5
    assert Style.intensity(3, 9).in_frame((5.0, 6.0, -7.5)).lo == 3.0
    h = lasio.LasHeader(format=3)
    assert Style.auto(h).attribute == abi.LAS_RGB
    h.format = 6
    assert Style.auto(h).attribute == abi.LAS_INTENSITY
    h.format = 8
    assert Style.auto(h).attribute == abi.LAS_RGB


def _bad_styles():
    """(what, record, bytesPerPoint, format) the call must refuse, and one of each kind it must accept."""
    ok = Style.intensity().record()
    bad = []

    def edit(what, bpp=34, fmt=3, **fields):
        r = ok.copy()
        for k, v in fields.items():
            r[k] = v
        bad.append((what, r, bpp, fmt))
    edit("unknown attribute", attribute=abi.LAS_ATTRIBUTE_COUNT)
    edit("attribute 2^31", attribute=1 << 31)
    edit("reserved", reserved=1)
    edit("reserved under rgb", attribute=abi.LAS_RGB, reserved=7)
    edit("lo nan", lo=np.nan)
    edit("hi inf", hi=np.inf)
    edit("lo -inf", lo=-np.inf)
    edit("hi == lo", lo=5.0, hi=5.0)
    edit("hi < lo", lo=5.0, hi=4.0)
    edit("gps time in format 0", bpp=20, fmt=0, attribute=abi.LAS_GPS_TIME)
    edit("gps time in format 2", bpp=26, fmt=2, attribute=abi.LAS_GPS_TIME)
    edit("gps time beyond the record", bpp=27, fmt=1, attribute=abi.LAS_GPS_TIME)
    edit("point source id beyond the record", bpp=19, fmt=0, attribute=abi.LAS_POINT_SOURCE_ID)
    edit("class beyond the record", bpp=16, fmt=6, attribute=abi.LAS_CLASSIFICATION)
    edit("rgb beyond the record", bpp=35, fmt=8, attribute=abi.LAS_RGB)
    edit("format 11", fmt=11)
    edit("format 11 under rgb", fmt=11, attribute=abi.LAS_RGB)
    edit("record shorter than xyz", bpp=11, fmt=0, attribute=abi.LAS_ELEVATION)
    edit("record beyond the staging limit", bpp=256, fmt=0)
    good = [("intensity", ok, 34, 3), ("rgb ignores the window", Style(abi.LAS_RGB, 1.0, 0.0).record(), 34, 3), ("rgb without a triple", Style.rgb().record(), 20, 0),
            ("gps time to the last byte", Style.of("gps_time", 0, 1).record(), 28, 1), ("point source id to the last byte", Style.of("point_source_id", 0, 1).record(), 20, 0),
            ("elevation", Style.elevation(0, 1).record(), 12, 0), ("class", Style.classification().record(), 17, 6)]
    return good, bad


def test_rules_header_under_the_sanitizers_and_the_struct_layout(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "las_style_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "las_style_check.cpp"), "-o", exe])
    good, bad = _bad_styles()
    every = [(f"{name} in format {fmt}", Style.of(name, *WINDOWS[name]).record(), lasio.FORMAT_BYTES[fmt], fmt) for name in ref.NAMES[1:] for fmt in range(11)
             if ref.has(abi.LAS_ATTRIBUTES[name], fmt)]
    cases = good + every + [c for c in bad if 12 <= c[2] <= 255]                 # (the record's length range is the launcher's own check)
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(cases)], "<u4").tobytes())
        for _, r, bpp, fmt in cases:
            f.write(r.tobytes() + np.array([bpp, fmt], "<u4").tobytes())
    run = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    got = np.fromfile(tmp_path / "out.bin", dtype="<u4").reshape(len(cases), 8)
    for k, (what, r, bpp, fmt) in enumerate(cases):
        assert int(got[k, 0]) == (1 if k < len(good) + len(every) else 0), what
    for k, (what, r, bpp, fmt) in enumerate(every, start=len(good)):            # the field the kernel is sent to is the field the mirror reads
        a = int(r["attribute"][0])
        if a == abi.LAS_ELEVATION:
            assert int(got[k, 1]) == 3, what
            continue
        off, kind, shift, mask = lasio.las_field(a, fmt)
        sign = (mask + 1) >> 1 if kind[0] == "i" else 0
        want = [2, off, 8, 0, 0, 0, 1000] if kind == "f8" else [1, off, int(kind[1]), shift, mask, sign, 6 if kind == "i2" else 1000]
        assert got[k, 1:].tolist() == want, what
    m = re.search(r"sizeof (\d+) attribute (\d+) reserved (\d+) lo (\d+) hi (\d+) lut (\d+) count (\d+)", run.stdout)
    d = abi.las_style_dtype
    assert [int(v) for v in m.groups()] == [1048, 0, 4, 8, 16, 24, abi.LAS_ATTRIBUTE_COUNT] == [d.itemsize] + [d.fields[n][1] for n in d.names] + [10]
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    enum = re.search(r"enum \{ (SIMLOD_LAS_RGB = 0,[^}]*)\}", src).group(1)
    names = [n.strip().split(" ")[0] for n in enum.split(",")]
    assert names == ["SIMLOD_LAS_" + n.upper() for n in ref.NAMES] + ["SIMLOD_LAS_ATTRIBUTE_COUNT"]
    assert [abi.LAS_ATTRIBUTES[n] for n in ref.NAMES] == list(range(10))


def test_library_exports_the_call_and_refuses_without_launching(built_libs):
    """With no points nothing is ever launched and no device pointer is looked at, so what is left of the call is its judgement of the style: this runs with or without a GPU."""
    from simlod_amd import runtime
    L = runtime.lib()
    assert "simlod_decode_las_styled" in runtime.EXPORTED_SYMBOLS and hasattr(L, "simlod_decode_las_styled")
    scale, offset = (ctypes.c_double * 3)(*SCALE), (ctypes.c_double * 3)(*OFFSET)
    call = lambda r, bpp, fmt: L.simlod_decode_las_styled(None, ctypes.c_uint64(0), ctypes.c_uint32(bpp), ctypes.c_uint32(fmt), scale, offset,
                                                          None if r is None else ctypes.c_void_p(r.ctypes.data), None, None)
    good, bad = _bad_styles()
    for what, r, bpp, fmt in good:
        assert call(r, bpp, fmt) == 0, what
    for what, r, bpp, fmt in bad:
        assert call(r, bpp, fmt) == 1, what                                       # hipErrorInvalidValue
        with pytest.raises(ValueError):
            s = Style(int(r["attribute"][0]), float(r["lo"][0]), float(r["hi"][0]))
            if int(r["reserved"][0]) != 0:
                raise ValueError("reserved")                                      # (a lasio.Style has no such field)
            lasio.decode_records(np.zeros((0, bpp), np.uint8), bpp, fmt, SCALE, OFFSET, s)
    assert call(None, 34, 3) == 0                                                 # no style: simlod_decode_las, which accepts an empty batch unseen
    # with points, null device pointers are refused like simlod_decode_las's
    assert L.simlod_decode_las_styled(None, ctypes.c_uint64(4), ctypes.c_uint32(34), ctypes.c_uint32(3), scale, offset, ctypes.c_void_p(good[0][1].ctypes.data), None, None) == 1
