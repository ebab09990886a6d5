"""GPU tier of the styled LAS decode (include/simlod_hip.h, "styled decode"): simlod_decode_las_styled against lasio.decode_records byte for byte
at the tile edges of both tile sizes, every byte shift and every kind of field; no style and the RGB style against simlod_decode_las; what the
call refuses; a LAS file coloured by intensity into an octree, through DeviceOctree.add_las and through the headless C++ host."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import las_style_ref as ref
import oracle
from simlod_amd import abi, camera, lasio, synthetic
from simlod_amd.lasio import Style
from test_gpu_parity import H, W, _device
from test_las_style import SCALE, OFFSET, WINDOWS, _bad_styles, _lut, _records
from util import STATS_BUILD_FIELDS, assert_stats_equal, host_image_of, voxel_colors_are_member

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 255, 256, 257, 511, 512, 513, 1025, 1537]
LAYOUTS = [(0, 20), (1, 28), (1, 29), (3, 34), (5, 63), (6, 30), (7, 37), (8, 38), (10, 67), (1, 65), (6, 255)]
MAIN = ["intensity", "classification", "point_source_id", "elevation", "gps_time"]
REST = ["return_number", "number_of_returns", "user_data", "scan_angle"]


def _decode(raw, n, bpp, fmt, style, plain=False, scale=SCALE, offset=OFFSET):
    """One call on the device (plain: simlod_decode_las; else simlod_decode_las_styled with `style`, a record or None) -> (rc, the points, the
    whole output buffer).  0x5A behind the output, checked after the call."""
    import torch
    from simlod_amd.runtime import lib
    L = lib()
    d_raw = torch.from_numpy(np.array(raw, dtype=np.uint8).reshape(-1)).to("cuda:0") if n else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((max(n, 1) * 16 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    head = (ctypes.c_void_p(d_raw.data_ptr()), ctypes.c_uint64(n), ctypes.c_uint32(bpp), ctypes.c_uint32(fmt), (ctypes.c_double * 3)(*scale), (ctypes.c_double * 3)(*offset))
    tail = (ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if plain:
        rc = L.simlod_decode_las(*head, *tail)
    else:
        rc = L.simlod_decode_las_styled(*head, None if style is None else ctypes.c_void_p(style.ctypes.data), *tail)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    assert np.all(host[n * 16:] == 0x5A), "decode wrote past its output"
    return rc, host[: n * 16].view(abi.point_dtype), host


def _assert_device_is_mirror(rec, n, bpp, fmt, style, what):
    rc, got, _ = _decode(rec[:n], n, bpp, fmt, style.record())
    assert rc == 0, what
    want = lasio.decode_records(rec[:n], bpp, fmt, SCALE, OFFSET, style)
    bad = np.nonzero(np.any(got.view(np.uint8).reshape(n, 16) != want.view(np.uint8).reshape(n, 16), axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {n} points differ, first at {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"


@pytest.mark.parametrize("fmt,bpp", LAYOUTS)
def test_device_equals_the_mirror_at_every_tile_edge(built_libs, fmt, bpp):
    """Random records (random GPS bit patterns, flag bits above the class), one set per layout cut to every size."""
    rec = _records(max(SIZES), fmt, bpp, seed=bpp)
    lut = _lut(bpp)
    for name in MAIN:
        if not ref.has(abi.LAS_ATTRIBUTES[name], fmt):
            continue
        for n in SIZES:
            _assert_device_is_mirror(rec, n, bpp, fmt, Style(name, *WINDOWS[name], lut), (name, fmt, bpp, n))


@pytest.mark.parametrize("fmt,bpp", [(1, 29), (6, 30)])
def test_device_equals_the_mirror_on_the_other_attributes_and_on_edge_values(built_libs, fmt, bpp):
    n = 513
    lut = _lut(1)
    rec = _records(n, fmt, bpp, seed=4)
    for name in REST:
        _assert_device_is_mirror(rec, n, bpp, fmt, Style(name, *WINDOWS[name], lut), (name, fmt, bpp))
    # values on the window's ends, NaNs, infinities and denormals as GPS times, both ends of the scan angle's range
    hi = 1000.0
    special = np.array([0.0, -0.0, hi, np.nextafter(hi, 0.0), np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1e308, -1e308], dtype=np.float64)
    angles = np.array([-128, 127, 0, -1]) if fmt <= 5 else np.array([-30000, 30000, 0, -1])
    rec = _records(n, fmt, bpp, seed=5, gps_time=np.resize(special, n), intensity=np.resize([0, 65535, 100, 355, 356, 99], n), scan_angle=np.resize(angles, n))
    rec[::3, 15 if fmt <= 5 else 16] = 0xff
    _assert_device_is_mirror(rec, n, bpp, fmt, Style("gps_time", 0.0, hi, lut), "gps time, special values")
    _assert_device_is_mirror(rec, n, bpp, fmt, Style("gps_time", -1e308, 1e308, lut), "gps time, a window wider than the doubles")
    _assert_device_is_mirror(rec, n, bpp, fmt, Style("intensity", 100.0, 356.0, lut), "intensity on the window's ends")
    _assert_device_is_mirror(rec, n, bpp, fmt, Style("intensity", 0.0, 65536.0, lut), "intensity, full window")
    _assert_device_is_mirror(rec, n, bpp, fmt, Style("scan_angle", *((-128.0, 128.0) if fmt <= 5 else (-30000 * 0.006, 181.0)), lut), "scan angle")
    _assert_device_is_mirror(rec, n, bpp, fmt, Style.classification(), "class 0xff")
    rec[:, 8:12] = np.ascontiguousarray((np.arange(n) - 20).astype("<i4")).view(np.uint8).reshape(n, 4)
    rc, got, _ = _decode(rec, n, bpp, fmt, Style("elevation", 0.0, 64.0, lut).record(), scale=(1.0, 1.0, 0.25), offset=(0.0, 0.0, 0.0))
    want = lasio.decode_records(rec, bpp, fmt, (1.0, 1.0, 0.25), (0.0, 0.0, 0.0), Style("elevation", 0.0, 64.0, lut))
    assert rc == 0 and np.array_equal(got.view(np.uint8), want.view(np.uint8)), "elevation with t on integers"


@pytest.mark.parametrize("fmt,bpp", [(2, 26), (3, 34), (5, 63), (7, 37), (1, 28), (8, 38), (10, 67), (10, 255)])
def test_no_style_forwards_and_rgb_style_is_the_plain_decode(built_libs, fmt, bpp):
    for n in (0, 513, 1025):
        rec = _records(n, fmt, bpp, seed=n)
        rc0, plain, _ = _decode(rec, n, bpp, fmt, None, plain=True)
        rc1, fwd, _ = _decode(rec, n, bpp, fmt, None)
        assert rc0 == 0 and rc1 == 0 and np.array_equal(fwd.view(np.uint8), plain.view(np.uint8))
        rc2, rgb, _ = _decode(rec, n, bpp, fmt, Style.rgb().record())
        assert rc2 == 0 and np.array_equal(rgb.view(np.uint8), lasio.decode_records(rec, bpp, fmt, SCALE, OFFSET, Style.rgb()).view(np.uint8))
        if fmt in (2, 3, 5, 7):
            assert np.array_equal(rgb.view(np.uint8), plain.view(np.uint8))
        elif fmt in (8, 10) and n:
            assert np.all(plain["color"] == 0xff000000) and len(np.unique(rgb["color"])) > 100


def test_every_rejection_leaves_the_output_untouched(built_libs):
    good, bad = _bad_styles()
    raw = np.zeros(4 * 256, dtype=np.uint8)
    for what, r, bpp, fmt in bad:
        rc, _, host = _decode(raw[: 4 * bpp], 4, bpp, fmt, r)
        assert rc != 0, what
        assert np.all(host == 0x5A), what
    for what, r, bpp, fmt in good:
        assert _decode(raw[: 4 * bpp], 4, bpp, fmt, r)[0] == 0, what
    # what simlod_decode_las refuses: a misaligned input, a format whose RGB does not fit (with and without a style)
    import torch
    from simlod_amd.runtime import lib
    d_raw = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda:0")
    style = Style.intensity().record()
    args = lambda src, bpp, fmt, s: (ctypes.c_void_p(src), ctypes.c_uint64(4), ctypes.c_uint32(bpp), ctypes.c_uint32(fmt), (ctypes.c_double * 3)(*SCALE),
                                    (ctypes.c_double * 3)(*OFFSET), s, ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert lib().simlod_decode_las_styled(*args(d_raw.data_ptr() + 4, 34, 3, ctypes.c_void_p(style.ctypes.data))) != 0
    assert lib().simlod_decode_las_styled(*args(d_raw.data_ptr(), 24, 2, ctypes.c_void_p(style.ctypes.data))) == 0          # (intensity needs no RGB)
    assert lib().simlod_decode_las_styled(*args(d_raw.data_ptr(), 24, 2, None)) != 0
    assert lib().simlod_decode_las_styled(*args(d_raw.data_ptr(), 24, 2, ctypes.c_void_p(Style.rgb().record().ctypes.data))) != 0
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy()[64:] == 0x5A)


# ---- end to end: a colourless file becomes an octree coloured by intensity ------------------------------------------------------------------------
BOX = (600.0, 400.0, 40.0)
WORLD_MIN = (694000.0, 3915000.0, -3.0)


@pytest.fixture(scope="module")
def intensity_file(built_libs, tmp_path_factory):
    """A format-1 file of 60 000 points (one batch), the mirror's points for it under Style.intensity(), and the oracle's octree of those points."""
    pts0, box = synthetic.terrain(60_000, seed=11, box=BOX, tile=50.0)
    path = str(tmp_path_factory.mktemp("las_style") / "grey.las")
    h = lasio.points_to_las(path, pts0, box, fmt=1, scale=0.001, world_min=WORLD_MIN, version=(1, 2))
    tr = tuple(-m for m in h.min)
    raw = lasio.read_records(path, h, 0, h.numPoints)
    pts = lasio.decode_records(raw, h.bytesPerPoint, h.format, h.scale, lasio.decode_offset(h, tr), Style.intensity().in_frame(tr))
    assert len(pts) == 60_000 and len(np.unique(pts["color"])) > 200
    T = camera.lookat_transform((1.8 * box[0], -1.2 * box[1], 1.4 * max(box)), (0.5 * box[0], 0.5 * box[1], 0.3 * box[2]), W, H)
    from cases import uniforms_for
    u = uniforms_for(np.asarray(box, np.float32), T, persistent=8 << 30)
    host = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=8)
    host.reset(u)
    host.add_points(u, pts)
    return path, h, pts, box, T, host.stats[0].copy()


def _sorted(samples, fields=("x", "y", "z", "color")):
    """The samples' bit patterns as rows, in lexicographic order."""
    rows = np.stack([np.ascontiguousarray(samples[f]).view(np.uint32) for f in fields], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def test_a_file_coloured_by_intensity_builds_the_octree_of_the_mirrors_points(intensity_file):
    """Stats against the oracle's octree of the mirror's points; the full export against a second device octree fed those points: the points of the
    leaves equal sample for sample (sorted), the voxels equal in position — a voxel's colour is the colour of whichever point of its cell the
    builder saw first, which two runs need not agree on (include/simlod_hip.h, "octree export / import"), so each must be the colour of a mirror
    point of its cell."""
    path, h, pts, box, T, want = intensity_file
    exports = []
    for feed in ("las", "points"):
        dev = _device(ring_slots=8)
        u = dev.uniforms(W, H, T, box)
        dev.reset(u)
        if feed == "las":
            dev.add_las(u, path, style=Style.intensity())
        else:
            dev.add_points(u, pts)
        ds = dev.read_stats()
        assert int(ds["dbg"]) == 0
        assert_stats_equal(ds, want, STATS_BUILD_FIELDS, feed)
        if feed == "las":
            nodes, pers, nn = host_image_of(dev)
            assert voxel_colors_are_member(nodes, nn, pts, box) > 0
        ex = dev.export_octree(u, select="all")
        leaf = np.repeat((ex.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0, ex.nodes["numSamples"])
        exports.append((ex.samples[leaf], ex.samples[~leaf]))
        dev.close()
    (leaves_a, voxels_a), (leaves_b, voxels_b) = exports
    assert len(leaves_a) == 60_000 and len(voxels_a) > 0
    assert np.array_equal(_sorted(leaves_a), _sorted(leaves_b)) and np.array_equal(_sorted(leaves_a), _sorted(pts))
    assert np.array_equal(_sorted(voxels_a, "xyz"), _sorted(voxels_b, "xyz"))
    assert int((leaves_a["color"] != 0xff000000).sum()) > 50_000 and int((voxels_a["color"] != 0xff000000).sum()) > 0


def test_headless_host_colours_by_intensity(intensity_file):
    """The C++ host with --las-colour intensity builds the oracle's octree of the mirror's points (its Stats line; the colours themselves are
    held by the export comparison above: the host's frame of this small file shows no point, with or without the option)."""
    path, h, pts, box, T, want = intensity_file
    exe = os.path.join(ROOT, "harness", "simlod_headless")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "harness")])
    out = subprocess.run([exe, path, "--las-colour", "intensity"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"numNodes (\d+) numInner (\d+) numLeaves (\d+) numPoints (\d+) numVoxels (\d+) persistentBytes (\d+) chunkPoolSize (\d+) dbg (\d+)", out.stdout)
    assert m, out.stdout
    assert [int(v) for v in m.groups()] == [int(want[k]) for k in ("numNodes", "numInner", "numLeaves", "numPoints", "numVoxels", "allocatedBytes_persistent", "chunkPoolSize")] + [0]
    assert "las colour: intensity" in out.stdout
