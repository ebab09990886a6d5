"""CPU tier of the packed samples (include/simlod_hip.h, "packed samples"): the ABI, the refusals, which precede device work, the numpy mirror
octree_io.pack_samples / unpack_samples against the per-record restatement of tests/pack_ref.py, rule K8 on oracle-built octrees, and PackedExport's
file format."""
import ctypes
import os
import re

import numpy as np
import pytest

import cases
import deep_ref
import pack_ref as kr
from region_ref import host_octree
from simlod_amd import abi
from simlod_amd.octree_io import OctreeExport, PackedExport, pack_samples, unpack_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUILT = {}

OCTREES = [(name, cut) for name in cases.CASES for cut in (False, True)] + [("terrain_4x100k@" + k, False) for k in ("dyadic", "inexact", "georef")] + \
          [("d13", False), ("d20", False)]


def octree(name, cut=False):
    """The oracle-built octree `name` as a full export, or truncated(2, "cut"), once per session."""
    if name not in _BUILT:
        if name in ("d13", "d20"):
            _BUILT[name] = deep_ref.built(name).export
        elif "@" in name:
            case, kind = name.split("@")
            _BUILT[name] = host_octree(case, box_min=cases.offset_of(kind, cases.case(case)[1]))[0]
        else:
            _BUILT[name] = host_octree(name)[0]
    ex = _BUILT[name]
    return ex.truncated(2, "cut") if cut else ex


def test_abi_matches_the_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodPackCounts\) == (\d+)", src).group(1)) == abi.pack_counts_dtype.itemsize == 40
    found = re.findall(r"offsetof\(SimlodPackCounts, (\w+)\) == (\d+)", src)
    assert [f for f, _ in found] == list(abi.pack_counts_dtype.names) == ["numSamples", "numClamped", "numInexact", "numAlpha", "error", "reserved"]
    for field, off in found:
        assert abi.pack_counts_dtype.fields[field][1] == int(off), field
    for name, value in (("SIMLOD_PACK_COLOR_BITS", abi.PACK_COLOR_BITS), ("SIMLOD_PACK_POINT_BITS", abi.PACK_POINT_BITS), ("SIMLOD_PACK_VOXEL_BITS", abi.PACK_VOXEL_BITS),
                        ("SIMLOD_PACK_SHIFT_X", abi.PACK_SHIFT_X), ("SIMLOD_PACK_SHIFT_Y", abi.PACK_SHIFT_Y), ("SIMLOD_PACK_SHIFT_Z", abi.PACK_SHIFT_Z)):
        assert int(re.search(rf"#define {name}\s+(\d+)u", src).group(1)) == value, name
    # rule K0: rgb, three fields of 13 bits, bit 63 free
    assert abi.PACK_SHIFT_X == abi.PACK_COLOR_BITS and abi.PACK_SHIFT_Y == abi.PACK_SHIFT_X + abi.PACK_POINT_BITS
    assert abi.PACK_SHIFT_Z == abi.PACK_SHIFT_Y + abi.PACK_POINT_BITS and abi.PACK_SHIFT_Z + abi.PACK_POINT_BITS == 63


def test_library_refuses_before_device_work(built_libs):
    """Every refusal of the two calls precedes device work: hipErrorInvalidValue (1) without a GPU, the buffers untouched."""
    from simlod_amd import runtime
    L = runtime.lib()
    for sym in ("simlod_pack_buffer_min_bytes", "simlod_pack_samples", "simlod_unpack_samples"):
        assert sym in runtime.EXPORTED_SYMBOLS and hasattr(L, sym)
    n = 8
    need = int(L.simlod_pack_buffer_min_bytes(n, 0))
    assert int(L.simlod_pack_buffer_min_bytes(n, 5000)) == need + 5 * abi.PACK_ITEM_BYTES
    assert int(L.simlod_pack_buffer_min_bytes(n + 100, 0)) >= need + 100 * abi.PACK_ITEM_BYTES and need >= (n + 1) * abi.PACK_ITEM_BYTES
    u = np.zeros(1, dtype=abi.uniforms_dtype)
    u["boxMin"], u["boxMax"] = (0, 0, 0), (1, 1, 1)
    bufs = {k: np.full(b, 0xA5, np.uint8) for k, b in (("table", 40 * n), ("entries", 24 * n), ("samples", 16 * 8), ("scratch", need), ("packed", 8 * 8), ("counts", 40))}
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(which, uu=u, null=(), num=n, scratch_bytes=need):
        g = {k: (None if k in null else b) for k, b in bufs.items()}
        src, dst = (g["samples"], g["packed"]) if which == "simlod_pack_samples" else (g["packed"], g["samples"])
        return getattr(L, which)(p(uu), p(g["table"]), p(g["entries"]), num, p(src), ctypes.c_uint64(8), p(g["scratch"]), ctypes.c_uint64(scratch_bytes), p(dst),
                                 p(g["counts"]), None)

    for which in ("simlod_pack_samples", "simlod_unpack_samples"):
        for k in ("table", "samples", "scratch", "packed", "counts"):
            assert call(which, null=(k,)) == 1, (which, k)
        for k in ((), ("entries",)):                     # with and without entries
            assert call(which, uu=None, null=k) == 1
            assert call(which, num=0, null=k) == 1
            assert call(which, scratch_bytes=need - 1, null=k) == 1
        for field, value in (("boxMin", (np.nan, 0, 0)), ("boxMax", (1, np.inf, 1)), ("boxMax", (0, 0, 0)), ("boxMin", (2, 2, 2)), ("boxMin", (-3e38, 0, 0))):
            w = u.copy()
            w[field] = value
            if field == "boxMin" and value[0] == -3e38:
                w["boxMax"] = (3e38, 1, 1)
            assert call(which, uu=w) == 1, (which, field, value)
    assert all((b == 0xA5).all() for b in bufs.values())


def _assert_mirror_is_ref(table, samples, mn, mx, pick=None):
    packed, c = pack_samples(table, samples, mn, mx)
    ref = kr.pack_ref(table, samples, mn, mx, pick=pick)
    assert len(ref) > 0
    for i, (word, _, _, _) in ref.items():
        assert int(packed[i]) == word, f"sample {i}: {int(packed[i]):#x}, the rules give {word:#x}"
    back, uc = unpack_samples(table, packed, mn, mx)
    for i, (x, y, z, color) in kr.unpack_ref(table, packed, mn, mx, pick=pick).items():
        got = back[i]
        assert (kr.bits(got["x"]), kr.bits(got["y"]), kr.bits(got["z"]), int(got["color"])) == (kr.bits(x), kr.bits(y), kr.bits(z), color), f"sample {i}"
    return packed, c, back, uc, ref


@pytest.mark.parametrize("where", ["origin", "georef"])
def test_mirror_is_the_rules_on_the_hand_table(where):
    mn = np.zeros(3, np.float32) if where == "origin" else np.asarray(cases.GEOREF, np.float32)
    mx = (mn + np.asarray((1, 1, 1) if where == "origin" else (600, 400, 40), np.float32)).astype(np.float32)
    table = kr.the_hand_table()
    from simlod_amd.octree_io import validate_table
    validate_table(table, int(table["numSamples"].astype(np.int64).sum()))
    assert sorted(set(table["numSamples"].tolist())) == sorted(kr.COUNTS)
    sel = (table["flags"] & abi.EXPORT_FLAG_SELECTED) != 0
    is_leaf = (table["flags"] & abi.EXPORT_FLAG_LEAF) != 0
    assert set(table["level"][sel & ~is_leaf].tolist()) == {0, 1, 7, 13, 19} and set(table["level"][sel & is_leaf].tolist()) == {1, 7, 13, 19, 20}
    assert kr.num_pieces(table) > len(table) + 2            # (the GPU tier's scratch buffer with one item too few lies above the refusal)
    samples, trouble = kr.hand_samples(table, mn, mx)
    assert sorted(trouble) == sorted(kr.TROUBLE)
    packed, c, back, uc, ref = _assert_mirror_is_ref(table, samples, mn, mx)
    assert len(ref) == len(samples)
    assert int(c["numSamples"]) == len(samples) and int(c["error"]) == 0
    assert int(c["numClamped"]) == sum(r[1] for r in ref.values()) and int(c["numInexact"]) == sum(r[2] for r in ref.values())
    assert int(c["numAlpha"]) == sum(r[3] for r in ref.values()) == 2
    for what in ("nan", "+inf", "-inf", "max face", "below min"):
        assert ref[trouble[what]][1], f"{what}: not clamped"
    assert ref[trouble["off centre"]][2] and not ref[trouble["off centre"]][1]
    i = trouble["nan"]
    assert (int(packed[i]) >> abi.PACK_SHIFT_Y) & 0x1FFF == 0
    assert (int(packed[trouble["+inf"]]) >> abi.PACK_SHIFT_X) & 0x1FFF == 8191 and (int(packed[trouble["max face"]]) >> abi.PACK_SHIFT_X) & 0x1FFF == 8191
    assert (int(packed[trouble["-inf"]]) >> abi.PACK_SHIFT_Z) & 0x1FFF == 0 and (int(packed[trouble["below min"]]) >> abi.PACK_SHIFT_Y) & 0x1FFF == 0
    assert not (packed >> np.uint64(63)).any() and (back["color"] >> 24 == 0xFF).all()
    assert uc.tobytes() == np.array((len(samples), 0, 0, 0, 0, 0), dtype=abi.pack_counts_dtype).tobytes()
    if where == "origin":
        # every voxel but the one moved off its centre comes back bit for bit (the two alpha samples by their xyz and rgb)
        vox = kr.voxel_mask(table, len(samples))
        vox[trouble["off centre"]] = False
        for f in "xyz":
            assert back[f][vox].tobytes() == samples[f][vox].tobytes()
        assert ((back["color"] ^ samples["color"]) & 0xFFFFFF == 0).all()
        assert int(c["numInexact"]) == 1
        n, worst = kr.assert_points_within_bound(table, samples, back, mn, mx, what="hand table")
        assert n > 5000


def test_mirror_is_the_rules_on_the_georef_terrain():
    ex = octree("terrain_4x100k@georef")
    pick = set(np.random.RandomState(23).choice(ex.num_samples, 2000, replace=False).tolist())
    _, c, _, _, ref = _assert_mirror_is_ref(ex.nodes, ex.samples, ex.box_min, ex.box_max, pick=pick)
    assert len(ref) == 2000


@pytest.mark.parametrize("name,cut", OCTREES, ids=[n + ("-cut2" if c else "") for n, c in OCTREES])
def test_oracle_octrees_round_trip(name, cut):
    """Rule K8 on what the oracle built: no voxel is inexact, no sample has another alpha than 0xff, voxel entries come back byte for byte, every
    point that was not clamped lies within the bound."""
    ex = octree(name, cut)
    t, s = ex.nodes, ex.samples
    packed, c = pack_samples(t, s, ex.box_min, ex.box_max)
    back, uc = unpack_samples(t, packed, ex.box_min, ex.box_max)
    print(f"{name} cut={cut}: {c}")
    assert int(c["error"]) == 0 and int(c["numSamples"]) == ex.num_samples == int(uc["numSamples"]) > 0
    assert int(c["numInexact"]) == 0 and int(c["numAlpha"]) == 0
    vox = kr.voxel_mask(t, len(s))
    assert back[vox].tobytes() == s[vox].tobytes()
    n, worst = kr.assert_points_within_bound(t, s, back, ex.box_min, ex.box_max, what=name)
    print(f"  {int(vox.sum())} voxels, {n} unclamped points, worst ratio to the bound {worst:.5f}")
    assert n + int(vox.sum()) + int(c["numClamped"]) == ex.num_samples
    if name == "terrain_4x100k@georef":
        assert int(c["numClamped"]) > 0                   # (fp32 puts a few points a step outside their leaf's cube there)
    if name == "hotspot_150k" and cut:
        assert vox.all() and back.tobytes() == s.tobytes()
    elif not cut:
        assert vox.any() and not vox.all()
    # the classes say the same
    px, pc = ex.pack(return_counts=True)
    assert isinstance(px, PackedExport) and px.packed.tobytes() == packed.tobytes() and pc.tobytes() == c.tobytes()
    again = px.unpack()
    assert isinstance(again, OctreeExport) and again.samples.tobytes() == back.tobytes() and again.nodes.tobytes() == t.tobytes()
    assert (again.select, again.max_level, again.box_min, again.box_max) == (ex.select, ex.max_level, ex.box_min, ex.box_max)


def test_packed_export_file(tmp_path):
    ex = octree("ragged_tiny")
    px = ex.pack()
    path = str(tmp_path / "ragged.simlodp")
    px.save(path)
    assert os.path.getsize(path) == 64 + 40 * ex.num_nodes + 8 * ex.num_samples
    back = PackedExport.load(path)
    assert back.packed.tobytes() == px.packed.tobytes() and back.nodes.tobytes() == px.nodes.tobytes()
    assert (back.select, back.max_level, back.box_min, back.box_max) == (px.select, px.max_level, px.box_min, px.box_max)
    assert back.unpack().samples.tobytes() == px.unpack().samples.tobytes()
    raw = open(path, "rb").read()
    assert raw[:8] == b"SIMLODP\0"

    def broken(data, what):
        bad = str(tmp_path / "bad.simlodp")
        with open(bad, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError):
            PackedExport.load(bad)
        return what

    broken(raw[:-8], "truncated")
    broken(raw[:40], "truncated header")
    broken(b"SIMLODX\0" + raw[8:], "the unpacked format's magic")
    broken(raw[:8] + (2).to_bytes(4, "little") + raw[12:], "version")
    t = np.frombuffer(raw[64: 64 + 40 * ex.num_nodes], dtype=abi.export_node_dtype).copy()
    t["firstSample"][1] += 1
    broken(raw[:64] + t.tobytes() + raw[64 + 40 * ex.num_nodes:], "bad table")
    t = np.frombuffer(raw[64: 64 + 40 * ex.num_nodes], dtype=abi.export_node_dtype).copy()
    t["parent"][1] = 5
    broken(raw[:64] + t.tobytes() + raw[64 + 40 * ex.num_nodes:], "bad table")
    # the unpacked format does not take a packed file either, and its own files are what they were
    with pytest.raises(ValueError):
        OctreeExport.load(path)
    from simlod_amd import octree_io
    assert octree_io.MAGIC == b"SIMLODX\0" and octree_io.VERSION == 1
