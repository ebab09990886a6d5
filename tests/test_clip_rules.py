"""CPU tier of the clip regions (include/simlod_hip.h, "clip regions"): simlod_amd/csrc/clip_rules.hpp — what the setter accepts, a node's class and
the action a mode asks for — checked on the host by a program of its own (tests/host/clip_rules_check.cpp, built with the address and undefined-
behaviour sanitizers) against octree_io.classify_nodes; the mirror of a clipped frame (tests/clip_ref.py) against what the region queries already
pin (OctreeExport.crop); the guard that a sample relocated to NaN does not exist for the oracle's rasteriser; octree_io.Clip and abi.clip_dtype."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import clip_ref
import region_ref
from simlod_amd import abi
from simlod_amd.octree_io import Clip, Region, classify_nodes
from util import node_keys, oracle_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["inside", "outside", "highlight"]
# rule C3's table: mode -> class -> action (clip_rules.hpp CLIP_ACT_*: 0 none, 1 keep passing, 2 keep failing, 3 colour passing, 4 colour all, 5 empty)
ACTIONS = {"off": {0: 0, 1: 0, 2: 0}, "inside": {0: 5, 1: 1, 2: 0}, "outside": {0: 0, 1: 2, 2: 5}, "highlight": {0: 0, 1: 3, 2: 4}}


def _nodes(rs, count):
    """(level, X, Y, Z) records: the root, every level, coordinates at both ends of their range and in between."""
    rec = np.zeros(count, dtype=[("level", "<u4"), ("X", "<u4"), ("Y", "<u4"), ("Z", "<u4")])
    rec["level"] = rs.randint(0, 21, size=count)
    for a in "XYZ":
        top = (1 << rec["level"].astype(np.int64))
        rec[a] = (rs.random_sample(count) * top).astype(np.int64).clip(0, top - 1)
        edge = rs.randint(0, 8, size=count)
        rec[a] = np.where(edge == 0, 0, np.where(edge == 1, top - 1, rec[a]))
    rec[0] = (0, 0, 0, 0)
    return rec


def _grazing(nodes, box_min, size):
    """Axis-aligned and oblique half-spaces whose boundary is a face (or a corner) of one of `nodes`, so that D_min / D_max come out at or next to 0
    with and without the inflation by one level-20 cell."""
    out = []
    e = size * 2.0 ** -20
    for nd in nodes:
        s = size / 2.0 ** int(nd["level"])
        lo = np.asarray(box_min, np.float64) + np.array([nd["X"], nd["Y"], nd["Z"]], np.float64) * s
        hi = lo + s
        for shift in (0.0, e, -e):
            out.append([[1.0, 0.0, 0.0, -(hi[0] + shift)]])                       # x >= the node's max face (inflated / deflated)
            out.append([[0.0, -1.0, 0.0, lo[1] + shift]])                         # y <= its min face
            n = np.array(region_ref.NORMAL)
            out.append([[*n, -float(n @ hi) - shift], [0.0, 0.0, 1.0, -(lo[2] - shift)]])      # through its far corner, and z >= its floor
    return out


def _case_file(path, box_min, box_max, clips, nodes):
    with open(path, "wb") as f:
        f.write(np.array([len(clips), len(nodes)], "<u4").tobytes())
        f.write(np.asarray(box_min, "<f4").tobytes() + np.asarray(box_max, "<f4").tobytes())
        f.write(np.concatenate(clips).tobytes())
        f.write(np.ascontiguousarray(nodes).tobytes())


def _bad_records():
    ok = Clip(Region.from_box((0.1, 0.2, 0.3), (0.5, 0.6, 0.7)), "inside").record()
    bad = []
    for edit in ("mode", "planes", "nan", "inf", "clip_reserved0", "clip_reserved1", "region_reserved"):
        r = ok.copy()
        if edit == "mode":
            r["mode"] = 4
        elif edit == "planes":
            r["region"]["numPlanes"] = 17
        elif edit == "nan":
            r["region"]["planes"][0, 3, 1] = np.nan
        elif edit == "inf":
            r["region"]["planes"][0, 0, 3] = np.inf
        elif edit == "clip_reserved0":
            r["reserved"][0, 0] = 1
        elif edit == "clip_reserved1":
            r["reserved"][0, 1] = 7
        else:
            r["region"]["reserved"][0, 2] = 1
        bad.append((edit, r))
    return ok, bad


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("clip_rules") / "clip_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "clip_rules_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("where", ["origin", "georef"])
def test_header_classifies_nodes_as_classify_nodes_does(checker, tmp_path, where):
    """A few thousand (level, X, Y, Z) x plane sets — the suite's regions, every mode, planes grazing node faces — on a unit box at the origin and on the
    600 x 400 x 40 box at cases.GEOREF: class and action from the header equal classify_nodes and rule C3's table; a refused record is refused."""
    rs = np.random.RandomState(5)
    box = (1.0, 1.0, 1.0) if where == "origin" else (600.0, 400.0, 40.0)
    mn = np.zeros(3, np.float32) if where == "origin" else np.asarray(cases.GEOREF, np.float32)
    mx = (mn + np.asarray(box, np.float32)).astype(np.float32)
    size = float((mx - mn).max())
    nodes = _nodes(rs, 1500)
    sets = [region_ref.region(k, box, mn.astype(np.float64)).planes for k in region_ref.REGION_NAMES] + _grazing(nodes[rs.choice(len(nodes), 12, replace=False)], mn, size)
    clips, want = [], []
    for j, planes in enumerate(sets):
        mode = (["off"] + MODES)[j % 4]
        region = Region(planes)
        clips.append(Clip(region, mode, color=0x00FF00).record())
        want.append((mode, region))
    ok, bad = _bad_records()
    clips += [r for _, r in bad]
    _case_file(tmp_path / "cases.bin", mn, mx, clips, nodes)
    run = subprocess.run([checker, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(len(clips), 1 + 2 * len(nodes))
    seen = set()
    for j, (mode, region) in enumerate(want):
        assert got[j, 0] == 1, f"set {j} refused"
        outside, inside = classify_nodes(region.planes.astype(np.float64), nodes, mn, mx)
        cls = np.where(outside, clip_ref.OUTSIDE, np.where(inside, clip_ref.COPIED, clip_ref.FILTERED))
        assert np.array_equal(got[j, 1::2], cls), f"set {j}: {int((got[j, 1::2] != cls).sum())} classes differ"
        assert np.array_equal(got[j, 2::2], np.array([ACTIONS[mode][c] for c in cls])), f"set {j} ({mode}): actions"
        seen |= set(cls.tolist())
    assert seen == {clip_ref.OUTSIDE, clip_ref.FILTERED, clip_ref.COPIED}
    for j, (edit, _) in enumerate(bad):
        assert got[len(want) + j, 0] == 0 and not got[len(want) + j, 1:].any(), f"a record with a bad {edit} was accepted"


@pytest.fixture(scope="module")
def host_tree():
    export, pts, box, ho = region_ref.host_octree("terrain_4x100k")
    u = cases.uniforms_for(box, cases.case("terrain_4x100k")[3])
    return export, box, ho, int(ho.stats["numNodes"][0]), int(ho.stats["allocatedBytes_persistent"][0]), u


@pytest.mark.parametrize("kind", region_ref.REGION_NAMES)
def test_mirror_agrees_with_the_region_query_mirror(built_libs, host_tree, kind):
    """On an oracle-built octree: what the INSIDE mirror keeps, node by node in chunk order, equals OctreeExport.crop(region, select="all"); the INSIDE
    and OUTSIDE mirrors partition every FILTERED node's samples; COPIED / OUTSIDE nodes are emptied in exactly one of the two modes."""
    export, box, ho, nn, used, u = host_tree
    nodes = ho.nodes
    region = region_ref.region(kind, box)
    ins = clip_ref.clip_image(nodes, ho.persistent, nn, Clip(region, "inside"), u, used)
    out = clip_ref.clip_image(nodes, ho.persistent, nn, Clip(region, "outside"), u, used)
    crop = export.crop(region, select="all")
    where = {int(k): t for t, k in enumerate(node_keys(crop.nodes))}
    has = (nodes["numPoints"][:nn] > 0) | (nodes["numVoxels"][:nn] > 0)
    compared = 0
    for i in np.nonzero(has)[0]:
        key = int(node_keys(nodes[i:i + 1])[0])
        kept_in, kept_out = clip_ref.kept_samples(ins, i), clip_ref.kept_samples(out, i)
        total = int(nodes["numPoints"][i]) + int(nodes["numVoxels"][i])
        cls = int(ins.cls[i])
        if cls == clip_ref.FILTERED:
            assert not ins.emptied[i] and not out.emptied[i]
            assert len(kept_in) + len(kept_out) == total, f"node {i}: the two mirrors do not partition its {total} samples"
            both = np.concatenate([kept_in, kept_out])
            region_ref.assert_same_multiset(both, np.concatenate([s for s, _ in ins.tested[int(i)]]), f"node {i}")
        else:
            assert bool(ins.emptied[i]) != bool(out.emptied[i]), f"node {i} (class {cls}) must be emptied in exactly one mode"
            assert bool(ins.emptied[i]) == (cls == clip_ref.OUTSIDE)
        # against the region query's mirror: a node the crop lists holds exactly what the INSIDE mirror kept, in order
        if key in where:
            t = where[key]
            a = int(crop.nodes["firstSample"][t])
            want = crop.samples[a: a + int(crop.nodes["numSamples"][t])]
            got = kept_in if not ins.emptied[i] else kept_in[:0]
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"node {i}: INSIDE keeps {len(got)} samples, crop {len(want)}"
            compared += len(want)
        else:
            assert ins.emptied[i] or len(kept_in) == 0, f"node {i} is not in the crop but the INSIDE mirror keeps {len(kept_in)} samples"
    assert compared == crop.num_samples
    if kind in ("oblique", "slab", "box"):
        assert compared > 0 and any(ins.cls[i] == clip_ref.FILTERED for i in np.nonzero(has)[0])


@pytest.mark.parametrize("name", ["terrain_4x100k", "uniform_3x40k"])
@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
def test_a_sample_at_nan_does_not_exist_for_the_oracle(built_libs, name, hqs):
    """The mirror removes a sample by relocating it to NaN: with EVERY sample there the oracle draws 0 pixels while the nodes stay visible."""
    _, pts, box, ho = region_ref.host_octree(name)
    nn = int(ho.stats["numNodes"][0])
    u = cases.uniforms_for(box, cases.case(name)[3], hqs=hqs)
    fb0, _, st0, _ = oracle_frame(ho.nodes, nn, u)
    assert int((fb0 != abi.CLEAR_PIXEL).sum()) > 2000
    n2, p2 = clip_ref.all_samples_to_nan(ho.nodes, ho.persistent, nn, int(ho.stats["allocatedBytes_persistent"][0]))
    fb, _, st, _ = oracle_frame(n2, nn, u)
    assert int((fb != abi.CLEAR_PIXEL).sum()) == 0
    for f in ("numVisibleNodes", "numVisiblePoints", "numVisibleVoxels"):
        assert int(st[f]) == int(st0[f]), f
    assert int(st["numVisibleNodes"]) > 0 and int(st["numVisiblePoints"]) + int(st["numVisibleVoxels"]) > 0


def test_clip_validates_as_the_c_call_does():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodClip\) == (\d+)", src).group(1)) == abi.clip_dtype.itemsize == 288
    assert int(re.search(r"offsetof\(SimlodClip, region\) == (\d+)", src).group(1)) == abi.clip_dtype.fields["region"][1] == 16
    for name, value in (("OFF", 0), ("INSIDE", 1), ("OUTSIDE", 2), ("HIGHLIGHT", 3)):
        assert int(re.search(rf"#define SIMLOD_CLIP_{name}\s+(\d+)u", src).group(1)) == abi.CLIP_MODES[name.lower()] == value
    r = Clip(Region.from_planes([[1, 2, 3, 4]]), "highlight", 0xFF00FF).record()
    assert r.dtype == abi.clip_dtype and int(r["mode"][0]) == 3 and int(r["color"][0]) == 0xFF00FF and not r["reserved"].any()
    assert int(r["region"]["numPlanes"][0]) == 1 and r["region"]["planes"][0, 0].tolist() == [1, 2, 3, 4]
    assert int(Clip(Region(), "off").record()["mode"][0]) == 0
    assert int(Clip([[0, 0, 1, 0]]).record()["mode"][0]) == 1                      # (planes in the place of a Region; mode "inside" by default)
    with pytest.raises(ValueError):
        Clip(Region(), "sideways")
    with pytest.raises(ValueError):
        Clip(Region(), 1)
    with pytest.raises(ValueError):
        Clip(np.zeros((17, 4)))
    with pytest.raises(ValueError):
        Clip([[np.nan, 0, 0, 0]])
    with pytest.raises(ValueError):
        Clip([[1e39, 0, 0, 0]])                                                    # (not finite as float32)
    with pytest.raises(ValueError):
        Clip(Region(), "highlight", color=1 << 32)
    with pytest.raises(ValueError):
        Clip(Region(), "highlight", color=-1)


def test_library_exports_the_clip_calls(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_context_set_clip", "simlod_set_clip"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    # the setter does no device work: it validates and stores, with or without a GPU (the default context here)
    ok, bad = _bad_records()
    import ctypes
    assert L.simlod_set_clip(ctypes.c_void_p(ok.ctypes.data)) == 0
    for edit, r in bad:
        assert L.simlod_set_clip(ctypes.c_void_p(r.ctypes.data)) == 1, edit         # hipErrorInvalidValue
    assert L.simlod_set_clip(None) == 0
