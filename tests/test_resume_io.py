"""CPU tier: the grid rebuild of simlod_import_octree_buildable as tests/resume_ref.py restates it, against the grids of octrees the oracle built
(byte for byte, every node that has one), and the host-side buildability checks of simlod_amd/octree_io.py."""
import numpy as np
import pytest

import cases
import oracle
from export_ref import export_host, keys_of
from resume_ref import grid_of_image, rebuild_grids, root_leaf_voxels
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import OctreeExport


def _oracle(pts, box, batches, box_min=(0.0, 0.0, 0.0)):
    T = cases._cam(box)
    u = cases.uniforms_for(box, T, box_min=box_min)
    ref = oracle.HostOctree("port", persistent_bytes=1 << 30, ring_slots=abi.BATCH_STREAM_SIZE)
    ref.reset(u)
    for b in batches:
        ref.upload(b)
        ref.construct(u)
        assert ref.last_error() == 0
    while int(ref.stats["batchletIndex"][0]) < int(ref.num_uploaded[0]):
        ref.construct(u)
    return ref, u


def _max_face():
    pts, box = synthetic.uniform_cube(60_000, seed=21)
    pts["x"][:500] = box[0]                 # exactly on the max face: quantised to 2^28, filed under cell 0 / node coordinate 0
    pts["y"][250:900] = box[1]
    pts["z"][700:1200] = box[2]
    return pts, box, [pts[i:i + 20_000] for i in range(0, len(pts), 20_000)]


def _input(name):
    if name == "terrain_2m":
        pts, box = synthetic.terrain(2_000_000, seed=8, box=(1200.0, 800.0, 60.0), tile=50.0)
        return pts, box, [pts[i:i + 500_000] for i in range(0, len(pts), 500_000)]
    if name == "hotspot_600k":
        pts, box = synthetic.hotspot(600_000, seed=12, level=4, cell=(9, 3, 12))
        return pts, box, [pts[i:i + 200_000] for i in range(0, len(pts), 200_000)]
    if name == "max_face":
        return _max_face()
    if name == "ragged_tiny_root_leaf":         # the batches before the root splits (50 000 points)
        pts, box, _, _ = cases.case("ragged_tiny")
        return pts, box, cases.batches_of("ragged_tiny", pts, None)[:4]
    pts, box, batch, _ = cases.case(name)
    return pts, box, cases.batches_of(name, pts, batch)


# "<input>@<offset>": the input moved into a box off the origin (cases.offset_of)
NAMES = cases.CASES + ["terrain_2m", "hotspot_600k", "max_face", "ragged_tiny_root_leaf", "terrain_4x100k@georef", "uniform_3x40k@inexact", "max_face@dyadic",
                       "ragged_tiny_root_leaf@inexact"]


def _built(name):
    name, _, offset = name.partition("@")
    pts, box, batches = _input(name)
    box_min = (0.0, 0.0, 0.0)
    if offset:
        off = cases.offset_of(offset, box)
        cuts = np.cumsum([0] + [len(b) for b in batches])
        pts = np.concatenate([cases.shift_points(pts[: cuts[-1]], off), pts[cuts[-1]:]])
        batches, box_min = [pts[a:b] for a, b in zip(cuts[:-1], cuts[1:])], tuple(float(np.float32(v)) for v in off)
    ref, u = _oracle(pts, box, batches, box_min)
    nn = int(ref.stats["numNodes"][0])
    t, s = export_host(ref.nodes, nn)
    return ref, u, nn, t, s, pts


@pytest.mark.parametrize("name", NAMES)
def test_rebuilt_grids_equal_the_oracles(name):
    ref, u, nn, t, s, pts = _built(name)
    grids = rebuild_grids(t, s, u)
    where = {int(k): i for i, k in enumerate(keys_of(t))}
    d = oracle.dump_image(ref.nodes, nn)
    with_grid = np.nonzero(ref.nodes["grid"][:nn] != 0)[0]
    assert len(with_grid) == len(grids) and len(grids) >= 1
    for i in with_grid:
        nd = ref.nodes[i]
        key = (int(nd["level"]) << 60) | (int(nd["X"]) << 40) | (int(nd["Y"]) << 20) | int(nd["Z"])
        got = grids[where[key]]
        want = grid_of_image(ref.nodes, i, ref.persistent)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{name}: node level={int(nd['level'])} XYZ=({int(nd['X'])},{int(nd['Y'])},{int(nd['Z'])}): {len(bad)} grid words differ, "
                                 f"first word {int(bad[0])}: {int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}")
    if name.startswith("max_face"):
        assert (pts["x"] == pts["x"].max()).sum() >= 500          # (the input really has points on the max face)
        assert pts["x"].max() == np.asarray(u["boxMax"], np.float32).reshape(3)[0]
    if "@" in name:
        # the case can tell "honours boxMin" from "ignores it": rebuilt in the box [0, boxMax] the grids are others
        other = rebuild_grids(t, s, cases.origin_box_uniforms(u))
        assert any(not np.array_equal(other.get(k), g) for k, g in grids.items())
    if t[0]["childMask"] == 0:
        # a root that is still a leaf: its voxels are rebuilt with the oracle root's cells and bit-equal positions
        cells, vox = root_leaf_voxels(t, s, u)
        nv = int(ref.nodes[0]["numVoxelsStored"])
        have = oracle.gather_samples(int(ref.nodes[0]["voxelChunks"]), nv)
        assert len(vox) == nv == int(d["gridPopcount"][0])
        key = lambda v: np.sort(np.stack([v["x"], v["y"], v["z"]], axis=1).view(np.uint32).copy().view(np.dtype((np.void, 12))).reshape(-1))
        assert np.array_equal(key(vox), key(have)), f"{name}: rebuilt root voxel positions differ from the oracle's"
        assert np.all(np.diff(cells) > 0)
        # colour: a point of the root's (the cell's lowest-index one: tests/test_gpu_resume.py pins the device to it)
        f, n = int(t[0]["firstSample"]), int(t[0]["numSamples"])
        assert set(vox["color"].tolist()) <= set(s[f: f + n]["color"].tolist())


def test_ragged_tiny_cuts_cover_both_root_states():
    a = _built("ragged_tiny_root_leaf")[3]
    b = _built("ragged_tiny")[3]
    assert a[0]["childMask"] == 0 and b[0]["childMask"] == 0xFF


def _full_export():
    ref, u, nn, t, s, pts = _built("uniform_3x40k")
    box_max = np.asarray(np.asarray(u).reshape(-1)[0]["boxMax"], np.float32)
    return OctreeExport(t, s, (0, 0, 0), box_max, 20, "all")


def _with(ex, table=None, max_level=None, select=None):
    return OctreeExport(ex.nodes.copy() if table is None else table, ex.samples, ex.box_min, ex.box_max,
                        ex.max_level if max_level is None else max_level, ex.select if select is None else select)


def test_validate_buildable_accepts_a_full_export():
    ex = _full_export()
    assert ex.validate(buildable=True) is ex and ex.is_buildable


@pytest.mark.parametrize("what", ["max_level", "cut", "visible", "leaf_flag", "seven_children", "unselected"])
def test_validate_buildable_rejects(what):
    ex = _full_export()
    t = ex.nodes.copy()
    inner = np.nonzero(t["childMask"] != 0)[0]
    leaves = np.nonzero(t["childMask"] == 0)[0]
    if what == "max_level":
        bad = _with(ex, max_level=4)
    elif what in ("cut", "visible"):
        bad = _with(ex, select=what)
    elif what == "leaf_flag":
        t["flags"][leaves[0]] &= ~np.uint8(abi.EXPORT_FLAG_LEAF)
        bad = _with(ex, t)
    elif what == "seven_children":
        # the last child of the last inner node dropped: a well-formed table (validate() passes) whose node has seven children
        p = int(inner[-1])
        last = int(t["firstChild"][p]) + 7
        assert last == len(t) - 1 and t["childMask"][last] == 0
        t = t[:-1].copy()
        t["childMask"][p] = 0x7F
        s = ex.samples[: int(t["firstSample"][-1]) + int(t["numSamples"][-1])]
        bad = OctreeExport(t, s, ex.box_min, ex.box_max, 20, "all")
        bad.validate()
    else:
        t["flags"][leaves[1]] &= ~np.uint8(abi.EXPORT_FLAG_SELECTED)
        t["numSamples"][leaves[1]] = 0
        t["firstSample"] = np.concatenate([[0], np.cumsum(t["numSamples"].astype(np.uint64))[:-1]])
        keep = np.ones(ex.num_samples, bool)
        f, n = int(ex.nodes["firstSample"][leaves[1]]), int(ex.nodes["numSamples"][leaves[1]])
        keep[f: f + n] = False
        bad = OctreeExport(t, ex.samples[keep], ex.box_min, ex.box_max, 20, "all")
        bad.validate()
    assert not bad.is_buildable
    with pytest.raises(ValueError):
        bad.validate(buildable=True)


def test_buildable_survives_save_load(tmp_path):
    _save_load(_full_export(), tmp_path)


def test_buildable_survives_save_load_in_a_box_off_the_origin(tmp_path):
    ref, u, nn, t, s, pts = _built("uniform_3x40k@inexact")
    u0 = np.asarray(u).reshape(-1)[0]
    ex = OctreeExport(t, s, u0["boxMin"], u0["boxMax"], 20, "all")
    assert ex.box_min == tuple(float(np.float32(v)) for v in cases.INEXACT_UNIT)
    _save_load(ex, tmp_path)


def _save_load(ex, tmp_path):
    ex.save(tmp_path / "full.simlodx")
    ld = OctreeExport.load(tmp_path / "full.simlodx")
    assert ld.is_buildable and ld.nodes.tobytes() == ex.nodes.tobytes() and ld.samples.tobytes() == ex.samples.tobytes()
    assert ld.box_min == ex.box_min and ld.box_max == ex.box_max
    cut = _with(ex, select="cut")
    cut.save(tmp_path / "cut.simlodx")
    assert not OctreeExport.load(tmp_path / "cut.simlodx").is_buildable
