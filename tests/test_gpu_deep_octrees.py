"""GPU tier: export, import, buildable import, resumed ingest, the region, ray, neighbour and footprint queries and clip regions on octrees 13
and 20 levels deep (tests/deep_ref.py), where every suite before this one stopped at about level 4.  The device octrees are built once per
module; each test asserts its precondition from the oracle, the mirrors and brute force (tests/test_deep_io.py states them on the CPU) and
then compares: export == the host restatement on the downloaded image == the oracle's export; import == source; resume == the continuous
build; queries == the mirror on the device's own export == brute force over the raw input (footprints: footprint_ref.contains_exact, rule F1
with exact signs); clipped frames == the oracle's rasteriser on the image edited by tests/clip_ref.py.  All comparisons are equalities, but
for the RGBA8 of a frame after EDL (within 1 per channel, util.assert_frame_equals_oracle)."""
import numpy as np
import pytest

import cases
import clip_ref
import deep_ref as dr
import footprint_ref as fr
import neighbours_ref as nr
import oracle
import rays_ref as yr
import region_ref as rr
import test_gpu_clip as on_clips
import test_gpu_footprint as on_footprints
import test_gpu_neighbours as on_spheres
import test_gpu_rays as on_rays
import test_gpu_region as on_regions
from simlod_amd import abi
from simlod_amd.octree_io import Clip, OctreeExport, Region
from test_gpu_export import _assert_export, _device, _frames_equal, _host_export
from test_gpu_resume import (RESUME_FIELDS, _assert_fields, _assert_stats, _check_import, _export_through_file, _feed, _import,
                             _resume_batches)
from util import assert_frame_equals_oracle, assert_stats_equal, host_image_of, node_keys

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
NONE = abi.EXPORT_NONE
_DEV, _MIRROR = {}, {}


def _close_cam(d):
    return dr.close_cam(d, W, H)


def _frame_floor(name):
    """D13 and D13x fill one level-11 cell, 1 / 2048 of their box: the cases' camera draws them into a single pixel (tests/test_deep_io.py)."""
    return 1000 if name == "d20" else 0


class Built:
    def __init__(self, name):
        self.d = d = dr.built(name)
        self.dev = _device()
        self.u = self.dev.uniforms(W, H, cases._cam(d.box), d.box)
        self.dev.reset(self.u)
        _feed(self.dev, self.u, d.batches)
        assert int(self.dev.read_stats()["dbg"]) == 0
        self.full = self.dev.export_octree(self.u)


def _built(name):
    if name not in _DEV:
        _DEV[name] = Built(name)
    return _DEV[name]


@pytest.fixture(scope="module", autouse=True)
def _release(built_libs):
    yield
    _DEV.clear()
    _MIRROR.clear()
    for cache in (on_clips._MIRRORS, on_clips._UNCLIPPED):          # the clipped images of this module's octrees
        for k in [k for k in cache if k[0][0].startswith(("d13x", "d20"))]:
            del cache[k]


def _assert_shape(name, export, what):
    d = dr.built(name)
    if name.startswith("d13"):
        dr.assert_d13_shape(export, what)
    else:
        dr.assert_d20_shape(export, d.k, what)


def _per_node(ex, leaves):
    """The samples of the leaves (16 bytes each) or of the inner nodes (positions only: which point coloured a voxel depends on the launch)
    in sorted order within each node."""
    t = ex.nodes
    owner = np.repeat(np.arange(len(t)), t["numSamples"].astype(np.int64))
    pick = (t["childMask"][owner] == 0) == leaves
    w = ex.samples.view(np.uint32).reshape(-1, 4)[pick]
    if not leaves:
        w = w[:, :3]
    cols = [w[:, c] for c in range(w.shape[1] - 1, -1, -1)] + [owner[pick]]
    return w[np.lexsort(cols)]


# ---- 1. export -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d13", "d13x", "d20"])
def test_export_equals_the_host_restatement_and_the_oracles(built_libs, name):
    b = _built(name)
    d, dev, u = b.d, b.dev, b.u
    _assert_shape(name, d.export, f"{name} (oracle)")
    t, s = _host_export(dev)
    _assert_export(b.full, t, s, f"{name} all@20")
    _assert_shape(name, b.full, f"{name} (device)")
    b.full.validate(buildable=True)
    for ml in ((12, 13) if name.startswith("d13") else (19, 20)):
        for sel in ("all", "cut"):
            t, s = _host_export(dev, ml, abi.EXPORT_SELECT[sel])
            ex = dev.export_octree(u, max_level=ml, select=sel)
            _assert_export(ex, t, s, f"{name} {sel}@{ml}")
            cut = b.full.truncated(ml, sel)
            assert ex.nodes.tobytes() == cut.nodes.tobytes() and ex.samples.tobytes() == cut.samples.tobytes(), f"{name} {sel}@{ml}: not the full export's cut"
            assert int(ex.nodes["level"].max()) == ml
    # the oracle's export (D20: with the k samples its level-20 leaf counted put in): the table byte for byte, every leaf's samples as a multiset,
    # every inner node's voxel positions as a multiset
    assert b.full.nodes.tobytes() == d.export.nodes.tobytes(), f"{name}: the table differs from the oracle's"
    for leaves in (True, False):
        assert np.array_equal(_per_node(b.full, leaves), _per_node(d.export, leaves)), f"{name}: samples differ from the oracle's (leaves={leaves})"


@pytest.mark.parametrize("name", ["d13x", "d20"])
def test_export_of_the_visible_nodes_after_a_frame(built_libs, name):
    b = _built(name)
    d, dev = b.d, b.dev
    u = dev.uniforms(W, H, _close_cam(d) if name == "d13x" else cases._cam(d.box), d.box)
    dev.render(u)
    nodes, pers, nn = host_image_of(dev)
    _, _, st, vis = assert_frame_equals_oracle(dev, nodes, nn, u, f"{name} close-up", 1000)
    if name == "d13x":
        assert int((vis["level"] == dr.LEAF_LEVEL).sum()) >= 8, "the oracle chooses fewer than eight level-13 nodes"
    ex = dev.export_octree(u, select="visible")
    t, s = _host_export(dev, 20, abi.EXPORT_VISIBLE)
    _assert_export(ex, t, s, f"{name} visible")
    sel = ex.nodes[(ex.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0]
    assert len(sel) == len(vis) and int(ex.nodes["numSamples"].sum()) == int(st["numVisiblePoints"]) + int(st["numVisibleVoxels"])
    if name == "d13x":
        assert int((sel["level"] == dr.LEAF_LEVEL).sum()) >= 8


# ---- 2. plain import through a file ----------------------------------------------------------------------------------------------------------
def _through_file(ex, tmp_path):
    ex.save(tmp_path / "deep.simlodx")
    return OctreeExport.load(tmp_path / "deep.simlodx")


@pytest.mark.parametrize("name", ["d13", "d13x", "d20"])
def test_plain_import_through_a_file(built_libs, tmp_path, name):
    b = _built(name)
    d, src, u = b.d, b.dev, b.u
    _assert_shape(name, d.export, f"{name} (oracle)")
    ld = _through_file(b.full, tmp_path)
    dst = _device()
    dst.nodes.fill_(0xA5)
    dst.import_octree(ld)
    assert int(dst.read_stats()["dbg"]) == 0
    re = dst.export_octree(u)
    assert re.nodes.tobytes() == b.full.nodes.tobytes() and re.samples.tobytes() == b.full.samples.tobytes(), f"{name}: the re-export differs"
    _frames_equal(src, dst, u, name, _frame_floor(name))
    if name == "d13x":
        close = dst.uniforms(W, H, _close_cam(d), d.box)
        _frames_equal(src, dst, close, f"{name} close-up")
        nodes, pers, nn = host_image_of(dst)
        for hqs in (0, 1):
            close["useHighQualityShading"] = hqs
            dst.render(close)
            _, _, _, vis = assert_frame_equals_oracle(dst, nodes, nn, close, f"{name} close-up hqs={hqs}", 1000)
            assert int((vis["level"] == dr.LEAF_LEVEL).sum()) >= 8, "the oracle chooses fewer than eight level-13 nodes"
    # the queries once on the imported copy: what the source returns (the mirror on the one export both have)
    _query_once(name, dst, u, b.full, f"{name} imported")


# ---- 3. buildable import ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d13", "d13x", "d20"])
def test_buildable_import_rebuilds_the_grids_of_every_level(built_libs, tmp_path, name):
    """D13 / D13x exported after batch B (64 leaves at level 13, grids at levels 0 .. 12), D20 after its third batch: twenty inner nodes, one
    per level 0 .. 19 — run_import's deepest == MAX_DEPTH - 1 == numInner - 1, both bounds tight at once."""
    d = dr.built(name)
    cut = 2 if name.startswith("d13") else 3
    src = _device()
    T = _close_cam(d) if name == "d13x" else cases._cam(d.box)
    u = src.uniforms(W, H, T, d.box)
    src.reset(u)
    _feed(src, u, d.batches[:cut])
    ex, ld = _export_through_file(src, u, tmp_path)
    inner = ex.nodes[ex.nodes["childMask"] != 0]
    if name == "d20":
        _assert_shape(name, d.export, "d20 (oracle)")
        assert ex.nodes.tobytes() == d.export.nodes.tobytes()
        assert sorted(inner["level"].tolist()) == list(range(abi.MAX_DEPTH)), "one inner node per level 0 .. 19"
    else:
        assert sorted(inner["level"].tolist()) == list(range(12)) + [12] * 8
    dst = _device()
    uu = _import(dst, ld, u)
    _check_import(src, dst, ex, uu, f"{name} buildable", 1000 if name != "d13" else 0)
    nodes, pers, nn = host_image_of(dst)
    assert sorted(nodes["level"][:nn][nodes["grid"][:nn] != 0].tolist()) == sorted(inner["level"].tolist()), "a grid per inner node, no other"


# ---- 4. resume -------------------------------------------------------------------------------------------------------------------------------
def _feed_one_group(dev, u, batches):
    """All batches uploaded, then ONE launch that takes them as one exact group."""
    dev.groups_ingested(zero=True)
    dev.set_batch_limit(len(batches))
    for b in batches:
        dev.upload(b)
    dev.construct(u)
    assert dev.processed() == len(batches) and dev.groups_ingested() == 1 and dev.group_size() == len(batches), "not one group"


def _feed_one_by_one(dev, u, batches):
    dev.groups_ingested(zero=True)
    _feed(dev, u, batches)
    assert dev.groups_ingested() == len(batches)


@pytest.mark.parametrize("mode", ["batch_by_batch", "one_group"])
@pytest.mark.parametrize("name", ["d13", "d13x"])
def test_resume_at_level_13_equals_the_oracles_continuous_build(built_libs, tmp_path, name, mode):
    """Import after B, feed C and D: k_begin rebuilds the continued ancestor-path rows of the level-13 leaves (the import keeps no side table)
    before k_voxelize's piece path (C) and small-item path (D) read them."""
    d = dr.built(name)
    dr.assert_d13_shape(d.export, f"{name} (oracle)")
    dr.assert_input_arithmetic(d.counts)
    dst = _device()
    dst.tune("SIMLOD_EXACT_GROUP", 1 if mode == "batch_by_batch" else 2)
    dst, uu, _ = _resume_batches(f"{name} {mode}", d.box, d.batches, 2, tmp_path, dst=dst, check_import=False,
                                 feed=_feed_one_by_one if mode == "batch_by_batch" else _feed_one_group)
    if mode == "one_group":
        _query_once(name, dst, uu, dst.export_octree(uu), f"{name} resumed")


def test_resume_into_the_level_20_leaf(built_libs, tmp_path):
    """D20 imported after its third batch (the level-20 leaf: 70 chunks linked by the import), then 5 000 more identical points and 5 000
    uniform ones: k_insert appends through the head chunk's tail word.  Node for node the continuous DEVICE build, the oracle's continuous
    build for every node above level 20, and the leaf: the oracle's count, that many copies of the point, ceil(n / 1000) chunks."""
    d = dr.built("d20r")
    dr.assert_d20_shape(d.export, d.k, "d20r (oracle)")
    assert d.k == 75_000 and dr.built("d20").k == 70_000
    src = _device()
    u = src.uniforms(W, H, cases._cam(d.box), d.box)
    src.reset(u)
    _feed(src, u, d.batches[:3])
    ex, ld = _export_through_file(src, u, tmp_path)
    assert dr.deep_entry(ex) == (dr.deep_entry(dr.built("d20").export)[0], 70_000)
    dst = _device()
    uu = _import(dst, ld, u)
    _feed(dst, uu, d.batches[3:])
    _feed(src, u, d.batches[3:])                                  # the continuous build: the source simply goes on
    st, sc = dst.read_stats(), src.read_stats()
    assert int(st["dbg"]) == 0 and int(sc["dbg"]) == 0 and int(st["batchletIndex"]) == 1 and int(st["numPointsProcessed"]) == len(d.batches[3])
    _assert_stats(st, sc, "d20 resume vs the continuous device build")
    assert_stats_equal(st, d.ho.stats[0], ["numNodes", "numInner", "numLeaves", "numNonemptyLeaves", "numPoints", "numVoxels", "numChunksVoxels"], "d20 resume vs oracle")
    nodes, pers, nn = host_image_of(dst)
    nodes_c, pers_c, nc = host_image_of(src)
    got, cont, want = oracle.dump_image(nodes, nn), oracle.dump_image(nodes_c, nc), d.ho.dump()
    _assert_fields(got, cont, RESUME_FIELDS, "d20 resume vs the continuous device build")
    oracle.check_invariants(nodes, nn)
    got, want = got[np.argsort(got["key"], kind="stable")], want[np.argsort(want["key"], kind="stable")]
    shallow = want["level"] < abi.MAX_DEPTH
    assert np.array_equal(got["level"], want["level"]) and int((~shallow).sum()) == 8
    _assert_fields(got[shallow], want[shallow], RESUME_FIELDS, "d20 resume vs the oracle above level 20")
    for f in ("numPoints", "numVoxels", "isLeaf", "childMask", "X", "Y", "Z"):
        assert np.array_equal(got[f][~shallow], want[f][~shallow]), f
    leaf = ~shallow & (got["numPoints"] > 0)
    assert int(leaf.sum()) == 1 and int(got["numPoints"][leaf][0]) == d.k and int(got["pointChunks"][leaf][0]) == -(-d.k // abi.POINTS_PER_CHUNK)
    re = dst.export_octree(uu)
    e, n = dr.deep_entry(re)
    f = int(re.nodes["firstSample"][e])
    assert n == d.k and re.samples[f: f + n].tobytes() == d.same[:n].tobytes(), "the leaf's samples are not k copies of the point"
    assert re.nodes.tobytes() == d.export.nodes.tobytes()
    assert np.array_equal(_per_node(re, True), _per_node(d.export, True))
    _query_once("d20r", dst, uu, re, "d20 resumed")


# ---- 5. queries ------------------------------------------------------------------------------------------------------------------------------
def _mirror(key, fn):
    if key not in _MIRROR:
        _MIRROR[key] = fn()
    return _MIRROR[key]


def _count_fields(c):
    return {f: int(c[f]) for f in c.dtype.names}


def _assert_rays(dev, u, full, rays, sel, what, key=None, ml=20):
    want = _mirror(key, lambda: full.cast(rays, ml, sel, return_counts=True)) if key else full.cast(rays, ml, sel, return_counts=True)
    raw = on_rays.Raw(dev, u, rays, ml, sel)
    on_rays._assert_matches(raw, want[0], want[1], what, full.truncated(ml, sel))
    only = on_rays.Raw(dev, u, rays, ml, sel, count_only=True)
    assert only.rc == 0 and _count_fields(only.counts) == _count_fields(want[1]), f"{what}: the count-only call"
    return raw.hits(), want[1]


def _assert_spheres(dev, u, full, q, k, sel, what, key=None, ml=20):
    want = _mirror(key, lambda: full.neighbours(q, k, ml, sel, return_counts=True)) if key else full.neighbours(q, k, ml, sel, return_counts=True)
    raw = on_spheres.Raw(dev, u, q, k, ml, sel)
    on_spheres._assert_matches(raw, want, what, full.truncated(ml, sel))
    only = on_spheres.Raw(dev, u, q, k, ml, sel, count_only=True)
    fields = on_spheres.COUNT_FIELDS
    assert only.rc == 0 and all(int(only.counts[f]) == int(want[2][f]) for f in fields[:6]) and int(only.counts["numFound"]) == 0, f"{what}: the count-only call"
    return raw.neighbours(), raw.within()


def _assert_region(dev, u, full, region, sel, what):
    mirror, cnt = full.crop(region, 20, sel, return_counts=True)
    raw = on_regions.Raw(dev, u, region, 20, sel)
    on_regions._assert_matches(raw, mirror, cnt, what)
    only = on_regions.Raw(dev, u, region, 20, sel, count_only=True)
    assert only.rc == 0 and _count_fields(only.counts) == _count_fields(cnt), f"{what}: the count-only call"
    return mirror


def _assert_footprint(dev, u, full, footprint, sel, what, region=None, ml=20):
    mirror, cnt = full.crop(Region() if region is None else region, ml, sel, return_counts=True, footprint=footprint)
    raw = on_footprints.Raw(dev, u, footprint, region, ml, sel)
    on_footprints._assert_matches(raw, mirror, cnt, what)
    only = on_footprints.Raw(dev, u, footprint, region, ml, sel, count_only=True)
    assert only.rc == 0 and _count_fields(only.counts) == _count_fields(cnt), f"{what}: the count-only call"
    return mirror


def _deep_samples(mirror):
    """The level-20 entries of a crop that hold samples."""
    return mirror.nodes[(mirror.nodes["level"] == abi.MAX_DEPTH) & (mirror.nodes["numSamples"] > 0)]


def _query_once(name, dev, u, full, what):
    """One ray set, one sphere set and one footprint on another device object that holds the octree `full` was exported from."""
    if name.startswith("d13"):
        d = dr.built(name)
        _assert_rays(dev, u, full, dr.d13_rays(d)["thin"][0], "cut", f"{what} thin rays")
        _assert_spheres(dev, u, full, dr.d13_spheres(d)["r-15"], dr.SPHERE_K, "cut", f"{what} spheres")
        mirror = _assert_footprint(dev, u, full, dr.d13_footprints(d)["cell12"], "cut", f"{what} footprint")
        assert 0 < mirror.num_samples < full.truncated(20, "cut").num_samples
    else:
        e, n = dr.deep_entry(full)
        hits, _ = _assert_rays(dev, u, full, dr.d20_rays()[0], "cut", f"{what} rays")
        assert (hits["node"][:-1] == e).all() and (hits["ordinal"][:-1] == 0).all()
        nb, within = _assert_spheres(dev, u, full, dr.d20_spheres(), dr.SPHERE_K, "cut", f"{what} spheres")
        assert (nb["node"] == e).all() and within[0] == n
        deep = _deep_samples(_assert_footprint(dev, u, full, dr.d20_footprints()["lo_x=x"][0], "cut", f"{what} footprint"))
        assert len(deep) == 1 and int(deep["numSamples"][0]) == n


@pytest.mark.parametrize("name", ["d13", "d13x"])
def test_rays_into_level_13(built_libs, name):
    b = _built(name)
    d, cut = b.d, b.d.export.truncated(20, "cut")
    for key, (rays, cone) in dr.d13_rays(d).items():
        hits, passing = _mirror((name, "oracle rays", key), lambda: d.export.cast(rays, 20, "cut", return_passing=True))
        yr.assert_not_vacuous(hits, False, f"{name} {key}", passing, cone)
        dr.assert_hits_at_level(hits, cut.nodes, dr.LEAF_LEVEL, f"{name} {key}")
        for sel in ("cut", "all"):
            got, _ = _assert_rays(b.dev, b.u, b.full, rays, sel, f"{name} {key} {sel}", key=(name, "rays", key, sel))
            if sel == "cut" and not cone:
                yr.assert_hits_are_brute(got, rays, d.pts, f"{name} {key}")
                assert got["t"].tobytes() == hits["t"].tobytes()


@pytest.mark.parametrize("name", ["d13", "d13x"])
def test_spheres_into_level_13(built_libs, name):
    b = _built(name)
    d = b.d
    sets = dr.d13_spheres(d)
    oracle_within = {key: _mirror((name, "oracle spheres", key), lambda: d.export.neighbours(q, dr.SPHERE_K, 20, "cut"))[1] for key, q in sets.items()}
    dr.assert_spheres_not_vacuous(oracle_within, name)
    for key, q in sets.items():
        for sel, k in (("cut", dr.SPHERE_K), ("all", dr.SPHERE_K), ("cut", 1)):
            nb, within = _assert_spheres(b.dev, b.u, b.full, q, k, sel, f"{name} {key} k={k} {sel}", key=(name, "spheres", key, k, sel))
            if (sel, k, key) == ("cut", dr.SPHERE_K, "r-17") or (sel, k, key) == ("cut", dr.SPHERE_K, "r-15"):
                nr.assert_found_are_brute(nb, within, q, d.pts, k, f"{name} {key}")


def test_regions_across_level_13(built_libs):
    b = _built("d13")
    d = b.d
    for key, region in dr.d13_regions(d).items():
        dr.assert_region_not_vacuous(d.export, region, dr.LEAF_LEVEL, key)
        mirror = _assert_region(b.dev, b.u, b.full, region, "cut", f"d13 {key} cut")
        rr.assert_same_multiset(mirror.samples, d.pts[rr.brute_mask(region, d.pts)], key)
        _assert_region(b.dev, b.u, b.full, region, "all", f"d13 {key} all")


def test_rays_through_the_level_20_leaf(built_libs):
    b = _built("d20")
    d = b.d
    dr.assert_d20_shape(d.export, d.k, "d20 (oracle)")
    e, k = dr.deep_entry(b.full)
    rays, miss = dr.d20_rays()
    through = np.arange(len(rays)) != miss
    for sel in ("cut", "all"):
        hits, cnt = _assert_rays(b.dev, b.u, b.full, rays, sel, f"d20 rays {sel}", key=("d20", "rays", sel))
        assert int(cnt["numHits"]) >= len(rays) - 1 and (hits["t"][through & (rays.record()["radius"] == 0)] == 0.25).all()
        if sel == "cut":
            # 70 000 exact ties in (t, node, ordinal): the first of them, and for the count-only call a first passing sample in a 70-chunk node
            assert (hits["node"][through] == e).all() and (hits["ordinal"][through] == 0).all() and hits["node"][miss] != e
            yr.assert_hits_are_brute(hits, rays, d.pts, "d20 rays")
    for ml in (19, 20):
        _assert_rays(b.dev, b.u, b.full, rays, "all", f"d20 rays all@{ml}", ml=ml)
    # more rays through the one node than a workgroup takes
    many = dr.d20_many_rays()
    assert len(many) >= 300 and int(b.full.truncated(20, "cut").rays_per_node(many)[e]) == len(many)
    hits, cnt = _assert_rays(b.dev, b.u, b.full, many, "cut", "d20 many rays", key=("d20", "many rays"))
    assert (hits["node"] == e).all() and (hits["ordinal"] == 0).all() and (hits["t"] == 0.25).all() and int(cnt["numHits"]) == len(many)
    _assert_rays(b.dev, b.u, b.full, many, "all", "d20 many rays all")


def test_spheres_at_the_level_20_leaf(built_libs):
    b = _built("d20")
    d = b.d
    dr.assert_d20_shape(d.export, d.k, "d20 (oracle)")
    e, n = dr.deep_entry(b.full)
    q = dr.d20_spheres()
    for k in (dr.SPHERE_K, 1):
        nb, within = _assert_spheres(b.dev, b.u, b.full, q, k, "cut", f"d20 spheres k={k} cut", key=("d20", "spheres", k))
        assert (nb["node"] == e).all() and (nb["ordinal"] == np.arange(k)[None, :]).all() and (nb["d2"] == 0).all() and within[0] == within[1] == n
        nr.assert_found_are_brute(nb, within, q, d.pts, k, f"d20 spheres k={k}")
        _assert_spheres(b.dev, b.u, b.full, q, k, "all", f"d20 spheres k={k} all")
    # the chain's voxels of levels 1 .. 19 behind and between the identical samples, ordered by (d2, node, ordinal)
    wide = dr.Spheres([dr.POINT], 0.75)
    for ml in (19, 20):
        nb, _ = _assert_spheres(b.dev, b.u, b.full, wide, abi.NEIGHBOURS_MAX_K, "all", f"d20 wide sphere all@{ml}", ml=ml)
        want, _ = nr.exhaustive(b.full.truncated(ml, "all"), wide, abi.NEIGHBOURS_MAX_K)
        assert nb.tobytes() == want.tobytes()
    many = dr.d20_many_spheres()
    assert len(many) >= 300 and int(b.full.truncated(20, "cut").spheres_per_node(many)[e]) == len(many)
    nb, within = _assert_spheres(b.dev, b.u, b.full, many, dr.SPHERE_K, "cut", "d20 many spheres", key=("d20", "many spheres"))
    assert (nb["node"] == e).all() and (within == n).all()


def test_regions_at_the_level_20_leaf(built_libs):
    b = _built("d20")
    d = b.d
    e, k = dr.deep_entry(d.export)
    assert k == d.k and dr.region_classes(d.export, dr.d20_regions(d.export)["x>=below"][0], abi.MAX_DEPTH)[0] == 1
    for key, (region, keeps) in dr.d20_regions(b.full).items():
        for sel in ("cut", "all"):
            mirror = _assert_region(b.dev, b.u, b.full, region, sel, f"d20 {key} {sel}")
            deep = mirror.nodes[(mirror.nodes["level"] == abi.MAX_DEPTH) & (mirror.nodes["numSamples"] > 0)]
            assert (len(deep) == 1 and int(deep["numSamples"][0]) == k) if keeps == "all" else len(deep) == 0, (key, sel)
            if sel == "cut":
                rr.assert_same_multiset(mirror.samples, d.pts[rr.brute_mask(region, d.pts)], key)


# ---- 6. footprints -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d13", "d13x"])
def test_footprints_across_level_13(built_libs, name):
    """Per footprint of dr.d13_footprints: nodes of level 13 are filtered (and, cell12, copied whole) by the ORACLE's export; then the device
    == the mirror on its own export, the cut == the input filtered by the exact rule F1, the count-only call agrees.  In D13x a level-13
    node is 1 wide at coordinates near 5 000: the rectangle (boxMin + X * size) - e has its inflation e = 2^-7 at the 20th bit."""
    b = _built(name)
    d = b.d
    prints = dr.d13_footprints(d)
    for key, f in prints.items():
        dr.assert_footprint_not_vacuous(d.export, f, dr.LEAF_LEVEL, f"{name} {key}", dr.D13_COPIES[key])
        mirror = _assert_footprint(b.dev, b.u, b.full, f, "cut", f"{name} {key} cut")
        rr.assert_same_multiset(mirror.samples, d.pts[fr.contains_exact(f, d.pts)], f"{name} {key}")
        _assert_footprint(b.dev, b.u, b.full, f, "all", f"{name} {key} all")
    slab = dr.d13_regions(d)["slab"]
    mirror = _assert_footprint(b.dev, b.u, b.full, prints["star7"], "cut", f"{name} star7 and slab", region=slab)
    both = fr.contains_exact(prints["star7"], d.pts) & rr.brute_mask(slab, d.pts)
    assert 0 < both.sum() < min(int(fr.contains_exact(prints["star7"], d.pts).sum()), int(rr.brute_mask(slab, d.pts).sum()))
    rr.assert_same_multiset(mirror.samples, d.pts[both], f"{name} star7 and slab")


def test_footprints_at_the_level_20_leaf(built_libs):
    """Rectangles with a side at the point's own fp32 x or y, or one step from it (Footprint.from_rect keeps lo_x <= x <= hi_x, lo_y <= y <
    hi_y): the level-20 entry comes back with all k samples or not at all."""
    b = _built("d20")
    d = b.d
    e, k = dr.deep_entry(d.export)
    prints = dr.d20_footprints()
    assert k == d.k and all(dr.footprint_classes(d.export, f, abi.MAX_DEPTH)[0] == 1 for f, _ in prints.values())
    for key, (f, keeps) in prints.items():
        for sel in ("cut", "all"):
            mirror = _assert_footprint(b.dev, b.u, b.full, f, sel, f"d20 {key} {sel}")
            deep = _deep_samples(mirror)
            assert (len(deep) == 1 and int(deep["numSamples"][0]) == k) if keeps == "all" else len(deep) == 0, (key, sel)
            if sel == "cut":
                exact = fr.contains_exact(f, d.pts)
                assert exact.any()
                rr.assert_same_multiset(mirror.samples, d.pts[exact], key)
        for ml in (19, 20):
            _assert_footprint(b.dev, b.u, b.full, f, "all", f"d20 {key} all@{ml}", ml=ml)


# ---- 7. clip regions ---------------------------------------------------------------------------------------------------------------------------
def _image(name):
    """The downloaded image of a module octree, once."""
    b = _built(name)
    if not hasattr(b, "image"):
        b.image = host_image_of(b.dev)
    return b.image


def _level_classes(vis, region, u, level):
    """How many records of `level` in an oracle's visible list a region leaves outside / filters / copies (rules 1 and 4)."""
    cls = clip_ref.node_classes(vis, len(vis), region, u)[vis["level"] == level]
    return [int((cls == c).sum()) for c in (clip_ref.OUTSIDE, clip_ref.FILTERED, clip_ref.COPIED)]


@pytest.mark.parametrize("hqs", [False, True], ids=["plain", "hqs"])
@pytest.mark.parametrize("mode", on_clips.MODES)
@pytest.mark.parametrize("region_kind", ["cell12", "slab", "frustum"])
def test_clipped_close_up_of_level_13(built_libs, region_kind, mode, hqs):
    """D13x under the close camera: the clip's node classes are decided for level-13 nodes 1 wide at coordinates near 5 000, in the draw and in
    the visibility pass.  The oracle's UNCLIPPED visible list holds level-13 nodes of every class."""
    b = _built("d13x")
    d, dev = b.d, b.dev
    nodes, pers, nn = _image("d13x")
    u = dev.uniforms(W, H, _close_cam(d), d.box, hqs=hqs)
    region = dr.d13_regions(d)[region_kind]
    vis_un = on_clips._unclipped(("d13x",), nodes, nn, u)[3]
    counts = _level_classes(vis_un, region, u, dr.LEAF_LEVEL)
    print(f"unclipped visible list: {len(vis_un)} nodes; at level 13 {counts[0]} outside / {counts[1]} filtered / {counts[2]} copied")
    assert min(counts) >= 1, counts
    on_clips._clipped_frame(dev, ("d13x",), nodes, pers, nn, u, Clip(region, mode, on_clips.COLOUR), region_kind, f"d13x close-up {region_kind} {mode} hqs={int(hqs)}")


@pytest.mark.parametrize("mode", on_clips.MODES)
def test_clipped_close_up_on_an_imported_octree(built_libs, tmp_path, mode):
    """The same octree after a plain import through a file: the clipped frames are the source's bit for bit (and the oracle's on the imported
    image)."""
    b = _built("d13x")
    d, src = b.d, b.dev
    dst = _device()
    dst.nodes.fill_(0xA5)
    dst.import_octree(_through_file(b.full, tmp_path))
    assert int(dst.read_stats()["dbg"]) == 0
    u = dst.uniforms(W, H, _close_cam(d), d.box, hqs=True)
    clip = Clip(dr.d13_regions(d)["slab"], mode, on_clips.COLOUR)
    nodes, pers, nn = host_image_of(dst)
    _, fb, _, _ = on_clips._clipped_frame(dst, ("d13x imported", mode), nodes, pers, nn, u, clip, "slab", f"d13x imported slab {mode}")
    src.set_clip(clip)
    try:
        src.render(u)
        assert np.array_equal(src.framebuffer(W, H), fb) and np.array_equal(src.color(W, H), dst.color(W, H)), "the imported octree draws another clipped frame"
    finally:
        src.set_clip(None)


def _leaf_uniforms(dev, d, nodes, nn, leaf):
    """The cases' camera with minNodeSize lowered until the ORACLE's visible list of this image holds the level-20 leaf: a level-20 node is
    2^-20 of the box, far below a pixel."""
    key = node_keys(nodes[leaf: leaf + 1])[0]
    for size in (0.0, -1.0):
        u = dev.uniforms(W, H, cases._cam(d.box), d.box)
        u["minNodeSize"] = size
        vis = on_clips._unclipped(("d20",), nodes, nn, u)[3]
        if (node_keys(vis) == key).any():
            return u
    raise AssertionError("no minNodeSize makes the oracle draw the level-20 leaf")


@pytest.mark.parametrize("mode", on_clips.MODES)
def test_clip_at_the_level_20_leaf(built_libs, mode):
    """The identical samples under a clip: the leaf is drawn (asserted from the oracle's visible list), and per region the mirror's image keeps
    all k of them or none — inside keeps what the region keeps, outside the rest, highlight recolours them.  They cover one pixel, so the
    frame need not differ from the unclipped one."""
    b = _built("d20")
    d, dev = b.d, b.dev
    nodes, pers, nn = _image("d20")
    at = np.nonzero((nodes["level"][:nn] == abi.MAX_DEPTH) & (nodes["numPoints"][:nn] > 0))[0]
    assert len(at) == 1 and int(nodes["numPoints"][at[0]]) == d.k
    leaf = int(at[0])
    u = _leaf_uniforms(dev, d, nodes, nn, leaf)
    for key, (region, keeps) in dr.d20_regions(b.full).items():
        clip = Clip(region, mode, on_clips.COLOUR)
        img, *_ = on_clips._clipped_frame(dev, ("d20",), nodes, pers, nn, u, clip, key, f"d20 {key} {mode}", floor=0, differs=False)
        kept = clip_ref.kept_samples(img, leaf)
        if mode == "highlight":
            assert len(kept) == d.k and ((kept["color"] == on_clips.COLOUR).all() if keeps == "all" else (kept["color"] != on_clips.COLOUR).all()), (key, mode)
        else:
            assert len(kept) == (d.k if (keeps == "all") == (mode == "inside") else 0), (key, mode, len(kept))
