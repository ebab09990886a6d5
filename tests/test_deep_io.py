"""CPU tier: the preconditions of tests/test_gpu_deep_octrees.py, from the oracle, the mirrors of simlod_amd/octree_io.py and brute force alone —
octrees 13 and 20 levels deep (tests/deep_ref.py) are what they are said to be, the mirrors' cuts, casts, neighbour searches, crops and
rebuilt grids hold on them, and every query set reaches the deepest nodes.  Footprints are held against footprint_ref.contains_exact, rule F1
with every edge's side decided exactly: on these inputs it agrees with the fp64 formula on every point, so the crops equal both filters."""
import numpy as np
import pytest

import cases
import clip_ref
import footprint_ref as fr
import neighbours_ref as nr
import rays_ref as yr
import region_ref as rr
import deep_ref as dr
from export_ref import entry_index, export_host
from resume_ref import grid_of_image, rebuild_grids
from simlod_amd import abi
from simlod_amd.octree_io import Region
from test_gpu_deep_paths import CELL_LEVELS, OFF_ORIGIN_MARGIN, assert_input_arithmetic, deep_case
from util import node_keys, oracle_frame

NONE = abi.EXPORT_NONE


def _old_deep_case(cell_level):
    """deep_case as it was before it took `scale` and `cell`, for the byte comparison below."""
    rs = np.random.RandomState(100 + cell_level)
    scale = np.float32(2.0 ** -(cell_level + 2))
    batches = []
    for n in (60_000, 400_000, 100_000, 2_000):
        cell = rs.randint(0, 4, size=(n, 3))
        v = (rs.random_sample((n, 3)) * 0.998 + 0.001).astype(np.float32)
        p = (cell.astype(np.float32) + v) * scale
        c = np.floor(v * np.float32(255.0)).astype(np.uint32)
        pts = np.empty(n, dtype=abi.point_dtype)
        pts["x"], pts["y"], pts["z"] = p[:, 0], p[:, 1], p[:, 2]
        pts["color"] = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | np.uint32(255 << 24)
        batches.append(pts)
    return batches


@pytest.mark.parametrize("cell_level", CELL_LEVELS)
def test_deep_case_defaults_are_the_arrays_they_were(cell_level):
    box, batches, counts = deep_case(cell_level)
    assert box.dtype == np.float32 and box.tolist() == [1.0, 1.0, 1.0]
    for got, want in zip(batches, _old_deep_case(cell_level)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def test_scaled_case_off_the_origin_keeps_every_point_in_its_cell():
    box, batches, counts, origin = dr.d13_input("d13x")
    _, _, base_counts, _ = dr.d13_input("d13")
    assert box.tolist() == [dr.SCALE_X] * 3 and all(np.array_equal(a, b) for a, b in zip(counts, base_counts))
    assert_input_arithmetic(counts)
    size13 = dr.SCALE_X * 2.0 ** -dr.LEAF_LEVEL
    for pts, cnt in zip(batches, counts):
        p = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float64)
        cell = np.floor(p / size13).astype(np.int64)
        sub = cell - 4 * np.asarray(dr.CELL_X)
        assert ((sub >= 0) & (sub < 4)).all(), "a point left the level-11 cell"
        assert np.array_equal(np.bincount(sub[:, 0] << 4 | sub[:, 1] << 2 | sub[:, 2], minlength=64), cnt)
        # strictly inside: further from every face of the level-13 cell than the fp32 spacing of a coordinate there
        frac = p / size13 - cell
        assert frac.min() > OFF_ORIGIN_MARGIN / 2 and frac.max() < 1.0 - OFF_ORIGIN_MARGIN / 2 and float(np.spacing(np.float32(p.max()))) < size13 * OFF_ORIGIN_MARGIN / 8
    assert 0.55 * dr.SCALE_X < origin.min() and origin.max() < 0.8 * dr.SCALE_X


# ---- shape --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d13", "d13x"])
def test_d13_shape(built_libs, name):
    d = dr.built(name)
    assert d.nn == 161 and d.export.num_nodes == 161
    dr.assert_d13_shape(d.export, name)
    d.export.validate(buildable=True)
    rr.assert_same_multiset(d.export.truncated(20, "cut").samples, d.pts, name)


@pytest.mark.parametrize("name", ["d20", "d20r"])
def test_d20_shape_and_the_completed_export(built_libs, name):
    d = dr.built(name)
    assert d.nn == 161
    # the reference keeps the count and no chunks: export_host cannot walk the image as it stands
    with pytest.raises(AssertionError, match="shorter than its count"):
        export_host(d.ho.nodes, d.nn)
    dump = d.ho.dump()
    deep = dump["level"] == abi.MAX_DEPTH
    assert int(deep.sum()) == 8 and int((dump["numPoints"][deep] > 0).sum()) == 1 and int(dump["pointChunks"][deep].sum()) == 0
    assert d.k == int(dump["numPoints"][deep].sum()) == (75_000 if name == "d20r" else 70_000)
    dr.assert_d20_shape(d.export, d.k, name)
    assert d.export.is_buildable
    assert int(d.ho.nodes["numPoints"][dr.deep_leaf(d.ho)]) == d.k, "completed_export restores the count"
    rr.assert_same_multiset(d.export.truncated(20, "cut").samples, d.pts, name)


# ---- cuts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select", ["all", "cut"])
def test_d13_cuts_equal_the_host_export(built_libs, select):
    d = dr.built("d13")
    for ml in (12, 13):
        t, s = export_host(d.ho.nodes, d.nn, ml, abi.EXPORT_SELECT[select])
        cut = d.export.truncated(ml, select)
        assert cut.nodes.tobytes() == t.tobytes() and cut.samples.tobytes() == s.tobytes(), (ml, select)
        assert int(cut.nodes["level"].max()) == ml


@pytest.mark.parametrize("select", ["all", "cut"])
def test_d20_cuts_follow_from_the_completed_table(built_libs, select):
    """export_host cannot cut the oracle's image at 20 (the leaf without chunks); at 19 it can, and both cuts must be the completed table's
    prefix: the entries of the levels up to the cut, byte for byte but for what a cut changes in its last level."""
    d = dr.built("d20")
    full = d.export
    t, s = export_host(d.ho.nodes, d.nn, 19, abi.EXPORT_SELECT[select])
    c19 = full.truncated(19, select)
    assert c19.nodes.tobytes() == t.tobytes() and c19.samples.tobytes() == s.tobytes()
    assert c19.num_nodes == 153 and (c19.nodes["childMask"][c19.nodes["level"] == 19] == 0).all()
    c20 = full.truncated(20, select)
    assert c20.num_nodes == 161 and dr.deep_entry(c20) == (dr.deep_entry(full)[0], d.k)
    if select == "all":
        assert c20.nodes.tobytes() == full.nodes.tobytes() and c20.samples.tobytes() == full.samples.tobytes()
    else:
        leaf = (full.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0
        assert np.array_equal(c20.nodes["numSamples"], np.where(leaf, full.nodes["numSamples"], 0)) and c20.num_samples == len(d.pts)
    c20.validate()


# ---- D13 / D13x queries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d13", "d13x"])
def test_d13_rays_hit_level_13_and_equal_the_brute_force(built_libs, name):
    d = dr.built(name)
    cut = d.export.truncated(20, "cut")
    for key, (rays, cone) in dr.d13_rays(d).items():
        hits, cnt, passing = d.export.cast(rays, 20, "cut", return_counts=True, return_passing=True)
        assert int(cnt["numInvalid"]) == 0
        share = yr.assert_not_vacuous(hits, False, f"{name} {key}", passing, cone)
        at = dr.assert_hits_at_level(hits, cut.nodes, dr.LEAF_LEVEL, f"{name} {key}")
        print(name, key, f"hit share {share:.2f}, at level 13 {at:.2f}", {f: int(cnt[f]) for f in cnt.dtype.names})
        yr.assert_hits_index_export(hits, cut, f"{name} {key}")
        yr.assert_hits_are_brute(hits, rays, d.pts, f"{name} {key}")
        # with the voxels of the twelve levels above in the table too: the exhaustive search over the export's own samples
        some = dr.Rays.from_records(rays.record()[:8])
        assert d.export.cast(some, 20, "all").tobytes() == yr.exhaustive(d.export, some).tobytes(), f"{name} {key} all"


@pytest.mark.parametrize("name", ["d13", "d13x"])
def test_d13_spheres_equal_the_brute_force(built_libs, name):
    d = dr.built(name)
    within = {}
    for key, q in dr.d13_spheres(d).items():
        nb, w, cnt = d.export.neighbours(q, dr.SPHERE_K, 20, "cut", return_counts=True)
        within[key] = w
        print(name, key, "within", int(w.min()), int(np.median(w)), int(w.max()), {f: int(cnt[f]) for f in cnt.dtype.names})
        nr.assert_found_are_brute(nb, w, q, d.pts, dr.SPHERE_K, f"{name} {key}")
        cut = d.export.truncated(20, "cut")
        nr.assert_found_index_export(nb, cut, f"{name} {key}")
        assert (cut.nodes["level"][nb["node"][nb["node"] != NONE]] == dr.LEAF_LEVEL).all()
    dr.assert_spheres_not_vacuous(within, name)


def test_d13_regions_equal_the_brute_force_filter(built_libs):
    d = dr.built("d13")
    for key, region in dr.d13_regions(d).items():
        filtered, copied = dr.assert_region_not_vacuous(d.export, region, dr.LEAF_LEVEL, key)
        crop, cnt = d.export.crop(region, 20, "cut", return_counts=True)
        print(key, f"{filtered} filtered at level 13, {copied} copied", {f: int(cnt[f]) for f in cnt.dtype.names})
        assert int(cnt["numFilteredNodes"]) >= filtered and int(cnt["numCopiedNodes"]) == copied
        want = d.pts[rr.brute_mask(region, d.pts)]
        assert 0 < len(want) < len(d.pts)
        rr.assert_same_multiset(crop.samples, want, key)
        crop.validate()


# the input points inside each footprint of deep_ref.d13_footprints, and how many of them contains_exact decided in Fractions
D13_INSIDE = {"d13": {"star7": 114_655, "cell12": 142_863, "oblique": 113_429}, "d13x": {"star7": 114_537, "cell12": 140_826, "oblique": 114_155}}
D13_FRACTIONS = {"d13": {"star7": 0, "cell12": 0, "oblique": 0}, "d13x": {"star7": 1, "cell12": 23, "oblique": 0}}


@pytest.mark.parametrize("name", ["d13", "d13x"])
def test_d13_footprints_equal_the_exact_brute_force_filter(built_libs, name):
    d = dr.built(name)
    for key, f in dr.d13_footprints(d).items():
        filtered, copied = dr.assert_footprint_not_vacuous(d.export, f, dr.LEAF_LEVEL, f"{name} {key}", dr.D13_COPIES[key])
        inside = f.contains(d.pts)
        exact, decided = fr.contains_exact(f, d.pts, return_decided=True)
        print(name, key, f"{filtered} filtered at level 13, {copied} copied, {int(inside.sum())} points inside, {int(decided.sum())} decided in Fractions")
        assert np.array_equal(inside, exact), f"{name} {key}: rule F1 in fp64 and the exact rule disagree on {int((inside != exact).sum())} points"
        assert int(inside.sum()) == D13_INSIDE[name][key] and int(decided.sum()) == D13_FRACTIONS[name][key]
        crop, cnt = d.export.crop(Region(), 20, "cut", return_counts=True, footprint=f)
        assert int(cnt["numFilteredNodes"]) >= filtered and int(cnt["numCopiedNodes"]) == copied
        rr.assert_same_multiset(crop.samples, d.pts[exact], f"{name} {key}")
        crop.validate()
    # composed with the slab of d13_regions: outside by either, copied iff copied by both
    f, slab = dr.d13_footprints(d)["star7"], dr.d13_regions(d)["slab"]
    both = fr.contains_exact(f, d.pts) & rr.brute_mask(slab, d.pts)
    assert 0 < both.sum() < min(int(fr.contains_exact(f, d.pts).sum()), int(rr.brute_mask(slab, d.pts).sum()))
    crop = d.export.crop(slab, 20, "cut", footprint=f)
    rr.assert_same_multiset(crop.samples, d.pts[both], f"{name} star7 and slab")


def test_d13x_close_up_lists_level_13_nodes_of_every_clip_class(built_libs):
    """What the clip tests of tests/test_gpu_deep_octrees.py rest on, from the oracle's own image and rasteriser: under the close camera the
    unclipped visible list is 57 nodes, 56 of them at level 13, and every region of d13_regions leaves some of those outside, filters some
    and copies some."""
    d = dr.built("d13x")
    u = cases.uniforms_for(d.box, dr.close_cam(d))
    fb, _, st, vis = oracle_frame(d.ho.nodes, d.nn, u)
    assert len(vis) == 57 and int((vis["level"] == dr.LEAF_LEVEL).sum()) == 56 and int((fb != abi.CLEAR_PIXEL).sum()) == 53_638
    want = {"cell12": [30, 18, 8], "slab": [8, 33, 15], "frustum": [4, 32, 20]}
    for key, region in dr.d13_regions(d).items():
        cls = clip_ref.node_classes(vis, len(vis), region, u)[vis["level"] == dr.LEAF_LEVEL]
        assert [int((cls == c).sum()) for c in (clip_ref.OUTSIDE, clip_ref.FILTERED, clip_ref.COPIED)] == want[key], key


# ---- D20 queries -------------------------------------------------------------------------------------------------------------------------------
def test_d20_rays_through_the_point_hit_the_first_of_the_identical_samples(built_libs):
    d = dr.built("d20")
    e, k = dr.deep_entry(d.export)
    rays, miss = dr.d20_rays()
    for select in ("cut", "all"):
        table = d.export.truncated(20, select)
        hits, cnt, passing = d.export.cast(rays, 20, select, return_counts=True, return_passing=True)
        assert int(cnt["numInvalid"]) == 0
        through = np.arange(len(rays)) != miss
        exact = through & (rays.record()["radius"] == 0)
        if select == "cut":
            assert (hits["node"][through] == e).all() and (hits["ordinal"][through] == 0).all() and (hits["t"][through] == 0.25).all(), hits[through]
        else:
            # below level 17 a voxel's cell is finer than the fp32 spacing at the point: the chain's deepest voxels ARE the point, and the tie in t
            # goes to the smaller node
            assert (hits["t"][exact] == 0.25).all() and (hits["node"][exact] < e).all() and (table.nodes["level"][hits["node"][exact]] >= 17).all(), hits[exact]
            assert all((hits["sample"][a][exact] == np.float32(v)).all() for a, v in zip("xyz", dr.POINT))
        assert (passing[through] >= k).all(), "all k identical samples pass: the first of them is chosen among exact ties"
        assert hits["node"][miss] != e and passing[miss] == 0
        assert hits.tobytes() == yr.exhaustive(table, rays).tobytes(), select
        yr.assert_hits_index_export(hits, table, f"d20 {select}")
    hits = d.export.cast(rays, 20, "cut")
    yr.assert_hits_are_brute(hits, rays, d.pts, "d20")
    assert int(d.export.rays_per_node(rays)[e]) == len(rays) - 1, "the ray two cells away forms no pair with the level-20 node"
    many = dr.d20_many_rays()
    hits = d.export.cast(many, 20, "cut")
    assert len(many) >= 300 and (hits["node"] == e).all() and (hits["ordinal"] == 0).all() and (hits["t"] == 0.25).all()


@pytest.mark.parametrize("k", [16, 1])
def test_d20_spheres_at_the_point(built_libs, k):
    d = dr.built("d20")
    e, n = dr.deep_entry(d.export)
    q = dr.d20_spheres()
    _, uniform_within = nr.brute(q, d.pts[(d.pts["x"] != np.float32(dr.POINT[0])) | (d.pts["y"] != np.float32(dr.POINT[1]))], 1)
    nb, within = d.export.neighbours(q, k, 20, "cut")
    assert (nb["node"] == e).all() and (nb["ordinal"] == np.arange(k)[None, :]).all() and (nb["d2"] == 0).all()
    assert np.array_equal(within, n + uniform_within) and within[0] == within[1] == n
    nr.assert_found_are_brute(nb, within, q, d.pts, k, f"d20 k={k}")
    # with the chain's voxels in the table: (d2, node, ordinal) over the export's own samples
    nb, within = d.export.neighbours(q, k, 20, "all")
    want, ww = nr.exhaustive(d.export, q, k)
    assert nb.tobytes() == want.tobytes() and np.array_equal(within, ww)
    if k == 16:
        wide, _ = d.export.neighbours(dr.Spheres([dr.POINT], 0.75), abi.NEIGHBOURS_MAX_K, 20, "all")
        nodes = wide["node"][0].astype(np.int64)
        assert (wide["d2"][0] == 0).all() and nodes[0] < e and nodes[-1] == e and (np.diff(nodes) >= 0).all(), \
            "the chain's deepest voxels coincide with the point: ties in d2 go by (node, ordinal), the voxels' smaller nodes first"
    many = dr.d20_many_spheres()
    nb, within = d.export.neighbours(many, k, 20, "cut")
    assert len(many) >= 300 and (nb["node"] == e).all() and (within == n).all()


def test_d20_chain_voxels_order_behind_the_identical_samples(built_libs):
    """Select "all" with the level-20 leaf cut away (max level 19): the chain's voxels of levels 1 .. 19 are what a sphere at the point finds,
    in the order (d2, node, ordinal)."""
    d = dr.built("d20")
    q = dr.Spheres([dr.POINT], 0.75)
    cut = d.export.truncated(19, "all")
    nb, within = d.export.neighbours(q, abi.NEIGHBOURS_MAX_K, 19, "all")
    want, ww = nr.exhaustive(cut, q, abi.NEIGHBOURS_MAX_K)
    assert nb.tobytes() == want.tobytes() and np.array_equal(within, ww)
    lv = cut.nodes["level"][nb["node"][0]]
    assert (np.diff(nb["d2"][0]) >= 0).all() and lv.max() == 19 and len(np.unique(lv)) >= 8, lv


def test_d20_regions_keep_all_of_the_identical_samples_or_none(built_libs):
    d = dr.built("d20")
    e, k = dr.deep_entry(d.export)
    same = (d.pts["x"] == np.float32(dr.POINT[0])) & (d.pts["y"] == np.float32(dr.POINT[1])) & (d.pts["z"] == np.float32(dr.POINT[2]))
    assert int(same.sum()) == k
    for key, (region, keeps) in dr.d20_regions(d.export).items():
        mask = rr.brute_mask(region, d.pts)
        assert int((mask & same).sum()) == (k if keeps == "all" else 0), key
        for select in ("cut", "all"):
            crop, cnt = d.export.crop(region, 20, select, return_counts=True)
            deep = crop.nodes[(crop.nodes["level"] == abi.MAX_DEPTH) & (crop.nodes["numSamples"] > 0)]
            assert (len(deep) == 1 and int(deep["numSamples"][0]) == k) if keeps == "all" else len(deep) == 0, (key, select)
            crop.validate()
        crop = d.export.crop(region, 20, "cut")
        rr.assert_same_multiset(crop.samples, d.pts[mask], key)
        if key == "cell20":
            assert crop.num_samples == k and int((crop.nodes["level"] == abi.MAX_DEPTH).sum()) >= 1
    # the level-20 node under a plane through its inflated cube is filtered sample by sample: inflated by one level-20 cell, a node of that
    # level is three cells wide
    f, c = dr.region_classes(d.export, dr.d20_regions(d.export)["x>=below"][0], abi.MAX_DEPTH)
    assert f == 1 and c >= 1


def test_d20_footprints_keep_all_of_the_identical_samples_or_none(built_libs):
    d = dr.built("d20")
    e, k = dr.deep_entry(d.export)
    same = (d.pts["x"] == np.float32(dr.POINT[0])) & (d.pts["y"] == np.float32(dr.POINT[1])) & (d.pts["z"] == np.float32(dr.POINT[2]))
    assert int(same.sum()) == k == d.k
    prints = dr.d20_footprints()
    assert sorted(key for key, (f, keeps) in prints.items() if keeps == "none") == ["hi_x=below", "hi_y=y", "lo_x=above"]
    for key, (f, keeps) in prints.items():
        inside = f.contains(d.pts)
        exact, decided = fr.contains_exact(f, d.pts, return_decided=True)
        print(key, f"keeps {int((inside & same).sum())} of the identical points, {int((inside & ~same).sum())} of the others; {int(decided.sum())} decided in Fractions")
        assert np.array_equal(inside, exact), f"{key}: rule F1 in fp64 and the exact rule disagree on {int((inside != exact).sum())} points"
        assert int((exact & same).sum()) == (k if keeps == "all" else 0), key
        # on a vertical edge through the point c is 0: all k points are decided in Fractions, and are one (u, v)
        assert int(decided.sum()) == (k if key in dr.FRACTION_DECIDED else 0) and not (decided & ~same).any(), key
        # an empty answer is no match: every boundary rectangle keeps some of the uniform points too, the cell keeps none
        others = int((exact & ~same).sum())
        assert others == 0 if key == "cell" else others >= 2000, (key, others)
        # the level-20 node is filtered sample by sample: inflated by one level-20 cell, it is cut by an edge of every rectangle
        assert dr.footprint_classes(d.export, f, abi.MAX_DEPTH)[0] == 1, key
        for select in ("cut", "all"):
            crop, cnt = d.export.crop(Region(), 20, select, return_counts=True, footprint=f)
            deep = crop.nodes[(crop.nodes["level"] == abi.MAX_DEPTH) & (crop.nodes["numSamples"] > 0)]
            assert (len(deep) == 1 and int(deep["numSamples"][0]) == k) if keeps == "all" else len(deep) == 0, (key, select)
            crop.validate()
        crop = d.export.crop(Region(), 20, "cut", footprint=f)
        rr.assert_same_multiset(crop.samples, d.pts[exact], key)
        # ... and without the identical points, which the oracle counts and does not store
        rr.assert_same_multiset(crop.samples[(crop.samples["x"] != np.float32(dr.POINT[0])) | (crop.samples["y"] != np.float32(dr.POINT[1]))], d.pts[exact & ~same], key)
        if key == "cell":
            assert crop.num_samples == k
    # one of them with the half-space x >= the fp32 below the point's x: still all k
    both, _ = dr.d20_regions(d.export)["x>=below"]
    crop = d.export.crop(both, 20, "cut", footprint=prints["hi_x=x"][0])
    want = fr.contains_exact(prints["hi_x=x"][0], d.pts) & rr.brute_mask(both, d.pts)
    assert int((want & same).sum()) == k and int((want & ~same).sum()) == 0
    rr.assert_same_multiset(crop.samples, d.pts[want], "hi_x=x and x>=below")


def test_d20_leaf_is_listed_only_without_a_minimum_node_size(built_libs):
    """A level-20 node is 2^-20 of the box, a ten-thousandth of a pixel under the cases' camera: the oracle's visibility pass lists the leaf
    only with minNodeSize 0, where every node with a nonzero extent on screen counts as large.  (showPoints 0: the oracle keeps the leaf's
    count and no chunks, so its own image cannot be drawn there; the clip test draws the device's.)"""
    d = dr.built("d20")
    leaf = node_keys(d.ho.nodes[dr.deep_leaf(d.ho):][:1])[0]
    listed = {}
    for size in (64.0, 1.0, 0.0):
        u = cases.uniforms_for(d.box, cases._cam(d.box))
        u["minNodeSize"], u["showPoints"] = size, 0
        vis = oracle_frame(d.ho.nodes, d.nn, u)[3]
        listed[size] = bool((node_keys(vis) == leaf).any())
    assert listed == {64.0: False, 1.0: False, 0.0: True}, listed


# ---- grids ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d13", "d20"])
def test_rebuilt_grids_equal_the_oracles_at_depth(built_libs, name):
    """resume_ref.rebuild_grids on the oracle's export against the oracle's own grids, every inner node: levels 0 .. 12 of D13, 0 .. 19 of the
    completed D20 — the oracle samples the level-19 node's grid from the points it then drops at level 20, so the identical samples put in by
    hand rebuild that grid too."""
    d = dr.built(name)
    grids = rebuild_grids(d.export.nodes, d.export.samples, d.u)
    where = entry_index(d.export.nodes)
    with_grid = np.nonzero(d.ho.nodes["grid"][:d.nn] != 0)[0]
    levels = sorted(int(l) for l in d.ho.nodes["level"][with_grid])
    assert levels == (list(range(12)) + [12] * 8 if name == "d13" else list(range(20))) and len(grids) == len(with_grid)
    for i in with_grid:
        nd = d.ho.nodes[i]
        key = (int(nd["level"]), int(nd["X"]), int(nd["Y"]), int(nd["Z"]))
        assert np.array_equal(grids[where[key]], grid_of_image(d.ho.nodes, i, d.ho.persistent)), f"{name}: the grid at level {int(nd['level'])} differs"
