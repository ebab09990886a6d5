"""CPU tier: region queries (include/simlod_hip.h, "region queries") — the ABI structs, octree_io.Region, and the host mirror
OctreeExport.crop against the export restatement (zero planes) and against a brute-force filter of the input points, on octrees built by
the oracle's port."""
import os
import re

import numpy as np
import pytest

import cases
import region_ref as rr
from export_ref import export_host
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import OctreeExport, Region

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_region_structs_match_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodRegion\) == (\d+)", src).group(1)) == abi.region_dtype.itemsize == 272
    assert int(re.search(r"offsetof\(SimlodRegion, planes\) == (\d+)", src).group(1)) == abi.region_dtype.fields["planes"][1]
    assert int(re.search(r"sizeof\(SimlodQueryCounts\) == (\d+)", src).group(1)) == abi.query_counts_dtype.itemsize == 32
    offs = dict(re.findall(r"offsetof\(SimlodQueryCounts, (\w+)\) == (\d+)", src))
    assert len(offs) == 4
    for f, o in offs.items():
        assert abi.query_counts_dtype.fields[f][1] == int(o), f
    assert abi.query_counts_dtype.fields["numNodes"][1] == 0 and abi.query_counts_dtype.fields["error"][1] == 4
    assert int(re.search(r"#define SIMLOD_REGION_MAX_PLANES (\d+)u", src).group(1)) == abi.REGION_MAX_PLANES == 16
    assert abi.EXPORT_REGION == 3
    r = Region.from_planes([[1, 2, 3, 4]]).record()
    assert r.dtype == abi.region_dtype and int(r["numPlanes"][0]) == 1 and r["planes"][0, 0].tolist() == [1, 2, 3, 4] and not r["reserved"].any()


def test_query_symbols_exported(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_query_buffer_min_bytes", "simlod_query_region"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    a = L.simlod_query_buffer_min_bytes(100, 0)
    assert L.simlod_query_buffer_min_bytes(100, 1_000_000) >= a + 1000 * 32 and L.simlod_query_buffer_min_bytes(200, 0) > a
    assert hasattr(runtime.DeviceOctree, "count_region") and hasattr(runtime.DeviceOctree, "query_region")


def test_region_constructors():
    b = Region.from_box((1, 2, 3), (4, 5, 6))
    assert b.planes.dtype == np.float32
    assert b.planes.tolist() == [[1, 0, 0, -1], [-1, 0, 0, 4], [0, 1, 0, -2], [0, -1, 0, 5], [0, 0, 1, -3], [0, 0, -1, 6]]
    assert Region().planes.shape == (0, 4) and Region.from_planes(np.zeros((16, 4))).planes.shape == (16, 4)
    with pytest.raises(ValueError):
        Region.from_planes(np.zeros((17, 4)))
    with pytest.raises(ValueError):
        Region.from_planes([[1, 0, 0, np.nan]])
    with pytest.raises(ValueError):
        Region.from_planes([[1e39, 0, 0, 0]])          # infinite as float32


def test_region_from_frustum():
    _, box, _, T = cases.case("terrain_4x100k")
    r = Region.from_frustum(T)
    assert r.planes.shape == (5, 4)
    rs = np.random.RandomState(5)
    p = (rs.rand(20000, 3) * 3 - 1) * np.asarray(box, np.float64)
    h = np.concatenate([p, np.ones((len(p), 1))], axis=1)
    clip = h @ np.asarray(T, np.float64).T                         # clip = M (p, 1), rows[i] = row i
    x, y, w = clip[:, 0], clip[:, 1], clip[:, 3]
    direct = np.stack([w + x, w - x, w + y, w - y, w], axis=1)
    # only points farther than a relative 1e-5 from every plane: the float32 rounding of the coefficients cannot flip them
    scale = np.abs(h) @ np.abs(np.stack([T[3] + T[0], T[3] - T[0], T[3] + T[1], T[3] - T[1], T[3]]).astype(np.float64)).T
    far = (np.abs(direct) > 1e-5 * scale).all(axis=1)
    assert far.sum() > 15000
    pts = np.zeros(len(p), dtype=abi.point_dtype)
    pts["x"], pts["y"], pts["z"] = p[:, 0], p[:, 1], p[:, 2]
    got = rr.brute_mask(r, pts)
    q = np.stack([pts["x"], pts["y"], pts["z"], np.ones(len(p), np.float32)], axis=1).astype(np.float64)
    clip32 = q @ np.asarray(T, np.float64).T
    want = ((clip32[:, 3] + clip32[:, 0] >= 0) & (clip32[:, 3] - clip32[:, 0] >= 0) & (clip32[:, 3] + clip32[:, 1] >= 0) &
            (clip32[:, 3] - clip32[:, 1] >= 0) & (clip32[:, 3] >= 0))
    assert np.array_equal(got[far], want[far]) and 0 < want[far].sum() < far.sum()


# (case, offset of its box: None = at the origin, as the reference host places it)
BUILT = [(n, None) for n in cases.CASES] + [("uniform_3x40k", "inexact"), ("terrain_4x100k", "georef"), ("hotspot_150k", "dyadic")]


@pytest.fixture(scope="module", params=BUILT, ids=lambda p: p[0] if p[1] is None else f"{p[0]}@{p[1]}")
def built(request):
    """-> (name, full export, points, (box size, box min), HostOctree)"""
    name, offset = request.param
    box_min = (0, 0, 0) if offset is None else cases.offset_of(offset, cases.case(name)[1])
    ex, pts, box, ho = rr.host_octree(name, box_min=box_min)
    if offset is not None:
        assert ex.box_min == tuple(float(np.float32(v)) for v in box_min) and (pts["x"] >= np.float32(box_min[0])).all()
    return name, ex, pts, (box, box_min), ho


def test_crop_without_planes_is_the_export(built):
    name, ex, pts, box, ho = built
    n = int(ho.stats["numNodes"][0])
    for ml in (0, 2, 20):
        for sel in (abi.EXPORT_ALL, abi.EXPORT_CUT):
            t, s = export_host(ho.nodes, n, ml, sel)
            c, cnt = ex.crop(Region(), ml, sel, return_counts=True)
            assert c.nodes.tobytes() == t.tobytes() and c.samples.tobytes() == s.tobytes(), (name, ml, sel)
            assert c.select == abi.EXPORT_REGION and c.max_level == ml
            assert int(cnt["numNodes"]) == len(t) and int(cnt["numSamples"]) == int(cnt["numCandidates"]) == len(s)
            assert int(cnt["numFilteredNodes"]) == 0 and int(cnt["numCopiedNodes"]) == int((t["numSamples"] != 0).sum())


@pytest.mark.parametrize("kind", ["oblique", "slab", "box"])
def test_crop_is_the_brute_force_filter(built, kind):
    name, ex, pts, box, ho = built
    r = rr.region(kind, *box)
    c, cnt = ex.crop(r, 20, "cut", return_counts=True)
    c.validate()
    inside = rr.brute_mask(r, pts)
    assert 0 < inside.sum() and (inside.sum() < len(pts) or "hotspot" in name), "the region must cut the cloud (the hotspot's one cell lies inside some)"
    rr.assert_same_multiset(c.samples, pts[inside], f"{name} {kind}")
    assert int(cnt["numSamples"]) == c.num_samples <= int(cnt["numCandidates"]) and int(cnt["numNodes"]) == c.num_nodes
    # per node: the source node's samples under the mask, in order
    src = {(int(e["level"]), int(e["X"]), int(e["Y"]), int(e["Z"])): e for e in ex.nodes}
    for e in c.nodes:
        s = src[(int(e["level"]), int(e["X"]), int(e["Y"]), int(e["Z"]))]
        got = c.samples[int(e["firstSample"]): int(e["firstSample"]) + int(e["numSamples"])]
        if not e["flags"] & abi.EXPORT_FLAG_SELECTED:
            assert len(got) == 0
            continue
        assert (e["flags"] & abi.EXPORT_FLAG_LEAF) == (s["flags"] & abi.EXPORT_FLAG_LEAF)
        seg = ex.samples[int(s["firstSample"]): int(s["firstSample"]) + int(s["numSamples"])]
        assert got.tobytes() == seg[rr.brute_mask(r, seg)].tobytes(), (name, kind, e)
    # select all: every listed node, the same rule
    a = ex.crop(r, 20, "all").validate()
    assert a.num_nodes == c.num_nodes and a.num_samples >= c.num_samples
    assert ((a.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0).all()


def test_crop_that_misses_the_box(built):
    name, ex, pts, box, ho = built
    c, cnt = ex.crop(rr.region("miss", *box), 20, "cut", return_counts=True)
    c.validate()
    assert c.num_nodes == 1 and c.num_samples == 0 and int(c.nodes["childMask"][0]) == 0 and int(c.nodes["firstChild"][0]) == abi.EXPORT_NONE
    assert [int(cnt[f]) for f in cnt.dtype.names] == [1, 0, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def face_octree():
    """A uniform cube plus points exactly on the planes x = y = z = size / 2 (node faces at every level) and one ulp to either side."""
    pts, box = synthetic.uniform_cube(600_000, seed=9)
    half = np.float32(0.5)
    vals = np.array([np.nextafter(half, np.float32(0)), half, np.nextafter(half, np.float32(1))], dtype=np.float32)
    extra = pts[:3000].copy()
    rs = np.random.RandomState(2)
    extra["x"] = vals[rs.randint(0, 3, 3000)]
    extra["y"][1000:2000] = vals[rs.randint(0, 3, 1000)]
    extra["z"][1500:2500] = vals[rs.randint(0, 3, 1000)]
    allp = np.concatenate([pts, extra])
    rs.shuffle(allp)
    ex, _, _, _ = rr.host_octree(pts=allp, box=box, batch=201_000)
    return ex, allp


@pytest.mark.parametrize("planes", [
    [[1, 0, 0, -0.5]],
    [[-1, 0, 0, 0.5]],
    [[1, 0, 0, -0.5], [0, 1, 0, -0.5], [0, 0, 1, -0.5]],
    [[-1, 0, 0, 0.5], [0, 1, 0, -0.5], [0, 0, -1, 0.5]],
])
def test_planes_on_node_faces(face_octree, planes):
    ex, allp = face_octree
    assert ex.nodes["level"].max() >= 2
    r = Region.from_planes(planes)
    c, cnt = ex.crop(r, 20, "cut", return_counts=True)
    c.validate()
    want = allp[rr.brute_mask(r, allp)]
    on = np.ones(len(want), bool)
    for a, p in zip("xyz", np.abs(np.asarray(planes)[:, :3]).sum(axis=0)):
        if p:
            assert (want[a] == np.float32(0.5)).sum() > 50       # points exactly on each plane of the region are part of the answer,
            on &= want[a] == np.float32(0.5)
    assert on.any()                                              # and some on all of them at once
    rr.assert_same_multiset(c.samples, want, str(planes))
    assert int(cnt["numNodes"]) < ex.num_nodes and int(cnt["numFilteredNodes"]) > 0


def test_points_on_the_max_faces_are_outside_the_contract():
    """Rule 4: a point with x == min + size is not stored under the nodes whose cubes hold it, so a region that selects the max face alone culls
    the nodes that store such points.  Pinned: what the oracle's octree gives."""
    pts, box = synthetic.uniform_cube(600_000, seed=9)
    extra = pts[:1000].copy()
    extra["x"] = np.float32(1.0)
    allp = np.concatenate([pts, extra])
    np.random.RandomState(1).shuffle(allp)
    ex, _, _, _ = rr.host_octree(pts=allp, box=box, batch=200_500)
    full = ex.crop(Region(), 20, "cut")
    rr.assert_same_multiset(full.samples, allp, "no planes")                           # nothing is lost without a region
    on_face = Region.from_planes([[1, 0, 0, -1.0]])
    assert int(rr.brute_mask(on_face, allp).sum()) == 1000
    assert ex.crop(on_face, 20, "cut").num_samples == 0                                # culled with the X = 0 nodes that store them
    upper = Region.from_planes([[1, 0, 0, -0.5]])
    c = ex.crop(upper, 20, "cut")
    inside = rr.brute_mask(upper, allp) & (allp["x"] < np.float32(1.0))
    rr.assert_same_multiset(c.samples[c.samples["x"] < np.float32(1.0)], allp[inside], "x >= 0.5, in-contract points")
    # the points on the face: deterministic — returned iff the node that stores them is copied, or filtered and they pass
    assert int((c.samples["x"] == np.float32(1.0)).sum()) == PINNED_MAX_FACE_POINTS_IN_UPPER_HALF


PINNED_MAX_FACE_POINTS_IN_UPPER_HALF = 0      # (they are stored under X = 0 nodes, which x >= size / 2 culls)


def test_crop_file_roundtrip_and_refusals(built, tmp_path):
    name, ex, pts, box, ho = built
    c = ex.crop(rr.region("oblique", *box), 20, "cut")
    p = tmp_path / "crop.simlodx"
    c.save(p)
    ld = OctreeExport.load(p)
    assert ld.select == abi.EXPORT_REGION and ld.max_level == 20 and ld.box_min == ex.box_min and ld.box_max == ex.box_max
    assert ld.nodes.tobytes() == c.nodes.tobytes() and ld.samples.tobytes() == c.samples.tobytes()
    with pytest.raises(ValueError, match="not a full export"):
        c.validate(buildable=True)
    assert not c.is_buildable
    # crop takes a full export only
    with pytest.raises(ValueError, match="full export"):
        c.crop(Region())
    n = int(ho.stats["numNodes"][0])
    t, s = export_host(ho.nodes, n, 20, abi.EXPORT_CUT)
    with pytest.raises(ValueError, match="full export"):
        OctreeExport(t, s, ex.box_min, ex.box_max, 20, "cut").crop(Region())
    t, s = export_host(ho.nodes, n, 1, abi.EXPORT_ALL)
    with pytest.raises(ValueError, match="full export"):
        OctreeExport(t, s, ex.box_min, ex.box_max, 1, "all").crop(Region())
    with pytest.raises(ValueError):
        ex.crop(Region(), select="visible")
