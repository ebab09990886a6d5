"""CPU tier of the ray queries (include/simlod_hip.h, "ray queries"): the ABI records, the Rays constructors, and the host mirror
OctreeExport.cast on octrees built by the oracle — against a brute force over the raw input points, against an exhaustive search over the
export's samples without any culling, on ties, on degenerate rays, and its pair counts."""
import os
import re

import numpy as np
import pytest

import cases
import rays_ref as yr
import region_ref as rr
from export_ref import export_host
from simlod_amd import abi, octree_io
from simlod_amd.octree_io import OctreeExport, Rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = abi.EXPORT_NONE


def test_ray_structs_match_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    for struct, dt, n_offsets in (("SimlodRay", abi.ray_dtype, 6), ("SimlodRayHit", abi.ray_hit_dtype, 3), ("SimlodRayCounts", abi.ray_counts_dtype, 4)):
        assert int(re.search(r"sizeof\(%s\) == (\d+)" % struct, src).group(1)) == dt.itemsize, struct
        offs = dict(re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % struct, src))
        assert len(offs) == n_offsets, struct
        for f, o in offs.items():
            assert dt.fields[f][1] == int(o), (struct, f)
    assert abi.ray_dtype.itemsize == 48 and abi.ray_hit_dtype.itemsize == 32 and abi.ray_counts_dtype.itemsize == 32
    assert abi.ray_dtype.fields["origin"][1] == 0 and abi.ray_hit_dtype.fields["t"][1] == 0
    assert abi.ray_counts_dtype.fields["numNodes"][1] == 0 and abi.ray_counts_dtype.fields["error"][1] == 4
    assert abi.ray_hit_dtype.fields["sample"][0] == abi.point_dtype
    assert int(re.search(r"#define SIMLOD_RAYS_MAX \(1u << (\d+)\)", src).group(1)) == 20 and abi.RAYS_MAX == 1 << 20


def test_ray_symbols_exported(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_rays_buffer_min_bytes", "simlod_query_rays"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    a = L.simlod_rays_buffer_min_bytes(100, 0, 128, 0, 0)
    assert L.simlod_rays_buffer_min_bytes(100, 1_000_000, 128, 0, 0) >= a + 1000 * 32
    assert L.simlod_rays_buffer_min_bytes(200, 0, 128, 0, 0) > a and L.simlod_rays_buffer_min_bytes(100, 0, 4096, 0, 0) > a
    # a pair costs 32 bytes (its record and one partial), a further thousand candidates 16
    assert L.simlod_rays_buffer_min_bytes(100, 0, 128, 10, 0) == a + 320 and L.simlod_rays_buffer_min_bytes(100, 0, 128, 0, 5000) == a + 80
    assert hasattr(runtime.DeviceOctree, "cast_rays") and hasattr(runtime.DeviceOctree, "count_rays")


def test_rays_constructors():
    r = Rays([[1, 2, 3], [4, 5, 6]], (0, 0, -1), 0.5, 9.0, 0.25, 0.125)
    rec = r.record()
    assert rec.dtype == abi.ray_dtype and len(r) == 2 and not rec["reserved"].any()
    assert rec["origin"].tolist() == [[1, 2, 3], [4, 5, 6]] and rec["dir"].tolist() == [[0, 0, -1]] * 2
    assert rec["tMin"].tolist() == [0.5, 0.5] and rec["tMax"].tolist() == [9.0, 9.0] and rec["radius"].tolist() == [0.25] * 2 and rec["spread"].tolist() == [0.125] * 2
    v = Rays.vertical([[10, 20], [30, 40]], 50.0, 0.5, -10.0).record()
    assert v["origin"].tolist() == [[10, 20, 50], [30, 40, 50]] and v["dir"].tolist() == [[0, 0, -1]] * 2 and v["tMax"].tolist() == [60.0, 60.0]
    assert Rays.from_records(rec).record().tobytes() == rec.tobytes()


def test_rays_from_pixels():
    """A point on a pixel's ray projects to that pixel's centre, and the cone is pixel_radius pixels wide at every distance."""
    _, box, _, T = cases.case("terrain_4x100k")
    W, H = cases.W, cases.H
    px = np.array([[0, 0], [128, 128], [255, 17], [40, 200]])
    rays = Rays.from_pixels(T, W, H, px, pixel_radius=0.5, t_max=5000.0).record()
    m = np.asarray(T, dtype=np.float64).reshape(4, 4)
    o, d = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6) and (rays["tMax"] == 5000.0).all() and (rays["tMin"] == 0).all()
    side = np.cross(d, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side, axis=1)[:, None]
    for t in (100.0, 1000.0):
        # (on the cone's rim, a horizontal step sideways: half a pixel in the image centre, up to about 0.7 towards the corners, where a
        # pixel's footprint is not a circle)
        for shift, lo, hi in ((0.0, 0.0, 0.05), (1.0, 0.45, 0.75)):
            rad = rays["radius"].astype(np.float64) + rays["spread"].astype(np.float64) * t
            p = o + t * d + shift * rad[:, None] * side
            c = np.concatenate([p, np.ones((len(p), 1))], axis=1) @ m.T
            ndc = c[:, :2] / c[:, 3:4]
            pix = (ndc * 0.5 + 0.5) * [W, H]
            off = np.linalg.norm(pix - (px + 0.5), axis=1)
            assert ((off >= lo) & (off <= hi)).all() and (shift == 0.0 or abs(off[1] - 0.5) < 0.01), (t, shift, off)


@pytest.fixture(scope="module")
def octrees(built_libs):
    cache = {}

    def get(name, offset=(0, 0, 0)):
        if (name, offset) not in cache:
            cache[name, offset] = rr.host_octree(name, box_min=offset)
        return cache[name, offset]
    return get


def test_truncated_is_the_export(octrees):
    for name in ("uniform_3x40k", "terrain_4x100k"):
        full, pts, box, ho = octrees(name)
        for sel, ml in (("cut", 20), ("all", 20), ("cut", 2), ("all", 1), ("cut", 0)):
            t, s = export_host(ho.nodes, int(ho.stats["numNodes"][0]), ml, abi.EXPORT_SELECT[sel])
            got = full.truncated(ml, sel)
            assert got.nodes.tobytes() == t.tobytes() and got.samples.tobytes() == s.tobytes(), (name, sel, ml)
    with pytest.raises(ValueError):
        full.truncated(2, "cut").cast(yr.vertical(pts, box, 0.5))          # not a full export
    with pytest.raises(ValueError):
        full.cast(yr.vertical(pts, box, 0.5), select="visible")


@pytest.mark.parametrize("name", cases.CASES)
def test_cast_is_the_brute_force_minimum(octrees, name):
    """CUT @ 20 holds every input point exactly once: the nearest passing sample is the nearest passing input point."""
    full, pts, box, ho = octrees(name)
    cut = full.truncated(20, "cut")
    for key, (rays, needs_misses, cone) in yr.ray_sets(name, pts, box).items():
        what = f"{name} {key}"
        hits, cnt, passing = full.cast(rays, 20, "cut", return_counts=True, return_passing=True)
        share = yr.assert_not_vacuous(hits, needs_misses, what, passing, cone)
        tmin, npass, nbest = yr.assert_hits_are_brute(hits, rays, pts, what)
        assert np.array_equal(passing, npass), what
        yr.assert_hits_index_export(hits, cut, what)
        assert int(cnt["numHits"]) == int((hits["node"] != NONE).sum()) and int(cnt["numInvalid"]) == 0 and int(cnt["numNodes"]) == cut.num_nodes
        print(what, f"hit share {share:.2f}, pairs {int(cnt['numPairs'])}, candidates {int(cnt['numCandidates'])}")


# (the terrain's shares by the brute force alone: vertical 0.62 / 0.30 / 0.95 for radius 0.5 / 0.25 / 1.0)
def test_terrain_shares(octrees):
    full, pts, box, ho = octrees("terrain_4x100k")
    for radius, lo, hi in ((0.5, 0.55, 0.70), (0.25, 0.25, 0.36), (1.0, 0.90, 1.0)):
        tmin, npass, nbest = yr.brute(yr.vertical(pts, box, radius), pts)
        assert lo <= float((npass > 0).mean()) <= hi and not (nbest > 1).any(), radius


@pytest.mark.parametrize("name,offset", [("uniform_3x40k", (0, 0, 0)), ("terrain_4x100k", (0, 0, 0)), ("uniform_3x40k", cases.DYADIC),
                                         ("terrain_4x100k", cases.GEOREF)])
def test_culling_never_loses_a_hit(octrees, name, offset):
    """CUT @ 2 and ALL: the hit equals an exhaustive search over all selected samples of the export, with no culling."""
    full, pts, box, ho = octrees(name, offset)
    base_pts, base_box, _, _ = cases.case(name)
    for sel, ml in (("cut", 2), ("all", 20)):
        ex = full.truncated(ml, sel)
        for key, (rays, needs_misses, cone) in yr.ray_sets(name, base_pts, base_box).items():
            if key == "vertical r0.25":
                continue                     # (at level 2, and on the 1/2-unit grid of the georeferenced box, too thin to hit a quarter of the time)
            if tuple(offset) != (0, 0, 0):
                rays = yr.shift_rays(rays, offset)
            what = f"{name} {offset} {sel}@{ml} {key}"
            hits, passing = full.cast(rays, ml, sel, return_passing=True)
            yr.assert_not_vacuous(hits, False, what, passing, cone)
            yr.assert_hits_index_export(hits, ex, what)
            want = yr.exhaustive(ex, rays)
            assert hits.tobytes() == want.tobytes(), f"{what}: rays {np.nonzero(hits != want)[0][:8]} differ from the exhaustive search"
            assert full.cast(rays, ml, sel).tobytes() == ex.cast_selected(rays).tobytes()


def test_ties_go_to_the_smaller_node_and_ordinal(built_libs):
    """500 points twice, the second time under another colour: a ray aimed exactly at such a point meets two samples at the same t."""
    pts, box, batch, _ = cases.case("uniform_3x40k")
    rs = np.random.RandomState(7)
    dup = pts[rs.choice(len(pts), 500, replace=False)].copy()
    dup["color"] ^= 0x00FFFFFF
    allpts = np.concatenate([pts, dup])
    full, _, _, _ = rr.host_octree(pts=allpts, box=box, batch=40_000)
    xy = np.stack([dup["x"], dup["y"]], axis=1).astype(np.float64)
    rays = Rays.vertical(xy, 2.0, 0.0, -1.0)                   # radius 0, through the point's own x and y: s2 == 0 at that point
    for sel, ml in (("cut", 20), ("all", 20)):
        ex = full.truncated(ml, sel)
        hits = full.cast(rays, ml, sel)
        want = yr.exhaustive(ex, rays)
        assert hits.tobytes() == want.tobytes(), (sel, ml)
        # how many rays had a tie at their minimum, and that the winner is the smaller (node, ordinal)
        x, y, z = (ex.samples[a].astype(np.float64) for a in "xyz")
        node = np.repeat(np.arange(ex.num_nodes), ex.nodes["numSamples"].astype(np.int64))
        ties = 0
        for i in range(len(rays)):
            t, ok = yr.sample_test(rays.record(), i, x, y, z)
            best = np.nonzero(ok & (t == hits["t"][i]))[0]
            assert len(best) >= 1
            if len(best) > 1:
                ties += 1
                k = best[0]
                assert int(hits["node"][i]) == node[k] and int(hits["ordinal"][i]) == k - int(ex.nodes["firstSample"][node[k]]), i
        assert ties >= 100, ties


def test_degenerate_rays(octrees):
    full, pts, box, ho = octrees("terrain_4x100k")
    good = yr.vertical(pts, box, 0.5, n=16).record()
    ref = full.cast(Rays.from_records(good))
    assert (ref["node"] != NONE).sum() >= 4
    bad = []
    def variant(**kw):
        r = good[:1].copy()
        for k, v in kw.items():
            r[k] = v
        bad.append(r)
    variant(dir=[[0, 0, 0]])
    variant(origin=[[np.nan, 1, 1]])
    variant(dir=[[0, np.inf, -1]])
    variant(tMax=np.inf)
    variant(tMin=np.nan)
    variant(tMin=70.0)                       # tMin > tMax (60)
    variant(tMin=-1.0)
    variant(radius=-0.5)
    variant(spread=-1e-3)
    variant(spread=np.nan)
    variant(reserved=[[0, 1]])
    mixed = np.concatenate([good[:8]] + bad + [good[8:]])
    hits, cnt = full.cast(Rays.from_records(mixed), return_counts=True)
    nb = len(bad)
    assert int(cnt["numInvalid"]) == nb
    assert (hits["node"][8:8 + nb] == NONE).all() and np.isposinf(hits["t"][8:8 + nb]).all()
    assert np.concatenate([hits[:8], hits[8 + nb:]]).tobytes() == ref.tobytes()
    only_bad, c2 = full.cast(Rays.from_records(np.concatenate(bad)), return_counts=True)
    assert int(c2["numPairs"]) == 0 and int(c2["numCandidates"]) == 0 and int(c2["numHits"]) == 0 and int(c2["numInvalid"]) == nb


def test_axis_parallel_rays(octrees):
    """The d_a == 0 paths of rule 3: rays along +x that start inside the box, outside it, and exactly on a face of the root's inflated cube
    widened by R — the last one still forms pairs, one ulp further out it forms none."""
    full, pts, box, ho = octrees("terrain_4x100k")
    size = np.float64(max(box))
    e = np.ldexp(size, -20)
    radius = np.float32(0.5)
    face = np.float32(-(e + np.float64(radius)))            # y of the root cube's low face, widened: L = (0 - e) - R
    assert np.float64(face) == (0.0 - e) - np.float64(radius), "the face is not a float32: choose another radius"
    z = float(np.median(pts["z"]))
    rows = [([-5.0, 200.0, z], "inside the footprint"), ([-5.0, 900.0, z], "outside in y"), ([-5.0, float(face), z], "on the face"),
            ([-5.0, float(np.nextafter(face, np.float32(-1e9))), z], "one ulp outside"), ([300.0, 200.0, z], "starts inside the box")]
    rays = Rays([r[0] for r in rows], (1.0, 0.0, 0.0), 0.0, 700.0, float(radius), 0.0)
    hits, cnt, passing = full.cast(rays, return_counts=True, return_passing=True)
    per_ray = [full.cast(Rays.from_records(rays.record()[i:i + 1]), return_counts=True)[1] for i in range(len(rows))]
    pairs = [int(c["numPairs"]) for c in per_ray]
    assert pairs[0] > 0 and pairs[1] == 0 and pairs[2] > 0 and pairs[3] == 0 and pairs[4] > 0, pairs
    assert sum(pairs) == int(cnt["numPairs"])
    want = yr.exhaustive(full.truncated(20, "cut"), rays)
    assert hits.tobytes() == want.tobytes()
    # vertical rays exactly at x == L of the root and one ulp beyond (two zero components)
    zr = Rays([[float(face), 100.0, 50.0], [float(np.nextafter(face, np.float32(-1e9))), 100.0, 50.0]], (0.0, 0.0, -1.0), 0.0, 60.0, float(radius), 0.0)
    c = [full.cast(Rays.from_records(zr.record()[i:i + 1]), return_counts=True)[1] for i in range(2)]
    assert int(c[0]["numPairs"]) > 0 and int(c[1]["numPairs"]) == 0


def test_pair_counts(octrees):
    """The culling culls: the candidates of the vertical radius-0.5 set are below 20 % of rays x samples (the split rule gives this case
    about a dozen leaves and one pair per ray: a share near 0.09), and every hit's node is among its ray's pairs."""
    full, pts, box, ho = octrees("terrain_4x100k")
    rays = yr.vertical(pts, box, 0.5)
    hits, cnt = full.cast(rays, 20, "cut", return_counts=True)
    cut = full.truncated(20, "cut")
    share = int(cnt["numCandidates"]) / (len(rays) * cut.num_samples)
    print("pairs", int(cnt["numPairs"]), "candidates", int(cnt["numCandidates"]), f"share {share:.3f}")
    assert int(cnt["numPairs"]) >= int((hits["node"] != NONE).sum()) and share < 0.20
    # per ray: its pairs by the mirror on that ray alone, counted from the table
    rec = rays.record()
    mn, size = octree_io._box_of(full.box_min, full.box_max)
    e = np.ldexp(size, -abi.MAX_DEPTH)
    total_pairs = total_cand = 0
    for i in range(len(rec)):
        one = Rays.from_records(rec[i:i + 1])
        h, c = full.cast(one, 20, "cut", return_counts=True)
        total_pairs += int(c["numPairs"]); total_cand += int(c["numCandidates"])
        assert h.tobytes() == hits[i:i + 1].tobytes()
        if int(h["node"][0]) != NONE:
            # the hit's node is one of the ray's pairs: it and all its listed ancestors pass rule 3 for this ray
            t = int(h["node"][0])
            while t != NONE:
                nd = cut.nodes[t]
                s = np.ldexp(size, -int(nd["level"]))
                A = np.array([nd["X"], nd["Y"], nd["Z"]], dtype=np.float64)
                lo, hi = (mn + A * s) - e, (mn + (A + 1.0) * s) + e
                o, d = rec["origin"][i:i + 1].astype(np.float64), rec["dir"][i:i + 1].astype(np.float64)
                tmin, tmax = rec["tMin"][i:i + 1].astype(np.float64), rec["tMax"][i:i + 1].astype(np.float64)
                R = rec["radius"][i:i + 1].astype(np.float64) + rec["spread"][i:i + 1].astype(np.float64) * tmax
                assert octree_io._slab(lo, hi, o, d, tmin, tmax, R)[0], (i, t)
                t = int(nd["parent"])
    assert total_pairs == int(cnt["numPairs"]) and total_cand == int(cnt["numCandidates"])
    # ALL selects inner nodes too: more pairs, a superset of candidates
    _, call = full.cast(rays, 20, "all", return_counts=True)
    assert int(call["numPairs"]) > int(cnt["numPairs"]) and int(call["numCandidates"]) > int(cnt["numCandidates"])


def test_sample_test_kernel_uses_no_scratch():
    """`make resource-usage` on export.hip: the ray query's six kernels (the pair pipeline of export_pairs.inc over RayQuery, k_r_test and
    k_r_reduce of export_rays.inc) keep everything in registers and LDS (a spill in the hot loop of k_r_test would halve it)."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "simlod_amd", "csrc"), "resource-usage", "RU_SRCS=export.hip"], capture_output=True, text=True, check=True).stdout
    blocks = re.split(r"Function Name: ", out)[1:]
    scratch = {b.split()[0]: int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) for b in blocks}
    rays = {k: v for k, v in scratch.items() if "k_p_hier" in k or ("k_p_" in k and "RayQuery" in k) or "k_r_" in k}
    assert len(rays) == 6 and sum("k_p_pairs" in k for k in rays) == 2, sorted(scratch)
    assert all(any(n in k for k in rays) for n in ("k_p_hier", "k_p_pairs", "k_p_scan", "k_r_test", "k_r_reduce")), sorted(scratch)
    assert all(v == 0 for v in rays.values()), rays
