"""CPU tier of the neighbour queries (include/simlod_hip.h, "neighbour queries"): the ABI records, the scratch formula, the Spheres
constructors, and the host mirror OctreeExport.neighbours on octrees built by the oracle — against a brute force over the raw input points,
against an exhaustive search over the export's samples without any culling, on exact ties, on degenerate queries, at the edge of rule 3, and
its pair counts."""
import os
import re

import numpy as np
import pytest

import cases
import neighbours_ref as nr
import region_ref as rr
from simlod_amd import abi, octree_io
from simlod_amd.octree_io import Spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = abi.EXPORT_NONE
COUNT_FIELDS = list(abi.neighbour_counts_dtype.names)


def test_neighbour_structs_match_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    for struct, dt, n_offsets in (("SimlodSphere", abi.sphere_dtype, 1), ("SimlodNeighbour", abi.neighbour_dtype, 3), ("SimlodNeighbourCounts", abi.neighbour_counts_dtype, 6)):
        assert int(re.search(r"sizeof\(%s\) == (\d+)" % struct, src).group(1)) == dt.itemsize, struct
        offs = dict(re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % struct, src))
        assert len(offs) == n_offsets, struct
        for f, o in offs.items():
            assert dt.fields[f][1] == int(o), (struct, f)
    assert abi.sphere_dtype.itemsize == 16 and abi.neighbour_dtype.itemsize == 32 and abi.neighbour_counts_dtype.itemsize == 48
    assert abi.sphere_dtype.fields["center"][1] == 0 and abi.neighbour_dtype.fields["d2"][1] == 0
    assert abi.neighbour_counts_dtype.fields["numNodes"][1] == 0 and abi.neighbour_counts_dtype.fields["error"][1] == 4
    assert abi.neighbour_dtype.fields["sample"][0] == abi.point_dtype
    assert [abi.neighbour_dtype.fields[f][1] for f in ("d2", "node", "ordinal", "sample")] == [abi.ray_hit_dtype.fields[f][1] for f in ("t", "node", "ordinal", "sample")]
    assert int(re.search(r"#define SIMLOD_NEIGHBOURS_MAX \(1u << (\d+)\)", src).group(1)) == 20 and abi.NEIGHBOURS_MAX == 1 << 20
    assert int(re.search(r"#define SIMLOD_NEIGHBOURS_MAX_K (\d+)u", src).group(1)) == 16 and abi.NEIGHBOURS_MAX_K == 16


def _formula(L, cap, bound, n, k, pairs, cand):
    """The documented sum: the ray query's part for nodeCapacity and as many rays, 32 bytes per chunk item for bound / 1000 + cap + 1 items,
    16 + 16 (k + 1) per pair, 16 (k + 1) per further thousand candidates."""
    fixed = int(L.simlod_rays_buffer_min_bytes(cap, 0, n, 0, 0)) - 32 * (cap + 1)
    return fixed + 32 * (bound // 1000 + cap + 1) + pairs * (16 + 16 * (k + 1)) + (cand // 1000) * 16 * (k + 1)


def test_neighbour_symbols_and_scratch_formula(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_neighbours_buffer_min_bytes", "simlod_query_neighbours"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    for m in ("find_neighbours", "count_neighbours", "k_nearest"):
        assert hasattr(runtime.DeviceOctree, m)
    f = lambda *a: int(L.simlod_neighbours_buffer_min_bytes(*a))
    for cap, bound, n, k, pairs, cand in ((100, 0, 128, 8, 0, 0), (100, 1_000_000, 128, 8, 0, 0), (4425, 36_000_000, 4096, 16, 5000, 70_000_000),
                                          (1, 999, 1, 1, 1, 999), (200_000, 0, 1 << 20, 16, 1 << 22, (1 << 32) + 123), (33, 400_000, 128, 1, 131, 4_963_332)):
        assert f(cap, bound, n, k, pairs, cand) == _formula(L, cap, bound, n, k, pairs, cand), (cap, bound, n, k, pairs, cand)
    a = f(100, 0, 128, 8, 0, 0)
    assert f(200, 0, 128, 8, 0, 0) > a and f(100, 0, 4096, 8, 0, 0) > a and f(100, 0, 128, 16, 0, 0) == a
    # one more pair, one more thousand candidates, at k = 1 and k = 16
    for k, pair, thousand in ((1, 48, 32), (16, 288, 272)):
        base = f(100, 0, 128, k, 10, 5000)
        assert f(100, 0, 128, k, 11, 5000) == base + pair and f(100, 0, 128, k, 10, 6000) == base + thousand and f(100, 0, 128, k, 10, 5999) == base


def test_spheres_constructors():
    s = Spheres([[1, 2, 3], [4, 5, 6]], 0.25)
    rec = s.record()
    assert rec.dtype == abi.sphere_dtype and len(s) == 2 and rec["center"].tolist() == [[1, 2, 3], [4, 5, 6]] and rec["radius"].tolist() == [0.25, 0.25]
    assert Spheres([[1, 2, 3], [4, 5, 6]], [0.5, 2.0]).record()["radius"].tolist() == [0.5, 2.0]
    assert Spheres.from_records(rec).record().tobytes() == rec.tobytes() and Spheres.from_records(rec.view(np.uint8)).record().tobytes() == rec.tobytes()
    pts = np.zeros(3, dtype=abi.point_dtype)
    pts["x"], pts["y"], pts["z"], pts["color"] = [1, 2, 3], [4, 5, 6], [7, 8, 9], 77
    p = Spheres.from_points(pts, 1.5).record()
    assert p["center"].tolist() == [[1, 4, 7], [2, 5, 8], [3, 6, 9]] and (p["radius"] == 1.5).all() and len(Spheres(np.zeros((0, 3)), 1.0)) == 0
    assert np.isnan(Spheres([[np.nan, 0, 0]], -1.0).record()["center"][0, 0])            # nothing is validated here


@pytest.fixture(scope="module")
def octrees(built_libs):
    cache = {}

    def get(name, offset=(0, 0, 0)):
        if (name, offset) not in cache:
            cache[name, offset] = rr.host_octree(name, box_min=offset)
        return cache[name, offset]
    return get


@pytest.mark.parametrize("name", cases.CASES)
def test_neighbours_are_the_brute_force(octrees, name):
    """CUT @ 20 holds every input point exactly once: the k nearest passing samples are the k nearest passing input points."""
    full, pts, box, ho = octrees(name)
    cut = full.truncated(20, "cut")
    for key, q in nr.query_sets(pts, box).items():
        res = {k: full.neighbours(q, k, 20, "cut", return_counts=True) for k in (1, 8, 16)}
        # k = 16 against the brute force; the total order makes k = 1 and k = 8 its prefixes
        nr.assert_found_are_brute(res[16][0], res[16][1], q, pts, 16, f"{name} {key}")
        for k, (nb, within, cnt) in res.items():
            what = f"{name} {key} k={k}"
            assert nb.shape == (nr.N_QUERIES, k) and nb.dtype == abi.neighbour_dtype
            assert nb.tobytes() == np.ascontiguousarray(res[16][0][:, :k]).tobytes() and np.array_equal(within, res[16][1]), what
            if k == nr.K:
                print(what, nr.assert_not_vacuous(key, within, what), {f: int(cnt[f]) for f in COUNT_FIELDS})
            nr.assert_found_index_export(nb, cut, what)
            nr.assert_misses_behind(nb, within, k, what)
            assert int(cnt["numFound"]) == int(np.minimum(within, k).sum()) == int((nb["node"] != NONE).sum()) and int(cnt["numWithin"]) == int(within.sum())
            assert int(cnt["numInvalid"]) == 0 and int(cnt["numNodes"]) == cut.num_nodes and int(cnt["k"]) == k and int(cnt["error"]) == 0


@pytest.mark.parametrize("name", cases.CASES)
def test_query_sets_have_the_stated_shares(name):
    """The conditions on the raw points alone (no octree): thin finds nothing / a few, wide has more than k to choose from."""
    pts, box, _, _ = cases.case(name)
    sets = nr.query_sets(pts, box)
    nr.assert_thin_not_vacuous(nr.brute(sets["thin"], pts, nr.K)[1], name)
    nr.assert_wide_not_vacuous(nr.brute(sets["wide"], pts, nr.K)[1], name)


@pytest.mark.parametrize("name,offset", [("uniform_3x40k", (0, 0, 0)), ("terrain_4x100k", (0, 0, 0)), ("uniform_3x40k", cases.DYADIC),
                                         ("terrain_4x100k", cases.GEOREF)])
def test_culling_never_changes_a_result(octrees, name, offset):
    """CUT @ 2 and ALL @ 20: the mirror equals an exhaustive search over all selected samples of the export, with no culling, byte for byte."""
    full, pts, box, ho = octrees(name, offset)
    base_pts, base_box, _, _ = cases.case(name)
    for sel, ml in (("cut", 2), ("all", 20)):
        ex = full.truncated(ml, sel)
        for key, q in nr.query_sets(base_pts, base_box).items():
            if tuple(offset) != (0, 0, 0):
                q = nr.shift_spheres(q, offset)
            what = f"{name} {offset} {sel}@{ml} {key}"
            nb, within = full.neighbours(q, nr.K, ml, sel)
            if key == "wide":
                nr.assert_wide_not_vacuous(within, what)
            nr.assert_found_index_export(nb, ex, what)
            nr.assert_misses_behind(nb, within, nr.K, what)
            want, ww = nr.exhaustive(ex, q, nr.K)
            assert nb.tobytes() == want.tobytes(), f"{what}: queries {np.nonzero((nb != want).any(1))[0][:8]} differ from the exhaustive search"
            assert np.array_equal(within, ww), what
            sel_nb, sel_w = ex.neighbours_selected(q, nr.K)
            assert sel_nb.tobytes() == nb.tobytes() and np.array_equal(sel_w, within)


def test_lattice_ties(built_libs):
    pts, box = nr.lattice()
    full, _, _, _ = rr.host_octree(pts=pts, box=box, batch=nr.LATTICE_BATCH)
    assert int(full.nodes["childMask"][0]) != 0, "the root has not split"
    q = nr.lattice_queries()
    assert (q.record()["center"][:, 0] == 0.5).all() and (q.record()["radius"] == 1.0 / 64).all()
    for sel in ("cut", "all"):
        ex = full.truncated(20, sel)
        nb, within = full.neighbours(q, nr.LATTICE_K, 20, sel)
        want, ww = nr.exhaustive(ex, q, nr.LATTICE_K)
        assert nb.tobytes() == want.tobytes() and np.array_equal(within, ww), sel
        if sel == "cut":
            nr.assert_lattice_ties(nb, within, ex, q, "lattice cut")
            own = (pts["x"][nb["sample"]["color"][:, 0]] == 0.5).all()                       # place 0 is the point itself (colour = index)
            c = q.record()["center"]
            assert own and np.array_equal(np.stack([nb["sample"][a][:, 0] for a in "xyz"], axis=1), c)


def test_degenerate_queries(octrees):
    pts, box, batch, _ = cases.case("uniform_3x40k")
    dup = pts[np.random.RandomState(7).choice(len(pts), 500, replace=False)].copy()
    dup["color"] ^= 0x00FFFFFF
    full, _, _, _ = rr.host_octree(pts=np.concatenate([pts, dup]), box=box, batch=40_000)
    cut = full.truncated(20, "cut")
    good = nr.wide(pts, box)
    ref, ref_w = full.neighbours(good, 8)
    q, bad, odd = nr.degenerate_batch(good, box, extra=[Spheres.from_points(dup[:8], 0.0).record()])
    nbad = bad.stop - bad.start
    assert nbad == 14
    nb, within, cnt = full.neighbours(q, 8, return_counts=True)
    assert int(cnt["numInvalid"]) == nbad and (within[bad] == 0).all() and (nb["node"][bad] == NONE).all() and np.isposinf(nb["d2"][bad]).all()
    nr.assert_misses_behind(nb, within, 8, "degenerate")
    n_odd = 11
    keep = np.r_[0:8, odd + n_odd:len(q)]
    assert nb[keep].tobytes() == ref.tobytes() and np.array_equal(within[keep], ref_w)       # the good queries around them are unchanged
    # radius 0 exactly on a duplicated point: both copies, ordered by (node, ordinal)
    for i in range(8):
        r = nb[odd + i]
        assert within[odd + i] == 2 and (r["d2"][:2] == 0).all() and (r["node"][0], r["ordinal"][0]) < (r["node"][1], r["ordinal"][1])
        assert {int(r["sample"]["color"][0]), int(r["sample"]["color"][1])} == {int(dup["color"][i]), int(dup["color"][i]) ^ 0x00FFFFFF}
    # far outside with a small radius: no pair; outside with a radius that reaches in; the whole box
    single = lambda i: full.neighbours(Spheres.from_records(q.record()[i:i + 1]), 8, return_counts=True)
    assert within[odd + 8] == 0 and int(single(odd + 8)[2]["numPairs"]) == 0
    assert within[odd + 9] > 8 and int(single(odd + 9)[2]["numPairs"]) > 0
    assert within[odd + 10] == cut.num_samples
    want, ww = nr.exhaustive(cut, q, 8)
    assert nb.tobytes() == want.tobytes() and np.array_equal(within, ww)
    only_bad, w2, c2 = full.neighbours(Spheres.from_records(q.record()[bad]), 8, return_counts=True)
    assert int(c2["numPairs"]) == 0 and int(c2["numCandidates"]) == 0 and int(c2["numFound"]) == 0 and int(c2["numWithin"]) == 0 and int(c2["numInvalid"]) == nbad
    # one radius that covers the whole box of ragged_tiny
    tiny, tp, tb, _ = octrees("ragged_tiny")
    for sel in ("cut", "all"):
        _, w, c = tiny.neighbours(Spheres([[0.5, 0.5, 0.5]], 2.0), 16, 20, sel, return_counts=True)
        assert int(w[0]) == tiny.truncated(20, sel).num_samples == int(c["numCandidates"]) and (sel != "cut" or int(w[0]) == len(tp))
    with pytest.raises(ValueError):
        full.neighbours(good, 0)
    with pytest.raises(ValueError):
        full.neighbours(good, 17)


def test_rule_3_at_its_edge(octrees):
    """A centre on the root cube's widened low face minus the radius still forms pairs; one ulp further out none; diagonally off a corner a
    query within the radius of the cube on every axis fails g2 <= rr."""
    full, pts, box, ho = octrees("terrain_4x100k")
    q = nr.edge_queries(box, 0.5)
    rec = q.record()
    per = [full.neighbours(Spheres.from_records(rec[i:i + 1]), 8, return_counts=True)[2] for i in range(3)]
    pairs = [int(c["numPairs"]) for c in per]
    assert pairs[0] > 0 and pairs[1] == 0 and pairs[2] == 0, pairs
    # the third passes a per-axis test against the widened cube
    mn, size = octree_io._box_of(full.box_min, full.box_max)
    e = np.ldexp(size, -abi.MAX_DEPTH)
    c, r = rec["center"][2].astype(np.float64), np.float64(rec["radius"][2])
    ex = np.maximum(np.maximum((mn - e) - c, 0.0), c - ((mn + size) + e))
    assert (ex <= r).all() and (ex[0] * ex[0] + ex[1] * ex[1]) + ex[2] * ex[2] > r * r
    assert np.array_equal(full.spheres_per_node(q) > 0, full.spheres_per_node(Spheres.from_records(rec[:1])) > 0)
    nb, within = full.neighbours(q, 8)
    want, ww = nr.exhaustive(full.truncated(20, "cut"), q, 8)
    assert nb.tobytes() == want.tobytes() and np.array_equal(within, ww)


def test_pair_counts(octrees):
    """The culling culls: the candidates of the wide terrain set stay below 20 % of queries x samples; the counts of a batch are the sums
    over its queries; every found node is among its query's pairs."""
    full, pts, box, ho = octrees("terrain_4x100k")
    q = nr.wide(pts, box)
    nb, within, cnt = full.neighbours(q, 8, 20, "cut", return_counts=True)
    cut = full.truncated(20, "cut")
    share = int(cnt["numCandidates"]) / (len(q) * cut.num_samples)
    print("pairs", int(cnt["numPairs"]), "candidates", int(cnt["numCandidates"]), f"share {share:.3f}")
    assert share < 0.20 and int(cnt["numPairs"]) >= len(q)
    rec = q.record()
    mn, size = octree_io._box_of(full.box_min, full.box_max)
    e = np.ldexp(size, -abi.MAX_DEPTH)
    total_pairs = total_cand = 0
    for i in range(len(rec)):
        one = Spheres.from_records(rec[i:i + 1])
        n1, w1, c1 = full.neighbours(one, 8, 20, "cut", return_counts=True)
        total_pairs += int(c1["numPairs"]); total_cand += int(c1["numCandidates"])
        assert n1.tobytes() == nb[i:i + 1].tobytes() and int(w1[0]) == int(within[i])
        paired = set(np.nonzero(cut.spheres_per_node(one))[0].tolist())
        c, r = rec["center"][i].astype(np.float64), np.float64(rec["radius"][i])
        for t in set(nb["node"][i][nb["node"][i] != NONE].tolist()):
            assert t in paired, (i, t)
            while t != NONE:                                 # it and all its listed ancestors pass rule 3 for this query
                nd = cut.nodes[t]
                s = np.ldexp(size, -int(nd["level"]))
                A = np.array([nd["X"], nd["Y"], nd["Z"]], dtype=np.float64)
                ex = np.maximum(np.maximum(((mn + A * s) - e) - c, 0.0), c - ((mn + (A + 1.0) * s) + e))
                assert (ex[0] * ex[0] + ex[1] * ex[1]) + ex[2] * ex[2] <= r * r, (i, t)
                t = int(nd["parent"])
    assert total_pairs == int(cnt["numPairs"]) and total_cand == int(cnt["numCandidates"])
    # ALL selects inner nodes too: more pairs, a superset of candidates
    _, _, call = full.neighbours(q, 8, 20, "all", return_counts=True)
    assert int(call["numPairs"]) > int(cnt["numPairs"]) and int(call["numCandidates"]) > int(cnt["numCandidates"])


def test_neighbour_kernels_use_no_scratch():
    """`make resource-usage` on export.hip: the neighbour query's five kernels of its own (the pair pipeline of export_pairs.inc over NbQuery,
    k_n_test and k_n_reduce of export_neighbours.inc) keep everything in registers and LDS, and sharing the pipeline left the ray query
    as it was — six kernels, none with scratch."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "simlod_amd", "csrc"), "resource-usage", "RU_SRCS=export.hip"], capture_output=True, text=True, check=True).stdout
    blocks = re.split(r"Function Name: ", out)[1:]
    scratch = {b.split()[0]: int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) for b in blocks}
    nbk = {k: v for k, v in scratch.items() if ("k_p_" in k and "NbQuery" in k) or "k_n_" in k}
    assert len(nbk) == 5 and sum("k_p_pairs" in k for k in nbk) == 2, sorted(scratch)
    assert all(any(n in k for k in nbk) for n in ("k_p_pairs", "k_p_scan", "k_n_test", "k_n_reduce")), sorted(scratch)
    assert all(v == 0 for v in nbk.values()), nbk
    rays = {k: v for k, v in scratch.items() if "k_p_hier" in k or ("k_p_" in k and "RayQuery" in k) or "k_r_" in k}
    assert len(rays) == 6 and all(v == 0 for v in rays.values()), rays
