"""CPU tier of the align queries (include/simlod_hip.h, "align queries"): the numpy mirror octree_io.align_samples against the per-sample
restatement tests/align_ref.py, byte for byte in the records and the summary, on every case; what the cases cover; the ABI records' sizes
and offsets against the header's; align_solve on hand-made sums and on known motions; compose_pose; AlignResult.transform; and the mirror's
own ICP on the registration scene, which must bring every sample of A back to within 4e-6 of where it was in 12 steps."""
import os
import re

import numpy as np
import pytest

import align_ref as ar
import compare_ref as cr
from simlod_amd import abi
from simlod_amd.octree_io import (Align, AlignResult, align_pose_points, align_samples, align_solve, bounding_corners, compare_samples, compose_pose,
                                  register_samples)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mirror(name, budget=0, count_only=False):
    a, b, mn, mx, radius, grid, pose = ar.case(name)
    return align_samples(a, b, (mn, mx), Align(radius, grid, budget), pose, count_only=count_only)


@pytest.fixture(scope="module")
def exact():
    return {name: ar.exact(name) for name in ar.CASES}


@pytest.mark.parametrize("name", ar.CASES)
def test_mirror_equals_the_reference(exact, name):
    want, got = exact[name], _mirror(name)
    assert got[1].tobytes() == want[1].tobytes(), [(f, got[1][f], want[1][f]) for f in abi.align_summary_dtype.names if np.asarray(got[1][f]).tobytes() != np.asarray(want[1][f]).tobytes()]
    assert got[0].tobytes() == want[0].tobytes()
    # count only, and a budget one below the count: the grid's fields alone, the rest zero, no records
    n = int(want[1]["numCandidates"])
    for kw in (dict(count_only=True), dict(budget=n - 1)) if n > 1 else (dict(count_only=True),):
        w, g = ar.exact(name, max_candidates=kw.get("budget", 0), count_only=kw.get("count_only", False)), _mirror(name, **kw)
        assert w[0] is None and g[0] is None and g[1].tobytes() == w[1].tobytes()
        assert int(g[1]["error"]) == (abi.ALIGN_ERR_BUDGET if "budget" in kw else 0) and int(g[1]["numCandidates"]) == n
        assert not g[1].tobytes()[40:].strip(b"\0")                         # every field after numCandidates is zero
    assert _mirror(name, budget=n)[1].tobytes() == want[1].tobytes()


def test_what_the_cases_cover(exact):
    s = {name: exact[name][1] for name in ar.CASES}
    r = {name: exact[name][0] for name in ar.CASES}
    # the lattice under the exact quarter turn: every sample lands on a lattice point, ties at d2 == rr, the lowest index wins
    assert (r["rot90_lattice"]["d2"] == 0.0).all() and r["rot90_lattice"]["within"].max() == 7 and int(s["rot90_lattice"]["sqLo"]) == 0
    a, b = ar.case("rot90_lattice")[:2]
    near = b[r["rot90_lattice"]["nearest"]]
    assert (near["x"] == 2.5 - a["y"]).all() and (near["y"] == a["x"]).all() and (near["z"] == a["z"]).all()
    assert (r["radius_0"]["within"] == 1).all() and r["radius_0"].tobytes() != r["rot90_lattice"].tobytes()
    assert int(s["radius_0"]["numCells"]) == int(s["rot90_lattice"]["numCells"])            # the grid is gridRadius's
    assert int(s["small_radius"]["numCells"]) < int(s["general"]["numCells"]) and int(s["small_radius"]["numCandidates"]) > int(s["general"]["numCandidates"])
    assert int(s["small_radius"]["numWithin"]) < int(s["general"]["numWithin"])
    # the overflow: exactly the samples with |z| = 1e38 are invalid, and they alone
    a = ar.case("overflow")[0]
    assert int(s["overflow"]["numInvalidA"]) == int((np.abs(a["z"]) > 1e37).sum()) == 13 and np.isfinite(a["z"]).all()
    assert (r["overflow"]["nearest"][np.abs(a["z"]) > 1e37] == ar.MISS).all() and int(s["overflow"]["numMatched"]) > 40
    # Q's edges: see the case; 3 pairs inside, 4 with a coordinate at or beyond min + size or below min
    assert (int(s["edges"]["numMatched"]), int(s["edges"]["numSummed"]), int(s["edges"]["numOutside"])) == (7, 3, 4)
    a, b, mn, mx, radius, grid, pose = ar.case("edges")
    cp = align_pose_points(a, pose)[1]
    assert cp[0][0] == np.nextafter(16.0, 0.0) and cp[1][0] == 0.0 and cp[1][1] == 16.0
    assert ar.q_of(float(cp[0][0]), 0.0, ar.invq_of(16.0)) == (True, (1 << 24) - 1) and ar.q_of(16.0, 0.0, ar.invq_of(16.0)) == (False, 0)
    assert r["edges"]["nearest"][0] == 0 and b["x"][0] == 16.0             # c' one step below min + size (inside), its nearest s ON it (outside)
    # c' outside with s inside and the reverse
    assert (int(s["outside_pairs"]["numMatched"]), int(s["outside_pairs"]["numSummed"]), int(s["outside_pairs"]["numOutside"])) == (6, 1, 5)
    assert int(s["b_outside"]["numOutside"]) == int(s["b_outside"]["numMatched"]) > 0 and int(s["b_outside"]["numSummed"]) == 0
    assert int(s["hot_cell"]["numCells"]) == 1 and int(s["hot_cell"]["maxCellPopulation"]) == 300
    assert int(s["invalid"]["numInvalidA"]) >= 6 and int(s["invalid"]["numInvalidB"]) >= 6 and int(s["invalid"]["numSummed"]) > 50
    assert int(s["cell_faces"]["numMatched"]) == 36
    assert int(s["two_pairs"]["numSummed"]) == 2 and align_solve(s["two_pairs"], (0, 0, 0), 4.0) is None
    for name in ar.CASES:
        assert int(s[name]["numSummed"]) + int(s[name]["numOutside"]) == int(s[name]["numMatched"]), name


def test_identity_is_the_compare_query():
    """Rule A10: under the identity pose with gridRadius == radius the records and the shared summary fields are compare_samples'."""
    from test_compare_io import _compare                                    # (the compare tier's parameters)
    for name in ("lattice", "lattice_ulp", "cell_faces", "invalid", "b_outside", "r0_duplicates", "h_floor"):
        a, b, mn, mx, radius = cr.case(name)
        want = compare_samples(a, b, (mn, mx), _compare(radius))
        got = align_samples(a, b, (mn, mx), Align(radius), None)
        assert got[0].tobytes() == want[0].tobytes(), name
        assert got[1].tobytes()[:48] == want[2].tobytes()[:48], name


def test_abi_records():
    text = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    for struct, dtype in (("SimlodAlignParams", abi.align_params_dtype), ("SimlodAlignSummary", abi.align_summary_dtype)):
        size = re.search(r"SIMLOD_STATIC_ASSERT\(sizeof\(%s\) == (\d+)," % struct, text)
        assert size and int(size.group(1)) == dtype.itemsize
        offsets = dict(re.findall(r"SIMLOD_STATIC_ASSERT\(offsetof\(%s, (\w+)\) == (\d+)," % struct, text))
        for name in dtype.names:
            at = dtype.fields[name][1]
            assert at == 0 or name in offsets or abi.compare_summary_dtype.fields[name][1] == at, name
            if name in offsets:
                assert int(offsets[name]) == at, name
    assert len(re.findall(r"SIMLOD_STATIC_ASSERT\(offsetof\(SimlodAlignSummary, \w+\) == offsetof\(SimlodCompareSummary", text)) == 9
    for name in abi.compare_summary_dtype.names[:-1]:                       # the shared fields at the compare summary's offsets
        assert abi.align_summary_dtype.fields[name] == abi.compare_summary_dtype.fields[name]
    for c in ("SIMLOD_ALIGN_ERR_BUDGET  0x1u", "SIMLOD_ALIGN_ERR_GRID    0x2u", "SIMLOD_ALIGN_COUNT_ONLY  0x1u", "SIMLOD_ALIGN_REUSE_GRID  0x2u"):
        assert "#define " + c in text
    assert (abi.ALIGN_ERR_BUDGET, abi.ALIGN_ERR_GRID, abi.ALIGN_COUNT_ONLY, abi.ALIGN_REUSE_GRID) == (1, 2, 1, 2)
    rec = Align(0.25, 0.5, 7, 3).record(ar.GENERAL, abi.ALIGN_REUSE_GRID)
    assert rec.tobytes() == ar.params(0.25, 0.5, ar.GENERAL, abi.ALIGN_REUSE_GRID, 7, 3).tobytes() and ar.params_acceptable(rec)
    assert Align.from_record(rec) == Align(0.25, 0.5, 7, 3) and Align(0.25) == Align(0.25, 0.25) and Align(0.25) != Align(0.25, 0.5)
    assert Align(0.25, 0.5).with_radius(0.1) == Align(0.1, 0.5)
    for bad in (dict(radius=-1.0), dict(radius=np.nan), dict(radius=1.0, grid_radius=0.5), dict(radius=1.0, grid_radius=np.inf), dict(radius=1.0, max_candidates=-1)):
        with pytest.raises(ValueError):
            Align(**bad)
    with pytest.raises(ValueError):
        Align(1.0).record(np.full(12, np.nan))


def test_library_sizes(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_align_buffer_min_bytes", "simlod_align_samples"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    for na, nb in ((1, 1), (5, 1000), (1000, 5), ((1 << 32) - 2, 3)):
        assert int(L.simlod_align_buffer_min_bytes(na, nb)) == int(L.simlod_compare_buffer_min_bytes(na, nb)) + 1024 * 256
    for na, nb in ((0, 5), (5, 0), ((1 << 32) - 1, 5), (5, 1 << 32)):
        assert int(L.simlod_align_buffer_min_bytes(na, nb)) == 0


def _summary_of(pa, pb, box_min, size):
    """The sums of rule A5 over hand-made pairs (float64 positions), as a summary record."""
    out = np.zeros((), dtype=abi.align_summary_dtype)
    invq = ar.invq_of(size)
    for p, q in zip(pa, pb):
        qa, qb = [ar.q_of(float(p[k]), box_min[k], invq) for k in range(3)], [ar.q_of(float(q[k]), box_min[k], invq) for k in range(3)]
        assert all(v[0] for v in qa + qb)
        out["numSummed"] += 1
        for k in range(3):
            out["sumA"][k] += qa[k][1]
            out["sumB"][k] += qb[k][1]
            for l in range(3):
                lo, hi = ar.lo_hi(qa[k][1] * qb[l][1])
                out["crossLo"][3 * k + l] += lo
                out["crossHi"][3 * k + l] += hi
        e = [qb[k][1] - qa[k][1] for k in range(3)]
        lo, hi = ar.lo_hi((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        out["sqLo"] += lo
        out["sqHi"] += hi
    out["numMatched"] = out["numSummed"]
    return out


def test_align_solve():
    rs = np.random.RandomState(3)
    step = 16.0 / (1 << 24)                                                 # one step of Q in a box of size 16
    # a pure shift by whole steps of Q, on positions in the middle of their steps: exact
    pa = (rs.randint(1 << 20, 1 << 23, (50, 3)) + 0.5) * step
    shift = np.array([1000, -2000, 37]) * step
    upd, rms = align_solve(_summary_of(pa, pa + shift, (0.0, 0.0, 0.0), 16.0), (0.0, 0.0, 0.0), 16.0)
    assert np.abs(upd[:, :3] - np.eye(3)).max() < 1e-12 and np.abs(upd[:, 3] - shift).max() < 1e-9
    assert abs(rms - np.linalg.norm(shift)) < 1e-12
    # known motions, in a box off the origin: recovered to the quantisation's step
    mn = (100.0, -50.0, 7.0)
    for axis, deg, shift in (((0.0, 0.0, 1.0), 90.0, (0.0, 0.0, 0.0)), ((0.2, -0.1, 1.0), 3.0, (0.08, -0.05, 0.04)), ((1.0, 1.0, 1.0), -140.0, (-0.5, 0.25, 1.0))):
        truth = ar.motion(axis, deg, np.array(mn) + 8.0, shift)
        pa = np.array(mn) + 5.0 + rs.rand(400, 3) * 6.0
        pb = pa @ truth[:, :3].T + truth[:, 3]
        upd, rms = align_solve(_summary_of(pa, pb, mn, 16.0), mn, 16.0)
        assert np.abs(upd[:, :3] @ upd[:, :3].T - np.eye(3)).max() < 1e-12 and np.linalg.det(upd[:, :3]) > 0.999
        assert np.abs((pa @ upd[:, :3].T + upd[:, 3]) - pb).max() < 4 * step, (axis, deg)
        assert abs(rms - np.sqrt(((pb - pa) ** 2).sum(-1).mean())) < 4 * step
    # a reflection would fit mirrored pairs better: the determinant's sign is corrected, the result is still a rotation
    pa = np.array(mn) + 5.0 + rs.rand(100, 3) * 6.0
    pb = pa.copy()
    pb[:, 0] = 2 * (mn[0] + 8.0) - pb[:, 0]
    upd, _ = align_solve(_summary_of(pa, pb, mn, 16.0), mn, 16.0)
    assert np.linalg.det(upd[:, :3]) > 0.999
    # fewer than 3 pairs, and pairs on one line (the second singular value is 0): nothing to solve
    two = _summary_of(pa[:2], pb[:2], mn, 16.0)
    assert align_solve(two, mn, 16.0) is None and align_solve(np.zeros((), abi.align_summary_dtype), mn, 16.0) is None
    line = np.array(mn) + np.outer(np.arange(1, 9), [1.0, 0.0, 0.0])
    assert align_solve(_summary_of(line, line, mn, 16.0), mn, 16.0) is None
    same = np.repeat(np.array(mn).reshape(1, 3) + 3.0, 5, axis=0)
    assert align_solve(_summary_of(same, same, mn, 16.0), mn, 16.0) is None
    # the sums are read as hi * 2^32 + lo in integers of any size: n * cross near 2^80 loses nothing
    big = _summary_of(pa, pa, mn, 16.0)
    assert np.abs(align_solve(big, mn, 16.0)[0] - np.hstack([np.eye(3), np.zeros((3, 1))])).max() < 1e-9


def test_compose_and_transform():
    p, q = ar.motion((0.0, 0.0, 1.0), 90.0, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0)), ar.motion((1.0, 0.0, 0.0), 90.0, (0.0, 0.0, 0.0), (0.5, 0.0, 0.0))
    x = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 9.0]])
    both = compose_pose(q, p)
    assert np.abs((x @ both[:, :3].T + both[:, 3]) - ((x @ p[:, :3].T + p[:, 3]) @ q[:, :3].T + q[:, 3])).max() < 1e-12
    assert np.abs(compose_pose(ar.inverse(p), p) - np.hstack([np.eye(3), np.zeros((3, 1))])).max() < 1e-12
    a, _, _, _, _, _, pose = ar.case("overflow")
    out = AlignResult(pose, [], [], True).transform(a)
    valid, cp = align_pose_points(a, pose)
    assert out["color"].tobytes() == a["color"].tobytes() and out["x"][valid].tobytes() == cp[0][valid].astype(np.float32).tobytes()
    assert np.isinf(out["x"][~valid]).all() and (out["z"] == a["z"]).all()
    assert bounding_corners(a).shape == (8, 3) and bounding_corners(a)[7].tolist() == [float(a[n].max()) for n in "xyz"]
    bad = a[:3].copy()
    bad["x"] = np.nan
    assert len(bounding_corners(bad)) == 0


def test_mirror_icp_on_the_scene():
    """The issue's bound: within 12 steps every sample of A lands within 4e-6 — four fp32 steps at 8 — of where it was."""
    a, b, original = ar.scene()
    assert len(b) == 6000 and len(a) == 2000
    res = register_samples(a, b, ar.SCENE_BOX, Align(ar.SCENE_RADIUS, max_candidates=0), iterations=ar.SCENE_STEPS)
    back = res.transform(a)
    err = max(float(np.abs(back[n].astype(np.float64) - original[n].astype(np.float64)).max()) for n in "xyz")
    print(f"steps {res.steps}, converged {res.converged}, rms {['%.3g' % r for r in res.rms]}, largest error {err:.3g}")
    assert res.steps <= ar.SCENE_STEPS and err <= ar.SCENE_BOUND
    assert res.converged and len(res.rms) == res.steps and all(int(s["error"]) == 0 for s in res.summaries)
    assert int(res.summaries[-1]["numSummed"]) == len(a) and res.rms[-1] < 2e-6 < res.rms[0]
    truth = ar.motion((0.2, -0.1, 1.0), 3.0, (5.0, 5.0, 2.0), (0.08, -0.05, 0.04))
    assert np.abs(res.pose - truth).max() < 1e-6
    # a start that is already right stops after one step; a budget exceeded ends the loop with its error bit
    again = register_samples(a, b, ar.SCENE_BOX, Align(ar.SCENE_RADIUS, max_candidates=0), pose=res.pose, iterations=5)
    assert again.steps == 1 and again.converged
    over = register_samples(a, b, ar.SCENE_BOX, Align(ar.SCENE_RADIUS, max_candidates=10), iterations=5)
    assert over.steps == 1 and not over.converged and int(over.summaries[0]["error"]) == abi.ALIGN_ERR_BUDGET and np.array_equal(over.pose[:, :3], np.eye(3))
