"""GPU tier: simlod_align_samples (include/simlod_hip.h, "align queries") through the C ABI against the host mirror
octree_io.align_samples, byte for byte — records and the summary record — with every buffer poisoned first: every case of tests/align_ref.py
with records, without and count-only; rule A10 against simlod_compare_samples itself; the bytes' independence of maxWorkgroups; hash
collisions made on purpose; the budget; grid reuse (rule A7) under other poses, a smaller radius and another maxWorkgroups, and every way a
stamp can fail to serve; every refused argument; and the ICP — DeviceOctree.register_samples on the registration scene against the mirror's
loop step by step, and register_region on a built, an imported and a shifted octree."""
import ctypes

import numpy as np
import pytest
import torch

import align_ref as ar
import compare_ref as cr
from simlod_amd import abi
from simlod_amd.octree_io import Align, Region, align_samples, register_samples
from test_gpu_compare import Raw as CompareRaw
from test_gpu_compare import _colliding, _compare, _octree, _uniforms
from util import _device

pytestmark = pytest.mark.gpu
SLACK = 64                                    # records behind numA
INVALID_VALUE = 1                             # hipErrorInvalidValue
SUMMARY = abi.align_summary_dtype.itemsize
POSES = [ar.GENERAL, ar.motion((1.0, 0.0, 0.3), -4.0, (2.0, 2.0, 2.0), (0.0, 0.1, 0.0)), np.hstack([np.eye(3), [[0.05], [0.0], [-0.05]]])]


@pytest.fixture(scope="module")
def dev(built_libs):
    return _device(persistent_bytes=1 << 28)


class Raw:
    """One simlod_align_samples call with every buffer poisoned: rc, the summary record and the buffers as the call left them.
    records=False: a null records pointer; scratch_bytes: what the call is told; offset: {name: bytes} — that pointer is passed so many
    bytes into its buffer (every buffer has 16 bytes to spare behind its content); grid: an earlier Raw whose scratch buffer and `b`
    tensor this call is given as they are (a reuse call's), other_b: with `grid`, a fresh copy of b at another address all the same."""

    def __init__(self, dev, u, a, b, record, *, records=True, scratch_bytes=None, null=(), na=None, nb=None, uniforms_record=None, offset=None, grid=None,
                 other_b=False, poison_scratch=True):
        L = dev.L
        self.na, self.nb = len(a), len(b)
        need = int(L.simlod_align_buffer_min_bytes(self.na, self.nb))
        told = need if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        up16 = lambda v: torch.from_numpy(np.concatenate([np.ascontiguousarray(v).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to(dev.device)
        self.scratch = mk(max(need, told) + 16) if grid is None else grid.scratch
        self.summary_t, self.records_t = mk(SUMMARY + SLACK), mk((self.na + SLACK) * 16)
        self.a_t = up16(a)
        self.b_t = up16(b) if grid is None or other_b else grid.b_t
        self.before = self.scratch.clone()
        uu, up = dev._u(u if uniforms_record is None else uniforms_record)
        p = np.ascontiguousarray(record)
        off = offset or {}
        dp = lambda name, t, on=True: None if name in null or not on else ctypes.c_void_p(t.data_ptr() + off.get(name, 0))
        self.rc = L.simlod_align_samples(None if "uniforms" in null else up, dp("a", self.a_t), ctypes.c_uint64(self.na if na is None else na),
                                         dp("b", self.b_t), ctypes.c_uint64(self.nb if nb is None else nb),
                                         None if "params" in null else ctypes.c_void_p(p.ctypes.data), dp("scratch", self.scratch), ctypes.c_uint64(told),
                                         dp("records", self.records_t, records), dp("summary", self.summary_t), dev._stream())
        torch.cuda.synchronize()
        self.summary = self.summary_t.cpu().numpy()[:SUMMARY].view(abi.align_summary_dtype)[0]

    def records(self):
        return self.records_t.cpu().numpy()[: self.na * 16].view(abi.compare_record_dtype)

    def slack_intact(self):
        """Nothing behind the last record or the summary was written."""
        return bool((self.records_t[self.na * 16:] == 0xA5).all()) and bool((self.summary_t[SUMMARY:] == 0xA5).all())

    def records_untouched(self):
        return bool((self.records_t == 0xA5).all())

    def untouched(self):
        return self.records_untouched() and bool((self.summary_t == 0xA5).all()) and bool((self.scratch == self.before).all())

    def scratch_kept_but_run(self):
        """The scratch buffer is what it was but for the header's `run` word (bytes 4 .. 8)."""
        now, was = self.scratch.clone(), self.before.clone()
        now[4:8], was[4:8] = 0, 0
        return bool((now == was).all())


def _params(case, pose=None, **kw):
    a, b, mn, mx, radius, grid, p = case
    return ar.params(kw.pop("radius", radius), kw.pop("grid", grid), p if pose is None else pose, **kw)


def _mirror(case, rec, count_only=False):
    a, b, mn, mx = case[:4]
    r = np.asarray(rec).reshape(-1)[0]
    return align_samples(a, b, (tuple(np.float32(mn).tolist()), tuple(np.float32(mx).tolist())), Align(r["radius"], r["gridRadius"], int(r["maxCandidates"])),
                         r["pose"].reshape(3, 4), count_only=count_only)


def _check(raw, want, what):
    """A call with records against the mirror's (records, summary)."""
    assert raw.rc == 0, what
    assert raw.summary.tobytes() == want[1].tobytes(), (what, [(f, raw.summary[f], want[1][f]) for f in abi.align_summary_dtype.names
                                                               if np.asarray(raw.summary[f]).tobytes() != np.asarray(want[1][f]).tobytes()])
    got = raw.records()
    if got.tobytes() != want[0].tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 16) != want[0].view(np.uint8).reshape(-1, 16)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} records differ, first {[(int(i), got[i], want[0][i]) for i in bad[:5]]}")
    assert raw.slack_intact(), what


GRID_ERROR = np.zeros((), dtype=abi.align_summary_dtype)
GRID_ERROR["error"] = abi.ALIGN_ERR_GRID


@pytest.mark.parametrize("name", ar.CASES)
def test_bare_call_equals_the_mirror(dev, name):
    case = ar.case(name)
    a, b, mn, mx = case[:4]
    u, box = _uniforms(dev, mn, mx)
    rec = _params(case)
    want = _mirror(case, rec)
    _check(Raw(dev, u, a, b, rec), want, name)
    # without records: a full call — the same summary — that leaves the records buffer alone (rule A6)
    r = Raw(dev, u, a, b, rec, records=False)
    assert r.rc == 0 and r.summary.tobytes() == want[1].tobytes() and r.records_untouched() and r.slack_intact()
    # count only: the grid's fields as the full call has them, the rest zero (the mirror's record), no record written though a buffer is there
    for records in (True, False):
        c = Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_COUNT_ONLY), records=records)
        assert c.rc == 0 and c.records_untouched() and c.slack_intact()
        assert c.summary.tobytes() == _mirror(case, rec, count_only=True)[1].tobytes()
        assert c.summary.tobytes()[:16] == want[1].tobytes()[:16] and int(c.summary["numCandidates"]) == int(want[1]["numCandidates"])
    if name == "rot90_lattice":                                             # b is a's array itself
        same = Raw(dev, u, a, a, rec)
        _check(same, want, name + " on itself")


@pytest.mark.parametrize("name", ["lattice", "lattice_ulp", "cell_faces", "invalid", "b_outside", "r0_duplicates", "h_floor", "hot_cell"])
def test_identity_is_the_compare_query(dev, name):
    """Rule A10: the records and the summary's fields up to maxD2 are simlod_compare_samples' on the same arrays, byte for byte."""
    a, b, mn, mx, radius = cr.case(name)
    u, box = _uniforms(dev, mn, mx)
    c = CompareRaw(dev, u, a, b, _compare(radius))
    r = Raw(dev, u, a, b, ar.params(radius))
    assert c.rc == 0 and r.rc == 0 and int(r.summary["numMatched"]) == int(c.summary["numMatched"])
    assert r.records().tobytes() == c.records().tobytes() and r.summary.tobytes()[:48] == c.summary.tobytes()[:48]


@pytest.mark.parametrize("name", ["general", "hot_cell", "invalid"])
def test_grid_independence_and_determinism(dev, name):
    """The same bytes with maxWorkgroups 1, 3 and 0, twice over."""
    case = ar.case(name)
    a, b, mn, mx = case[:4]
    u, box = _uniforms(dev, mn, mx)
    first = None
    for wg in (0, 1, 3, 0):
        r = Raw(dev, u, a, b, _params(case, wg=wg))
        assert r.rc == 0
        got = (r.records().tobytes(), r.summary.tobytes())
        first = got if first is None else first
        assert got == first, f"maxWorkgroups {wg}"
    assert first[1] == _mirror(case, _params(case))[1].tobytes()


def test_hash_collisions_made_on_purpose(dev):
    rs = np.random.RandomState(23)
    radius, (mn, mx) = 0.02, ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    u, box = _uniforms(dev, mn, mx)
    b, n_hot, slots = _colliding(radius, 4.0, 700, rs)                      # 64+ cells with one home slot, their probe run wrapping the table's end
    assert slots == 2048 and n_hot >= 64
    pose = ar.motion((0.0, 0.0, 1.0), 0.2, (0.5, 0.5, 0.5), (0.002, 0.0, -0.001))
    near = cr.points(np.concatenate([np.stack([b["x"], b["y"], b["z"]], -1)[:400].astype(np.float64) + (rs.rand(400, 3) - 0.5) * 0.02, rs.rand(200, 3) * 1.3]))
    a = ar.moved(near, ar.inverse(pose))
    case = (a, b, mn, mx, radius, radius, pose)
    want = _mirror(case, _params(case))
    assert int(want[1]["numMatched"]) >= 250
    _check(Raw(dev, u, a, b, _params(case)), want, "collisions")
    build = Raw(dev, u, a, b, _params(case), records=False)
    _check(Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_REUSE_GRID), grid=build), want, "collisions, reused")


def test_budget(dev):
    case = ar.case("hot_cell")
    a, b, mn, mx = case[:4]
    u, box = _uniforms(dev, mn, mx)
    n = int(Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_COUNT_ONLY)).summary["numCandidates"])
    assert n > 1
    for budget, runs in ((n + 1, True), (n, True), (n - 1, False)):
        rec = _params(case, budget=budget)
        r = Raw(dev, u, a, b, rec)
        want = _mirror(case, rec)
        assert r.rc == 0 and r.summary.tobytes() == want[1].tobytes() and int(r.summary["error"]) == (0 if runs else abi.ALIGN_ERR_BUDGET), budget
        if runs:
            _check(r, want, f"budget {budget}")
        else:
            assert want[0] is None and r.records_untouched() and int(r.summary["numCandidates"]) == n and int(r.summary["numCells"]) == 1
            assert not r.summary.tobytes()[40:].strip(b"\0")
            # the grid stands all the same: a reuse call with a budget that fits runs on it
            again = Raw(dev, u, a, b, _params(case, budget=n, flags=abi.ALIGN_REUSE_GRID), grid=r)
            _check(again, _mirror(case, _params(case, budget=n)), "reuse after a budget error")


def test_reuse_equals_a_fresh_build(dev):
    """Rule A9: after ONE build call, reuse calls under three other poses, a smaller radius and other maxWorkgroups return the bytes a
    build call with the same arguments returns — the mirror's."""
    case = ar.case("small_radius")
    a, b, mn, mx, radius, grid, pose = case
    u, box = _uniforms(dev, mn, mx)
    build = Raw(dev, u, a, b, _params(case, radius=grid), records=False)    # built at radius == gridRadius
    assert build.rc == 0 and int(build.summary["error"]) == 0
    seen = set()
    for p in POSES + [pose]:
        for kw in (dict(), dict(radius=radius), dict(radius=0.0), dict(wg=1), dict(wg=3, radius=radius)):
            fresh = Raw(dev, u, a, b, _params(case, pose=p, **dict(dict(radius=grid), **kw)))
            again = Raw(dev, u, a, b, _params(case, pose=p, flags=abi.ALIGN_REUSE_GRID, **dict(dict(radius=grid), **kw)), grid=build)
            want = _mirror(case, _params(case, pose=p, **dict(dict(radius=grid), **kw)))
            _check(fresh, want, ("fresh", kw))
            _check(again, want, ("reused", kw))
            seen.add(again.summary.tobytes())
    assert len(seen) >= 8
    # a count-only reuse call reads the table alone; without records the reuse call is the ICP's
    c = Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_REUSE_GRID | abi.ALIGN_COUNT_ONLY), grid=build)
    assert c.rc == 0 and c.summary.tobytes() == _mirror(case, _params(case), count_only=True)[1].tobytes() and c.records_untouched()
    n = Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_REUSE_GRID), grid=build, records=False)
    assert n.rc == 0 and n.summary.tobytes() == _mirror(case, _params(case))[1].tobytes() and n.records_untouched()


def test_a_stamp_that_does_not_serve(dev):
    """Rule A7: SIMLOD_ALIGN_ERR_GRID, a summary of zeroes otherwise, no record, and a scratch buffer that is what it was but for `run`."""
    case = ar.case("general")
    a, b, mn, mx, radius, grid, pose = case
    u, box = _uniforms(dev, mn, mx)
    reuse = _params(case, flags=abi.ALIGN_REUSE_GRID)

    def refused_by_stamp(r, what):
        assert r.rc == 0 and r.summary.tobytes() == GRID_ERROR.tobytes(), what
        assert r.records_untouched() and r.slack_intact() and r.scratch_kept_but_run(), what

    # a scratch buffer no call ever stamped
    for records in (True, False):
        refused_by_stamp(Raw(dev, u, a, b, reuse, records=records), "poisoned scratch")
    refused_by_stamp(Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_REUSE_GRID | abi.ALIGN_COUNT_ONLY)), "poisoned scratch, count only")
    # a count-only build leaves the grid records unfilled: a count-only reuse is served, a full one is not
    counted = Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_COUNT_ONLY))
    assert counted.rc == 0
    c = Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_REUSE_GRID | abi.ALIGN_COUNT_ONLY), grid=counted)
    assert c.rc == 0 and c.summary.tobytes() == counted.summary.tobytes()
    refused_by_stamp(Raw(dev, u, a, b, reuse, grid=counted), "after a count-only build")
    # a full build, then: another gridRadius, another b of equal length, another numB, another box
    build = Raw(dev, u, a, b, _params(case))
    want = _mirror(case, _params(case))
    _check(build, want, "build")
    refused_by_stamp(Raw(dev, u, a, b, _params(case, grid=np.float32(grid) * np.float32(1.5), flags=abi.ALIGN_REUSE_GRID), grid=build), "another gridRadius")
    refused_by_stamp(Raw(dev, u, a, b, reuse, grid=build, other_b=True), "another b")
    refused_by_stamp(Raw(dev, u, a, b, reuse, grid=build, nb=len(b) - 1), "another numB")
    u2, _ = _uniforms(dev, (0.0, 0.0, -0.5), (4.0, 4.0, 3.5))
    refused_by_stamp(Raw(dev, u2, a, b, reuse, grid=build), "another box")
    # and the grid still serves the call it was built for
    _check(Raw(dev, u, a, b, reuse, grid=build), want, "reuse after the refusals")
    # the compare query clears the stamp: its scratch is never honoured
    cmp = _compare(radius).record()
    out = torch.zeros(abi.compare_summary_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    uu, up = dev._u(u)
    rc = dev.L.simlod_compare_samples(up, ctypes.c_void_p(build.a_t.data_ptr()), ctypes.c_uint64(len(a)), ctypes.c_void_p(build.b_t.data_ptr()), ctypes.c_uint64(len(b)),
                                      ctypes.c_void_p(cmp.ctypes.data), ctypes.c_void_p(build.scratch.data_ptr()), ctypes.c_uint64(build.scratch.numel() - 16), None, None,
                                      ctypes.c_void_p(out.data_ptr()), dev._stream())
    torch.cuda.synchronize()
    assert rc == 0
    refused_by_stamp(Raw(dev, u, a, b, reuse, grid=build), "after a compare call on the buffer")


def test_refused_arguments(dev):
    case = ar.case("general")
    a, b, mn, mx, radius, grid, pose = case
    u, box = _uniforms(dev, mn, mx)
    good = _params(case)
    refused = lambda record=good, **kw: (lambda r: r.rc == INVALID_VALUE and r.untouched())(Raw(dev, u, a, b, record, **kw))
    for name in ("uniforms", "a", "b", "params", "scratch", "summary"):
        assert refused(null=(name,)), name
    for n in (0, (1 << 32) - 1, 1 << 32, 1 << 40):
        assert refused(na=n) and refused(nb=n), n
    bad_pose = lambda k, v: [v if i == k else x for i, x in enumerate(ar.IDENTITY)]
    for what, rec in (("radius < 0", ar.params(-1.0, 1.0)), ("radius NaN", ar.params(np.nan, 1.0)), ("radius inf", ar.params(np.inf, np.inf)),
                      ("gridRadius < radius", ar.params(0.25, 0.2)), ("gridRadius NaN", ar.params(0.25, np.nan)), ("gridRadius inf", ar.params(0.25, np.inf)),
                      ("reserved", ar.params(0.25, reserved=1)), ("flag 4", ar.params(0.25, flags=4)), ("flag 2^31", ar.params(0.25, flags=0x80000002)),
                      ("pose NaN", ar.params(0.25, pose=bad_pose(5, np.nan))), ("pose inf", ar.params(0.25, pose=bad_pose(3, np.inf))),
                      ("pose -inf", ar.params(0.25, pose=bad_pose(8, -np.inf)))):
        assert not ar.params_acceptable(rec) and refused(rec), what
    for what, change in (("no extent", dict(boxMax=(0.0, 0.0, 0.0))), ("NaN corner", dict(boxMin=(np.nan, 0.0, 0.0))), ("infinite extent", dict(boxMax=(np.inf, 4.0, 4.0))),
                         ("negative extent", dict(boxMin=(5.0, 5.0, 5.0)))):
        uu = np.array(u, copy=True).reshape(1)
        for k, v in change.items():
            uu[k][0] = v
        assert refused(uniforms_record=uu), what
    # alignment: a, b, scratch and records at 16 bytes, the summary at 8
    for name, by in (("a", 8), ("a", 4), ("b", 8), ("b", 1), ("scratch", 8), ("records", 8), ("records", 4), ("summary", 4)):
        assert refused(offset={name: by}), (name, by)
    ok = Raw(dev, u, a, b, good, offset={"a": 16, "b": 16, "summary": 8, "records": 16})     # aligned offsets are taken
    assert ok.rc == 0 and int(ok.summary_t.cpu().numpy()[8:8 + SUMMARY].view(abi.align_summary_dtype)[0]["numMatched"]) > 0
    # the scratch bound: one byte less is refused, the exact size is accepted — and suffices; a reuse call is held to the same bound
    need = int(dev.L.simlod_align_buffer_min_bytes(len(a), len(b)))
    assert need == int(dev.L.simlod_compare_buffer_min_bytes(len(a), len(b))) + 1024 * 256
    assert refused(scratch_bytes=need - 1) and refused(scratch_bytes=int(dev.L.simlod_compare_buffer_min_bytes(len(a), len(b))))
    build = Raw(dev, u, a, b, good, scratch_bytes=need)
    _check(build, _mirror(case, good), "exact scratch")
    short = Raw(dev, u, a, b, _params(case, flags=abi.ALIGN_REUSE_GRID), grid=build, scratch_bytes=need - 1)
    assert short.rc == INVALID_VALUE and short.untouched()


def test_the_python_call(dev):
    """DeviceOctree.align_samples: the house budget of 64 candidates per sample of a, the opt-out, records on request, reuse by hand."""
    case = ar.case("hot_cell")
    a, b, mn, mx, radius, grid, pose = case
    u, box = _uniforms(dev, mn, mx)
    al = Align(radius, grid)
    n = int(align_samples(a, b, box, al, pose, count_only=True)[1]["numCandidates"])
    assert n > dev.COMPARE_BUDGET_PER_SAMPLE * len(a)
    rec, s = dev.align_samples(u, a, b, al, pose, records=True)
    assert rec is None and int(s["error"]) == abi.ALIGN_ERR_BUDGET and int(s["numCandidates"]) == n
    want = align_samples(a, b, box, al, pose)
    rec, s = dev.align_samples(u, a, b, al, pose, records=True, max_candidates=0)
    assert rec.cpu().numpy().tobytes() == want[0].tobytes() and s.tobytes() == want[1].tobytes()
    assert dev.align_samples(u, a, b, al, pose, max_candidates=0)[0] is None
    assert dev.align_samples(u, a, b, al, pose, count_only=True, max_candidates=0)[1].tobytes() == align_samples(a, b, box, al, pose, count_only=True)[1].tobytes()
    tb, scratch = dev._samples_tensor(b), dev.align_scratch(a, b)
    assert dev.align_samples(u, a, tb, al, pose, scratch=scratch, max_candidates=0)[1].tobytes() == want[1].tobytes()
    for p in POSES:
        got = dev.align_samples(u, a, tb, al, p, scratch=scratch, reuse=True, max_candidates=0)[1]
        assert got.tobytes() == align_samples(a, b, box, al, p)[1].tobytes()
    assert int(dev.align_samples(u, a, tb, al, pose, scratch=dev.align_scratch(a, b).fill_(0), reuse=True, max_candidates=0)[1]["error"]) == abi.ALIGN_ERR_GRID
    with pytest.raises(ValueError):
        dev.align_samples(u, a, tb, al, pose, reuse=True)


def test_register_samples_on_the_scene(dev):
    """Every step's summary equals the mirror loop's, byte for byte: the final pose is therefore the mirror's, and within the same 4e-6."""
    a, b, original = ar.scene()
    u, box = _uniforms(dev, *ar.SCENE_BOX)
    al = Align(ar.SCENE_RADIUS, max_candidates=0)
    want = register_samples(a, b, box, al, iterations=ar.SCENE_STEPS)
    res = dev.register_samples(u, a, b, al, iterations=ar.SCENE_STEPS)
    assert res.steps == want.steps <= ar.SCENE_STEPS and res.converged and want.converged
    for i, (g, w) in enumerate(zip(res.summaries, want.summaries)):
        assert g.tobytes() == w.tobytes(), i
    assert res.pose.tobytes() == want.pose.tobytes() and res.rms == want.rms
    back = res.transform(dev._samples_tensor(a)).cpu().numpy().view(abi.point_dtype)
    assert back.tobytes() == want.transform(a).tobytes()
    err = max(float(np.abs(back[n].astype(np.float64) - original[n].astype(np.float64)).max()) for n in "xyz")
    print(f"steps {res.steps}, rms {['%.3g' % r for r in res.rms]}, largest error {err:.3g}")
    assert err <= ar.SCENE_BOUND
    from simlod_amd.runtime import SimlodError
    with pytest.raises(SimlodError, match="numCandidates.*maxCellPopulation"):
        dev.register_samples(u, a, b, Align(ar.SCENE_RADIUS, max_candidates=10), iterations=3)


@pytest.mark.parametrize("kind", ["built", "imported", "shifted"])
def test_register_region_through_octrees(built_libs, kind):
    dev, u, box, box_min = _octree(kind)
    size = float(max(box))
    centre = np.asarray(box_min, np.float64) + 0.5 * size
    boxes = (Region.from_box(tuple(centre - f * size), tuple(centre + f * size)) for f in (0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5))
    region = next(r for r in boxes if int(dev.count_region(u, r, 20, "all")["numSamples"]) >= 2000)     # a few thousand samples around the centre
    a, b = dev.query_region(u, region, 20, "all"), dev.export_octree(u)
    assert 2000 <= a.num_samples < b.num_samples and b.num_samples > 50_000
    start = ar.motion((0.1, 0.2, 1.0), 0.5, centre, (0.004 * size, -0.003 * size, 0.002 * size))      # a part of the octree against the whole, pushed off
    al = Align(0.02 * size, max_candidates=0)
    res = dev.register_region(u, dev, region, al, pose=start, iterations=8, max_level=20, select="all", other_select="all")
    assert res.a.samples.tobytes() == a.samples.tobytes() and res.b.samples.tobytes() == b.samples.tobytes() and res.selection["region"] is region
    want = register_samples(a.samples, b.samples, (b.box_min, b.box_max), al, pose=start, iterations=8)
    assert res.steps == want.steps >= 2 and res.converged == want.converged
    for i, (g, w) in enumerate(zip(res.summaries, want.summaries)):
        assert g.tobytes() == w.tobytes(), i
    assert res.pose.tobytes() == want.pose.tobytes() and res.rms[-1] < res.rms[0]
    assert int(res.summaries[0]["numSummed"]) > a.num_samples // 2
    c = dev.count_align(u, dev, region, al, pose=start, max_level=20, select="all", other_select="all")
    assert c.tobytes()[:16] == res.summaries[0].tobytes()[:16] and int(c["numCandidates"]) == int(res.summaries[0]["numCandidates"]) and int(c["numMatched"]) == 0
    assert res.transform(res.a.samples_tensor).cpu().numpy().tobytes() == want.transform(a.samples).tobytes()
