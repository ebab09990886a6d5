"""GPU tier: simlod_compare_samples (include/simlod_hip.h, "compare queries") through the C ABI against the host mirror
octree_io.compare_samples, byte for byte — records, colours and the summary record — with every buffer poisoned first: the smallest shapes at
which the hash grid can go wrong (tests/compare_ref.py case), hash collisions made on purpose, the count-only form, the budget, every refused
argument, the grid's independence of maxWorkgroups; and through octrees (DeviceOctree.compare_region, CompareResult.paint): an octree against
itself, against itself with a slab erased, and the colours painted back and undone, on a built, an imported and a shifted octree."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import compare_ref as cr
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Compare, Paint, Region, compare_cells, compare_h, compare_home, compare_samples
from util import _build, _device

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
SLACK = 64                                    # records and colour words behind numA
PALETTE = [0xFF0000FF, 0xFF00FFFF, 0xFF00FF00, 0xFFFF0000]
MISS = 0xFF123456
INVALID_VALUE = 1                             # hipErrorInvalidValue
GRID_FIELDS = ("error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numCandidates")


def _compare(radius, **kw):
    return Compare.linear(0.75 * radius if radius > 0 else 1.0, PALETTE, radius=radius, miss_color=MISS, **kw)


@pytest.fixture(scope="module")
def dev(built_libs):
    return _device(persistent_bytes=1 << 28)


def _uniforms(dev, mn, mx):
    box = tuple(float(np.float32(b) - np.float32(a)) for a, b in zip(mn, mx))
    u = dev.uniforms(W, H, cases._cam(box), box, box_min=tuple(float(v) for v in mn))
    rec = np.asarray(u).reshape(-1)[0]
    return u, (tuple(float(v) for v in rec["boxMin"]), tuple(float(v) for v in rec["boxMax"]))


class Raw:
    """One simlod_compare_samples call with every buffer poisoned: rc, the summary record and the buffers as the call left them.
    results=False: records and colours are null pointers (count only); colors=False: colours alone; scratch_bytes: what the call is told;
    offset: {name: bytes} — that pointer is passed so many bytes into its buffer (every buffer has 16 bytes to spare behind its content)."""

    def __init__(self, dev, u, a, b, cmp, *, results=True, colors=True, scratch_bytes=None, record=None, null=(), na=None, nb=None, uniforms_record=None, offset=None):
        L = dev.L
        self.na, self.nb = len(a), len(b)
        need = int(L.simlod_compare_buffer_min_bytes(self.na, self.nb))
        told = need if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        self.scratch, self.summary_t = mk(max(need, told) + 16), mk(abi.compare_summary_dtype.itemsize + SLACK)
        self.records_t, self.colors_t = mk((self.na + SLACK) * 16), mk((self.na + SLACK) * 4)
        up16 = lambda v: torch.from_numpy(np.concatenate([np.ascontiguousarray(v).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to(dev.device)
        self.a_t, self.b_t = up16(a), up16(b)
        uu, up = dev._u(u if uniforms_record is None else uniforms_record)
        p = cmp.record() if record is None else record
        off = offset or {}
        dp = lambda name, t, on=True: None if name in null or not on else ctypes.c_void_p(t.data_ptr() + off.get(name, 0))
        self.rc = L.simlod_compare_samples(None if "uniforms" in null else up, dp("a", self.a_t), ctypes.c_uint64(self.na if na is None else na),
                                           dp("b", self.b_t), ctypes.c_uint64(self.nb if nb is None else nb),
                                           None if "params" in null else ctypes.c_void_p(p.ctypes.data), dp("scratch", self.scratch), ctypes.c_uint64(told),
                                           dp("records", self.records_t, results), dp("colors", self.colors_t, results and colors),
                                           dp("summary", self.summary_t), dev._stream())
        torch.cuda.synchronize()
        self.summary = self.summary_t.cpu().numpy()[: abi.compare_summary_dtype.itemsize].view(abi.compare_summary_dtype)[0]

    def records(self):
        return self.records_t.cpu().numpy()[: self.na * 16].view(abi.compare_record_dtype)

    def colors(self):
        return self.colors_t.cpu().numpy()[: self.na * 4].view(np.uint32)

    def slack_intact(self):
        """Nothing behind the last record, the last colour or the summary was written."""
        return bool((self.records_t[self.na * 16:] == 0xA5).all()) and bool((self.colors_t[self.na * 4:] == 0xA5).all()) and \
            bool((self.summary_t[abi.compare_summary_dtype.itemsize:] == 0xA5).all())

    def results_untouched(self):
        return bool((self.records_t == 0xA5).all()) and bool((self.colors_t == 0xA5).all())

    def untouched(self):
        return self.results_untouched() and bool((self.summary_t == 0xA5).all()) and bool((self.scratch == 0xA5).all())


def _check(raw, want, what):
    """A call with results against the mirror's (records, colours, summary)."""
    assert raw.rc == 0, what
    assert raw.summary.tobytes() == want[2].tobytes(), (what, [(f, raw.summary[f], want[2][f]) for f in GRID_FIELDS + ("numMatched", "numWithin", "maxD2")])
    got = raw.records()
    if got.tobytes() != want[0].tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 16) != want[0].view(np.uint8).reshape(-1, 16)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} records differ, first {[(int(i), got[i], want[0][i]) for i in bad[:5]]}")
    assert raw.colors().tobytes() == want[1].tobytes(), what
    assert raw.slack_intact(), what


@pytest.mark.parametrize("name", cr.CASES)
def test_bare_call_equals_the_mirror(dev, name):
    a, b, mn, mx, radius = cr.case(name)
    u, box = _uniforms(dev, mn, mx)
    cmp = _compare(radius)
    want = compare_samples(a, b, box, cmp)
    _check(Raw(dev, u, a, b, cmp), want, name)
    # without colours: the same records and summary, no colour written
    r = Raw(dev, u, a, b, cmp, colors=False)
    assert r.rc == 0 and r.records().tobytes() == want[0].tobytes() and r.summary.tobytes() == want[2].tobytes() and bool((r.colors_t == 0xA5).all())
    # count only: the grid's fields as the call with results has them, the rest zero (the mirror's record), nothing else written
    c = Raw(dev, u, a, b, cmp, results=False)
    assert c.rc == 0 and c.results_untouched() and c.slack_intact()
    assert c.summary.tobytes() == compare_samples(a, b, box, cmp, count_only=True)[2].tobytes()
    assert all(int(c.summary[f]) == int(want[2][f]) for f in GRID_FIELDS)
    # b == a's array itself
    if name == "lattice":
        s = Raw(dev, u, a, a, cmp)
        _check(s, compare_samples(a, a, box, cmp), name + " on itself")
        assert (s.records()["nearest"] == np.arange(len(a))).all() and int(s.summary["hist"][0]) == len(a)


def _colliding(radius, size, num_b, rs):
    """b: num_b samples of which at least 64 lie in distinct cells whose keys share ONE home slot eight slots before the table's end, so that
    their probe run wraps round it; the rest random.  -> (b, the number of such cells, slots)"""
    slots = int(cr.table_slots(num_b))
    h = float(compare_h(radius, size))
    g = np.arange(64, dtype=np.uint64)
    cx, cy, cz = (v.reshape(-1) for v in np.meshgrid(g, g, g, indexing="ij"))
    keys = cx | cy << np.uint64(20) | cz << np.uint64(40)
    pick = np.flatnonzero(compare_home(keys, slots) == np.uint64(slots - 8))[:80]
    assert len(pick) >= 64
    hot = (np.stack([cx[pick], cy[pick], cz[pick]], -1).astype(np.float64) + 0.5) * h
    return cr.points(np.concatenate([hot, rs.rand(num_b - len(pick), 3) * 64 * h])), len(pick), slots


def test_hash_collisions_made_on_purpose(dev):
    rs = np.random.RandomState(23)
    radius, (mn, mx) = 0.02, ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    u, box = _uniforms(dev, mn, mx)
    b, n_hot, slots = _colliding(radius, 4.0, 700, rs)
    assert slots == int(dev.L.simlod_compare_table_slots(len(b))) == 2048
    valid, keys = compare_cells(b, np.zeros(3), np.float64(1.0) / compare_h(radius, 4.0))
    homes = compare_home(keys[:n_hot], slots)
    assert valid.all() and len(set(keys[:n_hot].tolist())) == n_hot >= 64 and (homes == slots - 8).all()    # 64+ cells, one home, a run past the end
    a = cr.points(np.concatenate([np.stack([b["x"], b["y"], b["z"]], -1)[:400].astype(np.float64) + (rs.rand(400, 3) - 0.5) * 0.02, rs.rand(200, 3) * 1.3]))
    cmp = _compare(radius)
    want = compare_samples(a, b, box, cmp)
    assert int(want[2]["numMatched"]) >= 300
    _check(Raw(dev, u, a, b, cmp), want, "collisions")


def test_budget(dev):
    a, b, mn, mx, radius = cr.case("hot_cell")
    u, box = _uniforms(dev, mn, mx)
    n = int(Raw(dev, u, a, b, _compare(radius), results=False).summary["numCandidates"])
    assert n > 1
    for budget, runs in ((n + 1, True), (n, True), (n - 1, False)):
        cmp = _compare(radius, max_candidates=budget)
        r = Raw(dev, u, a, b, cmp)
        want = compare_samples(a, b, box, cmp)
        assert r.rc == 0 and r.summary.tobytes() == want[2].tobytes() and int(r.summary["error"]) == (0 if runs else abi.COMPARE_ERR_BUDGET), budget
        if runs:
            _check(r, want, f"budget {budget}")
        else:
            assert want[0] is None and r.results_untouched() and int(r.summary["numCandidates"]) == n and int(r.summary["numCells"]) == 1
        # the count-only call reports the same bit and the same grid
        c = Raw(dev, u, a, b, cmp, results=False)
        assert c.rc == 0 and c.summary.tobytes() == compare_samples(a, b, box, cmp, count_only=True)[2].tobytes() and c.results_untouched() and c.slack_intact()


def test_refused_arguments(dev):
    a, b, mn, mx, radius = cr.case("lattice")
    u, box = _uniforms(dev, mn, mx)
    cmp = _compare(radius)
    refused = lambda **kw: (lambda r: r.rc == INVALID_VALUE and r.untouched())(Raw(dev, u, a, b, cmp, **kw))
    for name in ("uniforms", "a", "b", "params", "scratch", "summary"):
        assert refused(null=(name,)), name
    assert refused(null=("records",)), "colours without records"
    for n in (0, (1 << 32) - 1, 1 << 32, 1 << 40):
        assert refused(na=n) and refused(nb=n), n

    def rec(**kw):
        r = cmp.record()
        for k, v in kw.items():
            if k == "t":
                r["thresholds2"][0][v[0]] = v[1]
            else:
                with np.errstate(over="ignore"):
                    r[k] = v
        return r
    for what, r in (("radius < 0", rec(radius=-1.0)), ("radius NaN", rec(radius=np.nan)), ("radius inf", rec(radius=np.inf)), ("reserved", rec(reserved=1)),
                    ("threshold NaN", rec(t=(5, np.nan))), ("threshold inf", rec(t=(254, np.inf))), ("descending", rec(t=(100, 0.0)))):
        assert refused(record=r), what
    for what, change in (("no extent", dict(boxMax=(0.0, 0.0, 0.0))), ("NaN corner", dict(boxMin=(np.nan, 0.0, 0.0))), ("infinite extent", dict(boxMax=(np.inf, 4.0, 4.0))),
                         ("negative extent", dict(boxMin=(5.0, 5.0, 5.0)))):
        uu = np.array(u, copy=True).reshape(1)
        for k, v in change.items():
            uu[k][0] = v
        assert refused(uniforms_record=uu), what
    # alignment: a, b, scratch and records at 16 bytes, colours at 4, the summary at 8 (the buffers are torch allocations, aligned far beyond that)
    for name, by in (("a", 8), ("a", 4), ("b", 8), ("b", 1), ("scratch", 8), ("records", 8), ("colors", 2), ("colors", 1), ("summary", 4)):
        assert refused(offset={name: by}), (name, by)
    ok = Raw(dev, u, a, b, cmp, offset={"a": 16, "b": 16, "colors": 4, "summary": 8, "records": 16})     # aligned offsets are taken
    assert ok.rc == 0 and int(ok.summary_t.cpu().numpy()[8:8 + abi.compare_summary_dtype.itemsize].view(abi.compare_summary_dtype)[0]["numCells"]) > 0
    # the scratch bound: one byte less is refused, the exact size is accepted — and suffices
    need = int(dev.L.simlod_compare_buffer_min_bytes(len(a), len(b)))
    assert need > 0 and int(dev.L.simlod_compare_buffer_min_bytes(0, 5)) == 0 and int(dev.L.simlod_compare_buffer_min_bytes(5, (1 << 32) - 1)) == 0
    assert need == int(dev.L.simlod_compare_buffer_min_bytes(1, len(b))), "the size depends on numB only"
    assert refused(scratch_bytes=need - 1)
    _check(Raw(dev, u, a, b, cmp, scratch_bytes=need), compare_samples(a, b, box, cmp), "exact scratch")
    assert [int(dev.L.simlod_compare_table_slots(n)) for n in (0, 1, 2, 3, 700, (1 << 32) - 2, (1 << 32) - 1)] == [0, 2, 4, 8, 2048, 1 << 33, 0]


@pytest.mark.parametrize("name", ["hot_cell", "distinct_cells", "invalid"])
def test_grid_independence_and_determinism(dev, name):
    a, b, mn, mx, radius = cr.case(name)
    u, box = _uniforms(dev, mn, mx)
    first = None
    for wg in (0, 1, 2, 0):
        cmp = _compare(radius, max_workgroups=wg)
        r = Raw(dev, u, a, b, cmp)
        got = (r.records().tobytes(), r.colors().tobytes(), r.summary.tobytes())
        assert r.rc == 0
        first = got if first is None else first
        assert got == first, f"maxWorkgroups {wg}"


def test_the_python_call_always_carries_a_budget(dev):
    """Rule C6 through DeviceOctree.compare_samples: a Compare without a budget gets 64 candidates per sample of a, so the hot cell — thousands
    per sample — comes back with the error bit and no result; an explicit 0 is the opt-out, an explicit budget is taken as given."""
    a, b, mn, mx, radius = cr.case("hot_cell")
    u, box = _uniforms(dev, mn, mx)
    cmp = _compare(radius)
    assert cmp.max_candidates is None
    n = int(compare_samples(a, b, box, cmp, count_only=True)[2]["numCandidates"])
    assert n > dev.COMPARE_BUDGET_PER_SAMPLE * len(a)
    rec, col, s = dev.compare_samples(u, a, b, cmp)
    assert rec is None and col is None and int(s["error"]) == abi.COMPARE_ERR_BUDGET and int(s["numCandidates"]) == n and int(s["numMatched"]) == 0
    assert s.tobytes() == compare_samples(a, b, box, _compare(radius, max_candidates=dev.COMPARE_BUDGET_PER_SAMPLE * len(a)))[2].tobytes()
    want = compare_samples(a, b, box, cmp)
    for got in (dev.compare_samples(u, a, b, cmp, max_candidates=0), dev.compare_samples(u, a, b, _compare(radius, max_candidates=0)),
                dev.compare_samples(u, a, b, cmp, max_candidates=n)):
        assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[1].cpu().numpy().view(np.uint32).tobytes() == want[1].tobytes()
        assert int(got[2]["error"]) == 0 and got[2]["hist"].tobytes() == want[2]["hist"].tobytes()
    assert dev.compare_samples(u, a, b, cmp, max_candidates=n - 1)[0] is None
    # a cloud the default budget takes runs without a word
    a, b, mn, mx, radius = cr.case("lattice")
    u, box = _uniforms(dev, mn, mx)
    got, want = dev.compare_samples(u, a, b, _compare(radius)), compare_samples(a, b, box, _compare(radius))
    assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and int(got[2]["error"]) == 0


# ---- through octrees -------------------------------------------------------------------------------------------------------------------------
def _octree(kind):
    """-> (dev, u, box, box_min) of ragged_tiny: as built, imported into a fresh device from its export, or built in a box off the origin."""
    name = "ragged_tiny"
    if kind == "shifted":
        dev, u, pts, box = _build(name, cases.offset_of("dyadic", cases.case(name)[1]))
    else:
        dev, u, pts, box = _build(name)
    if kind == "imported":
        ex = dev.export_octree(u)
        dev = _device()
        dev.nodes.fill_(0xA5)
        dev.import_octree(ex)
        assert int(dev.read_stats()["dbg"]) == 0
    return dev, u, box, dev.export_octree(u).box_min


def _lowest_coincident(b):
    """Per sample of b the lowest index of a sample at the same position."""
    xyz = np.stack([b["x"], b["y"], b["z"]], -1).view(np.uint32)
    xyz = np.where(xyz == 0x80000000, 0, xyz)                               # (-0 == +0)
    _, first, inverse = np.unique(xyz, axis=0, return_index=True, return_inverse=True)
    return first[inverse.reshape(-1)]


@pytest.mark.parametrize("kind", ["built", "imported", "shifted"])
def test_compare_through_octrees(built_libs, kind):
    dev, u, box, box_min = _octree(kind)
    size = float(max(box))
    cmp = _compare(0.01 * size)
    full = dev.export_octree(u)
    # 1. the octree against itself: every sample finds itself, or a coincident one with a lower index
    res = dev.compare_region(u, dev, None, cmp, max_level=20, select="all", other_select="all")
    rec, smp = res.records_host(), full.samples
    assert res.a.samples.tobytes() == smp.tobytes() == res.b.samples.tobytes() and len(rec) == len(smp) > 50_000
    assert (rec["d2"] == 0.0).all() and (rec["nearest"] == _lowest_coincident(smp)).all() and (rec["within"] >= 1).all()
    assert int(res.summary["hist"][0]) == len(smp) == int(res.summary["numMatched"]) and float(res.summary["maxD2"]) == 0.0
    want = full.compare(full, cmp)
    assert rec.tobytes() == want[0].tobytes() and res.summary.tobytes() == want[2].tobytes()
    assert res.colors.cpu().numpy().view(np.uint32).tobytes() == want[1].tobytes()
    nodes = res.nearest_nodes()
    t = full.nodes
    assert ((t["firstSample"][nodes] <= rec["nearest"]) & (rec["nearest"] < t["firstSample"][nodes].astype(np.int64) + t["numSamples"][nodes])).all()
    c = dev.count_compare(u, dev, None, cmp, max_level=20, select="all", other_select="all")
    assert all(int(c[f]) == int(res.summary[f]) for f in GRID_FIELDS) and int(c["numMatched"]) == 0
    # the default budget is 64 candidates per sample of A: a radius that puts the whole cloud into a few cells is refused by name
    from simlod_amd.runtime import SimlodError
    with pytest.raises(SimlodError, match="numCandidates.*maxCellPopulation"):
        dev.compare_region(u, dev, None, _compare(0.5 * size), max_level=20, select="all", other_select="all")
    # 2. against the same octree with a slab erased: the unmatched samples are the brute force's, and lie in the slab
    slab = rr.region("slab", box, box_min)
    other = _device()
    other.nodes.fill_(0xA5)
    other.import_octree(full)
    other.erase_region(u, slab)
    res = dev.compare_region(u, other, None, cmp, max_level=20, select="all", other_select="all")
    rec, erased = res.records_host(), other.export_octree(u)
    assert 0 < erased.num_samples < full.num_samples
    want = full.compare(erased, cmp)
    assert rec.tobytes() == want[0].tobytes() and res.summary.tobytes() == want[2].tobytes()
    unmatched = rec["within"] == 0
    in_slab = rr.brute_mask(slab, smp)
    assert 0 < unmatched.sum() < in_slab.sum() and (in_slab[unmatched]).all()
    rs = np.random.RandomState(2)
    some = np.concatenate([rs.choice(np.flatnonzero(unmatched), 8), rs.choice(np.flatnonzero(in_slab & ~unmatched), 8), rs.choice(np.flatnonzero(~in_slab), 8)])
    mn32, mx32 = np.asarray(full.box_min, np.float32), np.asarray(full.box_max, np.float32)
    exact = cr.compare_exact(smp[some], erased.samples, full.box_min, float((mx32 - mn32).max()), float(cmp.radius), cmp.thresholds2, cmp.table, MISS)
    assert rec[some].tobytes() == exact[0].tobytes()
    # 3. the colours painted into the octree, and undone
    res = dev.compare_region(u, other, slab, cmp, max_level=20, select="all", other_select="all")
    index = full.crop(slab, 20, "all", return_index=True)[1]
    colors = res.colors.cpu().numpy().view(np.uint32)
    assert len(colors) == len(index) > 0 and set(colors.tolist()) <= set(cmp.table.tolist()) | {MISS} and (colors == MISS).any() and (colors != MISS).any()
    counts, previous = res.paint(dev, u, return_previous=True)
    assert int(counts["numSamples"]) == len(index)
    painted = dev.export_octree(u)
    expect = smp.copy()
    expect["color"][index] = colors
    assert painted.samples.tobytes() == expect.tobytes() and painted.nodes.tobytes() == full.nodes.tobytes()
    dev.paint_region(u, slab, Paint.array(), colors=previous)
    assert dev.export_octree(u).samples.tobytes() == smp.tobytes()
    with pytest.raises(ValueError):
        dev.compare_region(u, other, slab, cmp, max_level=2, select="cut").paint(dev, u)
