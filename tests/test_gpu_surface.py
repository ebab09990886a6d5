"""GPU tier: simlod_surface_samples (include/simlod_hip.h, "surface queries") through the C ABI against the host mirror
octree_io.surface_samples, byte for byte — records, colours and the summary record — with every buffer poisoned first: every case of
tests/surface_ref.py under both colourBy values and each of its orientations and lights, with and without colours and count-only; the
records' independence of maxWorkgroups and of the order of b; hash collisions made on purpose; the budget; every refused argument; and
through octrees (DeviceOctree.surface_region, count_surface, SurfaceResult.paint) on a built, an imported and a shifted octree."""
import ctypes

import numpy as np
import pytest
import torch

import compare_ref as cr
import surface_ref as sf
from simlod_amd import abi
from simlod_amd.octree_io import Paint, Surface, surface_samples
from test_gpu_compare import _colliding, _octree, _uniforms
from util import _device

pytestmark = pytest.mark.gpu
SLACK = 64                                    # records and colour words behind numA
INVALID_VALUE = 1                             # hipErrorInvalidValue
GRID_FIELDS = ("error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numCandidates")
RECORD = abi.surface_record_dtype.itemsize
PALETTE = [0xFF202020, 0xFF808080, 0xFFFFFFFF]


@pytest.fixture(scope="module")
def dev(built_libs):
    return _device(persistent_bytes=1 << 28)


class Raw:
    """One simlod_surface_samples call with every buffer poisoned: rc, the summary record and the buffers as the call left them.
    results=False: records and colours are null pointers (count only); colors=False: colours alone; scratch_bytes: what the call is told;
    offset: {name: bytes} — that pointer is passed so many bytes into its buffer (every buffer has 16 bytes to spare behind its content)."""

    def __init__(self, dev, u, a, b, record, *, results=True, colors=True, scratch_bytes=None, null=(), na=None, nb=None, uniforms_record=None, offset=None):
        L = dev.L
        self.na, self.nb = len(a), len(b)
        need = int(L.simlod_surface_buffer_min_bytes(self.na, self.nb))
        told = need if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        self.scratch, self.summary_t = mk(max(need, told) + 16), mk(abi.surface_summary_dtype.itemsize + SLACK)
        self.records_t, self.colors_t = mk((self.na + SLACK) * RECORD), mk((self.na + SLACK) * 4)
        up16 = lambda v: torch.from_numpy(np.concatenate([np.ascontiguousarray(v).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to(dev.device)
        self.a_t, self.b_t = up16(a), up16(b)
        uu, up = dev._u(u if uniforms_record is None else uniforms_record)
        p = np.ascontiguousarray(record)
        off = offset or {}
        dp = lambda name, t, on=True: None if name in null or not on else ctypes.c_void_p(t.data_ptr() + off.get(name, 0))
        self.rc = L.simlod_surface_samples(None if "uniforms" in null else up, dp("a", self.a_t), ctypes.c_uint64(self.na if na is None else na),
                                           dp("b", self.b_t), ctypes.c_uint64(self.nb if nb is None else nb),
                                           None if "params" in null else ctypes.c_void_p(p.ctypes.data), dp("scratch", self.scratch), ctypes.c_uint64(told),
                                           dp("records", self.records_t, results), dp("colors", self.colors_t, results and colors),
                                           dp("summary", self.summary_t), dev._stream())
        torch.cuda.synchronize()
        self.summary = self.summary_t.cpu().numpy()[: abi.surface_summary_dtype.itemsize].view(abi.surface_summary_dtype)[0]

    def records(self):
        return self.records_t.cpu().numpy()[: self.na * RECORD].view(abi.surface_record_dtype)

    def colors(self):
        return self.colors_t.cpu().numpy()[: self.na * 4].view(np.uint32)

    def slack_intact(self):
        """Nothing behind the last record, the last colour or the summary was written."""
        return bool((self.records_t[self.na * RECORD:] == 0xA5).all()) and bool((self.colors_t[self.na * 4:] == 0xA5).all()) and \
            bool((self.summary_t[abi.surface_summary_dtype.itemsize:] == 0xA5).all())

    def results_untouched(self):
        return bool((self.records_t == 0xA5).all()) and bool((self.colors_t == 0xA5).all())

    def untouched(self):
        return self.results_untouched() and bool((self.summary_t == 0xA5).all()) and bool((self.scratch == 0xA5).all())


def _check(raw, want, what):
    """A call with results against the mirror's (records, colours, summary)."""
    assert raw.rc == 0, what
    assert raw.summary.tobytes() == want[2].tobytes(), (what, [(f, raw.summary[f], want[2][f]) for f in GRID_FIELDS + ("numEstimated", "numWithin", "numDegenerate")])
    got = raw.records()
    if got.tobytes() != want[0].tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, RECORD) != want[0].view(np.uint8).reshape(-1, RECORD)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} records differ, first {[(int(i), got[i], want[0][i]) for i in bad[:5]]}")
    assert raw.colors().tobytes() == want[1].tobytes(), what
    assert raw.slack_intact(), what


@pytest.mark.parametrize("colour_by", [sf.SHADE, sf.VARIATION])
@pytest.mark.parametrize("name", sf.CASES)
def test_bare_call_equals_the_mirror(dev, name, colour_by):
    a, b, mn, mx, radius, _ = sf.case(name)
    u, box = _uniforms(dev, mn, mx)
    for variant, rec in enumerate(sf.case_params(name, colour_by)):
        want = surface_samples(a, b, box, Surface.from_record(rec))
        _check(Raw(dev, u, a, b, rec), want, (name, variant))
    # without colours: the same records and summary, no colour written
    r = Raw(dev, u, a, b, rec, colors=False)
    assert r.rc == 0 and r.records().tobytes() == want[0].tobytes() and r.summary.tobytes() == want[2].tobytes() and bool((r.colors_t == 0xA5).all())
    # count only: the grid's fields as the call with results has them, the rest zero (the mirror's record), nothing else written
    c = Raw(dev, u, a, b, rec, results=False)
    assert c.rc == 0 and c.results_untouched() and c.slack_intact()
    assert c.summary.tobytes() == surface_samples(a, b, box, Surface.from_record(rec), count_only=True)[2].tobytes()
    assert all(int(c.summary[f]) == int(want[2][f]) for f in GRID_FIELDS)
    if name == "plane_grid":                                               # b is a's array itself
        same = Raw(dev, u, a, a, rec)
        _check(same, want, name + " on itself")


@pytest.mark.parametrize("name", ["hot_cell", "cell_faces", "wide_sums"])
def test_grid_and_order_independence(dev, name):
    """The same bytes with maxWorkgroups 1, 3 and 0, twice over, and — the records and the summary — with b permuted."""
    a, b, mn, mx, radius, _ = sf.case(name)
    u, box = _uniforms(dev, mn, mx)
    first = None
    for wg in (0, 1, 3, 0):
        r = Raw(dev, u, a, b, sf.case_params(name, sf.VARIATION, wg=wg)[0])
        got = (r.records().tobytes(), r.colors().tobytes(), r.summary.tobytes())
        assert r.rc == 0
        first = got if first is None else first
        assert got == first, f"maxWorkgroups {wg}"
    rs = np.random.RandomState(3)
    for wg in (0, 1):
        r = Raw(dev, u, a, b[rs.permutation(len(b))], sf.case_params(name, sf.VARIATION, wg=wg)[0])
        assert r.rc == 0 and (r.records().tobytes(), r.colors().tobytes(), r.summary.tobytes()) == first, "b permuted"


def test_hash_collisions_made_on_purpose(dev):
    rs = np.random.RandomState(23)
    radius, (mn, mx) = 0.02, ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    u, box = _uniforms(dev, mn, mx)
    b, n_hot, slots = _colliding(radius, 4.0, 700, rs)                      # 64+ cells with one home slot, their probe run wrapping the table's end
    assert slots == 2048 and n_hot >= 64
    xyz = np.stack([b["x"], b["y"], b["z"]], -1).astype(np.float64)
    b = cr.points(np.concatenate([xyz] + [xyz[:n_hot] + (rs.rand(n_hot, 3) - 0.5) * 0.02 for _ in range(4)]))   # neighbours for the colliding cells
    a = cr.points(np.concatenate([xyz[:400] + (rs.rand(400, 3) - 0.5) * 0.01, rs.rand(200, 3) * 1.3]))
    rec = sf.params(radius, sf.SHADE)
    want = surface_samples(a, b, box, Surface.from_record(rec))
    assert int(want[2]["numEstimated"]) >= 64
    _check(Raw(dev, u, a, b, rec), want, "collisions")


def test_budget(dev):
    a, b, mn, mx, radius, _ = sf.case("hot_cell")
    u, box = _uniforms(dev, mn, mx)
    n = int(Raw(dev, u, a, b, sf.params(radius, sf.SHADE), results=False).summary["numCandidates"])
    assert n > 1
    for budget, runs in ((n + 1, True), (n, True), (n - 1, False)):
        rec = sf.params(radius, sf.SHADE, budget=budget)
        r = Raw(dev, u, a, b, rec)
        want = surface_samples(a, b, box, Surface.from_record(rec))
        assert r.rc == 0 and r.summary.tobytes() == want[2].tobytes() and int(r.summary["error"]) == (0 if runs else abi.SURFACE_ERR_BUDGET), budget
        if runs:
            _check(r, want, f"budget {budget}")
        else:
            assert want[0] is None and r.results_untouched() and int(r.summary["numCandidates"]) == n and int(r.summary["numCells"]) == 1
        c = Raw(dev, u, a, b, rec, results=False)
        assert c.rc == 0 and c.summary.tobytes() == surface_samples(a, b, box, Surface.from_record(rec), count_only=True)[2].tobytes()
        assert c.results_untouched() and c.slack_intact()


def test_refused_arguments(dev):
    a, b, mn, mx, radius, _ = sf.case("plane_grid")
    u, box = _uniforms(dev, mn, mx)
    good = sf.params(radius, sf.SHADE)
    refused = lambda record=good, **kw: (lambda r: r.rc == INVALID_VALUE and r.untouched())(Raw(dev, u, a, b, record, **kw))
    for name in ("uniforms", "a", "b", "params", "scratch", "summary"):
        assert refused(null=(name,)), name
    assert refused(null=("records",)), "colours without records"
    for n in (0, (1 << 32) - 1, 1 << 32, 1 << 40):
        assert refused(na=n) and refused(nb=n), n
    t = np.array(sf.shade_thresholds())

    def with_t(i, v):
        w = t.copy()
        w[i] = v
        return w
    for what, rec in (("radius < 0", sf.params(-1.0, sf.SHADE)), ("radius NaN", sf.params(np.nan, sf.SHADE)), ("radius inf", sf.params(np.inf, sf.SHADE)),
                      ("reserved", sf.params(radius, sf.SHADE, reserved=1)), ("threshold NaN", sf.params(radius, sf.SHADE, thresholds=with_t(5, np.nan))),
                      ("threshold inf", sf.params(radius, sf.SHADE, thresholds=with_t(254, np.inf))), ("descending", sf.params(radius, sf.SHADE, thresholds=with_t(100, -2.0))),
                      ("colourBy 2", sf.params(radius, 2)), ("orientMode 2", sf.params(radius, sf.SHADE, orient_mode=2)),
                      ("light NaN", sf.params(radius, sf.SHADE, light=(0.0, np.nan, 1.0))), ("light inf, unused", sf.params(radius, sf.VARIATION, light=(np.inf, 0.0, 0.0))),
                      ("orient inf", sf.params(radius, sf.SHADE, orient=(0.0, 0.0, np.inf))), ("orient NaN", sf.params(radius, sf.VARIATION, orient=(np.nan, 0.0, 0.0))),
                      ("zero light", sf.params(radius, sf.SHADE, light=(0.0, -0.0, 0.0)))):
        assert not sf.params_acceptable(rec) and refused(rec), what
    for what, change in (("no extent", dict(boxMax=(0.0, 0.0, 0.0))), ("NaN corner", dict(boxMin=(np.nan, 0.0, 0.0))), ("infinite extent", dict(boxMax=(np.inf, 4.0, 4.0))),
                         ("negative extent", dict(boxMin=(5.0, 5.0, 5.0)))):
        uu = np.array(u, copy=True).reshape(1)
        for k, v in change.items():
            uu[k][0] = v
        assert refused(uniforms_record=uu), what
    # alignment: a, b, scratch and records at 16 bytes, colours at 4, the summary at 8
    for name, by in (("a", 8), ("a", 4), ("b", 8), ("b", 1), ("scratch", 8), ("records", 8), ("records", 4), ("colors", 2), ("colors", 1), ("summary", 4)):
        assert refused(offset={name: by}), (name, by)
    ok = Raw(dev, u, a, b, good, offset={"a": 16, "b": 16, "colors": 4, "summary": 8, "records": 16})     # aligned offsets are taken
    assert ok.rc == 0 and int(ok.summary_t.cpu().numpy()[8:8 + abi.surface_summary_dtype.itemsize].view(abi.surface_summary_dtype)[0]["numEstimated"]) > 0
    # a zero light is fine where it is not used
    assert Raw(dev, u, a, b, sf.params(radius, sf.VARIATION, light=(0.0, 0.0, 0.0))).rc == 0
    # the scratch bound is the compare call's: one byte less is refused, the exact size is accepted — and suffices
    need = int(dev.L.simlod_surface_buffer_min_bytes(len(a), len(b)))
    assert need == int(dev.L.simlod_compare_buffer_min_bytes(len(a), len(b))) > 0
    assert int(dev.L.simlod_surface_buffer_min_bytes(0, 5)) == 0 and int(dev.L.simlod_surface_buffer_min_bytes(5, (1 << 32) - 1)) == 0
    assert refused(scratch_bytes=need - 1)
    _check(Raw(dev, u, a, b, good, scratch_bytes=need), surface_samples(a, b, box, Surface.from_record(good)), "exact scratch")


def test_the_python_call_always_carries_a_budget(dev):
    """Rule C6 through DeviceOctree.surface_samples: a Surface without a budget gets 64 candidates per sample of a, so the hot cell comes
    back with the error bit and no result; an explicit 0 is the opt-out, an explicit budget is taken as given."""
    a, b, mn, mx, radius, _ = sf.case("hot_cell")
    u, box = _uniforms(dev, mn, mx)
    s = Surface.hillshade(radius, (1.0, 1.0, 2.0), PALETTE, miss_color=sf.MISS_COLOR)
    assert s.max_candidates is None
    n = int(surface_samples(a, b, box, s, count_only=True)[2]["numCandidates"])
    assert n > dev.COMPARE_BUDGET_PER_SAMPLE * len(a)
    rec, col, summary = dev.surface_samples(u, a, b, s)
    assert rec is None and col is None and int(summary["error"]) == abi.SURFACE_ERR_BUDGET and int(summary["numCandidates"]) == n and int(summary["numEstimated"]) == 0
    want = surface_samples(a, b, box, s)
    zero = Surface.hillshade(radius, (1.0, 1.0, 2.0), PALETTE, miss_color=sf.MISS_COLOR, max_candidates=0)
    for got in (dev.surface_samples(u, a, b, s, max_candidates=0), dev.surface_samples(u, a, b, zero), dev.surface_samples(u, a, b, s, max_candidates=n)):
        assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[1].cpu().numpy().view(np.uint32).tobytes() == want[1].tobytes()
        assert int(got[2]["error"]) == 0 and got[2]["hist"].tobytes() == want[2]["hist"].tobytes()
    assert dev.surface_samples(u, a, b, s, max_candidates=n - 1)[0] is None
    # a cloud the default budget takes runs without a word
    a, b, mn, mx, radius, _ = sf.case("plane_grid")
    u, box = _uniforms(dev, mn, mx)
    s = Surface.variation(radius, 1.0 / 3.0, PALETTE)
    got, want = dev.surface_samples(u, a, b, s), surface_samples(a, b, box, s)
    assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and int(got[2]["error"]) == 0


# ---- through octrees -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["built", "imported", "shifted"])
def test_surface_through_octrees(built_libs, kind):
    dev, u, box, box_min = _octree(kind)
    size = float(max(box))
    s = Surface.hillshade(0.01 * size, (1.0, 1.0, 2.0), PALETTE, orient=(0.0, 0.0, 1.0), miss_color=sf.MISS_COLOR)
    full = dev.export_octree(u)
    smp = full.samples
    # the whole octree against itself: the mirror's bytes
    res = dev.surface_region(u, None, s, max_level=20, select="all")
    rec = res.records_host()
    assert res.a.samples.tobytes() == smp.tobytes() and res.b is res.a and len(rec) == len(smp) > 50_000
    want = full.surface(s)
    assert rec.tobytes() == want[0].tobytes() and res.summary.tobytes() == want[2].tobytes()
    colors = res.colors.cpu().numpy().view(np.uint32)
    assert colors.tobytes() == want[1].tobytes()
    estimated = rec["lambdaDen"] != 0
    assert int(res.summary["numEstimated"]) == estimated.sum() > 0 and (rec["normal"][estimated][:, 2] >= 0).all()
    assert (res.unit_normals()[estimated][:, 2] >= 0).all() and (res.variation() <= 1.0).all() and (res.variation() >= -1e-12).all()
    c = dev.count_surface(u, None, s, max_level=20, select="all")
    assert all(int(c[f]) == int(res.summary[f]) for f in GRID_FIELDS) and int(c["numEstimated"]) == 0
    from simlod_amd.runtime import SimlodError
    with pytest.raises(SimlodError, match="numCandidates.*maxCellPopulation"):
        dev.surface_region(u, None, Surface.variation(0.5 * size, 1.0 / 3.0, PALETTE), max_level=20, select="all")
    # the colours painted into the octree, and undone
    counts, previous = res.paint(dev, u, return_previous=True)
    assert int(counts["numSamples"]) == len(smp)
    painted = dev.export_octree(u)
    expect = smp.copy()
    expect["color"] = colors
    assert painted.samples.tobytes() == expect.tobytes() and painted.nodes.tobytes() == full.nodes.tobytes()
    assert set(colors.tolist()) <= set(s.table.tolist()) | {sf.MISS_COLOR} and len(set(colors.tolist())) > 2
    dev.paint_region(u, res.selection["region"], Paint.array(), colors=previous)
    assert dev.export_octree(u).samples.tobytes() == smp.tobytes()
    with pytest.raises(ValueError):
        dev.surface_region(u, None, s, max_level=2, select="cut").paint(dev, u)
