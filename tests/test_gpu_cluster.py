"""GPU tier: simlod_cluster_samples (include/simlod_hip.h, "cluster queries") through the C ABI against the host mirror
octree_io.cluster_samples, byte for byte — records, colours and the summary record, whose internal error bit must be zero — with every
buffer poisoned first: every case of tests/cluster_ref.py, with and without colours and count-only; the same bytes under maxWorkgroups 1, 2
and the default and twice in a row; hash collisions made on purpose; the budget; every refused argument; the exact scratch size; and through
octrees (DeviceOctree.cluster_region, count_cluster, ClusterResult.paint) on a built, an imported and a shifted octree."""
import ctypes

import numpy as np
import pytest
import torch

import cluster_ref as kr
import compare_ref as cr
from simlod_amd import abi
from simlod_amd.octree_io import Cluster, Paint, cluster_samples
from test_gpu_compare import _colliding, _octree, _uniforms
from util import _device

pytestmark = pytest.mark.gpu
SLACK = 64                                    # records and colour words behind numA
INVALID_VALUE = 1                             # hipErrorInvalidValue
GRID_FIELDS = ("error", "numCells", "maxCellPopulation", "numInvalidA", "numInvalidB", "numCandidates")
RECORD = abi.cluster_record_dtype.itemsize
SUMMARY = abi.cluster_summary_dtype.itemsize


@pytest.fixture(scope="module")
def dev(built_libs):
    return _device(persistent_bytes=1 << 28)


_MIRROR = {}


def _mirror(name, box):
    """The mirror's (records, colours, summary) of a case in the uniforms' box, computed once and not changed."""
    if name not in _MIRROR:
        _MIRROR[name] = (box, cluster_samples(kr.case(name)[0], box, Cluster.from_record(kr.case_record(name))))
    assert _MIRROR[name][0] == box
    return _MIRROR[name][1]


class Raw:
    """One simlod_cluster_samples call with every buffer poisoned: rc, the summary record and the buffers as the call left them.
    results=False: records and colours are null pointers (count only); colors=False: colours alone; scratch_bytes: what the call is told;
    offset: {name: bytes} — that pointer is passed so many bytes into its buffer (every buffer has 16 bytes to spare behind its content)."""

    def __init__(self, dev, u, a, record, *, results=True, colors=True, scratch_bytes=None, null=(), na=None, uniforms_record=None, offset=None):
        L = dev.L
        self.na = len(a)
        need = int(L.simlod_cluster_buffer_min_bytes(self.na))
        told = need if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        self.scratch, self.summary_t = mk(max(need, told) + 16), mk(SUMMARY + SLACK)
        self.records_t, self.colors_t = mk((self.na + SLACK) * RECORD), mk((self.na + SLACK) * 4)
        self.a_t = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to(dev.device)
        uu, up = dev._u(u if uniforms_record is None else uniforms_record)
        p = np.ascontiguousarray(record)
        off = offset or {}
        dp = lambda name, t, on=True: None if name in null or not on else ctypes.c_void_p(t.data_ptr() + off.get(name, 0))
        self.rc = L.simlod_cluster_samples(None if "uniforms" in null else up, dp("a", self.a_t), ctypes.c_uint64(self.na if na is None else na),
                                           None if "params" in null else ctypes.c_void_p(p.ctypes.data), dp("scratch", self.scratch), ctypes.c_uint64(told),
                                           dp("records", self.records_t, results), dp("colors", self.colors_t, results and colors),
                                           dp("summary", self.summary_t), dev._stream())
        torch.cuda.synchronize()
        self.summary = self.summary_t.cpu().numpy()[:SUMMARY].view(abi.cluster_summary_dtype)[0]

    def records(self):
        return self.records_t.cpu().numpy()[: self.na * RECORD].view(abi.cluster_record_dtype)

    def colors(self):
        return self.colors_t.cpu().numpy()[: self.na * 4].view(np.uint32)

    def slack_intact(self):
        """Nothing behind the last record, the last colour or the summary was written."""
        return bool((self.records_t[self.na * RECORD:] == 0xA5).all()) and bool((self.colors_t[self.na * 4:] == 0xA5).all()) and \
            bool((self.summary_t[SUMMARY:] == 0xA5).all())

    def results_untouched(self):
        return bool((self.records_t == 0xA5).all()) and bool((self.colors_t == 0xA5).all())

    def untouched(self):
        return self.results_untouched() and bool((self.summary_t == 0xA5).all()) and bool((self.scratch == 0xA5).all())


def _check(raw, want, what):
    """A call with results against the mirror's (records, colours, summary)."""
    assert raw.rc == 0, what
    assert int(raw.summary["error"]) & abi.CLUSTER_ERR_INTERNAL == 0, what
    assert raw.summary.tobytes() == want[2].tobytes(), (what, [(f, raw.summary[f], want[2][f]) for f in want[2].dtype.names if raw.summary[f].tobytes() != want[2][f].tobytes()])
    got = raw.records()
    if got.tobytes() != want[0].tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, RECORD) != want[0].view(np.uint8).reshape(-1, RECORD)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} records differ, first {[(int(i), got[i], want[0][i]) for i in bad[:5]]}")
    assert raw.colors().tobytes() == want[1].tobytes(), what
    assert raw.slack_intact(), what


@pytest.mark.parametrize("name", kr.CASES)
def test_bare_call_equals_the_mirror(dev, name):
    a, mn, mx = kr.case(name)[:3]
    u, box = _uniforms(dev, mn, mx)
    rec = kr.case_record(name)
    want = _mirror(name, box)
    _check(Raw(dev, u, a, rec), want, name)
    # without colours: the same records and summary, no colour written
    r = Raw(dev, u, a, rec, colors=False)
    assert r.rc == 0 and r.records().tobytes() == want[0].tobytes() and r.summary.tobytes() == want[2].tobytes() and bool((r.colors_t == 0xA5).all())
    # count only (rule C7): the grid's fields as the call with results has them, the rest zero (the mirror's record), nothing else written
    c = Raw(dev, u, a, rec, results=False)
    assert c.rc == 0 and c.results_untouched() and c.slack_intact()
    assert c.summary.tobytes() == cluster_samples(a, box, Cluster.from_record(rec), count_only=True)[2].tobytes()
    assert all(int(c.summary[f]) == int(want[2][f]) for f in GRID_FIELDS) and int(c.summary["numClusters"]) == 0


@pytest.mark.parametrize("name", ["chain", "hot_cell", "singletons", "blobs"])
def test_grid_independence_and_determinism(dev, name):
    """The same bytes — the mirror's — with maxWorkgroups 1, 2 and the default, each twice in a row."""
    a, mn, mx = kr.case(name)[:3]
    u, box = _uniforms(dev, mn, mx)
    want = _mirror(name, box)
    for wg in (1, 1, 2, 2, 0, 0):
        r = Raw(dev, u, a, kr.case_record(name, wg=wg))
        assert r.rc == 0 and int(r.summary["error"]) == 0, wg
        assert (r.records().tobytes(), r.colors().tobytes(), r.summary.tobytes()) == (want[0].tobytes(), want[1].tobytes(), want[2].tobytes()), f"maxWorkgroups {wg}"


def test_hash_collisions_made_on_purpose(dev):
    rs = np.random.RandomState(23)
    radius, (mn, mx) = 0.02, ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
    u, box = _uniforms(dev, mn, mx)
    b, n_hot, slots = _colliding(radius, 4.0, 700, rs)                      # 64+ cells with one home slot, their probe run wrapping the table's end
    xyz = np.stack([b["x"], b["y"], b["z"]], -1).astype(np.float64)
    # neighbours for the colliding cells, so that clusters form in them and across them; 1 024 samples: the same 2 048 slots
    a = cr.points(np.concatenate([xyz] + [xyz[:n_hot] + (rs.rand(n_hot, 3) - 0.5) * 0.02 for _ in range(4)])[:1024])
    assert n_hot >= 64 and slots == 2048 == int(dev.L.simlod_compare_table_slots(len(a)))
    rec = kr.params(radius, 3, 2)
    want = cluster_samples(a, box, Cluster.from_record(rec))
    assert int(want[2]["numClusters"]) >= 32 and int(want[2]["numBorder"]) > 0 and int(want[2]["numNoise"]) > 0
    _check(Raw(dev, u, a, rec), want, "collisions")


def test_budget(dev):
    a, mn, mx = kr.case("hot_cell")[:3]
    u, box = _uniforms(dev, mn, mx)
    n = int(Raw(dev, u, a, kr.case_record("hot_cell"), results=False).summary["numCandidates"])
    assert n == 600 * 600
    for budget, runs in ((n + 1, True), (n, True), (n - 1, False)):
        rec = kr.case_record("hot_cell", budget=budget)
        r = Raw(dev, u, a, rec)
        want = cluster_samples(a, box, Cluster.from_record(rec))
        assert r.rc == 0 and r.summary.tobytes() == want[2].tobytes() and int(r.summary["error"]) == (0 if runs else abi.CLUSTER_ERR_BUDGET), budget
        if runs:
            _check(r, want, f"budget {budget}")
        else:                                                               # rule C6: nothing is written
            assert want[0] is None and r.results_untouched() and r.slack_intact() and int(r.summary["numCandidates"]) == n and int(r.summary["numCells"]) == 1
        c = Raw(dev, u, a, rec, results=False)
        assert c.rc == 0 and c.summary.tobytes() == cluster_samples(a, box, Cluster.from_record(rec), count_only=True)[2].tobytes()
        assert c.results_untouched() and c.slack_intact()


def test_refused_arguments(dev):
    a, mn, mx, radius, min_neighbours, min_cluster_size = kr.case("invalid")
    u, box = _uniforms(dev, mn, mx)
    good = kr.case_record("invalid")
    refused = lambda record=good, **kw: (lambda r: r.rc == INVALID_VALUE and r.untouched())(Raw(dev, u, a, record, **kw))
    for name in ("uniforms", "a", "params", "scratch", "summary"):
        assert refused(null=(name,)), name
    assert refused(null=("records",)), "colours without records"
    for n in (0, (1 << 32) - 1, 1 << 32, 1 << 40):
        assert refused(na=n), n
    for what, rec in (("radius < 0", kr.params(-1.0)), ("radius NaN", kr.params(np.nan)), ("radius inf", kr.params(np.inf)), ("reserved", kr.params(radius, reserved=1)),
                      ("minNeighbours 0", kr.params(radius, 0, 1)), ("minClusterSize 0", kr.params(radius, 1, 0))):
        assert not kr.record_acceptable(rec) and refused(rec), what
    for what, change in (("no extent", dict(boxMax=tuple(mn))), ("NaN corner", dict(boxMin=(np.nan, 0.0, 0.0))), ("infinite extent", dict(boxMax=(np.inf, 4.0, 11.0))),
                         ("negative extent", dict(boxMin=(205.0, 5.0, 15.0)))):
        uu = np.array(u, copy=True).reshape(1)
        for k, v in change.items():
            uu[k][0] = v
        assert refused(uniforms_record=uu), what
    # alignment: a, scratch and records at 16 bytes, colours at 4, the summary at 8
    for name, by in (("a", 8), ("a", 4), ("a", 1), ("scratch", 8), ("records", 8), ("records", 4), ("colors", 2), ("colors", 1), ("summary", 4)):
        assert refused(offset={name: by}), (name, by)
    want = _mirror("invalid", box)
    ok = Raw(dev, u, a, good, offset={"a": 16, "colors": 4, "summary": 8, "records": 16})                 # aligned offsets are taken
    moved = np.concatenate([a[1:], np.zeros(1, a.dtype)])                                                # (a from its second sample on, and the spare zeros)
    assert ok.rc == 0 and ok.summary_t.cpu().numpy()[8:8 + SUMMARY].tobytes() == cluster_samples(moved, box, Cluster.from_record(good))[2].tobytes()
    # the scratch size is exact and a pure function of numA: one byte less is refused, the exact size is accepted — and suffices
    need = int(dev.L.simlod_cluster_buffer_min_bytes(len(a)))
    words = (4 * len(a) + 15) // 16 * 16
    assert need == int(dev.L.simlod_compare_buffer_min_bytes(len(a), len(a))) + 5 * words + 1024 * 208
    assert int(dev.L.simlod_cluster_buffer_min_bytes(0)) == 0 and int(dev.L.simlod_cluster_buffer_min_bytes((1 << 32) - 1)) == 0
    assert refused(scratch_bytes=need - 1) and refused(scratch_bytes=int(dev.L.simlod_compare_buffer_min_bytes(len(a), len(a))))
    _check(Raw(dev, u, a, good, scratch_bytes=need), want, "exact scratch")


def test_the_python_call_always_carries_a_budget(dev):
    """Rule C6 through DeviceOctree.cluster_samples: a Cluster without a budget gets 64 candidates per sample, so the hot cell comes back
    with the error bit and no result; an explicit 0 is the opt-out, an explicit budget is taken as given."""
    a, mn, mx = kr.case("hot_cell")[:3]
    u, box = _uniforms(dev, mn, mx)
    c = Cluster(0.25, table=kr.TABLE, noise_color=kr.NOISE_COLOR)
    want = _mirror("hot_cell", box)
    n = int(want[2]["numCandidates"])
    assert c.max_candidates is None and n > dev.COMPARE_BUDGET_PER_SAMPLE * len(a)
    rec, col, summary = dev.cluster_samples(u, a, c)
    assert rec is None and col is None and int(summary["error"]) == abi.CLUSTER_ERR_BUDGET and int(summary["numCandidates"]) == n and int(summary["numClusters"]) == 0
    zero = Cluster(0.25, table=kr.TABLE, noise_color=kr.NOISE_COLOR, max_candidates=0)
    for got in (dev.cluster_samples(u, a, c, max_candidates=0), dev.cluster_samples(u, a, zero), dev.cluster_samples(u, a, c, max_candidates=n)):
        assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[1].cpu().numpy().view(np.uint32).tobytes() == want[1].tobytes()
        assert got[2].tobytes() == want[2].tobytes()
    assert dev.cluster_samples(u, a, c, max_candidates=n - 1)[0] is None
    # a cloud the default budget takes runs without a word
    a, mn, mx = kr.case("chain")[:3]
    u, box = _uniforms(dev, mn, mx)
    got = dev.cluster_samples(u, a, Cluster.from_record(kr.case_record("chain", budget=0)), max_candidates=None)
    assert got[0].cpu().numpy().tobytes() == _mirror("chain", box)[0].tobytes() and int(got[2]["error"]) == 0


# ---- through octrees -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["built", "imported", "shifted"])
def test_cluster_through_octrees(built_libs, kind):
    dev, u, box, box_min = _octree(kind)
    size = float(max(box))
    c = Cluster(0.01 * size, 4, 10, noise_color=kr.NOISE_COLOR)
    full = dev.export_octree(u)
    smp = full.samples
    # the whole octree: the mirror's bytes
    res = dev.cluster_region(u, None, c, max_level=20, select="all")
    rec = res.records_host()
    assert res.a.samples.tobytes() == smp.tobytes() and len(rec) == len(smp) > 50_000
    want = full.cluster(c)
    assert rec.tobytes() == want[0].tobytes() and res.summary.tobytes() == want[2].tobytes() and int(res.summary["error"]) == 0
    colors = res.colors.cpu().numpy().view(np.uint32)
    assert colors.tobytes() == want[1].tobytes()
    assert int(res.summary["numClusters"]) >= 1 and int(res.summary["numNoise"]) > 0 and int(res.summary["numCore"]) > 0
    sizes = res.sizes()
    assert len(sizes) == int(res.summary["numClusters"]) and sizes.max() == int(res.summary["largestSize"]) and (sizes >= 10).all()
    k = int(res.summary["largestCluster"])
    assert len(res.members(k)) == sizes[k] and (res.labels[res.members(k)] == k).all() and ((res.labels == -1) == (colors == kr.NOISE_COLOR)).all()
    cnt = dev.count_cluster(u, None, c, max_level=20, select="all")
    assert all(int(cnt[f]) == int(res.summary[f]) for f in GRID_FIELDS) and int(cnt["numClusters"]) == 0
    from simlod_amd.runtime import SimlodError
    with pytest.raises(SimlodError, match="numCandidates.*maxCellPopulation"):
        dev.cluster_region(u, None, Cluster(0.5 * size), max_level=20, select="all")
    # the colours painted into the octree, and undone
    counts, previous = res.paint(dev, u, return_previous=True)
    assert int(counts["numSamples"]) == len(smp)
    painted = dev.export_octree(u)
    expect = smp.copy()
    expect["color"] = colors
    assert painted.samples.tobytes() == expect.tobytes() and painted.nodes.tobytes() == full.nodes.tobytes()
    assert set(colors.tolist()) <= set(c.table.tolist()) | {kr.NOISE_COLOR} and len(set(colors.tolist())) >= 2
    dev.paint_region(u, res.selection["region"], Paint.array(), colors=previous)
    assert dev.export_octree(u).samples.tobytes() == smp.tobytes()
    with pytest.raises(ValueError):
        dev.cluster_region(u, None, c, max_level=2, select="cut").paint(dev, u)
