"""GPU tier: simlod_query_view (include/simlod_hip.h, "view queries") through the C ABI — against a real frame's SIMLOD_EXPORT_VISIBLE export
(rule V8) and against the host mirror OctreeExport.view, byte for byte; the frozen camera, rule V9, the budget rule, a level of more than
1 024 entries, count-only calls, capacities, refused arguments, maxLevel."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import deep_ref
import view_ref as vr
from simlod_amd import abi, camera
from simlod_amd.runtime import SimlodError
from util import _build, _device, _ingest

pytestmark = pytest.mark.gpu
W, H = vr.WIDTH, vr.HEIGHT
GPU_CAMERAS = ["bird", "closer", "inside", "grazing"]
GPU_BIASES = [0, 1, 2, 4]


class Raw:
    """One simlod_query_view call with every buffer poisoned: rc, the counts record, and the buffers as the call left them."""

    def __init__(self, dev, u, view=None, max_level=20, *, table_cap=None, sample_cap=None, count_only=False, scratch_bytes=None, null=None):
        st = dev.read_stats()
        nn, bound = int(st["numNodes"]), int(st["numPoints"]) + int(st["numVoxels"])
        self.table_cap = nn if table_cap is None else table_cap
        self.sample_cap = bound if sample_cap is None else sample_cap
        L = dev.L
        need = int(L.simlod_export_buffer_min_bytes(self.table_cap, bound)) if scratch_bytes is None else scratch_bytes
        mk = lambda n: torch.full((max(int(n), 16),), 0xA5, dtype=torch.uint8, device=dev.device)
        self.scratch, self.table, self.samples = mk(need), mk((self.table_cap + 4) * 40), mk((self.sample_cap + 1000) * 16)
        self.counts_t = mk(abi.view_counts_dtype.itemsize + 56)
        uu, up = dev._u(u)
        v = abi.view_record() if view is None else view
        ptr = {k: (None if k == null else dev._p(t)) for k, t in (("nodes", dev.nodes), ("stats", dev.stats), ("scratch", self.scratch), ("table", self.table),
                                                                  ("counts", self.counts_t))}
        self.rc = L.simlod_query_view(ptr["nodes"], ptr["stats"], None if null == "uniforms" else up, None if null == "view" else ctypes.c_void_p(v.ctypes.data),
                                      max_level, ptr["scratch"], ctypes.c_uint64(need), ptr["table"], self.table_cap,
                                      None if count_only else dev._p(self.samples), ctypes.c_uint64(self.sample_cap), ptr["counts"], dev._stream())
        torch.cuda.synchronize()
        self.counts = self.counts_t.cpu().numpy()[:200].view(abi.view_counts_dtype)[0]

    def table_bytes(self, n=None):
        n = int(self.counts["numNodes"]) if n is None else n
        return self.table[: n * 40].cpu().numpy().tobytes()

    def sample_bytes(self, n=None):
        n = int(self.counts["numSamples"]) if n is None else n
        return self.samples[: n * 16].cpu().numpy().tobytes()

    def poison_behind(self, nodes, samples):
        return (bool((self.table[nodes * 40:] == 0xA5).all()) and bool((self.samples[samples * 16:] == 0xA5).all()) and
                bool((self.counts_t[200:] == 0xA5).all()))


def _assert_matches(raw, mirror, cnt, what):
    assert raw.rc == 0, what
    assert raw.counts.tobytes() == cnt.tobytes(), f"{what}: counts {raw.counts} against the mirror's {cnt}"
    assert raw.table_bytes() == mirror.nodes.tobytes(), f"{what}: the table differs"
    written = 0 if int(cnt["error"]) else mirror.num_samples
    assert raw.sample_bytes(written) == mirror.samples.tobytes(), f"{what}: the samples differ"
    assert raw.poison_behind(mirror.num_nodes, written), f"{what}: written past the result"


def _uniforms(dev, base, T, bias=0, frozen=None):
    """Uniforms of this device with the box of `base`, camera T (frozen: transform_updateBound), 1920 x 1080, minNodeSize 64 * 2^bias."""
    mn, mx = np.asarray(base["boxMin"], np.float32).reshape(3), np.asarray(base["boxMax"], np.float32).reshape(3)
    u = dev.uniforms(W, H, T, (1.0, 1.0, 1.0), transform_update_bound=frozen, min_node_size=vr.MIN_NODE_SIZE * 2.0 ** bias)
    u["boxMin"], u["boxMax"] = mn, mx
    return u


def _box_of(u):
    mn, mx = np.asarray(u["boxMin"], np.float64).reshape(3), np.asarray(u["boxMax"], np.float64).reshape(3)
    return tuple(mx - mn), tuple(mn)


def _check_v8(dev, base, what, cameras=GPU_CAMERAS, biases=GPU_BIASES, replace=True, max_level=20):
    """Rule V8 on `dev`: per camera and bias the raw call against the frame's VISIBLE export and against the mirror — with the builder's chunk
    table valid and, `replace`, after simlod_octree_image_replaced.  -> nodes selected over all calls."""
    box, mn = _box_of(base)
    full = dev.export_octree(base)
    want, selected = [], 0
    for cam in cameras:
        T = vr.transform_of(cam, box, mn) if isinstance(cam, str) else cam
        cam = cam if isinstance(cam, str) else "given camera"
        u0 = _uniforms(dev, base, T)
        for b in biases:
            dev.render(_uniforms(dev, base, T, b))
            frame = dev.export_octree(base, max_level=max_level, select="visible")
            mirror, cnt = full.view(u0, bias=b, max_bias=b, max_level=max_level, return_counts=True)
            assert frame.nodes.tobytes() == mirror.nodes.tobytes() and frame.samples.tobytes() == mirror.samples.tobytes(), f"{what} {cam} bias {b}: the mirror is not the frame"
            want.append((f"{what} {cam} bias {b}", u0, abi.view_record(b, b), mirror, cnt))
            selected += int(cnt["numSelected"])
    for source in (("chunk table", "walk") if replace else ("as it is",)):
        for tag, u0, view, mirror, cnt in want:
            _assert_matches(Raw(dev, u0, view, max_level), mirror, cnt, f"{tag} ({source})")
        if replace:
            dev.L.simlod_octree_image_replaced(dev._p(dev.nodes))        # the builder's chunk table no longer counts: every list is walked
    return selected


@pytest.fixture(scope="module")
def terrain3m(built_libs):
    batches, box = vr.terrain_3m_batches()
    dev = _device()
    u = dev.uniforms(W, H, vr.transform_of("bird", box), box)
    dev.reset(u)
    _ingest(dev, u, batches)
    return dev, u, box, dev.export_octree(u)


# ---- 1. rule V8 on the device ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CASES + ["georef"])
def test_view_equals_a_frames_visible_export(built_libs, name):
    dev, u, _, _ = _build("terrain_4x100k", cases.GEOREF) if name == "georef" else _build(name)
    assert _check_v8(dev, u, name) > 0


def test_view_equals_a_frame_on_the_3m_terrain(terrain3m):
    dev, u, box, full = terrain3m
    assert _check_v8(dev, u, "3 M terrain") > 100
    # the Python entry points: a count-only call, then exact buffers
    u0 = _uniforms(dev, u, vr.transform_of("closer", box))
    mirror, cnt = full.view(u0, bias=1, return_counts=True)
    ex, c = dev.query_view(u0, bias=1, return_counts=True)
    assert ex.select == abi.EXPORT_VISIBLE and ex.nodes.tobytes() == mirror.nodes.tobytes() and ex.samples.tobytes() == mirror.samples.tobytes()
    assert c.tobytes() == cnt.tobytes() == dev.count_view(u0, bias=1).tobytes()
    ex.validate()


def test_view_equals_a_frame_on_the_deep_octree(built_libs):
    d = deep_ref.built("d13x")
    dev = _device()
    u = dev.uniforms(W, H, vr.transform_of("bird", d.box), d.box)
    dev.reset(u)
    _ingest(dev, u, d.batches)
    _check_v8(dev, u, "d13x")
    # (the cases' cameras see the cloud as a few pixels: a camera a few level-13 node sizes from the middle of its level-11 cell selects level-13 nodes)
    mid = d.origin + 0.5 * np.ldexp(d.size, -deep_ref.CELL_LEVEL)
    close = camera.lookat_transform(tuple(mid + np.asarray((3.0, -2.5, 2.5)) * np.ldexp(d.size, -deep_ref.LEAF_LEVEL)), tuple(mid), W, H)
    assert _check_v8(dev, u, "d13x close-up", cameras=[close], biases=[0, 1], replace=False) > 0
    mirror = dev.export_octree(u).view(_uniforms(dev, u, close))
    assert int((mirror.nodes["level"][(mirror.nodes["flags"] & abi.EXPORT_FLAG_SELECTED) != 0] == deep_ref.LEAF_LEVEL).sum()) >= 8


# ---- 2. the frozen camera ------------------------------------------------------------------------------------------------------------------------
def test_view_follows_the_frozen_camera(terrain3m):
    dev, u, box, full = terrain3m
    live, frozen = cases.frozen_pair("closer", box, W, H)
    uf = _uniforms(dev, u, live, frozen=frozen)
    mirror, cnt = full.view(uf, return_counts=True)
    dev.render(uf)
    frame = dev.export_octree(u, select="visible")
    assert frame.nodes.tobytes() == mirror.nodes.tobytes() and frame.samples.tobytes() == mirror.samples.tobytes()
    _assert_matches(Raw(dev, uf), mirror, cnt, "frozen camera")
    other, _ = full.view(_uniforms(dev, u, live), return_counts=True)
    assert other.nodes.tobytes() != mirror.nodes.tobytes(), "the live camera must choose other nodes"
    same, _ = full.view(_uniforms(dev, u, frozen), return_counts=True)
    assert same.nodes.tobytes() == mirror.nodes.tobytes()


# ---- 3. rule V9 ----------------------------------------------------------------------------------------------------------------------------------
def test_view_leaves_the_frame_state_alone(terrain3m):
    dev, u, box, full = terrain3m
    dev.render(_uniforms(dev, u, vr.transform_of("bird", box)))
    before = dev.export_octree(u, select="visible")
    assert before.num_samples > 0
    ui = _uniforms(dev, u, vr.transform_of("inside", box))
    S, _ = vr.ladder_of(full, ui, cull=False)
    ex = dev.query_view(ui, cull=False, budget=S[3])
    assert 0 < ex.num_samples <= S[3] and ex.nodes.tobytes() != before.nodes.tobytes()
    dev.count_view(ui, cull=False, budget=0, draw_small_root=True)
    after = dev.export_octree(u, select="visible")
    assert after.nodes.tobytes() == before.nodes.tobytes() and after.samples.tobytes() == before.samples.tobytes()
    again = dev.export_octree(u)
    assert again.nodes.tobytes() == full.nodes.tobytes() and again.samples.tobytes() == full.samples.tobytes()


# ---- 4. budget and ladder ------------------------------------------------------------------------------------------------------------------------
def _budget_cases(full, box, to_uniforms):
    """The CPU tier's budget cases as (what, uniforms, SimlodView) on an octree whose `closer` ladder has the rungs and whose `inside` ladder is
    not monotone."""
    u = to_uniforms(vr.transform_of("closer", box))
    S, _ = vr.ladder_of(full, u)
    vr.assert_closer_ladder(S)
    out = [("S(1)", u, abi.view_record(budget=S[1])), ("S(1) - 1", u, abi.view_record(budget=S[1] - 1)), ("0", u, abi.view_record(budget=0)),
           ("minBias 2", u, abi.view_record(2)), ("none fits", u, abi.view_record(0, 6, S[6] - 1)),
           ("no cull, small root", u, abi.view_record(budget=0, cull=False, draw_small_root=True))]
    ui = to_uniforms(vr.transform_of("inside", box))
    Si, _ = vr.ladder_of(full, ui)
    up = vr.assert_not_monotone(Si)
    out.append(("not monotone", ui, abi.view_record(budget=(Si[up] + Si[up + 1]) // 2)))
    return out


def _mirror_of(full, u, v, max_level=None):
    v = v[0]
    return full.view(u, int(v["minBias"]), int(v["maxBias"]), None if int(v["sampleBudget"]) == abi.VIEW_NO_BUDGET else int(v["sampleBudget"]),
                     not int(v["flags"]) & abi.VIEW_NO_CULL, bool(int(v["flags"]) & abi.VIEW_DRAW_SMALL_ROOT), max_level, return_counts=True)


def test_budget_chooses_the_bias(terrain3m):
    dev, u, box, full = terrain3m
    seen = {}
    for what, uu, view in _budget_cases(full, box, lambda T: _uniforms(dev, u, T)):
        mirror, cnt = _mirror_of(full, uu, view)
        raw = Raw(dev, uu, view)
        _assert_matches(raw, mirror, cnt, f"budget {what}")
        seen[what] = (int(raw.counts["bias"]), int(raw.counts["error"]))
    assert seen["S(1)"] == (1, 0) and seen["S(1) - 1"] == (2, 0) and seen["minBias 2"] == (2, 0) and seen["none fits"] == (6, abi.EXPORT_ERR_BUDGET)
    with pytest.raises(SimlodError):
        dev.query_view(_uniforms(dev, u, vr.transform_of("closer", box)), max_bias=0, budget=1)
    ex, c = dev.query_view(_uniforms(dev, u, vr.transform_of("closer", box)), max_bias=0, budget=1, return_counts=True)
    assert int(c["error"]) == abi.EXPORT_ERR_BUDGET and ex.num_samples == 0 and int(ex.nodes["numSamples"].astype(np.int64).sum()) == int(c["numSamples"]) > 1


# ---- 5. many nodes per level ---------------------------------------------------------------------------------------------------------------------
def test_levels_of_more_than_1024_entries(built_libs):
    tree = vr.complete_tree()
    assert int((tree.nodes["level"] == 4).sum()) > 1024 and int((tree.nodes["level"] == 3).sum()) < 1024
    dev = _device()
    dev.import_octree(tree)
    box = (1.0, 1.0, 1.0)
    base = dev.uniforms(W, H, vr.transform_of("inside", box), box)
    full = dev.export_octree(base)
    assert full.nodes.tobytes() == tree.nodes.tobytes() and full.samples.tobytes() == tree.samples.tobytes()
    selected = _check_v8(dev, base, "complete tree", cameras=["inside", "closer"], replace=False)
    _, c = full.view(_uniforms(dev, base, vr.transform_of("inside", box)), return_counts=True)
    assert 0 < int(c["numSelected"]) < int(c["numInside"]) < tree.num_nodes and selected > 0
    ui = _uniforms(dev, base, vr.transform_of("inside", box))
    S, _ = vr.ladder_of(full, ui)
    for what, view in (("S(2)", abi.view_record(budget=S[2])), ("S(2) - 1", abi.view_record(budget=S[2] - 1)), ("none fits", abi.view_record(0, 3, min(S[:4]) - 1)),
                       ("no cull", abi.view_record(1, 20, S[1], cull=False)), ("small root", abi.view_record(budget=0, draw_small_root=True))):
        mirror, cnt = _mirror_of(full, ui, view)
        _assert_matches(Raw(dev, ui, view), mirror, cnt, f"complete tree, budget {what}")


# ---- 6. count only, capacities, refused arguments ----------------------------------------------------------------------------------------------
def test_count_only_and_capacities(terrain3m):
    dev, u, box, full = terrain3m
    uc = _uniforms(dev, u, vr.transform_of("closer", box))
    view = abi.view_record(1, 1)
    ref = Raw(dev, uc, view)
    nn, ns = int(ref.counts["numNodes"]), int(ref.counts["numSamples"])
    assert ref.rc == 0 and int(ref.counts["error"]) == 0 and nn > 1 and ns > 0
    cnt = Raw(dev, uc, view, count_only=True)
    assert cnt.rc == 0 and cnt.counts.tobytes() == ref.counts.tobytes()
    assert cnt.table_bytes() == ref.table_bytes() and cnt.poison_behind(nn, 0)          # the table is complete, no sample was written
    # a count-only call needs no more scratch than the table's part
    lean = Raw(dev, uc, view, count_only=True, scratch_bytes=int(dev.L.simlod_export_buffer_min_bytes(nn, 0)))
    assert lean.rc == 0 and lean.counts.tobytes() == ref.counts.tobytes() and lean.table_bytes() == ref.table_bytes()
    # exact capacities: the full result
    exact = Raw(dev, uc, view, table_cap=nn, sample_cap=ns, scratch_bytes=int(dev.L.simlod_export_buffer_min_bytes(nn, ns)))
    assert exact.rc == 0 and exact.counts.tobytes() == ref.counts.tobytes()
    assert exact.table_bytes() == ref.table_bytes() and exact.sample_bytes() == ref.sample_bytes() and exact.poison_behind(nn, ns)
    # one sample short: the error bit, the counts still say what is needed, no sample is written
    short = Raw(dev, uc, view, table_cap=nn, sample_cap=ns - 1)
    assert short.rc == 0 and int(short.counts["error"]) == abi.EXPORT_ERR_CAPACITY and int(short.counts["numSamples"]) == ns
    assert short.poison_behind(nn, 0)
    # one table entry short: the error bit, nothing behind the capacity
    small = Raw(dev, uc, view, table_cap=nn - 1, sample_cap=ns)
    assert small.rc == 0 and int(small.counts["error"]) & abi.EXPORT_ERR_CAPACITY and int(small.counts["numNodes"]) <= nn - 1
    assert small.poison_behind(nn - 1, 0)
    # a scratch buffer with room for the table's part but not for the items: the device says so
    tight = Raw(dev, uc, view, scratch_bytes=int(dev.L.simlod_export_buffer_min_bytes(nn, 0)))
    assert tight.rc == 0 and int(tight.counts["error"]) & abi.EXPORT_ERR_CAPACITY and tight.poison_behind(nn, 0)


def test_invalid_arguments_enqueue_nothing(built_libs):
    dev, u, _, box = _build("uniform_3x40k")
    nn = int(dev.read_stats()["numNodes"])
    ok = _uniforms(dev, u, vr.transform_of("bird", box))

    def refused(uu=ok, **kw):
        raw = Raw(dev, uu, **kw)
        assert raw.rc == 1, kw                                                          # hipErrorInvalidValue
        assert bool((raw.counts_t == 0xA5).all()) and raw.poison_behind(0, 0) and bool((raw.scratch == 0xA5).all()), kw

    for null in ("nodes", "stats", "uniforms", "view", "scratch", "table", "counts"):
        refused(null=null)
    for field, value in (("flags", 4), ("flags", 1 << 31), ("reserved", 1), ("minBias", 3), ("maxBias", 21)):
        v = abi.view_record(0, 2)
        v[field] = value
        refused(view=v)
    for field, value in (("minNodeSize", np.nan), ("minNodeSize", np.inf), ("width", np.nan), ("height", -np.inf)):
        w = np.array(ok, copy=True)
        w[field] = value
        refused(uu=w)
    w = np.array(ok, copy=True)
    w["transform_updateBound"][3, 0] = np.nan
    refused(uu=w)
    refused(scratch_bytes=int(dev.L.simlod_export_buffer_min_bytes(nn, 0)) - 1)
    # what the query does not read may be anything
    w = np.array(ok, copy=True)
    w["transform"][1, 1] = np.nan
    assert Raw(dev, w).rc == 0


# ---- 7. maxLevel < 20 ------------------------------------------------------------------------------------------------------------------------------
def test_max_level_truncates_as_the_visible_export_does(built_libs):
    dev, u, _, _ = _build("terrain_4x100k")
    assert int(dev.export_octree(u).nodes["level"].max()) > 1
    assert _check_v8(dev, u, "terrain_4x100k @1", cameras=["closer", "inside"], biases=[0, 1], replace=False, max_level=1) > 0
