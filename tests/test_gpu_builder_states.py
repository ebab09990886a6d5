"""GPU tier: export and every query of the read side (export.hip) on each octree state an ingest can leave behind — a full node array
(leaves of 75 chunks, half again a chunk-table row), an import of those leaves and the resumed ingest that has to split them, deferred splits,
coalesced mode, a launch that stopped short with no host wait before the export, a tripped memory guard, a foreign image, a rank's octree
under a trunk mask, two octrees in one context and a rebuild in the same buffers.  Every state first asserts its precondition from Stats and
the downloaded image, then goes through ONE battery: the export anchored byte for byte to export_ref.export_host of the downloaded image,
the chunk table's stamp through the rasteriser's counter, one query of each kind against the numpy mirrors on the anchored export (guarded
and held against brute force over the points the octree holds, tests/states_ref.py) — a profile, pack / unpack of the export, two paint
calls with their undo, a lasso on the screen of the view's camera (and the footprint once more as a lasso), summaries of the region, the lasso
and the whole box (each once more from one workgroup), and the inverse of the region, the footprint and the lasso as a query, a summary and
three paints on top of each other with their undo, one of them a SET without `previous` —, and all of it again with the table dropped.
State B goes through the same battery twice: the plain import of A, and the buildable import of A before its resume.
Where the builder goes on after a state (B, C, E), the octree is painted whole first and must end as the oracle's octree of the recoloured
input (paint rule E7).  erase_region ends in an import, which leaves an octree render-only: it runs on a copy of the state in a second device
object (A, C deferred, G's root leaf, H, the larger octree of I) against the frames the state itself draws with SIMLOD_CLIP_OUTSIDE; and state E
enqueues an inverse summary, like its export, directly behind the launch that stops short."""
import ctypes

import numpy as np
import pytest
import torch

import cases
import oracle
import region_ref as rr
import states_ref as sr
import test_gpu_footprint as on_footprints
import test_gpu_inverse as on_inverse
import test_gpu_lasso as on_lassos
import test_gpu_neighbours as on_spheres
import test_gpu_pack as on_pack
import test_gpu_paint as on_paint
import test_gpu_profile as on_profile
import test_gpu_rays as on_rays
import test_gpu_region as on_regions
import test_gpu_summary as on_summary
import test_gpu_view as on_view
import test_gpu_view_delta as on_delta
import view_ref as vr
from export_ref import export_host
from simlod_amd import abi, synthetic
from simlod_amd.octree_io import Clip, OctreeExport, Paint, Region
from states_ref import State
from test_gpu_deep_octrees import _count_fields, _feed_one_by_one, _feed_one_group
from test_gpu_export import _assert_export, _device, _frames_equal
from test_gpu_parity import GRANULARITY_FREE_FIELDS
from test_gpu_resume import _assert_fields, _feed, _import, _resume_batches
from test_gpu_trunk import _partition
from util import host_image_of, points_multiset_hash

pytestmark = pytest.mark.gpu
W, H = cases.W, cases.H
NODE_CAPACITY = 263_157


# ---- the battery -----------------------------------------------------------------------------------------------------------------------------
def _anchor(S, what):
    """Point 1: the full export, the cut one level above the deepest and `visible` after a frame, each byte-equal to export_host of the
    downloaded image; the cut's samples are the points held.  -> (the anchored full export, chunk lists the frame read through the table)"""
    dev, u = S.dev, S.u
    nodes, pers, nn = host_image_of(dev)
    t, s = export_host(nodes, nn)
    full = dev.export_octree(u)
    _assert_export(full, t, s, f"{what} all@20")
    ml = max(int(t["level"].max()) - 1, 0)
    tc, sc = export_host(nodes, nn, ml, abi.EXPORT_CUT)
    _assert_export(dev.export_octree(u, max_level=ml, select="cut"), tc, sc, f"{what} cut@{ml}")
    rr.assert_same_multiset(full.truncated(20, "cut").samples, S.pts, f"{what}: the cut against the points held")
    # the stamp's frame: minNodeSize 1 makes every node on the screen large, so leaves are drawn — the rasteriser takes a list from the table only
    # when it fits a row, and the inner nodes the cases' frames draw of a dense octree hold more voxel chunks than that
    us = np.array(u, copy=True)
    us["minNodeSize"] = 1.0
    dev.render(us)
    used = dev.lists_read_through_table()
    dev.render(u)
    nodes, pers, nn = host_image_of(dev)
    tv, sv = export_host(nodes, nn, 20, abi.EXPORT_VISIBLE)
    assert len(sv) > 0, f"{what}: the frame draws nothing"
    _assert_export(dev.export_octree(u, select="visible"), tv, sv, f"{what} visible")
    return full, used


def _crops(S, M, what):
    for (kind, sel), (mirror, cnt) in M["crop"].items():
        q = M["q"]
        mk = (lambda **kw: on_regions.Raw(S.dev, S.u, q.region, 20, sel, **kw)) if kind == "region" else (lambda **kw: on_footprints.Raw(S.dev, S.u, q.footprint, None, 20, sel, **kw))
        (on_regions if kind == "region" else on_footprints)._assert_matches(mk(), mirror, cnt, f"{what} {kind} {sel}")
        only = mk(count_only=True)
        assert only.rc == 0 and _count_fields(only.counts) == _count_fields(cnt), f"{what} {kind} {sel}: the count-only call"


def _pairs(S, full, M, what):
    q = M["q"]
    for sel, (hits, cnt) in M["rays"].items():
        on_rays._assert_matches(on_rays.Raw(S.dev, S.u, q.rays, 20, sel), hits, cnt, f"{what} rays {sel}", full.truncated(20, sel))
        only = on_rays.Raw(S.dev, S.u, q.rays, 20, sel, count_only=True)
        assert only.rc == 0 and _count_fields(only.counts) == _count_fields(cnt), f"{what} rays {sel}: the count-only call"
    for sel, want in M["spheres"].items():
        on_spheres._assert_matches(on_spheres.Raw(S.dev, S.u, q.spheres, sr.K, 20, sel), want, f"{what} spheres {sel}", full.truncated(20, sel))
        only = on_spheres.Raw(S.dev, S.u, q.spheres, sr.K, 20, sel, count_only=True)
        fields = on_spheres.COUNT_FIELDS
        assert only.rc == 0 and all(int(only.counts[f]) == int(want[2][f]) for f in fields[:6]) and int(only.counts["numFound"]) == 0, f"{what} spheres {sel}: the count-only call"


def _views(S, uv, M, what):
    dev = S.dev
    for tag, view, (mirror, cnt) in (("view", abi.view_record(), M["view"]), ("budget", abi.view_record(budget=M["budget"]), M["coarser"])):
        on_view._assert_matches(on_view.Raw(dev, uv, view), mirror, cnt, f"{what} {tag}")
        only = on_view.Raw(dev, uv, view, count_only=True)
        assert only.rc == 0 and only.counts.tobytes() == cnt.tobytes() and only.poison_behind(mirror.num_nodes, 0), f"{what} {tag}: the count-only call"
    raw = on_delta.RawDelta(dev, uv, M["held"], abi.view_record(), tails=True)
    on_delta._assert_delta(raw, M["delta"], f"{what} delta")
    on_delta._assert_merge(dev, raw, M["held"], uv, abi.view_record(), f"{what} delta")
    only = on_delta.RawDelta(dev, uv, M["held"], abi.view_record(), tails=True, count_only=True)
    assert only.rc == 0 and only.counts.tobytes() == M["delta"].counts.tobytes(), f"{what} delta: the count-only call"


def _profiles(S, M, what):
    """The corridor, cut and all: counts, table, samples and records byte for byte, poison behind them; the count-only call.
    -> the device's counts of the cut"""
    q = M["q"]
    for sel, (mirror, rec, cnt) in M["profile"].items():
        raw = on_profile.Raw(S.dev, S.u, q.profile, None, 20, sel)
        on_profile._assert_matches(raw, mirror, rec, cnt, f"{what} profile {sel}")
        only = on_profile.Raw(S.dev, S.u, q.profile, None, 20, sel, count_only=True, null_records=True)
        assert only.rc == 0 and _count_fields(only.counts) == _count_fields(cnt) and only.table_bytes() == mirror.nodes.tobytes(), f"{what} profile {sel}: the count-only call"
        assert only.poison_behind(mirror.num_nodes, 0), f"{what} profile {sel}: the count-only call wrote a sample or a record"
        if sel == "cut":
            counts = raw.counts
    return counts


def _packs(S, full, M, what):
    """simlod_pack_samples and simlod_unpack_samples on the anchored full export against the mirror; the calls leave their inputs alone."""
    px, pc, mback, uc = M["pack"]
    packed, c, back = on_pack._assert_raw_is_mirror(S.dev, full.nodes, full.samples, full.box_min, full.box_max, what=f"{what} pack")
    assert packed.tobytes() == px.packed.tobytes() and c.tobytes() == pc.tobytes() and back.tobytes() == mback.samples.tobytes(), f"{what} pack: not the battery's mirror"


def _paints(S, M, what):
    """The two paint calls of the mirror, then their undo in reverse order.  After each call: counts and table are the count-only query's,
    `previous` is the mirror's with poison behind numSamples, the export is the mirror's, the Node array and Stats are as before.  After the
    undo the image — Node array, Stats, every allocated byte of the persistent buffer — is the one taken before.  -> samples painted per call"""
    dev, u = S.dev, S.u
    before = on_paint._image(dev)
    painted = []
    for k, call in enumerate(M["paint"]):
        tag = f"{what} paint call {k + 1}"
        n = int(call.counts["numSamples"])
        qtable, qc = on_paint._count_only(dev, u, call.region, call.footprint)
        raw = on_paint.Raw(dev, u, call.paint, call.region, call.footprint, colors=call.colors)
        assert raw.rc == 0 and _count_fields(raw.counts) == _count_fields(call.counts), f"{tag}: counts {raw.counts}, the mirror has {call.counts}"
        assert raw.counts.tobytes() == qc.tobytes() and raw.table_bytes(int(qc["numNodes"])) == qtable, f"{tag}: not the count-only query's table"
        assert bool((raw.table[int(qc["numNodes"]) * 40:] == 0xA5).all()), f"{tag}: the table was written past numNodes"
        got = raw.previous()
        assert np.array_equal(got[:n], call.previous), f"{tag}: {int((got[:n] != call.previous).sum())} words of previous differ, the first at {int(np.argmax(got[:n] != call.previous))}"
        assert (got[n:] == on_paint.POISON).all(), f"{tag}: previous was written past numSamples"
        ex = dev.export_octree(u)
        assert ex.nodes.tobytes() == call.export.nodes.tobytes(), f"{tag}: the table of the export moved"
        assert ex.samples.tobytes() == call.export.samples.tobytes(), f"{tag}: {int((ex.samples['color'] != call.export.samples['color']).sum())} colours differ from the mirror's"
        nodes, stats, pers = on_paint._image(dev)
        assert nodes == before[0] and stats == before[1] and pers != before[2], f"{tag}: the Node array or Stats moved, or nothing was painted"
        painted.append(int(raw.counts["numSamples"]))
    for call in reversed(M["paint"]):
        raw = on_paint.Raw(dev, u, Paint.array(), call.region, call.footprint, colors=call.previous, previous=False)
        assert raw.rc == 0 and _count_fields(raw.counts) == _count_fields(call.counts), f"{what}: the undo's counts"
    after = on_paint._image(dev)
    assert after[0] == before[0] and after[1] == before[1], f"{what}: the Node array or Stats differ after the undo"
    assert after[2] == before[2], f"{what}: the persistent buffer differs after the undo"
    return painted


def _lassos(S, M, what):
    """simlod_query_lasso for the screen lasso, cut and all, and for the footprint's lasso: counts, table and samples byte for byte, poison
    behind them; the count-only call has the same counts and table and writes no sample.  -> the mirror's counts of the cut"""
    q = M["q"]
    for key, (mirror, cnt) in M["lasso"].items():
        lasso, sel = (q.foot_lasso, "cut") if key == "footprint" else (q.lasso, key)
        on_lassos._assert_matches(on_lassos.Raw(S.dev, S.u, lasso, None, 20, sel), mirror, cnt, f"{what} lasso {key}")
        only = on_lassos.Raw(S.dev, S.u, lasso, None, 20, sel, count_only=True)
        assert only.rc == 0 and _count_fields(only.counts) == _count_fields(cnt) and only.table_bytes() == mirror.nodes.tobytes(), f"{what} lasso {key}: the count-only call"
        assert only.poison_behind(mirror.num_nodes, 0), f"{what} lasso {key}: the count-only call wrote a sample"
    return M["lasso"]["cut"][1]


def _assert_summary(raw, want, cnt, table, what):
    """One raw summary call of any of the three entry points: counts, table and record are the mirror's, poison behind table and record."""
    assert raw.rc == 0 and _count_fields(raw.counts) == _count_fields(cnt), f"{what}: counts {raw.counts}, the mirror has {cnt}"
    n = int(cnt["numNodes"])
    assert raw.table[: n * 40].cpu().numpy().tobytes() == table.tobytes(), f"{what}: the table differs"
    assert bool((raw.table[n * 40:] == 0xA5).all()) and bool((raw.out_t[on_summary.NBYTES:] == 0xA5).all()), f"{what}: written past the table or the record"
    got = raw.out_t[: on_summary.NBYTES].cpu().numpy().view(abi.summary_dtype)[0]
    for f in abi.summary_dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), f"{what}: {f} differs: {got[f]} != {want[f]}"
    assert raw.summary_bytes() == want.tobytes(), what


def _summaries(S, M, what):
    """simlod_query_summary for the region (cut and all) and the whole box, simlod_query_summary_lasso for the screen lasso: the record byte
    for byte the mirror's, and once more from ONE workgroup (rule S7: the bytes do not depend on the grid).  -> the mirror's Summary of the
    region's cut"""
    q = M["q"]
    for (kind, sel), (want, cnt, table) in M["summary"].items():
        for wg in (0, 1):
            if kind == "lasso":
                raw = on_lassos.RawSummary(S.dev, S.u, Region(), q.lasso, ml=20, sel=sel, z0=q.z0, scale=q.scale, max_wg=wg)
            else:
                raw = on_summary.Raw(S.dev, S.u, q.region if kind == "region" else Region(), None, ml=20, sel=sel, z0=q.z0, scale=q.scale, max_wg=wg)
            _assert_summary(raw, want, cnt, table, f"{what} summary {kind} {sel}, maxWorkgroups {wg}")
    return M["summary"]["region", "cut"][0]


def _inverses(S, M, what):
    """simlod_query_inverse (cut, all and count-only), simlod_query_summary_inverse and simlod_paint_inverse for the region, the footprint and
    the screen lasso against the mirrors.  The three paints stand on top of each other — the first a SET without `previous`, the path that
    stores without loading on the chunks the positive query culls —; after each the export is the mirror's and the Node array and Stats are
    as before; ARRAY paints of `previous` in reverse order (for the SET: the colours the mirror remembers) give back the image taken before,
    Node array, Stats and every allocated byte of the persistent buffer.  -> the mirror's counts of the three cuts"""
    dev, u, q, I = S.dev, S.u, M["q"], M["inverse"]
    sels = sr.selections(q)
    for (kind, sel), (mirror, cnt) in I["query"].items():
        on_inverse._assert_matches(on_inverse.Raw(dev, u, sels[kind], 20, sel), mirror, cnt, f"{what} inverse {kind} {sel}")
        only = on_inverse.Raw(dev, u, sels[kind], 20, sel, count_only=True)
        assert only.rc == 0 and _count_fields(only.counts) == _count_fields(cnt) and only.table_bytes() == mirror.nodes.tobytes(), f"{what} inverse {kind} {sel}: the count-only call"
        assert only.poison_behind(mirror.num_nodes, 0), f"{what} inverse {kind} {sel}: the count-only call wrote a sample"
    for (kind, sel), (want, cnt) in I["summary"].items():
        raw = on_inverse.RawSummary(dev, u, sels[kind], ml=20, sel=sel, z0=q.z0, scale=q.scale)
        _assert_summary(raw, want, cnt, I["query"][kind, sel][0].nodes, f"{what} inverse summary {kind} {sel}")
    before = on_paint._image(dev)
    for kind, call in zip(sels, I["paint"]):
        tag = f"{what} inverse paint by the {kind}"
        n = int(call.counts["numSamples"])
        raw = on_inverse.RawPaint(dev, u, call.paint, call.sel3, colors=call.colors, previous=call.with_previous)
        assert raw.rc == 0 and _count_fields(raw.counts) == _count_fields(call.counts), f"{tag}: counts {raw.counts}, the mirror has {call.counts}"
        nn = int(call.counts["numNodes"])
        assert raw.table[: nn * 40].cpu().numpy().tobytes() == I["query"][kind, "all"][0].nodes.tobytes(), f"{tag}: not the inverse query's table (rule I8)"
        assert bool((raw.table[nn * 40:] == 0xA5).all()), f"{tag}: the table was written past numNodes"
        got = raw.previous()
        if call.with_previous:
            assert np.array_equal(got[:n], call.previous), f"{tag}: {int((got[:n] != call.previous).sum())} words of previous differ, the first at {int(np.argmax(got[:n] != call.previous))}"
            assert (got[n:] == on_inverse.POISON).all(), f"{tag}: previous was written past numSamples"
        else:
            assert (got == on_inverse.POISON).all(), f"{tag}: previous was written without being given"
        ex = dev.export_octree(u)
        assert ex.nodes.tobytes() == call.export.nodes.tobytes(), f"{tag}: the table of the export moved"
        assert ex.samples.tobytes() == call.export.samples.tobytes(), f"{tag}: {int((ex.samples['color'] != call.export.samples['color']).sum())} colours differ from the mirror's"
        # (the export above shows what was painted; the persistent buffer's bytes are compared once, after the undo)
        assert dev.nodes[: len(before[0])].cpu().numpy().tobytes() == before[0] and dev.stats.cpu().numpy().tobytes() == before[1], f"{tag}: the Node array or Stats moved"
    for call in reversed(I["paint"]):
        raw = on_inverse.RawPaint(dev, u, Paint.array(), call.sel3, colors=call.previous, previous=False)
        assert raw.rc == 0 and _count_fields(raw.counts) == _count_fields(call.counts), f"{what}: the counts of the inverse paints' undo"
    after = on_paint._image(dev)
    assert after[0] == before[0] and after[1] == before[1], f"{what}: the Node array or Stats differ after the inverse paints' undo"
    assert after[2] == before[2], f"{what}: the persistent buffer differs after the inverse paints' undo"
    return {kind: I["query"][kind, "cut"][1] for kind in sels}


def _battery(S, table, what, shape=sr.Shape(), pairs_all=False, between=None, erase=None, check=None, cache=None):
    """Points 1-4 of the battery on one state.  table: whether the state claims a valid chunk table — True: a frame reads lists through it;
    False: it must not; "long": the stamp holds, but every list a frame can draw is longer than a row and the rasteriser, which takes whole
    rows only, reads none (the read side takes the row and follows `next` behind it: the fault table of DESIGN §7 shows that it does).
    between(): called between the crops and the pair queries (a host whose launches keep coming).  erase ("frames" / "no frames"): after
    everything else, _erase_on_a_copy.  check(full, M): a guard of the state's own on the anchored export and the mirrors, before the device
    is asked.  cache (a dict): the mirrors of an anchored export are kept in it and taken from it for an export that is byte for byte the same (A and its
    imports: the mirrors depend on the export, the points and the camera alone).  -> the anchored full export"""
    dev = S.dev
    full, used = _anchor(S, what)
    print(f"{what}: {full.num_nodes} nodes, {full.num_samples} samples, {used} lists read through the table")
    assert (used > 0) if table is True else (used == 0), f"{what}: {used} chunk lists read through the table"
    uv = on_view._uniforms(dev, S.u, vr.transform_of(shape.camera, S.box))
    image = (full.nodes.tobytes(), full.samples.tobytes(), shape, pairs_all)
    if cache is not None and cache.get("image") == image:
        M = cache["mirrors"]
    else:
        M = sr.mirrors(full, S.pts, uv, what, shape, pairs_all)
        if cache is not None:
            cache.update(image=image, mirrors=M)
    if check is not None:
        check(full, M)
    for source in ("chunk table" if table else "no table", "walk"):
        _crops(S, M, f"{what} ({source})")
        if between is not None:
            between()
        _pairs(S, full, M, f"{what} ({source})")
        _views(S, uv, M, f"{what} ({source})")
        pc = _profiles(S, M, f"{what} ({source})")
        _packs(S, full, M, f"{what} ({source})")
        lc = _lassos(S, M, f"{what} ({source})")
        sm = _summaries(S, M, f"{what} ({source})")
        painted = _paints(S, M, f"{what} ({source})")           # last, with the inverses: they write the octree, and undo it
        ic = _inverses(S, M, f"{what} ({source})")
        print(f"{what} ({source}): the profile copies {int(pc['numCopiedNodes'])} nodes and filters {int(pc['numFilteredNodes'])} ({int(pc['numSamples'])} samples), "
              f"the paint calls recolour {painted[0]} and {painted[1]} samples")
        print(f"{what} ({source}): the lasso copies {int(lc['numCopiedNodes'])} nodes and filters {int(lc['numFilteredNodes'])} ({int(lc['numSamples'])} samples), the region's summary holds "
              f"{sm.num_samples} samples; the inverses (leaves copied / filtered / emptied, samples): "
              + ", ".join(f"{kind} {int(c['numCopiedNodes'])} / {int(c['numFilteredNodes'])} / {M['inverse']['classes'][kind][0]}, {int(c['numSamples'])}" for kind, c in ic.items())
              + f"; the inverse paints recolour {', '.join(str(int(p.counts['numSamples'])) for p in M['inverse']['paint'])} samples")
        if source != "walk":
            assert dev.L.simlod_octree_image_replaced(dev._p(dev.nodes)) == 0    # point 4, last: the builder's side tables go with it
    dev.render(S.u)
    assert dev.lists_read_through_table() == 0, f"{what}: the table is still read after simlod_octree_image_replaced"
    if erase is not None:
        _erase_on_a_copy(S, full, M, what, frames=erase == "frames")
    return full


def _erase_on_a_copy(S, full, M, what, frames=True):
    """erase_region on a state: the import it ends with leaves an octree render-only, so it runs on a COPY — the state's export imported into
    a second device object whose node array was poisoned — and the state's builder can go on.  What test_erase_makes_clip_outside_permanent
    asserts: the counts are the mirror's inverse (all@20) of the battery's region; Stats; the copy's frames, plain and HQS, are word for word
    the frames the SOURCE draws with Clip(region, "outside"); the re-export is the mirror's inverse byte for byte.  Then the footprint erased
    from what is left: the leaves the star holds whole are listed at zero samples.  frames=False: an octree whose root is a leaf — the export
    carries the root's points and not its voxel list, which a render-only import does not give back (include/simlod_hip.h: only the
    buildable import promises "a root that is still a leaf gets its voxels back"), so the header promises no equal frame there."""
    src, u = S.dev, S.u
    q = M["q"]
    mirror, cnt = M["inverse"]["query"]["region", "all"]
    dst = _device()
    dst.nodes.fill_(0xA5)
    dst.import_octree(src.export_octree(u))
    assert int(dst.read_stats()["dbg"]) == 0
    us = []
    for hqs in (False, True):
        us.append(np.array(u, copy=True))
        us[-1]["useHighQualityShading"], us[-1]["showBoundingBox"] = hqs, False
    clipped = []
    if frames:
        assert full.nodes["childMask"][0] != 0
        src.set_clip(Clip(q.region, "outside"))
        try:
            for v in us:
                src.render(v)
                clipped.append(src.framebuffer(W, H).copy())
        finally:
            src.set_clip(None)
        src.render(us[0])
        assert not np.array_equal(src.framebuffer(W, H), clipped[0]), f"{what}: the clip must change the frame"
    else:
        assert full.num_nodes == 1
    c = dst.erase_region(us[0], q.region)
    assert _count_fields(c) == _count_fields(cnt), f"{what} erase: counts {c}, the mirror's inverse has {cnt}"
    assert 0 < int(c["numSamples"]) < full.num_samples
    st = dst.read_stats()
    assert int(st["dbg"]) == 0 and int(st["numPoints"]) + int(st["numVoxels"]) == int(c["numSamples"]) and int(st["numNodes"]) == full.num_nodes
    for v, want in zip(us, clipped):
        dst.render(v)
        got = dst.framebuffer(W, H)
        assert int(dst.read_stats()["dbg"]) == 0
        diff = np.nonzero(got != want)[0]
        assert len(diff) == 0, f"{what} erase, hqs={int(v['useHighQualityShading'])}: {len(diff)} pixels differ from the clipped frame of the source, first {diff[:5]}"
        assert int((got != abi.CLEAR_PIXEL).sum()) > 100
    after = dst.export_octree(us[0]).to("cpu")
    assert after.nodes.tobytes() == mirror.nodes.tobytes() and after.samples.tobytes() == mirror.samples.tobytes(), f"{what} erase: the re-export is not the mirror's inverse"
    c2 = dst.erase_region(us[0], Region(), footprint=q.footprint)
    mirror2, cnt2 = after.crop(Region(), 20, "all", return_counts=True, footprint=q.footprint, invert=True)
    # (on G's root leaf, and only there, the star holds ALL the region's inverse left: the octree that is left is empty, and still the mirror's)
    assert _count_fields(c2) == _count_fields(cnt2) and (0 if frames else -1) < int(c2["numSamples"]) < int(c["numSamples"]), f"{what} erase, the footprint: counts {c2}, the mirror has {cnt2}"
    twice = dst.export_octree(us[0])
    assert twice.nodes.tobytes() == mirror2.nodes.tobytes() and twice.samples.tobytes() == mirror2.samples.tobytes(), f"{what} erase, the footprint: the re-export"
    emptied = int(((after.nodes["numSamples"] > 0) & (mirror2.nodes["numSamples"] == 0)).sum())
    print(f"{what} erase: {int(c['numSamples'])} of {full.num_samples} samples left by the region, {int(c2['numSamples'])} by the footprint, which empties {emptied} nodes")
    with pytest.raises(Exception):
        dst.construct(us[0])                 # render-only until a reset
    dst.close()


PAINTED = 0xFF57C0DE                         # a colour no input point carries (each test asserts it)


def _paint_everything(dev, u, pts):
    """Rule E7's setup: a whole-box SET with PAINTED, one simlod_paint_region call and nothing else -> its counts"""
    assert not (pts["color"] == PAINTED).any()
    c = dev.paint_region(u, Region(), Paint.set(PAINTED))
    assert int(c["numFilteredNodes"]) == 0 and int(c["numSamples"]) == int(c["numCandidates"]) > 0
    return c


def _recoloured(pts, n):
    """`pts` with the first n points in PAINTED: what the oracle is fed where the device painted after n points"""
    out = pts.copy()
    out["color"][:n] = PAINTED
    return out


def _leaf_mask(ex):
    return np.repeat((ex.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0, ex.nodes["numSamples"].astype(np.int64))


def _positions(p):
    w = np.stack([p[a].view(np.uint32) for a in ("x", "y", "z")], axis=1)
    return w[np.lexsort(w.T)]


def _new(box, **kw):
    dev = _device(**kw)
    u = dev.uniforms(W, H, cases._cam(box), box)
    dev.reset(u)
    return dev, u


def _oracle_export(box, batches, **kw):
    ho, u, _ = sr.oracle_build(box, batches, **kw)
    return sr.export_of(ho, u), ho


# ---- A. node array full: over-full leaves ----------------------------------------------------------------------------------------------------
_A, _A_MIRRORS = {}, {}


def _state_a():
    """State A once per module, with the delta of its growth across slot 50 checked on the way: -> (device, uniforms, points, box, the full
    export before the battery dropped the table)"""
    if "dev" not in _A:
        pts, box, batches = sr.a_input()
        dev, u = _new(box, ring_slots=4, max_nodes=9)
        _feed(dev, u, batches[:3])
        uc = on_view._uniforms(dev, u, vr.transform_of("closer", box))
        view = abi.view_record()
        held = on_delta._host(on_view.Raw(dev, uc, view), u)
        _feed(dev, u, batches[3:])
        st = dev.read_stats()
        full = dev.export_octree(u)
        sr.assert_state_a(st["dbg"], full.nodes)
        assert int(st["numNodes"]) == 9 and int(st["numPoints"]) == len(pts) == int(st["numPointsProcessed"])
        _A.update(dev=dev, u=u, pts=pts, box=box, full=full, held=held, uc=uc)
    return _A


@pytest.fixture(scope="module", autouse=True)
def _release(built_libs):
    from simlod_amd.runtime import lib
    yield
    _A.clear()
    _A_MIRRORS.clear()
    lib().simlod_set_node_capacity(NODE_CAPACITY)


def test_a_growth_across_slot_50_is_sent_as_tails(built_libs):
    """Held after three batches (55 905 .. 56 863 points per leaf), asked after the fourth (74 517 .. 75 680): all eight leaves GROWN, each
    first piece begins in chunk 55 or 56 — behind the row's 50 slots — and the merge is the raw view."""
    a = _state_a()
    dev, held, uc, full = a["dev"], a["held"], a["uc"], a["full"]
    hn = held.nodes["numSamples"][1:].astype(np.int64)
    assert held.num_nodes == 9 and (hn > sr.ROW * abi.POINTS_PER_CHUNK).all() and set((hn // abi.POINTS_PER_CHUNK).tolist()) <= {55, 56}, hn
    view = abi.view_record()
    for tails in (True, False):
        mirror = full.view_delta(uc, held, tails=tails)
        raw = on_delta.RawDelta(dev, uc, held, view, tails=tails)
        on_delta._assert_delta(raw, mirror, f"A growth, tails {tails}")
        on_delta._assert_merge(dev, raw, held, uc, view, f"A growth, tails {tails}")
        e = mirror.entries[1:]
        if tails:
            assert (e["state"] == abi.DELTA_GROWN).all() and np.array_equal(e["numKept"].astype(np.int64), hn) and (e["numDelta"] > 18_000).all()
            assert int(mirror.counts["numGrown"]) == 8 and mirror.num_samples == 600_000 - int(hn.sum())
            _pack_the_grown_delta(dev, uc, held, mirror, hn)
        else:
            assert (e["state"] == abi.DELTA_ADDED).all() and mirror.num_samples == 600_000


def _pack_the_grown_delta(dev, uc, held, mirror, hn):
    """Rule K5 on GROWN entries made by the device: eight ranges of 18 000 and more samples that begin at firstDelta behind numKept of 55 905 ..
    56 863 (no multiple of a piece), in level-1 leaf frames of 75 000 points — the packed words and counts are the mirror's, the unpacked delta
    is the mirror's, and the merge of the unpacked delta has the exact merge's table, its voxels bit for bit and its leaf points within rule
    K8's bound with their colours."""
    import pack_ref as kr
    delta = dev.query_view_delta(uc, held, tails=True)
    assert delta.entries.tobytes() == mirror.entries.tobytes() and delta.samples.tobytes() == mirror.samples.tobytes() and delta.nodes.tobytes() == mirror.nodes.tobytes()
    before = [x.clone() for x in (delta.table_tensor, delta.entries_tensor, delta.samples_tensor)]
    pd, c = dev.pack(delta, return_counts=True)
    mp, mc = mirror.pack(return_counts=True)
    assert c.tobytes() == mc.tobytes(), f"A growth, packed: counts {c}, the mirror has {mc}"
    assert int(c["numSamples"]) == delta.num_samples == 600_000 - int(hn.sum()) and int(c["numInexact"]) == 0 and int(c["numAlpha"]) == 0 and int(c["error"]) == 0
    assert pd.packed.tobytes() == mp.packed.tobytes(), f"A growth, packed: {int((pd.packed != mp.packed).sum())} words differ from the mirror's"
    back = dev.unpack(pd)
    assert back.samples.tobytes() == mp.unpack().samples.tobytes(), "A growth, unpacked: the samples differ from the mirror's"
    assert back.entries.tobytes() == delta.entries.tobytes() and back.nodes.tobytes() == delta.nodes.tobytes()
    assert all(bool((a == b).all()) for a, b in zip(before, (delta.table_tensor, delta.entries_tensor, delta.samples_tensor))), "A growth: pack or unpack changed its inputs"
    # the delta's own ranges: every sample of the eight GROWN leaf entries within the bound of a level-1 frame
    n, worst = kr.assert_points_within_bound(delta.nodes, delta.samples, back.samples, delta.box_min, delta.box_max, entries=delta.entries, what="A growth, the delta's ranges")
    assert n == delta.num_samples, f"{n} of {delta.num_samples} delta samples checked"
    exact, lossy = dev.merge_view_delta(held, delta), dev.merge_view_delta(held, back)
    assert lossy.nodes.tobytes() == exact.nodes.tobytes() and lossy.num_samples == exact.num_samples
    vox = kr.voxel_mask(exact.nodes, exact.num_samples)                     # (the root's voxels, where the camera selects it)
    assert int((~vox).sum()) == 600_000 and lossy.samples[vox].tobytes() == exact.samples[vox].tobytes()
    leaf = np.nonzero((exact.nodes["flags"] & abi.EXPORT_FLAG_LEAF) != 0)[0]
    assert len(leaf) == 8 and (exact.nodes["level"][leaf] == 1).all()
    n, worst = kr.assert_points_within_bound(exact.nodes, exact.samples, lossy.samples, exact.box_min, exact.box_max, what="A growth, merged leaf entries")
    assert n == 600_000 and (lossy.samples[~vox]["color"] == exact.samples[~vox]["color"]).all()
    # the kept heads are the receiver's own samples, exact; the tails did change (13 bits per axis)
    for t, k in zip(leaf, hn):
        a = int(exact.nodes["firstSample"][t])
        assert lossy.samples[a: a + int(k)].tobytes() == exact.samples[a: a + int(k)].tobytes()
    assert lossy.samples.tobytes() != exact.samples.tobytes()


def test_a_leaves_hold_what_the_oracles_subtrees_hold(built_libs):
    a = _state_a()
    pts, box, batches = sr.a_input()
    want, _ = _oracle_export(box, batches)
    assert want.num_nodes == 73 and not len(sr.overfull_leaves(want.nodes))
    sr.assert_same_per_node(a["full"], sr.collapse(want), "A against the oracle's octree collapsed onto level 1")


def test_a_battery(built_libs):
    a = _state_a()
    _battery(State(a["dev"], a["u"], a["pts"], a["box"]), "long", "A", sr.SHAPES["A"], pairs_all=True, erase="frames", cache=_A_MIRRORS)


# ---- B. import of A ---------------------------------------------------------------------------------------------------------------------------
def test_b_plain_import_through_a_file(built_libs, tmp_path):
    a = _state_a()
    src, u, full = a["dev"], a["u"], a["full"]
    full.save(tmp_path / "a.simlodx")
    ld = OctreeExport.load(tmp_path / "a.simlodx")
    dst = _device()
    dst.nodes.fill_(0xA5)
    dst.import_octree(ld)
    assert int(dst.read_stats()["dbg"]) == 0
    re = dst.export_octree(u)
    assert re.nodes.tobytes() == full.nodes.tobytes() and re.samples.tobytes() == full.samples.tobytes(), "the re-export differs"
    _frames_equal(src, dst, u, "B plain import")
    # the whole battery on the import: eight leaves of 75 chunks the IMPORT wrote, no chunk table (the import drops it), every list walked
    # by `next` from the first chunk on — with A's Shape, long_leaves among it: every inverse result and every summary reaches behind slot 50
    _battery(State(dst, u, a["pts"], a["box"]), False, "B plain import", sr.SHAPES["B"], pairs_all=True, cache=_A_MIRRORS)


@pytest.mark.parametrize("mode", ["batch_by_batch", "one_group"])
def test_b_resume_splits_the_imported_overfull_leaves(built_libs, tmp_path, mode):
    """The outcome: the resumed ingest catches up — the late splits of the eight imported leaves run from tables the import rebuilt, and the
    octree ends as the oracle's continuous build of all 800 000 points."""
    a = _state_a()
    pts, box, more = sr.b_input()
    a["full"].save(tmp_path / "a.simlodx")
    ld = OctreeExport.load(tmp_path / "a.simlodx")
    assert ld.is_buildable and len(sr.overfull_leaves(ld.nodes)) == 8
    dst = _device()
    dst.tune("SIMLOD_EXACT_GROUP", 1 if mode == "batch_by_batch" else 2)
    uu = _import(dst, ld, a["u"])
    if mode == "batch_by_batch":
        # the battery on the buildable import BEFORE its resume (grids rebuilt, a builder state as after a reset, the over-full leaves pending):
        # the builder goes on afterwards, from the tables it rebuilds behind the battery's simlod_octree_image_replaced
        _battery(State(dst, uu, a["pts"], a["box"]), False, "B buildable import", sr.SHAPES["B"], pairs_all=True, cache=_A_MIRRORS)
    (_feed_one_by_one if mode == "batch_by_batch" else _feed_one_group)(dst, uu, more)
    st = dst.read_stats()
    assert int(st["dbg"]) == 0 and int(st["numPoints"]) == len(pts) and int(st["numPointsProcessed"]) == 200_000
    want, ho = _oracle_export(box, sr.a_input()[2] + more)
    sr.assert_no_overfull(want.nodes)
    nodes, pers, nn = host_image_of(dst)
    got = oracle.dump_image(nodes, nn)
    _assert_fields(got, ho.dump(), GRANULARITY_FREE_FIELDS, f"B {mode} (resume vs continuous)")
    oracle.check_invariants(nodes, nn)
    hs, hx = points_multiset_hash(pts)
    with np.errstate(over="ignore"):
        assert hs == np.uint64(got["pointsSum"].sum()) and hx == np.bitwise_xor.reduce(got["pointsXor"])
    re = dst.export_octree(uu)
    sr.assert_no_overfull(re.nodes)
    assert re.nodes.tobytes() == want.nodes.tobytes()


@pytest.mark.parametrize("mode", ["batch_by_batch", "one_group"])
def test_b_painted_import_keeps_its_colours_through_the_late_splits(built_libs, tmp_path, mode):
    """Rule E7 on the late splits of imported over-full leaves: the buildable import of A painted whole, then the 200 000 further points.  Colour
    never steers the build, so the resumed octree is the oracle's continuous build of the 600 000 points recoloured and the 200 000 as they are
    — every leaf's 16-byte records, every inner node's voxel positions —, and the root, which exists at paint time, keeps its painted voxels."""
    a = _state_a()
    pts, box, more = sr.b_input()
    a["full"].save(tmp_path / "a.simlodx")
    ld = OctreeExport.load(tmp_path / "a.simlodx")
    dst = _device()
    dst.tune("SIMLOD_EXACT_GROUP", 1 if mode == "batch_by_batch" else 2)
    uu = _import(dst, ld, a["u"])
    imported = dst.export_octree(uu)
    n0 = int(imported.nodes["numSamples"][0])
    assert len(sr.overfull_leaves(imported.nodes)) == 8 and n0 > 0 and not imported.nodes["flags"][0] & abi.EXPORT_FLAG_LEAF
    c = _paint_everything(dst, uu, pts)
    assert int(c["numSamples"]) == imported.num_samples and (dst.export_octree(uu).samples["color"] == PAINTED).all()
    (_feed_one_by_one if mode == "batch_by_batch" else _feed_one_group)(dst, uu, more)
    st = dst.read_stats()
    assert int(st["dbg"]) == 0 and int(st["numPoints"]) == len(pts) and int(st["numPointsProcessed"]) == 200_000
    early = _recoloured(pts[:600_000], 600_000)
    want, _ = _oracle_export(box, [early[i:i + 150_000] for i in range(0, 600_000, 150_000)] + more)
    re = dst.export_octree(uu)
    sr.assert_no_overfull(re.nodes)
    sr.assert_same_per_node(re, want, f"B {mode}, painted before the resume, against the oracle's build of the recoloured input")
    nodes, pers, nn = host_image_of(dst)
    oracle.check_invariants(nodes, nn)
    leaf = _leaf_mask(re)
    assert int((re.samples["color"][leaf] == PAINTED).sum()) == 600_000
    root = re.samples[: int(re.nodes["numSamples"][0])]
    assert int(re.nodes["firstSample"][0]) == 0 and int((root["color"] == PAINTED).sum()) >= n0, f"the root lost painted voxels: {int((root['color'] == PAINTED).sum())} of {n0}"


# ---- C. deferred splits by scarce scratch -----------------------------------------------------------------------------------------------------
C_POINTS, C_PENDING = 1_000_000, 4          # (found on the device: at 500 000 nothing spills)


def _device_c():
    """A device whose launches are told a momentary buffer of the minimum plus 6 MB (the buffer itself has the default size, so that the
    capacity can be raised later) -> (device, the small capacity)"""
    from simlod_amd.runtime import lib
    small = int(lib().simlod_construct_buffer_min_bytes()) + 6_000_000
    dev = _device(ring_slots=8)
    assert small < dev.momentary_bytes
    return dev, small


def test_c_deferred_splits_and_the_catch_up(built_libs):
    """C_POINTS is the smallest multiple of 500 000 slab points that leaves the device with SIMLOD_ERR_SPILLED_OVERFLOW and leaves whose split
    is pending beside leaves that did split (C_PENDING of them); one more batch under the full capacity lets every late split catch up."""
    pts, box, batches = sr.c_input(C_POINTS + 500_000)
    dev, small = _device_c()
    u = dev.uniforms(W, H, cases._cam(box), box)
    full_capacity = int(u["momentaryBufferCapacity"])
    u["momentaryBufferCapacity"] = small
    dev.reset(u)
    _feed(dev, u, batches[:-1])
    st = dev.read_stats()
    assert int(st["numPoints"]) == C_POINTS == int(st["numPointsProcessed"])
    before = dev.export_octree(u)
    assert sr.assert_state_c(st["dbg"], before.nodes) == C_PENDING
    _battery(State(dev, u, pts[:C_POINTS], box), True, "C deferred", sr.SHAPES["C"], erase="frames")
    # rule E7 across the catch-up: everything painted while the splits are pending — the next batch moves those leaves' points
    st = dev.read_stats()
    pending = dev.export_octree(u)
    assert sr.assert_state_c(st["dbg"], pending.nodes) == C_PENDING and pending.nodes.tobytes() == before.nodes.tobytes()
    c = _paint_everything(dev, u, pts)
    assert int(c["numSamples"]) == pending.num_samples
    painted = _recoloured(pts, C_POINTS)
    u["momentaryBufferCapacity"] = full_capacity
    _feed(dev, u, batches[-1:])
    st = dev.read_stats()
    assert int(st["numPoints"]) == len(pts) and int(st["dbg"]) & ~sr.ERR_SPILLED == 0
    after = _battery(State(dev, u, painted, box), True, "C caught up", sr.SHAPES["C"])
    sr.assert_no_overfull(after.nodes)
    nodes, pers, nn = host_image_of(dev)
    oracle.check_invariants(nodes, nn)
    leaf = _leaf_mask(after)
    smp = after.samples
    assert int(leaf.sum()) == len(pts) and int((smp["color"][leaf] == PAINTED).sum()) == C_POINTS
    assert np.array_equal(_positions(smp[leaf & (smp["color"] == PAINTED)]), _positions(pts[:C_POINTS])), "the painted leaf points are not the points ingested before the paint"
    # the leaves per node are the oracle's of the recoloured input (its inner nodes sample their voxels at other moments: not compared)
    want, _ = _oracle_export(box, [painted[i:i + 500_000] for i in range(0, len(painted), 500_000)])
    assert np.array_equal(sr.per_node(after, True), sr.per_node(want, True)), "C caught up: the leaves differ per node from the oracle's of the recoloured input"


# ---- D. coalesced mode as the source ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hotspot_150k", "dense_cube"])
def test_d_coalesced_source(built_libs, tmp_path, name):
    pts, box, batches, cut = sr.d_input(name)
    shape = sr.SHAPES[f"D {name}"]
    dev, u = _new(box, coalesce=True)
    _feed(dev, u, batches)
    assert int(dev.read_stats()["dbg"]) == 0
    full = _battery(State(dev, u, pts, box), True, f"D {name}", shape)
    want, _ = _oracle_export(box, batches)
    sr.assert_same_per_node(full, want, f"D {name} against the oracle")
    del dev
    src = _device(coalesce=True)
    _resume_batches(f"D {name}", box, batches, cut, tmp_path, src=src, check_import=name == "dense_cube")       # (the hotspot fills one level-3 cell: its frame stays under _check_import's floor)


# ---- E. a launch that stops short, and no host wait -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stop", ["batch_limit", "time_budget"])
def test_e_export_directly_behind_a_launch_that_stops_short(built_libs, stop):
    pts, box, batches = sr.e_input()
    dev, u = _new(box)
    if stop == "batch_limit":
        dev.set_batch_limit(2)
    else:
        dev.tune("SIMLOD_DEBUG_BUDGET_US", 100)
    for b in batches:
        dev.upload(b)
    # capacities from what the host knows without a look at Stats: the node array's size, and two samples per uploaded point
    nn, ns = dev.max_nodes, 2 * len(pts)
    need = int(dev.L.simlod_export_buffer_min_bytes(nn, ns))
    scratch, table = torch.empty(need, dtype=torch.uint8, device=dev.device), torch.empty(nn * 40, dtype=torch.uint8, device=dev.device)
    samples, counts = torch.empty(ns * 16, dtype=torch.uint8, device=dev.device), torch.zeros(abi.export_counts_dtype.itemsize, dtype=torch.uint8, device=dev.device)
    # ... and an inverse summary behind the export, of a region and in bins the host can state before it knows what the launch took: the
    # box's oblique half-space, the bins of test_gpu_inverse._bins
    region, (z0, scale) = rr.region("oblique", box), on_inverse._bins(box)
    sneed = int(dev.L.simlod_summary_buffer_min_bytes(nn, ns))
    sscratch, stable = on_inverse._mk(dev, sneed), on_inverse._mk(dev, (nn + on_inverse.SLACK) * 40)
    sout, scounts = on_inverse._mk(dev, on_summary.NBYTES + on_inverse.SLACK), on_inverse._mk(dev, abi.query_counts_dtype.itemsize)
    rrec, prec = region.record(), np.zeros(1, dtype=abi.summary_params_dtype)
    prec["z0"], prec["scale"] = z0, scale
    uu, up = dev._u(u)
    torch.cuda.synchronize()
    dev.construct(u)                                                     # ... and, with nothing in between on the host, the export behind it
    rc = dev.L.simlod_export_octree(dev._p(dev.nodes), dev._p(dev.stats), abi.MAX_DEPTH, abi.EXPORT_ALL, dev._p(scratch), ctypes.c_uint64(need), dev._p(table), nn,
                                    dev._p(samples), ctypes.c_uint64(ns), dev._p(counts), dev._stream())
    src = dev.L.simlod_query_summary_inverse(dev._p(dev.nodes), dev._p(dev.stats), up, on_inverse._ptr(rrec), None, None, on_inverse._ptr(prec), abi.MAX_DEPTH,
                                             abi.EXPORT_ALL, dev._p(sscratch), ctypes.c_uint64(sneed), dev._p(stable), nn, dev._p(sout), dev._p(scounts), dev._stream())
    torch.cuda.synchronize()
    assert rc == 0 and src == 0
    c = counts.cpu().numpy().view(abi.export_counts_dtype)[0]
    st = dev.read_stats()
    b = int(st["batchletIndex"])
    assert (b == 2) if stop == "batch_limit" else (1 <= b < 6), f"{b} batches taken"
    sr.assert_stopped_short(st, b, len(batches) - b)
    assert int(c["error"]) == 0, f"export error bits {int(c['error']):#x}"
    ex = OctreeExport(table[: int(c["numNodes"]) * 40], samples[: int(c["numSamples"]) * 16], u["boxMin"], u["boxMax"])
    nodes, pers, n = host_image_of(dev)
    _assert_export(ex, *export_host(nodes, n), f"E {stop}: the export behind the launch")
    want, wc = ex.to("cpu").summarize(region, 20, "all", z0=z0, scale=scale, return_counts=True, invert=True)
    sc = scounts.cpu().numpy()[:32].view(abi.query_counts_dtype)[0]
    assert int(sc["error"]) == 0 and _count_fields(sc) == _count_fields(wc), f"E {stop}: the inverse summary behind the launch counts {sc}, the mirror of the export {wc}"
    assert 0 < int(wc["numSamples"]) < ex.num_samples and int(wc["numNodes"]) == ex.num_nodes
    assert sout[: on_summary.NBYTES].cpu().numpy().tobytes() == want.tobytes(), f"E {stop}: the inverse summary behind the launch is not the mirror's of the export behind it"
    assert stable[: ex.num_nodes * 40].cpu().numpy().tobytes() == ex.to("cpu").crop(region, 20, "all", invert=True).nodes.tobytes(), f"E {stop}: the inverse summary's table"
    assert bool((stable[ex.num_nodes * 40:] == 0xA5).all()) and bool((sout[on_summary.NBYTES:] == 0xA5).all()), f"E {stop}: the inverse summary wrote past its table or its record"
    want, _ = _oracle_export(box, batches[:b])
    sr.assert_same_per_node(ex, want, f"E {stop} against the oracle's octree of {b} batches")
    _battery(State(dev, u, np.concatenate(batches[:b]), box), True, f"E {stop}", sr.SHAPES.get(f"E{b}", sr.SHAPES["E"]))
    if stop != "batch_limit":
        return
    # rule E7 across a resumed launch sequence: paint with four batches pending in the ring, lift the limit, and the next launch directly
    # behind the paint — the host waits for nothing but what paint_region itself waits for
    sr.assert_stopped_short(dev.read_stats(), 2, 4)
    torch.cuda.synchronize()
    c = _paint_everything(dev, u, pts)
    dev.set_batch_limit(abi.MAX_BATCHES_PER_LAUNCH)
    dev.construct(u)
    dev.drain(u)
    st = dev.read_stats()
    assert int(st["dbg"]) == 0 and int(st["batchletIndex"]) == len(batches) and int(st["numPoints"]) == len(pts)
    assert int(c["numSamples"]) == ex.num_samples
    want, _ = _oracle_export(box, [_recoloured(bt, len(bt)) for bt in batches[:2]] + batches[2:])
    final = dev.export_octree(u)
    sr.assert_same_per_node(final, want, "E batch_limit, painted at two batches and drained, against the oracle's build of the recoloured input")
    assert int((final.samples["color"][_leaf_mask(final)] == PAINTED).sum()) == 200_000


# ---- F. memory guard tripped ------------------------------------------------------------------------------------------------------------------
def test_f_memory_guard_tripped(built_libs):
    pts, box, batches = sr.f_input()
    cap, _ = sr.f_capacity(box, batches)
    want, ho = _oracle_export(box, batches, capacity=cap)
    taken = int(ho.stats["batchletIndex"][0])
    dev = _device(ring_slots=8, persistent_bytes=cap + 4096)
    dev.persistent[cap:].fill_(0x3C)
    u = dev.uniforms(W, H, cases._cam(box), box)
    u["persistentBufferCapacity"] = cap
    dev.persistent_bytes = cap
    dev.reset(u)
    for b in batches:
        dev.upload(b)
    for _ in range(4):
        dev.construct(u)
    st = dev.read_stats()
    assert int(ho.stats["memCapacityReached"][0]) == 1 and 0 < taken < 4
    sr.assert_stopped_short(st, taken, len(batches) - taken, guard=True)
    full = _battery(State(dev, u, np.concatenate(batches[:taken]), box), True, "F", sr.SHAPES["F"], between=lambda: dev.construct(u))
    sr.assert_same_per_node(full, want, "F against the oracle's octree at the guard")
    st = dev.read_stats()
    sr.assert_stopped_short(st, taken, len(batches) - taken, guard=True)
    assert bool((dev.persistent[cap:] == 0x3C).all())


# ---- G. a foreign image, continued ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total,first,batch", sr.G_CASES)
def test_g_foreign_image_continued(built_libs, total, first, batch):
    pts, box = synthetic.terrain(total, seed=7)
    dev, u = _new(box, ring_slots=8)
    _feed(dev, u, [pts[i:i + batch] for i in range(0, first, batch)])
    nodes, pers, nn, nodes_base, pers_base = dev.download_image()
    st = dev.read_stats()
    heads = np.concatenate([nodes["points"][:nn], nodes["voxelChunks"][:nn]]).astype(np.uint64)
    heads = heads[heads != 0]
    assert (len(heads) > 20 and nodes["voxelChunks"][0] != 0 and nodes["points"][0] == 0) if total > 100_000 else (nn == 1 and len(heads) == 2)     # an inner root / a root that is a leaf
    # the image as another implementation leaves it (test_ingest_continues_into_an_image_this_library_did_not_build): the spare words of the lists'
    # head chunks poisoned, nothing in the momentary buffer but the recycle stack — and uploaded, so that nothing trusts the old stamp
    for h in heads:
        off = int(h - np.uint64(pers_base)) + 16000
        pers[off: off + 8] = 0xA5
    dev.momentary[4096 + 8_000_000:].fill_(0xA5)
    dev.upload_image(nodes, pers, nn, stats=st)
    small = total < 100_000
    _battery(State(dev, u, pts[:first], box), False, f"G {total} poisoned", sr.SHAPES[f"G {total} poisoned"], erase="no frames" if small else None)
    assert dev.uploaded_host == dev.processed_host == first // batch
    for i in range(first, total, batch):
        dev.upload(pts[i:i + batch])
        if small:
            dev.drain(u)
    dev.drain(u)
    ds = dev.read_stats()
    assert int(ds["dbg"]) == 0 and int(ds["numPoints"]) == total
    full = _battery(State(dev, u, pts, box), True, f"G {total} continued", sr.SHAPES[f"G {total} continued"])
    want, _ = _oracle_export(box, [pts[i:i + batch] for i in range(0, total, batch)])
    sr.assert_same_per_node(full, want, f"G {total} continued against the oracle")


# ---- H. a rank's octree under a trunk mask ----------------------------------------------------------------------------------------------------
def test_h_rank_octree_under_a_trunk_mask(built_libs):
    pts, box, mask, mine, batches = sr.h_input(_partition)
    dev, u = _new(box, ring_slots=8)
    dev.set_trunk_mask(*mask)
    _feed(dev, u, batches)
    assert int(dev.read_stats()["dbg"]) == 0
    want, _ = _oracle_export(box, batches, mask=mask)
    sr.assert_masked_rank(want.nodes, pts, mine, box, mask)
    # a node the mask forces is EMPTY before any query, and every inverse lists it at zero samples: the classes of rule I2 see a node without samples
    forced_empty = lambda full, M: print(f"H: {sr.assert_forced_empty_listed(full, M['inverse'], pts, mine, box)} nodes the mask forces are empty")
    full = _battery(State(dev, u, mine, box), True, "H", sr.SHAPES["H"], erase="frames", check=forced_empty)
    sr.assert_masked_rank(full.nodes, pts, mine, box, mask)
    sr.assert_same_per_node(full, want, "H against the oracle with the same mask")


# ---- I. two octrees in one context, and a rebuild in the same buffers --------------------------------------------------------------------------
def test_i_two_octrees_in_one_context_and_a_rebuild(built_libs):
    pa, box_a, batch_a, Ta = cases.case("terrain_4x100k")
    pb, box_b, batch_b, Tb = cases.case("uniform_3x40k")
    ba, bb = cases.batches_of("terrain_4x100k", pa, batch_a), cases.batches_of("uniform_3x40k", pb, batch_b)
    A, B = _device(persistent_bytes=1 << 30, ring_slots=8), _device(persistent_bytes=1 << 30, ring_slots=8)
    try:
        assert A.L.simlod_context_attach(A.ctx, B._p(B.nodes)) == 0      # both node arrays in A's context
        A.tune("SIMLOD_EXACT_GROUP", 1)
        ua, ub = A.uniforms(W, H, Ta, box_a), B.uniforms(W, H, Tb, box_b)

        def ingest(dev, u, batches, done):
            for k, b in enumerate(batches):
                dev.upload(b)
                dev.construct(u)
                assert dev.processed() == done + k + 1

        A.reset(ua)
        ingest(A, ua, ba[:2], 0)
        assert A.L.simlod_octree_image_replaced(A._p(A.nodes)) == 0
        B.reset(ub)
        ingest(B, ub, bb[:1], 0)
        ingest(A, ua, ba[2:], 2)
        ingest(B, ub, bb[1:], 1)
        assert int(A.read_stats()["dbg"]) == 0 and int(B.read_stats()["dbg"]) == 0
        # the stamps first, while both tables stand: the battery of A drops A's alone
        for dev, u in ((A, ua), (B, ub)):
            u1 = np.array(u, copy=True)
            u1["minNodeSize"] = 1.0
            dev.render(u1)
            assert dev.lists_read_through_table() > 0
        # each battery paints its octree (and undoes it): the OTHER octree of the context — Node array, Stats, every allocated byte — stays
        other = on_paint._image(B)
        fa = _battery(State(A, ua, pa, box_a), True, "I A", sr.SHAPES["I A"], erase="frames")
        assert on_paint._image(B) == other, "I: the battery of A, its paint calls among it, changed B"
        other = on_paint._image(A)
        fb = _battery(State(B, ub, pb, box_b), True, "I B", sr.SHAPES["I B"])
        assert on_paint._image(A) == other, "I: the battery of B, its paint calls among it, changed A"
        # ... and not only after the undo: one octree painted whole, the other looked at WHILE the paint stands
        for dev, u, pts, oth, full in ((A, ua, pa, B, fa), (B, ub, pb, A, fb)):
            other, own = on_paint._image(oth), on_paint._image(dev)
            c, prev = dev.paint_region(u, Region(), Paint.set(PAINTED), return_previous=True)
            assert not (pts["color"] == PAINTED).any() and int(c["numSamples"]) == full.num_samples
            assert (dev.export_octree(u).samples["color"] == PAINTED).all() and on_paint._image(oth) == other, "I: painting one octree changed the other"
            dev.paint_region(u, Region(), Paint.array(), colors=prev)
            assert on_paint._image(dev) == own
        assert fa.num_nodes > fb.num_nodes
        # the smaller octree into A's buffers: the rows of the larger one lie behind it
        A.reset(ua := A.uniforms(W, H, Tb, box_b))
        ingest(A, ua, bb, 0)
        assert int(A.read_stats()["dbg"]) == 0
        again = _battery(State(A, ua, pb, box_b), True, "I A rebuilt", sr.SHAPES["I B"])
        assert again.nodes.tobytes() == fb.nodes.tobytes()
    finally:
        A.L.simlod_context_attach(B.ctx, B._p(B.nodes))                  # back to its own context: each close() then destroys its own
        B.close()
        A.close()
