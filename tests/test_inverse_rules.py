"""CPU tier of the inverse selections (include/simlod_hip.h, "inverse selections"): the host mirrors OctreeExport.crop / paint /
summarize(invert=True) against rule I1 said once more per sample (tests/inverse_ref.py), rules I3, I6, I7 and I10 on octrees built by the
oracle's port, and simlod_amd/csrc/inverse_rules.hpp on the host by a program of its own (tests/host/inverse_rules_check.cpp, built with the
address and undefined-behaviour sanitizers) against the numpy class map."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import clip_ref
import footprint_ref as fr
import inverse_ref as ir
import lasso_ref as lr
import paint_ref as pf
import region_ref as rr
import summary_ref as sr
from simlod_amd import abi
from simlod_amd.octree_io import Clip, Paint, Profile, Region, classify_nodes
from util import node_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_FIELDS = list(abi.query_counts_dtype.names)
SHAPE_FIELDS = [f for f in abi.export_node_dtype.names if f not in ("numSamples", "firstSample")]
_BUILT = {}


def _case(name):
    """-> (full export, points, box, HostOctree), built once per module."""
    if name not in _BUILT:
        _BUILT[name] = rr.host_octree(name)
    return _BUILT[name]


def _all_selections(name, box):
    for family in ir.FAMILIES:
        for kind in ir.names_for(family, name):
            yield family, kind, ir.selection(family, kind, box)


def test_inverse_symbols_exported(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_inverse_buffer_min_bytes", "simlod_query_inverse", "simlod_paint_inverse", "simlod_query_summary_inverse"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    for nn, bound in ((0, 0), (100, 0), (7000, 5_000_000)):
        assert L.simlod_inverse_buffer_min_bytes(nn, bound) == L.simlod_footprint_buffer_min_bytes(nn, bound)
    for m in ("erase_region",):
        assert hasattr(runtime.DeviceOctree, m)
    # rule I9 precedes device work: hipErrorInvalidValue (1) without a GPU
    assert L.simlod_query_inverse(*([None] * 6), 20, 0, None, 0, None, 0, None, 0, None, None) == 1
    assert L.simlod_paint_inverse(*([None] * 8), 0, None, 0, None, None, 0, None, None) == 1
    assert L.simlod_query_summary_inverse(*([None] * 7), 20, 0, None, 0, None, 0, None, None, None) == 1


@pytest.mark.parametrize("name", cases.CASES)
def test_mirror_equals_the_per_sample_rule(name):
    """Per case x selection x MODES: the mirror's samples are, node by node, those the per-sample restatement of rule I1 picks (no node
    shortcut); the table is the export's in every field but numSamples and firstSample (I3); the counts are rule I4's; the positive and the
    inverse indices partition the selected nodes' samples (I6)."""
    full, pts, box, ho = _case(name)
    for family, kind, (region, fp, lasso) in _all_selections(name, box):
        mask = ir.passes_inverse(region, fp, lasso, full.samples)
        outside, inside = _classes(full, region, fp, lasso)
        cls = ir.class_map(outside, inside)
        for sel, ml in ir.MODES:
            what = f"{name} {family} {kind} {sel}@{ml}"
            inv, cnt, idx = full.crop(region, ml, sel, return_counts=True, footprint=fp, lasso=lasso, invert=True, return_index=True)
            inv.validate()
            assert inv.select == abi.EXPORT_REGION and inv.max_level == ml
            want = ir.inverse_per_node(full, mask, ml, sel)
            assert inv.num_nodes == len(want), what
            for t, w in enumerate(want):
                a = int(inv.nodes["firstSample"][t])
                got = inv.samples[a: a + int(inv.nodes["numSamples"][t])]
                assert got.tobytes() == w.tobytes(), f"{what}: node {t} holds {len(got)} samples, the per-sample rule {len(w)}"
            # I3
            export = full.crop(Region(), ml, sel)
            assert export.nodes.tobytes() == full.truncated(ml, sel).nodes.tobytes()
            for f in SHAPE_FIELDS:
                assert np.array_equal(inv.nodes[f], export.nodes[f]), f"{what}: {f} is not the export's"
            # I4
            ranges = ir.selected_ranges(full, ml, sel)
            size = np.array([b - a for a, b in ranges], np.int64)
            c = cls[: len(ranges)]
            assert int(cnt["numNodes"]) == len(ranges) and int(cnt["error"]) == 0 and int(cnt["numSamples"]) == inv.num_samples == sum(len(w) for w in want), what
            assert int(cnt["numCandidates"]) == int(size[c != ir.EMPTIED].sum()), what
            assert int(cnt["numCopiedNodes"]) == int(((c == ir.COPIED) & (size > 0)).sum()) and int(cnt["numFilteredNodes"]) == int(((c == ir.FILTERED) & (size > 0)).sum()), what
            assert (inv.nodes["numSamples"][c == ir.EMPTIED] == 0).all(), what
            # I6
            pos_idx = full.crop(region, ml, sel, footprint=fp, lasso=lasso, return_index=True)[1]
            assert len(np.intersect1d(pos_idx, idx)) == 0, what
            assert (np.diff(idx) > 0).all() and (np.diff(pos_idx) > 0).all(), what
            every = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in ranges]) if ranges else np.zeros(0, np.int64)
            assert np.array_equal(np.sort(np.concatenate([pos_idx, idx])), every), f"{what}: positive and inverse do not partition the selected nodes' samples"


def _classes(full, region, fp, lasso):
    """The positive query's final (outside, copied) per node of the full export, combined as rules F4 / L4 combine them."""
    from simlod_amd.octree_io import classify_footprint, classify_lasso
    outside, inside = classify_nodes(np.asarray(region.planes, np.float32).astype(np.float64), full.nodes, full.box_min, full.box_max)
    if fp is not None:
        near, corner = classify_footprint(fp, full.nodes, full.box_min, full.box_max)
        outside, inside = outside | (~near & ~corner), inside & ~near & corner
    if lasso is not None:
        behind, covered = classify_lasso(lasso, full.nodes, full.box_min, full.box_max)
        outside, inside = outside | behind, inside & covered
    return outside, inside


@pytest.mark.parametrize("family,name,kind", ir.ALL_CLASSES)
def test_the_battery_produces_emptied_nodes(family, name, kind):
    """A condition, not a measurement: each selector family holds a selection for which the POSITIVE mirror reports filtered nodes, copied nodes
    (the inverse's EMPTIED ones) and fewer listed nodes than the export (the inverse's COPIED ones)."""
    full, pts, box, ho = _case(name)
    assert kind in ir.names_for(family, name)
    region, fp, lasso = ir.selection(family, kind, box)
    pos, cnt = full.crop(region, 20, "all", return_counts=True, footprint=fp, lasso=lasso)
    print(family, name, kind, {k: int(cnt[k]) for k in COUNT_FIELDS}, "of", full.num_nodes, "nodes")
    assert int(cnt["numFilteredNodes"]) > 0 and int(cnt["numCopiedNodes"]) > 0 and int(cnt["numNodes"]) < full.num_nodes
    inv, icnt = full.crop(region, 20, "all", return_counts=True, footprint=fp, lasso=lasso, invert=True)
    # (the nodes the positive query leaves out may be empty ones: the inverse's copied count is not part of the condition)
    assert int(icnt["numFilteredNodes"]) == int(cnt["numFilteredNodes"]) and int(icnt["numNodes"]) == full.num_nodes
    assert (inv.nodes["numSamples"] == 0).sum() >= int(cnt["numCopiedNodes"])
    assert int(icnt["numSamples"]) + int(cnt["numSamples"]) == full.num_samples


@pytest.mark.parametrize("name", cases.CASES)
def test_degenerate_selections(name):
    """I7: zero planes and no polygon empty every node; a selection that selects nothing gives the export, byte for byte."""
    full, pts, box, ho = _case(name)
    for sel, ml in ir.MODES:
        export = full.truncated(ml, sel)
        inv, cnt = full.crop(Region(), ml, sel, return_counts=True, invert=True)
        assert inv.num_samples == 0 and not inv.nodes["numSamples"].any() and not inv.nodes["firstSample"].any()
        assert [int(cnt[k]) for k in COUNT_FIELDS] == [export.num_nodes, 0, 0, 0, 0, 0]
        for f in SHAPE_FIELDS:
            assert np.array_equal(inv.nodes[f], export.nodes[f]), f
        for family in ir.FAMILIES:
            region, fp, lasso = ir.selection(family, "miss", box)
            inv, cnt = full.crop(region, ml, sel, return_counts=True, footprint=fp, lasso=lasso, invert=True)
            assert inv.nodes.tobytes() == export.nodes.tobytes() and inv.samples.tobytes() == export.samples.tobytes(), (name, family, sel, ml)
            assert int(cnt["numSamples"]) == int(cnt["numCandidates"]) == export.num_samples and int(cnt["numFilteredNodes"]) == 0


def test_invert_refuses_a_profile_and_keeps_return_index():
    full, pts, box, ho = _case("ragged_tiny")
    p = Profile([(0.1 * box[0], 0.1 * box[1]), (0.9 * box[0], 0.8 * box[1])], 0.1 * box[0])
    with pytest.raises(ValueError):
        full.crop(Region(), 20, "all", profile=p, invert=True)
    region = rr.region("oblique", box)
    inv, idx = full.crop(region, 20, "all", invert=True, return_index=True)
    assert inv.samples.tobytes() == full.samples[idx].tobytes() and len(idx) == inv.num_samples > 0
    # invert=False is the call it was
    a, b = full.crop(region, 20, "cut"), full.crop(region, 20, "cut", invert=False)
    assert a.nodes.tobytes() == b.nodes.tobytes() and a.samples.tobytes() == b.samples.tobytes()


@pytest.mark.parametrize("name", ["terrain_4x100k", "hotspot_150k"])
def test_planes_inverse_keeps_what_clip_outside_keeps(name):
    """I10: for the plane regions the inverse at ALL@20 holds, node by node (matched by level and X, Y, Z), the samples the SIMLOD_CLIP_OUTSIDE
    edit of rule C3 keeps — of the list the export carries: a leaf's points, an inner node's voxels — in order."""
    full, pts, box, ho = _case(name)
    nn, used = int(ho.stats["numNodes"][0]), int(ho.stats["allocatedBytes_persistent"][0])
    u = cases.uniforms_for(box, cases.case(name)[3])
    for kind in rr.REGION_NAMES:
        region = rr.region(kind, box)
        img = clip_ref.clip_image(ho.nodes, ho.persistent, nn, Clip(region, "outside"), u, used)
        inv = full.crop(region, 20, "all", invert=True)
        where = {int(k): i for i, k in enumerate(node_keys(img.nodes[:nn]))}
        assert len(where) == nn == inv.num_nodes
        compared = 0
        for t, key in enumerate(node_keys(inv.nodes)):
            i = where[int(key)]
            leaf = (int(inv.nodes["flags"][t]) & abi.EXPORT_FLAG_LEAF) != 0
            head, count = clip_ref.LISTS[0 if leaf else 1]
            parts = [v[np.isfinite(v["x"])] for v in clip_ref.chunk_views(img.pers, img.nodes[head][i], img.nodes[count][i])]
            kept = np.concatenate(parts) if parts else np.zeros(0, dtype=abi.point_dtype)
            a = int(inv.nodes["firstSample"][t])
            got = inv.samples[a: a + int(inv.nodes["numSamples"][t])]
            assert got.tobytes() == kept.tobytes(), f"{name} {kind}: node {t} holds {len(got)} samples, the clip keeps {len(kept)}"
            compared += len(kept)
        assert compared == inv.num_samples
        if kind in ("oblique", "box"):
            assert 0 < compared < full.num_samples and bool(img.tested), (name, kind)
    # (the oblique region on the terrain and the box on the hotspot empty whole nodes: test_the_battery_produces_emptied_nodes)


@pytest.mark.parametrize("name,family,kind", [("hotspot_150k", "planes", "box"), ("hotspot_150k", "footprint", "rect"), ("ragged_tiny", "lasso", "half"),
                                              ("ragged_tiny", "planes", "oblique")])
def test_paint_and_summary_mirrors_on_the_inverse_set(name, family, kind):
    """I8: paint(invert=True) against paint_ref on the per-sample rule's set, mode by mode, `previous` and its ARRAY paint restoring the bytes;
    summarize(invert=True) against summary_ref on that set."""
    full, pts, box, ho = _case(name)
    region, fp, lasso = ir.selection(family, kind, box)
    mask = ir.passes_inverse(region, fp, lasso, full.samples)
    idx = np.nonzero(mask)[0]                          # (ALL@20: every node is selected, the export's order is the query's)
    assert 0 < len(idx) < full.num_samples
    rs = np.random.RandomState(11)
    for mode, paint in pf.paints(box).items():
        colors = rs.randint(0, 1 << 32, len(idx) + 3, dtype=np.uint64).astype(np.uint32) if mode == "array" else None
        got, cnt, prev = full.paint(region, paint, footprint=fp, lasso=lasso, colors=colors, return_previous=True, invert=True)
        want_col, want_prev = pf.paint(full.samples, idx.tolist(), paint.record(), None if colors is None else colors.tolist())
        assert int(cnt["numSamples"]) == len(idx) and np.array_equal(prev, np.asarray(want_prev, np.uint32)), (name, kind, mode)
        assert np.array_equal(got.samples["color"], want_col), (name, kind, mode)
        assert got.nodes.tobytes() == full.nodes.tobytes() and all(np.array_equal(got.samples[a], full.samples[a]) for a in "xyz")
        back, _ = got.paint(region, Paint.array(), footprint=fp, lasso=lasso, colors=prev, invert=True)
        assert back.samples.tobytes() == full.samples.tobytes(), f"{name} {kind} {mode}: undo"
    mn = np.asarray(full.box_min, np.float32)
    size = (np.asarray(full.box_max, np.float32) - mn).max()
    z0, scale = np.float32(0.1 * box[2]), np.float32(256.0 / (0.7 * box[2]))
    for sel, ml in ir.MODES:
        got, cnt = full.summarize(region, ml, sel, footprint=fp, lasso=lasso, z0=z0, scale=scale, return_counts=True, invert=True)
        smp = np.concatenate(ir.inverse_per_node(full, mask, ml, sel))
        want = sr.summarize_exact(smp, mn, size, z0, scale)
        assert got.tobytes() == want.tobytes() and int(cnt["numSamples"]) == len(smp), (name, kind, sel, ml)
        pos = full.summarize(region, ml, sel, footprint=fp, lasso=lasso, z0=z0, scale=scale)
        whole = full.summarize(Region(), ml, sel, z0=z0, scale=scale)
        assert got.num_samples + pos.num_samples == whole.num_samples
        assert np.array_equal(got["histC"] + pos["histC"], whole["histC"]) and np.array_equal(got["histZ"] + pos["histZ"], whole["histZ"])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("inverse_rules") / "inverse_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "inverse_rules_check.cpp"), "-o", exe])
    return exe


def test_header_maps_classes_as_the_mirror_does(checker, tmp_path):
    """The positive classes of a fixture table — terrain_4x100k's nodes against the oblique region, the box and the half-screen lasso — through
    inverse_rules.hpp on the host: the class map is the numpy one; rule I1 negates; a footprint and a lasso together are refused."""
    full, pts, box, ho = _case("terrain_4x100k")
    positive, want = [], []
    for family, kind in (("planes", "oblique"), ("planes", "box"), ("lasso", "half"), ("footprint", "rect")):
        outside, inside = _classes(full, *ir.selection(family, kind, box))
        assert not (outside & inside).any()
        positive.append(np.where(outside, ir.OUTSIDE, np.where(inside, ir.COPIED, ir.FILTERED)))
        want.append(ir.class_map(outside, inside))
    positive, want = np.concatenate(positive).astype("<u4"), np.concatenate(want).astype(np.uint8)
    assert set(positive.tolist()) == {0, 1, 2} and set(want.tolist()) == {ir.FILTERED, ir.COPIED, ir.EMPTIED}
    with open(tmp_path / "classes.bin", "wb") as f:
        f.write(np.array([len(positive)], "<u4").tobytes() + positive.tobytes())
    run = subprocess.run([checker, str(tmp_path / "classes.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8)
    assert len(got) == len(want) + 6
    assert np.array_equal(got[: len(want)], want), f"{int((got[: len(want)] != want).sum())} classes differ"
    assert got[len(want):].tolist() == [1, 0, 1, 1, 1, 0]
