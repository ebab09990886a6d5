"""CPU tier: paint regions (include/simlod_hip.h, "paint regions") — the ABI struct, octree_io.Paint, and the host mirror OctreeExport.paint
against tests/paint_ref.py (every rule one sample at a time, no node classified) on octrees built by the oracle's port: every mode, every
region of region_ref, with and without a footprint; undo; and that nothing but colours moves."""
import os
import re

import numpy as np
import pytest

import cases
import footprint_ref as fr
import paint_ref as pf
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Paint, Region

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["set", "blend", "ramp", "array"]
# (region kind, footprint kind or None): every region without a footprint; a non-convex and a convex footprint alone and with planes
COMBOS = [(k, None) for k in rr.REGION_NAMES] + [("none", "star7"), ("slab", "star7"), ("none", "oblique")]


def test_paint_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodPaint\) == (\d+)", src).group(1)) == abi.paint_dtype.itemsize == 1056
    offs = dict(re.findall(r"offsetof\(SimlodPaint, (\w+)\) == (\d+)", src))
    assert sorted(offs) == ["color", "scale", "strength", "table", "z0"]
    for f, o in offs.items():
        assert abi.paint_dtype.fields[f][1] == int(o), f
    assert abi.paint_dtype.fields["mode"][1] == 0 and abi.paint_dtype.fields["reserved"][1] == 12 and abi.paint_dtype.fields["reserved2"][1] == 24
    for name, value in (("SET", abi.PAINT_SET), ("BLEND", abi.PAINT_BLEND), ("RAMP", abi.PAINT_RAMP), ("ARRAY", abi.PAINT_ARRAY)):
        assert int(re.search(rf"#define SIMLOD_PAINT_{name}\s+(\d+)u", src).group(1)) == value
    r = Paint.ramp(1.0, 3.0, np.arange(256) * 3).record()
    assert r.dtype == abi.paint_dtype and int(r["mode"][0]) == abi.PAINT_RAMP and float(r["z0"][0]) == 1.0 and float(r["scale"][0]) == 128.0
    assert r["table"][0].tolist() == (np.arange(256) * 3).tolist() and not r["reserved"].any() and not r["reserved2"].any()
    r = Paint.blend(0x11223344, 9).record()
    assert (int(r["mode"][0]), int(r["color"][0]), int(r["strength"][0])) == (abi.PAINT_BLEND, 0x11223344, 9) and not r["table"].any()
    assert int(Paint.set(5).record()["color"][0]) == 5 and int(Paint.array().record()["mode"][0]) == abi.PAINT_ARRAY


def test_paint_symbols_exported(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_paint_buffer_min_bytes", "simlod_paint_region"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    # the footprint query's bytes plus a fixed block for the ramp's table
    block = L.simlod_paint_buffer_min_bytes(100, 0) - L.simlod_footprint_buffer_min_bytes(100, 0)
    assert block >= 256 * 4
    assert L.simlod_paint_buffer_min_bytes(7000, 5_000_000) - L.simlod_footprint_buffer_min_bytes(7000, 5_000_000) == block


@pytest.fixture(scope="module", params=cases.CASES)
def built(request):
    """-> (name, full export, box, {combo: (region, footprint, the reference's target indices)})"""
    name = request.param
    ex, pts, box, ho = rr.host_octree(name)
    assert pf.in_contract(ex.samples, ex.box_min, ex.box_max), name
    sets = {}
    for rk, fk in COMBOS:
        r, f = rr.region(rk, box), None if fk is None else fr.footprint(fk, box)
        sets[rk, fk] = (r, f, pf.targets(ex.samples, r.planes, f))
    return name, ex, box, sets


def test_mirror_paints_what_the_reference_paints(built):
    """Every mode x every combination: the mirror's colour column, its previous colours and its counts equal the reference's, and nothing
    but the colour column differs from the source."""
    name, ex, box, sets = built
    rs = np.random.RandomState(3)
    painted = 0
    for (rk, fk), (r, f, idx) in sets.items():
        if rk == "miss":
            assert idx == []
        elif rk == "none" and fk is None:
            assert idx == list(range(ex.num_samples))
        else:
            assert 0 < len(idx) < ex.num_samples or "hotspot" in name, (name, rk, fk)
        crop, cc = ex.crop(r, 20, "all", return_counts=True, footprint=f)
        for mode in MODES:
            p = pf.paints(box)[mode]
            colors = rs.randint(0, 1 << 32, len(idx) + 3, dtype=np.uint64).astype(np.uint32) if mode == "array" else None
            got, cnt, prev = ex.paint(r, p, footprint=f, colors=colors, return_previous=True)
            want, wprev = pf.paint(ex.samples, idx, p.record(), None if colors is None else colors.tolist())
            what = f"{name} {rk} {fk} {mode}"
            assert int(cnt["numSamples"]) == len(idx) == len(prev) and cnt.tobytes() == cc.tobytes(), what
            assert prev.dtype == np.uint32 and prev.tolist() == wprev, what
            assert np.array_equal(got.samples["color"], want), f"{what}: {int((got.samples['color'] != want).sum())} colours differ"
            assert got.nodes.tobytes() == ex.nodes.tobytes() and (got.select, got.max_level, got.box_min, got.box_max) == (ex.select, ex.max_level, ex.box_min, ex.box_max)
            for a in ("x", "y", "z"):
                assert got.samples[a].tobytes() == ex.samples[a].tobytes(), what
            changed = np.nonzero(got.samples["color"] != ex.samples["color"])[0]
            assert set(changed.tolist()) <= set(idx), what
            painted += len(changed)
            if mode == "ramp":
                # the painted samples, read back by the query, are the crop's samples with the new colours
                back = got.crop(r, 20, "all", footprint=f)
                assert back.nodes.tobytes() == crop.nodes.tobytes() and np.array_equal(back.samples["color"], want[np.asarray(idx, np.int64)]), what
    assert painted > 0
    # the source was not touched
    assert ex.paint(Region(), Paint.set(1))[0].samples_tensor.data_ptr() != ex.samples_tensor.data_ptr()
    assert not (ex.samples["color"] == 1).all()


def test_undo_restores_every_byte(built):
    name, ex, box, sets = built
    for (rk, fk), (r, f, idx) in sets.items():
        for mode in ("set", "blend", "ramp"):
            a, cnt, prev = ex.paint(r, pf.paints(box)[mode], footprint=f, return_previous=True)
            b, cnt2, prev2 = a.paint(r, Paint.array(), footprint=f, colors=prev, return_previous=True)
            assert b.samples.tobytes() == ex.samples.tobytes() and b.nodes.tobytes() == ex.nodes.tobytes(), (name, rk, fk, mode)
            assert cnt2.tobytes() == cnt.tobytes()
            assert np.array_equal(prev2, a.samples["color"][np.asarray(idx, np.int64)])
    with pytest.raises(ValueError):
        ex.paint(Region(), Paint.array())
    with pytest.raises(ValueError):
        ex.paint(Region(), Paint.array(), colors=np.zeros(max(ex.num_samples - 1, 0), np.uint32))


def test_paint_needs_a_full_export(built):
    name, ex, box, sets = built
    with pytest.raises(ValueError):
        ex.truncated(1, "cut").paint(Region(), Paint.set(0))
