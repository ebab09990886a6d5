"""CPU tier: profile queries (include/simlod_hip.h, "profile queries") — the ABI structs, octree_io.Profile, classify_profile and the host mirror
OctreeExport.profile on octrees built by the oracle's port, against profile_ref.locate_exact (rule P1 with every comparison decided exactly) on
every sample of every selected node."""
import os
import re

import numpy as np
import pytest

import cases
import profile_ref as pr
import region_ref as rr
from simlod_amd import abi
from simlod_amd.octree_io import Profile, Region, classify_profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("cut", 20), ("all", 20), ("cut", 2)]


def test_profile_structs_match_header():
    src = open(os.path.join(ROOT, "include", "simlod_hip.h")).read()
    assert int(re.search(r"sizeof\(SimlodProfile\) == (\d+)", src).group(1)) == abi.profile_dtype.itemsize == 576
    assert int(re.search(r"sizeof\(SimlodProfileSample\) == (\d+)", src).group(1)) == abi.profile_sample_dtype.itemsize == 16
    offs = dict(re.findall(r"offsetof\(SimlodProfile, (\w+)\) == (\d+)", src))
    assert sorted(offs) == ["axisH", "axisU", "axisV", "halfWidth", "vertices"]
    for f, o in offs.items():
        assert abi.profile_dtype.fields[f][1] == int(o), f
    assert abi.profile_dtype.fields["numVertices"][1] == 0 and abi.profile_dtype.fields["reserved"][1] == 8
    offs = dict(re.findall(r"offsetof\(SimlodProfileSample, (\w+)\) == (\d+)", src))
    assert sorted(offs) == ["height", "segment"]
    for f, o in offs.items():
        assert abi.profile_sample_dtype.fields[f][1] == int(o), f
    assert abi.profile_sample_dtype.fields["station"][1] == 0 and abi.profile_sample_dtype.fields["offset"][1] == 4
    assert int(re.search(r"#define SIMLOD_PROFILE_MAX_VERTICES (\d+)u", src).group(1)) == abi.PROFILE_MAX_VERTICES == 64
    assert int(re.search(r"#define SIMLOD_PROFILE_NO_SEGMENT\s+(0x[0-9a-f]+)u", src).group(1), 16) == abi.PROFILE_NO_SEGMENT
    r = Profile([(1, 2), (3, 4), (5, 7)], 0.5, (1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12)).record()
    assert r.dtype == abi.profile_dtype and int(r["numVertices"][0]) == 3 and float(r["halfWidth"][0]) == 0.5 and not r["reserved"].any()
    assert r["vertices"][0, :3].tolist() == [[1, 2], [3, 4], [5, 7]] and not r["vertices"][0, 3:].any()
    assert r["axisU"][0].tolist() == [1, 2, 3, 4] and r["axisV"][0].tolist() == [5, 6, 7, 8] and r["axisH"][0].tolist() == [9, 10, 11, 12]


def test_profile_symbols_exported(built_libs):
    from simlod_amd import runtime
    L = runtime.lib()
    for s in ("simlod_profile_buffer_min_bytes", "simlod_query_profile"):
        assert s in runtime.EXPORTED_SYMBOLS and hasattr(L, s)
    # the query's bytes plus a fixed 4 KB block for the segments
    assert L.simlod_profile_buffer_min_bytes(100, 0) - L.simlod_query_buffer_min_bytes(100, 0) == 4096
    assert L.simlod_profile_buffer_min_bytes(7000, 5_000_000) - L.simlod_query_buffer_min_bytes(7000, 5_000_000) == 4096
    assert 63 * abi.profile_segment_dtype.itemsize <= 4096


def test_record_refuses_what_the_call_refuses():
    line = [(0, 0), (1, 0), (1, 1)]
    f = Profile.from_xy(line, 0.25)
    assert f.vertices.dtype == f.axis_u.dtype == f.axis_v.dtype == f.axis_h.dtype == np.float32 and isinstance(f.half_width, np.float32)
    assert f.axis_u.tolist() == [1, 0, 0, 0] and f.axis_v.tolist() == [0, 1, 0, 0] and f.axis_h.tolist() == [0, 0, 1, 0]
    assert len(Profile(np.stack([np.arange(64), np.zeros(64)], axis=1), 1.0)) == 64 and len(Profile(line[:2], 1.0)) == 2
    for bad in (line[:1], np.stack([np.arange(65), np.zeros(65)], axis=1), [(0, 0), (1, np.nan)], [(0, 0), (1e39, 0)], [(0, 0), (np.inf, 0)],
                [(0, 0), (0, 0), (1, 1)], [(0, 0), (1, 1), (1, 1)], [(0.1, 3), (0.1 + 1e-12, 3)]):        # (the last: one fp32 point twice)
        with pytest.raises(ValueError):
            Profile(bad, 0.25)
    for w in (0.0, -1.0, np.nan, np.inf, 1e39, 1e-60):                  # (1e-60 is 0 as float32)
        with pytest.raises(ValueError):
            Profile(line, w)
    for k in ("axis_u", "axis_v", "axis_h"):
        with pytest.raises(ValueError):
            Profile(line, 0.25, **{k: (1, 0, np.nan, 0)})
        with pytest.raises(ValueError):
            Profile(line, 0.25, **{k: (0, 1e39, 0, 0)})             # infinite as float32
    # record() checks again: a profile edited after it was made
    for edit in ("width", "vertex", "axis", "zero", "count"):
        g = Profile.from_xy(line, 0.25)
        if edit == "width":
            g.half_width = np.float32(0.0)
        elif edit == "vertex":
            g.vertices[1, 0] = np.nan
        elif edit == "axis":
            g.axis_h[3] = np.inf
        elif edit == "zero":
            g.vertices[2] = g.vertices[1]
        else:
            g.vertices = g.vertices[:1]
        with pytest.raises(ValueError):
            g.record()


def _pts(xyz):
    p = np.zeros(len(xyz), dtype=abi.point_dtype)
    a = np.asarray(xyz, dtype=np.float32)
    p["x"], p["y"], p["z"] = a[:, 0], a[:, 1], a[:, 2]
    return p


def test_locate_on_a_hand_made_corner():
    """An L of two segments of length 4 with half-width 1: stations run on through the bend, the offset is positive to the left, the inside of
    the bend belongs to segment 0, the wedge outside it to nobody, and the ends are square."""
    f = Profile.from_xy([(0, 0), (4, 0), (4, 4)], 1.0)
    s = f.segments()
    assert s["s0"].tolist() == [0.0, 4.0] and s["L2"].tolist() == [16.0, 16.0] and s["W2"].tolist() == [16.0, 16.0] and s["inv"].tolist() == [0.25, 0.25]
    assert f.length == 8.0
    seg, station, offset, h = f.locate(_pts([(1, 0.5, 7), (1, -0.5, 8), (3.5, 0.5, 0), (4.5, 2, 1), (3.5, 2, 2), (4.5, -0.5, 0), (-0.5, 0, 0), (4, 4.5, 0),
                                              (4, 1, 0), (0, 1, 0), (2, 1.5, 0), (np.nan, 0, 0)]))
    assert seg.tolist() == [0, 0, 0, 1, 1, -1, -1, -1, 0, 0, -1, -1]
    assert station.tolist()[:5] == [1.0, 1.0, 3.5, 6.0, 6.0] and offset.tolist()[:5] == [0.5, -0.5, 0.5, -0.5, 0.5]
    assert h.tolist()[:5] == [7, 8, 0, 1, 2] and station[5:8].tolist() == [0, 0, 0] and offset[5:8].tolist() == [0, 0, 0]
    r = f.records(_pts([(1, 0.5, 7), (9, 9, 3)]))
    assert r.dtype == abi.profile_sample_dtype and r["segment"].tolist() == [0, abi.PROFILE_NO_SEGMENT] and r["height"].tolist() == [7, 3]
    assert pr.locate_exact(f, _pts([(1, 0.5, 7), (4.5, 2, 1), (4, 1, 0), (0, 1, 0), (2, 1.5, 0), (4.5, -0.5, 0)])).tolist() == [0, 1, 0, 0, -1, -1]
    # an oblique map and a height that is not z: u = 2x + 1, v = z, h = y - 1
    g = Profile([(1, 0), (9, 0)], 1.0, (2, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, -1))
    seg, station, offset, h = g.locate(_pts([(1, 5, 0.5), (1, 5, -1.5)]))
    assert seg.tolist() == [0, -1] and station[0] == 2.0 and offset[0] == 0.5 and h.tolist() == [4, 4]


def test_classify_profile_on_a_hand_made_table():
    # box [0, 8)^3; level-1 nodes are cubes of 4, level-3 nodes cubes of 1.  The corridor y in [1, 3] for x in [0.5, 7.5]:
    # node (0, 0, *) of level 1 is cut by it, node (0, 1, *) above it is FAR (c_min > w), the level-3 nodes (2, 2, 5) and (6, 1, 0) lie inside,
    # (0, 2, 0) has the segment's start inside it (al_min < 0), (2, 5, 0) is FAR
    t = np.zeros(7, dtype=abi.export_node_dtype)
    t["level"] = [0, 1, 1, 3, 3, 3, 3]
    t["X"], t["Y"], t["Z"] = [0, 0, 0, 2, 6, 0, 2], [0, 0, 1, 2, 1, 2, 5], [0, 1, 0, 5, 0, 0, 0]
    far, covered = classify_profile(Profile.from_xy([(0.5, 2), (7.5, 2)], 1.0 + 2.0 ** -10), t, (0, 0, 0), (8, 8, 8))
    assert far.tolist() == [False, False, True, False, False, False, True] and covered.tolist() == [False, False, False, True, True, False, False]
    # two segments: the second covers the level-3 node (7, 4, 0), which the first is far from; (7, 2, 0) at the bend reaches past the first's end
    # and before the second's start — covered by neither, far from neither
    b = np.zeros(3, dtype=abi.export_node_dtype)
    b["level"], b["X"], b["Y"] = 3, [7, 7, 2], [4, 2, 5]
    bend = Profile.from_xy([(0.5, 2), (7.5, 2), (7.5, 7.5)], 1.0 + 2.0 ** -10)
    far, covered = classify_profile(bend, b, (0, 0, 0), (8, 8, 8))
    assert far.tolist() == [False, False, True] and covered.tolist() == [True, False, False]
    far, covered = classify_profile(Profile.from_xy(bend.vertices[:2], bend.half_width), b, (0, 0, 0), (8, 8, 8))
    assert far.tolist() == [True, False, True] and not covered.any()
    # mixed signs in the axes: u = -x + 8
    far, covered = classify_profile(Profile([(0.5, 2), (7.5, 2)], 1.0 + 2.0 ** -10, (-1, 0, 0, 8)), t, (0, 0, 0), (8, 8, 8))
    assert far.tolist() == [False, False, True, False, False, False, True] and covered.tolist() == [False, False, False, True, True, False, False]


@pytest.fixture(scope="module", params=cases.CASES)
def built(request):
    """-> (name, full export, points, box)"""
    name = request.param
    ex, pts, box, ho = rr.host_octree(name)
    return name, ex, pts, box


def _selected_source_samples(ex, sel, ml):
    """The samples of the nodes (sel, ml) selects, in table order: what P1 applied to EVERY sample has to look at."""
    t = ex.truncated(ml, sel)
    return t.samples


def test_mirror_is_the_exact_rule_on_every_selected_sample(built):
    name, ex, pts, box = built
    fractions = 0
    for kind in pr.PROFILE_NAMES:
        f = pr.profile(kind, box)
        for sel, ml in MODES:
            c, rec, cnt = ex.profile(f, None, ml, sel, return_counts=True)
            c.validate()
            assert c.select == abi.EXPORT_REGION and c.max_level == ml and len(rec) == c.num_samples
            assert int(cnt["numNodes"]) == c.num_nodes and int(cnt["numSamples"]) == c.num_samples <= int(cnt["numCandidates"])
            src = _selected_source_samples(ex, sel, ml)
            seg, decided = pr.locate_exact(f, src, return_decided=True)
            fractions += int(decided.sum())
            # breadth-first order on both sides: the passing samples of the selected nodes in table order are the result, sample by sample
            assert c.samples.tobytes() == src[seg >= 0].tobytes(), f"{name} {kind} {sel}@{ml}: the sample set is not the exact rule's"
            assert np.array_equal(rec["segment"].astype(np.int64), seg[seg >= 0]), f"{name} {kind} {sel}@{ml}: segments"
            # the records are Profile.locate's
            s2, station, offset, h = f.locate(c.samples)
            assert np.array_equal(s2, seg[seg >= 0]) and rec["station"].tobytes() == station.tobytes() and rec["offset"].tobytes() == offset.tobytes()
            assert rec["height"].tobytes() == h.tobytes()
            # rule P3 changes nothing: the same query with every listed node tested sample by sample
            c2, rec2, cnt2 = ex.profile(f, None, ml, sel, return_counts=True, test_every_sample=True)
            assert c2.nodes.tobytes() == c.nodes.tobytes() and c2.samples.tobytes() == c.samples.tobytes() and rec2.tobytes() == rec.tobytes()
            assert int(cnt2["numCopiedNodes"]) == 0 and int(cnt2["numFilteredNodes"]) == int(cnt["numFilteredNodes"]) + int(cnt["numCopiedNodes"])
            if kind == "cover":
                t = ex.truncated(ml, sel)
                assert c.nodes.tobytes() == t.nodes.tobytes() and c.samples.tobytes() == t.samples.tobytes(), (name, sel, ml)
                assert int(cnt["numFilteredNodes"]) == 0 and int(cnt["numCopiedNodes"]) == int((t.nodes["numSamples"] != 0).sum())
                assert (rec["segment"] == 0).all()
            if kind == "miss":
                assert [int(cnt[k]) for k in cnt.dtype.names] == [1, 0, 0, 0, 0, 0] and len(rec) == 0
            if (sel, ml) == ("cut", 20):
                rr.assert_same_multiset(c.samples, pts[pr.locate_exact(f, pts) >= 0], f"{name} {kind}")
    print(name, f"{fractions} samples decided in Fractions")


def test_station_lies_in_its_segment(built):
    """station is non-decreasing in the segment's s0: s0_i <= station <= s0_i + len_i, each rounded to fp32 as the station is."""
    name, ex, pts, box = built
    seen = 0
    for kind in ("zigzag", "hairpin", "wave64", "oblique"):
        f = pr.profile(kind, box)
        c, rec = ex.profile(f, None, 20, "cut")
        s = f.segments()
        lo, hi = s["s0"].astype(np.float32), (s["s0"] + np.sqrt(s["L2"])).astype(np.float32)
        i = rec["segment"].astype(np.int64)
        seen += len(rec)
        assert (len(rec) > 0 or "hotspot" in name) and (i < len(s)).all()          # (the hotspot is one level-3 cell: not every corridor meets it)
        assert (rec["station"] >= lo[i]).all() and (rec["station"] <= hi[i]).all(), (name, kind)
        assert (np.abs(rec["offset"].astype(np.float64)) <= float(f.half_width) * (1 + 2.0 ** -23)).all(), (name, kind)
        order = np.argsort(rec["station"], kind="stable")
        assert (np.diff(s["s0"][i[order]]) >= 0).all(), f"{name} {kind}: a later station in an earlier segment"
    assert seen > 1000, name


def test_hairpin_the_lower_segment_owns_the_overlap(built):
    name, ex, pts, box = built
    f = pr.profile("hairpin", box)
    c, rec = ex.profile(f, None, 20, "cut")
    back = Profile(f.vertices[1:], f.half_width, f.axis_u, f.axis_v, f.axis_h)           # segment 1 alone
    in_both = (rec["segment"] == 0) & (back.locate(c.samples)[0] == 0)
    only_second = rec["segment"] == 1
    print(name, int(in_both.sum()), "samples in both segments,", int(only_second.sum()), "in the second only")
    assert int(in_both.sum()) >= 50 and (int(only_second.sum()) >= 1 or "hotspot" in name)      # (the hotspot's cell lies on the first segment's side)
    assert (back.locate(c.samples[only_second])[0] == 0).all()
    # none of the second segment's samples is in the first
    first = Profile(f.vertices[:2], f.half_width, f.axis_u, f.axis_v, f.axis_h)
    assert (first.locate(c.samples[only_second])[0] == -1).all() and (first.locate(c.samples[~only_second])[0] == 0).all()


def test_reversed_single(built):
    """The corridor travelled the other way: the same samples; the two stations add up to the length and the two offsets cancel.  In exact
    arithmetic al + al' = L2 and c' = -c, so station + station' = len and offset + offset' = 0.  What is compared are four fp32 roundings of fp64
    values: each is off by at most half the spacing of fp32 at its own magnitude, and the fp64 values under them by a few 2^-53 of the terms they
    are sums of, |du| (|pu| + |pv|) inv <= len + 2 w — 2^-45 (len + 2 w) covers them."""
    name, ex, pts, box = built
    f = pr.profile("single", box)
    g = f.reversed()
    a, ra = ex.profile(f, None, 20, "cut")
    b, rb = ex.profile(g, None, 20, "cut")
    rr.assert_same_multiset(a.samples, b.samples, f"{name}: single and its reverse")
    assert a.samples.tobytes() == b.samples.tobytes()                       # (the same nodes in the same order, hence the same pairing)
    assert len(ra) > 0 and (ra["segment"] == 0).all() and (rb["segment"] == 0).all()
    length, w = f.length, float(f.half_width)
    assert abs(g.length - length) <= 2.0 ** -50 * length
    half_ulp = lambda v: 0.5 * np.spacing(np.abs(v)).astype(np.float64)
    slack = 2.0 ** -45 * (length + 2 * w)
    sa, oa, sb, ob = ra["station"], ra["offset"], rb["station"], rb["offset"]
    err_s = np.abs(sa.astype(np.float64) + sb.astype(np.float64) - length)
    err_o = np.abs(oa.astype(np.float64) + ob.astype(np.float64))
    assert (err_s <= half_ulp(sa) + half_ulp(sb) + slack).all(), f"{name}: stations off by up to {err_s.max()}"
    assert (err_o <= half_ulp(oa) + half_ulp(ob) + slack).all(), f"{name}: offsets off by up to {err_o.max()}"
    assert ra["height"].tobytes() == rb["height"].tobytes()


def test_profile_composes_with_a_height_band(built):
    name, ex, pts, box = built
    z = np.sort(pts["z"].astype(np.float64))
    lo, hi = float(z[len(z) // 4]), float(z[3 * len(z) // 4])
    band = Region.from_planes([[0, 0, 1, -lo], [0, 0, -1, hi]])
    for kind in ("zigzag", "oblique"):
        f = pr.profile(kind, box)
        for sel, ml in MODES:
            a, ra, ca = ex.profile(f, None, ml, sel, return_counts=True)
            b, rb, cb = ex.profile(f, band, ml, sel, return_counts=True)
            b.validate()
            keep = rr.brute_mask(band, a.samples)
            assert 0 < keep.sum() < len(keep) or "hotspot" in name, (name, kind)
            assert b.samples.tobytes() == a.samples[keep].tobytes() and rb.tobytes() == ra[keep].tobytes(), (name, kind, sel, ml)
            assert int(cb["numSamples"]) == int(keep.sum())


@pytest.mark.parametrize("kind", ["single", "zigzag", "hairpin", "wave64"])
def test_profiles_are_not_vacuous(kind):
    ex, pts, box, ho = _terrain()
    f = pr.profile(kind, box)
    c, rec, cnt = ex.profile(f, None, 20, "all", return_counts=True)
    print(kind, {k: int(cnt[k]) for k in cnt.dtype.names}, "segments", np.unique(rec["segment"]).tolist())
    assert int(cnt["numSamples"]) > 1000 and int(cnt["numFilteredNodes"]) > 0 and int(cnt["numCopiedNodes"]) > 0
    assert int(cnt["numSamples"]) < int(cnt["numCandidates"])
    if kind != "single":
        assert len(np.unique(rec["segment"])) >= 2


_TERRAIN = []


def _terrain():
    if not _TERRAIN:
        _TERRAIN.append(rr.host_octree("terrain_4x100k"))
    return _TERRAIN[0]


def test_the_exact_path_is_not_dead():
    """Points ON a corridor's start line, end line and side lines (al == 0, al == L2, c*c == W2 exactly) are decided by Fractions, the same way as
    by the fp64 rule: all four lines belong to the corridor."""
    f = Profile.from_xy([(1, 2), (5, 2)], 0.5)
    on = _pts([(1, 2.25, 0), (5, 1.75, 0), (3, 2.5, 0), (3, 1.5, 0), (3, 2, 0), (0.75, 2, 0), (3, 2.75, 0)])
    seg, decided = pr.locate_exact(f, on, return_decided=True)
    assert seg.tolist() == [0, 0, 0, 0, 0, -1, -1] and decided.tolist() == [True, True, True, True, False, False, False]
    assert np.array_equal(seg, f.locate(on)[0])
    # the georef terrain: fp32 steps of 1/32 m and 1/4 m put input points on the lines of an axis-aligned corridor
    pts, box_min, box, _ = cases.shifted("terrain_4x100k", cases.GEOREF)
    g = Profile.from_xy([(box_min[0] + 100.0, box_min[1] + 200.0), (box_min[0] + 500.0, box_min[1] + 200.0)], 50.0)
    seg, decided = pr.locate_exact(g, pts, return_decided=True)
    print(int(decided.sum()), "georef points decided in Fractions")
    assert np.array_equal(seg, g.locate(pts)[0]) and int(decided.sum()) >= 10
