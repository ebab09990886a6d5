"""CPU tier of the profile queries' shared rules (include/simlod_hip.h, "profile queries"): simlod_amd/csrc/profile_rules.hpp — what the call accepts
(rule P6), the segment block of rule P0 and a node's class by the corridor (rule P3) — checked on the host by a program of its own
(tests/host/profile_rules_check.cpp, built with the address and undefined-behaviour sanitizers) against octree_io.Profile.segments and
octree_io.classify_profile, byte for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import profile_ref as pr
from simlod_amd import abi
from simlod_amd.octree_io import Profile, classify_profile
from test_clip_rules import _nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 63 * abi.profile_segment_dtype.itemsize


def _grazing(nodes, box_min, size):
    """Plan-view corridors whose start line, end line or side line runs through a corner of one of `nodes`, with and without the inflation by one
    level-20 cell: al_min, al_max - L2 and c*c - W2 come out at or next to 0."""
    out = []
    e = size * 2.0 ** -20
    for nd in nodes:
        s = size / 2.0 ** int(nd["level"])
        lo = np.asarray(box_min, np.float64)[:2] + np.array([nd["X"], nd["Y"]], np.float64) * s
        hi = lo + s
        w = 0.75 * s
        for shift in (0.0, e, -e):
            # along +x through the node: starting on its min-x face, ending on its max-x face, its side line on the node's max-y face
            out.append(Profile.from_xy([(lo[0] - shift, lo[1] + 0.5 * s), (hi[0] + 2 * s, lo[1] + 0.5 * s)], w))
            out.append(Profile.from_xy([(lo[0] - 2 * s, lo[1] + 0.5 * s), (hi[0] + shift, lo[1] + 0.5 * s)], w))
            out.append(Profile.from_xy([(lo[0] - s, hi[1] + shift - w), (hi[0] + s, hi[1] + shift - w)], w))
            # a diagonal whose side line passes through the far corner, and a bend at the near corner
            out.append(Profile.from_xy([(lo[0] - s, lo[1] - s), (hi[0] + s + shift, hi[1] + s - shift), (hi[0] + 2 * s, lo[1])], w))
            out.append(Profile.from_xy([(lo[0] - s, lo[1] + shift), (lo[0] + shift, lo[1] + shift), (lo[0] + shift, hi[1] + s)], 0.5 * s))
    return out


def _bad_records():
    ok = Profile.from_xy([(0.1, 0.2), (0.5, 0.6), (0.9, 0.3)], 0.05).record()
    bad = []
    for edit in ("n0", "n1", "n65", "nmax", "w0", "w-", "wnan", "winf", "vnan", "vinf", "unan", "vaxinf", "hnan", "zero_first", "zero_last", "reserved0", "reserved1"):
        r = ok.copy()
        if edit[0] == "n":
            r["numVertices"] = {"n0": 0, "n1": 1, "n65": 65, "nmax": 0xFFFFFFFF}[edit]
        elif edit[0] == "w":
            r["halfWidth"] = {"w0": 0.0, "w-": -0.05, "wnan": np.nan, "winf": np.inf}[edit]
        elif edit == "vnan":
            r["vertices"][0, 2, 1] = np.nan
        elif edit == "vinf":
            r["vertices"][0, 0, 0] = -np.inf
        elif edit == "unan":
            r["axisU"][0, 1] = np.nan
        elif edit == "vaxinf":
            r["axisV"][0, 3] = np.inf
        elif edit == "hnan":
            r["axisH"][0, 0] = np.nan
        elif edit == "zero_first":
            r["vertices"][0, 1] = r["vertices"][0, 0]
        elif edit == "zero_last":
            r["vertices"][0, 2] = r["vertices"][0, 1]
        elif edit == "reserved0":
            r["reserved"][0, 0] = 1
        else:
            r["reserved"][0, 1] = 7
        bad.append((edit, r))
    return ok, bad


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("profile_rules") / "profile_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "profile_rules_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("where", ["origin", "georef"])
def test_header_classifies_nodes_as_classify_profile_does(checker, tmp_path, where):
    """1 500 (level, X, Y, Z) x the suite's profiles and corridors grazing node corners, on a unit box at the origin and on the 600 x 400 x 40 box
    at cases.GEOREF: the segment block equals Profile.segments and the class equals classify_profile, byte for byte; a record rule P6 refuses is
    refused.  A vertex behind numVertices is not looked at."""
    rs = np.random.RandomState(7)
    box = (1.0, 1.0, 1.0) if where == "origin" else (600.0, 400.0, 40.0)
    mn = np.zeros(3, np.float32) if where == "origin" else np.asarray(cases.GEOREF, np.float32)
    mx = (mn + np.asarray(box, np.float32)).astype(np.float32)
    size = float((mx - mn).max())
    nodes = _nodes(rs, 1500)
    shallow = nodes[(nodes["level"] >= 1) & (nodes["level"] <= 8)]        # (at the georef offset fp32 steps are 1/32 m and 1/2 m: deeper nodes are smaller)
    profiles = [pr.profile(k, box, mn.astype(np.float64)) for k in pr.PROFILE_NAMES] + _grazing(shallow[rs.choice(len(shallow), 8, replace=False)], mn, size)
    records = [p.record() for p in profiles]
    beyond = records[0].copy()
    beyond["vertices"][0, 2, 0] = np.nan
    records.append(beyond)
    profiles.append(profiles[0])
    ok, bad = _bad_records()
    records += [r for _, r in bad]
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(records), len(nodes)], "<u4").tobytes())
        f.write(mn.astype("<f4").tobytes() + mx.astype("<f4").tobytes())
        f.write(np.concatenate(records).tobytes())
        f.write(np.ascontiguousarray(nodes).tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(len(records), 1 + BLOCK + len(nodes))
    seen = set()
    for j, p in enumerate(profiles):
        assert got[j, 0] == 1, f"profile {j} refused"
        block = p.segments().tobytes()
        assert got[j, 1: 1 + len(block)].tobytes() == block, f"profile {j}: the segment block differs"
        assert not got[j, 1 + len(block): 1 + BLOCK].any()
        far, covered = classify_profile(p, nodes, mn, mx)
        cls = np.where(far, 0, np.where(covered, 2, 1))
        assert np.array_equal(got[j, 1 + BLOCK:], cls), f"profile {j}: {int((got[j, 1 + BLOCK:] != cls).sum())} classes differ"
        seen |= set(cls.tolist())
    assert seen == {0, 1, 2}
    for j, (edit, _) in enumerate(bad):
        assert not got[len(profiles) + j].any(), f"a record with a bad {edit} was accepted"


def test_grazing_corridors_graze():
    """The corridors of _grazing put a corner value of their own node at or next to 0: per node all three classes occur over the shifts."""
    rs = np.random.RandomState(7)
    nodes = _nodes(rs, 200)
    nodes = nodes[(nodes["level"] >= 1) & (nodes["level"] <= 12)][:6]
    seen = set()
    for p in _grazing(nodes, np.zeros(3), 1.0):
        far, covered = classify_profile(p, nodes, (0, 0, 0), (1, 1, 1))
        seen |= set(np.where(far, 0, np.where(covered, 2, 1)).tolist())
    assert seen == {0, 1, 2}
    # the start line on the node's min face: covered with the line on the inflated face, filtered one level-20 cell inside it
    t = np.zeros(1, dtype=abi.export_node_dtype)
    t["level"], t["X"], t["Y"] = 3, 2, 5
    e = 2.0 ** -20
    cls = []
    for shift in (e, 0.0, -e):
        p = Profile.from_xy([(0.25 - shift, 0.6875), (0.75, 0.6875)], 0.125)
        far, covered = classify_profile(p, t, (0, 0, 0), (1, 1, 1))
        cls.append((bool(far[0]), bool(covered[0])))
    assert cls == [(False, True), (False, False), (False, False)]
