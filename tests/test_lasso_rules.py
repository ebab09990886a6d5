"""CPU tier of the lasso queries' shared rules (include/simlod_hip.h, "lasso queries"): simlod_amd/csrc/lasso_rules.hpp — what the call accepts
(rule L7), the rows and the edge block widened to fp64 and a node's class by the lasso (rules L2-L4) — checked on the host by a program of its
own (tests/host/lasso_rules_check.cpp, built with the address and undefined-behaviour sanitizers) against octree_io.Lasso.edges and
octree_io.classify_lasso, byte for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import lasso_ref as lr
from simlod_amd import abi
from simlod_amd.octree_io import Footprint, Lasso, classify_lasso
from test_clip_rules import _nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 12 * 8
BLOCK = abi.LASSO_MAX_VERTICES * 32


def _classes(lasso, nodes, mn, mx):
    outside, copied = classify_lasso(lasso, nodes, mn, mx)
    assert not (outside & copied).any()
    return np.where(outside, 0, np.where(copied, 2, 1))


def _grazing(nodes, box_min, size, T):
    """Lassos with an edge whose plane through the eye runs through a corner of one of `nodes`, and one level-20 cell to either side of it.
    Plan view (rows U = x, V = y, W = 1: the planes are exactly the node's faces, inflated or not) and on the screen of the camera T (the
    projected corner rounded to a float32 pixel: c comes out next to 0)."""
    out = []
    e = size * 2.0 ** -20
    m = np.asarray(T, np.float64).reshape(4, 4)
    for nd in nodes:
        s = size / 2.0 ** int(nd["level"])
        lo = np.asarray(box_min, np.float64) + np.array([nd["X"], nd["Y"], nd["Z"]], np.float64) * s
        hi = lo + s
        for shift in (0.0, e, -e, 2 * e):
            # a plan-view rectangle around the node whose min-x edge lies on the node's min-x face moved by `shift` (-e: the inflated face)
            f = Footprint.from_rect((lo[0] + shift, lo[1] - s), (hi[0] + 2 * s, hi[1] + s))
            out.append(Lasso.from_footprint(f))
            # ... and one that ends on the max-x face moved by `shift`
            out.append(Lasso.from_footprint(Footprint.from_rect((lo[0] - 2 * s, lo[1] - s), (hi[0] + shift, hi[1] + s))))
            # on the screen: a triangle with an edge from the picture of the node's min corner (moved by `shift`) to that of its max corner
            px = []
            for c in (lo + shift, hi - shift):
                h = m @ np.array([c[0], c[1], c[2], 1.0])
                if h[3] <= 0:
                    break
                px.append((0.5 * lr.W * (h[0] / h[3] + 1.0), 0.5 * lr.H * (h[1] / h[3] + 1.0)))
            if len(px) == 2 and px[0] != px[1]:
                out.append(Lasso.from_pixels(T, lr.W, lr.H, [px[0], px[1], (px[0][0] + 300.0, px[0][1] - 200.0)]))
    return out


def _bad_records(ok):
    bad = []
    for edit in ("n0", "n2", "n257", "nmax", "vnan", "vinf", "unan", "vrowinf", "wnan", "winf", "reserved0", "reserved1", "reserved2"):
        r = ok.copy()
        if edit[0] == "n":
            r["numVertices"] = {"n0": 0, "n2": 2, "n257": 257, "nmax": 0xFFFFFFFF}[edit]
        elif edit == "vnan":
            r["vertices"][0, 2, 1] = np.nan
        elif edit == "vinf":
            r["vertices"][0, 0, 0] = -np.inf
        elif edit == "unan":
            r["rowU"][0, 1] = np.nan
        elif edit == "vrowinf":
            r["rowV"][0, 3] = np.inf
        elif edit == "wnan":
            r["rowW"][0, 0] = np.nan
        elif edit == "winf":
            r["rowW"][0, 3] = -np.inf
        else:
            r["reserved"][0, int(edit[-1])] = 1 + int(edit[-1])
        bad.append((edit, r))
    return bad


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("lasso_rules") / "lasso_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "lasso_rules_check.cpp"), "-o", exe])
    return exe


def _setup(where):
    rs = np.random.RandomState(7)
    box = (1.0, 1.0, 1.0) if where == "origin" else (600.0, 400.0, 40.0)
    off = (0.0, 0.0, 0.0) if where == "origin" else cases.GEOREF
    mn = np.asarray(off, np.float32)
    mx = (mn + np.asarray(box, np.float32)).astype(np.float32)
    size = float((mx - mn).max())
    nodes = _nodes(rs, 1500)
    shallow = nodes[(nodes["level"] >= 1) & (nodes["level"] <= 8)]        # (at the georef offset fp32 steps are 1/32 m and 1/2 m: deeper nodes are smaller)
    picked = shallow[rs.choice(len(shallow), 8, replace=False)]
    named = [lr.lasso(kind, lr.transform(cam, box, off)) for cam in lr.CAMERAS for kind in lr.LASSO_NAMES]
    grazing = _grazing(picked, mn, size, lr.transform("bird", box, off))
    return box, mn, mx, nodes, picked, named, grazing


@pytest.mark.parametrize("where", ["origin", "georef"])
def test_header_classifies_nodes_as_classify_lasso_does(checker, tmp_path, where):
    """1 500 (level, X, Y, Z) x the named lassos under the four cameras and lassos grazing node corners, on a unit box at the origin and on the
    600 x 400 x 40 box at cases.GEOREF: the rows and the edge block equal Lasso's and the class equals classify_lasso, byte for byte; a record
    rule L7 refuses is refused.  A vertex behind numVertices is not looked at; a row W of zeros is legal and puts every node outside."""
    box, mn, mx, nodes, picked, named, grazing = _setup(where)
    lassos = named + grazing
    zero_w = Lasso(lr.pixels("tri"), named[0].row_u, named[0].row_v, (0, 0, 0, 0))
    lassos.append(zero_w)
    records = [l.record() for l in lassos]
    beyond = records[0].copy()
    beyond["vertices"][0, len(lassos[0]), 0] = np.nan
    records.append(beyond)
    lassos.append(lassos[0])
    bad = _bad_records(records[0])
    records += [r for _, r in bad]
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(records), len(nodes)], "<u4").tobytes())
        f.write(mn.astype("<f4").tobytes() + mx.astype("<f4").tobytes())
        f.write(np.concatenate(records).tobytes())
        f.write(np.ascontiguousarray(nodes).tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(len(records), 1 + ROWS + BLOCK + len(nodes))
    seen = set()
    for j, l in enumerate(lassos):
        assert got[j, 0] == 1, f"lasso {j} refused"
        rows = np.concatenate([l.row_u, l.row_v, l.row_w]).astype(np.float64).tobytes()
        assert got[j, 1: 1 + ROWS].tobytes() == rows, f"lasso {j}: the rows differ"
        block = l.edge_block().tobytes()
        assert got[j, 1 + ROWS: 1 + ROWS + len(block)].tobytes() == block, f"lasso {j}: the edge block differs"
        assert not got[j, 1 + ROWS + len(block): 1 + ROWS + BLOCK].any()
        cls = _classes(l, nodes, mn, mx)
        assert np.array_equal(got[j, 1 + ROWS + BLOCK:], cls), f"lasso {j}: {int((got[j, 1 + ROWS + BLOCK:] != cls).sum())} classes differ"
        seen |= set(cls.tolist())
    assert seen == {0, 1, 2}
    assert not got[lassos.index(zero_w), 1 + ROWS + BLOCK:].any()
    for j, (edit, _) in enumerate(bad):
        assert not got[len(lassos) + j].any(), f"a record with a bad {edit} was accepted"


@pytest.mark.parametrize("where", ["origin", "georef"])
def test_grazing_lassos_graze(where):
    """The lassos of _grazing put a corner value of their own node at or next to 0: over the shifts all three classes occur among the picked
    nodes."""
    box, mn, mx, nodes, picked, named, grazing = _setup(where)
    seen = set()
    for l in grazing:
        seen |= set(_classes(l, picked, mn, mx).tolist())
    assert seen == {0, 1, 2}


def test_grazing_plan_view_edge_on_the_inflated_face():
    """The min-u edge of a plan-view rectangle on the node's min face: copied with the edge on the inflated face or outside it, filtered one
    level-20 cell inside it."""
    t = np.zeros(1, dtype=abi.export_node_dtype)
    t["level"], t["X"], t["Y"] = 3, 2, 5
    e = 2.0 ** -20
    cls = []
    for shift in (-2 * e, -e, 0.0, e):
        l = Lasso.from_footprint(Footprint.from_rect((0.25 + shift, 0.0), (0.75, 1.0)))
        cls.append(int(_classes(l, t, (0, 0, 0), (1, 1, 1))[0]))
    assert cls == [2, 1, 1, 1], cls
