"""Host tier of the view queries (include/simlod_hip.h, "view queries"): simlod_amd/csrc/view_rules.hpp — what the call accepts, the frustum planes, a
node's inside, screen extents and rank, what is drawn at a bias — checked on the host by a program of its own (tests/host/view_rules_check.cpp, built
with the address and undefined-behaviour sanitizers) against the numpy mirror octree_io.view_geometry."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import view_ref
from simlod_amd import abi
from simlod_amd.octree_io import view_geometry
from test_clip_rules import _nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOXES = {"unit": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), "terrain": (view_ref.TERRAIN_BOX, (0.0, 0.0, 0.0)), "georef": (view_ref.TERRAIN_BOX, cases.GEOREF)}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("view_rules") / "view_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "view_rules_check.cpp"), "-o", exe])
    return exe


def _bad_cases(u):
    """(what, uniforms, view) the call refuses."""
    ok = abi.view_record()
    bad = []
    for what, field, value in (("flag", "flags", 4), ("reserved", "reserved", 1), ("order", "minBias", 21), ("range", "maxBias", 21)):
        v = ok.copy()
        v[field] = value
        bad.append((what, u, v))
    for what, field, value in (("minNodeSize", "minNodeSize", np.nan), ("width", "width", np.inf), ("height", "height", -np.inf)):
        w = np.array(u, copy=True)
        w[field] = value
        bad.append((what, w, ok))
    w = np.array(u, copy=True)
    w["transform_updateBound"][2, 1] = np.nan
    bad.append(("matrix", w, ok))
    return bad


def _bits(x):
    b = np.asarray(x, np.float32).view(np.uint32).copy()
    b[np.isnan(x)] = 0x7FC00000
    return b


@pytest.mark.parametrize("where", list(BOXES))
def test_header_agrees_with_the_mirror(checker, tmp_path, where):
    """A few thousand (level, X, Y, Z) over levels 0-20 under the five cameras, minNodeSize 64 and 1/8: inside, the bit patterns of dx and dy and the
    rank from the header equal the mirror's; every refusal is refused.  One matrix has a zero last row (w == 0 at every corner), so NaN and
    infinite extents are part of the comparison."""
    box, mn = BOXES[where]
    rs = np.random.RandomState(11)
    nodes = _nodes(rs, 3000)
    us = []
    for cam in view_ref.CAMERAS:
        T = view_ref.transform_of(cam, box, mn)
        us.append(view_ref.uniforms_of(box, T, box_min=mn))
        us.append(abi.make_uniforms(640, 480, T, box, min_node_size=0.125, box_min=mn))
    frozen = view_ref.uniforms_of(box, view_ref.transform_of("bird", box, mn), box_min=mn, frozen=view_ref.transform_of("inside", box, mn))
    us.append(frozen)
    flat = np.array(view_ref.transform_of("bird", box, mn), dtype=np.float32, copy=True).reshape(4, 4)
    flat[3] = 0.0                                                 # w == 0 at every corner: the divisions give infinities and NaNs, fminf / fmaxf drop the NaNs
    us.append(view_ref.uniforms_of(box, flat, box_min=mn))
    for size in (0.0, -1.0, 1e-30, 3e38):                         # not positive: the rank is counted bias by bias; tiny and huge: found by halving, as at 64
        us.append(abi.make_uniforms(view_ref.WIDTH, view_ref.HEIGHT, view_ref.transform_of("closer", box, mn), box, min_node_size=size, box_min=mn))
    good = [(u, abi.view_record()) for u in us] + [(us[0], abi.view_record(3, 7, 10, cull=False, draw_small_root=True))]
    bad = _bad_cases(us[0])
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(good) + len(bad), len(nodes)], "<u4").tobytes())
        for u, v in good + [(u, v) for _, u, v in bad]:
            f.write(np.asarray(u).tobytes() + v.tobytes())
        f.write(np.ascontiguousarray(nodes).tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint32).reshape(len(good) + len(bad), 1 + 4 * len(nodes))
    ranks, insides, odd = set(), set(), 0
    for j, (u, _) in enumerate(good):
        assert got[j, 0] == 1, f"case {j} refused"
        inside, dx, dy, rank = view_geometry(u, nodes)
        rows = got[j, 1:].reshape(len(nodes), 4)
        assert np.array_equal(rows[:, 0], inside.astype(np.uint32)), f"case {j}: {int((rows[:, 0] != inside).sum())} inside flags differ"
        assert np.array_equal(rows[:, 1], _bits(dx)) and np.array_equal(rows[:, 2], _bits(dy)), f"case {j}: extents differ"
        assert np.array_equal(rows[:, 3], rank.astype(np.uint32)), f"case {j}: ranks differ"
        ranks |= set(rank.tolist())
        insides |= set(inside.tolist())
        odd += int((~np.isfinite(dx)).sum())
    assert insides == {True, False} and {0, 21} <= ranks and len(ranks) >= 12, sorted(ranks)
    assert odd > 0
    # the frozen camera's geometry is transform_updateBound's
    assert np.array_equal(view_geometry(frozen, nodes)[3], view_geometry(us[4], nodes)[3])
    for j, (what, _, _) in enumerate(bad):
        assert got[len(good) + j, 0] == 0 and not got[len(good) + j, 1:].any(), f"a call with a bad {what} was accepted"
