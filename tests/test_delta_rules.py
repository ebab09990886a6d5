"""Host tier of the view deltas (include/simlod_hip.h, "view deltas"): simlod_amd/csrc/delta_rules.hpp — the key order of a table, the search of a
key in a held table, the state table of rules D3-D5, what the call refuses — checked on the host by a program of its own
(tests/host/delta_rules_check.cpp, built with the address and undefined-behaviour sanitizers) against the numpy mirror octree_io.delta_find /
delta_between."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import view_ref
from simlod_amd import abi
from simlod_amd.octree_io import OctreeExport, delta_between, delta_find, delta_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("delta_rules") / "delta_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "delta_rules_check.cpp"), "-o", exe])
    return exe


def _run(checker, tmp_path, held, keys, states, calls):
    keys, states, calls = (np.ascontiguousarray(a, dtype="<u4") for a in (keys, states, calls))
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(held), len(keys), len(states), len(calls)], "<u4").tobytes())
        f.write(np.ascontiguousarray(held).tobytes() + keys.tobytes() + states.tobytes() + calls.tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    out = np.fromfile(tmp_path / "out.bin", dtype=np.uint32)
    a, b = 3 * len(keys), 3 * len(keys) + 2 * len(states)
    return out[:a].reshape(-1, 3), out[a:b].reshape(-1, 2), out[b:]


def _key_records(keys):
    t = np.zeros(len(keys), dtype=abi.export_node_dtype)
    t["level"], t["X"], t["Y"], t["Z"] = np.asarray(keys, np.int64).reshape(-1, 4).T
    return t


def _deep_keys(rs, count):
    """Keys over levels 0-20 with every coordinate below 2^level, the corners of level 20 and two level-20 keys that differ in the top
    coordinate bit alone among them, in table order and without repeats."""
    level = rs.randint(0, 21, size=count)
    xyz = (rs.randint(0, 1 << 20, size=(count, 3)) >> (20 - level)[:, None])
    top = 1 << 19
    extra = [(20, 0, 0, 0), (20, top, 0, 0), (20, 0, top, 0), (20, 0, 0, top), (20, top - 1, top - 1, top - 1), (20, 2 * top - 1, 2 * top - 1, 2 * top - 1),
             (20, 5, 7, 9), (20, 5 + top, 7, 9), (0, 0, 0, 0)]
    keys = np.unique(np.concatenate([np.column_stack([level, xyz]), np.asarray(extra)]), axis=0)
    lv, m = delta_keys(_key_records(keys))
    return keys[np.lexsort((m, lv))]


def test_key_order_is_table_order():
    """The mirror's keys ascend strictly along every table of the suite's shapes: the complete tree (breadth-first, octant order) and a real view."""
    for t in (view_ref.complete_tree(3).nodes, view_ref.complete_tree(4).nodes):
        lv, m = delta_keys(t)
        later = (lv[1:] > lv[:-1]) | ((lv[1:] == lv[:-1]) & (m[1:] > m[:-1]))
        assert later.all()
        assert np.array_equal(delta_find(t, t), np.arange(len(t)))


def test_search_agrees_with_the_mirror(checker, tmp_path):
    rs = np.random.RandomState(5)
    keys = _deep_keys(rs, 4000)
    assert int((keys[:, 0] == 20).sum()) > 50
    top = 1 << 19
    pair = [int(np.nonzero((keys == k).all(1))[0][0]) for k in ((20, 5, 7, 9), (20, 5 + top, 7, 9))]
    held = _key_records(keys[rs.rand(len(keys)) < 0.6])
    held = np.concatenate([held, _key_records(keys[pair])])
    lv, m = delta_keys(held)
    held = np.unique(held[np.lexsort((m, lv))])                                # (np.unique sorts records by level, X, Y, Z: put back in key order below)
    lv, m = delta_keys(held)
    held = held[np.lexsort((m, lv))]
    for what, table in (("sorted", held), ("empty", held[:0]), ("one", held[:1]), ("shuffled", held[rs.permutation(len(held))])):
        found, _, _ = _run(checker, tmp_path, table, keys, np.zeros((0, 6)), np.zeros((0, 5)))
        mirror = delta_find(table, _key_records(keys))
        assert np.array_equal(found[:, 0], mirror.astype(np.uint32)), what
        hit = mirror != abi.EXPORT_NONE
        # never mistaken: what is found has the key; in key order nothing is missed
        assert all(tuple(table[int(h)][a] for a in ("level", "X", "Y", "Z")) == tuple(k) for h, k in zip(mirror[hit], keys[hit])), what
        if what == "sorted":
            have = {tuple(int(v) for v in (r["level"], r["X"], r["Y"], r["Z"])) for r in table}
            assert np.array_equal(hit, np.array([tuple(int(v) for v in k) in have for k in keys])), what
            assert hit[pair[0]] and hit[pair[1]] and mirror[pair[0]] != mirror[pair[1]]
            lvk, mk = delta_keys(_key_records(keys))
            assert np.array_equal(found[:, 1].astype(np.uint64) | found[:, 2].astype(np.uint64) << np.uint64(32), mk)
        elif what == "shuffled":
            assert 0 < hit.sum() < len(have)


def test_state_table_agrees_with_the_mirror(checker, tmp_path):
    """Every combination of the new entry's kind and SELECTED, a held entry found or not, its kind and SELECTED, n in {0, 1, 7} and the held count
    0, below, equal to and above n, with and without SIMLOD_DELTA_TAILS."""
    LEAF, SEL = abi.EXPORT_FLAG_LEAF, abi.EXPORT_FLAG_SELECTED
    rows = []
    for leaf, sel, found, hleaf, hsel, n, rel, tails in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 7), ("zero", "below", "equal", "above"), (0, 1)):
        hs = {"zero": 0, "below": max(n - 1, 0) if n != 1 else 0, "equal": n, "above": n + 3}[rel]
        if n == 7 and rel == "below":
            hs = 3
        rows.append((leaf * LEAF | sel * SEL, n if sel else 0, found, hleaf * LEAF | hsel * SEL, hs if hsel else 0, tails))
    rows = np.asarray(rows, np.int64)
    _, got, _ = _run(checker, tmp_path, np.zeros(0, abi.export_node_dtype), np.zeros((0, 4)), rows, np.zeros((0, 5)))
    seen = set()
    for tails in (0, 1):
        part = np.nonzero(rows[:, 5] == tails)[0]
        r = rows[part]
        # one table entry per row, in key order (level 7, Z ascending); the held table has the rows with `found`
        new = np.zeros(len(r), dtype=abi.export_node_dtype)
        new["level"], new["Z"], new["flags"], new["numSamples"] = 7, np.arange(len(r)), r[:, 0], r[:, 1]
        new["firstSample"] = np.concatenate([[0], np.cumsum(r[:, 1])[:-1]])
        held = new[r[:, 2] != 0].copy()
        held["flags"], held["numSamples"] = r[r[:, 2] != 0, 3], r[r[:, 2] != 0, 4]
        held["firstSample"] = np.concatenate([[0], np.cumsum(held["numSamples"].astype(np.int64))[:-1]])
        box = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        d = delta_between(OctreeExport(new, np.zeros(int(r[:, 1].sum()), abi.point_dtype), *box), OctreeExport(held, np.zeros(int(held["numSamples"].sum()), abi.point_dtype), *box),
                          tails=bool(tails))
        e = d.entries
        assert np.array_equal(got[part, 0], e["state"]) and np.array_equal(got[part, 1], e["numKept"]), f"tails {tails}"
        assert np.array_equal(e["numDelta"], new["numSamples"] - e["numKept"])
        seen |= set(e["state"].tolist())
        # the rules read back: KEPT and GROWN need a selected held entry of the same kind
        same_kind = (r[:, 2] != 0) & (((r[:, 0] ^ r[:, 3]) & LEAF) == 0) & ((r[:, 3] & SEL) != 0)
        assert not ((e["state"] == abi.DELTA_KEPT) & ~(same_kind & (r[:, 4] == r[:, 1]) & (r[:, 1] > 0))).any()
        assert not ((e["state"] == abi.DELTA_GROWN) & ~(same_kind & (r[:, 4] > 0) & (r[:, 4] < r[:, 1]))).any()
        assert ((e["state"] == abi.DELTA_GROWN).any()) == bool(tails)
        assert ((e["state"] == abi.DELTA_NONE) == ((r[:, 0] & SEL) == 0)).all()
    assert seen == {abi.DELTA_NONE, abi.DELTA_KEPT, abi.DELTA_GROWN, abi.DELTA_ADDED}


def test_refusals(checker, tmp_path):
    calls = [(0, 0, 5, 0, 3, 1), (1, 0, 5, 0, 3, 1), (0, 1, 0, 1, 0, 1), (1, 0, 0, 0, 0, 1), (0, 0, 5, 1, 0, 1),
             (2, 0, 5, 0, 3, 0), (0x80000001, 0, 5, 0, 3, 0), (0, 1, 1, 0, 3, 0), (0, 0, 5, 1, 1, 0), (3, 1, 0, 1, 0, 0)]
    _, _, got = _run(checker, tmp_path, np.zeros(0, abi.export_node_dtype), np.zeros((0, 4)), np.zeros((0, 6)), [c[:5] for c in calls])
    assert got.tolist() == [c[5] for c in calls]
