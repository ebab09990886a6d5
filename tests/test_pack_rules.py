"""CPU tier of the packed samples' shared rules (include/simlod_hip.h, "packed samples"): simlod_amd/csrc/pack_rules.hpp — the box a call accepts,
the ranges of rule K5, the records of rules K0-K4, their decode and the counts — checked on the host by a program of its own
(tests/host/pack_rules_check.cpp, built with the address and undefined-behaviour sanitizers) against octree_io.pack_samples / unpack_samples, byte
for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import pack_ref as kr
from simlod_amd import abi
from simlod_amd.octree_io import pack_samples, unpack_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("pack_rules") / "pack_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "pack_rules_check.cpp"), "-o", exe])
    return exe


def _run(checker, tmp_path, table, samples, mn, mx, entries=None):
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.array([len(table), 0 if entries is None else 1], "<u4").tobytes() + np.array([len(samples)], "<u8").tobytes())
        f.write(np.asarray(mn, "<f4").tobytes() + np.asarray(mx, "<f4").tobytes())
        f.write(np.ascontiguousarray(table).tobytes())
        if entries is not None:
            f.write(np.ascontiguousarray(entries).tobytes())
        f.write(np.ascontiguousarray(samples).tobytes())
    run = subprocess.run([checker, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.uint8)
    n = len(samples)
    assert raw.size == 1 + 8 * n + 40 + 16 * n + 40
    o = 1
    packed = raw[o: o + 8 * n].view(np.uint64); o += 8 * n
    pc = raw[o: o + 40].view(abi.pack_counts_dtype)[0]; o += 40
    back = raw[o: o + 16 * n].view(abi.point_dtype); o += 16 * n
    uc = raw[o: o + 40].view(abi.pack_counts_dtype)[0]
    return bool(raw[0]), packed, pc, back, uc


def _box(where):
    box = (1.0, 1.0, 1.0) if where == "origin" else (600.0, 400.0, 40.0)
    mn = np.zeros(3, np.float32) if where == "origin" else np.asarray(cases.GEOREF, np.float32)
    return mn, (mn + np.asarray(box, np.float32)).astype(np.float32)


@pytest.mark.parametrize("where", ["origin", "georef"])
def test_header_packs_as_the_mirror_does(checker, tmp_path, where):
    """The hand table with its trouble, on a unit box at the origin and on the 600 x 400 x 40 box at cases.GEOREF: packed words, unpacked samples and
    both counts records equal the mirror's byte for byte; the same with delta entries that take a part of every range."""
    mn, mx = _box(where)
    table = kr.the_hand_table()
    samples, trouble = kr.hand_samples(table, mn, mx)
    ok, packed, pc, back, uc = _run(checker, tmp_path, table, samples, mn, mx)
    want, wc = pack_samples(table, samples, mn, mx)
    assert ok and packed.tobytes() == want.tobytes() and pc.tobytes() == wc.tobytes()
    wback, wuc = unpack_samples(table, want | np.uint64(1 << 63), mn, mx)
    assert back.tobytes() == wback.tobytes() and uc.tobytes() == wuc.tobytes()
    assert int(pc["numClamped"]) >= 5 and int(pc["numInexact"]) >= 1 and int(pc["numAlpha"]) == 2 and int(pc["error"]) == 0
    assert int(pc["numSamples"]) == len(samples) == int(uc["numSamples"]) and not int(uc["numClamped"]) and not int(uc["numAlpha"])
    # delta entries: every third entry NONE, the others keep a head and send the rest
    entries = np.zeros(len(table), dtype=abi.delta_entry_dtype)
    n = table["numSamples"].astype(np.int64)
    entries["state"] = np.where(np.arange(len(table)) % 3 == 0, abi.DELTA_NONE, np.where(n > 300, abi.DELTA_GROWN, abi.DELTA_ADDED))
    entries["numKept"] = np.where(entries["state"] == abi.DELTA_GROWN, 300, 0)
    entries["numDelta"] = np.where(entries["state"] == abi.DELTA_NONE, 0, n - entries["numKept"])
    entries["firstDelta"] = np.concatenate([[0], np.cumsum(entries["numDelta"].astype(np.int64))[:-1]])
    delta = samples[: int(entries["numDelta"].astype(np.int64).sum())]
    ok, packed, pc, back, uc = _run(checker, tmp_path, table, delta, mn, mx, entries)
    want, wc = pack_samples(table, delta, mn, mx, entries)
    wback, wuc = unpack_samples(table, want | np.uint64(1 << 63), mn, mx, entries)
    assert ok and packed.tobytes() == want.tobytes() and pc.tobytes() == wc.tobytes() and back.tobytes() == wback.tobytes() and uc.tobytes() == wuc.tobytes()
    assert 0 < int(pc["numSamples"]) == len(delta)


def test_capacity_and_level_errors_as_the_mirror(checker, tmp_path):
    """Rule K7: a sample array one short of the last entry's end — that entry writes nothing, the others are complete — and an entry with level 21."""
    mn, mx = _box("origin")
    table = kr.the_hand_table()
    samples, _ = kr.hand_samples(table, mn, mx)
    short = samples[:-1]
    ok, packed, pc, back, uc = _run(checker, tmp_path, table, short, mn, mx)
    want, wc = pack_samples(table, short, mn, mx)
    last = int(table["numSamples"][-1])
    assert ok and int(pc["error"]) == abi.EXPORT_ERR_CAPACITY == int(uc["error"]) and int(pc["numSamples"]) == len(samples) - last
    assert packed.tobytes() == want.tobytes() and pc.tobytes() == wc.tobytes() and not packed[-(last - 1):].any() and packed[: len(samples) - last].all()
    assert back.tobytes() == unpack_samples(table, want, mn, mx)[0].tobytes()
    deep = table.copy()
    deep["level"][-1] = 21
    ok, packed, pc, _, _ = _run(checker, tmp_path, deep, samples, mn, mx)
    want, wc = pack_samples(deep, samples, mn, mx)
    assert ok and int(pc["error"]) == abi.EXPORT_ERR_NODE_COUNT and packed.tobytes() == want.tobytes() and pc.tobytes() == wc.tobytes()
    assert not packed[-last:].any()


def test_header_refuses_what_the_mirror_refuses(checker, tmp_path):
    """The argument check on the box: a corner that is not finite and a box without extent are refused by both; a box flat on two axes is not."""
    table = kr.the_hand_table()[:1].copy()
    table["childMask"], table["firstChild"], table["numSamples"] = 0, abi.EXPORT_NONE, 1
    samples = np.zeros(1, dtype=abi.point_dtype)
    for mn, mx, good in (((0, 0, 0), (1, 1, 1), True), ((0, 0, 0), (0, 0, 2), True), ((0, 0, 0), (0, 0, 0), False), ((1, 1, 1), (0, 0, 0), False),
                         ((np.nan, 0, 0), (1, 1, 1), False), ((0, 0, 0), (1, np.inf, 1), False), ((-3e38, 0, 0), (3e38, 1, 1), False),
                         ((0, -np.inf, 0), (1, 1, 1), False)):
        ok, packed, pc, back, uc = _run(checker, tmp_path, table, samples, mn, mx)
        assert ok == good, (mn, mx)
        if good:
            assert packed.tobytes() == pack_samples(table, samples, mn, mx)[0].tobytes()
        else:
            with pytest.raises(ValueError):
                pack_samples(table, samples, mn, mx)
            with pytest.raises(ValueError):
                unpack_samples(table, np.zeros(1, np.uint64), mn, mx)
            assert not packed.any() and not back.view(np.uint8).any() and not pc.tobytes().strip(b"\0") and not uc.tobytes().strip(b"\0")
    ok = _run(checker, tmp_path, table[:0], samples[:0], (0, 0, 0), (1, 1, 1))[0]
    assert not ok
    with pytest.raises(ValueError):
        pack_samples(table[:0], samples[:0], (0, 0, 0), (1, 1, 1))
