"""CPU tier of the cluster queries' shared rules (include/simlod_hip.h, "cluster queries"): simlod_amd/csrc/cluster_rules.hpp — which
SimlodClusterParams records a call accepts, rule K3's core test, rule K9's size bin and colour index, and the lock-free union-find
(cluster_find, cluster_link, cluster_root) under a std::atomic memory policy — checked on the host by a program of its own
(tests/host/cluster_rules_check.cpp, plain g++, run as a host binary with nothing preloaded) against tests/cluster_ref.py, line by line.  The
union-find runs the link lists of `chain`, `hot_cell` and `singletons` serially in five orders and from eight threads; the final root array
must equal the per-component minimum every time.  The program is built plain, with the address and undefined-behaviour sanitizers, and with
the thread sanitizer for the threaded part."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cluster_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = ["chain", "hot_cell", "singletons"]
SERIAL_RUNS, THREAD_RUNS = 5, 3


def _records():
    good = [kr.params(0.5), kr.params(0.0, 1, 1), kr.params(-0.0, 7, 3), kr.params(3.0e38, 0xFFFFFFFF, 0xFFFFFFFF, budget=(1 << 64) - 1, wg=0xFFFFFFFF)]
    bad = [(kr.params(-1.0), "radius < 0"), (kr.params(np.nan), "radius NaN"), (kr.params(np.inf), "radius inf"), (kr.params(-np.inf), "radius -inf"),
           (kr.params(1.0, 0, 1), "minNeighbours 0"), (kr.params(1.0, 1, 0), "minClusterSize 0"), (kr.params(1.0, reserved=1), "reserved"),
           (kr.params(1.0, reserved=0x80000000), "reserved high bit")]
    return good, bad


def _build(tmp, flags, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", *flags,
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "cluster_rules_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    """-> (the input file, the lines the serial part must print before the union-find's, the number of lists)"""
    good, bad = _records()
    records = good + [r for r, _ in bad]
    core = [(w, m) for m in (1, 2, 8, 0xFFFFFFFF) for w in (0, 1, 2, 7, 8, 9, 0xFFFFFFFE, 0xFFFFFFFF)]
    sizes = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 0xFFFFFFFE, 0xFFFFFFFF]
    clusters = [0, 1, 255, 256, 257, 511, 512, 65536 + 3, 0xFFFFFFFE]
    path = tmp_path_factory.mktemp("cluster_rules") / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(records), len(core), len(sizes), len(clusters), len(LISTS), 0], "<u4").tobytes())
        f.write(np.concatenate(records).tobytes())
        f.write(np.array(core, "<u4").tobytes())
        f.write(np.array(sizes, "<u4").tobytes())
        f.write(np.array(clusters, "<u4").tobytes())
        for name in LISTS:
            rec, _, summary, links = kr.exact(name)
            assert int(summary["numNoise"]) == 0 or name == "singletons"
            want = np.where(rec["root"] == kr.MISS, np.arange(len(rec)), rec["root"]).astype("<u4")       # (no sample of these is a border sample)
            assert int(summary["numBorder"]) == 0 and len(links) > 0 and all(i > j for i, j in links)
            f.write(np.array([len(rec), len(links)], "<u4").tobytes())
            f.write(want.tobytes())
            f.write(np.array(links, "<u4").tobytes())
    want = []
    for i, r in enumerate(records):
        ok = kr.record_acceptable(r)
        assert ok == (i < len(good)), (["ok"] * len(good) + [w for _, w in bad])[i]
        want.append(f"p {i:x} {int(ok):x}")
    want += [f"c {w:x} {m:x} {int(kr.is_core(w, m)):x}" for w, m in core]
    want += [f"b {s:x} {kr.size_bin(s):x} {int(s >= 5):x}" for s in sizes]
    want += [f"i {c:x} {kr.colour_index(c):x}" for c in clusters]
    want.append(f"k {(7 << 32) | 0xFFFFFFFF:x} {(7 << 32) | 0xFFFFFFFC:x}")
    assert {kr.size_bin(s) for s in sizes} >= {0, 1, 2, 3, 7, 8, 15, 16, 30, 31}
    return str(path), want


def _union_lines(what_runs):
    return [f"u {k:x} {what} 0 1 1" for k in range(len(LISTS)) for what, n in what_runs for _ in range(n)]


def _run(exe, path, mode):
    run = subprocess.run([exe, path, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.split("\n")
    assert lines.pop() == ""
    return lines


SERIAL = [("forward", 1), ("reverse", 1), ("shuffled", 3)]


def test_header_agrees_with_the_reference_plain(cases_file, tmp_path):
    path, want = cases_file
    lines = _run(_build(tmp_path, [], "plain"), path, "both")
    want = want + _union_lines(SERIAL + [("threads", THREAD_RUNS)])
    assert lines == want, [(a, b) for a, b in zip(lines, want) if a != b][:5]


def test_header_agrees_with_the_reference_under_asan_ubsan(cases_file, tmp_path):
    path, want = cases_file
    lines = _run(_build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "asan"), path, "both")
    want = want + _union_lines(SERIAL + [("threads", THREAD_RUNS)])
    assert lines == want, [(a, b) for a, b in zip(lines, want) if a != b][:5]


def test_threaded_links_under_the_thread_sanitizer(cases_file, tmp_path):
    """Eight threads on one parent array, every access an atomic: the thread sanitizer has nothing to report and the roots are the minima."""
    path, _ = cases_file
    lines = _run(_build(tmp_path, ["-fsanitize=thread"], "tsan"), path, "threads")
    assert lines == _union_lines([("threads", THREAD_RUNS)])
