"""simlod_amd/csrc/octree_state.hpp — the per-octree record, its registry and the launch sizing — checked on the host by a program of its own
(tests/host/octree_state_check.cpp: the sizing table row by row, the registry's rules), built with the address and undefined-behaviour sanitizers and run
as a child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_octree_state_header_holds_its_sizing_table_and_registry_rules(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "octree_state_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), os.path.join(ROOT, "tests", "host", "octree_state_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
