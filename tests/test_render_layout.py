"""simlod_amd/csrc/render_layout.hpp — the layout of kernel_render's buffer: capacities, counter and work-word indices, FrameLayout — checked on the host
by a program of its own (tests/host/render_layout_check.cpp: regions in order and without overlap at nine sizes, the offsets as literal numbers, the pool's
capacity rule, the index enums), built with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_layout_header_holds_its_regions_table_and_pool_rule(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "render_layout_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), os.path.join(ROOT, "tests", "host", "render_layout_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
