"""The host side of chained construct launches (simlod_launch_construct_chain; simlod_amd/csrc/octree_state.hpp): how a chain is sized, how many groups of
kernels it enqueues per segment, and where a chain is cut into several device launches.  Checked by a program of its own (tests/host/chain_plan_check.cpp),
built with the address and undefined-behaviour sanitizers and run as a child process.

The rows, worked by hand (L = the context's batch limit, 20 unless said; a chain of n launches is sized as ONE launch with limit n x L):

Sizing
  S1  told counter.  Reset through the library, not yet reported; the host has published 36.  pending = 36 - 0, nothing in flight: a chain of 2 (cap 40) is
      sized 36, a chain of 3 (cap 60) too.  50 published, chain of 2: min(50, 40) = 40; the launch behind it: 50 - 0 - 40 in flight = 10.
  S2  hint.  A hint wins and may name up to n x L: 36 of 40 -> 36; 50 -> 40.  L = 7, chain of 3 (cap 21): 20 -> 20, 25 -> 21.
  S3  reports only.  The reset reported (0, 0), one launch reported index 20 with 50 seen uploaded: pending 30; a single report says nothing about the
      uploader's pace, so arrivals = 20 and want = 50.  Chain of 2: min(50, 40) = 40.  Chain of 3: 50.
  S4  a silent host right after a reset (nothing reported, nothing told): nothing is known, the chain is sized for its cap — 40, 60; L = 7, chain of 3: 21.
      One launch stays 20.
  S5  a chain that goes launch by launch (take == 1) turns into the plan of its first launch: sized 36 -> 20, the history remembers 20, and the launch
      behind it finds 36 - 20 = 16.

Groups = sum over segments of ceil(segment / take); no group straddles a segment boundary
  21 by 5: 5,5,5,5 | 1 = 5          36 by 5: 5,5,5,5 | 5,5,5,1 = 8      41 by 5: 4 | 4 | 1 = 9        50 by 5: 4 | 4 | 5,5 = 10
  20 by 5: 4                         L = 7, 20 by 5: 5,2 | 5,2 | 5,1 = 6  50 by 2: 10 | 10 | 5 = 25     12 by 5: 5,5,2 = 3      0: 0
  coalesced 36 by 10: 10,10 | 10,6 = 4;  36 by 3: 7 | 6 = 13;  13 by 5 in one launch: ceil(13 / 5) = 3, as before chains;  36 by 1: 36
  plain launches: take == 1, or at most one group (5 by 5; 0) — not 6 by 5, not 36 by 5.

The ordinal cut (group ordinals index tables of 20): segments per device launch = floor(20 / groups per whole segment), at least 1
  take 5: 4 groups -> 5      take 2: 10 -> 2      take 3: 7 -> 2      take 12: 2 -> 10      take 20: 1 -> 20      take 1: 20 -> 1      L = 7, take 5: 2 -> 10
  SIMLOD_EXACT_GROUP=2, chain of 3 (50 batches): device launches of 2 and 1 segments, then none — 40 by 2 = 20 groups, 10 by 2 = 5.
  take 5: a chain of 3 is one device launch; a chain of 7 is 5 + 2.
  For every L and take in 1..20 a full device launch numbers at most 20 groups."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_sizing_groups_per_segment_and_ordinal_cut(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "chain_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "simlod_amd", "csrc"), os.path.join(ROOT, "tests", "host", "chain_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0, run.stdout
