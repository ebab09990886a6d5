#!/usr/bin/env python3
"""Generates tests/golden/oracle_pin.npz: every scenario of tests/test_oracle_pin.py (and the live LAS case of tests/test_las.py) run on oracle/_ref — the reference's OWN
sources compiled in place as host code (oracle/Makefile, `make -C oracle ref`; needs the reference checkout at build time).
Run from the repo root:  python tests/golden/make_golden_pin.py

Keys are "<scenario>__<what>"; the tests run the same record_* functions on the restatement and compare."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import oracle  # noqa: E402
import test_las  # noqa: E402
import test_oracle_pin as pin  # noqa: E402
from cases import CASES  # noqa: E402

assert oracle.have_ref() and oracle.have_ref_las(), "oracle/_ref not built: make -C oracle ref"
out = {}
for name in CASES:
    out.update({f"build_{name}__{k}": v for k, v in pin.record_build("ref", name)[1].items()})
out.update({f"modes__{k}": v for k, v in pin.record_modes("ref")[1].items()})
out.update({f"hazards__{k}": v for k, v in pin.record_hazards("ref")[1].items()})
for variant in pin.EDGE_VARIANTS:
    out.update({f"edge_{variant}__{k}": v for k, v in pin.record_edge_case("ref", variant)[1].items()})
for name, offset in pin.OFFSET_BOXES:
    out.update({f"offset_{offset}_{name}__{k}": v for k, v in pin.record_offset_box("ref", name, offset)[1].items()})
for name, live in pin.FROZEN_CASES:
    out.update({f"frozen_{name}_{live}__{k}": v for k, v in pin.record_frozen_camera("ref", name, live).items()})
with tempfile.TemporaryDirectory() as tmp:
    out.update({f"las_live__{k}": v for k, v in test_las.record_live("ref", tmp).items()})
np.savez_compressed(pin.GOLDEN_PIN, **out)
print(len(out), "arrays,", os.path.getsize(pin.GOLDEN_PIN), "bytes")
