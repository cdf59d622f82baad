"""GPU: the libuvit calls of every probe head's entry points, by name and in order, against tests/golden/probe_call_trace.json
(written by tools/record_probe_trace.py, which also defines the scenarios).  The Python side of the probe may be rearranged; which
kernels an entry point launches, and in which order, may not change without the golden being recorded again on purpose."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_every_entry_point_makes_the_recorded_calls(golden_dir):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from record_probe_trace import HEADS, SCENARIOS, record
    with open(os.path.join(golden_dir, "probe_call_trace.json")) as f:
        want = json.load(f)
    got = record()
    assert sorted(got) == sorted(want) and len(got) == len(HEADS) * (len(SCENARIOS) - 1) + 2
    for key in sorted(want):
        assert got[key] == want[key], f"{key}: the calls differ from the recorded ones"
        assert any(name.startswith("uvit_op_") for name in want[key]), key
