"""GPU, end to end: what run_linear_probe.main prints, writes into log.txt and --output_dir, returns and calls in libuvit, per command
line, against tests/golden/probe_cli_transcript.json (written by tools/record_probe_cli.py, which also defines the scenarios and what
the record leaves out: the digits).  main() may be rearranged; its lines, their order, log.txt's keys and the native calls may not
change without the golden being recorded again on purpose."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from record_probe_cli import SCENARIOS, record      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    pytest.importorskip("PIL")
    return str(tmp_path_factory.mktemp("probe_cli_transcript"))      # the inputs are drawn by the first scenario and shared


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "probe_cli_transcript.json")) as f:
        return json.load(f)


def test_the_golden_holds_the_scenarios(golden):
    assert sorted(golden) == sorted(SCENARIOS) and all(len(golden[name]) == len(SCENARIOS[name]) for name in SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_every_command_line_leaves_the_recorded_transcript(name, root, golden):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    got = record([name], root=root)[name]
    for i, (have, want) in enumerate(zip(got, golden[name])):
        for key in want:
            assert have[key] == want[key], f"{name}, call {i}: {key} differs from the recorded one"
        assert sorted(have) == sorted(want) and any(n.startswith("uvit_op_") for n in want["calls"]), (name, i)
