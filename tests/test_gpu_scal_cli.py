"""GPU, end to end: evaluate() with set-level calibration enabled on the tiny fixture probe of tests/test_gpu_probe.py (linear, GP and
ensemble heads, with and without a temperature) against tests/scal_ref.py applied to the probe's own logits; the switch off changes
neither the result nor the calls; then run_linear_probe.main --eval --set_calibration and one corruption set on the small image folder
of tests/test_gpu_calib_cli.py."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import scal_ref as sr
from test_gpu_calib_cli import CALIB_LINE, _image_tree, _pretraining_checkpoint
from test_gpu_detect import make_probe
from test_gpu_probe import case      # noqa: F401  (a fixture)
from test_gpu_scal import SETTINGS, SUM_TOL, L, close, softmax_into_store      # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SET_CAL_LINE = re.compile(r"^\* Set ECE (\S+) MCE (\S+) OE (\S+) NLL (\S+) Brier (\S+) SCE (\S+) ACE (\S+) TACE (\S+) AUROC (\S+) on (\d+) images "
                          r"\((\d+) classes with an AUROC\)$", re.M)
KEYS = ("ECE", "MCE", "OE", "NLL", "Brier", "SCE", "ACE", "TACE", "AUROC")


def batches_of(case, sizes=(5, 4, 3)):
    """Ragged labelled batches of the fixture's images, as the prefetcher hands them over: ((images, mask), labels on the host)."""
    images = case[5]
    g = torch.Generator().manual_seed(3)
    out, at = [], 0
    for n in sizes:
        x = images[[(at + i) % len(images) for i in range(n)]]
        x = x + 0.25 * torch.randn(x.shape, generator=g)                        # the fixture holds few images: make every row its own
        out.append(((x.cuda(), None), torch.randint(0, 10, (n,), generator=g)))
        at += n
    return out


def check_stats(L, sc, z, y, what):
    """stats["set_calibration"] against the restatement on the fp32 softmax of the probe's own logits z."""
    p = softmax_into_store(L, np.ascontiguousarray(z, dtype=np.float32), z.shape[1]).cpu().numpy()
    ref = sr.metrics(p, y, **SETTINGS)
    close([sc[k] for k in KEYS], [ref[k] for k in KEYS], SUM_TOL, "sum", (what, "named"))
    close([sc["acc"], sc["mean_conf"]], [ref["acc"], ref["mean_conf"]], SUM_TOL, "sum", (what, "acc, conf"))
    assert (sc["auroc_classes"], sc["n"], sc["n_bad"]) == (int(ref["auroc_classes"]), len(y), 0)
    close(np.array(sc["reliability"]), ref["top_table"], SUM_TOL, "sum", (what, "reliability"))
    for i, k in enumerate(("SCE", "ACE", "TACE", "AUROC", "n_pos", "n_over_threshold")):
        close(np.array(sc["per_class"][k]), ref["per_class"][:, i], SUM_TOL, "sum", (what, k))


@pytest.mark.parametrize("kind", ["linear", "gp", "ens"])
def test_evaluate_with_the_switch(L, case, kind):
    probe = make_probe(case, kind)
    batches = batches_of(case)
    y = torch.cat([b[1] for b in batches]).numpy()
    plain = probe.evaluate(batches)
    assert "set_calibration" not in plain
    probe.enable_set_calibration()
    stats = probe.evaluate(batches)
    sc = stats.pop("set_calibration")
    np.testing.assert_equal(stats, plain)                                       # everything else is what it was
    z = torch.cat([probe.logits(b[0][0]) for b in batches]).cpu().numpy()
    check_stats(L, sc, z, y, kind)
    np.testing.assert_equal(probe.evaluate(batches)["set_calibration"], sc)     # the same numbers on a second evaluation
    # temperature 2: the store is written behind uvit_op_ts_scale, which multiplies by 0.5 exactly
    hot = probe.evaluate(batches, temperature=2.0)
    check_stats(L, hot["set_calibration"], z * np.float32(0.5), y, (kind, "T = 2"))
    assert hot["set_calibration"]["NLL"] != sc["NLL"]
    probe.set_set_calibration(None)
    np.testing.assert_equal(probe.evaluate(batches), plain)


def test_switch_off_leaves_the_calls_as_they_were(case):
    """The libuvit calls of evaluate(), by name and in order: the same before the switch was ever on and after it went off; while on,
    one uvit_op_scal_probs per batch, one workspace query and one uvit_op_scal_metrics are all that is added."""
    from uncertainty_vit_amd import native
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from record_probe_trace import Recorder
    probe = make_probe(case, "linear")
    batches = batches_of(case)
    probe.evaluate(batches)                                                     # buffers grow here, outside the recording
    real = native.lib()

    def names():
        rec = Recorder(real)
        native._lib = rec
        try:
            probe.evaluate(batches)
        finally:
            native._lib = real
        return rec.names

    before = names()
    probe.enable_set_calibration()
    on = names()
    probe.set_set_calibration(None)
    assert names() == before
    added = [n for n in on if n.startswith("uvit_op_scal")]
    assert [n for n in on if not n.startswith("uvit_op_scal")] == before
    assert added == ["uvit_op_scal_probs"] * 3 + ["uvit_op_scal_ws_bytes", "uvit_op_scal_metrics"]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("scal_cli")
    val, ckpt = root / "val", root / "checkpoint-0.pth"
    _image_tree(str(val), 6)
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(val),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--eval"]
    return root, argv


def test_cli_eval_with_set_calibration(setup, capsys):
    import run_linear_probe as rlp
    root, argv = setup
    out = root / "out"
    out.mkdir()
    stats = rlp.main(rlp.get_args(argv + ["--output_dir", str(out), "--set_calibration", "--calibration", "--scal_ece_bins", "10"]))
    text = capsys.readouterr().out
    lines = text.splitlines()
    m, c = SET_CAL_LINE.search(text), CALIB_LINE.search(text)
    assert m and c and lines.index(m.group(0)) == lines.index(c.group(0)) + 1                  # behind the `* ECE` line
    sc = stats["set_calibration"]
    assert sc["n"] == 6 and int(m.group(10)) == 6 and int(m.group(11)) == sc["auroc_classes"] == 3 and sc["n_bad"] == 0
    for k, shown in zip(KEYS, m.groups()[:9]):
        assert f"{sc[k]:.5f}" == shown and np.isfinite(sc[k])
    # a head that starts at 1e-3 x N(0, 0.02): p = 1 / 3 everywhere up to 1e-4, so NLL = log 3 and Brier = 2 / 3
    assert abs(sc["NLL"] - np.log(3.0)) < 0.05 and abs(sc["Brier"] - 2.0 / 3.0) < 0.05 and len(sc["reliability"]) == 10
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1 and all(log[0][f"test_set_{k}"] == sc[k] for k in KEYS) and log[0]["test_set_reliability"] == sc["reliability"]
    rel = json.load(open(out / "reliability.json"))
    assert rel["reliability"] == sc["reliability"] and rel["per_class"] == sc["per_class"] and rel["n"] == 6


def test_cli_corruption_set_carries_the_set_entries(setup, capsys):
    import run_linear_probe as rlp
    root, argv = setup
    out = root / "out_c"
    out.mkdir()
    stats = rlp.main(rlp.get_args(argv + ["--output_dir", str(out), "--set_calibration", "--corruptions", "brightness",
                                          "--corruption_severities", "1"]))
    text = capsys.readouterr().out
    assert len(SET_CAL_LINE.findall(text)) == 2                                                # the evaluation and the one set
    sev = [ln for ln in text.splitlines() if ln.startswith("* Severity 1 ")]
    assert len(sev) == 1 and re.search(r" set-ECE \S+ Brier \S+$", sev[0])
    st = stats["corruptions"]["sets"][("brightness", 1)]["set_calibration"]
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 3                                                                        # the evaluation, the set, the summary
    assert all(log[1][f"test_c_brightness_1_set_{k}"] == st[k] for k in KEYS)
    summary = stats["corruptions"]["summary"]
    assert all(log[2][f"test_c_severity_set_{k}"] == summary[f"set_{k}"] == [st[k]] for k in ("ECE", "NLL", "Brier"))
