"""GPU, end to end: run_linear_probe.main --eval --calibration on the small image folder of tests/test_gpu_probe_cli.py (with its
helpers): beit_base_patch16_224 cut after block 0, a checkpoint of two blocks, 6 validation images in 3 classes."""
import json
import re

import numpy as np
import pytest

from test_gpu_probe_cli import _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

CALIB_LINE = re.compile(r"^\* ECE (\S+) TACE (\S+) NLL (\S+) AUROC (\S+)$", re.M)


def test_cli_eval_with_and_without_calibration(tmp_path, capsys):
    pytest.importorskip("PIL")
    import run_linear_probe as rlp
    val, out, ckpt = tmp_path / "val", tmp_path / "out", tmp_path / "checkpoint-0.pth"
    _image_tree(str(val), 6)
    out.mkdir()
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(val),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--output_dir", str(out),
            "--eval"]
    plain = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "* Acc@1" in text and not CALIB_LINE.search(text) and "ECE" not in text
    assert not (out / "log.txt").exists()                          # --eval alone writes no log entry, as before
    assert set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"}

    stats = rlp.main(rlp.get_args(argv + ["--calibration"]))
    text = capsys.readouterr().out
    lines = text.splitlines()
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    m = CALIB_LINE.search(text)
    assert len(acc) == 1 and m and lines[acc[0] + 1] == m.group(0)              # the second line follows the first
    shown = [float(v) for v in m.groups()]
    assert all(np.isfinite(shown))
    # batches of 4 and 2 images in 3 classes: every metric exists; ECE, TACE and AUROC lie in [0, 1], the NLL of a head that starts at
    # 1e-3 x N(0, 0.02) is log 3
    assert all(0.0 <= v <= 1.0 for v in (shown[0], shown[1], shown[3])) and abs(shown[2] - np.log(3.0)) < 0.05
    assert all(stats[k] == plain[k] for k in plain)
    for k, v in zip(("ECE", "TACE", "NLL", "AUROC"), shown):
        assert f"{stats[k]:.5f}" == f"{v:.5f}"
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1 and all(log[0][f"test_{k}"] == stats[k] for k in ("ECE", "TACE", "NLL", "AUROC", "loss", "acc1", "acc5"))
