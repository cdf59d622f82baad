"""GPU, end to end: run_linear_probe.main --eval --detection --ood_data_path on the small image folders of tests/test_gpu_calib_cli.py
(its helpers are imported): beit_base_patch16_224 cut after block 0, a checkpoint of two blocks, 6 validation images in 3 classes and
5 images of another folder."""
import json
import re

import numpy as np
import pytest

from test_gpu_calib_cli import _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

NUM = r"(-?\d+\.\d{5}|nan)"
MIS_LINE = re.compile(r"^\* Detect misclassification (\S+) AUROC " + NUM + " AUPR " + NUM + " FPR95 " + NUM + " AURC " + NUM + "$", re.M)
OOD_LINE = re.compile(r"^\* Detect OOD (\S+) AUROC " + NUM + " AUPR " + NUM + " FPR95 " + NUM + "$", re.M)
COLUMNS = ["msp", "entropy", "energy"]


def test_cli_eval_with_detection_and_ood(tmp_path, capsys):
    pytest.importorskip("PIL")
    import run_linear_probe as rlp
    val, ood, out, ckpt = tmp_path / "val", tmp_path / "ood", tmp_path / "out", tmp_path / "checkpoint-0.pth"
    _image_tree(str(val), 6)
    _image_tree(str(ood), 5)
    out.mkdir()
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(val),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--output_dir", str(out),
            "--eval", "--detection", "--ood_data_path", str(ood)]
    stats = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    lines = text.splitlines()
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    assert len(acc) == 1
    mis, oods = MIS_LINE.findall(text), OOD_LINE.findall(text)
    assert [m[0] for m in mis] == COLUMNS and [m[0] for m in oods] == COLUMNS
    assert lines[acc[0] + 1:acc[0] + 7] == [ln for ln in lines if ln.startswith("* Detect")]       # behind the existing line, in order
    det = stats["detection"]
    assert det["columns"] == COLUMNS and (det["n"], det["n_ood"]) == (6, 5) and det["n_wrong"] == 6 - stats["correct1"]
    for row, kind, keys in [(m, "misclassification", ("AUROC", "AUPR", "FPR95", "AURC")) for m in mis] + [(m, "ood", ("AUROC", "AUPR", "FPR95")) for m in oods]:
        for key, shown in zip(keys, row[1:]):
            assert f"{det[kind][row[0]][key]:.5f}" == shown
    # 6 and 5 different random images: both classes of the OOD question are present, every OOD figure is a number in [0, 1]
    assert all(0.0 <= det["ood"][c][k] <= 1.0 for c in COLUMNS for k in ("AUROC", "AUPR", "FPR95"))
    if 0 < det["n_wrong"] < 6:
        assert all(0.0 <= det["misclassification"][c][k] <= 1.0 for c in COLUMNS for k in ("AUROC", "AUPR", "FPR95", "AURC"))
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1
    want = {f"test_mis_{c}_{k}" for c in COLUMNS for k in ("AUROC", "AUPR", "FPR95", "AURC")} | {f"test_ood_{c}_{k}" for c in COLUMNS for k in ("AUROC", "AUPR", "FPR95")}
    assert want | {"test_loss", "test_acc1", "test_acc5"} == set(log[0])
    for c in COLUMNS:
        for k in ("AUROC", "AUPR", "FPR95"):
            assert log[0][f"test_ood_{c}_{k}"] == det["ood"][c][k]
            a, b = log[0][f"test_mis_{c}_{k}"], det["misclassification"][c][k]
            assert a == b or (np.isnan(a) and np.isnan(b))
