"""GPU, end to end: run_linear_probe.main --eval --ts_data_path ... --calibration on the small image folders and the checkpoint of
tests/test_gpu_calib_cli.py: beit_base_patch16_224 cut after block 0, 6 validation and 9 calibration images in 3 classes."""
import json
import re

import pytest

from test_gpu_calib_cli import _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

TS_LINE = re.compile(r"^\* Temperature (\d+\.\d{5}) NLL (\d+\.\d{5}) -> (\d+\.\d{5}) on (\d+) calibration images \((\d+) passes, "
                     r"(converged|clamped at T_max|clamped at T_min|iteration limit)\)$", re.M)
WORDS = ("converged", "clamped at T_max", "clamped at T_min", "iteration limit")


def test_cli_eval_with_a_fitted_and_a_given_temperature(tmp_path, capsys):
    pytest.importorskip("PIL")
    import run_linear_probe as rlp
    val, cal, out, ckpt = tmp_path / "val", tmp_path / "cal", tmp_path / "out", tmp_path / "checkpoint-0.pth"
    _image_tree(str(val), 6)
    _image_tree(str(cal), 9)
    out.mkdir()
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(val),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--output_dir", str(out),
            "--eval"]
    stats = rlp.main(rlp.get_args(argv + ["--ts_data_path", str(cal), "--calibration"]))
    text = capsys.readouterr().out
    lines = text.splitlines()
    m = TS_LINE.search(text)
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    assert m and len(TS_LINE.findall(text)) == 1 and len(acc) == 1 and lines[acc[0] - 1] == m.group(0)      # directly in front of * Acc@1
    fit = stats["temperature_fit"]
    assert m.groups() == (f"{fit['T']:.5f}", f"{fit['nll_before']:.5f}", f"{fit['nll_after']:.5f}", str(fit["n"]), str(fit["iterations"]),
                          WORDS[fit["status"]])
    assert fit["n"] == 9 and stats["temperature"] == fit["T"] and fit["nll_after"] <= fit["nll_before"] + 1e-6
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1 and set(log[0]) == {"test_loss", "test_acc1", "test_acc5", "test_ECE", "test_TACE", "test_NLL", "test_AUROC",
                                             "test_ts_temperature", "test_ts_nll_before", "test_ts_nll_after", "test_ts_n",
                                             "test_ts_iterations", "test_ts_status"}
    assert log[0]["test_ts_temperature"] == fit["T"] and log[0]["test_ts_n"] == 9 and log[0]["test_ts_status"] == fit["status"]
    assert log[0]["test_ts_nll_before"] == fit["nll_before"] and log[0]["test_ts_nll_after"] == fit["nll_after"]

    plain = rlp.main(rlp.get_args(argv + ["--calibration"]))
    text = capsys.readouterr().out
    assert "Temperature" not in text and "temperature" not in plain and "temperature_fit" not in plain
    assert plain["correct1"] == stats["correct1"] and plain["correct5"] == stats["correct5"] and plain["n"] == stats["n"] == 6
    assert set(json.loads(open(out / "log.txt").readlines()[1])) == {"test_loss", "test_acc1", "test_acc5", "test_ECE", "test_TACE", "test_NLL",
                                                                     "test_AUROC"}

    given = rlp.main(rlp.get_args(argv + ["--ts_temperature", "2.0"]))
    text = capsys.readouterr().out
    assert given["temperature"] == 2.0 and "* Temperature" not in text and given["correct1"] == plain["correct1"]
    assert json.loads(open(out / "log.txt").readlines()[2]) == {"test_loss": given["loss"], "test_acc1": given["acc1"], "test_acc5": given["acc5"],
                                                                "test_ts_temperature": 2.0}
