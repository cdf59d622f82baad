"""GPU, end to end: run_linear_probe.main --het_layer on a small image folder, as tests/test_gpu_gp_cli.py runs the GP head:
beit_base_patch16_224 cut after block 0 (--target_layer 0), a checkpoint of two blocks, 12 images in 3 classes, 2 factors, 40 samples."""
import json
import math

import pytest
import torch

from test_gpu_probe_cli import _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

R = 2
SHAPES = {"head._loc_layer.weight": (3, 768), "head._loc_layer.bias": (3,), "head._diag_layer.weight": (3, 768), "head._diag_layer.bias": (3,),
          "head._scale_layer.weight": (3 * R, 768), "head._scale_layer.bias": (3 * R,)}


def _setup(tmp_path):
    pytest.importorskip("PIL")
    train, val, out, ckpt = tmp_path / "train", tmp_path / "val", tmp_path / "out", tmp_path / "checkpoint-0.pth"
    _image_tree(str(train), 12)
    _image_tree(str(val), 6)
    out.mkdir()
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(train),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--epochs", "2",
            "--warmup_epochs", "0", "--lr", "1e-3", "--clip_grad", "1.0", "--output_dir", str(out), "--het_layer", "--het_num_factors", str(R),
            "--het_train_mc_samples", "40", "--het_test_mc_samples", "40"]
    return argv, out


def test_cli_het_trains_evaluates_and_resumes(tmp_path, capsys):
    import run_linear_probe as rlp
    argv, out = _setup(tmp_path)
    last = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "encoder: 1 blocks" in text and all(k in text for k in SHAPES)
    assert text.count("* Het variance mean ") == 2 and text.index("* Acc@1") < text.index("* Het variance mean ")
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert [e["epoch"] for e in log] == [0, 1]
    for e in log:
        assert math.isfinite(e["train_loss"]) and math.isfinite(e["test_loss"])
        assert math.isfinite(e["test_het_var_mean"]) and e["test_het_var_mean"] > 0.0
    print(f"\nhet_var_mean per epoch {[e['test_het_var_mean'] for e in log]}, loss {last['loss']:.4f}")
    assert last["n"] == 6 and last["het_var_mean"] == log[1]["test_het_var_mean"]
    saved = torch.load(out / "probe-1.pth", map_location="cpu", weights_only=False)
    assert {k: tuple(v.shape) for k, v in saved["model"].items()} == SHAPES
    assert saved["optimizer"]["step"] == 6 and sorted(saved["optimizer"]["exp_avg"]) == sorted(SHAPES)

    # --eval with the saved head: the evaluation's draws come from the fixed seed and the kernels fix their summation order, so the
    # figures of the last epoch come back bit for bit
    resume = argv + ["--eval", "--resume", str(out / "probe-1.pth")]
    again = rlp.main(rlp.get_args(resume))
    text = capsys.readouterr().out
    assert "* Acc@1" in text and "* Het variance mean " in text and "Epoch" not in text
    assert (again["n"], again["correct1"], again["correct5"]) == (6, last["correct1"], 6)
    assert again["loss"] == last["loss"] and again["het_var_mean"] == last["het_var_mean"]
    entry = json.loads(open(out / "log.txt").readlines()[-1])
    assert entry["test_het_var_mean"] == last["het_var_mean"] and "epoch" not in entry

    # another seed moves the evaluation's draws, and so the loss
    other = rlp.main(rlp.get_args(resume + ["--het_seed", "7"]))
    capsys.readouterr()
    assert other["loss"] != last["loss"]
