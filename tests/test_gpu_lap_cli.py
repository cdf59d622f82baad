"""GPU, end to end: run_linear_probe.main --eval --laplace --lap_data_path ... on a generated 10-class folder of 48 px images, 20
per class: beit_base_patch16_224 at 48 px cut after block 0, a one-block checkpoint, a head drawn here and saved as probe-0.pth."""
import json
import os
import re
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LAP_LINE = re.compile(r"^\* Laplace prior precision (\S+) \((given|marglik|marglik, grid edge)\) log-marglik (-?\d+\.\d{5}) NLL (\d+\.\d{5}) "
                      r"on (\d+) images$", re.M)
VAR_LINE = re.compile(r"^\* Laplace variance mean (\d+\.\d{6})$", re.M)


def _image_tree(root, per_class=20, classes=10, size=48):
    from PIL import Image
    rng = np.random.default_rng(23)
    for k in range(classes):
        os.makedirs(os.path.join(root, f"class{k}"), exist_ok=True)
        for i in range(per_class):
            px = np.clip(rng.normal(20 + 22 * k, 40, (size, size, 3)), 0, 255).astype(np.uint8)      # the class moves the brightness
            Image.fromarray(px).save(os.path.join(root, f"class{k}", f"img{i}.png"))


def _checkpoints(pre, head):
    """What run_cyclical.py leaves behind (utils.save_model) for a one-block ViT-B/16 at 48 px, and a linear head as probe-N.pth."""
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    torch.manual_seed(5)
    m = VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=768, depth=1, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                             norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1,
                                             use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    args = SimpleNamespace(rel_pos_bias=True, abs_pos_emb=False, layer_scale_init_value=0.1)
    torch.save({"model": m.state_dict(), "optimizer": {}, "epoch": 0, "scaler": {}, "args": args}, pre)
    w, b = 0.05 * torch.randn(10, 768), 0.1 * torch.randn(10)
    zeros = {"head.weight": torch.zeros(10, 768), "head.bias": torch.zeros(10)}
    torch.save({"model": {"head.weight": w, "head.bias": b}, "optimizer": {"step": 0, "exp_avg": zeros, "exp_avg_sq": zeros}, "epoch": 0}, head)


def _shown(text):
    lines = text.splitlines()
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    m, v = LAP_LINE.search(text), VAR_LINE.search(text)
    assert m and v and len(acc) == 1 and len(LAP_LINE.findall(text)) == 1
    assert lines[acc[0] - 2] == m.group(0) and lines[acc[0] - 1] == v.group(0)            # the two lines, directly in front of * Acc@1
    return m.groups(), v.group(1), lines[acc[0]]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The image folder and the two checkpoints, made once for the module."""
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("lap_cli")
    data, pre, head = root / "data", root / "checkpoint-0.pth", root / "probe-0.pth"
    _image_tree(str(data))
    _checkpoints(pre, head)
    return data, pre, head


def test_cli_eval_with_a_laplace_fit_a_saved_fit_and_marglik(tree, tmp_path, capsys):
    import run_linear_probe as rlp
    data, pre, head = tree
    out, out2 = tmp_path / "out", tmp_path / "out2"
    out.mkdir()
    out2.mkdir()
    argv = ["--model", "beit_base_patch16_224", "--input_size", "48", "--finetune", str(pre), "--resume", str(head), "--data_set", "image_folder",
            "--data_path", str(data), "--eval_data_path", str(data), "--nb_classes", "10", "--target_layer", "0", "--batch_size", "64",
            "--eval"]
    stats = rlp.main(rlp.get_args(argv + ["--laplace", "--lap_data_path", str(data), "--output_dir", str(out), "--detection"]))
    first = _shown(capsys.readouterr().out)
    fit = stats["laplace_fit"]
    assert first[0] == ("1", "given", f"{fit['log_marglik']:.5f}", f"{fit['nll'] / 200:.5f}", "200") and fit["n"] == 200 and fit["n_skipped"] == 0
    assert first[1] == f"{stats['lap_var_mean']:.6f}" and stats["lap_var_mean"] > 0 and stats["n"] == 200
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1 and {"test_loss", "test_acc1", "test_acc5", "test_lap_prior_precision", "test_lap_log_marglik", "test_lap_var_mean",
                              "test_mis_lap_var_AUROC", "test_mis_lap_var_AUPR", "test_mis_lap_var_FPR95", "test_mis_lap_var_AURC",
                              "test_mis_msp_AUROC"} <= set(log[0])
    assert log[0]["test_lap_prior_precision"] == 1.0 and log[0]["test_lap_var_mean"] == stats["lap_var_mean"]
    assert log[0]["test_lap_log_marglik"] == fit["log_marglik"] and stats["detection"]["columns"][-1] == "lap_var"
    saved = torch.load(out / "laplace.pth", map_location="cpu", weights_only=False)
    assert {"A", "G_sum", "sums", "prior_precision", "head_sha256"} <= set(saved) and tuple(saved["A"].shape) == (769, 769)
    assert tuple(saved["G_sum"].shape) == (10, 10) and saved["sums"].tolist()[1:] == [200.0, 0.0] and saved["prior_precision"] == 1.0

    again = rlp.main(rlp.get_args(argv + ["--laplace", "--lap_state", str(out / "laplace.pth"), "--detection"]))
    second = _shown(capsys.readouterr().out)
    assert second == first and again["lap_var_mean"] == stats["lap_var_mean"] and again["loss"] == stats["loss"]      # the same numbers

    plain = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "Laplace" not in text and set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"}
    assert abs(plain["loss"] - stats["loss"]) > 1e-4                                       # the probit link moved the logits

    ml = rlp.main(rlp.get_args(argv + ["--laplace", "--lap_data_path", str(data), "--lap_prior_precision", "marglik", "--output_dir", str(out2)]))
    third = _shown(capsys.readouterr().out)
    tau = ml["laplace_fit"]["prior_precision"]
    assert tau in np.logspace(-4.0, 8.0, 97).tolist() and third[0][0] == f"{tau:g}" and third[0][1].startswith("marglik")
    assert (third[0][1] == "marglik, grid edge") == ml["laplace_fit"]["on_grid_edge"] == (tau in (1e-4, 1e8))
    assert ml["laplace_fit"]["log_marglik"] >= fit["log_marglik"] and json.loads(open(out2 / "log.txt").readline())["test_lap_prior_precision"] == tau


def test_cli_training_with_laplace_fits_every_epoch(tree, tmp_path, capsys):
    """Without --eval, --laplace trains as a linear probe and, with --lap_data_path, every epoch's evaluation uses the fit of that
    epoch's head: two epochs print the two lines twice, with another NLL, and leave probe-N.pth (the two linear keys) and laplace.pth."""
    import run_linear_probe as rlp
    data, pre, _ = tree
    out = tmp_path / "train"
    out.mkdir()
    argv = ["--model", "beit_base_patch16_224", "--input_size", "48", "--finetune", str(pre), "--data_set", "image_folder", "--data_path", str(data),
            "--eval_data_path", str(data), "--nb_classes", "10", "--target_layer", "0", "--batch_size", "64", "--epochs", "2", "--warmup_epochs", "0",
            "--lr", "0.05", "--output_dir", str(out), "--laplace", "--lap_data_path", str(data)]
    stats = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    fits = LAP_LINE.findall(text)
    assert len(fits) == 2 and len(VAR_LINE.findall(text)) == 2 and fits[0][3] != fits[1][3] and all(f[4] == "200" for f in fits)
    assert stats["lap_var_mean"] > 0
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 2 and all({"epoch", "train_loss", "test_acc1", "test_lap_prior_precision", "test_lap_log_marglik", "test_lap_var_mean"} <= set(e)
                                 for e in log)
    assert list(torch.load(out / "probe-1.pth", map_location="cpu", weights_only=False)["model"]) == ["head.weight", "head.bias"]
    assert (out / "laplace.pth").exists()
