"""GPU, end to end: run_linear_probe.main --gp_layer on a small image folder, as tests/test_gpu_probe_cli.py runs the linear head:
beit_base_patch16_224 cut after block 0 (--target_layer 0), a checkpoint of two blocks, 12 images in 3 classes, 64 random features."""
import json
import math

import pytest
import torch

from test_gpu_probe_cli import _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

D, RIDGE = 64, 1e-3
SHAPES = {"head.precision_matrix": (D, D), "head._gp_input_normalize_layer.weight": (768,), "head._gp_input_normalize_layer.bias": (768,),
          "head._gp_output_layer.weight": (3, D), "head._random_feature.weight": (D, 768), "head._random_feature.bias": (D,)}
TRAINABLE = ["head._gp_input_normalize_layer.weight", "head._gp_input_normalize_layer.bias", "head._gp_output_layer.weight"]


def _setup(tmp_path):
    pytest.importorskip("PIL")
    train, val, out, ckpt = tmp_path / "train", tmp_path / "val", tmp_path / "out", tmp_path / "checkpoint-0.pth"
    _image_tree(str(train), 12)
    _image_tree(str(val), 6)
    out.mkdir()
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(train),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--epochs", "2",
            "--warmup_epochs", "0", "--lr", "1e-3", "--clip_grad", "1.0", "--output_dir", str(out), "--gp_layer", "--gp_num_inducing", str(D)]
    return argv, out


def test_cli_gp_trains_evaluates_and_resumes(tmp_path, capsys):
    import run_linear_probe as rlp
    argv, out = _setup(tmp_path)
    last = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "encoder: 1 blocks" in text and f"Trainable weights: {TRAINABLE}" in text
    assert text.count("* GP variance mean ") == 2 and text.index("* Acc@1") < text.index("* GP variance mean ")
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert [e["epoch"] for e in log] == [0, 1]
    for e in log:
        assert math.isfinite(e["train_loss"]) and math.isfinite(e["test_loss"])
        assert math.isfinite(e["test_gp_var_mean"]) and e["test_gp_var_mean"] > 0.0
    assert last["n"] == 6 and last["gp_var_mean"] == log[1]["test_gp_var_mean"]
    saved = torch.load(out / "probe-1.pth", map_location="cpu", weights_only=False)
    assert {k: tuple(v.shape) for k, v in saved["model"].items()} == SHAPES
    Pm = saved["model"]["head.precision_matrix"]
    assert torch.equal(Pm, Pm.t()) and not torch.equal(Pm, RIDGE * torch.eye(D))
    assert saved["optimizer"]["step"] == 6 and sorted(saved["optimizer"]["exp_avg"]) == sorted(TRAINABLE)
    assert float((saved["model"]["head._gp_input_normalize_layer.weight"] - 1).abs().max()) > 0.0

    # --eval with the saved head: nothing is drawn at random and the kernels fix their summation order, so the figures of the last
    # epoch come back bit for bit (inv(P) is formed from the same P by the same host routine)
    resume = argv + ["--eval", "--resume", str(out / "probe-1.pth")]
    again = rlp.main(rlp.get_args(resume))
    text = capsys.readouterr().out
    assert "* Acc@1" in text and "* GP variance mean " in text and "Epoch" not in text
    assert (again["n"], again["correct1"], again["correct5"]) == (6, last["correct1"], 6)
    assert again["loss"] == last["loss"] and again["gp_var_mean"] == last["gp_var_mean"]
    entry = json.loads(open(out / "log.txt").readlines()[-1])
    assert entry["test_gp_var_mean"] == last["gp_var_mean"] and "epoch" not in entry

    # mean-field logits move the loss and leave the variance alone
    mf = rlp.main(rlp.get_args(resume + ["--gp_mean_field", "0.4"]))
    capsys.readouterr()
    assert mf["loss"] != last["loss"] and mf["gp_var_mean"] == last["gp_var_mean"]


def test_cli_gp_exact_sum_counts_one_epoch(tmp_path, capsys, monkeypatch):
    """--gp_cov_momentum 0: the saved P is ridge * I plus the sum of phi^T phi over the three steps of the last epoch, not over the six
    of both.  The sum is restated in float64 from the phi each step left on the device; bound: 4 x the error of torch's fp32 CPU
    evaluation of the same three updates against that float64 sum (max-norm over max|P|), printed."""
    import run_linear_probe as rlp
    from uncertainty_vit_amd.gp_probe import GPProbe
    argv, out = _setup(tmp_path)
    phis, step = [], GPProbe.train_step

    def recording(self, images, labels, *a, **k):
        r = step(self, images, labels, *a, **k)
        phis.append(self._phi[:images.shape[0]].cpu())
        return r
    monkeypatch.setattr(GPProbe, "train_step", recording)
    rlp.main(rlp.get_args(argv + ["--gp_cov_momentum", "0"]))
    capsys.readouterr()
    assert len(phis) == 6
    saved = torch.load(out / "probe-1.pth", map_location="cpu", weights_only=False)["model"]["head.precision_matrix"]
    ref, cpu = RIDGE * torch.eye(D, dtype=torch.float64), (RIDGE * torch.eye(D, dtype=torch.float64)).float()
    both = ref.clone()
    for i, ph in enumerate(phis):
        both += ph.double().t() @ ph.double()
        if i >= 3:
            ref += ph.double().t() @ ph.double()
            cpu = cpu + ph.t() @ ph
    scale = float(ref.abs().max())
    err, cpu_err = float((saved.double() - ref).abs().max()) / scale, float((cpu.double() - ref).abs().max()) / scale
    print(f"\nexact-sum P: error {err:.3e}, fp32 CPU error {cpu_err:.3e}, distance to the two-epoch sum {float((saved.double() - both).abs().max()) / scale:.3e}")
    assert err <= 4 * cpu_err
    assert torch.equal(saved, saved.t())
