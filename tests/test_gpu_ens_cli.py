"""GPU, end to end: run_linear_probe.main --ensembles on a small image folder, as tests/test_gpu_het_cli.py runs the heteroscedastic
head: beit_base_patch16_224 cut after block 0 (--target_layer 0), a checkpoint of two blocks, 12 images in 3 classes, 3 members."""
import json
import math

import pytest
import torch

from test_gpu_probe_cli import _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

M = 3
SHAPES = {f"heads.{m}.{n}": s for m in range(M) for n, s in (("weight", (3, 768)), ("bias", (3,)))}
ENS_LOG = ["test_ens_total", "test_ens_aleatoric", "test_ens_mi", "test_ens_var", "test_ens_disagreement"]


def _setup(tmp_path):
    pytest.importorskip("PIL")
    train, val, out, ckpt = tmp_path / "train", tmp_path / "val", tmp_path / "out", tmp_path / "checkpoint-0.pth"
    _image_tree(str(train), 12)
    _image_tree(str(val), 6)
    out.mkdir()
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(train),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--epochs", "2",
            "--warmup_epochs", "0", "--lr", "1e-3", "--clip_grad", "1.0"]
    return argv, out


def test_cli_ensemble_trains_evaluates_and_resumes(tmp_path, capsys):
    import run_linear_probe as rlp
    argv, out = _setup(tmp_path)
    argv = argv + ["--output_dir", str(out), "--ensembles", "--ens_members", str(M), "--ens_bagging"]
    last = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "encoder: 1 blocks" in text and all(k in text for k in SHAPES)
    assert text.count("* Ens entropy ") == 2 and text.count("* Member ") == 2 * M
    assert text.index("* Acc@1") < text.index("* Member 0 Acc@1") < text.index("* Member 2 Acc@1") < text.index("* Ens entropy ")
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert [e["epoch"] for e in log] == [0, 1]
    for e in log:
        assert math.isfinite(e["train_loss"]) and math.isfinite(e["test_loss"])
        assert all(math.isfinite(e[k]) for k in ENS_LOG) and all(0.0 <= e[f"test_member{m}_acc1"] <= 100.0 for m in range(M))
        assert 0.0 < e["test_ens_total"] <= math.log(3) + 1e-6 and e["test_ens_mi"] >= 0.0 and 0.0 <= e["test_ens_disagreement"] <= 1.0
    print(f"\nensemble per epoch {[[e[k] for k in ENS_LOG] for e in log]}, loss {last['loss']:.4f}")
    assert last["n"] == 6 and last["ens_mi"] == log[1]["test_ens_mi"] and last["member_acc1"] == [log[1][f"test_member{m}_acc1"] for m in range(M)]
    saved = torch.load(out / "probe-1.pth", map_location="cpu", weights_only=False)
    assert {k: tuple(v.shape) for k, v in saved["model"].items()} == SHAPES
    assert saved["optimizer"]["step"] == 6 and sorted(saved["optimizer"]["exp_avg"]) == sorted(SHAPES)
    # bagging gave the members different data: they are different heads
    assert not torch.equal(saved["model"]["heads.0.bias"], saved["model"]["heads.1.bias"])

    # --eval --calibration with the saved heads: the kernels fix their summation order, so the figures of the last epoch come back
    resume = argv + ["--eval", "--calibration", "--resume", str(out / "probe-1.pth")]
    again = rlp.main(rlp.get_args(resume))
    text = capsys.readouterr().out
    assert "* Acc@1" in text and text.count("* Member ") == M and "* Ens entropy " in text and "* ECE " in text and "Epoch" not in text
    assert text.index("* Ens entropy ") < text.index("* ECE ")
    assert (again["n"], again["correct1"], again["correct5"]) == (6, last["correct1"], 6)
    assert again["loss"] == last["loss"] and again["member_loss"] == last["member_loss"]
    assert all(again[k[5:]] == last[k[5:]] for k in ENS_LOG)
    entry = json.loads(open(out / "log.txt").readlines()[-1])
    assert entry["test_ens_mi"] == last["ens_mi"] and "test_ECE" in entry and "test_member2_acc1" in entry and "epoch" not in entry

    # the other combination moves the loss, not the members
    other = rlp.main(rlp.get_args(resume + ["--ens_combine", "probs"]))
    capsys.readouterr()
    assert other["loss"] != last["loss"] and other["member_loss"] == last["member_loss"] and other["ens_total"] == last["ens_total"]


def test_cli_ensemble_of_separately_trained_heads(tmp_path, capsys):
    """Two plain linear probes trained under different seeds, then --ensembles --ens_heads a.pth b.pth --eval: the members' lines
    are the two probes' own evaluations."""
    import run_linear_probe as rlp
    argv, out = _setup(tmp_path)
    singles, paths = [], []
    for i in range(2):
        d = out / f"probe{i}"
        d.mkdir()
        singles.append(rlp.main(rlp.get_args(argv + ["--output_dir", str(d), "--seed", str(i)])))
        paths.append(str(d / "probe-1.pth"))
    capsys.readouterr()
    ens = rlp.main(rlp.get_args(argv + ["--ensembles", "--eval", "--ens_heads"] + paths))
    text = capsys.readouterr().out
    assert "Ensemble of 2 heads" in text and text.count("* Member ") == 2 and "* Ens entropy " in text
    print(f"\nsingles {[(s['correct1'], s['loss']) for s in singles]}; ensemble {ens}")
    assert ens["n"] == 6 and ens["member_correct1"] == [s["correct1"] for s in singles]
    assert ens["member_loss"] == pytest.approx([s["loss"] for s in singles], rel=1e-6)
    assert ens["ens_mi"] > 0.0
