"""GPU, end to end: run_linear_probe.main --learn_layer_weights --layernorm_before_combine --use_cls on a generated 10-class folder
of 48 px images, 20 per class: two epochs of training on a three-block encoder registered for this test, then --resume --eval
--calibration on its checkpoint, and the refusals that need a checkpoint."""
import json
import re

import pytest

from test_gpu_lap_cli import _image_tree

pytestmark = pytest.mark.gpu

LW_LINE = re.compile(r"^\* Layer weights ((?:\d\.\d{4} ?)+) \(argmax: block (\d+)\)$", re.M)
MODEL = "lw_cli_tiny_patch16_48"


def _tiny(pretrained=False, **kwargs):
    from uncertainty_vit_amd.modeling_cyclical import _build
    return _build(pretrained, kwargs, embed_dim=128, depth=3, num_heads=2)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The image folder and what run_cyclical.py leaves behind (utils.save_model) for the three-block encoder."""
    pytest.importorskip("PIL")
    from types import SimpleNamespace

    import torch
    root = tmp_path_factory.mktemp("lw_cli")
    data, pre = root / "data", root / "checkpoint-0.pth"
    _image_tree(str(data))
    torch.manual_seed(5)
    m = _tiny(img_size=48, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    args = SimpleNamespace(rel_pos_bias=True, abs_pos_emb=False, layer_scale_init_value=0.1)
    torch.save({"model": m.state_dict(), "optimizer": {}, "epoch": 0, "scaler": {}, "args": args}, pre)
    return data, pre


def test_cli_trains_resumes_and_refuses(tree, tmp_path, capsys, monkeypatch):
    import torch

    import run_linear_probe as rlp
    from uncertainty_vit_amd import modeling_cyclical
    monkeypatch.setitem(modeling_cyclical._REGISTRY, MODEL, _tiny)
    data, pre = tree
    out = tmp_path / "out"
    out.mkdir()
    base = ["--model", MODEL, "--input_size", "48", "--finetune", str(pre), "--data_set", "image_folder", "--data_path", str(data),
            "--eval_data_path", str(data), "--nb_classes", "10", "--batch_size", "50"]
    flags = ["--learn_layer_weights", "--layernorm_before_combine", "--use_cls"]
    stats = rlp.main(rlp.get_args(base + flags + ["--target_layer", "1", "--epochs", "2", "--warmup_epochs", "0", "--lr", "0.01",
                                                  "--output_dir", str(out)]))
    text = capsys.readouterr().out
    lines = text.splitlines()
    assert "--learn_layer_weights supersedes --target_layer 1: the encoder keeps every block" in lines
    assert "encoder: 3 blocks, 0 checkpoint entries not part of it" in text                    # not cut after block 1
    trainable = [ln for ln in lines if ln.startswith("Trainable weights:")]
    assert len(trainable) == 1 and all(repr(k) in trainable[0] for k in ("head.weight", "head.bias", "layer_log_weights"))
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    found = LW_LINE.findall(text)
    assert len(acc) == 2 and len(found) == 2 and all(LW_LINE.fullmatch(lines[i + 1]) for i in acc)                 # directly behind * Acc@1
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert [e["epoch"] for e in log] == [0, 1]
    for (shown, block), entry in zip(found, log):
        w = entry["test_layer_weights"]
        assert len(w) == 3 and sum(w) == pytest.approx(1.0, abs=1e-6) and shown.split() == [f"{v:.4f}" for v in w] and int(block) == w.index(max(w))
    assert stats["layer_weights"] == log[1]["test_layer_weights"]
    assert max(abs(v - 1 / 3) for v in log[1]["test_layer_weights"]) > 1e-3                  # eight steps of lr 0.01 moved them off the uniform start
    saved = torch.load(out / "probe-1.pth", map_location="cpu", weights_only=False)
    assert sorted(saved["model"]) == ["head.bias", "head.weight", "layer_log_weights"] and tuple(saved["model"]["layer_log_weights"].shape) == (3,)
    assert sorted(saved["optimizer"]["exp_avg"]) == sorted(saved["model"]) and saved["optimizer"]["step"] == 8

    ev = tmp_path / "eval"
    ev.mkdir()
    again = rlp.main(rlp.get_args(base + flags + ["--resume", str(out / "probe-1.pth"), "--eval", "--calibration", "--output_dir", str(ev)]))
    text = capsys.readouterr().out
    lines = text.splitlines()
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    assert len(acc) == 1 and LW_LINE.fullmatch(lines[acc[0] + 1]) and lines[acc[0] + 2].startswith("* ECE ")
    assert again["layer_weights"] == stats["layer_weights"] and again["acc1"] == stats["acc1"] and again["loss"] == stats["loss"]
    entry = [json.loads(line) for line in open(ev / "log.txt")]
    assert len(entry) == 1 and entry[0]["test_layer_weights"] == stats["layer_weights"] and "test_ECE" in entry[0]

    with pytest.raises(ValueError, match="mixes the features of the linear head"):
        rlp.main(rlp.get_args(base + flags + ["--ensembles"]))
    with pytest.raises(ValueError, match="--learn_layer_weights"):
        rlp.main(rlp.get_args(base + ["--use_cls"]))
    # a linear probe's checkpoint does not resume under the flag, and the flag's checkpoint does not resume without it
    plain = rlp.main(rlp.get_args(base + ["--epochs", "1", "--warmup_epochs", "0", "--output_dir", str(ev)]))
    assert "layer_weights" not in plain and "Layer weights" not in capsys.readouterr().out
    with pytest.raises(KeyError, match="layer_log_weights"):
        rlp.main(rlp.get_args(base + flags + ["--resume", str(ev / "probe-0.pth"), "--eval"]))
    with pytest.raises(RuntimeError, match="layer_log_weights"):
        rlp.main(rlp.get_args(base + ["--resume", str(out / "probe-1.pth"), "--eval"]))
