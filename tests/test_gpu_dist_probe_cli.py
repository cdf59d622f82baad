"""GPU, end to end: run_linear_probe.main with a two-stream --model on a small image folder: dist_beit_base_patch16_224 cut after
block 0 (--target_layer 0), a checkpoint of two blocks in utils.save_model's format, 12 images in 3 classes (the base model's run:
tests/test_gpu_probe_cli.py)."""
import json
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_probe_cli import _image_tree

pytestmark = pytest.mark.gpu


def _two_stream_checkpoint(path):
    from uncertainty_vit_amd.modeling_cyclical import DistVisionTransformerForCyclicalTraining
    torch.manual_seed(5)
    m = DistVisionTransformerForCyclicalTraining(img_size=224, patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                                 norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1,
                                                 use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    args = SimpleNamespace(rel_pos_bias=True, abs_pos_emb=False, layer_scale_init_value=0.1)
    torch.save({"model": m.state_dict(), "optimizer": {}, "epoch": 0, "scaler": {}, "args": args}, path)


def test_cli_trains_and_evaluates_a_two_stream_checkpoint(tmp_path, capsys):
    pytest.importorskip("PIL")
    import run_linear_probe as rlp
    train, val, out, ckpt = tmp_path / "train", tmp_path / "val", tmp_path / "out", tmp_path / "checkpoint-0.pth"
    _image_tree(str(train), 12)
    _image_tree(str(val), 6)
    out.mkdir()
    _two_stream_checkpoint(ckpt)
    argv = ["--model", "dist_beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(train),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--epochs", "1",
            "--warmup_epochs", "0", "--lr", "1e-3", "--clip_grad", "1.0", "--output_dir", str(out)]
    last = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "encoder: 1 blocks" in text and "Trainable weights: ['head.weight', 'head.bias']" in text
    assert "* Dist variance mean" in text and "Epoch 0: loss:" in text
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert [e["epoch"] for e in log] == [0]
    assert np.isfinite(log[0]["train_loss"]) and abs(log[0]["train_loss"] - np.log(3.0)) < 0.2
    assert log[0]["test_dist_var_mean"] == last["dist_var_mean"] > 0.0 and log[0]["test_dist_trace_mean"] == last["dist_trace_mean"] > 0.0
    saved = torch.load(out / "probe-0.pth", map_location="cpu", weights_only=False)
    assert {k: tuple(v.shape) for k, v in saved["model"].items()} == {"head.weight": (3, 768), "head.bias": (3,)}

    # --eval --resume at mean_field = 0: the last epoch's figures come back bit for bit (nothing is drawn at random, every sum has a
    # fixed order)
    again = rlp.main(rlp.get_args(argv + ["--eval", "--resume", str(out / "probe-0.pth")]))
    capsys.readouterr()
    assert (again["n"], again["correct1"], again["loss"]) == (6, last["correct1"], last["loss"])
    assert again["dist_var_mean"] == last["dist_var_mean"] and again["dist_trace_mean"] == last["dist_trace_mean"]

    # under the probit link: the two columns are formed from the unscaled logits and the features, so their means stay
    ev = rlp.main(rlp.get_args(argv + ["--eval", "--resume", str(out / "probe-0.pth"), "--detection", "--calibration",
                                       "--dist_mean_field", "0.3927"]))
    text = capsys.readouterr().out
    assert "* Dist variance mean" in text and "* Detect misclassification dist_var AUROC" in text
    assert "* Detect misclassification dist_trace AUROC" in text and "* ECE" in text
    assert 0.0 <= ev["acc1"] <= 100.0 and ev["loss"] != last["loss"] and ev["dist_trace_mean"] == last["dist_trace_mean"] and ev["dist_var_mean"] == last["dist_var_mean"]
    entry = [json.loads(line) for line in open(out / "log.txt")][-1]
    assert entry["test_dist_var_mean"] == ev["dist_var_mean"] and entry["test_dist_trace_mean"] == ev["dist_trace_mean"]
    assert "test_mis_dist_var_AUROC" in entry and "test_ECE" in entry

    # the flags belong to a two-stream model, and the other heads keep refusing one
    with pytest.raises(NotImplementedError):
        rlp.main(rlp.get_args(argv + ["--gp_layer"]))
