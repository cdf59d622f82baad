"""GPU, end to end: run_linear_probe.main on a small image folder -- the command line of README.md, reduced: beit_base_patch16_224
cut after block 0 (--target_layer 0), a checkpoint of two blocks in utils.save_model's format, 12 images in 3 classes."""
import json
import os
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _image_tree(root, n):
    from PIL import Image
    rng = np.random.default_rng(17)
    sizes = [(240, 320), (300, 200), (224, 224), (180, 260)]
    for k in range(n):
        h, w = sizes[k % len(sizes)]
        p = os.path.join(root, f"class{k % 3}", f"img{k}.{'png' if k % 2 else 'jpg'}")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)


def _pretraining_checkpoint(path):
    """What run_cyclical.py leaves behind (utils.save_model: `model`, `args`, ...), of a two-block ViT-B/16."""
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    torch.manual_seed(5)
    m = VisionTransformerForCyclicalTraining(img_size=224, patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                             norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1,
                                             use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    args = SimpleNamespace(rel_pos_bias=True, abs_pos_emb=False, layer_scale_init_value=0.1)
    torch.save({"model": m.state_dict(), "optimizer": {}, "epoch": 0, "scaler": {}, "args": args}, path)


def test_cli_trains_evaluates_and_resumes(tmp_path, capsys):
    pytest.importorskip("PIL")
    import run_linear_probe as rlp
    train, val, out, ckpt = tmp_path / "train", tmp_path / "val", tmp_path / "out", tmp_path / "checkpoint-0.pth"
    _image_tree(str(train), 12)
    _image_tree(str(val), 6)
    out.mkdir()
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(train),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--epochs", "2",
            "--warmup_epochs", "0", "--lr", "1e-3", "--clip_grad", "1.0", "--output_dir", str(out)]
    last = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "encoder: 1 blocks" in text and "Trainable weights: ['head.weight', 'head.bias']" in text
    assert "Epoch 0: loss:" in text and "acc1:" in text and "acc5:" in text and "lr:" in text

    log = [json.loads(line) for line in open(out / "log.txt")]
    assert [e["epoch"] for e in log] == [0, 1]
    for e in log:
        # the head starts at 1e-3 x N(0, 0.02): the smoothed loss of three classes starts at log 3 and two epochs of six steps
        # cannot take it far
        assert np.isfinite(e["train_loss"]) and abs(e["train_loss"] - np.log(3.0)) < 0.2
        assert 0.0 <= e["test_acc1"] <= 100.0 and e["test_acc5"] == 100.0          # fewer than five classes: every label is top-5
        assert np.isfinite(e["test_loss"])
    assert last["n"] == 6 and last["acc1"] == log[1]["test_acc1"]
    saved = torch.load(out / "probe-1.pth", map_location="cpu", weights_only=False)
    assert {k: tuple(v.shape) for k, v in saved["model"].items()} == {"head.weight": (3, 768), "head.bias": (3,)}
    assert saved["optimizer"]["step"] == 6 and float(saved["model"]["head.bias"].abs().max()) > 0.0

    # --eval with the saved head: the evaluation pipeline draws nothing at random and the kernels fix their summation order, so the
    # figures of the last epoch come back bit for bit
    again = rlp.main(rlp.get_args(argv + ["--eval", "--resume", str(out / "probe-1.pth")]))
    text = capsys.readouterr().out
    assert "* Acc@1" in text and "Epoch" not in text
    assert (again["n"], again["correct1"], again["correct5"]) == (6, last["correct1"], 6)
    assert again["loss"] == last["loss"]
