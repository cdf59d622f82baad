"""GPU, end to end: run_linear_probe.main with --mixup / --cutmix / --reprob on a drawn image folder, as the other test_gpu_*_cli.py
files run their flags: beit_base_patch16_224 cut after block 0 (--target_layer 0), a checkpoint of two blocks, 24 training images of
32 x 32 pixels in 3 classes, one epoch."""
import json
import math
import os
import random

import numpy as np
import pytest

from test_gpu_probe_cli import _pretraining_checkpoint

pytestmark = pytest.mark.gpu

MIX = ["--mixup", "0.8", "--cutmix", "1.0", "--reprob", "0.25"]


def _small_images(root, n):
    from PIL import Image
    rng = np.random.default_rng(23)
    for k in range(n):
        p = os.path.join(root, f"class{k % 3}", f"img{k}.png")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(p)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("mix_cli")
    train, val, ckpt = root / "train", root / "val", root / "checkpoint-0.pth"
    _small_images(str(train), 24)
    _small_images(str(val), 6)
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(train),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "8", "--epochs", "1",
            "--warmup_epochs", "0", "--lr", "1e-3", "--clip_grad", "1.0", "--seed", "1"]
    return root, argv


def _run(rlp, argv, out, capsys):
    out.mkdir()
    random.seed(7)          # the crop parameters come from Python's global stream, which main() leaves alone (--seed: torch and numpy)
    stats = rlp.main(rlp.get_args(argv + ["--output_dir", str(out)]))
    text = capsys.readouterr().out
    log = [json.loads(line) for line in open(out / "log.txt")]
    return stats, text, log


def test_cli_trains_with_mixing(setup, capsys):
    import run_linear_probe as rlp
    root, argv = setup
    stats, text, log = _run(rlp, argv + MIX, root / "a", capsys)
    assert text.count("Mixup is activated!") == 1 and "* Acc@1" in text
    assert [e["epoch"] for e in log] == [0] and math.isfinite(log[0]["train_loss"]) and math.isfinite(log[0]["test_loss"])
    assert (root / "a" / "probe-0.pth").exists() and stats["n"] == 6
    # the same seeds: the same draws, the same kernels in the same order, the same digits
    _, _, again = _run(rlp, argv + MIX, root / "b", capsys)
    assert again[0]["train_loss"] == log[0]["train_loss"] and again[0]["test_loss"] == log[0]["test_loss"]
    # without the flags the run says nothing of mixing and trains on another loss; another --mix_seed draws otherwise
    _, text, plain = _run(rlp, argv, root / "c", capsys)
    assert "Mixup is activated!" not in text and plain[0]["train_loss"] != log[0]["train_loss"]
    _, _, other = _run(rlp, argv + MIX + ["--mix_seed", "2"], root / "d", capsys)
    assert other[0]["train_loss"] != log[0]["train_loss"]


def test_cli_refuses_mixing_under_the_ensemble(setup, capsys):
    import run_linear_probe as rlp
    _, argv = setup
    with pytest.raises(ValueError, match="--ensembles"):
        rlp.main(rlp.get_args(argv + MIX + ["--ensembles"]))
    with pytest.raises(ValueError, match="--eval"):
        rlp.main(rlp.get_args(argv + MIX + ["--eval"]))
