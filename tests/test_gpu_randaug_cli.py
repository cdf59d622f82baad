"""GPU, end to end: run_linear_probe.main with --aa on a generated folder of 48-pixel images, as the other test_gpu_*_cli.py files run
their flags: beit_base_patch16_224 at --input_size 48 cut after block 0 (--target_layer 0), a one-block checkpoint, 24 training
images in 3 classes, two epochs of three steps."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

AA = ["--aa", "rand-m9-mstd0.5-inc1"]


def _small_images(root, n):
    from PIL import Image
    rng = np.random.default_rng(29)
    for k in range(n):
        p = os.path.join(root, f"class{k % 3}", f"img{k}.png")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)).save(p)


def _pretraining_checkpoint(path):
    """What run_cyclical.py leaves behind (utils.save_model) for a one-block ViT-B/16 at 48 px."""
    from functools import partial
    from types import SimpleNamespace
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    torch.manual_seed(5)
    m = VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=768, depth=1, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                             norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1,
                                             use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    args = SimpleNamespace(rel_pos_bias=True, abs_pos_emb=False, layer_scale_init_value=0.1)
    torch.save({"model": m.state_dict(), "optimizer": {}, "epoch": 0, "scaler": {}, "args": args}, path)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("randaug_cli")
    train, val, ckpt = root / "train", root / "val", root / "checkpoint-0.pth"
    _small_images(str(train), 24)
    _small_images(str(val), 6)
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--input_size", "48", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(train),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "8", "--epochs", "2",
            "--warmup_epochs", "0", "--lr", "1e-3", "--clip_grad", "1.0", "--seed", "1"]
    return root, argv


def _run(rlp, argv, out, capsys):
    out.mkdir()
    random.seed(7)          # the crop parameters come from Python's global stream, which main() leaves alone (--seed: torch and numpy)
    stats = rlp.main(rlp.get_args(argv + ["--output_dir", str(out)]))
    text = capsys.readouterr().out
    log = [json.loads(line) for line in open(out / "log.txt")]
    return stats, text, log


def test_cli_trains_and_resumes_with_randaugment(setup, capsys, monkeypatch):
    import run_linear_probe as rlp
    root, argv = setup
    # the uninterrupted run; the host's random streams (shuffling, crops) are recorded where epoch 0 ends, so that the resumed run can
    # be handed the data the uninterrupted run's epoch 1 saw -- the augmenter's own draws need no such help: they follow step_count
    states, save = {}, rlp.save_probe

    def save_and_record(args, probe, epoch):
        save(args, probe, epoch)
        if epoch == 0:
            states.update(py=random.getstate(), torch=torch.get_rng_state(), np=np.random.get_state())

    monkeypatch.setattr(rlp, "save_probe", save_and_record)
    stats, text, log = _run(rlp, argv + AA, root / "a", capsys)
    monkeypatch.setattr(rlp, "save_probe", save)
    assert text.count("RandAugment is activated: RandAugment(n=2, m=9, mstd=0.5, inc=1, interpolation=bicubic, fill=(128, 128, 128))") == 1
    assert "aa='rand-m9-mstd0.5-inc1'" in text.splitlines()[0] and "* Acc@1" in text
    assert [e["epoch"] for e in log] == [0, 1] and all(math.isfinite(e["train_loss"]) and math.isfinite(e["test_loss"]) for e in log)
    assert (root / "a" / "probe-1.pth").exists() and stats["n"] == 6
    # resumed behind epoch 0 with the streams of that moment: epoch 1 draws what it drew and ends on the same digits
    schedule = rlp.utils.cosine_scheduler

    def restore_then_schedule(*a, **kw):
        random.setstate(states["py"])
        torch.set_rng_state(states["torch"])
        np.random.set_state(states["np"])
        return schedule(*a, **kw)

    monkeypatch.setattr(rlp.utils, "cosine_scheduler", restore_then_schedule)
    _, text, resumed = _run(rlp, argv + AA + ["--resume", str(root / "a" / "probe-0.pth")], root / "b", capsys)
    monkeypatch.setattr(rlp.utils, "cosine_scheduler", schedule)
    assert "Resume checkpoint" in text and [e["epoch"] for e in resumed] == [1]
    assert resumed[0]["train_loss"] == log[1]["train_loss"] and resumed[0]["test_loss"] == log[1]["test_loss"]
    # without the flag the run says nothing of it, its first line holds no new argument, and it trains on other batches
    _, text, plain = _run(rlp, argv, root / "c", capsys)
    assert "RandAugment" not in text and "aa=" not in text.splitlines()[0] and plain[0]["train_loss"] != log[0]["train_loss"]
    # another --mix_seed draws otherwise
    _, _, other = _run(rlp, argv + AA + ["--mix_seed", "2"], root / "d", capsys)
    assert other[0]["train_loss"] != log[0]["train_loss"]


def test_cli_refusals(setup):
    import run_linear_probe as rlp
    _, argv = setup
    with pytest.raises(ValueError, match="--eval"):
        rlp.main(rlp.get_args(argv + AA + ["--eval"]))
    with pytest.raises(NotImplementedError, match="original"):
        rlp.main(rlp.get_args(argv + ["--aa", "original"]))


def test_cli_ensemble_takes_randaugment(setup, capsys):
    import run_linear_probe as rlp
    root, argv = setup
    _, text, log = _run(rlp, argv + AA + ["--ensembles", "--ens_members", "2", "--epochs", "1"], root / "e", capsys)
    assert "RandAugment is activated" in text and math.isfinite(log[0]["train_loss"])
