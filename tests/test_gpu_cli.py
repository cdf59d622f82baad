"""End-to-end: the reference's command line (README.md:27-61 recipe, reduced) through run_cyclical.main on the GPU --
synthetic images, block-wise masks, device prefetcher, cosine schedules, checkpoint + auto-resume."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu


def _argv(out, epochs, extra=()):
    return ["--model", "beit_base_patch16_224", "--data_set", "SYNTHETIC", "--synthetic_len", "32", "--batch_size", "8",
            "--epochs", str(epochs), "--warmup_epochs", "0", "--lr", "5e-4", "--target_layers", "[8,9,10,11]",
            "--num_mask_patches", "75", "--synthetic_masks", "block", "--num_workers", "0", "--output_dir", str(out),
            "--clip_grad", "3.0", "--ema_decay", "0.999", "--drop_path", "0.1", *extra]


@pytest.mark.parametrize("stochastic", [False, True])
def test_cli_trains_checkpoints_and_resumes(tmp_path, stochastic):
    import run_cyclical
    extra = ("--stochastic",) if stochastic else ()
    run_cyclical.main(run_cyclical.get_args(_argv(tmp_path, 2, extra)))
    log = [json.loads(l) for l in open(tmp_path / "log.txt")]
    assert [l["epoch"] for l in log] == [0, 1]
    assert all(0 < l["train_loss"] < 10 and l["train_grad_norm"] > 0 for l in log)
    assert (tmp_path / "checkpoint-1.pth").exists()
    ck = torch.load(tmp_path / "checkpoint-1.pth", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and "model_ema" in ck and "optimizer" in ck

    # a second invocation with more epochs resumes after the newest checkpoint (utils.py:491-521)
    args = run_cyclical.get_args(_argv(tmp_path, 3, extra))
    run_cyclical.main(args)
    assert args.start_epoch == 2
    log = [json.loads(l) for l in open(tmp_path / "log.txt")]
    assert [l["epoch"] for l in log] == [0, 1, 2] and 0 < log[2]["train_loss"] < 10
    # the resumed epoch continued the run: Adam step count, weights that moved, and the schedules of global iterations 8..11
    per_epoch = 32 // 8
    ck2 = torch.load(tmp_path / "checkpoint-2.pth", map_location="cpu", weights_only=False)
    assert ck2["epoch"] == 2 and {int(float(s["step"])) for s in ck2["optimizer"]["state"].values()} == {3 * per_epoch}
    assert {int(float(s["step"])) for s in ck["optimizer"]["state"].values()} == {2 * per_epoch}
    moved = [k for k, v in ck2["model"].items() if v.dtype.is_floating_point and not torch.equal(v, ck["model"][k])]
    assert len(moved) > 0.8 * len(ck["model"]), moved          # all but the index buffer and the two-stream model's dead cov_qkv weights
    assert any(not torch.equal(v, ck["model_ema"][k]) for k, v in ck2["model_ema"].items())
    lr, wd, decay = resumed_epoch_scalars(args, 3, per_epoch)
    # the log holds means of the host's float64 values, epoch_scalars the float32 values the device reads: 2^-23 apart at most
    assert log[2]["train_lr"] == pytest.approx(lr, rel=2 ** -23) and log[2]["train_lr"] != pytest.approx(log[1]["train_lr"], rel=1e-2)
    assert log[2]["train_weight_decay"] == pytest.approx(wd, rel=2 ** -23)
    assert log[2]["train_cur_decay"] == pytest.approx(decay, rel=2 ** -23)


def resumed_epoch_scalars(args, epochs, per_epoch):
    """Means over the last epoch's iterations of (lr, weight decay, EMA decay), from the schedules run_cyclical.main builds for `epochs`
    epochs and engine_for_cyclical.epoch_scalars at the global iterations (epochs - 1) * per_epoch ...; computed on the host."""
    from types import SimpleNamespace
    from uncertainty_vit_amd import utils
    from uncertainty_vit_amd.engine_for_cyclical import epoch_scalars
    assert args.tri_phase_schedule is None and args.epochs == epochs
    lrs = utils.cosine_scheduler(args.lr, args.min_lr, epochs, per_epoch, warmup_epochs=args.warmup_epochs, warmup_steps=args.warmup_steps)
    wds = utils.cosine_scheduler(args.weight_decay, args.weight_decay_end, epochs, per_epoch)
    opt = SimpleNamespace(param_groups=[dict(lr=args.lr, weight_decay=args.weight_decay, lr_scale=1.0)])
    rows = epoch_scalars(opt, (epochs - 1) * per_epoch, per_epoch, lrs, wds, args.ema_start_at, args.ema_decay_init, args.ema_decay, -1)
    assert all(d > 0 for _, _, d in rows) and len({r[0] for r in rows}) == per_epoch
    return tuple(sum(r[k] for r in rows) / per_epoch for k in range(3))


def test_cli_config1_plumbing_size(tmp_path):
    """BASELINE config 1 at its stated size: beit_base_patch16_224 through run_cyclical.main, batch 4, 120 masked patches per
    image, 2 steps (8 synthetic images, 1 epoch) -- the reference runs it on the CPU as a plumbing check; here every step is native."""
    import run_cyclical
    argv = ["--model", "beit_base_patch16_224", "--data_set", "SYNTHETIC", "--synthetic_len", "8", "--batch_size", "4", "--epochs", "1",
            "--warmup_epochs", "0", "--lr", "5e-4", "--target_layers", "[6,7,8,9,10,11]", "--num_mask_patches", "120", "--num_workers", "0",
            "--output_dir", str(tmp_path), "--clip_grad", "3.0", "--drop_path", "0.25", "--attn_drop_rate", "0.05"]
    run_cyclical.main(run_cyclical.get_args(argv))
    log = [json.loads(l) for l in open(tmp_path / "log.txt")]
    assert len(log) == 1 and 0 < log[0]["train_loss"] < 10 and log[0]["train_grad_norm"] > 0
