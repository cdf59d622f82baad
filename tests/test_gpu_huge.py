"""GPU: ViT-H/16 (beit_huge_patch16_224, head_dim 80) end to end -- the head_dim-80 tiny model against the reference's own
vectors (tests/golden/model_hd80.npz), the ViT-H step against the oracle in float64 on the device (the helpers of
tests/test_gpu_fullsize.py), and the command line with a checkpoint and a resume."""
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

import test_gpu_fullsize as fs
from golden_util import check_entry, entries
from gpu_util import assert_grads_close, full_size_step_properties, native_model, native_steps, native_trainer, oracle_state
from oracle import vit_oracle as vo
from oracle.closed_form import closed_form_images, exact_masks
from test_gpu_model import ACT_AT, ACT_RT, load_case

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
HUGE_TARGET_LAYERS = tuple(range(16, 32))


def test_hd80_forward_modes_vs_golden(golden_dir):
    fx, cfg, B, n_mask, _ = load_case(golden_dir, "hd80")
    assert cfg.head_dim == 80
    model, _ = native_model(cfg)
    model.eval()
    x = closed_form_images("hd80/0", B, cfg.img_size).cuda()
    mask = torch.from_numpy(fx["mask0"]).cuda()
    ends = model(x, None, True, layer_results="end")
    fcs = model(x, None, True, layer_results="fc")
    for i in range(cfg.depth):
        check_entry(fx, f"fwd/end{i}", ends[i], ACT_RT, ACT_AT)
        check_entry(fx, f"fwd/fc{i}", fcs[i], 5e-2, 3e-2 * cfg.init_values + 1e-6)
    check_entry(fx, "fwd/student_masked", model(x, mask, return_all_tokens=False), ACT_RT, ACT_AT)
    check_entry(fx, "fwd/student_all", model(x, mask, return_all_tokens=True), ACT_RT, ACT_AT)


def test_hd80_train_steps_vs_golden(golden_dir):
    fx, cfg, B, n_mask, steps = load_case(golden_dir, "hd80")
    model, sd0 = native_model(cfg)
    ema, opt = native_trainer(model)
    tl = [int(v) for v in fx["target_layers"]]
    batches = [(closed_form_images(f"hd80/{s}", B, cfg.img_size).cuda(), torch.from_numpy(fx[f"mask{s}"]).cuda()) for s in range(steps)]
    st = native_steps(model, ema, opt, batches[:1], tl)
    assert st[0]["loss"] == pytest.approx(float(fx["step/loss"][0]), rel=5e-3)
    assert st[0]["grad_norm"] == pytest.approx(float(fx["step/grad_norm"][0]), rel=3e-2)
    grads = {n: p.grad for n, p in model.named_parameters()}
    gmax = max(float(np.abs(fx[k]).max()) for k in fx.files if k.startswith("grad0/") and not k.endswith("/sum"))
    for n in entries(fx, "grad0"):
        check_entry(fx, "grad0/" + n, grads[n], 5e-2, 2e-2 * gmax, what="[hd80] ")
    p, e, m1, v1 = oracle_state(sd0)
    ref = vo.train_step(p, e, m1, v1, cfg, vo.StepHParams(target_layers=tuple(tl)), batches[0][0].cpu(), batches[0][1].cpu(), 1)
    assert_grads_close({n: g.clone() for n, g in grads.items()}, ref.grads, what="[hd80] ")
    st += native_steps(model, ema, opt, batches[1:], tl, start=1)
    for s in range(1, steps):
        assert st[s]["loss"] == pytest.approx(float(fx["step/loss"][s]), rel=2e-2)
    sd, esd = model.state_dict(), ema.module.state_dict()
    for n in entries(fx, "post"):
        check_entry(fx, "post/" + n, sd[n], 0, 3 * 2e-3 + 1e-4, what="post ")
    for n in entries(fx, "ema"):
        check_entry(fx, "ema/" + n, esd[n], 0, 3 * 2e-3 * 2e-4 + 1e-5, what="ema ")


def huge_cfg(**kw):
    return vo.VitConfig(embed_dim=1280, depth=32, num_heads=16, init_values=0.1, drop_path_rate=0.25, attn_drop_rate=0.05, **kw)


@pytest.mark.parametrize("B", [2, 16])
def test_huge_step_vs_fp64_oracle(B, monkeypatch):
    """beit_huge_patch16_224's step: 120/196 masked, drop-path 0.25, attn-drop 0.05, target layers 16..31, clip 3 -- loss,
    grad-norm, every gradient tensor, and every row of the targets, the student outputs and dL/d(block-0 input)."""
    monkeypatch.setattr(fs, "TARGET_LAYERS", HUGE_TARGET_LAYERS)
    cfg = huge_cfg()
    dev = torch.device("cuda")
    x = closed_form_images(f"huge-oracle-{B}", B, 224)
    mask = exact_masks(B, fs.N_PATCH, fs.N_MASK, 59)
    t0 = time.time()
    nat, sd = fs.native_full_step(cfg, B, x, mask, False, 1e-5)
    print(f"\n[ViT-H B={B}] native step {time.time() - t0:.1f} s, loss {nat['st']['loss']:.6f}, grad-norm {nat['st']['grad_norm']:.5f}")
    p1, p2 = vo.drop_path_scales(nat["seed"], fs.IT, cfg, B)
    drop = vo.DropState(path1=p1, path2=p2, attn=fs.replayed_masks(nat["seed"], fs.IT, B, cfg, dev))
    ref, rows = fs.oracle_full_step(sd, cfg, x, mask, drop, False, 1e-5, dev)
    del drop
    print(f"  oracle loss {ref.loss:.6f}, grad-norm {ref.grad_norm:.5f}")
    assert nat["st"]["loss"] == pytest.approx(ref.loss, rel=5e-3)
    assert nat["st"]["grad_norm"] == pytest.approx(ref.grad_norm, rel=3e-2)
    # relative-L2 bound 3e-2 (ViT-B: 2e-2): bf16 round-off through 32 layers instead of 12; measured worst tensor on an MI355X:
    # blocks.3.attn.q_bias at 2.2e-2 (B = 2), 1.8e-2 (B = 16)
    assert_grads_close(nat["grads"], {k: g.cpu() for k, g in ref.grads.items()}, l2_tol=3e-2, what=f"[ViT-H B={B} vs fp64] ")
    for name in ("targets", "outputs", "dx"):
        fs.rowwise(name, nat[name], rows[name], fs.ROW_TOL[name])


def test_huge_full_size_step_properties():
    """ViT-H/16 at bs=128 (120 masked patches, attn-drop 0.05, drop-path 0.25, clip 3): the size-independent properties of one
    full step (tests/gpu_util.py:full_size_step_properties)."""
    full_size_step_properties(huge_cfg(), vo.VitConfig(embed_dim=1280, depth=32, num_heads=16, init_values=1e-4), B=128, img=224,
                              n_patches=196, n_mask=120, target_layers=list(HUGE_TARGET_LAYERS), tag="huge-full")


def test_cli_huge_trains_checkpoints_and_resumes(tmp_path):
    import run_cyclical
    argv = lambda ep: ["--model", "beit_huge_patch16_224", "--data_set", "SYNTHETIC", "--synthetic_len", "8", "--batch_size", "4",  # noqa: E731
                       "--epochs", str(ep), "--warmup_epochs", "0", "--lr", "5e-4", "--target_layers", str(list(HUGE_TARGET_LAYERS)),
                       "--num_mask_patches", "75", "--num_workers", "0", "--output_dir", str(tmp_path), "--clip_grad", "3.0",
                       "--drop_path", "0.25", "--attn_drop_rate", "0.05"]
    run_cyclical.main(run_cyclical.get_args(argv(1)))
    assert (tmp_path / "checkpoint-0.pth").exists()
    args = run_cyclical.get_args(argv(2))
    run_cyclical.main(args)
    assert args.start_epoch == 1
    log = [json.loads(l) for l in open(tmp_path / "log.txt")]
    assert [l["epoch"] for l in log] == [0, 1] and all(0 < l["train_loss"] < 10 and l["train_grad_norm"] > 0 for l in log)
