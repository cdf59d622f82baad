"""The benchmarked step at its real size against the oracle run on the device in float64.

bench.py measures ViT-B/16 at bs=128 with 120 of 196 patches masked, drop-path 0.25, attention dropout 0.05, the drop-path
sample lists and the masked-row last block.  The oracle (oracle/vit_oracle.py, oracle/vit_oracle_dist.py) runs the same step
on the GPU in float64 with the kernels' dropout replayed, and every gradient tensor, and every row of the regression targets,
the student outputs and dL/d(block-0 input), is compared with it.  A summed weight gradient of 128 samples cannot see an error
confined to a few rows (one sample's attention, a slab tail, a wrong drop-path entry); the row checks can.

LayerScale is 0.1 (closed-form weights), as in the small-batch oracle tests: with bench.py's 1e-4 every Block branch would be
a 1e-4 perturbation of the residual stream and a wrong branch would hide in the rows."""
import time

import numpy as np
import pytest
import torch

from oracle import vit_oracle as vo
from oracle import vit_oracle_dist as vd
from oracle.closed_form import closed_form_images, exact_masks
from gpu_util import assert_grads_close, native_model, native_steps, native_trainer

pytestmark = pytest.mark.gpu

N_PATCH, N_MASK, TARGET_LAYERS, IT = 196, 120, tuple(range(6, 12)), 11
# Per-row bounds (see rowwise).  Worst rows measured on an MI355X (bf16 GEMM operands, fp32 residual stream, against fp64),
# B=2 / B=128 / two-stream B=128: targets 3.0e-3 / 3.1e-3 / 3.1e-3 (median 2.7e-3), outputs 8.0e-3 / 8.7e-3 / 9.3e-3 (median 7.3e-3),
# dx 1.2e-2 / 2.2e-2 / 2.3e-2 (median 1.0e-2).  The bounds leave a margin of 1.6-1.8x over the worst row; a row computed from
# the wrong sample, or left zero or stale, is an O(1) error.  Measured with faults injected in the kernels: the last head of
# the attention forward drawing head h-1's dropout mask puts outputs rows at 3.8e-2 and dx rows at 4.7e-2; the target
# finalize skipping post-LN on the last masked row puts that target row at 5.9e-3.
ROW_TOL = {"targets": 5e-3, "outputs": 1.5e-2, "dx": 4e-2}


def rowwise(name, got, ref, tol):
    """Every row's L2 error relative to the larger of its own reference norm and the median row norm of the reference (near-zero
    rows are judged against a typical row, rows far above the median -- the Wasserstein loss's arg-max row -- against
    themselves); prints and bounds the worst row."""
    ref = ref.reshape(-1, ref.shape[-1])
    got = got.to(ref.device, torch.float64).reshape(ref.shape)
    norms = ref.norm(dim=1)
    scale = norms.median()
    rel = (got - ref).norm(dim=1) / torch.maximum(norms, scale)
    worst = int(rel.argmax())
    print(f"  {name}: {ref.shape[0]} rows, worst row {worst} at {float(rel[worst]):.3e} (its norm {float(norms[worst]):.3e}, median "
          f"row norm {float(scale):.3e}, median row error {float(rel.median()):.3e}, largest row norm {float(norms.max()):.3e})")
    assert float(rel[worst]) <= tol, f"{name}: row {worst} off by {float(rel[worst]):.3e} (bound {tol})"
    return float(rel[worst])


def replayed_masks(seed, it, B, cfg, dev):
    """The attention-dropout keep masks the kernels drew (tests/test_gpu_model.py:test_dropout_step_matches_oracle_with_replayed_masks),
    built on the host and moved to the device one layer at a time."""
    aseed = int(vo._mix32(np.uint32(seed) ^ np.uint32((it * 0x85EBCA6B + 0x1234567) & 0xFFFFFFFF)))
    return [vo.attn_keep_mask(aseed, layer, B, cfg.num_heads, cfg.num_tokens, cfg.attn_drop_rate).to(dev) for layer in range(cfg.depth)]


def native_full_step(cfg, B, x, mask, two_stream, lam):
    """One step of the product on a host-side batch (the host counts the masked rows: the last block's row bound); returns what
    the comparison needs, copied, with the model freed."""
    model, sd = native_model(cfg, two_stream=two_stream)
    ema, opt = native_trainer(model)
    model.train()
    torch.manual_seed(4321)
    seed = torch.initial_seed() & 0xFFFFFFFF
    st = native_steps(model, ema, opt, [(x, mask)], list(TARGET_LAYERS), start=IT, stochastic=two_stream, lam=lam)[0]
    e, C, M = model._engine, cfg.embed_dim, int(mask.sum())
    assert e.drop_path_rows, "the step must run the drop-path sample lists"
    out = {"seed": seed, "st": st, "compact": e.compact_rows(),
           "grads": {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None},
           "targets": e.ws_tensor("targets", 0, (M, C)).clone(), "outputs": e.ws_tensor("outputs", 0, (M, C)).clone(),
           "dx": e.ws_tensor("dx", 0, (B * cfg.num_tokens, C)).clone()}
    if two_stream:
        cov = (e.ws_tensor("x_cov", 0, (1,)).data_ptr() - e.ws_tensor("x", 0, (1,)).data_ptr()) // 4   # stacked-stream offset
        dxa = e.ws_tensor("dx", 0, (cov + B * cfg.num_tokens * C,))
        out["dx_cov"] = dxa[cov:].view(B * cfg.num_tokens, C).clone()
        out["targets_cov"] = e.ws_tensor("targets_cov", 0, (M, C)).clone()
        out["outputs_cov"] = e.ws_tensor("outputs_cov", 0, (M, C)).clone()
    del model, ema, opt, e
    torch.cuda.empty_cache()
    return out, sd


def oracle_full_step(sd, cfg, x, mask, drop, two_stream, lam, dev):
    """The oracle's step in float64 on the device; prints its wall time and peak memory."""
    p = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    e = {k: v.clone() for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(t) for k, t in p.items()}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    rec = {}
    hp = vo.StepHParams(target_layers=TARGET_LAYERS)
    x64, m64 = x.to(dev, torch.float64), mask.to(dev)
    if two_stream:
        ref, _, cov_out, cov_tgt = vd.train_step(p, e, m, v, cfg, hp, x64, m64, 1, lam=lam, drop=drop, record=rec)
        extra = {"outputs_cov": cov_out, "targets_cov": cov_tgt, "dx_cov": rec["x0_cov"].grad}
    else:
        ref = vo.train_step(p, e, m, v, cfg, hp, x64, m64, 1, drop=drop, record=rec)
        extra = {}
    torch.cuda.synchronize()
    print(f"  fp64 oracle on the device: {time.time() - t0:.1f} s, peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    return ref, {"targets": ref.targets, "outputs": ref.outputs, "dx": rec["x0"].grad, **extra}


@pytest.mark.parametrize("B", [2, 128])
def test_base_step_vs_fp64_oracle(B):
    """ViT-B/16 (beit_base_patch16_224), BASELINE config 2's step: B=128, 120/196 masked, drop-path 0.25, attn-drop 0.05, target
    layers 6..11, clip 3.  B=2 is the same check at the size the host oracle already covers: it calibrates the row bounds."""
    cfg = vo.VitConfig(init_values=0.1, drop_path_rate=0.25, attn_drop_rate=0.05)
    dev = torch.device("cuda")
    x = closed_form_images(f"full-oracle-{B}", B, 224)
    mask = exact_masks(B, N_PATCH, N_MASK, 57)
    t0 = time.time()
    nat, sd = native_full_step(cfg, B, x, mask, False, 1e-5)
    print(f"\n[ViT-B B={B}] native step {time.time() - t0:.1f} s, loss {nat['st']['loss']:.6f}, grad-norm {nat['st']['grad_norm']:.5f}")
    count = int(mask.sum())
    if B == 128:                  # (the engine takes the row bound from 512 masked rows on: not at B=2)
        assert nat["compact"] == count, ("the masked-row last block did not run", nat["compact"], count)
    p1, p2 = vo.drop_path_scales(nat["seed"], IT, cfg, B)
    assert any(t is not None and (t == 0).any() for t in p1 + p2), "no sample dropped in any branch: the lists were not exercised"
    drop = vo.DropState(path1=p1, path2=p2, attn=replayed_masks(nat["seed"], IT, B, cfg, dev))
    ref, rows = oracle_full_step(sd, cfg, x, mask, drop, False, 1e-5, dev)
    del drop
    print(f"  oracle loss {ref.loss:.6f}, grad-norm {ref.grad_norm:.5f}")
    assert nat["st"]["loss"] == pytest.approx(ref.loss, rel=5e-3)
    assert nat["st"]["grad_norm"] == pytest.approx(ref.grad_norm, rel=3e-2)
    assert_grads_close(nat["grads"], {k: g.cpu() for k, g in ref.grads.items()}, what=f"[ViT-B B={B} vs fp64] ")
    for name in ("targets", "outputs", "dx"):
        rowwise(name, nat[name], rows[name], ROW_TOL[name])


def test_two_stream_step_vs_fp64_oracle():
    """dist_beit_base_patch16_224 (BASELINE config 3, `bench.py --model dist_...`): the same step, bs=128, both streams'
    targets, outputs and dL/d(block-0 input) row by row, and every gradient.  The Wasserstein weight is 1e-2 (bench.py: 1e-5)
    so that the covariance stream's backward weighs in the shared tensors."""
    cfg = vo.VitConfig(init_values=0.1, drop_path_rate=0.25, attn_drop_rate=0.05)
    dev, B, lam = torch.device("cuda"), 128, 1e-2
    x = closed_form_images("full-oracle-dist", B, 224)
    mask = exact_masks(B, N_PATCH, N_MASK, 59)
    t0 = time.time()
    nat, sd = native_full_step(cfg, B, x, mask, True, lam)
    print(f"\n[two-stream B={B}] native step {time.time() - t0:.1f} s, loss {nat['st']['loss']:.6f}, grad-norm {nat['st']['grad_norm']:.5f}")
    path = vd.drop_path_scales(nat["seed"], IT, cfg, B)
    assert any(t is not None and (t == 0).any() for row in path for t in row)
    drop = vd.DistDropState(path=path, attn=replayed_masks(nat["seed"], IT, B, cfg, dev))
    ref, rows = oracle_full_step(sd, cfg, x, mask, drop, True, lam, dev)
    del drop
    print(f"  oracle loss {ref.loss:.6f}, grad-norm {ref.grad_norm:.5f}")
    assert nat["st"]["loss"] == pytest.approx(ref.loss, rel=5e-3)
    assert nat["st"]["grad_norm"] == pytest.approx(ref.grad_norm, rel=3e-2)
    refg = {k: g.cpu() for k, g in ref.grads.items()}
    # the bounds of the two-stream B=2 oracle test (tests/test_gpu_dist.py): the q-side bias sums get their own
    qb = [n for n in refg if n.endswith("q_bias")]
    assert_grads_close(nat["grads"], refg, names=[n for n in refg if n not in qb], max_tol=5e-2, l2_tol=4e-2, what="[two-stream vs fp64] ")
    assert_grads_close(nat["grads"], refg, names=qb, max_tol=8e-2, l2_tol=6e-2, what="[two-stream q biases vs fp64] ")
    for name in ("targets", "outputs", "dx", "targets_cov", "outputs_cov", "dx_cov"):
        rowwise(name, nat[name], rows[name], ROW_TOL[name.replace("_cov", "")])
