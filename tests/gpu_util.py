"""Shared helpers for the GPU parity tests and smoke(): build the native model with closed-form
weights, run native training steps, run the oracle on the same inputs."""
from functools import partial

import torch

from oracle import vit_oracle as vo
from oracle import vit_oracle_dist as vd
from oracle.closed_form import closed_form_state


def native_model(cfg: vo.VitConfig, gamma=None, device="cuda", two_stream=False):
    """VisionTransformerForCyclicalTraining (or the two-stream Dist... model) with closed-form weights."""
    from uncertainty_vit_amd.modeling_cyclical import (DistVisionTransformerForCyclicalTraining,
                                                       VisionTransformerForCyclicalTraining)
    cls = DistVisionTransformerForCyclicalTraining if two_stream else VisionTransformerForCyclicalTraining
    m = cls(img_size=cfg.img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim, depth=cfg.depth,
            num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, qkv_bias=True,
            norm_layer=partial(torch.nn.LayerNorm, eps=cfg.ln_eps), init_values=cfg.init_values,
            use_shared_rel_pos_bias=cfg.use_shared_rel_pos_bias, use_abs_pos_emb=cfg.use_abs_pos_emb and not two_stream,
            drop_path_rate=cfg.drop_path_rate, attn_drop_rate=cfg.attn_drop_rate)
    shapes = vd.param_shapes(cfg) if two_stream else vo.param_shapes(cfg)
    sd = closed_form_state(shapes, gamma=cfg.init_values if gamma is None else gamma)
    m.load_state_dict(sd, strict=False)
    return m.to(device), sd


class Args:
    opt, lr, weight_decay, opt_eps, opt_betas, momentum = "adamw", 2e-3, 0.05, 1e-8, (0.9, 0.999), 0.9


def native_trainer(model, lr=2e-3, wd=0.05, decay=0.9998):
    from uncertainty_vit_amd import optim_factory, utils
    a = Args()
    a.lr, a.weight_decay = lr, wd
    ema = utils.ModelEmaV2(model, decay=decay)
    opt = optim_factory.create_optimizer(a, model)
    return ema, opt


def native_steps(model, ema, opt, batches, target_layers, start=0, clip=3.0, l1_beta=2.0, decay=0.9998, l2_loss=False,
                 loss_scale=-1, post_target_layer_norm=True, stochastic=False, lam=1e-5, layer_results="end", var_w0=0.0,
                 var_margin0=0.5, **target_flags):
    """Each batch through the product's train_one_epoch (one-iteration loader); returns per-step stats."""
    from uncertainty_vit_amd import engine_for_cyclical as eng, utils
    out = []
    for s, (x, m) in enumerate(batches):
        loader = [((x, m), torch.zeros(1))]
        st = eng.train_one_epoch(model, ema, 0, decay, decay, target_layers, loader, opt, torch.device("cuda"), 0,
                                 utils.NativeScalerWithGradNormCount(), max_norm=clip, l1_beta=l1_beta, start_steps=start + s,
                                 layer_results=layer_results, var_w0=var_w0, var_margin0=var_margin0, loss_scale=loss_scale,
                                 **{"target_layer_norm_last": True, "post_target_layer_norm": post_target_layer_norm, **target_flags},
                                 l2_loss=l2_loss, stochastic=stochastic, lambda_pretraining=lam)
        out.append(st)
    return out


def oracle_state(sd):
    """(params, ema, adam m, adam v) dictionaries for the oracle, cloned from a closed-form state."""
    p = {k: v.clone() for k, v in sd.items()}
    e = {k: v.clone() for k, v in sd.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(t) for k, t in p.items()}
    return p, e, m, v


def grad_errors(native_grads, ref_grads, names=None):
    """Per tensor: (max-norm error / max|ref|, relative L2 error ||g - r|| / ||r||)."""
    out = {}
    for n in (names if names is not None else ref_grads.keys()):
        g, r = native_grads[n].detach().float().cpu().double(), ref_grads[n].double()
        rmax, rl2 = r.abs().max().item(), r.norm().item()
        out[n] = ((g - r).abs().max().item() / (rmax + 1e-30), (g - r).norm().item() / (rl2 + 1e-30))
    return out


def assert_grads_close(native_grads, ref_grads, names=None, max_tol=5e-2, l2_tol=2e-2, what=""):
    """Two bounds per tensor: the max-norm one (|g - r| <= max_tol * max|r|) catches a wrong large entry, the relative-L2
    one (||g - r|| <= l2_tol * ||r||) catches errors confined to many small-magnitude entries (a mis-indexed bias slice, a
    pad row leaking into a column sum) that the max-norm bound lets through."""
    errs = grad_errors(native_grads, ref_grads, names)
    worst = sorted(errs.items(), key=lambda kv: -kv[1][1])[:5]
    print(f"{what}worst relative-L2 gradient errors:", [(n, f"{e[1]:.2e}", f"max {e[0]:.2e}") for n, e in worst])
    bad = {n: e for n, e in errs.items() if e[0] > max_tol or e[1] > l2_tol}
    assert not bad, f"{what}gradient mismatch (max-norm ratio, relative L2): {bad}"


TOKENS = 197
# model: (C, hidden, largest k of k x 197 rows: the benchmarked batch)
MODELS = {"vitb": (768, 3072, 128), "vitl": (1024, 4096, 64), "vith": (1280, 5120, 128)}
# epilogue modes of include/uvit.h, with the operands tests/test_gpu_ops.py::_epilogue_modes gives them
QKV, RESID, GELU_DG, MULAUX, BF16 = 1, 3, 8, 9, 0


def launches(model):
    """name -> (N, K, epilogue) of the forward and dgrad launches of one Block."""
    Cd, Hd, _ = MODELS[model]
    return {"qkv": (3 * Cd, Cd, QKV), "proj": (Cd, Cd, RESID), "fc1": (Hd, Cd, GELU_DG), "fc2": (Cd, Hd, RESID),
            "dgrad_fc2": (Hd, Cd, MULAUX), "dgrad_fc1": (Cd, Hd, BF16)}


def nt_auto_plan(M, N, K, mode, cu=256, persist=True):
    """The auto dispatch (nt_variant 3) of uvit_gemm_nt_launch for an M x N x K launch, restated from the comments of its
    plan function (gemm_nt_plan in csrc/gemm.hip): (kernel, tail_rows) with kernel one of "128" (the 128x128 kernel: N % 256 != 0, M < 1024, K < 128 or K % 64 != 0),
    "320" (320-row tiles, taken when they save more than 10 % of rounds x rows), "256p" (256-row tiles, persistent: more tiles
    than `cu & ~7` workgroups; never for the MULAUX / DGELU epilogues) and "256"; tail_rows > 0 when 256-row tiles overflow whole
    rounds of the CUs by at most a quarter of them: the overflowing row tiles go to a second, 128x128 launch (not PATCH)."""
    if (N % 256) or M < 1024 or K < 128 or (K % 64):
        return "128", 0
    tn = N // 256
    ceil = lambda a, b: (a + b - 1) // b                                      # noqa: E731
    c4, c5 = ceil(ceil(M, 256) * tn, cu) * 256, ceil(ceil(M, 320) * tn, cu) * 320
    if c5 * 10 < c4 * 9:
        return "320", 0
    tail = 0
    if mode != 5:
        tiles = ceil(M, 256) * tn
        rounds = tiles // cu
        over = tiles - rounds * cu
        if rounds >= 1 and 0 < over and over * 4 <= cu:
            rows_a = (rounds * cu // tn) * 256
            if 0 < rows_a < M:
                tail, M = M - rows_a, rows_a
    grid = ceil(M, 256) * tn
    return ("256p" if persist and grid > (cu & ~7) and mode not in (6, 9) else "256"), tail


def nt_boundary_rows(N, K, mode, m_max, cu=256, persist=True):
    """Every M in [1, m_max] just below, at and just above a row count where nt_auto_plan changes its kernel or starts / stops
    splitting rows off, plus one 256-row tile to either side of each change between the persistent and the one-tile-per-workgroup form."""
    out = set()
    prev = nt_auto_plan(1, N, K, mode, cu, persist)
    for M in range(2, m_max + 1):
        cur = nt_auto_plan(M, N, K, mode, cu, persist)
        if (cur[0], cur[1] > 0) != (prev[0], prev[1] > 0):
            out.update((M - 2, M - 1, M, M + 1))
            if {cur[0], prev[0]} == {"256", "256p"}:
                out.update((M - 1 - 256, M - 1 + 256))
        prev = cur
    return sorted(m for m in out if 1 <= m <= m_max)


# ---- schedules of tests/test_gpu_history.py (their properties are asserted without a GPU by tests/test_host_history.py) ----
HISTORY_SEED = 4321
# Per schedule: the model, the batch size, and the steps in order.  A step is ("step", iteration, options) or ("eval", batch size);
# options: lists=False switches the drop-path sample lists off for that step, masked=N gives the step host-side ragged masks with N
# masked patches in all (the host's count becomes n_rows_hint: the masked-row last block), oracle=True also compares the step on
# a fresh engine with the float64 oracle.
HISTORY = {
    # kept samples per (branch; layer 0..3) at B = 3: it 8 [[3,3,2,3],[3,3,2,2]], it 1 [[3,2,0,0],[3,3,3,2]], it 9 [[3,3,1,3],[3,3,0,0]],
    # it 15 [[3,2,2,2],[3,2,3,3]], it 16 [[3,2,3,1],[3,3,2,1]], it 21 [[3,3,2,1],[3,2,3,3]], it 5 [[3,2,2,1],[3,3,3,2]], it 12 [[3,3,1,2],[3,3,3,2]]
    "tiny": dict(cfg=dict(img_size=48, embed_dim=128, depth=4, num_heads=2, drop_path_rate=0.5, attn_drop_rate=0.1), B=3, n_mask=4,
                 target_layers=[2, 3], two_stream=False,
                 steps=[("step", 8, {}), ("step", 1, dict(oracle=True)), ("step", 9, dict(oracle=True)), ("step", 15, {}), ("step", 16, {}),
                        ("step", 21, dict(lists=False)), ("step", 5, {}), ("step", 12, {})]),
    # ViT-B/16, B = 32: R = roundup(masked, 64) = 2432, 2304 (a shrink across a multiple of 64), [eval forward at B = 5], 2432, 0 (device-side
    # masks: the dense last block), 1024, 1536
    "vitb32": dict(cfg=dict(drop_path_rate=0.5, attn_drop_rate=0.05), B=32, n_mask=75, target_layers=list(range(6, 12)), two_stream=False,
                   steps=[("step", 0, dict(masked=2400)), ("step", 1, dict(masked=2290)), ("eval", 5), ("step", 2, dict(masked=2400)),
                          ("step", 3, {}), ("step", 4, dict(masked=1000)), ("step", 5, dict(masked=1500))]),
    # kept samples of the MLP branch per layer (mean stream; covariance stream) at B = 4: it 10 [4,4,2,3; 4,3,3,3], it 5 [4,3,3,3; 4,2,2,2],
    # it 6 [4,4,3,2; 4,2,3,3] (layer 3: the mean stream's list shrinks 3 -> 2 while the covariance stream's grows 2 -> 3), it 8 [4,2,2,2; 4,3,4,0],
    # it 12 [4,3,4,3; 4,3,1,1], it 27 [4,4,4,2; 4,4,3,2]
    "tiny2": dict(cfg=dict(img_size=48, embed_dim=128, depth=4, num_heads=2, drop_path_rate=0.5, attn_drop_rate=0.05), B=4, n_mask=4,
                  target_layers=[2, 3], two_stream=True,
                  steps=[("step", 10, {}), ("step", 5, {}), ("step", 6, {}), ("step", 8, {}), ("step", 12, {}), ("step", 27, {})]),
    # the head_dim-80 fixture shape (tests/golden/model_hd80.npz); kept samples of layer 1 (attention, MLP) at B = 4: it 6 (4, 3), it 0 (3, 2), it 3 (1, 3)
    "hd80": dict(cfg=dict(img_size=48, embed_dim=320, depth=2, num_heads=4, drop_path_rate=0.5, attn_drop_rate=0.1), B=4, n_mask=4,
                 target_layers=[1], two_stream=False, steps=[("step", 6, {}), ("step", 0, {}), ("step", 3, {})]),
}


def history_cfg(name):
    return vo.VitConfig(init_values=0.1, **HISTORY[name]["cfg"])


def history_kept_counts(name, it):
    """(depth, draws) kept samples per (layer, draw) of a schedule's step, from the oracle's replay of the drop-path draws (pinned to
    uvit_drop_path_kept_counts by tests/test_host_cpu.py); draws = (attention, MLP), two-stream: (mean attn, mean MLP, cov attn, cov MLP)."""
    h, cfg = HISTORY[name], history_cfg(name)
    cols = vd.drop_path_scales(HISTORY_SEED, it, cfg, h["B"]) if h["two_stream"] else list(vo.drop_path_scales(HISTORY_SEED, it, cfg, h["B"]))
    return [[h["B"] if c[l] is None else int((c[l] != 0).sum()) for c in cols] for l in range(cfg.depth)]


def ragged_masks(B, n_patches, total, seed):
    """(B, g, g) int64 masks with `total` ones in all and another count per sample (the mean +- up to 8, in pairs that cancel)."""
    base, rem = divmod(total, B)
    counts = [base + (1 if i < rem else 0) for i in range(B)]
    for i in range(0, B - 1, 2):
        d = min(1 + (i // 2 + seed) % 8, counts[i + 1], n_patches - counts[i])
        counts[i] += d
        counts[i + 1] -= d
    assert sum(counts) == total and all(0 <= c <= n_patches for c in counts)
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, n_patches, dtype=torch.int64)
    for b in range(B):
        m[b, torch.randperm(n_patches, generator=g)[:counts[b]]] = 1
    side = int(round(n_patches ** 0.5))
    return m.reshape(B, side, side)


def history_batch(name, index):
    """(images, mask, host_side) of step `index` of a schedule: CPU tensors; host_side = the mask stays on the host (n_rows_hint)."""
    from oracle.closed_form import closed_form_images, exact_masks
    h, cfg = HISTORY[name], history_cfg(name)
    kind, arg, opt = (h["steps"][index] + ({},))[:3]
    B = h["B"] if kind == "step" else arg
    x = closed_form_images(f"history/{name}/{index}", B, cfg.img_size)
    if kind == "step" and "masked" in opt:
        return x, ragged_masks(B, cfg.num_patches, opt["masked"], 100 + index), True
    return x, exact_masks(B, cfg.num_patches, h["n_mask"], 100 + index), False


def full_size_step_properties(cfg_drop, cfg_nodrop, B, img, n_patches, n_mask, target_layers, two_stream=False, lam=1e-5,
                              lr=2e-3, wd=0.05, decay=0.9998, tag="full"):
    """Size-independent properties of ONE full-size step (the oracle cannot run these sizes in seconds):
    reported grad-norm = norm of the gradient arena, the AdamW bound |dw| <= lr (+ decay) with dw = -lr sign(g) where the
    clipped gradient is not tiny, the EMA identity, replay determinism of the counter-based dropout (same seed -> same
    loss, other seed -> other loss), frozen tensors untouched, and linearity of the gradient in the batch (dropout off:
    grad(B) = mean of the two half batches, every image having the same number of masked rows)."""
    import numpy as np
    import pytest
    from oracle.closed_form import closed_form_images, exact_masks
    x = closed_form_images(tag, B, img).cuda()
    mask = exact_masks(B, n_patches, n_mask, 77).cuda()

    def one_step(c, xs, ms, seed=99, lam=lam):
        model, _ = native_model(c, two_stream=two_stream)
        ema, opt = native_trainer(model, lr=lr, wd=wd, decay=decay)
        p0 = {n: t.detach().clone() for n, t in model.state_dict().items()}
        torch.manual_seed(seed)
        st = native_steps(model, ema, opt, [(xs, ms)], target_layers, start=3, clip=3.0, decay=decay, stochastic=two_stream,
                          lam=lam)[0]
        return model, ema, p0, st

    model, ema, p0, st = one_step(cfg_drop, x, mask)
    assert np.isfinite(st["loss"]) and 0.0 < st["loss"] < 10.0
    g = model._grad_arena
    gn = float(torch.sqrt((g.double() ** 2).sum()))
    assert st["grad_norm"] == pytest.approx(gn, rel=1e-4)
    coef = min(1.0, 3.0 / (gn + 1e-6))
    sd, esd = model.state_dict(), ema.module.state_dict()
    frozen = {n for n, _, _, _, dk in model._layout if dk == 2}
    decay_names = {n for n, p in model.named_parameters() if p.ndim > 1 and n not in ("cls_token", "pos_embed")}
    for n, p in model.named_parameters():
        if n in frozen:        # dead cov_qkv.weight: no gradient, no AdamW, no weight decay; EMA of an unchanged value
            assert torch.equal(sd[n], p0[n]) and float(p.grad.abs().sum()) == 0.0, n
            continue
        d = sd[n] - p0[n] * ((1 - lr * wd) if n in decay_names else 1.0)
        assert float(d.abs().max()) <= lr * (1 + 1e-3), n                    # first AdamW step: |m / sqrt(v)| <= 1
        big = (p.grad.abs() * coef) > 1e-5                                   # there the first step is exactly -lr * sign(g)
        if big.any():
            torch.testing.assert_close(d[big], -lr * torch.sign(p.grad[big]), rtol=0, atol=lr * 2e-3)
        torch.testing.assert_close(esd[n], decay * p0[n] + (1 - decay) * sd[n], rtol=0, atol=1e-7 + 2e-7 * float(p0[n].abs().max()))
    del model, ema
    # replay: same seed and iteration -> the same dropout masks -> the same loss (split-K atomics reorder fp32 sums)
    m2, _, _, st2 = one_step(cfg_drop, x, mask)
    del m2
    assert st2["loss"] == pytest.approx(st["loss"], rel=1e-5)
    m3, _, _, st3 = one_step(cfg_drop, x, mask, seed=100)
    del m3
    assert abs(st3["loss"] - st["loss"]) > 1e-7                              # another seed, another mask set
    # WassersteinLoss normalises by a batch-global max, so its gradient is not linear in the batch: lambda = 0 there
    ll = 0.0 if two_stream else lam
    mfull, _, _, _ = one_step(cfg_nodrop, x, mask, lam=ll)
    gfull = {n: p.grad.clone() for n, p in mfull.named_parameters()}
    del mfull
    h = B // 2
    ma, _, _, _ = one_step(cfg_nodrop, x[:h], mask[:h], lam=ll)
    ga = {n: p.grad.clone() for n, p in ma.named_parameters()}
    del ma
    mb, _, _, _ = one_step(cfg_nodrop, x[h:], mask[h:], lam=ll)
    for n, p in mb.named_parameters():
        if n in frozen:
            continue
        ref = 0.5 * (ga[n] + p.grad)
        err = float((gfull[n] - ref).abs().max())
        assert err <= 2e-2 * float(ref.abs().max()) + 1e-9, (n, err, float(ref.abs().max()))
        rl2 = float((gfull[n] - ref).norm() / (ref.norm() + 1e-30))
        assert rl2 <= 2e-2, (n, "relative L2", rl2)
    return st


# ---- the multi-step epoch of tests/test_gpu_epoch.py (its properties are asserted without a GPU by tests/test_host_epoch.py) ----
# One train_one_epoch call: 9 iterations from global iteration 3 (step != it; more than two laps of the 4-slot metrics ring).  The lr and
# weight-decay tables are indexed by GLOBAL iteration, neighbouring entries a factor >= 2 apart and not monotone, no lr entry equal to a
# weight-decay or EMA-decay value: a scalar read at a neighbouring index, or from another row of the device table, is far outside every bound.
# EMA: iterations 3..6 anneal (it < ema_start_at), 7..9 keep the value of iteration 6, 10..11 skip the update (it > start_lr_decay_at_step).
# n_mask / scale: masked patches per image and image scale of batch i.  The targets are layer-normed rows, so at the closed-form weights every
# batch of noise images has a loss near 0.28 whatever its scale; what moves the loss is learning.  The images of scale 0.02 are nearly constant:
# their targets are nearly one vector, which the student learns within a step, while the scale-2 noise batches between them stay near 0.28 --
# consecutive losses are >= 25 % apart, and not monotone.
EPOCH = dict(cfg=dict(img_size=48, embed_dim=128, depth=2, num_heads=2), B=3, target_layers=[1], start_steps=3, n_iters=9,
             ema_start_at=7, decay_init=0.99, decay=0.9998, start_lr_decay_at_step=9, max_norm=3.0, betas=(0.9, 0.999), eps=1e-8,
             lr=[7.5e-4, 2e-4, 6e-4, 1.5e-3, 5e-4, 1.25e-3, 2.5e-4, 1e-3, 4e-4, 1.4e-3, 4.5e-4, 1.2e-3],
             wd=[0.05, 0.2, 0.02, 0.1, 0.03, 0.12, 0.04, 0.16, 0.01, 0.08, 0.025, 0.11],
             n_mask=[2, 7, 3, 8, 1, 6, 2, 8, 4], scale=[0.02, 0.02, 2.0, 0.02, 2.0, 0.02, 2.0, 0.02, 2.0])


def epoch_cfg():
    return vo.VitConfig(init_values=0.1, **EPOCH["cfg"])


def epoch_batch(i, tag="epoch"):
    """(images, mask) of iteration i of the epoch: CPU tensors."""
    from oracle.closed_form import closed_form_images, exact_masks
    cfg = epoch_cfg()
    return (closed_form_images(f"{tag}/{i}", EPOCH["B"], cfg.img_size, EPOCH["scale"][i % len(EPOCH["scale"])]),
            exact_masks(EPOCH["B"], cfg.num_patches, EPOCH["n_mask"][i % len(EPOCH["n_mask"])], 200 + i))


def epoch_table(optimizer=None):
    """[(lr, weight_decay, ema_decay or -1.0)] of the epoch's iterations, from the product's epoch_scalars (float32 values)."""
    from types import SimpleNamespace
    from uncertainty_vit_amd.engine_for_cyclical import epoch_scalars
    E = EPOCH
    opt = optimizer or SimpleNamespace(param_groups=[dict(lr=Args.lr, weight_decay=Args.weight_decay, lr_scale=1.0)])
    return epoch_scalars(opt, E["start_steps"], E["n_iters"], E["lr"], E["wd"], E["ema_start_at"], E["decay_init"], E["decay"],
                         E["start_lr_decay_at_step"])


_oracle_epoch = None


def oracle_epoch():
    """The epoch in the oracle, computed once per process: per-iteration (loss, grad_norm) lists.  A skipped EMA update is decay = 1.0,
    which leaves the oracle's teacher bit for bit (1.0 * e + 0.0 * p)."""
    global _oracle_epoch
    if _oracle_epoch is None:
        cfg = epoch_cfg()
        p, e, m, v = oracle_state(closed_form_state(vo.param_shapes(cfg), gamma=cfg.init_values))
        hp = vo.StepHParams(target_layers=tuple(EPOCH["target_layers"]), clip_grad=EPOCH["max_norm"], betas=EPOCH["betas"], eps=EPOCH["eps"])
        loss, gnorm = [], []
        for i, (lr, wd, d) in enumerate(epoch_table()):
            if d < 0:
                before = {k: t.clone() for k, t in e.items()}
            x, mask = epoch_batch(i)
            r = vo.train_step(p, e, m, v, cfg, hp, x, mask, i + 1, lr=lr, wd=wd, decay=1.0 if d < 0 else d)
            if d < 0:
                assert all(torch.equal(before[k], e[k]) for k in e)
            loss.append(r.loss)
            gnorm.append(r.grad_norm)
        _oracle_epoch = (loss, gnorm)
    return _oracle_epoch


def epoch_run(model, ema, opt, loader, writer, **kw):
    """One train_one_epoch call with the EPOCH schedules (kw overrides) over `loader`."""
    from uncertainty_vit_amd import engine_for_cyclical as eng, utils
    E = EPOCH
    args = dict(max_norm=E["max_norm"], l1_beta=2.0, log_writer=writer, start_steps=E["start_steps"], lr_schedule_values=E["lr"],
                wd_schedule_values=E["wd"], start_lr_decay_at_step=E["start_lr_decay_at_step"], target_layer_norm_last=True,
                post_target_layer_norm=True)
    args.update(kw)
    return eng.train_one_epoch(model, ema, E["ema_start_at"], E["decay_init"], E["decay"], E["target_layers"], loader, opt,
                               torch.device("cuda"), 0, utils.NativeScalerWithGradNormCount(), **args)


class RecordingLoader:
    """An iterable of ((images, mask), label) batches that records the training state each time the next batch is requested.

    DevicePrefetcher.__iter__ asks for batch k on the compute stream after steps 0 .. k-2 have been enqueued and before step k-1 is, so
    snapshot k (clones enqueued on the current stream: no synchronisation, no launch between two steps' kernels other than the copies)
    is the state after k-1 steps with the raw gradients, the loss words and compact_rows() of step k-2.  When the loader runs out, one
    more snapshot is taken (index n: after n-1 steps); the test appends the last one after the epoch has returned."""

    def __init__(self, batches, model, ema, opt):
        self.batches, self.model, self.ema, self.opt = list(batches), model, ema, opt
        self.requested, self.snapshots = [], []

    def __len__(self):
        return len(self.batches)

    def snapshot(self):
        m, e = self.model, self.model._engine
        s = {"params": m._arena.clone(), "teacher": self.ema.module._arena.clone()}
        if self.opt.exp_avg is not None:
            s["m"], s["v"] = self.opt.exp_avg.clone(), self.opt.exp_avg_sq.clone()
        if m._grad_arena is not None:
            s["grads"] = m._grad_arena.clone()
        if e is not None:
            s["params_bf16"], s["ema_bf16"] = e.params_bf16.clone(), e.ema_bf16.clone()
            s["stats"] = e.ws_tensor("loss", 0, (8,)).clone()
            s["compact"] = e.compact_rows()
        self.snapshots.append(s)
        return s

    def __iter__(self):
        for k, (x, mask) in enumerate(self.batches):
            self.requested.append(k)
            self.snapshot()
            yield (x, mask), torch.zeros(1)
        self.snapshot()


class RecordingWriter:
    """utils.TensorboardLogger's update(head=..., **kw) / set_step() interface; one dict per set_step() with what was published."""

    def __init__(self):
        self.records, self._cur = [], {}

    def update(self, head="scalar", step=None, **kw):
        self._cur.update(kw)

    def set_step(self, step=None):
        self.records.append(self._cur)
        self._cur = {}

    def flush(self):
        pass


def expected_update(P0, M0, V0, E0, g, lr, wd, ema_decay, step, n_decay, clip, betas, eps):
    """Float64 restatement, on flat arenas, of global-norm clip (utils.py:375-376), torch.optim.AdamW with weight decay on [0, n_decay)
    only, and the EMA e <- d e + (1 - d) p_new; `step` is 1-based, ema_decay None = the teacher is returned unchanged.  The scalars are
    rounded to float32 first, as the C ABI carries them.  Returns (P, M, V, E, unclipped norm) as float64 CPU tensors."""
    import numpy as np
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    d64 = lambda t: t.detach().cpu().double()  # noqa: E731
    lr, wd, b1, b2, eps = f32(lr), f32(wd), f32(betas[0]), f32(betas[1]), f32(eps)
    P, M, V, E, g = d64(P0).clone(), d64(M0), d64(V0), d64(E0), d64(g)
    norm = float(torch.sqrt((g * g).sum()))
    if clip:
        g = g * min(1.0, f32(clip) / (norm + 1e-6))
    P[:n_decay] *= 1.0 - lr * wd
    M = b1 * M + (1.0 - b1) * g
    V = b2 * V + (1.0 - b2) * g * g
    P -= (lr / (1.0 - b1 ** step)) * M / (V.sqrt() / (1.0 - b2 ** step) ** 0.5 + eps)
    if ema_decay is not None:
        d = f32(ema_decay)
        E = d * E + (1.0 - d) * P
    return P, M, V, E, norm
