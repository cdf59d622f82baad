"""Time the GP probe head beside the linear head on synthetic data (default: beit_base_patch16_224, bs = 128, K = 1000, D = embed dim)
on one GPU.

    python tools/bench_gp.py [--model M] [--batch B] [--classes K] [--inducing D] [--iters N] [--warmup W] [--out FILE]

Prints one JSON line: the GP training step (encoder eval forward + pool/norm + features + logits + precision update + cross-entropy +
output-layer gradient + LayerNorm gradients + clip norm + AdamW), the linear head's training step and the encoder's eval forward alone
on the same batch, alternating, so that the ratios do not depend on which ran on a quieter machine; an evaluation batch (forward +
logits) with and without the predictive variance; and the time of each new op.  Every figure is a device-event bracket around `iters`
back-to-back calls after `warmup` calls of the same shape, divided by `iters`: for the small ops that is launch spacing as much as
kernel time.  inv(P) is formed on the host once before the timed region (P does not change during an evaluation).  Needs a GPU.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--inducing", type=int, default=0, help="random features D (0: the embed dim)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gp.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.gp_probe import LN_EPS, GPProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    gp, lin = GPProbe(model, a.classes, num_inducing=a.inducing or None), LinearProbe(model, a.classes)
    B, K, Cd, D = a.batch, a.classes, model.embed_dim, gp.num_inducing
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    for p in (gp, lin):
        loss, _ = p.train_step(x, y, 1e-3, 0.05, 1.0)
        assert bool(torch.isfinite(loss))
    L, s = lib(), cur_stream
    h, g = gp.head, gp._grad_arena.data_ptr()
    sigma = gp._sigma()
    parts = {
        "features": lambda: check(L.uvit_op_gp_features(ptr(gp._feat), ptr(h._gp_input_normalize_layer.weight), ptr(h._gp_input_normalize_layer.bias),
                                                        ptr(gp._w_rf), ptr(gp._b_rf), f32(gp.feature_scale), f32(LN_EPS), ptr(gp._ghat), ptr(gp._u),
                                                        ptr(gp._phi), B, Cd, D, s())),
        "precision_update": lambda: check(L.uvit_op_gp_precision_update(ptr(gp._phi), ptr(gp._P), B, D, C.c_double(0.999), s())),
        "ln_grad": lambda: check(L.uvit_op_gp_ln_grad(ptr(gp._dlogits), ptr(gp._arena), ptr(gp._u), ptr(gp._w_rf), ptr(gp._ghat), f32(gp.feature_scale),
                                                      C.c_void_p(g + 4 * K * D), C.c_void_p(g + 4 * (K * D + Cd)), ptr(gp._gp_scratch), B, K, Cd, D, s())),
        "variance": lambda: check(L.uvit_op_gp_variance(ptr(gp._phi), ptr(sigma), C.c_double(gp.ridge), ptr(gp._var), B, D, s())),
        "mean_field": lambda: check(L.uvit_op_gp_mean_field(ptr(gp._logits), ptr(gp._var), C.c_double(0.0), ptr(gp._logits), B, K, s())),
    }
    ms = {k: timed(fn, a.iters, a.warmup) for k, fn in parts.items()}
    gp.reset_cov()
    gp.train_step(x, y, 1e-3, 0.05, 1.0)
    gp._sigma()                                   # formed on the host, outside the timed region

    def eval_batch(variance):
        n = gp._features(x)
        gp._var_slabs = [] if variance else None
        gp._logits_into(n)
        gp._var_slabs = None

    groups = []
    for _ in range(a.repeats):
        fwd = timed(lambda: model.forward_features(x, None, None), a.iters, a.warmup)
        lin_step = timed(lambda: lin.train_step(x, y, 1e-3, 0.05, 1.0), a.iters, a.warmup)
        gp_step = timed(lambda: gp.train_step(x, y, 1e-3, 0.05, 1.0), a.iters, a.warmup)
        gp._sigma()
        ev = timed(lambda: eval_batch(False), a.iters, a.warmup)
        ev_var = timed(lambda: eval_batch(True), a.iters, a.warmup)
        groups.append((fwd, lin_step, gp_step, ev, ev_var))
    med = [sorted(grp[i] for grp in groups)[len(groups) // 2] for i in range(5)]
    fwd, lin_step, gp_step, ev, ev_var = med
    out = {"model": a.model, "batch": B, "classes": K, "inducing": D, "iters": a.iters, "encoder_forward_ms": round(fwd, 4),
           "linear_step_ms": round(lin_step, 4), "gp_step_ms": round(gp_step, 4), "linear_step_over_encoder_forward": round(lin_step / fwd, 4),
           "gp_step_over_encoder_forward": round(gp_step / fwd, 4), "gp_step_over_linear_step": round(gp_step / lin_step, 4),
           "eval_batch_ms": round(ev, 4), "eval_batch_variance_ms": round(ev_var, 4), "variance_over_eval_batch": round(ev_var / ev, 4),
           "groups_ms": [[round(v, 4) for v in grp] for grp in groups], "part_ms": {k: round(v, 4) for k, v in ms.items()},
           "variance_dfma": B * D * D + B * D, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
