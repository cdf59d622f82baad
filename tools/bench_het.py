"""Time the heteroscedastic probe head beside the linear head on synthetic data (default: beit_base_patch16_224, bs = 128, K = 1000,
R = 10 factors, S = 1000 Monte-Carlo samples) on one GPU.

    python tools/bench_het.py [--model M] [--batch B] [--classes K] [--factors R] [--samples S] [--iters N] [--warmup W] [--out FILE]

Prints one JSON line: the het training step (encoder eval forward + pool/norm + the (K (R + 2), C) head + Monte-Carlo softmax +
cross-entropy + Monte-Carlo backward + head gradient + clip norm + AdamW), the linear head's training step and the encoder's eval
forward alone on the same batch, alternating, so that the ratios do not depend on which ran on a quieter machine; an evaluation batch
(forward + head + Monte-Carlo softmax) with and without the predictive variance; and the time of each op alone.  Every figure is a
device-event bracket around `iters` back-to-back calls after `warmup` calls of the same shape, divided by `iters`.  Needs a GPU.
"""
import argparse
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
    ap.add_argument("--factors", type=int, default=10)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_het.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.het_probe import EPS, HetProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    het = HetProbe(model, a.classes, num_factors=a.factors, train_mc_samples=a.samples, test_mc_samples=a.samples)
    lin = LinearProbe(model, a.classes)
    B, K, Cd, R, S = a.batch, a.classes, model.embed_dim, a.factors, a.samples
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    for p in (het, lin):
        loss, _ = p.train_step(x, y, 1e-3, 0.05, 1.0)
        assert bool(torch.isfinite(loss))
    L, s, T = lib(), cur_stream, f32(het.temperature)
    rows = het._rows
    eR, eK = torch.zeros(4 * S * R, device="cuda"), torch.zeros(4 * S * K, device="cuda")
    parts = {
        "head_logits": lambda: check(L.uvit_op_probe_logits(ptr(het._feat), ptr(het._arena), het._bias_ptr(het._arena), ptr(het._lin), B, rows, Cd, s())),
        "mc_forward": lambda: check(L.uvit_op_het_mc_forward(ptr(het._lin), ptr(het._logits), ptr(het._p), None, ptr(het._het_scratch), B, S, K, R, T,
                                                             f32(EPS), 42, 0, s())),
        "mc_forward_pvar": lambda: check(L.uvit_op_het_mc_forward(ptr(het._lin), ptr(het._logits), ptr(het._p), ptr(het._pvar), ptr(het._het_scratch), B,
                                                                  S, K, R, T, f32(EPS), 42, 1, s())),
        "mc_backward": lambda: check(L.uvit_op_het_mc_backward(ptr(het._lin), ptr(het._p), ptr(het._dlogits), ptr(het._dlin), ptr(het._het_scratch), B, S,
                                                               K, R, T, f32(EPS), 42, 0, s())),
        "head_grad": lambda: check(L.uvit_op_probe_head_grad(ptr(het._dlin), ptr(het._feat), ptr(het._grad_arena), het._bias_ptr(het._grad_arena), B,
                                                             rows, Cd, s())),
        "noise_4_rows": lambda: check(L.uvit_op_het_noise(ptr(eR), ptr(eK), 4, S, K, R, 42, 0, s())),
    }
    ms = {k: timed(fn, a.iters, a.warmup) for k, fn in parts.items()}

    def eval_batch(variance):
        n = het._features(x)
        het._mc_into(n, het.test_mc_samples, het.seed, 1, pvar=variance)

    groups = []
    for _ in range(a.repeats):
        fwd = timed(lambda: model.forward_features(x, None, None), a.iters, a.warmup)
        lin_step = timed(lambda: lin.train_step(x, y, 1e-3, 0.05, 1.0), a.iters, a.warmup)
        het_step = timed(lambda: het.train_step(x, y, 1e-3, 0.05, 1.0), a.iters, a.warmup)
        ev = timed(lambda: eval_batch(False), a.iters, a.warmup)
        ev_var = timed(lambda: eval_batch(True), a.iters, a.warmup)
        groups.append((fwd, lin_step, het_step, ev, ev_var))
    med = [sorted(grp[i] for grp in groups)[len(groups) // 2] for i in range(5)]
    fwd, lin_step, het_step, ev, ev_var = med
    terms = B * S * K
    out = {"model": a.model, "batch": B, "classes": K, "factors": R, "samples": S, "iters": a.iters, "encoder_forward_ms": round(fwd, 4),
           "linear_step_ms": round(lin_step, 4), "het_step_ms": round(het_step, 4), "linear_step_over_encoder_forward": round(lin_step / fwd, 4),
           "het_step_over_encoder_forward": round(het_step / fwd, 4), "het_step_over_linear_step": round(het_step / lin_step, 4),
           "eval_batch_ms": round(ev, 4), "eval_batch_variance_ms": round(ev_var, 4), "variance_over_eval_batch": round(ev_var / ev, 4),
           "eval_batch_over_encoder_forward": round(ev / fwd, 4), "groups_ms": [[round(v, 4) for v in grp] for grp in groups],
           "part_ms": {k: round(v, 4) for k, v in ms.items()}, "softmax_terms": terms,
           "mc_forward_ns_per_kiloterm": round(ms["mc_forward"] * 1e6 / (terms / 1e3), 4),
           "mc_backward_ns_per_kiloterm": round(ms["mc_backward"] * 1e6 / (terms / 1e3), 4),
           "scratch_bytes": int(L.uvit_op_het_mc_ws_bytes(B, S, K, R)), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
