"""Time the linear-probe step on synthetic data (default: beit_base_patch16_224, bs = 128, K = 1000) on one GPU.

    python tools/bench_probe.py [--model M] [--batch B] [--classes K] [--iters N] [--warmup W] [--out FILE]

Prints one JSON line: img/s of the whole step (encoder eval forward + pool/norm + logits + cross-entropy + head gradient + clip
norm + AdamW), the time of each part, the step as a ratio over the encoder's eval forward alone (uvit_engine_forward_features with
training = 0 on the same batch -- the comparison DESIGN.md section 9 reports), and the pool kernel's GB/s (the bytes of the residual
stream it reads, B N C 4, over its time).  Every figure is a device-event bracket around `iters` back-to-back calls after `warmup`
calls of the same shape, divided by `iters`: for the four small parts that is launch spacing as much as kernel time.  Needs a GPU;
there is nothing to time without one.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters        # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the step / forward pair to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probe.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(model, a.classes)
    B, K, Cd, N = a.batch, a.classes, model.embed_dim, model.patch_embed.num_patches + 1
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    loss, _ = probe.train_step(x, y, 1e-3, 0.05, 1.0)
    assert bool(torch.isfinite(loss))
    L, e = lib(), model._engine
    xs = C.c_void_p(L.uvit_engine_ws_ptr(e.h, b"x", model.depth))
    bias = C.c_void_p(probe._arena.data_ptr() + 4 * K * Cd)
    dbias = C.c_void_p(probe._grad_arena.data_ptr() + 4 * K * Cd)
    n = probe._arena.numel()

    def adamw():
        probe._sumsq.zero_()
        check(L.uvit_op_sumsq(ptr(probe._grad_arena), n, ptr(probe._sumsq), cur_stream()))
        check(L.uvit_op_adamw(ptr(probe._arena), ptr(probe._grad_arena), ptr(probe.exp_avg), ptr(probe.exp_avg_sq), None, n, K * Cd,
                              f32(1e-3), f32(0.05), f32(0.9), f32(0.999), f32(1e-8), 2, ptr(probe._sumsq), f32(1.0), f32(1.0), None,
                              cur_stream()))

    parts = {
        "encoder_forward": lambda: model.forward_features(x, None, None),
        "pool_norm": lambda: check(L.uvit_op_probe_pool_norm(xs, ptr(probe._feat), ptr(probe._scratch), B, N, Cd, f32(1e-6), cur_stream())),
        "logits": lambda: check(L.uvit_op_probe_logits(ptr(probe._feat), ptr(probe._arena), bias, ptr(probe._logits), B, K, Cd, cur_stream())),
        "cross_entropy": lambda: check(L.uvit_op_probe_ce(ptr(probe._logits), ptr(y), f32(0.1), ptr(probe._dlogits), ptr(probe._row_loss),
                                                          ptr(probe._stats), None, B, K, cur_stream())),
        "head_grad": lambda: check(L.uvit_op_probe_head_grad(ptr(probe._dlogits), ptr(probe._feat), ptr(probe._grad_arena), dbias, B, K, Cd,
                                                             cur_stream())),
        "sumsq_adamw": adamw,
    }
    ms = {k: timed(fn, a.iters, a.warmup) for k, fn in parts.items()}
    # the step and the forward alone, alternating, so that the ratio does not depend on which ran on a quieter machine
    pairs = []
    for _ in range(a.repeats):
        fwd = timed(parts["encoder_forward"], a.iters, a.warmup)
        step = timed(lambda: probe.train_step(x, y, 1e-3, 0.05, 1.0), a.iters, a.warmup)
        pairs.append((step, fwd))
    step_ms = sorted(p[0] for p in pairs)[len(pairs) // 2]
    fwd_ms = sorted(p[1] for p in pairs)[len(pairs) // 2]
    pool_bytes = B * N * Cd * 4
    out = {"model": a.model, "batch": B, "classes": K, "iters": a.iters, "step_ms": round(step_ms, 4), "img_per_s": round(B / step_ms * 1e3, 1),
           "encoder_forward_ms": round(fwd_ms, 4), "step_over_encoder_forward": round(step_ms / fwd_ms, 4),
           "step_fwd_pairs_ms": [[round(s, 4), round(f, 4)] for s, f in pairs],
           "part_ms": {k: round(v, 4) for k, v in ms.items()}, "pool_bytes": pool_bytes,
           "pool_GBps": round(pool_bytes / (ms["pool_norm"] * 1e-3) / 1e9, 1),
           "head_gflop": round(2.0 * B * K * Cd / 1e9, 4), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
