"""Time the two-stream probe on synthetic data (default: dist_beit_base_patch16_224, bs = 128, K = 1000) on one GPU.

    python tools/bench_dist.py [--model M] [--batch B] [--classes K] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.  In every repeat, alternating, so that the ratios do not depend on which ran on a quieter machine: the pair op
uvit_op_dprobe_pool_norm on the engine's two last-block streams, two successive uvit_op_probe_pool_norm calls on the same streams,
uvit_op_dprobe_variance (with the trace) plus uvit_op_lap_probit, the encoder's eval forward alone and a DistProbe evaluation batch
(forward + pair op + logits + variance + link).  Every figure is a device-event bracket around `iters` back-to-back calls after
`warmup` calls of the same shape, divided by `iters`: for the small ops that is launch spacing as much as kernel time.  The reported
value is the median over the repeats, `spread` the (max - min) / median of each.  Needs a GPU.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_probe import timed  # noqa: E402

NAMES = ("pair_pool_norm", "two_pool_norm_calls", "variance_and_link", "encoder_forward", "dist_eval_batch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="dist_beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dist.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.dist_probe import DIST_MEAN_FIELD, DistProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    probe = DistProbe(model, a.classes, mean_field=DIST_MEAN_FIELD)
    B, K, Cd, N = a.batch, a.classes, model.embed_dim, model.patch_embed.num_patches + 1
    with torch.no_grad():
        probe.head.weight.normal_(0.0, 0.05)
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    probe.logits(x)                                      # allocates the buffers, leaves both streams in the engine workspace
    L, s = lib(), cur_stream
    e = model.engine(B)
    xm, xc = (C.c_void_p(L.uvit_engine_ws_ptr(e.h, name, model.depth)) for name in (b"x", b"x_cov"))
    feat2 = torch.zeros_like(probe._feat)
    eps = f32(model.ln_eps)

    def two_calls():
        check(L.uvit_op_probe_pool_norm(xm, ptr(probe._feat), ptr(probe._scratch), B, N, Cd, eps, s()))
        check(L.uvit_op_probe_pool_norm(xc, ptr(feat2), ptr(probe._scratch), B, N, Cd, eps, s()))

    def variance_and_link():
        probe._variance_into(B, trace=probe._dist_trace)
        check(L.uvit_op_lap_probit(ptr(probe._logits), K, ptr(probe._dist_var), C.c_double(probe.mean_field), ptr(probe._dlogits), K,
                                   ptr(probe._dist_col), B, K, s()))

    fns = (lambda: check(L.uvit_op_dprobe_pool_norm(xm, xc, ptr(probe._feat), ptr(probe._cfeat), ptr(probe._scratch), B, N, Cd, eps, s())),
           two_calls, variance_and_link, lambda: model.forward_features(x, None, None), lambda: probe._logits_into(probe._features(x)))
    two_calls()
    same = bool(torch.equal(feat2, probe._cfeat))        # the pair op's covariance feature, from the probe.logits call above
    groups = [[timed(fn, a.iters, a.warmup) for fn in fns] for _ in range(a.repeats)]
    cols = list(zip(*groups))
    med = {n: sorted(c)[len(c) // 2] for n, c in zip(NAMES, cols)}
    spread = {n: (max(c) - min(c)) / med[n] for n, c in zip(NAMES, cols)}
    pool_bytes = 2 * B * (N - 1) * Cd * 4                # both streams' patch tokens, read once
    out = {"model": a.model, "batch": B, "classes": K, "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
           "ms": {n: round(v, 4) for n, v in med.items()}, "spread": {n: round(v, 4) for n, v in spread.items()},
           "groups_ms": [[round(v, 4) for v in g] for g in groups],
           "pair_over_two_calls": round(med["pair_pool_norm"] / med["two_pool_norm_calls"], 4),
           "pair_gbytes_per_s": round(pool_bytes / med["pair_pool_norm"] / 1e6, 1),
           "variance_dfma": B * K * Cd, "variance_and_link_gdfma_per_s": round(B * K * Cd / med["variance_and_link"] / 1e6, 2),
           "dist_eval_over_forward": round(med["dist_eval_batch"] / med["encoder_forward"], 4),
           "pair_equals_single_calls": same, "mean_field": round(probe.mean_field, 6), "pi_over_8": round(math.pi / 8, 6),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
