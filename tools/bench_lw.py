"""Time the layer-weighted probe against the linear probe, and its four ops alone, on synthetic data (default: beit_base_patch16_224,
bs = 128, K = 1000) on one GPU.

    python tools/bench_lw.py [--model M] [--batch B] [--classes K] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.  Alternating, so that the ratios do not depend on which ran on a quieter machine:
  (a) a LinearProbe train step and the body of its evaluation batch (encoder forward, pool + norm, head, criterion);
  (b) the same two of a LayerWeightedProbe (mean over all tokens, no LayerNorm: the default flags);
  (c) alone, on the residual streams the forward left in the engine's workspace: uvit_op_lw_pool over all L blocks (mode 0, without and
      with the LayerNorm; mode 1), uvit_op_probe_pool_norm on the last block again and again (77.5 MB at ViT-B, bs = 128: it stays in
      the 256 MB last-level cache) and in rotation over the L blocks (the same bytes per call from memory that the call before did
      not touch, which is what uvit_op_lw_pool reads), uvit_op_lw_combine, uvit_op_probe_input_grad, uvit_op_lw_grad.
The pool rates are bytes of residual stream read per second: L B N C 4 for uvit_op_lw_pool, B (N - 1) C 4 for uvit_op_probe_pool_norm;
the scratch traffic (8 / N of that, written and read once) is not counted in either.  The batch ratios stand beside the model
1 + (L B N C 4 / measured pool rate + the extra contraction) / the linear batch's time.  Every figure is a
device-event bracket around `iters` back-to-back calls after `warmup` calls of the same shape, divided by `iters`; the median of
`repeats` groups is reported and the groups are kept.  Needs a GPU.
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lw.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.lw_probe import LW_LN_EPS, LayerWeightedProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    B, K, Ln, Cd = a.batch, a.classes, model.depth, model.embed_dim
    N = model.patch_embed.num_patches + 1
    plain, lw = LinearProbe(model, K), LayerWeightedProbe(model, K)
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, device="cuda")
    with torch.no_grad():
        for p in (plain, lw):
            p.head.weight.normal_(0.0, 0.05)
    L, s = lib(), cur_stream

    def evaluate(p):
        """The body of _evaluate's loop without calibration or detection."""
        n = p._features(x)
        p._logits_into(n)
        check(L.uvit_op_probe_ce(ptr(p._logits), ptr(y), f32(0.0), None, ptr(p._row_loss), ptr(slot), ptr(counters), n, K, s()), "uvit_op_probe_ce")

    def train(p):
        p.train_step(x, y, 1e-4, 0.05, 1.0)

    for p in (plain, lw):
        evaluate(p)
        train(p)
    e = model._engine
    layer_ptrs = [L.uvit_engine_ws_ptr(e.h, b"x", l + 1) for l in range(Ln)]
    layers = (C.c_void_p * Ln)(*layer_ptrs)
    turn = [0]

    def lw_pool(mode, ln):
        check(L.uvit_op_lw_pool(layers, Ln, ptr(lw._pooled), ptr(lw._lw_scratch), B, N, Cd, mode, ln, f32(LW_LN_EPS), s()), "uvit_op_lw_pool")

    def pool_norm(rotate):
        l = turn[0] % Ln if rotate else Ln - 1
        turn[0] += 1
        check(L.uvit_op_probe_pool_norm(C.c_void_p(layer_ptrs[l]), ptr(plain._feat), ptr(plain._scratch), B, N, Cd, f32(model.ln_eps), s()),
              "uvit_op_probe_pool_norm")

    ops = {
        "lw_pool_mean": lambda: lw_pool(0, 0),
        "lw_pool_mean_layernorm": lambda: lw_pool(0, 1),
        "lw_pool_cls": lambda: lw_pool(1, 0),
        "probe_pool_norm_same_block": lambda: pool_norm(False),
        "probe_pool_norm_rotating": lambda: pool_norm(True),
        "lw_combine": lambda: check(L.uvit_op_lw_combine(ptr(lw._pooled), lw._lw_ptr(lw._arena), ptr(lw._feat), ptr(lw._lw_w), B, Ln, Cd, s()),
                                    "uvit_op_lw_combine"),
        "probe_input_grad": lambda: check(L.uvit_op_probe_input_grad(ptr(lw._dlogits), ptr(lw._arena), ptr(lw._dfeat), B, K, Cd, s()),
                                          "uvit_op_probe_input_grad"),
        "lw_grad": lambda: check(L.uvit_op_lw_grad(ptr(lw._dfeat), ptr(lw._pooled), lw._lw_ptr(lw._arena), lw._lw_ptr(lw._grad_arena),
                                                   ptr(lw._lw_rows), B, Ln, Cd, s()), "uvit_op_lw_grad"),
    }
    batches = {"linear_train": lambda: train(plain), "lw_train": lambda: train(lw), "linear_eval": lambda: evaluate(plain),
               "lw_eval": lambda: evaluate(lw)}
    groups = []
    for _ in range(a.repeats):
        grp = {k: timed(fn, a.iters, a.warmup) for k, fn in batches.items()}
        grp.update({k: timed(fn, (12 if k == "probe_pool_norm_rotating" else 10) * a.iters, max(a.warmup, Ln)) for k, fn in ops.items()})
        groups.append(grp)
    med = lambda vals: sorted(vals)[len(vals) // 2]                                                                 # noqa: E731
    ms = {k: med([g[k] for g in groups]) for k in groups[0]}
    lw_bytes, one_bytes = Ln * B * N * Cd * 4, B * (N - 1) * Cd * 4
    rate = lambda nbytes, t_ms: nbytes / (t_ms * 1e-3) / 1e12                                                       # noqa: E731  TB/s
    rates = {"lw_pool_mean": rate(lw_bytes, ms["lw_pool_mean"]), "lw_pool_mean_layernorm": rate(lw_bytes, ms["lw_pool_mean_layernorm"]),
             "probe_pool_norm_same_block": rate(one_bytes, ms["probe_pool_norm_same_block"]),
             "probe_pool_norm_rotating": rate(one_bytes, ms["probe_pool_norm_rotating"])}
    ratio = lambda num, den: med([g[num] / g[den] for g in groups])                                                 # noqa: E731  each within its own group
    extra_ms = ms["lw_pool_mean"] + ms["lw_combine"] - ms["probe_pool_norm_rotating"]
    out = {"model": a.model, "batch": B, "classes": K, "depth": Ln, "tokens": N, "embed_dim": Cd, "iters": a.iters,
           "ms": {k: round(v, 5) for k, v in ms.items()},
           "pool_bytes": {"lw_pool": lw_bytes, "probe_pool_norm": one_bytes},
           "pool_rate_TBps": {k: round(v, 3) for k, v in rates.items()},
           "pool_rate_ratio_to_same_block": round(rates["lw_pool_mean"] / rates["probe_pool_norm_same_block"], 3),
           "pool_rate_ratio_to_rotating": round(rates["lw_pool_mean"] / rates["probe_pool_norm_rotating"], 3),
           "train_ratio_to_linear": round(ratio("lw_train", "linear_train"), 4),
           "eval_ratio_to_linear": round(ratio("lw_eval", "linear_eval"), 4),
           "train_model": round(1 + (extra_ms + ms["probe_input_grad"] + ms["lw_grad"]) / ms["linear_train"], 4),
           "eval_model": round(1 + extra_ms / ms["linear_eval"], 4),
           "groups_ms": [{k: round(v, 5) for k, v in g.items()} for g in groups],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
