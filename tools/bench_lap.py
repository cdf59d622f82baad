"""Time the Laplace probe beside the linear head on synthetic data (default: beit_base_patch16_224, bs = 128, K = 1000) on one GPU.

    python tools/bench_lap.py [--model M] [--batch B] [--classes K] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.  Alternating, so that the ratios do not depend on which ran on a quieter machine: the encoder's eval forward
alone, a linear evaluation batch (forward + pool/norm + logits), a Laplace evaluation batch (the same + variance + probit), one
uvit_op_lap_factors call and uvit_op_lap_prepare; then each op on its own, with uvit_op_gp_variance at D = the embed dim beside the
variance op for the rate per double FMA.  Every figure is a device-event bracket around `iters` back-to-back calls after `warmup`
calls of the same shape, divided by `iters`: for the small ops that is launch spacing as much as kernel time.  The fit (one batch,
its eigen-decompositions on the host) happens once before the timed region.  Needs a GPU.
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lap.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.lap_probe import PROBIT_FACTOR, LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    lap, lin = LaplaceProbe(model, a.classes), LinearProbe(model, a.classes)
    B, K, Cd = a.batch, a.classes, model.embed_dim
    D = Cd + 1
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    with torch.no_grad():
        for p in (lap, lin):
            p.head.weight.normal_(0.0, 0.05)               # logits of a few units: the softmax of the factors is not uniform
    fit = lap.fit_laplace([(x, y)], prior_precision=1.0)
    st, L, s = lap._lap, lib(), cur_stream
    acc = torch.zeros(D * D + K * K + 4, dtype=torch.float64, device="cuda")
    at = lambda off: C.c_void_p(acc.data_ptr() + 8 * off)      # noqa: E731
    sigma = torch.eye(Cd, dtype=torch.float64, device="cuda")
    gp_var = torch.zeros(B, dtype=torch.float64, device="cuda")
    parts = {
        "factors": lambda: check(L.uvit_op_lap_factors(ptr(lap._feat), ptr(lap._logits), K, ptr(y), at(0), at(D * D), at(D * D + K * K),
                                                       ptr(lap._lap_ws), lap._lap_ws.numel(), B, Cd, K, s())),
        "prepare": lambda: check(L.uvit_op_lap_prepare(ptr(st["UG"]), ptr(st["lam_a_dev"]), ptr(st["lam_g_dev"]), C.c_double(1.0), ptr(st["T"]),
                                                       Cd, K, s())),
        "variance": lambda: check(L.uvit_op_lap_variance(ptr(lap._feat), ptr(st["UA"]), ptr(st["T"]), ptr(lap._lap_var), ptr(lap._lap_ws),
                                                         lap._lap_ws.numel(), B, Cd, K, s())),
        "probit": lambda: check(L.uvit_op_lap_probit(ptr(lap._logits), K, ptr(lap._lap_var), C.c_double(PROBIT_FACTOR), ptr(lap._dlogits), K,
                                                     ptr(lap._lap_col), B, K, s())),
        "gp_variance": lambda: check(L.uvit_op_gp_variance(ptr(lap._feat), ptr(sigma), C.c_double(1e-3), ptr(gp_var), B, Cd, s())),
    }

    def eval_batch(p):
        p._logits_into(p._features(x))

    groups = []
    for _ in range(a.repeats):
        groups.append((timed(lambda: model.forward_features(x, None, None), a.iters, a.warmup),
                       timed(lambda: eval_batch(lin), a.iters, a.warmup), timed(lambda: eval_batch(lap), a.iters, a.warmup),
                       timed(parts["factors"], a.iters, a.warmup), timed(parts["prepare"], a.iters, a.warmup)))
    fwd, ev_lin, ev_lap, factors, prepare = (sorted(grp[i] for grp in groups)[len(groups) // 2] for i in range(5))
    ms = {k: timed(fn, a.iters, a.warmup) for k, fn in parts.items()}
    lap_fma, gp_fma = B * D * D + B * D * K, B * Cd * Cd + B * Cd
    out = {"model": a.model, "batch": B, "classes": K, "iters": a.iters, "fit_n": fit["n"], "encoder_forward_ms": round(fwd, 4),
           "linear_eval_batch_ms": round(ev_lin, 4), "laplace_eval_batch_ms": round(ev_lap, 4),
           "laplace_eval_over_linear_eval": round(ev_lap / ev_lin, 4), "factors_ms": round(factors, 4), "prepare_ms": round(prepare, 4),
           "groups_ms": [[round(v, 4) for v in grp] for grp in groups], "part_ms": {k: round(v, 4) for k, v in ms.items()},
           "variance_dfma": lap_fma, "variance_gdfma_per_s": round(lap_fma / ms["variance"] / 1e6, 2), "gp_variance_dfma": gp_fma,
           "gp_variance_gdfma_per_s": round(gp_fma / ms["gp_variance"] / 1e6, 2), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
