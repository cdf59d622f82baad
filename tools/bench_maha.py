"""Time the Mahalanobis ops and a detection batch with and without a density on synthetic data (default: beit_base_patch16_224,
bs = 128, K = 1000) on one GPU.

    python tools/bench_maha.py [--model M] [--batch B] [--classes K] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.  Alternating, so that the ratio does not depend on which ran on a quieter machine: the encoder's eval forward
alone, the body of an evaluate(detection=True) batch without a density (forward, pool + norm, logits, the rows op: what the commit
before this feature runs for the same call, launch for launch) and the same body with a density (the scores op and two column
copies more); then uvit_op_maha_accumulate and uvit_op_maha_scores on their own.  Every figure is a device-event bracket around
`iters` back-to-back calls after `warmup` calls of the same shape, divided by `iters`: for the small ops that is launch spacing as
much as kernel time.  Beside each op stands its floor max(double FLOPs / 78.6 TFLOP/s, bytes / 8 TB/s) (DESIGN.md section 4 has the
bf16 counterpart).  The fit (one batch of cluster features, its Cholesky factors on the host) happens once before the timed region.
Needs a GPU.
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

PEAK_F64, PEAK_HBM = 78.6e12, 8e12           # the part's double rate (vector = matrix) and HBM bandwidth, per second


def floor_ms(flops, nbytes):
    return 1e3 * max(flops / PEAK_F64, nbytes / PEAK_HBM)


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
        raise SystemExit("bench_maha.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    plain, dens = LinearProbe(model, a.classes), LinearProbe(model, a.classes)
    B, K, Cd = a.batch, a.classes, model.embed_dim
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    with torch.no_grad():
        for p in (plain, dens):
            p.head.weight.normal_(0.0, 0.05)
    # a density of 4 K cluster rows in feature space (the timing does not depend on the values; the factorisation must succeed)
    g = torch.Generator().manual_seed(1)
    rows = 2.0 * torch.randn(K, Cd, generator=g, dtype=torch.float64)[torch.arange(4 * K) % K] + 0.5 * torch.randn(4 * K, Cd, generator=g,
                                                                                                                   dtype=torch.float64)
    rows = rows - rows.mean(1, keepdim=True)
    rows = (rows / rows.pow(2).mean(1, keepdim=True).sqrt()).float().double()
    lab = torch.arange(4 * K) % K
    onehot = torch.zeros(4 * K, K, dtype=torch.float64)
    onehot[torch.arange(4 * K), lab] = 1.0
    fit = dens.load_density_state({"S": rows.T @ rows, "class_sum": onehot.T @ rows, "total_sum": rows.sum(0), "class_count": onehot.sum(0),
                                   "sums": torch.tensor([4.0 * K, 0.0]), "shrinkage": 1e-3})
    L, s, st, sc = lib(), cur_stream, dens._maha, dens._density
    n_acc = Cd * Cd + K * Cd + Cd + K + 2
    acc = torch.zeros(n_acc, dtype=torch.float64, device="cuda")
    at = lambda off: C.c_void_p(acc.data_ptr() + 8 * off)      # noqa: E731
    aws = torch.empty(int(L.uvit_op_maha_accumulate_ws_bytes(B, Cd, K)), dtype=torch.uint8, device="cuda")
    for p in (plain, dens):
        p._features(x)
    sc.buffers_for(B)
    parts = {
        "accumulate": lambda: check(L.uvit_op_maha_accumulate(ptr(dens._feat), ptr(y), at(0), at(Cd * Cd), at(Cd * Cd + K * Cd),
                                                              at(Cd * Cd + K * Cd + Cd), at(n_acc - 2), ptr(aws), aws.numel(), B, Cd, K, s())),
        "scores": lambda: check(L.uvit_op_maha_scores(ptr(dens._feat), ptr(st["W"]), ptr(st["W0"]), ptr(st["Wmu"]), ptr(st["Wmu0"]),
                                                      ptr(st["count_dev"]), ptr(sc.col), ptr(sc.rcol), ptr(sc.pred), None, K,
                                                      None, None, ptr(sc.ws), sc.ws.numel(), B, Cd, K, s())),
    }

    def det_batch(p):
        """The body of _evaluate's loop with detection=True, without the cross-entropy: one batch into an empty store."""
        n = p._features(x)
        p._det["n"] = 0
        p._det_reserve(n)
        for score, ev in p._score_eval:
            score.eval_batch(n, y, ev)
            ev["slabs"].clear()
        p._logits_into(n)
        p._det_rows(n, y)

    for p in (plain, dens):
        p._det = {"scores": None, "flags": None, "cap": 0, "n": 0}
    dens._score_eval = [(sc, {"correct": torch.zeros(1, dtype=torch.int32, device="cuda"), "slabs": []})]
    groups = []
    for _ in range(a.repeats):
        groups.append((timed(lambda: model.forward_features(x, None, None), a.iters, a.warmup),
                       timed(lambda: det_batch(plain), a.iters, a.warmup), timed(lambda: det_batch(dens), a.iters, a.warmup)))
    fwd, ev_plain, ev_dens = (sorted(grp[i] for grp in groups)[len(groups) // 2] for i in range(3))
    plain._det, dens._det, dens._score_eval = None, None, ()
    ms = {k: timed(fn, a.iters, a.warmup) for k, fn in parts.items()}
    # accumulate: B C^2 FMAs into S, B C adds twice; S read and written, the touched class rows, the features
    acc_flops, acc_bytes = 2 * B * Cd * Cd + 2 * B * Cd, 16 * Cd * Cd + 16 * min(B, K) * Cd + 4 * B * Cd
    # scores: two triangular whitenings (B C^2 / 2 FMAs each), B K C differences and FMAs; W, W0, Wmu and the features read once,
    # the whitened rows and the distances written and read
    sc_flops = 2 * B * Cd * Cd + 3 * B * K * Cd
    sc_bytes = 8 * Cd * Cd + 8 * K * Cd + 4 * B * Cd + 2 * (16 * B * Cd) + 16 * B * K
    out = {"model": a.model, "batch": B, "classes": K, "iters": a.iters, "fit_n": fit["n"], "encoder_forward_ms": round(fwd, 4),
           "detection_batch_ms": round(ev_plain, 4), "detection_batch_with_density_ms": round(ev_dens, 4),
           "with_density_over_without": round(ev_dens / ev_plain, 4), "groups_ms": [[round(v, 4) for v in grp] for grp in groups],
           "accumulate_ms": round(ms["accumulate"], 4), "accumulate_floor_ms": round(floor_ms(acc_flops, acc_bytes), 5),
           "scores_ms": round(ms["scores"], 4), "scores_floor_ms": round(floor_ms(sc_flops, sc_bytes), 5), "scores_dflop": sc_flops,
           "scores_gdflop_per_s": round(sc_flops / ms["scores"] / 1e6, 1), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
