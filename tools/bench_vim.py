"""Time uvit_op_vim_scores beside uvit_op_maha_scores at the same B, C and K, and a detection batch with and without a ViM state, on
synthetic data (default: beit_base_patch16_224, bs = 128, C = 768, D = 512, K = 1000) on one GPU.

    python tools/bench_vim.py [--model M] [--batch B] [--dim D] [--classes K] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.  Alternating, in one process, so that the ratios do not depend on which ran on a quieter machine:
  (a) uvit_op_vim_scores (two launches: the (B, C - D + K) product and the rows), and with `sums` (three);
  (b) uvit_op_maha_scores (three launches: two triangular (B, C) whitenings, the (B, K) distances, the rows);
  (c) the body of an evaluate(detection=True) batch with the ViM state (the op and two column copies more) and without.
Every figure is a device-event bracket around `iters` back-to-back calls after `warmup` calls of the same shape, divided by `iters`;
the median of `repeats` groups is reported and the groups are kept.  Needs a GPU.
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
    ap.add_argument("--dim", type=int, default=0, help="principal dimension D (0: the default of fit_vim for the model's C)")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vim.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import LinearProbe, vim_default_dim
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    plain, vim = LinearProbe(model, a.classes), LinearProbe(model, a.classes)
    B, K, Cd = a.batch, a.classes, model.embed_dim
    D = a.dim or vim_default_dim(Cd)
    Cn, F64 = Cd - D, torch.float64
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    with torch.no_grad():
        for p in (plain, vim):
            p.head.weight.normal_(0.0, 0.05)
            p._features(x)
    L, s = lib(), cur_stream
    feat = vim._feat[:B].clone()

    # a ViM state of the timed geometry: an orthonormal R, the probe's head, alpha 1 (the values do not steer the kernels)
    Q = torch.linalg.qr(torch.randn(Cd, Cd, dtype=F64))[0]
    W, b = vim.head.weight.detach().double().cpu(), torch.randn(K, dtype=F64)
    vim.load_vim_state({"R": Q[:, :Cn].T.contiguous(), "origin": -(torch.linalg.pinv(W) @ b), "weight": W, "bias": b, "alpha": 1.0, "dim": D,
                        "eigenvalues": torch.linspace(0.0, 1.0, Cd, dtype=F64), "sums": torch.tensor([float(B), float(B), float(B), 0.0])})
    st = vim._vim
    col, rcol, mcol, mrcol = (torch.zeros(B, dtype=torch.float32, device="cuda") for _ in range(4))
    pred = torch.zeros(B, dtype=torch.int32, device="cuda")
    sums = torch.zeros(4, dtype=F64, device="cuda")
    ws = torch.empty(int(L.uvit_op_vim_scores_ws_bytes(B, Cd, Cn, K)), dtype=torch.uint8, device="cuda")

    def vim_op(with_sums):
        check(L.uvit_op_vim_scores(ptr(feat), ptr(st["A"]), ptr(st["a"]), C.c_double(1.0), ptr(col), ptr(rcol), ptr(pred), None, None,
                                   ptr(sums) if with_sums else None, ptr(ws), ws.numel(), B, Cd, Cn, K, s()))

    # uvit_op_maha_scores on factors of the same geometry: lower-triangular W, W0, K whitened means, every class with a row
    Wl, W0l = (torch.randn(Cd, Cd, dtype=F64, device="cuda").tril() / Cd ** 0.5 for _ in range(2))
    Wmu, Wmu0, count = torch.randn(K, Cd, dtype=F64, device="cuda"), torch.randn(Cd, dtype=F64, device="cuda"), torch.ones(K, dtype=F64, device="cuda")
    mws = torch.empty(int(L.uvit_op_maha_scores_ws_bytes(B, Cd, K)), dtype=torch.uint8, device="cuda")
    maha_op = lambda: check(L.uvit_op_maha_scores(ptr(feat), ptr(Wl), ptr(W0l), ptr(Wmu), ptr(Wmu0), ptr(count), ptr(mcol), ptr(mrcol),      # noqa: E731
                                                  ptr(pred), None, K, None, None, ptr(mws), mws.numel(), B, Cd, K, s()))

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

    for p in (plain, vim):
        p._det = {"scores": None, "flags": None, "cap": 0, "n": 0}
    vim._score_eval = [(vim._vim_score, {"correct": torch.zeros(1, dtype=torch.int32, device="cuda"), "slabs": []})]
    groups = [(timed(lambda: vim_op(False), a.iters, a.warmup), timed(lambda: vim_op(True), a.iters, a.warmup), timed(maha_op, a.iters, a.warmup),
               timed(lambda: det_batch(plain), a.iters, a.warmup), timed(lambda: det_batch(vim), a.iters, a.warmup)) for _ in range(a.repeats)]
    plain._det, vim._det, vim._score_eval = None, None, ()
    t_vim, t_sums, t_maha, t_plain, t_with = (sorted(grp[i] for grp in groups)[len(groups) // 2] for i in range(5))
    flops_vim, flops_maha = 2.0 * B * Cd * (Cn + K), 2.0 * B * Cd * Cd + 3.0 * B * Cd * K      # maha: two triangular halves, then sub + fma
    out = {"model": a.model, "batch": B, "embed_dim": Cd, "dim": D, "null_dim": Cn, "classes": K, "iters": a.iters,
           "vim_scores_ms": round(t_vim, 4), "vim_scores_with_sums_ms": round(t_sums, 4), "maha_scores_ms": round(t_maha, 4),
           "vim_over_maha": round(t_vim / t_maha, 4), "vim_fp64_gflop": round(flops_vim / 1e9, 3), "maha_fp64_gflop": round(flops_maha / 1e9, 3),
           "vim_fp64_tflop_per_s": round(flops_vim / t_vim / 1e9, 2), "maha_fp64_tflop_per_s": round(flops_maha / t_maha / 1e9, 2),
           "detection_batch_ms": round(t_plain, 4), "detection_batch_with_vim_ms": round(t_with, 4), "with_vim_over_without": round(t_with / t_plain, 4),
           "groups_ms": [[round(v, 4) for v in grp] for grp in groups], "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
