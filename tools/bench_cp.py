"""Time the conformal-set kernels on synthetic data (default: beit_base_patch16_224, B = 128) on one GPU.

    python tools/bench_cp.py [--model M] [--batch B] [--classes K,K] [--cal N] [--iters N] [--warmup W] [--out FILE]

Prints one JSON line, the protocol of tools/bench_ts.py: every figure is a device-event bracket around `iters` back-to-back calls
after `warmup` calls of the same shape, divided by `iters`.
(a) The encoder eval forward + pool/norm of one batch of B images: what every conformal batch pays before its logits exist.
(b) Per K of --classes (default 100, 1000) and per score (lac, aps): uvit_op_cp_scores on B rows (what fit_conformal adds to a
    calibration batch) and on N = --cal rows (default 50 000) at once, uvit_op_cp_quantile over those N scores at two levels (its
    17 enqueues whole), uvit_op_cp_sets on a batch of B rows at two levels (what evaluate_conformal adds to a batch), and
    uvit_op_cp_finish.  `share_of_forward` is the batch figure over (a).
Needs a GPU; there is nothing to time without one.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--classes", default="100,1000")
    ap.add_argument("--cal", type=int, default=50000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cp.py measures on a GPU; none is visible")
    import cp_ref as cr
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(model, 10)
    B, N, L = a.batch, a.cal, lib()
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    forward_ms = timed(lambda: probe._features(x), a.iters, a.warmup)
    alphas = (C.c_double * 2)(0.1, 0.3)
    out = {}
    for K in (int(v) for v in a.classes.split(",")):
        zn, yn, un = cr.make_inputs(N, K, 1.0)
        zg, yg, ug = torch.from_numpy(zn).cuda(), torch.from_numpy(yn).cuda(), torch.from_numpy(un).cuda()
        scores = torch.zeros(N, dtype=torch.float64, device="cuda")
        ws = torch.empty(int(L.uvit_op_cp_ws_bytes(N, 2)), dtype=torch.uint8, device="cuda")
        table = torch.zeros(2, 16, dtype=torch.float64, device="cuda")
        counters = torch.zeros(int(L.uvit_op_cp_counter_count(K, 2)), dtype=torch.int64, device="cuda")
        for score in ("lac", "aps"):
            kind = cr.KINDS[score]

            def run_scores(rows):
                check(L.uvit_op_cp_scores(ptr(zg), K, ptr(yg), ptr(ug), rows, K, kind, 0.0, 0, ptr(scores), cur_stream()))

            def run_quantile():
                check(L.uvit_op_cp_quantile(ptr(scores), N, alphas, 2, ptr(table), ptr(ws), ws.numel(), cur_stream()))

            def run_sets():
                check(L.uvit_op_cp_sets(ptr(zg), K, ptr(yg), ptr(ug), B, K, kind, 0.0, 0, ptr(table), 2, ptr(counters), None, None, B, cur_stream()))

            def run_finish():
                check(L.uvit_op_cp_finish(ptr(counters), ptr(table), K, 2, cur_stream()))

            batch_scores = timed(lambda: run_scores(B), a.iters, a.warmup)
            all_scores = timed(lambda: run_scores(N), a.iters, a.warmup)
            quant = timed(run_quantile, a.iters, a.warmup)
            qhat = table[:, 1].cpu().tolist()
            sets_ms = timed(run_sets, a.iters, a.warmup)
            fin = timed(run_finish, a.iters, a.warmup)
            out[f"{score}:{K}"] = {
                "K": K, "score": score, "qhat": qhat, "cp_scores_batch_ms": round(batch_scores, 4), "cp_scores_N_ms": round(all_scores, 4),
                "cp_scores_N_TB_per_s": round(N * K * 4 / (all_scores * 1e-3) / 1e12, 3), "cp_quantile_N_ms": round(quant, 4),
                "cp_sets_batch_ms": round(sets_ms, 4), "cp_finish_ms": round(fin, 4),
                "share_of_forward": {"cp_scores_batch": round(batch_scores / forward_ms, 5), "cp_sets_batch": round(sets_ms / forward_ms, 5)}}
    res = {"model": a.model, "B": B, "N": N, "iters": a.iters, "warmup": a.warmup, "encoder_forward_ms": round(forward_ms, 4), "cases": out,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
