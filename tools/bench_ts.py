"""Time temperature scaling on synthetic data (default: beit_base_patch16_224, K = 1000, B = 128) on one GPU.

    python tools/bench_ts.py [--model M] [--batch B] [--classes K] [--iters N] [--warmup W] [--sets N:K,...] [--out FILE]

Prints one JSON line, the protocol of tools/bench_detect.py: every figure is a device-event bracket around `iters` back-to-back calls
after `warmup` calls of the same shape, divided by `iters`.
(a) One evaluation batch (encoder eval forward + pool/norm + logits + cross-entropy, what LinearProbe.evaluate() launches per batch)
    without and with uvit_op_ts_scale behind the logits, alternating, in `repeats` pairs, and the ratio; the scale op on its own.
(b) uvit_op_ts_fit on the inputs of tests/ts_ref.make_inputs at every N:K of --sets: the whole fit with the default stopping rule
    (2 x 16 launches, those behind convergence return at once), the fit with max_iter = the passes it used (no launch behind the
    end), and max_iter = 1 (the first pass: four points in one read).  Their difference over passes - 1 is one later pass with its
    step; N K 4 bytes over that time is the rate at which a row pass streams the logits.
(c) The float64 numpy restatement (tests/ts_ref.fit_newton) of the same fit on this host's CPU, and the difference in T.
Needs a GPU; there is nothing to time without one.
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="with / without pairs of (a)")
    ap.add_argument("--sets", default="10000:100,50000:1000,131072:1000", help="N:K of (b)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ts.py measures on a GPU; none is visible")
    import ts_ref as tr
    from uncertainty_vit_amd.linear_probe import TS_MAX_ITER, TS_T_MAX, TS_T_MIN, TS_TOL, LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(model, a.classes)
    probe.head.weight.data.normal_(0.0, 0.05)
    B, K, L = a.batch, a.classes, lib()
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    z = probe.logits(x)
    y = torch.where(torch.rand(B, device="cuda") < 0.66, z.argmax(1), torch.randint(0, K, (B,), device="cuda")).contiguous()
    loss_slot = torch.zeros(1, device="cuda")
    table = torch.tensor([1.5, 1.0 / 1.5, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device="cuda")

    def scale(t):
        check(L.uvit_op_ts_scale(ptr(t), ptr(t), K, K, ptr(table), B, K, cur_stream()))

    def eval_batch(temperature):
        probe._features(x)
        probe._logits_into(B)
        if temperature:
            scale(probe._logits)
        check(L.uvit_op_probe_ce(ptr(probe._logits), ptr(y), f32(0.0), None, ptr(probe._row_loss), ptr(loss_slot), None, B, K, cur_stream()))

    op_ms = timed(lambda: scale(z), a.iters, a.warmup)
    pairs = []
    for _ in range(a.repeats):
        off = timed(lambda: eval_batch(False), a.iters, a.warmup)
        on = timed(lambda: eval_batch(True), a.iters, a.warmup)
        pairs.append((on, off))
    batch = {"B": B, "K": K, "on_off_pairs_ms": [[round(o, 4), round(f, 4)] for o, f in pairs],
             "on_over_off": [round(o / f, 4) for o, f in pairs], "ts_scale_ms": round(op_ms, 4)}

    sets = {}
    for spec in a.sets.split(","):
        N, Kc = (int(v) for v in spec.split(":"))
        zn, yn = tr.make_inputs(N, Kc, 1.0)
        zg, yg = torch.from_numpy(zn).cuda(), torch.from_numpy(yn).cuda()
        ws = torch.empty(int(L.uvit_op_ts_ws_bytes(N, Kc)), dtype=torch.uint8, device="cuda")
        tab = torch.zeros(8, dtype=torch.float64, device="cuda")

        def fit(max_iter):
            check(L.uvit_op_ts_fit(ptr(zg), Kc, ptr(yg), N, Kc, TS_T_MIN, TS_T_MAX, TS_TOL, max_iter, ptr(tab), ptr(ws), ws.numel(), cur_stream()))

        fit(TS_MAX_ITER)
        out = tab.cpu().tolist()
        passes = int(out[5])
        fit_ms = timed(lambda: fit(TS_MAX_ITER), a.iters, a.warmup)
        exact_ms = timed(lambda: fit(passes), a.iters, a.warmup)
        first_ms = timed(lambda: fit(1), a.iters, a.warmup)
        pass_ms = (exact_ms - first_ms) / (passes - 1) if passes > 1 else float("nan")
        t0 = time.perf_counter()
        ref = tr.fit_newton(zn, yn)
        cpu_ms = 1e3 * (time.perf_counter() - t0)
        sets[spec] = {"N": N, "K": Kc, "T": out[0], "status": int(out[6]), "passes": passes, "launches": 2 * TS_MAX_ITER + 1,
                      "launches_that_work": 2 * passes + 1, "fit_ms": round(fit_ms, 4), "fit_max_iter_eq_passes_ms": round(exact_ms, 4),
                      "first_pass_ms": round(first_ms, 4), "later_pass_ms": round(pass_ms, 4),
                      "later_pass_TB_per_s": round(N * Kc * 4 / (pass_ms * 1e-3) / 1e12, 3),
                      "first_pass_TB_per_s": round(N * Kc * 4 / (first_ms * 1e-3) / 1e12, 3),
                      "numpy_ms": round(cpu_ms, 1), "numpy_passes": ref["passes"], "T_minus_numpy": out[0] - ref["T"]}
    res = {"model": a.model, "iters": a.iters, "warmup": a.warmup, "eval_batch": batch, "sets": sets,
           "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
