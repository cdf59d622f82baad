"""Time the detection ops on synthetic data (default: beit_base_patch16_224, K = 1000, B = 128) on one GPU.

    python tools/bench_detect.py [--model M] [--batch B] [--classes K] [--iters N] [--warmup W] [--out FILE]

Prints one JSON line, the protocol of tools/bench_calib.py: every figure is a device-event bracket around `iters` back-to-back calls
after `warmup` calls of the same shape, divided by `iters`.
(a) One evaluation batch (encoder eval forward + pool/norm + logits + cross-entropy, what LinearProbe.evaluate() launches per batch)
    without and with uvit_op_detect_rows, alternating, in `repeats` pairs, and the ratio; the rows op on its own beside
    uvit_op_calib_softmax on the same logits.
(b) uvit_op_detect_metrics at N = 50,000 with S = 3 and S = 8 and at N = 76,032 (50,000 + the 26,032 images of SVHN's test split)
    with S = 3, with the number of launches of each call (counted from the sizes as the launcher does); N = 4,096 (one chunk: no
    global pass) and N = 2^20 (the limit) stand beside them, so that what the global passes add can be read off.
(c) The numpy restatement (tests/detect_ref.py) of the same tables on this host's CPU, `cpu_runs` runs each, the best of them.
Needs a GPU; there is nothing to time without one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHUNK = 4096


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


def launches(N):
    """Launches of one uvit_op_detect_metrics call: (sort, of which global passes, scan, metrics)."""
    P = 1
    while P < N:
        P <<= 1
    levels = max(0, (P // CHUNK).bit_length() - 1)
    glob = levels * (levels + 1) // 2
    return {"sort": 1 + glob + levels, "global_passes": glob, "scan": 3, "metrics": 2, "total": 1 + glob + levels + 5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="with / without pairs of (a)")
    ap.add_argument("--cpu_runs", type=int, default=3)
    ap.add_argument("--sets", default="50000:3,50000:8,76032:3,4096:3,1048576:3", help="N:S of (b)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect.py measures on a GPU; none is visible")
    import detect_ref as dr
    from uncertainty_vit_amd.linear_probe import LinearProbe
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
    store, flags = torch.zeros(3, 4 * B, device="cuda"), torch.zeros(4 * B, dtype=torch.uint8, device="cuda")
    probs = torch.zeros(B, K, device="cuda")

    def rows(src):
        check(L.uvit_op_detect_rows(ptr(src), ptr(y), ptr(store), 4 * B, B + 1, ptr(flags), B, K, cur_stream()))

    def eval_batch(detection):
        probe._features(x)
        probe._logits_into(B)
        check(L.uvit_op_probe_ce(ptr(probe._logits), ptr(y), f32(0.0), None, ptr(probe._row_loss), ptr(loss_slot), None, B, K, cur_stream()))
        if detection:
            rows(probe._logits)

    op_ms = {"detect_rows": timed(lambda: rows(z), a.iters, a.warmup),
             "calib_softmax": timed(lambda: check(L.uvit_op_calib_softmax(ptr(z), ptr(probs), B, K, cur_stream())), a.iters, a.warmup)}
    pairs = []
    for _ in range(a.repeats):
        off = timed(lambda: eval_batch(False), a.iters, a.warmup)
        on = timed(lambda: eval_batch(True), a.iters, a.warmup)
        pairs.append((on, off))
    batch = {"B": B, "K": K, "on_off_pairs_ms": [[round(o, 4), round(f, 4)] for o, f in pairs],
             "on_over_off": [round(o / f, 4) for o, f in pairs], "op_ms": {k: round(v, 4) for k, v in op_ms.items()}}

    sets = {}
    rng = np.random.default_rng(0)
    for spec in a.sets.split(","):
        N, S = (int(v) for v in spec.split(":"))
        s = rng.standard_normal((S, N)).astype(np.float32)
        f = (rng.random(N) < 0.25 + 0.2 * np.tanh(s[0])).astype(np.uint8)
        sg, fg = torch.from_numpy(s).cuda(), torch.from_numpy(f).cuda()
        table = probe.detection_batch(sg, fg).cpu().numpy()
        ms = timed(lambda: probe.detection_batch(sg, fg), a.iters, a.warmup)
        cpu = []
        for _ in range(a.cpu_runs if N <= 100000 else 1):
            t0 = time.perf_counter()
            ref, _ = dr.table(s, f)
            cpu.append(1e3 * (time.perf_counter() - t0))
        err = float(np.nanmax(np.abs(table[:, :4] - ref[:, :4])))
        sets[spec] = {"N": N, "S": S, "metrics_ms": round(ms, 4), "launches": launches(N), "numpy_ms_best": round(min(cpu), 2),
                      "numpy_runs": len(cpu), "max_abs_difference_to_numpy": err, "AUROC": [round(float(v), 6) for v in table[:, 0]]}
    out = {"model": a.model, "iters": a.iters, "warmup": a.warmup, "eval_batch": batch, "sets": sets,
           "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads()}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
