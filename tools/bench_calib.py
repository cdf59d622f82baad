"""Time the calibration metrics on synthetic data (default: beit_base_patch16_224, K = 1000, B = 128 and 192) on one GPU.

    python tools/bench_calib.py [--model M] [--batches 128,192] [--classes K] [--iters N] [--warmup W] [--out FILE]

Prints one JSON line.  Per batch size: one evaluation batch (encoder eval forward + pool/norm + logits + cross-entropy, what
LinearProbe.evaluate() launches per batch) without and with the calibration ops, alternating on the same build, and their ratio; the
time of each op on its own (softmax, confidence, tace, auroc) and of calibration_batch as a whole.  Every figure is a device-event
bracket around `iters` back-to-back calls after `warmup` calls of the same shape, divided by `iters`: for the small ops that is
launch spacing as much as kernel time.  The labels follow the row maximum two times in three, so that the bins are populated as a
trained head populates them.  The reference's host path (numpy loops over classes x bins) is not timed here: the reference is not on
the GPU host.  Needs a GPU; there is nothing to time without one.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
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
    ap.add_argument("--batches", default="128,192")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the with / without pair to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_calib.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import ECE_BINS, TACE_BINS, TACE_THRESHOLD, LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(model, a.classes)
    probe.head.weight.data.normal_(0.0, 0.05)         # logits of spread ~1.4 on unit features: a head that has an opinion
    K, L = a.classes, lib()
    bounds = np.linspace(0, 1, ECE_BINS + 1)
    results = {}
    for B in (int(v) for v in a.batches.split(",")):
        x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
        z = probe.logits(x)
        y = torch.where(torch.rand(B, device="cuda") < 0.66, z.argmax(1), torch.randint(0, K, (B,), device="cuda")).contiguous()
        ece, tace, nll, auroc = (float(v) for v in probe.calibration_batch(z, y))
        assert all(np.isfinite((ece, tace, nll, auroc))), (ece, tace, nll, auroc)
        slot = torch.zeros(8, dtype=torch.float64, device="cuda")
        loss_slot = torch.zeros(1, device="cuda")

        def eval_batch(calibration):
            # what evaluate() launches for one batch
            probe._features(x)
            probe._logits_into(B)
            check(L.uvit_op_probe_ce(ptr(probe._logits), ptr(y), f32(0.0), None, ptr(probe._row_loss), ptr(loss_slot), None, B, K,
                                     cur_stream()))
            if calibration:
                probe._calibration_into(probe._logits, y, B, slot.data_ptr())

        p, s = probe._probs, cur_stream
        parts = {
            "softmax": lambda: check(L.uvit_op_calib_softmax(ptr(z), ptr(p), B, K, s())),
            "confidence": lambda: check(L.uvit_op_calib_confidence(ptr(p), ptr(y), bounds.ctypes.data_as(C.c_void_p), ECE_BINS, 1,
                                                                    ptr(probe._row_conf), ptr(probe._row_pred), ptr(probe._row_nll),
                                                                    ptr(probe._bin_table), ptr(slot), B, K, s())),
            "tace": lambda: check(L.uvit_op_calib_tace(ptr(p), ptr(y), C.c_double(TACE_THRESHOLD), TACE_BINS, 1, ptr(probe._per_class),
                                                       C.c_void_p(slot.data_ptr() + 16), B, K, s())),
            "auroc": lambda: check(L.uvit_op_calib_auroc(ptr(p), ptr(y), ptr(probe._auroc_rows), C.c_void_p(slot.data_ptr() + 24), B, K,
                                                         s())),
            "calibration_batch": lambda: probe._calibration_into(z, y, B, slot.data_ptr()),
        }
        ms = {k: timed(fn, a.iters, a.warmup) for k, fn in parts.items()}
        pairs = []
        for _ in range(a.repeats):          # alternating, so that the ratio does not depend on which ran on a quieter machine
            off = timed(lambda: eval_batch(False), a.iters, a.warmup)
            on = timed(lambda: eval_batch(True), a.iters, a.warmup)
            pairs.append((on, off))
        on_ms = sorted(p_[0] for p_ in pairs)[len(pairs) // 2]
        off_ms = sorted(p_[1] for p_ in pairs)[len(pairs) // 2]
        results[str(B)] = {"eval_batch_ms": round(off_ms, 4), "eval_batch_calibration_ms": round(on_ms, 4),
                           "calibration_on_over_off": round(on_ms / off_ms, 4),
                           "on_off_pairs_ms": [[round(o, 4), round(f, 4)] for o, f in pairs],
                           "op_ms": {k: round(v, 4) for k, v in ms.items()},
                           "metrics": {"ECE": ece, "TACE": tace, "NLL": nll, "AUROC": auroc}}
    out = {"model": a.model, "classes": K, "iters": a.iters, "warmup": a.warmup, "ece_bins": ECE_BINS, "tace_bins": TACE_BINS,
           "batch": results, "reference_host_path": "not timed: the reference is not on the GPU host",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
