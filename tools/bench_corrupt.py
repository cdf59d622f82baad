"""Time uvit_op_corrupt_batch for every kind at severities 1 and 5, uvit_op_corrupt_pack, and an evaluation batch with and without a
corruption in front of the encoder forward, on synthetic data (default: beit_base_patch16_224, bs = 128, S = 224) on one GPU.

    python tools/bench_corrupt.py [--model M] [--batch B] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line and writes it to --out (default: profiles/corrupt_bench.json).  Per (kind, severity): the op's time, its byte floor
-- B 3 S S bytes read and four times as many written, over the HBM peak (8.0 TB/s, the spec; 6.29 TB/s is what a float4 copy reaches) --
and, for defocus_blur, its FLOP floor: two unfused fp32 operations per non-zero tap and output over half the 157.3 TFLOP/s vector peak,
which counts an fma as two.  `batch` is the encoder forward and the pooling of an evaluation batch (LinearProbe._features); `ratio` is
(op + batch) / batch measured as one sequence.  Every figure is a device-event bracket around `iters` back-to-back calls after `warmup`
calls of the same shape, divided by `iters`; the median of `repeats` groups is reported.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_probe import timed  # noqa: E402

HBM_PEAK, HBM_COPY, FP32_UNFUSED = 8.0e12, 6.29e12, 157.3e12 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "corrupt_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_corrupt.py measures on a GPU; none is visible")
    from uncertainty_vit_amd import corruptions as co
    from uncertainty_vit_amd.datasets import IMAGENET_DEFAULT_MEAN as MEAN, IMAGENET_DEFAULT_STD as STD
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(model, 1000)
    B, S = a.batch, model.img_size
    u8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device="cuda")
    packed = torch.empty_like(u8)
    owner = type("Owner", (), {})()
    med = lambda vals: sorted(vals)[len(vals) // 2]      # noqa: E731
    with torch.no_grad():
        co.corrupt(owner, u8, "contrast", torch.from_numpy(co.corruption_params("contrast", 1, S)).cuda(), 0, 0, MEAN, STD, out=out)
        probe._features(out)
    n_bytes = B * 3 * S * S * 5
    t_batch = med([timed(lambda: probe._features(out), a.iters, a.warmup) for _ in range(a.repeats)])
    t_pack = med([timed(lambda: co.pack(out, MEAN, STD, out=packed), a.iters, a.warmup) for _ in range(a.repeats)])
    kinds = {}
    for kind in co.CORRUPTIONS:
        for sev in (1, 5):
            table = co.corruption_params(kind, sev, S)
            params = torch.from_numpy(table).cuda()
            seed = co.set_seed(0, sev)
            op = lambda: co.corrupt(owner, u8, kind, params, seed, 0, MEAN, STD, out=out)      # noqa: E731

            def both():
                op()
                probe._features(out)
            t_op = med([timed(op, a.iters, a.warmup) for _ in range(a.repeats)])
            t_both = med([timed(both, a.iters, a.warmup) for _ in range(a.repeats)])
            row = {"op_ms": round(t_op, 4), "byte_floor_ms": round(n_bytes / HBM_PEAK * 1e3, 4), "byte_floor_copy_rate_ms": round(n_bytes / HBM_COPY * 1e3, 4),
                   "with_batch_ms": round(t_both, 4), "ratio": round(t_both / t_batch, 4)}
            if kind == "defocus_blur":
                taps = int(np.count_nonzero(table))
                row["nonzero_taps"] = taps
                row["flop_floor_ms"] = round(2.0 * taps * B * 3 * S * S / FP32_UNFUSED * 1e3, 4)
            kinds[f"{kind}_{sev}"] = row
    res = {"model": a.model, "batch": B, "img_size": S, "iters": a.iters, "bytes_read_mb": round(B * 3 * S * S / 1e6, 1),
           "bytes_written_mb": round(B * 3 * S * S * 4 / 1e6, 1), "batch_ms": round(t_batch, 4), "pack_ms": round(t_pack, 4), "kinds": kinds,
           "worst_ratio": max(r["ratio"] for r in kinds.values()), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
