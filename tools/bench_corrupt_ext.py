"""Time uvit_op_corrupt_ext_batch for pixelate, jpeg_compression, motion_blur and zoom_blur at severities 1 and 5, beside a plain
evaluation batch timed in the same run, on synthetic data (default: beit_base_patch16_224, bs = 128, S = 224) on one GPU.

    python tools/bench_corrupt_ext.py [--model M] [--batch B] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line and writes it to --out (default: profiles/corrupt_ext_bench.json).  Per (kind, severity): the op's time, its ratio
to the batch (`op_over_batch`; DESIGN.md section 9.16 wants no corruption above a tenth of its batch's encoder forward, `within_tenth`)
and to the byte floor -- B 3 S S bytes read and four times as many written over the HBM peak (8.0 TB/s, the spec; 6.29 TB/s is what a
float4 copy reaches) -- and the workspace it needs.  `batch` is the encoder forward and the pooling of an evaluation batch
(LinearProbe._features).  Every figure is a device-event bracket around `iters` back-to-back calls after `warmup` calls of the same
shape, divided by `iters`; the median of `repeats` groups is reported.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_probe import timed  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "corrupt_ext_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_corrupt_ext.py measures on a GPU; none is visible")
    from uncertainty_vit_amd import corruptions as co, corruptions_ext as cx
    from uncertainty_vit_amd.datasets import IMAGENET_DEFAULT_MEAN as MEAN, IMAGENET_DEFAULT_STD as STD
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import lib
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(model, 1000)
    B, S = a.batch, model.img_size
    u8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device="cuda")
    owner = type("Owner", (), {})()
    med = lambda vals: sorted(vals)[len(vals) // 2]      # noqa: E731
    with torch.no_grad():
        cx.corrupt_ext(owner, u8, "zoom_blur", cx.ext_params("zoom_blur", 1, S).to("cuda"), 0, 0, MEAN, STD, out=out)
        probe._features(out)
    n_bytes = B * 3 * S * S * 5
    floor = n_bytes / HBM_PEAK * 1e3
    t_batch = med([timed(lambda: probe._features(out), a.iters, a.warmup) for _ in range(a.repeats)])
    kinds = {}
    for kind in cx.CORRUPTIONS_EXT:
        for sev in (1, 5):
            table = cx.ext_params(kind, sev, S).to("cuda")
            seed = co.set_seed(0, sev)
            op = lambda: cx.corrupt_ext(owner, u8, kind, table, seed, 0, MEAN, STD, out=out)      # noqa: E731
            t_op = med([timed(op, a.iters, a.warmup) for _ in range(a.repeats)])
            kinds[f"{kind}_{sev}"] = {"op_ms": round(t_op, 4), "op_over_batch": round(t_op / t_batch, 4), "within_tenth": t_op <= 0.1 * t_batch,
                                      "op_over_byte_floor": round(t_op / floor, 2),
                                      "workspace_mb": round(lib().uvit_op_corrupt_ext_ws_bytes(cx.ext_kind_id(kind), B, S, table.arg) / 1e6, 1)}
    res = {"model": a.model, "batch": B, "img_size": S, "iters": a.iters, "bytes_read_mb": round(B * 3 * S * S / 1e6, 1),
           "bytes_written_mb": round(B * 3 * S * S * 4 / 1e6, 1), "byte_floor_ms": round(floor, 4), "byte_floor_copy_rate_ms": round(n_bytes / HBM_COPY * 1e3, 4),
           "batch_ms": round(t_batch, 4), "kinds": kinds, "worst_op_over_batch": max(r["op_over_batch"] for r in kinds.values()),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
