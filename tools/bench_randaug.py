"""Time the probe's RandAugment on synthetic data (default: beit_base_patch16_224, bs = 128, S = 224, K = 1000) on one GPU.

    python tools/bench_randaug.py [--model M] [--batch B] [--classes K] [--iters N] [--op_iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line and writes it to --out (default: profiles/randaug_bench.json):
  copy       a float4 copy of the batch (torch's copy_ of the fp32 images) in this run, and the rate it reaches
  ops        uvit_op_randaug_batch with the same single layer on every image, per mechanism: `none` (the pack and its inverse alone),
             the table ops `invert` (from its integers) and `equalize` (with the statistics pass), the blend ops `color`, `contrast`
             (statistics pass) and `sharpness` (the 3 x 3 filter), the affine op `rotate` at 20 degrees under each filter.  Beside the
             time: the bytes of the model of DESIGN.md section 9.21 (with N = 3 B S S values: 5 N for the pack, 5 N for the inverse,
             2 N per applied layer, N more for a statistics pass), that count at the HBM peak (8.0 TB/s, the spec), at section 9.20's
             float4 copy rate (6.29 TB/s) and at this run's copy rate, and the op's ratio to each
  default    the op under the draws of rand-m9-mstd0.5-inc1 (mean over the first eight iterations' draws), and the host time of a draw
  step       LinearProbe.train_step with that augmenter against one without, alternating
Every device figure is a device-event bracket around back-to-back calls after `warmup` calls of the same shape, divided by their
number; the median of `repeats` groups is reported.  Needs a GPU.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_probe import timed  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--op_iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "randaug_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_randaug.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.datasets import IMAGENET_DEFAULT_MEAN as MEAN, IMAGENET_DEFAULT_STD as STD
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, lib, ptr
    from uncertainty_vit_amd.probe_randaug import RANDAUG_DESC, RANDAUG_FILTERS, RANDAUG_OPS, RandAugmenter, rotate_matrix
    torch.manual_seed(0)
    L = lib()
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    B, S, K = a.batch, model.img_size, a.classes
    x = torch.randn(B, 3, S, S, device="cuda")
    out = torch.empty_like(x)
    med = lambda vals: sorted(vals)[len(vals) // 2]      # noqa: E731
    N = B * 3 * S * S
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    need = L.uvit_op_randaug_ws_bytes(B, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    pinned = []

    def op_of(desc):
        host = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8).reshape(-1).copy()).pin_memory()
        pinned.append(host)
        hp = host.data_ptr()
        return lambda: check(L.uvit_op_randaug_batch(ptr(x), ptr(out), C.c_void_p(hp), B, S, mean, std, ptr(ws), need, cur_stream()),
                             "uvit_op_randaug_batch")

    def model_bytes(desc):
        """DESIGN.md section 9.21's byte model for these descriptors."""
        n, per = 10 * N, 3 * S * S
        stats = {RANDAUG_OPS.index(k) for k in ("AutoContrast", "Equalize", "Contrast")}
        for d in desc:
            for e in d["layers"][:int(d["n_layers"])]:
                n += (2 * per if int(e["op"]) else 0) + (per if int(e["op"]) in stats else 0)
        return n

    copy = lambda: out.copy_(x)      # noqa: E731
    t_copy = med([timed(copy, a.op_iters, a.warmup) for _ in range(a.repeats)])
    copy_rate = 8 * N / (t_copy * 1e-3)

    def report(t, n_bytes):
        floors = {"byte_floor_ms": n_bytes / HBM_PEAK * 1e3, "byte_floor_copy_rate_ms": n_bytes / HBM_COPY * 1e3, "byte_floor_this_run_ms": n_bytes / copy_rate * 1e3}
        r = {"op_ms": round(t, 4), "bytes_mb": round(n_bytes / 1e6, 1), **{k: round(v, 4) for k, v in floors.items()}}
        r.update(ratio_to_floor=round(t / floors["byte_floor_ms"], 3), ratio_to_copy_rate_floor=round(t / floors["byte_floor_copy_rate_ms"], 3),
                 ratio_to_this_run_floor=round(t / floors["byte_floor_this_run_ms"], 3), tb_per_s=round(n_bytes / (t * 1e-3) / 1e12, 3))
        return r

    def single(name, **kw):
        desc = np.zeros(B, dtype=RANDAUG_DESC)
        if name != "None":
            desc["n_layers"] = 1
            desc["layers"]["op"][:, 0] = RANDAUG_OPS.index(name)
            desc["layers"]["matrix"][:, 0] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
            for k, v in kw.items():
                desc["layers"][k][:, 0] = v
        return desc

    fill = 124 | 116 << 8 | 104 << 16
    cases = {"none": single("None"), "invert": single("Invert"), "equalize": single("Equalize"), "color": single("Color", factor=1.5),
             "contrast": single("Contrast", factor=1.5), "sharpness": single("Sharpness", factor=1.5)}
    for flt in ("nearest", "bilinear", "bicubic"):
        cases[f"rotate_{flt}"] = single("Rotate", filter=RANDAUG_FILTERS[flt], fill=fill, matrix=rotate_matrix(20.0, S))
    ops = {}
    for name, desc in cases.items():
        op = op_of(desc)
        op()
        ops[name] = report(med([timed(op, a.op_iters, a.warmup) for _ in range(a.repeats)]), model_bytes(desc))

    aug = RandAugmenter("rand-m9-mstd0.5-inc1", MEAN, "bicubic", seed=0, std=STD)
    draws = [aug.draw(B, S, it).desc for it in range(8)]
    t_def = [med([timed(op_of(d), a.op_iters // 4, a.warmup) for _ in range(a.repeats)]) for d in draws]
    default = report(sum(t_def) / len(t_def), sum(model_bytes(d) for d in draws) / len(draws))
    t0 = time.perf_counter()
    for it in range(20):
        aug.draw(B, S, it)
    default["draw_host_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 3)

    y = torch.randint(0, K, (B,), device="cuda")
    plain, augmented = LinearProbe(model, K), LinearProbe(model, K)
    augmented.enable_randaug(aug)
    step = lambda p: (lambda: p.train_step(x, y, 1e-3, 0.05, 1.0))      # noqa: E731
    t_plain, t_aug = [], []
    for _ in range(a.repeats):                                        # alternating: the two share whatever else the machine does
        t_plain.append(timed(step(plain), a.iters, a.warmup))
        t_aug.append(timed(step(augmented), a.iters, a.warmup))

    res = {"model": a.model, "batch": B, "img_size": S, "classes": K, "iters": a.iters, "op_iters": a.op_iters, "values_m": round(N / 1e6, 2),
           "copy": {"ms": round(t_copy, 4), "tb_per_s": round(copy_rate / 1e12, 3)}, "ops": ops, "default": default,
           "step": {"plain_ms": round(med(t_plain), 4), "randaug_ms": round(med(t_aug), 4), "ratio": round(med(t_aug) / med(t_plain), 4)},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
