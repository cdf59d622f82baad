"""Time the probe's training-time mixing on synthetic data (default: beit_base_patch16_224, bs = 128, S = 224, K = 1000) on one GPU.

    python tools/bench_mix.py [--model M] [--batch B] [--classes K] [--iters N] [--op_iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line and writes it to --out (default: profiles/mix_bench.json):
  ops        uvit_op_mix_batch per (kind, erase mode): the op's time with its two descriptor copies from pinned memory, the bytes its
             descriptors make it move (the output written once; a row's own image read outside its cutmix box, its partner's inside it
             or, for mixup, everywhere; erased pixels are read all the same), that count over the HBM peak (8.0 TB/s, the spec) and over
             what a float4 copy reaches (6.29 TB/s), and the op's ratio to both and to uvit_op_corrupt_batch brightness timed in the
             same run (a streaming op with the same output, reading a quarter as much)
  criterion  uvit_op_probe_ce_mix against uvit_op_probe_ce on the same logits
  step       LinearProbe.train_step with an `elem` mixer (mixup 0.8, cutmix 1.0, reprob 0.25, pixel) against one without, and the host
             time of one BatchMixer.draw
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


def moved_bytes(desc, S):
    """Bytes uvit_op_mix_batch has to move for these descriptors: out written once; none reads its own image, mixup both, cutmix its
    own outside the box and its partner's inside it (one image's worth together)."""
    plane = 3 * S * S * 4
    return sum(plane + (2 * plane if int(d["kind"]) == 1 else plane) for d in desc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--op_iters", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mix_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix.py measures on a GPU; none is visible")
    from uncertainty_vit_amd import corruptions as co
    from uncertainty_vit_amd.datasets import IMAGENET_DEFAULT_MEAN as MEAN, IMAGENET_DEFAULT_STD as STD
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    from uncertainty_vit_amd.probe_mix import MIX_DESC, BatchMixer
    torch.manual_seed(0)
    L = lib()
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    B, S, K = a.batch, model.img_size, a.classes
    x = torch.randn(B, 3, S, S, device="cuda")
    out = torch.empty_like(x)
    med = lambda vals: sorted(vals)[len(vals) // 2]      # noqa: E731
    plane_bytes = B * 3 * S * S * 4

    # ---- the op per (kind, erase mode) ----
    erase = BatchMixer(reprob=0.25, recount=1, seed=0).draw(B, S, 0).boxes            # a quarter of the rows, one box each
    kinds = {"none": (0, 1.0, (0, 0, 0, 0)), "mixup": (1, 0.5, (0, 0, 0, 0)), "cutmix": (2, 0.5, (S // 4, S // 4 + S // 2, 0, S))}
    pinned = []

    def op_case(kind, boxes, mode):
        desc = np.zeros(B, dtype=MIX_DESC)
        desc["partner"] = B - 1 - np.arange(B)
        desc["kind"], desc["lam"] = kinds[kind][0], kinds[kind][1]
        desc["yl"], desc["yh"], desc["xl"], desc["xh"] = kinds[kind][2]
        R = boxes.shape[1]
        pack = np.concatenate([desc.view(np.uint8).reshape(-1), np.ascontiguousarray(boxes).view(np.uint8).reshape(-1)])
        hostbuf = torch.from_numpy(pack.copy()).pin_memory()
        pinned.append(hostbuf)
        need = L.uvit_op_mix_ws_bytes(B, R)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        hp = hostbuf.data_ptr()

        def op():
            check(L.uvit_op_mix_batch(ptr(x), ptr(out), C.c_void_p(hp), C.c_void_p(hp + desc.nbytes) if R else None, B, S, R, mode, 1, 0, ptr(ws), need,
                                      cur_stream()), "uvit_op_mix_batch")
        return op, moved_bytes(desc, S)

    u8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device="cuda")
    owner = type("Owner", (), {})()
    bright = torch.from_numpy(co.corruption_params("brightness", 3, S)).cuda()
    op_bright = lambda: co.corrupt(owner, u8, "brightness", bright, 0, 0, MEAN, STD, out=out)      # noqa: E731
    op_bright()
    t_bright = med([timed(op_bright, a.op_iters, a.warmup) for _ in range(a.repeats)])
    ops = {}
    no_boxes = np.zeros((B, 0, 4), dtype=np.int32)
    for kind in kinds:
        for name, boxes, mode in (("off", no_boxes, 0), ("const", erase, 0), ("rand", erase, 1), ("pixel", erase, 2)):
            op, n_bytes = op_case(kind, boxes, mode)
            t = med([timed(op, a.op_iters, a.warmup) for _ in range(a.repeats)])
            floor, floor_copy = n_bytes / HBM_PEAK * 1e3, n_bytes / HBM_COPY * 1e3
            ops[f"{kind}_{name}"] = {"op_ms": round(t, 4), "bytes_mb": round(n_bytes / 1e6, 1), "byte_floor_ms": round(floor, 4),
                                     "byte_floor_copy_rate_ms": round(floor_copy, 4), "ratio_to_floor": round(t / floor, 3),
                                     "ratio_to_copy_rate_floor": round(t / floor_copy, 3), "ratio_to_brightness": round(t / t_bright, 3),
                                     "tb_per_s": round(n_bytes / (t * 1e-3) / 1e12, 3)}

    # ---- the criterion ----
    logits = torch.randn(B, K, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    partner = torch.arange(B - 1, -1, -1, dtype=torch.int32, device="cuda")
    lam = torch.rand(B, device="cuda")
    d, rows, slot = torch.empty(B, K, device="cuda"), torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
    ce = lambda: check(L.uvit_op_probe_ce(ptr(logits), ptr(y), f32(0.1), ptr(d), ptr(rows), ptr(slot), None, B, K, cur_stream()), "uvit_op_probe_ce")      # noqa: E731
    ce_mix = lambda: check(L.uvit_op_probe_ce_mix(ptr(logits), ptr(y), ptr(partner), ptr(lam), f32(0.1), ptr(d), ptr(rows), ptr(slot), B, K,      # noqa: E731
                                                  cur_stream()), "uvit_op_probe_ce_mix")
    t_ce = med([timed(ce, a.op_iters, a.warmup) for _ in range(a.repeats)])
    t_ce_mix = med([timed(ce_mix, a.op_iters, a.warmup) for _ in range(a.repeats)])

    # ---- the step ----
    mixer = BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", reprob=0.25, seed=0)
    plain, mixed = LinearProbe(model, K), LinearProbe(model, K)
    mixed.enable_mix(mixer)
    step = lambda p: (lambda: p.train_step(x, y, 1e-3, 0.05, 1.0))      # noqa: E731
    t_plain, t_mixed = [], []
    for _ in range(a.repeats):                                        # alternating: the two share whatever else the machine does
        t_plain.append(timed(step(plain), a.iters, a.warmup))
        t_mixed.append(timed(step(mixed), a.iters, a.warmup))
    t0 = time.perf_counter()
    for it in range(20):
        mixer.draw(B, S, it)
    draw_ms = (time.perf_counter() - t0) / 20 * 1e3

    res = {"model": a.model, "batch": B, "img_size": S, "classes": K, "iters": a.iters, "op_iters": a.op_iters, "image_mb": round(plane_bytes / 1e6, 1),
           "brightness_ms": round(t_bright, 4), "ops": ops, "worst_ratio_to_copy_rate_floor": max(r["ratio_to_copy_rate_floor"] for r in ops.values()),
           "criterion": {"ce_ms": round(t_ce, 4), "ce_mix_ms": round(t_ce_mix, 4), "ratio": round(t_ce_mix / t_ce, 3)},
           "step": {"plain_ms": round(med(t_plain), 4), "mixed_ms": round(med(t_mixed), 4), "ratio": round(med(t_mixed) / med(t_plain), 4),
                    "draw_host_ms": round(draw_ms, 3)},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
