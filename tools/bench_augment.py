"""Cost of the image-folder augmentation on the GPU (uvit_op_augment_batch), per 128-image batch.

    python tools/bench_augment.py [--batch 128] [--iters 50] [--steps 20] [--out profiles/augment_bench.json]

1. device time of one uvit_op_augment_batch launch (HIP events, pixels already resident) over an ImageNet-like mix of decoded
   sizes (SIZE_MIX, fixed below) at the default --aug_level -1 parameters;
2. the host-to-device bytes of such a batch (packed uint8 pixels + descriptors) against the fp32 batch it replaces;
3. the ViT-B/16 bs=128 training step fed (a) a resident fp32 batch and (b) packed batches through DevicePrefetcher, which uploads
   and augments batch i+1 on its side stream while step i runs; (a) and (b) alternate, 3 rounds each.
Needs a GPU; prints and writes one JSON object.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# decoded (height, width) of an ImageNet-1k-like training set: the common JPEG shapes (landscape 4:3 dominates) with weights
SIZE_MIX = [((375, 500), 40), ((500, 375), 12), ((333, 500), 10), ((500, 333), 5), ((334, 500), 3), ((281, 500), 3),
            ((400, 500), 3), ((500, 500), 3), ((480, 640), 3), ((240, 320), 2), ((600, 800), 2), ((1200, 1600), 1),
            ((150, 200), 2), ((375, 375), 2), ((768, 1024), 1), ((2000, 3000), 1), ((90, 120), 1), ((250, 500), 2)]


def packed_batches(n_batches, B, S, seed=0):
    from uncertainty_vit_amd import datasets as ds
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    random.seed(seed)
    aug = ds.BEiTAugment(S, -1, "bicubic")
    sizes, w = zip(*SIZE_MIX)
    p = np.asarray(w, np.float64) / sum(w)
    gen = ds.MaskingGenerator((S // 16, S // 16), 75, min_num_patches=16)
    out = []
    for _ in range(n_batches):
        items = []
        for k in rng.choice(len(sizes), B, p=p):
            h, wd = sizes[k]
            img = rng.integers(0, 256, (h, wd, 3), dtype=np.uint8)
            items.append(((img, aug(h, wd), gen(), aug.size, aug.mean, aug.std), 0))
        out.append(ds.collate_packed(items).pin_memory())
    return out


def kernel_time(batches, S, iters):
    from uncertainty_vit_amd import native
    dev = torch.device("cuda")
    res = []
    for pb in batches:
        px = pb.pixels.to(dev)
        out = torch.empty((len(pb), 3, S, S), device=dev)
        ws = torch.empty(native.augment_ws_bytes(pb.desc, S), dtype=torch.uint8, device=dev)
        s = native.cur_stream()
        for _ in range(3):
            native.augment_batch(px, pb.desc, S, pb.mean, pb.std, out, ws, s)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            native.augment_batch(px, pb.desc, S, pb.mean, pb.std, out, ws, s)
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / iters)
    return res


def step_times(batches, B, S, steps):
    """ms per step: resident fp32 batch vs packed batches through the prefetcher (augmentation on its side stream)."""
    from uncertainty_vit_amd import optim_factory, utils
    from uncertainty_vit_amd.engine_for_cyclical import DevicePrefetcher, make_step_params, native_step
    from uncertainty_vit_amd.modeling_cyclical import create_model
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = create_model("beit_base_patch16_224", pretrained=False, drop_path_rate=0.1, drop_rate=0.0, use_shared_rel_pos_bias=True,
                         use_abs_pos_emb=False, init_values=0.1, attn_drop_rate=0.0, gp_layer=False, gumbel_softmax=False,
                         sinkformer=False, h_sto_trans=False).to(dev)
    ema = utils.ModelEmaV2(model, decay=0.9998)

    class A:
        opt, lr, weight_decay, opt_eps, opt_betas = "adamw", 2e-5, 0.05, 1e-8, (0.9, 0.999)
    opt = optim_factory.create_optimizer(A(), model)
    opt._ensure_state()
    engine = model.engine(B, teacher=ema.module, adam_m=opt.exp_avg, adam_v=opt.exp_avg_sq)
    depth = model.depth

    def step(i, x, mask, rows):
        hp = make_step_params(list(range(depth // 2, depth)), opt, 3.0, 0.12, False, -1, True, False, 0.9998, True, 1, 0, i,
                              depth=depth, n_rows_hint=rows)
        hp.lr = 2e-5
        native_step(engine, None, x, mask.reshape(B, -1).to(torch.int64).contiguous(), hp)

    (x_res, m_res), _ = next(iter(DevicePrefetcher(batches[:1], dev)))
    x_res, m_res = x_res.clone(), m_res.clone()
    rows_res = int(m_res.sum().item())
    it = [0]

    def resident():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(it[0], x_res, m_res, rows_res)
            it[0] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def augmented():
        loader = [batches[i % len(batches)] for i in range(steps + 1)]
        pf = DevicePrefetcher(loader, dev)
        torch.cuda.synchronize()
        t0 = None
        for k, ((x, m), _) in enumerate(pf):
            if k == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            step(it[0], x, m, pf.mask_rows)
            it[0] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    resident()
    augmented()                     # warm-up of both paths
    res, aug = [], []
    for _ in range(3):
        res.append(resident())
        aug.append(augmented())
    return res, aug


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--n-batches", type=int, default=4)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_augment measures the GPU kernel: no GPU, no number"
    batches = packed_batches(a.n_batches, a.batch, a.size)
    us = kernel_time(batches, a.size, a.iters)
    h2d = [int(b.pixels.numel() + b.desc.numel()) for b in batches]
    res, aug = step_times(batches, a.batch, a.size, a.steps)
    r = {"batch": a.batch, "size": a.size, "aug_level": -1, "interpolation": "bicubic", "device": torch.cuda.get_device_name(),
         "kernel_us_per_batch": [round(v, 1) for v in us], "kernel_us_per_batch_mean": round(float(np.mean(us)), 1),
         "h2d_bytes_per_batch_mean": int(np.mean(h2d)), "fp32_batch_bytes": a.batch * 3 * a.size * a.size * 4,
         "step_ms_resident": [round(v, 3) for v in res], "step_ms_augmented_side_stream": [round(v, 3) for v in aug],
         "step_overhead_pct": round(100 * (min(aug) / min(res) - 1), 2),
         "method": f"kernel: HIP events over {a.iters} launches per batch, {a.n_batches} batches of the SIZE_MIX; steps: {a.steps} "
                   "ViT-B/16 steps per round, resident vs prefetcher-augmented alternating, 3 rounds, overhead from the best rounds"}
    print(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
