"""Time the set-level calibration ops on synthetic data (default: beit_base_patch16_224, K = 1000, B = 128) on one GPU.

    python tools/bench_scal.py [--model M] [--batch B] [--classes K] [--iters N] [--warmup W] [--sets N:K,...] [--out FILE]

Prints one JSON line, the protocol of tools/bench_detect.py: every figure is a device-event bracket around `iters` back-to-back calls
after `warmup` calls of the same shape, divided by `iters`.
(a) One evaluation batch (encoder eval forward + pool/norm + logits + cross-entropy, what LinearProbe.evaluate() launches per batch)
    without and with the switch (uvit_op_scal_probs into the store and the device copy of the labels), alternating, in `repeats`
    pairs, and the ratio; the softmax op on its own beside uvit_op_calib_softmax on the same logits.
(b) uvit_op_scal_metrics at every N:K of --sets with its number of launches (uvit_op_scal_launches), and in the same run on the same
    device: torch.sort of the same values as a (K, N) fp32 matrix (the vendor's segmented sort: values and indices); the floor of one
    read of the store, N K 4 bytes at the rate a device copy of the store reaches (read + write); and the per-batch ops of
    csrc/calib.hip (softmax + confidence + tace + auroc) summed over the same set in batches of `batch` rows, `batch_passes` passes.
Needs a GPU; there is nothing to time without one.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="with / without pairs of (a)")
    ap.add_argument("--batch_passes", type=int, default=2, help="timed passes of the per-batch ops over a set (after one warm-up pass); 0 leaves them out")
    ap.add_argument("--sets", default="50000:1000,10000:100,1048576:10,4096:1000", help="N:K of (b)")
    ap.add_argument("--skip_eval_batch", action="store_true", help="(b) only: no encoder is built")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scal.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    from uncertainty_vit_amd.probe_setcalib import SCAL_DEFAULTS
    torch.manual_seed(0)
    L, B = lib(), a.batch
    out = {"model": a.model, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}

    if not a.skip_eval_batch:
        K = a.classes
        model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
        probe = LinearProbe(model, K)
        probe.head.weight.data.normal_(0.0, 0.05)
        x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
        z = probe.logits(x)
        y = torch.where(torch.rand(B, device="cuda") < 0.66, z.argmax(1), torch.randint(0, K, (B,), device="cuda")).contiguous()
        loss_slot = torch.zeros(1, device="cuda")
        store, labels = torch.zeros(4 * B, K, device="cuda"), torch.zeros(4 * B, dtype=torch.int64, device="cuda")
        probs = torch.zeros(B, K, device="cuda")

        def into_store(src):
            check(L.uvit_op_scal_probs(ptr(src), ptr(store[B:]), K, B, K, cur_stream()))
            labels[B:2 * B].copy_(y)

        def eval_batch(on):
            probe._features(x)
            probe._logits_into(B)
            check(L.uvit_op_probe_ce(ptr(probe._logits), ptr(y), f32(0.0), None, ptr(probe._row_loss), ptr(loss_slot), None, B, K, cur_stream()))
            if on:
                into_store(probe._logits)

        op_ms = {"scal_probs_and_label_copy": timed(lambda: into_store(z), a.iters, a.warmup),
                 "calib_softmax": timed(lambda: check(L.uvit_op_calib_softmax(ptr(z), ptr(probs), B, K, cur_stream())), a.iters, a.warmup)}
        pairs = []
        for _ in range(a.repeats):
            off = timed(lambda: eval_batch(False), a.iters, a.warmup)
            on = timed(lambda: eval_batch(True), a.iters, a.warmup)
            pairs.append((on, off))
        out["eval_batch"] = {"B": B, "K": K, "on_off_pairs_ms": [[round(o, 4), round(f, 4)] for o, f in pairs],
                             "on_over_off": [round(o / f, 4) for o, f in pairs], "op_ms": {k: round(v, 4) for k, v in op_ms.items()}}
        del probe, model, x

    from functools import partial
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    # (b) runs on given logits: the encoder behind the probe is never run, a small one carries the K-class head
    tiny = VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=128, depth=1, num_heads=2,
                                                norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1,
                                                use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    sets = {}
    for spec in a.sets.split(","):
        N, K = (int(v) for v in spec.split(":"))
        g = torch.Generator(device="cuda").manual_seed(N + K)
        z = torch.randn(N, K, device="cuda", generator=g) * 2.5
        y = torch.where(torch.rand(N, device="cuda", generator=g) < 0.66, z.argmax(1), torch.randint(0, K, (N,), device="cuda", generator=g)).contiguous()
        p = torch.empty(N, K, device="cuda")
        check(L.uvit_op_scal_probs(ptr(z), ptr(p), K, N, K, cur_stream()))
        h = LinearProbe(tiny, K)
        run = lambda: h._scal_metrics(p, K, y, N, SCAL_DEFAULTS)      # noqa: E731
        table = run()[0].cpu().tolist()
        ms = timed(run, a.iters, a.warmup)
        ws_bytes = int(L.uvit_op_scal_ws_bytes(N, K))
        pt = p.t().contiguous()
        sort_ms = timed(lambda: torch.sort(pt, dim=1), a.iters, a.warmup)
        copy_ms = timed(lambda: p.clone(), a.iters, a.warmup)
        rate = 2.0 * 4 * N * K / (copy_ms * 1e-3)                                   # bytes per second, read + write
        del pt
        # the per-batch ops over the same set
        h._buffers_for(B, calibration=True)
        slab = torch.zeros(5, dtype=torch.float64, device="cuda")

        def per_batch_pass():
            for n0 in range(0, N, B):
                b = min(B, N - n0)
                h._calibration_into(z[n0:n0 + b], y[n0:n0 + b], b, slab.data_ptr(), reference_bin_accuracy=False)

        pb_ms = timed(per_batch_pass, a.batch_passes, 1) if a.batch_passes else float("nan")      # 0: a profiler run of the set op alone
        sets[spec] = {"N": N, "K": K, "metrics_ms": round(ms, 4), "launches": int(L.uvit_op_scal_launches(N, K, ws_bytes)), "ws_bytes": ws_bytes,
                      "torch_sort_ms": round(sort_ms, 4), "metrics_over_torch_sort": round(ms / sort_ms, 3),
                      "store_bytes": 4 * N * K, "copy_rate_GBps": round(rate / 1e9, 1), "read_floor_ms": round(4 * N * K / rate * 1e3, 4),
                      "metrics_over_read_floor": round(ms / (4 * N * K / rate * 1e3), 1),
                      "per_batch_ops_ms": round(pb_ms, 3), "per_batch_batches": (N + B - 1) // B, "metrics_over_per_batch_ops": round(ms / pb_ms, 4),
                      "ECE": round(table[0], 6), "SCE": round(table[5], 6), "TACE": round(table[7], 6), "AUROC": round(table[8], 6)}
        del z, p, y, h
        torch.cuda.empty_cache()
    out["sets"] = sets
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
