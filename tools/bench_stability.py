"""Time the stability ops of perturbation sequences on synthetic data (default: beit_base_patch16_224, K = 100 and 1000, V = 4
sequences of F = 31 frames per batch) on one GPU.

    python tools/bench_stability.py [--model M] [--classes 100,1000] [--frames F] [--sequences V] [--iters N] [--warmup W] [--out FILE]

Prints one JSON line.  Per class count: one evaluation batch of V F images (encoder eval forward + pool/norm + logits, what
LinearProbe.evaluate_stability() launches per batch) without and with the two stability ops, alternating on the same build, and their
ratio; the time of each op on its own (ranks, sequences) and of both as stability_batch issues them.  Every figure is a device-event
bracket around `iters` back-to-back calls after `warmup` calls of the same shape, divided by `iters`: for the small ops that is
launch spacing as much as kernel time.  The frames of a sequence drift (a tenth of the logits changes from frame to frame), so that
the pairs have something to count.  The reference's host path (scipy rankdata per frame, numpy per pair) is not timed here: the
reference is not on the GPU host.  Needs a GPU; there is nothing to time without one.
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--classes", default="100,1000")
    ap.add_argument("--frames", type=int, default=31)
    ap.add_argument("--sequences", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the with / without pair to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stability.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    V, F, L = a.sequences, a.frames, lib()
    B = V * F
    base = torch.randn(V, 1, 3, model.img_size, model.img_size, device="cuda")
    x = (base + 0.3 * torch.randn(V, F, 3, model.img_size, model.img_size, device="cuda").cumsum(1)).view(B, 3, model.img_size, model.img_size)
    results = {}
    for K in (int(v) for v in a.classes.split(",")):
        probe = LinearProbe(model, K)
        probe.head.weight.data.normal_(0.0, 0.05)         # logits of spread ~1.4 on unit features: a head that has an opinion
        z = probe.logits(x)
        sums = probe.stability_batch(z, F, False).clone()
        per_seq = (sums / (F - 1)).cpu()
        assert bool(torch.isfinite(per_seq).all()), per_seq
        slot = torch.zeros(V, 3, dtype=torch.float64, device="cuda")

        def eval_batch(stability):
            # what evaluate_stability() launches for one batch
            probe._features(x)
            probe._logits_into(B)
            if stability:
                probe._stability_into(probe._logits, V, F, False, slot.data_ptr())

        s = cur_stream
        parts = {
            "ranks": lambda: check(L.uvit_op_stability_ranks(ptr(z), ptr(probe._ranks), B, K, s())),
            "sequences": lambda: check(L.uvit_op_stability_sequences(ptr(probe._ranks), ptr(slot), V, F, K, 0, s())),
            "stability_batch": lambda: probe._stability_into(z, V, F, False, slot.data_ptr()),
        }
        ms = {k: timed(fn, a.iters, a.warmup) for k, fn in parts.items()}
        pairs = []
        for _ in range(a.repeats):          # alternating, so that the ratio does not depend on which ran on a quieter machine
            off = timed(lambda: eval_batch(False), a.iters, a.warmup)
            on = timed(lambda: eval_batch(True), a.iters, a.warmup)
            pairs.append((on, off))
        on_ms = sorted(p_[0] for p_ in pairs)[len(pairs) // 2]
        off_ms = sorted(p_[1] for p_ in pairs)[len(pairs) // 2]
        results[str(K)] = {"eval_batch_ms": round(off_ms, 4), "eval_batch_stability_ms": round(on_ms, 4),
                           "stability_on_over_off": round(on_ms / off_ms, 4),
                           "on_off_pairs_ms": [[round(o, 4), round(f, 4)] for o, f in pairs],
                           "op_ms": {k: round(v, 4) for k, v in ms.items()},
                           "metrics": {"flip_prob": float(per_seq[:, 0].mean()), "top5_dist": float(per_seq[:, 1].mean()),
                                       "zipf_dist": float(per_seq[:, 2].mean())}}
    out = {"model": a.model, "frames": F, "sequences": V, "batch": B, "iters": a.iters, "warmup": a.warmup, "classes": results,
           "reference_host_path": "not timed: the reference is not on the GPU host", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
