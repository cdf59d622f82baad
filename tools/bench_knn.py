"""Time the k-NN search against the unfused vendor baseline and its floor, and a detection batch with and without a neighbour bank, on
synthetic data (default: beit_base_patch16_224, bs = 128, k = 20, banks of 2^17 and 2^20 random unit rows) on one GPU.

    python tools/bench_knn.py [--model M] [--batch B] [--k K] [--banks N [N ...]] [--classes K] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.  Per bank size, alternating so that the ratios do not depend on which ran on a quieter machine:
  (a) uvit_op_knn_search (both kernels: the streaming search and the merge), slabs chosen by the op;
  (b) torch.topk(q @ bank.T, k) on the same bf16 data: the vendor GEMM writes the (B, N) similarities, a second kernel selects;
  (c) the floor max(2 B N C / 2.5 PFLOP/s, bank bytes / 8 TB/s) with the constants of DESIGN.md section 4;
  (d) the body of an evaluate(detection=True) batch with the bank (rows, search, scores and one column copy more) and without.
Every figure is a device-event bracket around `iters` back-to-back calls after `warmup` calls of the same shape, divided by `iters`;
the median of `repeats` groups is reported and the groups are kept.  The two searches' results are compared at the timed size: the
share of rows whose nearest index agrees and the largest difference of the k-th similarity (bf16 output of the vendor GEMM against
fp32).  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_probe import timed  # noqa: E402

PEAK_BF16, PEAK_HBM = 2.5e15, 8e12           # dense bf16 matrix rate and HBM bandwidth, per second


def unit_rows(n, c, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(n, c, dtype=torch.bfloat16, device="cuda")
    for lo in range(0, n, 1 << 16):                                           # in pieces: the fp32 draw of 2^20 x 768 would be 3 GB
        x = torch.randn(min(1 << 16, n - lo), c, generator=g, device="cuda")
        out[lo:lo + len(x)] = (x / x.norm(dim=1, keepdim=True)).bfloat16()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--banks", type=int, nargs="+", default=[1 << 17, 1 << 20])
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    plain, near = LinearProbe(model, a.classes), LinearProbe(model, a.classes)
    B, K, Cd, k = a.batch, a.classes, model.embed_dim, a.k
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    with torch.no_grad():
        for p in (plain, near):
            p.head.weight.normal_(0.0, 0.05)
            p._features(x)
    L, s = lib(), cur_stream
    q = unit_rows(B, Cd, 1)
    valid = torch.zeros(B, dtype=torch.int32, device="cuda")
    sim = torch.zeros(B, k, dtype=torch.float32, device="cuda")
    idx = torch.zeros(B, k, dtype=torch.int32, device="cuda")

    def det_batch(p):
        """The body of _evaluate's loop with detection=True, without the cross-entropy: one batch into an empty store."""
        n = p._features(x)
        p._det["n"] = 0
        p._det_reserve(n)
        for score, ev in p._score_eval:
            score.eval_batch(n, y, ev)
            ev["slabs"].clear()
        p._logits_into(n)
        p._det_rows(n, y)

    results = []
    for N in a.banks:
        bank = unit_rows(N, Cd, 2)
        labels = torch.randint(0, K, (N,), device="cuda").int()
        ws = torch.empty(int(L.uvit_op_knn_search_ws_bytes(B, Cd, N, k, 0)), dtype=torch.uint8, device="cuda")
        fused = lambda: check(L.uvit_op_knn_search(ptr(q), ptr(valid), ptr(bank), ptr(labels), ptr(sim), ptr(idx), k, ptr(ws), ws.numel(),      # noqa: E731
                                                   B, Cd, N, k, 0, s()))
        vendor = lambda: torch.topk(q @ bank.T, k)                                                                                             # noqa: E731
        near.set_neighbours(None)
        near.load_neighbour_state({"bank": bank, "labels": labels, "sums": torch.tensor([float(N), 0.0]), "k": k, "temperature": 0.07})
        for p in (plain, near):
            p._det = {"scores": None, "flags": None, "cap": 0, "n": 0}
        near._score_eval = [(near._bank, {"correct": torch.zeros(1, dtype=torch.int32, device="cuda"), "slabs": []})]
        groups = [(timed(fused, a.iters, a.warmup), timed(vendor, a.iters, a.warmup), timed(lambda: det_batch(plain), a.iters, a.warmup),
                   timed(lambda: det_batch(near), a.iters, a.warmup)) for _ in range(a.repeats)]
        plain._det, near._det, near._score_eval = None, None, ()
        t_fused, t_vendor, t_plain, t_near = (sorted(grp[i] for grp in groups)[len(groups) // 2] for i in range(4))
        fused()
        tv, ti = vendor()
        torch.cuda.synchronize()
        flops, nbytes = 2.0 * B * N * Cd, 2.0 * N * Cd
        floor = 1e3 * max(flops / PEAK_BF16, nbytes / PEAK_HBM)
        results.append({"bank_rows": N, "slabs": int(ws.numel() // (B * k * 8)), "search_ms": round(t_fused, 4), "torch_topk_ms": round(t_vendor, 4),
                        "floor_ms": round(floor, 4), "floor_bound": "flops" if flops / PEAK_BF16 > nbytes / PEAK_HBM else "bytes",
                        "search_over_torch": round(t_fused / t_vendor, 4), "search_over_floor": round(t_fused / floor, 3),
                        "search_tflop_per_s": round(flops / t_fused / 1e9, 1), "search_bank_tb_per_s": round(nbytes / t_fused / 1e9, 3),
                        "detection_batch_ms": round(t_plain, 4), "detection_batch_with_bank_ms": round(t_near, 4),
                        "with_bank_over_without": round(t_near / t_plain, 4), "groups_ms": [[round(v, 4) for v in grp] for grp in groups],
                        "nearest_index_agreement": round(float((ti[:, 0].int() == idx[:, 0]).float().mean()), 4),
                        "kth_similarity_max_diff": float((tv[:, -1].float() - sim[:, -1]).abs().max())})
        del bank, labels, ws, tv, ti
        near.set_neighbours(None)
        torch.cuda.empty_cache()
    out = {"model": a.model, "batch": B, "k": k, "embed_dim": Cd, "classes": K, "iters": a.iters, "banks": results,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
