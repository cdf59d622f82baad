"""Time an MC-dropout evaluation batch against the deterministic one, and the two combination ops alone, on synthetic data (default:
beit_base_patch16_224, bs = 128, K = 1000) on one GPU.

    python tools/bench_mcd.py [--model M] [--batch B] [--classes K] [--configs T:n [T:n ...]] [--iters N] [--warmup W] [--repeats R] [--out FILE]

Prints one JSON line.  Alternating, so that the ratios do not depend on which ran on a quieter machine:
  (a) the body of a LinearProbe evaluation batch: the deterministic encoder forward, pool + norm, the head, the criterion;
  (b) per (T, n) (default 8:12, 8:3, 32:3), the body of an MCDropoutProbe evaluation batch: (a)'s forward, then T times the tail of the
      last n blocks, pool + norm, the head and uvit_op_mcd_accumulate, then uvit_op_mcd_finalize and the criterion;
  (c) uvit_op_mcd_accumulate and uvit_op_mcd_finalize alone at (B, K).
Each MC batch is reported as a ratio to the deterministic batch of the same group beside the model value 1 + T n / L (DESIGN.md
section 9.14); the reference pays T.  Every figure is a device-event bracket around `iters` back-to-back calls after `warmup` calls of
the same shape, divided by `iters`; the median of `repeats` groups is reported and the groups are kept.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="beit_base_patch16_224")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--configs", nargs="+", default=["8:12", "8:3", "32:3"], metavar="T:n", help="passes : blocks under dropout")
    ap.add_argument("--attn_drop_rate", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcd.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.mcd_probe import MCDropoutProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False,
                         attn_drop_rate=a.attn_drop_rate).cuda().eval()
    B, K, depth = a.batch, a.classes, model.depth
    configs = [tuple(int(v) for v in c.split(":")) for c in a.configs]
    plain = LinearProbe(model, K)
    probes = [MCDropoutProbe(model, K, passes=T, layers=n) for T, n in configs]
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, device="cuda")
    with torch.no_grad():
        for p in [plain] + probes:
            p.head.weight.normal_(0.0, 0.05)
    L, s = lib(), cur_stream

    def batch(p):
        """The body of _evaluate's loop without calibration or detection."""
        n = p._features(x)
        p._mc_batch = 0
        p._logits_into(n)
        check(L.uvit_op_probe_ce(ptr(p._logits), ptr(y), f32(0.0), None, ptr(p._row_loss), ptr(slot), ptr(counters), n, K, s()), "uvit_op_probe_ce")

    for p in [plain] + probes:
        batch(p)
    lin = torch.randn(B, K, device="cuda")
    state = torch.empty(int(L.uvit_op_mcd_state_bytes(B, K)), dtype=torch.uint8, device="cuda")
    z, unc = torch.zeros(B, K, device="cuda"), torch.zeros(B, 5, dtype=torch.float64, device="cuda")
    check(L.uvit_op_mcd_accumulate(ptr(lin), ptr(state), 1, B, K, s()), "uvit_op_mcd_accumulate")
    acc = lambda: check(L.uvit_op_mcd_accumulate(ptr(lin), ptr(state), 0, B, K, s()), "uvit_op_mcd_accumulate")      # noqa: E731
    fin = lambda: check(L.uvit_op_mcd_finalize(ptr(state), 8, 0, ptr(z), ptr(unc), B, K, s()), "uvit_op_mcd_finalize")      # noqa: E731
    groups = []
    for _ in range(a.repeats):
        grp = [timed(lambda: batch(plain), a.iters, a.warmup)]
        grp += [timed(lambda p=p: batch(p), a.iters, a.warmup) for p in probes]
        grp += [timed(acc, 10 * a.iters, a.warmup), timed(fin, 10 * a.iters, a.warmup)]
        groups.append(grp)
    med = lambda vals: sorted(vals)[len(vals) // 2]                                                                 # noqa: E731
    det_ms = med([g[0] for g in groups])
    rows = []
    for i, (T, n) in enumerate(configs):
        ratios = [g[1 + i] / g[0] for g in groups]                     # each against the deterministic batch of its own group
        rows.append({"passes": T, "layers": n, "batch_ms": round(med([g[1 + i] for g in groups]), 4), "ratio_to_deterministic": round(med(ratios), 3),
                     "ratios": [round(r, 3) for r in ratios], "model_1_plus_Tn_over_L": round(1 + T * n / depth, 3), "reference_passes": T})
    out = {"model": a.model, "batch": B, "classes": K, "depth": depth, "attn_drop_rate": a.attn_drop_rate, "iters": a.iters,
           "deterministic_batch_ms": round(det_ms, 4), "mc_batches": rows,
           "mcd_accumulate_ms": round(med([g[-2] for g in groups]), 5), "mcd_finalize_ms": round(med([g[-1] for g in groups]), 5),
           "mcd_state_bytes": int(state.numel()), "groups_ms": [[round(v, 4) for v in g] for g in groups],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
