"""Time the ensemble probe head beside the linear head on synthetic data (default: beit_base_patch16_224, bs = 128, K = 1000, M = 5
members) on one GPU.

    python tools/bench_ens.py [--model M] [--batch B] [--classes K] [--members M] [--iters N] [--warmup W] [--out FILE]

Prints one JSON line: the ensemble training step (encoder eval forward + pool/norm + the (M K, C) head + the members' cross-entropies
+ head gradient + per-member clip + clip norm + AdamW) without and with bagging plus clip, the linear head's training step and the
encoder's eval forward alone on the same batch, alternating, so that the ratios do not depend on which ran on a quieter machine; an
evaluation batch of the linear head (forward + head + cross-entropy) and of the ensemble without and with the members' criterion and
the uncertainty columns; and the time of each op alone.  Every figure is a device-event bracket around `iters` back-to-back calls
after `warmup` calls of the same shape, divided by `iters`.  Needs a GPU.
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
    ap.add_argument("--members", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="repeat the alternating group to show the spread")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ens.py measures on a GPU; none is visible")
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import create_model
    from uncertainty_vit_amd.native import check, cur_stream, f32, lib, ptr
    torch.manual_seed(0)
    model = create_model(a.model, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()
    ens = EnsembleProbe(model, a.classes, members=a.members)
    bag = EnsembleProbe(model, a.classes, members=a.members, bagging=True)
    lin = LinearProbe(model, a.classes)
    B, K, Cd, M = a.batch, a.classes, model.embed_dim, a.members
    x = torch.randn(B, 3, model.img_size, model.img_size, device="cuda")
    y = torch.randint(0, K, (B,), device="cuda")
    for p in (ens, bag, lin):
        loss, _ = p.train_step(x, y, 1e-3, 0.05, 1.0)
        assert bool(torch.isfinite(loss))
    L, s = lib(), cur_stream
    rows = ens._rows
    counters, unc = torch.zeros(M, 2, dtype=torch.int32, device="cuda"), torch.zeros(B, 5, dtype=torch.float64, device="cuda")
    parts = {
        "linear_logits": lambda: check(L.uvit_op_probe_logits(ptr(lin._feat), ptr(lin._arena), torch_ptr(lin._arena, K * Cd), ptr(lin._logits), B, K,
                                                              Cd, s())),
        "head_logits": lambda: check(L.uvit_op_probe_logits(ptr(ens._feat), ptr(ens._arena), ens._bias_ptr(ens._arena), ptr(ens._lin), B, rows, Cd, s())),
        "bag_weights": lambda: check(L.uvit_op_ens_bag_weights(ptr(ens._bag), B, M, 42, s())),
        "ens_ce": lambda: check(L.uvit_op_ens_ce(ptr(ens._lin), ptr(y), None, f32(0.1), ptr(ens._dlin), ptr(ens._member_rows), ptr(ens._member_loss),
                                                 None, B, M, K, s())),
        "ens_ce_weighted": lambda: check(L.uvit_op_ens_ce(ptr(ens._lin), ptr(y), ptr(ens._bag), f32(0.1), ptr(ens._dlin), ptr(ens._member_rows),
                                                          ptr(ens._member_loss), None, B, M, K, s())),
        "ens_ce_eval": lambda: check(L.uvit_op_ens_ce(ptr(ens._lin), ptr(y), None, f32(0.0), None, ptr(ens._member_rows), ptr(ens._member_loss),
                                                      ptr(counters), B, M, K, s())),
        "linear_head_grad": lambda: check(L.uvit_op_probe_head_grad(ptr(lin._dlogits), ptr(lin._feat), ptr(lin._grad_arena),
                                                                    torch_ptr(lin._grad_arena, K * Cd), B, K, Cd, s())),
        "head_grad": lambda: check(L.uvit_op_probe_head_grad(ptr(ens._dlin), ptr(ens._feat), ptr(ens._grad_arena), ens._bias_ptr(ens._grad_arena), B,
                                                             rows, Cd, s())),
        "ens_clip_norms": lambda: check(L.uvit_op_ens_clip(ptr(ens._grad_arena), ptr(ens.member_norms), M, K, Cd, f32(0.0), s())),
        "ens_clip": lambda: check(L.uvit_op_ens_clip(ptr(ens._grad_arena), ptr(ens.member_norms), M, K, Cd, f32(1.0), s())),
        "combine_logits": lambda: check(L.uvit_op_ens_combine(ptr(ens._lin), 0, ptr(ens._logits), None, B, M, K, s())),
        "combine_probs": lambda: check(L.uvit_op_ens_combine(ptr(ens._lin), 1, ptr(ens._logits), None, B, M, K, s())),
        "combine_logits_unc": lambda: check(L.uvit_op_ens_combine(ptr(ens._lin), 0, ptr(ens._logits), ptr(unc), B, M, K, s())),
        "linear_update": lambda: update(lin),
        "ens_update": lambda: update(ens),
    }

    def update(p):
        p._clip_and_update(1e-3, 0.05, None)
        p.step_count -= 1

    ms = {k: timed(fn, a.iters, a.warmup) for k, fn in parts.items()}

    def lin_eval():
        n = lin._features(x)
        lin._logits_into(n)
        check(L.uvit_op_probe_ce(ptr(lin._logits), ptr(y), f32(0.0), None, ptr(lin._row_loss), ptr(lin._stats), ptr(counters), n, K, s()))

    def ens_eval(full):
        n = ens._features(x)
        ens._lin_into(n)
        ens._combine_into(n, unc if full else None)
        check(L.uvit_op_probe_ce(ptr(ens._logits), ptr(y), f32(0.0), None, ptr(ens._row_loss), ptr(ens._stats), ptr(counters), n, K, s()))
        if full:
            check(L.uvit_op_ens_ce(ptr(ens._lin), ptr(y), None, f32(0.0), None, ptr(ens._member_rows), ptr(ens._member_loss), ptr(counters), n, M, K,
                                   s()))

    names = ("encoder_forward", "linear_step", "ens_step", "ens_step_bagging_clip", "linear_eval_batch", "ens_eval_batch", "ens_eval_batch_members_unc")
    groups = []
    for _ in range(a.repeats):
        groups.append((timed(lambda: model.forward_features(x, None, None), a.iters, a.warmup),
                       timed(lambda: lin.train_step(x, y, 1e-3, 0.05), a.iters, a.warmup),
                       timed(lambda: ens.train_step(x, y, 1e-3, 0.05), a.iters, a.warmup),
                       timed(lambda: bag.train_step(x, y, 1e-3, 0.05, 1.0), a.iters, a.warmup),
                       timed(lin_eval, a.iters, a.warmup),
                       timed(lambda: ens_eval(False), a.iters, a.warmup),
                       timed(lambda: ens_eval(True), a.iters, a.warmup)))
    med = dict(zip(names, (sorted(grp[i] for grp in groups)[len(groups) // 2] for i in range(len(names)))))
    out = {"model": a.model, "batch": B, "classes": K, "members": M, "iters": a.iters, **{k + "_ms": round(v, 4) for k, v in med.items()},
           "linear_step_over_encoder_forward": round(med["linear_step"] / med["encoder_forward"], 4),
           "ens_step_over_linear_step": round(med["ens_step"] / med["linear_step"], 4),
           "ens_step_bagging_clip_over_linear_step": round(med["ens_step_bagging_clip"] / med["linear_step"], 4),
           "ens_eval_over_linear_eval": round(med["ens_eval_batch"] / med["linear_eval_batch"], 4),
           "ens_eval_members_unc_over_linear_eval": round(med["ens_eval_batch_members_unc"] / med["linear_eval_batch"], 4),
           "group_names": list(names), "groups_ms": [[round(v, 4) for v in grp] for grp in groups],
           "part_ms": {k: round(v, 4) for k, v in ms.items()}, "head_parameters": int(ens._arena.numel()), "lin_bytes": 4 * B * rows,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def torch_ptr(t, offset):
    """Device pointer `offset` floats into the fp32 tensor t."""
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * offset)


if __name__ == "__main__":
    main()
