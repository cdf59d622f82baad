"""GPU: a training step does not depend on what the engine ran before it.

The engine keeps invariants across steps in a workspace that is zeroed once, at creation: the pad rows of every activation
and dY buffer up to the wgrads' reduction length are zero, the dense dXb / dY2 of a masked-row step are zero outside the listed
rows, the tile counters are back at zero.  Every oracle test runs ONE step on a FRESH engine, where all of that holds trivially.
Here one engine runs a schedule of steps (tests/gpu_util.py::HISTORY: drop-path lists that shrink, grow and run empty, lists
switched off and on, masked-row counts that change, a dense step between compact ones, an eval forward at another batch size),
and every step is compared with the same step -- same weights and EMA weights, batch, seed and iteration -- on a fresh engine,
which is what the oracle tests validate.  The steps with an empty list, which no oracle test reaches, are also compared, on the
fresh engine, with the float64 oracle with the kernels' masks replayed.

Bounds, used against fresh: those of "same step, other row plan" (test_drop_path_sample_lists_equal_all_samples): loss rel 2e-5,
grad-norm rel 2e-4, every gradient tensor max-norm 2e-3 and relative L2 2e-3 -- the two runs differ by nothing but the order of
the fp32 atomics of the split wgrads and column sums.  Targets and student outputs come out of forward passes without atomics:
every row to 1e-5 of its norm (the bound test_target_builder_production holds fp32 rows to).

Measured on an MI355X: the file takes 12 s; used against fresh is at most 5.5e-7 (loss) and 4.2e-7 / 1.9e-7 (gradients, max-norm /
relative L2), targets and outputs are bit-identical, and fresh against fresh is of the same size (<= 7e-8 on the tiny models).
The oracle steps run on the host (no device memory).  Found by the `tiny2` schedule (step it 8 after it 6) and fixed in
uvit_step_backward_layer: a dense two-stream MLP branch read the covariance stream's compact rows of an earlier stacked-list
launch in the pad rows M .. Mpad of dY1 (blocks.3.mlp.fc1.bias off by 2.3e-1 relative L2, fresh against fresh 6e-9)."""
import copy
import time

import pytest
import torch

import test_gpu_fullsize as fs
from gpu_util import (HISTORY, HISTORY_SEED, assert_grads_close, grad_errors, history_batch, history_cfg, history_kept_counts,
                      native_model, native_steps, native_trainer)
from oracle import vit_oracle as vo

pytestmark = pytest.mark.gpu
LAM = 1e-2             # Wasserstein weight of the two-stream schedule (as in the two-stream oracle tests: the covariance stream weighs in)


def set_lists(model, on):
    model.drop_path_rows = on
    if model._engine is not None:
        model._engine.set_drop_path_rows(on)


def run_step(model, ema, opt, batch, it, h):
    x, mask, host = batch
    b = (x, mask) if host else (x.cuda(), mask.cuda())
    st = native_steps(model, ema, opt, [b], h["target_layers"], start=it, stochastic=h["two_stream"], lam=LAM)[0]
    e, C, n = model._engine, model.embed_dim, int(mask.sum())
    out = {"loss": st["loss"], "grad_norm": st["grad_norm"], "compact": e.compact_rows(), "lists": e.drop_path_rows,
           "grads": {k: q.grad.detach().float().cpu().clone() for k, q in model.named_parameters() if q.grad is not None}}
    for name in ("targets", "outputs") + (("targets_cov", "outputs_cov") if h["two_stream"] else ()):
        out[name] = e.ws_tensor(name, 0, (n, C)).clone()
    return out


def fresh_copy(model, ema, lists):
    """A new model, EMA model, optimizer and (at its first step) engine holding the weights `model` and `ema` hold now."""
    m = copy.deepcopy(model)
    m.drop_path_rows = lists
    e, o = native_trainer(m)
    e.module._arena.copy_(ema.module._arena)
    e.module.mark_weights_changed()
    return m, e, o


def figures(a, b):
    errs = grad_errors(a["grads"], b["grads"])
    return (abs(a["loss"] - b["loss"]) / abs(b["loss"]), abs(a["grad_norm"] - b["grad_norm"]) / b["grad_norm"],
            max(e[0] for e in errs.values()), max(e[1] for e in errs.values()))


def compare(used, fresh, what):
    f = figures(used, fresh)
    print(f"{what}: loss rel {f[0]:.2e}, grad-norm rel {f[1]:.2e}, worst gradient max-norm {f[2]:.2e}, relative L2 {f[3]:.2e}")
    assert used["compact"] == fresh["compact"] and used["lists"] == fresh["lists"], what
    assert used["loss"] == pytest.approx(fresh["loss"], rel=2e-5), what
    assert used["grad_norm"] == pytest.approx(fresh["grad_norm"], rel=2e-4), what
    assert_grads_close(used["grads"], fresh["grads"], max_tol=2e-3, l2_tol=2e-3, what=what + " ")
    for name in [k for k in fresh if k.startswith(("targets", "outputs"))]:
        fs.rowwise(f"{what} {name}", used[name], fresh[name].double(), 1e-5)


def oracle_check(name, model, ema, batch, it, fresh, names):
    """The step the fresh engine ran, in float64 with the drop-path draws and the attention-dropout masks replayed; bounds of
    test_dropout_step_matches_oracle_with_replayed_masks."""
    h, cfg = HISTORY[name], history_cfg(name)
    x, mask, _ = batch
    p = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items() if k in names}
    e = {k: v.detach().float().cpu().clone() for k, v in ema.module.state_dict().items() if k in names}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(t) for k, t in p.items()}
    p1, p2 = vo.drop_path_scales(HISTORY_SEED, it, cfg, h["B"])
    assert any(t is not None and (t == 0).all() for t in p1 + p2), "the step has no empty list"
    drop = vo.DropState(path1=p1, path2=p2, attn=fs.replayed_masks(HISTORY_SEED, it, h["B"], cfg, "cpu"))
    ref = vo.train_step(p, e, m, v, cfg, vo.StepHParams(target_layers=tuple(h["target_layers"])), x, mask, 1, drop=drop)
    print(f"  [{name} it {it}] fresh engine loss {fresh['loss']:.6f} grad-norm {fresh['grad_norm']:.5f}, oracle {ref.loss:.6f} {ref.grad_norm:.5f}")
    assert fresh["loss"] == pytest.approx(ref.loss, rel=5e-3)
    assert fresh["grad_norm"] == pytest.approx(ref.grad_norm, rel=3e-2)
    assert_grads_close(fresh["grads"], ref.grads, what=f"[{name} it {it}: empty list vs oracle] ")
    return ref


@pytest.mark.parametrize("name", list(HISTORY))
def test_step_equals_the_same_step_on_a_fresh_engine(name):
    """One engine through the schedule `name` of tests/gpu_util.py::HISTORY (see there and tests/test_host_history.py for what each
    visits); every training step against a fresh engine, and for the tiny schedules a second fresh engine beside it: the
    fresh-against-fresh figures say how far two correct runs of a step are apart."""
    h, cfg = HISTORY[name], history_cfg(name)
    model, sd = native_model(cfg, two_stream=h["two_stream"])
    ema, opt = native_trainer(model)
    model.train()
    torch.manual_seed(HISTORY_SEED)
    assert torch.initial_seed() & 0xFFFFFFFF == HISTORY_SEED
    t0, compact = time.time(), []
    for i, (kind, arg, *rest) in enumerate(h["steps"]):
        batch = history_batch(name, i)
        if kind == "eval":                                   # the drop-in forward on the training engine, at another batch size
            engine = model._engine
            model.eval()
            out = model(batch[0].cuda(), batch[1].cuda())
            model.train()
            assert model._engine is engine and torch.isfinite(out).all() and out.shape[0] == int(batch[1].sum())
            continue
        opt_i = rest[0] if rest else {}
        lists = opt_i.get("lists", True)
        what = f"[{name} step {i} it {arg}{'' if lists else ' lists off'}]"
        print(f"\n{what} kept samples per (layer; draw) {history_kept_counts(name, arg)}")
        fm, fe, fo = fresh_copy(model, ema, lists)
        fresh = run_step(fm, fe, fo, batch, arg, h)
        if opt_i.get("oracle"):
            oracle_check(name, model, ema, batch, arg, fresh, set(sd))
        if cfg.embed_dim < 768:
            fm2, fe2, fo2 = fresh_copy(model, ema, lists)
            f = figures(run_step(fm2, fe2, fo2, batch, arg, h), fresh)
            print(f"{what} fresh against fresh: loss rel {f[0]:.2e}, grad-norm rel {f[1]:.2e}, worst gradient max-norm {f[2]:.2e}, relative L2 {f[3]:.2e}")
            del fm2, fe2, fo2
        del fm, fe, fo
        set_lists(model, lists)
        used = run_step(model, ema, opt, batch, arg, h)
        assert used["lists"] == lists
        compact.append(used["compact"])
        compare(used, fresh, what + " used against fresh")
    if name == "vitb32":
        masked = [s[2].get("masked", 0) for s in h["steps"] if s[0] == "step"]
        assert compact == [(n + 63) // 64 * 64 for n in masked], compact
    print(f"\n[{name}] {time.time() - t0:.1f} s")
