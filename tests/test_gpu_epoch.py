"""GPU: one multi-iteration train_one_epoch call -- what every real run does on every step and the one-iteration loaders of
tests/gpu_util.py::native_steps cannot reach.

The epoch (tests/gpu_util.py::EPOCH, its properties asserted by tests/test_host_epoch.py): nine iterations from global iteration 3, lr and
weight-decay tables whose neighbours differ by a factor >= 2, an EMA decay that anneals, freezes and is then skipped, batches whose losses
are >= 24 % apart.  A RecordingLoader snapshots the training state each time the prefetcher asks for a batch (between two steps, on the
compute stream), a RecordingWriter keeps what is published.

  A  update identity: the state after step j = clip + AdamW + EMA in float64 of the state before it and the DEVICE's own gradient of step j,
     with the scalars of table entry j -- isolates the device-resident schedule (stride, index, the "skip EMA" sign) and the fused
     AdamW + EMA path from gradient noise;
  B  the published loss / grad-norm of every iteration against the oracle's epoch;
  C  every published record belongs to its iteration (the four-slot ring, read one step late);
  D  a NaN / Inf pixel: SystemExit, the poisoned step and the good step behind it leave every buffer bit for bit, and so does a later epoch;
  E  n_rows_hint follows the batch handed out, not the one uploaded ahead (row totals that go down and up, a device-side mask between them);
  F  an n_rows_hint below the count: NaN loss, step skipped.  Before it ran, every masked-row path was read for its bounds: ln_fwd_kernel
     returns for row >= M before it reads the list; the GEMM row map, ln_bwd_kernel, ls_bwd_kernel use min(*count, M) with M = R; the target
     builder, smooth_l1 and gather_masked_rows use min(*count, B x P), the capacity of the list, of targets / outputs / dout (B x P rounded
     up to 64 rows) -- rows R .. count of `outputs` are stale but inside the buffer.  Nothing to fix there.

Found by tests/test_gpu_ops.py::test_adamw_skips_a_non_finite_norm, which belongs to this set: a sum of squares that is finite as a double
and infinite as the float adamw_kernel tests (1e40) skipped the step but reported the finite norm 1e20, so train_one_epoch's publish() would
have gone on with weights that never move again.  adamw_kernel now reports the float it tested.

Measured on an MI355X: see each test's docstring."""
import math
from types import SimpleNamespace

import pytest
import torch

from gpu_util import (EPOCH, Args, RecordingLoader, RecordingWriter, epoch_batch, epoch_cfg, epoch_run, epoch_table,
                      expected_update, grad_errors, native_model, native_steps, native_trainer, oracle_epoch, ragged_masks)
from oracle import vit_oracle as vo
from oracle.closed_form import closed_form_images

pytestmark = pytest.mark.gpu
STATE = ("params", "teacher", "m", "v", "params_bf16", "ema_bf16")


def fresh(cfg):
    model, _ = native_model(cfg)
    ema, opt = native_trainer(model, lr=Args.lr, wd=Args.weight_decay, decay=EPOCH["decay"])
    model.train()
    torch.manual_seed(0)
    return model, ema, opt


def run_epoch(cfg, batches, **kw):
    model, ema, opt = fresh(cfg)
    loader, writer = RecordingLoader(batches, model, ema, opt), RecordingWriter()
    stats = epoch_run(model, ema, opt, loader, writer, **kw)
    torch.cuda.synchronize()
    loader.snapshot()
    return SimpleNamespace(model=model, ema=ema, opt=opt, loader=loader, writer=writer, stats=stats, snaps=loader.snapshots)


def state_equal(a, b, keys=STATE):
    return {k: torch.equal(a[k], b[k]) for k in keys}


@pytest.fixture(scope="module")
def epoch():
    """The EPOCH run.  Step j: state before = snapshot j + 1, state after, raw gradients and loss words = snapshot j + 2."""
    n = EPOCH["n_iters"]
    r = run_epoch(epoch_cfg(), [epoch_batch(i) for i in range(n)])
    assert r.loader.requested == list(range(n)) and len(r.snaps) == n + 2
    assert "m" not in r.snaps[1] and "stats" not in r.snaps[1] and "stats" in r.snaps[2]        # the engine exists from the first step on
    return r


def test_epoch_schedules_update_identity(epoch):
    """After-state of every step against expected_update (pinned to torch.optim.AdamW by tests/test_host_epoch.py) of its before-state, the
    device's own raw gradient and the scalars of its table entry, Adam step j + 1.  Bounds: params and moments (relative to their own maximum)
    rtol 1e-5, atol 1e-6 (test_ema_adamw_sumsq_against_torch); teacher atol 1e-7 + 2e-7 max|p| (full_size_step_properties); teacher and its
    bf16 shadow bit-equal across the two skipped updates; both shadows = the arenas rounded to bf16 after every step.
    Measured, worst over the nine steps: params 6.0e-8 max abs (|p| <= 1.2), exp_avg 4.5e-8 and exp_avg_sq 3.7e-8 of their maximum, teacher
    1.2e-7 against a bound of 3.3e-7, 0 on the skipped updates."""
    E, table, snaps = EPOCH, epoch_table(), epoch.snaps
    n_decay = epoch.model._n_decay
    assert 0 < n_decay < epoch.model._arena.numel()
    worst = dict(params=0.0, m=0.0, v=0.0, teacher=0.0)
    regimes = set()
    for j, (lr, wd, d) in enumerate(table):
        b, a = snaps[j + 1], snaps[j + 2]
        zeros = torch.zeros_like(b["params"])
        P, M, V, T, norm = expected_update(b["params"], b.get("m", zeros), b.get("v", zeros), b["teacher"], a["grads"], lr, wd,
                                           None if d < 0 else d, j + 1, n_decay, E["max_norm"], E["betas"], E["eps"])
        got = {k: a[k].double().cpu() for k in ("params", "m", "v", "teacher")}
        tb = 1e-7 + 2e-7 * float(b["params"].abs().max())
        err = dict(params=float((got["params"] - P).abs().max()), m=float((got["m"] - M).abs().max() / M.abs().max()),
                   v=float((got["v"] - V).abs().max() / V.abs().max()), teacher=float((got["teacher"] - T).abs().max()))
        print(f"step {j} (it {E['start_steps'] + j}, lr {lr:.2e} wd {wd:.3f} decay {d:.6f}, grad norm {norm:.4f}): params max abs {err['params']:.2e}, "
              f"moments / max {err['m']:.2e} {err['v']:.2e}, teacher max abs {err['teacher']:.2e} (bound {tb:.2e})")
        worst = {k: max(worst[k], err[k]) for k in worst}
        what = f"step {j}"
        torch.testing.assert_close(got["params"], P, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} params: {m}")
        torch.testing.assert_close(got["m"] / M.abs().max(), M / M.abs().max(), rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} exp_avg: {m}")
        torch.testing.assert_close(got["v"] / V.abs().max(), V / V.abs().max(), rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} exp_avg_sq: {m}")
        assert err["teacher"] <= tb, (what, "teacher", err["teacher"], tb)
        assert not torch.equal(a["params"], b["params"]), what
        if d < 0:                        # it > start_lr_decay_at_step: no EMA update
            assert torch.equal(a["teacher"], b["teacher"]) and torch.equal(a["ema_bf16"], b["ema_bf16"]), f"{what}: a skipped EMA update moved the teacher"
            regimes.add("skipped")
        else:
            assert not torch.equal(a["teacher"], b["teacher"]), what
            regimes.add("frozen" if j > 0 and table[j - 1][2] == d else "annealed")
        assert torch.equal(a["params_bf16"], a["params"].to(torch.bfloat16)), f"{what}: params_bf16"
        assert torch.equal(a["ema_bf16"], a["teacher"].to(torch.bfloat16)), f"{what}: ema_bf16"
    assert regimes == {"annealed", "frozen", "skipped"}
    assert epoch.opt.step_count == E["n_iters"]
    print("worst over the epoch:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_epoch_trajectory_vs_oracle(epoch):
    """Published loss and grad-norm of every iteration against the oracle's epoch; bounds of test_train_steps_vs_golden: loss rel 5e-3 at the
    first step and 2e-2 afterwards, grad-norm rel 3e-2.  Measured: loss 1.6e-4 at the first step, <= 2.5e-4 afterwards; grad-norm <= 1.3e-3."""
    loss, gnorm = oracle_epoch()
    rec = epoch.writer.records
    assert len(rec) == len(loss)
    figs = [(abs(r["loss"] - l) / l, abs(r["grad_norm"] - g) / g) for r, l, g in zip(rec, loss, gnorm)]
    print("loss rel", [f"{f[0]:.2e}" for f in figs], "grad-norm rel", [f"{f[1]:.2e}" for f in figs])
    for i, (r, l, g) in enumerate(zip(rec, loss, gnorm)):
        assert r["loss"] == pytest.approx(l, rel=5e-3 if i == 0 else 2e-2), i
        assert r["grad_norm"] == pytest.approx(g, rel=3e-2), i


def test_epoch_metrics_belong_to_their_iteration(epoch):
    """Nine records; record i carries bit for bit the loss the device held after step i, the norm of the gradient arena of step i (rel 1e-4,
    the bound of full_size_step_properties; measured 4.2e-8), and the lr / weight decay / EMA decay of global iteration 3 + i."""
    E, rec, snaps = EPOCH, epoch.writer.records, epoch.snaps
    assert len(rec) == E["n_iters"]
    table = epoch_table()
    cur, worst = None, 0.0
    for i, r in enumerate(rec):
        it = E["start_steps"] + i
        stats = snaps[i + 2]["stats"].cpu()
        assert r["loss"] == float(stats[0]) and r["grad_norm"] == float(stats[1]), (i, r, stats)
        gn = math.sqrt(float((snaps[i + 2]["grads"].double() ** 2).sum()))
        worst = max(worst, abs(r["grad_norm"] - gn) / gn)
        assert r["grad_norm"] == pytest.approx(gn, rel=1e-4), i
        if it < E["ema_start_at"]:
            cur = E["decay_init"] + it * (E["decay"] - E["decay_init"]) / E["ema_start_at"]
        if it > E["start_lr_decay_at_step"]:
            cur = 0
        assert (r["lr"], r["min_lr"], r["weight_decay"], r["cur_decay"]) == (E["lr"][it], E["lr"][it], E["wd"][it], cur), (i, r)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()  # noqa: E731
        assert (f32(r["lr"]), f32(r["weight_decay"])) == table[i][:2] and (table[i][2] == -1.0 if cur == 0 else f32(cur) == table[i][2])
    losses = [r["loss"] for r in rec]
    assert len(set(losses)) == len(losses)
    assert epoch.stats["loss"] == pytest.approx(sum(losses) / len(losses), rel=1e-12)
    assert epoch.stats["grad_norm"] == pytest.approx(sum(r["grad_norm"] for r in rec) / len(rec), rel=1e-12)
    print(f"published grad-norm against the float64 norm of the gradient arena: worst rel {worst:.2e}")


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_epoch_stops_on_a_non_finite_batch(kind):
    """Six batches, one pixel of one sample of batch 2 NaN / +Inf.  train_one_epoch exits while publishing iteration 2, after iteration 3
    has been enqueued: both steps must leave params, teacher, moments and shadows as the two good steps left them, and a later epoch on the
    same engine runs (finite loss) and still moves nothing (include/uvit.h: "... and so does every later step of that engine")."""
    batches = [epoch_batch(i) for i in range(6)]
    batches[2][0][1, 2, 17, 30] = float(kind)
    model, ema, opt = fresh(epoch_cfg())
    loader, writer = RecordingLoader(batches, model, ema, opt), RecordingWriter()
    with pytest.raises(SystemExit):
        epoch_run(model, ema, opt, loader, writer)
    torch.cuda.synchronize()
    assert loader.requested == [0, 1, 2, 3, 4]
    assert len(writer.records) == 2 and all(math.isfinite(r["loss"]) for r in writer.records)
    good = loader.snapshots[3]                   # taken when batch 3 was requested: after the steps on batches 0 and 1
    assert not torch.equal(good["params"], loader.snapshots[0]["params"]) and not torch.equal(good["teacher"], loader.snapshots[0]["teacher"])
    assert float(good["m"].abs().max()) > 0 and float(good["v"].abs().max()) > 0
    now = loader.snapshot()
    assert math.isfinite(float(now["stats"][0]))              # the last step enqueued is the good one behind the poisoned one
    eq = state_equal(now, good)
    assert all(eq.values()), f"a step after a non-finite loss moved {[k for k, v in eq.items() if not v]}"
    st = native_steps(model, ema, opt, [tuple(t.cuda() for t in epoch_batch(5))], EPOCH["target_layers"], start=20)[0]
    torch.cuda.synchronize()
    assert math.isfinite(st["loss"]) and 0 < st["loss"] < 10
    eq = state_equal(loader.snapshot(), good)
    assert all(eq.values()), f"a later epoch on the poisoned engine moved {[k for k, v in eq.items() if not v]}"


ROWS_CFG = dict(img_size=224, embed_dim=128, depth=2, num_heads=2)       # 4 x 196 = 784 patch rows, 788 token rows: 512 <= R < M engages
ROWS_B = 4
ROWS_TOTALS = [600, 530, 560, 700, 515]                                   # position 2: the mask is already on the device (no host count)


def rows_batches(dense):
    out = []
    for i, total in enumerate(ROWS_TOTALS):
        x, m = closed_form_images(f"epoch_rows/{i}", ROWS_B, 224), ragged_masks(ROWS_B, 196, total, 300 + i)
        out.append((x, m.cuda() if dense or i == 2 else m))
    return out


def layout_views(model, arena):
    return {n: arena[o:o + k] for n, o, k, _, dk in model._layout if dk != 2}


def test_epoch_row_hints_follow_their_batch():
    """Five iterations with host-side masks of 600, 530, (device-side 560), 700, 515 masked patches: the last block runs on 640, 576, all, 704,
    576 rows.  A hint taken from the batch uploaded ahead would be below the count at 600 -> 530 and 700 -> 515 ... and the step would be
    skipped with a NaN loss (SystemExit).  Every step against the same epoch with every mask on the device (dense last block); bounds of
    "same step, other row plan" (tests/test_gpu_history.py): loss rel 2e-5, grad-norm rel 2e-4, every gradient tensor max-norm 2e-3 and
    relative L2 2e-3.  The gradient bounds hold the first step only: from the second step on the two runs no longer start from the same
    weights -- the fp32 atomics of step 0 leave 6e3 of 1.2e6 weights one ulp (<= 6.6e-8) apart, which moves some of their bf16 images by a
    bf16 ulp, and AdamW turns near-zero gradients of either sign into steps of +- lr (5e5 weights up to 1.5e-4 apart before step 4) -- so
    their gradients are those of two slightly different models, and later steps are held to the loss and grad-norm bounds.
    Measured (two pairs of runs): step 0 loss 3.2e-7, grad-norm 0, gradients 3.3e-7 max-norm / 2.4e-7 relative L2; steps 1 - 4 loss
    <= 5.3e-6, grad-norm <= 6.4e-5, gradients up to 3.8e-3 max-norm / 5.1e-3 relative L2 (rel_pos_bias table), printed with the number of
    weights that differ before each step."""
    cfg = vo.VitConfig(init_values=0.1, **ROWS_CFG)
    n = len(ROWS_TOTALS)
    runs = {dense: run_epoch(cfg, rows_batches(dense)) for dense in (False, True)}
    compact = {d: [r.snaps[j + 2]["compact"] for j in range(n)] for d, r in runs.items()}
    assert compact[True] == [0] * n and compact[False] == [640, 576, 0, 704, 576], compact
    a, b = runs[False], runs[True]
    assert len(a.writer.records) == n and len(b.writer.records) == n
    bad = []
    for j in range(n):
        ra, rb = a.writer.records[j], b.writer.records[j]
        errs = grad_errors(layout_views(a.model, a.snaps[j + 2]["grads"]), {k: v.cpu() for k, v in layout_views(b.model, b.snaps[j + 2]["grads"]).items()})
        f = (abs(ra["loss"] - rb["loss"]) / rb["loss"], abs(ra["grad_norm"] - rb["grad_norm"]) / rb["grad_norm"],
             max(e[0] for e in errs.values()), max(e[1] for e in errs.values()))
        dp = (a.snaps[j + 1]["params"] - b.snaps[j + 1]["params"]).abs()
        wt = max(errs, key=lambda k: errs[k][1])
        print(f"step {j} ({ROWS_TOTALS[j]} masked, {compact[False][j]} rows): loss {ra['loss']:.6f} rel {f[0]:.2e}, grad-norm rel {f[1]:.2e}, "
              f"worst gradient max-norm {f[2]:.2e}, relative L2 {f[3]:.2e} ({wt}); weights before the step differ in {int((dp > 0).sum())} "
              f"elements, at most {float(dp.max()):.2e}")
        if f[0] > 2e-5 or f[1] > 2e-4 or (j == 0 and (f[2] > 2e-3 or f[3] > 2e-3)):
            bad.append((j, f))
    assert not bad, bad


def test_row_hint_below_the_count_skips_the_step():
    """600 masked patches, n_rows_hint = 520: the last block runs on 576 rows, rows_guard_kernel makes the loss NaN and nothing moves -- nor
    in a following step whose hint is right (the engine stays poisoned).  The bounds of every masked-row path: this file's docstring."""
    import ctypes as C
    from uncertainty_vit_amd.engine_for_cyclical import make_step_params, native_step
    from uncertainty_vit_amd.native import check, cur_stream, lib
    cfg = vo.VitConfig(init_values=0.1, **ROWS_CFG)
    model, ema, opt = fresh(cfg)
    x, mask = rows_batches(True)[0]
    x = x.cuda()
    assert int(mask.sum()) == 600
    opt._ensure_state()
    engine = model.engine(ROWS_B, teacher=ema.module, adam_m=opt.exp_avg, adam_v=opt.exp_avg_sq)
    loader = RecordingLoader([], model, ema, opt)
    before = loader.snapshot()

    def step(hint):
        hp = make_step_params([1], opt, 3.0, 2.0, False, -1, True, True, 0.9998, True, 1, 0, opt.step_count, depth=cfg.depth, n_rows_hint=hint)
        native_step(engine, None, x, mask.reshape(ROWS_B, -1).contiguous(), hp)
        opt.step_count += 1
        out = (C.c_float * 2)()
        check(lib().uvit_engine_read_stats(engine.h, out, cur_stream()), "read_stats")
        return out[0], out[1], engine.compact_rows()

    loss, gnorm, rows = step(520)
    assert rows == 576 and math.isnan(loss) and not math.isfinite(gnorm), (loss, gnorm, rows)
    eq = state_equal(loader.snapshot(), before)
    assert all(eq.values()), f"the step with a hint below the count moved {[k for k, v in eq.items() if not v]}"
    loss, gnorm, rows = step(600)
    assert rows == 640 and math.isfinite(loss) and 0 < loss < 10, (loss, gnorm, rows)
    eq = state_equal(loader.snapshot(), before)
    assert all(eq.values()), f"a step after the skipped one moved {[k for k, v in eq.items() if not v]}"
