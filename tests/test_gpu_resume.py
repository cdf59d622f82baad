"""GPU: state that reaches the engine from outside it -- a checkpoint file, and edits of the weights under a live engine.

The epoch of tests/gpu_util.py::EPOCH is split across a file: run A does iterations 0..3 (global 3..6, the annealed EMA decays) and
utils.save_model writes it; run B starts from new objects that hold other weights (another gamma, every arena element + 0.01),
utils.auto_load_model fills them, and iterations 4..8 run with start_steps = 7 (the last two skip the EMA update).  Run C is the same
nine iterations on a third set of objects with no file between them.

What an uninterrupted run is.  train_one_epoch starts every call from `cur_decay = decay`, as the reference does
(engine_for_cyclical.py:44): the annealed value survives past ema_start_at only until the call returns.  So B's iterations at global
7..9 use the final decay 0.9998, where ONE nine-iteration call keeps 0.9984 (gpu_util.oracle_epoch, epoch_table()[4:7]).  That is the
reference's behaviour at every epoch boundary, with or without a file, so C is two calls (4 + 5 iterations), which is what run_cyclical's
epoch loop does; the update identity takes lr and weight decay from epoch_table() at the global index and the EMA decay from that rule.
Against the single call (run S) B still has to agree where the two coincide: loss and grad-norm of iteration 4, whose teacher no changed
decay has touched yet.  Later iterations of S are printed, not asserted (measured: loss up to 2.7e-4, grad-norm up to 8.1e-4 away, the final teacher 2.2e-5).

The arena has alignment pads (8 floats in this model) that belong to no state-dict entry: a file does not carry them, B keeps its 0.01
there, and they are inert (zero gradient, zero moments).  "Bit for bit" below is over the entries of model._layout.

C against C' (same code, same inputs, other objects), measured on an MI355X over the 15 pairs of six runs, largest figure of each kind
(CC below): loss 1.55e-7 relative (one or two float32 ulps of the loss; most pairs 7.75e-8), grad-norm 0, final student and teacher
arenas 0 -- at this size the gradients come out bit-identical from run to run and only the loss sum is reordered.  The bound for B
against C is four times that, and at least one float32 ulp of the arena's largest magnitude (1.18: 2^-23; 2^-23 of a relative figure):
loss 6.2e-7, grad-norm 1.2e-7, arenas 1.2e-7 (bounds() below).  Measured B against C: loss 7.7e-8, everything else 0.

Weight edits under a used engine: tests/test_host_resume.py has the bookkeeping; here the step that follows an edit is compared with the
same step on a fresh trainer built from the edited weights (bounds of tests/test_gpu_history.py::compare).  Found by the teacher cases
and fixed in VisionTransformerForCyclicalTraining.engine(): the student's engine owns the teacher's bf16 copy but looked only at the
student's stale flag, so ModelEmaV2.set / .update / a load_state_dict on the teacher under a live engine left the old teacher in the
next step's targets: ema_bf16 differed from the teacher arena before the step in all eight teacher cases, target rows up to 2.5e-2
(set, load) and 1.2e-2 (update) of their norm from the fresh trainer's against a bound of 1e-5; with the EMA update skipped, in every
later step too.  The old and the new teacher's targets are 0.31 .. 0.74 apart on every row.

Measured on an MI355X: the file takes 5 s (the split fixture 0.5 s, no test above 0.3 s)."""
import copy
import math
import time
from types import SimpleNamespace

import pytest
import torch

import test_gpu_fullsize as fs
from gpu_util import (EPOCH, Args, RecordingLoader, RecordingWriter, assert_grads_close, epoch_batch, epoch_cfg, epoch_run,
                      epoch_table, expected_update, native_model, native_trainer, oracle_epoch)
from oracle import vit_oracle as vo
from oracle.closed_form import closed_form_state
from test_gpu_history import compare

pytestmark = pytest.mark.gpu
SPLIT = 4                          # run A: iterations 0..3, run B: 4..8
OTHER_GAMMA = 0.3
# largest C-against-C' figures measured (loss rel, grad-norm rel over the nine iterations; final arenas max abs) and the bounds from them
CC = dict(loss=1.55e-7, grad_norm=0.0, params=0.0, teacher=0.0)


def bounds(arena_max):
    """Four times the measured figure; at least one float32 ulp: 2^-23 of a relative figure, the ulp of the arena's largest magnitude."""
    ulp = dict(loss=2.0 ** -23, grad_norm=2.0 ** -23, params=2.0 ** (math.floor(math.log2(arena_max)) - 23))
    ulp["teacher"] = ulp["params"]
    return {k: max(4 * v, ulp[k]) for k, v in CC.items()}


def trainer(gamma=None, perturb=False):
    model, _ = native_model(epoch_cfg(), gamma=gamma)
    if perturb:
        with torch.no_grad():
            model._arena.add_(0.01)
        model.mark_weights_changed()
    ema, opt = native_trainer(model, lr=Args.lr, wd=Args.weight_decay, decay=EPOCH["decay"])
    model.train()
    torch.manual_seed(0)
    return model, ema, opt


def run(model, ema, opt, iters, **kw):
    """One epoch_run over iterations `iters` of the epoch, start_steps = 3 + iters[0]; the snapshots end with the state after the last step."""
    loader, writer = RecordingLoader([epoch_batch(i) for i in iters], model, ema, opt), RecordingWriter()
    stats = epoch_run(model, ema, opt, loader, writer, start_steps=EPOCH["start_steps"] + iters[0], **kw)
    torch.cuda.synchronize()
    loader.snapshot()
    assert loader.requested == list(range(len(iters))) and len(writer.records) == len(iters)
    return SimpleNamespace(snaps=loader.snapshots, records=writer.records, stats=stats)


def live_mask(model):
    live = torch.zeros(model._arena.numel(), dtype=torch.bool, device=model._arena.device)
    for _, off, numel, _, _ in model._layout:
        live[off:off + numel] = True
    return live


def arenas(model, ema, opt):
    return {"params": model._arena.clone(), "teacher": ema.module._arena.clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone()}


def load_args(out, **kw):
    return SimpleNamespace(output_dir=str(out), auto_resume=True, resume="", start_epoch=0, **kw)


def run_a(out):
    from uncertainty_vit_amd import utils
    model, ema, opt = trainer()
    a = run(model, ema, opt, range(SPLIT))
    utils.save_model(SimpleNamespace(output_dir=str(out)), 0, model, model, opt, utils.NativeScalerWithGradNormCount(), model_ema=ema)
    a.model, a.ema, a.opt, a.final = model, ema, opt, arenas(model, ema, opt)
    model._engine.sync_shadows(1)
    a.params_bf16_t = model._engine.params_bf16_t.clone()
    return a


def resumed(out, **flags):
    """New objects with other contents, auto_load_model, the engine train_one_epoch will ask for; nothing has run yet."""
    from uncertainty_vit_amd import utils
    model, ema, opt = trainer(gamma=OTHER_GAMMA, perturb=True)
    b = SimpleNamespace(model=model, ema=ema, opt=opt, built={"params": model._arena.clone(), "teacher": ema.module._arena.clone()})
    b.args = load_args(out, **flags)
    utils.auto_load_model(b.args, model, model, opt, utils.NativeScalerWithGradNormCount(), model_ema=ema)
    b.loaded, b.step_count = arenas(model, ema, opt), opt.step_count
    b.engine = model.engine(EPOCH["B"], teacher=ema.module, adam_m=opt.exp_avg, adam_v=opt.exp_avg_sq)
    e = b.engine
    b.shadows = {"params_bf16": e.params_bf16.clone(), "ema_bf16": e.ema_bf16.clone(), "params_bf16_t": e.params_bf16_t.clone()}
    return b


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """A, the file, B.  B's step j (iteration SPLIT + j): state before = snapshot j + 1, after, raw gradients and loss words = snapshot j + 2."""
    t0 = time.time()
    out = tmp_path_factory.mktemp("resume")
    a = run_a(out)
    b = resumed(out, model_ema=True)
    r = run(b.model, b.ema, b.opt, range(SPLIT, EPOCH["n_iters"]))
    assert b.model._engine is b.engine, "train_one_epoch built another engine"
    b.snaps, b.records = r.snaps, r.records
    print(f"split fixture: {time.time() - t0:.1f} s")
    return SimpleNamespace(a=a, b=b, out=out)


def test_loaded_state_is_the_saved_state(split):
    """After auto_load_model and before any step: student, teacher and both moments are run A's last state bit for bit (and are not what B
    was built with), step_count = 4, start_epoch = saved epoch + 1.  After B's engine exists: both bf16 shadows are the arenas rounded to
    bf16, and the transposed weights are bit for bit those of A's engine (pure data movement)."""
    a, b = split.a, split.b
    live = live_mask(b.model)
    assert 0 < int((~live).sum()) < 64
    for k in ("params", "teacher", "m", "v"):
        assert torch.equal(b.loaded[k][live], a.final[k][live]), k
    assert not torch.equal(b.built["params"][live], a.final["params"][live]) and not torch.equal(b.built["teacher"][live], a.final["teacher"][live])
    assert float(a.final["m"].abs().max()) > 0 and float(a.final["v"].abs().max()) > 0
    assert not torch.equal(a.final["teacher"], a.final["params"])
    assert b.step_count == SPLIT == a.opt.step_count and b.args.start_epoch == 1
    assert torch.equal(b.shadows["params_bf16"], b.loaded["params"].to(torch.bfloat16))
    assert torch.equal(b.shadows["ema_bf16"], b.loaded["teacher"].to(torch.bfloat16))
    assert float(b.shadows["params_bf16_t"].float().abs().max()) > 0
    assert torch.equal(b.shadows["params_bf16_t"], a.params_bf16_t)
    assert b.snaps[0]["stats"] is not None and torch.equal(b.snaps[1]["params"], b.loaded["params"])


def b_table():
    """(lr, weight decay, EMA decay or -1) of B's iterations: lr and weight decay of epoch_table() at the global index; the EMA decay by the
    rule of engine_for_cyclical.py:44,55-56,182-185 for a call that starts at ema_start_at: the final decay, then skipped."""
    import numpy as np
    E, full = EPOCH, epoch_table()
    rows = []
    for j in range(SPLIT, E["n_iters"]):
        it = E["start_steps"] + j
        assert it >= E["ema_start_at"]
        rows.append((full[j][0], full[j][1], -1.0 if it > E["start_lr_decay_at_step"] else float(np.float32(E["decay"]))))
        assert (rows[-1][2] < 0) == (full[j][2] < 0)
    return rows


def test_resumed_iterations_update_identity(split):
    """tests/test_gpu_epoch.py::test_epoch_schedules_update_identity on run B, with its bounds: params and moments (relative to their own
    maximum) rtol 1e-5, atol 1e-6; teacher atol 1e-7 + 2e-7 max|p|; teacher and its bf16 shadow bit-equal across the two skipped updates;
    both shadows = the arenas rounded to bf16 after every step.  Adam step 5 + j: pins the restored step count (bias correction), the
    schedule index (neighbouring lr / weight-decay entries are a factor >= 2 apart) and the restored moments."""
    E, b = EPOCH, split.b
    n_decay = b.model._n_decay
    table = b_table()
    assert [d < 0 for _, _, d in table] == [False, False, False, True, True]
    worst = dict(params=0.0, m=0.0, v=0.0, teacher=0.0)
    for j, (lr, wd, d) in enumerate(table):
        s0, s1 = b.snaps[j + 1], b.snaps[j + 2]
        P, M, V, T, norm = expected_update(s0["params"], s0["m"], s0["v"], s0["teacher"], s1["grads"], lr, wd, None if d < 0 else d,
                                           SPLIT + 1 + j, n_decay, E["max_norm"], E["betas"], E["eps"])
        got = {k: s1[k].double().cpu() for k in ("params", "m", "v", "teacher")}
        tb = 1e-7 + 2e-7 * float(s0["params"].abs().max())
        err = dict(params=float((got["params"] - P).abs().max()), m=float((got["m"] - M).abs().max() / M.abs().max()),
                   v=float((got["v"] - V).abs().max() / V.abs().max()), teacher=float((got["teacher"] - T).abs().max()))
        print(f"B step {j} (it {E['start_steps'] + SPLIT + j}, Adam step {SPLIT + 1 + j}, lr {lr:.2e} wd {wd:.3f} decay {d:.6f}, grad norm {norm:.4f}): "
              f"params max abs {err['params']:.2e}, moments / max {err['m']:.2e} {err['v']:.2e}, teacher max abs {err['teacher']:.2e} (bound {tb:.2e})")
        worst = {k: max(worst[k], err[k]) for k in worst}
        what = f"B step {j}"
        torch.testing.assert_close(got["params"], P, rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} params: {m}")
        torch.testing.assert_close(got["m"] / M.abs().max(), M / M.abs().max(), rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} exp_avg: {m}")
        torch.testing.assert_close(got["v"] / V.abs().max(), V / V.abs().max(), rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} exp_avg_sq: {m}")
        assert err["teacher"] <= tb, (what, "teacher", err["teacher"], tb)
        assert not torch.equal(s1["params"], s0["params"]), what
        if d < 0:
            assert torch.equal(s1["teacher"], s0["teacher"]) and torch.equal(s1["ema_bf16"], s0["ema_bf16"]), f"{what}: a skipped EMA update moved the teacher"
        else:
            assert not torch.equal(s1["teacher"], s0["teacher"]), what
        assert torch.equal(s1["params_bf16"], s1["params"].to(torch.bfloat16)), f"{what}: params_bf16"
        assert torch.equal(s1["ema_bf16"], s1["teacher"].to(torch.bfloat16)), f"{what}: ema_bf16"
    assert b.opt.step_count == E["n_iters"]
    print("worst over run B:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_resumed_trajectory_vs_oracle(split):
    """B's published loss and grad-norm against iterations 4..8 of the oracle's uninterrupted epoch, which never saw a file; bounds of
    test_epoch_trajectory_vs_oracle for iterations past the first: loss rel 2e-2, grad-norm rel 3e-2.  (The oracle's epoch keeps the
    annealed EMA decay at global 7..9 where B has the final one: 1.4e-3 of the distance between teacher and student, far inside.)"""
    loss, gnorm = oracle_epoch()
    rec = split.b.records
    ref = list(zip(loss, gnorm))[SPLIT:EPOCH["n_iters"]]
    assert len(rec) == len(ref) == 5
    print("loss rel", [f"{abs(r['loss'] - l) / l:.2e}" for r, (l, _) in zip(rec, ref)],
          "grad-norm rel", [f"{abs(r['grad_norm'] - g) / g:.2e}" for r, (_, g) in zip(rec, ref)])
    for i, (r, (l, g)) in enumerate(zip(rec, ref)):
        assert r["loss"] == pytest.approx(l, rel=2e-2), i
        assert r["grad_norm"] == pytest.approx(g, rel=3e-2), i


def two_calls():
    """The nine iterations with no file between them: one set of objects, an epoch boundary where the file was."""
    model, ema, opt = trainer()
    first = run(model, ema, opt, range(SPLIT))
    second = run(model, ema, opt, range(SPLIT, EPOCH["n_iters"]))
    return SimpleNamespace(records=first.records + second.records, final=arenas(model, ema, opt), model=model)


def distance(x, y, live):
    """Largest loss rel and grad-norm rel over the iterations, max abs difference of the final student and teacher arenas."""
    n = min(len(x.records), len(y.records))
    rx, ry = x.records[-n:], y.records[-n:]
    return dict(loss=max(abs(p["loss"] - q["loss"]) / q["loss"] for p, q in zip(rx, ry)),
                grad_norm=max(abs(p["grad_norm"] - q["grad_norm"]) / q["grad_norm"] for p, q in zip(rx, ry)),
                params=float((x.final["params"][live] - y.final["params"][live]).abs().max()),
                teacher=float((x.final["teacher"][live] - y.final["teacher"][live]).abs().max()))


def test_resumed_run_equals_the_uninterrupted_run(split):
    """A + file + B against C (this file's docstring): per-iteration loss and grad-norm of all nine iterations, final student and teacher
    arenas, under bounds().  C against C' is measured again and printed beside the recorded CC.  Run S, the nine iterations in ONE call:
    iteration 4 under the same bounds, the rest printed."""
    a, b = split.a, split.b
    live = live_mask(b.model)
    resumed_run = SimpleNamespace(records=a.records + b.records, final=arenas(b.model, b.ema, b.opt))
    c, c2 = two_calls(), two_calls()
    BOUNDS = bounds(float(c.final["params"].abs().max()))
    cc = distance(c, c2, live)
    bc = distance(resumed_run, c, live)
    print("C against C':", {k: f"{v:.2e}" for k, v in cc.items()}, "recorded:", CC)
    print("B against C :", {k: f"{v:.2e}" for k, v in bc.items()}, "bounds:", {k: f"{v:.2e}" for k, v in BOUNDS.items()})
    model, ema, opt = trainer()
    s = run(model, ema, opt, range(EPOCH["n_iters"]))
    rs = [(abs(p["loss"] - q["loss"]) / q["loss"], abs(p["grad_norm"] - q["grad_norm"]) / q["grad_norm"]) for p, q in zip(b.records, s.records[SPLIT:])]
    print("B against the single call, iterations 4..8: loss rel", [f"{f[0]:.2e}" for f in rs], "grad-norm rel", [f"{f[1]:.2e}" for f in rs],
          "final teacher max abs", f"{float((resumed_run.final['teacher'][live] - ema.module._arena[live]).abs().max()):.2e}")
    assert not [k for k in bc if bc[k] > BOUNDS[k]], (bc, BOUNDS)
    assert rs[0][0] <= BOUNDS["loss"] and rs[0][1] <= BOUNDS["grad_norm"], rs[0]


def state_dicts(model, arena_by_name):
    lay = {n: (o, k, shape) for n, o, k, shape, _ in model._layout}
    return [{n: a[o:o + k].view(shape).float().cpu().clone() for n, (o, k, shape) in lay.items()} for a in arena_by_name]


def test_resume_without_the_teacher_flag_restarts_the_teacher(split):
    """args without model_ema (the reference's command line has no such flag; utils.auto_load_model's docstring): the
    teacher stays bit for bit what ModelEmaV2(model) copied when B was built -- not the file's model_ema -- while student, moments and
    step count come back.  One resumed step (global iteration 7, Adam step 5) against vo.train_step given that teacher; bounds of
    test_train_steps_vs_golden's first step: loss rel 5e-3, grad-norm rel 3e-2, gradients max-norm 5e-2 and relative L2 2e-2."""
    E, a = EPOCH, split.a
    b = resumed(split.out)
    live = live_mask(b.model)
    assert torch.equal(b.loaded["teacher"], b.built["teacher"]) and not torch.equal(b.loaded["teacher"][live], a.final["teacher"][live])
    for k in ("params", "m", "v"):
        assert torch.equal(b.loaded[k][live], a.final[k][live]), k
    assert b.step_count == SPLIT and b.args.start_epoch == 1
    assert torch.equal(b.shadows["ema_bf16"], b.built["teacher"].to(torch.bfloat16))
    p, e, m, v = state_dicts(b.model, [b.loaded[k] for k in ("params", "teacher", "m", "v")])
    r = run(b.model, b.ema, b.opt, [SPLIT])
    it = E["start_steps"] + SPLIT
    x, mask = epoch_batch(SPLIT)
    hp = vo.StepHParams(target_layers=tuple(E["target_layers"]), clip_grad=E["max_norm"], betas=E["betas"], eps=E["eps"])
    ref = vo.train_step(p, e, m, v, epoch_cfg(), hp, x, mask, SPLIT + 1, lr=E["lr"][it], wd=E["wd"][it], decay=E["decay"])
    rec = r.records[0]
    print(f"restarted teacher, it {it}: loss {rec['loss']:.6f} (oracle {ref.loss:.6f}), grad-norm {rec['grad_norm']:.5f} (oracle {ref.grad_norm:.5f})")
    assert rec["loss"] == pytest.approx(ref.loss, rel=5e-3)
    assert rec["grad_norm"] == pytest.approx(ref.grad_norm, rel=3e-2)
    assert_grads_close({n: q.grad.clone() for n, q in b.model.named_parameters()}, ref.grads, what="[restarted teacher] ")


# ---- edits of the weights under a used engine ----
def other_state():
    cfg = epoch_cfg()
    sd = closed_form_state(vo.param_shapes(cfg), gamma=OTHER_GAMMA)
    sd["patch_embed.proj.weight"] = sd["patch_embed.proj.weight"] + 0.05
    return sd


def student_inplace(model, ema, donor, x, mask):
    with torch.no_grad():
        model._arena.mul_(1.01)
    model.mark_weights_changed()


def teacher_set(model, ema, donor, x, mask):
    ema.set(donor)


def teacher_update(model, ema, donor, x, mask):
    decay, ema.decay = ema.decay, 0.5
    ema.update(donor)
    ema.decay = decay


def teacher_load(model, ema, donor, x, mask):
    ema.module.load_state_dict(other_state(), strict=False)


def teacher_load_after_teacher_forward(model, ema, donor, x, mask):
    """The teacher module gets an engine of its own, and that engine consumes the teacher's own stale state after the load."""
    teacher = ema.module
    assert not teacher.training
    before = teacher(x, mask)
    teacher_load(model, ema, donor, x, mask)
    after = teacher(x, mask)
    assert teacher._engine is not None and teacher._engine is not model._engine and not teacher._shadows_stale
    assert not torch.allclose(before, after, rtol=1e-2, atol=1e-2)


# set / update take the weights of a donor model (other_state) instead of the student's: three steps move the student too little for a
# stale teacher to be unmistakable, and an edit of the student itself would refresh both shadows on its own
EDITS = {"student_inplace": student_inplace, "student_load": lambda model, *a: model.load_state_dict(other_state(), strict=False),
         "teacher_set": teacher_set, "teacher_update": teacher_update, "teacher_load": teacher_load,
         "teacher_load_after_teacher_forward": teacher_load_after_teacher_forward}
CASES = [(e, skip) for e in EDITS for skip in ((False, True) if e.startswith("teacher") else (False,))]


def one_step(model, ema, opt, i, **kw):
    """Iteration i in a train_one_epoch call of its own; what tests/test_gpu_history.py::compare reads."""
    r = run(model, ema, opt, [i], **kw)
    e, n = model._engine, int(epoch_batch(i)[1].sum())
    out = {"loss": r.records[0]["loss"], "grad_norm": r.records[0]["grad_norm"], "compact": e.compact_rows(), "lists": e.drop_path_rows,
           "grads": {k: q.grad.detach().float().cpu().clone() for k, q in model.named_parameters() if q.grad is not None}}
    for name in ("targets", "outputs"):
        out[name] = e.ws_tensor(name, 0, (n, model.embed_dim)).clone()
    return out


def fresh_of(model, ema, opt):
    """tests/test_gpu_history.py::fresh_copy with the moments and the step count as well: new objects and (at their first step) a new engine."""
    m = copy.deepcopy(model)
    e, o = native_trainer(m, lr=Args.lr, wd=Args.weight_decay, decay=EPOCH["decay"])
    e.module._arena.copy_(ema.module._arena)
    e.module.mark_weights_changed()
    o._ensure_state()
    o.exp_avg.copy_(opt.exp_avg)
    o.exp_avg_sq.copy_(opt.exp_avg_sq)
    o.step_count = opt.step_count
    m.train()
    return m, e, o


def row_distance(a, b):
    rel = (a.double() - b.double()).norm(dim=1) / b.double().norm(dim=1)
    return float(rel.min()), float(rel.max())


@pytest.mark.parametrize("edit,skip", CASES, ids=[f"{e}-{'ema_skipped' if s else 'ema_on'}" for e, s in CASES])
def test_weight_edits_reach_a_used_engine(edit, skip):
    """One trainer runs iterations 0..2, its weights are edited, iteration 3 runs (with `skip`: the EMA update is skipped from iteration 3
    on -- start_lr_decay_at_step = 5 -- and iteration 4 runs too).  After engine() and before the step both bf16 shadows are their arenas
    rounded to bf16 on the engine that ran the three iterations; the step is test_gpu_history.compare's distance from the same step on a
    fresh trainer built from the edited weights (loss rel 2e-5, grad-norm rel 2e-4, gradients 2e-3, target and output rows 1e-5); the
    second step's targets likewise.  Teacher edits: a fresh trainer with the OLD teacher has targets more than 1e-2 (relative L2) away on
    every row, so a stale teacher cannot pass."""
    kw = dict(start_lr_decay_at_step=5) if skip else {}
    model, ema, opt = trainer()
    run(model, ema, opt, range(3), **kw)
    engine = model._engine
    assert opt.step_count == 3 and engine is not None
    donor, _ = native_model(epoch_cfg(), gamma=OTHER_GAMMA)
    donor.load_state_dict(other_state(), strict=False)
    x, mask = (t.cuda() for t in epoch_batch(3))
    what = f"[{edit}{', EMA skipped' if skip else ''}]"
    old = None
    if edit.startswith("teacher"):
        old = one_step(*fresh_of(model, ema, opt), 3, **kw)
    EDITS[edit](model, ema, donor, x, mask)
    fm, fe, fo = fresh_of(model, ema, opt)
    fresh = one_step(fm, fe, fo, 3, **kw)
    if old is not None:
        lo, hi = row_distance(old["targets"], fresh["targets"])
        print(f"{what} targets of the old against the new teacher: every row between {lo:.2e} and {hi:.2e} of its norm apart")
        assert lo > 1e-2, f"{what} the edit does not move the targets enough to tell a stale teacher"
    e = model.engine(EPOCH["B"], teacher=ema.module, adam_m=opt.exp_avg, adam_v=opt.exp_avg_sq)
    assert e is engine, "the used engine was replaced"
    shadows = dict(params_bf16=torch.equal(e.params_bf16, model._arena.to(torch.bfloat16)),
                   ema_bf16=torch.equal(e.ema_bf16, ema.module._arena.to(torch.bfloat16)))
    used = one_step(model, ema, opt, 3, **kw)
    assert model._engine is engine
    stale = row_distance(used["targets"], fresh["targets"])
    print(f"{what} shadows current before the step: {shadows}; used against fresh targets: rows up to {stale[1]:.2e} apart")
    assert all(shadows.values()), f"{what} stale before the step: {[k for k, v in shadows.items() if not v]}; target rows up to {stale[1]:.2e} off"
    compare(used, fresh, f"{what} used against fresh")
    if skip:
        fresh2, used2 = one_step(fm, fe, fo, 4, **kw), one_step(model, ema, opt, 4, **kw)
        assert torch.equal(fe.module._arena, ema.module._arena), f"{what} the skipped EMA updates moved a teacher"
        fs.rowwise(f"{what} second step targets", used2["targets"], fresh2["targets"].double(), 1e-5)
        assert math.isfinite(used2["loss"]) and math.isfinite(fresh2["loss"])
