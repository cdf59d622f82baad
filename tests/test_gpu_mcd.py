"""GPU: MC-dropout (csrc/mcd.hip, uvit_engine_forward_tail, uncertainty-vit_amd/mcd_probe.py) against the
float64 restatement of tests/mcd_ref.py on the same inputs.  Every bound is derived in mcd_ref's docstring from the unit round-off of
the operations the kernels perform; none comes from running them.  Every op test prints the worst |error| / bound before it asserts."""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

import detect_ref as dr
import mcd_ref as mr
from gpu_util import assert_grads_close, native_model, native_steps, native_trainer
from oracle import vit_oracle as vo
from oracle.closed_form import closed_form_images, exact_masks
from test_gpu_maha import EXACT_TOL, SUM_TOL, batches_of, same
from test_gpu_probe import P, S, f32, frozen_state, ok

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ACT_RT, ACT_AT = 2e-2, 2e-2      # tests/test_gpu_model.py: the native forward of the same tiny models against the oracle
ARG, SHAPE = -1, -2
GUARD = 64


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n, dtype, fill=7.0):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def intact(t, n, fill=7.0):
    return bool((t[n:] == fill).all())


def run_mcd(L, stack, mode, unc=True, rows=None):
    """T uvit_op_mcd_accumulate calls and one uvit_op_mcd_finalize on rows [lo, hi) of a (T, B, K) stack, on a state of exactly the
    size asked for plus a guard: (z (B', K) fp32, unc (B', 5) float64 or None)."""
    T, B, K = stack.shape
    lo, hi = rows if rows is not None else (0, B)
    n = hi - lo
    nbytes = L.uvit_op_mcd_state_bytes(n, K)
    assert nbytes == n * L.uvit_op_mcd_state_bytes(1, K)
    state = guarded(nbytes, torch.uint8, 7)
    state[:nbytes] = 0xA5                                     # first = 1 overwrites: no memset is needed
    z, u = guarded(n * K, F32), guarded(n * 5, F64) if unc else None
    passes = [dev(stack[t, lo:hi]) for t in range(T)]
    for t, x in enumerate(passes):
        ok(L.uvit_op_mcd_accumulate(P(x), P(state), 1 if t == 0 else 0, n, K, S()))
    ok(L.uvit_op_mcd_finalize(P(state), T, mode, P(z), P(u), n, K, S()))
    torch.cuda.synchronize()
    assert intact(state, nbytes, 7) and intact(z, n * K) and (u is None or intact(u, n * 5))
    return z[:n * K].view(n, K).cpu().numpy(), None if u is None else u[:n * 5].view(n, 5).cpu().numpy()


@lru_cache(maxsize=None)
def shape_case(shape, mode):
    """Per (shape, mode), computed once and left unchanged: the stack, the restatement and its bounds."""
    x = mr.logits_case(shape)
    return x, mr.combine(x, mode), mr.bounds(x, mode)


def check_against(z, unc, ref, bd, what):
    zr, ur, kstar, _ = ref
    m = bd["z_mask"]
    rz = (np.abs(z.astype(np.float64) - zr)[m] / bd["z"][m]).max()
    cols = [np.abs(unc[:, i] - ur[:, i]) / bd[k] for i, k in enumerate(("total", "aleatoric", "mi", "var"))]
    print(f"\n{what}: |error| / bound  z {rz:.3f}  total {cols[0].max():.3f}  aleatoric {cols[1].max():.3f}  mi {cols[2].max():.3f}  "
          f"var {cols[3].max():.3f}; unc row 0 {unc[0].tolist()}")
    assert rz < 1.0 and all(c.max() < 1.0 for c in cols) and z.dtype == np.float32
    assert bd["gap_ok"].all() and np.array_equal(z.argmax(1), kstar)
    assert np.abs(unc[:, 4] - ur[:, 4]).max() <= 2 * mr.UD                 # the votes are exact; 1 - votes / T is two roundings


# ------------------------------------------------------------------------------------------------------------------------ the ops
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", mr.SHAPES)
def test_combination(L, shape, mode):
    """z and the five columns against mcd_ref within the bounds; the same bits on a second run, when the rows go in two calls, and
    for z with and without unc; for T <= 16, unc against uvit_op_ens_combine on the stacked logits."""
    B, K, T = shape
    x, ref, bd = shape_case(shape, mode)
    z, unc = run_mcd(L, x, mode)
    check_against(z, unc, ref, bd, f"combination {shape} mode {mode}")
    z2, unc2 = run_mcd(L, x, mode)
    assert z2.tobytes() == z.tobytes() and unc2.tobytes() == unc.tobytes()
    z3, none = run_mcd(L, x, mode, unc=False)
    assert none is None and z3.tobytes() == z.tobytes()
    if B > 1:
        cut = min(17, B - 1)
        parts = [run_mcd(L, x, mode, rows=r) for r in ((0, cut), (cut, B))]
        assert np.concatenate([p[0] for p in parts]).tobytes() == z.tobytes()
        assert np.concatenate([p[1] for p in parts]).tobytes() == unc.tobytes()
    # the ensemble's combination of the same passes as members: the same fp32 softmax and double sums, so the same bounds hold for
    # it (its variance is the centred form: also within (4 eps + (T + 8) ud) m2) and the two agree within their sum.  Its z is an
    # fp32 sum of T terms; its k* is the restatement's where the gap exceeds that rounding as well.
    lin = dev(np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(B, T * K))
    ze, ue = guarded(B * K, F32), guarded(B * 5, F64)
    ok(L.uvit_op_ens_combine(P(lin), mode, P(ze), P(ue), B, T, K, S()))
    torch.cuda.synchronize()
    ue = ue[:B * 5].view(B, 5).cpu().numpy()
    zr = ref[0]
    if K > 1:
        top = np.sort(zr, axis=1)[:, -2:]
        assert ((top[:, 1] - top[:, 0]) > 2 * ((T + 2) * mr.U * np.abs(zr).max(1) + bd["z"].max(1))).all()
    for i, k in enumerate(("total", "aleatoric", "mi", "var")):
        assert (np.abs(unc[:, i] - ue[:, i]) <= 2 * bd[k]).all(), k
    assert np.abs(unc[:, 4] - ue[:, 4]).max() <= 2 * mr.UD


def test_nan_row_and_its_neighbours(L):
    """A NaN in one pass and a +inf in another flag their rows: five NaNs; every other row keeps the bits of the clean call."""
    x = mr.logits_case((17, 65, 5)).copy()
    clean_z, clean_u = run_mcd(L, x, 0)
    x[2, 3, 64], x[4, 9, 0] = np.nan, np.inf
    z, unc = run_mcd(L, x, 0)
    bad = np.zeros(17, dtype=bool)
    bad[[3, 9]] = True
    assert np.isnan(unc[bad]).all() and unc[~bad].tobytes() == clean_u[~bad].tobytes() and z[~bad].tobytes() == clean_z[~bad].tobytes()
    assert np.isnan(z[3, 64]) and z[9, 0] == np.inf
    _, ur, _, _ = mr.combine(x, 0)
    assert np.array_equal(np.isnan(ur), np.isnan(unc))


def test_ties_take_the_lowest_index(L):
    """Whole-number logits and T = 2: the means and the ties are exact.  Row 1 ties two classes in every pass, row 2's passes vote
    for classes 1 and 3 and their mean ties them."""
    x = np.zeros((2, 3, 70), dtype=np.float32)
    x[:, 1, [2, 66]] = 3.0                                  # a tie across two lanes' strides
    x[0, 2, 1], x[1, 2, 3] = 2.0, 2.0
    for mode in (0, 1):
        z, unc = run_mcd(L, x, mode)
        _, ur, kstar, _ = mr.combine(x, mode)
        assert kstar.tolist() == [0, 2, 1] and unc[:, 4].tolist() == ur[:, 4].tolist() == [0.0, 0.0, 0.5]
        if mode == 0:
            assert z[1, 2] == z[1, 66] == 3.0 and z[2, 1] == z[2, 3] == 1.0


# ---------------------------------------------------------------------------------------------------------------------- the tail
TAIL_SEED, TAIL_IT = 77, 5
MODELS = {"d4": (dict(img_size=48, embed_dim=128, depth=4, num_heads=2, attn_drop_rate=0.1), 3),
          "hd80": (dict(img_size=48, embed_dim=320, depth=2, num_heads=4, attn_drop_rate=0.1), 5)}


def tail_cfg(name, **over):
    return vo.VitConfig(init_values=0.1, **{**MODELS[name][0], **over})


def forward(L, model, x, train=0, seed=TAIL_SEED, it=TAIL_IT):
    """uvit_engine_forward_features with the student weights; returns the engine."""
    e = model.engine(x.shape[0])
    ok(L.uvit_engine_forward_features(e.h, 0, P(x), None, x.shape[0], train, seed, it, S()))
    model._fwd_batch = x.shape[0]
    return e


def tail(L, e, B, first, train=1, seed=TAIL_SEED, it=TAIL_IT, which=0):
    return L.uvit_engine_forward_tail(e.h, which, B, first, train, seed, it, S())


def streams(e, cfg, B):
    return [e.ws_tensor("x", l, (B, cfg.num_tokens, cfg.embed_dim)).clone() for l in range(cfg.depth + 1)]


@lru_cache(maxsize=None)
def tail_case(name):
    """Per model, computed once and left unchanged: config, images, the closed-form state and the oracle's X[depth] per first_layer
    with the kernel's masks replayed in blocks >= first_layer and none below."""
    cfg, B = tail_cfg(name), MODELS[name][1]
    x = closed_form_images(f"mcd-tail/{name}", B, cfg.img_size)
    _, sd = native_model(cfg, device="cpu")
    aseed = int(vo._mix32(np.uint32(TAIL_SEED) ^ np.uint32((TAIL_IT * 0x85EBCA6B + 0x1234567) & 0xFFFFFFFF)))
    want = {}
    for first in range(cfg.depth):
        keep = [vo.attn_keep_mask(aseed, l, B, cfg.num_heads, cfg.num_tokens, cfg.attn_drop_rate) if l >= first else None
                for l in range(cfg.depth)]
        with torch.no_grad():
            want[first] = vo.forward_features({k: v.clone() for k, v in sd.items()}, cfg, x, None, "end", drop=vo.DropState(attn=keep))[-1]
    return cfg, B, x, want


@pytest.mark.parametrize("name", list(MODELS))
def test_tail_reproduces_the_forward(L, name):
    """(a) without dropout every tail reproduces the deterministic X[depth] bit for bit; (b) from block 0 with dropout it is the
    training-mode forward at (seed, it); (c) from every first_layer it matches the oracle with the masks replayed from that block on;
    (d) X[0 .. first_layer] keep their bits through three tails."""
    cfg, B, x, want = tail_case(name)
    model, _ = native_model(cfg)
    model.eval()
    xg = x.cuda()
    e = forward(L, model, xg)
    det = streams(e, cfg, B)
    for first in reversed(range(cfg.depth)):               # downwards: a tail above an earlier tail's block is refused
        ok(tail(L, e, B, first, train=0))
        assert all(torch.equal(a, b) for a, b in zip(streams(e, cfg, B), det)), first                         # (a)
    e = forward(L, model, xg, train=1)
    drop = streams(e, cfg, B)
    assert not torch.equal(drop[-1], det[-1])
    e = forward(L, model, xg)
    ok(tail(L, e, B, 0))
    assert all(torch.equal(a, b) for a, b in zip(streams(e, cfg, B), drop))                                   # (b)
    for first in range(cfg.depth):
        e = forward(L, model, xg)                          # a tail from a lower block has overwritten X[first]: the engine would refuse
        for it in (TAIL_IT + 1, TAIL_IT + 2, TAIL_IT):
            ok(tail(L, e, B, first, it=it))
        got = streams(e, cfg, B)
        assert all(torch.equal(got[l], det[l]) for l in range(first + 1)), first                               # (d)
        assert not torch.equal(got[-1], det[-1])
        err = (got[-1].cpu() - want[first]).abs() / (ACT_AT + ACT_RT * want[first].abs())
        print(f"\ntail {name} from block {first}: worst |error| / tolerance against the oracle {float(err.max()):.3f}")
        torch.testing.assert_close(got[-1].cpu(), want[first], rtol=ACT_RT, atol=ACT_AT)                       # (c)
    if cfg.depth > 2:        # the masks of a block are part of the answer: another block's masks are another answer
        assert float((want[1] - want[2]).abs().max()) > 1e-4


def test_tail_draws_no_drop_path(L):
    """(e) with drop_path_rate > 0 in the config the tail is that of the same weights without drop-path, bit for bit, and not the
    training-mode forward (which drops paths)."""
    cfg, B, x, _ = tail_case("d4")
    xg = x.cuda()
    with_dp, _ = native_model(tail_cfg("d4", drop_path_rate=0.5))
    without, _ = native_model(cfg)
    e1, e0 = forward(L, with_dp.eval(), xg), forward(L, without.eval(), xg)
    ok(tail(L, e1, B, 0))
    ok(tail(L, e0, B, 0))
    a, b = streams(e1, cfg, B), streams(e0, cfg, B)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    e1 = forward(L, with_dp, xg, train=1)
    assert not torch.equal(streams(e1, cfg, B)[-1], a[-1])


def test_tails_change_nothing_later(L):
    """(f) a forward, and a training step, after tails are what they are without them."""
    cfg, B, x, _ = tail_case("d4")
    cfg = tail_cfg("d4", drop_path_rate=0.5)               # the step draws drop-path and runs on its sample lists
    xg, mask = x.cuda(), exact_masks(B, cfg.num_patches, 4, 31).cuda()
    lr, runs = 2e-3, []
    for with_tails in (False, True):
        model, _ = native_model(cfg)
        ema, opt = native_trainer(model, lr=0.0)
        # The trainer builds its own engine (with the teacher and the optimizer's moments) at its first step.  That step runs at
        # lr = 0, so both runs reach the compared step with the same parameter bits, whatever order its atomics summed in.
        torch.manual_seed(1234)
        native_steps(model, ema, opt, [(xg, mask)], [2, 3], start=6)
        for g in opt.param_groups:
            g["lr"] = lr
        e = forward(L, model.eval(), xg)
        assert e is model._engine
        if with_tails:
            for first, it in ((3, 1), (2, 2), (0, 3), (0, 4)):
                ok(tail(L, e, B, first, it=it))
            assert not torch.equal(streams(e, cfg, B)[-1], runs[0][0][-1])
        e = forward(L, model, xg)
        fwd = streams(e, cfg, B)
        model.train()
        st = native_steps(model, ema, opt, [(xg, mask)], [2, 3], start=7)[0]
        assert model._engine is e                          # the step ran on the engine that ran the tails
        runs.append((fwd, st, {n: q.grad.detach().float().cpu().clone() for n, q in model.named_parameters()}, model._arena.clone()))
    (f0, s0, g0, p0), (f1, s1, g1, p1) = runs
    assert all(torch.equal(a, b) for a, b in zip(f0, f1))
    # Same model, same batch, same seeds, twice: the tolerances of tests/test_gpu_model.py::test_last_block_on_masked_rows_equals_all_rows
    # (the weight gradients are summed in an order that is not fixed); the parameters one AdamW step later: a sign flip on a ~0
    # gradient is 2 lr apart (the same file's rule for its two-step comparison, per step).
    assert s1["loss"] == pytest.approx(s0["loss"], rel=1e-6) and s1["grad_norm"] == pytest.approx(s0["grad_norm"], rel=1e-5)
    assert_grads_close(g1, g0, max_tol=1e-4, l2_tol=1e-4, what="[step after tails vs step without] ")
    torch.testing.assert_close(p1, p0, rtol=0, atol=2 * lr + 1e-6)
    assert not torch.equal(p0, native_model(cfg)[0]._arena)                   # the compared step did move the parameters


def test_tail_refusals(L):
    """(g) no forward yet, a stale tail behind a training step, another batch or weight set, a block out of range or above an earlier
    tail's, the two-stream model, a NULL engine: refused, and nothing is launched (the residual streams keep their bits)."""
    cfg, B, x, _ = tail_case("d4")
    xg, mask = x.cuda(), exact_masks(B, cfg.num_patches, 4, 31).cuda()
    model, _ = native_model(cfg)
    ema, opt = native_trainer(model)
    e = model.engine(B)
    assert tail(L, e, B, 0) == ARG                                           # a fresh engine
    e = forward(L, model.eval(), xg)
    kept = streams(e, cfg, B)
    assert tail(L, e, B - 1, 0) == ARG and tail(L, e, B + 1, 0) == ARG and tail(L, e, B, 0, which=1) == ARG and tail(L, e, B, 0, which=2) == ARG
    assert tail(L, e, B, -1) == ARG and tail(L, e, B, cfg.depth) == ARG
    assert L.uvit_engine_forward_tail(None, 0, B, 0, 1, 0, 0, S()) == ARG
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(streams(e, cfg, B), kept))
    ok(tail(L, e, B, cfg.depth - 1))
    ok(tail(L, e, B, 0))                                                     # a tail follows a tail, downwards
    after = streams(e, cfg, B)
    assert tail(L, e, B, 1) == ARG and tail(L, e, B, cfg.depth - 1) == ARG   # X[1] is the last tail's, not the forward's
    ok(tail(L, e, B, 0, it=TAIL_IT))                                         # the same block again: the same bits
    assert all(torch.equal(a, b) for a, b in zip(streams(e, cfg, B), after))
    model.train()
    native_steps(model, ema, opt, [(xg, mask)], [2, 3])                      # (the trainer builds its own engine)
    e = forward(L, model.eval(), xg)
    ok(tail(L, e, B, 1))
    model.train()
    native_steps(model, ema, opt, [(xg, mask)], [2, 3], start=1)
    model.eval()
    assert model._engine is e and tail(L, e, B, 0) == ARG                    # stale: a training step came between
    from uncertainty_vit_amd.native import UvitError
    with pytest.raises(UvitError):
        model.forward_tail(0, 0, 0)
    forward(L, model, xg[:2])
    assert tail(L, model._engine, 2, 1) == 0 and tail(L, model._engine, B, 1) == ARG
    two, _ = native_model(vo.VitConfig(img_size=48, embed_dim=128, depth=2, num_heads=2, init_values=0.1, use_abs_pos_emb=False), two_stream=True)
    e2 = forward(L, two.eval(), xg)
    assert tail(L, e2, B, 0) == SHAPE


# --------------------------------------------------------------------------------------------------------------------- the probe
K_, T_ = 10, 4
PROBE_CFG = dict(img_size=48, embed_dim=128, depth=3, num_heads=2, attn_drop_rate=0.2)


@pytest.fixture(scope="module")
def encoder():
    model, _ = native_model(vo.VitConfig(init_values=0.1, **PROBE_CFG))
    return model.eval()


def make(enc, **kw):
    from uncertainty_vit_amd.mcd_probe import MCDropoutProbe
    torch.manual_seed(5)
    return MCDropoutProbe(enc, K_, **{"passes": T_, "layers": 2, "seed": 9, "init_scale": 5.0, **kw})


def linear(enc):
    from uncertainty_vit_amd.linear_probe import LinearProbe
    torch.manual_seed(5)
    return LinearProbe(enc, K_, init_scale=5.0)


def manual_stack(L, probe, x, it0):
    """The T passes composed by hand: deterministic forward, then per pass the tail, pool + norm and the head; (T, B, K) fp32."""
    enc, B = probe.encoder, x.shape[0]
    e = enc.forward_features(x, bool_masked_pos=None, layer_results=None)
    N, Cd = enc.patch_embed.num_patches + 1, enc.embed_dim
    feat, scratch = torch.zeros(B, Cd, device="cuda"), torch.zeros(L.uvit_op_probe_pool_ws_bytes(B, N, Cd) // 4, device="cuda")
    out = []
    for t in range(probe.passes):
        ok(L.uvit_engine_forward_tail(e.h, 0, B, probe.first_layer, 1, probe.seed, it0 + t, S()))
        xl = L.uvit_engine_ws_ptr(e.h, b"x", enc.depth)
        ok(L.uvit_op_probe_pool_norm(C.c_void_p(xl), P(feat), P(scratch), B, N, Cd, f32(enc.ln_eps), S()))
        z = torch.zeros(B, K_, device="cuda")
        ok(L.uvit_op_probe_logits(P(feat), P(probe._arena), probe._bias_ptr(probe._arena), P(z), B, K_, Cd, S()))
        out.append(z.cpu().numpy())
    return np.stack(out)


def pass_logits(probe, x, it, dropout=True):
    """(B, K) fp32: the logits of the probe's own single pass at (seed, it); without `dropout`, the deterministic ones through the tail."""
    B = probe._features(x)
    probe._pass_into(B, it, dropout=dropout)
    return probe._mc_lin[:B].clone()


@pytest.mark.parametrize("combine", ["logits", "probs"])
def test_predictive_is_the_composition(L, encoder, combine):
    """predictive() against tail + pool + head per pass fed to the restatement, within its bounds; two passes differ; the
    deterministic feature stays in place; the encoder keeps its bits."""
    probe = make(encoder, combine=combine)
    x = closed_form_images("mcd-probe/0", 5, 48).cuda()
    probe.features(x)
    before = frozen_state(probe)
    mode = 0 if combine == "logits" else 1
    for it0 in (0, 3 * T_):
        got = probe.predictive(x, it0)
        stack = manual_stack(L, probe, x, it0)
        assert not np.array_equal(stack[0], stack[1])
        check_against(got["logits"].cpu().numpy(), got["unc"].cpu().numpy(), mr.combine(stack, mode), mr.bounds(stack, mode),
                      f"predictive {combine} it0 {it0}")
        assert torch.equal(pass_logits(probe, x, it0 + 1), torch.from_numpy(stack[1]).cuda())
    a, b = probe.predictive(x, 0), probe.predictive(x, T_)
    assert not torch.equal(a["logits"], b["logits"]) and torch.equal(probe.logits(x), a["logits"]) and float(a["unc"][:, 2].max()) > 0
    lin = linear(encoder)
    assert torch.equal(probe._feat[:5], lin.features(x)) and torch.equal(pass_logits(probe, x, 0, dropout=False), lin.logits(x))
    assert all(torch.equal(p, q) for p, q in zip(before, frozen_state(probe)))


def test_train_step_and_state_are_a_linear_probes(encoder):
    probe, lin = make(encoder), linear(encoder)
    x, y = closed_form_images("mcd-train", 6, 48).cuda(), torch.arange(6).cuda() % K_
    probe.predictive(x)                                                     # tails before the step change nothing
    for _ in range(2):
        a, b = probe.train_step(x, y, 1e-2, 0.05, 1.0), lin.train_step(x, y, 1e-2, 0.05, 1.0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(probe._arena, lin._arena) and torch.equal(probe.exp_avg, lin.exp_avg) and probe.step_count == 2
    fresh = make(encoder)
    fresh.load_state_dict({k: v.cpu() for k, v in lin.state_dict().items()})             # a linear probe-N.pth
    fresh.load_optimizer_state_dict(lin.optimizer_state_dict())
    assert torch.equal(fresh._arena, probe._arena) and torch.equal(fresh.predictive(x)["logits"], probe.predictive(x)["logits"])
    assert list(fresh.state_dict()) == list(lin.state_dict())


def test_evaluate_stores_predictive_and_scores_it(L, encoder):
    """evaluate(detection, ood, uncertainty): the stored columns are predictive()'s bits at it0 = n T with the OOD batches continuing
    the count, the metrics are detect_ref's on them, the means and det_acc1 are what they say, and a second run gives the same."""
    from uncertainty_vit_amd.mcd_probe import UNC_KEYS
    cfg = vo.VitConfig(init_values=0.1, **PROBE_CFG)
    probe, lin = make(encoder), linear(encoder)
    eval_b, ood_b = batches_of(cfg, "mcd-eval", (4, 3), K=K_), batches_of(cfg, "mcd-ood!", (3, 2), labelled=False)
    stores, metrics_op = [], probe._det_metrics
    probe._det_metrics = lambda scores, ld, flags, N, S, order=None: (stores.append(scores[:, :N].clone()), metrics_op(scores, ld, flags, N, S, order))[1]
    try:
        stats = probe.evaluate(eval_b, detection=True, ood_loader=ood_b, uncertainty=True, calibration=True)
    finally:
        del probe._det_metrics
    xs = [x for (x, _), _ in eval_b] + list(ood_b)
    pred = [probe.predictive(x, n * T_) for n, x in enumerate(xs)]
    unc = torch.cat([p["unc"] for p in pred])
    store = stores[-1].cpu().numpy()
    assert store.shape == (8, 12) and store[3:].tobytes() == unc.t().float().contiguous().cpu().numpy().tobytes()
    assert same(stats, probe.evaluate(eval_b, detection=True, ood_loader=ood_b, uncertainty=True, calibration=True))
    det = stats["detection"]
    y = np.concatenate([y.numpy() for _, y in eval_b])
    z = torch.cat([p["logits"] for p in pred[:2]]).cpu().numpy()
    wrong = (z.argmax(1) != y).astype(np.uint8)
    assert det["columns"] == ["msp", "entropy", "energy"] + list(UNC_KEYS) and (det["n"], det["n_ood"], det["n_wrong"]) == (7, 5, int(wrong.sum()))
    assert stats["acc1"] == 100.0 * int((z.argmax(1) == y).sum()) / 7
    mis, _ = dr.table(store[3:, :7], wrong)
    ood, _ = dr.table(store[3:], np.concatenate([np.zeros(7, dtype=np.uint8), np.ones(5, dtype=np.uint8)]))
    for s, name in enumerate(UNC_KEYS):
        for table, entry, keys in ((mis, det["misclassification"][name], ("AUROC", "AUPR", "FPR95", "AURC")), (ood, det["ood"][name], ("AUROC", "AUPR", "FPR95"))):
            for k, key in enumerate(keys):
                r, g = table[s, k], entry[key]
                assert (math.isnan(r) and math.isnan(g)) or abs(g - r) <= (EXACT_TOL if key in ("AUROC", "FPR95") else SUM_TOL), (name, key, g, r)
    rows = unc[:7].cpu().tolist()
    for col, key in enumerate(UNC_KEYS):
        assert stats[key] == math.fsum(r[col] for r in rows) / 7
    assert (stats["mcd_passes"], stats["mcd_layers"]) == (T_, 2)
    assert stats["det_acc1"] == lin.evaluate(eval_b)["acc1"]
    plain = probe.evaluate(eval_b)
    assert set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"} and plain["loss"] == stats["loss"]


def test_feature_scores_read_the_deterministic_feature(encoder):
    """Beside a density, a bank and a ViM fit, their columns are those of a LinearProbe on the same images: 13 columns in all."""
    cfg = vo.VitConfig(init_values=0.1, **PROBE_CFG)
    fit_b, eval_b = batches_of(cfg, "mcd-fit", (5, 4, 3), K=K_), batches_of(cfg, "mcd-eval", (4, 3), K=K_)
    ood_b = batches_of(cfg, "mcd-ood!", (3, 2), labelled=False)
    got = {}
    for name, probe in (("mcd", make(encoder)), ("linear", linear(encoder))):
        probe.fit_density(fit_b)
        probe.fit_neighbours(fit_b, k=3)
        probe.fit_vim(fit_b, dim=4)
        stores, metrics_op = [], probe._det_metrics
        probe._det_metrics = lambda scores, ld, flags, N, S, order=None, m=metrics_op, st=stores: (st.append(scores[:, :N].clone()), m(scores, ld, flags, N, S, order))[1]
        try:
            stats = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
        finally:
            del probe._det_metrics
        got[name] = (stats, stores[-1].cpu().numpy())
    (sm, am), (sl, al) = got["mcd"], got["linear"]
    assert am.shape == (13, 12) and al.shape == (8, 12) and am[8:].tobytes() == al[3:].tobytes()
    assert sm["detection"]["columns"][8:] == sl["detection"]["columns"][3:] == ["maha", "rmaha", "knn", "vim", "residual"]
    for key in ("maha_mean", "maha_acc1", "knn_mean", "knn_acc1", "vim_mean", "vim_acc1"):
        assert sm[key] == sl[key], key


def test_post_hoc_families_see_the_combination(encoder):
    """Temperature, conformal sets and stability run on the combined logits of it0 = n T: each equals its *_batch form on
    predictive()'s logits."""
    cfg = vo.VitConfig(init_values=0.1, **PROBE_CFG)
    probe = make(encoder)
    cal_b = batches_of(cfg, "mcd-cal", (6, 5), K=K_)
    z = torch.cat([probe.predictive(x, n * T_)["logits"] for n, ((x, _), _) in enumerate(cal_b)])
    y = torch.cat([y for _, y in cal_b]).cuda()
    fit = probe.fit_temperature(cal_b)
    table = probe.temperature_batch(z, y).cpu().tolist()
    assert fit["T"] == table[0] and fit["nll_before"] == table[2] and fit["n"] == 11
    probe.set_temperature(None)
    cp = probe.fit_conformal(cal_b, alpha=0.2, score="aps")
    assert cp["qhat"] == probe.conformal_calibrate(z, y, alpha=0.2, score="aps")["table"][:, 1].cpu().tolist()
    ev = probe.evaluate_conformal(cal_b, sizes=True)
    sets = probe.conformal_sets(z, y, probe.conformal)
    assert torch.equal(ev["sizes"], sets["sizes"]) and ev["conformal"][0.2]["n"] == 11
    seq_b = [closed_form_images(f"mcd-seq/{i}", 6, 48).cuda() for i in range(2)]            # 2 sequences of 3 frames per batch
    st = probe.evaluate_stability(seq_b, frames=3, noise=False, n_sequences=4)
    sums = torch.cat([probe.stability_batch(probe.predictive(x, n * T_)["logits"], 3, False).clone() for n, x in enumerate(seq_b)]).cpu()
    assert st["n_sequences"] == 4 and st["flip_prob"] == sum(r / 2 for r in sums[:, 0].tolist()) / 4
    assert st["zipf_dist"] == sum(r / 2 for r in sums[:, 2].tolist()) / 4
