"""GPU: learned layer weights (csrc/layerweights.hip, uncertainty-vit_amd/lw_probe.py) against the float64
restatement of tests/lw_ref.py on the same inputs and against what the reference classifier computed
(tests/golden/probe_lw_t48.npz).  Every bound is derived in lw_ref's docstring from the kernels' summation lengths; none comes from
running them.  Every op test prints the worst |error| / bound before it asserts."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import lw_ref as lr
import probe_ref as pr
from gpu_util import expected_update, native_model
from oracle import vit_oracle as vo
from oracle.closed_form import closed_form_images
from test_gpu_maha import batches_of, same
from test_gpu_probe import ACT_AT, ACT_RT, P, S, f32, fixture_probe, frozen_state, guard_intact, guarded, ok

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
COMBOS = [(False, False), (False, True), (True, False), (True, True)]      # (use_cls, layernorm_before_combine)
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]                                   # (mode, layernorm)


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def within(got, ref, bound, what):
    """|got - ref| <= bound element by element (a zero bound: equality); prints the worst ratio."""
    err = (got.detach().cpu().to(F64) - ref).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, bound)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    print(f"\n{what}: worst |error| / bound {float(ratio.max()):.3f} (largest |ref| {float(ref.abs().max()):.3e})")
    assert bool((ratio <= 1.0).all()), (what, int(ratio.argmax()), float(ratio.max()))


# ------------------------------------------------------------------------------------------------------------------------ the pool
def run_pool(L, xs, mode, ln, reverse=False):
    """uvit_op_lw_pool twice on L device copies of `xs` (one allocation, the layers in ascending or descending address order) with
    guarded outputs: pooled (B, L, C) on the device; the two runs give the same bits."""
    B, N, Cd = xs[0].shape
    Ln = len(xs)
    slab = torch.empty(Ln, B, N, Cd, device="cuda")
    slots = list(reversed(range(Ln))) if reverse else list(range(Ln))
    for l, x in enumerate(xs):
        slab[slots[l]].copy_(x)
    ptrs = (C.c_void_p * Ln)(*[slab[slots[l]].data_ptr() for l in range(Ln)])
    ws = L.uvit_op_lw_pool_ws_bytes(B, Ln, N, Cd)
    assert ws == B * Ln * 8 * Cd * 4
    outs = []
    for _ in range(2):
        pooled, scratch = guarded(B * Ln * Cd), guarded(ws // 4)
        ok(L.uvit_op_lw_pool(ptrs, Ln, P(pooled), P(scratch), B, N, Cd, mode, ln, f32(lr.LN_EPS), S()))
        torch.cuda.synchronize()
        assert guard_intact(pooled, B * Ln * Cd) and guard_intact(scratch, ws // 4)
        if mode == 1:
            assert bool((scratch == 7.5).all())                   # token 0 alone: the scratch is not touched
        outs.append(pooled[:B * Ln * Cd].view(B, Ln, Cd).clone())
    assert torch.equal(outs[0], outs[1])
    return outs[0]


@lru_cache(maxsize=None)
def pool_case(shape, mode, ln):
    """Per (shape, mode, layernorm), computed once and left unchanged: the streams, the restatement and its bound."""
    xs = lr.stream_case(shape)
    return xs, lr.pool(xs, mode, bool(ln)), lr.pool_bound(xs, mode, bool(ln))


@pytest.mark.parametrize("mode,ln", MODES)
@pytest.mark.parametrize("shape", lr.POOL_SHAPES)
def test_pool(L, shape, mode, ln):
    """pooled against float64 within lw_ref.pool_bound: one token and one float4 (1, 1, 1, 4); fewer float4 than lanes, B no multiple
    of the four rows of a workgroup, empty slices (N = 10 < 16) (5, 2, 10, 128); ViT-B's row (3, 12, 197, 768); ViT-H's (2, 3, 197,
    1280); the deepest and widest the op takes, with slices of one token (2, 64, 7, 2048).  mode 1 without layernorm is a copy: bit
    equality."""
    xs, ref, bound = pool_case(shape, mode, ln)
    got = run_pool(L, xs, mode, ln)
    within(got, ref, bound, f"lw_pool {shape} mode {mode} layernorm {ln}")
    if mode == 1 and not ln:
        assert torch.equal(got.cpu(), torch.stack([x[:, 0] for x in xs], 1))


def test_pool_takes_the_layers_in_any_address_order(L):
    xs, ref, bound = pool_case((5, 2, 10, 128), 0, 1)
    xs3 = lr.stream_case((3, 12, 197, 768))
    for streams in (xs, xs3):
        for mode in (0, 1):
            assert torch.equal(run_pool(L, streams, mode, 1, reverse=True), run_pool(L, streams, mode, 1))
    within(run_pool(L, xs, 0, 1, reverse=True), ref, bound, "lw_pool, descending addresses")


def test_pool_counts_the_cls_token_in_the_mean_and_nothing_else_in_mode_1(L):
    """Token 0 of layer 1 is 1e4, everything else of spread 0.01: the mean over ALL tokens is about 1e3 there (x[:, 1:].mean(1), the
    default path's pool, would be about 0), mode 1 returns 1e4 bit for bit there and layer 0's small token 0 elsewhere."""
    B, N, Cd = 2, 10, 128
    xs = [lr.rnd(B, N, Cd, seed=40 + l, scale=0.01) for l in range(2)]
    xs[1][:, 0, :] = 1e4
    got = run_pool(L, xs, 0, 0)
    within(got, lr.pool(xs, 0, False), lr.pool_bound(xs, 0, False), "lw_pool, cls token 1e4, mode 0")
    assert float(got[:, 1].min()) > 999.0 and float(got[:, 0].abs().max()) < 0.05
    patches_only = torch.stack([x[:, 1:].to(F64).mean(1) for x in xs], 1)
    assert float((got.cpu().to(F64) - patches_only)[:, 1].abs().min()) > 999.0
    cls = run_pool(L, xs, 1, 0).cpu()
    assert torch.equal(cls[:, 1], torch.full((B, Cd), 1e4)) and torch.equal(cls[:, 0], xs[0][:, 0])


@pytest.mark.parametrize("mode", [0, 1])
def test_pool_layernorm_of_a_constant_row_is_zero(L, mode):
    """Every element 3: the sums 7 x 3 and 128 x 3 are exact, 21 / 7 is 3, the variance is 0 and (3 - 3) * rsqrt(eps) is 0, not NaN."""
    xs = [torch.full((2, 7, 128), 3.0) for _ in range(2)]
    got = run_pool(L, xs, mode, 1)
    assert bool((got == 0).all())


# --------------------------------------------------------------------------------------------------------------------- the combine
def run_combine(L, pooled, log_w, want_w=True):
    B, Ln, Cd = pooled.shape
    pg, wg = pooled.contiguous().cuda(), log_w.to(F32).cuda()
    outs = []
    for _ in range(2):
        feat, w = guarded(B * Cd), guarded(Ln) if want_w else None
        ok(L.uvit_op_lw_combine(P(pg), P(wg), P(feat), P(w), B, Ln, Cd, S()))
        torch.cuda.synchronize()
        assert guard_intact(feat, B * Cd) and (w is None or guard_intact(w, Ln))
        outs.append((feat[:B * Cd].view(B, Cd).clone(), None if w is None else w[:Ln].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and (not want_w or torch.equal(outs[0][1], outs[1][1]))
    return outs[0]


@lru_cache(maxsize=None)
def mix_case(blc):
    """Per (B, L, C), computed once and left unchanged: pooled vectors of spread 1, log-weights, an upstream gradient of size 1 / B."""
    B, Ln, Cd = blc
    return lr.rnd(B, Ln, Cd, seed=50) + lr.rnd(1, Ln, 1, seed=51), lr.log_w_case(Ln), lr.rnd(B, Cd, seed=52, scale=1.0 / B)


MIX_SHAPES = [(b, l, c) for b, l, _, c in lr.POOL_SHAPES]


@pytest.mark.parametrize("blc", MIX_SHAPES)
def test_combine(L, blc):
    pooled, log_w, _ = mix_case(blc)
    feat, w = run_combine(L, pooled, log_w)
    within(feat, lr.combine(pooled, log_w), lr.combine_bound(pooled, log_w), f"lw_combine {blc}")
    wr = lr.softmax_w(log_w)
    within(w, wr, lr.SLACK * lr.softmax_rel(log_w) * wr, f"lw_combine {blc} weights")
    assert torch.equal(run_combine(L, pooled, log_w, want_w=False)[0], feat)          # the same bits without w_out


def test_combine_exact_cases(L):
    """(a) log-weights (0, -1e4, -1e4): exp(-1e4) is 0, w = (1, 0, 0) and the fma chain returns layer 0's bits.  (b) equal log-weights at
    L = 4 and inputs on the grid of 1 / 8: every w is exactly 1 / 4 and every partial sum is a multiple of 1 / 32 below 2^24 / 32: the
    exact mean.  (c) +-30: the softmax saturates to (1, e^-60) without a NaN."""
    pooled = lr.rnd(5, 3, 132, seed=60)
    feat, w = run_combine(L, pooled, torch.tensor([0.0, -1e4, -1e4]))
    assert w.tolist() == [1.0, 0.0, 0.0] and torch.equal(feat.cpu(), pooled[:, 0])
    grid = torch.randint(-64, 65, (3, 4, 260), generator=torch.Generator().manual_seed(61)).float() / 8.0
    feat, w = run_combine(L, grid, torch.full((4,), 1.25))
    assert w.tolist() == [0.25] * 4 and torch.equal(feat.cpu().to(F64), grid.to(F64).mean(1))
    feat, w = run_combine(L, pooled[:, :2].contiguous(), torch.tensor([30.0, -30.0]))
    assert w[0].item() == 1.0 and 0.0 < w[1].item() < 1e-25 and bool(torch.isfinite(feat).all())


# ------------------------------------------------------------------------------------------------------------- the input gradient
@lru_cache(maxsize=None)
def input_grad_case(bkc):
    B, K, Cd = bkc
    d, W = lr.rnd(B, K, seed=4, scale=1.0 / B), lr.rnd(K, Cd, seed=2, scale=0.05)
    return d, W, lr.input_grad(d, W), lr.input_grad_bound(d, W)


@pytest.mark.parametrize("bkc", lr.INPUT_GRAD_SHAPES)
def test_input_grad(L, bkc):
    """dfeat = dlogits . W against float64: one element (1, 1, 4); K no multiple of 4 or of the tile (5, 10, 128); partial tiles in all
    three dimensions and more than one workgroup each way (67, 130, 260); the benchmarked head (128, 1000, 768).  The output held 5.0
    before (it is overwritten) and two runs give the same bits."""
    B, K, Cd = bkc
    d, W, ref, bound = input_grad_case(bkc)
    dg, Wg = d.cuda(), W.cuda()
    runs = []
    for _ in range(2):
        out = guarded(B * Cd, 5.0)
        ok(L.uvit_op_probe_input_grad(P(dg), P(Wg), P(out), B, K, Cd, S()))
        torch.cuda.synchronize()
        assert guard_intact(out, B * Cd, 5.0)
        runs.append(out[:B * Cd].view(B, Cd).clone())
    assert torch.equal(runs[0], runs[1])
    within(runs[0], ref, bound, f"probe_input_grad {bkc}")


# -------------------------------------------------------------------------------------------------------------- the layer gradient
def run_lw_grad(L, dfeat, pooled, log_w):
    B, Ln, Cd = pooled.shape
    dg, pg, wg = dfeat.contiguous().cuda(), pooled.contiguous().cuda(), log_w.to(F32).cuda()
    runs = []
    for _ in range(2):
        out = guarded(Ln, 5.0)
        scratch = torch.full((B * Ln + 8,), 7.0, dtype=F64, device="cuda")
        ok(L.uvit_op_lw_grad(P(dg), P(pg), P(wg), P(out), P(scratch), B, Ln, Cd, S()))
        torch.cuda.synchronize()
        assert guard_intact(out, Ln, 5.0) and bool((scratch[B * Ln:] == 7.0).all())
        runs.append(out[:Ln].clone())
    assert torch.equal(runs[0], runs[1])
    return runs[0]


@pytest.mark.parametrize("blc", MIX_SHAPES)
def test_lw_grad(L, blc):
    pooled, log_w, dfeat = mix_case(blc)
    ref, _ = lr.lw_grad(dfeat, pooled, log_w)
    within(run_lw_grad(L, dfeat, pooled, log_w), ref, lr.lw_grad_bound(dfeat, pooled, log_w), f"lw_grad {blc}")


def test_lw_grad_of_identical_layers_is_zero_within_the_bound(L):
    """Every g_l is equal, so every dlog_w_l is 0 in exact arithmetic: what remains is the rounding of w, and the bound on it is at
    least a hundred times below each term w_l g_l of the difference."""
    B, Ln, Cd = 6, 12, 768
    pooled = (lr.rnd(B, 1, Cd, seed=70) + 3.0).expand(B, Ln, Cd).contiguous()
    dfeat, log_w = lr.rnd(B, Cd, seed=71, scale=1.0 / B), lr.log_w_case(Ln)
    ref, g = lr.lw_grad(dfeat, pooled, log_w)
    got = run_lw_grad(L, dfeat, pooled, log_w)
    bound = lr.lw_grad_bound(dfeat, pooled, log_w)
    within(got, ref, bound, "lw_grad, identical layers")
    assert float(ref.abs().max()) <= 16 * lr.UD * lr.lw_grad_scale(dfeat, pooled)
    assert bool((bound < 1e-2 * (lr.softmax_w(log_w) * g).abs()).all())            # the bound is far below each term w_l g_l of the difference


# ------------------------------------------------------------------------------------------------------------------- the module
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir), np.load(os.path.join(golden_dir, "probe_lw_t48.npz"))


def lw_probe(encoder, K, log_w=None, **kw):
    from uncertainty_vit_amd.lw_probe import LayerWeightedProbe
    torch.manual_seed(5)
    probe = LayerWeightedProbe(encoder, K, **kw)
    if log_w is not None:
        with torch.no_grad():
            probe.layer_log_weights.copy_(log_w)
    return probe


def fixture_lw_probe(case, c, encoder=None):
    (fx, cfg, enc, W, bias, _, _), lw = case
    use_cls, ln = COMBOS[c]
    encoder = encoder if encoder is not None else fixture_probe(case[0]).encoder
    probe = lw_probe(encoder, W.shape[0], smoothing=float(fx["smoothing"]), use_cls=use_cls, layernorm_before_combine=ln)
    probe.load_state_dict({"head.weight": W, "head.bias": bias, "layer_log_weights": torch.from_numpy(lw["layer_log_weights"])})
    return probe


def kernel_streams(probe, B):
    """The residual stream behind every block as the last forward left it in the engine's workspace: L tensors (B, N, C) on the host."""
    enc = probe.encoder
    N = enc.patch_embed.num_patches + 1
    return [enc._engine.ws_tensor("x", l + 1, (B, N, enc.embed_dim)).clone().cpu() for l in range(enc.depth)]


@pytest.mark.parametrize("c", range(4))
def test_probe_against_reference_fixture_and_restatement(case, c):
    """(a) Features and logits against what the reference classifier computed, within the activation bound tests/test_gpu_probe.py has
    for the same bf16 encoder.  (b) Three train_steps, each against lw_ref.step_bounds fed the kernels' own pooled vectors and the
    parameters the step started from: pooled against the engine's own residual streams, _feat, logits, loss, dlogits-derived dW,
    dbias, dfeat and dlog_w, the reported norm against the gradient arena's, and the update against gpu_util.expected_update of the
    arena's before-state and its own gradient (rtol 1e-5, atol 1e-6: tests/test_gpu_epoch.py).  (c) layer_log_weights moves, the
    encoder keeps its bits, and a LinearProbe on the same encoder gives the bits it gave before."""
    from uncertainty_vit_amd.linear_probe import LinearProbe
    (fx, cfg, enc, W, bias, images, labels), lw = case
    use_cls, ln = COMBOS[c]
    lrate, wd, s = float(fx["lr"]), float(fx["weight_decay"]), float(fx["smoothing"])
    probe = fixture_lw_probe(case, c)
    lin = LinearProbe(probe.encoder, W.shape[0], smoothing=s)
    lin.load_state_dict({"head.weight": W, "head.bias": bias})
    xg, yg = images.cuda(), labels.cuda()
    B, K, Cd, Ln = images.shape[0], W.shape[0], cfg.embed_dim, cfg.depth
    lin_before = (lin.features(xg), lin.logits(xg))
    key = f"c{c}/"
    feat = probe.features(xg)
    torch.testing.assert_close(feat.cpu(), torch.from_numpy(lw[key + "features"]), rtol=ACT_RT, atol=ACT_AT)
    logits = probe.logits(xg)
    torch.testing.assert_close(logits.cpu(), torch.from_numpy(lw[key + "logits"]), rtol=ACT_RT, atol=ACT_AT)
    w = probe.layer_weights().cpu()
    within(w, lr.softmax_w(torch.from_numpy(lw["layer_log_weights"])), 1e-6, "layer_weights()")
    frozen = frozen_state(probe)
    lo = probe._lw_offset()
    for step in range(3):
        P0, M0, V0 = probe._arena.clone(), probe.exp_avg.clone(), probe.exp_avg_sq.clone()
        W0, b0, l0 = (t.detach().clone().cpu() for t in (probe.head.weight, probe.head.bias, probe.layer_log_weights))
        loss, gnorm = probe.train_step(xg, yg, lrate, wd)
        assert float(loss) == pytest.approx(float(lw[key + "step_loss"][step]), rel=5e-3)            # the bf16 encoder: tests/test_gpu_probe.py
        pooled = probe._pooled[:B].clone().cpu()
        xs = kernel_streams(probe, B)
        within(pooled, lr.pool(xs, 1 if use_cls else 0, ln), lr.pool_bound(xs, 1 if use_cls else 0, ln), f"combo {c} step {step} pooled")
        r, bd = lr.step_bounds(pooled, W0, b0, l0, labels, s)
        g = probe._grad_arena.clone()
        got = dict(feat=probe._feat[:B], logits=probe._logits[:B], dlogits=probe._dlogits[:B], dW=g[:K * Cd].view(K, Cd), dbias=g[K * Cd:K * Cd + K],
                   dfeat=probe._dfeat[:B], dlog_w=g[lo:lo + Ln])
        for name, t in got.items():
            within(t, r[name], bd[name], f"combo {c} step {step} {name}")
        assert abs(float(loss) - float(r["loss"])) <= bd["loss"]
        assert float(g[K * Cd + K:lo].abs().max()) == 0.0 and float(g[lo + Ln:].abs().sum()) == 0.0          # the pads hold no gradient
        assert float(gnorm) == pytest.approx(float(g.double().norm()), rel=1e-5)
        Pn, Mn, Vn, _, _ = expected_update(P0, M0, V0, P0, g, lrate, wd, None, step + 1, probe._n_decay, None, probe.BETAS, probe.EPS)
        torch.testing.assert_close(probe._arena.double().cpu(), Pn, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(probe.exp_avg.double().cpu(), Mn, rtol=1e-5, atol=1e-6 * float(Mn.abs().max()))
    sd = probe.state_dict()
    assert float((sd["layer_log_weights"].cpu() - torch.from_numpy(lw["layer_log_weights"])).abs().min()) > lrate          # three steps of lr
    assert all(torch.equal(a, b) for a, b in zip(frozen, frozen_state(probe)))
    assert torch.equal(lin.features(xg), lin_before[0]) and torch.equal(lin.logits(xg), lin_before[1])


def test_depth_four_through_the_module(L):
    """L = 4 on the tiny encoder of tests/test_gpu_mcd.py: features against lw_ref on the oracle's per-layer outputs (the activation
    bound of the bf16 encoder), in the four combinations; pooled against the engine's own streams within the pool's bound, which a
    pool that started at the embedding's output instead of block 0's would miss."""
    cfg = vo.VitConfig(init_values=0.1, img_size=48, embed_dim=128, depth=4, num_heads=2)
    model, sd = native_model(cfg)
    model.eval()
    x = closed_form_images("lw-d4", 3, cfg.img_size)
    log_w = torch.tensor([0.3, -0.6, 0.9, 0.1])
    with torch.no_grad():
        streams = vo.forward_features({k: v.clone() for k, v in sd.items()}, cfg, x, None, "end")
    assert len(streams) == 4
    for use_cls, ln in COMBOS:
        probe = lw_probe(model, 10, log_w=log_w, use_cls=use_cls, layernorm_before_combine=ln)
        feat = probe.features(x.cuda())
        ref = lr.combine(lr.pool(streams, 1 if use_cls else 0, ln), log_w)
        torch.testing.assert_close(feat.cpu().double(), ref, rtol=ACT_RT, atol=ACT_AT)
        xs = kernel_streams(probe, 3)
        within(probe._pooled[:3], lr.pool(xs, 1 if use_cls else 0, ln), lr.pool_bound(xs, 1 if use_cls else 0, ln), f"d4 pooled cls {use_cls} ln {ln}")
        assert not torch.equal(xs[0], model._engine.ws_tensor("x", 0, xs[0].shape).cpu())


def test_state_dict_round_trip(case):
    """Two steps, a checkpoint's three keys and optimizer state into a fresh probe, one more step on both: the same bits."""
    (fx, _, _, _, _, images, labels), _ = case
    a = fixture_lw_probe(case, 1)
    xg, yg = images.cuda(), labels.cuda()
    for _ in range(2):
        a.train_step(xg, yg, 1e-2, 0.05, 1.0)
    b = fixture_lw_probe(case, 1, encoder=a.encoder)
    b.load_state_dict({k: v.cpu() for k, v in a.state_dict().items()})
    b.load_optimizer_state_dict(a.optimizer_state_dict())
    assert sorted(a.state_dict()) == ["head.bias", "head.weight", "layer_log_weights"] and b.step_count == 2
    assert torch.equal(a._arena, b._arena) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    ra, rb = a.train_step(xg, yg, 1e-2, 0.05, 1.0), b.train_step(xg, yg, 1e-2, 0.05, 1.0)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and torch.equal(a._arena, b._arena)
    assert float(a.layer_log_weights.grad.abs().max()) > 0.0
    with pytest.raises(KeyError, match="layer_log_weights"):
        b.load_state_dict({k: v for k, v in a.state_dict().items() if k.startswith("head.")})


def test_post_hoc_families_read_the_mixed_feature(case):
    """evaluate(calibration, detection, OOD) beside a density, a bank and a ViM fit, the temperature and the conformal calibration on
    a LayerWeightedProbe: every figure equals that of a LinearProbe whose feature buffer is overwritten with the mixed feature of the
    same images -- the families read self._feat / self._logits and nothing of the pool."""
    from uncertainty_vit_amd.linear_probe import LinearProbe
    (fx, cfg, _, W, bias, _, _), _ = case
    probe = fixture_lw_probe(case, 1)
    with torch.no_grad():
        probe.head.weight.mul_(20.0)                       # logits of spread 1: the columns differ from sample to sample

    class Borrowed(LinearProbe):
        def _features(self, images):
            B = probe._features(images)
            self._buffers_for(B)
            self._feat[:B].copy_(probe._feat[:B])
            return B

    other = Borrowed(probe.encoder, W.shape[0], smoothing=float(fx["smoothing"]))
    other.load_state_dict({k: v.cpu() for k, v in probe.state_dict().items() if k.startswith("head.")})
    fit_b, eval_b = batches_of(cfg, "lw-fit", (5, 4, 3), K=W.shape[0]), batches_of(cfg, "lw-eval", (4, 3), K=W.shape[0])
    ood_b = batches_of(cfg, "lw-ood!", (3, 2), labelled=False)
    got = []
    for p in (probe, other):
        fits = [p.fit_density(fit_b), p.fit_neighbours(fit_b, k=3), p.fit_vim(fit_b, dim=4)]
        stats = p.evaluate(eval_b, calibration=True, detection=True, ood_loader=ood_b)
        fits.append(p.fit_temperature(fit_b))
        scaled = p.evaluate(eval_b, calibration=True, temperature=True)
        p.set_temperature(None)
        fits.append({k: v for k, v in p.fit_conformal(fit_b, alpha=0.2, score="aps").items() if not torch.is_tensor(v)})
        got.append((fits, stats, scaled, p.evaluate_conformal(eval_b)["conformal"]))
    for a, b in zip(*got):
        assert same(a, b)
    stats = got[0][1]
    assert stats["detection"]["columns"] == ["msp", "entropy", "energy", "maha", "rmaha", "knn", "vim", "residual"]
    assert stats["n"] == 7 and stats["detection"]["n_ood"] == 5 and np.isfinite(stats["ECE"]) and np.isfinite(stats["vim_mean"])
