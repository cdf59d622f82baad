"""GPU: the post-hoc last-layer K-FAC Laplace probe (csrc/laplace.hip, uncertainty-vit_amd/lap_probe.py) against the float64
restatement of tests/lap_ref.py on the same inputs.  Every bound is derived in lap_ref's docstring from the unit roundoff of the
double operations the kernels perform; tests/test_host_lap.py shows that the float64 reference itself stays within a quarter of
each.  Every test prints the worst |error| / bound before it asserts."""
import ctypes as C
import math
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

import lap_ref as lr
import probe_ref as pr
from oracle.closed_form import closed_form_images
from test_gpu_probe import GUARD, P, S, frozen_state, ok

pytestmark = pytest.mark.gpu

F64 = torch.float64
TAUS = (1e-4, 1.0, 1e4)


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def d64(v):
    return C.c_double(v)


def guarded64(n, fill=0.0):
    """n doubles of `fill` on the device followed by GUARD sentinels (7.5) that no kernel may touch."""
    t = torch.full((n + GUARD,), 7.5, device="cuda", dtype=F64)
    t[:n] = fill
    return t


def intact(t, n):
    return bool((t[n:] == 7.5).all())


def workspace(nbytes):
    return torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")


def run_factors(L, batches, Cd, K):
    """uvit_op_lap_factors over consecutive batches into the same accumulators; host float64 (A, G_sum, sums)."""
    D = Cd + 1
    A, G, sums = guarded64(D * D), guarded64(K * K), guarded64(3)
    for f, z, y in batches:
        B = f.shape[0]
        ws = workspace(L.uvit_op_lap_factors_ws_bytes(B, Cd, K))
        dev = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (f, z, y)]
        ok(L.uvit_op_lap_factors(P(dev[0]), P(dev[1]), z.shape[1], P(dev[2]), P(A), P(G), P(sums), P(ws), ws.numel(), B, Cd, K, S()))
    torch.cuda.synchronize()
    assert intact(A, D * D) and intact(G, K * K) and intact(sums, 3)
    return A[:D * D].view(D, D).cpu().numpy(), G[:K * K].view(K, K).cpu().numpy(), sums[:3].cpu().numpy()


@lru_cache(maxsize=None)
def fitted(shape):
    """Per shape, computed once: the two batches, the device's factors over them, lap_ref's factors and its eigh of the device's."""
    from uncertainty_vit_amd import native
    B, Cd, K = shape
    case = lr.make_case(B, Cd, K)
    A, G, sums = run_factors(native.lib(), case, Cd, K)
    ref = [lr.factors(*c) for c in case]
    for v in (A, G, sums):
        v.setflags(write=False)
    return {"case": case, "A": A, "G": G, "sums": sums, "ref": tuple(sum(r[i] for r in ref) for i in range(3)),
            "eig": lr.eig(A, G / sums[1])}


# ----------------------------------------------------------------------------------------------------------------------- factors
@pytest.mark.parametrize("shape", lr.SHAPES)
def test_factors(L, shape):
    """Two consecutive calls into the same A and G against lap_ref within the A, G and nll bounds; A and G symmetric bit for bit;
    a second run gives the same bits.  D = C + 1 is never a multiple of the tile: every tile edge is ragged."""
    B, Cd, K = shape
    fit = fitted(shape)
    fs, zs, ys = ([c[i] for c in fit["case"]] for i in range(3))
    A, G, sums = fit["A"], fit["G"], fit["sums"]
    A_ref, G_ref, sums_ref = fit["ref"]
    rA = np.abs(A - A_ref) / lr.bound_A(fs, zs, ys)
    rG = np.abs(G - G_ref) / lr.bound_G(zs, ys)
    rn = abs(sums[0] - sums_ref[0]) / lr.bound_nll(zs, ys)
    print(f"\nfactors {shape}: |error| / bound  A {rA.max():.3f}  G {rG.max():.3f}  nll {rn:.3f}")
    assert rA.max() <= 1.0 and rG.max() <= 1.0 and rn <= 1.0
    assert sums[1] == 2 * B and sums[2] == 0
    assert np.array_equal(A, A.T) and np.array_equal(G, G.T)
    again = run_factors(L, fit["case"], Cd, K)
    for a, b in zip((A, G, sums), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape", [(3, 8, 10), (130, 128, 100)])
def test_factors_leave_out_bad_rows(L, shape):
    """A row with a NaN logit and a row whose label is K are left out of everything and counted: A and G hold the bits of the call
    on the batch without the two rows (they add exact zeros to every chain), nll is within its bound, skipped == 2."""
    B, Cd, K = shape
    f, z, y = (v.copy() for v in lr.make_case(B, Cd, K, seed=1)[0])
    z[0, K // 2] = np.nan
    y[B - 1] = K
    A, G, sums = run_factors(L, [(f, z, y)], Cd, K)
    keep = lr.usable_rows(z, y)
    assert keep.sum() == B - 2
    A2, G2, sums2 = run_factors(L, [(f[keep], z[keep], y[keep])], Cd, K)
    assert A.tobytes() == A2.tobytes() and G.tobytes() == G2.tobytes()
    assert (sums[1], sums[2]) == (B - 2, 2) and (sums2[1], sums2[2]) == (B - 2, 0)
    A_ref, G_ref, sums_ref = lr.factors(f, z, y)
    rA = np.abs(A - A_ref) / lr.bound_A([f], [z], [y])
    rG = np.abs(G - G_ref) / lr.bound_G([z], [y])
    rn = abs(sums[0] - sums_ref[0]) / lr.bound_nll([z], [y])
    print(f"\nfactors with two bad rows {shape}: |error| / bound  A {rA.max():.3f}  G {rG.max():.3f}  nll {rn:.3f}")
    assert rA.max() <= 1.0 and rG.max() <= 1.0 and rn <= 1.0 and np.isfinite(A).all() and np.isfinite(G).all()


# ---------------------------------------------------------------------------------------------------------- prepare and variance
def run_prepare(L, UG, la, lg, tau, Cd, K):
    D = Cd + 1
    T = guarded64(D * K)
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (UG, la, lg)]
    ok(L.uvit_op_lap_prepare(P(dev[0]), P(dev[1]), P(dev[2]), d64(tau), P(T), Cd, K, S()))
    torch.cuda.synchronize()
    assert intact(T, D * K)
    return T


def run_variance(L, f, UA_dev, T_dev, Cd, K):
    B = f.shape[0]
    var, ws = guarded64(B * K, fill=-1.0), workspace(L.uvit_op_lap_variance_ws_bytes(B, Cd, K))
    ok(L.uvit_op_lap_variance(P(torch.from_numpy(f).cuda()), P(UA_dev), P(T_dev), P(var), P(ws), ws.numel(), B, Cd, K, S()))
    torch.cuda.synchronize()
    assert intact(var, B * K)
    return var[:B * K].view(B, K).cpu().numpy()


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("shape", lr.SHAPES)
def test_prepare_and_variance(L, shape, tau):
    """T against float64 to (K + 8) 2^-53 relative (all terms are non-negative); var against float64 on the device's T within the
    variance bound; two runs give the same bits.  The eigenvectors and eigenvalues are lap_ref's eigh of the device's factors."""
    B, Cd, K = shape
    D = Cd + 1
    fit = fitted(shape)
    la, UA, lg, UG = fit["eig"]
    T_dev = run_prepare(L, UG, la, lg, tau, Cd, K)
    T = T_dev[:D * K].view(D, K).cpu().numpy()
    T_ref = lr.t_matrix(UG, la, lg, tau)
    assert (T_ref > 0).all()
    rT = np.abs(T / T_ref - 1) / lr.bound_T_rel(K)
    UA_dev = torch.from_numpy(np.ascontiguousarray(UA)).cuda()
    f = fit["case"][0][0]
    var = run_variance(L, f, UA_dev, T_dev, Cd, K)
    rv = np.abs(var - lr.variance(f, UA, T)) / lr.bound_var(f, UA, T)
    print(f"\nprepare / variance {shape} tau {tau:g}: |error| / bound  T {rT.max():.3f}  var {rv.max():.3f}")
    assert rT.max() <= 1.0 and rv.max() <= 1.0 and (var >= 0).all()
    assert run_prepare(L, UG, la, lg, tau, Cd, K)[:D * K].cpu().numpy().tobytes() == T.tobytes()
    assert run_variance(L, f, UA_dev, T_dev, Cd, K).tobytes() == var.tobytes()


# ------------------------------------------------------------------------------------------------------------------------ probit
def run_probit(L, z, var, factor, alias, want_col=True, pad=0):
    B, K = z.shape
    ld = K + pad
    src = torch.full((B * ld + GUARD,), 7.5, device="cuda")
    src[:B * ld].view(B, ld)[:, :K] = torch.from_numpy(z).cuda()
    out = src if alias else torch.full((B * ld + GUARD,), 7.5, device="cuda")
    col = torch.full((B + GUARD,), 7.5, device="cuda")
    ok(L.uvit_op_lap_probit(P(src), ld, P(torch.from_numpy(var).cuda()), d64(factor), P(out), ld, P(col if want_col else None), B, K, S()))
    torch.cuda.synchronize()
    assert bool((out[B * ld:] == 7.5).all()) and bool((col[B:] == 7.5).all())
    if pad:
        assert bool((out[:B * ld].view(B, ld)[:, K:] == 7.5).all())
    return out[:B * ld].view(B, ld)[:, :K].cpu().numpy().copy(), col[:B].cpu().numpy().copy()


@pytest.mark.parametrize("shape", lr.SHAPES)
def test_probit(L, shape):
    """Within 2 fp32 ulp of the float64 value rounded to fp32 (the GP mean-field op's bound); factor 0 returns the input bits; the
    aliased and the separate output agree bit for bit, with a row stride above K as well; lap_var takes the lowest index on a
    constructed tie; a NaN variance turns that entry alone into NaN."""
    B, _, K = shape
    rng = np.random.default_rng(11 * B + K)
    z = (4.0 * rng.standard_normal((B, K))).astype(np.float32)
    var = rng.gamma(2.0, 1.5, size=(B, K))
    hi, lo = (K - 1, K // 2) if K > 2 else (1, 0)
    z[0, [lo, hi]] = np.float32(z[0].max() + 1.0)                    # row 0: the largest logit twice
    got, col = run_probit(L, z, var, lr.PROBIT, alias=False)
    want = lr.probit(z, var).astype(np.float32)
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print(f"\nprobit {shape}: worst error {ulps.max():.2f} ulp")
    assert ulps.max() <= 2.0
    assert np.array_equal(col, lr.lap_var(z, var).astype(np.float32)) and col[0] == np.float32(var[0, lo])
    for pad in (0, 3):
        a, ca = run_probit(L, z, var, lr.PROBIT, alias=True, pad=pad)
        b, cb = run_probit(L, z, var, lr.PROBIT, alias=False, pad=pad)
        assert a.tobytes() == b.tobytes() == got.tobytes() and ca.tobytes() == cb.tobytes() == col.tobytes()
    same, _ = run_probit(L, z, var, 0.0, alias=True, want_col=False)
    assert same.tobytes() == z.tobytes()
    bad = var.copy()
    bad[B - 1, K - 1] = np.nan
    nan, _ = run_probit(L, z, bad, lr.PROBIT, alias=False)
    mask = np.zeros((B, K), dtype=bool)
    mask[B - 1, K - 1] = True
    assert np.array_equal(np.isnan(nan), mask) and np.array_equal(nan[~mask], got[~mask])


# --------------------------------------------------------------------------------------------------------------- the module
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


def head_of(case):
    """A head with logits of a few units on the fixture's features (the fixture's own head is 1e-3 x N(0, 0.02): all logits alike)."""
    K, Cd = case[3].shape
    g = torch.Generator().manual_seed(77)
    return {"head.weight": 0.4 * torch.randn(K, Cd, generator=g), "head.bias": 0.1 * torch.randn(K, generator=g)}


def encoder_of(case):
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    _, cfg, enc = case[:3]
    model = VisionTransformerForCyclicalTraining(img_size=cfg.img_size, patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth,
                                                 num_heads=cfg.num_heads, norm_layer=partial(torch.nn.LayerNorm, eps=cfg.ln_eps),
                                                 init_values=cfg.init_values, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    model.load_state_dict(enc, strict=False)
    return model.cuda().eval()


def batches_of(case, tag, n=3):
    """n batches of 4 images as the prefetcher's items ((images, mask), labels on the host), labels drawn once per tag."""
    cfg, K = case[1], case[3].shape[0]
    rng = np.random.default_rng(len(tag))
    return [((closed_form_images(f"{tag}/{i}", 4, cfg.img_size).cuda(), None), torch.from_numpy(rng.integers(0, K, 4))) for i in range(n)]


@pytest.fixture(scope="module")
def world(case):
    """One encoder, a LinearProbe and a LaplaceProbe on the same head, fitted on 3 batches of 4 images; the device's own features
    and unscaled logits of the fit and evaluation images (from the LinearProbe), read once."""
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    enc = encoder_of(case)
    K = case[3].shape[0]
    plain, probe = LinearProbe(enc, K, smoothing=0.0), LaplaceProbe(enc, K, smoothing=0.0)
    plain.load_state_dict(head_of(case))
    probe.load_state_dict(head_of(case))
    fit_b, eval_b = batches_of(case, "lap-fit"), batches_of(case, "lap-eval!")
    plain.features(fit_b[0][0][0])                       # the first forward builds the engine and its bf16 shadows
    before = frozen_state(probe)
    rows = lambda bs: (np.concatenate([plain.features(x).cpu().numpy() for (x, _), _ in bs]),              # noqa: E731
                       np.concatenate([plain.logits(x).cpu().numpy() for (x, _), _ in bs]), np.concatenate([y.numpy() for _, y in bs]))
    unfitted = probe.evaluate(eval_b, calibration=True, detection=True)
    fit = probe.fit_laplace(fit_b, prior_precision=1.0)
    return {"case": case, "enc": enc, "plain": plain, "probe": probe, "before": before, "fit_b": fit_b, "eval_b": eval_b, "fit_rows": rows(fit_b),
            "eval_rows": rows(eval_b), "unfitted": unfitted, "fit": fit}


def same(a, b):
    """Equal stats, key for key, with equal floats (NaN equal to NaN)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b


def test_unfitted_probe_is_a_linear_probe(world):
    w = world
    want = w["plain"].evaluate(w["eval_b"], calibration=True, detection=True)
    print("\nunfitted:", {k: v for k, v in w["unfitted"].items() if k != "detection"})
    assert same(w["unfitted"], want) and "lap_var_mean" not in want and want["detection"]["columns"] == ["msp", "entropy", "energy"]
    fresh = type(w["probe"])(w["enc"], 10, smoothing=0.0)
    fresh.load_state_dict(head_of_world(w))
    assert same(fresh.evaluate(w["eval_b"]), w["plain"].evaluate(w["eval_b"]))
    x = w["eval_b"][0][0][0]
    assert torch.equal(fresh.logits(x), w["plain"].logits(x))


def head_of_world(w):
    return {k: v.detach().cpu().clone() for k, v in w["plain"].state_dict().items()}


def state_arrays(probe):
    st = probe._lap
    return [st[k].cpu().numpy() for k in ("UA", "T", "UG", "lam_a_dev", "lam_g_dev")]


def test_fit_and_predictive_variance(world):
    """The factors of the fit against lap_ref on the device's own features and logits; predictive_variance against lap_ref's
    eigen-form on the probe's own U_A and T within the variance bound, and against lap_ref's whole pipeline (its own eigh of the same
    factors) to 1e-9 relative: the two decompositions agree to D u |A| / tau, about 1e-13 here, on a variance that does not depend on
    the basis chosen inside an eigenspace."""
    w, probe = world, world["probe"]
    f, z, y = w["fit_rows"]
    fit, sd = w["fit"], probe.laplace_state_dict()
    assert (fit["n"], fit["n_skipped"], fit["prior_precision"], fit["on_grid_edge"]) == (12, 0, 1.0, False) and probe.laplace == fit
    A, G, sums = (sd[k].numpy() for k in ("A", "G_sum", "sums"))
    A_ref, G_ref, sums_ref = lr.factors(f, z, y)
    rA, rG = np.abs(A - A_ref) / lr.bound_A([f], [z], [y]), np.abs(G - G_ref) / lr.bound_G([z], [y])
    rn = abs(sums[0] - sums_ref[0]) / lr.bound_nll([z], [y])
    print(f"\nfit: |error| / bound  A {rA.max():.3f}  G {rG.max():.3f}  nll {rn:.3f}; nll {fit['nll']:.4f} log-marglik {fit['log_marglik']:.4f}")
    assert rA.max() <= 1 and rG.max() <= 1 and rn <= 1 and fit["nll"] == sums[0] and list(sums[1:]) == [12, 0]
    la, UA_ref, lg, UG_ref = lr.eig(A, G / 12)
    theta_sq = float(sum((v.double() ** 2).sum() for v in head_of_world(w).values()))
    assert fit["log_marglik"] == pytest.approx(lr.log_marglik(1.0, sums[0], theta_sq, la, lg), rel=1e-10)
    UA, T = state_arrays(probe)[:2]
    fe, ze, _ = w["eval_rows"]
    var = np.concatenate([probe.predictive_variance(x).cpu().numpy() for (x, _), _ in w["eval_b"]])
    assert var.dtype == np.float64 and var.shape == (12, 10)
    rv = np.abs(var - lr.variance(fe, UA, T)) / lr.bound_var(fe, UA, T)
    full = lr.variance(fe, UA_ref, lr.t_matrix(UG_ref, la, lg, 1.0))
    rel = np.abs(var / full - 1).max()
    print(f"predictive_variance: |error| / bound {rv.max():.3f}; against lap_ref's own eigh {rel:.2e} relative; mean {var.mean():.4f}")
    assert rv.max() <= 1.0 and rel <= 1e-9 and (var > 0).all()


def test_evaluate_on_the_probit_logits(world):
    """lap_var_mean is the mean of the fp32 column var[argmax z]; acc1, acc5 and loss are those of lap_ref's z~ (loss: 1e-5 relative,
    the fp32 cross-entropy op on fp32 logits against float64)."""
    w, probe = world, world["probe"]
    _, ze, ye = w["eval_rows"]
    var = np.concatenate([probe.predictive_variance(x).cpu().numpy() for (x, _), _ in w["eval_b"]])
    out = probe.evaluate(w["eval_b"])
    col = lr.lap_var(ze, var).astype(np.float32)
    assert out["lap_var_mean"] == pytest.approx(math.fsum(col.tolist()) / 12, rel=1e-12) and out["n"] == 12
    zt = torch.from_numpy(lr.probit(ze, var))
    y = torch.from_numpy(ye)
    assert pr.no_ties_among_top(zt)
    c1, c5 = pr.topk_counts(zt, y)
    _, loss, _ = pr.smoothed_ce(zt, y, 0.0)
    plain = w["plain"].evaluate(w["eval_b"])
    print(f"\nevaluate: loss {out['loss']:.5f} (linear {plain['loss']:.5f}), correct {out['correct1']}/{out['correct5']}, lap_var_mean {out['lap_var_mean']:.5f}")
    assert (out["correct1"], out["correct5"]) == (c1, c5) and out["loss"] == pytest.approx(float(loss), rel=1e-5)
    assert abs(out["loss"] - plain["loss"]) > 1e-3 * plain["loss"]                      # the link did change the logits
    x = w["eval_b"][0][0][0]
    got = probe.logits(x).cpu().numpy()
    want = lr.probit(ze[:4], var[:4]).astype(np.float32)
    assert np.abs(got - want).max() <= 2 * np.spacing(np.abs(want)).max()
    assert "lap_var_mean" not in probe.evaluate(w["eval_b"], variance=False)


def test_set_prior_precision_and_marglik(world):
    """Another tau re-runs uvit_op_lap_prepare alone: var is lap_ref's on the probe's own eigenvectors at the new tau (the variance
    bound plus T's relative bound), strictly below the variance at the smaller tau; 'marglik' returns a grid point."""
    w, probe = world, world["probe"]
    fe = w["eval_rows"][0][:4]
    x = w["eval_b"][0][0][0]
    v1 = probe.predictive_variance(x).cpu().numpy()
    info = probe.set_prior_precision(10.0)
    UA, T, UG, la, lg = state_arrays(probe)
    v10 = probe.predictive_variance(x).cpu().numpy()
    want = lr.variance(fe, UA, lr.t_matrix(UG, la, lg, 10.0))
    r = np.abs(v10 - want) / (lr.bound_var(fe, UA, T) + lr.bound_T_rel(10) * want)
    print(f"\ntau 1 -> 10: |error| / bound {r.max():.3f}; mean variance {v1.mean():.4f} -> {v10.mean():.4f}")
    assert r.max() <= 1.0 and (v10 < v1).all() and info["prior_precision"] == 10.0 and info["n"] == 12
    ml = probe.set_prior_precision("marglik")
    assert ml["prior_precision"] in lr.marglik_grid().tolist() and ml["on_grid_edge"] == (ml["prior_precision"] in (1e-4, 1e8))
    theta_sq = float(sum((v.double() ** 2).sum() for v in head_of_world(w).values()))
    tau, val, edge = lr.choose_prior_precision(ml["nll"], theta_sq, la, lg)
    assert (ml["prior_precision"], ml["on_grid_edge"]) == (tau, edge) and ml["log_marglik"] == pytest.approx(val, rel=1e-10)
    back = probe.set_prior_precision(1.0)
    assert back["prior_precision"] == 1.0 and probe.predictive_variance(x).cpu().numpy().tobytes() == v1.tobytes()


def test_state_round_trip_and_what_drops_the_fit(world):
    from uncertainty_vit_amd.native import UvitError
    w, probe = world, world["probe"]
    x, y = w["eval_b"][0][0][0], w["eval_b"][0][1].cuda()
    v = probe.predictive_variance(x)
    sd = probe.laplace_state_dict()
    assert set(sd) == {"A", "G_sum", "sums", "prior_precision", "head_sha256"} and list(probe.state_dict()) == ["head.weight", "head.bias"]
    fresh = type(probe)(w["enc"], 10, smoothing=0.0)
    fresh.load_state_dict(head_of_world(w))
    info = fresh.load_laplace_state(sd)
    assert info == probe.laplace and torch.equal(fresh.predictive_variance(x), v)                 # bit for bit
    other = type(probe)(w["enc"], 10, smoothing=0.0)
    head = head_of_world(w)
    head["head.bias"][3] += 1e-3
    other.load_state_dict(head)
    with pytest.raises(UvitError):
        other.load_laplace_state(sd)
    assert other.laplace is None
    fresh.train_step(x, y, 1e-3, 0.05)
    assert fresh.laplace is None and fresh.DETECT_COLUMNS == ("msp", "entropy", "energy")
    with pytest.raises(UvitError):
        fresh.predictive_variance(x)
    other.load_state_dict(head_of_world(w))
    other.set_laplace(sd)
    assert other.laplace == probe.laplace
    other.load_state_dict(head_of_world(w))                                                      # loading a head drops the fit
    assert other.laplace is None
    other.set_laplace(None)


def test_everything_downstream_runs_on_the_probit_logits(world):
    """Calibration, detection with the lap_var column, a temperature, conformal sets and stability run on z~ unchanged; the
    encoder's parameters and bf16 shadows keep their bits through all of the above."""
    w, probe = world, world["probe"]
    ood = [x for (x, _), _ in batches_of(w["case"], "lap-ood", 2)]
    out = probe.evaluate(w["eval_b"], calibration=True, detection=True, ood_loader=ood, temperature=2.0)
    det = out["detection"]
    assert det["columns"] == ["msp", "entropy", "energy", "lap_var"] and out["temperature"] == 2.0 and det["n_ood"] == 8
    assert all(math.isfinite(out[k]) for k in ("ECE", "TACE", "NLL", "lap_var_mean", "loss"))
    assert 0.0 <= det["ood"]["lap_var"]["AUROC"] <= 1.0 and set(det["misclassification"]["lap_var"]) == {"AUROC", "AUPR", "FPR95", "AURC"}
    # the column is the one evaluate() averages: the temperature does not reach it
    assert out["lap_var_mean"] == probe.evaluate(w["eval_b"])["lap_var_mean"]
    fit = probe.fit_conformal(w["fit_b"], alpha=0.2, score="aps")
    zt = torch.cat([probe.logits(x) for (x, _), _ in w["fit_b"]])
    yt = torch.cat([y for _, y in w["fit_b"]]).cuda()
    direct = probe.conformal_calibrate(zt, yt, alpha=0.2, score="aps")["table"].cpu()
    assert fit["qhat"][0] == float(direct[0, 1]) and fit["n"] == 12                             # calibrated on z~, bit for bit
    cp = probe.evaluate_conformal(w["eval_b"])["conformal"][0.2]
    assert cp["n"] == 12 and 0.0 <= cp["coverage"] <= 1.0 and 0.0 <= cp["size"] <= 10.0
    probe.set_conformal(None)
    ts = probe.fit_temperature(w["fit_b"])
    assert ts["n"] == 12 and math.isfinite(ts["T"])
    probe.set_temperature(None)
    frames = torch.cat([x for (x, _), _ in w["eval_b"]])[:8]
    st = probe.evaluate_stability([frames], 4, False, n_sequences=2)
    assert st["n_sequences"] == 2 and st["nan_sequences"] == 0
    for a, b in zip(w["before"], frozen_state(probe)):
        assert torch.equal(a, b)
