"""GPU: the random-feature Gaussian-process probe head (csrc/gp.hip, uncertainty-vit_amd/gp_probe.py) against float64 torch on the
same inputs (tests/gp_ref.py) and against what the reference's SNGP class computed (tests/golden/gp_head.npz).

Where a bound is "the fp32 CPU error", it is CPU_ERR below: torch's own fp32 CPU result against float64 on the inputs of the test,
(max-norm error / max|ref|, relative L2 error), measured once on the CPU and written here; the kernel is allowed 4 x that (the margin
for another summation order), as tests/test_gpu_probe.py does.  Every test prints what it measures before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import gp_ref as gr
import probe_ref as pr
from oracle.closed_form import closed_form_images
from test_gpu_probe import ACT_AT, ACT_RT, GUARD, P, S, f32, fixture_probe, frozen_state, guard_intact, guarded, metrics, ok, rnd

pytestmark = pytest.mark.gpu

F64 = torch.float64
RIDGE = gr.RIDGE


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def d64(v):
    return C.c_double(v)


def uni(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def guarded64(n, fill=7.5):
    return torch.full((n + GUARD,), fill, device="cuda", dtype=torch.float64)


# fp32 CPU error against float64 on the inputs below: {op: {shape or (shape, variant): {output: (max-norm / max|ref|, relative L2)}}}
# BEGIN CPU_ERR
CPU_ERR = {'features': {(1, 64, 64): {'ghat': (1.32e-07, 1.09e-07), 'u': (4.7e-08, 3.09e-08), 'phi': (3.07e-07, 1.44e-07)},
              (3, 128, 128): {'ghat': (1.23e-07, 9.35e-08), 'u': (6.44e-08, 3.29e-08), 'phi': (3.83e-07, 1.5e-07)},
              (5, 128, 260): {'ghat': (1.23e-07, 1.08e-07), 'u': (6.27e-08, 3.41e-08), 'phi': (3.83e-07, 1.45e-07)},
              (130, 64, 68): {'ghat': (1.28e-07, 9.3e-08), 'u': (8.55e-08, 3.11e-08), 'phi': (6.35e-07, 1.31e-07)},
              (7, 768, 768): {'ghat': (1.05e-07, 6.33e-08), 'u': (1.1e-07, 6.25e-08), 'phi': (8.18e-07, 2.44e-07)}},
 'precision': {(1, 64, 0.999, 'ridge'): {'P1': (9.17e-08, 5.61e-08), 'P3': (1.04e-07, 8.32e-08)},
               (3, 128, 0.999, 'ridge'): {'P1': (7.86e-08, 6.45e-08), 'P3': (1.35e-07, 8.66e-08)},
               (5, 260, 0.999, 'ridge'): {'P1': (7.84e-08, 6.97e-08), 'P3': (1.35e-07, 9.07e-08)},
               (70, 68, 0.999, 'ridge'): {'P1': (1.49e-07, 6.69e-08), 'P3': (2.05e-07, 9.25e-08)},
               (128, 768, 0.999, 'ridge'): {'P1': (1.76e-07, 1.41e-07), 'P3': (2.27e-07, 1.55e-07)},
               (1, 64, 0.0, 'ridge'): {'P1': (4.66e-08, 2.36e-08), 'P3': (9.27e-08, 4.28e-08)},
               (3, 128, 0.0, 'ridge'): {'P1': (7.49e-08, 3.55e-08), 'P3': (7.79e-08, 4.88e-08)},
               (5, 260, 0.0, 'ridge'): {'P1': (1e-07, 4.43e-08), 'P3': (1.03e-07, 5.61e-08)},
               (70, 68, 0.0, 'ridge'): {'P1': (2.31e-07, 1.34e-07), 'P3': (1.8e-07, 1.05e-07)},
               (128, 768, 0.0, 'ridge'): {'P1': (4.87e-07, 1.98e-07), 'P3': (2.48e-07, 1.78e-07)},
               (1, 64, 0.999, 'random'): {'P1': (8.39e-08, 6.01e-08), 'P3': (1.35e-07, 8.21e-08)},
               (3, 128, 0.999, 'random'): {'P1': (9.56e-08, 6.8e-08), 'P3': (1.08e-07, 8.73e-08)},
               (5, 260, 0.999, 'random'): {'P1': (1.03e-07, 7.34e-08), 'P3': (1.57e-07, 9.19e-08)},
               (70, 68, 0.999, 'random'): {'P1': (1.33e-07, 6.8e-08), 'P3': (1.93e-07, 8.99e-08)},
               (128, 768, 0.999, 'random'): {'P1': (2.04e-07, 1.38e-07), 'P3': (2.54e-07, 1.55e-07)},
               (1, 64, 0.0, 'random'): {'P1': (5.89e-08, 3.4e-08), 'P3': (8.33e-08, 4.47e-08)},
               (3, 128, 0.0, 'random'): {'P1': (9.83e-08, 4.33e-08), 'P3': (7.93e-08, 5.12e-08)},
               (5, 260, 0.0, 'random'): {'P1': (1.02e-07, 5.09e-08), 'P3': (8.87e-08, 5.77e-08)},
               (70, 68, 0.0, 'random'): {'P1': (2.58e-07, 1.33e-07), 'P3': (1.73e-07, 1.07e-07)},
               (128, 768, 0.0, 'random'): {'P1': (4.29e-07, 2e-07), 'P3': (2.93e-07, 1.78e-07)}},
 'ln_grad': {(1, 10, 64, 64): {'dgamma': (1.36e-07, 1.1e-07), 'dbeta': (1.33e-07, 1.12e-07)},
             (7, 200, 128, 260): {'dgamma': (4.57e-07, 4.24e-07), 'dbeta': (4.06e-07, 4.01e-07)},
             (128, 1000, 768, 768): {'dgamma': (5.93e-07, 5.06e-07), 'dbeta': (4.74e-07, 4.69e-07)}}}
# END CPU_ERR


def assert_within_4x(op, key, name, got, ref, cpu):
    m, now = metrics(got, ref), metrics(cpu, ref)
    lit = CPU_ERR[op][key][name]
    print(f"\n{op} {key} {name}: GPU (max-norm, rel L2) = ({m[0]:.3e}, {m[1]:.3e}); fp32 CPU here ({now[0]:.3e}, {now[1]:.3e}), recorded {lit}")
    assert m[0] <= 4 * lit[0] and m[1] <= 4 * lit[1], (op, key, name, m, lit)


# ------------------------------------------------------------------------------------------------------------------------ features
FEATURE_SHAPES = [(1, 64, 64), (3, 128, 128), (5, 128, 260), (130, 64, 68), (7, 768, 768)]
SCALE = 0.75


def feature_inputs(B, Cd, D):
    """Rows with mean 3 and standard deviation 2 (a kernel that skips the LayerNorm fails), gamma and beta away from (1, 0)."""
    return (3.0 + 2.0 * rnd(B, Cd, seed=31), 1.0 + 0.1 * rnd(Cd, seed=32), rnd(Cd, seed=33, scale=0.05), rnd(D, Cd, seed=34, scale=0.05),
            2.0 * math.pi * uni(D, seed=35))


def features_cpu(f, gamma, beta, W, b):
    """torch's fp32 CPU evaluation: (ghat, u, phi)."""
    Cd = f.shape[1]
    u = torch.nn.functional.layer_norm(f, (Cd,), gamma, beta, gr.LN_EPS) @ W.t() + b
    return torch.nn.functional.layer_norm(f, (Cd,), None, None, gr.LN_EPS), u, SCALE * torch.cos(u)


@pytest.mark.parametrize("B,Cd,D", FEATURE_SHAPES)
def test_gp_features(L, B, Cd, D):
    """ghat, u and phi against float64 within 4 x the fp32 CPU error; a tile edge in D (260, 68), B across a tile edge (130) and the
    production C (768) are in the list.  The call with NULL ghat and u gives the same phi bits, two runs give the same bits, and
    nothing is written behind an output."""
    f, gamma, beta, W, b = feature_inputs(B, Cd, D)
    ref = dict(zip(("ghat", "u", "phi"), gr.features(f, gamma, beta, W, b, SCALE)))
    cpu = dict(zip(("ghat", "u", "phi"), features_cpu(f, gamma, beta, W, b)))
    dev = [t.cuda() for t in (f, gamma, beta, W, b)]
    runs = []
    for keep in (True, True, False):
        ghat, u, phi = guarded(B * Cd), guarded(B * D), guarded(B * D)
        ok(L.uvit_op_gp_features(*[P(t) for t in dev], f32(SCALE), f32(gr.LN_EPS), P(ghat if keep else None), P(u if keep else None), P(phi),
                                 B, Cd, D, S()))
        torch.cuda.synchronize()
        assert guard_intact(ghat, B * Cd) and guard_intact(u, B * D) and guard_intact(phi, B * D)
        if not keep:
            assert bool((ghat == 7.5).all()) and bool((u == 7.5).all())
        runs.append({"ghat": ghat[:B * Cd].view(B, Cd).clone(), "u": u[:B * D].view(B, D).clone(), "phi": phi[:B * D].view(B, D).clone()})
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]) and torch.equal(runs[0]["phi"], runs[2]["phi"])
    for name in ("ghat", "u", "phi"):
        assert_within_4x("features", (B, Cd, D), name, runs[0][name], ref[name], cpu[name])


# ----------------------------------------------------------------------------------------------------------------------- precision
PRECISION_SHAPES = [(1, 64), (3, 128), (5, 260), (70, 68), (128, 768)]


def phi_like(B, D, seed):
    """What the feature op produces: the cosine of a phase spread over the circle."""
    return torch.cos(2.0 * math.pi * uni(B, D, seed=seed) + rnd(B, D, seed=seed + 1))


def precision_start(D, start):
    if start == "ridge":
        return (RIDGE * torch.eye(D, dtype=F64)).float()
    A = rnd(D, D, seed=41, scale=0.01)
    Pm = A @ A.t() / D + (RIDGE * torch.eye(D, dtype=F64)).float()
    return (Pm + Pm.t()) / 2                        # a + b == b + a: symmetric bit for bit


def precision_cpu(Pm, phi, m):
    M = phi.t() @ phi
    return m * Pm + (1.0 - m) * (M / phi.shape[0]) if m > 0 else Pm + M


@pytest.mark.parametrize("start", ["ridge", "random"])
@pytest.mark.parametrize("momentum", [0.999, 0.0])
@pytest.mark.parametrize("B,D", PRECISION_SHAPES)
def test_gp_precision_update(L, B, D, momentum, start):
    """One update and three successive updates (three different batches) against the restatement's within 4 x the fp32 CPU error;
    P == P.T bit for bit after each; two runs give the same bits; nothing is written behind P."""
    P0 = precision_start(D, start)
    assert torch.equal(P0, P0.t())
    phis = [phi_like(B, D, seed=50 + 3 * i) for i in range(3)]
    ref, cpu, refs, cpus = P0.double(), P0.clone(), [], []
    for ph in phis:
        ref, cpu = gr.precision_update(ref, ph, momentum), precision_cpu(cpu, ph, momentum)
        refs.append(ref)
        cpus.append(cpu)
    runs = []
    for _ in range(2):
        Pg = guarded(D * D)
        Pg[:D * D] = P0.flatten().cuda()
        out = []
        for ph in phis:
            phg = ph.cuda()
            ok(L.uvit_op_gp_precision_update(P(phg), P(Pg), B, D, d64(momentum), S()))
            torch.cuda.synchronize()
            assert guard_intact(Pg, D * D)
            out.append(Pg[:D * D].view(D, D).clone())
        runs.append(out)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    for i, name in ((0, "P1"), (2, "P3")):
        got = runs[0][i]
        assert torch.equal(got, got.t()), name
        assert_within_4x("precision", (B, D, momentum, start), name, got, refs[i], cpus[i])


# --------------------------------------------------------------------------------------------------------------------- LayerNorm grads
LN_GRAD_SHAPES = [(1, 10, 64, 64), (7, 200, 128, 260), (128, 1000, 768, 768)]


def ln_grad_inputs(B, K, Cd, D):
    return (rnd(B, K, seed=61, scale=1.0 / B), rnd(K, D, seed=62, scale=0.05), 2.0 * math.pi * uni(B, D, seed=63) + rnd(B, D, seed=64),
            rnd(D, Cd, seed=65, scale=0.05), rnd(B, Cd, seed=66))


def ln_grad_cpu(dz, W_out, u, W_rf, ghat):
    dg = (-SCALE * torch.sin(u) * (dz @ W_out)) @ W_rf
    return (dg * ghat).sum(0), dg.sum(0)


@pytest.mark.parametrize("B,K,Cd,D", LN_GRAD_SHAPES)
def test_gp_ln_grad(L, B, K, Cd, D):
    """dgamma and dbeta against float64 within 4 x the fp32 CPU error; the outputs held 5.0 before (they are overwritten, not added
    to), two runs give the same bits, nothing is written behind an output or behind the scratch the size call asks for."""
    dz, W_out, u, W_rf, ghat = ln_grad_inputs(B, K, Cd, D)
    ref = dict(zip(("dgamma", "dbeta"), gr.ln_grads(dz, W_out, u, W_rf, ghat, SCALE)))
    cpu = dict(zip(("dgamma", "dbeta"), ln_grad_cpu(dz, W_out, u, W_rf, ghat)))
    ws = L.uvit_op_gp_ln_grad_ws_bytes(B, Cd, D)
    assert ws == 4 * (B * D + B * Cd)
    dev = [t.cuda() for t in (dz, W_out, u, W_rf, ghat)]
    runs = []
    for _ in range(2):
        dgamma, dbeta, scratch = guarded(Cd, 5.0), guarded(Cd, 5.0), guarded(ws // 4)
        ok(L.uvit_op_gp_ln_grad(*[P(t) for t in dev], f32(SCALE), P(dgamma), P(dbeta), P(scratch), B, K, Cd, D, S()))
        torch.cuda.synchronize()
        assert guard_intact(dgamma, Cd, 5.0) and guard_intact(dbeta, Cd, 5.0) and guard_intact(scratch, ws // 4)
        runs.append({"dgamma": dgamma[:Cd].clone(), "dbeta": dbeta[:Cd].clone()})
    for name in ("dgamma", "dbeta"):
        assert torch.equal(runs[0][name], runs[1][name])
        assert_within_4x("ln_grad", (B, K, Cd, D), name, runs[0][name], ref[name], cpu[name])


# ------------------------------------------------------------------------------------------------------------------------ variance
@pytest.mark.parametrize("B,D", [(1, 64), (5, 260), (128, 768), (3, 2048)])
def test_gp_variance(L, B, D):
    """var = ridge phi_b^T Sigma phi_b in double for Sigma = inv(P), P made by three restatement updates of one row each (its
    condition number, about 1 + D / 2, is printed).
    Bound from the arithmetic: a double sum of D^2 <= 2^22 terms is within 2^22 x 2^-53 = 4.7e-10 of the sum of the terms'
    magnitudes, for the kernel and for the float64 reference alike: |var - ref| <= 1e-9 ridge sum_ij |phi_i Sigma_ij phi_j|.  Two runs give
    the same bits; nothing is written behind var."""
    Pm = gr.initial_precision(D)
    for i in range(3):
        Pm = gr.precision_update(Pm, phi_like(1, D, seed=70 + 3 * i))
    Sigma = torch.linalg.inv(Pm).contiguous()
    phi = phi_like(B, D, seed=81)
    ref = RIDGE * ((phi.double() @ Sigma) * phi.double()).sum(-1)
    bound = 1e-9 * gr.variance_magnitude(phi, Sigma, RIDGE)
    pg, sg = phi.cuda(), Sigma.cuda()
    runs = []
    for _ in range(2):
        var = guarded64(B)
        ok(L.uvit_op_gp_variance(P(pg), P(sg), d64(RIDGE), P(var), B, D, S()))
        torch.cuda.synchronize()
        assert bool((var[B:] == 7.5).all())
        runs.append(var[:B].clone())
    assert torch.equal(runs[0], runs[1])
    err = (runs[0].cpu() - ref).abs()
    print(f"\nvariance {(B, D)}: cond(P) {float(torch.linalg.cond(Pm)):.0f}, var in [{float(ref.min()):.4f}, {float(ref.max()):.4f}], "
          f"worst error / bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------------------------------- mean field
@pytest.mark.parametrize("B,K", [(3, 10), (5, 1003)])
def test_gp_mean_field(L, B, K):
    """Factor 0 returns the logits bit for bit; factor pi / 8 is within 2 ulp of the fp32 value of the float64 formula; the call
    whose output is its input gives what the other gives."""
    z = rnd(B, K, seed=91, scale=3.0)
    var = (0.05 + uni(B, seed=92)).double()
    zg, vg = z.cuda(), var.cuda()

    def run(factor, alias):
        src = guarded(B * K)
        src[:B * K] = zg.flatten()
        out = src if alias else guarded(B * K)
        ok(L.uvit_op_gp_mean_field(P(src), P(vg), d64(factor), P(out), B, K, S()))
        torch.cuda.synchronize()
        assert guard_intact(out, B * K) and guard_intact(src, B * K)
        if not alias:
            assert torch.equal(src[:B * K], zg.flatten())
        return out[:B * K].view(B, K).cpu()

    assert torch.equal(run(0.0, False), z) and torch.equal(run(0.0, True), z)
    got = run(math.pi / 8, False)
    assert torch.equal(run(math.pi / 8, True), got)
    want = gr.mean_field(z, var, math.pi / 8).float()
    ulp = torch.from_numpy(np.spacing(want.abs().numpy()))
    worst = float(((got - want).abs() / ulp).max())
    print(f"\nmean_field {(B, K)}: worst error {worst:.2f} ulp")
    assert worst <= 2.0 and not torch.equal(got, z)


# --------------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def gp_case(golden_dir):
    return gr.load_fixture(golden_dir)


GP_SD = {"gamma": "head._gp_input_normalize_layer.weight", "beta": "head._gp_input_normalize_layer.bias", "W_out": "head._gp_output_layer.weight",
         "W_rf": "head._random_feature.weight", "b_rf": "head._random_feature.bias"}


def gp_probe(case, gp_case, **kw):
    """GPProbe on the encoder of probe_t48.npz with the head of gp_head.npz on its arena, P = ridge * I."""
    from uncertainty_vit_amd.gp_probe import GPProbe
    fx, head, _, _ = gp_case
    enc_probe = fixture_probe(case)
    probe = GPProbe(enc_probe.encoder, head["W_out"].shape[0], smoothing=float(fx["smoothing"]), **kw)
    sd = {GP_SD[k]: v for k, v in head.items()}
    sd["head.precision_matrix"] = probe.state_dict()["head.precision_matrix"]
    probe.load_state_dict(sd)
    return probe


def feed_features(probe, feats):
    """Bypass the bf16 encoder: the head path reads these pooled features instead of the encoder's."""
    fg = feats.cuda()

    def _features(images):
        B = fg.shape[0]
        probe._buffers_for(B)
        probe._feat[:B].copy_(fg)
        return B
    probe._features = _features


def within(name, got, ref, dev):
    """max-norm error / max|ref| within 4 x the fp32 CPU error `dev` (for the fixture: the reference's own, stored by the generator)."""
    err = metrics(torch.as_tensor(got), torch.as_tensor(ref).double())[0]
    print(f"{name:12s} error {err:.3e}, fp32 CPU error {dev:.3e}")
    assert err <= 4 * dev, (name, err, dev)


def test_gp_probe_against_reference_fixture(case, gp_case):
    """The fixture's head on the probe's arena, the fixture's features fed straight into the head path: logits, loss, the three
    gradients, P after one and three steps and the parameters after three train_steps against gp_ref (pinned to the reference by
    tests/test_host_gp.py), each within 4 x the fp32 CPU error of that quantity -- the reference class's own deviation from float64
    on these inputs, stored in the fixture; predictive_variance within 4 x the stored deviation of the reference's diagonal."""
    fx, head, feats, labels = gp_case
    s, lr, wd = float(fx["smoothing"]), float(fx["lr"]), float(fx["weight_decay"])
    probe = gp_probe(case, gp_case)
    feed_features(probe, feats)
    dummy, yg = torch.zeros(1, device="cuda"), labels.cuda()
    D = probe.num_inducing
    loss_ref, dW, dgamma, dbeta, _, z = gr.grads(feats, head, labels, s)
    losses, _, Ps, h = gr.train_steps(feats, head, labels, s, lr, wd, 3)
    print()
    within("logits", probe.logits(dummy).cpu(), z, float(fx["dev/logits"]))
    assert torch.equal(probe._P.cpu(), (RIDGE * torch.eye(D, dtype=F64)).float())            # a forward outside training leaves P alone
    for step in range(3):
        loss, _ = probe.train_step(dummy, yg, lr, wd)
        assert abs(float(loss) - losses[step]) <= 4 * float(fx["dev/step_loss"]) * max(losses), (step, float(loss), losses[step])
        if step == 0:
            assert abs(float(loss) - float(loss_ref)) <= 4 * float(fx["dev/loss"]) * float(loss_ref)
            within("grad/W_out", probe.head._gp_output_layer.weight.grad.cpu(), dW, float(fx["dev/grad/W_out"]))
            within("grad/gamma", probe.head._gp_input_normalize_layer.weight.grad.cpu(), dgamma, float(fx["dev/grad/gamma"]))
            within("grad/beta", probe.head._gp_input_normalize_layer.bias.grad.cpu(), dbeta, float(fx["dev/grad/beta"]))
            within("P1", probe._P.cpu(), Ps[0], float(fx["dev/P1"]))
    within("P3", probe._P.cpu(), Ps[2], float(fx["dev/P3"]))
    assert torch.equal(probe._P, probe._P.t())
    sd = probe.state_dict()
    for k in ("W_out", "gamma", "beta"):
        within("post/" + k, sd[GP_SD[k]].cpu(), h[k], float(fx["dev/post/" + k]))
    _, _, phi3 = gr.features(feats, h["gamma"], h["beta"], head["W_rf"], head["b_rf"])
    var = probe.predictive_variance(dummy)
    assert var.dtype == torch.float64 and tuple(var.shape) == (feats.shape[0],)
    within("var", var.cpu(), gr.variance(phi3, Ps[2]), float(fx["dev/var"]))
    within("var (ref.)", var.cpu(), fx["var"], float(fx["dev/var"]))               # against the reference's own diagonal


def test_gp_probe_behind_the_encoder_and_frozen_state(case, gp_case):
    """With the fixture's encoder and images: logits and variance within the activation bound of tests/test_gpu_probe.py of the
    restatement on the float64 encoder features.  Every encoder parameter and bf16 shadow, W_rf and b_rf keep their bits through
    three train_steps; evaluate() and logits() leave P alone, train_step changes it, reset_cov() restores ridge * I exactly; the
    optimizer state round-trips."""
    fx, cfg, enc, _, _, images, labels = case
    _, head, _, _ = gp_case
    probe = gp_probe(case, gp_case)
    xg, yg = images.cuda(), labels.cuda()
    feats = pr.features(enc, cfg, images)
    _, _, phi = gr.features(feats, head["gamma"], head["beta"], head["W_rf"], head["b_rf"])
    z = probe.logits(xg)
    torch.testing.assert_close(z.cpu().double(), gr.logits(phi, head["W_out"]), rtol=ACT_RT, atol=ACT_AT)
    D = probe.num_inducing
    ridge_I = (RIDGE * torch.eye(D, dtype=F64)).float()
    var0 = probe.predictive_variance(xg)
    torch.testing.assert_close(var0.cpu(), gr.variance(phi, ridge_I), rtol=ACT_RT, atol=ACT_AT)
    before = frozen_state(probe) + [probe._w_rf.clone(), probe._b_rf.clone()]
    arena0 = probe._arena.clone()
    for _ in range(3):
        Pb = probe._P.clone()
        probe.train_step(xg, yg, 1e-3, 0.05)
        assert not torch.equal(Pb, probe._P)
    for a, b in zip(before, frozen_state(probe) + [probe._w_rf, probe._b_rf]):
        assert torch.equal(a, b)
    assert not torch.equal(arena0, probe._arena)
    # the variance under the updated P and head, against the restatement on the float64 features
    h = {"W_out": probe.head._gp_output_layer.weight.detach().cpu(), "gamma": probe.head._gp_input_normalize_layer.weight.detach().cpu(),
         "beta": probe.head._gp_input_normalize_layer.bias.detach().cpu()}
    _, _, phi3 = gr.features(feats, h["gamma"], h["beta"], head["W_rf"], head["b_rf"])
    var3 = probe.predictive_variance(xg)
    torch.testing.assert_close(var3.cpu(), gr.variance(phi3, probe._P.cpu()), rtol=ACT_RT, atol=ACT_AT)
    assert float((var3 - var0).abs().max()) > 0.1                      # inv(P) was formed again after the steps
    P3 = probe._P.clone()
    probe.evaluate([((xg, None), labels)], variance=True, mean_field=0.3)
    probe.logits(xg)
    assert torch.equal(P3, probe._P)
    osd = probe.optimizer_state_dict()
    assert osd["step"] == 3 and float(osd["exp_avg_sq"]["head._gp_input_normalize_layer.weight"].abs().max()) > 0
    m0 = probe.exp_avg.clone()
    probe.exp_avg.zero_()
    probe.load_optimizer_state_dict(osd)
    assert torch.equal(m0, probe.exp_avg)
    probe.reset_cov()
    assert torch.equal(probe._P.cpu(), ridge_I)
    assert probe.step_count == 3


def test_gp_evaluate_variance_mean_field_calibration_stability(case, gp_case):
    """evaluate(variance=True) over two batches of 4 and 3 images returns the restatement's mean variance (activation bound) and
    mean_field = 0 returns the same loss and counts as a call without it, bit for bit; mean_field > 0 moves the loss and leaves
    gp_var_mean alone; calibration_batch and stability_batch run on GP logits."""
    fx, cfg, enc, _, _, _, _ = case
    _, head, _, _ = gp_case
    probe = gp_probe(case, gp_case)
    warm = closed_form_images("gp-eval/train", 4, cfg.img_size).cuda()
    probe.train_step(warm, torch.tensor([0, 9, 3, 6], device="cuda"), 0.0, 0.0)          # lr 0: the head stays, P takes one batch
    Pm = probe._P.cpu()
    batches, vs = [], []
    for i, n in enumerate((4, 3)):
        x = closed_form_images(f"gp-eval/{i}", n, cfg.img_size)
        _, _, phi = gr.features(pr.features(enc, cfg, x), head["gamma"], head["beta"], head["W_rf"], head["b_rf"])
        vs.append(gr.variance(phi, Pm))
        batches.append(((x.cuda(), None), torch.arange(n) % 10))
    want = float(torch.cat(vs).mean())
    plain = probe.evaluate(batches)
    out = probe.evaluate(batches, variance=True, mean_field=0.0)
    print(f"\ngp_var_mean {out['gp_var_mean']:.6f}, restatement {want:.6f}")
    assert out["n"] == 7 and "gp_var_mean" not in plain
    assert out["gp_var_mean"] == pytest.approx(want, rel=ACT_RT, abs=ACT_AT)
    assert {k: out[k] for k in plain} == plain
    mf = probe.evaluate(batches, calibration=True, variance=True, mean_field=0.4)
    assert mf["gp_var_mean"] == out["gp_var_mean"] and mf["loss"] != out["loss"] and math.isfinite(mf["ECE"])
    assert torch.equal(probe._P.cpu(), Pm)
    z = probe.logits(batches[0][0][0])
    ece, tace, nll, auroc = probe.calibration_batch(z, torch.arange(4, device="cuda"))
    assert all(math.isfinite(float(v)) for v in (ece, tace, nll))
    seq = probe.stability_batch(z, 2, False)
    assert tuple(seq.shape) == (2, 3) and bool(torch.isfinite(seq).all())


def test_linear_probe_beside_the_gp_module(L, case):
    """A plain LinearProbe built after the GP module was imported: logits, train_step and evaluate return the bits of the existing ops
    called directly on its features."""
    import uncertainty_vit_amd.gp_probe  # noqa: F401
    fx, cfg, enc, W, bias, images, labels = case
    probe = fixture_probe(case)
    xg, yg = images.cuda(), labels.cuda()
    B, K, Cd = images.shape[0], W.shape[0], cfg.embed_dim
    feat = probe.features(xg)
    Wg, bg = W.cuda(), bias.cuda()
    z, dz, rows, loss, cnt = (torch.zeros(B, K, device="cuda"), torch.zeros(B, K, device="cuda"), torch.zeros(B, device="cuda"),
                              torch.zeros(1, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))
    ok(L.uvit_op_probe_logits(P(feat), P(Wg), P(bg), P(z), B, K, Cd, S()))
    assert torch.equal(probe.logits(xg), z)
    ok(L.uvit_op_probe_ce(P(z), P(yg), f32(0.0), None, P(rows), P(loss), P(cnt), B, K, S()))
    ev = probe.evaluate([((xg, None), labels)])
    assert sorted(ev) == ["acc1", "acc5", "correct1", "correct5", "loss", "n"]
    assert ev["loss"] == float(loss) and [ev["correct1"], ev["correct5"]] == cnt.tolist()
    ok(L.uvit_op_probe_ce(P(z), P(yg), f32(probe.smoothing), P(dz), P(rows), P(loss), None, B, K, S()))
    dW, db = torch.zeros(K, Cd, device="cuda"), torch.zeros(K, device="cuda")
    ok(L.uvit_op_probe_head_grad(P(dz), P(feat), P(dW), P(db), B, K, Cd, S()))
    got_loss, _ = probe.train_step(xg, yg, 1e-3, 0.05)
    assert float(got_loss) == float(loss)
    assert torch.equal(probe.head.weight.grad, dW) and torch.equal(probe.head.bias.grad, db)
    assert [n for n, _ in probe.named_parameters()] == ["head.weight", "head.bias"]
