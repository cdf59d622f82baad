"""GPU: the heteroscedastic probe head (csrc/het.hip, uncertainty-vit_amd/het_probe.py) against the float64 restatement of
tests/het_ref.py on the same inputs and the same counter-based draws.

Tolerance: CPU_ERR below is the error of torch's fp32 CPU evaluation of het_ref's formulas against their float64 form on the inputs
of the test, (max-norm error / max|ref|, relative L2 error), measured once on the CPU (`PYTHONPATH=. python tests/test_gpu_het.py` prints the table)
and written here; the kernel is allowed 4 x that -- the margin for another summation order and the device's logf / cosf / expf -- as
tests/test_gpu_gp.py does.  Inputs are chosen so that no p[b, k] lies in [eps / 2, 2 eps] (asserted on the float64 p): the clamp
takes the same branch in both precisions; the clamp has a case of its own.  Every test prints what it measures before it asserts."""
import math

import pytest
import torch

import het_ref as hr
import probe_ref as pr
from test_gpu_probe import P, S as STREAM, f32, fixture_probe, guard_intact, guarded, metrics, ok, rnd

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = hr.EPS
SEED = 42


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


# (B, S, K, R): K and R odd in places, so the last Box-Muller pair is half used
NOISE_SHAPES = [(1, 1, 3, 1), (2, 5, 67, 3), (3, 130, 130, 10), (1, 4, 1000, 10)]
# (B, S, K, R, T).  The partition of the samples is chunks of 64 ceil(S / 512): S = 128 ends on a chunk edge, 129 is one past it, 130
# has a last chunk of two; K = 67, 130, 1000 and 1030 take the four class widths the kernels are instantiated for (128, 512, 1024,
# 4096); at (2, 4, 600, 32) K R is above the 16384 floats of V the kernels keep in LDS (V is read from memory) and the backward's dV
# sums take two factor tiles (27 + 5)
MC_CASES = [(1, 1, 3, 1, 1.0), (3, 5, 10, 3, 0.5), (2, 64, 67, 1, 1.0), (5, 130, 130, 10, 1.0), (5, 128, 130, 10, 1.0), (5, 129, 130, 10, 1.0),
            (2, 16, 1000, 10, 1.0), (2, 4, 600, 32, 1.0), (1, 3, 1030, 2, 1.0)]
MODEL_CASE = dict(K=10, R=3, S=40, lr=1e-3, wd=0.05)

# fp32 CPU error against float64: {op: {case: {output: (max-norm / max|ref|, relative L2)}}}
# BEGIN CPU_ERR
CPU_ERR = {'noise': {(1, 1, 3, 1): {'epsR': (2.17e-08, 2.17e-08), 'epsK': (1.1e-07, 1.16e-07)},
           (2, 5, 67, 3): {'epsR': (2.36e-07, 1.28e-07), 'epsK': (2.51e-07, 1.38e-07)},
           (3, 130, 130, 10): {'epsR': (3.57e-07, 1.5e-07), 'epsK': (3.13e-07, 1.45e-07)},
           (1, 4, 1000, 10): {'epsR': (2.23e-07, 1.12e-07), 'epsK': (2.24e-07, 1.46e-07)}},
 'forward': {((1, 1, 3, 1, 1.0), 0): {'z': (1.19e-07, 1.19e-07), 'p': (4.99e-08, 6.47e-08), 'pvar': (0.0, 0.0)},
             ((1, 1, 3, 1, 1.0), 1): {'z': (1.19e-07, 1.19e-07), 'p': (4.99e-08, 6.47e-08), 'pvar': (0.0, 0.0)},
             ((3, 5, 10, 3, 0.5), 0): {'z': (6.02e-08, 4.88e-08), 'p': (2.15e-07, 1.28e-07), 'pvar': (7.03e-07, 4.48e-07)},
             ((3, 5, 10, 3, 0.5), 1): {'z': (6.53e-08, 4.36e-08), 'p': (2e-07, 1.39e-07), 'pvar': (3.91e-07, 3.1e-07)},
             ((2, 64, 67, 1, 1.0), 0): {'z': (3.92e-08, 2.8e-08), 'p': (5.83e-08, 5.69e-08), 'pvar': (2.87e-07, 2.3e-07)},
             ((2, 64, 67, 1, 1.0), 1): {'z': (3.52e-08, 2.82e-08), 'p': (6.93e-08, 5.39e-08), 'pvar': (1.33e-07, 1.25e-07)},
             ((5, 130, 130, 10, 1.0), 0): {'z': (4.67e-08, 2.87e-08), 'p': (1.25e-07, 9.17e-08), 'pvar': (2.39e-07, 2.25e-07)},
             ((5, 130, 130, 10, 1.0), 1): {'z': (5.15e-08, 2.88e-08), 'p': (1.72e-07, 9.05e-08), 'pvar': (2.14e-07, 1.97e-07)},
             ((5, 128, 130, 10, 1.0), 0): {'z': (4.87e-08, 2.88e-08), 'p': (1.02e-07, 7.94e-08), 'pvar': (2.41e-07, 2.1e-07)},
             ((5, 128, 130, 10, 1.0), 1): {'z': (5.04e-08, 2.81e-08), 'p': (1.54e-07, 8.33e-08), 'pvar': (1.86e-07, 2.11e-07)},
             ((5, 129, 130, 10, 1.0), 0): {'z': (5.36e-08, 2.85e-08), 'p': (1.02e-07, 7.97e-08), 'pvar': (2.7e-07, 2.61e-07)},
             ((5, 129, 130, 10, 1.0), 1): {'z': (5.03e-08, 2.72e-08), 'p': (1.74e-07, 9.39e-08), 'pvar': (2.31e-07, 2.33e-07)},
             ((2, 16, 1000, 10, 1.0), 0): {'z': (7.21e-08, 3.03e-08), 'p': (2.16e-07, 1.55e-07), 'pvar': (6.13e-07, 5.97e-07)},
             ((2, 16, 1000, 10, 1.0), 1): {'z': (9.04e-08, 3.05e-08), 'p': (2.65e-07, 1.93e-07), 'pvar': (1.03e-06, 7.96e-07)},
             ((2, 4, 600, 32, 1.0), 0): {'z': (1.04e-07, 3.6e-08), 'p': (2.73e-07, 2.12e-07), 'pvar': (5.24e-07, 4.26e-07)},
             ((2, 4, 600, 32, 1.0), 1): {'z': (1.04e-07, 3.45e-08), 'p': (2.73e-07, 1.95e-07), 'pvar': (5.47e-07, 4.39e-07)},
             ((1, 3, 1030, 2, 1.0), 0): {'z': (7.48e-08, 3.15e-08), 'p': (1.24e-07, 1.38e-07), 'pvar': (7.74e-07, 6.93e-07)},
             ((1, 3, 1030, 2, 1.0), 1): {'z': (7.48e-08, 3.15e-08), 'p': (1.24e-07, 1.38e-07), 'pvar': (7.74e-07, 6.93e-07)},
             ('clamp', 0): {'z': (1.57e-08, 1.92e-08)}},
 'backward': {((1, 1, 3, 1, 1.0), 0): {'dlin': (2.8e-07, 2.45e-07)},
              ((1, 1, 3, 1, 1.0), 1): {'dlin': (2.8e-07, 2.45e-07)},
              ((3, 5, 10, 3, 0.5), 0): {'dlin': (4.24e-07, 3.45e-07)},
              ((3, 5, 10, 3, 0.5), 1): {'dlin': (4.15e-07, 2.52e-07)},
              ((2, 64, 67, 1, 1.0), 0): {'dlin': (1.21e-07, 1.13e-07)},
              ((2, 64, 67, 1, 1.0), 1): {'dlin': (1.21e-07, 1.09e-07)},
              ((5, 130, 130, 10, 1.0), 0): {'dlin': (2.93e-07, 2.34e-07)},
              ((5, 130, 130, 10, 1.0), 1): {'dlin': (3.06e-07, 1.91e-07)},
              ((5, 128, 130, 10, 1.0), 0): {'dlin': (2.71e-07, 1.76e-07)},
              ((5, 128, 130, 10, 1.0), 1): {'dlin': (2.62e-07, 1.85e-07)},
              ((5, 129, 130, 10, 1.0), 0): {'dlin': (3.38e-07, 2.09e-07)},
              ((5, 129, 130, 10, 1.0), 1): {'dlin': (3.68e-07, 1.97e-07)},
              ((2, 16, 1000, 10, 1.0), 0): {'dlin': (4.25e-07, 3.32e-07)},
              ((2, 16, 1000, 10, 1.0), 1): {'dlin': (4.25e-07, 3.05e-07)},
              ((2, 4, 600, 32, 1.0), 0): {'dlin': (4.46e-07, 2.85e-07)},
              ((2, 4, 600, 32, 1.0), 1): {'dlin': (2.73e-07, 2.26e-07)},
              ((1, 3, 1030, 2, 1.0), 0): {'dlin': (9.87e-08, 8.67e-08)},
              ((1, 3, 1030, 2, 1.0), 1): {'dlin': (9.87e-08, 8.67e-08)},
              ('clamp', 0): {'dlin': (1.28e-07, 1.16e-07)}},
 'step': {'model': {'z': (5.59e-08, 4.1e-08), 'dW': (1.88e-07, 1.51e-07), 'dbias': (2.41e-07, 1.66e-07)}}}
# END CPU_ERR


def assert_within_4x(op, key, name, got, ref):
    m, lit = metrics(got, ref), CPU_ERR[op][key][name]
    print(f"\n{op} {key} {name}: GPU (max-norm, rel L2) = ({m[0]:.3e}, {m[1]:.3e}); fp32 CPU recorded {lit}")
    assert m[0] <= 4 * lit[0] and m[1] <= 4 * lit[1], (op, key, name, m, lit)


# ------------------------------------------------------------------------------------------------------------------------ inputs
def mc_inputs(B, S, K, R):
    """lin (B, K (R + 2)) fp32: loc of spread 1, draw of spread 0.7 with both signs, V of spread 1 / sqrt(R): the diagonal and the
    factor term are each of the order of the spread of loc, so a kernel that drops one fails."""
    return torch.cat([rnd(B, K, seed=101), rnd(B, K, seed=102, scale=0.7), rnd(B, K * R, seed=103, scale=1.0 / math.sqrt(R))], dim=1)


def mc_reference(B, S, K, R, T, share, dtype=F64):
    """(z, p, pvar, dz, dlin) of het_ref in `dtype`.  dz is the smoothed cross-entropy's gradient at the float64 z, rounded to fp32;
    the backward reads the float64 p rounded to fp32, in both precisions and on the GPU: its error is the backward's own."""
    lin = mc_inputs(B, S, K, R)
    e64 = hr.noise(B, S, K, R, SEED, share)
    z64, p64, _, _ = hr.forward(lin, *e64, K, R, T)
    assert not bool(((p64 >= EPS / 2) & (p64 <= 2 * EPS)).any()), "a p at the clamp's edge"
    labels = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(104))
    dz = pr.smoothed_ce(z64, labels, 0.1)[2].float()
    p32 = p64.float()
    eps = hr.noise(B, S, K, R, SEED, share, dtype)
    z, p, pvar, _ = hr.forward(lin, *eps, K, R, T, EPS, dtype)
    return z, p, pvar, dz, p32, hr.backward(lin, p32, dz, *eps, K, R, T, EPS, dtype)


_REF = {}


def reference(case, share):
    if (case, share) not in _REF:
        _REF[(case, share)] = mc_reference(*case, share)
    return _REF[(case, share)]


# ------------------------------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("B,S,K,R", NOISE_SHAPES)
def test_het_noise(L, B, S, K, R):
    """epsR and epsK against the restatement within 4 x the fp32 CPU error; with share = 1 every row equals row 0 of share = 0; a NULL
    output is left alone; nothing is written behind an output; two runs give the same bits."""
    ref = dict(zip(("epsR", "epsK"), hr.noise(B, S, K, R, SEED, 0)))

    def run(share, wantR=True, wantK=True):
        eR, eK = guarded(B * S * R), guarded(B * S * K)
        ok(L.uvit_op_het_noise(P(eR if wantR else None), P(eK if wantK else None), B, S, K, R, SEED, share, STREAM()))
        torch.cuda.synchronize()
        assert guard_intact(eR, B * S * R) and guard_intact(eK, B * S * K)
        if not wantR:
            assert bool((eR == 7.5).all())
        if not wantK:
            assert bool((eK == 7.5).all())
        return eR[:B * S * R].view(B, S, R).clone(), eK[:B * S * K].view(B, S, K).clone()

    a, b = run(0), run(0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(run(0, wantK=False)[0], a[0]) and torch.equal(run(0, wantR=False)[1], a[1])
    sh = run(1)
    for row in range(B):
        assert torch.equal(sh[0][row], a[0][0]) and torch.equal(sh[1][row], a[1][0])
    assert float(a[1].abs().max()) <= 5.8
    assert_within_4x("noise", (B, S, K, R), "epsR", a[0], ref["epsR"])
    assert_within_4x("noise", (B, S, K, R), "epsK", a[1], ref["epsK"])


# ------------------------------------------------------------------------------------------------------------- forward and backward
def run_forward(L, lin_g, B, S, K, R, T, share, seed=SEED, want=True):
    ws = L.uvit_op_het_mc_ws_bytes(B, S, K, R)
    assert ws == -(-S // hr.chunk_size(S)) * B * K * (R + 2) * 4
    z, p, pvar, scratch = guarded(B * K), guarded(B * K), guarded(B * K), guarded(ws // 4)
    ok(L.uvit_op_het_mc_forward(P(lin_g), P(z if want else None), P(p), P(pvar if want else None), P(scratch), B, S, K, R, f32(T), f32(EPS),
                                seed, share, STREAM()))
    torch.cuda.synchronize()
    assert guard_intact(z, B * K) and guard_intact(p, B * K) and guard_intact(pvar, B * K) and guard_intact(scratch, ws // 4)
    if not want:
        assert bool((z == 7.5).all()) and bool((pvar == 7.5).all())
    return {n: t[:B * K].view(B, K).clone() for n, t in (("z", z), ("p", p), ("pvar", pvar))}


def run_backward(L, lin_g, p_g, dz_g, B, S, K, R, T, share, seed=SEED):
    ws, n = L.uvit_op_het_mc_ws_bytes(B, S, K, R), B * K * (R + 2)
    dlin, scratch = guarded(n, 5.0), guarded(ws // 4)
    ok(L.uvit_op_het_mc_backward(P(lin_g), P(p_g), P(dz_g), P(dlin), P(scratch), B, S, K, R, f32(T), f32(EPS), seed, share, STREAM()))
    torch.cuda.synchronize()
    assert guard_intact(dlin, n, 5.0) and guard_intact(scratch, ws // 4)
    return dlin[:n].view(B, K * (R + 2)).clone()


@pytest.mark.parametrize("share", [0, 1])
@pytest.mark.parametrize("case", MC_CASES)
def test_het_mc_forward(L, case, share):
    """z, p and pvar against float64 within 4 x the fp32 CPU error; the call with NULL z and pvar gives the same p bits; two runs
    give the same bits; nothing is written behind an output or behind the scratch the size call asks for; sum_k p = 1 to 1e-5."""
    B, S, K, R, T = case
    z, p, pvar, _, _, _ = reference(case, share)
    lin_g = mc_inputs(B, S, K, R).cuda()
    a, b = run_forward(L, lin_g, B, S, K, R, T, share), run_forward(L, lin_g, B, S, K, R, T, share)
    assert all(torch.equal(a[n], b[n]) for n in a)
    assert torch.equal(run_forward(L, lin_g, B, S, K, R, T, share, want=False)["p"], a["p"])
    total = float((a["p"].double().sum(-1) - 1).abs().max())
    print(f"\nforward {case} share {share}: |sum_k p - 1| {total:.2e}, p in [{float(p.min()):.2e}, {float(p.max()):.3f}]")
    assert total <= 1e-5
    assert bool((a["pvar"] >= 0).all())
    assert not torch.equal(run_forward(L, lin_g, B, S, K, R, T, share, seed=SEED + 1)["p"], a["p"])
    if S == 1:      # one sample: the variance is 0 in exact arithmetic; the device's y^2 and p^2 differ by one rounding of a square <= 1
        print(f"pvar at S = 1: max {float(a['pvar'].max()):.2e}")
        assert float(pvar.abs().max()) == 0.0 and float(a["pvar"].max()) <= 2.0 ** -23
    for name, ref in (("z", z), ("p", p)) + ((("pvar", pvar),) if S > 1 else ()):
        assert_within_4x("forward", (case, share), name, a[name], ref)


@pytest.mark.parametrize("share", [0, 1])
@pytest.mark.parametrize("case", MC_CASES)
def test_het_mc_backward(L, case, share):
    """dlin against float64 within 4 x the fp32 CPU error; dlin held 5.0 before (it is overwritten); two runs give the same bits;
    guards intact; each row of dloc sums to 0 within K x the bound of one element; with the draws of another seed dlin is far from
    the reference (relative L2 above 0.1): the seed reaches the backward as it reaches the forward."""
    B, S, K, R, T = case
    _, _, _, dz, p32, dlin = reference(case, share)
    lin_g, p_g, dz_g = mc_inputs(B, S, K, R).cuda(), p32.cuda(), dz.cuda()
    a, b = run_backward(L, lin_g, p_g, dz_g, B, S, K, R, T, share), run_backward(L, lin_g, p_g, dz_g, B, S, K, R, T, share)
    assert torch.equal(a, b)
    lit = CPU_ERR["backward"][(case, share)]["dlin"]
    rowsum, bound = float(a[:, :K].double().sum(1).abs().max()), K * 4 * lit[0] * float(dlin.abs().max())
    other = metrics(run_backward(L, lin_g, p_g, dz_g, B, S, K, R, T, share, seed=SEED + 1), dlin)
    print(f"\nbackward {case} share {share}: |sum_k dloc| {rowsum:.2e} (bound {bound:.2e}); another seed: rel L2 {other[1]:.3f}")
    assert rowsum <= bound
    assert other[1] > 0.1
    assert_within_4x("backward", (case, share), "dlin", a, dlin)


def test_het_clamp(L):
    """Classes with loc = -60: p is below eps / 2 on the device as in float64, z is log(eps) there (the bound of the forward, and one
    value bit for bit), a dz that is non-zero only at those classes gives a dlin of exact zeros, and a full dz gives dlin within the
    bound."""
    case, share = (2, 8, 10, 2, 1.0), 0
    B, S, K, R, T = case
    lin = mc_inputs(B, S, K, R)
    lin[:, [3, 7]] = -60.0
    eps = hr.noise(B, S, K, R, SEED, share)
    z, p, _, _ = hr.forward(lin, *eps, K, R, T)
    assert float(p[:, [3, 7]].max()) < EPS / 2 and float(p[:, [0, 1, 2, 4, 5, 6, 8, 9]].min()) > 2 * EPS
    lin_g = lin.cuda()
    out = run_forward(L, lin_g, B, S, K, R, T, share)
    zc = out["z"][:, [3, 7]]
    print(f"\nclamp: device p {float(out['p'][:, [3, 7]].max()):.3e}, z {float(zc[0, 0]):.6f}, log(eps) {math.log(EPS):.6f}")
    assert float(out["p"][:, [3, 7]].max()) < EPS / 2 and bool((zc == zc[0, 0]).all())
    assert_within_4x("forward", ("clamp", share), "z", out["z"], z)
    only = torch.zeros(B, K)
    only[:, [3, 7]] = 1.0
    assert float(run_backward(L, lin_g, out["p"], only.cuda(), B, S, K, R, T, share).abs().max()) == 0.0
    dz = rnd(B, K, seed=105, scale=1.0 / B)
    ref = hr.backward(lin, p.float(), dz, *eps, K, R, T)
    assert_within_4x("backward", ("clamp", share), "dlin", run_backward(L, lin_g, p.float().cuda(), dz.cuda(), B, S, K, R, T, share), ref)


# --------------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


def het_probe(case, **kw):
    """HetProbe on the encoder of probe_t48.npz, its head drawn under seed 5."""
    from uncertainty_vit_amd.het_probe import HetProbe
    fx = case[0]
    enc = fixture_probe(case).encoder
    torch.manual_seed(5)
    m = MODEL_CASE
    return HetProbe(enc, m["K"], smoothing=float(fx["smoothing"]), num_factors=m["R"], train_mc_samples=m["S"], test_mc_samples=m["S"], **kw)


def head_of(probe):
    """(W (K (R + 2), C), bias) of the arena, on the host."""
    n, rows = probe._n_decay, probe._rows
    return probe._arena[:n].view(rows, probe.embed_dim).cpu().clone(), probe._arena[n:n + rows].cpu().clone()


def test_het_probe_train_step_against_het_ref(case):
    """One train_step's loss and gradient arena against het_ref on the features the probe itself pooled, within 4 x the fp32 CPU
    error recorded for this head (z, dW, dbias) on the float64 oracle's features of the same images (the probe's differ from those by the bf16
    encoder's error, which does not change the size of the head's round-off).  Then two more steps against float64 AdamW under the
    seeds of steps 1 and 2: losses within the same bound; every weight within 2 x 3 lr (Adam moves a weight by at most about lr a
    step); and the weights whose first gradient is at least 1e-3 of the largest within 1 % of 3 lr: with the gradient accurate to 1e-6
    of its largest element, Adam's g / (|g| + eps) is accurate to 1e-3 there."""
    fx, cfg, enc, _, _, images, labels = case
    m = MODEL_CASE
    probe = het_probe(case)
    xg, yg = images.cuda(), labels.cuda()
    feats = probe.features(xg).cpu()
    W, bias = head_of(probe)
    s = float(fx["smoothing"])
    loss_ref, dW, db, z_ref, _ = hr.grads(feats, W, bias, labels, m["K"], m["R"], m["S"], probe.step_seed(0), 0, s)
    losses, _, _, (Wp, bp) = hr.train_steps(feats, W, bias, labels, m["K"], m["R"], m["S"], SEED, s, m["lr"], m["wd"], 3)
    lit = CPU_ERR["step"]["model"]
    got = []
    for step in range(3):
        loss, _ = probe.train_step(xg, yg, m["lr"], m["wd"])
        got.append(float(loss))
        if step == 0:
            n, rows = probe._n_decay, probe._rows
            assert_within_4x("step", "model", "dW", probe._grad_arena[:n].view(rows, -1), dW)
            assert_within_4x("step", "model", "dbias", probe._grad_arena[n:n + rows], db)
    # the loss: the cross-entropy op's own bound (tests/test_gpu_probe.py: 1e-5 (1 + |loss|)) plus what the error allowed on z can move it by
    loss_bound = 1e-5 * (1 + abs(float(loss_ref))) + 4 * lit["z"][0] * float(z_ref.abs().max())
    print(f"\nlosses {got}, float64 {losses}; first loss error {abs(got[0] - float(loss_ref)):.2e}, bound {loss_bound:.2e}")
    assert abs(got[0] - float(loss_ref)) <= loss_bound
    W3, b3 = head_of(probe)
    err = (W3.double() - Wp).abs()
    big = dW.abs() >= 1e-3 * dW.abs().max()
    print(f"weights after 3 steps: max error {float(err.max()):.2e}, where the gradient is large {float(err[big].max()):.2e} (3 lr = {3 * m['lr']:.0e})")
    assert float(err.max()) <= 2 * 3 * m["lr"] and float((b3.double() - bp).abs().max()) <= 2 * 3 * m["lr"]
    assert int(big.sum()) > 100 and float(err[big].max()) <= 0.01 * 3 * m["lr"]
    for a, b in zip(got[1:], losses[1:]):
        assert abs(a - b) <= loss_bound + 1e-4      # the weights are within 3e-5 and the loss has a gradient norm of O(1) in them
    assert probe.step_count == 3


def test_het_probe_evaluation_is_a_function_of_the_image(case):
    """evaluate twice gives identical numbers; the logits of an image are bit-equal in two batch positions (share = 1); state_dict
    into a new HetProbe gives equal logits; predictive_variance is (B, K) fp32, non-negative, and evaluate(variance=True) returns
    its mean at the predicted classes; calibration_batch and stability_batch accept z; the optimizer state round-trips."""
    fx, cfg, _, _, _, images, labels = case
    probe = het_probe(case)
    xg = images.cuda()
    batches = [((xg, None), labels), ((xg[:3], None), labels[:3])]
    e1, e2 = probe.evaluate(batches, variance=True), probe.evaluate(batches, variance=True)
    plain = probe.evaluate(batches)
    print(f"\nevaluate: {e1}")
    assert e1 == e2 and "het_var_mean" not in plain and {k: e1[k] for k in plain} == plain
    z = probe.logits(xg)
    perm = torch.arange(xg.shape[0] - 1, -1, -1, device="cuda")
    assert torch.equal(probe.logits(xg[perm]), z[perm])
    assert torch.equal(probe.logits(xg[1:3]), z[1:3])
    var = probe.predictive_variance(xg)
    assert var.dtype == torch.float32 and tuple(var.shape) == (xg.shape[0], MODEL_CASE["K"]) and bool((var >= 0).all()) and float(var.max()) > 0
    v1, v2 = var.gather(1, z.argmax(1, keepdim=True)).squeeze(1).cpu().tolist(), var[:3].gather(1, z[:3].argmax(1, keepdim=True)).squeeze(1).cpu().tolist()
    assert e1["het_var_mean"] == math.fsum(v1 + v2) / (len(v1) + len(v2))
    torch.testing.assert_close(z.exp().sum(-1), torch.ones(xg.shape[0], device="cuda"), rtol=0, atol=1e-5)
    twin = het_probe(case)
    twin.load_state_dict({k: v.cpu() + 0 for k, v in probe.state_dict().items()})
    assert torch.equal(twin.logits(xg), z)
    ece, tace, nll, auroc = probe.calibration_batch(z, labels.cuda())
    assert all(math.isfinite(float(v)) for v in (ece, tace, nll))
    seq = probe.stability_batch(z, 2, False)
    assert tuple(seq.shape) == (xg.shape[0] // 2, 3) and bool(torch.isfinite(seq).all())
    probe.train_step(xg, labels.cuda(), 1e-3, 0.05)
    osd = probe.optimizer_state_dict()
    m0 = probe.exp_avg.clone()
    probe.exp_avg.zero_()
    probe.load_optimizer_state_dict(osd)
    assert osd["step"] == 1 and torch.equal(m0, probe.exp_avg) and float(m0.abs().max()) > 0


def test_linear_probe_beside_the_het_module(L, case):
    """A plain LinearProbe built after the module was imported: logits, train_step and evaluate return the bits of the existing ops
    called directly on its features."""
    import uncertainty_vit_amd.het_probe  # noqa: F401
    fx, cfg, enc, W, bias, images, labels = case
    probe = fixture_probe(case)
    xg, yg = images.cuda(), labels.cuda()
    B, K, Cd = images.shape[0], W.shape[0], cfg.embed_dim
    feat = probe.features(xg)
    Wg, bg = W.cuda(), bias.cuda()
    z, dz, rows, loss, cnt = (torch.zeros(B, K, device="cuda"), torch.zeros(B, K, device="cuda"), torch.zeros(B, device="cuda"),
                              torch.zeros(1, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))
    ok(L.uvit_op_probe_logits(P(feat), P(Wg), P(bg), P(z), B, K, Cd, STREAM()))
    assert torch.equal(probe.logits(xg), z)
    ok(L.uvit_op_probe_ce(P(z), P(yg), f32(0.0), None, P(rows), P(loss), P(cnt), B, K, STREAM()))
    ev = probe.evaluate([((xg, None), labels)])
    assert sorted(ev) == ["acc1", "acc5", "correct1", "correct5", "loss", "n"]
    assert ev["loss"] == float(loss) and [ev["correct1"], ev["correct5"]] == cnt.tolist()
    ok(L.uvit_op_probe_ce(P(z), P(yg), f32(probe.smoothing), P(dz), P(rows), P(loss), None, B, K, STREAM()))
    dW, db = torch.zeros(K, Cd, device="cuda"), torch.zeros(K, device="cuda")
    ok(L.uvit_op_probe_head_grad(P(dz), P(feat), P(dW), P(db), B, K, Cd, STREAM()))
    got_loss, _ = probe.train_step(xg, yg, 1e-3, 0.05)
    assert float(got_loss) == float(loss)
    assert torch.equal(probe.head.weight.grad, dW) and torch.equal(probe.head.bias.grad, db)
    assert [n for n, _ in probe.named_parameters()] == ["head.weight", "head.bias"]


# ------------------------------------------------------------------------------------------------- the table above, measured on the CPU
def measure_cpu_err():
    """CPU_ERR: torch's fp32 CPU evaluation of het_ref against its float64 form on the inputs of the tests above."""
    import os
    import pprint
    r3 = lambda m: tuple(float(f"{v:.2e}") if v == v else 0.0 for v in m)      # noqa: E731  (0 / 0 at S = 1: pvar is exactly 0)
    out = {"noise": {}, "forward": {}, "backward": {}, "step": {}}
    for shape in NOISE_SHAPES:
        ref, cpu = hr.noise(*shape, SEED, 0), hr.noise(*shape, SEED, 0, torch.float32)
        out["noise"][shape] = {"epsR": r3(metrics(cpu[0], ref[0])), "epsK": r3(metrics(cpu[1], ref[1]))}
    for case in MC_CASES:
        for share in (0, 1):
            ref, cpu = mc_reference(*case, share), mc_reference(*case, share, torch.float32)
            out["forward"][(case, share)] = {n: r3(metrics(cpu[i], ref[i])) for i, n in enumerate(("z", "p", "pvar"))}
            out["backward"][(case, share)] = {"dlin": r3(metrics(cpu[5], ref[5]))}
    B, S, K, R, T = 2, 8, 10, 2, 1.0
    lin = mc_inputs(B, S, K, R)
    lin[:, [3, 7]] = -60.0
    dz = rnd(B, K, seed=105, scale=1.0 / B)
    res = []
    for dt in (F64, torch.float32):
        eps = hr.noise(B, S, K, R, SEED, 0, dt)
        p32 = hr.forward(lin, *hr.noise(B, S, K, R, SEED, 0), K, R, T)[1].float()
        res.append((hr.forward(lin, *eps, K, R, T, EPS, dt)[0], hr.backward(lin, p32, dz, *eps, K, R, T, EPS, dt)))
    out["forward"][("clamp", 0)] = {"z": r3(metrics(res[1][0], res[0][0]))}
    out["backward"][("clamp", 0)] = {"dlin": r3(metrics(res[1][1], res[0][1]))}
    # the module's step on the float64 oracle's features of the fixture's images, the head HetProbe draws under seed 5
    fx, cfg, enc, _, _, images, labels = pr.load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    m = MODEL_CASE
    feats = pr.features(enc, cfg, images).float()
    torch.manual_seed(5)
    lins = [torch.nn.Linear(cfg.embed_dim, rows) for rows in (m["K"], m["K"], m["K"] * m["R"])]
    W, bias = torch.cat([x.weight.data for x in lins]), torch.cat([x.bias.data for x in lins])
    s, seed = float(fx["smoothing"]), hr.step_seed(SEED, 0)
    ref = hr.grads(feats, W, bias, labels, m["K"], m["R"], m["S"], seed, 0, s)
    cpu = hr.grads(feats, W, bias, labels, m["K"], m["R"], m["S"], seed, 0, s, dtype=torch.float32)
    out["step"]["model"] = {"z": r3(metrics(cpu[3], ref[3])), "dW": r3(metrics(cpu[1], ref[1])), "dbias": r3(metrics(cpu[2], ref[2]))}
    return "CPU_ERR = " + pprint.pformat(out, width=150, sort_dicts=False)


if __name__ == "__main__":
    print(measure_cpu_err())
