"""CPU: the ensemble probe head's host-side pieces -- the online-bagging weights of tests/ens_ref.py (the thresholds, the law, the
seeds), its float64 criterion against M independent cross-entropies and against autograd, its combination against the literal
expression of the reference's engine_for_finetuning.py:288-290 and the properties of the entropy split, the argument checks of every
uvit_op_ens_* entry point (they return before anything touches a device), the EnsembleProbe module's state dict, arena and members,
and the command line's new flags.  Every test prints what it measures."""
import ctypes as C
import math

import pytest
import torch

import ens_ref as er
import probe_ref as pr
from test_host_probe import tiny_encoder

F64 = torch.float64


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


# ---- the bagging weights ----
def poisson_cdf(n):
    return math.exp(-1) * sum(1.0 / math.factorial(i) for i in range(n + 1))


def test_thresholds_are_the_poisson_cdf():
    want = [math.ceil(2 ** 23 * poisson_cdf(n)) for n in range(8)]
    print(f"\nT = {want}")
    assert list(er.T) == want
    # the law the thresholds define on the 23-bit uniform: P(w = v) = (T[v] - T[v - 1]) / 2^23
    edges = [0] + list(er.T) + [2 ** 23]
    pmf = [(edges[i + 1] - edges[i]) / 2 ** 23 for i in range(9)]
    mean = sum(v * p for v, p in enumerate(pmf))
    var = sum(v * v * p for v, p in enumerate(pmf)) - mean ** 2
    print(f"law: mean {mean:.7f}, variance {var:.5f}")
    assert abs(mean - 0.9999983) < 1e-7 and abs(var - 0.99998) < 1e-5


def test_weights_follow_poisson_one():
    """2^20 (b, m) pairs: mean and variance within 5 standard errors of (1, 1) (the variance of Poisson(1)'s sample variance is
    (mu4 - 1) / n with mu4 = 4), and the frequency of every value 0..8 within 5 standard errors sqrt(p (1 - p) / n) of Poisson(1)
    (8 stands for the tail >= 8)."""
    B, M = 2 ** 16, 16
    n = B * M
    w = er.bag_weights(B, M, 0).view(-1)
    mean, var = float(w.mean()), float(w.var(unbiased=False))
    print(f"\nmean {mean:.5f} (se {1 / math.sqrt(n):.1e}), variance {var:.5f} (se {math.sqrt(3 / n):.1e}), max {int(w.max())}")
    assert abs(mean - 1) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(3 / n)
    assert int(w.min()) == 0 and int(w.max()) <= 8 and bool((w == w.round()).all())
    for v in range(9):
        p = math.exp(-1) / math.factorial(v) if v < 8 else 1 - poisson_cdf(7)
        got, se = float((w == v).double().mean()), math.sqrt(p * (1 - p) / n)
        print(f"P(w = {v}) {got:.3e}, Poisson(1) {p:.3e}, se {se:.1e}")
        assert abs(got - p) <= 5 * se, v


def test_seeds_and_steps_differ():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    a, b = er.bag_weights(64, 5, 0), er.bag_weights(64, 5, 1)
    s0, s1 = er.step_seed(0, 0), er.step_seed(0, 1)
    print(f"\nseeds 0 / 1 differ in {int((a != b).sum())} of 320 weights; step seeds {s0:#x}, {s1:#x}")
    assert not torch.equal(a, b) and s0 != s1 and s0 != 0
    assert not torch.equal(er.bag_weights(64, 5, s0), er.bag_weights(64, 5, s1))
    assert torch.equal(er.bag_weights(64, 5, 0), a)
    # the rows of a smaller batch are a prefix: the counter is b M + m
    assert torch.equal(er.bag_weights(7, 5, 0), a[:7])
    probe = EnsembleProbe(tiny_encoder().eval(), 10, members=2, seed=9)
    assert probe.step_seed(0) == er.step_seed(9, 0) and probe.step_seed(5) == er.step_seed(9, 5)


# ---- the criterion ----
@pytest.mark.parametrize("s", [0.1, 0.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_ce_is_m_cross_entropies_and_its_gradient_is_autograds(s, weighted):
    B, M, K = 6, 3, 7
    lin = rnd(B, M, K, seed=1, scale=2.0)
    labels = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(2))
    w = er.bag_weights(B, M, 5) if weighted else None
    rows, loss, d, counters = er.ce(lin, labels, w, s)
    if not weighted:
        for m in range(M):
            r, mean, dz = pr.smoothed_ce(lin[:, m], labels, s)
            assert float((rows[:, m] - r).abs().max()) <= 1e-12 and abs(float(loss[m] - mean)) <= 1e-12
            assert float((d[:, m] - dz).abs().max()) <= 1e-12
            assert tuple(counters[m].tolist()) == pr.topk_counts(lin[:, m], labels)
    x = lin.clone().requires_grad_(True)
    logp = torch.log_softmax(x, -1)
    per = (1 - s) * -logp.gather(2, labels.view(B, 1, 1).expand(B, M, 1)).squeeze(2) + s * -logp.mean(-1)
    loss_m = ((w if weighted else torch.ones(B, M, dtype=F64)) * per).mean(0)
    auto, = torch.autograd.grad(loss_m.sum(), x)
    err = float((d - auto).abs().max())
    print(f"\ns {s} weighted {weighted}: dlin against autograd {err:.2e}, losses {loss.tolist()}")
    assert err <= 1e-12 and float((loss[:M] - loss_m.detach()).abs().max()) <= 1e-12
    assert abs(float(loss[M]) - float(loss_m.detach().mean())) <= 1e-12
    if weighted:
        assert bool((w == 0).any()) and float(d[w == 0].abs().max()) == 0.0          # a weight of 0 takes the sample from that member


def test_ce_label_out_of_range():
    lin = rnd(4, 2, 5, seed=3)
    labels = torch.tensor([0, 5, 4, -1])
    rows, loss, d, counters = er.ce(lin, labels, None, 0.1)
    assert bool(torch.isnan(rows[[1, 3]]).all()) and bool(torch.isnan(d[[1, 3]]).all()) and bool(torch.isnan(loss).all())
    assert bool(torch.isfinite(rows[[0, 2]]).all())
    keep = torch.tensor([0, 2])
    assert torch.equal(counters, er.ce(lin[keep], labels[keep], None, 0.1)[3])


# ---- the combination ----
def test_combine_modes():
    """Mode 0 is the literal torch.mean(torch.stack(outputs), 0) of engine_for_finetuning.py:288-290 on the members' logits; mode 1 is
    log(mean softmax); pbar sums to 1; total <= log K; mi >= 0."""
    B, M, K = 5, 4, 9
    lin = rnd(B, M * K, seed=4, scale=3.0)
    outputs = [lin[:, m * K:(m + 1) * K] for m in range(M)]
    z0, unc0, k0, km = er.combine(lin, M, 0)
    assert torch.equal(z0, torch.mean(torch.stack(outputs), 0))
    z1, unc1, k1, _ = er.combine(lin, M, 1)
    want = torch.log(torch.stack([torch.softmax(o, -1) for o in outputs]).mean(0))
    print(f"\nmode 1 against log(mean softmax): {float((z1 - want).abs().max()):.2e}; unc row 0 {unc0[0].tolist()}")
    assert float((z1 - want).abs().max()) <= 1e-12
    assert torch.equal(unc0[:, :3], unc1[:, :3])                                      # the entropies do not depend on the mode
    assert torch.equal(km, torch.stack([o.argmax(-1) for o in outputs], 1))
    for unc in (unc0, unc1):
        assert bool((unc[:, 0] <= math.log(K)).all()) and bool((unc[:, 2] >= 0).all()) and bool((unc[:, 1] <= unc[:, 0] + 1e-12).all())
        assert bool((unc[:, 4] * M == (unc[:, 4] * M).round()).all())
    pbar = torch.stack([torch.softmax(o, -1) for o in outputs]).mean(0)
    assert float((unc0[:, 0] + (pbar * pbar.log()).sum(-1)).abs().max()) <= 1e-12
    assert float((unc0[:, 3] - torch.stack([torch.softmax(o, -1) for o in outputs], 1).gather(
        2, k0.view(B, 1, 1).expand(B, M, 1)).squeeze(2).var(1, unbiased=False)).abs().max()) <= 1e-15


def test_identical_members_have_no_disagreement():
    B, M, K = 4, 5, 11
    one = rnd(B, K, seed=5, scale=2.0)
    lin = one.repeat(1, M)
    for mode in (0, 1):
        z, unc, _, _ = er.combine(lin, M, mode)
        print(f"\nmode {mode}: mi {float(unc[:, 2].max()):.2e}, var {float(unc[:, 3].max()):.2e}")
        assert float(unc[:, 2].max()) <= 1e-12 and float(unc[:, 4].max()) == 0.0 and float(unc[:, 3].max()) <= 1e-24
        ref = one if mode == 0 else torch.log_softmax(one, -1)
        assert float((z - ref).abs().max()) <= 1e-12


def test_disjoint_members_have_mi_log_m():
    """Member m puts (nearly) all its mass on class m: the expected entropy is about 0 and the entropy of the mean is log M."""
    B, M, K = 2, 4, 6
    lin = torch.zeros(B, M, K, dtype=F64)
    for m in range(M):
        lin[:, m, m] = 40.0
    _, unc, kstar, km = er.combine(lin.view(B, M * K), M, 1)
    print(f"\nmi {unc[0, 2]:.9f}, log M {math.log(M):.9f}, disagreement {unc[0, 4]}")
    assert abs(float(unc[0, 2]) - math.log(M)) <= 1e-6 and float(unc[0, 4]) == (M - 1) / M
    assert km[0].tolist() == list(range(M)) and int(kstar[0]) == 0                    # ties go to the lowest index


def test_nan_logit_gives_nan_uncertainty():
    lin = rnd(3, 2 * 5, seed=6)
    lin[1, 7] = float("nan")
    _, unc, _, _ = er.combine(lin, 2, 0)
    assert bool(torch.isnan(unc[1]).all()) and bool(torch.isfinite(unc[[0, 2]]).all())


def test_clip_is_per_member():
    M, K, Cd = 3, 3, 8
    g = torch.cat([rnd(M * K * Cd + M * K, seed=7), torch.zeros(3, dtype=F64)]).float()
    g[:K * Cd] *= 10
    norms, same = er.clip(g, M, K, Cd, 0.0)
    assert torch.equal(same, g.double())
    mid = float(norms.sort().values[1]) * 0.99
    _, out = er.clip(g, M, K, Cd, mid)
    after, _ = er.clip(out, M, K, Cd, 0.0)
    print(f"\nnorms {norms.tolist()} -> {after.tolist()} at max_norm {mid:.4f}")
    for m, (wl, wh, bl, bh) in enumerate(er.segments(M, K, Cd)):
        if float(norms[m]) > mid:
            assert abs(float(after[m]) - mid) <= 1e-5
        else:
            assert torch.equal(out[wl:wh], g[wl:wh].double()) and torch.equal(out[bl:bh], g[bl:bh].double())
    bad = g.clone()
    bad[K * Cd + 1] = float("inf")
    n2, out2 = er.clip(bad, M, K, Cd, mid)
    assert math.isinf(float(n2[1])) and torch.equal(out2[K * Cd:2 * K * Cd], bad[K * Cd:2 * K * Cd].double())


def test_training_restatement_is_probe_refs():
    """One member without weights trains as probe_ref.train_steps trains a linear head; the fp32 form stays within 1e-4 of it."""
    B, K, Cd = 6, 5, 16
    feat, W, bias = rnd(B, Cd, seed=8), rnd(K, Cd, seed=9, scale=0.1), rnd(K, seed=10, scale=0.1)
    labels = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(11))
    for max_norm in (None, 0.05):
        losses, norms, _, (Wp, bp) = pr.train_steps(feat, W, bias, labels, 0.1, 1e-3, 0.05, 3, max_norm)
        l2, n2, (W2, b2) = er.train_steps(feat, W, bias, labels, 1, 0.1, 1e-3, 0.05, 3, None, max_norm)
        assert torch.equal(W2, Wp) and torch.equal(b2, bp) and [float(x[0]) for x in l2] == losses and [n[0] for n in n2] == norms
        _, _, (W3, _) = er.train_steps(feat, W, bias, labels, 1, 0.1, 1e-3, 0.05, 3, None, max_norm, torch.float32)
        print(f"\nmax_norm {max_norm}: fp32 against float64 after 3 steps {float((W3.double() - Wp).abs().max()):.2e}")
        assert W3.dtype == torch.float32 and float((W3.double() - Wp).abs().max()) <= 1e-4
    # two members with different weights drift apart; without weights and from equal heads they stay equal
    W2m, b2m = torch.cat([W, W]), torch.cat([bias, bias])
    _, _, (Wa, _) = er.train_steps(feat, W2m, b2m, labels, 2, 0.1, 1e-3, 0.05, 2)
    _, _, (Wb, _) = er.train_steps(feat, W2m, b2m, labels, 2, 0.1, 1e-3, 0.05, 2, bagging_seed=3)
    assert torch.equal(Wa[:K], Wa[K:]) and not torch.equal(Wb[:K], Wb[K:])


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE = -1, -2
BAD_BMK = [(0, 3, 5), (-1, 3, 5), (2, 0, 5), (2, 17, 5), (2, -1, 5), (2, 3, 0), (2, 3, -4)]


def f(v):
    return C.c_float(v)


def test_symbols_are_bound():
    from uncertainty_vit_amd import native
    for name in ("uvit_op_ens_bag_weights", "uvit_op_ens_ce", "uvit_op_ens_clip", "uvit_op_ens_combine"):
        assert name in native.SYMBOLS and getattr(native.lib(), name).argtypes is not None


def test_bag_weights_rejects_bad_arguments(L):
    assert L.uvit_op_ens_bag_weights(NUL, 2, 3, 0, NUL) == ARG
    for B, M in ((0, 3), (-1, 3), (2, 0), (2, 17)):
        assert L.uvit_op_ens_bag_weights(P1, B, M, 0, NUL) == SHAPE, (B, M)


def test_ce_rejects_bad_arguments(L):
    call = lambda p, s=0.1, shape=(2, 3, 5): L.uvit_op_ens_ce(p[0], p[1], p[2], f(s), p[3], p[4], p[5], p[6], *shape, NUL)      # noqa: E731
    for shape in BAD_BMK:
        assert call([P1] * 7, shape=shape) == SHAPE, shape
    for i in (0, 1, 4, 5):                        # lin, labels, row_loss and loss_out are required; weights, dlin and counters are not
        a = [P1] * 7
        a[i] = NUL
        assert call(a) == ARG, i
    for s in (-0.1, 1.0, 1.5, float("nan")):
        assert call([P1] * 7, s=s) == ARG, s


def test_clip_rejects_bad_arguments(L):
    call = lambda g, n, shape=(3, 5, 8), mx=1.0: L.uvit_op_ens_clip(g, n, *shape, f(mx), NUL)      # noqa: E731
    assert call(NUL, P1) == ARG and call(P1, NUL) == ARG
    for shape in ((0, 5, 8), (17, 5, 8), (3, 0, 8), (3, 5, 6), (3, 5, 0), (3, 5, 2)):
        assert call(P1, P1, shape) == SHAPE, shape


def test_combine_rejects_bad_arguments(L):
    call = lambda lin, z, mode=0, shape=(2, 3, 5), unc=P1: L.uvit_op_ens_combine(lin, mode, z, unc, *shape, NUL)      # noqa: E731
    for shape in BAD_BMK:
        assert call(P1, P1, shape=shape) == SHAPE, shape
    assert call(NUL, P1) == ARG and call(P1, NUL) == ARG
    for mode in (-1, 2):
        assert call(P1, P1, mode=mode) == ARG, mode


# ---- the module ----
K_, C_, M_ = 10, 128, 3


def ens_keys(M=M_):
    return {f"heads.{m}.{n}": s for m in range(M) for n, s in (("weight", (K_, C_)), ("bias", (K_,)))}


def test_ensemble_probe_state_dict_arena_and_init():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe, _timm_trunc_normal_
    from uncertainty_vit_amd.native import UvitError
    torch.manual_seed(3)
    probe = EnsembleProbe(tiny_encoder().eval(), K_, members=M_)
    assert isinstance(probe, LinearProbe)
    sd = probe.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == ens_keys()
    assert sorted(n for n, p in probe.named_parameters() if p.requires_grad) == sorted(ens_keys())
    # one arena [W (M K, C) | bias (M K) | pad to 4]: the weights decay, the biases do not
    rows = M_ * K_
    assert probe._n_decay == rows * C_ and probe._arena.numel() == (rows * C_ + rows + 3) // 4 * 4
    base = probe._arena.data_ptr()
    for m in range(M_):
        assert sd[f"heads.{m}.weight"].data_ptr() == base + 4 * m * K_ * C_ and sd[f"heads.{m}.bias"].data_ptr() == base + 4 * (rows * C_ + m * K_)
        assert float(sd[f"heads.{m}.bias"].abs().max()) == 0.0
    # member 0 holds the bits of a LinearProbe built under the same seed; the members after it are the next draws
    torch.manual_seed(3)
    lin = LinearProbe(tiny_encoder().eval(), K_)
    assert torch.equal(sd["heads.0.weight"], lin.head.weight.data)
    second = _timm_trunc_normal_(torch.empty(K_, C_), std=0.02).mul_(0.001)
    assert torch.equal(sd["heads.1.weight"], second) and not torch.equal(sd["heads.1.weight"], sd["heads.0.weight"])
    dflt = EnsembleProbe(tiny_encoder().eval(), 100)
    assert (dflt.members, dflt.smoothing, dflt.combine, dflt.bagging, dflt.seed) == (5, 0.1, "logits", False, 0)
    osd = probe.optimizer_state_dict()
    assert osd["step"] == 0 and {k: tuple(v.shape) for k, v in osd["exp_avg"].items()} == ens_keys()
    probe.exp_avg[:] = torch.arange(probe.exp_avg.numel())
    osd = probe.optimizer_state_dict()
    probe.exp_avg.zero_()
    probe.load_optimizer_state_dict({**osd, "step": 4})
    assert probe.step_count == 4 and torch.equal(probe.exp_avg[:rows * C_ + rows], torch.arange(rows * C_ + rows).float())
    assert tuple(probe.member_norms.shape) == (M_,)
    # no CPU fallback
    x = torch.zeros(2, 3, 48, 48)
    for call in (probe.logits, probe.member_logits, probe.uncertainty):
        with pytest.raises(UvitError):
            call(x)
    with pytest.raises(UvitError):
        probe.train_step(x, torch.zeros(2, dtype=torch.int64), 1e-3, 0.05)


def test_members_round_trip():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    torch.manual_seed(4)
    probe = EnsembleProbe(tiny_encoder().eval(), K_, members=M_)
    heads = [probe.member_state_dict(m) for m in range(M_)]
    assert all(sorted(h) == ["head.bias", "head.weight"] for h in heads)
    lin = LinearProbe(tiny_encoder().eval(), K_)
    lin.load_state_dict(heads[1])                                                     # a member loads into a LinearProbe
    assert torch.equal(lin.head.weight.data, probe.state_dict()["heads.1.weight"])
    twin = EnsembleProbe.from_heads(tiny_encoder().eval(), heads, combine="probs")
    assert twin.members == M_ and twin.combine == "probs" and twin.num_classes == K_
    assert all(torch.equal(a, b) for a, b in zip(twin.state_dict().values(), probe.state_dict().values()))
    probe.load_member(2, {"head.weight": torch.full((K_, C_), 0.5), "head.bias": torch.full((K_,), 0.25)})
    w0 = M_ * K_ * C_
    assert float(probe._arena[2 * K_ * C_:w0].min()) == 0.5 and float(probe._arena[w0 + 2 * K_:w0 + 3 * K_].min()) == 0.25
    assert torch.equal(probe.member_state_dict(0)["head.weight"], heads[0]["head.weight"])
    with pytest.raises(IndexError):
        probe.member_state_dict(M_)
    with pytest.raises(ValueError):
        probe.load_member(0, {"head.weight": torch.zeros(K_ + 1, C_), "head.bias": torch.zeros(K_ + 1)})
    with pytest.raises(ValueError):
        EnsembleProbe.from_heads(tiny_encoder().eval(), [])


def test_ensemble_probe_rejects_what_is_not_built():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    with pytest.raises(NotImplementedError):
        EnsembleProbe(tiny_encoder(two_stream=True).eval(), 10)
    for kw in (dict(members=0), dict(members=17), dict(combine="mean"), dict(num_classes=0), dict(smoothing=1.0)):
        with pytest.raises(ValueError):
            EnsembleProbe(tiny_encoder().eval(), **{"num_classes": 10, **kw})
    assert EnsembleProbe(tiny_encoder().eval(), 1, members=16).members == 16


def test_linear_probe_is_what_it_was():
    """Importing the module leaves the linear head's state, arena and draws alone."""
    import uncertainty_vit_amd.ens_probe  # noqa: F401
    from uncertainty_vit_amd.linear_probe import LinearProbe, _timm_trunc_normal_
    torch.manual_seed(3)
    probe = LinearProbe(tiny_encoder().eval(), 10)
    torch.manual_seed(3)
    tiny_encoder()
    want = _timm_trunc_normal_(torch.empty(10, 128), std=0.02).mul_(0.001)
    assert list(probe.state_dict()) == ["head.weight", "head.bias"] and torch.equal(probe.head.weight.data, want)
    assert probe._arena.numel() == 10 * 128 + 12 and probe._n_decay == 10 * 128


# ---- the command line ----
def test_cli_flags_are_absent_unless_given(monkeypatch):
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()                                  # the parsed defaults without --ensembles equal today's
    got = vars(rlp.get_args([]))
    assert not [k for k in got if k.startswith("ens")]
    a = rlp.get_args(["--ensembles"])
    assert a.ensembles is True and not any(hasattr(a, k) for k in rlp.ENS_FLAGS) and rlp.ens_member_count(a) == 5
    a = rlp.get_args(["--ensembles", "--ens_members", "3", "--ens_combine", "probs", "--ens_bagging", "--ens_seed", "7"])
    assert (a.ens_members, a.ens_combine, a.ens_bagging, a.ens_seed) == (3, "probs", True, 7) and rlp.ens_member_count(a) == 3
    a = rlp.get_args(["--ensembles", "--eval", "--ens_heads", "a.pth", "b.pth"])
    assert a.ens_heads == ["a.pth", "b.pth"] and rlp.ens_member_count(a) == 2          # the files set the member count
    with pytest.raises(SystemExit):
        rlp.get_args(["--ensembles", "--ens_combine", "median"])
    stats = {"member_acc1": [50.0, 25.0], "member_acc5": [100.0, 75.0], "member_loss": [1.5, 2.25], "ens_total": 1.0, "ens_aleatoric": 0.75,
             "ens_mi": 0.25, "ens_var": 0.125, "ens_disagreement": 0.5}
    assert rlp.ens_lines(stats) == ["* Member 0 Acc@1 50.000 Acc@5 100.000 loss 1.500", "* Member 1 Acc@1 25.000 Acc@5 75.000 loss 2.250",
                                    "* Ens entropy 1.00000 expected 0.75000 MI 0.25000 variance 0.125000 disagreement 0.50000"]
    assert rlp.ens_log_entries(stats) == {"test_member0_acc1": 50.0, "test_member1_acc1": 25.0, "test_ens_total": 1.0, "test_ens_aleatoric": 0.75,
                                          "test_ens_mi": 0.25, "test_ens_var": 0.125, "test_ens_disagreement": 0.5}
    # the errors come before anything is loaded
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    base = ["--nb_classes", "10", "--finetune", "none.pth"]
    for flags in (["--ens_members", "3"], ["--ens_combine", "probs"], ["--ens_bagging"], ["--ens_seed", "1"], ["--ens_heads", "a.pth"]):
        with pytest.raises(ValueError, match="--ensembles"):
            rlp.main(rlp.get_args(base + flags))
    for other in ("--gp_layer", "--het_layer"):
        with pytest.raises(ValueError, match="ensemble of linear heads"):
            rlp.main(rlp.get_args(base + ["--ensembles", other]))
    with pytest.raises(ValueError, match="--eval"):
        rlp.main(rlp.get_args(base + ["--ensembles", "--ens_heads", "a.pth"]))
    with pytest.raises(ValueError, match="names 2 files"):
        rlp.main(rlp.get_args(base + ["--ensembles", "--eval", "--ens_heads", "a.pth", "b.pth", "--ens_members", "3"]))
