"""CPU: the heteroscedastic probe head's host-side pieces -- the counter-based noise of tests/het_ref.py (exact uniforms, moments,
stream independence), its float64 forward and backward against autograd and against the literal einsum of the reference's
modeling_finetune.py:1158, the clamp, the argument checks of every uvit_op_het_* entry point (they return before anything touches a
device), the HetProbe module's state dict and arena, and the command line's new flags.  Every test prints what it measures."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import het_ref as hr
import probe_ref as pr
from test_host_probe import tiny_encoder

F64 = torch.float64


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the noise ----
def test_uniforms_are_exact_in_float32():
    """(h >> 9) + 0.5 has 24 significant bits and the factor 2^-23 is a power of two: float32 and float64 hold the same numbers,
    all inside (0, 1).  The vectorised hash equals the scalar one the module uses for its step seeds."""
    from uncertainty_vit_amd.het_probe import _hash32
    for x in (0, 1, 42, 0x9E3779B9, 0xFFFFFFFF):
        assert int(hr.hash32(x)) == _hash32(x), x
    a, b = hr.uniform_bits(42, 1, 3, 5, 67, 0)
    assert a.shape == (3, 5, 34) and int(a.max()) < 2 ** 23 and int(b.max()) < 2 ** 23
    u32s, u64s = hr.uniforms(42, 1, 3, 5, 67, 0, torch.float32), hr.uniforms(42, 1, 3, 5, 67, 0, F64)
    for bits, u32, u64 in zip((a, b), u32s, u64s):
        assert u32.dtype == torch.float32 and torch.equal(u32.double(), u64)
        assert torch.equal(u64, (torch.from_numpy(bits.astype(np.int64)).double() * 2 + 1) / 2 ** 24)
        assert float(u64.min()) > 0.0 and float(u64.max()) < 1.0
    bound = math.sqrt(-2 * math.log(2.0 ** -24))
    print(f"\nuniforms in [{float(u64s[0].min()):.3e}, {float(u64s[0].max()):.7f}]; the smallest possible is 2^-24: |n| <= {bound:.3f}")
    assert bound <= 5.8


def test_moments_of_the_draws():
    """2^20 draws (2^19 pairs): mean, variance and the correlation of the two values of a pair within 5 standard errors of (0, 1, 0).
    Standard errors at n values: mean 1 / sqrt(n); variance sqrt(2 / n) (the fourth moment of a normal is 3); correlation over n / 2
    pairs 1 / sqrt(n / 2)."""
    n = 2 ** 20
    x = hr.normals(42, 1, 1, 1, n, 0).view(-1)
    mean, var = float(x.mean()), float(x.var(unbiased=False))
    a, b = x[0::2], x[1::2]
    corr = float((a * b).mean() / (a.std() * b.std()))
    print(f"\nmean {mean:+.3e} (se {1 / math.sqrt(n):.1e}), variance {var:.5f} (se {math.sqrt(2 / n):.1e}), pair correlation {corr:+.3e} "
          f"(se {1 / math.sqrt(n / 2):.1e}), max |n| {float(x.abs().max()):.3f}")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n) and abs(corr) <= 5 / math.sqrt(n / 2)
    assert float(x.abs().max()) <= 5.8


def test_streams_rows_and_seeds_are_independent():
    """share = 1 equals row 0 of share = 0 in every row; streams 0 and 1, two rows, two samples and two seeds differ; the draws of a
    shorter vector are a prefix of a longer one's (the pair index is the counter)."""
    B, S, K, R = 3, 4, 7, 3
    eR0, eK0 = hr.noise(B, S, K, R, 42, 0)
    eR1, eK1 = hr.noise(B, S, K, R, 42, 1)
    for b in range(B):
        assert torch.equal(eR1[b], eR0[0]) and torch.equal(eK1[b], eK0[0])
    assert not torch.equal(eR0[1], eR0[0]) and not torch.equal(eK0[0, 1], eK0[0, 0])
    assert not torch.equal(eK0[:, :, :R], eR0)                                   # stream 0 against stream 1 at the same counters
    assert not torch.equal(hr.noise(B, S, K, R, 43, 0)[1], eK0)
    assert torch.equal(hr.normals(42, 1, B, S, 6, 0), eK0[:, :, :6])
    assert hr.step_seed(42, 0) != hr.step_seed(42, 1) != 42


# ---- forward and backward ----
def het_case(B=3, S=5, K=10, R=3, seed=7):
    """lin whose noise terms are of the order of the spread of loc; draw takes both signs."""
    lin = torch.cat([rnd(B, K, seed=seed), rnd(B, K, seed=seed + 1, scale=0.7), rnd(B, K * R, seed=seed + 2, scale=0.5)], dim=1).double()
    epsR, epsK = hr.noise(B, S, K, R, 42, 0)
    return lin, epsR, epsK, torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(seed + 3))


@pytest.mark.parametrize("temperature,smoothing", [(1.0, 0.1), (1.0, 0.0), (0.5, 0.1), (0.5, 0.0)])
def test_backward_is_the_autograd_gradient(temperature, smoothing):
    """dlin of the restatement against autograd on a float64 torch graph of the forward, given the same draws, to 1e-12."""
    B, S, K, R = 3, 5, 10, 3
    lin, epsR, epsK, labels = het_case(B, S, K, R)
    x = lin.clone().requires_grad_(True)
    loc, draw, V = x[:, :K], x[:, K:2 * K], x[:, 2 * K:].view(B, K, R)
    u = loc[:, None, :] + (V[:, None, :, :] * epsR[:, :, None, :]).sum(-1) + (draw + 1e-3)[:, None, :] * epsK
    p = torch.softmax(u / temperature, dim=-1).mean(1)
    z = torch.log(torch.clamp(p, 1e-7, 1.0))
    logp = torch.log_softmax(z, -1)
    loss = ((1 - smoothing) * -logp.gather(1, labels.view(-1, 1)).squeeze(1) + smoothing * -logp.mean(-1)).mean()
    auto, = torch.autograd.grad(loss, x)
    mz, mp, _, _ = hr.forward(lin, epsR, epsK, K, R, temperature)
    _, mloss, dz = pr.smoothed_ce(mz, labels, smoothing)
    mine = hr.backward(lin, mp, dz, epsR, epsK, K, R, temperature)
    err = float((mine - auto).abs().max() / auto.abs().max())
    print(f"\nT {temperature} smoothing {smoothing}: dlin error / max|dlin| {err:.2e}, loss {float(mloss):.6f}")
    torch.testing.assert_close(mz, z.detach(), rtol=1e-12, atol=1e-14)
    assert float(mloss) == pytest.approx(float(loss.detach()), rel=1e-12)
    assert err <= 1e-12
    assert float(mine[:, :K].sum(1).abs().max()) <= 1e-14                         # each row of dloc sums to 0


def test_factor_term_is_the_reference_einsum():
    """The low-rank term V . epsR_s against the literal expression of modeling_finetune.py:1158,
    torch.einsum('ijk,iak->iaj', factor_loadings, standard_normal) with factor_loadings (B, K, R) and the draws (B, S, R)."""
    B, S, K, R = 3, 5, 10, 3
    lin, epsR, epsK, _ = het_case(B, S, K, R)
    loc, d, V = hr.split(lin, K, R)
    ref = torch.einsum('ijk,iak->iaj', V, epsR)
    mine = hr.latents(lin, epsR, epsK, K, R) - loc[:, None, :] - d[:, None, :] * epsK
    print(f"\nfactor term: max difference {float((mine - ref).abs().max()):.2e}, max |term| {float(ref.abs().max()):.3f}")
    torch.testing.assert_close(mine, ref, rtol=0, atol=1e-13)
    assert float(ref.abs().max()) > 0.5
    assert torch.equal(d, lin[:, K:2 * K] + 1e-3) and bool((d < 0).any()) and bool((d > 0).any())


def test_clamp_gives_log_eps_and_no_gradient():
    """A class with loc = -60: p < 1e-7, z = log(1e-7) exactly, and dlin is zero at its loc, draw and V entries when only that
    class's dz is non-zero; the other classes' gradients are what they are."""
    B, S, K, R = 2, 5, 6, 2
    lin, epsR, epsK, _ = het_case(B, S, K, R, seed=11)
    lin[:, 4] = -60.0
    z, p, pvar, _ = hr.forward(lin, epsR, epsK, K, R)
    print(f"\nclamped class: p {float(p[:, 4].max()):.3e}, z {float(z[0, 4]):.6f}, log(1e-7) {math.log(1e-7):.6f}")
    assert float(p[:, 4].max()) < 1e-7 / 2 and bool((z[:, 4] == math.log(1e-7)).all())
    only = torch.zeros(B, K, dtype=F64)
    only[:, 4] = 1.0
    assert float(hr.backward(lin, p, only, epsR, epsK, K, R).abs().max()) == 0.0
    full = hr.backward(lin, p, torch.ones(B, K, dtype=F64) * torch.arange(K), epsR, epsK, K, R)
    assert float(full[:, :4].abs().max()) > 0.0
    torch.testing.assert_close(p.sum(-1), torch.ones(B, dtype=F64), rtol=0, atol=1e-14)
    assert bool((pvar >= 0).all())


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE = -1, -2
BAD_SHAPES = [(0, 5, 10, 3), (-1, 5, 10, 3), (65536, 5, 10, 3), (2, 0, 10, 3), (2, 65536, 10, 3), (2, 5, 2, 1), (2, 5, 4097, 3), (2, 5, 10, 0),
              (2, 5, 10, 33), (2, 5, 40, 33), (2, 5, 3, 4)]


def f(v):
    return C.c_float(v)


def test_symbols_are_bound():
    from uncertainty_vit_amd import native
    for name in ("uvit_op_het_noise", "uvit_op_het_mc_ws_bytes", "uvit_op_het_mc_forward", "uvit_op_het_mc_backward"):
        assert name in native.SYMBOLS and getattr(native.lib(), name).argtypes is not None


def test_noise_rejects_bad_arguments(L):
    for shape in BAD_SHAPES:
        assert L.uvit_op_het_noise(P1, P1, *shape, 42, 0, NUL) == SHAPE, shape
    for share in (-1, 2):
        assert L.uvit_op_het_noise(P1, P1, 2, 5, 10, 3, 42, share, NUL) == ARG, share
    assert L.uvit_op_het_noise(NUL, NUL, 2, 5, 10, 3, 42, 0, NUL) == 0            # nothing asked for: nothing launched


def test_ws_bytes_and_the_partition(L):
    """The scratch is (chunks of the row's samples) x B x K (R + 2) floats with chunks = ceil(S / (64 ceil(S / 512))) <= 8."""
    for shape in BAD_SHAPES:
        assert L.uvit_op_het_mc_ws_bytes(*shape) == SHAPE, shape
    for S, chunks in ((1, 1), (64, 1), (65, 2), (130, 3), (512, 8), (513, 5), (1000, 8), (65535, 8)):
        assert -(-S // hr.chunk_size(S)) == chunks
        assert L.uvit_op_het_mc_ws_bytes(2, S, 10, 3) == chunks * 2 * 10 * 5 * 4, S
    assert L.uvit_op_het_mc_ws_bytes(128, 1000, 1000, 10) == 8 * 128 * 12000 * 4


def test_forward_rejects_bad_arguments(L):
    call = lambda p, shape=(2, 5, 10, 3), T=1.0, eps=1e-7, share=0: L.uvit_op_het_mc_forward(*p, *shape, f(T), f(eps), 42, share, NUL)      # noqa: E731
    for shape in BAD_SHAPES:
        assert call([P1] * 5, shape) == SHAPE, shape
    for i in (0, 2, 4):                            # lin, p and scratch are required; z and pvar are not
        a = [P1] * 5
        a[i] = NUL
        assert call(a) == ARG, i
    for T in (0.0, -1.0, float("nan"), float("inf")):
        assert call([P1] * 5, T=T) == ARG, T
    for share in (-1, 2):
        assert call([P1] * 5, share=share) == ARG, share
    assert call([P1] * 5, eps=float("nan")) == ARG and call([P1] * 5, eps=1.0) == ARG


def test_backward_rejects_bad_arguments(L):
    call = lambda p, shape=(2, 5, 10, 3), T=1.0, eps=1e-7, share=0: L.uvit_op_het_mc_backward(*p, *shape, f(T), f(eps), 42, share, NUL)      # noqa: E731
    for shape in BAD_SHAPES:
        assert call([P1] * 5, shape) == SHAPE, shape
    for i in range(5):
        a = [P1] * 5
        a[i] = NUL
        assert call(a) == ARG, i
    for T in (0.0, -1.0, float("nan")):
        assert call([P1] * 5, T=T) == ARG, T
    for share in (-1, 2):
        assert call([P1] * 5, share=share) == ARG, share


# ---- the module ----
K_, C_, R_ = 10, 128, 3
HET_KEYS = {"head._loc_layer.weight": (K_, C_), "head._loc_layer.bias": (K_,), "head._diag_layer.weight": (K_, C_), "head._diag_layer.bias": (K_,),
            "head._scale_layer.weight": (K_ * R_, C_), "head._scale_layer.bias": (K_ * R_,)}


def test_het_probe_state_dict_arena_and_init():
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    torch.manual_seed(3)
    probe = HetProbe(tiny_encoder().eval(), K_, num_factors=R_)
    assert isinstance(probe, LinearProbe)
    sd = probe.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == HET_KEYS
    assert sorted(n for n, p in probe.named_parameters() if p.requires_grad) == sorted(HET_KEYS)
    # one arena [W_loc | W_diag | W_scale | b_loc | b_diag | b_scale | pad to 4]: the weights are one (K (R + 2), C) matrix and decay
    rows = K_ * (R_ + 2)
    assert probe._n_decay == rows * C_ and probe._arena.numel() == (rows * C_ + rows + 3) // 4 * 4 and probe._arena.numel() % 4 == 0
    base = probe._arena.data_ptr()
    for key, off in (("head._loc_layer.weight", 0), ("head._diag_layer.weight", K_ * C_), ("head._scale_layer.weight", 2 * K_ * C_),
                     ("head._loc_layer.bias", rows * C_), ("head._diag_layer.bias", rows * C_ + K_), ("head._scale_layer.bias", rows * C_ + 2 * K_)):
        assert sd[key].data_ptr() == base + 4 * off, key
    # nn.Linear's default initial values: U(-1 / sqrt(C), 1 / sqrt(C)) for weights and biases, drawn under the caller's seed
    bound = 1 / math.sqrt(C_)
    for key, v in sd.items():
        assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.8 * bound, key
    torch.manual_seed(3)
    tiny_encoder()
    want = torch.nn.Linear(C_, K_)
    assert torch.equal(sd["head._loc_layer.weight"], want.weight.data) and torch.equal(sd["head._loc_layer.bias"], want.bias.data)
    # loading goes through the views; the defaults are the reference's
    probe.load_state_dict({k: torch.full(s, 0.5) for k, s in HET_KEYS.items()})
    assert float(probe._arena[:rows * C_ + rows].min()) == 0.5
    dflt = HetProbe(tiny_encoder().eval(), 100)
    assert (dflt.num_factors, dflt.temperature, dflt.train_mc_samples, dflt.test_mc_samples, dflt.seed) == (10, 1.0, 1000, 1000, 42)
    assert probe.step_seed(0) == hr.step_seed(42, 0) and probe.step_seed(5) == hr.step_seed(42, 5)
    osd = probe.optimizer_state_dict()
    assert osd["step"] == 0 and {k: tuple(v.shape) for k, v in osd["exp_avg"].items()} == HET_KEYS
    # no CPU fallback
    with pytest.raises(UvitError):
        probe.logits(torch.zeros(2, 3, 48, 48))
    with pytest.raises(UvitError):
        probe.predictive_variance(torch.zeros(2, 3, 48, 48))
    with pytest.raises(UvitError):
        probe.train_step(torch.zeros(2, 3, 48, 48), torch.zeros(2, dtype=torch.int64), 1e-3, 0.05)


def test_het_probe_rejects_what_is_not_built():
    from uncertainty_vit_amd.het_probe import HetProbe
    with pytest.raises(NotImplementedError):
        HetProbe(tiny_encoder(two_stream=True).eval(), 10)
    for kw in (dict(num_classes=2), dict(num_classes=4097), dict(num_factors=0), dict(num_factors=33), dict(num_classes=5, num_factors=6),
               dict(temperature=0.0), dict(train_mc_samples=0), dict(test_mc_samples=65536)):
        with pytest.raises(ValueError):
            HetProbe(tiny_encoder().eval(), **{"num_classes": 10, **kw})


def test_linear_probe_is_what_it_was():
    """Importing the module leaves the linear head's state, arena and draws alone."""
    import uncertainty_vit_amd.het_probe  # noqa: F401
    from uncertainty_vit_amd.linear_probe import LinearProbe, _timm_trunc_normal_
    torch.manual_seed(3)
    probe = LinearProbe(tiny_encoder().eval(), 10)
    torch.manual_seed(3)
    tiny_encoder()
    want = _timm_trunc_normal_(torch.empty(10, 128), std=0.02).mul_(0.001)
    assert list(probe.state_dict()) == ["head.weight", "head.bias"] and torch.equal(probe.head.weight.data, want)
    assert probe._arena.numel() == 10 * 128 + 12 and probe._n_decay == 10 * 128


def test_cli_flags_are_absent_unless_given(monkeypatch):
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()                                  # the parsed defaults without --het_layer equal today's
    got = vars(rlp.get_args([]))
    assert not [k for k in got if k.startswith("het_")]
    a = rlp.get_args(["--het_layer"])
    assert a.het_layer is True and not any(hasattr(a, k) for k in rlp.HET_FLAGS)
    a = rlp.get_args(["--het_layer", "--het_num_factors", "4", "--het_temperature", "0.5", "--het_train_mc_samples", "100",
                      "--het_test_mc_samples", "200", "--het_seed", "7"])
    assert (a.het_num_factors, a.het_temperature, a.het_train_mc_samples, a.het_test_mc_samples, a.het_seed) == (4, 0.5, 100, 200, 7)
    assert rlp.het_variance_line({"het_var_mean": 0.25}) == "* Het variance mean 0.250000"
    # the errors come before anything is loaded: a --het_* option without --het_layer, and both heads at once
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    base = ["--nb_classes", "10", "--finetune", "none.pth"]
    with pytest.raises(ValueError, match="--het_layer"):
        rlp.main(rlp.get_args(base + ["--het_num_factors", "4"]))
    with pytest.raises(ValueError, match="two heads"):
        rlp.main(rlp.get_args(base + ["--het_layer", "--gp_layer"]))
