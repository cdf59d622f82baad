"""CPU: the GP probe head's host-side pieces -- the float64 restatement (tests/gp_ref.py) against what the reference's SNGP class
computed (tests/golden/gp_head.npz, written by tools/gen_golden_gp.py), its gradients against autograd, the argument checks of every
uvit_op_gp_* entry point (they return before anything touches a device), the GPProbe module's state dict and arena, and the command
line's new flags."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_ref as gr
import probe_ref as pr
from test_host_probe import tiny_encoder

F64 = torch.float64


@pytest.fixture(scope="module")
def case(golden_dir):
    return gr.load_fixture(golden_dir)


def rel_max(got, ref):
    """max |got - ref| / max |ref|: the measure tools/gen_golden_gp.py stores the reference's own deviation in."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max())


def test_gp_ref_reproduces_reference(case):
    """Every stored quantity within 4 x the reference's own stored deviation from float64: the restatement is float64, so what
    remains between the two is the reference's fp32 round-off."""
    fx, head, feats, labels = case
    Cd, D, K, B, steps = [int(v) for v in fx["cfg"]]
    assert (Cd, D, K, B) == (128, 128, 10, 4) and tuple(head["W_rf"].shape) == (D, Cd)
    assert float((head["gamma"] - 1).abs().max()) > 0.1 and float(head["beta"].abs().max()) > 0.05      # away from (1, 0)
    s, lr, wd = float(fx["smoothing"]), float(fx["lr"]), float(fx["weight_decay"])
    assert (float(fx["ridge"]), float(fx["momentum"]), float(fx["scale"])) == (gr.RIDGE, gr.MOMENTUM, 1.0)
    loss, dW, dgamma, dbeta, phi, z = gr.grads(feats, head, labels, s)
    losses, _, Ps, h = gr.train_steps(feats, head, labels, s, lr, wd, steps)
    _, _, phi3 = gr.features(feats, h["gamma"], h["beta"], head["W_rf"], head["b_rf"])
    mine = {"logits": z, "loss": loss, "grad/W_out": dW, "grad/gamma": dgamma, "grad/beta": dbeta,
            "P1": gr.precision_update(gr.initial_precision(D), phi), "P3": Ps[-1], "step_loss": torch.tensor(losses),
            "post/W_out": h["W_out"], "post/gamma": h["gamma"], "post/beta": h["beta"], "var": gr.variance(phi3, Ps[-1])}
    for key, val in mine.items():
        dev = float(fx["dev/" + key])
        err = rel_max(fx[key], val)
        print(f"{key:12s} error {err:.3e}, stored deviation {dev:.3e}")
        assert 0.0 < dev < 5e-6, key                    # fp32 round-off, not a disagreement of formulas
        assert err <= 4 * dev, (key, err, dev)
    assert torch.equal(Ps[0], mine["P1"])               # the first of three steps starts where the single forward did
    assert np.array_equal(fx["P1"], fx["P1"].T) and np.array_equal(fx["P3"], fx["P3"].T)     # the reference's P is exactly symmetric
    assert 50 < float(fx["cond_P3"]) < 1000
    assert float((h["gamma"].float() - head["gamma"]).abs().max()) > 1e-3          # three steps of lr 1e-3 did move the head


def test_gradients_are_the_autograd_gradients(case):
    """dgamma, dbeta, dW_out of gp_ref against autograd on a float64 torch graph of the forward, to 1e-12."""
    _, head, feats, labels = case
    for scale, s in ((1.0, 0.1), (0.125, 0.0)):
        p = {k: head[k].to(F64).clone().requires_grad_(True) for k in ("gamma", "beta", "W_out")}
        g = torch.nn.functional.layer_norm(feats.to(F64), (feats.shape[1],), p["gamma"], p["beta"], gr.LN_EPS)
        z = (scale * torch.cos(g @ head["W_rf"].to(F64).t() + head["b_rf"].to(F64))) @ p["W_out"].t()
        logp = torch.log_softmax(z, -1)
        loss = ((1 - s) * -logp.gather(1, labels.view(-1, 1)).squeeze(1) + s * -logp.mean(-1)).mean()
        auto = torch.autograd.grad(loss, [p["W_out"], p["gamma"], p["beta"]])
        mine_loss, dW, dgamma, dbeta, _, mz = gr.grads(feats, head, labels, s, scale)
        torch.testing.assert_close(mz, z.detach(), rtol=1e-12, atol=1e-14)
        assert float(mine_loss) == pytest.approx(float(loss.detach()), rel=1e-12)
        for got, ref in zip((dW, dgamma, dbeta), auto):
            torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12 * float(ref.abs().max()))


def test_variance_and_mean_field_restatement(case):
    """var is the diagonal of ridge phi inv(P) phi^T; with P = ridge I it is |phi_b|^2; factor 0 returns the logits."""
    _, head, feats, _ = case
    _, _, phi = gr.features(feats, head["gamma"], head["beta"], head["W_rf"], head["b_rf"])
    P = gr.precision_update(gr.initial_precision(phi.shape[1]), phi)
    full = gr.RIDGE * phi @ torch.linalg.inv(P) @ phi.t()
    torch.testing.assert_close(gr.variance(phi, P), torch.diagonal(full), rtol=1e-12, atol=0)
    torch.testing.assert_close(gr.variance(phi, gr.initial_precision(phi.shape[1])), (phi ** 2).sum(-1), rtol=1e-12, atol=0)
    z = gr.logits(phi, head["W_out"])
    assert torch.equal(gr.mean_field(z, gr.variance(phi, P), 0.0), z)
    assert bool((gr.mean_field(z, gr.variance(phi, P), 0.4).abs() < z.abs()).all())


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE = -1, -2
BAD_BCD = [(0, 64, 64), (-1, 64, 64), (65536, 64, 64), (4, 66, 64), (4, 0, 64), (4, 2052, 64), (4, 64, 66), (4, 64, 0), (4, 64, 2052)]


def f(v):
    return C.c_float(v)


def d(v):
    return C.c_double(v)


def test_symbols_are_bound():
    from uncertainty_vit_amd import native
    for name in ("uvit_op_gp_features", "uvit_op_gp_precision_update", "uvit_op_gp_ln_grad_ws_bytes", "uvit_op_gp_ln_grad",
                 "uvit_op_gp_variance", "uvit_op_gp_mean_field"):
        assert name in native.SYMBOLS and getattr(native.lib(), name).argtypes is not None


def test_features_rejects_bad_arguments(L):
    call = lambda p, B, Cd, D, eps=1e-12: L.uvit_op_gp_features(*p[:5], f(1.0), f(eps), *p[5:], B, Cd, D, NUL)      # noqa: E731
    for B, Cd, D in BAD_BCD:
        assert call([P1] * 8, B, Cd, D) == SHAPE, (B, Cd, D)
    for i in (0, 1, 2, 3, 4, 7):                   # feat, gamma, beta, W_rf, b_rf, phi are required
        a = [P1] * 8
        a[i] = NUL
        assert call(a, 4, 64, 64) == ARG, i
    assert call([P1] * 8, 4, 64, 64, eps=-1.0) == ARG and call([P1] * 8, 4, 64, 64, eps=float("nan")) == ARG


def test_precision_update_rejects_bad_arguments(L):
    for B, D in ((0, 64), (-2, 64), (65536, 64), (4, 66), (4, 0), (4, 2052)):
        assert L.uvit_op_gp_precision_update(P1, P1, B, D, d(0.999), NUL) == SHAPE, (B, D)
    assert L.uvit_op_gp_precision_update(NUL, P1, 4, 64, d(0.999), NUL) == ARG
    assert L.uvit_op_gp_precision_update(P1, NUL, 4, 64, d(0.999), NUL) == ARG
    for m in (1.0, 1.5, float("nan")):
        assert L.uvit_op_gp_precision_update(P1, P1, 4, 64, d(m), NUL) == ARG, m


def test_ln_grad_rejects_bad_arguments(L):
    assert L.uvit_op_gp_ln_grad_ws_bytes(128, 768, 768) == 4 * (128 * 768 + 128 * 768)
    assert L.uvit_op_gp_ln_grad_ws_bytes(3, 64, 260) == 4 * (3 * 260 + 3 * 64)
    call = lambda p, B, K, Cd, D: L.uvit_op_gp_ln_grad(*p[:5], f(1.0), *p[5:], B, K, Cd, D, NUL)      # noqa: E731
    for B, Cd, D in BAD_BCD:
        assert L.uvit_op_gp_ln_grad_ws_bytes(B, Cd, D) == SHAPE, (B, Cd, D)
        assert call([P1] * 8, B, 10, Cd, D) == SHAPE, (B, Cd, D)
    assert call([P1] * 8, 4, 0, 64, 64) == SHAPE
    for i in range(8):
        a = [P1] * 8
        a[i] = NUL
        assert call(a, 4, 10, 64, 64) == ARG, i


def test_variance_rejects_bad_arguments(L):
    for B, D in ((0, 64), (65536, 64), (4, 66), (4, 0), (4, 2052)):
        assert L.uvit_op_gp_variance(P1, P1, d(1e-3), P1, B, D, NUL) == SHAPE, (B, D)
    for i in range(3):
        a = [P1] * 3
        a[i] = NUL
        assert L.uvit_op_gp_variance(a[0], a[1], d(1e-3), a[2], 4, 64, NUL) == ARG, i
    for ridge in (-1e-3, float("nan")):
        assert L.uvit_op_gp_variance(P1, P1, d(ridge), P1, 4, 64, NUL) == ARG, ridge


def test_mean_field_rejects_bad_arguments(L):
    for B, K in ((0, 10), (-1, 10), (65536, 10), (4, 0)):
        assert L.uvit_op_gp_mean_field(P1, P1, d(0.4), P1, B, K, NUL) == SHAPE, (B, K)
    for i in range(3):
        a = [P1] * 3
        a[i] = NUL
        assert L.uvit_op_gp_mean_field(a[0], a[1], d(0.4), a[2], 4, 10, NUL) == ARG, i
    for factor in (-0.1, float("nan")):
        assert L.uvit_op_gp_mean_field(P1, P1, d(factor), P1, 4, 10, NUL) == ARG, factor


# ---- the module ----
GP_KEYS = {"head.precision_matrix": (64, 64), "head._gp_input_normalize_layer.weight": (128,), "head._gp_input_normalize_layer.bias": (128,),
           "head._gp_output_layer.weight": (10, 64), "head._random_feature.weight": (64, 128), "head._random_feature.bias": (64,)}
TRAINABLE = ["head._gp_input_normalize_layer.weight", "head._gp_input_normalize_layer.bias", "head._gp_output_layer.weight"]


def test_gp_probe_state_dict_arena_and_init(case):
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    fx = case[0]
    torch.manual_seed(3)
    probe = GPProbe(tiny_encoder().eval(), 10, num_inducing=64)
    assert isinstance(probe, LinearProbe)
    sd = probe.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == GP_KEYS
    assert sorted(k[5:] for k in sd) == fx["state_dict_keys"].tolist()          # the names the reference class gives its state
    assert [n for n, p in probe.named_parameters() if p.requires_grad] == TRAINABLE
    # one arena [W_out (K D) | gamma (C) | beta (C) | pad to 4] whose decay group is W_out: one-dimensional parameters do not decay
    K, Cd, D = 10, 128, 64
    assert probe._n_decay == K * D and probe._arena.numel() == K * D + 2 * Cd and probe._arena.numel() % 4 == 0
    base = probe._arena.data_ptr()
    assert sd["head._gp_output_layer.weight"].data_ptr() == base
    assert sd["head._gp_input_normalize_layer.weight"].data_ptr() == base + 4 * K * D
    assert sd["head._gp_input_normalize_layer.bias"].data_ptr() == base + 4 * (K * D + Cd)
    # the class's own initial values
    assert bool((sd["head._gp_input_normalize_layer.weight"] == 1).all()) and bool((sd["head._gp_input_normalize_layer.bias"] == 0).all())
    assert torch.equal(sd["head.precision_matrix"], 1e-3 * torch.eye(D))
    w, b, wo = sd["head._random_feature.weight"], sd["head._random_feature.bias"], sd["head._gp_output_layer.weight"]
    assert 0.045 < float(w.std()) < 0.055 and abs(float(w.mean())) < 0.005
    assert 0.0 <= float(b.min()) and float(b.max()) <= 2 * np.pi and float(b.max()) > 5.0 and float(b.min()) < 1.0
    assert float(wo.abs().max()) <= 1 / np.sqrt(D) and float(wo.abs().max()) > 0.9 / np.sqrt(D)          # nn.Linear's default
    # loading the reference's keys goes through the views; the default D is the embed dim
    probe.load_state_dict({k: torch.full(s, 0.5) for k, s in GP_KEYS.items()})
    assert float(probe._arena.min()) == 0.5 and float(probe._P.min()) == 0.5 and float(probe._w_rf.max()) == 0.5
    probe.reset_cov()
    assert torch.equal(probe._P, 1e-3 * torch.eye(D))
    assert GPProbe(tiny_encoder().eval(), 10).num_inducing == 128
    osd = probe.optimizer_state_dict()
    assert osd["step"] == 0 and {k: tuple(v.shape) for k, v in osd["exp_avg"].items()} == {"head." + k[5:]: GP_KEYS[k] for k in TRAINABLE}
    # no CPU fallback
    with pytest.raises(UvitError):
        probe.logits(torch.zeros(2, 3, 48, 48))
    with pytest.raises(UvitError):
        probe.predictive_variance(torch.zeros(2, 3, 48, 48))
    with pytest.raises(UvitError):
        probe.train_step(torch.zeros(2, 3, 48, 48), torch.zeros(2, dtype=torch.int64), 1e-3, 0.05)


def test_gp_probe_rejects_what_is_not_built():
    from uncertainty_vit_amd.gp_probe import GPProbe
    with pytest.raises(NotImplementedError):
        GPProbe(tiny_encoder(two_stream=True).eval(), 10)
    for bad in (66, 0, 2052):
        with pytest.raises(ValueError):
            GPProbe(tiny_encoder().eval(), 10, num_inducing=bad)
    with pytest.raises(ValueError):
        GPProbe(tiny_encoder().eval(), 10, cov_ridge_penalty=0.0)
    with pytest.raises(ValueError):
        GPProbe(tiny_encoder().eval(), 10, cov_momentum=1.0)


def test_linear_probe_is_what_it_was():
    """Importing the GP module leaves the linear head's state, arena and draws alone."""
    import uncertainty_vit_amd.gp_probe  # noqa: F401
    from uncertainty_vit_amd.linear_probe import LinearProbe, _timm_trunc_normal_
    torch.manual_seed(3)
    probe = LinearProbe(tiny_encoder().eval(), 10)
    torch.manual_seed(3)
    tiny_encoder()
    want = _timm_trunc_normal_(torch.empty(10, 128), std=0.02).mul_(0.001)
    assert list(probe.state_dict()) == ["head.weight", "head.bias"] and torch.equal(probe.head.weight.data, want)
    assert probe._arena.numel() == 10 * 128 + 12 and probe._n_decay == 10 * 128


def test_cli_flags_are_absent_unless_given():
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()                                  # the parsed defaults without --gp_layer equal today's
    got = vars(rlp.get_args([]))
    assert not [k for k in got if k.startswith("gp_")]
    a = rlp.get_args(["--gp_layer"])
    assert a.gp_layer is True and not any(hasattr(a, k) for k in rlp.GP_FLAGS)
    a = rlp.get_args(["--gp_layer", "--gp_num_inducing", "64", "--gp_cov_momentum", "0", "--gp_cov_ridge_penalty", "0.01",
                      "--gp_kernel_scale", "2.0", "--gp_mean_field", "0.4"])
    assert (a.gp_num_inducing, a.gp_cov_momentum, a.gp_cov_ridge_penalty, a.gp_kernel_scale, a.gp_mean_field) == (64, 0.0, 0.01, 2.0, 0.4)
    assert rlp.gp_variance_line({"gp_var_mean": 0.25}) == "* GP variance mean 0.250000"
