"""Learned layer weights without a GPU: the float64 restatement of tests/lw_ref.py against torch's own
expressions and autograd and against what the reference classifier computed (tests/golden/probe_lw_t48.npz, written by
tools/gen_golden_probe_lw.py), the argument checks of the five entry points (they return before anything touches a device), the
exported symbols, the module's refusals and state dict, and the command line."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lw_ref as lr
import probe_ref as pr

F64 = torch.float64
COMBOS = [(False, False), (False, True), (True, False), (True, True)]      # (use_cls, layernorm_before_combine)
RT, AT = 2e-4, 1e-5      # tests/test_host_probe.py: fp32 round-off between two eager CPU formulations


# ---- the restatement against torch ----
def log_weights(L, kind):
    if kind == "spread":
        return lr.log_w_case(L).to(F64)
    v = lr.log_w_case(L, seed=9).to(F64)              # saturated: +-30 at the ends, the softmax's smallest weight is about e^-60
    v[0], v[-1] = 30.0, -30.0 if L > 1 else 30.0
    return v


@pytest.mark.parametrize("kind", ["spread", "saturated"])
@pytest.mark.parametrize("L", [1, 2, 12])
@pytest.mark.parametrize("use_cls,ln", COMBOS)
def test_restatement_is_the_torch_expression_and_its_autograd(use_cls, ln, L, kind):
    """stack, softmax, F.linear and F.layer_norm as modeling_finetune.py:499-510 writes them, in float64, and torch.autograd of the
    smoothed cross-entropy behind them.  Two float64 evaluations of the same expressions: 1e-12 relative to each tensor's maximum."""
    B, N, Cd, K = 3, 5, 8, 6
    xs = [lr.rnd(B, N, Cd, seed=30 + l).to(F64) + 0.5 * l for l in range(L)]
    W, bias = lr.rnd(K, Cd, seed=1, scale=0.3).to(F64).requires_grad_(), lr.rnd(K, seed=2, scale=0.1).to(F64).requires_grad_()
    log_w = log_weights(L, kind).requires_grad_()
    labels = torch.tensor([0, K - 1, 2])
    layer_xs = [x[:, 0] if use_cls else x.mean(1) for x in xs]
    layer_xs = [F.layer_norm(p, p.shape[-1:]) if ln else p for p in layer_xs]
    feat = F.linear(torch.stack(layer_xs, -1), log_w.softmax(-1))
    logits = F.linear(feat, W, bias)
    loss = pr.smoothed_ce(logits, labels, 0.1)[1]
    gW, gb, gl = torch.autograd.grad(loss, (W, bias, log_w))

    pooled = lr.pool(xs, 1 if use_cls else 0, ln)
    assert pooled.shape == (B, L, Cd)
    r = lr.step(pooled, W.detach(), bias.detach(), log_w.detach(), labels, 0.1)
    for got, ref in ((pooled, torch.stack(layer_xs, 1)), (r["feat"], feat), (r["logits"], logits), (r["loss"], loss), (r["dW"], gW),
                     (r["dbias"], gb), (r["dlog_w"], gl)):
        ref = ref.detach()
        assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1e-3)
    assert float(lr.softmax_w(log_w.detach()).sum()) == pytest.approx(1.0, abs=1e-14)
    if L == 1:
        assert torch.equal(r["feat"], pooled[:, 0]) and float(r["dlog_w"].abs().max()) == 0.0      # one layer: w = 1, no gradient


def test_identical_layers_have_no_layer_gradient():
    """Every g_l is equal, so w_l (g_l - sum_j w_j g_j) = 0 up to the rounding of sum_j w_j: what the gradient's bound is relative to."""
    pooled = lr.rnd(4, 1, 16, seed=3).to(F64).expand(4, 5, 16).contiguous()
    dfeat, log_w = lr.rnd(4, 16, seed=4).to(F64), lr.log_w_case(5).to(F64)
    d, g = lr.lw_grad(dfeat, pooled, log_w)
    assert float((g - g[0]).abs().max()) == 0.0
    assert float(d.abs().max()) <= 8 * lr.UD * lr.lw_grad_scale(dfeat, pooled)
    assert float(lr.lw_grad_bound(dfeat.float(), pooled.float(), log_w.float()).min()) > 0.0


# ---- the restatement against the reference's fixture ----
@pytest.fixture(scope="module")
def case(golden_dir):
    import os
    return pr.load_fixture(golden_dir), np.load(os.path.join(golden_dir, "probe_lw_t48.npz"))


def close(got, ref, rtol, atol, what):
    torch.testing.assert_close(got.float(), torch.from_numpy(np.asarray(ref)).float(), rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def test_fixture_is_data_only(case):
    _, lw = case
    assert lw["combos"].tolist() == [[int(a), int(b)] for a, b in COMBOS] and int(lw["steps"]) == 3
    assert lw["layer_log_weights"].tolist() == pytest.approx([0.7, -0.4]) and not [k for k in lw.files if k.startswith("enc")]
    assert all(lw[k].dtype.kind in "fi" for k in lw.files)


@pytest.mark.parametrize("c", range(4))
def test_lw_ref_reproduces_reference(case, c):
    """Features, logits, loss, the three gradients and the three parameters after three AdamW steps against the reference's fp32
    results, with the tolerances tests/test_host_probe.py has for the same encoder.  The layer gradient cancels: the reference's own
    fp32 sum of B C products leaves up to 2 B C u S on it (S = sum |dfeat| |pooled|, lw_ref.lw_grad_scale), which is its atol."""
    (fx, cfg, enc, W, bias, images, labels), lw = case
    use_cls, ln = COMBOS[c]
    log_w = torch.from_numpy(lw["layer_log_weights"])
    s, lrate, wd = float(fx["smoothing"]), float(fx["lr"]), float(fx["weight_decay"])
    key = f"c{c}/"
    pooled = lr.pool(lr.layer_streams(enc, cfg, images), 1 if use_cls else 0, ln)
    assert pooled.shape == (images.shape[0], cfg.depth, cfg.embed_dim)
    close(lr.features(enc, cfg, images, log_w, use_cls, ln), lw[key + "features"], RT, AT, "features")
    losses, _, r, (Wn, bn, ln_) = lr.train_steps(pooled, W, bias, log_w, labels, s, lrate, wd, 3)
    close(r["logits"], lw[key + "logits"], RT, AT, "logits")
    assert float(r["loss"]) == pytest.approx(float(lw[key + "loss"]), rel=2e-4)
    close(r["dW"], lw[key + "grad/weight"], 2e-3, 2e-7, "head.weight gradient")
    close(r["dbias"], lw[key + "grad/bias"], 2e-3, 2e-7, "head.bias gradient")
    B, _, Cd = pooled.shape
    S = lr.lw_grad_scale(r["dfeat"], pooled)
    print(f"\ncombo {c}: dlog_w {r['dlog_w'].tolist()} reference {lw[key + 'grad/layer_log_weights'].tolist()}, S {S:.3e}, atol {2 * B * Cd * lr.U * S:.3e}")
    close(r["dlog_w"], lw[key + "grad/layer_log_weights"], 2e-3, 2 * B * Cd * lr.U * S, "layer_log_weights gradient")
    assert float(r["dlog_w"].abs().min()) > 2 * 2 * B * Cd * lr.U * S           # the gradient stands clear of that worst case
    np.testing.assert_allclose(losses, lw[key + "step_loss"], rtol=2e-4)
    close(Wn, lw[key + "post/weight"], 1e-3, 2e-5, "head.weight after 3 steps")
    close(bn, lw[key + "post/bias"], 1e-3, 2e-5, "head.bias after 3 steps")
    close(ln_, lw[key + "post/layer_log_weights"], 1e-3, 2e-5, "layer_log_weights after 3 steps")
    assert float((ln_.float() - log_w).abs().min()) > 1e-3                      # three steps of lr 1e-3 did move both weights


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL, 16-byte aligned pointer: the checks return before it is used
ODD = C.c_void_p(4100)     # 4-byte aligned only
NUL = C.c_void_p(0)
ARG, SHAPE = -1, -2
BAD_BLC = [(0, 2, 64), (-1, 2, 64), (65536, 2, 64), (4, 0, 64), (4, 65, 64), (4, -1, 64), (4, 2, 66), (4, 2, 0), (4, 2, 2052)]      # (B, L, C)
NAMES = ("uvit_op_lw_pool_ws_bytes", "uvit_op_lw_pool", "uvit_op_lw_combine", "uvit_op_probe_input_grad", "uvit_op_lw_grad")


def f(v):
    return C.c_float(v)


def layer_array(n, hole=None):
    return (C.c_void_p * max(n, 1))(*[None if l == hole else 4096 + 64 * l for l in range(max(n, 1))])


def test_symbols_are_bound():
    from uncertainty_vit_amd import native
    for name in NAMES:
        assert name in native.SYMBOLS and getattr(native.lib(), name).argtypes is not None
    assert native.lib().uvit_version() == 100 and native.MAX_DEPTH == 64


def test_pool_rejects_bad_arguments(L):
    assert L.uvit_op_lw_pool_ws_bytes(128, 12, 197, 768) == 128 * 12 * 8 * 768 * 4
    assert L.uvit_op_lw_pool_ws_bytes(1, 64, 1, 2048) == 64 * 8 * 2048 * 4
    call = lambda x, pooled, scratch, B=4, Ln=2, N=5, Cd=64, mode=0, ln=0, eps=1e-5: \
        L.uvit_op_lw_pool(x, Ln, pooled, scratch, B, N, Cd, mode, ln, f(eps), NUL)      # noqa: E731
    for B, Ln, Cd in BAD_BLC:
        assert L.uvit_op_lw_pool_ws_bytes(B, Ln, 5, Cd) == SHAPE, (B, Ln, Cd)
        assert call(layer_array(Ln), P1, P1, B=B, Ln=Ln, Cd=Cd) == SHAPE, (B, Ln, Cd)
    for N in (0, -3):
        assert L.uvit_op_lw_pool_ws_bytes(4, 2, N, 64) == SHAPE and call(layer_array(2), P1, P1, N=N) == SHAPE
    x = layer_array(2)
    assert call(None, P1, P1) == ARG and call(x, NUL, P1) == ARG and call(x, P1, NUL) == ARG
    for hole in (0, 1):
        assert call(layer_array(2, hole=hole), P1, P1) == ARG, hole          # a NULL layer pointer
    for mode in (-1, 2):
        assert call(x, P1, P1, mode=mode) == ARG, mode
    for ln in (-1, 2):
        assert call(x, P1, P1, ln=ln) == ARG, ln
    for eps in (-1e-5, float("nan")):
        assert call(x, P1, P1, ln=1, eps=eps) == ARG, eps


def test_combine_rejects_bad_arguments(L):
    call = lambda pooled, log_w, feat, shape=(4, 2, 64), w_out=P1: L.uvit_op_lw_combine(pooled, log_w, feat, w_out, *shape, NUL)      # noqa: E731
    assert call(NUL, P1, P1) == ARG and call(P1, NUL, P1) == ARG and call(P1, P1, NUL) == ARG
    for shape in BAD_BLC:
        assert call(P1, P1, P1, shape=shape) == SHAPE, shape
        assert call(P1, P1, P1, shape=shape, w_out=NUL) == SHAPE, shape      # w_out may be NULL: the shape is still checked


def test_input_grad_rejects_bad_arguments(L):
    for B, K, Cd in ((0, 10, 64), (4, 0, 64), (4, 10, 66), (4, 10, 0), (-3, 10, 64), (4, -1, 64)):
        assert L.uvit_op_probe_input_grad(P1, P1, P1, B, K, Cd, NUL) == SHAPE, (B, K, Cd)
    for i in range(3):
        a = [P1] * 3
        a[i] = NUL
        assert L.uvit_op_probe_input_grad(*a, 4, 10, 64, NUL) == ARG, i


def test_grad_rejects_bad_arguments(L):
    call = lambda a, shape=(4, 2, 64): L.uvit_op_lw_grad(*a, *shape, NUL)      # noqa: E731
    for i in range(5):
        a = [P1] * 5                                  # dfeat, pooled, log_w, dlog_w, scratch
        a[i] = NUL
        assert call(a) == ARG, i
    assert call([P1, P1, P1, P1, ODD]) == ARG         # the scratch holds doubles
    for shape in BAD_BLC:
        assert call([P1] * 5, shape=shape) == SHAPE, shape


# ---- the module ----
def tiny_encoder(depth=3, two_stream=False):
    from uncertainty_vit_amd.modeling_cyclical import DistVisionTransformerForCyclicalTraining, VisionTransformerForCyclicalTraining
    cls = DistVisionTransformerForCyclicalTraining if two_stream else VisionTransformerForCyclicalTraining
    return cls(img_size=48, patch_size=16, embed_dim=128, depth=depth, num_heads=2, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
               init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)


def test_probe_state_dict_and_arena():
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.lw_probe import LW_LN_EPS, LayerWeightedProbe
    from uncertainty_vit_amd.native import UvitError
    torch.manual_seed(3)
    probe = LayerWeightedProbe(tiny_encoder().eval(), 10, use_cls=True, layernorm_before_combine=True)
    torch.manual_seed(3)
    lin = LinearProbe(tiny_encoder().eval(), 10)
    assert isinstance(probe, LinearProbe) and (probe.depth, probe.use_cls, probe.layernorm_before_combine) == (3, True, True)
    assert LW_LN_EPS == lr.LN_EPS == 1e-5
    sd = probe.state_dict()
    assert sorted(sd) == ["head.bias", "head.weight", "layer_log_weights"]                      # the reference's names
    assert sorted(n for n, p in probe.named_parameters() if p.requires_grad) == sorted(sd)
    assert torch.equal(sd["head.weight"], lin.state_dict()["head.weight"])                      # the head starts as a linear probe's
    assert sd["layer_log_weights"].tolist() == [0.0, 0.0, 0.0]                                  # modeling_finetune.py:436
    # one arena [W | bias, padded to 4 | layer_log_weights, padded to 4] whose decay group is W: the log-weights do not decay
    assert probe._arena.numel() == 10 * 128 + 12 + 4 and probe._n_decay == 10 * 128
    assert sd["layer_log_weights"].data_ptr() == probe._arena.data_ptr() + 4 * (10 * 128 + 12)
    assert probe.layer_log_weights.grad.data_ptr() == probe._grad_arena.data_ptr() + 4 * (10 * 128 + 12)
    probe.load_state_dict({"head.weight": torch.full((10, 128), 0.5), "head.bias": torch.arange(10.0),
                           "layer_log_weights": torch.tensor([1.0, 2.0, 3.0])})
    assert probe._arena[1292:].tolist() == [1.0, 2.0, 3.0, 0.0] and probe._arena[1280:1290].tolist() == list(range(10))
    # the optimizer state carries the three names
    osd = probe.optimizer_state_dict()
    assert sorted(osd["exp_avg"]) == sorted(sd) and tuple(osd["exp_avg_sq"]["layer_log_weights"].shape) == (3,)
    osd["exp_avg"]["layer_log_weights"] = torch.tensor([0.25, 0.5, 0.75])
    osd["step"] = 7
    probe.load_optimizer_state_dict(osd)
    assert probe.exp_avg[1292:1295].tolist() == [0.25, 0.5, 0.75] and probe.step_count == 7
    x = torch.zeros(2, 3, 48, 48)                                                               # no CPU fallback
    for call in (probe.logits, probe.features):
        with pytest.raises(UvitError):
            call(x)
    with pytest.raises(UvitError):
        probe.layer_weights()
    with pytest.raises(UvitError):
        probe.train_step(x, torch.zeros(2, dtype=torch.int64), 1e-3, 0.05)


def test_probe_rejects_what_is_not_built():
    from uncertainty_vit_amd.lw_probe import LayerWeightedProbe
    with pytest.raises(NotImplementedError):
        LayerWeightedProbe(tiny_encoder(two_stream=True).eval(), 10)
    with pytest.raises(ValueError):
        LayerWeightedProbe(tiny_encoder().train(), 10)             # the encoder must be frozen in eval mode
    with pytest.raises(ValueError):
        LayerWeightedProbe(tiny_encoder().eval(), 0)


def test_state_dict_refusals():
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.lw_probe import LayerWeightedProbe
    probe = LayerWeightedProbe(tiny_encoder(depth=3).eval(), 10)
    before = probe._arena.clone()
    with pytest.raises(KeyError, match="layer_log_weights"):
        probe.load_state_dict(LinearProbe(tiny_encoder().eval(), 10).state_dict())              # a linear probe's checkpoint
    with pytest.raises(ValueError, match="another depth"):
        probe.load_state_dict(LayerWeightedProbe(tiny_encoder(depth=2).eval(), 10).state_dict())
    assert torch.equal(probe._arena, before)
    probe.load_state_dict(LayerWeightedProbe(tiny_encoder(depth=3).eval(), 10).state_dict())


# ---- the command line ----
def test_cli(monkeypatch, capsys):
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()                                  # the parsed defaults without the flags equal today's
    flags = ("learn_layer_weights", "layernorm_before_combine", "use_cls")
    assert not [k for k in vars(rlp.get_args([])) if k in flags]
    assert rlp.check_lw_flags(rlp.get_args([])) is False
    a = rlp.get_args(["--learn_layer_weights", "--layernorm_before_combine", "--use_cls"])
    assert rlp.check_lw_flags(a) is True and all(getattr(a, k) is True for k in flags)
    assert rlp.layer_weights_line([0.25, 0.5, 0.125, 0.125]) == "* Layer weights 0.2500 0.5000 0.1250 0.1250 (argmax: block 1)"
    # the errors come before anything is loaded
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    base = ["--nb_classes", "10", "--finetune", "none.pth"]
    for alone in (["--layernorm_before_combine"], ["--use_cls"], ["--use_cls", "--layernorm_before_combine"]):
        with pytest.raises(ValueError, match="--learn_layer_weights"):
            rlp.main(rlp.get_args(base + alone))
    for other in (["--gp_layer"], ["--het_layer"], ["--ensembles"], ["--laplace"], ["--mc_dropout_forwards", "4", "--attn_drop_rate", "0.1"]):
        with pytest.raises(ValueError, match="mixes the features of the linear head"):
            rlp.main(rlp.get_args(base + ["--learn_layer_weights"] + other))
    capsys.readouterr()
    # what it works with passes the flag checks and stops at the checkpoint that does not exist; --target_layer is ignored with its line
    for extra in (["--calibration"], ["--eval", "--detection"], ["--eval", "--ts_temperature", "1.5"], ["--eval", "--vim_state", "v.pth"],
                  ["--eval", "--maha_state", "m.pth", "--knn_state", "k.pth"], ["--eval", "--perturbation_path", "p"],
                  ["--layernorm_before_combine", "--use_cls"]):
        with pytest.raises(FileNotFoundError):
            rlp.main(rlp.get_args(base + ["--learn_layer_weights"] + extra))
    assert "supersedes --target_layer" not in capsys.readouterr().out
    with pytest.raises(FileNotFoundError):
        rlp.main(rlp.get_args(base + ["--learn_layer_weights", "--target_layer", "7"]))
    assert "--learn_layer_weights supersedes --target_layer 7: the encoder keeps every block" in capsys.readouterr().out
