"""CPU: the two-stream probe's host side (uncertainty-vit_amd/dist_probe.py, run_linear_probe.py), the argument checks of its two ops
(csrc/dprobe.hip: they return before any launch) and the restatement its GPU tests compare against (tests/dprobe_ref.py)."""
from functools import partial

import numpy as np
import pytest
import torch

import detect_ref as dr
import dprobe_ref as dp


def tiny_encoder(two_stream=True, depth=2):
    from uncertainty_vit_amd.modeling_cyclical import DistVisionTransformerForCyclicalTraining, VisionTransformerForCyclicalTraining
    cls = DistVisionTransformerForCyclicalTraining if two_stream else VisionTransformerForCyclicalTraining
    return cls(img_size=48, patch_size=16, embed_dim=128, depth=depth, num_heads=2, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
               init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_dist_probe_takes_a_two_stream_encoder_in_eval_mode():
    from uncertainty_vit_amd.dist_probe import DistProbe
    with pytest.raises(TypeError):
        DistProbe(tiny_encoder(two_stream=False).eval(), 10)
    with pytest.raises(TypeError):
        DistProbe(torch.nn.Linear(4, 4), 10)
    with pytest.raises(ValueError, match="eval"):
        DistProbe(tiny_encoder(), 10)                                        # training mode
    for kw in (dict(num_classes=1), dict(num_classes=4097), dict(mean_field=-0.1), dict(mean_field=float("inf")), dict(var_scale=0.0),
               dict(var_scale=float("nan")), dict(smoothing=1.0)):
        with pytest.raises(ValueError):
            DistProbe(tiny_encoder().eval(), **{"num_classes": 10, **kw})
    probe = DistProbe(tiny_encoder().eval(), 10, mean_field=0.25, var_scale=2.0)
    assert (probe.mean_field, probe.var_scale) == (0.25, 2.0)
    assert DistProbe.DETECT_COLUMNS == ("msp", "entropy", "energy", "dist_var", "dist_trace")


def test_the_other_heads_still_refuse_a_two_stream_encoder():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.lw_probe import LayerWeightedProbe
    from uncertainty_vit_amd.mcd_probe import MCDropoutProbe
    for cls in (LinearProbe, GPProbe, HetProbe, EnsembleProbe, LaplaceProbe, LayerWeightedProbe):
        with pytest.raises(NotImplementedError):
            cls(tiny_encoder().eval(), 10)
    enc = tiny_encoder()
    enc.attn_drop_rate = 0.1                                                 # past the probe's own check of the rate
    with pytest.raises(NotImplementedError):
        MCDropoutProbe(enc.eval(), 10)


# ------------------------------------------------------------------------------------------------------------------------- state
def test_state_dict_and_arena_are_the_linear_probe_s():
    from uncertainty_vit_amd.dist_probe import DistProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    enc2, enc1 = tiny_encoder().eval(), tiny_encoder(two_stream=False).eval()
    torch.manual_seed(3)
    dist = DistProbe(enc2, 10)
    torch.manual_seed(3)
    lin = LinearProbe(enc1, 10)
    sd, ref = dist.state_dict(), lin.state_dict()
    assert list(sd) == list(ref) == ["head.weight", "head.bias"]
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"head.weight": (10, 128), "head.bias": (10,)}
    assert torch.equal(dist._arena, lin._arena) and dist._n_decay == lin._n_decay == 10 * 128     # the same draw into the same layout
    assert [(lo, hi, shape) for _, lo, hi, shape in dist._views()] == [(lo, hi, shape) for _, lo, hi, shape in lin._views()]
    assert set(dist.optimizer_state_dict()) == set(lin.optimizer_state_dict())
    dist.load_state_dict({k: v + 1.0 for k, v in ref.items()})                # a linear probe-N.pth resumes
    assert torch.equal(dist.head.weight.data, ref["head.weight"] + 1.0) and dist.head.weight.data_ptr() == dist._arena.data_ptr()
    x = torch.zeros(2, 3, 48, 48)
    for call in (dist.features, dist.cov_features, dist.feature_variance, dist.predictive_variance, dist.logits):
        with pytest.raises(UvitError):                                       # no CPU fallback
            call(x)


def test_build_probe_encoder_cuts_a_two_stream_model():
    from uncertainty_vit_amd.linear_probe import build_probe_encoder
    from uncertainty_vit_amd.modeling_cyclical import DistVisionTransformerForCyclicalTraining
    enc = build_probe_encoder("dist_beit_base_patch16_224", target_layer=1, init_values=0.1, use_shared_rel_pos_bias=True,
                              use_abs_pos_emb=False)
    assert isinstance(enc, DistVisionTransformerForCyclicalTraining) and enc._two_stream and enc.depth == 2 and not enc.training
    assert len(enc.blocks) == 2 and hasattr(enc.blocks[1].attn, "cov_proj")


# ------------------------------------------------------------------------------------------------------------------- CLI arguments
def test_cli_dist_flags():
    import run_linear_probe as rlp
    base = ["--model", "beit_base_patch16_224", "--nb_classes", "3", "--finetune", "x.pth"]
    assert rlp.check_dist_flags(rlp.get_args(base), two_stream=False) is None
    for extra in (["--dist_mean_field", "0.3927"], ["--dist_var_scale", "2.0"], ["--dist_mean_field", "0"]):
        with pytest.raises(ValueError, match="two-stream"):
            rlp.check_dist_flags(rlp.get_args(base + extra), two_stream=False)
    assert rlp.check_dist_flags(rlp.get_args(base), two_stream=True) == {"mean_field": 0.0, "var_scale": 1.0}
    got = rlp.check_dist_flags(rlp.get_args(base + ["--dist_mean_field", "0.3927", "--dist_var_scale", "0.5"]), two_stream=True)
    assert got == {"mean_field": 0.3927, "var_scale": 0.5}
    for extra in (["--dist_mean_field", "-1"], ["--dist_mean_field", "inf"], ["--dist_var_scale", "0"], ["--dist_var_scale", "nan"],
                  ["--eval", "--dist_mean_field", "0.3927", "--vim_data_path", "d"]):
        with pytest.raises(ValueError):
            rlp.check_dist_flags(rlp.get_args(base + extra), two_stream=True)
    assert rlp.check_dist_flags(rlp.get_args(base + ["--eval", "--vim_data_path", "d"]), two_stream=True) is not None      # affine at factor 0
    assert "dist_mean_field" not in vars(rlp.get_args(base))                 # absent unless given: the printed arguments are what they were
    line = rlp.dist_variance_line({"dist_var_mean": 0.5, "dist_trace_mean": 1.25})
    assert line == "* Dist variance mean 0.500000 trace mean 1.250000"


# --------------------------------------------------------------------------------------------------------- argument checks of the ops
def test_ops_reject_bad_arguments():
    from uncertainty_vit_amd import native
    hdr = open(native.LIB_PATH.replace("uncertainty-vit_amd/libuvit.so", "include/uvit.h")).read()
    for name in ("uvit_op_dprobe_pool_ws_bytes", "uvit_op_dprobe_pool_norm", "uvit_op_dprobe_variance"):
        assert name in native.SYMBOLS and name + "(" in hdr
    for what, got, want in dp.bad_calls(native.lib()):
        assert got == want, (what, got, want)


# ------------------------------------------------------------------------------------------------------- the restatement's exact cases
def test_restatement_exact_cases():
    rng = np.random.default_rng(0)
    W = rng.standard_normal((7, 32)).astype(np.float32)
    w2sum = np.cumsum(W.astype(np.float64) ** 2, axis=-1)[:, -1]
    for s in (1.0, 0.5, 4.0):                                                # powers of two: s w^2 is exact
        var = dp.variance_chain(np.zeros((3, 32), np.float32), W, s)          # c = 0: v = s exp(0) = s
        assert np.array_equal(var, np.broadcast_to(s * w2sum, (3, 7)))
        assert np.array_equal(dp.trace(np.zeros((3, 32), np.float32), s), np.full(3, s))
    c = rng.standard_normal((4, 32)).astype(np.float32) * 3
    c[0, 5], c[1, 5], c[2, 5] = 0.0, -100.0, 50.0
    onehot = np.zeros((2, 32), np.float32)
    onehot[0, 5], onehot[1, 31] = 1.0, -1.0
    v = dp.feature_variance(c, 0.75)
    for fn in (dp.variance, dp.variance_chain):
        assert np.array_equal(fn(c, onehot, 0.75), v[:, [5, 31]])              # a one-hot row of W picks v_c
    assert v[0, 5] == 0.75 and v[1, 5] == 0.75 * np.exp(-100.0) and v[2, 5] == 0.75 * 51.0 and (v > 0).all()
    assert np.allclose(dp.variance(c, W, 0.75), dp.variance_chain(c, W, 0.75), rtol=32 * 2.0 ** -52, atol=0)
    bad = c.copy()
    bad[2, 7] = np.nan
    var = dp.variance(bad, W)
    assert np.isnan(var[2]).all() and np.isnan(dp.trace(bad)[2]) and np.isfinite(np.delete(var, 2, 0)).all()
    z = rng.standard_normal((4, 7)).astype(np.float32)
    assert np.array_equal(dp.link(z, dp.variance(c, W), 0.0), z.astype(np.float64))
    assert (np.abs(dp.link(z, dp.variance(c, W), np.pi / 8)) < np.abs(z)).all()
    x = rng.standard_normal((2, 10, 32)).astype(np.float32)
    f = dp.pool_norm(x)
    assert np.allclose(f.mean(-1), 0, atol=1e-12) and np.allclose((f * f).mean(-1), 1, atol=1e-4)
    f32 = torch.nn.functional.layer_norm(torch.from_numpy(x)[:, 1:].mean(1), (32,), eps=1e-6).numpy()
    assert (np.abs(f32 - f) <= dp.pool_norm_bound(x)).all()                  # torch's fp32 in another order is inside the derived bound


# ---------------------------------------------------------------------------------------------------------------- a hand-made case
def test_covariance_columns_separate_what_the_logits_cannot():
    """Two groups of six rows with the same six mean features, so the same logits row for row: msp, entropy and energy are tied
    across the groups and rank them at AUROC 0.5.  The covariance features differ: about -3 in group 0 and +3 in group 1, so every v
    of group 1 exceeds every v of group 0 by a factor (checked below) that is larger than the spread of sum_c W[k, c]^2 over the
    classes: whatever class a row predicts, var of a group-1 row is above var of any group-0 row, and so is the trace: dist_var and
    dist_trace rank the groups at AUROC 1.0."""
    rng = np.random.default_rng(1)
    Cd, K, n = 16, 5, 6
    W = rng.standard_normal((K, Cd)).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    m = np.tile(rng.standard_normal((n, Cd)).astype(np.float32), (2, 1))
    c = (rng.standard_normal((2 * n, Cd)) * 0.1).astype(np.float32) - 3.0
    c[n:] += 6.0
    v, w2 = dp.feature_variance(c), (W.astype(np.float64) ** 2).sum(-1)
    assert v[n:].min() / v[:n].max() > w2.max() / w2.min()
    flags = np.repeat([0, 1], n).astype(np.uint8)
    z = (m.astype(np.float64) @ W.astype(np.float64).T + b).astype(np.float32)
    assert np.array_equal(z[:n], z[n:])
    var = dp.variance(c, W)
    zl = dp.link(z, var, 0.0).astype(np.float32)
    scores, _, _ = dr.row_scores(zl)
    for col in scores:
        assert dr.metrics(col, flags)["AUROC"] == 0.5
    for col in (dp.predicted_variance(z, var), dp.trace(c)):
        got = dr.metrics(col.astype(np.float32), flags)
        assert got["AUROC"] == 1.0 and got["FPR95"] == 0.0
    # under the link the groups' logits differ, and the larger variance flattens group 1: its msp uncertainty is larger row for row
    s1, _, _ = dr.row_scores(dp.link(z, var, np.pi / 8).astype(np.float32))
    assert (s1[0][n:] > s1[0][:n]).all()
