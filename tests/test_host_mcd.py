"""MC-dropout without a GPU: the float64 restatement of tests/mcd_ref.py against a brute-force evaluation of
the definitions, what the five columns mean, the argument checks of the three ops and of uvit_engine_forward_tail, the exported
symbols, the constructor's refusals and the command line."""
import ctypes as C
import math
from functools import partial

import numpy as np
import pytest
import torch

import mcd_ref as mr


def stacks():
    """name -> (T, B, K) fp32: random, tied (whole numbers), saturated (|z| up to 80)."""
    rng = np.random.default_rng(11)
    out = {f"random{s}": mr.logits_case(s) for s in mr.SHAPES}
    out["tied"] = rng.integers(-2, 3, size=(4, 9, 7)).astype(np.float32)
    sat = rng.uniform(-80.0, 80.0, size=(3, 6, 12)).astype(np.float32)
    sat[:, 0, :] = 80.0                                  # flat at the edge
    sat[:, 1, 3] = 80.0
    sat[:, 1, 4:] = -80.0
    out["saturated"] = sat
    return out


@pytest.mark.parametrize("name", list(stacks()))
@pytest.mark.parametrize("mode", [0, 1])
def test_restatement_is_the_definition(name, mode):
    x = stacks()[name]
    T, B, K = x.shape
    z, unc, kstar, state = mr.combine(x, mode)
    zb, ub, kb = mr.brute(x, mode)
    fin = np.isfinite(zb)
    assert np.array_equal(fin, np.isfinite(z))
    np.testing.assert_allclose(z[fin], zb[fin], rtol=1e-13, atol=1e-13)
    assert np.array_equal(kstar, kb)
    np.testing.assert_allclose(unc[:, :3], ub[:, :3], rtol=0, atol=1e-12 * (1 + math.log(K)))
    # the raw-moment variance against the centred one: both double, the difference is rounding relative to the second moment
    np.testing.assert_allclose(unc[:, 3], ub[:, 3], rtol=0, atol=(T + 8) * mr.UD)
    np.testing.assert_allclose(unc[:, 4], ub[:, 4], rtol=0, atol=2 * mr.UD)      # 1 - votes / T against differing / T: two roundings
    assert state["votes"].sum(-1).tolist() == [T] * B and not state["flag"].any()
    assert (unc[:, 2] >= 0).all() and (unc[:, 3] >= 0).all() and ((unc[:, 4] >= 0) & (unc[:, 4] <= 1)).all()
    if T == 1:        # one pass: no epistemic part
        assert np.abs(unc[:, 2]).max() <= 1e-12 and (unc[:, 3] <= 8 * mr.UD).all() and (unc[:, 4] == 0).all()


def test_ties_take_the_lowest_index():
    x = np.zeros((2, 3, 5), dtype=np.float32)
    x[:, 1, [2, 4]] = 3.0                                # row 1: classes 2 and 4 tie in every pass
    x[0, 2, 1], x[1, 2, 3] = 2.0, 2.0                    # row 2: pass 0 says 1, pass 1 says 3; their mean ties 1 and 3
    for mode in (0, 1):
        z, unc, kstar, state = mr.combine(x, mode)
        assert kstar.tolist() == [0, 2, 1]
        assert state["votes"][1].tolist() == [0, 0, 2, 0, 0] and state["votes"][2].tolist() == [0, 1, 0, 1, 0]
        assert unc[:, 4].tolist() == [0.0, 0.0, 0.5]


def test_bad_rows_give_nan_and_leave_their_neighbours():
    x = mr.logits_case((4, 6, 3))
    clean = mr.combine(x, 0)[1]
    y = x.copy()
    y[1, 2, 4] = np.nan
    y[2, 3, 0] = np.inf
    z, unc, kstar, state = mr.combine(y, 0)
    assert state["flag"].tolist() == [False, False, True, True]
    assert np.isnan(unc[2:]).all() and np.array_equal(unc[:2], clean[:2])


def test_mi_finds_disagreement_where_entropy_cannot():
    """The hand-made case of mcd_ref.meaning_case: 12 rows whose 8 passes agree on a flat distribution against 12 rows whose passes
    are each confident of another class.  Positive = the passes disagree.  Recorded: AUROC of mcd_mi 1.0, of mcd_disagreement 1.0,
    of mcd_var 1.0, in both modes; AUROC of the entropy of the combined logits 0.4028 with combine="logits", the reference's
    combination (the mean of eight one-hot logit rows is as flat as the flat rows: chance).  With combine="probs" both groups sit
    within 2e-3 nats of ln 8 and the entropy happens to order them (AUROC 1.0 on a margin that small); the claim is about "logits"."""
    x, flags = mr.meaning_case()
    got = {}
    for mode in (0, 1):
        z, unc, _, _ = mr.combine(x, mode)
        got[mode] = (mr.auroc(unc[:, 2], flags), mr.auroc(mr.entropy_of_logits(z.astype(np.float32)), flags))
        assert mr.auroc(unc[:, 2], flags) == 1.0 and mr.auroc(unc[:, 4], flags) == 1.0 and mr.auroc(unc[:, 3], flags) == 1.0
        # the flat rows: no mutual information; the others: nearly all of their entropy is mutual information
        assert unc[~flags, 2].max() < 1e-12 and (unc[flags, 2] > 0.9 * unc[flags, 0]).all()
    print("\nAUROC (mcd_mi, entropy of the combination) by mode:", got)
    assert 0.3 < got[0][1] < 0.7                          # chance: the entropy of the reference's combination does not separate them
    ent = mr.entropy_of_logits(mr.combine(x, 1)[0].astype(np.float32))
    assert np.abs(ent - math.log(8)).max() < 2e-3


def test_every_gpu_case_decides_its_prediction():
    """The cases of tests/test_gpu_mcd.py: in every row the two largest combined logits are further apart than their bounds, so
    pred, var_pred and disagreement are compared in every row; and the bounds are what their derivation says they are at K = 1000."""
    for shape in mr.SHAPES:
        for mode in (0, 1):
            b = mr.bounds(mr.logits_case(shape), mode)
            assert b["gap_ok"].all(), (shape, mode)
            assert b["z_mask"].all(), (shape, mode)
    b = mr.bounds(mr.logits_case((130, 1000, 4)), 1)
    assert 1e-6 < b["z"].max() < 1e-5 and b["total"].max() < 1e-4 and b["var"].max() < 1e-5


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL, 16-byte aligned pointer: the checks return before it is used
ODD = C.c_void_p(4104)     # 8-byte aligned only
NUL = C.c_void_p(0)
ARG, SHAPE = -1, -2
BAD_BK = [(0, 5), (-1, 5), (2, 0), (2, -3)]


def test_symbols_are_bound():
    from uncertainty_vit_amd import native
    for name in ("uvit_op_mcd_state_bytes", "uvit_op_mcd_accumulate", "uvit_op_mcd_finalize", "uvit_engine_forward_tail"):
        assert name in native.SYMBOLS and getattr(native.lib(), name).argtypes is not None


def test_state_bytes(L):
    for B, K in BAD_BK:
        assert L.uvit_op_mcd_state_bytes(B, K) == SHAPE, (B, K)
    for K in (1, 2, 10, 65, 1000):
        row = L.uvit_op_mcd_state_bytes(1, K)
        assert row % 16 == 0 and 8 * (3 * K + 1) + 4 * (K + 1) <= row < 8 * (3 * K + 1) + 4 * (K + 1) + 16
        assert L.uvit_op_mcd_state_bytes(130, K) == 130 * row


def test_accumulate_rejects_bad_arguments(L):
    call = lambda z, st, first=1, shape=(2, 5): L.uvit_op_mcd_accumulate(z, st, first, *shape, NUL)      # noqa: E731
    assert call(NUL, P1) == ARG and call(P1, NUL) == ARG and call(P1, ODD) == ARG
    for first in (-1, 2):
        assert call(P1, P1, first=first) == ARG
    for shape in BAD_BK:
        assert call(P1, P1, shape=shape) == SHAPE, shape


def test_finalize_rejects_bad_arguments(L):
    call = lambda st, z, T=3, mode=0, shape=(2, 5), unc=P1: L.uvit_op_mcd_finalize(st, T, mode, z, unc, *shape, NUL)      # noqa: E731
    assert call(NUL, P1) == ARG and call(P1, NUL) == ARG and call(ODD, P1) == ARG
    for mode in (-1, 2):
        assert call(P1, P1, mode=mode) == ARG, mode
    for T in (0, -1):
        assert call(P1, P1, T=T) == SHAPE, T
    for shape in BAD_BK:
        assert call(P1, P1, shape=shape) == SHAPE, shape


def test_forward_tail_rejects_a_null_engine(L):
    assert L.uvit_engine_forward_tail(NUL, 0, 1, 0, 1, 0, 0, NUL) == ARG


# ---- the module ----
def tiny_encoder(attn_drop_rate=0.1, depth=3, two_stream=False):
    from uncertainty_vit_amd.modeling_cyclical import DistVisionTransformerForCyclicalTraining, VisionTransformerForCyclicalTraining
    cls = DistVisionTransformerForCyclicalTraining if two_stream else VisionTransformerForCyclicalTraining
    return cls(img_size=48, patch_size=16, embed_dim=128, depth=depth, num_heads=2, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
               init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False, attn_drop_rate=attn_drop_rate)


def test_probe_is_a_linear_probe_with_its_keys():
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.mcd_probe import UNC_KEYS, MCDropoutProbe
    from uncertainty_vit_amd.native import UvitError
    torch.manual_seed(3)
    probe = MCDropoutProbe(tiny_encoder().eval(), 10, passes=4, layers=2, combine="probs", seed=2 ** 32 + 5)
    torch.manual_seed(3)
    lin = LinearProbe(tiny_encoder().eval(), 10)
    assert isinstance(probe, LinearProbe) and list(probe.state_dict()) == ["head.weight", "head.bias"]
    assert torch.equal(probe.head.weight.data, lin.head.weight.data) and probe._arena.numel() == lin._arena.numel()
    assert (probe.passes, probe.layers, probe.first_layer, probe.combine, probe.seed) == (4, 2, 1, "probs", 5)
    probe.load_state_dict(lin.state_dict())                                  # a linear probe-N.pth resumes
    probe.load_optimizer_state_dict(lin.optimizer_state_dict())
    dflt = MCDropoutProbe(tiny_encoder().eval(), 10)
    assert (dflt.passes, dflt.layers, dflt.first_layer, dflt.combine, dflt.seed) == (8, 0, 0, "logits", 0)
    assert MCDropoutProbe(tiny_encoder().eval(), 10, layers=3).first_layer == 0
    assert UNC_KEYS == mr.UNC_KEYS and probe.DETECT_COLUMNS == LinearProbe.DETECT_COLUMNS + UNC_KEYS and len(probe.DETECT_COLUMNS) == 8
    # with a density, a bank and a ViM fit: 8 + 2 + 1 + 2 = 13 of the store's 16 columns
    from uncertainty_vit_amd.linear_probe import KNN_COLUMNS, MAHA_COLUMNS, VIM_COLUMNS
    from uncertainty_vit_amd.probe_detect import DETECT_MAX_S
    assert len(probe.DETECT_COLUMNS) + len(MAHA_COLUMNS) + len(KNN_COLUMNS) + len(VIM_COLUMNS) <= 14 <= DETECT_MAX_S
    x = torch.zeros(2, 3, 48, 48)                                             # no CPU fallback
    for call in (probe.logits, probe.predictive):
        with pytest.raises(UvitError):
            call(x)
    with pytest.raises(UvitError):
        probe.encoder.forward_tail(0, 0, 0)                                   # no forward to continue


def test_probe_rejects_what_is_not_built():
    from uncertainty_vit_amd.mcd_probe import MCDropoutProbe
    for kw in (dict(passes=0), dict(passes=-2), dict(layers=4), dict(layers=-1), dict(combine="mean"), dict(num_classes=0)):
        with pytest.raises(ValueError):
            MCDropoutProbe(tiny_encoder().eval(), **{"num_classes": 10, **kw})
    with pytest.raises(ValueError, match="attn_drop_rate"):
        MCDropoutProbe(tiny_encoder(attn_drop_rate=0.0).eval(), 10)
    with pytest.raises((NotImplementedError, ValueError)):
        MCDropoutProbe(tiny_encoder(two_stream=True).eval(), 10)
    with pytest.raises(ValueError):
        MCDropoutProbe(tiny_encoder(), 10)                                    # the encoder must be in eval mode
    with pytest.raises(NotImplementedError):
        tiny_encoder(two_stream=True).forward_tail(0, 0, 0)


# ---- the command line ----
def test_cli_flags_are_absent_unless_given(monkeypatch):
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()                                  # the parsed defaults without the flags equal today's
    got = vars(rlp.get_args([]))
    assert not [k for k in got if k.startswith("mc_") or k == "attn_drop_rate"]
    assert rlp.check_mcd_flags(rlp.get_args([])) == 0 and rlp.check_mcd_flags(rlp.get_args(["--mc_dropout_forwards", "0"])) == 0
    a = rlp.get_args(["--mc_dropout_forwards", "8", "--attn_drop_rate", "0.1"])
    assert rlp.check_mcd_flags(a) == 8 and not any(hasattr(a, k) for k in rlp.MCD_FLAGS)
    a = rlp.get_args(["--mc_dropout_forwards", "4", "--attn_drop_rate", "0.05", "--mc_dropout_layers", "3", "--mc_combine", "probs", "--mc_seed", "7"])
    assert (a.mc_dropout_forwards, a.attn_drop_rate, a.mc_dropout_layers, a.mc_combine, a.mc_seed) == (4, 0.05, 3, "probs", 7)
    with pytest.raises(SystemExit):
        rlp.get_args(["--mc_dropout_forwards", "4", "--mc_combine", "median"])
    stats = {"mcd_total": 1.0, "mcd_aleatoric": 0.75, "mcd_mi": 0.25, "mcd_var": 0.125, "mcd_disagreement": 0.5, "det_acc1": 62.5,
             "mcd_passes": 8, "mcd_layers": 3}
    assert rlp.mcd_lines(stats, 12, 0.1) == ["* MC-dropout passes 8 layers 3 of 12 rate 0.1 entropy 1.00000 expected 0.75000 MI 0.25000 "
                                             "variance 0.125000 disagreement 0.50000", "* Deterministic Acc@1 62.500"]
    assert rlp.mcd_log_entries(stats) == {"test_mcd_total": 1.0, "test_mcd_aleatoric": 0.75, "test_mcd_mi": 0.25, "test_mcd_var": 0.125,
                                          "test_mcd_disagreement": 0.5, "test_mcd_det_acc1": 62.5, "test_mcd_passes": 8}
    # the errors come before anything is loaded
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    base = ["--nb_classes", "10", "--finetune", "none.pth"]
    on = ["--mc_dropout_forwards", "4", "--attn_drop_rate", "0.1"]
    for flags in (["--mc_dropout_layers", "3"], ["--mc_combine", "probs"], ["--mc_seed", "1"], ["--attn_drop_rate", "0.1"],
                  ["--attn_drop_rate", "0.1", "--mc_dropout_forwards", "0"]):
        with pytest.raises(ValueError, match="--mc_dropout_forwards"):
            rlp.main(rlp.get_args(base + flags))
    for other in ("--gp_layer", "--het_layer", "--ensembles", "--laplace"):
        with pytest.raises(ValueError, match="samples the linear head"):
            rlp.main(rlp.get_args(base + on + [other]))
    for flags in (["--mc_dropout_forwards", "4"], ["--mc_dropout_forwards", "4", "--attn_drop_rate", "0"]):
        with pytest.raises(ValueError, match="--attn_drop_rate"):
            rlp.main(rlp.get_args(base + flags))
    with pytest.raises(ValueError, match=">= 0"):
        rlp.main(rlp.get_args(base + ["--mc_dropout_forwards", "-1"]))
    # what it works with passes the flag checks and stops at the checkpoint that does not exist
    for flags in (["--calibration"], ["--eval", "--detection"], ["--eval", "--ts_temperature", "1.5"], ["--eval", "--vim_state", "v.pth"],
                  ["--eval", "--maha_state", "m.pth", "--knn_state", "k.pth"], ["--eval", "--perturbation_path", "p"]):
        with pytest.raises(FileNotFoundError):
            rlp.main(rlp.get_args(base + on + flags))
