"""CPU: the detection metrics' host-side pieces -- the float64 restatement (tests/detect_ref.py) against what scikit-learn returned
(tests/golden/detect.npz, written by tools/gen_golden_detect.py), a brute-force AURC, answers worked out by hand, the argument
checks of every uvit_op_detect_* entry point (they return before anything touches a device), and the command line's new flags."""
import ctypes as C
import os

import numpy as np
import pytest

import detect_ref as dr


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "detect.npz"))


def cases(fx):
    return [str(n) for n in fx["names"]]


# ---- the restatement against the fixture ----
def test_fixture_holds_the_cases(fx, golden_dir):
    """At most 300 samples per case, heavy ties, both signs of zero and P = 1 among them; the file is tens of KB at the most."""
    assert os.path.getsize(os.path.join(golden_dir, "detect.npz")) < 64 * 1024
    sizes = {n: fx["scores/" + n].shape[0] for n in cases(fx)}
    assert max(sizes.values()) <= 300 and len(sizes) >= 6
    assert any(int(fx["flags/" + n].sum()) == 1 for n in cases(fx))
    assert any(len(np.unique(fx["scores/" + n])) <= 7 and sizes[n] >= 200 for n in cases(fx))
    z = fx["scores/ties3_signed_zero_41"]
    assert bool((np.signbit(z) & (z == 0)).any()) and bool((~np.signbit(z) & (z == 0)).any())
    for n in cases(fx):
        assert fx["scores/" + n].dtype == np.float32 and fx["flags/" + n].dtype == np.uint8


def test_restatement_against_scikit_learn(fx):
    """AUROC, average precision and FPR95 within 1e-12 of roc_auc_score, average_precision_score and roc_curve."""
    worst = []
    for n in cases(fx):
        m = dr.metrics(fx["scores/" + n], fx["flags/" + n])
        d = [m["AUROC"] - float(fx["auroc/" + n]), m["AUPR"] - float(fx["ap/" + n]), m["FPR95"] - float(fx["fpr95/" + n])]
        print(f"\n{n}: detect_ref - scikit-learn: AUROC {d[0]:+.3e}, AUPR {d[1]:+.3e}, FPR95 {d[2]:+.3e}")
        worst.append((n, d))
    assert all(abs(v) <= 1e-12 for _, d in worst for v in d), worst


def test_aurc_against_brute_force(fx):
    for n in cases(fx):
        s, f = fx["scores/" + n], fx["flags/" + n]
        a, b = dr.metrics(s, f)["AURC"], dr.aurc_brute(s, f)
        print(f"\n{n}: AURC {a:.12f}, brute force {b:.12f}")
        assert abs(a - b) <= 1e-12


# ---- answers worked out by hand ----
def test_all_scores_equal():
    """One tie group: the ROC curve is the diagonal, the precision is the base rate, FPR95 is 1."""
    f = np.array([1, 0, 0, 1, 0, 0, 0, 0], dtype=np.uint8)
    m = dr.metrics(np.full(8, 0.25, dtype=np.float32), f)
    assert m["AUROC"] == 0.5 and m["AUPR"] == 0.25 and m["FPR95"] == 1.0 and (m["n"], m["P"], m["nan"]) == (8, 2, 0)
    assert m["order"].tolist() == list(range(8))                  # ties go to the lower index
    # ascending (score, index) order is the sample order: wrong counts 1 1 1 2 2 2 2 2 over coverages 1 .. 8
    assert abs(m["AURC"] - (1 + 1 / 2 + 1 / 3 + 2 / 4 + 2 / 5 + 2 / 6 + 2 / 7 + 2 / 8) / 8) <= 1e-15


def test_perfect_separation():
    """Every positive above every negative: AUROC 1, AUPR 1, FPR95 0, AURC the closed form; reversed: AUROC 0, FPR95 1."""
    n, P = 40, 7
    s = np.arange(n, dtype=np.float32) / 8
    f = (np.arange(n) >= n - P).astype(np.uint8)
    m = dr.metrics(s, f)
    assert m["AUROC"] == 1.0 and m["AUPR"] == 1.0 and m["FPR95"] == 0.0
    assert abs(m["AURC"] - dr.aurc_perfect(n, P)) <= 1e-15
    r = dr.metrics(-s, f)
    assert r["AUROC"] == 0.0 and r["FPR95"] == 1.0


def test_small_case_by_hand():
    """scores 1 2 2 3, positives at the 3 and at one of the 2s.  Groups from the top: {3}: TP 1 FP 0; {2, 2}: TP 2 FP 1; {1}: TP 2 FP 2.
    AUROC = (0 + 1 * 3 + 1 * 4) / (2 * 2 * 2) = 7 / 8; AUPR = 1 / 2 * 1 + 1 / 2 * 2 / 3 = 5 / 6; ceil(0.95 * 2) = 2: FPR95 = 1 / 2;
    ascending order by (score, index) is 0 1 2 3 with flags 0 0 1 1: AURC = (0 + 0 + 1 / 3 + 2 / 4) / 4."""
    m = dr.metrics(np.array([1, 2, 2, 3], dtype=np.float32), np.array([0, 0, 1, 1], dtype=np.uint8))
    assert m["AUROC"] == 7 / 8 and abs(m["AUPR"] - 5 / 6) <= 1e-15 and m["FPR95"] == 0.5 and abs(m["AURC"] - (1 / 3 + 1 / 2) / 4) <= 1e-15


def test_nan_scores_degenerate_sets_and_bad_flags():
    """NaN scores are counted, left out and listed last by index; -0 ties with +0; P = 0, Nn = 0 and n = 0 give the NaNs the header
    states; a flag 2 makes all four NaN and leaves the counts."""
    s = np.array([np.nan, 0.5, -0.0, 0.0, np.nan, 0.25], dtype=np.float32)
    f = np.array([1, 1, 0, 1, 0, 0], dtype=np.uint8)
    m = dr.metrics(s, f)
    assert m["order"].tolist() == [2, 3, 5, 1, 0, 4] and (m["n"], m["P"], m["nan"]) == (4, 2, 2)
    # (positive, negative) pairs: (.5, .25) and (.5, -0) ranked right, (0, .25) wrong, (0, -0) tied: (1 + 1 + 0 + 1 / 2) / 4
    assert m["AUROC"] == 2.5 / 4
    none = dr.metrics(s, np.zeros(6, dtype=np.uint8))
    assert np.isnan(none["AUROC"]) and np.isnan(none["AUPR"]) and np.isnan(none["FPR95"]) and none["AURC"] == 0.0
    every = dr.metrics(s, np.ones(6, dtype=np.uint8))
    assert np.isnan(every["AUROC"]) and np.isnan(every["FPR95"]) and every["AUPR"] == 1.0 and every["AURC"] == 1.0
    empty = dr.metrics(np.full(3, np.nan, dtype=np.float32), np.ones(3, dtype=np.uint8))
    assert all(np.isnan(empty[k]) for k in ("AUROC", "AUPR", "FPR95", "AURC")) and (empty["n"], empty["P"], empty["nan"]) == (0, 0, 3)
    f2 = f.copy()
    f2[5] = 2
    bad = dr.metrics(s, f2)
    assert all(np.isnan(bad[k]) for k in ("AUROC", "AUPR", "FPR95", "AURC")) and (bad["n"], bad["P"]) == (4, 2)


def test_row_scores_by_hand():
    """Uniform logits: msp 1 - 1 / K, entropy log K, energy -(c + log K).  A one-hot row of huge logits: three finite values, entropy
    0.  Flags: the lowest index wins an argmax tie; a label outside [0, K) is flag 2."""
    z = np.full((2, 4), 3.0, dtype=np.float32)
    sc, bd, fl = dr.row_scores(z, [0, 1])
    assert np.allclose(sc[:, 0], [0.75, np.log(4.0), -(3.0 + np.log(4.0))], atol=1e-15) and fl.tolist() == [0, 1]
    assert bool((bd > 0).all()) and bool((bd < 1e-6).all())         # a few fp32 ulps of values of order 1
    big = np.array([[3e38, -3e38, 0.0], [0.0, 1e30, 1e30]], dtype=np.float32)
    sc, bd, fl = dr.row_scores(big, [0, 2])
    assert np.isfinite(sc).all() and sc[0, 0] == 0.0 and sc[1, 0] == 0.0 and abs(sc[1, 1] - np.log(2.0)) < 1e-15 and fl.tolist() == [0, 1]
    assert dr.row_scores(z, [-1, 4])[2].tolist() == [2, 2]


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL, 16-byte aligned pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE, WORKSPACE = -1, -2, -4
NAMES = ("uvit_op_detect_rows", "uvit_op_detect_column", "uvit_op_detect_ws_bytes", "uvit_op_detect_metrics")


def test_symbols_are_declared_and_exported():
    from uncertainty_vit_amd import native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uvit.h")).read()
    for name in NAMES:
        assert name in native.SYMBOLS and name + "(" in hdr and getattr(native.lib(), name).argtypes is not None
    assert native.lib().uvit_version() == 100


def test_ws_bytes(L):
    """Refuses N = 0, N > 2^20, S = 0 and S > 16; grows with N and S; holds at least the keys and the prefix counts."""
    for N, S in [(0, 1), (-1, 1), ((1 << 20) + 1, 1), (10, 0), (10, 17)]:
        assert L.uvit_op_detect_ws_bytes(N, S) == SHAPE, (N, S)
    assert L.uvit_op_detect_ws_bytes(1, 1) > 0
    a, b, c = L.uvit_op_detect_ws_bytes(4096, 1), L.uvit_op_detect_ws_bytes(4097, 1), L.uvit_op_detect_ws_bytes(4097, 3)
    assert 12 * 4096 <= a < b < c and b >= 12 * 8192 and c >= 3 * 12 * 8192
    assert L.uvit_op_detect_ws_bytes(1 << 20, 16) >= 16 * 12 * (1 << 20)


def test_metrics_rejects_bad_arguments(L):
    ws = L.uvit_op_detect_ws_bytes(100, 3)
    good = dict(scores=P1, ld=100, flags=P1, N=100, S=3, order=NUL, out=P1, ws=P1, ws_bytes=ws)

    def call(**kw):
        a = {**good, **kw}
        return L.uvit_op_detect_metrics(a["scores"], a["ld"], a["flags"], a["N"], a["S"], a["order"], a["out"], a["ws"], a["ws_bytes"], NUL)

    for kw in (dict(N=0), dict(N=-3), dict(N=(1 << 20) + 1, ld=1 << 21, ws_bytes=1 << 40), dict(S=0), dict(S=17, ws_bytes=1 << 40), dict(ld=99)):
        assert call(**kw) == SHAPE, kw
    for name in ("scores", "flags", "out", "ws"):
        assert call(**{name: NUL}) == ARG, name
    assert call(ws=C.c_void_p(4100)) == ARG                        # not 16-byte aligned
    assert call(ws_bytes=ws - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE


def test_rows_rejects_bad_arguments(L):
    call = L.uvit_op_detect_rows
    for B, K, ld, n0 in [(0, 10, 8, 0), (-1, 10, 8, 0), (4, 0, 8, 0), (4, 10, 3, 0), (4, 10, 8, 5), (4, 10, 8, -1), (4, 10, 0, 0)]:
        assert call(P1, P1, P1, ld, n0, P1, B, K, NUL) == SHAPE, (B, K, ld, n0)
    assert call(NUL, P1, P1, 8, 0, P1, 4, 10, NUL) == ARG and call(P1, P1, NUL, 8, 0, P1, 4, 10, NUL) == ARG
    assert call(P1, P1, P1, 8, 0, NUL, 4, 10, NUL) == ARG          # labels without a place for the flags


def test_column_rejects_bad_arguments(L):
    call = L.uvit_op_detect_column
    assert call(NUL, 0, 1, P1, 4, NUL) == ARG and call(P1, 0, 1, NUL, 4, NUL) == ARG and call(P1, 2, 1, P1, 4, NUL) == ARG
    assert call(P1, 1, 1, P1, 0, NUL) == SHAPE and call(P1, 1, 0, P1, 4, NUL) == SHAPE


# ---- the module and the command line ----
def test_detection_needs_a_gpu():
    """No CPU fallback: detection_batch refuses host tensors."""
    import torch
    from test_host_probe import tiny_encoder
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    probe = LinearProbe(tiny_encoder().eval(), 10)
    with pytest.raises(UvitError):
        probe.detection_batch(torch.zeros(3, 8), torch.zeros(8, dtype=torch.uint8))


def test_detection_columns_of_the_heads():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    assert LinearProbe.DETECT_COLUMNS == ("msp", "entropy", "energy")
    assert GPProbe.DETECT_COLUMNS == LinearProbe.DETECT_COLUMNS + ("gp_var",)
    assert HetProbe.DETECT_COLUMNS == LinearProbe.DETECT_COLUMNS + ("het_var",)
    assert EnsembleProbe.DETECT_COLUMNS == LinearProbe.DETECT_COLUMNS + ("ens_total", "ens_aleatoric", "ens_mi", "ens_var", "ens_disagreement")


def test_cli_flags_are_absent_unless_given():
    """Without the new flags the parsed arguments are today's; with them they parse; both belong to an evaluation."""
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()
    base = vars(rlp.get_args([]))
    assert "detection" not in base and "ood_data_path" not in base
    assert rlp.get_args(["--detection"]).detection is True and rlp.get_args(["--ood_data_path", "x"]).ood_data_path == "x"
    for flags in (["--detection"], ["--ood_data_path", "x"]):
        with pytest.raises(ValueError, match="--eval"):
            rlp.check_detection_flags(rlp.get_args(flags))
    assert rlp.check_detection_flags(rlp.get_args(["--eval", "--ood_data_path", "x"])) is True
    assert rlp.check_detection_flags(rlp.get_args(["--eval", "--detection"])) is True
    assert rlp.check_detection_flags(rlp.get_args(["--eval"])) is False


def test_cli_lines():
    import run_linear_probe as rlp
    det = {"columns": ["msp"], "misclassification": {"msp": {"AUROC": 0.75, "AUPR": 0.5, "FPR95": 0.25, "AURC": 0.125}},
           "ood": {"msp": {"AUROC": 0.5, "AUPR": 0.25, "FPR95": 1.0}}, "n": 8, "n_wrong": 2, "n_ood": 4}
    assert rlp.detection_lines(det) == ["* Detect misclassification msp AUROC 0.75000 AUPR 0.50000 FPR95 0.25000 AURC 0.12500",
                                        "* Detect OOD msp AUROC 0.50000 AUPR 0.25000 FPR95 1.00000"]
    assert rlp.detection_log_entries(det) == {"test_mis_msp_AUROC": 0.75, "test_mis_msp_AUPR": 0.5, "test_mis_msp_FPR95": 0.25, "test_mis_msp_AURC": 0.125,
                                              "test_ood_msp_AUROC": 0.5, "test_ood_msp_AUPR": 0.25, "test_ood_msp_FPR95": 1.0}
