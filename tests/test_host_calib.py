"""CPU: the calibration metrics' host-side pieces -- the float64 restatement (tests/calib_ref.py) against what the reference classes
computed (tests/golden/calib.npz, written by tools/gen_golden_calib.py), known answers worked out by hand, the argument checks of
every uvit_op_calib_* entry point (they return before anything touches a device), and the command line's new flag."""
import ctypes as C

import numpy as np
import pytest

import calib_ref as cr


@pytest.fixture(scope="module")
def fx(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, "calib.npz"))


def cases(fx):
    return [str(n) for n in fx["names"]]


def bins_of(fx):
    return int(fx["ece_bins"]), int(fx["tace_bins"]), float(fx["tace_threshold"])


# ---- the restatement against the fixture ----
def test_fixture_holds_the_cases(fx):
    """(B, K) of the stored cases, the bin_n = 0 case (B < 30 bins) and the 1/64 grid among them; the file is under 100 KB."""
    shapes = {n: fx["probs/" + n].shape for n in cases(fx)}
    assert [shapes[n] for n in cases(fx)] == [(48, 10), (37, 10), (29, 10), (30, 10), (64, 100), (40, 10)]
    grid = fx["probs/" + cases(fx)[-1]]
    assert np.array_equal(grid * 64, np.round(grid * 64)) and int((grid < 0.01).sum()) > 10
    for n in cases(fx):
        p = fx["probs/" + n]
        top = np.sort(p, axis=1)[:, -2:]
        assert bool((top[:, 1] > top[:, 0]).all()), n            # no tied row maximum
        assert fx["probs/" + n].dtype == np.float32 and fx["labels/" + n].dtype == np.int64


def test_ece_and_tace_against_reference_fixture(fx):
    """calib_ref's ECE and TACE, in the reference's reading of the bin accuracy (positional_acc), within 1e-12 of what the unmodified
    reference classes returned on the same float64 inputs: same memberships, only the order of the sums differs."""
    eb, tb, thr = bins_of(fx)
    worst = []
    for n in cases(fx):
        p, y = fx["probs/" + n], fx["labels/" + n]
        e = cr.confidence(p, y, eb, positional_acc=True)["ECE"] - float(fx["ece/" + n])
        t = cr.tace(p, y, thr, tb, positional_acc=True)[0] - float(fx["tace/" + n])
        print(f"\n{n}: calib_ref - reference: ECE {e:+.3e}, TACE {t:+.3e}")
        worst.append((n, e, t))
    assert all(abs(e) <= 1e-12 and abs(t) <= 1e-12 for _, e, t in worst), worst


def test_bin_tables_against_reference_fixture(fx):
    """The reference's own per-bin arrays (its ECELoss object: prop, acc, conf) within 1e-12 of calib_ref's table with
    positional_acc.  With the mean over the rows of the bin instead, proportions and confidences still agree and the accuracies do
    not: the reference's `accuracies[in_bin]` indexes rows 0 and 1 by position (calib_ref._bin_acc), and its ECE / TACE are far from
    the textbook ones (fixture: ECE by 0.05 to 0.30, TACE by 0.003 to 0.09)."""
    eb, tb, thr = bins_of(fx)
    differs = 0
    for n in cases(fx):
        p, y = fx["probs/" + n], fx["labels/" + n]
        ref = fx["ece_bins/" + n]                                   # (n_bins, 3): prop, acc, conf of the reference's ECELoss
        np.testing.assert_allclose(cr.confidence(p, y, eb, positional_acc=True)["table"], ref, rtol=0, atol=1e-12)
        own = cr.confidence(p, y, eb)
        np.testing.assert_allclose(own["table"][:, [0, 2]], ref[:, [0, 2]], rtol=0, atol=1e-12)
        differs += int(np.abs(own["table"][:, 1] - ref[:, 1]).max() > 1e-3 and abs(own["ECE"] - float(fx["ece/" + n])) > 1e-2)
    assert differs == len(cases(fx))


def test_positional_bin_accuracy_by_hand():
    """Four rows, 2 ECE bins, conf = (0.75, 0.75, 0.75, 1.0): all in bin (0.5, 1], mean 0.8125; three rows are right.  In the
    reference's reading rows 0 and 1 decide every bin's accuracy: a[0] = 1 (row 0 right), a[1] = 0 (row 1 wrong), and a bin with
    count c of B = 4 has acc (c a[1] + (4 - c) a[0]) / 4, here a[1] = 0."""
    p = np.array([[0.75, 0.25], [0.75, 0.25], [0.25, 0.75], [1.0, 0.0]], dtype=np.float32)
    y = np.array([0, 1, 1, 0])                                      # correct = 1, 0, 1, 1; all four conf in (0.5, 1]
    pos, own = cr.confidence(p, y, 2, positional_acc=True), cr.confidence(p, y, 2)
    assert own["table"][1].tolist() == [1.0, 0.75, 0.8125] and own["ECE"] == 0.0625
    assert pos["table"][1].tolist() == [1.0, 0.0, 0.8125] and pos["ECE"] == 0.8125           # count 4: (4 a[1] + 0 a[0]) / 4 = a[1] = 0
    # one row: the reference cannot index row 1; a[1] is a[0] and both readings agree
    one = np.array([[0.75, 0.25]], dtype=np.float32)
    assert cr.confidence(one, np.array([0]), 2, positional_acc=True)["ECE"] == cr.confidence(one, np.array([0]), 2)["ECE"] == 0.25


def test_auroc_against_scikit_learn_fixture(fx):
    """Per-class one-vs-rest AUROC within 1e-12 of roc_auc_score(y == c, p[:, c]) (stored), for exactly the classes that have a
    positive and a negative row; sum and count follow."""
    for n in cases(fx):
        p, y = fx["probs/" + n], fx["labels/" + n]
        a, ref = cr.auroc(p, y), fx["auroc/" + n]
        present = set(np.nonzero(np.isfinite(ref))[0].tolist())
        assert set(a["per_class"]) == present and a["count"] == len(present), n
        err = max(abs(a["per_class"][c] - ref[c]) for c in present)
        print(f"\n{n}: {len(present)} classes, worst AUROC error {err:.2e}")
        assert err <= 1e-12
        assert a["sum"] == pytest.approx(float(np.nansum(ref)), abs=1e-11)


def test_nll_against_reference_fixture(fx):
    """NLL within 1e-5 relative of the reference's NLL(logits, y), an fp32 softmax-then-log chain whose round-off is about 1e-6.
    The restatement takes the stored fp32 probabilities (torch.softmax of the stored logits)."""
    for n in cases(fx):
        ref = float(fx["nll/" + n])
        if np.isnan(ref):
            assert "logits/" + n not in fx.files                    # the grid case has no logits
            continue
        got = cr.confidence(fx["probs/" + n], fx["labels/" + n])["NLL"]
        print(f"\n{n}: NLL {got:.9f}, reference {ref:.9f}, relative error {abs(got - ref) / ref:.2e}")
        assert abs(got - ref) <= 1e-5 * ref


def test_stored_probabilities_are_the_softmax_of_the_stored_logits(fx):
    for n in cases(fx):
        if "logits/" + n in fx.files:
            np.testing.assert_allclose(fx["probs/" + n], cr.softmax(fx["logits/" + n]), rtol=1e-6, atol=1e-9)


def test_stored_probabilities_keep_clear_of_every_bound(fx):
    """What the GPU end-to-end check relies on: no stored probability of a case with logits within 1e-6 relative of an ECE bin
    edge, of the TACE threshold, or of another element of its column that serves as an adaptive bound."""
    eb, tb, thr = bins_of(fx)
    m = float(fx["margin"])
    for n in cases(fx):
        if "logits/" + n not in fx.files:
            continue
        p = fx["probs/" + n].astype(np.float64)
        conf = p.max(1)
        for b in np.linspace(0, 1, eb + 1)[1:]:
            assert not (np.abs(conf - b) <= m * b).any(), (n, b)
        assert not (np.abs(p - thr) <= m * thr).any(), n
        v = np.where(p < thr, 0.0, p)
        for c in range(p.shape[1]):
            s = np.sort(v[:, c])
            for i in range(tb):
                b = s[i * (p.shape[0] // tb)]
                assert b == 0.0 or int((np.abs(s - b) <= m * b).sum()) == 1, (n, c, i)


# ---- known answers by hand ----
def test_one_hot_all_right():
    """One-hot rows with every label right: every conf is 1 (last bin), acc 1, ECE 0; NLL = -log(1 - eps) (Categorical's clamp)."""
    y = np.array([0, 3, 1, 3, 2])
    p = np.eye(4, dtype=np.float32)[y]
    out = cr.confidence(p, y, 15)
    assert out["ECE"] == 0.0 and cr.confidence(p, y, 15, positional_acc=True)["ECE"] == 0.0
    assert out["NLL"] == pytest.approx(-np.log(1.0 - 2.0 ** -23), rel=1e-12) and out["NLL"] > 0.0
    assert out["table"][-1].tolist() == [1.0, 1.0, 1.0] and float(np.abs(out["table"][:-1]).max()) == 0.0
    # all wrong: the clamp from below, -log(eps), and ECE 1
    wrong = cr.confidence(p, (y + 1) % 4, 15)
    assert wrong["ECE"] == 1.0 and wrong["NLL"] == pytest.approx(23 * np.log(2.0), rel=1e-12)


def test_bin_edges():
    """n_bins = 16: the edges k / 16 are exact.  conf == 0.5 lands in bin 7 = (0.4375, 0.5], conf == 1.0 in the last bin, a conf of
    exactly 0 in none."""
    p = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5625, 0.4375, 0.0]], dtype=np.float32)
    y = np.array([0, 1, 0, 1])
    out = cr.confidence(p, y, 16)
    assert out["table"][:, 0].tolist() == [0, 0, 0, 0, 0, 0, 0, 0.25, 0.25, 0, 0, 0, 0, 0, 0, 0.25]
    assert out["table"][7].tolist() == [0.25, 1.0, 0.5] and out["table"][15].tolist() == [0.25, 0.0, 1.0]
    assert out["table"][8].tolist() == [0.25, 0.0, 0.5625]
    assert out["ECE"] == pytest.approx(0.25 * 0.5 + 0.25 * 1.0 + 0.25 * 0.5625, abs=1e-15)
    assert out["pred"].tolist() == [0, 0, 0, 0] and out["correct"].tolist() == [1, 0, 1, 0]      # row 2: a tie, the lowest index wins


def test_tace_by_hand():
    """B = 4, n_bins = 2, threshold 0.3, one class column v = (0.5, 0.25 -> 0, 0.75, 0.5), y == c on rows 0 and 2.  Sorted:
    0, 0.5, 0.5, 0.75; bin_n = 2: lo = (0, 0.5), up = (0.5, 1).  Bin 0 = {0.5, 0.5}: prop 0.5, conf 0.5, acc 0.5, score 0.  Bin 1 =
    {0.75}: prop 0.25, conf 0.75, acc 1, score 0.25.  The zero falls in no bin.  Class value 0.0625."""
    col = np.array([0.5, 0.25, 0.75, 0.5], dtype=np.float32)
    p = np.stack([col, 1.0 - col], axis=1)
    y = np.array([0, 1, 0, 1])
    t, per = cr.tace(p, y, 0.3, 2)
    assert per[0] == 0.0625
    # column 1 = (0.5, 0.75, 0.25 -> 0, 0.5): the same values in another order, y == 1 on rows 1 and 3: bin 0 acc 0.5, bin 1 acc 1
    assert per[1] == 0.0625 and t == 0.0625
    # B < n_bins: bin_n = 0, every lower bound is the column minimum and only the last bin (min, 1] holds anything
    t5, per5 = cr.tace(p, y, 0.3, 5)
    assert per5[0] == pytest.approx(0.75 * abs((0.5 + 0.75 + 0.5) / 3 - 2 / 3), abs=1e-15)


def test_auroc_by_hand():
    """B = 1: no class has a negative row, count 0.  All labels equal: count 0.  Two classes, a tie: AUC = (1 + 0.5) / 2."""
    one = cr.auroc(np.array([[0.25, 0.75]], dtype=np.float32), np.array([1]))
    assert one["count"] == 0 and one["sum"] == 0.0 and one["u2"].tolist() == [0]
    same = cr.auroc(np.full((3, 2), 0.5, dtype=np.float32), np.array([1, 1, 1]))
    assert same["count"] == 0 and same["n_pos"].tolist() == [3, 3, 3] and same["first"].tolist() == [1, 0, 0]
    p = np.array([[0.75, 0.25], [0.5, 0.5], [0.5, 0.5]], dtype=np.float32)
    a = cr.auroc(p, np.array([0, 0, 1]))
    assert a["per_class"][0] == 0.75 and a["per_class"][1] == 0.75 and a["count"] == 2      # class 0: (1 + 0.5) / 2; class 1: (1 + 0.5) / 2
    assert a["u2"].tolist() == [2, 1, 3] and cr.batch_metrics(p, np.array([0, 0, 1]))["AUROC"] == 0.75


def test_label_out_of_range_gives_nan():
    p = np.full((3, 4), 0.25, dtype=np.float32)
    for bad in (-1, 4):
        m = cr.batch_metrics(p, np.array([0, bad, 1]))
        assert all(np.isnan(m[k]) for k in ("ECE", "TACE", "NLL", "auroc_sum")), (bad, m)


def test_weighted_means():
    """The meters: batch-size-weighted; a batch without an AUROC leaves only that mean."""
    per = [{"ECE": 0.5, "TACE": 0.25, "NLL": 1.0, "auroc_sum": 1.5, "auroc_count": 2},
           {"ECE": 0.25, "TACE": 0.5, "NLL": 2.0, "auroc_sum": 0.0, "auroc_count": 0}]
    w = cr.weighted(per, [3, 1], 10)
    assert w["ECE"] == 0.4375 and w["TACE"] == 0.3125 and w["NLL"] == 1.25 and w["AUROC"] == 0.75
    assert w["AUROC_zero_absent"] == pytest.approx(0.15 * 3 / 4)


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE = -1, -2
BAD_BK = [(0, 10), (1025, 3), (-1, 10), (4, 0), (4, -2)]


def test_softmax_rejects_bad_arguments(L):
    for B, K in BAD_BK:
        assert L.uvit_op_calib_softmax(P1, P1, B, K, NUL) == SHAPE, (B, K)
    assert L.uvit_op_calib_softmax(NUL, P1, 4, 10, NUL) == ARG and L.uvit_op_calib_softmax(P1, NUL, 4, 10, NUL) == ARG


def test_confidence_rejects_bad_arguments(L):
    for B, K in BAD_BK:
        assert L.uvit_op_calib_confidence(*[P1] * 3, 15, 1, *[P1] * 5, B, K, NUL) == SHAPE, (B, K)
    for nb in (0, 65, -1):
        assert L.uvit_op_calib_confidence(*[P1] * 3, nb, 0, *[P1] * 5, 4, 10, NUL) == SHAPE, nb
    for i in range(8):
        a = [P1] * 8
        a[i] = NUL
        assert L.uvit_op_calib_confidence(*a[:3], 15, 1, *a[3:], 4, 10, NUL) == ARG, i
    for mode in (2, -1):
        assert L.uvit_op_calib_confidence(*[P1] * 3, 15, mode, *[P1] * 5, 4, 10, NUL) == ARG, mode


def test_tace_rejects_bad_arguments(L):
    d = C.c_double(0.01)
    for B, K in BAD_BK:
        assert L.uvit_op_calib_tace(P1, P1, d, 30, 1, P1, P1, B, K, NUL) == SHAPE, (B, K)
    for nb in (0, 65, -1):
        assert L.uvit_op_calib_tace(P1, P1, d, nb, 0, P1, P1, 4, 10, NUL) == SHAPE, nb
    for i in range(4):
        a = [P1] * 4
        a[i] = NUL
        assert L.uvit_op_calib_tace(a[0], a[1], d, 30, 1, a[2], a[3], 4, 10, NUL) == ARG, i
    for mode in (2, -1):
        assert L.uvit_op_calib_tace(P1, P1, d, 30, mode, P1, P1, 4, 10, NUL) == ARG, mode


def test_auroc_rejects_bad_arguments(L):
    for B, K in BAD_BK:
        assert L.uvit_op_calib_auroc(P1, P1, P1, P1, B, K, NUL) == SHAPE, (B, K)
    for i in range(4):
        a = [P1] * 4
        a[i] = NUL
        assert L.uvit_op_calib_auroc(*a, 4, 10, NUL) == ARG, i


# ---- the module and the command line ----
def test_calibration_needs_a_gpu():
    """No CPU fallback: calibration_batch refuses host tensors."""
    import torch
    from test_host_probe import tiny_encoder
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    probe = LinearProbe(tiny_encoder().eval(), 10)
    with pytest.raises(UvitError):
        probe.calibration_batch(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64))


def test_cli_flag_is_absent_unless_given():
    """--calibration is off by default and leaves the parsed arguments (the first line run_linear_probe prints) as they were."""
    import run_linear_probe as rlp
    assert "calibration" not in vars(rlp.get_args([]))
    assert rlp.get_args(["--calibration"]).calibration is True
    line = rlp.calibration_line({"ECE": 0.25, "TACE": 0.125, "NLL": 1.5, "AUROC": 0.75, "acc1": 1.0})
    assert line == "* ECE 0.25000 TACE 0.12500 NLL 1.50000 AUROC 0.75000"
