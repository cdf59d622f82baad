"""CPU: conformal prediction sets' host-side pieces -- the float64 restatement (tests/cp_ref.py) against the O(K^2) definition and
the identities of split conformal prediction, the condition that keeps the GPU comparison from being vacuous, the argument checks of
every uvit_op_cp_* entry point (they return before anything touches a device), the module's members that need no GPU, and the command
line's new flags."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cp_ref as cr


# ---- the restatement ----
@pytest.mark.parametrize("kind", ["lac", "aps", "raps"])
def test_restatement_against_the_definition(kind):
    """Every class of every row: the sorted cumulative sum equals the sum over {i : p_i > p_j or (p_i == p_j and i < j)}."""
    z, _, u = cr.make_inputs(7, 23, 3.0)
    z[2, 5] = z[2, 11] = z[2, 20]                         # a three-way tie inside a row
    lam, kreg = cr.params(kind)
    for uu in (None, u):
        s = cr.all_scores(z, kind, uu, lam, kreg)
        for r in range(7):
            want = cr.brute_scores(z[r], kind, 1.0 if uu is None else float(uu[r]), lam, kreg)
            assert np.abs(s[r] - want).max() <= 1e-14, (kind, r)
    assert (np.diff(np.sort(cr.ranks(z), axis=1), axis=1) == 1).all()                  # a permutation of 1 .. K in every row


def test_raps_at_lambda_zero_is_aps():
    z, y, u = cr.make_inputs(65, 100, 1.0)
    assert np.array_equal(cr.all_scores(z, "raps", u, 0.0, 5), cr.all_scores(z, "aps", u))
    assert (cr.all_scores(z, "raps", u, 0.01, 5) >= cr.all_scores(z, "aps", u)).all()


def test_scores_grow_with_the_rank_and_sets_grow_as_alpha_shrinks():
    z, y, u = cr.make_inputs(257, 10, 1.0)
    for kind in ("lac", "aps", "raps"):
        s = cr.all_scores(z, kind, u, *cr.params(kind))
        by_rank = np.take_along_axis(s, np.argsort(cr.ranks(z), axis=1), axis=1)
        assert (np.diff(by_rank, axis=1) >= 0).all()                                   # a set is always "the top m classes"
        sy = cr.label_scores(z, y, kind, scores=s)
        sizes = [cr.set_sizes(s, cr.quantile(sy, a)["qhat"]) for a in (0.5, 0.3, 0.1, 0.01)]
        for small, large in zip(sizes, sizes[1:]):
            assert (small <= large).all()


def test_a_tie_inside_a_row_goes_to_the_smaller_index():
    z = np.zeros((1, 6), dtype=np.float32)
    assert cr.ranks(z).tolist() == [[1, 2, 3, 4, 5, 6]]
    s = cr.all_scores(z, "aps")
    assert np.allclose(s[0], np.arange(1, 7) / 6.0, atol=1e-15)
    assert cr.set_sizes(s, 0.5 + 1e-12).tolist() == [3]                               # classes 0, 1, 2
    z[0, 4] = -0.0
    assert cr.ranks(z).tolist() == [[1, 2, 3, 4, 5, 6]]                               # +0 == -0
    z[0, 3] = 1.0
    assert cr.ranks(z).tolist() == [[2, 3, 4, 1, 5, 6]]


@pytest.mark.parametrize("kind", ["lac", "aps", "raps"])
def test_coverage_on_the_calibration_rows_is_k_over_n(kind):
    z, y, u = cr.make_inputs(257, 10, 1.0)
    s = cr.all_scores(z, kind, u, *cr.params(kind))
    sy = cr.label_scores(z, y, kind, scores=s)
    assert np.unique(sy).size == sy.size
    for alpha in (0.1, 0.3):
        cal = cr.quantile(sy, alpha)
        assert cal["k"] == math.ceil(258 * (1.0 - alpha)) and int((sy <= cal["qhat"]).sum()) == cal["k"]
        m = cr.metrics(cr.set_sizes(s, cal["qhat"]), sy <= cal["qhat"], y, alpha)
        assert m["coverage"] == cal["k"] / 257 and m["n"] == 257


def test_too_few_rows_give_full_sets():
    z, y, _ = cr.make_inputs(3, 10, 1.0)
    s = cr.all_scores(z, "aps")
    cal = cr.quantile(cr.label_scores(z, y, "aps", scores=s), 0.1)                    # k = ceil(4 * 0.9) = 4 > 3
    assert cal == {"qhat": math.inf, "k": 4, "n": 3, "n_skipped": 0, "status": 1}
    assert cr.set_sizes(s, cal["qhat"]).tolist() == [10, 10, 10]
    assert cr.quantile(cr.label_scores(z, y, "aps", scores=s), 0.3)["status"] == 0    # k = ceil(4 * 0.7) = 3


def test_rows_with_a_non_finite_logit_are_left_out():
    z, y, _ = cr.make_inputs(65, 10, 1.0)
    z[0, 3], z[31, 0], z[64, 9] = np.nan, np.inf, -np.inf
    sy = cr.label_scores(z, y, "aps")
    assert np.isnan(sy[[0, 31, 64]]).all() and cr.quantile(sy, 0.1)["n"] == 62 and cr.quantile(sy, 0.1)["n_skipped"] == 3
    assert cr.set_sizes(cr.all_scores(z, "aps"), 0.5)[[0, 31, 64]].tolist() == [-1, -1, -1]
    with pytest.raises(ValueError):
        cr.label_scores(z, np.full(65, 10), "aps")


def test_metrics_by_hand():
    sizes, covered, y = [0, 1, 1, 2, 5, -1, 12], [0, 1, 0, 1, 1, 0, 1], [0, 0, 1, 1, 2, 2, 2]
    m = cr.metrics(sizes, covered, y, 0.1)
    assert (m["n"], m["n_skipped"], m["covered"], m["size_sum"], m["n_empty"], m["n_singleton"], m["max_size"]) == (6, 1, 4, 21, 1, 2, 12)
    assert m["sscv"] == pytest.approx(0.9 - 1.0 / 3.0, abs=1e-15) and m["worst_class"] == 0.5       # bin [0, 1]: 1 of 3 covered


def test_the_bound_is_derived_and_small():
    assert cr.delta(2) == pytest.approx(2 * (2.0 ** -23 + 2.0 ** -24 * math.log(2)), rel=1e-5)
    assert 1.2e-6 < cr.delta(4096) < 1.3e-6 and cr.delta(4096, 0.01, 5) - cr.delta(4096) < 1e-10
    assert all(cr.delta(K) < cr.delta(2 * K) for K in (2, 64, 2048))


def test_the_gpu_comparison_is_not_vacuous():
    """On every GRID case and level: size_ref(qhat + delta) - size_ref(qhat - delta) <= 1 in every row, so the GPU test's two-sided
    bound pins the kernel's size to one of two neighbours.  The one exception is derived, not observed: with qhat >= 1 - (2 K + 1) delta
    the threshold lies in the saturated tail (two classes inside the window have p <= 2 delta, so has every class behind them, and the
    mass that remains is at most 2 K delta): there fp32 exponentials cannot tell the classes of the tail apart and the window is as
    wide as the tail.  The generator's peaked cases (scale 8, the label raised by two standard deviations) put the 90 % quantile of the
    aps score there.  Those levels are counted; every K, every kind and every scale keeps levels outside the exception."""
    wide, seen, narrow = 0, 0, set()
    for case in cr.GRID + cr.GRID_PATHS:
        N, K, scale, kind, with_u = case
        g = cr.grid_case(*case)
        for alpha, cal in zip(cr.ALPHAS, g["cal"]):
            if cal["status"]:
                continue
            seen += 1
            width = int((cr.set_sizes(g["scores"], cal["qhat"] + g["delta"]) - cr.set_sizes(g["scores"], cal["qhat"] - g["delta"])).max())
            saturated = cal["qhat"] >= 1.0 - (2 * K + 1) * g["delta"]
            assert width <= 1 or saturated, (case, alpha, width, cal["qhat"])
            wide += width > 1
            if width <= 1:
                narrow |= {("K", K), ("kind", kind), ("scale", scale), ("u", with_u), ("N", N)}
    print(f"\n{len(cr.GRID + cr.GRID_PATHS)} cases, {seen} levels with a finite qhat, {wide} of them in the saturated tail")
    assert wide * 4 <= seen
    for K in (2, 10, 63, 64, 65, 100, 1003, 4096):
        assert ("K", K) in narrow
    assert {("kind", k) for k in ("lac", "aps", "raps")} | {("scale", s) for s in (1.0, 3.0, 8.0)} | {("u", False), ("u", True)} <= narrow


def test_the_grid_covers_what_it_should():
    Ns, Ks = {c[0] for c in cr.GRID}, {c[1] for c in cr.GRID}
    assert {1, 3, 63, 64, 65, 257} <= Ns and Ks == {2, 10, 63, 64, 65, 100, 1003, 4096}
    for K in Ks:
        assert {c[0] for c in cr.GRID if c[1] == K} & {65, 130, 257}, K                # more than one workgroup of rows
        assert {c[3] for c in cr.GRID if c[1] == K} == {"lac", "aps", "raps"}, K
        assert {c[4] for c in cr.GRID if c[1] == K} == {False, True}, K
    assert {c[2] for c in cr.GRID} == {1.0, 3.0, 8.0}


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL, 16-byte aligned pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE, WORKSPACE = -1, -2, -4
NAMES = ("uvit_op_cp_scores", "uvit_op_cp_ws_bytes", "uvit_op_cp_quantile", "uvit_op_cp_counter_count", "uvit_op_cp_sets", "uvit_op_cp_finish")
BAD_KIND = (dict(kind=-1), dict(kind=3), dict(kind=2, lam=-0.01), dict(kind=2, lam=float("nan")), dict(kind=2, lam=float("inf")),
            dict(kind=2, kreg=-1))
BAD_K = (dict(K=1), dict(K=0), dict(K=4097), dict(K=10, ld=9))


def test_symbols_are_declared_and_exported():
    from uncertainty_vit_amd import native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uvit.h")).read()
    for name in NAMES:
        assert name in native.SYMBOLS and name + "(" in hdr and getattr(native.lib(), name).argtypes is not None
    assert native.lib().uvit_version() == 100


def test_scores_rejects_bad_arguments(L):
    good = dict(logits=P1, ld=10, labels=P1, u=NUL, N=100, K=10, kind=1, lam=0.0, kreg=0, scores=P1)

    def call(**kw):
        a = {**good, **kw}
        return L.uvit_op_cp_scores(a["logits"], a["ld"], a["labels"], a["u"], a["N"], a["K"], a["kind"], a["lam"], a["kreg"], a["scores"], NUL)

    for kw in (dict(N=0), dict(N=-1), dict(N=(1 << 20) + 1)) + BAD_K + BAD_KIND:
        assert call(**kw) == SHAPE, kw
    for name in ("logits", "labels", "scores"):
        assert call(**{name: NUL}) == ARG, name


def test_quantile_rejects_bad_arguments(L):
    for N, A in [(0, 1), (-1, 1), ((1 << 20) + 1, 1), (10, 0), (10, 9), (10, -1)]:
        assert L.uvit_op_cp_ws_bytes(N, A) == SHAPE, (N, A)
    ws = L.uvit_op_cp_ws_bytes(100, 2)
    assert 0 < ws <= 1 << 20 and ws == L.uvit_op_cp_ws_bytes(1 << 20, 8)
    alphas = (C.c_double * 8)(0.1, 0.3, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
    good = dict(scores=P1, N=100, alphas=alphas, A=2, table=P1, ws=P1, ws_bytes=ws)

    def call(**kw):
        a = {**good, **kw}
        return L.uvit_op_cp_quantile(a["scores"], a["N"], a["alphas"], a["A"], a["table"], a["ws"], a["ws_bytes"], NUL)

    for kw in (dict(N=0), dict(N=(1 << 20) + 1), dict(A=0), dict(A=9)):
        assert call(**kw) == SHAPE, kw
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert call(alphas=(C.c_double * 8)(0.1, bad), A=2) == SHAPE, bad
    for name in ("scores", "alphas", "table", "ws"):
        assert call(**{name: NUL}) == ARG, name
    assert call(ws=C.c_void_p(4100)) == ARG                        # not 16-byte aligned
    assert call(ws_bytes=ws - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE


def test_sets_and_finish_reject_bad_arguments(L):
    for K, A in [(1, 1), (4097, 1), (10, 0), (10, 9)]:
        assert L.uvit_op_cp_counter_count(K, A) == SHAPE, (K, A)
    assert L.uvit_op_cp_counter_count(10, 2) == 4 + 20 * 2 + 10 * 3
    good = dict(logits=P1, ld=10, labels=P1, u=NUL, B=100, K=10, kind=1, lam=0.0, kreg=0, table=P1, A=2, counters=P1, sizes=NUL, covered=NUL,
                ld_out=100)

    def call(**kw):
        a = {**good, **kw}
        return L.uvit_op_cp_sets(a["logits"], a["ld"], a["labels"], a["u"], a["B"], a["K"], a["kind"], a["lam"], a["kreg"], a["table"], a["A"],
                                 a["counters"], a["sizes"], a["covered"], a["ld_out"], NUL)

    for kw in (dict(B=0), dict(B=(1 << 20) + 1), dict(A=0), dict(A=9), dict(sizes=P1, ld_out=99), dict(covered=P1, ld_out=0)) + BAD_K + BAD_KIND:
        assert call(**kw) == SHAPE, kw
    for name in ("logits", "labels", "table", "counters"):
        assert call(**{name: NUL}) == ARG, name
    assert L.uvit_op_cp_finish(NUL, P1, 10, 2, NUL) == ARG and L.uvit_op_cp_finish(P1, NUL, 10, 2, NUL) == ARG
    for K, A in [(1, 1), (4097, 1), (10, 0), (10, 9)]:
        assert L.uvit_op_cp_finish(P1, P1, K, A, NUL) == SHAPE, (K, A)


# ---- the module and the command line ----
def _probe():
    from test_host_probe import tiny_encoder
    from uncertainty_vit_amd.linear_probe import LinearProbe
    return LinearProbe(tiny_encoder().eval(), 10)


def test_conformal_sets_need_a_gpu():
    """No CPU fallback: host tensors are refused; evaluate_conformal needs a fitted or set state; bad settings are refused."""
    import torch
    from uncertainty_vit_amd.native import UvitError
    probe = _probe()
    z, y = torch.zeros(8, 10), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(UvitError):
        probe.conformal_calibrate(z, y)
    with pytest.raises(UvitError):
        probe.conformal_sets(z, y, {"alpha": [0.1], "score": "aps", "lam": 0.0, "kreg": 0, "table": None})
    with pytest.raises(UvitError):
        probe.evaluate_conformal([])
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha=[0.1] * 9), dict(alpha=[]), dict(score="top"), dict(score="raps", lam=-1.0),
               dict(score="raps", kreg=-1)):
        with pytest.raises(UvitError):
            probe.conformal_calibrate(z, y, **kw)
    with pytest.raises(UvitError):
        probe.set_conformal({"alpha": [0.1]})


def test_the_state_is_no_parameter_and_no_buffer():
    probe = _probe()
    keys = list(probe.state_dict())
    assert probe.conformal is None
    state = {"table": None, "alpha": [0.1], "score": "lac", "lam": 0.0, "kreg": 0}
    probe.set_conformal(state)
    assert probe.conformal["score"] == "lac"
    assert list(probe.state_dict()) == keys == ["head.weight", "head.bias"]
    assert [n for n, _ in probe.named_buffers()] == []
    probe.set_conformal(None)
    assert probe.conformal is None


def test_every_head_inherits_the_members():
    import inspect
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    for cls in (LinearProbe, GPProbe, HetProbe, EnsembleProbe):
        for name in ("fit_conformal", "evaluate_conformal", "conformal_calibrate", "conformal_sets", "set_conformal", "conformal"):
            assert hasattr(cls, name), (cls, name)
        assert list(inspect.signature(cls.evaluate).parameters)[-1] == "temperature"          # evaluate() is not touched
        assert "conformal" not in "".join(inspect.signature(cls.evaluate).parameters)
    want = ["self", "loader", "alpha", "score", "lam", "kreg", "randomized", "seed", "temperature"]
    assert list(inspect.signature(LinearProbe.fit_conformal).parameters) == want
    assert list(inspect.signature(LinearProbe.evaluate_conformal).parameters) == ["self", "loader", "sizes", "temperature"]
    assert "mean_field" in inspect.signature(GPProbe.fit_conformal).parameters
    assert "mean_field" in inspect.signature(GPProbe.evaluate_conformal).parameters


def test_cli_flags_are_absent_unless_given():
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()
    base = vars(rlp.get_args([]))
    assert not any(k.startswith("cp_") for k in base)
    a = rlp.get_args(["--eval", "--cp_data_path", "x", "--cp_alpha", "0.1", "0.3", "--cp_score", "raps", "--cp_lambda", "0.02", "--cp_kreg", "3",
                      "--cp_randomized", "--cp_seed", "7"])
    assert (a.cp_data_path, a.cp_alpha, a.cp_score, a.cp_lambda, a.cp_kreg, a.cp_randomized, a.cp_seed) == ("x", [0.1, 0.3], "raps", 0.02, 3, True, 7)
    assert rlp.check_cp_flags(a) is True
    for flags in (["--cp_data_path", "x"], ["--cp_alpha", "0.2"], ["--cp_score", "lac"], ["--cp_lambda", "0.1"], ["--cp_kreg", "2"],
                  ["--cp_randomized"], ["--cp_seed", "1"]):
        with pytest.raises(ValueError, match="--eval"):
            rlp.check_cp_flags(rlp.get_args(flags))
    for flags in (["--cp_alpha", "0.2"], ["--cp_score", "lac"], ["--cp_randomized"], ["--cp_seed", "1"], ["--cp_score", "raps", "--cp_kreg", "2"]):
        with pytest.raises(ValueError, match="--cp_data_path"):
            rlp.check_cp_flags(rlp.get_args(["--eval"] + flags))
    for flags in (["--cp_lambda", "0.1"], ["--cp_kreg", "2"], ["--cp_score", "aps", "--cp_lambda", "0.1"], ["--cp_score", "lac", "--cp_kreg", "2"]):
        with pytest.raises(ValueError, match="raps"):
            rlp.check_cp_flags(rlp.get_args(["--eval", "--cp_data_path", "x"] + flags))
    assert rlp.check_cp_flags(rlp.get_args(["--eval", "--cp_data_path", "x"])) is True
    assert rlp.check_cp_flags(rlp.get_args(["--eval"])) is False and rlp.check_cp_flags(rlp.get_args([])) is False
    with pytest.raises(SystemExit):
        rlp.get_args(["--cp_score", "top"])


def test_cli_lines_and_log_entries():
    import run_linear_probe as rlp
    fit = {"score": "raps", "alpha": [0.1, 0.3], "qhat": [0.987654321, math.inf], "k": [9, 7], "n": 9, "n_skipped": 0, "status": [0, 1]}
    row = dict(coverage=1.0, size=2.5, empty=0.0, singleton=0.25, max_size=3, sscv=0.1, worst_class=0.5, n=6, n_skipped=0)
    conf = {0.1: row, 0.3: {**row, "coverage": 0.75, "size": 3.0}}
    assert rlp.conformal_lines(fit, conf) == [
        "* Conformal raps alpha 0.1 qhat 0.98765 coverage 1.00000 size 2.500 empty 0.00000 singleton 0.25000 SSCV 0.10000 worst-class 0.50000 "
        "on 9 calibration images",
        "* Conformal raps alpha 0.3 qhat inf coverage 0.75000 size 3.000 empty 0.00000 singleton 0.25000 SSCV 0.10000 worst-class 0.50000 "
        "on 9 calibration images"]
    assert rlp.conformal_log_entries(fit, conf) == {
        "test_cp_alpha": [0.1, 0.3], "test_cp_qhat": [0.987654321, math.inf], "test_cp_coverage": [1.0, 0.75], "test_cp_size": [2.5, 3.0],
        "test_cp_empty": [0.0, 0.0], "test_cp_singleton": [0.25, 0.25], "test_cp_sscv": [0.1, 0.1], "test_cp_worst_class": [0.5, 0.5],
        "test_cp_n_cal": 9}
