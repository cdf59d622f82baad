"""CPU: the Laplace probe's host-side pieces -- the float64 restatement (tests/lap_ref.py) against the dense K D x K D matrices it
abbreviates, float64's own error against np.longdouble (a quarter of every bound the GPU tests use), the marginal-likelihood grid
search, the argument checks of every uvit_op_lap_* entry point (they return before anything touches a device), the LaplaceProbe
module's state dict and signatures, and the command line's new flags."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import lap_ref as lr
from test_host_probe import tiny_encoder

LD = np.longdouble


# ---- the restatement against the dense matrices ----
@pytest.fixture(scope="module")
def small():
    """C = 7, K = 5, n = 40: float64 features, logits and labels, their factors and eigen-decompositions."""
    rng = np.random.default_rng(5)
    f, z, y = rng.standard_normal((40, 7)), 2.0 * rng.standard_normal((40, 5)), rng.integers(0, 5, 40)
    A, Gs, sums = lr.factors(f, z, y)
    G = Gs / sums[1]
    return f, z, y, A, G, sums, lr.eig(A, G)


def test_eigen_form_variance_is_the_dense_diagonal(small):
    """var = (phi U_A)^2 T equals diag(J (kron(G, A) + tau I)^-1 J^T) within 1e-12 relative (4e-15 observed)."""
    f, _, _, A, G, _, (la, UA, lg, UG) = small
    for tau in (1e-2, 1.0, 30.0):
        got = lr.variance(f, UA, lr.t_matrix(UG, la, lg, tau))
        want = lr.variance_dense(f, A, G, tau)
        err = float(np.abs(got / want - 1).max())
        print(f"tau {tau}: largest relative difference {err:.2e}")
        assert err <= 1e-12


def test_kron_is_the_ggn_of_one_sample(small):
    """For n = 1, kron(G_1, A_1) = J^T H J with H = diag(p) - p p^T the Hessian of the cross-entropy in the logits."""
    f, z, y = small[:3]
    A, Gs, sums = lr.factors(f[:1], z[:1], y[:1])
    assert sums[1] == 1
    p = lr.softmax_parts(z[:1])[0][0]
    J = lr.jacobian(lr.phi_of(f[:1])[0], 5)
    np.testing.assert_allclose(np.kron(Gs, A), J.T @ (np.diag(p) - np.outer(p, p)) @ J, rtol=0, atol=1e-14 * float(np.abs(A).max()))


def test_log_determinant_term_is_slogdet_of_the_dense_matrix(small):
    _, _, _, A, G, sums, (la, _, lg, _) = small
    for tau in (1e-3, 1.0, 100.0):
        sign, logdet = np.linalg.slogdet(lr.dense_precision(A, G, tau))
        assert sign == 1.0 and float(np.log(np.outer(la, lg) + tau).sum()) == pytest.approx(logdet, rel=1e-12)
        # and so the marginal likelihood is the textbook -nll - tau |theta|^2 / 2 + (P log tau - logdet) / 2
        assert lr.log_marglik(tau, sums[0], 3.0, la, lg) == pytest.approx(-sums[0] - 1.5 * tau + 0.5 * (40 * np.log(tau) - logdet), rel=1e-12)


def test_variance_decreases_in_tau_and_the_link_vanishes(small):
    f, z, _, _, _, _, (la, UA, lg, UG) = small
    taus = [1e-4, 1e-2, 1.0, 1e2, 1e4, 1e12]
    var = [lr.variance(f, UA, lr.t_matrix(UG, la, lg, t)) for t in taus]
    for a, b in zip(var, var[1:]):
        assert bool((b < a).all())
    assert bool((np.abs(lr.probit(z, var[0])) < np.abs(z)).all())
    np.testing.assert_allclose(lr.probit(z, var[-1]), z, rtol=1e-10)                  # z~ -> z as tau -> infinity
    # lap_var: the variance at the arg-max of the unscaled logits, the lowest index on ties
    zt = np.array([[1.0, 3.0, 3.0, 0.0, 3.0]])
    assert lr.lap_var(zt, np.arange(5.0)[None])[0] == 1.0
    # a NaN or negative variance gives NaN in that entry alone
    v = var[2][:1].copy()
    v[0, 1], v[0, 3] = np.nan, -1.0
    assert np.isnan(lr.probit(z[:1], v)[0]).tolist() == [False, True, False, True, False]


def test_grid_search_returns_the_brute_force_arg_max(small):
    from uncertainty_vit_amd import lap_probe as lp
    _, _, _, _, _, sums, (la, _, lg, _) = small
    grid = lr.marglik_grid()
    assert len(grid) == 97 and grid[0] == pytest.approx(1e-4) and grid[-1] == pytest.approx(1e8) and np.array_equal(grid, lp.marglik_grid())
    for theta_sq, nll in ((3.0, float(sums[0])), (0.0, 0.0), (1e12, 5.0)):
        vals = [lr.log_marglik(t, nll, theta_sq, la, lg) for t in grid]
        best = max(range(97), key=lambda i: (vals[i], -i))                             # the first point wins ties
        tau, ml, edge = lr.choose_prior_precision(nll, theta_sq, la, lg)
        assert (tau, edge) == (grid[best], best in (0, 96)) and ml == vals[best]
        tau2, ml2, edge2 = lp.choose_prior_precision(nll, theta_sq, torch.from_numpy(la), torch.from_numpy(lg))
        assert (tau2, edge2) == (tau, edge) and ml2 == pytest.approx(ml, rel=1e-12)
        assert lp.log_marglik(2.5, nll, theta_sq, la, lg) == pytest.approx(lr.log_marglik(2.5, nll, theta_sq, la, lg), rel=1e-12)
    assert lr.choose_prior_precision(0.0, 0.0, la, lg)[2] and lr.choose_prior_precision(5.0, 1e12, la, lg)[2]      # both ends of the grid
    assert not lr.choose_prior_precision(float(sums[0]), 3.0, la, lg)[2]


# ---- float64 against np.longdouble: the reference's own error is a quarter of every bound at most ----
def _some(n, k=8):
    return np.unique(np.linspace(0, n - 1, min(n, k)).round().astype(int))


@pytest.mark.skipif(np.finfo(LD).eps >= np.finfo(np.float64).eps, reason="np.longdouble is float64 on this platform")
@pytest.mark.parametrize("B,Cd,K", lr.SHAPES)
def test_float64_restatement_stays_within_a_quarter_of_the_bounds(B, Cd, K):
    """NumPy float64 against the same formulas in np.longdouble on the cases the GPU tests use (at the largest shape on rows and
    columns spread over the outputs: longdouble products do not go through BLAS).  Observed |error| / bound, the largest over the
    five shapes and the three tau: A 0.066, G 0.061, nll 0.0027, T 0.17 (at K = 10, where the bound is 18 u), var 0.068."""
    case = lr.make_case(B, Cd, K)
    fs, zs, ys = ([c[i] for c in case] for i in range(3))
    rows_a, rows_g = _some(Cd + 1), _some(K)
    A = sum(lr.factors(*c)[0] for c in case)
    G = sum(lr.factors(*c)[1] for c in case)
    nll = sum(lr.factors(*c)[2][0] for c in case)
    A_ld, G_ld, nll_ld = 0, 0, LD(0)
    for f, z, y in case:
        ph = lr.phi_of(f, LD)
        p, logs, m = lr.softmax_parts(z, LD)
        A_ld = A_ld + ph[:, rows_a].T @ ph
        Gd = -(p[:, rows_g].T @ p)
        Gd[np.arange(len(rows_g)), rows_g] += p[:, rows_g].sum(axis=0)
        G_ld = G_ld + Gd
        nll_ld += (logs - (z.astype(LD)[np.arange(B), y] - m)).sum()
    ratio = {"A": np.abs(A[rows_a] - A_ld).astype(float) / lr.bound_A(fs, zs, ys)[rows_a],
             "G": np.abs(G[rows_g] - G_ld).astype(float) / lr.bound_G(zs, ys)[rows_g],
             "nll": np.array([abs(float(nll - nll_ld)) / lr.bound_nll(zs, ys)])}
    la, UA, lg, UG = lr.eig(A, G / (2 * B))
    some_b = _some(B, 4)
    for tau in (1e-4, 1.0, 1e4):
        T = lr.t_matrix(UG, la, lg, tau)
        cols = _some(K)
        inv = 1 / (la.astype(LD)[rows_a, None] * lg.astype(LD)[None, :] + LD(tau))
        T_ld = inv @ (UG.astype(LD)[cols] ** 2).T
        ratio[f"T {tau:g}"] = np.abs(T[np.ix_(rows_a, cols)] / T_ld.astype(float) - 1) / lr.bound_T_rel(K)
        f = fs[0][some_b]
        a_ld = lr.phi_of(f, LD) @ UA.astype(LD)
        var_ld = (a_ld ** 2) @ T.astype(LD)[:, cols]
        ratio[f"var {tau:g}"] = np.abs(lr.variance(f, UA, T)[:, cols] - var_ld).astype(float) / lr.bound_var(f, UA, T)[:, cols]
    for key, r in ratio.items():
        print(f"{(B, Cd, K)} {key}: |float64 - longdouble| / bound = {float(r.max()):.3g}")
        assert float(r.max()) <= 0.25, key


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any aligned non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE, WORKSPACE = -1, -2, -4
BAD_CK = [(6, 10), (0, 10), (2052, 10), (64, 1), (64, 4097)]
BAD_B = [0, 65536]
SYMBOLS = ("uvit_op_lap_factors_ws_bytes", "uvit_op_lap_factors", "uvit_op_lap_prepare", "uvit_op_lap_variance_ws_bytes",
           "uvit_op_lap_variance", "uvit_op_lap_probit")


def d(v):
    return C.c_double(v)


def off(n):
    return C.c_void_p(4096 + n)


def test_symbols_are_declared_exported_and_bound():
    import os
    from uncertainty_vit_amd import native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uvit.h")).read()
    raw = C.CDLL(native.LIB_PATH)
    for name in SYMBOLS:
        assert name in native.SYMBOLS and name + "(" in hdr and hasattr(raw, name) and getattr(native.lib(), name).argtypes is not None
    assert native.lib().uvit_version() == 100


def test_factors_rejects_bad_arguments(L):
    ws = L.uvit_op_lap_factors_ws_bytes(4, 64, 10)
    assert ws == (4 * 10 + 4) * 8 + 16
    assert L.uvit_op_lap_factors_ws_bytes(128, 768, 1000) == (128 * 1000 + 128) * 8 + 512
    call = lambda p, B=4, Cd=64, K=10, ld=10, nb=ws: L.uvit_op_lap_factors(p[0], p[1], ld, *p[2:7], nb, B, Cd, K, NUL)      # noqa: E731
    assert call([P1] * 7, 0) == SHAPE
    for Cd, K in BAD_CK:
        assert L.uvit_op_lap_factors_ws_bytes(4, Cd, K) == SHAPE and call([P1] * 7, Cd=Cd, K=K, ld=max(K, 1)) == SHAPE, (Cd, K)
    for B in BAD_B:
        assert L.uvit_op_lap_factors_ws_bytes(B, 64, 10) == SHAPE and call([P1] * 7, B=B) == SHAPE, B
    assert call([P1] * 7, ld=9) == SHAPE
    for i in range(7):                           # feat, logits, labels, A, G, sums, ws
        a = [P1] * 7
        a[i] = NUL
        assert call(a) == ARG, i
        a[i] = off(2)                            # not aligned to a float, a double, an int64 or 16 bytes
        assert call(a) == ARG, i
    for i, n in ((2, 4), (3, 4), (4, 4), (5, 4), (6, 8)):      # 8-byte elements at a multiple of 4, the workspace at a multiple of 8
        a = [P1] * 7
        a[i] = off(n)
        assert call(a) == ARG, (i, n)
    assert call([P1] * 7, nb=ws - 1) == WORKSPACE


def test_prepare_rejects_bad_arguments(L):
    call = lambda p, tau=1.0, Cd=64, K=10: L.uvit_op_lap_prepare(*p[:3], d(tau), p[3], Cd, K, NUL)      # noqa: E731
    for Cd, K in BAD_CK:
        assert call([P1] * 4, Cd=Cd, K=K) == SHAPE, (Cd, K)
    for i in range(4):
        a = [P1] * 4
        a[i] = NUL
        assert call(a) == ARG, i
        a[i] = off(4)
        assert call(a) == ARG, i
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert call([P1] * 4, tau=tau) == ARG, tau


def test_variance_rejects_bad_arguments(L):
    ws = L.uvit_op_lap_variance_ws_bytes(3, 64, 10)
    assert ws == (3 * 65 * 8 + 15) // 16 * 16
    call = lambda p, B=3, Cd=64, K=10, nb=ws: L.uvit_op_lap_variance(*p, nb, B, Cd, K, NUL)      # noqa: E731
    for Cd, K in BAD_CK:
        assert L.uvit_op_lap_variance_ws_bytes(3, Cd, K) == SHAPE and call([P1] * 5, Cd=Cd, K=K) == SHAPE, (Cd, K)
    for B in BAD_B:
        assert L.uvit_op_lap_variance_ws_bytes(B, 64, 10) == SHAPE and call([P1] * 5, B=B) == SHAPE, B
    for i in range(5):                           # feat, UA, T, var, ws
        a = [P1] * 5
        a[i] = NUL
        assert call(a) == ARG, i
        a[i] = off(2)
        assert call(a) == ARG, i
    a = [P1] * 5
    a[4] = off(8)
    assert call(a) == ARG
    assert call([P1] * 5, nb=ws - 1) == WORKSPACE


def test_probit_rejects_bad_arguments(L):
    call = lambda p, B=4, K=10, ld=10, ldo=10, fac=0.4: L.uvit_op_lap_probit(p[0], ld, p[1], d(fac), p[2], ldo, p[3], B, K, NUL)      # noqa: E731
    for B in BAD_B:
        assert call([P1] * 4, B=B) == SHAPE, B
    for K in (1, 4097):
        assert call([P1] * 4, K=K, ld=K, ldo=K) == SHAPE, K
    assert call([P1] * 4, ld=9) == SHAPE and call([P1] * 4, ldo=9) == SHAPE
    for i in range(3):                           # logits, var, out are required; lap_var is not
        a = [P1] * 4
        a[i] = NUL
        assert call(a) == ARG, i
    for i in range(4):
        a = [P1] * 4
        a[i] = off(2)
        assert call(a) == ARG, i
    for fac in (-0.1, float("nan"), float("inf")):
        assert call([P1] * 4, fac=fac) == ARG, fac


# ---- the module ----
def test_laplace_probe_state_dict_signature_and_no_cpu_fallback():
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    torch.manual_seed(3)
    probe = LaplaceProbe(tiny_encoder().eval(), 10)
    torch.manual_seed(3)
    plain = LinearProbe(tiny_encoder().eval(), 10)
    assert isinstance(probe, LinearProbe) and probe.laplace is None
    keys = {"head.weight": (10, 128), "head.bias": (10,)}
    assert {k: tuple(v.shape) for k, v in probe.state_dict().items()} == keys
    assert all(torch.equal(v, plain.state_dict()[k]) for k, v in probe.state_dict().items())           # the linear head's draws
    assert not list(probe.buffers()) and [n for n, _ in probe.named_parameters()] == list(keys)
    assert probe.DETECT_COLUMNS == LinearProbe.DETECT_COLUMNS                   # unfitted: what a LinearProbe stores and launches
    # a fit state set by hand: neither a parameter nor a buffer, and the fitted probe has the class's columns
    probe._lap = {"info": {"n": 3, "n_skipped": 0, "nll": 1.0, "prior_precision": 1.0, "log_marglik": -2.0, "on_grid_edge": False}}
    probe.__dict__.pop("DETECT_COLUMNS")
    assert {k: tuple(v.shape) for k, v in probe.state_dict().items()} == keys and not list(probe.buffers())
    assert probe.laplace["n"] == 3 and probe.DETECT_COLUMNS[-1] == "lap_var"
    probe.load_state_dict(plain.state_dict())                                   # a linear probe's checkpoint loads and drops the fit
    assert probe.laplace is None and probe.DETECT_COLUMNS == LinearProbe.DETECT_COLUMNS
    probe.set_laplace(None)
    params = list(inspect.signature(LaplaceProbe.evaluate).parameters)
    assert params == ["self", "loader", "calibration", "detection", "ood_loader", "variance", "temperature"]
    assert list(inspect.signature(LaplaceProbe.fit_laplace).parameters) == ["self", "loader", "prior_precision"]
    # no CPU fallback
    x, y = torch.zeros(2, 3, 48, 48), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(UvitError):
        probe.logits(x)
    with pytest.raises(UvitError):
        probe.fit_laplace([(x, y)])
    with pytest.raises(UvitError):
        probe.predictive_variance(x)
    with pytest.raises(UvitError):
        probe.evaluate([(x, y)])
    with pytest.raises(UvitError):
        probe.set_prior_precision(2.0)
    with pytest.raises(UvitError):
        probe.laplace_state_dict()
    with pytest.raises(UvitError):
        probe.load_laplace_state({"A": 0})
    with pytest.raises(ValueError):
        probe.fit_laplace([], prior_precision=0.0)
    with pytest.raises(ValueError):
        probe.fit_laplace([], prior_precision="evidence")
    with pytest.raises(NotImplementedError):
        LaplaceProbe(tiny_encoder(two_stream=True).eval(), 10)
    with pytest.raises(ValueError):
        LaplaceProbe(tiny_encoder().eval(), 1)


def test_detect_columns_of_all_five_classes():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    base = ("msp", "entropy", "energy")
    assert LinearProbe.DETECT_COLUMNS == base
    assert GPProbe.DETECT_COLUMNS == base + ("gp_var",)
    assert HetProbe.DETECT_COLUMNS == base + ("het_var",)
    assert EnsembleProbe.DETECT_COLUMNS == base + ("ens_total", "ens_aleatoric", "ens_mi", "ens_var", "ens_disagreement")
    assert LaplaceProbe.DETECT_COLUMNS == base + ("lap_var",)


# ---- the command line ----
def test_cli_flags_are_absent_unless_given():
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()                                  # the parsed defaults without --laplace equal today's
    got = vars(rlp.get_args([]))
    assert not [k for k in got if k.startswith("lap")]
    assert rlp.check_lap_flags(rlp.get_args([])) is False
    a = rlp.get_args(["--laplace"])
    assert a.laplace is True and not any(hasattr(a, k) for k in rlp.LAP_FLAGS) and rlp.check_lap_flags(a) is True
    a = rlp.get_args(["--eval", "--laplace", "--lap_data_path", "d", "--lap_prior_precision", "marglik"])
    assert (a.lap_data_path, a.lap_prior_precision) == ("d", "marglik") and rlp.check_lap_flags(a) and rlp.lap_prior_precision(a) == "marglik"
    a = rlp.get_args(["--eval", "--laplace", "--lap_state", "s.pth", "--lap_prior_precision", "2.5"])
    assert rlp.check_lap_flags(a) and rlp.lap_prior_precision(a) == 2.5 and rlp.lap_prior_precision(rlp.get_args(["--laplace"])) is None


def test_cli_refuses_what_does_not_go_together():
    import run_linear_probe as rlp
    for head in ("--gp_layer", "--het_layer", "--ensembles"):
        with pytest.raises(ValueError):
            rlp.check_lap_flags(rlp.get_args(["--laplace", head]))
    with pytest.raises(ValueError):                                          # an evaluation needs the data to fit on, or a saved fit
        rlp.check_lap_flags(rlp.get_args(["--eval", "--laplace"]))
    with pytest.raises(ValueError):
        rlp.check_lap_flags(rlp.get_args(["--eval", "--laplace", "--lap_data_path", "d", "--lap_state", "s.pth"]))
    with pytest.raises(ValueError):
        rlp.check_lap_flags(rlp.get_args(["--laplace", "--lap_state", "s.pth"]))
    for flag, val in (("--lap_data_path", "d"), ("--lap_prior_precision", "1.0"), ("--lap_state", "s.pth")):
        with pytest.raises(ValueError):
            rlp.check_lap_flags(rlp.get_args(["--eval", flag, val]))
    for bad in ("0", "-1", "nan", "inf", "evidence"):
        with pytest.raises(ValueError):
            rlp.check_lap_flags(rlp.get_args(["--laplace", "--lap_data_path", "d", "--lap_prior_precision", bad]))


def test_cli_lines_and_log_entries():
    import run_linear_probe as rlp
    fit = {"n": 200, "n_skipped": 0, "nll": 460.0, "prior_precision": 10.0, "log_marglik": -512.25, "on_grid_edge": False, "source": "marglik"}
    stats = {"lap_var_mean": 0.125}
    assert rlp.laplace_lines(fit, stats) == ["* Laplace prior precision 10 (marglik) log-marglik -512.25000 NLL 2.30000 on 200 images",
                                             "* Laplace variance mean 0.125000"]
    fit.update(on_grid_edge=True, prior_precision=1e-4)
    assert rlp.laplace_lines(fit, stats)[0].startswith("* Laplace prior precision 0.0001 (marglik, grid edge) log-marglik")
    fit.update(on_grid_edge=False, source="given")
    assert "(given)" in rlp.laplace_lines(fit, stats)[0]
    assert rlp.laplace_log_entries(fit, stats) == {"test_lap_prior_precision": 1e-4, "test_lap_log_marglik": -512.25, "test_lap_var_mean": 0.125}
