"""CPU: the Mahalanobis scores' host-side pieces -- the float64 restatement (tests/maha_ref.py) against the brute-force inverse form,
the null direction of the tied covariance, the argument checks of the uvit_op_maha_* entry points (they return before anything
touches a device), the density state of the five probe classes and their detection columns, and the command line's new flags."""
import ctypes as C

import numpy as np
import pytest
import torch

import maha_ref as mr
from test_host_probe import tiny_encoder


# ---- the restatement ----
@pytest.fixture(scope="module")
def meaning():
    K, Cd, fit_set, held_out, noise = mr.meaning_case(0)
    return K, Cd, fit_set, held_out, noise, mr.accumulate(*fit_set, K)


@pytest.mark.parametrize("rho", [1e-6, 1e-3, 1e-2])
def test_whitened_form_is_the_brute_force_inverse_form(meaning, rho):
    """|W f - W mu|^2 equals (f - mu)^T Sigma_reg^-1 (f - mu) through np.linalg.inv to 1e-10 relative (1e-10 observed at rho = 1e-6,
    where the condition number is largest; 6e-14 at 1e-3), for the class distances and the background's."""
    K, Cd, _, (f, _), noise, sums = meaning
    ft = mr.fit(*sums, rho)
    for x in (f, noise):
        got = mr.scores(x, ft["W"], ft["W0"], ft["Wmu"], ft["Wmu0"], ft["class_count"])
        d, d0 = mr.scores_brute_force(x, ft["mu"], ft["mu0"], ft["sigma"], ft["sigma0"])
        err, err0 = float(np.abs(got["dist"] / d - 1).max()), float(np.abs(got["d0"] / d0 - 1).max())
        print(f"rho {rho}: largest relative difference  d_k {err:.2e}  d_0 {err0:.2e}")
        assert err <= 1e-10 and err0 <= 1e-10
        np.testing.assert_array_equal(got["maha"], got["dist"].min(axis=1))
        np.testing.assert_array_equal(got["rmaha"], got["maha"] - got["d0"])


def test_meaning_of_the_scores_on_the_synthetic_set(meaning):
    """Held-out cluster rows against normalised noise: OOD AUROC 1.0 for both columns and nearest-class-mean accuracy 1.0."""
    K, Cd, _, (f, y), noise, sums = meaning
    for rho in (1e-6, 1e-3, 1e-2):
        ft = mr.fit(*sums, rho)
        a, b = (mr.scores(x, ft["W"], ft["W0"], ft["Wmu"], ft["Wmu0"], ft["class_count"]) for x in (f, noise))
        assert mr.auroc(a["maha"], b["maha"]) == 1.0 and mr.auroc(a["rmaha"], b["rmaha"]) == 1.0 and bool((a["pred"] == y).all())


def test_null_direction_of_the_tied_covariance(meaning):
    """The normalisation removes the mean over the C entries of every feature, so Sigma 1 = 0: without shrinkage the smallest
    eigenvalue is below 1e-12 tr Sigma / C (7.6e-17 observed at C = 16), and the Cholesky factorisation needs the shrinkage."""
    K, Cd, (f, _), _, _, sums = meaning
    assert float(np.abs(f.astype(np.float64).sum(axis=1)).max()) < 1e-5
    _, _, sigma, sigma0 = mr.covariances(*sums, 0.0)
    for m in (sigma, sigma0):
        lam = np.linalg.eigvalsh(m)
        print(f"smallest eigenvalue {lam[0]:.2e}, tr / C {np.trace(m) / Cd:.3f}")
        assert abs(lam[0]) < 1e-12 * np.trace(m) / Cd
    _, _, reg, _ = mr.covariances(*sums, 1e-3)
    assert np.linalg.eigvalsh(reg)[0] == pytest.approx(1e-3 * np.trace(sigma) / Cd, rel=1e-6)


def test_rules_of_the_restatement():
    """Skipped rows, the tie rule, the empty-class rule and the NaN rule."""
    f = mr.normalise(np.random.default_rng(1).standard_normal((6, 4)))
    f[2, 1] = np.nan
    y = np.array([0, 1, 1, -1, 3, 2])
    S, cs, ts, cc, sums = mr.accumulate(f, y, 3)
    assert sums.tolist() == [3, 3] and cc.tolist() == [1, 1, 1]
    np.testing.assert_array_equal(ts, f[[0, 1, 5]].astype(np.float64).sum(axis=0))
    eye = np.eye(4)
    Wmu = np.array([[9.0, 0, 0, 0], [1.0, 0, 0, 0], [-1.0, 0, 0, 0], [0.0, 0, 0, 0]])
    x = np.zeros((2, 4), dtype=np.float32)
    x[1, 3] = np.inf
    out = mr.scores(x, eye, eye, Wmu, np.zeros(4), np.array([1.0, 2.0, 2.0, 0.0]))
    assert out["pred"].tolist() == [1, -1] and out["maha"][0] == 1.0 and np.isnan(out["maha"][1]) and np.isnan(out["rmaha"][1])
    assert np.isnan(out["dist"][1]).all() and out["dist"][0].tolist() == [81.0, 1.0, 1.0, 0.0]      # class 3 is nearest but empty
    assert mr.scores(x, eye, eye, Wmu, np.zeros(4), np.zeros(4))["pred"].tolist() == [-1, -1]


@pytest.mark.parametrize("shape", mr.SHAPES)
def test_pred_is_decided_on_the_gpu_cases(shape):
    """On the shapes the GPU tests use, the restatement's two smallest distances differ by more than their bounds in at least 99 % of
    the rows (all of them, observed), and the bounds are a few fp32 ulps of the scores."""
    case = mr.make_case(*shape)
    ft = case["fit"]
    ref = mr.scores(case["feat"], ft["W"], ft["W0"], ft["Wmu"], ft["Wmu0"], ft["class_count"])
    bm, br, decided = mr.bounds_scores(case["feat"], ft, ref)
    assert decided.mean() >= 0.99
    assert float((bm / np.abs(ref["maha"])).max()) < 2 * mr.U32


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
SYMBOLS = ("uvit_op_maha_accumulate_ws_bytes", "uvit_op_maha_accumulate", "uvit_op_maha_scores_ws_bytes", "uvit_op_maha_scores")


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


def test_accumulate_rejects_bad_arguments(L):
    ws = L.uvit_op_maha_accumulate_ws_bytes(5, 64, 10)
    assert ws == 32 and L.uvit_op_maha_accumulate_ws_bytes(128, 768, 1000) == 512
    call = lambda p, B=5, Cd=64, K=10, nb=ws: L.uvit_op_maha_accumulate(*p, nb, B, Cd, K, NUL)      # noqa: E731
    assert call([P1] * 8, nb=ws - 1) == WORKSPACE
    for Cd, K in BAD_CK:
        assert L.uvit_op_maha_accumulate_ws_bytes(5, Cd, K) == SHAPE and call([P1] * 8, Cd=Cd, K=K) == SHAPE, (Cd, K)
    for B in BAD_B:
        assert L.uvit_op_maha_accumulate_ws_bytes(B, 64, 10) == SHAPE and call([P1] * 8, B=B) == SHAPE, B
    for i in range(8):                           # feat, labels, S, class_sum, total_sum, class_count, sums, ws
        a = [P1] * 8
        a[i] = NUL
        assert call(a) == ARG, i
        a[i] = off(2)                            # not aligned to a float, a double, an int64 or 16 bytes
        assert call(a) == ARG, i
    for i, n in ((1, 4), (2, 4), (3, 4), (4, 4), (5, 4), (6, 4), (7, 8)):      # 8-byte elements at a multiple of 4, the workspace at 8
        a = [P1] * 8
        a[i] = off(n)
        assert call(a) == ARG, (i, n)


def test_scores_rejects_bad_arguments(L):
    ws = L.uvit_op_maha_scores_ws_bytes(3, 64, 10)
    assert ws == (2 * 3 * 64 + 3 * 10) * 8 and L.uvit_op_maha_scores_ws_bytes(128, 768, 1000) == (2 * 128 * 768 + 128 * 1000) * 8

    def call(p, B=3, Cd=64, K=10, ld=10, nb=ws):      # p: feat, W, W0, Wmu, Wmu0, class_count, maha, rmaha, pred, dist, labels, correct, ws
        return L.uvit_op_maha_scores(*p[:10], ld, p[10], p[11], p[12], nb, B, Cd, K, NUL)

    assert call([P1] * 13, nb=ws - 1) == WORKSPACE
    for Cd, K in BAD_CK:
        assert L.uvit_op_maha_scores_ws_bytes(3, Cd, K) == SHAPE and call([P1] * 13, Cd=Cd, K=K, ld=max(K, 1)) == SHAPE, (Cd, K)
    for B in BAD_B:
        assert L.uvit_op_maha_scores_ws_bytes(B, 64, 10) == SHAPE and call([P1] * 13, B=B) == SHAPE, B
    assert call([P1] * 13, ld=9) == SHAPE
    nullable = (9, 10, 11)                       # dist, labels, correct
    for i in range(13):
        a = [P1] * 13
        a[i] = NUL
        if i in nullable:
            assert call(a, nb=ws - 1) == WORKSPACE, i        # accepted: the next check is reached
        else:
            assert call(a) == ARG, i
        a[i] = off(2)
        assert call(a) == ARG, i
    a = [P1] * 13
    a[9] = NUL
    assert call(a, ld=0, nb=ws - 1) == WORKSPACE             # without dist, ld is not looked at
    for i, n in ((1, 4), (2, 4), (3, 4), (4, 4), (5, 4), (9, 4), (10, 4), (12, 8)):
        a = [P1] * 13
        a[i] = off(n)
        assert call(a) == ARG, (i, n)


# ---- the module ----
def five_probes():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    return [LinearProbe, GPProbe, HetProbe, EnsembleProbe, LaplaceProbe]


def host_state(K=10, Cd=128, n=400, seed=2):
    """A density state built on the host from cluster features, as density_state_dict() returns it."""
    _, f, y = mr.clusters(K, Cd, n, seed=seed)
    S, cs, ts, cc, sums = mr.accumulate(f, y, K)
    return {"S": torch.from_numpy(S), "class_sum": torch.from_numpy(cs), "total_sum": torch.from_numpy(ts),
            "class_count": torch.from_numpy(cc), "sums": torch.from_numpy(sums), "shrinkage": 1e-3}


def test_detect_columns_of_all_five_classes():
    base = ("msp", "entropy", "energy")
    own = [(), ("gp_var",), ("het_var",), ("ens_total", "ens_aleatoric", "ens_mi", "ens_var", "ens_disagreement"), ("lap_var",)]
    for cls, cols in zip(five_probes(), own):
        assert cls.DETECT_COLUMNS == base + cols


def test_density_state_columns_and_round_trip():
    from uncertainty_vit_amd.linear_probe import MAHA_COLUMNS, LinearProbe
    from uncertainty_vit_amd.native import UvitError
    assert MAHA_COLUMNS == ("maha", "rmaha")
    sd = host_state()
    ref = mr.fit(*(sd[k].numpy() for k in ("S", "class_sum", "total_sum", "class_count", "sums")), 1e-3)
    for cls in five_probes():
        torch.manual_seed(3)
        probe = cls(tiny_encoder().eval(), 10)
        before, keys = probe.DETECT_COLUMNS, list(probe.state_dict())
        assert probe.density is None
        info = probe.set_density(sd)
        assert probe.DETECT_COLUMNS == before + MAHA_COLUMNS and "DETECT_COLUMNS" in probe.__dict__ and type(probe).DETECT_COLUMNS != probe.DETECT_COLUMNS
        assert len(probe.DETECT_COLUMNS) <= 16
        assert info == probe.density and (info["n"], info["skipped"], info["classes"], info["empty_classes"], info["shrinkage"]) == (400, 0, 10, 0, 1e-3)
        assert info["logdet"] == pytest.approx(ref["logdet"], rel=1e-9) and info["logdet0"] == pytest.approx(ref["logdet0"], rel=1e-9)
        st = probe._maha
        np.testing.assert_allclose(st["W"].numpy(), ref["W"], rtol=1e-7, atol=1e-9 * np.abs(ref["W"]).max())
        np.testing.assert_allclose(st["Wmu"].numpy(), ref["Wmu"], rtol=1e-7, atol=1e-9 * np.abs(ref["Wmu"]).max())
        assert bool((st["W"].triu(1) == 0).all()) and bool((st["W0"].triu(1) == 0).all())
        assert list(probe.state_dict()) == keys and not [n for n, _ in probe.named_buffers() if "maha" in n]      # neither parameter nor buffer
        # round trip, another shrinkage from the kept sums, and back
        again = probe.density_state_dict()
        assert set(again) == set(sd) and all(torch.equal(again[k], sd[k]) for k in sd if k != "shrinkage") and again["shrinkage"] == 1e-3
        looser = probe.set_density_shrinkage(1e-1)
        assert looser["shrinkage"] == 1e-1 and looser["logdet"] > info["logdet"] and probe.density_state_dict()["shrinkage"] == 1e-1
        assert probe.load_density_state(again) == info
        moved = probe.float()                                  # _apply keeps the density, in float64
        assert moved.density == info and moved._maha["W"].dtype == torch.float64 and np.array_equal(moved._maha["W"].numpy(), st["W"].numpy())
        probe.set_density(None)
        assert probe.density is None and probe.DETECT_COLUMNS == before
        if cls is LinearProbe:
            assert "DETECT_COLUMNS" not in probe.__dict__
        # refusals
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(UvitError):
                probe.load_density_state({**sd, "shrinkage": bad})
        with pytest.raises(UvitError):
            probe.load_density_state({"S": sd["S"]})
        with pytest.raises(UvitError):
            probe.load_density_state(host_state(K=9))          # another K
        with pytest.raises(UvitError):
            probe.load_density_state(host_state(Cd=64))        # another C
        with pytest.raises(UvitError):
            probe.load_density_state({**sd, "sums": torch.tensor([1.0, 399.0])})      # fewer than two rows used
        with pytest.raises(UvitError):
            probe.load_density_state({**sd, "S": torch.zeros(128, 128, dtype=torch.float64)})      # not positive definite
        assert probe.density is None
        for call in (probe.density_state_dict, lambda: probe.set_density_shrinkage(1e-2), lambda: probe.feature_scores(torch.zeros(2, 3, 48, 48)),
                     lambda: probe.fit_density([], shrinkage=0.0), lambda: probe.fit_density([]),
                     lambda: probe.fit_density([(torch.zeros(2, 3, 48, 48), torch.zeros(2, dtype=torch.int64))])):
            with pytest.raises(UvitError):
                call()
        probe.set_density(sd)
        for call in (lambda: probe.feature_scores(torch.zeros(2, 3, 48, 48)), lambda: probe.density_batch(torch.zeros(2, 128))):
            with pytest.raises(UvitError):                     # no CPU fallback
                call()


def test_density_and_laplace_columns_compose_in_both_orders():
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    base, sd = LinearProbe.DETECT_COLUMNS, host_state()
    lap_state = {"info": {"n": 3, "n_skipped": 0, "nll": 1.0, "prior_precision": 1.0, "log_marglik": -2.0, "on_grid_edge": False}}

    def set_lap(probe, on):                      # a Laplace fit installed by hand: the kernels of a real one need a GPU
        if on:
            probe._lap = dict(lap_state)
            probe._det_refresh()
        else:
            probe.set_laplace(None)

    probe = LaplaceProbe(tiny_encoder().eval(), 10)
    assert probe.DETECT_COLUMNS == base
    set_lap(probe, True)
    assert probe.DETECT_COLUMNS == base + ("lap_var",)
    probe.set_density(sd)
    assert probe.DETECT_COLUMNS == base + ("lap_var", "maha", "rmaha")
    set_lap(probe, False)
    assert probe.DETECT_COLUMNS == base + ("maha", "rmaha") and probe.density is not None
    set_lap(probe, True)
    assert probe.DETECT_COLUMNS == base + ("lap_var", "maha", "rmaha")
    probe.set_density(None)
    assert probe.DETECT_COLUMNS == base + ("lap_var",) and "DETECT_COLUMNS" not in probe.__dict__
    set_lap(probe, False)
    assert probe.DETECT_COLUMNS == base
    probe.set_density(sd)
    assert probe.DETECT_COLUMNS == base + ("maha", "rmaha")
    probe.load_state_dict(probe.state_dict())    # drops a Laplace fit, keeps the density: it does not depend on the head
    assert probe.DETECT_COLUMNS == base + ("maha", "rmaha")
    probe.set_density(None)
    assert probe.DETECT_COLUMNS == base and LaplaceProbe.DETECT_COLUMNS == base + ("lap_var",)


# ---- the command line ----
def test_cli_flags_are_absent_unless_given():
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()
    assert not [k for k in vars(rlp.get_args([])) if k.startswith("maha")]
    assert rlp.check_maha_flags(rlp.get_args([])) is None and rlp.check_maha_flags(rlp.get_args(["--eval"])) is None
    a = rlp.get_args(["--eval", "--maha_data_path", "d"])
    assert a.maha_data_path == "d" and not hasattr(a, "maha_shrinkage") and rlp.check_maha_flags(a) == "fit"
    a = rlp.get_args(["--eval", "--maha_state", "s.pth", "--maha_shrinkage", "0.01"])
    assert a.maha_shrinkage == 0.01 and rlp.check_maha_flags(a) == "state"
    for head in ("--gp_layer", "--het_layer", "--ensembles", "--laplace"):
        assert rlp.check_maha_flags(rlp.get_args(["--eval", head, "--maha_data_path", "d"])) == "fit"


def test_cli_refuses_what_does_not_go_together():
    import run_linear_probe as rlp
    for argv in (["--maha_data_path", "d"], ["--maha_state", "s.pth"], ["--maha_shrinkage", "0.1"],                # all three need --eval
                 ["--eval", "--maha_shrinkage", "0.1"],                                                           # the shrinkage alone
                 ["--eval", "--maha_data_path", "d", "--maha_state", "s.pth"],                                    # two sources
                 ["--eval", "--maha_data_path", "d", "--maha_shrinkage", "0"], ["--eval", "--maha_data_path", "d", "--maha_shrinkage", "-1"],
                 ["--eval", "--maha_data_path", "d", "--maha_shrinkage", "nan"], ["--eval", "--maha_state", "s", "--maha_shrinkage", "inf"]):
        with pytest.raises(ValueError):
            rlp.check_maha_flags(rlp.get_args(argv))


def test_cli_lines_and_log_entries():
    import run_linear_probe as rlp
    fit = {"n": 240, "skipped": 2, "classes": 10, "empty_classes": 1, "shrinkage": 1e-3, "logdet": -123.456789, "logdet0": -45.5}
    stats = {"maha_acc1": 87.5, "maha_mean": 130.25}
    assert rlp.maha_lines(fit, stats) == [
        "* Mahalanobis fit on 240 images (2 skipped), 10 classes (1 empty), shrinkage 0.001, log-det -123.45679 background -45.50000",
        "* Mahalanobis Acc@1 87.500 mean 130.25000"]
    assert rlp.maha_log_entries(fit, stats) == {"test_maha_acc1": 87.5, "test_maha_mean": 130.25, "test_maha_shrinkage": 1e-3}
