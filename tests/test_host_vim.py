"""CPU: the ViM score's host-side pieces -- the float64 restatement (tests/vim_ref.py) against a brute-force projector, the meaning of
the scores on the hand-made case, the argument checks of the uvit_op_vim_* entry points (they return before anything touches a
device), the ViM state of the five probe classes, their detection columns and their head rule, and the command line's new flags."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import maha_ref as mr
import vim_ref as vr
from test_host_knn import density_state, five_probes, host_state as bank_state
from test_host_probe import tiny_encoder


# ---- the restatement ----
@pytest.mark.parametrize("shape", vr.SHAPES[:4])
def test_restatement_is_the_brute_force_projector(shape):
    """residual through A = [R ; W], a = [-R o ; b] equals |(I - P P^T)(f - o)| with P the D principal eigenvectors, and the logits
    behind it are W f + b; R has orthonormal rows, and o is where the head's logits are closest to zero."""
    B, Cd, Cn, K = shape
    c = vr.make_case(*shape)
    ft = c["fit"]
    ref = vr.scores(c["feat"], ft["A"], ft["a"], Cn, ft["alpha"])
    S, t, n = vr.moments(*c["fit_set"], K)
    M = (S - np.outer(ft["origin"], t) - np.outer(t, ft["origin"]) + n * np.outer(ft["origin"], ft["origin"])) / n
    lam, V = np.linalg.eigh(0.5 * (M + M.T))
    res, vim = vr.scores_brute_force(c["feat"], c["W"], c["b"], ft["origin"], V[:, Cn:], ft["alpha"])
    scale = np.abs(c["feat"].astype(np.float64) - ft["origin"]).max() * Cd
    assert np.abs(res - ref["residual"]).max() <= 1e-12 * scale and np.abs(vim - ref["vim"]).max() <= 1e-12 * scale * max(1.0, abs(ft["alpha"]))
    assert np.abs(ft["R"] @ ft["R"].T - np.eye(Cn)).max() <= 1e-12 and ft["dim"] == Cd - Cn and 0.0 < ft["explained"] <= 1.0
    assert np.abs(c["W"].T @ (c["W"] @ ft["origin"] + c["b"])).max() <= 1e-9          # the normal equations of min |W o + b|
    assert np.array_equal(ref["pred"], (c["feat"].astype(np.float64) @ c["W"].T + c["b"]).argmax(1))


@pytest.mark.parametrize("shape", vr.SHAPES)
def test_gpu_cases_are_what_their_test_assumes(shape):
    """On the shapes the GPU test uses: every row's arg max is decided (its two largest logits differ by more than their bounds), the
    fit's alpha is positive and finite, and the bounds are small against the values."""
    B, Cd, Cn, K = shape
    c = vr.make_case(*shape)
    ft = c["fit"]
    ref = vr.scores(c["feat"], ft["A"], ft["a"], Cn, ft["alpha"])
    bd = vr.bounds(c["feat"], ft["A"], ft["a"], Cn, ft["alpha"], ref)
    assert bd["decided"].all() and 0.0 < ft["alpha"] < np.inf
    assert (bd["residual"] <= 1e-6 * np.maximum(ref["residual"], 1e-3)).all() and (bd["vim"] <= 1e-6 * np.maximum(np.abs(ref["vim"]), 1.0)).all()


def test_default_dim_is_the_papers():
    from uncertainty_vit_amd.probe_vim import vim_default_dim
    for Cd, want in ((2048, 1000), (1024, 512), (768, 512), (764, 382), (128, 64), (4, 2)):
        assert vr.default_dim(Cd) == vim_default_dim(Cd) == want


def test_meaning_of_the_scores_on_the_hand_made_case():
    """Held-out rows against rows shifted off the principal space (same logits) and rows inside it with flat logits: residual and vim
    rank the first kind perfectly, vim the second; energy misses the first and residual the second (printed, not asserted)."""
    K, Cd, D, (W, b), (f_fit, y_fit), f_in, f_shift, f_flat = vr.meaning_case(0)
    ft = vr.fit(*vr.moments(f_fit, y_fit, K), W, b, D)
    alpha = vr.alpha_of(vr.scores(f_fit, ft["A"], ft["a"], Cd - D))[0]
    s_in, s_shift, s_flat = (vr.scores(f, ft["A"], ft["a"], Cd - D, alpha) for f in (f_in, f_shift, f_flat))
    got = {("residual", "shifted"): mr.auroc(s_in["residual"], s_shift["residual"]), ("vim", "shifted"): mr.auroc(s_in["vim"], s_shift["vim"]),
           ("vim", "flat"): mr.auroc(s_in["vim"], s_flat["vim"])}
    print(f"\nalpha {alpha:.4f}, explained {ft['explained']:.5f}; AUROC {got}")
    print(f"energy on the shifted rows {mr.auroc(vr.energy(f_in, W, b), vr.energy(f_shift, W, b)):.3f}, "
          f"residual on the flat rows {mr.auroc(s_in['residual'], s_flat['residual']):.3f}")
    assert all(v == 1.0 for v in got.values()), got


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any aligned non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE, WORKSPACE = -1, -2, -4
SYMBOLS = ("uvit_op_vim_scores_ws_bytes", "uvit_op_vim_scores", "uvit_op_maha_accumulate_ws_bytes", "uvit_op_maha_accumulate")      # the fit's four


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


def test_ws_bytes_and_its_refusals(L):
    assert L.uvit_op_vim_scores_ws_bytes(128, 768, 256, 1000) == (128 * 1256 + 2 * 128) * 8
    assert L.uvit_op_vim_scores_ws_bytes(1, 4, 1, 2) == 48 and L.uvit_op_vim_scores_ws_bytes(1, 4, 3, 2) == 64      # padded to 16 bytes
    assert L.uvit_op_vim_scores_ws_bytes(65535, 2048, 2047, 4096) == (65535 * (2047 + 4096) + 2 * 65535) * 8 + 8
    for bad in ((0, 8, 4, 3), (65536, 8, 4, 3), (5, 0, 1, 3), (5, 6, 3, 3), (5, 2052, 4, 3), (5, 8, 0, 3), (5, 8, 8, 3), (5, 8, -1, 3), (5, 8, 4, 1),
                (5, 8, 4, 4097)):
        assert L.uvit_op_vim_scores_ws_bytes(*bad) == SHAPE, bad


def test_scores_rejects_bad_arguments(L):
    ws = L.uvit_op_vim_scores_ws_bytes(5, 8, 4, 3)

    def call(p, B=5, Cd=8, Cn=4, K=3, alpha=1.5, nb=ws):      # p: feat, A, a, vim, residual, pred, labels, correct, sums, ws
        return L.uvit_op_vim_scores(p[0], p[1], p[2], C.c_double(alpha), *p[3:10], nb, B, Cd, Cn, K, NUL)

    assert call([P1] * 10, nb=ws - 1) == WORKSPACE
    for kw in ({"B": 0}, {"B": 65536}, {"Cd": 0}, {"Cd": 6}, {"Cd": 2052}, {"Cn": 0}, {"Cn": 8}, {"Cn": -1}, {"K": 1}, {"K": 4097}):
        assert call([P1] * 10, **kw) == SHAPE, kw
    for alpha in (float("nan"), float("inf"), -float("inf")):
        assert call([P1] * 10, alpha=alpha) == ARG, alpha
    for i in (0, 1, 2, 3, 4, 5, 9):                                            # the seven that are not nullable
        a = [P1] * 10
        a[i] = NUL
        assert call(a) == ARG, i
    for i, n in ((0, 2), (1, 4), (2, 4), (3, 2), (4, 2), (5, 2), (6, 4), (7, 2), (8, 4), (9, 8)):      # floats, doubles, int32, int64, 16 bytes
        a = [P1] * 10
        a[i] = off(n)
        assert call(a) == ARG, (i, n)
    a = [P1] * 6 + [NUL] * 3 + [P1]
    assert call(a, Cd=6) == SHAPE and call(a, nb=0) == WORKSPACE               # the nullable ones are accepted: the next checks are reached
    assert call([P1] * 10, alpha=float("nan"), Cd=6) == ARG                   # the pointers and alpha come first


# ---- the module ----
def vim_state(K=10, Cd=128, n=300, dim=40, seed=2):
    """A ViM state built on the host from cluster features, as vim_state_dict() returns it."""
    _, f, y = mr.clusters(K, Cd, n, seed=seed)
    W, b = vr.make_head(K, Cd, seed)
    ft = vr.fit(*vr.moments(f, y, K), W, b, dim)
    alpha, sm, sr, used, skipped = vr.alpha_of(vr.scores(f, ft["A"], ft["a"], Cd - dim))
    t = torch.from_numpy
    return {"R": t(ft["R"]), "origin": t(ft["origin"]), "weight": t(W), "bias": t(b), "alpha": alpha, "dim": dim,
            "eigenvalues": t(ft["eigenvalues"]), "sums": torch.tensor([sm, sr, used, skipped], dtype=torch.float64)}, ft


def test_vim_state_columns_and_round_trip():
    from uncertainty_vit_amd.linear_probe import KNN_COLUMNS, MAHA_COLUMNS, VIM_COLUMNS, LinearProbe
    from uncertainty_vit_amd.native import UvitError
    assert VIM_COLUMNS == ("vim", "residual")
    (sd, ft), dens, bank = vim_state(), density_state(), bank_state()
    for cls in five_probes():
        torch.manual_seed(3)
        probe = cls(tiny_encoder().eval(), 10)
        before, keys = probe.DETECT_COLUMNS, list(probe.state_dict())
        assert probe.vim is None and probe._vim is None and probe._scores == (probe._density, probe._bank, probe._vim_score)
        info = probe.set_vim(sd)
        assert info == probe.vim == {"n": 300, "skipped": 0, "classes": 10, "dim": 40, "alpha": sd["alpha"], "explained": ft["explained"]}
        assert probe.DETECT_COLUMNS == before + VIM_COLUMNS and "DETECT_COLUMNS" in probe.__dict__
        assert list(probe.state_dict()) == keys and not [n for n, _ in probe.named_buffers() if "vim" in n]      # neither parameter nor buffer
        # the stacked matrix is the restatement's bit for bit, the vector up to the order of the 128 products of -R o
        assert probe._vim["A"].dtype == torch.float64 and np.array_equal(probe._vim["A"].numpy(), ft["A"])
        assert np.abs(probe._vim["a"].numpy() - ft["a"]).max() <= 2 * vr.gamma(128) * np.abs(ft["R"]).max() * np.abs(ft["origin"]).sum()
        # beside a density and a bank: behind both, in every order of setting and clearing; thirteen columns at most
        switch = {"maha": lambda on: probe.set_density(dens if on else None), "knn": lambda on: probe.set_neighbours(bank if on else None),
                  "vim": lambda on: probe.set_vim(sd if on else None)}
        cols = {"maha": MAHA_COLUMNS, "knn": KNN_COLUMNS, "vim": VIM_COLUMNS}
        probe.set_vim(None)
        for on_order in itertools.permutations(switch):
            for off_order in itertools.permutations(switch):
                have = set()
                assert probe.DETECT_COLUMNS == before
                for name, on in [(n, True) for n in on_order] + [(n, False) for n in off_order]:
                    switch[name](on)
                    have = have | {name} if on else have - {name}
                    assert probe.DETECT_COLUMNS == before + tuple(c for n in ("maha", "knn", "vim") if n in have for c in cols[n]), (on_order, off_order, name)
                    assert len(probe.DETECT_COLUMNS) <= 13
        if cls is LinearProbe:
            assert "DETECT_COLUMNS" not in probe.__dict__
        # round trip; load_state_dict and _apply keep the state, in float64
        probe.set_vim(sd)
        again = probe.vim_state_dict()
        assert set(again) == set(sd) and all(torch.equal(again[k], sd[k]) and again[k].dtype == torch.float64 for k in sd if torch.is_tensor(sd[k]))
        assert (again["alpha"], again["dim"]) == (sd["alpha"], 40) and probe.load_vim_state(again) == info
        probe.load_state_dict(probe.state_dict())
        moved = probe.float()
        assert moved.vim == info and moved._vim["A"].dtype == torch.float64 and np.array_equal(moved._vim["A"].numpy(), ft["A"])
        # refusals: another C, another K, a dim that does not fit R, a non-finite alpha, short sums, a missing key
        other_c, other_k = vim_state(Cd=64, dim=20)[0], vim_state(K=7)[0]
        for bad in (other_c, other_k, {**sd, "dim": 41}, {**sd, "dim": 0}, {**sd, "dim": 128}, {**sd, "dim": 2.5}, {**sd, "alpha": float("nan")},
                    {**sd, "alpha": float("inf")}, {**sd, "sums": torch.zeros(2)}, {**sd, "R": sd["R"][:-1]}, {**sd, "origin": sd["origin"][:-1]},
                    {**sd, "eigenvalues": sd["eigenvalues"][:-1]}, {**sd, "bias": sd["bias"][:-1]}, {k: v for k, v in sd.items() if k != "R"}, "x"):
            with pytest.raises(UvitError):
                probe.load_vim_state(bad)
        assert probe.vim == info                                               # a refused state leaves the one in use
        for call in (lambda: probe.vim_scores(torch.zeros(2, 3, 48, 48)), lambda: probe.vim_batch(torch.zeros(2, 128))):
            with pytest.raises(UvitError):                                     # no CPU fallback
                call()
        probe.set_vim(None)
        assert probe.vim is None and probe.DETECT_COLUMNS == before
        for call in (probe.vim_state_dict, lambda: probe.vim_scores(torch.zeros(2, 3, 48, 48)), lambda: probe.vim_batch(torch.zeros(2, 128)),
                     lambda: probe.fit_vim([], head=(sd["weight"], sd["bias"])), lambda: probe.fit_vim([], dim=0, head=(sd["weight"], sd["bias"])),
                     lambda: probe.fit_vim([], dim=128, head=(sd["weight"], sd["bias"])),
                     lambda: probe.fit_vim([], head=(sd["weight"][:, :64], sd["bias"])),
                     lambda: probe.fit_vim([], head=(sd["weight"], sd["bias"]), moments={"S": torch.zeros(64, 64), "total_sum": torch.zeros(64), "sums": torch.zeros(2)}),
                     lambda: probe.fit_vim([(torch.zeros(2, 3, 48, 48), torch.zeros(2, dtype=torch.int64))], head=(sd["weight"], sd["bias"]))):
            with pytest.raises(UvitError):
                call()


def test_head_rule_per_class():
    """LinearProbe and LaplaceProbe: their own weight and bias; EnsembleProbe: the members' mean with combine="logits"; combine="probs",
    GPProbe and HetProbe raise and point to head=(W, b)."""
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    enc = tiny_encoder().eval()
    for cls in (LinearProbe, LaplaceProbe):
        probe = cls(enc, 10, init_scale=5.0)
        probe.head.bias.data.normal_()
        W, b = probe._vim_score.head(None)
        assert W.dtype == b.dtype == torch.float64 and torch.equal(W, probe.head.weight.detach().double()) and torch.equal(b, probe.head.bias.detach().double())
        probe.head.weight.data.add_(1.0)
        assert not torch.equal(W, probe.head.weight.detach().double())         # a snapshot, not a view
    ens = EnsembleProbe(enc, 10, members=3, init_scale=5.0)
    W, b = ens._vim_score.head(None)
    ws = torch.stack([getattr(ens.heads, str(m)).weight.detach().double() for m in range(3)])
    assert tuple(W.shape) == (10, 128) and torch.equal(W, ws.mean(0)) and torch.equal(b, torch.zeros(10, dtype=torch.float64))
    given = (torch.ones(10, 128), torch.arange(10.0))
    for probe in (EnsembleProbe(enc, 10, members=3, combine="probs"), GPProbe(enc, 10, num_inducing=64), HetProbe(enc, 10, num_factors=4)):
        with pytest.raises(UvitError, match=r"not affine in the feature.*head=\(W, b\)"):
            probe._vim_score.head(None)
        with pytest.raises(UvitError, match=r"not affine in the feature.*head=\(W, b\)"):
            probe.fit_vim([])
        W, b = probe._vim_score.head(given)                                    # an explicit head is taken by every class
        assert W.dtype == torch.float64 and torch.equal(W, given[0].double()) and torch.equal(b, given[1].double())
    for bad in ((torch.ones(9, 128), torch.zeros(10)), (torch.ones(10, 128), torch.zeros(9)), (torch.full((10, 128), float("nan")), torch.zeros(10))):
        with pytest.raises(UvitError):
            ens._vim_score.head(bad)


# ---- the command line ----
def test_cli_flags_are_absent_unless_given():
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()
    assert not [k for k in vars(rlp.get_args([])) if k.startswith("vim")]
    assert rlp.check_vim_flags(rlp.get_args([])) is None and rlp.check_vim_flags(rlp.get_args(["--eval"])) is None
    a = rlp.get_args(["--eval", "--vim_data_path", "d"])
    assert a.vim_data_path == "d" and not hasattr(a, "vim_dim") and rlp.check_vim_flags(a) == "fit"
    a = rlp.get_args(["--eval", "--vim_data_path", "d", "--vim_dim", "200"])
    assert a.vim_dim == 200 and rlp.check_vim_flags(a) == "fit"
    assert rlp.check_vim_flags(rlp.get_args(["--eval", "--vim_state", "s.pth"])) == "state"
    for head in (["--laplace"], ["--ensembles"], ["--ensembles", "--ens_combine", "logits"]):
        assert rlp.check_vim_flags(rlp.get_args(["--eval", *head, "--vim_data_path", "d", "--maha_data_path", "d", "--knn_data_path", "k"])) == "fit"


def test_cli_refuses_what_does_not_go_together():
    import run_linear_probe as rlp
    for argv in (["--vim_data_path", "d"], ["--vim_state", "s.pth"], ["--vim_dim", "5"],                                 # all three need --eval
                 ["--eval", "--vim_data_path", "d", "--vim_state", "s.pth"],                                           # two sources
                 ["--eval", "--vim_dim", "5"], ["--eval", "--vim_state", "s", "--vim_dim", "5"],                       # the dim belongs to a fit
                 ["--eval", "--vim_data_path", "d", "--vim_dim", "0"], ["--eval", "--vim_data_path", "d", "--vim_dim", "-3"],
                 ["--eval", "--gp_layer", "--vim_data_path", "d"], ["--eval", "--het_layer", "--vim_state", "s"],
                 ["--eval", "--ensembles", "--ens_combine", "probs", "--vim_data_path", "d"]):
        with pytest.raises(ValueError):
            rlp.check_vim_flags(rlp.get_args(argv))


def test_cli_lines_and_log_entries():
    import run_linear_probe as rlp
    fit = {"n": 240, "skipped": 2, "classes": 10, "dim": 64, "alpha": 1.25, "explained": 0.96875}
    stats = {"vim_acc1": 87.5, "vim_mean": -3.125}
    assert rlp.vim_lines(fit, stats, 128) == ["* ViM fit on 240 images (2 skipped), dim 64 of 128, alpha 1.25000, explained 0.96875",
                                              "* ViM Acc@1 87.500 mean -3.12500"]
    assert rlp.vim_log_entries(fit, stats) == {"test_vim_acc1": 87.5, "test_vim_mean": -3.125, "test_vim_dim": 64, "test_vim_alpha": 1.25}
