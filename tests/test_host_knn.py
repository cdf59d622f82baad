"""CPU: the k-nearest-neighbour score's host-side pieces -- the float64 restatement (tests/knn_ref.py) against a brute-force argsort,
its bf16 rounding against torch's, the meaning of the scores on the synthetic clusters, the argument checks of the uvit_op_knn_*
entry points (they return before anything touches a device), the neighbour state of the five probe classes and their detection
columns, and the command line's new flags."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_ref as kr
import maha_ref as mr
from test_host_probe import tiny_encoder


# ---- the restatement ----
def test_bf16_rounding_is_torch_bfloat16():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 10.0 ** rng.integers(-6, 6, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895314e38, np.inf, -np.inf, 1e-40], dtype=np.float32)])
    want = torch.from_numpy(x).bfloat16()
    got = kr.bf16_round(x)
    assert got.tobytes() == want.float().numpy().tobytes()
    assert kr.bf16_bits(got).tobytes() == want.view(torch.int16).numpy().tobytes()
    assert kr.from_bf16_bits(kr.bf16_bits(got)).tobytes() == got.tobytes()
    assert np.isnan(kr.bf16_round(np.array([np.nan], dtype=np.float32))).all()


def test_rows_of_the_restatement():
    """Unit rows: the two accepted values differ in at most a few elements and by one bf16 step; the norm of the result is 1 to bf16
    precision; bad rows are zero rows labelled -1 and counted."""
    rng = np.random.default_rng(1)
    f = rng.standard_normal((9, 96)).astype(np.float32) * 3
    y = np.array([0, 1, 2, -1, 3, 4, 1, 0, 2])
    f[5, 7], f[6, 0], f[7] = np.nan, np.inf, 0.0
    lo, hi, lab, sums = kr.rows(f, y, 4)
    assert lab.tolist() == [0, 1, 2, -1, 3, -1, -1, -1, 2] and sums.tolist() == [5, 4]
    assert not lo[[3, 5, 6, 7]].any() and not hi[[3, 5, 6, 7]].any()
    assert (lo != hi).mean() < 0.01 and np.all(hi >= lo) and np.all(np.abs(hi - lo) <= np.abs(lo) * 2.0 ** -7)
    norms = np.sqrt((lo[[0, 1, 2, 4, 8]].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(norms - 1).max() < 2.0 ** -8
    assert kr.rows(f[:3])[2].tolist() == [0, 0, 0]                             # without labels a usable row gets 0


@pytest.mark.parametrize("case", ["random", "clustered", "ties"])
def test_search_is_the_brute_force_argsort(case):
    if case == "random":
        c, k = kr.search_case(17, 96, 127, 5), 5
    elif case == "clustered":
        c, k = kr.clustered_case(), 20
    else:                                                                      # whole-number rows: many exactly equal similarities
        rng = np.random.default_rng(4)
        bank = rng.integers(-2, 3, (60, 32)).astype(np.float32)
        c = {"q": bank[:8].copy(), "valid": np.zeros(8, dtype=np.int32), "bank": bank, "labels": np.where(np.arange(60) % 5 == 2, -1, 0).astype(np.int32)}
        k = 64
    c["valid"][min(3, len(c["valid"]) - 1)] = -1
    sim, idx = kr.search(c["q"], c["valid"], c["bank"], c["labels"], k)
    bsim, bidx = kr.search_brute_force(c["q"], c["valid"], c["bank"], c["labels"], k)
    assert np.array_equal(idx, bidx) and np.array_equal(sim, bsim, equal_nan=True)
    assert np.isnan(sim[min(3, len(sim) - 1)]).all()
    if case == "ties":
        assert np.isneginf(sim[0, 48:]).all() and (idx[0, 48:] == -1).all() and (np.diff(sim[0, :48]) == 0).sum() > 10


@pytest.mark.parametrize("shape", kr.SHAPES)
def test_gpu_cases_are_what_their_test_assumes(shape):
    """On the shapes the GPU test uses: every query whose own bank row is live finds it first (so does the restatement, which also breaks
    the tie with its duplicate towards the lower index), dead rows never appear, k > live rows leaves a tail, and the k-NN vote of every row is
    decided (its two largest votes differ by more than their bounds)."""
    B, Cd, N, k = shape
    c = kr.search_case(*shape)
    sim, idx = kr.search(c["q"], c["valid"], c["bank"], c["labels"], k)
    own = c["first"] >= 0
    assert np.array_equal(idx[own, 0], c["first"][own]) and own.sum() >= min(B, 3) - 1 + (B == 1)
    live = int((c["labels"] >= 0).sum())
    assert (idx[:, min(k, live):] == -1).all() and (c["labels"][idx[:, :min(k, live)]] >= 0).all()
    if shape == (5, 32, 9, 9):
        assert live == 8 and np.isneginf(sim[:, 8]).all()
    if N >= 9 and B > 1:
        assert idx[1, 1] == N - 2 and sim[1, 0] == sim[1, 1]                   # the duplicate of row 1 follows it
    if live >= k:
        _, _, pred, decided = kr.votes(sim.astype(np.float32), idx, c["labels"], c["K"], 0.07)
        assert decided.all() and (pred >= 0).all()


def test_scores_of_the_restatement():
    sim, idx, lab, K, T, want = kr.scores_cases()
    v, bound, pred, decided = kr.votes(sim, idx, lab, K, T)
    assert pred.tolist() == want and v[0, 1] == v[0, 2] and v[0, 0] == 0 and np.isnan(v[2:]).all()
    assert not decided[0] and decided[1]                                       # the tie is exact, by construction
    assert v[1, 0] == 1.0 and v[1, 1] == pytest.approx(3 * np.exp(-0.25 / 0.07), rel=1e-14)
    knn = kr.knn_score(sim[:, -1])
    assert knn[:2].tolist() == [1.5, 1.0] and np.isnan(knn[2:]).all() and knn.dtype == np.float32


def test_meaning_of_the_scores_on_the_synthetic_set():
    """Held-out cluster rows against normalised noise, the bank = the 240 fit rows: OOD AUROC 1.0 for knn and k-NN accuracy 1.0 for
    k in {1, 5, 20}."""
    K, Cd, (f_fit, y_fit), (f_in, y_in), f_out = mr.meaning_case(0)
    bank, q_in, q_out = (kr.unit_bf16(kr.meaning_rows(x)) for x in (f_fit, f_in, f_out))
    lab = y_fit.astype(np.int32)
    for k in (1, 5, 20):
        s_in, i_in = kr.search(q_in, np.zeros(60), bank, lab, k)
        s_out, _ = kr.search(q_out, np.zeros(60), bank, lab, k)
        a = kr.auroc(kr.knn_score(s_in[:, -1].astype(np.float32)), kr.knn_score(s_out[:, -1].astype(np.float32)))
        _, _, pred, decided = kr.votes(s_in.astype(np.float32), i_in, lab, K, 0.07)
        print(f"k {k}: OOD AUROC {a}, k-NN accuracy {(pred == y_in).mean()}, decided {decided.mean()}")
        assert a == 1.0 and bool((pred == y_in).all()) and decided.all()


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any aligned non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE, WORKSPACE = -1, -2, -4
SYMBOLS = ("uvit_op_knn_rows", "uvit_op_knn_search_ws_bytes", "uvit_op_knn_search", "uvit_op_knn_scores")


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


def test_rows_rejects_bad_arguments(L):
    call = lambda p, B=5, Cd=64, K=10: L.uvit_op_knn_rows(*p, B, Cd, K, NUL)      # noqa: E731   p: feat, labels, out, out_labels, sums
    for Cd in (0, 16, 48, 2080):
        assert call([P1] * 5, Cd=Cd) == SHAPE, Cd
    for B in (0, (1 << 22) + 1):
        assert call([P1] * 5, B=B) == SHAPE, B
    for K in (1, 4097):
        assert call([P1] * 5, K=K) == SHAPE, K
    for i in (0, 2, 3):
        a = [P1] * 5
        a[i] = NUL
        assert call(a) == ARG, i
    for i, n in ((0, 2), (1, 4), (2, 8), (3, 2), (4, 4)):                       # a float, an int64, 16 bytes, an int32, a double
        a = [P1] * 5
        a[i] = off(n)
        assert call(a) == ARG, (i, n)
    a = [P1, NUL, P1, P1, NUL]
    assert call(a, Cd=40) == SHAPE and call(a, K=0, Cd=40) == SHAPE             # the nullable ones are accepted: the next check is reached


def test_search_rejects_bad_arguments(L):
    ws = L.uvit_op_knn_search_ws_bytes(5, 64, 100, 3, 7)
    assert ws == (5 * 7 * 3 * 8 + 15) // 16 * 16 and L.uvit_op_knn_search_ws_bytes(128, 768, 1 << 20, 20, 128) == 128 * 128 * 20 * 8
    auto = L.uvit_op_knn_search_ws_bytes(128, 768, 1 << 20, 20, 0)
    assert auto > 0 and auto % (128 * 20 * 8) == 0 and auto // (128 * 20 * 8) <= 1024      # O(B slabs k), never (B, N)
    assert L.uvit_op_knn_search_ws_bytes(3, 64, 500, 4, 0) == 3 * 1 * 4 * 8                  # at least 1024 bank rows per slab

    def call(p, B=5, Cd=64, N=100, k=3, slabs=7, ld=3, nb=ws):      # p: query, query_valid, bank, bank_labels, sim, idx, ws
        return L.uvit_op_knn_search(*p[:6], ld, p[6], nb, B, Cd, N, k, slabs, NUL)

    assert call([P1] * 7, nb=ws - 1) == WORKSPACE
    for kw in ({"B": 0}, {"B": 65536}, {"Cd": 48}, {"Cd": 0}, {"Cd": 2080}, {"N": 0}, {"N": (1 << 22) + 1}, {"k": 0}, {"k": 257, "ld": 257},
               {"slabs": -1}, {"slabs": 1025}, {"ld": 2}):
        assert call([P1] * 7, **kw) == SHAPE, kw
        kw.pop("ld", None)
        if kw:
            assert L.uvit_op_knn_search_ws_bytes(*(kw.get(n, d) for n, d in (("B", 5), ("Cd", 64), ("N", 100), ("k", 3), ("slabs", 7)))) == SHAPE, kw
    for i in range(7):
        a = [P1] * 7
        a[i] = NUL
        assert call(a) == ARG, i
        a[i] = off(2)
        assert call(a) == ARG, i
    for i in (0, 2, 6):                                                        # query, bank and workspace at 16 bytes
        a = [P1] * 7
        a[i] = off(8)
        assert call(a) == ARG, i


def test_scores_rejects_bad_arguments(L):
    def call(p, B=5, N=100, k=3, K=10, ld=3, ldv=10, T=0.07):      # p: sim, idx, bank_labels, knn, pred, votes, labels, correct
        return L.uvit_op_knn_scores(p[0], p[1], ld, p[2], N, p[3], p[4], p[5], ldv, p[6], p[7], B, k, K, C.c_double(T), NUL)

    for kw in ({"B": 0}, {"B": 65536}, {"N": 0}, {"k": 0}, {"k": 257, "ld": 257}, {"K": 1}, {"K": 4097, "ldv": 4097}, {"ld": 2}, {"ldv": 9}):
        assert call([P1] * 8, **kw) == SHAPE, kw
    for T in (0.0, -1.0, float("nan"), float("inf")):
        assert call([P1] * 8, T=T) == ARG, T
    for i in range(5):
        a = [P1] * 8
        a[i] = NUL
        assert call(a) == ARG, i
    for i, n in ((0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (5, 4), (6, 4), (7, 2)):
        a = [P1] * 8
        a[i] = off(n)
        assert call(a) == ARG, (i, n)
    a = [P1] * 5 + [NUL] * 3
    assert call(a, ldv=0, K=1) == SHAPE                                        # the nullable ones are accepted, ldv is not looked at


# ---- the module ----
def five_probes():
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.het_probe import HetProbe
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    return [LinearProbe, GPProbe, HetProbe, EnsembleProbe, LaplaceProbe]


def host_state(K=10, Cd=128, n=60, seed=2, k=5, skipped=2):
    """A neighbour state built on the host from cluster features, as neighbour_state_dict() returns it."""
    _, f, y = mr.clusters(K, Cd, n, seed=seed)
    y = y.copy()
    y[:skipped] = -1
    lo, _, lab, sums = kr.rows(f, y, K)
    return {"bank": torch.from_numpy(kr.bf16_bits(lo)).view(torch.bfloat16), "labels": torch.from_numpy(lab), "sums": torch.from_numpy(sums),
            "k": k, "temperature": 0.07}


def density_state(K=10, Cd=128, n=400):
    _, f, y = mr.clusters(K, Cd, n, seed=2)
    return {**{key: torch.from_numpy(v) for key, v in zip(("S", "class_sum", "total_sum", "class_count", "sums"), mr.accumulate(f, y, K))},
            "shrinkage": 1e-3}


def test_neighbour_state_columns_and_round_trip():
    from uncertainty_vit_amd.linear_probe import KNN_COLUMNS, MAHA_COLUMNS, LinearProbe
    from uncertainty_vit_amd.native import UvitError
    assert KNN_COLUMNS == ("knn",)
    sd, dens = host_state(), density_state()
    for cls in five_probes():
        torch.manual_seed(3)
        probe = cls(tiny_encoder().eval(), 10)
        before, keys = probe.DETECT_COLUMNS, list(probe.state_dict())
        assert probe.neighbours is None
        info = probe.set_neighbours(sd)
        assert info == probe.neighbours == {"n": 58, "skipped": 2, "classes": 10, "k": 5, "temperature": 0.07}
        assert probe.DETECT_COLUMNS == before + KNN_COLUMNS and "DETECT_COLUMNS" in probe.__dict__ and type(probe).DETECT_COLUMNS != probe.DETECT_COLUMNS
        assert list(probe.state_dict()) == keys and not [n for n, _ in probe.named_buffers() if "knn" in n]      # neither parameter nor buffer
        # with a density: behind its columns, whichever is set first; eleven columns at most
        probe.set_density(dens)
        assert probe.DETECT_COLUMNS == before + MAHA_COLUMNS + KNN_COLUMNS and len(probe.DETECT_COLUMNS) <= 11
        probe.set_neighbours(None)
        assert probe.DETECT_COLUMNS == before + MAHA_COLUMNS and probe.neighbours is None
        probe.set_neighbours(sd)
        assert probe.DETECT_COLUMNS == before + MAHA_COLUMNS + KNN_COLUMNS
        probe.set_density(None)
        assert probe.DETECT_COLUMNS == before + KNN_COLUMNS
        # round trip, another k without a refit, load_state_dict and _apply keep the bank
        again = probe.neighbour_state_dict()
        assert set(again) == set(sd) and again["bank"].dtype == torch.bfloat16 and again["labels"].dtype == torch.int32
        assert all(torch.equal(again[key], sd[key]) for key in ("bank", "labels", "sums")) and (again["k"], again["temperature"]) == (5, 0.07)
        assert probe.set_neighbours_k(20) == {**info, "k": 20} and probe.set_neighbours_k(3, 0.1) == {**info, "k": 3, "temperature": 0.1}
        assert probe.neighbour_state_dict()["k"] == 3 and probe.load_neighbour_state(again) == info
        probe.load_state_dict(probe.state_dict())
        moved = probe.float()
        assert moved.neighbours == info and moved._knn["bank"].dtype == torch.bfloat16 and torch.equal(moved._knn["bank"], sd["bank"])
        assert probe.DETECT_COLUMNS == before + KNN_COLUMNS
        # refusals
        for bad in ({"k": 0}, {"k": 257}, {"k": 2.5}, {"k": 59}, {"temperature": 0.0}, {"temperature": -1.0}, {"temperature": float("nan")},
                    {"temperature": float("inf")}, {"bank": sd["bank"].float()}, {"labels": sd["labels"].long()}, {"labels": sd["labels"][:-1]},
                    {"sums": torch.zeros(3)}, {"sums": torch.tensor([4.0, 56.0])}):
            with pytest.raises(UvitError):
                probe.load_neighbour_state({**sd, **bad})
        with pytest.raises(UvitError):
            probe.load_neighbour_state({"bank": sd["bank"]})
        with pytest.raises(UvitError):
            probe.load_neighbour_state(host_state(Cd=64))                      # another C
        with pytest.raises(UvitError):
            probe.load_neighbour_state({**sd, "labels": torch.where(sd["labels"] == 9, 10, sd["labels"]).int()})      # another K
        for call in (lambda: probe.set_neighbours_k(0), lambda: probe.set_neighbours_k(59), lambda: probe.set_neighbours_k(5, 0.0)):
            with pytest.raises(UvitError):
                call()
        assert probe.neighbours == info                                        # a refused state or k leaves the one in use
        for call in (lambda: probe.neighbour_scores(torch.zeros(2, 3, 48, 48)), lambda: probe.neighbour_batch(torch.zeros(2, 128))):
            with pytest.raises(UvitError):                                     # no CPU fallback
                call()
        probe.set_neighbours(None)
        assert probe.neighbours is None and probe.DETECT_COLUMNS == before
        if cls is LinearProbe:
            assert "DETECT_COLUMNS" not in probe.__dict__
        for call in (probe.neighbour_state_dict, lambda: probe.set_neighbours_k(5), lambda: probe.neighbour_scores(torch.zeros(2, 3, 48, 48)),
                     lambda: probe.neighbour_batch(torch.zeros(2, 128)), lambda: probe.fit_neighbours([]), lambda: probe.fit_neighbours([], k=0),
                     lambda: probe.fit_neighbours([(torch.zeros(2, 3, 48, 48), torch.zeros(2, dtype=torch.int64))])):
            with pytest.raises(UvitError):
                call()


def test_columns_compose_with_laplace_and_density_in_every_order():
    import itertools
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    from uncertainty_vit_amd.linear_probe import LinearProbe
    base, sd, dens = LinearProbe.DETECT_COLUMNS, host_state(), density_state()
    lap_state = {"info": {"n": 3, "n_skipped": 0, "nll": 1.0, "prior_precision": 1.0, "log_marglik": -2.0, "on_grid_edge": False}}

    def set_lap(probe, on):                      # a Laplace fit installed by hand: the kernels of a real one need a GPU
        if on:
            probe._lap = dict(lap_state)
            probe._det_refresh()
        else:
            probe.set_laplace(None)

    switch = {"lap": set_lap, "maha": lambda p, on: p.set_density(dens if on else None), "knn": lambda p, on: p.set_neighbours(sd if on else None)}
    cols = {"lap": ("lap_var",), "maha": ("maha", "rmaha"), "knn": ("knn",)}
    probe = LaplaceProbe(tiny_encoder().eval(), 10)
    for on_order in itertools.permutations(switch):
        for off_order in itertools.permutations(switch):
            have = set()
            assert probe.DETECT_COLUMNS == base
            for name, order in [(n, True) for n in on_order] + [(n, False) for n in off_order]:
                switch[name](probe, order)
                have = have | {name} if order else have - {name}
                want = base + tuple(c for n in ("lap", "maha", "knn") if n in have for c in cols[n])
                assert probe.DETECT_COLUMNS == want, (on_order, off_order, name, order)
    assert LaplaceProbe.DETECT_COLUMNS == base + ("lap_var",)


# ---- the command line ----
def test_cli_flags_are_absent_unless_given():
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()
    assert not [k for k in vars(rlp.get_args([])) if k.startswith("knn")]
    assert rlp.check_knn_flags(rlp.get_args([])) is None and rlp.check_knn_flags(rlp.get_args(["--eval"])) is None
    a = rlp.get_args(["--eval", "--knn_data_path", "d"])
    assert a.knn_data_path == "d" and not hasattr(a, "knn_k") and not hasattr(a, "knn_temperature") and rlp.check_knn_flags(a) == "fit"
    a = rlp.get_args(["--eval", "--knn_state", "s.pth", "--knn_k", "200", "--knn_temperature", "0.1"])
    assert (a.knn_k, a.knn_temperature) == (200, 0.1) and rlp.check_knn_flags(a) == "state"
    for head in ("--gp_layer", "--het_layer", "--ensembles", "--laplace"):
        assert rlp.check_knn_flags(rlp.get_args(["--eval", head, "--knn_data_path", "d", "--maha_data_path", "m"])) == "fit"


def test_cli_refuses_what_does_not_go_together():
    import run_linear_probe as rlp
    for argv in (["--knn_data_path", "d"], ["--knn_state", "s.pth"], ["--knn_k", "5"], ["--knn_temperature", "0.1"],      # all four need --eval
                 ["--eval", "--knn_data_path", "d", "--knn_state", "s.pth"],                                            # two sources
                 ["--eval", "--knn_data_path", "d", "--knn_k", "0"], ["--eval", "--knn_data_path", "d", "--knn_k", "257"],
                 ["--eval", "--knn_state", "s", "--knn_k", "-3"],
                 ["--eval", "--knn_data_path", "d", "--knn_temperature", "0"], ["--eval", "--knn_data_path", "d", "--knn_temperature", "-1"],
                 ["--eval", "--knn_data_path", "d", "--knn_temperature", "nan"], ["--eval", "--knn_state", "s", "--knn_temperature", "inf"]):
        with pytest.raises(ValueError):
            rlp.check_knn_flags(rlp.get_args(argv))


def test_cli_lines_and_log_entries():
    import run_linear_probe as rlp
    fit = {"n": 240, "skipped": 2, "classes": 10, "k": 20, "temperature": 0.07}
    stats = {"knn_acc1": 87.5, "knn_mean": 0.3125}
    assert rlp.knn_lines(fit, stats) == ["* kNN bank of 240 images (2 skipped), 10 classes, k 20, temperature 0.07",
                                         "* kNN Acc@1 87.500 mean 0.31250"]
    assert rlp.knn_log_entries(fit, stats) == {"test_knn_acc1": 87.5, "test_knn_mean": 0.3125, "test_knn_k": 20}
