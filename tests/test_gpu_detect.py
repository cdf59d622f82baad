"""GPU: the detection ops (csrc/detect.hip) against the float64 restatement (tests/detect_ref.py), then evaluate(detection=True,
ood_loader=...) of the four probes against the restatement applied to the probe's own per-sample columns.

Metrics op: the sample order, the counts, AUROC and FPR95 are exact quantities (integers and one division): order and counts are
compared for equality, AUROC and FPR95 to 1e-12.  AUPR and AURC are double sums in a fixed order that differs from numpy's: 1e-9
absolute, the project's bound for fixed-order double sums (N 2^-53 is 1e-10 at N = 2^20 for terms below 1); the worst seen is printed.
Rows op: the bounds of detect_ref.row_scores, derived from the ulp bounds of the fp32 steps; the worst |error| / bound is printed."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import detect_ref as dr
import probe_ref as pr
from test_gpu_probe import P, S as STREAM, fixture_probe, ok, rnd

pytestmark = pytest.mark.gpu

EXACT_TOL, SUM_TOL = 1e-12, 1e-9
SIZES = [1, 2, 3, 4095, 4096, 4097, 12293, 32769]      # one chunk (five sizes), one global level, two with a ragged pad, four
REGIMES = ["continuous", "quantised", "equal"]
WORST = {"AUPR": 0.0, "AURC": 0.0, "rows": 0.0}


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


# ------------------------------------------------------------------------------------------------------------------------ inputs
_SETS, _REF = {}, {}


def score_set(N, regime):
    """(scores (3, N) fp32, flags (N,) uint8): three columns of one regime; the flags lean towards the high scores of column 0."""
    if (N, regime) not in _SETS:
        rng = np.random.default_rng(1000 * N + REGIMES.index(regime))
        if regime == "continuous":
            s = rng.standard_normal((3, N)).astype(np.float32)
        elif regime == "quantised":                    # about 7 values: tie groups far longer than a chunk at the larger N
            s = (rng.integers(0, 7, (3, N)) / 8.0).astype(np.float32)
        else:
            s = np.full((3, N), 0.375, dtype=np.float32)
        f = (rng.random(N) < 0.3 + 0.2 * np.tanh(s[0])).astype(np.uint8)
        _SETS[(N, regime)] = (s, f)
    return _SETS[(N, regime)]


def reference(key, scores, flags):
    """The restatement's table and orders, computed once per input."""
    if key not in _REF:
        _REF[key] = dr.table(scores, flags)
    return _REF[key]


def run_metrics(L, scores, flags, ld=None, want_order=True):
    """uvit_op_detect_metrics on host arrays: (table (S, 8), order (S, N) or None) as numpy; guards behind every output intact."""
    scores = np.atleast_2d(scores)
    S, N = scores.shape
    ld = N if ld is None else ld
    sg = torch.full((S, ld), 7.5, dtype=torch.float32, device="cuda")
    sg[:, :N] = torch.from_numpy(scores).cuda()
    fg = torch.from_numpy(flags).cuda()
    ws_bytes = L.uvit_op_detect_ws_bytes(N, S)
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = 0x5A
    out = torch.full((8 * S + 16,), 7.5, dtype=torch.float64, device="cuda")
    order = torch.full((S * N + 16,), -7, dtype=torch.int32, device="cuda") if want_order else None
    ok(L.uvit_op_detect_metrics(P(sg), ld, P(fg), N, S, P(order), P(out), P(ws), ws_bytes, STREAM()))
    torch.cuda.synchronize()
    assert bool((out[8 * S:] == 7.5).all()) and bool((ws[ws_bytes:] == 0x5A).all())
    if want_order:
        assert bool((order[S * N:] == -7).all())
    return out[:8 * S].view(S, 8).cpu().numpy(), (order[:S * N].view(S, N).cpu().numpy() if want_order else None)


def check_table(got, ref, what):
    """Counts exact, AUROC / FPR95 to 1e-12, AUPR / AURC to 1e-9; NaN where the restatement has NaN."""
    assert np.array_equal(got[:, 4:], ref[:, 4:]), (what, got[:, 4:], ref[:, 4:])
    for col, (name, tol) in enumerate((("AUROC", EXACT_TOL), ("AUPR", SUM_TOL), ("FPR95", EXACT_TOL), ("AURC", SUM_TOL))):
        g, r = got[:, col], ref[:, col]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, name, g, r)
        err = float(np.nanmax(np.abs(g - r))) if not np.isnan(r).all() else 0.0
        if name in WORST:
            WORST[name] = max(WORST[name], err)
        assert err <= tol, (what, name, err, g, r)


# -------------------------------------------------------------------------------------------------------------------- metrics op
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_metrics_against_restatement(L, N, S, regime):
    """Every path of the sort in every score regime: the order equals the restatement's permutation, the counts are exact, the four
    metrics hold their bounds; a second call gives the same bits; ld > N changes nothing."""
    scores, flags = score_set(N, regime)
    scores = scores[:S]
    ref, ref_order = reference((N, regime, S), scores, flags)
    got, order = run_metrics(L, scores, flags)
    assert np.array_equal(order, ref_order), (N, S, regime)
    check_table(got, ref, (N, S, regime))
    again, order2 = run_metrics(L, scores, flags, ld=N + 37)
    assert got.tobytes() == again.tobytes() and np.array_equal(order, order2)
    print(f"\nN {N} S {S} {regime}: AUROC {got[0, 0]:.6f} AUPR {got[0, 1]:.6f} FPR95 {got[0, 2]:.6f} AURC {got[0, 3]:.6f}; "
          f"worst so far AUPR {WORST['AUPR']:.2e} AURC {WORST['AURC']:.2e} (bound {SUM_TOL:.0e})")


@pytest.mark.parametrize("N", [3, 4097, 12293])
def test_columns_are_independent(L, N):
    """A column gives the same bits alone and beside others, and without the order output."""
    scores, flags = score_set(N, "quantised")
    scores = np.stack([scores[0], score_set(N, "continuous")[0][1], scores[2]])
    together, order = run_metrics(L, scores, flags)
    for c in range(3):
        alone, order1 = run_metrics(L, scores[c], flags)
        assert alone[0].tobytes() == together[c].tobytes() and np.array_equal(order1[0], order[c])
    assert run_metrics(L, scores, flags, want_order=False)[0].tobytes() == together.tobytes()


@pytest.mark.parametrize("case", ["P0", "Nn0", "P1_top", "P1_bottom", "P1_tied"])
def test_degenerate_positive_counts(L, case):
    N = 5000
    scores = score_set(4097, "quantised" if case == "P1_tied" else "continuous")[0][:2, :N - 903].copy()
    scores = np.concatenate([scores, scores[:, :903] + np.float32(0.25)], axis=1)
    flags = np.zeros(N, dtype=np.uint8)
    if case == "Nn0":
        flags[:] = 1
    elif case.startswith("P1"):
        flags[{"P1_top": int(scores[0].argmax()), "P1_bottom": int(scores[0].argmin()), "P1_tied": 4099}[case]] = 1
    ref, ref_order = dr.table(scores, flags)
    got, order = run_metrics(L, scores, flags)
    print(f"\n{case}: {got[0].tolist()}")
    assert np.array_equal(order, ref_order)
    check_table(got, ref, case)
    if case == "P1_top":
        assert got[0, 0] == 1.0 and got[0, 1] == 1.0 and got[0, 2] == 0.0
    if case == "P0":
        assert np.isnan(got[:, :3]).all() and (got[:, 3] == 0.0).all()
    if case == "Nn0":
        assert np.isnan(got[:, 0]).all() and (np.abs(got[:, 1] - 1.0) <= SUM_TOL).all() and (np.abs(got[:, 3] - 1.0) <= SUM_TOL).all()


def test_nan_scores_are_counted_and_left_out(L):
    """NaN at the first and the last index and in the middle of a chunk, both signs of zero, +-inf: the NaN rows come last by index,
    n and the NaN count are exact, the metrics are those of the remaining rows; a column of NaN alone gives n = 0 and four NaNs."""
    N = 6001
    scores, flags = (a.copy() for a in score_set(12293, "continuous"))
    scores, flags = scores[:, :N].copy(), flags[:N].copy()
    scores[0, [0, N - 1, 2048 + 17, 4096]] = np.nan
    scores[0, [5, 9]] = [0.0, -0.0]
    scores[0, [11, 12]] = [np.inf, -np.inf]
    scores[1, :] = np.nan
    flags[[0, N - 1]] = 1
    ref, ref_order = dr.table(scores, flags)
    got, order = run_metrics(L, scores, flags)
    print(f"\nNaN rows: {got[:, 4:7].tolist()}")
    assert np.array_equal(order, ref_order) and order[0, -4:].tolist() == [0, 2048 + 17, 4096, N - 1] and order[1].tolist() == list(range(N))
    assert got[0, 4:7].tolist() == [N - 4, float(flags.sum() - flags[[0, N - 1, 2048 + 17, 4096]].sum()), 4.0]
    assert got[1, 4:7].tolist() == [0.0, 0.0, float(N)] and np.isnan(got[1, :4]).all()
    check_table(got, ref, "nan")


def test_bad_label_flag_makes_every_metric_nan(L):
    """One flag 2, on a row whose score is NaN in column 0: all four metrics are NaN in every column, the counts stay."""
    N = 4500
    scores, flags = (a.copy() for a in score_set(12293, "continuous"))
    scores, flags = scores[:2, :N].copy(), flags[:N].copy()
    scores[0, 4321] = np.nan
    flags[4321] = 2
    got, _ = run_metrics(L, scores, flags)
    ref, _ = dr.table(scores, flags)
    assert np.isnan(got[:, :4]).all() and np.array_equal(got[:, 4:], ref[:, 4:]) and got[0, 6] == 1.0


def test_golden_sets_on_the_device(L, golden_dir):
    """The scikit-learn fixture through the kernel: AUROC, average precision and FPR95 as stored."""
    import os
    fx = np.load(os.path.join(golden_dir, "detect.npz"))
    for n in [str(v) for v in fx["names"]]:
        got, _ = run_metrics(L, fx["scores/" + n], fx["flags/" + n])
        d = [got[0, 0] - float(fx["auroc/" + n]), got[0, 1] - float(fx["ap/" + n]), got[0, 2] - float(fx["fpr95/" + n])]
        print(f"\n{n}: kernel - scikit-learn: AUROC {d[0]:+.2e} AUPR {d[1]:+.2e} FPR95 {d[2]:+.2e}")
        assert abs(d[0]) <= EXACT_TOL and abs(d[1]) <= SUM_TOL and abs(d[2]) <= EXACT_TOL


# ----------------------------------------------------------------------------------------------------------------------- rows op
def row_logits(B, K):
    """Logits of spread 3 with, from row 1 on, an argmax tie in every second row (the maximum copied to a later class)."""
    z = rnd(B, K, seed=400 + B + K, scale=3.0).numpy()
    for b in range(1, B, 2):
        first = int(z[b].argmax())
        z[b, (first + 1 + b) % K] = z[b, first]
    return z


def row_labels(z):
    """Per row in turn: the prediction, the later index of a tie (or another class), class 0, the last class."""
    B, K = z.shape
    pred = z.argmax(1)
    y = np.empty(B, dtype=np.int64)
    for b in range(B):
        tied = np.nonzero(z[b] == z[b].max())[0]
        y[b] = [pred[b], tied[-1] if len(tied) > 1 else (pred[b] + 1) % K, 0, K - 1][b % 4]
    return y


def run_rows(L, z, y, n0, ld):
    """(scores (3, ld), flags (ld,)) after the call, on buffers filled with sentinels."""
    B, K = z.shape
    sg = torch.full((3, ld), 7.5, dtype=torch.float32, device="cuda")
    fg = torch.full((ld,), 9, dtype=torch.uint8, device="cuda")
    zg = torch.from_numpy(z).cuda()
    yg = None if y is None else torch.from_numpy(y).cuda()
    ok(L.uvit_op_detect_rows(P(zg), P(yg), P(sg), ld, n0, P(fg), B, K, STREAM()))
    torch.cuda.synchronize()
    return sg.cpu().numpy(), fg.cpu().numpy()


@pytest.mark.parametrize("K", [2, 10, 1000])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_rows_against_restatement(L, B, K):
    """The three scores within the derived bounds, the flags exact (argmax ties included), nothing written outside the batch's
    positions, no flag written without labels, two calls give the same bits."""
    z = row_logits(B, K)
    y = row_labels(z)
    n0, ld = 3 + 2 * B + K % 7, 3 + 2 * B + K % 7 + B + 5
    ref, bound, fref = dr.row_scores(z, y)
    sc, fl = run_rows(L, z, y, n0, ld)
    keep = np.ones(ld, dtype=bool)
    keep[n0:n0 + B] = False
    assert (sc[:, keep] == 7.5).all() and (fl[keep] == 9).all()
    assert np.array_equal(fl[n0:n0 + B], fref) and set(fref.tolist()) <= {0, 1}
    if B >= 5:
        assert 0 < int(fref.sum()) < B
    ratio = np.abs(sc[:, n0:n0 + B].astype(np.float64) - ref) / bound
    WORST["rows"] = max(WORST["rows"], float(ratio.max()))
    print(f"\nrows ({B}, {K}) n0 {n0}: worst |error| / bound per column {ratio.max(1).tolist()} (worst so far {WORST['rows']:.3f})")
    assert float(ratio.max()) <= 1.0
    sc2, fl2 = run_rows(L, z, y, n0, ld)
    assert sc.tobytes() == sc2.tobytes() and np.array_equal(fl, fl2)
    sc3, fl3 = run_rows(L, z, None, n0, ld)
    assert sc3.tobytes() == sc.tobytes() and (fl3 == 9).all()


def test_rows_extreme_logits_and_bad_labels(L):
    """One-hot and very large logits give finite scores within their bounds (entropy 0 at a one-hot row, never negative); a label
    outside [0, K) is flag 2."""
    z = np.zeros((6, 5), dtype=np.float32)
    z[0, 2] = 200.0
    z[1] = [3e38, -3e38, 0.0, 1e30, -1e30]
    z[2] = [1e30, 1e30, -1e30, 0.0, 0.0]
    z[3] = -3e38
    z[4] = [-100.0, -100.0, -100.0, -100.0, -20.0]
    y = np.array([2, 0, 1, -1, 5, 0], dtype=np.int64)
    ref, bound, fref = dr.row_scores(z, y)
    sc, fl = run_rows(L, z, y, 1, 9)
    got = sc[:, 1:7].astype(np.float64)
    print(f"\nextreme rows: {got.tolist()}")
    assert np.isfinite(got).all() and (got[1] >= 0).all() and got[1, 0] == 0.0 and got[0, 0] == 0.0
    assert (np.abs(got - ref) <= bound).all()
    assert fl[1:7].tolist() == fref.tolist() == [0, 0, 1, 2, 2, 0]


def test_column_op(L):
    """float and double sources with a row stride, into the middle of a column."""
    src = torch.arange(40, dtype=torch.float64, device="cuda").view(8, 5) / 3
    for t in (src, src.float()):
        dst = torch.full((20,), 7.5, dtype=torch.float32, device="cuda")
        ok(L.uvit_op_detect_column(P(t[:, 2]), int(t.dtype == torch.float64), 5, C.c_void_p(dst.data_ptr() + 4 * 6), 8, STREAM()))
        torch.cuda.synchronize()
        assert torch.equal(dst[6:14], t[:, 2].float()) and bool((dst[:6] == 7.5).all()) and bool((dst[14:] == 7.5).all())


# --------------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


def make_probe(case, kind):
    linear = fixture_probe(case)
    if kind == "linear":
        return linear
    enc = linear.encoder
    torch.manual_seed(5)
    if kind == "gp":
        from uncertainty_vit_amd.gp_probe import GPProbe
        return GPProbe(enc, 10, num_inducing=64)
    if kind == "het":
        from uncertainty_vit_amd.het_probe import HetProbe
        return HetProbe(enc, 10, num_factors=4, test_mc_samples=64)
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    return EnsembleProbe(enc, 10, members=3, init_scale=5.0)


def own_columns(L, probe, kind, x):
    """The probe's per-sample columns of a batch from its public methods, as fp32: (columns (S, B), logits (B, K)).  The three
    columns of the logits are the rows op's on probe.logits(x), held here against the float64 restatement within its bounds: two
    roundings of the same value to fp32 can differ in the last place, and a rank must not hang on that (the het head's energy is
    -log sum p = 0 up to rounding for every sample)."""
    zg = probe.logits(x)
    z = zg.cpu().numpy()
    B = z.shape[0]
    sg = torch.zeros(3, B, dtype=torch.float32, device="cuda")
    ok(L.uvit_op_detect_rows(P(zg), None, P(sg), B, 0, None, B, z.shape[1], STREAM()))
    sc, bound, _ = dr.row_scores(z)
    assert (np.abs(sg.cpu().numpy().astype(np.float64) - sc) <= bound).all()
    cols = [sg.cpu().numpy()]
    if kind == "gp":
        cols.append(probe.predictive_variance(x).cpu().numpy().astype(np.float32)[None])
    elif kind == "het":
        pv = probe.predictive_variance(x).cpu().numpy()
        cols.append(pv[np.arange(len(z)), z.argmax(1)][None])
    elif kind == "ens":
        cols.append(probe.uncertainty(x).cpu().numpy().astype(np.float32).T)
    return np.concatenate(cols), z


@pytest.mark.parametrize("kind", ["linear", "gp", "het", "ens"])
def test_evaluate_detection_end_to_end(L, case, kind):
    """Two ragged evaluation batches and two ragged OOD batches: stats["detection"] equals the restatement applied to the probe's
    own per-sample columns; the other keys equal those of the plain evaluation; evaluate() without the arguments returns today's
    keys; twice gives the same numbers."""
    _, _, _, _, _, images, _ = case
    probe = make_probe(case, kind)
    x4 = images.cuda()                              # the fixture's four images, varied into 13 evaluation and 11 OOD images
    pool = torch.cat([x4, x4.flip(-1), x4.flip(-2), 0.5 * x4 + 0.25, x4.transpose(-1, -2).contiguous(), 0.7 * x4 - 0.1])
    xg, xo = pool[:13].contiguous(), pool[13:].contiguous()
    pred = probe.logits(xg).argmax(1).cpu()
    labels = torch.where(torch.arange(len(pred)) % 2 == 0, pred, (pred + 1) % probe.num_classes)      # every second prediction is wrong
    eval_batches = [((xg, None), labels), ((xg[:3], None), labels[:3])]
    ood_batches = [xo[:7], ((xo[7:], None), labels[:xo.shape[0] - 7])]
    plain = probe.evaluate(eval_batches)
    assert sorted(plain) == ["acc1", "acc5", "correct1", "correct5", "loss", "n"]
    e1 = probe.evaluate(eval_batches, detection=True, ood_loader=ood_batches)
    e2 = probe.evaluate(eval_batches, detection=True, ood_loader=ood_batches)
    only = probe.evaluate(eval_batches, detection=True)
    det = e1.pop("detection")
    assert e1 == plain and str(e2.pop("detection")) == str(det) and probe.evaluate(eval_batches) == plain
    assert "ood" not in only["detection"] and str(only["detection"]["misclassification"]) == str(det["misclassification"])
    assert det["columns"] == list(probe.DETECT_COLUMNS) and probe._det is None

    parts = [own_columns(L, probe, kind, x) for x in (xg, xg[:3], xo[:7], xo[7:])]
    cols = np.concatenate([p[0] for p in parts], axis=1)
    y = torch.cat([labels, labels[:3]]).numpy()
    z_eval = np.concatenate([parts[0][1], parts[1][1]])
    wrong = (z_eval.argmax(1) != y).astype(np.uint8)
    n, n_ood = len(y), xo.shape[0]
    assert (det["n"], det["n_wrong"], det["n_ood"]) == (n, int(wrong.sum()), n_ood) and n - plain["correct1"] == det["n_wrong"]
    mis, _ = dr.table(cols[:, :n], wrong)
    ood, _ = dr.table(cols, np.concatenate([np.zeros(n, dtype=np.uint8), np.ones(n_ood, dtype=np.uint8)]))
    print(f"\n{kind}: n {n}, wrong {det['n_wrong']}, OOD {n_ood}")
    for s, name in enumerate(det["columns"]):
        print(f"  {name}: misclassification {det['misclassification'][name]}  ood {det['ood'][name]}")
        for table, entry, keys in ((mis, det["misclassification"][name], ("AUROC", "AUPR", "FPR95", "AURC")), (ood, det["ood"][name], ("AUROC", "AUPR", "FPR95"))):
            assert tuple(entry) == keys
            for k, key in enumerate(keys):
                r, g = table[s, k], entry[key]
                assert (math.isnan(r) and math.isnan(g)) or abs(g - r) <= (EXACT_TOL if key in ("AUROC", "FPR95") else SUM_TOL), (name, key, g, r)
    assert 0 < det["n_wrong"] < n


def test_store_grows(case, L):
    """Three batches of 600 rows: the store grows from 1024 to 2048 places and keeps what it held; detection_batch on its columns
    equals the direct call."""
    probe = fixture_probe(case)
    B, K = 600, probe.num_classes
    probe._buffers_for(B)
    probe._det = {"scores": None, "flags": None, "cap": 0, "n": 0}
    zs, ys = [], []
    try:
        for i in range(3):
            z = rnd(B, K, seed=700 + i, scale=2.0)
            y = torch.from_numpy(row_labels(z.numpy()))
            probe._logits[:B].copy_(z.cuda())
            probe._det_reserve(B)
            probe._det_rows(B, y.cuda())
            zs.append(z.numpy())
            ys.append(y.numpy())
        d = probe._det
        assert (d["n"], d["cap"]) == (1800, 2048)
        scores, flags = d["scores"][:, :1800].contiguous(), d["flags"][:1800].contiguous()
    finally:
        probe._det = None
    ref, bound, fref = dr.row_scores(np.concatenate(zs), np.concatenate(ys))
    assert np.array_equal(flags.cpu().numpy(), fref) and (np.abs(scores.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    table, order = probe.detection_batch(scores, flags, order=True)
    want, want_order = dr.table(scores.cpu().numpy(), fref)
    assert np.array_equal(order.cpu().numpy(), want_order)
    check_table(table.cpu().numpy(), want, "store")
    from uncertainty_vit_amd.native import UvitError
    with pytest.raises(UvitError):
        probe.detection_batch(scores.double(), flags)
    with pytest.raises(UvitError):
        probe.detection_batch(scores, flags[:-1])
