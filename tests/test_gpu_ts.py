"""GPU: temperature scaling (csrc/tscale.hip) against the float64 restatement (tests/ts_ref.py), then fit_temperature() and
evaluate(temperature=...) of the four probes.

Fit: the status equals that of the independent bisection; for an interior optimum the float64 gradient at the device's s is within
bound_g + tol s h of zero and s within that over h of the bisection's root; the two NLLs are within bound_nll of float64 at the same
s.  The bounds are derived in ts_ref's docstring from the ulp bounds of the kernel's fp32 steps; the worst |error| / bound is printed.
The grid is ts_ref.GRID: the sizes on both sides of the 16 rows of a workgroup (and of the 4 of a wave), of the 256 partials per
stride of the summing step (N = 4096 | 4097) and of the row pass's register paths (K = 64 | 65, 256 | 257, 1024 | 1025)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import detect_ref as dr
import ts_ref as tr
from test_gpu_detect import EXACT_TOL, SUM_TOL, make_probe
from test_gpu_probe import P, S as STREAM, ok

pytestmark = pytest.mark.gpu

WORST = {"g": 0.0, "s": 0.0, "nll": 0.0}
D = C.c_double


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def run_fit(L, z, y, ld=None, t_min=tr.T_MIN, t_max=tr.T_MAX, tol=tr.TOL, max_iter=tr.MAX_ITER):
    """The (8,) table of one call, on a workspace of exactly the size asked for and a padded copy of the logits when ld > K."""
    N, K = z.shape
    ld = K if ld is None else ld
    zg = torch.full((N, ld), float("nan"), dtype=torch.float32, device="cuda")      # the padding is NaN: reading it would show
    zg[:, :K] = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    yg = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int64)).cuda()
    ws_bytes = L.uvit_op_ts_ws_bytes(N, K)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.full((8,), 7.5, dtype=torch.float64, device="cuda")
    ok(L.uvit_op_ts_fit(P(zg), ld, P(yg), N, K, D(t_min), D(t_max), D(tol), max_iter, P(out), P(ws), ws_bytes, STREAM()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_fit(out, rows, ref, tol=tr.TOL, label=""):
    """The issue's checks of one table against the bisection's result `ref` on the usable rows `rows`."""
    T, s, nll1, nll, g, passes, status, skipped = out.tolist()
    assert int(status) == ref["status"], (label, out.tolist(), ref)
    assert 1 <= passes <= 16 and skipped == rows.N - rows.n
    bf1 = rows.bounds(1.0)[0]
    bf, bg = rows.bounds(s)
    f_ref, g_ref, h_ref = rows.fgh(s)
    r_nll = max(abs(nll1 - rows.fgh(1.0)[0]) / bf1, abs(nll - f_ref) / bf)
    r_g = abs(g - g_ref) / bg
    WORST["nll"], WORST["g"] = max(WORST["nll"], r_nll), max(WORST["g"], r_g)
    msg = f"\n{label}: T {T:.6f} status {int(status)} passes {int(passes)}; |error| / bound: NLL {r_nll:.3f}, g {r_g:.3f}"
    assert r_nll <= 1.0 and r_g <= 1.0, msg
    if ref["status"] == 0:
        slack = bg + tol * s * h_ref
        r_s = abs(s - ref["s"]) / (slack / h_ref)
        WORST["s"] = max(WORST["s"], r_s)
        msg += f", s {r_s:.3f}"
        assert abs(g_ref) <= slack and r_s <= 1.0, msg
        assert abs(T - 1.0 / s) <= 1e-15 * T
    else:
        assert s == ref["s"] and T == ref["T"], msg
    print(msg + f" (worst so far: NLL {WORST['nll']:.3f}, g {WORST['g']:.3f}, s {WORST['s']:.3f})")


@pytest.mark.parametrize("N,K,scale", tr.GRID)
def test_fit_against_restatement(L, N, K, scale):
    z, y, rows, ref = tr.grid_case(N, K, scale)
    out = run_fit(L, z, y)
    check_fit(out, rows, ref, label=f"({N}, {K}) x {scale}")
    assert run_fit(L, z, y).tobytes() == out.tobytes()              # a second call gives the same bits


@pytest.mark.parametrize("N,K", [(65, 10), (257, 1003), (4097, 100), (65, 1025)])
def test_row_stride_does_not_change_the_bits(L, N, K):
    z, y, _, _ = tr.grid_case(N, K, 1.0)
    assert run_fit(L, z, y, ld=K + 5).tobytes() == run_fit(L, z, y).tobytes()


def test_grid_holds_what_float64_gives():
    """Interior optima with T in (0.11, 11.6) from N = 63 on; both clamps occur among the smallest sets."""
    assert tr.grid_case(3, 2, 1.0)[3]["status"] == 2 and tr.grid_case(1, 1003, 1.0)[3]["status"] == 1
    assert {(16, 10, 1.0), (17, 10, 1.0), (4096, 100, 1.0), (4097, 100, 1.0), (257, 1024, 1.0), (257, 1025, 1.0)} <= set(tr.GRID)


@pytest.mark.parametrize("bad", [-1, 10])
def test_a_label_outside_the_classes_makes_the_table_nan(L, bad):
    z, y, _, _ = tr.grid_case(257, 10, 1.0)
    for at in (0, 100, 256):
        yb = y.copy()
        yb[at] = bad
        assert np.isnan(run_fit(L, z, yb)).all(), at


def test_rows_with_a_non_finite_logit_are_left_out(L):
    """NaN in the first, a middle and the last row (and an infinity): counted, and the fit is the fit without those rows -- within
    the restatement's bounds, and within 1e-12 of the device's own fit of the set without them (taking rows out moves the others to
    other waves and workgroups, so the fixed order of the double sums is another one and the last bits may differ)."""
    z, y, _, _ = tr.grid_case(257, 10, 1.0)
    zb = z.copy()
    zb[0, 3], zb[128, 0], zb[256, 9], zb[77, 5] = np.nan, np.nan, np.nan, np.inf
    keep = np.ones(257, dtype=bool)
    keep[[0, 128, 256, 77]] = False
    out = run_fit(L, zb, y)
    assert out[7] == 4.0
    rows = tr.Rows(z[keep], y[keep])
    ref = tr.fit_bisect(None, None, rows=rows)
    rows.N += 4                                                     # the table counts the four rows the restatement never saw
    check_fit(out, rows, ref, label="non-finite rows")
    clean = run_fit(L, z[keep], y[keep])
    assert clean[7] == 0.0 and clean[5:7].tolist() == out[5:7].tolist()
    assert all(abs(out[i] - clean[i]) <= 1e-12 * abs(clean[i]) for i in range(4)) and abs(out[4] - clean[4]) <= 1e-12
    every = run_fit(L, np.full((5, 10), np.nan, dtype=np.float32), y[:5])
    assert np.isnan(every[:5]).all() and every[5:].tolist() == [1.0, 0.0, 5.0]


def test_limits_of_the_iteration(L):
    """max_iter = 1 stops after the first pass with status 3 at s_0 = 1; a temperature range that leaves 1 outside starts from its
    nearer end and agrees with the bisection over the same range; a wide tolerance stops early."""
    z, y, rows, ref = tr.grid_case(257, 10, 4.0)
    one = run_fit(L, z, y, max_iter=1)
    assert one[5:7].tolist() == [1.0, 3.0] and one[1] == 1.0 and one[0] == 1.0
    assert abs(one[3] - one[2]) <= 2 * rows.bounds(1.0)[0]
    for t_min, t_max in ((2.0, 50.0), (0.05, 0.5), (ref["T"] * 1.5, 90.0)):
        check_fit(run_fit(L, z, y, t_min=t_min, t_max=t_max), rows, tr.fit_bisect(None, None, t_min, t_max, rows=rows), label=f"T in [{t_min}, {t_max}]")
    loose = run_fit(L, z, y, tol=1e-2)
    assert loose[6] == 0.0 and loose[5] <= run_fit(L, z, y)[5] and abs(loose[1] - ref["s"]) <= 0.05 * ref["s"]


@pytest.mark.parametrize("B,K", [(1, 2), (5, 10), (64, 1000), (130, 257), (1500, 3)])
def test_scale_op(L, B, K):
    """dst = (float)((double) src * s), exactly, out of place with two row strides and in place; a NaN s gives NaN."""
    rng = np.random.default_rng(31 * B + K)
    z = (rng.standard_normal((B, K)) * 5).astype(np.float32)
    s = 1.0 / 1.7320508
    table = torch.tensor([1.0 / s, s, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device="cuda")
    want = (z.astype(np.float64) * s).astype(np.float32)
    src = torch.full((B, K + 3), 7.5, dtype=torch.float32, device="cuda")
    src[:, :K] = torch.from_numpy(z).cuda()
    dst = torch.full((B, K + 6), 9.5, dtype=torch.float32, device="cuda")
    ok(L.uvit_op_ts_scale(P(src), P(dst), K + 3, K + 6, P(table), B, K, STREAM()))
    torch.cuda.synchronize()
    assert dst[:, :K].cpu().numpy().tobytes() == want.tobytes() and bool((dst[:, K:] == 9.5).all())
    ok(L.uvit_op_ts_scale(P(src), P(src), K + 3, K + 3, P(table), B, K, STREAM()))
    torch.cuda.synchronize()
    assert src[:, :K].cpu().numpy().tobytes() == want.tobytes() and bool((src[:, K:] == 7.5).all())
    order = np.argsort(z, axis=1, kind="stable")
    assert bool((np.diff(np.take_along_axis(want, order, 1), axis=1) >= 0).all())           # monotone: no pair of a row changes its order
    table[1] = float("nan")
    ok(L.uvit_op_ts_scale(P(src), P(src), K + 3, K + 3, P(table), B, K, STREAM()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(src[:, :K]).all()) and bool((src[:, K:] == 7.5).all())


def test_temperature_batch(L):
    """The module's entry point on caller-supplied logits: the table of the direct call, nothing set on the probe."""
    z, y, _, _ = tr.grid_case(257, 10, 1.0)
    from test_host_probe import tiny_encoder
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    probe = LinearProbe(tiny_encoder().eval().cuda(), 10)
    table = probe.temperature_batch(torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda())
    assert table.dtype == torch.float64 and table.shape == (8,) and table.is_cuda
    torch.cuda.synchronize()
    assert table.cpu().numpy().tobytes() == run_fit(L, z, y).tobytes() and probe.temperature is None
    with pytest.raises(UvitError):
        probe.temperature_batch(torch.from_numpy(z).cuda().double(), torch.from_numpy(y).cuda())
    with pytest.raises(UvitError):
        probe.temperature_batch(torch.from_numpy(z).cuda(), torch.from_numpy(y[:-1]).cuda())


# --------------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def case(golden_dir):
    import probe_ref as pr
    return pr.load_fixture(golden_dir)


def scaled_columns(L, probe, x):
    """The three row columns of the probe's own logits of a batch after the scale op with the probe's table, as the device forms them
    (held here against the restatement on the float64-scaled logits within its bounds), and the unscaled logits."""
    zg = probe.logits(x)
    z = zg.cpu().numpy()
    B, K = z.shape
    table = probe._ts_begin(True)[0]
    ok(L.uvit_op_ts_scale(P(zg), P(zg), K, K, P(table), B, K, STREAM()))
    want = (z.astype(np.float64) * probe._ts[1]).astype(np.float32)
    assert zg.cpu().numpy().tobytes() == want.tobytes()
    sg = torch.zeros(3, B, dtype=torch.float32, device="cuda")
    ok(L.uvit_op_detect_rows(P(zg), None, P(sg), B, 0, None, B, K, STREAM()))
    sc, bound, _ = dr.row_scores(want)
    assert (np.abs(sg.cpu().numpy().astype(np.float64) - sc) <= bound).all()
    return sg.cpu().numpy(), z


@pytest.mark.parametrize("kind", ["linear", "gp", "het", "ens"])
def test_fit_and_evaluate_end_to_end(L, case, kind):
    """Two ragged calibration batches: fit_temperature equals the restatement on the head's own logits; evaluate(temperature=True)
    keeps the counts of the unscaled evaluation, its loss is nll_after (5e-3 relative, the evaluation loss's tolerance in
    tests/test_gpu_probe.py), its detection row columns are those of the scaled logits; without the argument nothing changes."""
    _, _, _, _, _, images, _ = case
    probe = make_probe(case, kind)
    x4 = images.cuda()
    pool = torch.cat([x4, x4.flip(-1), x4.flip(-2), 0.5 * x4 + 0.25, x4.transpose(-1, -2).contiguous(), 0.7 * x4 - 0.1])
    xa, xb = pool[:13].contiguous(), pool[13:20].contiguous()
    za, zb = probe.logits(xa).cpu().numpy(), probe.logits(xb).cpu().numpy()
    z = np.concatenate([za, zb])
    pred = torch.from_numpy(z.argmax(1))
    labels = torch.where(torch.arange(len(pred)) % 3 != 2, pred, (pred + 1) % probe.num_classes)      # every third prediction is wrong
    batches = [((xa, None), labels[:13]), ((xb, None), labels[13:])]

    plain = probe.evaluate(batches)
    assert probe.evaluate(batches, temperature=None) == plain and "temperature" not in plain
    from uncertainty_vit_amd.native import UvitError
    with pytest.raises(UvitError):
        probe.evaluate(batches, temperature=True)                   # nothing fitted, nothing set

    fit = probe.fit_temperature(batches)
    rows = tr.Rows(z, labels.numpy())
    ref = tr.fit_bisect(None, None, rows=rows)
    print(f"\n{kind}: fit {fit}\n  bisection {ref}")
    assert sorted(fit) == ["T", "grad", "iterations", "n", "n_skipped", "nll_after", "nll_before", "status"]
    assert (fit["n"], fit["n_skipped"]) == (20, 0) and probe.post_hoc_temperature == fit["T"]
    if kind != "het":
        assert probe.temperature == fit["T"]
    table = probe._ts_table.cpu().numpy()
    check_fit(table, rows, ref, label=kind)
    assert fit["T"] == table[0] and fit["status"] == ref["status"] and fit["nll_after"] <= fit["nll_before"] + rows.bounds(1.0)[0]

    det = probe.evaluate(batches, detection=True, temperature=True)
    again = probe.evaluate(batches, temperature=True)
    assert det["temperature"] == fit["T"] == again["temperature"]
    assert (det["correct1"], det["correct5"], det["n"]) == (plain["correct1"], plain["correct5"], plain["n"]) and again["loss"] == det["loss"]
    assert det["loss"] == pytest.approx(fit["nll_after"], rel=5e-3)
    if ref["status"] == 0 and abs(fit["T"] - 1.0) > 0.05:
        assert det["loss"] < plain["loss"]
    parts = [scaled_columns(L, probe, x) for x in (xa, xb)]
    cols = np.concatenate([p[0] for p in parts], axis=1)
    wrong = (z.argmax(1) != labels.numpy()).astype(np.uint8)
    mis, _ = dr.table(cols, wrong)
    d = det["detection"]
    assert d["columns"][:3] == ["msp", "entropy", "energy"] and d["n_wrong"] == int(wrong.sum()) == 20 - plain["correct1"]
    for s_, name in enumerate(d["columns"][:3]):
        for k, key in enumerate(("AUROC", "AUPR", "FPR95", "AURC")):
            r, g = mis[s_, k], d["misclassification"][name][key]
            assert (math.isnan(r) and math.isnan(g)) or abs(g - r) <= (EXACT_TOL if key in ("AUROC", "FPR95") else SUM_TOL), (name, key, g, r)
    # the head's own columns do not depend on the temperature
    unscaled = probe.evaluate(batches, detection=True)["detection"]
    for name in d["columns"][3:]:
        assert str(d["misclassification"][name]) == str(unscaled["misclassification"][name]), name

    given = probe.evaluate(batches, temperature=2.0)
    assert given["temperature"] == 2.0 and probe.post_hoc_temperature == fit["T"] and given["correct1"] == plain["correct1"]
    probe.set_temperature(2.0)
    assert probe.evaluate(batches, temperature=True)["loss"] == given["loss"]
    probe.set_temperature(None)
    assert probe.evaluate(batches) == plain and probe._ts_on is None
