"""GPU: conformal prediction sets (csrc/conformal.hip) against the float64 restatement (tests/cp_ref.py), then fit_conformal() and
evaluate_conformal() of the four probes.

On cp_ref.GRID: every label score within the derived delta(K, lam, kreg) of float64; qhat bitwise the k-th order statistic of the
kernel's own score column; per row size_ref(qhat - delta) <= size <= size_ref(qhat + delta) and the same for the covered flag; the
counters and the table equal the metrics recomputed on the host from the kernel's own per-row sizes and flags (counts exactly, ratios
to 1e-12).  The identities that need no tolerance follow.  The worst |error| / delta is printed."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cp_ref as cr
from test_gpu_detect import make_probe
from test_gpu_probe import P, S as STREAM, ok

pytestmark = pytest.mark.gpu

D = C.c_double
WORST = {"score": 0.0}
RATIO_TOL = 1e-12
G, LV = 4, 20                   # counters: 4 global, 20 per level (include/uvit.h)


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def up(z, ld=None):
    """The logits on the device, in rows of ld floats; the padding is NaN: reading it would show."""
    N, K = z.shape
    ld = K if ld is None else ld
    zg = torch.full((N, ld), float("nan"), dtype=torch.float32, device="cuda")
    zg[:, :K] = torch.from_numpy(np.array(z, dtype=np.float32)).cuda()
    return zg, ld


def dev(a, dtype):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def calibrate(L, z, y, u, kind, lam, kreg, alphas=cr.ALPHAS, ld=None):
    """(scores (N,), table (A, 16)) of uvit_op_cp_scores + uvit_op_cp_quantile, on a workspace of exactly the size asked for."""
    N, K = z.shape
    zg, ld = up(z, ld)
    yg, ug = dev(y, np.int64), dev(u, np.float32)
    scores = torch.full((N,), 7.5, dtype=torch.float64, device="cuda")
    ok(L.uvit_op_cp_scores(P(zg), ld, P(yg), P(ug), N, K, cr.KINDS[kind], D(lam), kreg, P(scores), STREAM()))
    A = len(alphas)
    ws_bytes = L.uvit_op_cp_ws_bytes(N, A)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    table = torch.full((A, 16), 7.5, dtype=torch.float64, device="cuda")
    ok(L.uvit_op_cp_quantile(P(scores), N, (D * A)(*alphas), A, P(table), P(ws), ws_bytes, STREAM()))
    torch.cuda.synchronize()
    return scores, table


def sets(L, z, y, u, kind, lam, kreg, table, counters=None, ld=None, finish=True):
    """(sizes (A, B), covered (A, B), counters, finished table) of uvit_op_cp_sets (+ uvit_op_cp_finish) as numpy arrays; `counters`
    (a device tensor) goes on from an earlier batch."""
    B, K = z.shape
    A = table.shape[0]
    zg, ld = up(z, ld)
    yg, ug = dev(y, np.int64), dev(u, np.float32)
    if counters is None:
        n = L.uvit_op_cp_counter_count(K, A)
        assert n == G + LV * A + K * (A + 1)
        counters = torch.zeros(n, dtype=torch.int64, device="cuda")
    sizes = torch.full((A, B), -7, dtype=torch.int32, device="cuda")
    covered = torch.full((A, B), 9, dtype=torch.uint8, device="cuda")
    ok(L.uvit_op_cp_sets(P(zg), ld, P(yg), P(ug), B, K, cr.KINDS[kind], D(lam), kreg, P(table), A, P(counters), P(sizes), P(covered), B, STREAM()))
    out = table.clone()
    if finish:
        ok(L.uvit_op_cp_finish(P(counters), P(out), K, A, STREAM()))
    torch.cuda.synchronize()
    return sizes.cpu().numpy(), covered.cpu().numpy(), counters, out.cpu().numpy()


def check_metrics(counters, table, sizes, covered, y, alphas, K):
    """The counters and the finished table against the metrics recomputed from the kernel's own per-row sizes and flags."""
    c = counters.cpu().numpy()
    A = len(alphas)
    for a, alpha in enumerate(alphas):
        m = cr.metrics(sizes[a], covered[a], y, alpha)
        lv = c[G + LV * a:G + LV * (a + 1)]
        assert (c[0], c[1], c[2]) == (m["n"], m["n_skipped"], 0)
        assert (lv[0], lv[1], lv[2], lv[3]) == (m["covered"], m["size_sum"], m["n_empty"], m["n_singleton"]), (a, lv, m)
        use = sizes[a] >= 0
        bins = np.array([cr.size_bin(int(v)) for v in sizes[a][use]], dtype=np.int64)
        assert lv[5:12].tolist() == np.bincount(bins, minlength=7).tolist()
        assert lv[12:19].tolist() == np.bincount(bins, weights=covered[a][use], minlength=7).astype(np.int64).tolist()
        tot = c[G + LV * A:G + LV * A + K]
        cov = c[G + LV * A + K * (a + 1):G + LV * A + K * (a + 2)]
        assert tot.tolist() == np.bincount(y[use], minlength=K).tolist()
        assert cov.tolist() == np.bincount(y[use], weights=covered[a][use], minlength=K).astype(np.int64).tolist()
        t = table[a]
        assert (t[13], t[14], t[15]) == (m["n"], m["n_skipped"], 0.0)
        if m["n"]:
            assert lv[4] == m["max_size"] == t[10]
            for slot, key in ((6, "coverage"), (7, "size"), (8, "empty"), (9, "singleton"), (11, "sscv"), (12, "worst_class")):
                assert abs(t[slot] - m[key]) <= RATIO_TOL, (a, key, t[slot], m[key])
        else:
            assert np.isnan(t[6:13]).all()


def check_case(L, case, g):
    N, K, scale, kind, with_u = case
    z, y, u, lam, kreg, delta = g["z"], g["y"], g["u"], g["lam"], g["kreg"], g["delta"]
    scores, table = calibrate(L, z, y, u, kind, lam, kreg)
    s, t = scores.cpu().numpy(), table.cpu().numpy()
    # scores within the derived bound
    ratio = float(np.abs(s - g["label_scores"]).max() / delta)
    WORST["score"] = max(WORST["score"], ratio)
    print(f"\n{case}: worst |score error| / delta {ratio:.3f} (delta {delta:.3e}; worst so far {WORST['score']:.3f})")
    assert ratio <= 1.0
    # qhat: bitwise the k-th order statistic of the kernel's own column
    srt = np.sort(s)
    for a, (alpha, cal) in enumerate(zip(cr.ALPHAS, g["cal"])):
        assert (t[a, 0], t[a, 2], t[a, 3], t[a, 4], t[a, 5]) == (alpha, cal["k"], cal["n"], 0.0, cal["status"]), (a, t[a], cal)
        want = np.float64(math.inf) if cal["status"] else srt[cal["k"] - 1]
        assert t[a, 1].tobytes() == want.tobytes(), (a, t[a, 1], want)
        assert (t[a, 6:] == 0.0).all()
    # the calibration rows against their own qhat
    sizes, covered, counters, full = sets(L, z, y, u, kind, lam, kreg, table)
    distinct = np.unique(s).size == N
    for a, cal in enumerate(g["cal"]):
        q = t[a, 1]
        assert np.array_equal(covered[a].astype(bool), s <= q)              # the very score uvit_op_cp_scores wrote
        lo, hi = cr.set_sizes(g["scores"], q - delta), cr.set_sizes(g["scores"], q + delta)
        assert (lo <= sizes[a]).all() and (sizes[a] <= hi).all(), (a, int((sizes[a] - lo).min()), int((hi - sizes[a]).min()))
        cov = covered[a].astype(bool)
        assert (cov | ~(g["label_scores"] <= q - delta)).all() and (~cov | (g["label_scores"] <= q + delta)).all()
        if not cal["status"]:
            assert int(cov.sum()) == cal["k"] if distinct else int(cov.sum()) >= cal["k"]
        else:
            assert (sizes[a] == K).all() and cov.all()
    check_metrics(counters, full, sizes, covered, y, cr.ALPHAS, K)
    # a second call gives the same bits
    scores2, table2 = calibrate(L, z, y, u, kind, lam, kreg)
    sizes2, covered2, counters2, full2 = sets(L, z, y, u, kind, lam, kreg, table2)
    assert scores2.cpu().numpy().tobytes() == s.tobytes() and table2.cpu().numpy().tobytes() == t.tobytes()
    assert sizes2.tobytes() == sizes.tobytes() and covered2.tobytes() == covered.tobytes() and full2.tobytes() == full.tobytes()
    assert torch.equal(counters, counters2)
    return scores, table


@pytest.mark.parametrize("case", cr.GRID, ids=lambda c: "-".join(str(v) for v in c))
def test_against_restatement(L, case):
    check_case(L, case, cr.grid_case(*case))


@pytest.mark.parametrize("case", cr.GRID_PATHS, ids=lambda c: "-".join(str(v) for v in c))
def test_every_padded_size_and_both_workgroup_shapes(L, case):
    """K on both sides of 128 (one wave per row | four), 256, 512, 1024 and 2048 (the padded sizes of the sort)."""
    check_case(L, case, cr.grid_case(*case))


@pytest.mark.parametrize("case", cr.GRID_DENSE, ids=lambda c: "-".join(str(v) for v in c))
def test_dense_lac_cases_keep_the_bounds(L, case):
    """lac over a thousand classes in the flat regime: many classes lie within delta of qhat, the two-sided bound still has to hold."""
    check_case(L, case, cr.grid_case(*case))


@pytest.mark.parametrize("kind,K", [("lac", 10), ("aps", 100), ("raps", 1003)])
def test_batches_add_up_and_the_row_stride_does_not_matter(L, kind, K):
    """64 + 1 + 192 rows give the counters of one batch of 257; ld = K + 3 gives the bits of ld = K."""
    g = cr.grid_case(257, K, 1.0, kind, True) if (257, K, 1.0, kind, True) in cr.GRID else None
    z, y, u = cr.make_inputs(257, K, 1.0)
    lam, kreg = cr.params(kind)
    scores, table = calibrate(L, z, y, u, kind, lam, kreg)
    sizes, covered, counters, full = sets(L, z, y, u, kind, lam, kreg, table)
    run, parts = None, []
    for lo, hi in ((0, 64), (64, 65), (65, 257)):
        sz, cv, run, part = sets(L, z[lo:hi], y[lo:hi], u[lo:hi], kind, lam, kreg, table, counters=run)
        parts.append((sz, cv))
    assert torch.equal(run, counters) and part.tobytes() == full.tobytes()
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), sizes) and np.array_equal(np.concatenate([p[1] for p in parts], axis=1), covered)
    scores3, table3 = calibrate(L, z, y, u, kind, lam, kreg, ld=K + 3)
    assert scores3.cpu().numpy().tobytes() == scores.cpu().numpy().tobytes() and torch.equal(table3, table)
    sizes3, covered3, counters3, full3 = sets(L, z, y, u, kind, lam, kreg, table, ld=K + 3)
    assert sizes3.tobytes() == sizes.tobytes() and covered3.tobytes() == covered.tobytes() and torch.equal(counters3, counters)
    assert g is None or np.abs(scores.cpu().numpy() - g["label_scores"]).max() <= g["delta"]


@pytest.mark.parametrize("kind", ["lac", "aps", "raps"])
def test_non_finite_rows_are_left_out_on_both_sides(L, kind):
    z, y, u = cr.make_inputs(65, 100, 1.0)
    z = z.copy()
    z[0, 3], z[31, 0], z[64, 99] = np.nan, np.inf, -np.inf
    lam, kreg = cr.params(kind)
    keep = np.ones(65, dtype=bool)
    keep[[0, 31, 64]] = False
    scores, table = calibrate(L, z, y, u, kind, lam, kreg)
    s, t = scores.cpu().numpy(), table.cpu().numpy()
    clean, tclean = calibrate(L, z[keep], y[keep], u[keep], kind, lam, kreg)
    assert np.isnan(s[~keep]).all() and s[keep].tobytes() == clean.cpu().numpy().tobytes()
    tc = tclean.cpu().numpy()
    assert (t[:, 3] == 62).all() and (t[:, 4] == 3).all() and t[:, 1].tobytes() == tc[:, 1].tobytes() and np.array_equal(t[:, 2], tc[:, 2])
    sizes, covered, counters, full = sets(L, z, y, u, kind, lam, kreg, table)
    sizes_c, covered_c, counters_c, full_c = sets(L, z[keep], y[keep], u[keep], kind, lam, kreg, table)
    assert (sizes[:, ~keep] == -1).all() and (covered[:, ~keep] == 0).all()
    assert np.array_equal(sizes[:, keep], sizes_c) and np.array_equal(covered[:, keep], covered_c)
    c, cc = counters.cpu().numpy(), counters_c.cpu().numpy()
    assert (c[0], c[1], c[2]) == (62, 3, 0) and np.array_equal(c[3:], cc[3:])
    assert (full[:, 13] == 62).all() and (full[:, 14] == 3).all() and full[:, 6:13].tobytes() == full_c[:, 6:13].tobytes()
    check_metrics(counters, full, sizes, covered, y, cr.ALPHAS, 100)


def test_a_bad_label_turns_the_table_to_nan(L):
    z, y, u = cr.make_inputs(65, 10, 1.0)
    for bad in (10, -1, 1 << 40):
        yb = y.copy()
        yb[17] = bad
        scores, table = calibrate(L, z, yb, None, "aps", 0.0, 0)
        s = scores.cpu().numpy()
        assert np.isnan(s[17]) and not np.isnan(np.delete(s, 17)).any() and np.isnan(table.cpu().numpy()).all()
        _, good = calibrate(L, z, y, None, "aps", 0.0, 0)
        sizes, covered, counters, full = sets(L, z, yb, None, "aps", 0.0, 0, good)
        assert counters.cpu().numpy()[:3].tolist() == [64, 0, 1] and sizes[0, 17] == -1 and np.isnan(full[:, 6:13]).all()


def test_ties_inside_a_row_follow_the_index_rule(L):
    """All-equal logits: class j has rank j + 1 and the aps score (j + 1) / K, so a threshold of 1 / 2 keeps the first K / 2 classes and
    covers the labels among them; lac gives every class the score 1 - 1 / K: all or nothing."""
    K = 6
    z = np.zeros((K, K), dtype=np.float32)
    z[3] = -0.0
    z[4, ::2] = -0.0                                    # +0 == -0
    y = np.arange(K)
    table = torch.zeros(2, 16, dtype=torch.float64, device="cuda")
    table[0, 0], table[0, 1], table[1, 0], table[1, 1] = 0.1, 0.5 + 1e-12, 0.3, 1.0 / 3.0 + 1e-12
    sizes, covered, _, _ = sets(L, z, y, None, "aps", 0.0, 0, table)
    assert (sizes[0] == 3).all() and (sizes[1] == 2).all()
    assert covered[0].tolist() == [1, 1, 1, 0, 0, 0] and covered[1].tolist() == [1, 1, 0, 0, 0, 0]
    sizes, covered, _, _ = sets(L, z, y, None, "raps", 0.25, 1, table)                 # + 0.25 (rank - 1): only rank 1 stays below 1 / 2
    assert (sizes[0] == 1).all() and (sizes[1] == 1).all() and covered[0].tolist() == [1, 0, 0, 0, 0, 0]
    table[0, 1], table[1, 1] = 1.0 - 1.0 / K + 1e-12, 1.0 - 1.0 / K - 1e-12
    sizes, covered, _, _ = sets(L, z, y, None, "lac", 0.0, 0, table)
    assert (sizes[0] == K).all() and covered[0].all() and (sizes[1] == 0).all() and not covered[1].any()
    scores, _ = calibrate(L, z, y, None, "aps", 0.0, 0)
    assert np.abs(scores.cpu().numpy() - np.arange(1, K + 1) / K).max() <= cr.delta(K)


@pytest.mark.parametrize("kind,K", [("lac", 10), ("aps", 65), ("raps", 1003)])
def test_too_few_rows_give_full_sets(L, kind, K):
    z, y, u = cr.make_inputs(3, K, 1.0)
    lam, kreg = cr.params(kind)
    _, table = calibrate(L, z, y, u, kind, lam, kreg, alphas=(0.1, 0.3))               # k = 4 > 3 | k = 3
    t = table.cpu().numpy()
    assert (t[0, 1], t[0, 2], t[0, 5]) == (math.inf, 4, 1) and (t[1, 2], t[1, 5]) == (3, 0) and math.isfinite(t[1, 1])
    ze, ye, ue = cr.make_inputs(65, K, 3.0, seed=1)
    sizes, covered, counters, full = sets(L, ze, ye, ue, kind, lam, kreg, table)
    assert (sizes[0] == K).all() and covered[0].all() and full[0, 6] == 1.0 and full[0, 7] == K and full[0, 10] == K
    check_metrics(counters, full, sizes, covered, ye, (0.1, 0.3), K)


# ---- the module ----
@pytest.fixture(scope="module")
def case(golden_dir):
    import probe_ref as pr
    return pr.load_fixture(golden_dir)


def test_module_on_caller_supplied_logits(L, case):
    """conformal_calibrate / conformal_sets equal the direct calls; raps at lam = 0 equals aps bit for bit."""
    probe = make_probe(case, "linear")
    z, y, u = cr.make_inputs(257, probe.num_classes, 1.0)
    zg, yg, ug = dev(z, np.float32), dev(y, np.int64), dev(u, np.float32)
    for kind in ("lac", "aps", "raps"):
        lam, kreg = cr.params(kind)
        st = probe.conformal_calibrate(zg, yg, alpha=list(cr.ALPHAS), score=kind, lam=lam, kreg=kreg, u=ug)
        scores, table = calibrate(L, z, y, u, kind, lam, kreg)
        assert torch.equal(st["scores"], scores) and torch.equal(st["table"], table)
        out = probe.conformal_sets(zg, yg, st, u=ug)
        sizes, covered, counters, full = sets(L, z, y, u, kind, lam, kreg, table)
        assert np.array_equal(out["sizes"].cpu().numpy(), sizes) and np.array_equal(out["covered"].cpu().numpy(), covered)
        assert torch.equal(out["counters"], counters) and out["table"].cpu().numpy().tobytes() == full.tobytes()
    a = probe.conformal_calibrate(zg, yg, score="aps", u=ug)
    b = probe.conformal_calibrate(zg, yg, score="raps", lam=0.0, kreg=5, u=ug)
    assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["table"], b["table"])
    assert probe.conformal is None


@pytest.mark.parametrize("kind", ["linear", "gp", "het", "ens"])
def test_fit_and_evaluate_end_to_end(L, case, kind):
    """Two ragged batches: fit_conformal equals the restatement's calibration on the head's own logits; evaluate_conformal on the same
    batches covers exactly k rows; the sizes go through detection_batch; the state is not in state_dict()."""
    from uncertainty_vit_amd.native import UvitError
    _, _, _, _, _, images, _ = case
    probe = make_probe(case, kind)
    keys = list(probe.state_dict())
    x4 = images.cuda()
    pool = torch.cat([x4, x4.flip(-1), x4.flip(-2), 0.5 * x4 + 0.25, x4.transpose(-1, -2).contiguous(), 0.7 * x4 - 0.1])
    xa, xb = pool[:13].contiguous(), pool[13:20].contiguous()
    z = np.concatenate([probe.logits(xa).cpu().numpy(), probe.logits(xb).cpu().numpy()])
    pred = torch.from_numpy(z.argmax(1))
    labels = torch.where(torch.arange(len(pred)) % 3 != 2, pred, (pred + 1) % probe.num_classes)      # every third prediction is wrong
    batches = [((xa, None), labels[:13]), ((xb, None), labels[13:])]
    with pytest.raises(UvitError):
        probe.evaluate_conformal(batches)
    K, y = probe.num_classes, labels.numpy()
    if kind == "het":
        # the Monte-Carlo logits of an evaluation are drawn per call: compare with what the same call order gives
        z = None
    for score in ("lac", "aps"):
        fit = probe.fit_conformal(batches, alpha=[0.1, 0.3], score=score)
        assert fit["n"] == 20 and fit["n_skipped"] == 0 and fit["alpha"] == [0.1, 0.3] and fit["score"] == score and fit["n_rows"] == 20
        assert fit["k"] == [math.ceil(21 * 0.9), math.ceil(21 * 0.7)] and fit["status"] == [0, 0]
        if z is not None:
            sy = cr.label_scores(z, y, score)
            for a, alpha in enumerate((0.1, 0.3)):
                assert abs(fit["qhat"][a] - cr.quantile(sy, alpha)["qhat"]) <= cr.delta(K), (score, alpha)
        res = probe.evaluate_conformal(batches, sizes=True)
        conf, sizes = res["conformal"], res["sizes"]
        assert sizes.shape == (2, 20) and sizes.dtype == torch.int32 and sizes.is_cuda
        for a, alpha in enumerate((0.1, 0.3)):
            c = conf[alpha]
            print(f"\n{kind} {score} alpha {alpha}: {c}")
            assert c["n"] == 20 and c["n_skipped"] == 0 and c["qhat"] == fit["qhat"][a]
            if kind != "het":
                assert c["coverage"] >= fit["k"][a] / 20 and c["coverage"] >= 1.0 - alpha      # the calibration rows themselves
            assert abs(c["size"] - float(sizes[a].sum()) / 20) <= RATIO_TOL and c["max_size"] == int(sizes[a].max())
            assert 0.0 <= c["sscv"] <= 1.0 and 0.0 <= c["worst_class"] <= c["coverage"] + RATIO_TOL
        assert (conf[0.1]["size"] >= conf[0.3]["size"])                                # sets grow as alpha shrinks
    # set size as an uncertainty column: wrong predictions against right ones
    wrong = torch.from_numpy((probe.logits(pool[:20].contiguous()).argmax(1).cpu().numpy() != y).astype(np.uint8)).cuda()
    det = probe.detection_batch(res["sizes"].to(torch.float32), wrong).cpu().numpy()
    assert 0 < int(wrong.sum()) < 20 and np.isfinite(det[:, 0]).all() and ((0.0 <= det[:, 0]) & (det[:, 0] <= 1.0)).all()
    # the temperature reaches both sides; the state is a plain attribute
    t2 = probe.fit_conformal(batches, alpha=0.1, score="lac", temperature=2.0)
    t1 = probe.fit_conformal(batches, alpha=0.1, score="lac")
    if kind != "het":
        assert t2["qhat"] != t1["qhat"]
    assert list(probe.state_dict()) == keys and probe._ts_on is None
    probe.set_conformal(None)
    with pytest.raises(UvitError):
        probe.evaluate_conformal(batches)


def test_duplicated_rows_cover_at_least_k(L):
    z, y, _ = cr.make_inputs(65, 10, 1.0)
    z, y = np.concatenate([z, z[:31]]), np.concatenate([y, y[:31]])
    scores, table = calibrate(L, z, y, None, "aps", 0.0, 0)
    s, t = scores.cpu().numpy(), table.cpu().numpy()
    assert np.unique(s).size == 65
    _, covered, _, _ = sets(L, z, y, None, "aps", 0.0, 0, table)
    for a in range(2):
        k = int(t[a, 2])
        assert t[a, 1] == np.sort(s)[k - 1] and int(covered[a].sum()) >= k and np.array_equal(covered[a].astype(bool), s <= t[a, 1])


def test_quantile_of_a_long_column_with_ties_and_eight_levels(L):
    """300 000 scores (more than the 1024 x 256 one sweep of the histogram grid holds), a third of them duplicated, NaN rows among
    them, zeros at the low end, eight levels in one call: every qhat is bitwise numpy's order statistic."""
    rng = np.random.default_rng(3)
    N = 300_000
    s = rng.random(N) * rng.choice([1.0, 1e-3, 1.5], size=N)
    s[rng.integers(0, N, N // 3)] = s[rng.integers(0, N, N // 3)]
    s[rng.integers(0, N, 500)] = 0.0
    s[rng.integers(0, N, 77)] = np.nan
    alphas = (0.001, 0.05, 0.1, 0.3, 0.5, 0.9, 0.999, 0.999999)
    sg = torch.from_numpy(s).cuda()
    ws_bytes = L.uvit_op_cp_ws_bytes(N, 8)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    tables = []
    for _ in range(2):
        table = torch.full((8, 16), 7.5, dtype=torch.float64, device="cuda")
        ok(L.uvit_op_cp_quantile(P(sg), N, (D * 8)(*alphas), 8, P(table), P(ws), ws_bytes, STREAM()))
        torch.cuda.synchronize()
        tables.append(table.cpu().numpy())
    t = tables[0]
    assert tables[1].tobytes() == t.tobytes()
    good = np.sort(s[~np.isnan(s)])
    for a, alpha in enumerate(alphas):
        ref = cr.quantile(s, alpha)
        assert (t[a, 0], t[a, 2], t[a, 3], t[a, 4], t[a, 5]) == (alpha, ref["k"], good.size, N - good.size, 0)
        assert t[a, 1].tobytes() == np.float64(good[ref["k"] - 1]).tobytes(), (alpha, t[a, 1], good[ref["k"] - 1])


def test_randomized_fit_is_seeded(case):
    """`randomized` draws u on the device: the same seed gives the same table, another seed or no u another one; aps with u < 1 scores
    every label lower than without (u p_y < p_y), so qhat does not grow."""
    _, _, _, _, _, images, _ = case
    probe = make_probe(case, "linear")
    x4 = images.cuda()
    xa = torch.cat([x4, x4.flip(-1), x4.flip(-2), 0.5 * x4 + 0.25]).contiguous()
    labels = probe.logits(xa).argmax(1).cpu()
    batches = [((xa[:9].contiguous(), None), labels[:9]), ((xa[9:].contiguous(), None), labels[9:])]
    plain = probe.fit_conformal(batches, alpha=0.3, score="aps")
    a = probe.fit_conformal(batches, alpha=0.3, score="aps", randomized=True, seed=5)
    b = probe.fit_conformal(batches, alpha=0.3, score="aps", randomized=True, seed=5)
    c = probe.fit_conformal(batches, alpha=0.3, score="aps", randomized=True, seed=6)
    assert a == b and a["randomized"] and a["seed"] == 5 and a["qhat"] != c["qhat"] and a["qhat"][0] < plain["qhat"][0]
    r1, r2 = probe.evaluate_conformal(batches), probe.evaluate_conformal(batches)
    assert r1 == r2 and r1["conformal"][0.3]["n"] == 16
