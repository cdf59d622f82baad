"""GPU: the calibration ops (csrc/calib.hip) one by one against the float64 restatement (tests/calib_ref.py) on the GPU's own
probabilities, on crafted probabilities (ties, exact bin edges), and through LinearProbe against the reference's stored numbers
(tests/golden/calib.npz).  Every output sits in front of guard elements that no kernel may touch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import calib_ref as cr
from oracle.closed_form import closed_form_images

pytestmark = pytest.mark.gpu

SHAPES = [(1, 10), (7, 200), (29, 10), (30, 10), (37, 10), (64, 1003), (192, 1000), (1024, 3)]
ECE_BINS, TACE_BINS, THR = 15, 30, 0.01
ATOL = 1e-9            # fp64 sums of at most 1024 terms in [0, 1]: round-off near 1e-13; one misplaced sample moves a bin by >= 1 / 1024
GUARD = 64
FILL = {torch.float32: 7.5, torch.float64: 7.5, torch.int32: 7777}


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "calib.npz"))


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(n, dtype=torch.float64):
    """n elements on the device followed by GUARD sentinels that no kernel may touch; the n elements hold the sentinel too."""
    return torch.full((n + GUARD,), FILL[dtype], dtype=dtype, device="cuda")


def intact(t, n):
    return bool((t[n:] == FILL[t.dtype]).all())


def untouched(t):
    return bool((t == FILL[t.dtype]).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


# ---- inputs ----
def calib_logits(B, K):
    """Logits of spread 2.5; row 0 is lifted by 90 (softmax does not change; exp overflows fp32 without the max shift)."""
    z = torch.randn(B, K, generator=torch.Generator().manual_seed(31 + B + K)) * 2.5
    z[0] += 90.0
    return z


def calib_labels(z):
    """Labels that follow the row maximum two times in three, and contain class 0 and class K - 1 when there is room."""
    B, K = z.shape
    g = torch.Generator().manual_seed(32 + B + K)
    y = torch.where(torch.rand(B, generator=g) < 0.66, z.argmax(1), torch.randint(0, K, (B,), generator=g))
    if B >= 3:
        y[1], y[2] = 0, K - 1
    return y.to(torch.int64)


# ---- the ops, each on its own; every call returns (rc, outputs) and checks the guards ----
def run_softmax(L, z):
    B, K = z.shape
    zg, out = z.cuda(), guarded(B * K, torch.float32)
    rc = L.uvit_op_calib_softmax(P(zg), P(out), B, K, S())
    torch.cuda.synchronize()
    assert intact(out, B * K)
    return rc, out


def run_confidence(L, p, y, n_bins, pos):
    B, K = p.shape
    pg, yg = p.cuda(), y.cuda()
    o = {"conf": guarded(B, torch.float32), "pred": guarded(2 * B, torch.int32), "nll_rows": guarded(B), "table": guarded(3 * n_bins),
         "ece_nll": guarded(2)}
    bounds = np.linspace(0, 1, n_bins + 1)
    rc = L.uvit_op_calib_confidence(P(pg), P(yg), bounds.ctypes.data_as(C.c_void_p), n_bins, int(pos), P(o["conf"]), P(o["pred"]), P(o["nll_rows"]),
                                    P(o["table"]), P(o["ece_nll"]), B, K, S())
    torch.cuda.synchronize()
    sizes = {"conf": B, "pred": 2 * B, "nll_rows": B, "table": 3 * n_bins, "ece_nll": 2}
    assert all(intact(o[k], n) for k, n in sizes.items())
    return rc, o, sizes


def run_tace(L, p, y, thr, n_bins, pos):
    B, K = p.shape
    pg, yg = p.cuda(), y.cuda()
    o = {"per_class": guarded(K), "tace": guarded(1)}
    rc = L.uvit_op_calib_tace(P(pg), P(yg), C.c_double(thr), n_bins, int(pos), P(o["per_class"]), P(o["tace"]), B, K, S())
    torch.cuda.synchronize()
    sizes = {"per_class": K, "tace": 1}
    assert all(intact(o[k], n) for k, n in sizes.items())
    return rc, o, sizes


def run_auroc(L, p, y):
    B, K = p.shape
    pg, yg = p.cuda(), y.cuda()
    o = {"rows": guarded(3 * B, torch.int32), "out": guarded(2)}
    rc = L.uvit_op_calib_auroc(P(pg), P(yg), P(o["rows"]), P(o["out"]), B, K, S())
    torch.cuda.synchronize()
    sizes = {"rows": 3 * B, "out": 2}
    assert all(intact(o[k], n) for k, n in sizes.items())
    return rc, o, sizes


def host(o, sizes, key):
    return o[key][:sizes[key]].cpu().numpy()


def check_metric_ops(L, p, y, ece_bins, tace_bins, thr, what, pos=True):
    """The three metric ops on probabilities p (fp32 host tensor) against calib_ref on the same values, in the reading `pos` of the
    bin accuracy (True: the reference's positional one): sums within ATOL, NLL within 1e-9 relative, integers exact; a second
    call gives the same bits in every output."""
    B, K = p.shape
    pn, yn = p.numpy(), y.numpy()
    ref_c, (ref_t, ref_pc), ref_a = cr.confidence(pn, yn, ece_bins, pos), cr.tace(pn, yn, thr, tace_bins, pos), cr.auroc(pn, yn)
    runs = []
    for _ in range(2):
        rc, oc, sc = run_confidence(L, p, y, ece_bins, pos)
        assert rc == 0
        rt, ot, st = run_tace(L, p, y, thr, tace_bins, pos)
        assert rt == 0
        ra, oa, sa = run_auroc(L, p, y)
        assert ra == 0
        runs.append([bits(o[k][:s[k]]) for o, s in ((oc, sc), (ot, st), (oa, sa)) for k in s])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two calls on the same input differ"
    # confidence
    assert np.array_equal(host(oc, sc, "conf").astype(np.float64), ref_c["conf"])                 # the row maximum: exact
    pred = host(oc, sc, "pred")
    assert np.array_equal(pred[:B], ref_c["pred"]) and np.array_equal(pred[B:], ref_c["correct"])
    table = host(oc, sc, "table").reshape(ece_bins, 3)
    ece, nll = host(oc, sc, "ece_nll")
    e_tab, e_ece = float(np.abs(table - ref_c["table"]).max()), abs(ece - ref_c["ECE"])
    e_rows = float((np.abs(host(oc, sc, "nll_rows") - ref_c["nll_rows"]) / np.abs(ref_c["nll_rows"])).max())
    e_nll = abs(nll - ref_c["NLL"]) / abs(ref_c["NLL"])
    # tace
    per_class, tace = host(ot, st, "per_class"), float(host(ot, st, "tace")[0])
    e_pc, e_tace = float(np.abs(per_class - ref_pc).max()), abs(tace - ref_t)
    # auroc
    rows, (asum, acount) = host(oa, sa, "rows").reshape(3, B), host(oa, sa, "out")
    e_auc = abs(asum - ref_a["sum"])
    print(f"\n{what}: table {e_tab:.1e} ECE {e_ece:.1e} NLL rows {e_rows:.1e} NLL {e_nll:.1e} per-class {e_pc:.1e} TACE {e_tace:.1e} "
          f"AUROC sum {e_auc:.1e} (count {int(acount)}); ECE {ece:.6f} TACE {tace:.6f} NLL {nll:.6f}")
    assert e_tab <= ATOL and e_ece <= ATOL
    assert e_rows <= 1e-9 and e_nll <= 1e-9
    assert e_pc <= ATOL and e_tace <= ATOL
    assert np.array_equal(rows[0], ref_a["u2"]) and np.array_equal(rows[1], ref_a["n_pos"]) and np.array_equal(rows[2], ref_a["first"])
    assert acount == ref_a["count"] and e_auc <= ATOL
    return ref_c, ref_a


# ---- softmax ----
# torch's own fp32 CPU softmax against float64 on calib_logits(B, K): (max-norm error / max|ref|, relative L2 error)
CPU_ERR = {
    "softmax": {(1, 10): (3.74e-8, 3.74e-8), (7, 200): (2.74e-8, 3.18e-8), (29, 10): (8.63e-8, 5.98e-8), (30, 10): (9.39e-8, 6.47e-8),
                (37, 10): (1.49e-7, 7.20e-8), (64, 1003): (9.64e-8, 7.73e-8), (192, 1000): (1.64e-7, 9.07e-8),
                (1024, 3): (1.34e-7, 4.47e-8)},
}


def metrics(got, ref):
    """(max-norm error / max|ref|, relative L2 error) against a float64 reference."""
    d = got.detach().cpu().double() - ref
    return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())


@pytest.mark.parametrize("B,K", SHAPES)
def test_softmax(L, B, K):
    """probs = softmax(logits) against float64 under the project's rule for fp32 kernels (tests/test_gpu_probe.py): the GPU's
    max-norm and relative-L2 errors are at most 4 x those of torch's own fp32 CPU softmax on the same logits (CPU_ERR above; the
    test prints what the CPU it runs on gives).  Rows sum to 1 within fp32 round-off; two calls give the same bits."""
    z = calib_logits(B, K)
    ref = torch.from_numpy(cr.softmax(z.numpy()))
    rc, out = run_softmax(L, z)
    assert rc == 0
    rc2, out2 = run_softmax(L, z)
    assert rc2 == 0 and torch.equal(bits(out), bits(out2))
    got = out[:B * K].view(B, K).cpu()
    m, now, lit = metrics(got, ref), metrics(torch.softmax(z, dim=1), ref), CPU_ERR["softmax"][(B, K)]
    print(f"\nsoftmax {(B, K)}: GPU (max-norm, rel L2) = ({m[0]:.3e}, {m[1]:.3e}); fp32 CPU here ({now[0]:.3e}, {now[1]:.3e}), recorded {lit}")
    assert bool(torch.isfinite(got).all()) and float((got.double().sum(1) - 1.0).abs().max()) <= 1e-5
    assert m[0] <= 4 * lit[0] and m[1] <= 4 * lit[1], ((B, K), m, lit)


# ---- the metric ops on the GPU's own probabilities ----
@pytest.mark.parametrize("pos", [True, False])
@pytest.mark.parametrize("B,K", SHAPES)
def test_metric_ops_on_gpu_probabilities(L, B, K, pos):
    """Softmax on the GPU, read back, and the three ops against calib_ref on those very fp32 values: memberships are the same by
    construction (fp32 widened to double, double bounds), so ECE, TACE, every per_class[c], the bin table and the AUROC sum agree
    within 1e-9 absolute, NLL within 1e-9 relative, and every integer output exactly.  Both readings of the bin accuracy: the
    reference's positional one (pos) and the mean over the rows of the bin."""
    z = calib_logits(B, K)
    y = calib_labels(z)
    rc, out = run_softmax(L, z)
    assert rc == 0
    p = out[:B * K].view(B, K).cpu()
    check_metric_ops(L, p, y, ECE_BINS, TACE_BINS, THR, f"gpu probs {(B, K)} positional {pos}", pos)


def test_batch_above_the_limit_is_refused(L):
    """B = 1025: every op returns UVIT_ERR_SHAPE and leaves its outputs untouched."""
    B, K = 1025, 3
    z = calib_logits(B, K)
    y = calib_labels(z)
    rc, out = run_softmax(L, z)
    assert rc == -2 and untouched(out)
    p = torch.softmax(z, dim=1)
    for rc, o, _ in (run_confidence(L, p, y, ECE_BINS, 1), run_tace(L, p, y, THR, TACE_BINS, 1), run_auroc(L, p, y)):
        assert rc == -2 and all(untouched(t) for t in o.values())


# ---- crafted probabilities on the 1/64 grid, handed straight to the ops ----
def crafted(fx):
    """Six rows made by hand in front of the fixture's grid case (K = 10): conf == 0.5, two one-hot rows (conf == 1.0, one right, one
    wrong), two tied row maxima (label on the higher / on the lower index) and a row of eight 1/16 with a tied maximum of 1/4."""
    name = str(fx["names"][-1])
    g, yg = fx["probs/" + name], fx["labels/" + name]
    r = np.zeros((6, 10), dtype=np.float32)
    r[0, :3] = (0.5, 0.25, 0.25)
    r[1, 3] = 1.0
    r[2, 9] = 1.0
    r[3, 1:3] = 0.5
    r[4, 0] = r[4, 3] = 0.5
    r[5, :8], r[5, 8:] = 0.0625, 0.25
    y = np.array([0, 3, 0, 2, 0, 8], dtype=np.int64)
    p = np.concatenate([r, g])
    assert np.array_equal(p * 64, np.round(p * 64)) and bool((p.astype(np.float64).sum(1) == 1.0).all())
    return torch.from_numpy(p), torch.from_numpy(np.concatenate([y, yg]))


@pytest.mark.parametrize("pos", [True, False])
@pytest.mark.parametrize("tace_bins", [8, 30, 64])
def test_crafted_probabilities(L, fx, tace_bins, pos):
    """Columns full of ties and of values under the threshold (0.0625 = 4/64: the values 1/64 .. 3/64 and the zeros fall under it, a
    value of exactly 4/64 does not), values exactly on an adaptive bound (every bound is a column element, most of them repeated)
    and on the last upper bound 1.0, 16 ECE bins with conf == 0.5 in (0.4375, 0.5] and conf == 1.0 in the last bin, and tied row
    maxima: the lowest index wins.  46 rows: bin_n = 5, 1 and 0 for 8, 30 and 64 bins.  The gates of the test above."""
    p, y = crafted(fx)
    assert int((p == 0.0625).sum()) > 0 and int(((p > 0) & (p < 0.0625)).sum()) > 10
    ref_c, _ = check_metric_ops(L, p, y, 16, tace_bins, 0.0625, f"crafted, {tace_bins} TACE bins, positional {pos}", pos)
    assert ref_c["table"][7, 0] >= 1 / 46 and ref_c["table"][15, 0] >= 2 / 46          # conf == 0.5 -> bin 7, conf == 1.0 -> bin 15
    assert ref_c["pred"][:6].tolist() == [0, 3, 9, 1, 0, 8] and ref_c["correct"][:6].tolist() == [1, 1, 0, 0, 1, 1]


def test_all_labels_equal(L, fx):
    """One class only: no class has a negative row, the AUROC sum is 0 and the count 0; the other outputs stay as calib_ref has them."""
    p, y = crafted(fx)
    y = torch.full_like(y, 3)
    _, ref_a = check_metric_ops(L, p, y, 16, 30, 0.0625, "all labels equal")
    assert ref_a["count"] == 0 and ref_a["sum"] == 0.0


@pytest.mark.parametrize("bad", [-1, 10])
def test_label_out_of_range(L, fx, bad):
    """A label of -1 and one of K: ECE, NLL, TACE and the AUROC sum are NaN, that row's NLL is NaN and its integer outputs are zero,
    the rows beside it and the per-class values are finite and what calib_ref gives, and the guards are intact (run_* check them)."""
    p, y = crafted(fx)
    B, K = p.shape
    yb = y.clone()
    yb[4] = bad
    pn, yn = p.numpy(), yb.numpy()
    assert bool(torch.isfinite(p).all())
    rc, oc, sc = run_confidence(L, p, yb, 16, 1)
    rt, ot, st = run_tace(L, p, yb, 0.0625, 30, 1)
    ra, oa, sa = run_auroc(L, p, yb)
    assert (rc, rt, ra) == (0, 0, 0)
    ece, nll = host(oc, sc, "ece_nll")
    asum, acount = host(oa, sa, "out")
    assert np.isnan(ece) and np.isnan(nll) and np.isnan(host(ot, st, "tace")[0]) and np.isnan(asum)
    rows_nll = host(oc, sc, "nll_rows")
    keep = [i for i in range(B) if i != 4]
    ref_c, (_, ref_pc), ref_a = cr.confidence(pn, yn, 16, True), cr.tace(pn, yn, 0.0625, 30, True), cr.auroc(pn, yn)
    assert np.isnan(rows_nll[4]) and bool(np.isfinite(rows_nll[keep]).all())
    assert float((np.abs(rows_nll[keep] - ref_c["nll_rows"][keep]) / np.abs(ref_c["nll_rows"][keep])).max()) <= 1e-9
    pred = host(oc, sc, "pred")
    assert np.array_equal(pred[:B], ref_c["pred"]) and np.array_equal(pred[B:], ref_c["correct"]) and pred[B + 4] == 0
    assert float(np.abs(host(oc, sc, "table").reshape(16, 3) - ref_c["table"]).max()) <= ATOL
    per_class = host(ot, st, "per_class")
    assert bool(np.isfinite(per_class).all()) and float(np.abs(per_class - ref_pc).max()) <= ATOL
    rows = host(oa, sa, "rows").reshape(3, B)
    assert rows[:, 4].tolist() == [0, 0, 0]
    assert np.array_equal(rows[0], ref_a["u2"]) and np.array_equal(rows[1], ref_a["n_pos"]) and np.array_equal(rows[2], ref_a["first"])
    assert acount == ref_a["count"]


# ---- LinearProbe ----
@pytest.fixture(scope="module")
def case(golden_dir):
    import probe_ref as pr
    return pr.load_fixture(golden_dir)


def gpu_probs(L, logits):
    rc, out = run_softmax(L, logits.cpu())
    assert rc == 0
    return out[:logits.numel()].view(logits.shape).cpu().numpy()


def test_evaluate_with_calibration(L, case):
    """evaluate(calibration=True) over batches of 4, 4 and 3 images (K = 10; the last batch carries one class only, so it has no
    AUROC): ECE and TACE (with the reference's bin accuracy), NLL and AUROC are calib_ref's per-batch values on the GPU's own softmax
    of probe.logits(), weighted by batch size (the batch without an AUROC left out of that mean only), within 1e-9; the keys of the plain evaluate() come back with the
    same values, and evaluate() without the flag returns exactly its six keys."""
    from test_gpu_probe import fixture_probe
    _, cfg, _, W, _, _, _ = case
    K = W.shape[0]
    probe = fixture_probe(case)
    labels = [torch.tensor([0, 9, 3, 6]), torch.tensor([2, 2, 7, 5]), torch.tensor([4, 4, 4])]
    batches = [((closed_form_images(f"calib-eval/{i}", len(y), cfg.img_size).cuda(), None), y) for i, y in enumerate(labels)]
    per_batch = [cr.batch_metrics(gpu_probs(L, probe.logits(x)), y.numpy(), positional_acc=True) for (x, _), y in batches]
    assert [m["auroc_count"] for m in per_batch][2] == 0 and per_batch[0]["auroc_count"] == 4
    want = cr.weighted(per_batch, [4, 4, 3], K)
    plain = probe.evaluate(batches)
    assert set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"} and plain["n"] == 11
    out = probe.evaluate(batches, calibration=True)
    assert set(out) == set(plain) | {"ECE", "TACE", "NLL", "AUROC", "AUROC_zero_absent"}
    assert all(out[k] == plain[k] for k in plain)
    for k in ("ECE", "TACE", "NLL", "AUROC", "AUROC_zero_absent"):
        print(f"\nevaluate {k}: {out[k]:.9f}, calib_ref {want[k]:.9f}")
        assert out[k] == pytest.approx(want[k], abs=1e-9, rel=1e-9 if k == "NLL" else 0), k
    again = probe.evaluate(batches)
    assert again == plain


def fixture_calibration(case, fx, name, reference_bin_accuracy=True):
    from test_gpu_probe import fixture_probe
    probe = fixture_probe(case)
    z, y = torch.from_numpy(fx["logits/" + name]), torch.from_numpy(fx["labels/" + name])
    if z.shape[1] != probe.num_classes:
        from uncertainty_vit_amd.linear_probe import LinearProbe
        probe = LinearProbe(probe.encoder, z.shape[1])
    ece, tace, nll, auroc = (float(v) for v in probe.calibration_batch(z.cuda(), y.cuda(), reference_bin_accuracy=reference_bin_accuracy))
    return ece, tace, nll, auroc, probe


def logit_cases(fx):
    return [str(n) for n in fx["names"] if "logits/" + str(n) in fx.files]


def test_calibration_batch_against_reference_fixture(case, fx):
    """calibration_batch on the fixture's logits, end to end (GPU softmax included), against the unmodified reference classes' own
    numbers: ECE and TACE within 1e-6 (the fixture keeps every probability 1e-6 clear of the bounds it is compared with, so the GPU's
    softmax and torch's give the same memberships), the bin table within 1e-6 of the reference's ECE object, NLL within 1e-5
    relative of the reference's NLL(logits, y), AUROC within 1e-6 of the mean of scikit-learn's per-class values."""
    worst = []
    for name in logit_cases(fx):
        ece, tace, nll, auroc, probe = fixture_calibration(case, fx, name)
        e, t = ece - float(fx["ece/" + name]), tace - float(fx["tace/" + name])
        ref_auc = float(np.nanmean(fx["auroc/" + name]))
        print(f"\n{name}: kernel - reference: ECE {e:+.3e}, TACE {t:+.3e}; NLL {nll:.9f} ({float(fx['nll/' + name]):.9f}) "
              f"AUROC {auroc:.9f} ({ref_auc:.9f})")
        worst.append((name, e, t))
        table = probe._bin_table[:3 * ECE_BINS].cpu().numpy().reshape(ECE_BINS, 3)
        assert float(np.abs(table - fx["ece_bins/" + name]).max()) <= 1e-6
        assert abs(nll - float(fx["nll/" + name])) <= 1e-5 * float(fx["nll/" + name])
        assert abs(auroc - ref_auc) <= 1e-6
    assert all(abs(e) <= 1e-6 and abs(t) <= 1e-6 for _, e, t in worst), worst


def test_calibration_batch_with_the_mean_over_the_bin(case, fx):
    """reference_bin_accuracy=False: ECE and TACE with the mean over the rows of each bin, within 1e-6 of calib_ref on the fixture's
    probabilities, and not the reference's numbers (they differ by 0.05 to 0.30 in ECE on these cases)."""
    for name in logit_cases(fx):
        ece, tace, _, _, _ = fixture_calibration(case, fx, name, reference_bin_accuracy=False)
        m = cr.batch_metrics(fx["probs/" + name], fx["labels/" + name])
        print(f"\n{name}: ECE {ece:.9f} ({m['ECE']:.9f}) TACE {tace:.9f} ({m['TACE']:.9f}); reference's {float(fx['ece/' + name]):.6f}")
        assert abs(ece - m["ECE"]) <= 1e-6 and abs(tace - m["TACE"]) <= 1e-6
        assert abs(ece - float(fx["ece/" + name])) > 1e-2


def test_calibration_batch_refuses_what_it_cannot_run(case):
    from test_gpu_probe import fixture_probe
    from uncertainty_vit_amd.native import UvitError
    probe = fixture_probe(case)
    y = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(UvitError):
        probe.calibration_batch(torch.zeros(4, 11, device="cuda"), y)                # K of the head is 10
    with pytest.raises(UvitError):
        probe.calibration_batch(torch.zeros(4, 10, device="cuda"), y, ece_bins=65)
    with pytest.raises(UvitError):
        probe.calibration_batch(torch.zeros(1025, 10, device="cuda"), torch.zeros(1025, dtype=torch.int64, device="cuda"))
