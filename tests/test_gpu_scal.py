"""GPU: the set-level calibration ops (csrc/setcalib.hip) against the float64 restatement (tests/scal_ref.py) applied to the
probabilities read back from the device.

Counts (n_pos, values over the threshold, classes with an AUROC, N, bad rows) are compared for equality; AUROC_c and the accuracy are
one division of integers: 1e-12; every other metric and table entry is a double sum in a fixed order that differs from numpy's: 1e-9
absolute, the project's bound for fixed-order double sums (tests/test_gpu_detect.py).  The worst seen is printed.
Sizes: the sort has one launch up to N = 8192 and gains a level of global passes at every power of two above, hence one below, at and
one above 8192, 16384 and 32768; 8192 is also where the column owner's prefix count takes a second round."""
import ctypes as C

import numpy as np
import pytest
import torch

import scal_ref as sr
from test_gpu_probe import P, S as STREAM, case, fixture_probe, ok      # noqa: F401  (case: a fixture)

pytestmark = pytest.mark.gpu

EXACT_TOL, SUM_TOL = 1e-12, 1e-9
SIZES = [1, 2, 29, 1024, 1025, 4097, 8191, 8192, 8193, 12293, 16383, 16384, 16385, 32767, 32768, 32769]
CLASSES = [1, 2, 10, 17]
SETTINGS = dict(ece_bins=15, cw_bins=15, ace_bins=15, tace_bins=30, tace_threshold=0.01)
WORST = {"exact": 0.0, "sum": 0.0}
GUARD = 16


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


# ------------------------------------------------------------------------------------------------------------------------ inputs
def labels_for(rng, p, K):
    """Labels that follow the row maximum two times in three."""
    N = p.shape[0]
    return np.where(rng.random(N) < 0.66, p.argmax(1), rng.integers(0, K, N)).astype(np.int64)


def draw_logits(N, K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, K)) * 2.5).astype(np.float32), rng


def grid_probs(N, K, seed):
    """Probabilities k / 64 with rows that sum to 1: column ties, most values under the TACE threshold."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, 65, (N, K - 1)), axis=1)
    parts = np.diff(np.concatenate([np.zeros((N, 1), np.int64), cuts, np.full((N, 1), 64)], axis=1), axis=1)
    p = (parts / 64.0).astype(np.float32)
    return p, labels_for(rng, p, K)


def regime_set(N, regime):
    rng = np.random.default_rng(7000 + N)
    if regime == "grid":
        return grid_probs(N, 10, 7000 + N)
    if regime == "equal":
        p = np.full((N, 4), 0.25, dtype=np.float32)
        return p, rng.integers(0, 4, N).astype(np.int64)
    p = np.zeros((N, 10), dtype=np.float32)                   # saturated: exactly 1 and 0
    p[np.arange(N), rng.integers(0, 10, N)] = 1.0
    return p, labels_for(rng, p, 10)


# ------------------------------------------------------------------------------------------------------------------------ running
def store_of(p, ld):
    N, K = p.shape
    st = torch.full((N, ld), 7.5, dtype=torch.float32, device="cuda")
    st[:, :K] = torch.from_numpy(p).cuda()
    return st


def softmax_into_store(L, z, ld, batch=None):
    """uvit_op_scal_probs of z (N, K) into an (N, ld) store, `batch` rows per call; the columns behind K stay untouched."""
    N, K = z.shape
    zg = torch.from_numpy(z).cuda()
    st = torch.full((N * ld + GUARD,), 7.5, dtype=torch.float32, device="cuda")
    step = N if batch is None else batch
    for n0 in range(0, N, step):
        B = min(step, N - n0)
        ok(L.uvit_op_scal_probs(C.c_void_p(zg.data_ptr() + 4 * K * n0), C.c_void_p(st.data_ptr() + 4 * ld * n0), ld, B, K, STREAM()))
    torch.cuda.synchronize()
    assert bool((st[N * ld:] == 7.5).all())
    view = st[:N * ld].view(N, ld)
    assert bool((view[:, K:] == 7.5).all())
    return view


def run_metrics(L, store, labels, K, ws_bytes=None, **kw):
    """uvit_op_scal_metrics on a device store (N, ld): (out (16,), top_table, per_class) as numpy; guards behind every output and
    behind the workspace intact."""
    s = {**SETTINGS, **kw}
    N, ld = store.shape
    yg = torch.from_numpy(np.asarray(labels, dtype=np.int64)).cuda()
    full = L.uvit_op_scal_ws_bytes(N, K)
    assert full > 0
    ws_bytes = full if ws_bytes is None else ws_bytes
    ws = torch.zeros(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = 0x5A
    nt, nc = 3 * s["ece_bins"], 6 * K
    out = torch.full((16 + GUARD,), 7.5, dtype=torch.float64, device="cuda")
    top = torch.full((nt + GUARD,), 7.5, dtype=torch.float64, device="cuda")
    pc = torch.full((nc + GUARD,), 7.5, dtype=torch.float64, device="cuda")
    eb, cb = np.linspace(0, 1, s["ece_bins"] + 1), np.linspace(0, 1, s["cw_bins"] + 1)
    ok(L.uvit_op_scal_metrics(P(store), ld, P(yg), N, K, eb.ctypes.data_as(C.c_void_p), s["ece_bins"], cb.ctypes.data_as(C.c_void_p),
                              s["cw_bins"], s["ace_bins"], s["tace_bins"], C.c_double(s["tace_threshold"]), P(out), P(top), P(pc), P(ws),
                              ws_bytes, STREAM()))
    torch.cuda.synchronize()
    assert bool((out[16:] == 7.5).all()) and bool((top[nt:] == 7.5).all()) and bool((pc[nc:] == 7.5).all())
    assert bool((ws[ws_bytes:] == 0x5A).all())
    return out[:16].cpu().numpy(), top[:nt].view(-1, 3).cpu().numpy(), pc[:nc].view(K, 6).cpu().numpy()


def close(got, ref, tol, kind, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    err = float(np.nanmax(np.abs(got - ref))) if not np.isnan(ref).all() else 0.0
    WORST[kind] = max(WORST[kind], err)
    assert err <= tol, (what, err, got, ref)


def check_against_ref(got, p, y, what, **kw):
    out, top, pc = got
    ref = sr.metrics(p, y, **{**SETTINGS, **kw})
    r_out, r_pc = ref["out"], ref["per_class"]
    assert np.array_equal(pc[:, 4:], r_pc[:, 4:]), (what, "n_pos / over threshold")
    assert out[9] == r_out[9] and out[12] == r_out[12] and out[13] == r_out[13] and out[14] == 0.0 and out[15] == 0.0, (what, out, r_out)
    close(pc[:, 3], r_pc[:, 3], EXACT_TOL, "exact", (what, "AUROC_c"))
    close(out[10], r_out[10], EXACT_TOL, "exact", (what, "accuracy"))
    close(pc[:, :3], r_pc[:, :3], SUM_TOL, "sum", (what, "SCE_c ACE_c TACE_c"))
    close(top, ref["top_table"], SUM_TOL, "sum", (what, "reliability table"))
    close(out[:9], r_out[:9], SUM_TOL, "sum", (what, "out[0..8]"))
    close(out[11], r_out[11], SUM_TOL, "sum", (what, "mean confidence"))
    return ref


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# -------------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("N", SIZES)
def test_continuous_softmax(L, N, K):
    """Every launch plan at every class count: softmax on the device, the metrics against the restatement on the probabilities read
    back; a second call and a store with ld = K + 5 give the same bits."""
    z, rng = draw_logits(N, K, 100 * N + K)
    store = softmax_into_store(L, z, K)
    p = store.cpu().numpy()
    y = labels_for(rng, p, K)
    got = run_metrics(L, store, y, K)
    ref = check_against_ref(got, p, y, (N, K))
    assert same_bits(got, run_metrics(L, store, y, K))
    wide = softmax_into_store(L, z, K + 5)
    assert wide[:, :K].cpu().numpy().tobytes() == p.tobytes()
    assert same_bits(got, run_metrics(L, wide, y, K))
    print(f"\nN {N} K {K}: ECE {ref['ECE']:.6f} SCE {ref['SCE']:.6f} ACE {ref['ACE']:.6f} TACE {ref['TACE']:.6f} Brier {ref['Brier']:.6f} "
          f"AUROC {ref['AUROC']:.6f}; worst so far exact {WORST['exact']:.2e} (bound {EXACT_TOL:.0e}) sums {WORST['sum']:.2e} (bound {SUM_TOL:.0e})")


@pytest.mark.parametrize("K", [100, 1000])
def test_many_classes(L, K):
    """N = 1025: a ragged last tile of 64 classes in the key builder, and more columns than one tile row."""
    N = 1025
    z, rng = draw_logits(N, K, 31 * K)
    store = softmax_into_store(L, z, K)
    p = store.cpu().numpy()
    y = labels_for(rng, p, K)
    got = run_metrics(L, store, y, K)
    check_against_ref(got, p, y, (N, K))
    print(f"\nN {N} K {K}: worst so far exact {WORST['exact']:.2e} sums {WORST['sum']:.2e}")


@pytest.mark.parametrize("regime", ["grid", "equal", "saturated"])
@pytest.mark.parametrize("N", SIZES)
def test_tied_regimes(L, N, regime):
    """Column ties longer than a chunk, all rows equal (one tie group per column), and rows of exact ones and zeros: conf = 1 sits in
    the last bin, the zeros fall in no bin."""
    p, y = regime_set(N, regime)
    K = p.shape[1]
    store = store_of(p, K)
    got = run_metrics(L, store, y, K)
    check_against_ref(got, p, y, (N, regime))
    assert same_bits(got, run_metrics(L, store_of(p, K + 5), y, K))
    if regime == "saturated":
        assert got[1][-1, 0] == 1.0 and got[1][-1, 2] == 1.0           # every row in the last bin, at confidence 1


@pytest.mark.parametrize("N", [29, 1025, 8193])
def test_batches_do_not_matter(L, N):
    """The set written in batches of 7, of 128 and at once holds the same bytes and gives the same bits."""
    K = 10
    z, rng = draw_logits(N, K, 55 + N)
    whole = softmax_into_store(L, z, K)
    y = labels_for(rng, whole.cpu().numpy(), K)
    got = run_metrics(L, whole, y, K)
    for batch in (7, 128):
        st = softmax_into_store(L, z, K, batch=batch)
        assert st.cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()
        assert same_bits(got, run_metrics(L, st, y, K))


def test_smaller_workspace_same_bits(L):
    """A workspace with room for two columns of keys: nine groups of columns instead of one, more launches, the same bits."""
    N, K = 1025, 17
    z, rng = draw_logits(N, K, 99)
    store = softmax_into_store(L, z, K)
    y = labels_for(rng, store.cpu().numpy(), K)
    full, small = L.uvit_op_scal_ws_bytes(N, K), L.uvit_op_scal_ws_bytes(N, 1)
    assert small < full and L.uvit_op_scal_launches(N, K, small) == 2 + 9 * 3 and L.uvit_op_scal_launches(N, K, full) == 2 + 3
    assert same_bits(run_metrics(L, store, y, K), run_metrics(L, store, y, K, ws_bytes=small))


def test_other_bin_counts(L):
    """Bin counts at the limits and a threshold that cuts through the column."""
    N, K = 4097, 10
    kw = dict(ece_bins=64, cw_bins=1, ace_bins=64, tace_bins=7, tace_threshold=0.05)
    z, rng = draw_logits(N, K, 5)
    store = softmax_into_store(L, z, K)
    p = store.cpu().numpy()
    y = labels_for(rng, p, K)
    check_against_ref(run_metrics(L, store, y, K, **kw), p, y, "bins", **kw)
    p29 = p[:29].copy()                                                # N < bins: every lower bound is the column minimum
    check_against_ref(run_metrics(L, store_of(p29, K), y[:29], K, **kw), p29, y[:29], "bins, N 29", **kw)


@pytest.mark.parametrize("B", [1, 37, 1024])
def test_probs_equal_calib_softmax(L, B):
    K = 100
    z = torch.from_numpy(draw_logits(B, K, B)[0]).cuda()
    a = torch.zeros(B, K, device="cuda")
    ok(L.uvit_op_calib_softmax(P(z), P(a), B, K, STREAM()))
    b = softmax_into_store(L, z.cpu().numpy(), K)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("bad", ["label -1", "label K", "NaN logit"])
def test_bad_rows(L, bad):
    """A bad row is counted, makes out[0 .. 11] NaN and nothing leaves its array (guards in run_metrics)."""
    N, K = 1025, 10
    z, rng = draw_logits(N, K, 12)
    if bad == "NaN logit":
        z[[3, 700], 4] = np.nan
    store = softmax_into_store(L, z, K)
    p = store.cpu().numpy()
    y = labels_for(rng, np.nan_to_num(p), K)
    if bad != "NaN logit":
        y[[0, 511, 1024]] = -1 if bad == "label -1" else K
    out, top, pc = run_metrics(L, store, y, K)
    assert np.isnan(out[:12]).all() and out[12] == N and out[13] == (2 if bad == "NaN logit" else 3) and out[14] == 0.0 and out[15] == 0.0
    ref = sr.metrics(p, y, **SETTINGS)
    assert np.isnan(ref["out"][:12]).all() and ref["out"][13] == out[13]
    if bad != "NaN logit":                                             # the columns themselves are ordinary data
        assert np.array_equal(pc[:, 4:], ref["per_class"][:, 4:])
        close(pc[:, :4], ref["per_class"][:, :4], SUM_TOL, "sum", bad)


def test_calibration_set_against_per_batch_ops(case):
    """LinearProbe.calibration_set at N <= 1024: ECE, TACE and NLL equal calibration_batch(..., reference_bin_accuracy=False), the
    per-batch ops' textbook reading, to 1e-9; the per-class TACE values too."""
    probe = fixture_probe(case)
    K = probe.num_classes
    for N in (1, 29, 1024):
        z, rng = draw_logits(N, K, 400 + N)
        y = torch.from_numpy(labels_for(rng, z, K)).cuda()
        zg = torch.from_numpy(z).cuda()
        out, top, pc = probe.calibration_set(zg, y)
        ece, tace, nll, _ = (float(v) for v in probe.calibration_batch(zg, y, reference_bin_accuracy=False))
        o = out.cpu().numpy()
        close([o[0], o[7], o[3]], [ece, tace, nll], SUM_TOL, "sum", ("per-batch ops", N))
        close(pc[:, 2].cpu().numpy(), probe._per_class[:K].cpu().numpy(), SUM_TOL, "sum", ("per-batch TACE_c", N))
        close(top.cpu().numpy().ravel(), probe._bin_table[:45].cpu().numpy(), SUM_TOL, "sum", ("per-batch bin table", N))
