"""CPU: the set-level calibration restatement (tests/scal_ref.py) against the reference's own classes (tests/golden/scal.npz, written
by tools/gen_golden_scal.py), against calib_ref and scikit-learn at per-batch sizes and against a case worked by hand; then the host
side of the feature: the exported symbols, the launchers' refusals (they validate before anything touches a device), the workspace
query, the module's settings and the command line."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import calib_ref as cr
import scal_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_ULP = 2.0 ** -23          # the largest relative spacing of fp32


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "scal.npz"))


def case_of(fx, name):
    """(probs fp32, labels, logits fp32 or None) of a case: the continuous cases store grid logits, the last one grid probabilities."""
    y = fx["labels/" + name].astype(np.int64)
    if "logits_q2/" + name in fx.files:
        q = fx["logits_q2/" + name]
        p = sr.probs_from_grid_logits(q)
        assert zlib.crc32(p.astype("<f4").tobytes()) == int(fx["probs_crc/" + name]), "the probabilities differ from the generator's"
        return p, y, (q.astype(np.float32) / np.float32(2.0))
    return (fx["probs_q64/" + name].astype(np.float64) / 64.0).astype(np.float32), y, None


# ---- the restatement ----
def test_fixture_holds_the_cases(fx, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "scal.npz")) < 100 * 1024
    shapes = {n: case_of(fx, n)[0].shape for n in fx["names"]}
    assert shapes == {"n1100_k6": (1100, 6), "n1536_k10": (1536, 10), "grid64_n1200_k10": (1200, 10)}
    assert all(N > 1024 for N, _ in shapes.values())                            # more rows than a per-batch op takes
    assert (int(fx["ece_bins"]), int(fx["cw_bins"]), int(fx["ace_bins"]), int(fx["tace_bins"]), float(fx["tace_threshold"])) == (15, 15, 15, 30, 0.01)


def test_restatement_equals_the_reference_classes(fx):
    """ECELoss, MCELoss, OELoss, SCELoss, ACELoss and TACELoss of the reference, whose bin accuracy is positional: 1e-12."""
    for name in fx["names"]:
        p, y, _ = case_of(fx, name)
        m = sr.metrics(p, y, positional_acc=True)
        for key in ("ECE", "MCE", "OE", "SCE", "ACE", "TACE"):
            want = float(fx[key.lower() + "/" + name])
            assert abs(m[key] - want) <= 1e-12, (name, key, m[key], want)
        plain = sr.metrics(p, y)
        print(f"\n{name}: reference ECE {m['ECE']:.6f} SCE {m['SCE']:.6f} TACE {m['TACE']:.6f}; textbook ECE {plain['ECE']:.6f} "
              f"SCE {plain['SCE']:.6f} TACE {plain['TACE']:.6f}")


def test_brier_against_the_reference(fx):
    """BrierScore of the reference takes scipy's fp32 softmax of the logits, the restatement the correctly rounded fp32 probabilities.
    With eps = 2^-23: an fp32 exp is within 3 eps (relative), the K-term fp32 sum adds (K - 1) eps / 2 to the 3 eps of its terms, the
    quotient eps / 2, the other side's single rounding eps / 2: two probabilities differ by at most d = (7 + K / 2) eps (relative).
    d/dp sum_k (p_k - o_k)^2 = 2 (p_k - o_k) with |p_k - o_k| <= 1 and sum_k p_k = 1, so a row's score, and the mean, moves by at most 2 d."""
    worst = 0.0
    for name in fx["names"]:
        p, y, z = case_of(fx, name)
        if z is None:
            continue
        bound = 2.0 * (7.0 + p.shape[1] / 2.0) * F32_ULP
        err = abs(sr.metrics(p, y)["Brier"] - float(fx["brier/" + name]))
        worst = max(worst, err / bound)
        print(f"\n{name}: |Brier - reference| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
    print(f"worst |error| / bound {worst:.3e}")


def test_per_batch_sizes_equal_calib_ref_and_sklearn(golden_dir):
    """At N <= 1024 ECE, TACE and the per-class values are calib_ref's at positional_acc=False; the per-class AUROC is calib_ref's and
    scikit-learn's (tests/golden/calib.npz)."""
    cal = np.load(os.path.join(golden_dir, "calib.npz"))
    for name in cal["names"]:
        p, y = cal["probs/" + name], cal["labels/" + name]
        m = sr.metrics(p, y)
        cf, (t, t_c), a = cr.confidence(p, y, 15), cr.tace(p, y, 0.01, 30), cr.auroc(p, y)
        assert m["ECE"] == cf["ECE"] and m["TACE"] == t and np.array_equal(m["per_class"][:, 2], t_c) and m["NLL"] == cf["NLL"]
        assert np.array_equal(m["top_table"], cf["table"])
        skl = cal["auroc/" + name]
        got = m["per_class"][:, 3]
        assert np.array_equal(np.isnan(got), np.isnan(skl)) and np.nanmax(np.abs(got - skl)) <= 1e-12
        # calib_ref adds u2 / (2 n_pos n_neg) per positive row: up to n_pos roundings per class
        assert all(abs(got[c] - v) <= 1e-12 for c, v in a["per_class"].items()) and m["auroc_classes"] == a["count"]


def test_mean_of_batch_values_is_not_the_set_value(fx):
    """What --calibration reports against the set's own value, both with the textbook bin accuracy: the batch-size-weighted mean of
    per-batch ECE / TACE lies above the set's value and moves with the batch size (a bin of a small batch holds a handful of rows,
    and |conf - acc| of a handful of rows is biased upwards); NLL is a row mean either way."""
    p, y, _ = case_of(fx, "n1536_k10")
    m = sr.metrics(p, y)
    seen = {}
    for bs in (32, 128, 512):
        per, sizes = [], []
        for i in range(0, len(y), bs):
            per.append(cr.batch_metrics(p[i:i + bs], y[i:i + bs]))
            sizes.append(len(y[i:i + bs]))
        seen[bs] = cr.weighted(per, sizes, p.shape[1])
        assert abs(seen[bs]["NLL"] - m["NLL"]) < 1e-12
    print("\nset ECE %.6f TACE %.6f; batch means " % (m["ECE"], m["TACE"])
          + ", ".join("B = %d: ECE %.6f TACE %.6f" % (bs, w["ECE"], w["TACE"]) for bs, w in seen.items()))
    assert seen[32]["ECE"] > seen[128]["ECE"] > seen[512]["ECE"] > m["ECE"]
    assert seen[32]["ECE"] - m["ECE"] > 0.05 and seen[32]["TACE"] > 1.9 * m["TACE"] and seen[128]["TACE"] > m["TACE"]


def test_case_by_hand():
    """p = [[.75, .25], [.75, .25], [.25, .75], [.5, .5]], y = [0, 1, 1, 0], 15 bins of width 1/15.
    conf = .75, .75, .75, .5; pred = 0, 0, 1, 0 (the tie goes to the lowest index); correct = 1, 0, 1, 1.
    Bin (7/15, 8/15] holds row 3: prop 1/4, acc 1, conf .5; bin (11/15, 12/15] holds rows 0-2: prop 3/4, acc 2/3, conf .75.
    ECE = 1/4 * 1/2 + 3/4 * 1/12 = 3/16; MCE = 1/2; OE = 3/4 * 3/4 * 1/12 = 3/64 (the first bin is under-confident: 0).
    Brier rows = 2 * (1/16, 9/16, 1/16, 1/4) = 1/8, 9/8, 1/8, 1/2: mean 15/32.  NLL = -(2 ln .75 + ln .25 + ln .5) / 4 = 0.66370142...
    Class 0: positives .75, .5 against negatives .75, .25: (1/2 + 1 + 0 + 1) / 4 = 5/8; class 1: positives .25, .75 against negatives
    .25, .5: (1/2 + 0 + 1 + 1) / 4 = 5/8."""
    p = np.array([[.75, .25], [.75, .25], [.25, .75], [.5, .5]], dtype=np.float32)
    m = sr.metrics(p, [0, 1, 1, 0])
    assert m["ECE"] == pytest.approx(0.1875, abs=1e-15) and m["MCE"] == pytest.approx(0.5, abs=1e-15)
    assert m["OE"] == pytest.approx(0.046875, abs=1e-15) and m["Brier"] == 0.46875
    assert m["NLL"] == pytest.approx(-(2 * np.log(0.75) + np.log(0.25) + np.log(0.5)) / 4, abs=1e-15)
    assert f"{m['NLL']:.6f}" == "0.663701"
    assert m["per_class"][:, 3].tolist() == [0.625, 0.625] and m["AUROC"] == 0.625 and m["auroc_classes"] == 2
    assert m["acc"] == 0.75 and m["mean_conf"] == 0.6875 and m["n"] == 4 and m["n_bad"] == 0
    assert m["per_class"][:, 4].tolist() == [2.0, 2.0]


def test_bad_rows():
    p = np.array([[.75, .25], [.5, .5], [.25, .75]], dtype=np.float32)
    for y in ([0, -1, 1], [0, 2, 1]):
        m = sr.metrics(p, y)
        assert np.isnan(m["out"][:12]).all() and m["n_bad"] == 1 and m["n"] == 3
    q = p.copy()
    q[2, 0] = np.nan
    m = sr.metrics(q, [0, 1, 1])
    assert np.isnan(m["out"][:12]).all() and m["n_bad"] == 1
    assert sr.metrics(p, [0, 1, 1])["n_bad"] == 0


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL, 16-byte aligned pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE, WORKSPACE = -1, -2, -4
NAMES = ("uvit_op_scal_probs", "uvit_op_scal_ws_bytes", "uvit_op_scal_launches", "uvit_op_scal_metrics")


def test_symbols_are_declared_and_exported():
    from uncertainty_vit_amd import native
    hdr = open(os.path.join(ROOT, "include", "uvit.h")).read()
    for name in NAMES:
        assert name in native.SYMBOLS and name + "(" in hdr and getattr(native.lib(), name).argtypes is not None
    build = open(os.path.join(ROOT, "uncertainty-vit_amd", "csrc", "build.sh")).read()
    strict = build.split('STRICT_FILES="')[1].split('"')[0].split()
    assert "setcalib" in strict
    assert "#error" in open(os.path.join(ROOT, "uncertainty-vit_amd", "csrc", "setcalib.hip")).read().split("#include")[0]


def test_ws_bytes_limits_and_monotony(L):
    """Refuses N = 0, N > 2^20, K = 0 and N K > 2^30; never shrinks when N or K grows; holds the row arrays (21 N bytes) and the keys
    of all K + 1 columns while they fit 2^26 keys, and stays under 21 N + 2^28 + slack beyond."""
    for N, K in [(0, 1), (-1, 1), ((1 << 20) + 1, 1), (10, 0), (10, -1), (1 << 20, 1025), (1 << 16, (1 << 14) + 1)]:
        assert L.uvit_op_scal_ws_bytes(N, K) == SHAPE, (N, K)
        assert L.uvit_op_scal_launches(N, K, 1 << 40) == SHAPE
    assert L.uvit_op_scal_ws_bytes(1, 1) > 0 and L.uvit_op_scal_ws_bytes(1 << 20, 1024) > 0
    sizes_n = [L.uvit_op_scal_ws_bytes(N, 10) for N in (1, 2, 1000, 1024, 1025, 8192, 8193, 50000, 1 << 19, 1 << 20)]
    sizes_k = [L.uvit_op_scal_ws_bytes(50000, K) for K in (1, 2, 10, 100, 1000, 1023, 1024, 5000, 20000)]
    assert sizes_n == sorted(sizes_n) and sizes_k == sorted(sizes_k) and len(set(sizes_n)) > 5
    assert L.uvit_op_scal_ws_bytes(1025, 10) >= 21 * 1025 + 11 * 2048 * 4
    assert L.uvit_op_scal_ws_bytes(50000, 1000) >= 21 * 50000 + 1001 * 65536 * 4
    assert max(sizes_k) <= 21 * 50000 + (1 << 28) + 64 and L.uvit_op_scal_ws_bytes(1 << 20, 1024) <= 21 * (1 << 20) + (1 << 28) + 64
    # launches: rows + finish, and per group of columns the builder, the sort (1 launch up to 8192 rows) and the column owner
    assert L.uvit_op_scal_launches(8192, 10, 1 << 40) == 5 and L.uvit_op_scal_launches(8193, 10, 1 << 40) == 7
    assert L.uvit_op_scal_launches(50000, 1000, 1 << 40) == 2 + 1 + 10 + 1
    assert L.uvit_op_scal_launches(50000, 1000, 1 << 40) == L.uvit_op_scal_launches(50000, 10, 1 << 40)        # not a function of K


def test_metrics_rejects_bad_arguments(L):
    """Every refusal returns before the device is touched and leaves the (host) outputs as they were."""
    N, K = 100, 7
    ws = L.uvit_op_scal_ws_bytes(N, K)
    out, top, pc = np.full(16, 7.5), np.full(45, 7.5), np.full(6 * K, 7.5)
    eb, cb = np.linspace(0, 1, 16), np.linspace(0, 1, 16)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    good = dict(probs=P1, ld=K, labels=P1, N=N, K=K, eb=hp(eb), ece=15, cb=hp(cb), cw=15, ace=15, tace=30, thr=0.01, out=hp(out), top=hp(top),
                pc=hp(pc), ws=P1, ws_bytes=ws)

    def call(**kw):
        a = {**good, **kw}
        return L.uvit_op_scal_metrics(a["probs"], a["ld"], a["labels"], a["N"], a["K"], a["eb"], a["ece"], a["cb"], a["cw"], a["ace"], a["tace"],
                                      C.c_double(a["thr"]), a["out"], a["top"], a["pc"], a["ws"], a["ws_bytes"], NUL)

    shapes = [dict(N=0), dict(N=-3), dict(N=(1 << 20) + 1, ws_bytes=1 << 40), dict(K=0), dict(N=1 << 20, K=1025, ld=1025, ws_bytes=1 << 40),
              dict(ld=K - 1)] + [{b: v} for b in ("ece", "cw", "ace", "tace") for v in (0, -1, 65)]
    for kw in shapes:
        assert call(**kw) == SHAPE, kw
    for name in ("probs", "labels", "eb", "cb", "out", "top", "pc", "ws"):
        assert call(**{name: NUL}) == ARG, name
    assert call(ws=C.c_void_p(4100)) == ARG and call(thr=float("nan")) == ARG
    assert call(ws_bytes=0) == WORKSPACE and call(ws_bytes=21 * N + 64) == WORKSPACE
    assert (out == 7.5).all() and (top == 7.5).all() and (pc == 7.5).all()


def test_probs_rejects_bad_arguments(L):
    call = L.uvit_op_scal_probs
    for N, K, ld in [(0, 10, 10), (-1, 10, 10), (4, 0, 10), (4, 10, 9), (4, 10, 0)]:
        assert call(P1, P1, ld, N, K, NUL) == SHAPE, (N, K, ld)
    assert call(NUL, P1, 10, 4, 10, NUL) == ARG and call(P1, NUL, 10, 4, 10, NUL) == ARG


# ---- the module and the command line ----
def test_module_settings_and_no_cpu_fallback():
    import torch
    from test_host_probe import tiny_encoder
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    from uncertainty_vit_amd.probe_setcalib import SCAL_DEFAULTS
    probe = LinearProbe(tiny_encoder().eval(), 10)
    assert probe._scal is None
    probe.enable_set_calibration()
    assert probe._scal == SCAL_DEFAULTS == dict(ece_bins=15, cw_bins=15, ace_bins=15, tace_bins=30, tace_threshold=0.01)
    probe.enable_set_calibration(ece_bins=10, tace_threshold=0.0)
    assert probe._scal["ece_bins"] == 10 and probe._scal["tace_threshold"] == 0.0 and probe._scal["tace_bins"] == 30
    probe.set_set_calibration(None)
    assert probe._scal is None
    for kw in (dict(ece_bins=0), dict(cw_bins=65), dict(ace_bins=2.5), dict(tace_threshold=1.5), dict(tace_threshold=-0.1)):
        with pytest.raises(UvitError):
            probe.enable_set_calibration(**kw)
    assert probe._scal is None
    with pytest.raises(UvitError):
        probe.calibration_set(torch.zeros(8, 10), torch.zeros(8, dtype=torch.int64))


def test_cli_flags_and_refusals():
    """Without the new flags the parsed arguments are today's; the --scal_* flags are refused without --set_calibration, as are values
    outside the kernels' limits; --set_calibration stands beside --calibration."""
    import run_linear_probe as rlp
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()
    base = vars(rlp.get_args([]))
    assert not any(k.startswith("scal_") or k == "set_calibration" for k in base)
    assert rlp.check_scal_flags(rlp.get_args([])) is None and rlp.check_scal_flags(rlp.get_args(["--calibration"])) is None
    for flag, v in (("--scal_ece_bins", "10"), ("--scal_cw_bins", "10"), ("--scal_ace_bins", "10"), ("--scal_tace_bins", "10"),
                    ("--scal_tace_threshold", "0.05")):
        with pytest.raises(ValueError, match="--set_calibration"):
            rlp.check_scal_flags(rlp.get_args([flag, v]))
    assert rlp.check_scal_flags(rlp.get_args(["--set_calibration"])) == {}
    a = rlp.get_args(["--set_calibration", "--calibration", "--scal_ece_bins", "10", "--scal_cw_bins", "12", "--scal_ace_bins", "20",
                      "--scal_tace_bins", "64", "--scal_tace_threshold", "0.05"])
    assert a.calibration is True
    assert rlp.check_scal_flags(a) == dict(ece_bins=10, cw_bins=12, ace_bins=20, tace_bins=64, tace_threshold=0.05)
    for bad in (["--scal_ece_bins", "0"], ["--scal_tace_bins", "65"], ["--scal_tace_threshold", "1.5"]):
        with pytest.raises(ValueError):
            rlp.check_scal_flags(rlp.get_args(["--set_calibration"] + bad))


SC = {"ECE": 0.125, "MCE": 0.5, "OE": 0.0625, "NLL": 1.25, "Brier": 0.75, "SCE": 0.03125, "ACE": 0.015625, "TACE": 0.25, "AUROC": 0.875,
      "auroc_classes": 9, "acc": 0.5, "mean_conf": 0.625, "n": 1100, "n_bad": 0, "reliability": [[0.25, 1.0, 0.5], [0.75, 0.5, 0.75]],
      "per_class": {"SCE": [0.5], "ACE": [0.5], "TACE": [0.5], "AUROC": [0.875], "n_pos": [3.0], "n_over_threshold": [7.0]}}


def test_cli_lines_and_log_entries(tmp_path):
    import json

    import run_linear_probe as rlp
    assert rlp.set_calibration_line(SC) == ("* Set ECE 0.12500 MCE 0.50000 OE 0.06250 NLL 1.25000 Brier 0.75000 SCE 0.03125 ACE 0.01562 TACE 0.25000 "
                                            "AUROC 0.87500 on 1100 images (9 classes with an AUROC)")
    log = rlp.set_calibration_log_entries(SC)
    assert set(log) == {f"test_set_{k}" for k in ("ECE", "MCE", "OE", "NLL", "Brier", "SCE", "ACE", "TACE", "AUROC", "reliability")}
    assert log["test_set_Brier"] == 0.75 and log["test_set_reliability"] == SC["reliability"]
    rlp.write_reliability(str(tmp_path), SC)
    rel = json.load(open(tmp_path / "reliability.json"))
    assert rel == {"n": 1100, "n_bad": 0, "reliability": SC["reliability"], "per_class": SC["per_class"]}
    # the corruption sweep: the set's block, its log line, the per-severity summary
    stats = {"acc1": 50.0, "acc5": 75.0, "loss": 1.5, "n": 8, "set_calibration": SC}
    assert rlp.corruption_set_lines(stats) == [rlp.corruption_set_line(stats), rlp.set_calibration_line(SC)]
    entry = rlp.corruption_log_entries("brightness", 1, stats)
    assert all(entry[f"test_c_brightness_1_set_{k}"] == SC[k] for k in rlp.SCAL_LINE_KEYS) and "test_c_brightness_1_set_reliability" not in entry
    other = {**stats, "set_calibration": {**SC, "ECE": 0.375, "Brier": 0.25}}
    summary = rlp.corruption_summary({("brightness", 1): stats, ("contrast", 1): other}, {"acc1": 60.0})
    assert summary["set_ECE"] == [0.25] and summary["set_Brier"] == [0.5] and summary["set_NLL"] == [1.25]
    assert rlp.corruption_summary_lines(summary)[1].endswith(" set-ECE 0.25000 Brier 0.50000")
    slog = rlp.corruption_summary_log(summary)
    assert slog["test_c_severity_set_ECE"] == [0.25] and slog["test_c_severity_set_NLL"] == [1.25] and slog["test_c_severity_set_Brier"] == [0.5]
    # without the switch, not a byte changes
    plain = {k: v for k, v in stats.items() if k != "set_calibration"}
    assert rlp.corruption_set_lines(plain) == [rlp.corruption_set_line(plain)]
    assert not any("set_" in k for k in rlp.corruption_log_entries("brightness", 1, plain))
    assert not any("set_" in k for k in rlp.corruption_summary({("brightness", 1): plain}, {"acc1": 60.0}))
