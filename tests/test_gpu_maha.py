"""GPU: the Mahalanobis / relative Mahalanobis scores (csrc/maha.hip, LinearProbe.fit_density / feature_scores / density_batch)
against the float64 restatement of tests/maha_ref.py on the same inputs.  Every bound is derived in maha_ref's docstring from the
unit roundoff of the double operations the kernels perform; none comes from running them.  Every test prints the worst
|error| / bound before it asserts."""
import math
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

import detect_ref as dr
import maha_ref as mr
import probe_ref as pr
from oracle.closed_form import closed_form_images
from test_gpu_probe import GUARD, P, S, frozen_state, ok

pytestmark = pytest.mark.gpu

F64 = torch.float64
EXACT_TOL, SUM_TOL = 1e-12, 1e-9             # tests/test_gpu_detect.py: AUROC / FPR95 and AUPR / AURC of uvit_op_detect_metrics


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def guarded(n, dtype=F64, fill=0.0):
    """n elements of `fill` on the device followed by GUARD sentinels (7) that no kernel may touch."""
    t = torch.full((n + GUARD,), 7, device="cuda", dtype=dtype)
    t[:n] = fill
    return t


def intact(t, n):
    return bool((t[n:] == 7).all())


def workspace(nbytes):
    assert nbytes >= 0
    return torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_accumulate(L, batches, Cd, K):
    """uvit_op_maha_accumulate over consecutive batches into the same accumulators; host float64 (S, class_sum, total_sum,
    class_count, sums)."""
    sizes = (Cd * Cd, K * Cd, Cd, K, 2)
    acc = [guarded(n) for n in sizes]
    for f, y in batches:
        B = f.shape[0]
        ws = workspace(L.uvit_op_maha_accumulate_ws_bytes(B, Cd, K))
        fd, yd = dev(f), dev(y)
        ok(L.uvit_op_maha_accumulate(P(fd), P(yd), *(P(a) for a in acc), P(ws), ws.numel(), B, Cd, K, S()))
    torch.cuda.synchronize()
    assert all(intact(a, n) for a, n in zip(acc, sizes))
    out = [a[:n].cpu().numpy() for a, n in zip(acc, sizes)]
    return out[0].reshape(Cd, Cd), out[1].reshape(K, Cd), out[2], out[3], out[4]


def check_accumulated(got, batches, K, what):
    ref = mr.accumulate_batches(batches, K)
    bS, (bc, bt) = mr.bound_S(batches, K), mr.bound_sums(batches, K)
    rS = np.abs(got[0] - ref[0]) / np.maximum(bS, 1e-300)
    rc = np.abs(got[1] - ref[1]) / np.maximum(bc, 1e-300)
    rt = np.abs(got[2] - ref[2]) / np.maximum(bt, 1e-300)
    print(f"\naccumulate {what}: |error| / bound  S {rS.max():.3f}  class sums {rc.max():.3f}  total {rt.max():.3f}")
    assert rS.max() <= 1.0 and rc.max() <= 1.0 and rt.max() <= 1.0
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[4], ref[4])
    assert np.array_equal(got[0], got[0].T)                                   # bit-symmetric


# -------------------------------------------------------------------------------------------------------------------- accumulate
@pytest.mark.parametrize("shape", mr.SHAPES)
def test_accumulate(L, shape):
    """Two consecutive batches into the same sums against maha_ref within the bounds; S symmetric bit for bit; counts exact; a second
    run gives the same bits."""
    B, Cd, K = shape
    a, b = mr.make_case(B, Cd, K, with_fit=False), mr.make_case(B, Cd, K, seed=1, with_fit=False)
    batches = [(a["feat"], a["labels"]), (b["feat"], b["labels"])]
    got = run_accumulate(L, batches, Cd, K)
    check_accumulated(got, batches, K, shape)
    assert got[4].tolist() == [2 * B, 0]
    again = run_accumulate(L, batches, Cd, K)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))


@pytest.mark.parametrize("Cd,K", [(12, 3), (132, 65)])
def test_accumulate_one_batch_or_two(L, Cd, K):
    """130 rows as one batch and as batches of 17 + 113: both within the bounds of the restatement (so within twice the bound of each
    other), each the same bits on a second run."""
    c = mr.make_case(130, Cd, K, with_fit=False)
    f, y = c["feat"], c["labels"]
    one, two = [(f, y)], [(f[:17], y[:17]), (f[17:], y[17:])]
    g1, g2 = run_accumulate(L, one, Cd, K), run_accumulate(L, two, Cd, K)
    check_accumulated(g1, one, K, f"(130, {Cd}, {K}) in one batch")
    check_accumulated(g2, two, K, f"(130, {Cd}, {K}) as 17 + 113")
    for g, batches in ((g1, one), (g2, two)):
        assert all(x.tobytes() == z.tobytes() for x, z in zip(g, run_accumulate(L, batches, Cd, K)))


@pytest.mark.parametrize("B,Cd,K", [(17, 12, 3), (130, 132, 65)])
def test_accumulate_leaves_out_bad_rows(L, B, Cd, K):
    """A class without rows, a label of -1, a label of K, a row with a NaN and a row with an inf: four rows skipped and counted, and
    every sum holds the bits of the call on the batch without them (they add exact zeros, or nothing, to every chain)."""
    c = mr.make_case(B, Cd, K, seed=2, with_fit=False)
    f, y = c["feat"].copy(), c["labels"].copy()
    y[y == K - 1] = 0                                                          # class K - 1 has no rows
    y[0], y[B - 1] = -1, K
    f[2, Cd - 1], f[B // 2, 0] = np.nan, np.inf
    keep = mr.usable_rows(f, y, K)
    assert keep.sum() == B - 4
    got = run_accumulate(L, [(f, y)], Cd, K)
    clean = run_accumulate(L, [(f[keep], y[keep])], Cd, K)
    assert got[4].tolist() == [B - 4, 4] and clean[4].tolist() == [B - 4, 0] and got[3][K - 1] == 0 and got[3].sum() == B - 4
    assert all(x.tobytes() == z.tobytes() for x, z in zip(got[:4], clean[:4]))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and not got[1][K - 1].any()
    check_accumulated(got, [(f, y)], K, f"({B}, {Cd}, {K}) with four bad rows")


# ------------------------------------------------------------------------------------------------------------------------ scores
def run_scores(L, feat, ft, Cd, K, dist=True, pad=0, labels=None):
    """uvit_op_maha_scores on host arrays: (maha, rmaha, pred, dist or None, correct or None), outputs behind guards."""
    B = feat.shape[0]
    ld = K + pad
    maha, rmaha = guarded(B, torch.float32, -1.0), guarded(B, torch.float32, -1.0)
    pred = guarded(B, torch.int32, -5)
    d = guarded(B * ld, F64, -2.0) if dist else None
    correct = guarded(1, torch.int32, 0) if labels is not None else None
    ws = workspace(L.uvit_op_maha_scores_ws_bytes(B, Cd, K))
    args = [dev(feat)] + [dev(ft[k]) for k in ("W", "W0", "Wmu", "Wmu0", "class_count")]
    yd = dev(labels) if labels is not None else None
    ok(L.uvit_op_maha_scores(*(P(a) for a in args), P(maha), P(rmaha), P(pred), P(d), ld, P(yd), P(correct), P(ws), ws.numel(), B, Cd, K, S()))
    torch.cuda.synchronize()
    assert intact(maha, B) and intact(rmaha, B) and intact(pred, B) and (d is None or intact(d, B * ld)) and (correct is None or intact(correct, 1))
    dd = d[:B * ld].view(B, ld).cpu().numpy() if dist else None
    return maha[:B].cpu().numpy(), rmaha[:B].cpu().numpy(), pred[:B].cpu().numpy(), dd, None if correct is None else int(correct[0])


@lru_cache(maxsize=None)
def scored(shape):
    """Per shape, computed once: the case, the restatement's scores on the host-made fit and their bounds."""
    case = mr.make_case(*shape)
    ft = case["fit"]
    ref = mr.scores(case["feat"], ft["W"], ft["W0"], ft["Wmu"], ft["Wmu0"], ft["class_count"])
    return case, ref, mr.bounds_scores(case["feat"], ft, ref), mr.bound_dist(case["feat"], ft["W"], ft["Wmu"])


@pytest.mark.parametrize("shape", mr.SHAPES)
def test_scores(L, shape):
    """maha, rmaha and every d_k against maha_ref on the same host-made W, W0, Wmu, Wmu0 within the derived bounds; pred equal
    wherever the restatement's two smallest distances differ by more than their bounds (at least 99 % of the rows); the padding of
    dist (ld = K + 3) untouched; dist = NULL and a second run give the same bits; the counter equals the rows with pred == label."""
    B, Cd, K = shape
    case, ref, (bm, br, decided), bd = scored(shape)
    ft, feat, y = case["fit"], case["feat"], case["labels"]
    maha, rmaha, pred, dist, correct = run_scores(L, feat, ft, Cd, K, pad=3, labels=y)
    rm = np.abs(maha.astype(np.float64) - ref["maha"]) / bm
    rr = np.abs(rmaha.astype(np.float64) - ref["rmaha"]) / br
    rd = np.abs(dist[:, :K] - ref["dist"]) / bd
    print(f"\nscores {shape}: |error| / bound  maha {rm.max():.3f}  rmaha {rr.max():.3f}  dist {rd.max():.3f}; decided {decided.mean():.3f}, "
          f"nearest-class-mean accuracy {(ref['pred'] == y).mean():.3f}")
    assert rm.max() <= 1.0 and rr.max() <= 1.0 and rd.max() <= 1.0
    assert decided.mean() >= 0.99 and np.array_equal(pred[decided], ref["pred"][decided])
    assert (dist[:, K:] == -2.0).all() and correct == int((pred == y).sum())
    for kw in ({"dist": False}, {"pad": 0}):
        m2, r2, p2, _, _ = run_scores(L, feat, ft, Cd, K, **kw)
        assert m2.tobytes() == maha.tobytes() and r2.tobytes() == rmaha.tobytes() and p2.tobytes() == pred.tobytes()


def test_scores_tie_empty_class_and_nan_row(L):
    """With W = W0 = I at C = 4: classes 1 and 2 at the same exact distance give the lower index; class 3, the nearest, has no rows
    and is never chosen; a row with a NaN and a row with an inf give NaN, NaN, -1 and a NaN row of dist and leave their neighbours'
    bits as they are without them; with every class empty all rows give NaN, NaN, -1."""
    Cd, K = 4, 4
    eye = np.eye(Cd)
    ft = {"W": eye, "W0": eye, "Wmu": np.array([[9.0, 0, 0, 0], [1.0, 0, 0, 0], [-1.0, 0, 0, 0], [0.0, 0, 0, 0]]), "Wmu0": np.array([0.5, 0, 0, 0]),
          "class_count": np.array([1.0, 2.0, 2.0, 0.0])}
    x = np.zeros((5, Cd), dtype=np.float32)
    x[3, 1] = 0.25
    clean = run_scores(L, x, ft, Cd, K)
    assert clean[2].tolist() == [1] * 5 and clean[0].tolist() == [1.0, 1.0, 1.0, 1.0625, 1.0] and clean[1].tolist() == [0.75] * 5
    assert clean[3][0].tolist() == [81.0, 1.0, 1.0, 0.0]
    bad = x.copy()
    bad[1, 2], bad[4, 0] = np.nan, -np.inf
    maha, rmaha, pred, dist, _ = run_scores(L, bad, ft, Cd, K)
    ref = mr.scores(bad, ft["W"], ft["W0"], ft["Wmu"], ft["Wmu0"], ft["class_count"])
    assert pred.tolist() == [1, -1, 1, 1, -1] == ref["pred"].tolist()
    for got, want in ((maha, clean[0]), (rmaha, clean[1])):
        assert np.isnan(got[[1, 4]]).all() and got[[0, 2, 3]].tobytes() == want[[0, 2, 3]].tobytes()
    assert np.isnan(dist[[1, 4]]).all() and dist[[0, 2, 3]].tobytes() == clean[3][[0, 2, 3]].tobytes()
    none = run_scores(L, x, {**ft, "class_count": np.zeros(K)}, Cd, K)
    assert np.isnan(none[0]).all() and np.isnan(none[1]).all() and none[2].tolist() == [-1] * 5 and np.array_equal(none[3], clean[3])


# ---------------------------------------------------------------------------------------------------------------------- meaning
def test_meaning_through_density_batch_and_detection_batch(L):
    """The synthetic set of the issue (K = 5, C = 16, 240 fit rows, 60 held-out rows, 60 rows of normalised noise, seed 0): OOD AUROC
    1.0 for both columns and nearest-class-mean accuracy 1.0, as the restatement gives, for rho in {1e-6, 1e-3, 1e-2}.  The encoder's
    attention needs an embed dim of at least 64, so the 16 features are the first 16 of 64, the others zero: every covariance is then
    block diagonal with rho tr / 64 in the empty block, and a shrinkage of 4 rho is the C = 16 problem at rho exactly (the zero
    entries add nothing to any distance)."""
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    K, Cd, (f_fit, y_fit), (f_in, y_in), f_out = mr.meaning_case(0)
    enc = VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=64, depth=1, num_heads=1, init_values=0.1,
                                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), use_shared_rel_pos_bias=True,
                                               use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(enc, K)
    wide = lambda f: np.concatenate([f, np.zeros((len(f), 64 - Cd), dtype=np.float32)], axis=1)      # noqa: E731
    sums = run_accumulate(L, [(wide(f_fit), y_fit)], 64, K)
    for rho in (1e-6, 1e-3, 1e-2):
        info = probe.load_density_state({**{k: torch.from_numpy(v.copy()) for k, v in zip(("S", "class_sum", "total_sum", "class_count", "sums"), sums)},
                                         "shrinkage": 4 * rho})
        assert (info["n"], info["skipped"], info["empty_classes"]) == (240, 0, 0)
        inn, out = probe.density_batch(dev(wide(f_in))), probe.density_batch(dev(wide(f_out)), distances=True)
        assert tuple(out["dist"].shape) == (60, K) and out["dist"].dtype == F64
        ft = mr.fit(*mr.accumulate(f_fit, y_fit, K), rho)
        for x, got in ((f_in, inn), (f_out, out)):
            ref = mr.scores(x, ft["W"], ft["W0"], ft["Wmu"], ft["Wmu0"], ft["class_count"])
            rel = max(float(np.abs(got[k].cpu().numpy() / ref[k] - 1).max()) for k in ("maha", "rmaha"))
            assert rel <= 1e-5, rel                                           # another factorisation of the same matrix, then fp32
        cols = torch.stack([torch.cat([inn["maha"], out["maha"]]), torch.cat([inn["rmaha"], out["rmaha"]])]).contiguous()
        flags = torch.cat([torch.zeros(60), torch.ones(60)]).to(torch.uint8).cuda()
        table = probe.detection_batch(cols, flags).cpu().numpy()
        acc = float((inn["pred"].cpu().numpy() == y_in).mean())
        print(f"\nrho {rho}: OOD AUROC maha {table[0, 0]}, rmaha {table[1, 0]}; nearest-class-mean accuracy {acc}")
        assert table[0, 0] == 1.0 and table[1, 0] == 1.0 and acc == 1.0


# ------------------------------------------------------------------------------------------------------------------- the module
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def encoder(case):
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    _, cfg, enc = case[:3]
    model = VisionTransformerForCyclicalTraining(img_size=cfg.img_size, patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth,
                                                 num_heads=cfg.num_heads, norm_layer=partial(torch.nn.LayerNorm, eps=cfg.ln_eps),
                                                 init_values=cfg.init_values, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    model.load_state_dict(enc, strict=False)
    return model.cuda().eval()


def batches_of(cfg, tag, sizes, K=10, labelled=True):
    """Batches of closed-form images as the prefetcher's items ((images, mask), labels on the host), labels drawn once per tag."""
    rng = np.random.default_rng(len(tag))
    xs = [closed_form_images(f"{tag}/{i}", n, cfg.img_size).cuda() for i, n in enumerate(sizes)]
    return [((x, None), torch.from_numpy(rng.integers(0, K, len(x)))) for x in xs] if labelled else xs


def make_probe(enc, kind):
    torch.manual_seed(5)
    if kind == "linear":
        from uncertainty_vit_amd.linear_probe import LinearProbe
        return LinearProbe(enc, 10, init_scale=5.0)
    if kind == "gp":
        from uncertainty_vit_amd.gp_probe import GPProbe
        return GPProbe(enc, 10, num_inducing=64)
    if kind == "het":
        from uncertainty_vit_amd.het_probe import HetProbe
        return HetProbe(enc, 10, num_factors=4, test_mc_samples=64)
    if kind == "ens":
        from uncertainty_vit_amd.ens_probe import EnsembleProbe
        return EnsembleProbe(enc, 10, members=3, init_scale=5.0)
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    return LaplaceProbe(enc, 10, init_scale=5.0)


def same(a, b):
    """Equal stats, key for key, with equal floats (NaN equal to NaN)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b


@pytest.mark.parametrize("kind", ["linear", "gp", "het", "ens", "lap"])
def test_density_end_to_end(L, case, encoder, kind):
    """fit_density on three ragged batches, then evaluate(detection=True, ood_loader=...) on two evaluation and two OOD batches, for
    every probe class (the Laplace probe with a Laplace fit, set before the density and cleared after it)."""
    from uncertainty_vit_amd.linear_probe import MAHA_COLUMNS
    cfg = case[1]
    probe = make_probe(encoder, kind)
    fit_b, eval_b = batches_of(cfg, "maha-fit", (5, 4, 3)), batches_of(cfg, "maha-eval!", (4, 3))
    ood_b = batches_of(cfg, "maha-ood", (3, 2), labelled=False)
    probe.features(fit_b[0][0][0])                                            # the first forward builds the engine and its bf16 shadows
    before = frozen_state(probe)
    if kind == "lap":
        probe.fit_laplace(fit_b, prior_precision=1.0)
    own = probe.DETECT_COLUMNS
    without = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    assert without["detection"]["columns"] == list(own) and "maha_mean" not in without

    # the fit: the restatement's sums from the probe's own features, within the bounds
    info = probe.fit_density(fit_b)
    f_fit = [probe.features(x).cpu().numpy() for (x, _), _ in fit_b]
    rows = [(f, y.numpy()) for f, (_, y) in zip(f_fit, fit_b)]
    sd = probe.density_state_dict()
    check_accumulated([sd[k].numpy() for k in ("S", "class_sum", "total_sum", "class_count", "sums")], rows, 10, f"fit_density ({kind})")
    counts = np.bincount(np.concatenate([y for _, y in rows]), minlength=10)
    assert info == probe.density and (info["n"], info["skipped"], info["classes"], info["empty_classes"], info["shrinkage"]) == \
        (12, 0, 10, int((counts == 0).sum()), 1e-3)
    ref_fit = mr.fit(*(sd[k].numpy() for k in ("S", "class_sum", "total_sum", "class_count", "sums")), 1e-3)
    assert info["logdet"] == pytest.approx(ref_fit["logdet"], rel=1e-9) and info["logdet0"] == pytest.approx(ref_fit["logdet0"], rel=1e-9)
    assert probe.DETECT_COLUMNS == own + MAHA_COLUMNS and len(probe.DETECT_COLUMNS) <= 16

    # feature_scores against the restatement on the probe's own uploaded factors
    st = probe._maha
    ft = {k: st[k].cpu().numpy() for k in ("W", "W0", "Wmu", "Wmu0")}
    ft["class_count"] = st["count_dev"].cpu().numpy()
    xs = [x for (x, _), _ in eval_b] + list(ood_b)
    got = [probe.feature_scores(x, distances=True) for x in xs]
    feats = np.concatenate([probe.features(x).cpu().numpy() for x in xs])
    ref = mr.scores(feats, ft["W"], ft["W0"], ft["Wmu"], ft["Wmu0"], ft["class_count"])
    bm, br, decided = mr.bounds_scores(feats, ft, ref)
    maha, rmaha, pred = (np.concatenate([g[k].cpu().numpy() for g in got]) for k in ("maha", "rmaha", "pred"))
    rm, rr = np.abs(maha - ref["maha"]) / bm, np.abs(rmaha - ref["rmaha"]) / br
    print(f"feature_scores ({kind}): |error| / bound  maha {rm.max():.3f}  rmaha {rr.max():.3f}; decided {decided.mean():.2f}; maha {maha.min():.1f} .. {maha.max():.1f}")
    assert rm.max() <= 1.0 and rr.max() <= 1.0 and np.array_equal(pred[decided], ref["pred"][decided]) and pred.dtype == np.int32
    assert tuple(got[0]["dist"].shape) == (4, 10) and "dist" not in probe.feature_scores(xs[0])

    # evaluate: the stored columns are feature_scores' bits, so the metrics are detect_ref's on them
    stores, metrics_op = [], probe._det_metrics
    probe._det_metrics = lambda scores, ld, flags, N, S, order=None: (stores.append(scores[:, :N].clone()), metrics_op(scores, ld, flags, N, S, order))[1]
    try:
        with_d = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    finally:
        del probe._det_metrics
    store = stores[-1].cpu().numpy()                                         # the OOD question's call sees all 12 rows
    assert store.shape == (len(own) + 2, 12) and store[-2].tobytes() == maha.tobytes() and store[-1].tobytes() == rmaha.tobytes()
    twice = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    assert same(with_d, twice)
    det = with_d["detection"]
    assert det["columns"] == list(own) + ["maha", "rmaha"] and (det["n"], det["n_ood"]) == (7, 5)
    y_eval = np.concatenate([y.numpy() for _, y in eval_b])
    wrong = (np.concatenate([probe.logits(x).cpu().numpy() for (x, _), _ in eval_b]).argmax(1) != y_eval).astype(np.uint8)
    assert det["n_wrong"] == int(wrong.sum())
    cols = np.stack([maha, rmaha])
    mis, _ = dr.table(cols[:, :7], wrong)
    ood, _ = dr.table(cols, np.concatenate([np.zeros(7, dtype=np.uint8), np.ones(5, dtype=np.uint8)]))
    for s, name in enumerate(("maha", "rmaha")):
        print(f"  {name}: misclassification {det['misclassification'][name]}  ood {det['ood'][name]}")
        for table, entry, keys in ((mis, det["misclassification"][name], ("AUROC", "AUPR", "FPR95", "AURC")), (ood, det["ood"][name], ("AUROC", "AUPR", "FPR95"))):
            assert tuple(entry) == keys
            for k, key in enumerate(keys):
                r, g = table[s, k], entry[key]
                assert (math.isnan(r) and math.isnan(g)) or abs(g - r) <= (EXACT_TOL if key in ("AUROC", "FPR95") else SUM_TOL), (name, key, g, r)
    assert with_d["maha_acc1"] == 100.0 * int((pred[:7] == y_eval).sum()) / 7 and with_d["maha_mean"] == pytest.approx(mr.maha_mean(maha[:7]), rel=1e-12)

    # every other key is what it was without the density, and the columns of the head itself keep their numbers
    rest = {k: v for k, v in with_d.items() if k not in ("detection", "maha_mean", "maha_acc1")}
    assert same(rest, {k: v for k, v in without.items() if k != "detection"})
    for q in ("misclassification", "ood"):
        assert same({c: det[q][c] for c in own}, without["detection"][q])
    plain = probe.evaluate(eval_b)
    assert "maha_mean" not in plain and "detection" not in plain             # without detection a density launches and returns nothing

    # another shrinkage from the kept sums, a state round trip, and the density cleared
    kept = {k: v.clone() for k, v in got[0].items()}
    looser = probe.set_density_shrinkage(0.1)
    assert looser["shrinkage"] == 0.1 and not torch.equal(probe.feature_scores(xs[0])["maha"], kept["maha"])
    probe.load_density_state(sd)
    assert all(torch.equal(v, kept[k]) for k, v in probe.feature_scores(xs[0], distances=True).items())
    if kind == "lap":
        probe.set_laplace(None)
        assert probe.DETECT_COLUMNS == ("msp", "entropy", "energy", "maha", "rmaha")
        probe.fit_laplace(fit_b, prior_precision=1.0)
        assert probe.DETECT_COLUMNS == own + MAHA_COLUMNS
    probe.set_density(None)
    assert probe.density is None and probe.DETECT_COLUMNS == own
    assert same(probe.evaluate(eval_b, detection=True, ood_loader=ood_b), without)
    for a, b in zip(before, frozen_state(probe)):
        assert torch.equal(a, b)
