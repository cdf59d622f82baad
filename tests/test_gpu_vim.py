"""GPU: the ViM and residual scores (csrc/vim.hip, LinearProbe.fit_vim / vim_scores / vim_batch) against the float64 restatement of
tests/vim_ref.py on the same inputs.  Every bound is derived in vim_ref's docstring from the unit roundoff of the double operations the
kernels perform; none comes from running them.  Every test prints the worst |error| / bound before it asserts."""
import ctypes as C
import math
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

import detect_ref as dr
import vim_ref as vr
from test_gpu_maha import EXACT_TOL, SUM_TOL, batches_of, case, dev, encoder, guarded, intact, make_probe, same, workspace      # noqa: F401
from test_gpu_probe import P, S, frozen_state, ok

pytestmark = pytest.mark.gpu

F32, I32, F64 = torch.float32, torch.int32, torch.float64


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


@lru_cache(maxsize=None)
def shape_case(shape):
    """Per shape, computed once and left unchanged: the case, the restatement at the fit's alpha and its bounds."""
    c = vr.make_case(*shape)
    ft = c["fit"]
    ref = vr.scores(c["feat"], ft["A"], ft["a"], shape[2], ft["alpha"])
    return c, ref, vr.bounds(c["feat"], ft["A"], ft["a"], shape[2], ft["alpha"], ref)


def run_scores(L, feat, A, a, Cn, alpha, labels=None, sums=None):
    """uvit_op_vim_scores on host arrays, on a workspace of exactly the size asked for: (vim, residual, pred, correct or None), the
    outputs behind guards."""
    B, Cd = feat.shape
    K = A.shape[0] - Cn
    vim, res, pred = guarded(B, F32, 3.0), guarded(B, F32, 3.0), guarded(B, I32, 5)
    correct = guarded(1, I32, 0) if labels is not None else None
    ws = workspace(L.uvit_op_vim_scores_ws_bytes(B, Cd, Cn, K))
    fd, Ad, ad, yd = dev(feat), dev(A), dev(a), dev(labels) if labels is not None else None      # held until the synchronize below
    ok(L.uvit_op_vim_scores(P(fd), P(Ad), P(ad), C.c_double(alpha), P(vim), P(res), P(pred), P(yd), P(correct), P(sums), P(ws), ws.numel(), B, Cd, Cn, K, S()))
    torch.cuda.synchronize()
    assert intact(vim, B) and intact(res, B) and intact(pred, B) and (correct is None or intact(correct, 1))
    return vim[:B].cpu().numpy(), res[:B].cpu().numpy(), pred[:B].cpu().numpy(), None if correct is None else int(correct[0])


# ------------------------------------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("shape", vr.SHAPES)
def test_scores(L, shape):
    """vim, residual and pred against vim_ref within the bounds, guard words behind every output, labels / correct, `sums` against
    math.fsum within its bound and added in place over two calls, the same bits on a second run and when the rows are sent as two
    batches, and alpha = 0 giving -lse whatever the residual is."""
    B, Cd, Cn, K = shape
    c, ref, bd = shape_case(shape)
    ft, feat = c["fit"], c["feat"]
    A, a, alpha = ft["A"], ft["a"], ft["alpha"]
    y = np.where(np.arange(B) % 2 == 0, ref["pred"], (ref["pred"] + 1) % K).astype(np.int64)
    sums = guarded(4, F64, 0.0)
    vim, res, pred, correct = run_scores(L, feat, A, a, Cn, alpha, labels=y, sums=sums)
    rv, rr = np.abs(vim - ref["vim"]) / bd["vim"], np.abs(res - ref["residual"]) / bd["residual"]
    _, sm, sr, used, skipped = vr.alpha_of(ref)
    got = sums[:4].cpu().numpy()
    bm, br = vr.bound_sum(ref["zmax"], bd["zmax"]), vr.bound_sum(ref["residual"], bd["residual64"])
    print(f"\nscores {shape}: |error| / bound  vim {rv.max():.3f}  residual {rr.max():.3f}  sum max z {abs(got[0] - sm) / bm:.3f}  "
          f"sum residual {abs(got[1] - sr) / br:.3f}; alpha {alpha:.3f}, residual {ref['residual'].min():.3f} .. {ref['residual'].max():.3f}")
    assert rv.max() < 1.0 and rr.max() < 1.0 and vim.dtype == np.float32 and res.dtype == np.float32
    assert bd["decided"].all() and np.array_equal(pred, ref["pred"]) and pred.dtype == np.int32
    assert correct == int((ref["pred"] == y).sum()) == (B + 1) // 2
    assert abs(got[0] - sm) < bm and abs(got[1] - sr) < br and got[2:].tolist() == [used, skipped] == [B, 0] and intact(sums, 4)
    # a second run: the same bits; its sums are added in place
    v2, r2, p2, _ = run_scores(L, feat, A, a, Cn, alpha, sums=sums)
    assert v2.tobytes() == vim.tobytes() and r2.tobytes() == res.tobytes() and p2.tobytes() == pred.tobytes()
    twice = sums[:4].cpu().numpy()
    assert twice[2:].tolist() == [2 * B, 0] and abs(twice[0] - 2 * sm) < 2 * bm + vr.U * abs(2 * sm) and abs(twice[1] - 2 * sr) < 2 * br + vr.U * abs(2 * sr)
    # the rows in two batches: every row's bits are its own
    if B > 1:
        cut = min(17, B - 1)
        parts = [run_scores(L, feat[s], A, a, Cn, alpha) for s in (slice(0, cut), slice(cut, B))]
        for i, whole in enumerate((vim, res, pred)):
            assert np.concatenate([p[i] for p in parts]).tobytes() == whole.tobytes()
    # alpha = 0: vim = -lse, within the bound of lse, and does not depend on the residual (R scaled by 3 changes it alone)
    ref0 = vr.scores(feat, A, a, Cn, 0.0)
    bd0 = vr.bounds(feat, A, a, Cn, 0.0, ref0)
    v0, r0, _, _ = run_scores(L, feat, A, a, Cn, 0.0)
    A3, a3 = A.copy(), a.copy()
    A3[:Cn] *= 3.0
    a3[:Cn] *= 3.0
    v3, r3, _, _ = run_scores(L, feat, A3, a3, Cn, 0.0)
    assert (np.abs(v0 - (-ref0["lse"])) < bd0["vim"]).all() and r0.tobytes() == res.tobytes() and v3.tobytes() == v0.tobytes()
    assert (r3 != r0).any() or not ref["residual"].any()


@pytest.mark.parametrize("shape", [(17, 12, 11, 3), (130, 132, 1, 65)])
def test_bad_rows(L, shape):
    """A row with a NaN and a row with an inf give NaN, NaN, -1, are counted in sums[3] and left out of the two sums, and every other
    row holds the bits of the call without them."""
    B, Cd, Cn, K = shape
    c, ref, _ = shape_case(shape)
    ft = c["fit"]
    feat = c["feat"].copy()
    feat[2, Cd - 1], feat[B // 2, 0] = np.nan, -np.inf
    dead = np.array([2, B // 2])
    keep = np.setdiff1d(np.arange(B), dead)
    sums, clean_sums = guarded(4, F64, 0.0), guarded(4, F64, 0.0)
    y = ref["pred"].astype(np.int64)
    vim, res, pred, correct = run_scores(L, feat, ft["A"], ft["a"], Cn, ft["alpha"], labels=y, sums=sums)
    cv, cr, cp, _ = run_scores(L, c["feat"][keep], ft["A"], ft["a"], Cn, ft["alpha"], sums=clean_sums)
    assert np.isnan(vim[dead]).all() and np.isnan(res[dead]).all() and (pred[dead] == -1).all() and correct == B - 2
    assert vim[keep].tobytes() == cv.tobytes() and res[keep].tobytes() == cr.tobytes() and pred[keep].tobytes() == cp.tobytes()
    got, clean = sums[:4].cpu().numpy(), clean_sums[:4].cpu().numpy()
    assert got[2:].tolist() == [B - 2, 2] and clean[2:].tolist() == [B - 2, 0] and np.isfinite(got).all()
    rbad = vr.scores(feat, ft["A"], ft["a"], Cn, ft["alpha"])
    bd = vr.bounds(feat, ft["A"], ft["a"], Cn, ft["alpha"], rbad)
    _, sm, sr, used, skipped = vr.alpha_of(rbad)
    assert (used, skipped) == (B - 2, 2)
    assert abs(got[0] - sm) < vr.bound_sum(rbad["zmax"][keep], bd["zmax"][keep]) and abs(got[1] - sr) < vr.bound_sum(rbad["residual"][keep], bd["residual64"][keep])


def test_exact_tie_gives_the_lower_class(L):
    """Two classes with the same weight row and bias have the same fma chain: an exact tie in z.  Where they are the largest, pred is the
    lower of the two; with K = 2 that is every row."""
    shape = (17, 12, 11, 3)
    c, _, _ = shape_case(shape)
    feat, A, a = c["feat"], c["fit"]["A"].copy(), c["fit"]["a"].copy()
    A[13], a[13] = A[12], a[12]                                                # classes 1 and 2 of K = 3
    ref = vr.scores(feat, A, a, 11, 1.0)
    z = ref["y"][:, 11:]
    assert (z[:, 1] == z[:, 2]).all() and (z[:, 1] > z[:, 0]).sum() >= 3 and (z[:, 1] < z[:, 0]).sum() >= 3
    _, _, pred, _ = run_scores(L, feat, A, a, 11, 1.0)
    assert np.array_equal(pred, np.where(z[:, 1] > z[:, 0], 1, 0))
    A2, a2 = np.concatenate([A[:11], A[12:14]]), np.concatenate([a[:11], a[12:14]])
    _, _, pred2, _ = run_scores(L, feat, A2, a2, 11, 1.0)
    assert not pred2.any()


# ----------------------------------------------------------------------------------------------------------------------- meaning
def test_meaning_through_the_probe(L):
    """The hand-made case through load_vim_state + vim_batch + detection_batch: OOD AUROC 1.0 for residual and vim on the shifted rows
    and for vim on the flat rows, as the restatement gives.  The encoder's attention needs an embed dim of at least 64, so the 32
    features are the first 32 of 64, the others zero: the second moment is block diagonal with a zero block, whose directions join
    the null space and add exact zeros to every residual."""
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    K, Cd, Dm, (W, b), (f_fit, y_fit), f_in, f_shift, f_flat = vr.meaning_case(0)
    enc = VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=64, depth=1, num_heads=1, init_values=0.1,
                                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), use_shared_rel_pos_bias=True,
                                               use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(enc, K)
    wide = lambda f: np.concatenate([f, np.zeros((len(f), 64 - Cd), dtype=f.dtype)], axis=1)      # noqa: E731
    ft = vr.fit(*vr.moments(wide(f_fit), y_fit, K), wide(W), b, Dm)
    alpha, sm, sr, used, skipped = vr.alpha_of(vr.scores(wide(f_fit), ft["A"], ft["a"], 64 - Dm))
    t = torch.from_numpy
    info = probe.load_vim_state({"R": t(ft["R"]), "origin": t(ft["origin"]), "weight": t(wide(W)), "bias": t(b), "alpha": alpha, "dim": Dm,
                                 "eigenvalues": t(ft["eigenvalues"]), "sums": torch.tensor([sm, sr, used, skipped], dtype=F64)})
    assert (info["n"], info["skipped"], info["dim"]) == (240, 0, 8)
    inn, shift, flat = (probe.vim_batch(dev(wide(f))) for f in (f_in, f_shift, f_flat))
    flags = torch.cat([torch.zeros(60), torch.ones(60)]).to(torch.uint8).cuda()
    for name, out, want in (("shifted", shift, (1.0, 1.0)), ("flat", flat, (1.0, None))):
        cols = torch.stack([torch.cat([inn["vim"], out["vim"]]), torch.cat([inn["residual"], out["residual"]])]).contiguous()
        table = probe.detection_batch(cols, flags).cpu().numpy()
        print(f"\n{name} rows: OOD AUROC vim {table[0, 0]}, residual {table[1, 0]}")
        assert table[0, 0] == want[0] and (want[1] is None or table[1, 0] == want[1])


# -------------------------------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("kind", ["linear", "gp", "het", "ens", "lap"])
def test_vim_end_to_end(L, case, encoder, kind):
    """fit_vim on three ragged batches, then evaluate(detection=True, ood_loader=...) on two evaluation and two OOD batches, for every
    probe class (GPProbe and HetProbe with an explicit head), alone and beside a density and a bank."""
    from uncertainty_vit_amd.linear_probe import VIM_COLUMNS
    from uncertainty_vit_amd.native import UvitError
    cfg = case[1]
    Cd, K, dim = cfg.embed_dim, 10, 4
    probe = make_probe(encoder, kind)
    fit_b, eval_b = batches_of(cfg, "vim-fit", (5, 4, 3)), batches_of(cfg, "vim-eval!", (4, 3))
    ood_b = batches_of(cfg, "vim-ood", (3, 2), labelled=False)
    probe.features(fit_b[0][0][0])                                            # the first forward builds the engine and its bf16 shadows
    before = frozen_state(probe)
    if kind == "lap":
        probe.fit_laplace(fit_b, prior_precision=1.0)
    own = probe.DETECT_COLUMNS
    without = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    assert without["detection"]["columns"] == list(own) and "vim_mean" not in without
    head = None
    if kind in ("gp", "het"):
        with pytest.raises(UvitError, match="not affine"):
            probe.fit_vim(fit_b, dim=dim)
        W0, b0 = vr.make_head(K, Cd, 5)
        head = (torch.from_numpy(W0), torch.from_numpy(b0))

    # the fit against the restatement: the moments are the density's, R spans numpy's null space, alpha within its bound
    info = probe.fit_vim(fit_b, dim=dim, head=head)
    sd = probe.vim_state_dict()
    W, b = sd["weight"].numpy(), sd["bias"].numpy()
    if kind in ("linear", "lap"):
        assert np.array_equal(W, probe.head.weight.detach().double().cpu().numpy()) and np.array_equal(b, probe.head.bias.detach().double().cpu().numpy())
    elif kind == "ens":
        assert np.array_equal(W, torch.stack([getattr(probe.heads, str(m)).weight.detach().double().cpu() for m in range(3)]).mean(0).numpy())
    dens = probe.fit_density(fit_b)
    dsd = probe.density_state_dict()
    probe.set_density(None)
    assert dens["n"] == 12
    ref_fit = vr.fit(dsd["S"].numpy(), dsd["total_sum"].numpy(), 12.0, W, b, dim)
    R, lam = sd["R"].numpy(), ref_fit["eigenvalues"]
    gap = (lam[Cd - dim] - lam[Cd - dim - 1]) / lam[-1]
    proj = np.abs(R.T @ R - ref_fit["R"].T @ ref_fit["R"]).max()
    print(f"\nfit_vim ({kind}): eigen-gap {gap:.3e} of the largest eigenvalue, projector difference {proj:.3e}, explained {info['explained']:.5f}")
    assert np.abs(R @ R.T - np.eye(Cd - dim)).max() <= 1e-12 and tuple(R.shape) == (Cd - dim, Cd)
    # Davis-Kahan: the two projectors differ by at most 2 |dM| / gap; each eigh is backward stable with |dM| <= p(C) u |M|, and
    # p(C) = C^2 is far above LAPACK's own statement (a modest multiple of C)
    assert gap > 1e-6 and proj <= 4 * Cd * Cd * vr.U / gap
    assert np.abs(sd["origin"].numpy() - ref_fit["origin"]).max() <= 1e-9 * max(1.0, np.abs(ref_fit["origin"]).max())
    assert info == probe.vim and (info["n"], info["skipped"], info["classes"], info["dim"]) == (12, 0, K, dim)
    assert info["explained"] == pytest.approx(ref_fit["explained"], rel=1e-9)
    st = probe._vim
    A, a = st["A"].cpu().numpy(), st["a"].cpu().numpy()
    assert np.array_equal(A, np.concatenate([R, W])) and A.dtype == np.float64
    f_fit = np.concatenate([probe.features(x).cpu().numpy() for (x, _), _ in fit_b])
    rfit = vr.scores(f_fit, A, a, Cd - dim)
    bfit = vr.bounds(f_fit, A, a, Cd - dim, 0.0, rfit)
    alpha, sm, sr, used, skipped = vr.alpha_of(rfit)
    dsm = sum(vr.bound_sum(rfit["zmax"][s], bfit["zmax"][s]) for s in (slice(0, 5), slice(5, 9), slice(9, 12))) + \
        3 * vr.U * np.abs(rfit["zmax"]).sum()                                 # three calls added in turn, against one fsum of the twelve
    dsr = sum(vr.bound_sum(rfit["residual"][s], bfit["residual64"][s]) for s in (slice(0, 5), slice(5, 9), slice(9, 12))) + 3 * vr.U * abs(sr)
    balpha = vr.bound_alpha(alpha, sr, dsm, dsr)
    print(f"  alpha {info['alpha']:.6f}: |error| / bound {abs(info['alpha'] - alpha) / balpha:.3f}; sums {sd['sums'].tolist()}")
    assert abs(info["alpha"] - alpha) < balpha and sd["sums"][2:].tolist() == [12, 0] and sd["alpha"] == info["alpha"] and sr > 0
    assert probe.DETECT_COLUMNS == own + VIM_COLUMNS and len(probe.DETECT_COLUMNS) <= 16

    # moments= from a density on the same data: the bits of the two-pass fit
    probe.fit_vim(fit_b, dim=dim, head=head, moments=dsd)
    sd2 = probe.vim_state_dict()
    assert all(torch.equal(sd2[k], sd[k]) for k in ("R", "origin", "weight", "bias", "eigenvalues", "sums")) and sd2["alpha"] == sd["alpha"]
    with pytest.raises(UvitError):
        probe.fit_vim(fit_b, dim=dim, head=head, moments={**dsd, "S": dsd["S"][:-1]})
    with pytest.raises(UvitError):
        probe.fit_vim(fit_b, dim=Cd, head=head)
    assert probe.vim == info                                                   # a refused fit leaves the one in use

    # vim_scores against the restatement on the probe's own uploaded A
    xs = [x for (x, _), _ in eval_b] + list(ood_b)
    got = [probe.vim_scores(x) for x in xs]
    feats = np.concatenate([probe.features(x).cpu().numpy() for x in xs])
    ref = vr.scores(feats, A, a, Cd - dim, info["alpha"])
    bd = vr.bounds(feats, A, a, Cd - dim, info["alpha"], ref)
    vim, res, pred = (np.concatenate([g[k].cpu().numpy() for g in got]) for k in ("vim", "residual", "pred"))
    rv, rr = np.abs(vim - ref["vim"]) / bd["vim"], np.abs(res - ref["residual"]) / bd["residual"]
    print(f"  vim_scores: |error| / bound  vim {rv.max():.3f}  residual {rr.max():.3f}; decided {bd['decided'].mean():.2f}; vim {vim.min():.2f} .. {vim.max():.2f}")
    assert rv.max() < 1.0 and rr.max() < 1.0 and np.array_equal(pred[bd["decided"]], ref["pred"][bd["decided"]]) and pred.dtype == np.int32
    one = probe.vim_batch(probe.features(xs[0]))
    assert all(torch.equal(one[k], got[0][k]) for k in one) and set(one) == {"vim", "residual", "pred"}

    # evaluate: the stored columns are vim_scores' bits, so the metrics are detect_ref's on them
    stores, metrics_op = [], probe._det_metrics
    probe._det_metrics = lambda scores, ld, flags, N, S, order=None: (stores.append(scores[:, :N].clone()), metrics_op(scores, ld, flags, N, S, order))[1]
    try:
        with_v = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    finally:
        del probe._det_metrics
    store = stores[-1].cpu().numpy()                                          # the OOD question's call sees all 12 rows
    assert store.shape == (len(own) + 2, 12) and store[-2].tobytes() == vim.tobytes() and store[-1].tobytes() == res.tobytes()
    assert same(with_v, probe.evaluate(eval_b, detection=True, ood_loader=ood_b))
    det = with_v["detection"]
    assert det["columns"] == list(own) + ["vim", "residual"] and (det["n"], det["n_ood"]) == (7, 5)
    y_eval = np.concatenate([y.numpy() for _, y in eval_b])
    wrong = (np.concatenate([probe.logits(x).cpu().numpy() for (x, _), _ in eval_b]).argmax(1) != y_eval).astype(np.uint8)
    cols = np.stack([vim, res])
    mis, _ = dr.table(cols[:, :7], wrong)
    ood, _ = dr.table(cols, np.concatenate([np.zeros(7, dtype=np.uint8), np.ones(5, dtype=np.uint8)]))
    for s, name in enumerate(("vim", "residual")):
        print(f"  {name}: misclassification {det['misclassification'][name]}  ood {det['ood'][name]}")
        for table, entry, keys in ((mis, det["misclassification"][name], ("AUROC", "AUPR", "FPR95", "AURC")), (ood, det["ood"][name], ("AUROC", "AUPR", "FPR95"))):
            assert tuple(entry) == keys
            for k, key in enumerate(keys):
                r, g = table[s, k], entry[key]
                assert (math.isnan(r) and math.isnan(g)) or abs(g - r) <= (EXACT_TOL if key in ("AUROC", "FPR95") else SUM_TOL), (name, key, g, r)
    assert with_v["vim_acc1"] == 100.0 * int((pred[:7] == y_eval).sum()) / 7
    assert with_v["vim_mean"] == pytest.approx(math.fsum(vim[:7].astype(np.float64).tolist()) / 7, rel=1e-12)
    if kind == "linear" and np.array_equal(pred[:7], np.concatenate([probe.logits(x).cpu().numpy() for (x, _), _ in eval_b]).argmax(1)):
        assert with_v["vim_acc1"] == with_v["acc1"]                            # the snapshot is the head in use

    # every other key and column is what it was without the ViM state, also beside a density and a bank
    rest = {k: v for k, v in with_v.items() if k not in ("detection", "vim_mean", "vim_acc1")}
    assert same(rest, {k: v for k, v in without.items() if k != "detection"})
    for q in ("misclassification", "ood"):
        assert same({c: det[q][c] for c in own}, without["detection"][q])
    plain = probe.evaluate(eval_b)
    assert "vim_mean" not in plain and "detection" not in plain               # without detection a ViM state launches and returns nothing
    probe.set_vim(None)
    probe.load_density_state(dsd)
    probe.fit_neighbours(fit_b, k=3)
    beside = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    probe.load_vim_state(sd)
    all3 = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    assert all3["detection"]["columns"] == list(own) + ["maha", "rmaha", "knn", "vim", "residual"]
    assert same({k: v for k, v in all3.items() if k not in ("detection", "vim_mean", "vim_acc1")}, {k: v for k, v in beside.items() if k != "detection"})
    for q in ("misclassification", "ood"):
        assert same({c: all3["detection"][q][c] for c in beside["detection"]["columns"]}, beside["detection"][q])
        assert same({c: all3["detection"][q][c] for c in VIM_COLUMNS}, {c: det[q][c] for c in VIM_COLUMNS})
    assert (all3["vim_mean"], all3["vim_acc1"]) == (with_v["vim_mean"], with_v["vim_acc1"])

    # a state round trip, and everything cleared
    assert all(torch.equal(v, got[0][k]) for k, v in probe.vim_scores(xs[0]).items())
    probe.set_density(None)
    probe.set_neighbours(None)
    probe.set_vim(None)
    assert probe.vim is None and probe.DETECT_COLUMNS == own
    assert same(probe.evaluate(eval_b, detection=True, ood_loader=ood_b), without)
    for x, z in zip(before, frozen_state(probe)):
        assert torch.equal(x, z)
