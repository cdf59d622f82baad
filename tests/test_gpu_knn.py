"""GPU: the k-nearest-neighbour score and classifier (csrc/knn.hip, LinearProbe.fit_neighbours / neighbour_scores / neighbour_batch)
against the float64 restatement of tests/knn_ref.py on the same inputs.  Every bound is derived in knn_ref's docstring from the number
formats; none comes from running the kernels.  The search tests print the worst |error| / bound before they assert (the observed
ratios are recorded in DESIGN.md section 9.11)."""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

import detect_ref as dr
import knn_ref as kr
import maha_ref as mr
from test_gpu_maha import EXACT_TOL, SUM_TOL, batches_of, case, dev, encoder, guarded, intact, make_probe, same, workspace      # noqa: F401
from test_gpu_probe import P, S, frozen_state, ok

pytestmark = pytest.mark.gpu

F32, I32, F64 = torch.float32, torch.int32, torch.float64


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def bf16_dev(x):
    """fp32 array of bf16 values -> a bfloat16 device tensor of the same bits."""
    return torch.from_numpy(kr.bf16_bits(x)).view(torch.bfloat16).cuda()


# -------------------------------------------------------------------------------------------------------------------------- rows
def run_rows(L, feat, labels, K, bank_rows=0, row0=0, sums=None):
    """uvit_op_knn_rows on host arrays, written at row `row0` of a guarded bank of max(bank_rows, B) rows filled with 1.0 / label 5:
    (bank fp32 (rows, C), labels int32 (rows), sums or None)."""
    B, Cd = feat.shape
    rows = max(bank_rows, row0 + B)
    out, lab = guarded(rows * Cd, torch.bfloat16, 1.0), guarded(rows, I32, 5)
    fd, yd = dev(feat), dev(labels) if labels is not None else None          # held until the synchronize below
    ok(L.uvit_op_knn_rows(P(fd), P(yd), out.data_ptr() + 2 * row0 * Cd, lab.data_ptr() + 4 * row0, P(sums), B, Cd, K, S()))
    torch.cuda.synchronize()
    assert intact(out, rows * Cd) and intact(lab, rows)
    return out[:rows * Cd].view(rows, Cd).float().cpu().numpy(), lab[:rows].cpu().numpy()


@pytest.mark.parametrize("B,Cd", [(1, 32), (17, 96), (130, 768), (5, 2048)])
def test_rows(L, B, Cd):
    """Every element is one of the restatement's two accepted bf16 values (no tolerance); bad rows (a NaN, an inf, a zero row, a label
    of -1, a label of K) are zero rows labelled -1 and counted, and every other row holds the bits of the call without them; an
    append at a row offset leaves the other rows of the bank as they were; without labels a usable row gets 0; sums add up over calls."""
    rng = np.random.default_rng(70 + B + Cd)
    K = 6
    f = (rng.standard_normal((B, Cd)) * 10.0 ** rng.integers(-3, 4, (B, 1))).astype(np.float32)
    y = rng.integers(0, K, B)
    sums = guarded(2, F64, 0.0)
    got, lab = run_rows(L, f, y, K, bank_rows=B + 7, row0=3, sums=sums)
    lo, hi, want_lab, want_sums = kr.rows(f, y, K)
    g = got[3:3 + B]
    assert ((g == lo) | (g == hi)).all() and np.array_equal(lab[3:3 + B], want_lab)
    print(f"\nrows ({B}, {Cd}): {(lo != hi).sum()} of {lo.size} elements at a rounding boundary, {(g != lo).sum()} took the upper value")
    assert (got[:3] == 1.0).all() and (got[3 + B:] == 1.0).all() and (lab[:3] == 5).all() and (lab[3 + B:] == 5).all()
    assert sums[:2].tolist() == want_sums.tolist() == [B, 0] and intact(sums, 2)
    again, _ = run_rows(L, f, y, K, bank_rows=B + 7, row0=3)
    assert again.tobytes() == got.tobytes()
    plain, plab = run_rows(L, f, None, 0)
    assert plain.tobytes() == g.tobytes() and not plab.any()
    if B >= 17:
        fb, yb = f.copy(), y.copy()
        fb[1, Cd - 1], fb[4, 0], fb[7], yb[9], yb[B - 1] = np.nan, -np.inf, 0.0, -1, K
        bad, blab = run_rows(L, fb, yb, K, sums=sums)
        dead = np.array([1, 4, 7, 9, B - 1])
        keep = np.setdiff1d(np.arange(B), dead)
        assert not bad[dead].any() and (blab[dead] == -1).all() and bad[keep].tobytes() == g[keep].tobytes() and np.array_equal(blab[keep], y[keep])
        assert sums[:2].tolist() == [2 * B - 5, 5]
        assert np.array_equal(blab, kr.rows(fb, yb, K)[2])


# ------------------------------------------------------------------------------------------------------------------------ search
def run_search(L, c, k, slabs, pad=3, valid=None):
    """uvit_op_knn_search on a case of knn_ref: (sim (B, k) fp32, idx (B, k) int32), the outputs behind guards, the padding checked."""
    q, bank, labels = c["q"], c["bank"], c["labels"]
    B, Cd, N, ld = q.shape[0], q.shape[1], bank.shape[0], k + pad
    sim, idx = guarded(B * ld, F32, -2.0), guarded(B * ld, I32, -7)
    nbytes = L.uvit_op_knn_search_ws_bytes(B, Cd, N, k, slabs)
    ws = workspace(nbytes)
    valid = c["valid"] if valid is None else valid
    args = [bf16_dev(q), dev(valid), bf16_dev(bank), dev(labels)]             # held until the synchronize below
    ok(L.uvit_op_knn_search(*(P(a) for a in args), P(sim), P(idx), ld, P(ws), ws.numel(), B, Cd, N, k, slabs, S()))
    torch.cuda.synchronize()
    assert intact(sim, B * ld) and intact(idx, B * ld)
    s, i = sim[:B * ld].view(B, ld).cpu().numpy(), idx[:B * ld].view(B, ld).cpu().numpy()
    assert (s[:, k:] == -2.0).all() and (i[:, k:] == -7).all()
    return np.ascontiguousarray(s[:, :k]), np.ascontiguousarray(i[:, :k])


@lru_cache(maxsize=None)
def searched(shape):
    return kr.search_case(*shape)


@pytest.mark.parametrize("shape", kr.SHAPES)
def test_search(L, shape):
    """sim and idx against the restatement within the derived bounds, for slabs in {1, 3, 7, 0}: equal bits across them and on a second
    run; the padding (ld = k + 3) untouched; every query whose bank row is live reports it first (the lower index of a duplicate
    pair), dead rows never appear, fewer than k live rows leave -inf / -1."""
    B, Cd, N, k = shape
    c = searched(shape)
    runs = [run_search(L, c, k, slabs) for slabs in kr.SLABS]
    sim, idx = runs[0]
    worst = kr.check_search(sim, idx, c["q"], c["valid"], c["bank"], c["labels"], k, what=str(shape))
    for slabs, (s2, i2) in zip(kr.SLABS[1:], runs[1:]):
        assert s2.tobytes() == sim.tobytes() and i2.tobytes() == idx.tobytes(), slabs
    s2, i2 = run_search(L, c, k, 3, pad=0)
    assert s2.tobytes() == sim.tobytes() and i2.tobytes() == idx.tobytes()
    own = c["first"] >= 0
    assert np.array_equal(idx[own, 0], c["first"][own])
    if N >= 9 and B > 1:
        assert idx[1, 1] == N - 2 and sim[1, 0] == sim[1, 1]                   # duplicated bank rows: the lower index first
    assert worst <= 1.0


def test_search_invalid_query_and_no_live_row(L):
    """Invalid query rows get NaN / -1 and leave their neighbours' bits; a bank without a live row gives -inf / -1 throughout."""
    shape = (17, 96, 127, 5)
    c = searched(shape)
    sim, idx = run_search(L, c, 5, 3)
    valid = c["valid"].copy()
    valid[[0, 8, 16]] = -1
    s2, i2 = run_search(L, c, 5, 3, valid=valid)
    keep = valid >= 0
    assert np.isnan(s2[~keep]).all() and (i2[~keep] == -1).all()
    assert s2[keep].tobytes() == sim[keep].tobytes() and i2[keep].tobytes() == idx[keep].tobytes()
    kr.check_search(s2, i2, c["q"], valid, c["bank"], c["labels"], 5, what="with three invalid queries")
    s3, i3 = run_search(L, {**c, "labels": np.full(127, -1, dtype=np.int32)}, 5, 0)
    assert np.isneginf(s3).all() and (i3 == -1).all()


def test_search_exact_ties_are_ordered_by_index(L):
    """Whole-number rows (exact in bf16, every product and sum exact in fp32): the similarities equal the restatement's bit for bit and
    the many equal ones are ordered by index, also across slab borders."""
    rng = np.random.default_rng(4)
    bank = rng.integers(-2, 3, (300, 64)).astype(np.float32)
    labels = np.where(np.arange(300) % 5 == 2, -1, 0).astype(np.int32)
    c = {"q": bank[:20].copy(), "valid": np.zeros(20, dtype=np.int32), "bank": bank, "labels": labels}
    ref_s, ref_i = kr.search(c["q"], c["valid"], bank, labels, 100)
    for slabs in (1, 5):
        sim, idx = run_search(L, c, 100, slabs)
        assert np.array_equal(sim.astype(np.float64), ref_s) and np.array_equal(idx, ref_i), slabs
    assert (np.diff(ref_s[0]) == 0).sum() > 30


# ------------------------------------------------------------------------------------------------------------------------ scores
def run_scores(L, sim, idx, lab, K, T, votes=True, pad=0, labels=None):
    B, k = sim.shape
    N, ldv = len(lab), K + pad
    knn, pred = guarded(B, F32, -1.0), guarded(B, I32, -5)
    v = guarded(B * ldv, F64, -2.0) if votes else None
    correct = guarded(1, I32, 0) if labels is not None else None
    yd = dev(labels) if labels is not None else None
    sd, xd, ld_ = dev(sim), dev(idx), dev(lab)                                # held until the synchronize below
    ok(L.uvit_op_knn_scores(P(sd), P(xd), k, P(ld_), N, P(knn), P(pred), P(v), ldv, P(yd), P(correct), B, k, K, T, S()))
    torch.cuda.synchronize()
    assert intact(knn, B) and intact(pred, B) and (v is None or intact(v, B * ldv)) and (correct is None or intact(correct, 1))
    vv = v[:B * ldv].view(B, ldv).cpu().numpy() if votes else None
    return knn[:B].cpu().numpy(), pred[:B].cpu().numpy(), vv, None if correct is None else int(correct[0])


def check_scores(L, sim, idx, lab, K, T, y, what):
    knn, pred, v, correct = run_scores(L, sim, idx, lab, K, T, pad=3, labels=y)
    rv, bound, rpred, decided = kr.votes(sim, idx, lab, K, T)
    assert knn.tobytes() == kr.knn_score(sim[:, -1]).tobytes()
    live = ~np.isnan(rv[:, 0])
    ratio = (np.abs(v[live, :K] - rv[live]) / np.maximum(bound[live], 1e-300)).max(initial=0.0)
    print(f"\nscores {what}: worst |votes error| / bound {ratio:.4f}; decided {decided.mean():.3f}")
    assert ratio <= 1.0 and np.isnan(v[~live, :K]).all() and (v[:, K:] == -2.0).all()
    assert np.array_equal(pred[decided], rpred[decided]) and correct == int((pred == y).sum())
    k2, p2, _, _ = run_scores(L, sim, idx, lab, K, T, votes=False)
    assert k2.tobytes() == knn.tobytes() and p2.tobytes() == pred.tobytes()
    return pred, decided


def test_scores_hand_made(L):
    """An exact tie goes to the lower class; a missing k-th entry and a NaN row give NaN / -1 and NaN votes."""
    sim, idx, lab, K, T, want = kr.scores_cases()
    pred, _ = check_scores(L, sim, idx, lab, K, T, np.array([1, 1, 0, 0]), "hand-made")
    assert pred.tolist() == want
    knn, _, v, _ = run_scores(L, sim, idx, lab, K, T)
    assert knn[:2].tolist() == [1.5, 1.0] and np.isnan(knn[2:]).all() and v[0, 1] == v[0, 2] and v[0, 0] == 0.0 and v[1, 0] == 1.0


@pytest.mark.parametrize("shape", [s for s in kr.SHAPES if s != (5, 32, 9, 9)])
def test_scores_on_the_search_output(L, shape):
    """The device's own sim / idx through the scores op: knn bit for bit, votes within the bound, pred wherever decided (every row)."""
    c = searched(shape)
    sim, idx = run_search(L, c, shape[3], 0, pad=0)
    y = np.random.default_rng(1).integers(0, c["K"], shape[0])
    _, decided = check_scores(L, sim, idx, c["labels"], c["K"], 0.07, y, str(shape))
    assert decided.all()


# ----------------------------------------------------------------------------------------------------------------------- meaning
def test_meaning_through_neighbour_batch_and_detection_batch(L):
    """The synthetic clusters of maha_ref.meaning_case(0), padded to 64 features: OOD AUROC 1.0 for knn and k-NN accuracy 1.0 for
    k in {1, 5, 20}, as the restatement gives on the CPU (tests/test_host_knn.py)."""
    from functools import partial
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    K, _, (f_fit, y_fit), (f_in, y_in), f_out = mr.meaning_case(0)
    enc = VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=64, depth=1, num_heads=1, init_values=0.1,
                                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), use_shared_rel_pos_bias=True,
                                               use_abs_pos_emb=False).cuda().eval()
    probe = LinearProbe(enc, K)
    bank, lab = run_rows(L, kr.meaning_rows(f_fit), y_fit, K)
    state = {"bank": bf16_dev(bank).cpu(), "labels": torch.from_numpy(lab), "sums": torch.tensor([240.0, 0.0], dtype=F64), "k": 1, "temperature": 0.07}
    assert probe.load_neighbour_state(state)["n"] == 240
    for k in (1, 5, 20):
        probe.set_neighbours_k(k)
        inn = probe.neighbour_batch(dev(kr.meaning_rows(f_in)), neighbours=True)
        out = probe.neighbour_batch(dev(kr.meaning_rows(f_out)))
        assert tuple(inn["sim"].shape) == (60, k) and inn["idx"].dtype == I32 and set(out) == {"knn", "pred"}
        flags = torch.cat([torch.zeros(60), torch.ones(60)]).to(torch.uint8).cuda()
        table = probe.detection_batch(torch.cat([inn["knn"], out["knn"]]).contiguous(), flags).cpu().numpy()
        acc = float((inn["pred"].cpu().numpy() == y_in).mean())
        print(f"\nk {k}: OOD AUROC knn {table[0, 0]}; k-NN accuracy {acc}")
        assert table[0, 0] == 1.0 and acc == 1.0


# -------------------------------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("kind", ["linear", "gp", "het", "ens", "lap"])
def test_neighbours_end_to_end(L, case, encoder, kind):
    """fit_neighbours on three ragged batches with k = 3, then evaluate(detection=True, ood_loader=...) on two evaluation and two OOD
    batches, for every probe class (the Laplace probe with a Laplace fit), alone and with a density set at the same time."""
    from uncertainty_vit_amd.linear_probe import KNN_COLUMNS, MAHA_COLUMNS
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
    assert without["detection"]["columns"] == list(own) and "knn_mean" not in without

    # the fit: the bank holds one of the two accepted values of the probe's own features, row for row
    info = probe.fit_neighbours(fit_b, k=3)
    assert info == probe.neighbours == {"n": 12, "skipped": 0, "classes": 10, "k": 3, "temperature": 0.07}
    sd = probe.neighbour_state_dict()
    f_fit = np.concatenate([probe.features(x).cpu().numpy() for (x, _), _ in fit_b])
    y_fit = np.concatenate([y.numpy() for _, y in fit_b])
    lo, hi, lab, sums = kr.rows(f_fit, y_fit, 10)
    bank = sd["bank"].float().numpy()
    assert tuple(bank.shape) == (12, cfg.embed_dim) and ((bank == lo) | (bank == hi)).all()
    assert np.array_equal(sd["labels"].numpy(), lab) and sd["sums"].tolist() == sums.tolist() and (sd["k"], sd["temperature"]) == (3, 0.07)
    assert probe.DETECT_COLUMNS == own + KNN_COLUMNS

    # neighbour_scores against the restatement on the stored bank and the probe's own features
    xs = [x for (x, _), _ in eval_b] + list(ood_b)
    got = [probe.neighbour_scores(x, neighbours=True) for x in xs]
    feats = np.concatenate([probe.features(x).cpu().numpy() for x in xs])
    qlo, qhi, qlab, _ = kr.rows(feats)
    knn, pred, sim, idx = (np.concatenate([g[key].cpu().numpy() for g in got]) for key in ("knn", "pred", "sim", "idx"))
    assert sim.shape == (12, 3) and pred.dtype == np.int32 and "sim" not in probe.neighbour_scores(xs[0])
    if (qlo == qhi).all():                                                    # no query element at a rounding boundary: one bf16 query
        kr.check_search(sim, idx, qlo, qlab, bank, lab, 3, what=f"neighbour_scores ({kind})")
    assert knn.tobytes() == kr.knn_score(sim[:, -1]).tobytes()
    _, _, rpred, decided = kr.votes(sim, idx, lab, 10, 0.07)
    assert np.array_equal(pred[decided], rpred[decided])

    # evaluate: the stored column is neighbour_scores' bits, so the metrics are detect_ref's on it
    stores, metrics_op = [], probe._det_metrics
    probe._det_metrics = lambda scores, ld, flags, N, S, order=None: (stores.append(scores[:, :N].clone()), metrics_op(scores, ld, flags, N, S, order))[1]
    try:
        with_k = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    finally:
        del probe._det_metrics
    store = stores[-1].cpu().numpy()
    assert store.shape == (len(own) + 1, 12) and store[-1].tobytes() == knn.tobytes()
    assert same(with_k, probe.evaluate(eval_b, detection=True, ood_loader=ood_b))
    det = with_k["detection"]
    assert det["columns"] == list(own) + ["knn"] and (det["n"], det["n_ood"]) == (7, 5)
    y_eval = np.concatenate([y.numpy() for _, y in eval_b])
    wrong = (np.concatenate([probe.logits(x).cpu().numpy() for (x, _), _ in eval_b]).argmax(1) != y_eval).astype(np.uint8)
    mis, _ = dr.table(knn[None, :7], wrong)
    ood, _ = dr.table(knn[None, :], np.concatenate([np.zeros(7, dtype=np.uint8), np.ones(5, dtype=np.uint8)]))
    print(f"  knn ({kind}): misclassification {det['misclassification']['knn']}  ood {det['ood']['knn']}")
    for table, entry, keys in ((mis, det["misclassification"]["knn"], ("AUROC", "AUPR", "FPR95", "AURC")), (ood, det["ood"]["knn"], ("AUROC", "AUPR", "FPR95"))):
        assert tuple(entry) == keys
        for j, key in enumerate(keys):
            r, g = table[0, j], entry[key]
            assert (math.isnan(r) and math.isnan(g)) or abs(g - r) <= (EXACT_TOL if key in ("AUROC", "FPR95") else SUM_TOL), (key, g, r)
    assert with_k["knn_acc1"] == 100.0 * int((pred[:7] == y_eval).sum()) / 7 and with_k["knn_mean"] == pytest.approx(kr.knn_mean(knn[:7]), rel=1e-12)

    # every other key and column is what it was without the bank
    rest = {key: v for key, v in with_k.items() if key not in ("detection", "knn_mean", "knn_acc1")}
    assert same(rest, {key: v for key, v in without.items() if key != "detection"})
    for q in ("misclassification", "ood"):
        assert same({c: det[q][c] for c in own}, without["detection"][q])
    plain = probe.evaluate(eval_b)
    assert "knn_mean" not in plain and "detection" not in plain               # without detection a bank launches and returns nothing

    # with a density at the same time: its columns in front, every number of either unchanged
    probe.fit_density(fit_b)
    assert probe.DETECT_COLUMNS == own + MAHA_COLUMNS + KNN_COLUMNS and len(probe.DETECT_COLUMNS) <= 11
    both = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    probe.set_neighbours(None)
    dens_only = probe.evaluate(eval_b, detection=True, ood_loader=ood_b)
    assert both["detection"]["columns"] == list(own) + ["maha", "rmaha", "knn"]
    assert same({key: v for key, v in both.items() if key not in ("detection", "knn_mean", "knn_acc1")}, {key: v for key, v in dens_only.items() if key != "detection"})
    assert (both["knn_mean"], both["knn_acc1"]) == (with_k["knn_mean"], with_k["knn_acc1"])
    for q in ("misclassification", "ood"):
        assert same(both["detection"][q]["knn"], det[q]["knn"])
        assert same({c: both["detection"][q][c] for c in own + MAHA_COLUMNS}, dens_only["detection"][q])
    probe.set_density(None)

    # the state round trip gives equal bits; another k without a refit; the bank cleared
    probe.load_neighbour_state(sd)
    back = probe.neighbour_scores(xs[0], neighbours=True)
    assert all(torch.equal(v, got[0][key]) for key, v in back.items())
    assert probe.set_neighbours_k(1)["k"] == 1
    one = probe.neighbour_scores(xs[0], neighbours=True)
    assert tuple(one["sim"].shape) == (4, 1) and torch.equal(one["sim"][:, 0], got[0]["sim"][:, 0]) and torch.equal(one["idx"][:, 0], got[0]["idx"][:, 0])
    probe.set_neighbours(None)
    assert probe.neighbours is None and probe.DETECT_COLUMNS == own
    assert same(probe.evaluate(eval_b, detection=True, ood_loader=ood_b), without)
    for a, b in zip(before, frozen_state(probe)):
        assert torch.equal(a, b)
