"""Test helper: the set-level calibration metrics of csrc/setcalib.hip restated in float64 numpy on given fp32 probabilities, with the
kernels' comparison rule (an fp32 probability widened to float64 against a float64 bound), so that bin membership is the same by
construction and only the order of the sums differs.  `confidence` and `tace` are calib_ref's; this adds MCE, OE (MCELoss, OELoss:
uncertainty_evaluations.py:205-220), SCE (SCELoss :223-241), ACE (ACELoss :264-268), Brier (BrierScore :99-109, on probabilities),
the per-class AUROC and the bad-row rule.  `positional_acc` exists for pinning to the reference's own numbers only
(tests/test_host_scal.py); the device computes the reading positional_acc=False.  numpy only."""
import numpy as np

import calib_ref as cr

OUT_KEYS = ("ECE", "MCE", "OE", "NLL", "Brier", "SCE", "ACE", "TACE", "AUROC", "auroc_classes", "acc", "mean_conf", "n", "n_bad")


def probs_from_grid_logits(q, with_margin=False):
    """The fp32 probabilities of tests/golden/scal.npz from its int8 logits (z = q / 2): the float64 softmax exp(z - max) / sum with the
    sum added left to right, rounded once to fp32.  Everything but exp is exact IEEE arithmetic; tools/gen_golden_scal.py keeps only
    cases in which no float64 value lies within 2^-40 (relative) of a midpoint between two fp32 values, which `with_margin` reports."""
    z = np.asarray(q).astype(np.float64) / 2.0
    e = np.exp(z - z.max(1, keepdims=True))
    s = e[:, 0].copy()
    for k in range(1, e.shape[1]):
        s = s + e[:, k]
    p = e / s[:, None]
    p32 = p.astype(np.float32)
    if not with_margin:
        return p32
    ulp = np.spacing(np.abs(p32)).astype(np.float64)
    off = np.abs(np.abs(p - p32.astype(np.float64)) - ulp / 2)           # distance from the midpoint on either side
    return p32, bool((off > p * 2.0 ** -40).all())


def sce(probs, labels, n_bins=15, positional_acc=False):
    """SCELoss -> (SCE, per_class (K,)): per class the equal-width bins lo < p[:, c] <= up with hit = [y == c]."""
    p = cr._widen(probs)
    N, K = p.shape
    y, _ = cr._labels(labels, K)
    bounds = np.linspace(0, 1, n_bins + 1)
    per_class = np.zeros(K)
    for c in range(K):
        col, hit = p[:, c], (y == c).astype(np.float64)
        for i in range(n_bins):
            m = (col > bounds[i]) & (col <= bounds[i + 1])
            if m.any():
                per_class[c] += (m.sum() / N) * abs(col[m].mean() - cr._bin_acc(hit, m, positional_acc))
    return float(per_class.sum() / K), per_class


def brier_rows(probs, labels):
    """sum_k (p_k - [k == y])^2 per row; a label outside [0, K) has no one-hot entry."""
    p = cr._widen(probs)
    N, K = p.shape
    y, valid = cr._labels(labels, K)
    one_hot = np.zeros((N, K))
    one_hot[np.arange(N)[valid], y[valid]] = 1.0
    return ((p - one_hot) ** 2).sum(1)


def auroc_classes(probs, labels):
    """(auroc (K,), n_pos (K,)): AUROC_c = P(p_pos > p_neg) + P(p_pos == p_neg) / 2 from integer pair counts (ranks of the sorted
    column), NaN without a positive or without a negative row."""
    p = cr._widen(probs)
    N, K = p.shape
    y, _ = cr._labels(labels, K)
    out, n_pos = np.full(K, np.nan), np.zeros(K, np.int64)
    for c in range(K):
        col, pos = p[:, c], y == c
        n_pos[c] = int(pos.sum())
        n_neg = N - int(n_pos[c])
        if n_pos[c] and n_neg:
            neg = np.sort(col[~pos])
            below = np.searchsorted(neg, col[pos], side="left").astype(np.int64)
            upto = np.searchsorted(neg, col[pos], side="right").astype(np.int64)
            out[c] = int((below + upto).sum()) / (2.0 * int(n_pos[c]) * n_neg)
    return out, n_pos


def metrics(probs, labels, ece_bins=15, cw_bins=15, ace_bins=15, tace_bins=30, tace_threshold=0.01, positional_acc=False):
    """Everything uvit_op_scal_metrics writes -> dict with `out` (16,), `top_table` (ece_bins, 3), `per_class` (K, 6) and the named
    entries of OUT_KEYS.  One bad row (a label outside [0, K) or a probability that is not finite) makes out[0 .. 11] NaN."""
    p32 = np.asarray(probs)
    p = cr._widen(p32)
    N, K = p.shape
    y, valid = cr._labels(labels, K)
    bad = ~valid | ~np.isfinite(p).all(1)
    n_bad = int(bad.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        cf = cr.confidence(p32, y, ece_bins, positional_acc)
        table = cf["table"]
        gap = np.abs(table[:, 2] - table[:, 1])
        ece, mce = float(np.dot(table[:, 0], gap)), float(gap.max())
        oe = float(np.dot(table[:, 0], table[:, 2] * np.maximum(table[:, 2] - table[:, 1], 0.0)))
        sce_v, sce_c = sce(p32, y, cw_bins, positional_acc)
        _, ace_c = cr.tace(p32, y, 0.0, ace_bins, positional_acc)
        _, tace_c = cr.tace(p32, y, tace_threshold, tace_bins, positional_acc)
        auc, n_pos = auroc_classes(p32, y)
        brier = float(brier_rows(p32, y).mean())
    have = int(np.isfinite(auc).sum())
    per_class = np.stack([sce_c, ace_c, tace_c, auc, n_pos.astype(np.float64), (p >= tace_threshold).sum(0).astype(np.float64)], axis=1)
    vals = [ece, mce, oe, float(cf["nll_rows"].mean()), brier, sce_v, float(ace_c.sum() / K), float(tace_c.sum() / K),
            float(np.nansum(auc) / have) if have else float("nan"), float(have), float(cf["correct"].sum() / N), float(cf["conf"].mean())]
    if n_bad:
        vals = [float("nan")] * 12
    out = np.array(vals + [float(N), float(n_bad), 0.0, 0.0])
    res = dict(zip(OUT_KEYS, out[:14]))
    res.update(out=out, top_table=table, per_class=per_class)
    return res
