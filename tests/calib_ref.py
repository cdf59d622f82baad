"""Test helper: the calibration metrics of csrc/calib.hip restated in float64 numpy on given fp32 probabilities, with the kernels'
comparison rule -- an fp32 probability is widened to float64 and compared with a float64 bound -- so that bin membership is the
same by construction and only the order of the sums differs.  Each function cites the reference lines it follows
(uncertainty_evaluations.py); tests/test_host_calib.py pins it to tests/golden/calib.npz, which the reference classes wrote.
ECE and TACE come in two readings of the bin accuracy (positional_acc, see _bin_acc): the reference's own, and the mean over the
rows of the bin.  numpy only."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)            # torch.finfo(torch.float32).eps = 2^-23: Categorical's clamp


def _widen(probs):
    p32 = np.asarray(probs)
    assert p32.dtype == np.float32 and p32.ndim == 2, "the metrics take (B, K) fp32 probabilities"
    return p32.astype(np.float64)


def _labels(labels, K):
    y = np.asarray(labels).astype(np.int64)
    return y, (y >= 0) & (y < K)


def softmax(logits):
    """Row softmax in float64 (the reference for uvit_op_calib_softmax)."""
    z = np.asarray(logits).astype(np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _bin_acc(hit, m, positional_acc):
    """Accuracy of a bin with member mask m.  positional_acc False: the mean of `hit` over the rows of the bin.  True: what the
    reference's `accuracies[in_bin]` computes (uncertainty_evaluations.py:184), where in_bin is a uint8 0/1 array (np.greater on a torch
    tensor comes back through Tensor.__array_wrap__ as uint8) and numpy indexes with an integer array by position, not as a mask:
    the mean over ALL rows b of hit[in_bin[b]], i.e. (count hit[1] + (B - count) hit[0]) / B.  At B = 1 the reference cannot index
    row 1; hit[1] is then hit[0].  The kernels' positional_acc argument (include/uvit.h) selects the same two readings."""
    return hit[np.minimum(m.astype(np.int64), len(hit) - 1)].mean() if positional_acc else hit[m].mean()


def confidence(probs, labels, n_bins=15, positional_acc=False):
    """MaxProbCELoss / ECELoss (uncertainty_evaluations.py:134-202) and NLL (:270-272) -> dict with conf, pred, correct (per row),
    table (n_bins, 3) = (prop, acc, conf), ECE, nll_rows, NLL.  Bin i holds lo_i < conf <= up_i with the bounds of np.linspace;
    pred is the lowest index of the row maximum.  NLL: Categorical(probs) renormalises and clamps to [eps, 1 - eps] before the log.
    A label outside [0, K): ECE and NLL are NaN."""
    p = _widen(probs)
    B, K = p.shape
    y, valid = _labels(labels, K)
    conf, pred = p.max(1), p.argmax(1)
    correct = valid & (pred == y)
    bounds = np.linspace(0, 1, n_bins + 1)
    table = np.zeros((n_bins, 3))
    for i in range(n_bins):
        m = (conf > bounds[i]) & (conf <= bounds[i + 1])
        if m.any():
            table[i] = (m.sum() / B, _bin_acc(correct.astype(np.float64), m, positional_acc), conf[m].mean())
    ece = float(np.dot(table[:, 0], np.abs(table[:, 2] - table[:, 1])))
    py = np.where(valid, p[np.arange(B), np.where(valid, y, 0)], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):             # an all-zero row: 0 / 0, NaN as on the device
        nll_rows = np.where(valid, -np.log(np.clip(py / p.sum(1), EPS, 1.0 - EPS)), np.nan)
    bad = not valid.all()
    return {"conf": conf, "pred": pred, "correct": correct.astype(np.int32), "table": table, "bounds": bounds,
            "ECE": float("nan") if bad else ece, "nll_rows": nll_rows, "NLL": float(nll_rows.mean())}


def tace(probs, labels, threshold=0.01, n_bins=30, positional_acc=False):
    """TACELoss (uncertainty_evaluations.py:112-132, 159-186, 241-261) -> (TACE, per_class (K,)).  Per class: values under the
    threshold become 0, the bounds are every (B // n_bins)-th sorted value plus 1.0, bin i holds lo_i < v <= up_i."""
    p = _widen(probs)
    B, K = p.shape
    y, valid = _labels(labels, K)
    v = np.where(p < threshold, 0.0, p)
    bin_n = B // n_bins
    per_class = np.zeros(K)
    for c in range(K):
        col = v[:, c]
        s = np.sort(col)
        bounds = np.append(s[np.arange(n_bins) * bin_n], 1.0)
        hit = (y == c).astype(np.float64)
        for i in range(n_bins):
            m = (col > bounds[i]) & (col <= bounds[i + 1])
            if m.any():
                per_class[c] += (m.sum() / B) * abs(col[m].mean() - _bin_acc(hit, m, positional_acc))
    return (float("nan") if not valid.all() else float(per_class.sum() / K)), per_class


def auroc(probs, labels):
    """One-vs-rest AUROC over the classes present in the batch -> dict with u2, n_pos, first (per row, integers), per_class
    {c: AUC_c} for the classes with a positive and a negative row, sum and count.  AUC_c = P(p_pos > p_neg) + P(p_pos == p_neg) / 2."""
    p = _widen(probs)
    B, K = p.shape
    y, valid = _labels(labels, K)
    u2, n_pos, first = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    per_class, total = {}, 0.0
    for i in range(B):
        if not valid[i]:
            continue
        c = int(y[i])
        neg = y != c
        col = p[:, c]
        u2[i] = int(2 * (col[i] > col[neg]).sum() + (col[i] == col[neg]).sum())
        n_pos[i] = int((~neg).sum())
        first[i] = int(not (y[:i] == c).any())
        n_neg = B - int(n_pos[i])
        if n_neg >= 1:
            t = u2[i] / (2.0 * n_pos[i] * n_neg)
            per_class[c] = per_class.get(c, 0.0) + t
            total += t
    count = len(per_class)
    return {"u2": u2, "n_pos": n_pos, "first": first, "per_class": per_class, "sum": float("nan") if not valid.all() else total,
            "count": count}


def batch_metrics(probs, labels, ece_bins=15, tace_bins=30, tace_threshold=0.01, positional_acc=False):
    """The four per-batch numbers of the reference's evaluate() (engine_for_finetuning.py:199-204); AUROC = sum / count (NaN when no
    class has both a positive and a negative row)."""
    cf = confidence(probs, labels, ece_bins, positional_acc)
    t, _ = tace(probs, labels, tace_threshold, tace_bins, positional_acc)
    a = auroc(probs, labels)
    return {"ECE": cf["ECE"], "TACE": t, "NLL": cf["NLL"], "AUROC": a["sum"] / a["count"] if a["count"] else float("nan"),
            "auroc_sum": a["sum"], "auroc_count": a["count"]}


def weighted(per_batch, sizes, K):
    """The reference's meters (engine_for_finetuning.py:207-213): batch-size-weighted means of the per-batch values; a batch without an
    AUROC (count 0) is left out of the AUROC mean only.  AUROC_zero_absent: the mean of sum / K."""
    n = float(sum(sizes))
    out = {k: sum(m[k] * b for m, b in zip(per_batch, sizes)) / n for k in ("ECE", "TACE", "NLL")}
    have = [(m, b) for m, b in zip(per_batch, sizes) if m["auroc_count"] > 0]
    out["AUROC"] = sum(m["auroc_sum"] / m["auroc_count"] * b for m, b in have) / sum(b for _, b in have) if have else float("nan")
    out["AUROC_zero_absent"] = sum(m["auroc_sum"] / K * b for m, b in zip(per_batch, sizes)) / n
    return out
