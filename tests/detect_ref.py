"""Test helper: the detection ops of csrc/detect.hip restated in float64 numpy -- the three row scores of a batch of logits with the
error bounds of the kernel's fp32 steps, and the four set-level metrics of one column of fp32 scores.  numpy only.

Metrics.  Columns are ranked as fp32: the restatement sorts the fp32 values with np.lexsort((index, score)), so ties in score go to
the lower sample index, -0 is +0 (the comparison of the values says so), NaN scores are left out and listed last by index.  Tie
groups are runs of equal value.  Walking from the most uncertain end, with TP_i and FP_i the cumulative positives and negatives at
the end of group i and P, Nn the totals over the n ranked samples:
    AUROC = sum_i (FP_i - FP_{i-1}) (TP_i + TP_{i-1}) / (2 P Nn)          Python integers, one division
    AUPR  = sum_i ((TP_i - TP_{i-1}) / P) TP_i / (TP_i + FP_i)            average precision
    FPR95 = FP_i / Nn at the first group with TP_i >= ceil(19 P / 20)     TP / P >= 0.95 in integers
    AURC  = (1 / n) sum_{k=1..n} (positives among the k least uncertain) / k
positive = flag 1; a flag >= 2 (a bad label) anywhere makes all four NaN.

Row scores, bounds (u = 2^-24, derived, not tuned).  The kernel forms d_k = fl(z_k - m) (|error| <= u |d_k|), e_k = expf(d_k) (at
most 1 ulp: relative 2^-23) and from there on works in double: S = sum e_k, T = sum e_k d_k, msp = 1 - 1 / S, entropy = log S - T / S,
energy = -(m + log S), each rounded once to fp32 (u relative).  So e_k carries the relative error eta_k <= 2^-23 + u |d_k| and S the
relative error rho <= 2^-23 + u A + K 2^-126 / S (A = sum_k p_k |d_k|; the last term: e_k below the fp32 normal range) + 2^-50 for
the double sums.  Then
    |msp - ref|     <= max_k p_k rho + u |ref|                                      d(1 / S) = (1 / S) rho
    |energy - ref|  <= rho + u |ref|                                                d(log S) = rho
    |entropy - ref| <= rho + (2^-23 + rho + u) A + u A2 + u |ref|,  A2 = sum_k p_k d_k^2      T / S = sum_k p~_k d_k, p~_k off by eta_k + rho
plus 1e-15 each for the double arithmetic of the restatement itself."""
import numpy as np

U = 2.0 ** -24
ROW_COLUMNS = ("msp", "entropy", "energy")
MAX_N, MAX_S = 1 << 20, 16


def row_scores(z, labels=None):
    """z (B, K) fp32.  Returns (scores (3, B) float64, bounds (3, B) float64, flags (B,) uint8 or None)."""
    z = np.asarray(z, dtype=np.float32)
    B, K = z.shape
    x = z.astype(np.float64)
    m = x.max(1, keepdims=True)
    d = x - m
    e = np.exp(d)
    S = e.sum(1)
    p = e / S[:, None]
    logS = np.log(S)
    msp = 1.0 - 1.0 / S
    with np.errstate(invalid="ignore", divide="ignore"):
        ent = -np.where(p > 0, p * (d - logS[:, None]), 0.0).sum(1)
    ent = np.maximum(ent, 0.0)
    energy = -(m[:, 0] + logS)
    A = (p * np.abs(d)).sum(1)
    A2 = (p * d * d).sum(1)
    rho = 2.0 ** -23 + U * A + K * 2.0 ** -126 / S + 2.0 ** -50
    bounds = np.stack([p.max(1) * rho + U * np.abs(msp), rho + (2.0 ** -23 + rho + U) * A + U * A2 + U * np.abs(ent), rho + U * np.abs(energy)]) + 1e-15
    flags = None
    if labels is not None:
        y = np.asarray(labels, dtype=np.int64)
        pred = z.argmax(1)                                   # the lowest index attaining the maximum
        flags = np.where((y < 0) | (y >= K), 2, (pred != y).astype(np.int64)).astype(np.uint8)
    return np.stack([msp, ent, energy]), bounds, flags


def order_of(scores):
    """(order (N,) int64: the sample indices in ascending (score, index) order with the NaN rows last by index, n ranked)."""
    s = np.asarray(scores, dtype=np.float32)
    idx = np.arange(s.shape[0], dtype=np.int64)
    nan = np.isnan(s)
    good = idx[~nan]
    sv = s[good] + np.float32(0.0)                           # -0 + 0 = +0
    return np.concatenate([good[np.lexsort((good, sv))], idx[nan]]), int(good.shape[0])


def metrics(scores, flags):
    """One column.  Returns {"AUROC", "AUPR", "FPR95", "AURC", "n", "P", "nan", "order"}."""
    s = np.asarray(scores, dtype=np.float32)
    f = np.asarray(flags, dtype=np.uint8)
    N = s.shape[0]
    order, n = order_of(s)
    ranked = order[:n]
    pos = f[ranked] == 1
    P = int(pos.sum())
    Nn = n - P
    out = {"AUROC": np.nan, "AUPR": np.nan, "FPR95": np.nan, "AURC": np.nan, "n": n, "P": P, "nan": N - n, "order": order}
    if bool((f >= 2).any()) or n == 0:
        return out
    out["AURC"] = float((np.cumsum(pos) / np.arange(1, n + 1)).sum() / n)
    if P == 0:
        return out
    vd, pd = (s[ranked] + np.float32(0.0))[::-1], pos[::-1]
    tp, fp = np.cumsum(pd), np.cumsum(~pd)
    ends = np.concatenate([np.nonzero(vd[1:] != vd[:-1])[0], [n - 1]]).astype(np.int64)
    TP, FP = tp[ends].astype(np.int64), fp[ends].astype(np.int64)
    TPp, FPp = np.concatenate([[0], TP[:-1]]), np.concatenate([[0], FP[:-1]])
    out["AUPR"] = float((((TP - TPp) / P) * (TP / (TP + FP))).sum())
    if Nn == 0:
        return out
    num = int(((FP - FPp) * (TP + TPp)).sum())              # int64: at most 2 P Nn <= 2^39
    out["AUROC"] = num / (2.0 * P * Nn)
    need = (19 * P + 19) // 20
    out["FPR95"] = float(FP[int(np.argmax(TP >= need))]) / Nn
    return out


def aurc_brute(scores, flags):
    """AURC by the definition, one coverage at a time."""
    order, n = order_of(scores)
    f = np.asarray(flags)
    total, wrong = 0.0, 0
    for k in range(1, n + 1):
        wrong += int(f[order[k - 1]] == 1)
        total += wrong / k
    return total / n if n else float("nan")


def aurc_perfect(n, P):
    """Closed form when every positive is ranked above every negative: (1 / n) sum_{k = n - P + 1 .. n} (k - (n - P)) / k."""
    return sum((k - (n - P)) / k for k in range(n - P + 1, n + 1)) / n


def table(scores, flags):
    """(S, N) columns -> (S, 8) float64 as uvit_op_detect_metrics writes it, and the (S, N) orders."""
    rows, orders = [], []
    for col in np.atleast_2d(np.asarray(scores, dtype=np.float32)):
        m = metrics(col, flags)
        rows.append([m["AUROC"], m["AUPR"], m["FPR95"], m["AURC"], m["n"], m["P"], m["nan"], 0.0])
        orders.append(m["order"])
    return np.array(rows, dtype=np.float64), np.stack(orders)
