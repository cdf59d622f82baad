"""Test helper: split conformal prediction sets (csrc/conformal.hip) restated in float64 numpy -- the three
scores, the calibration quantile, the sets and the set-level metrics -- and the derived bound on a kernel score's error.  numpy only.

For a row of logits z (K classes, fp32 on input), p = softmax(z) and o_j = the 1-based ordinal rank of class j by descending p, ties to
the smaller index.  p is a strictly increasing function of z, so o_j = 1 + #{i : z_i > z_j} + #{i < j : z_i == z_j} and the restatement
(like the kernel) ranks the fp32 logits themselves: that is exact, where ranking a rounded p could merge or swap close classes.
With a per-row u in [0, 1] (None: 1):
    lac   s_j = 1 - p_j
    aps   s_j = sum_{i : o_i < o_j} p_i + u p_j
    raps  s_j = aps + lam * max(0, o_j - kreg)
Calibration: n usable rows, k = ceil((n + 1) (1 - alpha)), qhat = the k-th smallest label score, +inf (status 1) when k > n.
Prediction: the set is {j : s_j <= qhat}; the row is covered when s_y <= qhat.

The bound delta(K, lam, kreg) on |kernel s_j - float64 s_j| (U = 2^-24; to first order, from the arithmetic the file header of conformal.hip
fixes, not tuned).  The kernel forms d_k = fl32(z_k - m), relative error U, so the argument of the exponential is off by at most
U |d_k|; e_k = expf(d_k), at most 1 ulp: relative 2^-23.  So e_k carries the relative error eta_k <= 2^-23 + U |d_k|.  Everything after
that is double.  Both ranks are exact integers and agree.  A score is a ratio A / S of two sums of e_k (A over the classes ranked
before j plus u e_j; for lac 1 - e_j / S), so
    |d(A / S)| <= |dA| / S + (A / S) |dS| / S <= 2 sum_k p_k eta_k = 2 (2^-23 + U sum_k p_k |d_k|)
and sum_k p_k |d_k| = -sum_k p_k log(p_k S) = H(p) - log S <= log K, because S >= 1 (the maximum contributes e^0).  Hence the
leading term 2 (2^-23 + U log K).  The rest: a factor 1 + 2^-20 for the second order; exponentials below the fp32 normal range, an
absolute 2^-126 each against S >= 1, in A and in S: 2 K 2^-126; the double sums, products, the quotient and the penalty
lam * (o - kreg) <= lam K of the kernel and of this restatement: 4 (K + 4) 2^-53 (1 + lam max(0, K - kreg)).
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
KINDS = {"lac": 0, "aps": 1, "raps": 2}
MAX_N, MAX_K, MAX_A = 1 << 20, 4096, 8
BINS = ((0, 1), (2, 3), (4, 6), (7, 10), (11, 100), (101, 1000), (1001, None))
RAPS_LAM, RAPS_KREG = 0.01, 5
ALPHAS = (0.1, 0.3)


def delta(K, lam=0.0, kreg=0):
    lead = 2.0 * (2.0 ** -23 + U * math.log(K))
    return lead * (1.0 + 2.0 ** -20) + 2.0 * K * 2.0 ** -126 + 4.0 * (K + 4) * 2.0 ** -53 * (1.0 + lam * max(0, K - kreg))


def usable(z):
    return np.isfinite(np.asarray(z, dtype=np.float32)).all(1)


def ranks(z):
    """(N, K) int64: ordinal ranks by descending logit, ties to the smaller index (+0 == -0)."""
    z = np.asarray(z, dtype=np.float32) + np.float32(0.0)
    order = np.argsort(-z, axis=1, kind="stable")
    o = np.empty_like(order)
    np.put_along_axis(o, order, np.arange(1, z.shape[1] + 1)[None, :], axis=1)
    return o


def all_scores(z, kind, u=None, lam=0.0, kreg=0):
    """(N, K) float64: s_j of every class of every row (rows with a non-finite logit: NaN)."""
    z = np.asarray(z, dtype=np.float32)
    N, K = z.shape
    out = np.full((N, K), np.nan)
    keep = usable(z)
    if not keep.any():
        return out
    x = z[keep].astype(np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    S = e.sum(1, keepdims=True)
    if kind == "lac":
        out[keep] = 1.0 - e / S
        return out
    uu = np.ones(N) if u is None else np.asarray(u, dtype=np.float32).astype(np.float64)
    o = ranks(z[keep])
    order = np.argsort(o, axis=1)                       # order[:, r] = the class of rank r + 1
    es = np.take_along_axis(e, order, axis=1)
    before = np.cumsum(es, axis=1) - es
    s = (before + uu[keep][:, None] * es) / S
    if kind == "raps":
        s = s + lam * np.maximum(0, np.arange(1, K + 1) - kreg)[None, :]
    res = np.empty_like(s)
    np.put_along_axis(res, order, s, axis=1)
    out[keep] = res
    return out


def label_scores(z, y, kind, u=None, lam=0.0, kreg=0, scores=None):
    y = np.asarray(y, dtype=np.int64)
    z = np.asarray(z, dtype=np.float32)
    if bool(((y < 0) | (y >= z.shape[1])).any()):
        raise ValueError("a label outside [0, K)")
    s = all_scores(z, kind, u, lam, kreg) if scores is None else scores
    return s[np.arange(z.shape[0]), y]


def quantile(label_s, alpha):
    """{"qhat", "k", "n", "n_skipped", "status"} of one level from the label scores (NaN = a row left out)."""
    s = np.asarray(label_s, dtype=np.float64)
    good = np.sort(s[~np.isnan(s)])
    n = good.size
    k = int(math.ceil((n + 1) * (1.0 - alpha)))
    if k > n:
        return {"qhat": math.inf, "k": k, "n": n, "n_skipped": s.size - n, "status": 1}
    return {"qhat": float(good[k - 1]), "k": k, "n": n, "n_skipped": s.size - n, "status": 0}


def set_sizes(scores, q):
    """(N,) sizes of {j : s_j <= q}; rows left out (NaN scores): -1."""
    size = (scores <= q).sum(1)
    return np.where(np.isnan(scores).any(1), -1, size)


def size_bin(size):
    for b, (lo, hi) in enumerate(BINS):
        if size >= lo and (hi is None or size <= hi):
            return b
    raise ValueError(size)


def metrics(sizes, covered, y, alpha):
    """The table's metrics from per-row sizes (-1: row left out) and covered flags, as exact integer counts and float64 ratios."""
    sizes, covered, y = np.asarray(sizes), np.asarray(covered).astype(bool), np.asarray(y)
    use = sizes >= 0
    sz, cv, yy = sizes[use], covered[use], y[use]
    n = int(use.sum())
    out = {"n": n, "n_skipped": int((~use).sum()), "covered": int(cv.sum()), "size_sum": int(sz.sum()), "n_empty": int((sz == 0).sum()),
           "n_singleton": int((sz == 1).sum())}
    nan = float("nan")
    if not n:
        out.update(coverage=nan, size=nan, empty=nan, singleton=nan, max_size=nan, sscv=nan, worst_class=nan)
        return out
    bins = np.array([size_bin(int(v)) for v in sz])
    sscv = 0.0
    for b in range(len(BINS)):
        if (bins == b).any():
            sscv = max(sscv, abs(float(cv[bins == b].sum()) / float((bins == b).sum()) - (1.0 - alpha)))
    worst = min(float(cv[yy == c].sum()) / float((yy == c).sum()) for c in np.unique(yy))
    out.update(coverage=out["covered"] / n, size=out["size_sum"] / n, empty=out["n_empty"] / n, singleton=out["n_singleton"] / n,
               max_size=int(sz.max()), sscv=sscv, worst_class=worst)
    return out


def brute_scores(z_row, kind, u=1.0, lam=0.0, kreg=0):
    """The O(K^2) definition on one row, no sort: rank by descending p with ties to the smaller index, then the sum over the classes
    ranked before."""
    x = np.asarray(z_row, dtype=np.float32).astype(np.float64)
    p = np.exp(x - x.max())
    p = p / p.sum()
    K = p.size
    out = np.empty(K)
    for j in range(K):
        ahead = [i for i in range(K) if p[i] > p[j] or (p[i] == p[j] and i < j)]
        if kind == "lac":
            out[j] = 1.0 - p[j]
        else:
            out[j] = math.fsum(p[i] for i in ahead) + u * p[j] + (lam * max(0, len(ahead) + 1 - kreg) if kind == "raps" else 0.0)
    return out


# ---- the inputs of the GPU grid, shared by tests/test_host_cp.py and tests/test_gpu_cp.py ----
# (N, K, scale, kind, with_u).  N in {1, 3, 63, 64, 65, 257} (uvit_op_cp_scores: four rows per workgroup, the quantile's histogram:
# 256 scores per workgroup; 257 straddles both), K in {2, 10, 63, 64, 65, 100, 1003, 4096} (the sets kernel pads K to 64, 128, ...,
# 4096 and goes from one wave to four at K > 128: GRID_PATHS), scale in {1, 3, 8} with the label's logit raised by 2 * scale: the flat regime and
# the peaked regime of a trained head.  Thinned: every K meets N = 65 and N = 257 (or 130 / 65 where 257 rows would only cost time),
# every N meets K = 10 and K = 100, every scale meets every K, every kind meets every K, with and without u.
# lac at K >= 1003 appears at scale 8 only: in the flat regime 1 - p_j of a thousand classes is so dense near qhat that dozens of
# classes lie within delta of it, and a two-sided test qhat -+ delta would say nothing (GRID_DENSE keeps those cases for the GPU test,
# where the sandwich still has to hold; the host test does not ask them for a narrow window).
def _grid():
    g = []
    for K in (2, 10, 63, 64, 65, 100):
        for N in (65, 257):
            for i, kind in enumerate(("lac", "aps", "raps")):
                g.append((N, K, (1.0, 3.0, 8.0)[(i + K + N) % 3], kind, (i + N) % 2 == 1))
    for N in (1, 3, 63, 64):
        for K in (10, 100):
            for i, kind in enumerate(("lac", "aps", "raps")):
                g.append((N, K, (1.0, 3.0, 8.0)[(i + N) % 3], kind, (i + K // 10) % 2 == 0))
    for K, rows in ((1003, (65, 130)), (4096, (3, 65))):
        for N in rows:
            g += [(N, K, 8.0, "lac", N != 65), (N, K, 1.0, "aps", N == 65), (N, K, 3.0, "raps", N != 65), (N, K, 8.0, "aps", False),
                  (N, K, 1.0, "raps", True)]
    for K in (2, 10, 100):                                    # every scale and both u settings at one shape per small K
        for scale in (1.0, 3.0, 8.0):
            for kind in ("lac", "aps", "raps"):
                for with_u in (False, True):
                    g.append((257, K, scale, kind, with_u))
    return sorted(set(g))


GRID = _grid()
# the sets kernel gives a row one wave up to K = 128 and four waves above, and pads K to 256, 512, 1024: both sides of each step
GRID_PATHS = [(65, 128, 1.0, "aps", True), (65, 129, 1.0, "aps", False), (65, 129, 3.0, "lac", True), (65, 256, 3.0, "raps", False),
              (65, 257, 1.0, "aps", True), (65, 512, 1.0, "raps", True), (65, 513, 3.0, "aps", False), (65, 1024, 1.0, "aps", True),
              (65, 1025, 1.0, "raps", False), (3, 2048, 3.0, "aps", True), (3, 2049, 1.0, "aps", False)]
GRID_DENSE = [(65, 1003, 1.0, "lac", False), (65, 4096, 1.0, "lac", True), (65, 4096, 3.0, "lac", False)]


def params(kind):
    return (RAPS_LAM, RAPS_KREG) if kind == "raps" else (0.0, 0)


def make_inputs(N, K, scale, seed=0):
    """z (N, K) fp32 = scale * normal with the label's logit raised by 2 * scale, y (N,) int64, u (N,) fp32 in [0, 1)."""
    rng = np.random.default_rng(1000003 * seed + 7 * N + K + int(16 * scale))
    y = rng.integers(0, K, size=N).astype(np.int64)
    z = rng.standard_normal((N, K)).astype(np.float32)
    z[np.arange(N), y] += np.float32(2.0)
    z = (z * np.float32(scale)).astype(np.float32)
    u = rng.random(N).astype(np.float32)
    return z, y, u


SEEDS = {}          # (N, K, scale, kind, with_u) -> seed, for a case whose window qhat -+ delta held two classes of a row with seed 0


@functools.lru_cache(maxsize=None)
def grid_case(N, K, scale, kind, with_u):
    """One grid point, computed once per process: z, y, u (None without), lam, kreg, the (N, K) float64 scores, the label scores and
    the calibration of both levels of ALPHAS on these rows."""
    z, y, u = make_inputs(N, K, scale, SEEDS.get((N, K, scale, kind, with_u), 0))
    u = u if with_u else None
    lam, kreg = params(kind)
    s = all_scores(z, kind, u, lam, kreg)
    sy = label_scores(z, y, kind, scores=s)
    for a in (z, y, s, sy):
        a.setflags(write=False)
    return {"z": z, "y": y, "u": u, "lam": lam, "kreg": kreg, "scores": s, "label_scores": sy, "cal": [quantile(sy, a) for a in ALPHAS],
            "delta": delta(K, lam, kreg)}
