"""Float64 restatement of the Mahalanobis / relative Mahalanobis scores of the probe's feature (csrc/maha.hip,
LinearProbe.fit_density / feature_scores), and the error bounds the GPU tests hold the device to.  NumPy throughout.

    usable rows: every feature finite and the label inside [0, K); n of them, n_k of class k
    S = sum f f^T      class_sum[k] = sum of the rows of class k      total_sum = sum f      mu_k = class_sum[k] / n_k      mu_0 = total_sum / n
    Sigma = (S - sum_k n_k mu_k mu_k^T) / n        Sigma_0 = S / n - mu_0 mu_0^T        X_reg = X + rho (tr X / C) I
    Sigma_reg = L L^T, W = L^-1;  Sigma_0,reg = L_0 L_0^T, W_0 = L_0^-1;  Wmu[k] = W mu_k,  Wmu0 = W_0 mu_0
    d_k(f) = |W f - Wmu[k]|^2      maha = min_k d_k over n_k > 0      pred = arg min (lowest index on ties)
    d_0(f) = |W_0 f - Wmu0|^2      rmaha = maha - d_0
    a row with a non-finite feature: maha = rmaha = NaN, pred = -1, its distances NaN

The bounds, with u = 2^-53.  Every device operation is an IEEE double operation on widened fp32 inputs; a product of two widened
fp32 values is exact; a sum or fma chain of m terms t_i, in any order, is within m u sum |t_i| of the exact sum.  The restatement
is float64 as well and errs by no more than the same expression, so every bound below counts it twice: once for the device, once
for the reference.

  S           |dS_ij| <= 2 n u sum_b |f_bi f_bj|, n the usable rows accumulated (one chain over b per call, the calls added in turn).
  class_sum   |d class_sum_kc| <= 2 n_k u sum_{b in k} |f_bc|;  total_sum likewise with n;  the counts are whole numbers and exact.
  g = W f     e_c = 2 (C + 2) u sum_j |W_cj f_j|: a chain of C products, each rounded once.
  d_k         with t_c = g_c - Wmu[k, c]: the difference adds u |t_c| to e_c, the squares and their chain of C non-negative terms add
              (C + 2) u sum t_c^2 per side:  |d d_k| <= sum_c (2 |t_c| e_c + e_c^2) + 2 (C + 4) u sum_c t_c^2.  d_0 likewise from W_0.
  maha        the bound of its d_k plus one rounding to fp32, 2^-24 |maha|.
  rmaha       the bounds of d_pred and d_0, one subtraction (u |rmaha|) and one rounding to fp32, 2^-24 |rmaha|.
  pred        equal wherever the restatement's two smallest distances differ by more than the sum of their two bounds.
"""
import numpy as np

U = 2.0 ** -53
U32 = 2.0 ** -24
F64 = np.float64
EPS = 1e-6                   # the encoder's ln_eps in the probe's normalisation of synthetic features


def normalise(x, eps=EPS):
    """The probe's LayerNorm without affine over the C entries of every row, rounded to fp32 as the device holds it."""
    x = np.asarray(x, dtype=F64)
    x = x - x.mean(axis=1, keepdims=True)
    return (x / np.sqrt((x * x).mean(axis=1, keepdims=True) + eps)).astype(np.float32)


def usable_rows(feat, labels, K):
    feat, labels = np.asarray(feat), np.asarray(labels)
    return np.isfinite(feat.astype(F64)).all(axis=1) & (labels >= 0) & (labels < K)


def accumulate(feat, labels, K, dtype=F64):
    """(S (C, C), class_sum (K, C), total_sum (C), class_count (K), sums = [rows used, rows skipped]) of one batch."""
    feat, labels = np.asarray(feat), np.asarray(labels)
    ok = usable_rows(feat, labels, K)
    f, y = feat[ok].astype(dtype), labels[ok]
    class_sum, count = np.zeros((K, feat.shape[1]), dtype=dtype), np.zeros(K, dtype=dtype)
    for k in range(K):
        class_sum[k] = f[y == k].sum(axis=0)
        count[k] = (y == k).sum()
    return f.T @ f, class_sum, f.sum(axis=0), count, np.array([ok.sum(), (~ok).sum()], dtype=dtype)


def accumulate_batches(batches, K):
    parts = [accumulate(f, y, K) for f, y in batches]
    return tuple(sum(p[i] for p in parts) for i in range(5))


def covariances(S, class_sum, total_sum, class_count, sums, rho):
    """(mu (K, C) with zero rows for empty classes, mu_0, Sigma_reg, Sigma_0,reg) in float64."""
    n, Cd = float(sums[0]), S.shape[0]
    mu = class_sum / np.maximum(class_count, 1.0)[:, None]
    mu0 = total_sum / n
    sigma = (S - class_sum.T @ mu) / n
    sigma = 0.5 * (sigma + sigma.T)
    sigma0 = S / n - np.outer(mu0, mu0)
    reg = lambda m: m + rho * (np.trace(m) / Cd) * np.eye(Cd)           # noqa: E731
    return mu, mu0, reg(sigma), reg(sigma0)


def fit(S, class_sum, total_sum, class_count, sums, rho=1e-3):
    """The host fit: {W, W0 (lower triangular), Wmu, Wmu0, class_count, logdet, logdet0, mu, mu0, sigma, sigma0}."""
    mu, mu0, sigma, sigma0 = covariances(S, class_sum, total_sum, class_count, sums, rho)
    L, L0 = np.linalg.cholesky(sigma), np.linalg.cholesky(sigma0)
    W, W0 = np.tril(np.linalg.inv(L)), np.tril(np.linalg.inv(L0))
    return {"W": W, "W0": W0, "Wmu": mu @ W.T, "Wmu0": W0 @ mu0, "class_count": np.asarray(class_count, dtype=F64),
            "logdet": 2.0 * np.log(np.diag(L)).sum(), "logdet0": 2.0 * np.log(np.diag(L0)).sum(), "mu": mu, "mu0": mu0,
            "sigma": sigma, "sigma0": sigma0}


def scores(feat, W, W0, Wmu, Wmu0, class_count):
    """{"dist" (B, K), "d0" (B), "maha", "rmaha" (B) float64 (not yet rounded to fp32), "pred" (B) int}: every d_k as the sum of squared
    differences; empty classes never win, np.argmin takes the lowest index on ties, NaN rows as documented."""
    feat = np.asarray(feat)
    f = feat.astype(F64)
    bad = ~np.isfinite(f).all(axis=1)
    f = np.where(bad[:, None], 0.0, f)
    g, g0 = f @ W.T, f @ W0.T
    dist = np.concatenate([((g[i:i + 8, None, :] - Wmu[None, :, :]) ** 2).sum(axis=2) for i in range(0, len(g), 8)])      # 8 rows at a time
    d0 = ((g0 - Wmu0[None, :]) ** 2).sum(axis=1)
    live = np.asarray(class_count) > 0
    masked = np.where(live[None, :], dist, np.inf)
    pred = masked.argmin(axis=1)
    maha = masked[np.arange(len(f)), pred]
    none = ~live.any()
    dist[bad], d0[bad] = np.nan, np.nan
    maha = np.where(bad | none, np.nan, maha)
    return {"dist": dist, "d0": d0, "maha": maha, "rmaha": maha - d0, "pred": np.where(bad | none, -1, pred)}


def scores_brute_force(feat, mu, mu0, sigma, sigma0):
    """(d (B, K), d0 (B)) as (f - mu)^T Sigma_reg^-1 (f - mu) through np.linalg.inv: what the whitened form must equal."""
    f = np.asarray(feat, dtype=F64)
    P, P0 = np.linalg.inv(sigma), np.linalg.inv(sigma0)
    t = f[:, None, :] - mu[None, :, :]
    t0 = f - mu0[None, :]
    return np.einsum("bkc,cd,bkd->bk", t, P, t), np.einsum("bc,cd,bd->b", t0, P0, t0)


def auroc(scores_in, scores_out):
    """P(out > in) + P(out == in) / 2 over all pairs."""
    a, b = np.asarray(scores_in, dtype=F64)[:, None], np.asarray(scores_out, dtype=F64)[None, :]
    return float(((b > a).sum() + 0.5 * (b == a).sum()) / (a.size * b.size))


def maha_mean(maha):
    """The evaluation's maha_mean: the mean of the fp32 column over the rows that are not NaN."""
    v = np.asarray(maha, dtype=F64)
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else float("nan")


# ---- the bounds ----
def bound_S(batches, K):
    n, mag = 0, 0.0
    for f, y in batches:
        ok = usable_rows(f, y, K)
        a = np.abs(np.asarray(f)[ok].astype(F64))
        n += int(ok.sum())
        mag = mag + a.T @ a
    return 2 * max(n, 1) * U * mag


def bound_sums(batches, K):
    """(bound on |d class_sum| (K, C), bound on |d total_sum| (C))."""
    Cd = np.asarray(batches[0][0]).shape[1]
    mag, count = np.zeros((K, Cd)), np.zeros(K)
    for f, y in batches:
        ok = usable_rows(f, y, K)
        a, yy = np.abs(np.asarray(f)[ok].astype(F64)), np.asarray(y)[ok]
        for k in range(K):
            mag[k] += a[yy == k].sum(axis=0)
            count[k] += (yy == k).sum()
    return 2 * np.maximum(count, 1)[:, None] * U * mag, 2 * max(count.sum(), 1) * U * mag.sum(axis=0)


def bound_dist(feat, W, Wmu):
    """(B, K) bound on |d d_k| (Wmu (K, C)), or (B,) for one mean Wmu (C,)."""
    f = np.asarray(feat, dtype=F64)
    Cd = f.shape[1]
    g = f @ W.T
    e = 2 * (Cd + 2) * U * (np.abs(f) @ np.abs(W).T)                     # (B, C)
    if Wmu.ndim == 1:
        t = np.abs(g - Wmu[None, :])
        return (2 * t * e + e * e).sum(axis=1) + 2 * (Cd + 4) * U * (t * t).sum(axis=1)
    out = []
    for i in range(0, len(g), 8):                                        # 8 rows at a time
        t, ei = np.abs(g[i:i + 8, None, :] - Wmu[None, :, :]), e[i:i + 8, None, :]
        out.append((2 * t * ei + ei * ei).sum(axis=2) + 2 * (Cd + 4) * U * (t * t).sum(axis=2))
    return np.concatenate(out)


def bounds_scores(feat, fitd, ref):
    """(bound on |d maha|, bound on |d rmaha|, rows whose pred is decided) for the fp32 outputs against `ref` = scores(...)."""
    bd = bound_dist(feat, fitd["W"], fitd["Wmu"])
    b0 = bound_dist(feat, fitd["W0"], fitd["Wmu0"])
    rows = np.arange(len(bd))
    pred = np.maximum(ref["pred"], 0)
    bm = bd[rows, pred] + U32 * np.abs(ref["maha"])
    br = bd[rows, pred] + b0 + (U + U32) * np.abs(ref["rmaha"])
    live = np.asarray(fitd["class_count"]) > 0
    masked = np.where(live[None, :], ref["dist"], np.inf)
    order = np.argsort(masked, axis=1, kind="stable")
    first, second = order[:, 0], order[:, min(1, masked.shape[1] - 1)]
    gap = masked[rows, second] - masked[rows, first]
    decided = gap > bd[rows, first] + bd[rows, second]
    return bm, br, decided


# ---- shared synthetic cases ----
def clusters(K, Cd, n, seed=0, mean_std=2.0, noise=0.5):
    """Gaussian class clusters through the probe's normalisation: (means (K, C), f (n, C) fp32, y (n) int64), labels cycling 0 .. K - 1."""
    rng = np.random.default_rng(seed)
    means = mean_std * rng.standard_normal((K, Cd))
    y = (np.arange(n) % K).astype(np.int64)
    return means, normalise(means[y] + noise * rng.standard_normal((n, Cd))), y


def meaning_case(seed=0):
    """The issue's synthetic set: K = 5, C = 16, 240 fit rows, 60 held-out in-distribution rows, 60 rows of normalised N(0, 2) noise."""
    rng = np.random.default_rng(seed)
    K, Cd = 5, 16
    means = 2.0 * rng.standard_normal((K, Cd))
    y_fit, y_in = (np.arange(240) % K).astype(np.int64), (np.arange(60) % K).astype(np.int64)
    f_fit = normalise(means[y_fit] + 0.5 * rng.standard_normal((240, Cd)))
    f_in = normalise(means[y_in] + 0.5 * rng.standard_normal((60, Cd)))
    f_out = normalise(2.0 * rng.standard_normal((60, Cd)))
    return K, Cd, (f_fit, y_fit), (f_in, y_in), f_out


C_SIZES, K_SIZES, B_SIZES = (4, 12, 68, 132), (2, 3, 33, 65), (1, 17, 33, 130)
SHAPES = [(1, 4, 2), (17, 12, 3), (33, 68, 33), (130, 132, 65), (130, 12, 65), (17, 132, 2), (128, 768, 1000)]      # (B, C, K)


def make_rows(B, Cd, K, means, seed):
    """B test rows (fp32 features, int64 labels): cluster rows and, from row 1 on, every third a noise row."""
    rng = np.random.default_rng(5000 + 1000 * seed + 7 * B + 3 * Cd + K)
    y = rng.integers(0, K, size=B)
    x = means[y] + 0.5 * rng.standard_normal((B, Cd))
    noise = 2.0 * rng.standard_normal((B, Cd))
    x[1::3] = noise[1::3]
    return normalise(x), y.astype(np.int64)


def make_case(B, Cd, K, seed=0, with_fit=True):
    """Per shape: a fit set of max(4 K, 2 C + 8) cluster rows (so that the tied covariance has rank without the shrinkage doing all the
    work), its host fit at rho = 1e-3 (with_fit), and B test rows of the same clusters (make_rows)."""
    n_fit = max(4 * K, 2 * Cd + 8)
    means, f_fit, y_fit = clusters(K, Cd, n_fit, seed=1000 * seed + 7 * B + 3 * Cd + K)
    feat, labels = make_rows(B, Cd, K, means, seed)
    return {"fit_set": (f_fit, y_fit), "fit": fit(*accumulate(f_fit, y_fit, K)) if with_fit else None, "feat": feat, "labels": labels}
