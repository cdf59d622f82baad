"""Float64 restatement of the ViM and residual scores of the probe's feature (csrc/vim.hip,
LinearProbe.fit_vim / vim_scores), and the error bounds the GPU tests hold the device to.  NumPy throughout.

    head (W (K, C), b (K)); usable rows: every feature finite and the label inside [0, K); n of them
    o = -pinv(W) b                                                     the origin: the point the head maps closest to zero logits
    S = sum f f^T, t = sum f      M = (S - o t^T - t o^T + n o o^T) / n = (1 / n) sum (f - o)(f - o)^T, symmetrised
    M = V diag(lambda) V^T (eigh, ascending)      R (Cn, C) = the eigenvectors of the Cn = C - D smallest eigenvalues, as rows
    A = [R ; W] (Cn + K, C)      a = [-R o ; b] (Cn + K)               y = A f + a:  y[:Cn] = R (f - o),  y[Cn:] = z = W f + b
    residual = |y[:Cn]|_2      lse = logsumexp(z)      vim = alpha residual - lse      pred = arg max z (lowest class on ties)
    alpha = sum max_k z / sum residual over the usable rows of the fit set
    a row with a non-finite feature: vim = residual = NaN, pred = -1

The bounds, with u = 2^-53 and gamma_m = m u / (1 - m u).  Every device operation is an IEEE double operation on widened fp32
features; a sum or fma chain of m terms t_i, in any order, is within gamma_m sum |t_i| of the exact sum.  The restatement is float64
as well (its sums run in numpy's order) and errs by no more than the same expression, so every bound below counts such a term twice:
once for the device, once for the reference.

  y          one fma chain of C products from zero and one addition of a_j: C + 1 roundings,
             |dy_j| <= 2 gamma_{C+1} (sum_c |A_jc f_c| + |a_j|).
  residual   r = sqrt(sum_{j<Cn} y_j^2).  The norm is 1-Lipschitz in y: |y + dy| differs from |y| by at most |dy|_2.  Squares, their
             chain of Cn non-negative terms and the square root are Cn + 2 roundings of a sum of non-negative terms, whose relative
             error the root halves; we keep the whole: |dr| <= |dy[:Cn]|_2 + 2 gamma_{Cn+2} r, then one rounding to fp32 of the device's
             double, 2^-24 (r + |dr|).
  lse        logsumexp is 1-Lipschitz in the maximum norm: the dz contribute max_k |dz_k|.  On the z at hand, with m = max z (exact),
             d_k = z_k - m is rounded once (u |d_k|, which exp turns into a relative u |d_k| of its value), exp is within one unit
             in the last place (2 u relative; the ROCm device library documents 1 ulp for the double exp and log), the K non-negative
             terms add gamma_K: the sum s has relative error rho <= sum_k e_k (3 u + u |d_k|) / s + gamma_K.  log(s (1 + rho)) moves by
             at most rho / (1 - rho) <= 1.01 rho, the log itself rounds 2 u |log s|, the addition m + log s rounds u |lse|:
             |d lse| <= max_k |dz_k| + 2 (1.01 rho + 2 u |log s| + u |lse|).
  vim        fma(alpha, r, -lse) rounds once: |d vim| <= |alpha| |dr| + |d lse| + 2 u |vim|, then one rounding to fp32, 2^-24 (|vim| + |d vim|).
  pred       equal wherever the restatement's two largest logits differ by more than the sum of their two |dz|.
  sums       B values, each within its row's bound, added in some fixed order: sum_b bound_b + gamma_{B+1} sum_b |v_b| against the
             correctly rounded math.fsum of the restatement's values (u |sum| more), one addition to the old value included.
  alpha      Sm / Sr with |dSm|, |dSr| as above, per call: |d alpha| <= (|dSm| + |alpha| |dSr|) / (Sr - |dSr|) + 2 u |alpha|.
"""
import math

import numpy as np

import maha_ref as mr

U = 2.0 ** -53
U32 = 2.0 ** -24
F64 = np.float64


def gamma(m):
    return m * U / (1.0 - m * U)


def default_dim(Cd):
    """The paper's principal dimension: 1000 for C >= 2048, 512 for C >= 768, otherwise C // 2."""
    return 1000 if Cd >= 2048 else 512 if Cd >= 768 else Cd // 2


def moments(feat, labels, K):
    """(S (C, C), t (C), n) over the usable rows, as uvit_op_maha_accumulate's S, total_sum and sums[0]."""
    S, _, t, _, sums = mr.accumulate(feat, labels, K)
    return S, t, float(sums[0])


def fit(S, t, n, W, b, dim=None):
    """The host fit without alpha: {"origin", "R" (Cn, C), "A", "a", "eigenvalues" (ascending), "dim", "explained"}."""
    W, b, S, t = (np.asarray(v, dtype=F64) for v in (W, b, S, t))
    Cd = W.shape[1]
    D = default_dim(Cd) if dim is None else int(dim)
    if not 1 <= D <= Cd - 1:
        raise ValueError(f"dim must lie in [1, {Cd - 1}], got {D}")
    o = -np.linalg.pinv(W) @ b
    M = (S - np.outer(o, t) - np.outer(t, o) + n * np.outer(o, o)) / n
    M = 0.5 * (M + M.T)
    lam, V = np.linalg.eigh(M)
    R = np.ascontiguousarray(V[:, :Cd - D].T)
    return {"origin": o, "R": R, "A": np.concatenate([R, W]), "a": np.concatenate([-R @ o, b]), "eigenvalues": lam, "dim": D,
            "explained": float(lam[Cd - D:].sum() / lam.sum())}


def scores(feat, A, a, Cn, alpha=0.0):
    """{"y" (B, Cn + K), "residual", "lse", "zmax", "vim" (B) float64 (not yet rounded to fp32), "pred" (B) int}; NaN rows as documented."""
    f = np.asarray(feat).astype(F64)
    bad = ~np.isfinite(f).all(axis=1)
    f = np.where(bad[:, None], 0.0, f)
    y = f @ np.asarray(A, dtype=F64).T + np.asarray(a, dtype=F64)[None, :]
    res = np.sqrt((y[:, :Cn] ** 2).sum(axis=1))
    z = y[:, Cn:]
    zmax = z.max(axis=1)
    lse = zmax + np.log(np.exp(z - zmax[:, None]).sum(axis=1))
    vim = alpha * res - lse
    nan = lambda v: np.where(bad, np.nan, v)                             # noqa: E731
    return {"y": y, "residual": nan(res), "lse": nan(lse), "zmax": nan(zmax), "vim": nan(vim), "pred": np.where(bad, -1, z.argmax(axis=1)),
            "bad": bad}


def scores_brute_force(feat, W, b, origin, P, alpha=0.0):
    """(residual, vim) through the projector I - P P^T on the principal space P (C, D): what the stacked form must equal."""
    f = np.asarray(feat, dtype=F64) - origin[None, :]
    off = f - (f @ P) @ P.T
    res = np.sqrt((off * off).sum(axis=1))
    z = np.asarray(feat, dtype=F64) @ W.T + b[None, :]
    m = z.max(axis=1)
    return res, alpha * res - (m + np.log(np.exp(z - m[:, None]).sum(axis=1)))


def alpha_of(ref):
    """(alpha, Sm, Sr, used, skipped) of the fit rows' scores: both sums by math.fsum."""
    ok = ~ref["bad"]
    sm, sr = math.fsum(ref["zmax"][ok].tolist()), math.fsum(ref["residual"][ok].tolist())
    return sm / sr, sm, sr, int(ok.sum()), int((~ok).sum())


# ---- the bounds ----
def bounds(feat, A, a, Cn, alpha, ref):
    """{"y" (B, Cn + K), "residual", "vim", "zmax" (B), "residual64", "decided" (B) bool} for the device's outputs against `ref` =
    scores(...): "residual" and "vim" hold for the fp32 outputs, "zmax" and "residual64" for the doubles that enter `sums`."""
    f = np.abs(np.where(ref["bad"][:, None], 0.0, np.asarray(feat).astype(F64)))
    A, a = np.asarray(A, dtype=F64), np.asarray(a, dtype=F64)
    Cd, K = A.shape[1], A.shape[0] - Cn
    dy = 2 * gamma(Cd + 1) * (f @ np.abs(A).T + np.abs(a)[None, :])
    res = np.nan_to_num(ref["residual"])
    dres = np.sqrt((dy[:, :Cn] ** 2).sum(axis=1)) + 2 * gamma(Cn + 2) * res
    z, dz = ref["y"][:, Cn:], dy[:, Cn:]
    d = z - z.max(axis=1, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=1)
    rho = (e * (3 * U + U * np.abs(d))).sum(axis=1) / s + gamma(K)
    lse = np.nan_to_num(ref["lse"])
    dlse = dz.max(axis=1) + 2 * (1.01 * rho + 2 * U * np.abs(np.log(s)) + U * np.abs(lse))
    vim = np.nan_to_num(ref["vim"])
    dvim = abs(alpha) * dres + dlse + 2 * U * np.abs(vim)
    order = np.argsort(-z, axis=1, kind="stable")
    rows = np.arange(len(z))
    first, second = order[:, 0], order[:, 1]
    decided = (z[rows, first] - z[rows, second]) > dz[rows, first] + dz[rows, second]
    return {"y": dy, "residual": (1 + U32) * dres + U32 * res, "vim": (1 + U32) * dvim + U32 * np.abs(vim), "zmax": dz.max(axis=1), "residual64": dres,
            "decided": decided | ref["bad"]}


def bound_sum(values, row_bounds):
    """The bound of a device sum of `values` (each within its entry of `row_bounds`) against math.fsum(values)."""
    v = np.asarray(values, dtype=F64)
    return float(np.sum(row_bounds) + gamma(len(v) + 1) * np.abs(v).sum() + U * abs(math.fsum(v.tolist())))


def bound_alpha(alpha, sr, dsm, dsr):
    return (dsm + abs(alpha) * dsr) / (sr - dsr) + 2 * U * abs(alpha)


# ---- shared synthetic cases ----
# (B, C, Cn, K): the smallest; D = 1; Cn + K across a 32-column tile with C no multiple of the reduction tile; B across 16, 64 and
# 128 with Cn = 1; the row kernel's K loop; the real geometry
SHAPES = [(1, 4, 1, 2), (17, 12, 11, 3), (33, 68, 30, 33), (130, 132, 1, 65), (5, 32, 16, 4096), (128, 768, 256, 1000)]


def make_head(K, Cd, seed):
    """An affine head of the size a trained probe's has on normalised features: logits of order one."""
    rng = np.random.default_rng(9000 + seed)
    return (rng.standard_normal((K, Cd)) / np.sqrt(Cd)).astype(np.float32).astype(F64), (0.5 * rng.standard_normal(K)).astype(np.float32).astype(F64)


def make_case(B, Cd, Cn, K, seed=0):
    """Per shape: a fit set of 2 C + 8 cluster rows of min(K, 10) classes through the probe's normalisation, a head, the fit at
    dim = C - Cn with its alpha, and B test rows of the same clusters with every third a noise row (maha_ref.make_rows)."""
    Kc = min(K, 10)
    means, f_fit, y_fit = mr.clusters(Kc, Cd, 2 * Cd + 8, seed=1000 * seed + 7 * B + 3 * Cd + K)
    W, b = make_head(K, Cd, seed + B + Cd + K)
    S, t, n = moments(f_fit, y_fit, K)
    ft = fit(S, t, n, W, b, Cd - Cn)
    ft["alpha"] = alpha_of(scores(f_fit, ft["A"], ft["a"], Cn))[0]
    feat, labels = mr.make_rows(B, Cd, Kc, means, seed)
    return {"fit_set": (f_fit, y_fit), "W": W, "b": b, "fit": ft, "feat": feat, "labels": labels}


def meaning_case(seed=0):
    """The issue's hand-made case.  K = 5, C = 32; U (C, 8) an orthonormal basis; class means 2 N(0, I_8) inside U, within-class 0.5,
    0.02 isotropic noise in all 32 directions; the head of the matching Gaussian classifier, W = means U^T, b = -|mean|^2 / 2.
    240 fit rows, 60 held-out rows, 60 held-out rows shifted by 0.5 N(0, I_32) projected off U (their logits are the held-out rows':
    W annihilates the shift), 60 rows 0.3 N(0, I_8) inside U (flat logits, no residual).  Features are fp32, not normalised.
    Returns (K, C, D, (W, b), (f_fit, y_fit), f_in, f_shift, f_flat)."""
    rng = np.random.default_rng(seed)
    K, Cd, D = 5, 32, 8
    Ub = np.linalg.qr(rng.standard_normal((Cd, D)))[0]
    means = 2.0 * rng.standard_normal((K, D))
    W, b = means @ Ub.T, -0.5 * (means * means).sum(axis=1)

    def rows(n):
        y = (np.arange(n) % K).astype(np.int64)
        return (means[y] + 0.5 * rng.standard_normal((n, D))) @ Ub.T + 0.02 * rng.standard_normal((n, Cd)), y

    f_fit, y_fit = rows(240)
    f_in, _ = rows(60)
    base, _ = rows(60)
    noise = rng.standard_normal((60, Cd))
    f_shift = base + 0.5 * (noise - (noise @ Ub) @ Ub.T)
    f_flat = (0.3 * rng.standard_normal((60, D))) @ Ub.T + 0.02 * rng.standard_normal((60, Cd))
    f32 = lambda x: x.astype(np.float32)                                 # noqa: E731
    return K, Cd, D, (W, b), (f32(f_fit), y_fit), f32(f_in), f32(f_shift), f32(f_flat)


def energy(feat, W, b):
    """-logsumexp(z), the detection's `energy` column (larger = more out of distribution)."""
    z = np.asarray(feat, dtype=F64) @ W.T + b[None, :]
    m = z.max(axis=1)
    return -(m + np.log(np.exp(z - m[:, None]).sum(axis=1)))
