"""Float64 restatement of the post-hoc last-layer K-FAC Laplace probe (csrc/laplace.hip, lap_probe.py), and
the error bounds the GPU tests hold the device to.  NumPy throughout; every function takes `dtype` where the CPU tests repeat it in
np.longdouble to measure float64's own error.

    phi = [f, 1] (D = C + 1)        z = W f + b        p = softmax(z)        theta ordered (k, c')
    A = sum_n phi phi^T             G = (1 / n) sum_n (diag(p) - p p^T)       nll = -sum_n log p[y]       precision = G (x) A + tau I
    A = U_A diag(lam_A) U_A^T,  G = U_G diag(lam_G) U_G^T  (eigenvalues clamped at 0)
    var_k = sum_i a_i^2 T[i, k],  a = U_A^T phi,  T[i, k] = sum_j U_G[k, j]^2 / (lam_A[i] lam_G[j] + tau)
    z~_k = z_k / sqrt(1 + (pi / 8) var_k)          lap_var = var[argmax_k z_k]  (lowest index on ties)
    log ml(tau) = -nll - tau |theta|^2 / 2 + K D log(tau) / 2 - sum_ij log(lam_A[i] lam_G[j] + tau) / 2

Rows with a non-finite logit or a label outside [0, K) are left out of A, G, nll and n.

The bounds, with u = 2^-53 (every device operation is an IEEE double operation: relative error <= u; a product of two widened
fp32 values is exact; a recursive sum or fma chain of m terms t_i errs by at most (m - 1) u sum |t_i| to first order, and the
reference's own pairwise sums by less):

  A     |dA_ij| <= 2 n u sum_b |phi_bi phi_bj|: n exact products in one chain per side (device and reference), n the rows accumulated.
  G     |dG_kl| <= (2 n + 2 K + 64) u sum_b (delta_kl p_bk + p_bk p_bl): the chains over b as for A; every p carries the relative
        error of its softmax, K u for the sum of K positive terms per side plus the exponential's and the quotient's.  The HIP math
        API documentation lists the double-precision exp at 1 ulp (log at 1 ulp), NumPy's is within 1 ulp as well, and the argument
        z - max is the same IEEE difference on both sides: 64 covers two factors p with a few ulp each with room to spare, so the
        constant stands.
  nll   |dnll| <= (2 n + 2 K + 64) u sum_b (|log S_b| + |z_by - max_b| + 1): per row the logarithm of a sum of K positive terms
        (relative K u on S is absolute K u on log S), the logarithm's own ulp, one subtraction; then the sum over rows.
  T     all terms are non-negative: relative error <= (K + 8) u (K - 1 additions; square, product, sum, quotient per term).
  var   a_i errs by e_i = (D + 2) u sum_c |phi_c U_A[c, i]| (a chain of D products, each rounded once);
        |dvar_k| <= sum_i (2 |a_i| e_i + e_i^2) T_ik + (D + 8) u var_k (the square, the product and the chain of D non-negative terms).
  probit  2 fp32 ulp of the float64 value rounded to fp32 (one rounding to fp32 of a double that agrees to ~1e-15).
"""
import numpy as np

U = 2.0 ** -53
F64 = np.float64
PROBIT = np.pi / 8.0


def phi_of(feat, dtype=F64):
    feat = np.asarray(feat, dtype=dtype)
    return np.concatenate([feat, np.ones((feat.shape[0], 1), dtype=dtype)], axis=1)


def usable_rows(logits, labels):
    """Boolean mask of the rows the fit uses: every logit finite and the label inside [0, K)."""
    logits, labels = np.asarray(logits), np.asarray(labels)
    return np.isfinite(logits.astype(F64)).all(axis=1) & (labels >= 0) & (labels < logits.shape[1])


def softmax_parts(logits, dtype=F64):
    """(p, log S, max) of the max-shifted softmax, rows as given (call it on usable rows)."""
    z = np.asarray(logits, dtype=dtype)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    return e / s, np.log(s)[:, 0], m[:, 0]


def factors(feat, logits, labels, dtype=F64):
    """(A (D, D), G_sum (K, K) -- not divided by n --, sums = [nll, rows used, rows skipped]) of one batch."""
    feat, logits, labels = np.asarray(feat), np.asarray(logits), np.asarray(labels)
    ok = usable_rows(logits, labels)
    f, z, y = feat[ok], logits[ok], labels[ok]
    K = logits.shape[1]
    ph = phi_of(f, dtype)
    A = ph.T @ ph
    if len(z):
        p, logs, m = softmax_parts(z, dtype)
        G = np.diag(p.sum(axis=0)) - p.T @ p
        nll = (logs - (z.astype(dtype)[np.arange(len(y)), y] - m)).sum()
    else:
        G, nll = np.zeros((K, K), dtype=dtype), dtype(0)
    return A, G, np.array([nll, ok.sum(), (~ok).sum()], dtype=dtype)


def eig(A, G):
    """(lam_A, U_A, lam_G, U_G) in float64, eigenvalues clamped at 0 (G has the all-ones null vector: eigh returns about -1e-17)."""
    la, UA = np.linalg.eigh(np.asarray(A, dtype=F64))
    lg, UG = np.linalg.eigh(np.asarray(G, dtype=F64))
    return np.maximum(la, 0.0), UA, np.maximum(lg, 0.0), UG


def t_matrix(UG, lam_a, lam_g, tau, dtype=F64):
    """T (D, K): T[i, k] = sum_j UG[k, j]^2 / (lam_a[i] lam_g[j] + tau)."""
    UG, lam_a, lam_g = (np.asarray(v, dtype=dtype) for v in (UG, lam_a, lam_g))
    inv = 1.0 / (lam_a[:, None] * lam_g[None, :] + dtype(tau))          # (D, K): i, j
    return inv @ (UG ** 2).T


def projections(feat, UA, dtype=F64):
    """a (B, D) = phi U_A."""
    return phi_of(feat, dtype) @ np.asarray(UA, dtype=dtype)


def variance(feat, UA, T, dtype=F64):
    """var (B, K) = (phi U_A)^2 T."""
    return projections(feat, UA, dtype) ** 2 @ np.asarray(T, dtype=dtype)


def dense_precision(A, G, tau):
    """G (x) A + tau I, (K D, K D), for theta ordered (k, c')."""
    A, G = np.asarray(A, dtype=F64), np.asarray(G, dtype=F64)
    return np.kron(G, A) + tau * np.eye(A.shape[0] * G.shape[0])


def jacobian(phi_row, K):
    """J (K, K D) = I_K (x) phi^T: the Jacobian of the logits in theta."""
    return np.kron(np.eye(K), np.asarray(phi_row, dtype=F64)[None, :])


def variance_dense(feat, A, G, tau):
    """diag(J (G (x) A + tau I)^-1 J^T) per row, through the dense inverse: what the eigen-form must equal."""
    ph, K = phi_of(feat), np.asarray(G).shape[0]
    S = np.linalg.inv(dense_precision(A, G, tau))
    return np.stack([np.diag(jacobian(r, K) @ S @ jacobian(r, K).T) for r in ph])


def probit(logits, var, factor=PROBIT):
    """z / sqrt(1 + factor var) in float64; a NaN or negative variance gives NaN in that entry."""
    z, var = np.asarray(logits, dtype=F64), np.asarray(var, dtype=F64)
    with np.errstate(invalid="ignore"):
        den = np.where(var >= 0.0, np.sqrt(1.0 + factor * var), np.nan)
        return z / den


def lap_var(logits, var):
    """var[b, argmax_k z[b, k]]: the arg-max over the unscaled logits, the lowest index on ties."""
    z = np.asarray(logits)
    return np.asarray(var)[np.arange(z.shape[0]), z.argmax(axis=1)]


def marglik_grid():
    return np.logspace(-4.0, 8.0, 97)


def log_marglik(tau, nll, theta_sq, lam_a, lam_g):
    lam_a, lam_g = np.asarray(lam_a, dtype=F64), np.asarray(lam_g, dtype=F64)
    logdet = np.log(np.outer(lam_a, lam_g) + tau).sum()
    return -nll - 0.5 * tau * theta_sq + 0.5 * lam_a.size * lam_g.size * np.log(tau) - 0.5 * logdet


def choose_prior_precision(nll, theta_sq, lam_a, lam_g):
    """(tau, log ml, on_grid_edge): the arg-max over the grid; the first point wins ties."""
    grid = marglik_grid()
    vals = np.array([log_marglik(t, nll, theta_sq, lam_a, lam_g) for t in grid])
    i = int(np.argmax(vals))
    return float(grid[i]), float(vals[i]), i in (0, len(grid) - 1)


# ---- the bounds ----
def bound_A(feats, logits, labels):
    """(D, D) bound on |dA| after accumulating the given batches (lists of arrays): 2 n u sum_b |phi_bi phi_bj|."""
    n, mag = 0, 0.0
    for f, z, y in zip(feats, logits, labels):
        ok = usable_rows(z, y)
        ph = np.abs(phi_of(np.asarray(f)[ok]))
        n += int(ok.sum())
        mag = mag + ph.T @ ph
    return 2 * n * U * mag


def bound_G(logits, labels):
    """(K, K) bound on |dG_sum|: (2 n + 2 K + 64) u sum_b (delta_kl p_bk + p_bk p_bl)."""
    n, mag, K = 0, 0.0, np.asarray(logits[0]).shape[1]
    for z, y in zip(logits, labels):
        ok = usable_rows(z, y)
        if ok.any():
            p = softmax_parts(np.asarray(z)[ok])[0]
            mag = mag + np.diag(p.sum(axis=0)) + p.T @ p
        n += int(ok.sum())
    return (2 * n + 2 * K + 64) * U * mag


def bound_nll(logits, labels):
    n, mag, K = 0, 0.0, np.asarray(logits[0]).shape[1]
    for z, y in zip(logits, labels):
        z, y = np.asarray(z), np.asarray(y)
        ok = usable_rows(z, y)
        if ok.any():
            _, logs, m = softmax_parts(z[ok])
            mag += float((np.abs(logs) + np.abs(z[ok].astype(F64)[np.arange(ok.sum()), y[ok]] - m) + 1.0).sum())
        n += int(ok.sum())
    return (2 * n + 2 * K + 64) * U * mag


def bound_T_rel(K):
    return (K + 8) * U


def bound_var(feat, UA, T):
    """(B, K) bound on |dvar|: sum_i (2 |a_i| e_i + e_i^2) T_ik + (D + 8) u var_k, e_i = (D + 2) u sum_c |phi_c U_A[c, i]|."""
    ph, UA, T = phi_of(feat), np.asarray(UA, dtype=F64), np.asarray(T, dtype=F64)
    D = ph.shape[1]
    a = ph @ UA
    e = (D + 2) * U * (np.abs(ph) @ np.abs(UA))
    return (2 * np.abs(a) * e + e * e) @ T + (D + 8) * U * (a * a @ T)


# ---- shared random cases (the GPU op tests and the CPU quarter-of-the-bound checks use the same ones) ----
SHAPES = [(1, 4, 2), (3, 8, 10), (64, 128, 65), (130, 128, 100), (128, 768, 1000)]


def make_case(B, Cd, K, seed=0):
    """fp32 features of unit row variance (the probe's normalised features), logits of a few units, labels; two batches."""
    rng = np.random.default_rng(1000 * seed + 7 * B + 3 * Cd + K)
    out = []
    for _ in range(2):
        f = rng.standard_normal((B, Cd)).astype(np.float32)
        z = (3.0 * rng.standard_normal((B, K))).astype(np.float32)
        y = rng.integers(0, K, size=B).astype(np.int64)
        out.append((f, z, y))
    return out
