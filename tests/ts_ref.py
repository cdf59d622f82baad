"""Test helper: temperature scaling (csrc/tscale.hip) restated in float64 numpy -- the mean NLL of softmax(s z)
and its first two derivatives in s = 1 / T, an independent fit by bisection, the kernel's bracketed Newton iteration, and the error
bounds of the kernel's fp32 steps.  numpy only.

    f(s) = (1 / n) sum_i [ log sum_k exp(s d_ik) - s d_i,y ],  d_ik = z_ik - max_k z_ik        mean NLL at temperature 1 / s
    g(s) = f'(s)  = (1 / n) sum_i [ sum_k p_ik d_ik - d_i,y ]
    h(s) = f''(s) = (1 / n) sum_i [ sum_k p_ik d_ik^2 - (sum_k p_ik d_ik)^2 ] >= 0
f is convex and g non-decreasing: the minimiser over [1 / t_max, 1 / t_min] is the root of g when it lies inside, else a bound.  Rows with
a non-finite logit take no part (the kernel leaves them out and counts them).

Bounds (u = 2^-24; derived to first order from the arithmetic the file header of tscale.hip states, not tuned).  Per row at the point s
the kernel forms d_k = fl(z_k - m), relative error u; a_k = fl32(s d_k), one more u, so the argument of the exponential is off by at
most 2 u s |d_k|; e_k = expf(a_k), at most 1 ulp: relative 2^-23.  So e_k carries the relative error eta_k <= 2^-23 + 2 u s |d_k|.
From there on the kernel works in double.  With p_k the softmax at s, A = sum_k p_k |d_k| and A2 = sum_k p_k d_k^2, the sum S = sum e_k
has the relative error
    rho <= sum_k p_k eta_k + K 2^-126 / S + 2^-50 = 2^-23 + 2 u s A + K 2^-126 / S + 2^-50
(K 2^-126 / S: exponentials below the fp32 normal range; 2^-50: the double sums), the weights p~_k = e_k / S are off by eta_k + rho, and
the multiplier d_k of sum_k p~_k d_k and the label's d_y carry u each.  Hence, per row,
    |g_i - ref| <= sum_k p_k |d_k| (eta_k + rho) + u A + u |d_y| = (2^-23 + rho + u) A + 2 u s A2 + u |d_y|
    |f_i - ref| <= rho + u s |d_y|                                                   d(log S) = rho
The means over the rows are double sums of at most 2^20 terms in some fixed order: at most 2^-33 times the mean absolute row value,
plus 1e-15 for the restatement itself.  bound_g and bound_nll are the means of the row bounds plus those two terms.
"""
import functools

import numpy as np

U = 2.0 ** -24
T_MIN, T_MAX, TOL, MAX_ITER = 0.01, 100.0, 1e-7, 16
MAX_N = 1 << 20
STATUS = ("converged", "clamped at T_max", "clamped at T_min", "iteration limit")


class Rows:
    """The usable rows of a set: d (n, K) float64 = z - row max, dy (n,) = d at the label."""

    def __init__(self, z, y):
        z = np.asarray(z, dtype=np.float32)
        y = np.asarray(y, dtype=np.int64)
        if z.ndim != 2 or y.shape != (z.shape[0],):
            raise ValueError("z (N, K) and y (N,)")
        if bool(((y < 0) | (y >= z.shape[1])).any()):
            raise ValueError("a label outside [0, K)")
        keep = np.isfinite(z).all(1)
        x = z[keep].astype(np.float64)
        self.N, self.K, self.n = z.shape[0], z.shape[1], int(keep.sum())
        self.d = x - x.max(1, keepdims=True) if self.n else x
        self.dy = self.d[np.arange(self.n), y[keep]]

    def moments(self, s):
        """Per row at s: log S, S, mu = sum p d, q = sum p d^2, A = sum p |d|."""
        e = np.exp(s * self.d)
        S = e.sum(1)
        ed = e * self.d
        mu = ed.sum(1) / S
        q = (ed * self.d).sum(1) / S
        return np.log(S), S, mu, q, -mu                     # d <= 0: A = -mu

    def fgh(self, s):
        if not self.n:
            return (float("nan"),) * 3
        logS, _, mu, q, _ = self.moments(s)
        return float((logS - s * self.dy).mean()), float((mu - self.dy).mean()), float((q - mu * mu).mean())

    def g(self, s):
        return self.fgh(s)[1]

    def bounds(self, s):
        """(bound on |f_dev - f_ref|, bound on |g_dev - g_ref|) at the same s."""
        logS, S, mu, q, A = self.moments(s)
        rho = 2.0 ** -23 + 2.0 * U * s * A + self.K * 2.0 ** -126 / S + 2.0 ** -50
        ady = np.abs(self.dy)
        bf = rho + U * s * ady
        bg = (2.0 ** -23 + rho + U) * A + 2.0 * U * s * q + U * ady
        tail = 2.0 ** -33
        return (float(bf.mean() + tail * np.abs(logS - s * self.dy).mean() + 1e-15),
                float(bg.mean() + tail * np.abs(mu - self.dy).mean() + 1e-15))


def nll_g_h(z, y, s):
    """(f, g, h) at s."""
    return Rows(z, y).fgh(float(s))


def bound_g(z, y, s):
    return Rows(z, y).bounds(float(s))[1]


def bound_nll(z, y, s):
    return Rows(z, y).bounds(float(s))[0]


def _range(t_min, t_max):
    s_min, s_max = 1.0 / t_max, 1.0 / t_min
    return s_min, s_max, max(t_min, 1.0 / s_max), min(t_max, 1.0 / s_min)


def _result(rows, s, status, t_lo, t_hi, passes=None):
    f, g, _ = rows.fgh(s)
    return {"s": s, "T": min(max(1.0 / s, t_lo), t_hi), "status": status, "nll_before": rows.fgh(1.0)[0], "nll_after": f, "grad": g,
            "passes": passes, "n": rows.n, "n_skipped": rows.N - rows.n}


def fit_bisect(z, y, t_min=T_MIN, t_max=T_MAX, rows=None):
    """The independent answer: the bounds first, then the root of g by bisection in log s until hi / lo - 1 <= 1e-13."""
    rows = rows if rows is not None else Rows(z, y)
    s_min, s_max, t_lo, t_hi = _range(t_min, t_max)
    if rows.g(s_max) <= 0.0:
        return _result(rows, s_max, 2, t_lo, t_hi)
    if rows.g(s_min) >= 0.0:
        return _result(rows, s_min, 1, t_lo, t_hi)
    lo, hi = np.log(s_min), np.log(s_max)
    while hi - lo > 1e-13:
        mid = 0.5 * (lo + hi)
        if rows.g(float(np.exp(mid))) < 0.0:
            lo = mid
        else:
            hi = mid
    return _result(rows, float(np.exp(0.5 * (lo + hi))), 0, t_lo, t_hi)


def fit_newton(z, y, t_min=T_MIN, t_max=T_MAX, tol=TOL, max_iter=MAX_ITER, rows=None):
    """The kernel's iteration: pass 1 at s_max, s_min and s_0 = clamp(1); then the bracketed Newton.  Reports the passes and the status."""
    rows = rows if rows is not None else Rows(z, y)
    s_min, s_max, t_lo, t_hi = _range(t_min, t_max)
    if rows.g(s_max) <= 0.0:
        return _result(rows, s_max, 2, t_lo, t_hi, 1)
    if rows.g(s_min) >= 0.0:
        return _result(rows, s_min, 1, t_lo, t_hi, 1)
    lo, hi, s, passes = s_min, s_max, min(max(1.0, s_min), s_max), 1
    while True:
        _, g, h = rows.fgh(s)
        if g < 0.0:
            lo = s
        else:
            hi = s
        with np.errstate(all="ignore"):
            cand = s - np.float64(g) / np.float64(h)
        if not (h > 0.0 and np.isfinite(h)) or not (lo < cand < hi):
            cand = float(np.sqrt(lo * hi))
        if abs(cand - s) <= tol * s or g == 0.0:
            return _result(rows, s, 0, t_lo, t_hi, passes)
        if passes >= max_iter:
            return _result(rows, s, 3, t_lo, t_hi, passes)
        s, passes = float(cand), passes + 1


# ---- the inputs of the GPU grid, shared by tests/test_host_ts.py and tests/test_gpu_ts.py ----
GRID_N = (1, 2, 3, 63, 64, 65, 257, 4097, 20011,
          15, 16, 17, 4095, 4096)   # 16 rows per workgroup: 15 | 16 | 17; 256 partials per stride of the summing step: 16 * 256 = 4096 | 4097
GRID_K = (2, 3, 10, 100, 1000, 1003)
GRID_SCALE = (0.25, 1.0, 4.0)
GRID = [(N, K, sc) for N in GRID_N for K in GRID_K for sc in GRID_SCALE if N * K <= 3_000_000]
# the row pass keeps 1, 4 or 16 columns per lane in registers (K <= 64, 256, 1024) and reads longer rows twice: both sides of each
GRID += [(N, K, 1.0) for N in (65, 257) for K in (64, 65, 256, 257, 1024, 1025, 2500)]


def make_inputs(N, K, scale):
    rng = np.random.default_rng(7 * N + K)
    y = rng.integers(0, K, size=N)
    z = rng.standard_normal((N, K)).astype(np.float32)
    z[np.arange(N), y] += np.float32(3.0)
    z = (z * np.float32(scale)).astype(np.float32)
    redraw = rng.random(N) < 0.3
    y = np.where(redraw, rng.integers(0, K, size=N), y).astype(np.int64)
    return z, y


@functools.lru_cache(maxsize=None)
def _grid_fit(N, K, scale):
    z, y = make_inputs(N, K, scale)
    return fit_bisect(z, y)


def grid_case(N, K, scale):
    """(z, y, rows, fit_bisect's result) of one grid point; the fit, the expensive part, is computed once per process."""
    z, y = make_inputs(N, K, scale)
    return z, y, Rows(z, y), dict(_grid_fit(N, K, scale))
