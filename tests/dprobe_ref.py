"""float64 restatement (numpy, CPU) of the two-stream probe and the bounds its tests hold, written from the
definition and not from the kernels:

    pool + norm   t = mean of tokens 1 .. N-1; feat = (t - mean t) / sqrt(var t + eps), eps = 1e-6 (the encoder's ln_eps), no affine
    v             s (c > 0 ? c + 1 : exp(c)) = s (ELU(c) + 1) of the covariance stream's feature c
    var           var[b, k] = sum_c W[k, c]^2 v[b, c]
    trace         trace[b] = mean_c v[b, c]
    link          z / sqrt(1 + factor var)

Bounds, with u = 2^-53 for the double ops and u32 = 2^-24 for the fp32 ones (derived, not tuned):
  var, trace      |got - ref| <= 2 (C + 4) u ref.  Every term w^2 v is non-negative, w^2 is exact, v costs a rounding of c + 1 or a
                  1-ulp exp and one product with s (3 u with room), a C-term fma chain in any one order is within C u of the exact sum,
                  and numpy's sum in another order obeys the same bound: hence the factor 2.  HIP documents its double-precision exp
                  at 1 ulp, so nothing wider is needed.  trace is rounded to fp32 once more: + 2^-24 |ref|.
  pool + norm     the pooled mean is a sum of R = N - 1 fp32 terms in some order, e_t <= (R + 8) u32 mean_tokens |x| per column
                  (tests/rowwise_ref.py's column-sum bound, divided by R); the LayerNorm behind it is a row operator with rowwise_ref's
                  g_row(C) on its own sums, and it carries e_t through y = (t - mu) r:
                  |dy| <= r (e_t + mean e_t) + |t - mu| r^3 mean_c(|t - mu| (e_t + mean e_t)) + g_row ((|t| + mean |t|) r + |t - mu| r).
"""
import ctypes as C
import math

import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24
LN_EPS = 1e-6


def gamma_row(C):
    """tests/rowwise_ref.py's g_row: a lane's serial adds, the wave shuffle tree, slack for the products."""
    return (4 * math.ceil(C / 256) + 16) * U32


def pool_norm(x, eps=LN_EPS):
    """x (B, N, C) -> (B, C) float64."""
    t = np.asarray(x, dtype=np.float64)[:, 1:].mean(1)
    d = t - t.mean(-1, keepdims=True)
    return d / np.sqrt((d * d).mean(-1, keepdims=True) + eps)


def pool_norm_bound(x, eps=LN_EPS, e_in=None):
    """Per-element bound (B, C) on |fp32 pool + norm - pool_norm(x)| for fp32 inputs x.  `e_in` (B, N, C): an error bound the inputs
    themselves carry (the golden comparison), which the mean and the normalisation carry on."""
    x = np.asarray(x, dtype=np.float64)
    R, Cd = x.shape[1] - 1, x.shape[2]
    ax = np.abs(x[:, 1:]).mean(1)
    e_t = (R + 8) * U32 * ax
    if e_in is not None:
        e_t = e_t + np.asarray(e_in, dtype=np.float64)[:, 1:].mean(1)
    t = x[:, 1:].mean(1)
    d = t - t.mean(-1, keepdims=True)
    r = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    e_d = e_t + e_t.mean(-1, keepdims=True)
    g = gamma_row(Cd)
    return r * e_d + np.abs(d) * r ** 3 * (np.abs(d) * e_d).mean(-1, keepdims=True) + g * ((np.abs(t) + np.abs(t).mean(-1, keepdims=True)) * r + np.abs(d) * r)


def feature_variance(c, scale=1.0):
    """v (B, C) float64 of the fp32 covariance feature c."""
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    return scale * np.where(c > 0, c + 1.0, np.exp(np.minimum(c, 0.0)))      # np.minimum carries a NaN c on: the row stays NaN


def variance(c, W, scale=1.0):
    """var (B, K) float64: sum_c W[k, c]^2 v[b, c]."""
    w2 = np.asarray(W, dtype=np.float32).astype(np.float64) ** 2
    return feature_variance(c, scale) @ w2.T


def variance_chain(c, W, scale=1.0):
    """The same sum, the columns one by one in ascending order (np.cumsum adds sequentially): what one fma chain gives wherever every
    product w^2 v is exact."""
    v = feature_variance(c, scale)
    w2 = np.asarray(W, dtype=np.float32).astype(np.float64) ** 2
    return np.cumsum(v[:, None, :] * w2[None, :, :], axis=-1)[..., -1]


def trace(c, scale=1.0):
    return feature_variance(c, scale).mean(-1)


def variance_bound(ref, C):
    return 2 * (C + 4) * U64 * np.abs(ref)


def trace_bound(ref, C):
    return (2 * (C + 4) * U64 + U32) * np.abs(ref)


def link(z, var, factor):
    """(B, K) float64: z / sqrt(1 + factor var) of fp32 logits z."""
    return np.asarray(z, dtype=np.float32).astype(np.float64) / np.sqrt(1.0 + factor * np.asarray(var, dtype=np.float64))


def predicted_variance(z, var):
    """var at the arg-max of the unscaled logits (the lowest index on ties), (B,) float64."""
    z = np.asarray(z)
    return np.asarray(var)[np.arange(z.shape[0]), z.argmax(-1)]


# ---- what the launchers refuse -------------------------------------------------------------------------------------------------
P1, NUL = C.c_void_p(4096), C.c_void_p(0)
ARG, SHAPE = -1, -2


def bad_calls(L):
    """(what, return code, expected code): every refusal of the three entry points; none of them reaches a launch."""
    f, d = C.c_float(1e-6), C.c_double
    out = [("pool ws", L.uvit_op_dprobe_pool_ws_bytes(3, 10, 128), 2 * L.uvit_op_probe_pool_ws_bytes(3, 10, 128)),
           ("pool ws value", L.uvit_op_dprobe_pool_ws_bytes(3, 10, 128), 2 * 3 * 8 * 128 * 4)]
    pool = lambda p, B=3, N=10, Cd=128: L.uvit_op_dprobe_pool_norm(*p, B, N, Cd, f, NUL)                      # noqa: E731
    var = lambda p, s=1.0, B=3, K=5, Cd=128: L.uvit_op_dprobe_variance(p[0], p[1], d(s), p[2], p[3], B, K, Cd, NUL)      # noqa: E731
    for i in range(5):                                                       # x_mean, x_cov, feat_mean, feat_cov, scratch
        a = [P1] * 5
        a[i] = NUL
        out.append((f"pool NULL {i}", pool(a), ARG))
    for kw in (dict(B=0), dict(B=65536), dict(N=1), dict(Cd=0), dict(Cd=6), dict(Cd=2052)):      # uvit_op_probe_pool_norm's limits
        out.append((f"pool {kw}", pool([P1] * 5, **kw), SHAPE))
        out.append((f"pool ws {kw}", L.uvit_op_dprobe_pool_ws_bytes(kw.get("B", 3), kw.get("N", 10), kw.get("Cd", 128)), SHAPE))
        out.append((f"probe pool {kw}", L.uvit_op_probe_pool_norm(P1, P1, P1, kw.get("B", 3), kw.get("N", 10), kw.get("Cd", 128), f, NUL), SHAPE))
    for i in range(3):                                                       # cfeat, W, var are required; trace is not
        a = [P1] * 4
        a[i] = NUL
        out.append((f"variance NULL {i}", var(a), ARG))
    for s in (0.0, -1.0, float("nan"), float("inf")):
        out.append((f"variance scale {s}", var([P1] * 4, s=s), ARG))
    for kw in (dict(B=0), dict(B=65536), dict(K=0), dict(K=65536), dict(Cd=0), dict(Cd=6), dict(Cd=2052)):
        out.append((f"variance {kw}", var([P1] * 4, **kw), SHAPE))
    return out
