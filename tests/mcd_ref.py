"""Test helper: the MC-dropout combination (csrc/mcd.hip) restated on the host in float64 -- the streaming
accumulation of T passes into a per-row state, the finalisation into combined logits and five uncertainty columns, an independent
brute-force form over the whole (T, B, K) stack, and the derived bounds of tests/test_gpu_mcd.py.  numpy only.

The bounds.  u = 2^-24 is the unit round-off of fp32, ud = 2^-53 that of double.  The device's expf / logf are documented at 1 ulp;
the bounds take 2 ulp = 4 u relative for each.  For one pass of a row with logits z (exact fp32 inputs), R = max z - min z:
  d_k = fl(z_k - max)                  |error| <= u R
  e_k = expf(d_k)                      relative <= (R + 4) u
  se  = sum_k e_k                      ceil(K / 64) terms per lane, then a 6-level tree: relative <= (R + 4 + ceil(K / 64) + 6) u =: a
  lg  = logf(se), 0 <= lg <= ln K      |error| <= a + 4 u ln K
  x_k = fl(d_k - lg), |x_k| <= R + ln K  |error| <= u R + a + 4 u ln K + u (R + ln K)
  p_k = expf(x_k)                      relative <= that + 4 u = u (3 R + 5 ln K + ceil(K / 64) + 14) =: eps_p      (first order; x 1.01)
and absolutely no better than the smallest normal fp32, 2^-126, where expf underflows.  The sums over t are double sums of T terms:
relative T ud of the sum of magnitudes, so with eps = max_t eps_p of the row
  pbar_k       |error| <= (eps + T ud) pbar_k + 2^-126
  z, mode 0    (float)(sum_z / T): |error| <= (u + (T + 1) ud) |z|
  z, mode 1    (float) log(pbar): |error| <= (eps + T ud) + 2^-126 / pbar + (u + 4 ud) |z|; compared where pbar >= 2^-100
  h_t          d(p log p) = (1 + log p) dp: |error| <= eps sum_k p (1 + |log p|) + K 2^-119
  aleatoric    the mean of those (+ T ud);   total: the same expression in pbar;   mi: the sum of the two (max(., 0) is 1-Lipschitz)
  var_pred     the raw-moment form m2 - pbar^2 with m2 = sum_p2[k*] / T: p^2 has relative error 2 eps, and pbar^2 <= m2, so
               |error| <= (4 eps + (T + 8) ud) m2 -- relative to the second moment, not to the variance: the price of one pass
The votes are exact: each pass's arg max is taken on exact fp32 inputs.  pred, var_pred and disagreement hang on k* = argmax z, which
is compared only where the gap between the two largest z of the reference exceeds twice the bound of z."""
import math

import numpy as np

U, UD, TINY = 2.0 ** -24, 2.0 ** -53, 2.0 ** -126
F64 = np.float64
P_FLOOR = 2.0 ** -100          # mode 1 compares z where the reference's pbar is at least this
UNC_KEYS = ("mcd_total", "mcd_aleatoric", "mcd_mi", "mcd_var", "mcd_disagreement")

# (B, K, T) of the op tests: one row, one class, one pass; fewer classes than lanes; K across the 64-lane boundary; more than one
# workgroup; the ImageNet head
SHAPES = [(1, 1, 1), (3, 2, 2), (5, 10, 3), (17, 65, 5), (130, 1000, 4)]


def logits_case(shape, seed=0, scale=3.0):
    """(T, B, K) fp32 random logits of a shape (B, K, T)."""
    B, K, T = shape
    rng = np.random.default_rng(1000 * seed + 7 * B + K + T)
    return (scale * rng.standard_normal((T, B, K))).astype(np.float32)


def xlogx(p):
    return np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)


def softmax64(z):
    """Rows of an (.., K) fp32 array -> float64 softmax, formed as the device forms it: (z - max) - log(sum exp(z - max))."""
    x = np.asarray(z, dtype=np.float32).astype(F64)
    d = x - x.max(-1, keepdims=True)
    return np.exp(d - np.log(np.exp(d).sum(-1, keepdims=True)))


def first_argmax(z):
    """The lowest index of the largest value; -1 for a row without a value above -inf or with a NaN."""
    z = np.asarray(z)
    bad = np.isnan(z).any(-1) | ~(z > -np.inf).any(-1)
    return np.where(bad, -1, np.argmax(np.where(np.isnan(z), -np.inf, z), axis=-1))


def bad_rows(z):
    """Rows without a softmax: a NaN or +inf logit, or nothing above -inf."""
    z = np.asarray(z, dtype=np.float32)
    return np.isnan(z).any(-1) | np.isposinf(z).any(-1) | ~(z > -np.inf).any(-1)


def accumulate(state, z, first):
    """One pass z (B, K) fp32 into `state` (a dict, or None with first): the streaming form of uvit_op_mcd_accumulate."""
    z = np.asarray(z, dtype=np.float32)
    B, K = z.shape
    with np.errstate(all="ignore"):
        p = softmax64(z)
        h = -xlogx(p).sum(-1)
    votes = np.zeros((B, K), dtype=np.int64)
    k = first_argmax(z)
    rows = np.nonzero(k >= 0)[0]
    votes[rows, k[rows]] = 1
    new = {"sum_z": z.astype(F64), "sum_p": p, "sum_p2": p * p, "votes": votes, "sum_h": h, "flag": bad_rows(z)}
    if first:
        return new
    return {key: (state[key] | new[key]) if key == "flag" else state[key] + new[key] for key in new}


def finalize(state, T, mode):
    """(z (B, K) float64 before the final rounding to fp32, unc (B, 5) float64, k* (B)) of a state after T passes."""
    with np.errstate(all="ignore"):
        pbar = state["sum_p"] / T
        z = state["sum_z"] / T if mode == 0 else np.log(pbar)
        kstar = first_argmax(z.astype(np.float32))
        total = -xlogx(pbar).sum(-1)
        aleatoric = state["sum_h"] / T
        rows = np.arange(z.shape[0])
        ks = np.maximum(kstar, 0)
        pk = pbar[rows, ks]
        var = np.maximum(state["sum_p2"][rows, ks] / T - pk * pk, 0.0)
        dis = 1.0 - state["votes"][rows, ks] / T
        unc = np.stack([total, aleatoric, np.maximum(total - aleatoric, 0.0), var, dis], axis=1)
    unc[state["flag"] | (kstar < 0)] = np.nan
    return z, unc, kstar


def combine(stack, mode):
    """The restatement over a (T, B, K) stack: accumulate pass by pass, then finalize."""
    state = None
    for t, z in enumerate(stack):
        state = accumulate(state, z, t == 0)
    return finalize(state, len(stack), mode) + (state,)


def brute(stack, mode):
    """The same quantities by their definitions over the whole stack: means over axis 0, the centred variance, the per-pass
    predictions compared with the combination's.  (z, unc, k*)."""
    x = np.asarray(stack, dtype=np.float32)
    T, B, K = x.shape
    with np.errstate(all="ignore"):
        p = softmax64(x)                                   # (T, B, K)
        pbar = p.mean(0)
        z = x.astype(F64).mean(0) if mode == 0 else np.log(pbar)
        kstar = first_argmax(z.astype(np.float32))
        ks = np.maximum(kstar, 0)
        total = -xlogx(pbar).sum(-1)
        aleatoric = (-xlogx(p).sum(-1)).mean(0)
        rows = np.arange(B)
        pk = p[:, rows, ks]                                # (T, B)
        var = ((pk - pk.mean(0)) ** 2).mean(0)
        km = np.stack([first_argmax(x[t]) for t in range(T)])
        dis = (km != ks[None]).sum(0) / T
        unc = np.stack([total, aleatoric, np.maximum(total - aleatoric, 0.0), var, dis], axis=1)
    unc[bad_rows(x.transpose(1, 0, 2).reshape(B, T * K)) | (kstar < 0)] = np.nan
    return z, unc, kstar


def eps_p(stack):
    """(B,) the relative error bound of a pass's fp32 softmax, the largest over the passes of each row."""
    x = np.asarray(stack, dtype=np.float32).astype(F64)
    K = x.shape[-1]
    R = (x.max(-1) - x.min(-1)).max(0)
    return 1.01 * U * (3.0 * R + 5.0 * math.log(K) + math.ceil(K / 64) + 14.0)


def bounds(stack, mode):
    """The derived bounds of the module docstring for a stack without bad rows: {"z" (B, K), "z_mask" (B, K) bool: entries that are
    compared, "total", "aleatoric", "mi", "var" (B,), "gap_ok" (B,) bool: k* is decided}."""
    x = np.asarray(stack, dtype=np.float32)
    T, B, K = x.shape
    z, unc, kstar, state = combine(x, mode)
    eps = eps_p(x) + T * UD
    p = softmax64(x)
    pbar = p.mean(0)
    if mode == 0:
        zb, mask = (U + (T + 1) * UD) * np.abs(z), np.ones((B, K), dtype=bool)
    else:
        mask = pbar >= P_FLOOR
        with np.errstate(all="ignore"):
            zb = np.where(mask, eps[:, None] + TINY / np.where(mask, pbar, 1.0) + (U + 4 * UD) * np.abs(z), np.inf)
    w = lambda q: (q * (1.0 + np.abs(np.log(np.where(q > 0, q, 1.0))))).sum(-1)      # noqa: E731
    small = K * 2.0 ** -119
    aleatoric = eps * w(p).mean(0) + small + T * UD
    total = eps * w(pbar) + small
    m2 = state["sum_p2"][np.arange(B), np.maximum(kstar, 0)] / T
    var = (4.0 * eps + (T + 8) * UD) * m2 + TINY
    # k* is decided when the two largest z are further apart than both of their bounds together
    if K == 1:
        gap_ok = np.ones(B, dtype=bool)
    else:
        order = np.argsort(-z, axis=-1, kind="stable")[:, :2]
        rows = np.arange(B)
        gap = z[rows, order[:, 0]] - z[rows, order[:, 1]]
        gap_ok = gap > zb[rows, order[:, 0]] + zb[rows, order[:, 1]]
    return {"z": zb, "z_mask": mask, "total": total, "aleatoric": aleatoric, "mi": total + aleatoric, "var": var, "gap_ok": gap_ok}


def auroc(scores, positive):
    """The probability that a positive row scores above a negative one, ties counting a half."""
    s, f = np.asarray(scores, dtype=F64), np.asarray(positive, dtype=bool)
    pos, neg = s[f], s[~f]
    return float(((pos[:, None] > neg[None]).sum() + 0.5 * (pos[:, None] == neg[None]).sum()) / (len(pos) * len(neg)))


def entropy_of_logits(z):
    """The entropy of softmax(z) per row: the `entropy` detection column of the combined logits."""
    return -xlogx(softmax64(z)).sum(-1)


def meaning_case(K=8, rows=12, seed=5):
    """(T, 2 rows, K) fp32 with T = K passes, and the (2 rows,) flags.  Rows [0, rows): every pass gives the same nearly flat logits --
    the model is sure that it does not know.  Rows [rows, 2 rows): pass t is confident of class (t + shift) % K -- the passes disagree.
    Both groups have a nearly flat mean, so the entropy of the combination cannot tell them apart; the mutual information can."""
    rng = np.random.default_rng(seed)
    T = K
    x = np.zeros((T, 2 * rows, K), dtype=np.float32)
    x[:, :rows] = (0.05 * rng.standard_normal((1, rows, K))).astype(np.float32)
    for b in range(rows):
        for t in range(T):
            x[t, rows + b, (t + b) % K] = 8.0
    x[:, rows:] += (0.05 * rng.standard_normal((1, rows, K))).astype(np.float32)
    flags = np.arange(2 * rows) >= rows
    return x, flags
