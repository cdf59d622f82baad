"""Float64 restatement of the k-nearest-neighbour score and classifier of the probe's feature (csrc/knn.hip,
LinearProbe.fit_neighbours / neighbour_scores), the shared cases and the bounds the GPU tests hold the device to.  NumPy throughout.

    rows     u = f / |f|, every element rounded to fp32 once and then to bf16 (nearest even); a row with a non-finite element, a
             zero norm or a label outside [0, K) is a zero row with label -1
    search   s(q, b) = sum_c q_c b_c over the bf16 values; per query the k largest among the bank rows with label >= 0, sorted by
             (s descending, index ascending); missing places hold -inf / -1, an invalid query NaN / -1
    scores   knn = 2 - 2 s_k;  votes_c = sum_j exp((s_j - s_1) / T) [label_j == c], pred = arg max (lowest class on ties)

The bounds.

  rows      The device sums |f|^2 in double: squares of widened fp32 values are exact, so a sum of C of them in any order has relative
            error <= (C - 1) u, u = 2^-53; sqrt, the reciprocal and the product f_c * (1 / |f|) add one rounding each: the device's
            scale lies within (C + 3) u of the exact 1 / |f|.  The restatement forms |f|^2 with math.fsum (one rounding), then
            sqrt, reciprocal and product (four roundings): together the exact factor lies within DELTA = (C + 8) u of the
            restatement's.  Rounding is monotone, so the device's bf16 value lies between bf16(fp32(f_c s (1 - DELTA))) and
            bf16(fp32(f_c s (1 + DELTA))); these are the same value except at a rounding boundary, where they are neighbours.  The
            accepted outputs are those two; there is no tolerance.
  search    A product of two bf16 numbers has 16 significant bits and is exact in fp32, so only the C accumulations inside the matrix
            instruction round.  With u32 = 2^-23 (which covers round-to-nearest and truncation) the standard bound of a C-term sum
            in any order is gamma_C sum_c |q_c b_c|, gamma_C = C u32 / (1 - C u32).  The restatement's float64 sum errs by at most
            C u sum_c |q_c b_c|, which is added:  bound(q, b) = (gamma_C + C u) sum_c |q_c b_c|.
            Sorted similarities: the j-th order statistic is 1-Lipschitz in the sup norm, so |sim[j] - ref_sorted[j]| <=
            max_b bound(q, b) for every j.  Indices: every idx[j] is distinct, in range, labelled >= 0, and
            |ref(q, idx[j]) - sim[j]| <= bound(q, idx[j]).
  knn       2 - 2 s_k is exact in float64 for an fp32 s_k with |s_k| <= 2, and the device rounds fmaf(-2, s_k, 2) once: the fp32
            value of the float64 expression, bit for bit.
  votes     x_j = (s_j - s_1) / T: the difference of two widened fp32 values (one rounding) and a division (one rounding), so x_j has
            relative error <= 2 u and exp(x_j) <= 2 |x_j| u from it; the double exp is within one ulp on the device and here.  A
            sum of at most k non-negative terms adds k u.  Per side (2 |x|_max + 2 + k) u votes_c, both sides:
            bound_c = 2 (k + 2 + 2 |x|_max) u votes_c.  pred is compared where the two largest votes differ by more than the sum of
            their two bounds.
"""
import math

import numpy as np

U = 2.0 ** -53
U32 = 2.0 ** -23
F64 = np.float64

# (B, C, N, k): one and three k-steps of 32, an odd step count, B and N on neither side of a tile, k across the 64-lane boundary, k = N
SHAPES = [(1, 32, 1, 1), (17, 96, 127, 5), (130, 96, 1000, 64), (33, 768, 1000, 65), (64, 128, 600, 256), (5, 32, 9, 9)]
SLABS = (1, 3, 7, 0)


# ---- bf16 ----
def bf16_round(x):
    """fp32 array -> the nearest bf16 value (ties to even), returned as fp32.  NaN stays NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, out).astype(np.float32)


def bf16_bits(x):
    """fp32 array of bf16 values -> their 16 bits as int16 (what a torch.bfloat16 tensor holds)."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def from_bf16_bits(b):
    return (np.ascontiguousarray(b).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---- rows ----
def usable_rows(feat, labels, K):
    f = np.asarray(feat, dtype=F64)
    ok = np.isfinite(f).all(axis=1) & ((f * f).sum(axis=1) > 0)
    if labels is not None:
        y = np.asarray(labels)
        ok &= (y >= 0) & (y < K)
    return ok


def rows(feat, labels=None, K=0):
    """(lo, hi, out_labels, sums): the two accepted bf16 values per element (fp32 arrays, equal except at a rounding boundary), the
    int32 labels (-1 for an unusable row, 0 for a usable row without labels) and [rows used, rows skipped]."""
    feat = np.asarray(feat, dtype=np.float32)
    ok = usable_rows(feat, labels, K)
    B, Cd = feat.shape
    delta = (Cd + 8) * U
    lo, hi = np.zeros((B, Cd), dtype=np.float32), np.zeros((B, Cd), dtype=np.float32)
    for b in np.nonzero(ok)[0]:
        f = feat[b].astype(F64)
        s = 1.0 / math.sqrt(math.fsum((f * f).tolist()))
        a, c = bf16_round((f * (s * (1 - delta))).astype(np.float32)), bf16_round((f * (s * (1 + delta))).astype(np.float32))
        lo[b], hi[b] = np.minimum(a, c), np.maximum(a, c)
    out_labels = np.where(ok, 0 if labels is None else np.asarray(labels), -1).astype(np.int32)
    return lo, hi, out_labels, np.array([ok.sum(), (~ok).sum()], dtype=F64)


def unit_bf16(feat):
    """Usable fp32 rows -> unit bf16 rows (the lower accepted value; fp32 array of bf16 values), for building search inputs."""
    return rows(feat)[0]


# ---- search ----
def similarities(q, bank):
    """(s (B, N), mag (B, N)) in float64: the dot products of the bf16 values and sum_c |q_c b_c|."""
    q, bank = np.asarray(q, dtype=F64), np.asarray(bank, dtype=F64)
    return q @ bank.T, np.abs(q) @ np.abs(bank).T


def bound_sim(mag, Cd):
    return (Cd * U32 / (1 - Cd * U32) + Cd * U) * mag


def search(q, valid, bank, bank_labels, k):
    """(sim (B, k) float64, idx (B, k) int64) of the restatement: -inf / -1 in missing places, NaN / -1 for an invalid query."""
    s, _ = similarities(q, bank)
    s = s + 0.0                                                                # -0 -> +0
    live = np.asarray(bank_labels) >= 0
    B, N = s.shape
    sim, idx = np.full((B, k), -np.inf), np.full((B, k), -1, dtype=np.int64)
    cand = np.nonzero(live)[0]
    for b in range(B):
        if valid[b] < 0:
            sim[b] = np.nan
            continue
        order = cand[np.lexsort((cand, -s[b, cand]))][:k]                      # similarity descending, index ascending
        sim[b, :len(order)], idx[b, :len(order)] = s[b, order], order
    return sim, idx


def search_brute_force(q, valid, bank, bank_labels, k):
    """The same through a stable argsort of the negated similarities over all rows, the dead ones pushed to -inf."""
    s, _ = similarities(q, bank)
    s = np.where(np.asarray(bank_labels)[None, :] >= 0, s + 0.0, -np.inf)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    sim = np.take_along_axis(s, order, axis=1)
    idx = np.where(np.isinf(sim), -1, order)
    pad = k - sim.shape[1]
    if pad > 0:
        sim, idx = np.pad(sim, ((0, 0), (0, pad)), constant_values=-np.inf), np.pad(idx, ((0, 0), (0, pad)), constant_values=-1)
    bad = np.asarray(valid) < 0
    sim[bad], idx[bad] = np.nan, -1
    return sim, idx


def check_search(sim, idx, q, valid, bank, bank_labels, k, what=""):
    """The device's (B, k) sim (fp32) and idx (int32) against the restatement within the derived bounds.  Prints the worst
    |error| / bound, asserts, and returns it."""
    sim, idx = np.asarray(sim), np.asarray(idx)
    B, Cd, N = q.shape[0], q.shape[1], bank.shape[0]
    s, mag = similarities(q, bank)
    bound = bound_sim(mag, Cd)
    ref_sim, _ = search(q, valid, bank, bank_labels, k)
    n_live = int((np.asarray(bank_labels) >= 0).sum())
    m = min(k, n_live)
    worst = 0.0
    for b in range(B):
        if valid[b] < 0:
            assert np.isnan(sim[b]).all() and (idx[b] == -1).all(), b
            continue
        assert np.isneginf(sim[b, m:]).all() and (idx[b, m:] == -1).all(), b
        got, ids = sim[b, :m].astype(F64), idx[b, :m].astype(np.int64)
        assert len(set(ids.tolist())) == m and ids.min(initial=0) >= 0 and ids.max(initial=0) < N, b
        assert (np.asarray(bank_labels)[ids] >= 0).all(), b
        assert all((got[j] > got[j + 1]) or (got[j] == got[j + 1] and ids[j] < ids[j + 1]) for j in range(m - 1)), b      # the total order
        sup = bound[b].max()
        r1 = np.abs(got - ref_sim[b, :m]).max(initial=0.0) / max(sup, 1e-300)
        r2 = (np.abs(s[b, ids] - got) / np.maximum(bound[b, ids], 1e-300)).max(initial=0.0)
        worst = max(worst, r1, r2)
    print(f"\nsearch {what}: worst |error| / bound {worst:.4f}")
    assert worst <= 1.0
    return worst


# ---- scores ----
def knn_score(s_k):
    """fp32 2 - 2 s_k, rounded once (NaN for a missing or NaN k-th similarity)."""
    s_k = np.asarray(s_k, dtype=F64)
    return np.where(np.isfinite(s_k), 2.0 - 2.0 * s_k, np.nan).astype(np.float32)


def votes(sim, idx, bank_labels, K, T):
    """(votes (B, K) float64, bound (B, K), pred (B) int, decided (B) bool) from the (B, k) similarities (as the device reports them, fp32)
    and indices.  A row whose k-th entry is missing or NaN: NaN votes, pred -1, decided."""
    sim, idx, lab = np.asarray(sim, dtype=F64), np.asarray(idx), np.asarray(bank_labels)
    B, k = sim.shape
    v, bound = np.zeros((B, K)), np.zeros((B, K))
    pred, decided = np.full(B, -1), np.ones(B, dtype=bool)
    for b in range(B):
        if not np.isfinite(sim[b, k - 1]) or idx[b, k - 1] < 0:
            v[b] = np.nan
            continue
        x = (sim[b] - sim[b, 0]) / T
        w = np.exp(x)
        for j in range(k):
            c = lab[idx[b, j]]
            if 0 <= c < K:
                v[b, c] += w[j]
        bound[b] = 2 * (k + 2 + 2 * np.abs(x).max()) * U * v[b]
        order = np.argsort(-v[b], kind="stable")                               # the lowest class among equals first
        pred[b] = order[0]
        decided[b] = v[b, order[0]] - v[b, order[1]] > bound[b, order[0]] + bound[b, order[1]]
    return v, bound, pred, decided


def auroc(scores_in, scores_out):
    """P(out > in) + P(out == in) / 2 over all pairs."""
    a, b = np.asarray(scores_in, dtype=F64)[:, None], np.asarray(scores_out, dtype=F64)[None, :]
    return float(((b > a).sum() + 0.5 * (b == a).sum()) / (a.size * b.size))


def knn_mean(knn):
    v = np.asarray(knn, dtype=F64)
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else float("nan")


# ---- shared cases ----
def search_case(B, Cd, N, k, seed=0):
    """{"q", "valid", "bank", "labels", "K", "first"}: a random asymmetric bank of unit bf16 rows with classes 0 .. 6; from N >= 9 on,
    every row n % 7 == 3 is dead (label -1) and row N - 2 repeats row 1, row N - 1 repeats row 4.  The queries are the bank rows
    0 .. B - 1 (an identity-like product: a row/column swap in the accumulator write shows at once); `first` (B) is the index each
    query must report first: itself, or -1 where its own bank row is dead (then the restatement decides)."""
    rng = np.random.default_rng(9000 + 131 * B + 17 * Cd + 3 * N + k + 7919 * seed)
    bank = unit_bf16(rng.standard_normal((N, Cd)).astype(np.float32))
    labels = rng.integers(0, 7, size=N).astype(np.int32)
    if N >= 9:
        bank[N - 2], bank[N - 1] = bank[1], bank[4]
        labels[np.arange(N) % 7 == 3] = -1
        labels[[N - 2, N - 1]] = labels[[1, 4]]                                # the two repeats are live, as rows 1 and 4 are
    q = bank[:B].copy()
    first = np.where(labels[:B] >= 0, np.arange(B), -1)
    return {"q": q, "valid": np.zeros(B, dtype=np.int32), "bank": bank, "labels": labels, "K": 7, "first": first}


def clustered_case(B=40, Cd=64, N=500, K=5, seed=3):
    """Clustered unit rows (class means plus noise): many close similarities, labels = the cluster."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((K, Cd))
    y = (np.arange(N) % K).astype(np.int32)
    bank = unit_bf16((means[y] + 0.3 * rng.standard_normal((N, Cd))).astype(np.float32))
    yq = (np.arange(B) % K).astype(np.int64)
    q = unit_bf16((means[yq] + 0.3 * rng.standard_normal((B, Cd))).astype(np.float32))
    return {"q": q, "valid": np.zeros(B, dtype=np.int32), "bank": bank, "labels": y, "K": K, "yq": yq}


def scores_cases():
    """Hand-made (sim (B, k) fp32, idx (B, k) int32, bank_labels, K, T, pred wanted): an exact tie between two classes goes to the
    lower class; a single neighbour; a row with a missing tail and a NaN row give NaN / -1."""
    lab = np.array([2, 1, 1, 2, 0, -1], dtype=np.int32)
    sim = np.array([[0.5, 0.5, 0.25, 0.25],          # classes 2, 1, 1, 2: equal votes, class 1 wins
                    [0.75, 0.5, 0.5, 0.5],           # class 0 alone against three of class 1 at exp(-0.25 / T)
                    [0.5, 0.25, -np.inf, -np.inf],   # fewer than k neighbours
                    [np.nan] * 4], dtype=np.float32)
    idx = np.array([[0, 1, 2, 3], [4, 1, 2, 1], [0, 1, -1, -1], [-1] * 4], dtype=np.int32)
    return sim, idx, lab, 3, 0.07, [1, 0, -1, -1]


def meaning_rows(f, width=64):
    """maha_ref.meaning_case's 16 features as the first 16 of `width` (the encoder's attention needs an embed dim of at least 64): the
    zero entries change no norm and no dot product."""
    f = np.asarray(f, dtype=np.float32)
    return np.concatenate([f, np.zeros((len(f), width - f.shape[1]), dtype=np.float32)], axis=1)
