"""NumPy restatement of the stability metrics of perturbation sequences (the reference's p_evaluate: uncertainty_evaluations.py
flip_prob, ranking_dist, dist), the yardstick of csrc/stability.hip.  numpy only.

Ordinal rank of class k in a logit row z:  r[k] = 1 + #{j : z_j > z_k} + #{j < k : z_j == z_k}  (= rankdata(-z, method='ordinal')):
rank 1 is the largest logit, ties go to the lower index, +0 == -0, +-inf order like any other value.  A row with a NaN has no
ranks: all 0.  `ranks_by_definition` counts literally (O(K^2) per row); `ranks` forms the same two counts from one stable sort per row
and is what the large shapes use; tests/test_host_stability.py holds the two equal.

The three metrics of a pair (a = ranks of the reference frame, b = ranks of frame t) exist twice: per class (`pair_per_class`, the
form the kernel computes) and per rank position, the way the reference arranges it (`pair_permutation`, for K >= 6; for K < 6 only
the per-class form is defined).  The tie to the reference itself is the fixture, tests/golden/stability.npz.
"""
import numpy as np


def ranks_by_definition(z):
    """(R, K) float -> (R, K) int32, literally from the definition."""
    z = np.asarray(z)
    R, K = z.shape
    out = np.zeros((R, K), dtype=np.int32)
    lower = np.tril(np.ones((K, K), dtype=bool), -1)                      # lower[k, j] = j < k
    for r in range(R):
        row = z[r]
        if np.isnan(row).any():
            continue
        greater = row[None, :] > row[:, None]                            # [k, j] = z_j > z_k
        equal_before = (row[None, :] == row[:, None]) & lower
        out[r] = 1 + greater.sum(1) + equal_before.sum(1)
    return out


def ranks(z):
    """The same counts from a stable ascending sort: #{z_j > z_k} = K - (end of z_k's run), #{j < k : z_j == z_k} = k's place within
    its run (a stable sort keeps equal values in index order)."""
    z = np.asarray(z)
    R, K = z.shape
    out = np.zeros((R, K), dtype=np.int32)
    for r in range(R):
        row = z[r]
        if np.isnan(row).any():
            continue
        order = np.argsort(row, kind="stable")
        s = row[order]
        run_start, run_end = np.searchsorted(s, s, side="left"), np.searchsorted(s, s, side="right")
        rk = np.empty(K, dtype=np.int64)
        rk[order] = 1 + (K - run_end) + (np.arange(K) - run_start)
        out[r] = rk
    return out


def pair_per_class(a, b):
    """(flip, top-5 distance, Zipf distance) of one pair from ranks a (reference frame) and b, class by class."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    flip = int(np.argmin(a) != np.argmin(b))                              # the class with rank 1
    top = a <= 5
    top5 = int(np.abs((a[top] - 1) - np.minimum(b[top] - 1, 5)).sum())
    af, bf = a.astype(np.float64), b.astype(np.float64)
    zipf = float((np.abs(1.0 / af - 1.0 / bf) / af).sum())
    return flip, top5, zipf


def pair_permutation(a, b):
    """The same three numbers summed over rank positions instead of classes (K >= 6), the way the reference arranges the work:
    sigma[p] = the rank in b of the class that a puts at position p (rank p + 1).  top-5: the first five positions, each compared
    with where its class went, capped at 5; Zipf: |1 / (p + 1) - 1 / sigma[p]| / (p + 1) over all positions."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    K = a.shape[0]
    sigma = b[np.argsort(a)]
    place = np.arange(1, K + 1, dtype=np.float64)
    top5 = int(np.abs(np.arange(5) - np.minimum(sigma[:5] - 1, 5)).sum())
    zipf = float((np.abs(1.0 / place - 1.0 / sigma) / place).sum())
    return int(sigma[0] != 1), top5, zipf


def sequence_sums(rk, noise, pair=pair_per_class):
    """rk (F, K) ranks of one sequence -> [flips, top-5 sum, Zipf sum] over its F - 1 pairs, pairs in frame order; NaN x 3 when a
    row has no ranks (a rank of 0)."""
    rk = np.asarray(rk)
    if (rk < 1).any():
        return [float("nan")] * 3
    acc = [0, 0, 0.0]
    for t in range(1, rk.shape[0]):
        v = pair(rk[0 if noise else t - 1], rk[t])
        acc = [acc[0] + v[0], acc[1] + v[1], acc[2] + v[2]]
    return [float(acc[0]), float(acc[1]), float(acc[2])]


def sequences(rk, V, F, noise, pair=pair_per_class):
    """rk (V F, K), sequence-major -> (V, 3) float64 of sequence_sums."""
    rk = np.asarray(rk).reshape(V, F, -1)
    return np.array([sequence_sums(rk[v], noise, pair) for v in range(V)], dtype=np.float64).reshape(V, 3)


def dataset_values(sums, F):
    """(V, 3) per-sequence sums -> what evaluate_stability returns: means, in sequence order, of sum / (F - 1) over the sequences
    without a NaN."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 3)
    good = [r for r in sums.tolist() if not any(np.isnan(r))]
    out = {"n_sequences": len(sums), "frames": F, "nan_sequences": len(sums) - len(good)}
    for col, key in enumerate(("flip_prob", "top5_dist", "zipf_dist")):
        out[key] = sum(r[col] / (F - 1) for r in good) / len(good) if good else float("nan")
    return out


def evaluate(logits, V, F, noise):
    """logits (V F, K) -> dataset_values of the per-class form on ranks()."""
    return dataset_values(sequences(ranks(logits), V, F, noise), F)
