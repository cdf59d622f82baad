"""Generate tests/golden/stability.npz by running the UNMODIFIED reference functions (uncertainty_evaluations.flip_prob /
ranking_dist / dist and the rankdata it imports, reached through tools/ref_harness.py).  Build-container only; never runs on the GPU
box.

    python tools/gen_golden_stability.py [--out FILE]

Logits: 6 sequences x 5 frames x 100 classes, fp32 on a half-integer grid (so every tie is exact in any precision):
    0  values in [-8, 8]: about three classes per value
    1  the same, frame 2 a copy of frame 1 (a pair without any change)
    2  every logit of every frame 1.5 (all ranks decided by the class index)
    3  frames made of -0.0, +0.0 and +-0.5 only: the two zeros must tie
    4  values in [-2, 2]: about eleven classes per value
    5  values in [-2, 2], frames 1.. = frame 0 with a few classes moved
For each frame the reference's own expression np.uint16(rankdata(-frame, method='ordinal')) (uncertainty_evaluations.py:641) and
vid.argmax(1) (numpy: the first index among equals); for noise_perturbation False and True the reference's flip_prob(predictions),
ranking_dist(ranks, mode='top5') and ranking_dist(ranks, mode='zipf') over the six sequences, and the same three per sequence (the
functions called on one sequence at a time).  The fixture is data only; a second run gives the same bytes.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ref_harness  # noqa: E402
from gen_golden_calib import write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "stability.npz")
V, F, K = 6, 5, 100


def crafted_logits():
    rng = np.random.default_rng(2024)
    half = lambda lo, hi, shape: rng.integers(2 * lo, 2 * hi + 1, shape).astype(np.float32) / 2      # noqa: E731
    z = np.empty((V, F, K), dtype=np.float32)
    z[0] = half(-8, 8, (F, K))
    z[1] = half(-8, 8, (F, K))
    z[1, 2] = z[1, 1]
    z[2] = 1.5
    z[3] = rng.choice(np.array([-0.0, 0.0, 0.5, -0.5], dtype=np.float32), (F, K))
    z[4] = half(-2, 2, (F, K))
    z[5, 0] = half(-2, 2, K)
    for t in range(1, F):
        z[5, t] = z[5, t - 1]
        moved = rng.choice(K, 7, replace=False)
        z[5, t, moved] = half(-2, 3, 7)
    assert np.array_equal(z * 2, np.round(z * 2))
    assert bool(np.signbit(z[3][z[3] == 0]).any()) and not bool(np.signbit(z[3][z[3] == 0]).all())       # both zeros occur
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    ref_harness.install()
    import uncertainty_evaluations as ue

    z = crafted_logits()
    predictions = [vid.argmax(1) for vid in z]
    ranks = np.asarray([[np.uint16(ue.rankdata(-frame, method="ordinal")) for frame in vid] for vid in z])
    assert ranks.dtype == np.uint16 and ranks.shape == (V, F, K)
    out = {"logits": z, "ranks": ranks, "predictions": np.asarray(predictions).astype(np.int64)}
    for noise in (False, True):
        m = "noise%d" % int(noise)
        out["flip/" + m] = np.float64(ue.flip_prob(predictions, noise))
        out["top5/" + m] = np.float64(ue.ranking_dist(ranks, noise, mode="top5"))
        out["zipf/" + m] = np.float64(ue.ranking_dist(ranks, noise, mode="zipf"))
        out["flip_seq/" + m] = np.array([ue.flip_prob(predictions[v:v + 1], noise) for v in range(V)], dtype=np.float64)
        out["top5_seq/" + m] = np.array([ue.ranking_dist(ranks[v:v + 1], noise, mode="top5") for v in range(V)], dtype=np.float64)
        out["zipf_seq/" + m] = np.array([ue.ranking_dist(ranks[v:v + 1], noise, mode="zipf") for v in range(V)], dtype=np.float64)
        print(m, "flip", out["flip/" + m], "top5", out["top5/" + m], "zipf", out["zipf/" + m])
    write_npz(a.out, out)
    size = os.path.getsize(a.out)
    assert size < 100 * 1024, size
    print("wrote", a.out, size, "bytes")


if __name__ == "__main__":
    main()
