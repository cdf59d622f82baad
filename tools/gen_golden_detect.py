#!/usr/bin/env python
"""Writes tests/golden/detect.npz: a few score / flag sets (N <= 300) with what scikit-learn returns for them --
roc_auc_score, average_precision_score and the false-positive rate at the first threshold of roc_curve(drop_intermediate=False)
whose true-positive rate reaches 0.95.  tests/test_host_detect.py holds the float64 restatement (tests/detect_ref.py) against them.
Needs numpy and scikit-learn only.

    python tools/gen_golden_detect.py
"""
import os

import numpy as np
from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    rng = np.random.default_rng(20240611)
    out = {}
    s = rng.standard_normal(300).astype(np.float32)
    out["continuous_300"] = (s, (rng.random(300) < 0.3 + 0.2 * np.tanh(s)).astype(np.uint8))
    s = rng.random(257).astype(np.float32)
    out["rare_positive_257"] = (s, (rng.random(257) < 0.04 * (1 + 3 * s)).astype(np.uint8))
    q = (rng.integers(0, 7, 300) / 8.0).astype(np.float32)                      # heavy ties: 7 values
    out["ties7_300"] = (q, (rng.random(300) < 0.15 + 0.6 * q).astype(np.uint8))
    q = (rng.integers(0, 3, 41) - 1.0).astype(np.float32)                       # -1, 0, 1 with both signs of zero
    q[::5] = np.where(q[::5] == 0, np.float32(-0.0), q[::5])
    out["ties3_signed_zero_41"] = (q, (rng.random(41) < 0.5).astype(np.uint8))
    s = rng.standard_normal(100).astype(np.float32)
    f = np.zeros(100, dtype=np.uint8)
    f[int(np.argsort(s)[70])] = 1
    out["one_positive_100"] = (s, f)
    q = (rng.integers(0, 4, 64) / 4.0).astype(np.float32)
    f = np.zeros(64, dtype=np.uint8)
    f[int(np.nonzero(q == 0.5)[0][0])] = 1
    out["one_positive_tied_64"] = (q, f)
    s = rng.standard_normal(20).astype(np.float32)
    out["p20_exact_95_percent_20"] = (np.concatenate([s, s + 0.5]).astype(np.float32), np.repeat(np.array([0, 1], dtype=np.uint8), 20))
    out["two_2"] = (np.array([0.25, 0.75], dtype=np.float32), np.array([1, 0], dtype=np.uint8))
    return out


def main():
    data, names = {}, []
    for name, (s, f) in cases().items():
        assert s.dtype == np.float32 and f.dtype == np.uint8 and 0 < int(f.sum()) < len(f)
        fpr, tpr, _ = roc_curve(f, s, drop_intermediate=False)
        names.append(name)
        data["scores/" + name], data["flags/" + name] = s, f
        data["auroc/" + name] = np.float64(roc_auc_score(f, s))
        data["ap/" + name] = np.float64(average_precision_score(f, s))
        data["fpr95/" + name] = np.float64(fpr[int(np.argmax(tpr >= 0.95))])
        print(f"{name}: N {len(s)}, P {int(f.sum())}, AUROC {data['auroc/' + name]:.6f}, AP {data['ap/' + name]:.6f}, FPR95 {data['fpr95/' + name]:.6f}")
    data["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "detect.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
