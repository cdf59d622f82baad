"""Generate tests/golden/scal.npz by running the UNMODIFIED reference metric classes (uncertainty_evaluations.ECELoss, MCELoss, OELoss,
SCELoss, ACELoss, TACELoss and BrierScore, imported from the reference checkout through tools/ref_harness.py) on sets of more than 1024
rows, which the per-batch ops cannot take.  Build-container only; never runs on the GPU box.

    python tools/gen_golden_scal.py [--out FILE]

As tools/gen_golden_calib.py explains, the six calibration classes run, unmodified, with logits=False on a torch float64 copy of fp32
probabilities; BrierScore().loss is called on the fp32 logits (it applies scipy's softmax itself).  The stored values carry the
reference's positional reading of the bin accuracy (tests/calib_ref.py: _bin_acc); tests/test_host_scal.py pins tests/scal_ref.py to
them at positional_acc=True.

To keep the archive under 100 KB (22 000 fp32 probabilities alone do not deflate below 77 KB) the fixture stores the logits, which lie
on a 1/2 grid, as int8 (`logits_q2/<case>`, z = q / 2) and NOT the probabilities: those are tests/scal_ref.py's
probs_from_grid_logits(q), the float64 softmax with its sum added left to right, rounded once to fp32.  The only step of it that is not
exactly specified by IEEE 754 is exp, so the generator accepts a case only when every float64 probability is at least 2^-40
(relative) away from a midpoint between two fp32 values: any exp within a thousand ulps of the correctly rounded one then gives the
same fp32 bits, and the test reproduces the probabilities the reference saw.  `probs_crc/<case>` (zlib.crc32 of the fp32 bytes) lets
the test say so.  Labels are uint8.  The last case has no logits: its probabilities lie on a 1/64
grid.  The margin rule of gen_golden_calib.py holds for every bound a probability is compared with: the top-label and class-wise
equal-width bin edges, the TACE threshold and the adaptive bounds of ACE and TACE.  A drawn case that violates it takes the next seed.
The fixture is data only; a second run gives the same bytes."""
import argparse
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness  # noqa: E402
import scal_ref as sr  # noqa: E402
from gen_golden_calib import MARGIN, grid_case, untied_maximum, write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "scal.npz")
CASES = [("n1100_k6", 1100, 6), ("n1536_k10", 1536, 10)]
GRID = ("grid64_n1200_k10", 1200, 10)
ECE_BINS, CW_BINS, ACE_BINS, TACE_BINS, TACE_THR = 15, 15, 15, 30, 0.01


def draw(N, K, seed):
    """int8 logits q (z = q / 2, spread 2.5, no tied row maximum) and labels that follow the row maximum two times in three."""
    g = torch.Generator().manual_seed(seed)
    q = torch.clamp(torch.round(torch.randn(N, K, generator=g) * 5.0), -126, 126).to(torch.int8)
    top = q.max(1, keepdim=True).values
    first = (q == top).int().argmax(1)                       # a grid has tied maxima: the first of them goes one step up
    q[torch.arange(N), first] += ((q == top).sum(1) > 1).to(torch.int8)
    y = torch.randint(0, K, (N,), generator=g)
    follow = torch.rand(N, generator=g) < 0.66
    y = torch.where(follow, q.float().argmax(1), y)
    return q, y.to(torch.int64)


def adaptive_clear(p, thr, bins):
    N, K = p.shape
    v = np.where(p < thr, 0.0, p)
    bin_n = N // bins
    for c in range(K):
        s = np.sort(v[:, c])
        for i in range(bins):
            b = s[i * bin_n]
            if b == 0.0:
                continue                             # thresholded values: equal zeros stay equal zeros
            if ((np.abs(s - b) <= MARGIN * b).sum()) != 1:
                return False
    return True


def clear_of_bounds(p32):
    """No probability within MARGIN (relative) of a bound it is compared with."""
    p = p32.astype(np.float64)
    conf = p.max(1)
    for b in np.linspace(0, 1, ECE_BINS + 1)[1:]:
        if (np.abs(conf - b) <= MARGIN * b).any():
            return False
    for b in np.linspace(0, 1, CW_BINS + 1)[1:]:
        if (np.abs(p - b) <= MARGIN * b).any():
            return False
    if (np.abs(p - TACE_THR) <= MARGIN * TACE_THR).any():
        return False
    return adaptive_clear(p, 0.0, ACE_BINS) and adaptive_clear(p, TACE_THR, TACE_BINS)


def reference_metrics(ue, out, name, p64, y):
    out["ece/" + name] = np.float64(ue.ECELoss().loss(p64, y, n_bins=ECE_BINS, logits=False))
    out["mce/" + name] = np.float64(ue.MCELoss().loss(p64, y, n_bins=ECE_BINS, logits=False))
    out["oe/" + name] = np.float64(ue.OELoss().loss(p64, y, n_bins=ECE_BINS, logits=False))
    out["sce/" + name] = np.float64(ue.SCELoss().loss(p64, y, n_bins=CW_BINS, logits=False))
    out["ace/" + name] = np.float64(ue.ACELoss().loss(p64.clone(), y, n_bins=ACE_BINS, logits=False))
    out["tace/" + name] = np.float64(ue.TACELoss().loss(p64.clone(), y, threshold=TACE_THR, n_bins=TACE_BINS, logits=False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    ref_harness.install()
    import uncertainty_evaluations as ue

    out = {"names": np.array([c[0] for c in CASES] + [GRID[0]]), "ece_bins": np.int64(ECE_BINS), "cw_bins": np.int64(CW_BINS),
           "ace_bins": np.int64(ACE_BINS), "tace_bins": np.int64(TACE_BINS), "tace_threshold": np.float64(TACE_THR), "margin": np.float64(MARGIN)}
    for n, (name, N, K) in enumerate(CASES):
        seed = 2000 * (n + 1)
        while True:
            q, y = draw(N, K, seed)
            z = q.float() / 2.0
            p32, clear = sr.probs_from_grid_logits(q.numpy(), with_margin=True)
            p32 = torch.from_numpy(p32)
            if clear and untied_maximum(p32.numpy()) and clear_of_bounds(p32.numpy()):
                break
            seed += 1
        out["logits_q2/" + name], out["labels/" + name] = q.numpy(), y.numpy().astype(np.uint8)
        out["probs_crc/" + name] = np.int64(zlib.crc32(p32.numpy().astype("<f4").tobytes()))
        out["seed/" + name] = np.int64(seed)
        reference_metrics(ue, out, name, p32.double(), y)
        out["brier/" + name] = np.float64(ue.BrierScore().loss(z.numpy(), y.numpy()))
        print(name, "seed", seed, {k: float(out[k + "/" + name]) for k in ("ece", "mce", "oe", "sce", "ace", "tace", "brier")})
    name, N, K = GRID
    p32, y = grid_case(N, K, 78)
    assert untied_maximum(p32) and np.array_equal(p32 * 64, np.round(p32 * 64)) and bool((p32.astype(np.float64).sum(1) == 1.0).all())
    out["probs_q64/" + name], out["labels/" + name] = np.round(p32 * 64).astype(np.uint8), y.astype(np.uint8)
    reference_metrics(ue, out, name, torch.from_numpy(p32).double(), torch.from_numpy(y))
    print(name, {k: float(out[k + "/" + name]) for k in ("ece", "mce", "oe", "sce", "ace", "tace")})
    write_npz(a.out, out)
    size = os.path.getsize(a.out)
    assert size < 100 * 1024, size
    print("wrote", a.out, size, "bytes")


if __name__ == "__main__":
    main()
