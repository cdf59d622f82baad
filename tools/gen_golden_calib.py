"""Generate tests/golden/calib.npz by running the UNMODIFIED reference metric classes (uncertainty_evaluations.ECELoss / TACELoss /
NLL, imported from the reference checkout through tools/ref_harness.py).  Build-container only; never runs on the GPU box.

    python tools/gen_golden_calib.py [--out FILE]

Under the scipy installed here the reference classes do not run on logits (scipy.special.softmax returns an ndarray and
`confidences, _ = probabilities.max(axis=1)` then fails); they do run, unmodified, with logits=False on a torch float64 probability
tensor.  So each case draws fp32 logits, forms fp32 probabilities with torch.softmax, widens them to float64 and calls
ECELoss().loss(p, y, logits=False) and TACELoss().loss(p.clone(), y, logits=False) (TACELoss thresholds its input in place);
NLL(logits, y) is called on the logits as the reference's evaluate() does.  The last case has no logits: its probabilities lie on a
1/64 grid (column ties, many values under the TACE threshold) and its NLL entry is NaN.

AUROC has no pin from the reference (torchmetrics is not installed): `auroc/<case>` holds scikit-learn's
roc_auc_score(y == c, p[:, c]) for every class with a positive and a negative row, NaN elsewhere.

What the stored ECE / TACE are: the reference's `in_bin` is a uint8 0/1 array (np.greater on a torch tensor returns through
Tensor.__array_wrap__, which turns bool into uint8) and `accuracies` is a numpy array, so `accuracies[in_bin]` indexes by position:
the stored bin accuracy is the mean over ALL rows b of accuracies[in_bin[b]], not the mean over the rows of the bin.  The bin
proportions and bin confidences (`ece_bins/<case>`, columns 0 and 2) are masked means;
tests/calib_ref.py restates both readings (positional_acc), as the kernels compute both (include/uvit.h).

The fixture is data only.  The generator asserts what the tests rely on: no row has a tied maximum; and, for the cases with logits,
no probability lies within 1e-6 relative of a bound it is compared with (an ECE bin edge, the TACE threshold, another element of
its column that serves as an adaptive bound), so a softmax that differs from torch's in the last bits leaves every bin membership
as it is.  A drawn case that violates this takes the next seed.  The archive is written with fixed time stamps: a second run gives
the same bytes.
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "calib.npz")
CASES = [("b48_k10", 48, 10), ("b37_k10", 37, 10), ("b29_k10", 29, 10), ("b30_k10", 30, 10), ("b64_k100", 64, 100)]
GRID = ("grid64_b40_k10", 40, 10)
ECE_BINS, TACE_BINS, TACE_THR = 15, 30, 0.01
MARGIN = 1e-6


def draw(B, K, seed):
    """fp32 logits of spread 2.5 and labels that follow the row maximum two times in three (a classifier that is often right)."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, K, generator=g) * 2.5).float()
    y = torch.randint(0, K, (B,), generator=g)
    follow = torch.rand(B, generator=g) < 0.66
    y = torch.where(follow, z.argmax(1), y)
    return z, y.to(torch.int64)


def untied_maximum(p):
    top = np.sort(p, axis=1)[:, -2:]
    return p.shape[1] == 1 or bool((top[:, 1] > top[:, 0]).all())


def clear_of_bounds(p32):
    """No probability within MARGIN (relative) of a bound it is compared with."""
    p = p32.astype(np.float64)
    B, K = p.shape
    conf = p.max(1)
    for b in np.linspace(0, 1, ECE_BINS + 1)[1:]:
        if (np.abs(conf - b) <= MARGIN * b).any():
            return False
    if (np.abs(p - TACE_THR) <= MARGIN * TACE_THR).any():
        return False
    v = np.where(p < TACE_THR, 0.0, p)
    bin_n = B // TACE_BINS
    for c in range(K):
        s = np.sort(v[:, c])
        for i in range(TACE_BINS):
            b = s[i * bin_n]
            if b == 0.0:
                continue                             # thresholded values: equal zeros stay equal zeros
            if ((np.abs(s - b) <= MARGIN * b).sum()) != 1:
                return False
    return True


def grid_case(B, K, seed):
    """Probabilities k / 64 with rows that sum to 1 and a single largest entry; labels as in draw()."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < B:
        cuts = np.sort(rng.integers(0, 65, K - 1))
        parts = np.diff(np.concatenate([[0], cuts, [64]]))
        top = np.sort(parts)[-2:]
        if top[1] > top[0]:
            rows.append(parts)
    p = (np.array(rows, dtype=np.float64) / 64.0).astype(np.float32)
    y = np.where(rng.random(B) < 0.66, p.argmax(1), rng.integers(0, K, B)).astype(np.int64)
    return p, y


def sklearn_auroc(p32, y):
    from sklearn.metrics import roc_auc_score
    B, K = p32.shape
    out = np.full(K, np.nan)
    for c in range(K):
        pos = y == c
        if pos.any() and not pos.all():
            out[c] = roc_auc_score(pos, p32[:, c].astype(np.float64))
    return out


def reference_metrics(ue, out, name, p64, y):
    """ECELoss / TACELoss of the reference on float64 probabilities, and the ECE object's own per-bin arrays."""
    ece = ue.ECELoss()
    out["ece/" + name] = np.float64(ece.loss(p64, y, n_bins=ECE_BINS, logits=False))
    out["ece_bins/" + name] = np.stack([ece.bin_prop, ece.bin_acc, ece.bin_conf], axis=1)        # (n_bins, 3): prop, acc, conf
    out["tace/" + name] = np.float64(ue.TACELoss().loss(p64.clone(), y, threshold=TACE_THR, n_bins=TACE_BINS, logits=False))


def write_npz(path, arrays):
    """np.savez_compressed with fixed member time stamps (a second run gives the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    ref_harness.install()
    import uncertainty_evaluations as ue

    out = {"names": np.array([c[0] for c in CASES] + [GRID[0]]), "ece_bins": np.int64(ECE_BINS), "tace_bins": np.int64(TACE_BINS),
           "tace_threshold": np.float64(TACE_THR), "margin": np.float64(MARGIN)}
    for n, (name, B, K) in enumerate(CASES):
        seed = 1000 * (n + 1)
        while True:
            z, y = draw(B, K, seed)
            p32 = torch.softmax(z, dim=1)
            if untied_maximum(p32.numpy()) and clear_of_bounds(p32.numpy()):
                break
            seed += 1
        p64 = p32.double()
        out["logits/" + name], out["probs/" + name], out["labels/" + name] = z.numpy(), p32.numpy(), y.numpy()
        out["seed/" + name] = np.int64(seed)
        reference_metrics(ue, out, name, p64, y)
        out["nll/" + name] = np.float64(ue.NLL(z, y).item())
        out["auroc/" + name] = sklearn_auroc(p32.numpy(), y.numpy())
        print(name, "seed", seed, "ECE", out["ece/" + name], "TACE", out["tace/" + name], "NLL", out["nll/" + name],
              "classes with an AUROC", int(np.isfinite(out["auroc/" + name]).sum()))
    name, B, K = GRID
    p32, y = grid_case(B, K, 77)
    assert untied_maximum(p32) and np.array_equal(p32 * 64, np.round(p32 * 64)) and bool((p32.astype(np.float64).sum(1) == 1.0).all())
    p64, yt = torch.from_numpy(p32).double(), torch.from_numpy(y)
    out["probs/" + name], out["labels/" + name] = p32, y
    reference_metrics(ue, out, name, p64, yt)
    out["nll/" + name] = np.float64("nan")
    out["auroc/" + name] = sklearn_auroc(p32, y)
    print(name, "ECE", out["ece/" + name], "TACE", out["tace/" + name], "values under the threshold",
          int((p32 < TACE_THR).sum()), "of", p32.size)
    write_npz(a.out, out)
    size = os.path.getsize(a.out)
    assert size < 100 * 1024, size
    print("wrote", a.out, size, "bytes")


if __name__ == "__main__":
    main()
