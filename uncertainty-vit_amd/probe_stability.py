"""Stability under perturbation sequences for every probe head (csrc/stability.hip): a mixin of LinearProbe."""
import ctypes as C
import math

import torch

from . import native
from .native import check, cur_stream, lib, ptr
from .probe_util import image_batches

STABILITY_MAX_FRAMES = 256   # csrc/stability.hip: 2 <= F <= 256, 1 <= V <= 65535, 1 <= K <= 4096


class StabilityMixin:
    def _stability_buffers_for(self, R, V):
        """Ranks (R, K) int32 and per-sequence sums (V, 3) float64 of the stability ops (csrc/stability.hip), grown on demand."""
        self._need_gpu("the stability ops run")
        dev = self._arena.device
        if R > self._rank_rows:
            self._ranks = torch.zeros(R, self.num_classes, dtype=torch.int32, device=dev)
            self._rank_rows = R
        if V > self._seq_rows:
            self._seq = torch.zeros(V, 3, dtype=torch.float64, device=dev)
            self._seq_rows = V

    def _stability_into(self, logits, V, F, noise, out):
        """The two ops on `logits` (V F, K) on the current stream; `out` is a device pointer to V x 3 doubles."""
        K, L, s = self.num_classes, lib(), cur_stream()
        check(L.uvit_op_stability_ranks(ptr(logits), ptr(self._ranks), V * F, K, s), "uvit_op_stability_ranks")
        check(L.uvit_op_stability_sequences(ptr(self._ranks), C.c_void_p(out), V, F, K, 1 if noise else 0, s), "uvit_op_stability_sequences")

    @staticmethod
    def _frames(frames):
        F = int(frames)
        if not 2 <= F <= STABILITY_MAX_FRAMES:
            raise native.UvitError(f"frames must be in [2, {STABILITY_MAX_FRAMES}], got {frames}")
        return F

    def stability_batch(self, logits, frames, noise):
        """The reference's per-sequence stability sums (uncertainty_evaluations.py: flip_prob, ranking_dist) of caller-supplied GPU
        logits (V * frames, K) fp32, the frames of a sequence adjacent: a (V, 3) float64 device tensor {flips, top-5 distance, Zipf
        distance} summed over each sequence's frames - 1 pairs (divide by frames - 1 for the sequence's values), valid until the next
        call; nothing synchronises with the host.  `noise`: every frame is compared with frame 0 instead of with the frame before it
        (the reference's rule for perturbations with 'noise' in their name).  A sequence that holds a NaN logit gives three NaNs.  The
        ordinal ranks (rank 1 = the largest logit, ties to the lower index, 0 in a row with a NaN) stay in self._ranks[:V * frames]."""
        R = self._check_logits(logits, "V * frames")
        F = self._frames(frames)
        if R < F or R % F:
            raise native.UvitError(f"{R} logit rows are not whole sequences of {F} frames")
        V = R // F
        self._stability_buffers_for(R, V)
        self._stability_into(logits, V, F, noise, self._seq.data_ptr())
        return self._seq[:V]

    def evaluate_stability(self, loader, frames, noise, n_sequences=None):
        """The reference's p_evaluate() for one perturbation.  `loader` yields batches of V * frames GPU images, sequence-major, as
        images, (images, labels) or ((images, mask), labels) (the device prefetcher's items over datasets.PerturbationSequences).  Per
        batch: encoder eval forward, pool + norm, logits, ranks, per-sequence sums, written on the device at the running sequence
        offset of one slab sized for the data set: `n_sequences`, by default len(loader.dataset) or len(loader.loader.dataset) (a
        loader that says neither needs the argument; more sequences than that are an error).  One read after the last batch.  The
        host divides by frames - 1 and takes the means in float64, in sequence order, over the sequences without a NaN logit;
        `nan_sequences` counts the others.  Per-sequence values do not depend on how the sequences are batched: each is a function
        of its own logits."""
        F = self._frames(frames)
        if n_sequences is None:
            ds = getattr(getattr(loader, "loader", loader), "dataset", None)
            if ds is None or not hasattr(ds, "__len__"):
                raise native.UvitError("evaluate_stability sizes its slab for the data set: pass n_sequences (the loader has no dataset to count)")
            n_sequences = len(ds)
        slab, n = None, 0
        for images, B in image_batches(self, loader):
            if B % F:
                raise native.UvitError(f"a batch of {B} images is not whole sequences of {F} frames")
            V = B // F
            if n + V > n_sequences:
                raise native.UvitError(f"the loader holds more than the {n_sequences} sequences the slab was sized for")
            self._logits_into(B)
            self._stability_buffers_for(B, 0)
            if slab is None:
                slab = torch.zeros(int(n_sequences), 3, dtype=torch.float64, device=images.device)
            self._stability_into(self._logits, V, F, noise, slab.data_ptr() + 24 * n)
            n += V
        out = {"flip_prob": float("nan"), "top5_dist": float("nan"), "zipf_dist": float("nan"), "n_sequences": n, "frames": F,
               "nan_sequences": 0}
        if not n:
            return out
        rows = slab[:n].cpu().tolist()                                                  # the one read
        good = [r for r in rows if not any(math.isnan(v) for v in r)]
        out["nan_sequences"] = n - len(good)
        for col, key in enumerate(("flip_prob", "top5_dist", "zipf_dist")):
            if good:
                out[key] = sum(r[col] / (F - 1) for r in good) / len(good)
        return out
