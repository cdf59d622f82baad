"""MC-dropout probe on the frozen encoder: T stochastic passes of the encoder under attention dropout, combined on the device -- what
the reference evaluates with `--mc_dropout_forwards T` (uncertainty_evaluations.py: evaluate_MC_dropout :42-89, mc_dropout_c_evaluate,
mc_dropout_p_evaluate; enable_dropout() :35-39 switches the Dropout modules to train mode, T passes run over the whole loader, every
pass's logits are kept and torch.mean(outputs, 0) is scored), DESIGN.md section 9.14.

    one deterministic forward (LinearProbe._features)            -> the pooled feature of maha / knn / vim, and every X[l]
    T x { blocks first_layer .. depth-1 again under the masks of (seed, it)  (uvit_engine_forward_tail)
          -> pool + norm -> head -> uvit_op_mcd_accumulate }     -> one uvit_op_mcd_finalize: z and five uncertainty columns

With dropout in the last n of L blocks only, the blocks in front of them compute the same thing in every pass, so a batch costs
1 + T n / L encoder passes instead of the reference's T.  The head, its arenas and its checkpoint keys are a LinearProbe's, and so is
train_step (a deterministic encoder, no tails): the head is trained as the reference trains it and sampled only when it is evaluated.
Nothing of size (T, B, K) is stored and nothing is read back between the passes.
"""
import ctypes as C
import math

import torch

from .linear_probe import LinearProbe
from .native import check, cur_stream, f32, lib, ptr
from .probe_util import ws_size

__all__ = ["MCDropoutProbe"]

COMBINE_MODES = {"logits": 0, "probs": 1}
UNC_KEYS = ("mcd_total", "mcd_aleatoric", "mcd_mi", "mcd_var", "mcd_disagreement")      # the columns of uvit_op_mcd_finalize's unc


class MCDropoutProbe(LinearProbe):
    """state_dict() holds a LinearProbe's `head.weight` and `head.bias`: any linear probe-N.pth resumes.  `passes`: T.  `layers`: n,
    attention dropout in the last n blocks only (0: in all of them).  `combine`: "logits" (the mean of the passes' logits, the
    reference's) or "probs" (the logarithm of the mean of their softmaxes).  The masks of pass t of the n-th batch of an evaluation are
    those of a training-mode forward at (seed, n * passes + t), so a repeated evaluation gives the same bits."""

    DETECT_COLUMNS = LinearProbe.DETECT_COLUMNS + UNC_KEYS

    def __init__(self, encoder, num_classes, passes=8, layers=0, combine="logits", seed=0, smoothing=0.1, init_scale=0.001):
        T, n = int(passes), int(layers)
        if T < 1:
            raise ValueError(f"passes must be >= 1, got {passes}")
        if combine not in COMBINE_MODES:
            raise ValueError(f"combine must be one of {sorted(COMBINE_MODES)}, got {combine!r}")
        if not float(getattr(encoder, "attn_drop_rate", 0.0) or 0.0) > 0.0:
            raise ValueError("MC-dropout samples the encoder's attention dropout: build the encoder with attn_drop_rate > 0")
        depth = int(getattr(encoder, "depth", 0))
        if not 0 <= n <= depth:
            raise ValueError(f"layers must be in [0, {depth}] (0: every block), got {layers}")
        self.passes, self.layers, self.combine, self.seed = T, n, combine, int(seed) & 0xFFFFFFFF
        self.first_layer = depth - n if n else 0
        self._mc_batch, self._mc_train, self._eval = 0, False, None
        super().__init__(encoder, num_classes, smoothing=smoothing, init_scale=init_scale)

    def _head_buffers_for(self, B):
        K, Cd, dev = self.num_classes, self.embed_dim, self._arena.device
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
        self._mc_feat, self._mc_lin, self._unc = z(B, Cd), z(B, K), z(B, 5, dt=torch.float64)
        self._mc_state = z(ws_size(lib().uvit_op_mcd_state_bytes, B, K), dt=torch.uint8)
        self._mc_det = z(2)                      # the loss slot of the deterministic pass's criterion (not reported)

    # ---- forward ----
    def _pass_into(self, B, it, dropout=True):
        """One pass behind the deterministic forward: the tail at (seed, it), pool + norm into self._mc_feat, the head into
        self._mc_lin.  self._feat keeps the deterministic feature."""
        enc, K, Cd, L, s = self.encoder, self.num_classes, self.embed_dim, lib(), cur_stream()
        e = enc.forward_tail(self.first_layer, self.seed, it, dropout=dropout)
        x = L.uvit_engine_ws_ptr(e.h, b"x", enc.depth)
        N = enc.patch_embed.num_patches + 1
        check(L.uvit_op_probe_pool_norm(C.c_void_p(x), ptr(self._mc_feat), ptr(self._scratch), B, N, Cd, f32(enc.ln_eps), s),
              "uvit_op_probe_pool_norm")
        check(L.uvit_op_probe_logits(ptr(self._mc_feat), ptr(self._arena), self._bias_ptr(self._arena), ptr(self._mc_lin), B, K, Cd, s),
              "uvit_op_probe_logits")

    def _combine_into(self, B, it0, unc):
        """T passes at (seed, it0 + t) into the state, then z into self._logits and the five columns into `unc` (B, 5) float64."""
        L, K, s = lib(), self.num_classes, cur_stream()
        for t in range(self.passes):
            self._pass_into(B, it0 + t)
            check(L.uvit_op_mcd_accumulate(ptr(self._mc_lin), ptr(self._mc_state), 1 if t == 0 else 0, B, K, s), "uvit_op_mcd_accumulate")
        check(L.uvit_op_mcd_finalize(ptr(self._mc_state), self.passes, COMBINE_MODES[self.combine], ptr(self._logits), ptr(unc), B, K, s),
              "uvit_op_mcd_finalize")

    def _labels(self, labels, B):
        labels = super()._labels(labels, B)
        if self._eval is not None:
            self._eval["labels"] = labels
        return labels

    def _logits_into(self, B):
        """The combined logits of the batch whose deterministic forward _features has just run.  Inside train_step: a LinearProbe's.
        Inside evaluate(): the five columns go to the detection store and to the slabs of their means, and with `uncertainty` the
        deterministic pass is scored beside the combination."""
        if self._mc_train:
            return super()._logits_into(B)
        ev, det = self._eval, self._det is not None
        want = ev is not None and ev["unc"] is not None
        slab = torch.zeros(B, 5, dtype=torch.float64, device=self._arena.device) if det or want else self._unc
        self._combine_into(B, self._mc_batch * self.passes, slab)
        self._mc_batch += 1
        if det:
            for col, name in enumerate(UNC_KEYS):
                self._own_column(name, slab[:, col], B, None)
        if want and not self._in_ood:
            ev["unc"].append(slab)
            if ev.get("labels") is not None:
                L, K, s = lib(), self.num_classes, cur_stream()
                if ev["counters"] is None:
                    ev["counters"] = torch.zeros(2, dtype=torch.int32, device=self._arena.device)
                check(L.uvit_op_probe_logits(ptr(self._feat), ptr(self._arena), self._bias_ptr(self._arena), ptr(self._mc_lin), B, K,
                                             self.embed_dim, s), "uvit_op_probe_logits")
                check(L.uvit_op_probe_ce(ptr(self._mc_lin), ptr(ev["labels"]), f32(0.0), None, ptr(self._row_loss), ptr(self._mc_det),
                                         ptr(ev["counters"]), B, K, s), "uvit_op_probe_ce")
        if ev is not None:
            ev["labels"] = None

    def _from_batch_zero(self, fn, *a, **kw):
        """An evaluation entry point: its batches count from 0, so the n-th batch draws the masks of it = n * passes + t."""
        self._mc_batch = 0
        return fn(*a, **kw)

    def logits(self, images):
        return self._from_batch_zero(super().logits, images)

    forward = logits

    def predictive(self, images, it0=0):
        """{"logits": (B, K) fp32, "unc": (B, 5) float64} on the device: the combination of the passes at (seed, it0 + t), t = 0 ..
        passes - 1, and its columns {predictive entropy of the mean softmax, mean entropy of the passes, their difference (the mutual
        information, clamped at 0), variance over the passes of the probability of the predicted class, share of the passes whose
        prediction differs from the combination's}.  The n-th batch of an evaluation is predictive(images, n * passes)."""
        B = self._features(images)
        self._combine_into(B, int(it0), self._unc)
        return {"logits": self._logits[:B].clone(), "unc": self._unc[:B].clone()}

    # ---- training: a LinearProbe's, on the deterministic forward ----
    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        self._mc_train = True
        try:
            return super().train_step(images, labels, lr, weight_decay, max_norm)
        finally:
            self._mc_train = False

    # ---- evaluation ----
    def evaluate(self, loader, calibration=False, uncertainty=False, detection=False, ood_loader=None, temperature=None):
        """LinearProbe.evaluate on the combined logits.  `uncertainty`: the means over the set of the five columns of predictive() as
        `mcd_total`, `mcd_aleatoric`, `mcd_mi`, `mcd_var`, `mcd_disagreement`, over the rows without a NaN; `det_acc1`, the top-1 accuracy in percent of the deterministic pass (one more head and criterion call per batch),
        which shows what sampling does to the accuracy; `mcd_passes` and `mcd_layers`.  Everything comes from per-batch device slabs
        that are read once, after the last batch.  `detection`, `ood_loader`: as LinearProbe.evaluate, with the five columns beside
        the three of the logits, the OOD batches continuing the count of `it`.  `temperature`: on the combined logits; the five
        columns come from the passes and are not scaled.  maha, knn and vim read the deterministic feature."""
        self._eval = {"unc": [] if uncertainty else None, "counters": None, "labels": None}
        try:
            stats = self._from_batch_zero(super().evaluate, loader, calibration=calibration, detection=detection, ood_loader=ood_loader,
                                          temperature=temperature)
            if uncertainty:
                ev, n = self._eval, stats["n"]
                rows = torch.cat(ev["unc"]).cpu().tolist() if ev["unc"] else []
                good = [r for r in rows if not any(math.isnan(v) for v in r)]
                for col, key in enumerate(UNC_KEYS):
                    stats[key] = math.fsum(r[col] for r in good) / len(good) if good else float("nan")
                stats["det_acc1"] = 100.0 * int(ev["counters"].cpu()[0]) / n if n and ev["counters"] is not None else float("nan")
                stats["mcd_passes"], stats["mcd_layers"] = self.passes, self.encoder.depth - self.first_layer
        finally:
            self._eval = None
        return stats

    def evaluate_stability(self, loader, frames, noise, n_sequences=None):
        """StabilityMixin.evaluate_stability on the combined logits: the reference's mc_dropout_p_evaluate."""
        return self._from_batch_zero(super().evaluate_stability, loader, frames, noise, n_sequences=n_sequences)

    def fit_temperature(self, loader, *a, **kw):
        return self._from_batch_zero(super().fit_temperature, loader, *a, **kw)

    def fit_conformal(self, loader, *a, **kw):
        return self._from_batch_zero(super().fit_conformal, loader, *a, **kw)

    def evaluate_conformal(self, loader, *a, **kw):
        return self._from_batch_zero(super().evaluate_conformal, loader, *a, **kw)
