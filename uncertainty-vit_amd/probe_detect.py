"""Detection for every probe head: does an uncertainty column rank the wrong predictions, or another data set's images, above the
rest?  (csrc/detect.hip)  A mixin of LinearProbe: the evaluation's device store, a head's own columns, the
out-of-distribution loop and the set-level metrics."""
import ctypes as C

import torch

from . import native
from .native import check, cur_stream, lib, ptr
from .probe_util import grown, image_batches, workspace

DETECT_MAX_N, DETECT_MAX_S = 1 << 20, 16     # csrc/detect.hip: 1 <= N <= 2^20 samples, 1 <= S <= 16 columns
DETECT_KEYS = ("AUROC", "AUPR", "FPR95", "AURC")        # the first four entries of a row of uvit_op_detect_metrics' table


class DetectionMixin:
    def _det_reserve(self, B):
        """Room for B more samples in the evaluation's store: S fp32 columns of `cap` elements and one uint8 flag per sample, grown
        geometrically (what is there is copied on the device)."""
        d = self._det
        have = (d["scores"], d["flags"]) if d["cap"] else None
        specs = (((len(self.DETECT_COLUMNS), None), torch.float32, 0), ((None,), torch.uint8, 0))
        out = grown(have, d["n"], d["n"] + B, DETECT_MAX_N, f"detection ranks at most {DETECT_MAX_N} samples, the loaders hold more", specs,
                    self._arena.device)
        if out is not have:
            d.update(scores=out[0], flags=out[1], cap=out[1].shape[0])

    def _det_column(self, name, src, B):
        """A head's own column of the current batch -- `src` holds one float or double per row, any row stride -- into the store as
        fp32, behind the samples stored so far."""
        d = self._det
        at = d["scores"].data_ptr() + 4 * (self.DETECT_COLUMNS.index(name) * d["cap"] + d["n"])
        check(lib().uvit_op_detect_column(ptr(src), int(src.dtype == torch.float64), src.stride(0) if B > 1 else 1, C.c_void_p(at), B,
                                          cur_stream()), "uvit_op_detect_column")

    def _own_column(self, name, src, B, slabs, fresh=False):
        """A per-sample column that is not one of the three of the logits: into the detection store while there is one, and, for the
        evaluation set's rows (not the OOD images'), kept in `slabs` (None: not asked for) for column_mean() after the last batch.
        `fresh`: `src` was allocated for this batch and is kept as it is; a buffer of the probe is copied."""
        if self._det is not None:
            self._det_column(name, src, B)
        if slabs is not None and not self._in_ood:
            slabs.append(src[:B] if fresh else src[:B].clone())

    def _det_rows(self, B, labels):
        """The three scores of self._logits[:B] and, with labels, the wrong-prediction flags into the store; the batch is then stored."""
        d = self._det
        check(lib().uvit_op_detect_rows(ptr(self._logits), ptr(labels), ptr(d["scores"]), d["cap"], d["n"], ptr(d["flags"]), B,
                                        self.num_classes, cur_stream()), "uvit_op_detect_rows")
        d["n"] += B

    def _det_metrics(self, scores, ld, flags, N, S, order=None):
        """uvit_op_detect_metrics on the current stream: the (S, 8) float64 device table."""
        ws = workspace(self, "_det_ws", scores.device, lib().uvit_op_detect_ws_bytes, N, S)
        out = torch.zeros(S, 8, dtype=torch.float64, device=scores.device)
        check(lib().uvit_op_detect_metrics(ptr(scores), int(ld), ptr(flags), N, S, ptr(order), ptr(out), ptr(ws), ws.numel(), cur_stream()),
              "uvit_op_detect_metrics")
        return out

    def detection_batch(self, scores, flags, order=False):
        """The set-level metrics of caller-supplied GPU columns: `scores` (S, N) or (N,) fp32 with larger = more uncertain, `flags` (N,)
        uint8 with 1 = positive (2: a bad label).  Returns the (S, 8) float64 device table {AUROC, AUPR (average precision), FPR at
        95 % TPR, AURC, samples ranked, positives among them, NaN scores left out, 0} (include/uvit.h has the definitions); nothing
        synchronises with the host.  With `order`, also the (S, N) int32 sample indices in ascending (score, index) order, NaN rows
        last."""
        if not torch.is_tensor(scores) or not scores.is_cuda or not torch.is_tensor(flags) or not flags.is_cuda:
            raise native.UvitError("scores and flags must be GPU tensors: the HIP path has no CPU fallback")
        if scores.ndim == 1:
            scores = scores.unsqueeze(0)
        if scores.dtype != torch.float32 or scores.ndim != 2 or not scores.is_contiguous():
            raise native.UvitError("scores must be a contiguous float32 tensor of shape (S, N)")
        S, N = scores.shape
        if not (1 <= S <= DETECT_MAX_S and 1 <= N <= DETECT_MAX_N):
            raise native.UvitError(f"detection ranks 1 .. {DETECT_MAX_N} samples in 1 .. {DETECT_MAX_S} columns, got {N} in {S}")
        if flags.dtype != torch.uint8 or flags.shape != (N,) or not flags.is_contiguous():
            raise native.UvitError(f"flags must be a contiguous uint8 tensor of shape ({N},)")
        perm = torch.zeros(S, N, dtype=torch.int32, device=scores.device) if order else None
        out = self._det_metrics(scores, N, flags, N, S, perm)
        return (out, perm) if order else out

    def _det_launch(self, n_eval, ood_loader):
        """Behind the last evaluation batch: the out-of-distribution images through the same forward and columns, then one metrics
        call per question.  Returns the device tables (misclassification, OOD or None) and the number of OOD images."""
        d, S, n_ood = self._det, len(self.DETECT_COLUMNS), 0
        mis = self._det_metrics(d["scores"], d["cap"], d["flags"], n_eval, S) if n_eval else None
        if ood_loader is not None:
            self._in_ood = True
            for _, B in image_batches(self, ood_loader):
                self._det_reserve(B)
                for score, ev in self._score_eval:
                    score.eval_batch(B, None, ev)
                self._logits_into(B)
                self._ts_apply(B)
                self._det_rows(B, None)
            n_ood = d["n"] - n_eval
        ood = None
        if n_eval + n_ood and ood_loader is not None:
            is_ood = torch.zeros(d["cap"], dtype=torch.uint8, device=d["flags"].device)
            is_ood[n_eval:n_eval + n_ood] = 1
            ood = self._det_metrics(d["scores"], d["cap"], is_ood, n_eval + n_ood, S)
        return mis, ood, n_ood

    def _det_stats(self, mis, ood, n, n_wrong, n_ood, with_ood):
        """stats["detection"] from the two tables (read here: the evaluation's one synchronisation has happened with the losses)."""
        cols = list(self.DETECT_COLUMNS)
        nan = [float("nan")] * 4
        rows = mis.cpu().tolist() if mis is not None else [nan] * len(cols)
        out = {"columns": cols, "n": n, "n_wrong": n_wrong,
               "misclassification": {c: dict(zip(DETECT_KEYS, r[:4])) for c, r in zip(cols, rows)}}
        if with_ood:
            rows = ood.cpu().tolist() if ood is not None else [nan] * len(cols)
            out["ood"] = {c: dict(zip(DETECT_KEYS[:3], r[:3])) for c, r in zip(cols, rows)}
            out["n_ood"] = n_ood
        return out

    def _det_class_columns(self):
        """The columns of the head itself (LaplaceProbe: a LinearProbe's while it has no fit)."""
        return type(self).DETECT_COLUMNS

    def _det_refresh(self):
        """The instance's DETECT_COLUMNS: the head's own columns, followed by the columns of every feature-side score that has a state
        (MAHA_COLUMNS, then KNN_COLUMNS, then VIM_COLUMNS).  An instance attribute only where that differs from the class's."""
        cols = tuple(self._det_class_columns()) + tuple(c for score in self._scores if score.state is not None for c in score.columns)
        if cols == type(self).DETECT_COLUMNS:
            self.__dict__.pop("DETECT_COLUMNS", None)
        else:
            self.DETECT_COLUMNS = cols
