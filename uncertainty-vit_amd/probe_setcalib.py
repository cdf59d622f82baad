"""Set-level calibration for every probe head: ECE / MCE / OE with the reliability table, NLL, Brier, SCE, ACE, TACE and per-class
AUROC of the whole evaluation set, not means of per-batch values (csrc/setcalib.hip).  A mixin of
LinearProbe: the evaluation's device store of probabilities and labels, the one set-level call behind the last batch, and the same
on caller-supplied logits."""
import ctypes as C

import numpy as np
import torch

from . import native
from .native import check, cur_stream, lib, ptr
from .probe_util import grown, workspace

SCAL_MAX_N, SCAL_MAX_NK, SCAL_MAX_BINS = 1 << 20, 1 << 30, 64       # csrc/setcalib.hip: N <= 2^20 rows, N K <= 2^30, 1 .. 64 bins
SCAL_DEFAULTS = {"ece_bins": 15, "cw_bins": 15, "ace_bins": 15, "tace_bins": 30, "tace_threshold": 0.01}
SCAL_KEYS = ("ECE", "MCE", "OE", "NLL", "Brier", "SCE", "ACE", "TACE", "AUROC")      # out[0 .. 8] of uvit_op_scal_metrics
SCAL_CLASS_KEYS = ("SCE", "ACE", "TACE", "AUROC", "n_pos", "n_over_threshold")      # a row of per_class


def scal_settings(**kw):
    """The five settings, checked: every bin count in 1 .. 64, a threshold in [0, 1]."""
    unknown = set(kw) - set(SCAL_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown set-calibration setting(s): {sorted(unknown)}")
    s = {**SCAL_DEFAULTS, **{k: v for k, v in kw.items() if v is not None}}
    for k in ("ece_bins", "cw_bins", "ace_bins", "tace_bins"):
        if int(s[k]) != s[k] or not 1 <= int(s[k]) <= SCAL_MAX_BINS:
            raise native.UvitError(f"{k} must be an integer in [1, {SCAL_MAX_BINS}], got {s[k]}")
        s[k] = int(s[k])
    s["tace_threshold"] = float(s["tace_threshold"])
    if not 0.0 <= s["tace_threshold"] <= 1.0:
        raise native.UvitError(f"tace_threshold must be in [0, 1], got {s['tace_threshold']}")
    return s


class SetCalibrationMixin:
    def enable_set_calibration(self, ece_bins=15, cw_bins=15, ace_bins=15, tace_bins=30, tace_threshold=0.01):
        """From now on every evaluate() also stores each labelled batch's probabilities (behind the post-hoc temperature and a head's
        own link) and labels on the device and adds stats["set_calibration"], computed by one call behind the last batch."""
        self.set_set_calibration(scal_settings(ece_bins=ece_bins, cw_bins=cw_bins, ace_bins=ace_bins, tace_bins=tace_bins,
                                               tace_threshold=tace_threshold))

    def set_set_calibration(self, settings):
        """None switches the set-level calibration off: evaluate() then launches and returns exactly what it did before."""
        self._scal = None if settings is None else scal_settings(**settings)

    def _scal_reserve(self, B):
        """Room for B more rows in the evaluation's store: (cap, K) fp32 probabilities and one int64 label per row."""
        d, K = self._scal_eval, self.num_classes
        limit = min(SCAL_MAX_N, SCAL_MAX_NK // K)
        have = (d["probs"], d["labels"]) if d["cap"] else None
        specs = (((None, K), torch.float32, 0), ((None,), torch.int64, 0))
        out = grown(have, d["n"], d["n"] + B, limit,
                    f"set-level calibration holds at most {SCAL_MAX_N} rows and {SCAL_MAX_NK} probabilities, the loader holds more", specs,
                    self._arena.device)
        if out is not have:
            d.update(probs=out[0], labels=out[1], cap=out[1].shape[0])

    def _scal_rows(self, B, labels):
        """softmax(self._logits[:B]) and the labels into the store, behind the rows stored so far."""
        d, K = self._scal_eval, self.num_classes
        self._scal_reserve(B)
        at = C.c_void_p(d["probs"].data_ptr() + 4 * K * d["n"])
        check(lib().uvit_op_scal_probs(ptr(self._logits), at, K, B, K, cur_stream()), "uvit_op_scal_probs")
        d["labels"][d["n"]:d["n"] + B].copy_(labels)
        d["n"] += B

    def _scal_metrics(self, probs, ld, labels, N, s):
        """uvit_op_scal_metrics on the current stream: the device tables (out (16,), top_table (ece_bins, 3), per_class (K, 6))."""
        K, dev = self.num_classes, probs.device
        ws = workspace(self, "_scal_ws", dev, lib().uvit_op_scal_ws_bytes, N, K)
        out = torch.zeros(16, dtype=torch.float64, device=dev)
        top = torch.zeros(s["ece_bins"], 3, dtype=torch.float64, device=dev)
        per_class = torch.zeros(K, 6, dtype=torch.float64, device=dev)
        eb, cb = np.linspace(0, 1, s["ece_bins"] + 1), np.linspace(0, 1, s["cw_bins"] + 1)
        check(lib().uvit_op_scal_metrics(ptr(probs), int(ld), ptr(labels), N, K, eb.ctypes.data_as(C.c_void_p), s["ece_bins"],
                                         cb.ctypes.data_as(C.c_void_p), s["cw_bins"], s["ace_bins"], s["tace_bins"],
                                         C.c_double(s["tace_threshold"]), ptr(out), ptr(top), ptr(per_class), ptr(ws), ws.numel(),
                                         cur_stream()), "uvit_op_scal_metrics")
        return out, top, per_class

    def _scal_launch(self):
        """Behind the last evaluation batch: the one set-level call (None for an empty set)."""
        d = self._scal_eval
        return self._scal_metrics(d["probs"], self.num_classes, d["labels"], d["n"], self._scal) if d["n"] else None

    def _scal_stats(self, tables):
        """stats["set_calibration"] from the device tables (read here: the evaluation's one synchronisation has happened)."""
        if tables is None:
            nan = float("nan")
            return {**{k: nan for k in SCAL_KEYS}, "auroc_classes": 0, "acc": nan, "mean_conf": nan, "n": 0, "n_bad": 0,
                    "reliability": [], "per_class": {k: [] for k in SCAL_CLASS_KEYS}}
        out, top, per_class = (t.cpu() for t in tables)
        o = out.tolist()
        stats = dict(zip(SCAL_KEYS, o[:9]))
        stats.update(auroc_classes=int(o[9]), acc=o[10], mean_conf=o[11], n=int(o[12]), n_bad=int(o[13]), reliability=top.tolist(),
                     per_class={k: per_class[:, i].tolist() for i, k in enumerate(SCAL_CLASS_KEYS)})
        return stats

    def calibration_set(self, logits, labels, **bins):
        """The set-level calibration of caller-supplied GPU logits (N, K) fp32, N <= 2^20, N K <= 2^30, and int64 labels (N,):
        (out (16,), top_table (ece_bins, 3), per_class (K, 6)) as float64 device tensors in the layout of uvit_op_scal_metrics
        (include/uvit.h); nothing synchronises with the host.  `bins`: the settings of enable_set_calibration."""
        s = scal_settings(**bins)
        N = self._check_logits(logits, "N")
        labels = self._labels(labels, N)
        K = self.num_classes
        if not (1 <= N <= SCAL_MAX_N and N * K <= SCAL_MAX_NK):
            raise native.UvitError(f"set-level calibration takes 1 .. {SCAL_MAX_N} rows and at most {SCAL_MAX_NK} probabilities, got {N} x {K}")
        probs = torch.empty(N, K, dtype=torch.float32, device=logits.device)
        check(lib().uvit_op_scal_probs(ptr(logits), ptr(probs), K, N, K, cur_stream()), "uvit_op_scal_probs")
        return self._scal_metrics(probs, K, labels, N, s)
