"""Linear probe on the frozen encoder: the reference's `run_class_finetuning.py --linear_classifier`.

    frozen encoder (eval forward, native) -> mean of the last block's patch tokens -> LayerNorm without affine
    -> one nn.Linear -> (label-smoothing) cross-entropy          modeling_finetune.py:410-412,421,439-441,476-517

Only `head.weight` / `head.bias` train (run_class_finetuning.py:529-538: every weight the checkpoint provides is frozen).
Everything behind the last block runs as the HIP kernels of csrc/probe.hip on the stream of the encoder forward; the update is
uvit_op_adamw on the head's own flat arena [W (K C) | bias (K, padded to 4)] whose decay group (head.weight) comes first.  No gradient
ever reaches the encoder: its arenas and bf16 shadows are only read.  There is no eager fallback and no torch arithmetic on the
step path; the one torch call there is the 8-byte fill that clears the gradient sum-of-squares before uvit_op_sumsq adds to it.
"""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn

from . import native
from .modeling_cyclical import VisionTransformerForCyclicalTraining, _Holder, create_model
from .native import check, cur_stream, f32, lib, ptr

__all__ = ["LinearProbe", "build_probe_encoder", "load_encoder_checkpoint"]

CALIB_MAX_BINS = 64          # csrc/calib.hip: 1 <= n_bins <= 64, 1 <= B <= 1024
ECE_BINS, TACE_BINS, TACE_THRESHOLD = 15, 30, 0.01      # the reference's defaults (uncertainty_evaluations.py:200,243)
STABILITY_MAX_FRAMES = 256   # csrc/stability.hip: 2 <= F <= 256, 1 <= V <= 65535, 1 <= K <= 4096
DETECT_MAX_N, DETECT_MAX_S = 1 << 20, 16     # csrc/detect.hip: 1 <= N <= 2^20 samples, 1 <= S <= 16 columns
DETECT_KEYS = ("AUROC", "AUPR", "FPR95", "AURC")        # the first four entries of a row of uvit_op_detect_metrics' table
TS_MAX_N = 1 << 20           # csrc/tscale.hip: 1 <= N <= 2^20 calibration samples, K >= 2
TS_T_MIN, TS_T_MAX, TS_TOL, TS_MAX_ITER = 0.01, 100.0, 1e-7, 16
TS_STATUS = ("converged", "clamped at T_max", "clamped at T_min", "iteration limit")     # status 0 .. 3 of uvit_op_ts_fit
CP_MAX_N, CP_MAX_K, CP_MAX_A, CP_TABLE = 1 << 20, 4096, 8, 16      # csrc/conformal.hip: rows, classes, levels, doubles per table row
CP_KINDS = {"lac": 0, "aps": 1, "raps": 2}                         # the `kind` of uvit_op_cp_scores / uvit_op_cp_sets
MAHA_MAX_C, MAHA_MAX_K = 2048, 4096          # csrc/maha.hip: C % 4 == 0, 4 <= C <= 2048, 2 <= K <= 4096, 1 <= B <= 65535
MAHA_COLUMNS = ("maha", "rmaha")             # the detection columns a fitted density appends to the class's
MAHA_SHRINKAGE = 1e-3                        # an option's default, not a measured optimum
KNN_MAX_K, KNN_MAX_N, KNN_MAX_C = 256, 1 << 22, 2048       # csrc/knn.hip: 1 <= k <= 256, 1 <= N <= 2^22, C % 32 == 0, 32 <= C <= 2048
KNN_COLUMNS = ("knn",)                       # the detection column a neighbour bank appends behind the class's and MAHA_COLUMNS
KNN_K, KNN_TEMPERATURE = 20, 0.07            # the weighted k-NN classifier of DINO / iBOT


def _timm_trunc_normal_(t, std):
    """timm's trunc_normal_(t, std=std) as modeling_finetune.py:439 calls it: bounds a = -2, b = 2."""
    lo = (1.0 + math.erf(-2.0 / std / math.sqrt(2.0))) / 2.0
    hi = (1.0 + math.erf(2.0 / std / math.sqrt(2.0))) / 2.0
    with torch.no_grad():
        t.uniform_(2 * lo - 1, 2 * hi - 1).erfinv_().mul_(std * math.sqrt(2.0)).clamp_(-2.0, 2.0)
    return t


class LinearProbe(nn.Module):
    """`encoder`: a VisionTransformerForCyclicalTraining in .eval() (it is NOT a sub-module: state_dict() holds `head.weight`
    (K, C) and `head.bias` (K,), the reference's keys).  Owns the head, gradient and Adam moment arenas."""

    BETAS, EPS = (0.9, 0.999), 1e-8          # create_optimizer's adamw defaults (optim_factory.py:133-134)
    # per-sample uncertainty columns of evaluate(detection=True), larger = more uncertain: the three of uvit_op_detect_rows on the
    # logits; a head with an uncertainty of its own appends its columns
    DETECT_COLUMNS = ("msp", "entropy", "energy")

    def __init__(self, encoder, num_classes, smoothing=0.1, init_scale=0.001):
        super().__init__()
        if getattr(encoder, "_two_stream", False):
            raise NotImplementedError("the linear probe reads the base model; the two-stream (mean, covariance) model is not supported")
        if not isinstance(encoder, VisionTransformerForCyclicalTraining):
            raise TypeError("encoder must be a VisionTransformerForCyclicalTraining")
        if encoder.training:
            raise ValueError("the encoder is frozen: call encoder.eval() first (no dropout, no drop-path in the probe's forward)")
        K, Cd = int(num_classes), int(encoder.embed_dim)
        if K < 1:
            raise ValueError(f"num_classes must be >= 1, got {num_classes}")
        if not 0.0 <= float(smoothing) < 1.0:
            raise ValueError(f"smoothing must be in [0, 1), got {smoothing}")
        object.__setattr__(self, "encoder", encoder)
        self.num_classes, self.embed_dim, self.smoothing = K, Cd, float(smoothing)
        self._det, self._det_ws, self._in_ood = None, None, False
        # post-hoc temperature: host (T, s) of the fitted or set value, its device table, the table of the running evaluation, the
        # fit's workspace.  Plain attributes: state_dict() does not see them
        self._ts, self._ts_table, self._ts_on, self._ts_ws = None, None, None, None
        # conformal sets: the fitted or set state (settings and the device table of uvit_op_cp_quantile) and the quantile's workspace
        self._cp, self._cp_ws = None, None
        # feature density (Mahalanobis scores): the fitted or loaded state and the largest batch its buffers hold
        self._maha, self._maha_batch, self._maha_eval = None, 0, None
        # neighbour bank (k-NN score and classifier): the fitted or loaded state and the largest batch its buffers hold
        self._knn, self._knn_batch, self._knn_eval = None, 0, None
        self._setup_head(init_scale)
        self._buf_batch = self._calib_batch = self._rank_rows = self._seq_rows = 0

    # ---- arena plumbing (as the encoder's) ----
    def _setup_head(self, init_scale):
        """The head's flat arenas, its parameters as views of them, and their initial values (a subclass lays out another head)."""
        K, Cd = self.num_classes, self.embed_dim
        self._n_decay = K * Cd
        n = K * Cd + (K + 3) // 4 * 4
        dev = self.encoder._arena.device
        self._arena = torch.zeros(n, dtype=torch.float32, device=dev)
        self._grad_arena = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_count = 0
        self.head = _Holder()
        self.head.register_parameter("weight", nn.Parameter(self._arena[:K * Cd].view(K, Cd)))
        self.head.register_parameter("bias", nn.Parameter(self._arena[K * Cd:K * Cd + K]))
        self._rebind()
        _timm_trunc_normal_(self.head.weight.data, std=0.02).mul_(init_scale)     # modeling_finetune.py:439-441
        self.head.bias.data.zero_()                                               # constant 0 times init_scale

    def _rebind(self):
        K, Cd = self.num_classes, self.embed_dim
        for p, lo, hi, shape in ((self.head.weight, 0, K * Cd, (K, Cd)), (self.head.bias, K * Cd, K * Cd + K, (K,))):
            p.data = self._arena[lo:hi].view(shape)
            p.grad = self._grad_arena[lo:hi].view(shape)

    def _apply(self, fn, recurse=True):
        new = fn(self._arena)
        if new.dtype != torch.float32:
            raise NotImplementedError("the head stays fp32")
        self._arena = new.contiguous()
        self._grad_arena, self.exp_avg, self.exp_avg_sq = (fn(t).contiguous() for t in (self._grad_arena, self.exp_avg, self.exp_avg_sq))
        self._buf_batch = self._calib_batch = self._rank_rows = self._seq_rows = 0
        self._det_ws = self._ts_table = self._ts_ws = self._cp = self._cp_ws = None
        self._maha_batch = 0
        if self._maha is not None:                   # the density moves with the module and stays float64; its sums stay on the host
            for key in ("W", "W0", "Wmu", "Wmu0", "count_dev"):
                self._maha[key] = self._maha[key].to(new.device)
        self._knn_batch = 0
        if self._knn is not None:                    # the bank moves with the module and stays bf16
            for key in ("bank", "labels"):
                self._knn[key] = self._knn[key].to(new.device)
        self._rebind()
        return self

    def _buffers_for(self, B, calibration=False):
        """Caller-allocated device buffers of the probe's launches, grown to the largest batch seen; with `calibration`, those of the
        calibration ops (csrc/calib.hip) as well."""
        dev = self._arena.device
        if dev.type != "cuda":
            raise native.UvitError("the linear probe runs as HIP kernels: move the encoder and the probe to a GPU (no CPU fallback)")
        if B > self._buf_batch:
            K, Cd, N = self.num_classes, self.embed_dim, self.encoder.patch_embed.num_patches + 1
            ws = lib().uvit_op_probe_pool_ws_bytes(B, N, Cd)
            if ws < 0:
                check(int(ws), "uvit_op_probe_pool_ws_bytes")
            z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
            self._scratch, self._feat, self._logits, self._dlogits = z(ws // 4), z(B, Cd), z(B, K), z(B, K)
            self._row_loss = z(B)
            self._stats = z(2)                       # {loss, grad norm} of the last train_step
            self._sumsq = z(1, dt=torch.float64)
            self._buf_batch = B
        if calibration and B > self._calib_batch:
            K = self.num_classes
            z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
            self._probs, self._row_conf = z(B, K, dt=torch.float32), z(B, dt=torch.float32)
            self._row_pred, self._auroc_rows = z(2 * B, dt=torch.int32), z(3 * B, dt=torch.int32)
            self._row_nll, self._bin_table, self._per_class = z(B), z(3 * CALIB_MAX_BINS), z(K)
            self._calib_out = z(5)                   # {ECE, NLL, TACE, AUROC sum, AUROC class count} of the last calibration_batch
            self._calib_batch = B
        return self._buf_batch

    # ---- forward ----
    def _check_images(self, images):
        if not torch.is_tensor(images) or not images.is_cuda:
            raise native.UvitError("the linear probe needs GPU tensors: the HIP path has no CPU fallback")
        if self.encoder.training:
            raise native.UvitError("the encoder left eval mode: the probe reads a frozen, dropout-free forward")

    def _features(self, images):
        """Encoder eval forward, then pool + norm into self._feat[:B] on the current stream; returns B."""
        self._check_images(images)
        B = images.shape[0]
        self._buffers_for(B)
        enc = self.encoder
        e = enc.forward_features(images, bool_masked_pos=None, layer_results=None)
        x = lib().uvit_engine_ws_ptr(e.h, b"x", enc.depth)
        if not x:
            raise native.UvitError("no residual stream of the last block in the engine workspace")
        N = enc.patch_embed.num_patches + 1
        check(lib().uvit_op_probe_pool_norm(C.c_void_p(x), ptr(self._feat), ptr(self._scratch), B, N, self.embed_dim, f32(enc.ln_eps),
                                            cur_stream()), "uvit_op_probe_pool_norm")
        return B

    def _logits_into(self, B):
        K, Cd = self.num_classes, self.embed_dim
        check(lib().uvit_op_probe_logits(ptr(self._feat), ptr(self._arena), C.c_void_p(self._arena.data_ptr() + 4 * K * Cd),
                                         ptr(self._logits), B, K, Cd, cur_stream()), "uvit_op_probe_logits")

    def features(self, images):
        """(B, C) fp32: fc_norm(x[:, 1:].mean(1)) of the last block (modeling_finetune.py:512-515)."""
        B = self._features(images)
        return self._feat[:B].clone()

    def logits(self, images):
        B = self._features(images)
        self._logits_into(B)
        return self._logits[:B].clone()

    forward = logits

    def _labels(self, labels, B):
        if not torch.is_tensor(labels) or not labels.is_cuda:
            raise native.UvitError("labels must be a GPU tensor: the HIP path has no CPU fallback")
        if labels.dtype != torch.int64 or labels.shape != (B,) or not labels.is_contiguous():
            raise native.UvitError(f"labels must be a contiguous int64 tensor of shape ({B},)")
        return labels

    # ---- training ----
    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        """One step on the head: forward, smoothed cross-entropy, head gradients, global-norm clip (max_norm) + AdamW.  Returns
        (loss, grad_norm) as device scalars, valid until the next step; nothing synchronises with the host.  A non-finite loss
        (an out-of-range label) makes the gradients non-finite and uvit_op_adamw then leaves the head untouched.  `step_count`
        (Adam's bias correction) counts calls: the host cannot know of a skipped update without reading the loss, so a caller that
        sees a non-finite loss stops, as the reference and run_linear_probe.py do, or takes the call back with `step_count -= 1`."""
        B = self._features(images)
        labels = self._labels(labels, B)
        K, Cd, L, s = self.num_classes, self.embed_dim, lib(), cur_stream()
        self._logits_into(B)
        check(L.uvit_op_probe_ce(ptr(self._logits), ptr(labels), f32(self.smoothing), ptr(self._dlogits), ptr(self._row_loss),
                                 ptr(self._stats), None, B, K, s), "uvit_op_probe_ce")
        check(L.uvit_op_probe_head_grad(ptr(self._dlogits), ptr(self._feat), ptr(self._grad_arena),
                                        C.c_void_p(self._grad_arena.data_ptr() + 4 * K * Cd), B, K, Cd, s), "uvit_op_probe_head_grad")
        return self._clip_and_update(lr, weight_decay, max_norm)

    def _clip_and_update(self, lr, weight_decay, max_norm):
        """Global-norm clip + AdamW of the head arena from the gradient arena; returns (loss, grad_norm) of self._stats."""
        L, s, n = lib(), cur_stream(), self._arena.numel()
        self._sumsq.zero_()
        check(L.uvit_op_sumsq(ptr(self._grad_arena), n, ptr(self._sumsq), s), "uvit_op_sumsq")
        self.step_count += 1
        check(L.uvit_op_adamw(ptr(self._arena), ptr(self._grad_arena), ptr(self.exp_avg), ptr(self.exp_avg_sq), None, n, self._n_decay,
                              f32(lr), f32(weight_decay), f32(self.BETAS[0]), f32(self.BETAS[1]), f32(self.EPS), self.step_count,
                              ptr(self._sumsq), f32(max_norm if max_norm is not None and max_norm > 0 else 0.0), f32(1.0),
                              C.c_void_p(self._stats.data_ptr() + 4), s), "uvit_op_adamw")
        return self._stats[0], self._stats[1]

    # ---- calibration ----
    def _calibration_into(self, logits, labels, B, out, ece_bins=ECE_BINS, tace_bins=TACE_BINS, tace_threshold=TACE_THRESHOLD,
                          reference_bin_accuracy=True):
        """Softmax plus the three metric ops of csrc/calib.hip on `logits` (B, K) on the current stream; `out` is a device pointer to
        five doubles: ECE, NLL, TACE, AUROC sum over the classes counted, number of classes counted."""
        K, L, s = self.num_classes, lib(), cur_stream()
        if not 1 <= int(ece_bins) <= CALIB_MAX_BINS:
            raise native.UvitError(f"ece_bins must be in [1, {CALIB_MAX_BINS}], got {ece_bins}")
        bounds = np.linspace(0, 1, int(ece_bins) + 1)            # the reference's bin edges, bit for bit (uncertainty_evaluations.py:116)
        at = lambda i: C.c_void_p(out + 8 * i)                   # noqa: E731
        pos = 1 if reference_bin_accuracy else 0
        check(L.uvit_op_calib_softmax(ptr(logits), ptr(self._probs), B, K, s), "uvit_op_calib_softmax")
        check(L.uvit_op_calib_confidence(ptr(self._probs), ptr(labels), bounds.ctypes.data_as(C.c_void_p), int(ece_bins), pos,
                                         ptr(self._row_conf), ptr(self._row_pred), ptr(self._row_nll), ptr(self._bin_table), at(0), B, K,
                                         s), "uvit_op_calib_confidence")
        check(L.uvit_op_calib_tace(ptr(self._probs), ptr(labels), C.c_double(float(tace_threshold)), int(tace_bins), pos, ptr(self._per_class),
                                   at(2), B, K, s), "uvit_op_calib_tace")
        check(L.uvit_op_calib_auroc(ptr(self._probs), ptr(labels), ptr(self._auroc_rows), at(3), B, K, s), "uvit_op_calib_auroc")

    def calibration_batch(self, logits, labels, ece_bins=ECE_BINS, tace_bins=TACE_BINS, tace_threshold=TACE_THRESHOLD,
                          reference_bin_accuracy=True):
        """The reference's four per-batch calibration numbers (engine_for_finetuning.py:199-204) of caller-supplied GPU logits (B, K)
        fp32, B <= 1024: (ECE, TACE, NLL, AUROC) as float64 device scalars, valid until the next call; nothing synchronises with the
        host.  AUROC is the one-vs-rest mean over the classes with a positive and a negative row in the batch (NaN when there is
        none); a label outside [0, K) makes all four NaN.  `reference_bin_accuracy`: ECE and TACE as the reference's classes return them,
        whose bin accuracy indexes rows 0 and 1 of the batch by position (include/uvit.h, positional_acc); False
        gives the mean over the rows of each bin, the textbook ECE / TACE.  The bin table, the per-class TACE values and the per-row outputs of the
        ops stay in self._bin_table, self._per_class, self._row_conf, self._row_pred, self._auroc_rows, the sum and count of the
        AUROC in self._calib_out[3:5]."""
        if not torch.is_tensor(logits) or not logits.is_cuda:
            raise native.UvitError("logits must be a GPU tensor: the HIP path has no CPU fallback")
        if logits.dtype != torch.float32 or logits.ndim != 2 or logits.shape[1] != self.num_classes or not logits.is_contiguous():
            raise native.UvitError(f"logits must be a contiguous float32 tensor of shape (B, {self.num_classes})")
        B = logits.shape[0]
        labels = self._labels(labels, B)
        self._buffers_for(B, calibration=True)
        self._calibration_into(logits, labels, B, self._calib_out.data_ptr(), ece_bins, tace_bins, tace_threshold, reference_bin_accuracy)
        o = self._calib_out
        return o[0], o[2], o[1], o[3] / o[4]

    # ---- detection: does an uncertainty column rank the wrong predictions, or another data set's images, above the rest? ----
    def _det_reserve(self, B):
        """Room for B more samples in the evaluation's store: S fp32 columns of `cap` elements and one uint8 flag per sample, grown
        geometrically (what is there is copied on the device)."""
        d = self._det
        need = d["n"] + B
        if need > DETECT_MAX_N:
            raise native.UvitError(f"detection ranks at most {DETECT_MAX_N} samples, the loaders hold more")
        if need > d["cap"]:
            cap, dev = min(DETECT_MAX_N, max(need, 2 * d["cap"], 1024)), self._arena.device
            scores = torch.zeros(len(self.DETECT_COLUMNS), cap, dtype=torch.float32, device=dev)
            flags = torch.zeros(cap, dtype=torch.uint8, device=dev)
            if d["n"]:
                scores[:, :d["n"]].copy_(d["scores"][:, :d["n"]])
                flags[:d["n"]].copy_(d["flags"][:d["n"]])
            d.update(scores=scores, flags=flags, cap=cap)

    def _det_column(self, name, src, B):
        """A head's own column of the current batch -- `src` holds one float or double per row, any row stride -- into the store as
        fp32, behind the samples stored so far."""
        d = self._det
        at = d["scores"].data_ptr() + 4 * (self.DETECT_COLUMNS.index(name) * d["cap"] + d["n"])
        check(lib().uvit_op_detect_column(ptr(src), int(src.dtype == torch.float64), src.stride(0) if B > 1 else 1, C.c_void_p(at), B,
                                          cur_stream()), "uvit_op_detect_column")

    def _det_rows(self, B, labels):
        """The three scores of self._logits[:B] and, with labels, the wrong-prediction flags into the store; the batch is then stored."""
        d = self._det
        check(lib().uvit_op_detect_rows(ptr(self._logits), ptr(labels), ptr(d["scores"]), d["cap"], d["n"], ptr(d["flags"]), B,
                                        self.num_classes, cur_stream()), "uvit_op_detect_rows")
        d["n"] += B

    def _det_metrics(self, scores, ld, flags, N, S, order=None):
        """uvit_op_detect_metrics on the current stream: the (S, 8) float64 device table."""
        ws = lib().uvit_op_detect_ws_bytes(N, S)
        if ws < 0:
            check(int(ws), "uvit_op_detect_ws_bytes")
        if self._det_ws is None or self._det_ws.numel() < ws:
            self._det_ws = torch.empty(int(ws), dtype=torch.uint8, device=scores.device)
        out = torch.zeros(S, 8, dtype=torch.float64, device=scores.device)
        check(lib().uvit_op_detect_metrics(ptr(scores), int(ld), ptr(flags), N, S, ptr(order), ptr(out), ptr(self._det_ws),
                                           self._det_ws.numel(), cur_stream()), "uvit_op_detect_metrics")
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
            for item in ood_loader:
                images = item
                while isinstance(images, (tuple, list)):
                    images = images[0]
                B = self._features(images)
                self._det_reserve(B)
                if self._maha_eval is not None:
                    self._maha_columns(B, None)
                if self._knn_eval is not None:
                    self._knn_columns(B, None)
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

    # ---- feature density: Mahalanobis and relative Mahalanobis scores (csrc/maha.hip) ----
    def _det_class_columns(self):
        """The columns of the head itself (LaplaceProbe: a LinearProbe's while it has no fit)."""
        return type(self).DETECT_COLUMNS

    def _det_refresh(self):
        """The instance's DETECT_COLUMNS: the head's own columns, followed by MAHA_COLUMNS while a density is set and by KNN_COLUMNS
        while a neighbour bank is set.  An instance attribute only where that differs from the class's."""
        cols = tuple(self._det_class_columns()) + (MAHA_COLUMNS if self._maha is not None else ()) + \
            (KNN_COLUMNS if self._knn is not None else ())
        if cols == type(self).DETECT_COLUMNS:
            self.__dict__.pop("DETECT_COLUMNS", None)
        else:
            self.DETECT_COLUMNS = cols

    @staticmethod
    def _maha_shrinkage(shrinkage):
        rho = float(shrinkage)
        if not 0.0 < rho < math.inf:
            raise native.UvitError(f"the shrinkage must be positive and finite, got {shrinkage}")
        return rho

    def _maha_install(self, S, class_sum, total_sum, class_count, sums, shrinkage):
        """Host float64 sums -> the two shrunk covariances, their Cholesky factors, the whitened means and the uploads."""
        rho = self._maha_shrinkage(shrinkage)
        K, Cd, F64 = self.num_classes, self.embed_dim, torch.float64
        if Cd < 4 or Cd % 4 or Cd > MAHA_MAX_C or not 2 <= K <= MAHA_MAX_K:
            raise native.UvitError(f"the Mahalanobis ops take an embed dim that is a multiple of 4 in [4, {MAHA_MAX_C}] and 2 .. {MAHA_MAX_K} "
                                   f"classes, got {Cd} and {K}")
        S, class_sum, total_sum, class_count, sums = (torch.as_tensor(t, dtype=F64).cpu().contiguous()
                                                      for t in (S, class_sum, total_sum, class_count, sums))
        if (tuple(S.shape), tuple(class_sum.shape), tuple(total_sum.shape), tuple(class_count.shape), tuple(sums.shape)) != \
                ((Cd, Cd), (K, Cd), (Cd,), (K,), (2,)):
            raise native.UvitError(f"the density state belongs to another probe: its sums must have shapes ({Cd}, {Cd}), ({K}, {Cd}), "
                                   f"({Cd},), ({K},) and (2,)")
        n, skipped = float(sums[0]), float(sums[1])
        if not n >= 2:
            raise native.UvitError("the density fit needs at least two usable rows (finite features, a label inside [0, K))")
        mu = class_sum / class_count.clamp_min(1.0)[:, None]                 # an empty class: a zero row, never chosen
        mu0 = total_sum / n
        sigma = (S - class_sum.T @ mu) / n                                   # sum_k n_k mu_k mu_k^T = class_sum^T mu
        sigma = 0.5 * (sigma + sigma.T)
        sigma0 = S / n - torch.outer(mu0, mu0)
        eye = torch.eye(Cd, dtype=F64)
        fac = []
        for m in (sigma, sigma0):
            reg = m + rho * (float(torch.trace(m)) / Cd) * eye
            L, info = torch.linalg.cholesky_ex(reg)
            if int(info) != 0 or not bool(torch.isfinite(L).all()):
                raise native.UvitError("the density fit failed: a shrunk covariance is not positive definite (constant or non-finite "
                                       "features?); try a larger shrinkage")
            fac.append((torch.linalg.solve_triangular(L, eye, upper=False).tril(), 2.0 * float(torch.log(torch.diagonal(L)).sum())))
        (W, logdet), (W0, logdet0) = fac
        dev = self._arena.device
        up = lambda t: t.contiguous().to(dev)                                # noqa: E731
        self._maha = {"S": S, "class_sum": class_sum, "total_sum": total_sum, "class_count": class_count, "sums": sums,
                      "W": up(W), "W0": up(W0), "Wmu": up(mu @ W.T), "Wmu0": up(W0 @ mu0), "count_dev": up(class_count),
                      "info": {"n": int(n), "skipped": int(skipped), "classes": K, "empty_classes": int((class_count <= 0).sum()),
                               "shrinkage": rho, "logdet": logdet, "logdet0": logdet0}}
        self._det_refresh()
        return dict(self._maha["info"])

    def fit_density(self, loader, shrinkage=MAHA_SHRINKAGE):
        """Class-conditional Gaussians with one tied covariance, and one background Gaussian, on the probe's features: one pass over a
        labelled loader (items as evaluate()'s) of the encoder forward, pool + norm and uvit_op_maha_accumulate into device
        accumulators, one read of the sums, then the host's two covariances, their shrinkage Sigma + shrinkage tr(Sigma) / C I and
        Cholesky factors in float64 (torch.linalg on the CPU) and the upload of W = L^-1, W0 = L0^-1 and the whitened means.  The head
        takes no part: any trained or untrained head gets the columns.  Returns {n, skipped (rows with a non-finite feature or a label
        outside [0, K)), classes, empty_classes, shrinkage, logdet, logdet0 (log-determinants of the two shrunk covariances)}."""
        rho = self._maha_shrinkage(shrinkage)
        K, Cd, acc, ws = self.num_classes, self.embed_dim, None, None
        o_cs, o_ts, o_cc, o_sums = Cd * Cd, Cd * Cd + K * Cd, Cd * Cd + K * Cd + Cd, Cd * Cd + K * Cd + Cd + K
        for item in loader:
            images, labels = item
            if isinstance(images, (tuple, list)):
                images = images[0]
            B = self._features(images)
            if torch.is_tensor(labels) and not labels.is_cuda:
                labels = labels.to(images.device, non_blocking=True)
            labels = self._labels(labels, B)
            if acc is None:
                acc = torch.zeros(o_sums + 2, dtype=torch.float64, device=images.device)     # S | class sums | total | counts | sums
            need = lib().uvit_op_maha_accumulate_ws_bytes(B, Cd, K)
            if need < 0:
                check(int(need), "uvit_op_maha_accumulate_ws_bytes")
            if ws is None or ws.numel() < need:
                ws = torch.empty(int(need), dtype=torch.uint8, device=images.device)
            at = lambda off: C.c_void_p(acc.data_ptr() + 8 * off)                             # noqa: E731
            check(lib().uvit_op_maha_accumulate(ptr(self._feat), ptr(labels), at(0), at(o_cs), at(o_ts), at(o_cc), at(o_sums), ptr(ws),
                                                ws.numel(), B, Cd, K, cur_stream()), "uvit_op_maha_accumulate")
        if acc is None:
            raise native.UvitError("the density fit needs at least two labelled samples")
        host = acc.cpu()                                                                      # the one read
        return self._maha_install(host[:o_cs].view(Cd, Cd), host[o_cs:o_ts].view(K, Cd), host[o_ts:o_cc], host[o_cc:o_sums],
                                  host[o_sums:o_sums + 2], rho)

    def set_density(self, state):
        """None forgets the density (the detection columns are the class's again); a dict of density_state_dict() is loaded."""
        if state is not None:
            return self.load_density_state(state)
        self._maha = None
        self._det_refresh()

    @property
    def density(self):
        """{n, skipped, classes, empty_classes, shrinkage, logdet, logdet0} of the density in use, None when there is none."""
        return dict(self._maha["info"]) if self._maha is not None else None

    def set_density_shrinkage(self, shrinkage):
        """Another shrinkage for the density in use: the host factorises again from the kept sums, the data are not read."""
        st = self._maha
        if st is None:
            raise native.UvitError("set_density_shrinkage needs fit_density() or load_density_state() first")
        return self._maha_install(st["S"], st["class_sum"], st["total_sum"], st["class_count"], st["sums"], shrinkage)

    def density_state_dict(self):
        """What a density is made of, on the host: the float64 sums S, class_sum, total_sum, class_count, sums = {rows used, rows
        skipped} and the shrinkage.  Not part of state_dict(): neither a parameter nor a buffer."""
        st = self._maha
        if st is None:
            raise native.UvitError("density_state_dict needs fit_density() or load_density_state() first")
        return {**{k: st[k].clone() for k in ("S", "class_sum", "total_sum", "class_count", "sums")}, "shrinkage": st["info"]["shrinkage"]}

    def load_density_state(self, sd):
        """Install a saved density (density_state_dict()); one of another embed dim or class count is refused."""
        keys = ("S", "class_sum", "total_sum", "class_count", "sums", "shrinkage")
        if not (isinstance(sd, dict) and set(keys) <= set(sd)):
            raise native.UvitError("load_density_state takes a dict of density_state_dict()")
        return self._maha_install(*(sd[k] for k in keys))

    def _maha_buffers_for(self, B):
        if B > self._maha_batch:
            dev = self._arena.device
            ws = lib().uvit_op_maha_scores_ws_bytes(B, self.embed_dim, self.num_classes)
            if ws < 0:
                check(int(ws), "uvit_op_maha_scores_ws_bytes")
            self._maha_ws = torch.empty(int(ws), dtype=torch.uint8, device=dev)
            self._maha_col, self._rmaha_col = (torch.zeros(B, dtype=torch.float32, device=dev) for _ in range(2))
            self._maha_pred = torch.zeros(B, dtype=torch.int32, device=dev)
            self._maha_batch = B
        if self._maha_ws.device != self._maha["W"].device:
            raise native.UvitError("the density and the probe are on different devices")

    def _maha_into(self, feat, B, dist=None, labels=None, correct=None):
        """uvit_op_maha_scores of feat[:B] on the current stream into self._maha_col, self._rmaha_col and self._maha_pred."""
        st = self._maha
        if st is None:
            raise native.UvitError("the Mahalanobis scores need fit_density() or load_density_state() first")
        if self._arena.device.type != "cuda":
            raise native.UvitError("the Mahalanobis scores run as HIP kernels: move the encoder and the probe to a GPU (no CPU fallback)")
        self._maha_buffers_for(B)
        K = self.num_classes
        check(lib().uvit_op_maha_scores(ptr(feat), ptr(st["W"]), ptr(st["W0"]), ptr(st["Wmu"]), ptr(st["Wmu0"]), ptr(st["count_dev"]),
                                        ptr(self._maha_col), ptr(self._rmaha_col), ptr(self._maha_pred), ptr(dist), K, ptr(labels),
                                        ptr(correct), ptr(self._maha_ws), self._maha_ws.numel(), B, self.embed_dim, K, cur_stream()),
              "uvit_op_maha_scores")

    def _maha_result(self, feat, B, distances):
        dist = torch.zeros(B, self.num_classes, dtype=torch.float64, device=feat.device) if distances else None
        self._maha_into(feat, B, dist)
        out = {"maha": self._maha_col[:B].clone(), "rmaha": self._rmaha_col[:B].clone(), "pred": self._maha_pred[:B].clone()}
        if distances:
            out["dist"] = dist
        return out

    def feature_scores(self, images, distances=False):
        """{"maha", "rmaha" (B) fp32, "pred" (B) int32} of the images' features against the density in use, device tensors; with
        `distances`, also "dist" (B, K) float64, the squared distance to every class mean.  maha = the smallest squared Mahalanobis
        distance to a class mean under the tied covariance, pred = that class (the nearest class mean), rmaha = maha minus the squared
        distance to the background Gaussian; larger = more out of distribution.  A row with a non-finite feature: NaN, NaN, -1."""
        if self._maha is None:
            raise native.UvitError("feature_scores needs fit_density() or load_density_state() first")
        B = self._features(images)
        return self._maha_result(self._feat, B, distances)

    def density_batch(self, feat, distances=False):
        """feature_scores() of caller-supplied GPU features (B, C) fp32; nothing synchronises with the host."""
        if not torch.is_tensor(feat) or not feat.is_cuda:
            raise native.UvitError("feat must be a GPU tensor: the HIP path has no CPU fallback")
        if feat.dtype != torch.float32 or feat.ndim != 2 or feat.shape[1] != self.embed_dim or not feat.is_contiguous() or not feat.shape[0]:
            raise native.UvitError(f"feat must be a contiguous float32 tensor of shape (B, {self.embed_dim})")
        return self._maha_result(feat, feat.shape[0], distances)

    def _maha_columns(self, B, labels):
        """Inside evaluate(detection=True) with a density: the two columns of self._feat[:B] into the store (behind _det_reserve, in
        front of _det_rows).  The evaluation set's rows (labels given) are also counted against their labels and kept for the mean."""
        ev = self._maha_eval
        self._maha_into(self._feat, B, None, labels, ev["correct"] if labels is not None else None)
        self._det_column("maha", self._maha_col, B)
        self._det_column("rmaha", self._rmaha_col, B)
        if labels is not None:
            ev["slabs"].append(self._maha_col[:B].clone())

    # ---- neighbour bank: k-NN OOD score and weighted k-NN classifier (csrc/knn.hip) ----
    @staticmethod
    def _knn_settings(k, temperature):
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= KNN_MAX_K:
            raise native.UvitError(f"k must be a whole number in [1, {KNN_MAX_K}], got {k}")
        T = float(temperature)
        if not 0.0 < T < math.inf:
            raise native.UvitError(f"the k-NN temperature must be positive and finite, got {temperature}")
        return int(k), T

    def _knn_check_dims(self):
        K, Cd = self.num_classes, self.embed_dim
        if Cd < 32 or Cd % 32 or Cd > KNN_MAX_C or not 2 <= K <= MAHA_MAX_K:
            raise native.UvitError(f"the k-NN ops take an embed dim that is a multiple of 32 in [32, {KNN_MAX_C}] and 2 .. {MAHA_MAX_K} "
                                   f"classes, got {Cd} and {K}")

    def _knn_install(self, bank, labels, sums, k, temperature, own=False):
        """A bank of unit bf16 rows (n, C), their int32 labels (-1: a skipped row) and sums = {rows used, rows skipped} become the
        state in use, on the probe's device (`own`: written by fit_neighbours just now, the labels need no look)."""
        k, T = self._knn_settings(k, temperature)
        self._knn_check_dims()
        K, Cd = self.num_classes, self.embed_dim
        if not (torch.is_tensor(bank) and torch.is_tensor(labels)) or bank.dtype != torch.bfloat16 or labels.dtype != torch.int32:
            raise native.UvitError("the neighbour state holds a bfloat16 bank and int32 labels")
        if bank.ndim != 2 or bank.shape[1] != Cd or tuple(labels.shape) != (bank.shape[0],) or not 1 <= bank.shape[0] <= KNN_MAX_N:
            raise native.UvitError(f"the neighbour state belongs to another probe: its bank must have shape (n, {Cd}) with 1 <= n <= "
                                   f"{KNN_MAX_N} and one label per row")
        sums = torch.as_tensor(sums, dtype=torch.float64).cpu().contiguous()
        if tuple(sums.shape) != (2,):
            raise native.UvitError("the neighbour state's sums must be {rows used, rows skipped}")
        if not own and (int(labels.max()) >= K or int(labels.min()) < -1):
            raise native.UvitError(f"the neighbour state belongs to another probe: its labels must lie in [-1, {K})")
        n, skipped = int(sums[0]), int(sums[1])
        if n < k:
            raise native.UvitError(f"the neighbour bank holds {n} usable rows (finite features, a label inside [0, K)), fewer than k = {k}")
        dev = self._arena.device
        self._knn = {"bank": bank.contiguous().to(dev), "labels": labels.contiguous().to(dev), "sums": sums,
                     "info": {"n": n, "skipped": skipped, "classes": K, "k": k, "temperature": T}}
        self._knn_batch = 0
        self._det_refresh()
        return dict(self._knn["info"])

    def fit_neighbours(self, loader, k=KNN_K, temperature=KNN_TEMPERATURE):
        """A bank of the training features for nearest-neighbour search: one pass over a labelled loader (items as evaluate()'s) of
        the encoder forward, pool + norm and uvit_op_knn_rows, which appends the batch's unit bf16 rows and int32 labels to a device
        bank (allocated once when the loader's data set has a length, grown geometrically otherwise); the two counters are read once,
        at the end.  Nothing is trained and the head takes no part.  Returns {n (usable rows), skipped (rows with a non-finite
        feature, a zero norm or a label outside [0, K): kept as zero rows that are never a neighbour), classes, k, temperature};
        fewer usable rows than k are refused."""
        k, T = self._knn_settings(k, temperature)
        self._knn_check_dims()
        K, Cd = self.num_classes, self.embed_dim
        try:
            cap = min(KNN_MAX_N, max(0, len(loader.dataset)))
        except (AttributeError, TypeError):
            cap = 0
        bank = lab = sums = None
        n = 0
        for item in loader:
            images, labels = item
            if isinstance(images, (tuple, list)):
                images = images[0]
            B = self._features(images)
            if torch.is_tensor(labels) and not labels.is_cuda:
                labels = labels.to(images.device, non_blocking=True)
            labels = self._labels(labels, B)
            if n + B > KNN_MAX_N:
                raise native.UvitError(f"a neighbour bank holds at most {KNN_MAX_N} rows, the loader holds more")
            if bank is None or n + B > bank.shape[0]:
                cap = min(KNN_MAX_N, max(n + B, cap, 2 * (bank.shape[0] if bank is not None else 0), 1024))
                grown = torch.zeros(cap, Cd, dtype=torch.bfloat16, device=images.device)
                glab = torch.full((cap,), -1, dtype=torch.int32, device=images.device)
                if n:
                    grown[:n].copy_(bank[:n])
                    glab[:n].copy_(lab[:n])
                bank, lab = grown, glab
            if sums is None:
                sums = torch.zeros(2, dtype=torch.float64, device=images.device)
            check(lib().uvit_op_knn_rows(ptr(self._feat), ptr(labels), C.c_void_p(bank.data_ptr() + 2 * n * Cd),
                                         C.c_void_p(lab.data_ptr() + 4 * n), ptr(sums), B, Cd, K, cur_stream()), "uvit_op_knn_rows")
            n += B
        if bank is None:
            raise native.UvitError("the neighbour fit needs at least k labelled samples")
        return self._knn_install(bank[:n].clone(), lab[:n].clone(), sums.cpu(), k, T, own=True)  # the one read

    def set_neighbours(self, state):
        """None forgets the bank (the detection columns are what they were); a dict of neighbour_state_dict() is loaded."""
        if state is not None:
            return self.load_neighbour_state(state)
        self._knn, self._knn_batch = None, 0
        self._det_refresh()

    @property
    def neighbours(self):
        """{n, skipped, classes, k, temperature} of the bank in use, None when there is none."""
        return dict(self._knn["info"]) if self._knn is not None else None

    def set_neighbours_k(self, k, temperature=None):
        """Another k (and temperature) for the bank in use; the data are not read again."""
        st = self._knn
        if st is None:
            raise native.UvitError("set_neighbours_k needs fit_neighbours() or load_neighbour_state() first")
        k, T = self._knn_settings(k, st["info"]["temperature"] if temperature is None else temperature)
        if st["info"]["n"] < k:
            raise native.UvitError(f"the neighbour bank holds {st['info']['n']} usable rows, fewer than k = {k}")
        st["info"].update(k=k, temperature=T)
        self._knn_batch = 0
        return dict(st["info"])

    def neighbour_state_dict(self):
        """What a bank is made of, on the host: bank (n, C) bfloat16, labels (n) int32, sums = {rows used, rows skipped}, k and
        temperature.  Not part of state_dict(): neither a parameter nor a buffer."""
        st = self._knn
        if st is None:
            raise native.UvitError("neighbour_state_dict needs fit_neighbours() or load_neighbour_state() first")
        return {"bank": st["bank"].cpu().clone(), "labels": st["labels"].cpu().clone(), "sums": st["sums"].clone(), "k": st["info"]["k"],
                "temperature": st["info"]["temperature"]}

    def load_neighbour_state(self, sd):
        """Install a saved bank (neighbour_state_dict()); one of another embed dim or class count is refused."""
        keys = ("bank", "labels", "sums", "k", "temperature")
        if not (isinstance(sd, dict) and set(keys) <= set(sd)):
            raise native.UvitError("load_neighbour_state takes a dict of neighbour_state_dict()")
        return self._knn_install(*(sd[k] for k in keys))

    def _knn_buffers_for(self, B):
        st = self._knn
        k, n, Cd, dev = st["info"]["k"], st["bank"].shape[0], self.embed_dim, self._arena.device
        if st["bank"].device != dev:
            raise native.UvitError("the neighbour bank and the probe are on different devices")
        if B > self._knn_batch:
            self._knn_query = torch.zeros(B, Cd, dtype=torch.bfloat16, device=dev)
            self._knn_valid, self._knn_pred = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
            self._knn_sim = torch.zeros(B, k, dtype=torch.float32, device=dev)
            self._knn_idx = torch.zeros(B, k, dtype=torch.int32, device=dev)
            self._knn_col = torch.zeros(B, dtype=torch.float32, device=dev)
            self._knn_ws = torch.empty(0, dtype=torch.uint8, device=dev)
            self._knn_batch = B
        ws = lib().uvit_op_knn_search_ws_bytes(B, Cd, n, k, 0)
        if ws < 0:
            check(int(ws), "uvit_op_knn_search_ws_bytes")
        if self._knn_ws.numel() < ws:
            self._knn_ws = torch.empty(int(ws), dtype=torch.uint8, device=dev)

    def _knn_into(self, feat, B, labels=None, correct=None):
        """uvit_op_knn_rows, uvit_op_knn_search and uvit_op_knn_scores of feat[:B] on the current stream into self._knn_sim,
        self._knn_idx (B, k), self._knn_col and self._knn_pred."""
        st = self._knn
        if st is None:
            raise native.UvitError("the k-NN scores need fit_neighbours() or load_neighbour_state() first")
        if self._arena.device.type != "cuda":
            raise native.UvitError("the k-NN scores run as HIP kernels: move the encoder and the probe to a GPU (no CPU fallback)")
        self._knn_buffers_for(B)
        K, Cd, k, n = self.num_classes, self.embed_dim, st["info"]["k"], st["bank"].shape[0]
        s = cur_stream()
        check(lib().uvit_op_knn_rows(ptr(feat), None, ptr(self._knn_query), ptr(self._knn_valid), None, B, Cd, K, s), "uvit_op_knn_rows")
        check(lib().uvit_op_knn_search(ptr(self._knn_query), ptr(self._knn_valid), ptr(st["bank"]), ptr(st["labels"]), ptr(self._knn_sim),
                                       ptr(self._knn_idx), k, ptr(self._knn_ws), self._knn_ws.numel(), B, Cd, n, k, 0, s),
              "uvit_op_knn_search")
        check(lib().uvit_op_knn_scores(ptr(self._knn_sim), ptr(self._knn_idx), k, ptr(st["labels"]), n, ptr(self._knn_col),
                                       ptr(self._knn_pred), None, 0, ptr(labels), ptr(correct), B, k, K,
                                       C.c_double(st["info"]["temperature"]), s), "uvit_op_knn_scores")

    def _knn_result(self, feat, B, neighbours):
        self._knn_into(feat, B)
        out = {"knn": self._knn_col[:B].clone(), "pred": self._knn_pred[:B].clone()}
        if neighbours:
            out["sim"], out["idx"] = self._knn_sim[:B].clone(), self._knn_idx[:B].clone()
        return out

    def neighbour_scores(self, images, neighbours=False):
        """{"knn" (B) fp32, "pred" (B) int32} of the images' features against the bank in use, device tensors; with `neighbours`, also
        "sim" (B, k) fp32 and "idx" (B, k) int32, the k nearest bank rows by (similarity descending, index ascending).  knn = 2 - 2 s_k,
        the squared distance between the unit vectors to the k-th nearest bank row (larger = more out of distribution); pred = the
        class with the largest vote sum_j exp((s_j - s_1) / T) over the k neighbours.  A row with a non-finite feature: NaN, -1."""
        if self._knn is None:
            raise native.UvitError("neighbour_scores needs fit_neighbours() or load_neighbour_state() first")
        B = self._features(images)
        return self._knn_result(self._feat, B, neighbours)

    def neighbour_batch(self, feat, neighbours=False):
        """neighbour_scores() of caller-supplied GPU features (B, C) fp32; nothing synchronises with the host."""
        if not torch.is_tensor(feat) or not feat.is_cuda:
            raise native.UvitError("feat must be a GPU tensor: the HIP path has no CPU fallback")
        if feat.dtype != torch.float32 or feat.ndim != 2 or feat.shape[1] != self.embed_dim or not feat.is_contiguous() or not feat.shape[0]:
            raise native.UvitError(f"feat must be a contiguous float32 tensor of shape (B, {self.embed_dim})")
        return self._knn_result(feat, feat.shape[0], neighbours)

    def _knn_columns(self, B, labels):
        """Inside evaluate(detection=True) with a bank: the column of self._feat[:B] into the store (behind _maha_columns, in front of
        _det_rows).  The evaluation set's rows (labels given) are also counted against their labels and kept for the mean."""
        ev = self._knn_eval
        self._knn_into(self._feat, B, labels, ev["correct"] if labels is not None else None)
        self._det_column("knn", self._knn_col, B)
        if labels is not None:
            ev["slabs"].append(self._knn_col[:B].clone())

    # ---- post-hoc temperature scaling (csrc/tscale.hip) ----
    def _ts_fit(self, logits, ld, labels, N, t_min, t_max, tol, max_iter):
        """uvit_op_ts_fit on the current stream: the (8,) float64 device table."""
        K = self.num_classes
        ws = lib().uvit_op_ts_ws_bytes(N, K)
        if ws < 0:
            check(int(ws), "uvit_op_ts_ws_bytes")
        if self._ts_ws is None or self._ts_ws.numel() < ws or self._ts_ws.device != logits.device:
            self._ts_ws = torch.empty(int(ws), dtype=torch.uint8, device=logits.device)
        out = torch.zeros(8, dtype=torch.float64, device=logits.device)
        check(lib().uvit_op_ts_fit(ptr(logits), int(ld), ptr(labels), N, K, float(t_min), float(t_max), float(tol), int(max_iter), ptr(out),
                                   ptr(self._ts_ws), self._ts_ws.numel(), cur_stream()), "uvit_op_ts_fit")
        return out

    def temperature_batch(self, logits, labels, t_min=TS_T_MIN, t_max=TS_T_MAX, tol=TS_TOL, max_iter=TS_MAX_ITER):
        """The temperature T that minimises the mean NLL of softmax(logits / T) over caller-supplied GPU logits (N, K) fp32, N <= 2^20,
        with int64 labels (N,): the (8,) float64 device table {T, s = 1 / T, NLL at T = 1, NLL at T, dNLL/ds at s, passes used, status,
        rows left out} of uvit_op_ts_fit (include/uvit.h; status 0 converged, 1 clamped at t_max, 2 clamped at t_min, 3 max_iter passes
        used up).  Nothing synchronises with the host, and the probe's own temperature is not touched."""
        if not torch.is_tensor(logits) or not logits.is_cuda:
            raise native.UvitError("logits must be a GPU tensor: the HIP path has no CPU fallback")
        if logits.dtype != torch.float32 or logits.ndim != 2 or logits.shape[1] != self.num_classes or not logits.is_contiguous():
            raise native.UvitError(f"logits must be a contiguous float32 tensor of shape (N, {self.num_classes})")
        N = logits.shape[0]
        if not 1 <= N <= TS_MAX_N:
            raise native.UvitError(f"the temperature fit takes 1 .. {TS_MAX_N} samples, got {N}")
        return self._ts_fit(logits, self.num_classes, self._labels(labels, N), N, t_min, t_max, tol, max_iter)

    def fit_temperature(self, loader, t_min=TS_T_MIN, t_max=TS_T_MAX, tol=TS_TOL, max_iter=TS_MAX_ITER):
        """Fit the temperature on a calibration loader (items as evaluate()'s): every batch goes through the forward and the
        _logits_into of evaluate(), its logits and labels into a device store grown geometrically (at most 2^20 samples), then one
        uvit_op_ts_fit over the store.  The table stays on the device for evaluate(temperature=True) and is read once:
        {"T", "nll_before" (at T = 1), "nll_after", "grad" (dNLL/ds at the result), "iterations", "status", "n", "n_skipped" (rows with
        a non-finite logit)}.  The fit sees the combined logits of an ensemble and the logits a GP or heteroscedastic evaluation sees."""
        K, store, lab, n = self.num_classes, None, None, 0
        for item in loader:
            images, labels = item
            if isinstance(images, (tuple, list)):
                images = images[0]
            B = self._features(images)
            if torch.is_tensor(labels) and not labels.is_cuda:
                labels = labels.to(images.device, non_blocking=True)
            labels = self._labels(labels, B)
            if n + B > TS_MAX_N:
                raise native.UvitError(f"the temperature fit takes at most {TS_MAX_N} samples, the loader holds more")
            if store is None or n + B > store.shape[0]:
                cap = min(TS_MAX_N, max(n + B, 2 * (store.shape[0] if store is not None else 0), 1024))
                grown, glab = torch.zeros(cap, K, dtype=torch.float32, device=images.device), torch.zeros(cap, dtype=torch.int64, device=images.device)
                if n:
                    grown[:n].copy_(store[:n])
                    glab[:n].copy_(lab[:n])
                store, lab = grown, glab
            self._logits_into(B)
            store[n:n + B].copy_(self._logits[:B])
            lab[n:n + B].copy_(labels)
            n += B
        if not n:
            raise native.UvitError("the temperature fit needs at least one calibration sample")
        table = self._ts_fit(store, K, lab, n, t_min, t_max, tol, max_iter)
        t = table.cpu().tolist()                                                         # the one read
        self._ts, self._ts_table = (t[0], t[1]), table
        nan = math.isnan(t[6])
        return {"T": t[0], "nll_before": t[2], "nll_after": t[3], "grad": t[4], "iterations": -1 if nan else int(t[5]),
                "status": -1 if nan else int(t[6]), "n": n, "n_skipped": -1 if nan else int(t[7])}

    def set_temperature(self, T):
        """Use the temperature T (a positive finite number) in evaluate(temperature=True); None forgets it.  Not a parameter and not
        a buffer: state_dict() and the checkpoints keep their keys."""
        if T is None:
            self._ts = self._ts_table = None
            return
        T = float(T)
        if not 0.0 < T < math.inf:
            raise ValueError(f"the temperature must be positive and finite, got {T}")
        self._ts, self._ts_table = (T, 1.0 / T), None

    @property
    def post_hoc_temperature(self):
        """The fitted or set post-hoc temperature, None when there is none."""
        return self._ts[0] if self._ts is not None else None

    @property
    def temperature(self):
        """post_hoc_temperature (HetProbe keeps its own `temperature`, the softmax temperature of the Monte-Carlo samples: read
        `post_hoc_temperature` there)."""
        return self.post_hoc_temperature

    @staticmethod
    def _ts_make_table(T, s, device):
        nan = float("nan")
        return torch.tensor([T, s, nan, nan, nan, 0.0, 0.0, 0.0], dtype=torch.float64).to(device)

    def _ts_begin(self, temperature):
        """(device table, host T) of evaluate(temperature=...): None leaves the evaluation as it is."""
        if temperature is None or temperature is False:
            return None, None
        dev = self._arena.device
        if dev.type != "cuda":
            raise native.UvitError("the linear probe runs as HIP kernels: move the encoder and the probe to a GPU (no CPU fallback)")
        if temperature is True:
            if self._ts is None:
                raise native.UvitError("evaluate(temperature=True) needs fit_temperature() or set_temperature() first")
            if self._ts_table is None or self._ts_table.device != dev:
                self._ts_table = self._ts_make_table(self._ts[0], self._ts[1], dev)
            return self._ts_table, self._ts[0]
        T = float(temperature)
        if not 0.0 < T < math.inf:
            raise ValueError(f"the temperature must be positive and finite, got {temperature}")
        return self._ts_make_table(T, 1.0 / T, dev), T

    def _ts_apply(self, B):
        """Inside evaluate(temperature=...): self._logits[:B] <- (float)((double) z * s), in place, directly behind _logits_into."""
        if self._ts_on is not None:
            K = self.num_classes
            check(lib().uvit_op_ts_scale(ptr(self._logits), ptr(self._logits), K, K, ptr(self._ts_on), B, K, cur_stream()), "uvit_op_ts_scale")

    # ---- split conformal prediction sets (csrc/conformal.hip) ----
    @staticmethod
    def _cp_settings(alpha, score, lam, kreg):
        """([alpha, ...], kind, lam, kreg) checked on the host; lam and kreg belong to raps and are 0 for the other two scores."""
        alphas = [float(a) for a in (alpha if isinstance(alpha, (list, tuple)) else [alpha])]
        if not 1 <= len(alphas) <= CP_MAX_A or not all(0.0 < a < 1.0 for a in alphas):
            raise native.UvitError(f"alpha must be 1 .. {CP_MAX_A} numbers in (0, 1), got {alpha}")
        if score not in CP_KINDS:
            raise native.UvitError(f"score must be one of {list(CP_KINDS)}, got {score!r}")
        lam, kreg = (float(lam), int(kreg)) if score == "raps" else (0.0, 0)
        if not 0.0 <= lam < math.inf or kreg < 0:
            raise native.UvitError(f"raps needs lam >= 0 and kreg >= 0, got {lam}, {kreg}")
        return alphas, score, lam, kreg

    def _cp_check(self, logits, labels, u, limit=CP_MAX_N):
        """Caller-supplied logits (N, K) fp32, labels (N,) int64 and u (N,) fp32 or None, all on the GPU; returns N."""
        if not torch.is_tensor(logits) or not logits.is_cuda:
            raise native.UvitError("logits must be a GPU tensor: the HIP path has no CPU fallback")
        if logits.dtype != torch.float32 or logits.ndim != 2 or logits.shape[1] != self.num_classes or not logits.is_contiguous():
            raise native.UvitError(f"logits must be a contiguous float32 tensor of shape (N, {self.num_classes})")
        N = logits.shape[0]
        if not 1 <= N <= limit or not 2 <= self.num_classes <= CP_MAX_K:
            raise native.UvitError(f"conformal sets take 1 .. {limit} rows of 2 .. {CP_MAX_K} classes, got {N} of {self.num_classes}")
        self._labels(labels, N)
        if u is not None and (not torch.is_tensor(u) or not u.is_cuda or u.dtype != torch.float32 or u.shape != (N,) or not u.is_contiguous()):
            raise native.UvitError(f"u must be a contiguous float32 GPU tensor of shape ({N},)")
        return N

    def _cp_scores_into(self, logits, ld, labels, u, N, st, dst):
        """uvit_op_cp_scores of N rows on the current stream; `dst` is a device pointer to N doubles."""
        check(lib().uvit_op_cp_scores(ptr(logits), int(ld), ptr(labels), ptr(u), N, self.num_classes, CP_KINDS[st["score"]], st["lam"],
                                      st["kreg"], C.c_void_p(dst), cur_stream()), "uvit_op_cp_scores")

    def _cp_quantile(self, scores, N, alphas):
        """uvit_op_cp_quantile on the current stream: the (A, 16) float64 device table."""
        A = len(alphas)
        ws = lib().uvit_op_cp_ws_bytes(N, A)
        if ws < 0:
            check(int(ws), "uvit_op_cp_ws_bytes")
        if self._cp_ws is None or self._cp_ws.numel() < ws or self._cp_ws.device != scores.device:
            self._cp_ws = torch.empty(int(ws), dtype=torch.uint8, device=scores.device)
        table = torch.zeros(A, CP_TABLE, dtype=torch.float64, device=scores.device)
        host = (C.c_double * A)(*alphas)
        check(lib().uvit_op_cp_quantile(ptr(scores), N, host, A, ptr(table), ptr(self._cp_ws), self._cp_ws.numel(), cur_stream()),
              "uvit_op_cp_quantile")
        return table

    def _cp_counters(self, A, device):
        n = lib().uvit_op_cp_counter_count(self.num_classes, A)
        if n < 0:
            check(int(n), "uvit_op_cp_counter_count")
        return torch.zeros(int(n), dtype=torch.int64, device=device)

    def _cp_sets_into(self, logits, ld, labels, u, B, st, counters, sizes=None, covered=None):
        A = len(st["alpha"])
        check(lib().uvit_op_cp_sets(ptr(logits), int(ld), ptr(labels), ptr(u), B, self.num_classes, CP_KINDS[st["score"]], st["lam"], st["kreg"],
                                    ptr(st["table"]), A, ptr(counters), ptr(sizes), ptr(covered), B, cur_stream()), "uvit_op_cp_sets")

    def _cp_finish(self, st, counters):
        """The state's table with the metric slots filled from `counters` (a copy: the fitted table keeps its zeros)."""
        table = st["table"].clone()
        check(lib().uvit_op_cp_finish(ptr(counters), ptr(table), self.num_classes, len(st["alpha"]), cur_stream()), "uvit_op_cp_finish")
        return table

    @staticmethod
    def _cp_result(st, rows, n_cal):
        """fit_conformal's / conformal_calibrate's host view of the table rows {alpha, q, k, n, rows left out, status}."""
        nan = any(math.isnan(r[5]) for r in rows)
        return {"alpha": list(st["alpha"]), "qhat": [r[1] for r in rows], "k": [-1 if nan else int(r[2]) for r in rows],
                "n": -1 if nan else int(rows[0][3]), "n_skipped": -1 if nan else int(rows[0][4]),
                "status": [-1 if nan else int(r[5]) for r in rows], "score": st["score"], "lam": st["lam"], "kreg": st["kreg"],
                "randomized": st["randomized"], "seed": st["seed"], "n_rows": n_cal}

    def conformal_calibrate(self, logits, labels, alpha=0.1, score="aps", lam=0.0, kreg=0, u=None):
        """Split-conformal calibration on caller-supplied GPU logits (N, K) fp32 with int64 labels (N,) and an optional fp32 u (N,) in
        [0, 1] (None: not randomised): the label scores (uvit_op_cp_scores) and their order statistics (uvit_op_cp_quantile) for one
        alpha or a list of up to 8.  Returns the state conformal_sets() and set_conformal() take: {"table": (A, 16) float64 device table
        {alpha, qhat, k, n, rows left out, status, ...}, "scores": the (N,) float64 device column, "alpha", "score", "lam", "kreg"}.
        Nothing synchronises with the host and the probe's own state is not touched."""
        alphas, score, lam, kreg = self._cp_settings(alpha, score, lam, kreg)
        N = self._cp_check(logits, labels, u)
        st = {"alpha": alphas, "score": score, "lam": lam, "kreg": kreg, "randomized": u is not None, "seed": None}
        col = torch.zeros(N, dtype=torch.float64, device=logits.device)
        self._cp_scores_into(logits, self.num_classes, labels, u, N, st, col.data_ptr())
        st["scores"], st["table"] = col, self._cp_quantile(col, N, alphas)
        return st

    def conformal_sets(self, logits, labels, state, u=None, counters=None):
        """The sets of caller-supplied GPU logits (B, K) against a state of conformal_calibrate(): {"sizes": (A, B) int32 (-1: a row
        with a non-finite logit), "covered": (A, B) uint8, "counters": the int64 device counters (pass them in again to go on adding
        over consecutive batches), "table": the (A, 16) table with the metric slots of uvit_op_cp_finish over everything the counters
        hold}.  Nothing synchronises with the host."""
        B = self._cp_check(logits, labels, u)
        A = len(state["alpha"])
        if counters is None:
            counters = self._cp_counters(A, logits.device)
        sizes = torch.zeros(A, B, dtype=torch.int32, device=logits.device)
        covered = torch.zeros(A, B, dtype=torch.uint8, device=logits.device)
        self._cp_sets_into(logits, self.num_classes, labels, u, B, state, counters, sizes, covered)
        return {"sizes": sizes, "covered": covered, "counters": counters, "table": self._cp_finish(state, counters)}

    def set_conformal(self, state):
        """Use a state of conformal_calibrate() in evaluate_conformal(); None forgets the fitted one.  Not a parameter and not a
        buffer: state_dict() and the checkpoints keep their keys."""
        if state is not None and not (isinstance(state, dict) and {"table", "alpha", "score", "lam", "kreg"} <= set(state)):
            raise native.UvitError("set_conformal takes a state of conformal_calibrate() or None")
        self._cp = None if state is None else {"randomized": False, "seed": None, **state}

    @property
    def conformal(self):
        """The fitted or set conformal state, None when there is none."""
        return self._cp

    def _cp_u(self, B, gen, device):
        return torch.rand(B, generator=gen, device=device, dtype=torch.float32) if gen is not None else None

    def fit_conformal(self, loader, alpha=0.1, score="aps", lam=0.0, kreg=0, randomized=False, seed=0, temperature=None):
        """Calibrate conformal sets on a loader (items as evaluate()'s): every batch goes through the forward, the _logits_into and the
        post-hoc temperature of evaluate(temperature=...), uvit_op_cp_scores writes its label scores into a float64 device column grown
        geometrically (at most 2^20 entries; the logits are not kept), then one uvit_op_cp_quantile.  `randomized` draws the rows' u
        from a device generator seeded with `seed` (evaluate_conformal then draws its own from seed + 1).  The table stays on the
        device for evaluate_conformal() and is read once: {"alpha", "qhat", "k", "status" (lists in the order of `alpha`; status 0: a
        finite qhat, 1: fewer rows than the level needs, qhat = +inf and every set is full), "n", "n_skipped" (rows with a non-finite
        logit), "score", "lam", "kreg", "randomized", "seed", "n_rows"}.  An ensemble contributes its combined logits, a GP or
        heteroscedastic head the logits its evaluation sees."""
        alphas, score, lam, kreg = self._cp_settings(alpha, score, lam, kreg)
        st = {"alpha": alphas, "score": score, "lam": lam, "kreg": kreg, "randomized": bool(randomized), "seed": int(seed)}
        if not 2 <= self.num_classes <= CP_MAX_K:
            raise native.UvitError(f"conformal sets take 2 .. {CP_MAX_K} classes, the head has {self.num_classes}")
        self._ts_on, _ = self._ts_begin(temperature)
        col, n, gen = None, 0, None
        try:
            for item in loader:
                images, labels = item
                if isinstance(images, (tuple, list)):
                    images = images[0]
                B = self._features(images)
                if torch.is_tensor(labels) and not labels.is_cuda:
                    labels = labels.to(images.device, non_blocking=True)
                labels = self._labels(labels, B)
                if n + B > CP_MAX_N:
                    raise native.UvitError(f"conformal calibration takes at most {CP_MAX_N} samples, the loader holds more")
                if col is None or n + B > col.shape[0]:
                    grown = torch.zeros(min(CP_MAX_N, max(n + B, 2 * (col.shape[0] if col is not None else 0), 1024)), dtype=torch.float64,
                                        device=images.device)
                    if n:
                        grown[:n].copy_(col[:n])
                    col = grown
                if randomized and gen is None:
                    gen = torch.Generator(device=images.device).manual_seed(int(seed))
                self._logits_into(B)
                self._ts_apply(B)
                self._cp_scores_into(self._logits, self.num_classes, labels, self._cp_u(B, gen, images.device), B, st, col.data_ptr() + 8 * n)
                n += B
        finally:
            self._ts_on = None
        if not n:
            raise native.UvitError("conformal calibration needs at least one calibration sample")
        st["table"] = self._cp_quantile(col, n, alphas)
        rows = st["table"].cpu().tolist()                                              # the one read
        self._cp = st
        st["fit"] = self._cp_result(st, rows, n)
        return dict(st["fit"])

    def evaluate_conformal(self, loader, sizes=False, temperature=None):
        """The conformal sets of an evaluation loader against the fitted or set state (an error when there is none): every batch goes
        through the forward, the _logits_into and the temperature of evaluate(temperature=...), then uvit_op_cp_sets adds it to integer
        device counters; uvit_op_cp_finish and one host read follow the last batch.  Returns {"conformal": {alpha: {"coverage", "size"
        (mean), "empty", "singleton" (shares), "max_size", "sscv", "worst_class", "n", "n_skipped", "qhat"}}}; with `sizes`, also
        "sizes": the (A, n) int32 device tensor of the set sizes in loader order (-1: a row left out), an uncertainty column for
        detection_batch()."""
        st = self._cp
        if st is None:
            raise native.UvitError("evaluate_conformal needs fit_conformal() or set_conformal() first")
        A = len(st["alpha"])
        self._ts_on, _ = self._ts_begin(temperature)
        counters, gen, kept = None, None, []
        try:
            for item in loader:
                images, labels = item
                if isinstance(images, (tuple, list)):
                    images = images[0]
                B = self._features(images)
                if torch.is_tensor(labels) and not labels.is_cuda:
                    labels = labels.to(images.device, non_blocking=True)
                labels = self._labels(labels, B)
                if counters is None:
                    counters = self._cp_counters(A, images.device)
                    if st["randomized"]:
                        gen = torch.Generator(device=images.device).manual_seed(int(st["seed"] or 0) + 1)
                out = torch.zeros(A, B, dtype=torch.int32, device=images.device) if sizes else None
                self._logits_into(B)
                self._ts_apply(B)
                self._cp_sets_into(self._logits, self.num_classes, labels, self._cp_u(B, gen, images.device), B, st, counters, out)
                if sizes:
                    kept.append(out)
        finally:
            self._ts_on = None
        nan = float("nan")
        keys = ("coverage", "size", "empty", "singleton", "max_size", "sscv", "worst_class")
        if counters is None:
            res = {"conformal": {a: {**{k: nan for k in keys}, "n": 0, "n_skipped": 0, "qhat": nan} for a in st["alpha"]}}
        else:
            rows = self._cp_finish(st, counters).cpu().tolist()                        # the one read
            res = {"conformal": {a: {**dict(zip(keys, r[6:13])), "n": int(r[13]), "n_skipped": int(r[14]), "qhat": r[1]}
                                 for a, r in zip(st["alpha"], rows)}}
            for v in res["conformal"].values():
                if not math.isnan(v["max_size"]):
                    v["max_size"] = int(v["max_size"])
        if sizes:
            res["sizes"] = torch.cat(kept, dim=1) if kept else None
        return res

    # ---- evaluation ----
    def evaluate(self, loader, calibration=False, detection=False, ood_loader=None, temperature=None):
        """`loader` yields (images, labels) or ((images, mask), labels) on the GPU (the device prefetcher's items).  Plain cross-entropy
        (the reference's evaluate() uses nn.CrossEntropyLoss) and top-1 / top-5 accuracy in percent, from device-side per-batch
        losses and integer counters that are read once, after the last batch.  With `calibration`, every batch (at most 1024 samples)
        also runs the calibration ops on its logits and the result gains ECE, TACE, NLL and AUROC: batch-size-weighted means of the
        per-batch values, the reference's meters (engine_for_finetuning.py:207-213), ECE and TACE with the reference's bin accuracy
        (calibration_batch's reference_bin_accuracy=True).  A batch in which no class has both a positive
        and a negative row has no AUROC and is left out of that mean only; AUROC_zero_absent is the weighted mean of
        (sum of the per-class values) / K, i.e. with every class absent from a batch scored 0.
        With `detection` (implied by `ood_loader`), every batch also writes its per-sample uncertainty columns (DETECT_COLUMNS) and
        wrong-prediction flags into a device store, and one set-level call behind the last batch ranks all samples per column:
        stats["detection"] = {"columns", "n", "n_wrong", "misclassification": {column: {AUROC, AUPR, FPR95, AURC}}} with positive =
        wrong prediction.  `ood_loader` yields images of another data set (labels, if any, are ignored): they go through the same
        forward and columns behind the evaluation set, take no part in loss, accuracy, calibration or any mean, and a second call
        with positive = OOD image adds "ood": {column: {AUROC, AUPR, FPR95}} and "n_ood".  The two small tables are read with the
        losses.  Without the two arguments nothing else is launched or returned.
        While a density is set (fit_density, load_density_state), detection also stores the columns `maha` and `rmaha` of every batch's
        features, the OOD images' included, behind the head's own columns, and stats gains "maha_mean" (the mean of `maha` over the
        evaluation rows that are not NaN) and "maha_acc1" (the nearest-class-mean accuracy in percent, counted on the device).
        While a neighbour bank is set (fit_neighbours, load_neighbour_state), detection also stores the column `knn` of every batch's
        features, the OOD images' included, behind those, and stats gains "knn_mean" (the mean of `knn` over the evaluation rows that
        are not NaN) and "knn_acc1" (the weighted k-NN accuracy in percent, counted on the device).
        `temperature`: None launches and returns exactly the above.  True applies the fitted or set post-hoc temperature
        (fit_temperature, set_temperature; an error when there is none), a number applies that T: uvit_op_ts_scale then runs in place
        on the logits directly behind every _logits_into of the evaluation, the OOD images included, with 1 / T read from a device
        table, so loss, accuracy counters, the calibration ops and the three detection columns of the logits (msp, entropy, energy)
        see z / T, and stats gains "temperature".  Not scaled, because they are formed before the combination or do not depend on the
        scale of the logits: the members' own lines and the ens_* columns of an ensemble, gp_var, het_var, and everything
        evaluate_stability reports (ranks do not depend on T)."""
        detection = bool(detection) or ood_loader is not None
        self._ts_on, ts_value = self._ts_begin(temperature)
        self._det = {"scores": None, "flags": None, "cap": 0, "n": 0} if detection else None
        self._maha_eval = {"correct": None, "slabs": []} if detection and self._maha is not None else None
        self._knn_eval = {"correct": None, "slabs": []} if detection and self._knn is not None else None
        try:
            stats = self._evaluate(loader, calibration, ood_loader)
            if ts_value is not None:
                stats["temperature"] = ts_value
            return stats
        finally:
            self._det, self._in_ood, self._ts_on, self._maha_eval, self._knn_eval = None, False, None, None, None

    def _evaluate(self, loader, calibration, ood_loader):
        detection = self._det is not None
        losses, sizes, counters = [], [], None
        calib = []
        for item in loader:
            images, labels = item
            if isinstance(images, (tuple, list)):
                images = images[0]
            B = self._features(images)
            if torch.is_tensor(labels) and not labels.is_cuda:
                labels = labels.to(images.device, non_blocking=True)
            labels = self._labels(labels, B)
            if counters is None:
                counters = torch.zeros(2, dtype=torch.int32, device=images.device)
            if len(losses) % 256 == 0:
                slab = torch.zeros(256, dtype=torch.float32, device=images.device)
            if detection:
                self._det_reserve(B)
                if self._maha_eval is not None:
                    if self._maha_eval["correct"] is None:
                        self._maha_eval["correct"] = torch.zeros(1, dtype=torch.int32, device=images.device)
                    self._maha_columns(B, labels)
                if self._knn_eval is not None:
                    if self._knn_eval["correct"] is None:
                        self._knn_eval["correct"] = torch.zeros(1, dtype=torch.int32, device=images.device)
                    self._knn_columns(B, labels)
            self._logits_into(B)
            self._ts_apply(B)
            slot = C.c_void_p(slab.data_ptr() + 4 * (len(losses) % 256))
            check(lib().uvit_op_probe_ce(ptr(self._logits), ptr(labels), f32(0.0), None, ptr(self._row_loss), slot, ptr(counters), B,
                                         self.num_classes, cur_stream()), "uvit_op_probe_ce")
            if calibration:
                self._buffers_for(B, calibration=True)
                if len(calib) % 256 == 0:
                    cslab = torch.zeros(256, 5, dtype=torch.float64, device=images.device)
                self._calibration_into(self._logits, labels, B, cslab.data_ptr() + 40 * (len(calib) % 256))
                calib.append((cslab, len(calib) % 256))
            if detection:
                self._det_rows(B, labels)
            losses.append((slab, len(losses) % 256))
            sizes.append(B)
        if detection:
            mis, ood, n_ood = self._det_launch(sum(sizes), ood_loader)
        if not sizes:
            empty = {"loss": float("nan"), "acc1": float("nan"), "acc5": float("nan"), "n": 0}
            if calibration:
                empty.update({k: float("nan") for k in ("ECE", "TACE", "NLL", "AUROC", "AUROC_zero_absent")})
            if detection:
                empty["detection"] = self._det_stats(mis, ood, 0, 0, n_ood, ood_loader is not None)
            if self._maha_eval is not None:
                empty.update(maha_mean=float("nan"), maha_acc1=float("nan"))
            if self._knn_eval is not None:
                empty.update(knn_mean=float("nan"), knn_acc1=float("nan"))
            return empty
        slabs = {id(s): s for s, _ in losses}
        host = {k: v.cpu() for k, v in slabs.items()}                       # the one read
        c1, c5 = (int(v) for v in counters.cpu())
        n = sum(sizes)
        loss = sum(float(host[id(s)][i]) * b for (s, i), b in zip(losses, sizes)) / n
        stats = {"loss": loss, "acc1": 100.0 * c1 / n, "acc5": 100.0 * c5 / n, "n": n, "correct1": c1, "correct5": c5}
        if calibration:
            chost = {k: v.cpu() for k, v in {id(s): s for s, _ in calib}.items()}          # read with the losses, after the last batch
            rows = [chost[id(s)][i].tolist() for s, i in calib]                            # per batch: ECE, NLL, TACE, AUROC sum, count
            for key, col in (("ECE", 0), ("TACE", 2), ("NLL", 1)):
                stats[key] = sum(r[col] * b for r, b in zip(rows, sizes)) / n
            have = [(r[3] / r[4], b) for r, b in zip(rows, sizes) if r[4] > 0]
            stats["AUROC"] = sum(a * b for a, b in have) / sum(b for _, b in have) if have else float("nan")
            stats["AUROC_zero_absent"] = sum(r[3] / self.num_classes * b for r, b in zip(rows, sizes)) / n
        if detection:
            stats["detection"] = self._det_stats(mis, ood, n, n - c1, n_ood, ood_loader is not None)
        if self._maha_eval is not None:                                     # read with the counters, after the last batch
            vals = [v for v in torch.cat(self._maha_eval["slabs"]).cpu().tolist() if not math.isnan(v)]
            stats["maha_mean"] = math.fsum(vals) / len(vals) if vals else float("nan")
            stats["maha_acc1"] = 100.0 * int(self._maha_eval["correct"].cpu()) / n
        if self._knn_eval is not None:
            vals = [v for v in torch.cat(self._knn_eval["slabs"]).cpu().tolist() if not math.isnan(v)]
            stats["knn_mean"] = math.fsum(vals) / len(vals) if vals else float("nan")
            stats["knn_acc1"] = 100.0 * int(self._knn_eval["correct"].cpu()) / n
        return stats

    # ---- stability under perturbation sequences ----
    def _stability_buffers_for(self, R, V):
        """Ranks (R, K) int32 and per-sequence sums (V, 3) float64 of the stability ops (csrc/stability.hip), grown on demand."""
        dev = self._arena.device
        if dev.type != "cuda":
            raise native.UvitError("the stability ops run as HIP kernels: move the encoder and the probe to a GPU (no CPU fallback)")
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
        if not torch.is_tensor(logits) or not logits.is_cuda:
            raise native.UvitError("logits must be a GPU tensor: the HIP path has no CPU fallback")
        if logits.dtype != torch.float32 or logits.ndim != 2 or logits.shape[1] != self.num_classes or not logits.is_contiguous():
            raise native.UvitError(f"logits must be a contiguous float32 tensor of shape (V * frames, {self.num_classes})")
        F = self._frames(frames)
        R = logits.shape[0]
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
        for item in loader:
            images = item
            while isinstance(images, (tuple, list)):
                images = images[0]
            B = self._features(images)
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

    # ---- optimizer state beside head.* in a checkpoint ----
    def optimizer_state_dict(self):
        K, Cd = self.num_classes, self.embed_dim
        cut = lambda t: {"head.weight": t[:K * Cd].view(K, Cd).cpu().clone(), "head.bias": t[K * Cd:K * Cd + K].cpu().clone()}  # noqa: E731
        return {"step": self.step_count, "exp_avg": cut(self.exp_avg), "exp_avg_sq": cut(self.exp_avg_sq)}

    def load_optimizer_state_dict(self, sd):
        K, Cd = self.num_classes, self.embed_dim
        self.step_count = int(sd["step"])
        for arena, key in ((self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq")):
            arena[:K * Cd].view(K, Cd).copy_(sd[key]["head.weight"])
            arena[K * Cd:K * Cd + K].copy_(sd[key]["head.bias"])


def build_probe_encoder(model_name, target_layer=-1, **kwargs):
    """The frozen encoder of a probe: `create_model(model_name, **kwargs)`, or, with target_layer = L >= 0, the same architecture cut
    after block L (run_class_finetuning.py:520-522 truncates model.blocks), i.e. built with depth = L + 1.  In eval mode."""
    full = create_model(model_name, pretrained=False, **kwargs)
    if target_layer is not None and target_layer != -1:
        if not 0 <= target_layer < full.depth:
            raise ValueError(f"--target_layer {target_layer} outside [0, {full.depth})")
        if target_layer + 1 < full.depth:
            full = type(full)(**{**full._ctor, "depth": target_layer + 1})
    return full.eval()


def load_encoder_checkpoint(encoder, checkpoint, model_key="model|module", model_prefix=""):
    """Load a pre-training checkpoint (utils.save_model's dict, or a bare state dict) into the encoder.  `model_key` picks the entry as
    run_class_finetuning.py:400-406 does; `model_prefix` is stripped from the keys.  Every tensor the encoder has must be there;
    what the encoder does not have (deeper blocks of a truncated encoder) is left out.  Returns the names left out."""
    sd = checkpoint
    for key in model_key.split("|"):
        if isinstance(checkpoint, dict) and key in checkpoint:
            sd = checkpoint[key]
            print("Load state_dict by model_key = %s" % key)
            break
    if model_prefix:
        sd = {k[len(model_prefix):]: v for k, v in sd.items() if k.startswith(model_prefix)}
    own = encoder.state_dict()
    missing = [k for k in own if k not in sd]
    if missing:
        raise KeyError(f"checkpoint lacks encoder tensors: {missing[:8]}{' ...' if len(missing) > 8 else ''}")
    encoder.load_state_dict({k: sd[k] for k in own}, strict=True)
    return sorted(k for k in sd if k not in own)
