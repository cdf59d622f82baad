"""Linear probe of the two-stream (mean, covariance) model, with the covariance stream read as a predictive variance (DESIGN.md
section 9.17).

    frozen two-stream encoder (eval forward, native) -> both streams of the last block: mean of the patch tokens -> LayerNorm
    without affine -> m (mean stream), c (covariance stream)          modeling_finetune_dist.py:280-326
    logits z = W m + b, trained with the linear probe's loss: the reference's classifier with a frozen encoder, where its
    Wasserstein term (engine_for_finetuning_dist.py:286-304) has no trainable parameter.

The reference never turns c into an uncertainty.  This project's definition: v = s (ELU(c) + 1), the map the model applies to its
own covariances, is the variance of a feature f ~ N(m, diag(v)); the head carries it to z ~ N(W m + b, W diag(v) W^T), of which the
diagonal var[b, k] = sum_c W[k, c]^2 v[b, c] is built (uvit_op_dprobe_variance), with the mean-field probit link
z / sqrt(1 + mean_field var) of the Laplace probe (uvit_op_lap_probit) and two detection columns: `dist_var`, the variance of the
class the unscaled logits predict, and `dist_trace` = mean_c v[b, c], which does not depend on the head.  Everything behind the last
block runs as the HIP kernels of csrc/dprobe.hip, csrc/probe.hip and csrc/laplace.hip on the stream of the encoder forward.  There
is no CPU fallback.
"""
import ctypes as C
import math

import torch

from . import native
from .linear_probe import LinearProbe
from .native import check, cur_stream, f32, lib, ptr
from .probe_util import column_mean, ws_size

__all__ = ["DistProbe", "DIST_MEAN_FIELD"]

DIST_MAX_C, DIST_MAX_K = 2048, 4096        # csrc/dprobe.hip and uvit_op_lap_probit: C % 4 == 0, 4 <= C <= 2048, 2 <= K <= 4096
DIST_MEAN_FIELD = math.pi / 8.0            # the probit link of the literature; the default is 0: the reference's logits
F64 = torch.float64


def _factor(value, what, positive=False):
    v = float(value)
    if not (0.0 < v < math.inf if positive else 0.0 <= v < math.inf):
        raise ValueError(f"{what} must be finite and {'greater than 0' if positive else 'at least 0'}, got {value}")
    return v


class DistProbe(LinearProbe):
    """A LinearProbe on a DistVisionTransformerForCyclicalTraining in .eval().  state_dict() holds exactly `head.weight` and
    `head.bias` and the arenas are the linear probe's, so a linear probe-N.pth resumes; train_step is the linear probe's, on the mean
    stream's feature.  `mean_field` (default 0: the evaluated logits are the reference's, bit for bit) is the factor of the probit
    link on every logit the probe reports outside train_step; `var_scale` is s."""

    TWO_STREAM = True
    DETECT_COLUMNS = LinearProbe.DETECT_COLUMNS + ("dist_var", "dist_trace")

    def __init__(self, encoder, num_classes, smoothing=0.1, init_scale=0.001, mean_field=0.0, var_scale=1.0):
        super().__init__(encoder, num_classes, smoothing=smoothing, init_scale=init_scale)
        Cd, K = self.embed_dim, self.num_classes
        if Cd < 4 or Cd % 4 or Cd > DIST_MAX_C or not 2 <= K <= DIST_MAX_K:
            raise ValueError(f"the two-stream probe's ops take an embed dim that is a multiple of 4 in [4, {DIST_MAX_C}] and 2 .. {DIST_MAX_K} "
                             f"classes, got {Cd} and {K}")
        self.mean_field, self.var_scale = _factor(mean_field, "mean_field"), _factor(var_scale, "var_scale", positive=True)
        self._link, self._trace_slabs, self._eye = True, None, None

    def _apply(self, fn, recurse=True):
        self._eye = None
        return super()._apply(fn, recurse)

    def _head_buffers_for(self, B):
        K, Cd, dev = self.num_classes, self.embed_dim, self._arena.device
        N = self.encoder.patch_embed.num_patches + 1
        self._scratch = torch.zeros(ws_size(lib().uvit_op_dprobe_pool_ws_bytes, B, N, Cd) // 4, dtype=torch.float32, device=dev)
        self._cfeat = torch.zeros(B, Cd, dtype=torch.float32, device=dev)
        self._dist_var = torch.zeros(B, K, dtype=F64, device=dev)
        self._dist_col = torch.zeros(B, dtype=torch.float32, device=dev)
        self._dist_trace = torch.zeros(B, dtype=torch.float32, device=dev)

    # ---- forward ----
    def _features(self, images):
        """Encoder eval forward, then pool + norm of both streams of the last block into self._feat[:B] and self._cfeat[:B] in one
        launch pair on the current stream; returns B."""
        self._check_images(images)
        B = images.shape[0]
        self._buffers_for(B)
        enc = self.encoder
        e = enc.forward_features(images, bool_masked_pos=None, layer_results=None)
        x, xc = (lib().uvit_engine_ws_ptr(e.h, name, enc.depth) for name in (b"x", b"x_cov"))
        if not x or not xc:
            raise native.UvitError("the two residual streams of the last block are not both in the engine workspace")
        N = enc.patch_embed.num_patches + 1
        check(lib().uvit_op_dprobe_pool_norm(C.c_void_p(x), C.c_void_p(xc), ptr(self._feat), ptr(self._cfeat), ptr(self._scratch), B, N,
                                             self.embed_dim, f32(enc.ln_eps), cur_stream()), "uvit_op_dprobe_pool_norm")
        return B

    def _variance_into(self, B, W=None, K=None, var=None, trace=None):
        """var of self._cfeat[:B] under the head (or `W` (K, C)) into self._dist_var[:B] (or `var`), the trace into `trace`."""
        check(lib().uvit_op_dprobe_variance(ptr(self._cfeat), ptr(self._arena if W is None else W), C.c_double(self.var_scale),
                                            ptr(self._dist_var if var is None else var), ptr(trace), B, self.num_classes if K is None else K,
                                            self.embed_dim, cur_stream()), "uvit_op_dprobe_variance")

    def _logits_into(self, B):
        super()._logits_into(B)
        if not self._link:                                       # train_step: the linear probe's logits and nothing behind them
            return
        K = self.num_classes
        self._variance_into(B, trace=self._dist_trace)
        check(lib().uvit_op_lap_probit(ptr(self._logits), K, ptr(self._dist_var), C.c_double(self.mean_field), ptr(self._logits), K,
                                       ptr(self._dist_col), B, K, cur_stream()), "uvit_op_lap_probit")
        self._own_column("dist_var", self._dist_col, B, self._var_slabs)          # the variance of the predicted class
        self._own_column("dist_trace", self._dist_trace, B, self._trace_slabs)

    def cov_features(self, images):
        """(B, C) fp32: fc_norm(x_cov[:, 1:].mean(1)) of the last block's covariance stream."""
        B = self._features(images)
        return self._cfeat[:B].clone()

    def feature_variance(self, images):
        """(B, C) float64 on the device: v = var_scale (ELU(c) + 1) of the covariance feature c, uvit_op_dprobe_variance under the
        identity in place of the head (fma(v, 1, 0) and fma(v, 0, acc) are exact)."""
        B, Cd = self._features(images), self.embed_dim
        if self._eye is None:
            self._eye = torch.eye(Cd, dtype=torch.float32, device=self._arena.device)
        v = torch.zeros(B, Cd, dtype=F64, device=self._arena.device)
        self._variance_into(B, W=self._eye, K=Cd, var=v)
        return v

    def predictive_variance(self, images):
        """(B, K) float64 on the device: the diagonal of W diag(v) W^T at the images' covariance features."""
        B = self._features(images)
        self._variance_into(B)
        return self._dist_var[:B].clone()

    # ---- training: the linear probe's, on the mean stream ----
    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        """LinearProbe.train_step on the mean stream's feature: the loss sees W m + b whatever `mean_field` says."""
        self._link = False
        try:
            return super().train_step(images, labels, lr, weight_decay, max_norm)
        finally:
            self._link = True

    # ---- ViM: the reported logits are affine in the mean feature at mean_field = 0 only ----
    def _vim_head(self):
        if self.mean_field != 0.0:
            self._vim_not_affine("the two-stream probe with mean_field > 0 divides every logit by a function of the covariance feature")
        return super()._vim_head()

    # ---- evaluation ----
    def evaluate(self, loader, calibration=False, detection=False, ood_loader=None, variance=True, mean_field=None, temperature=None):
        """LinearProbe.evaluate on z / sqrt(1 + mean_field var) (`mean_field`: None takes the probe's; 0 leaves the logits as they
        are): loss, accuracy, calibration and the msp / entropy / energy columns see them, the post-hoc temperature is applied behind
        them.  Detection gains the columns `dist_var` and `dist_trace`, and with `variance` the result gains `dist_var_mean` and
        `dist_trace_mean`, the means of the two columns over the evaluation set, from per-batch device slabs read after the last
        batch.  A ViM fit and mean_field > 0 are refused together."""
        keep = self.mean_field
        if mean_field is not None:
            self.mean_field = _factor(mean_field, "mean_field")
        self._var_slabs, self._trace_slabs = ([], []) if variance else (None, None)
        try:
            if self.mean_field != 0.0 and self._vim is not None and (detection or ood_loader is not None):
                self._vim_head()
            stats = LinearProbe.evaluate(self, loader, calibration=calibration, detection=detection, ood_loader=ood_loader,
                                         temperature=temperature)
            if variance:
                stats["dist_var_mean"], stats["dist_trace_mean"] = column_mean(self._var_slabs), column_mean(self._trace_slabs)
            return stats
        finally:
            self.mean_field, self._var_slabs, self._trace_slabs = keep, None, None
