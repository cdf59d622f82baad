"""Heteroscedastic probe head on the frozen encoder: Monte-Carlo softmax over logits with an input-dependent low-rank-plus-diagonal
Gaussian noise (Collier et al., CVPR 2021), the layer `run_class_finetuning.py --het_layer` names (`modeling_finetune.MCSoftmaxDenseFA`,
:904-1217), behind the pooled features of the linear probe.

    pooled features f (linear_probe.py) -> lin = f . W^T + bias, W (K (R + 2), C) -> [ loc (K) | draw (K) | V (K, R) ]
    u_s = loc + V . epsR_s + (draw + 1e-3) * epsK_s   ->   p = mean_s softmax(u_s / T)   ->   z = log(clamp(p, 1e-7, 1))

The three nn.Linear layers of the class (`_loc_layer`, `_diag_layer`, `_scale_layer`) are the rows of ONE matrix in one arena, so the
forward is one uvit_op_probe_logits call and the head gradient one uvit_op_probe_head_grad call; the Monte-Carlo softmax and its
backward are the kernel pair of csrc/het.hip, which regenerate their counter-based noise and store no draw.  The specification is
what the class's docstrings describe (edward2's MCSoftmaxDenseFA), not what its forward computes: it creates its layers anew on every
call and takes the softmax over the batch axis (section 9.4).  Evaluation shares the draws across the batch under the fixed seed, so a
prediction is a function of the image alone; training draws per row under a seed that changes with every step.
"""
import math

import torch
import torch.nn as nn

from .linear_probe import LinearProbe
from .modeling_cyclical import _Holder
from .native import check, cur_stream, f32, lib, ptr
from .probe_util import ws_size

__all__ = ["HetProbe"]

EPS = 1e-7                   # the clamp under the logarithm
MAX_CLASSES, MAX_FACTORS, MAX_SAMPLES = 4096, 32, 65535      # csrc/het.hip: 3 <= K <= 4096, 1 <= R <= min(32, K), 1 <= S <= 65535


def _hash32(x):
    """uvit_hash32 of csrc/common.h."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


class HetProbe(LinearProbe):
    """state_dict() holds the class's attribute names: head._loc_layer.{weight (K, C), bias (K)}, head._diag_layer.{weight (K, C),
    bias (K)}, head._scale_layer.{weight (K R, C), bias (K R)}.  `num_factors` R is the rank of the noise covariance's low-rank part;
    the reference re-seeds with 42 on every forward, `seed` has that default."""

    # the softmax temperature of the Monte-Carlo samples, a constructor argument: it keeps the name, so on this head the post-hoc
    # temperature of LinearProbe is read as `post_hoc_temperature`
    temperature = 1.0

    def __init__(self, encoder, num_classes, smoothing=0.1, num_factors=10, temperature=1.0, train_mc_samples=1000, test_mc_samples=1000,
                 seed=42):
        K, R = int(num_classes), int(num_factors)
        if not 3 <= K <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in [3, {MAX_CLASSES}] for the heteroscedastic head, got {num_classes}")
        if not 1 <= R <= min(MAX_FACTORS, K):
            raise ValueError(f"num_factors must be in [1, min({MAX_FACTORS}, num_classes)], got {num_factors}")
        if not 0.0 < float(temperature) < math.inf:
            raise ValueError(f"temperature must be positive, got {temperature}")
        for name, v in (("train_mc_samples", train_mc_samples), ("test_mc_samples", test_mc_samples)):
            if not 1 <= int(v) <= MAX_SAMPLES:
                raise ValueError(f"{name} must be in [1, {MAX_SAMPLES}], got {v}")
        self.num_factors, self.temperature, self.seed = R, float(temperature), int(seed) & 0xFFFFFFFF
        self.train_mc_samples, self.test_mc_samples = int(train_mc_samples), int(test_mc_samples)
        super().__init__(encoder, num_classes, smoothing=smoothing)

    # ---- arena plumbing ----
    _OPT_KEYS = ("head._loc_layer.weight", "head._diag_layer.weight", "head._scale_layer.weight", "head._loc_layer.bias", "head._diag_layer.bias",
             "head._scale_layer.bias")

    def _views(self):
        """(parameter, lo, hi, shape) in arena order: [W_loc | W_diag | W_scale | b_loc | b_diag | b_scale | pad to 4]."""
        K, Cd, R = self.num_classes, self.embed_dim, self.num_factors
        h, w0 = self.head, K * (R + 2) * Cd
        return ((h._loc_layer.weight, 0, K * Cd, (K, Cd)), (h._diag_layer.weight, K * Cd, 2 * K * Cd, (K, Cd)),
                (h._scale_layer.weight, 2 * K * Cd, w0, (K * R, Cd)), (h._loc_layer.bias, w0, w0 + K, (K,)),
                (h._diag_layer.bias, w0 + K, w0 + 2 * K, (K,)), (h._scale_layer.bias, w0 + 2 * K, w0 + K * (R + 2), (K * R,)))

    def _setup_head(self, init_scale):
        K, Cd, R = self.num_classes, self.embed_dim, self.num_factors
        self._rows = K * (R + 2)                 # the three layers as one (K (R + 2), C) matrix and one bias vector
        self._n_decay = self._rows * Cd          # the weights decay, the biases do not
        n = (self._n_decay + self._rows + 3) // 4 * 4
        dev = self.encoder._arena.device
        self._arena, self._grad_arena, self.exp_avg, self.exp_avg_sq = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(4))
        self.step_count = 0
        self.head = h = _Holder()
        w0 = self._n_decay
        for name, rows, wlo, blo in (("_loc_layer", K, 0, w0), ("_diag_layer", K, K * Cd, w0 + K), ("_scale_layer", K * R, 2 * K * Cd, w0 + 2 * K)):
            layer = _Holder()
            layer.register_parameter("weight", nn.Parameter(self._arena[wlo:wlo + rows * Cd].view(rows, Cd)))
            layer.register_parameter("bias", nn.Parameter(self._arena[blo:blo + rows]))
            setattr(h, name, layer)
        self._rebind()
        # nn.Linear's default initial values, drawn on the host under the caller's seed in the order the class creates its layers
        with torch.no_grad():
            for name, rows in (("_loc_layer", K), ("_diag_layer", K), ("_scale_layer", K * R)):
                lin = nn.Linear(Cd, rows)
                getattr(h, name).weight.copy_(lin.weight)
                getattr(h, name).bias.copy_(lin.bias)

    def _vim_head(self):
        self._vim_not_affine("the heteroscedastic head reports the logarithm of a Monte-Carlo mean of softmaxes")

    def _head_buffers_for(self, B):
        K, R, dev = self.num_classes, self.num_factors, self._arena.device
        ws = max(ws_size(lib().uvit_op_het_mc_ws_bytes, B, S, K, R) for S in (self.train_mc_samples, self.test_mc_samples))
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)      # noqa: E731
        self._lin, self._dlin, self._p, self._pvar, self._het_scratch = z(B, self._rows), z(B, self._rows), z(B, K), z(B, K), z(ws // 4)

    # ---- forward ----
    def _mc_into(self, B, samples, seed, share, pvar=False):
        """lin of self._feat[:B], then z into self._logits, p into self._p and, with `pvar`, the predictive variance into self._pvar."""
        K, Cd, R, L, s = self.num_classes, self.embed_dim, self.num_factors, lib(), cur_stream()
        check(L.uvit_op_probe_logits(ptr(self._feat), ptr(self._arena), self._bias_ptr(self._arena), ptr(self._lin), B, self._rows, Cd, s),
              "uvit_op_probe_logits")
        check(L.uvit_op_het_mc_forward(ptr(self._lin), ptr(self._logits), ptr(self._p), ptr(self._pvar if pvar else None), ptr(self._het_scratch),
                                       B, samples, K, R, f32(self.temperature), f32(EPS), seed, share, s), "uvit_op_het_mc_forward")

    def _logits_into(self, B):
        """Evaluation: the draws are shared across the batch under the fixed seed, so a row's logits do not depend on its place."""
        want = self._det is not None or (self._var_slabs is not None and not self._in_ood)
        self._mc_into(B, self.test_mc_samples, self.seed, 1, pvar=want)
        if want:     # the variance at the predicted class: a column of evaluate(detection=True), kept for evaluate(variance=True)'s mean
            pred = self._logits[:B].argmax(1, keepdim=True)
            self._own_column("het_var", self._pvar[:B].gather(1, pred).squeeze(1), B, self._var_slabs, fresh=True)

    def predictive_variance(self, images):
        """(B, K) fp32: the variance over the Monte-Carlo samples of each class's softmax probability (compute_pred_variance)."""
        B = self._features(images)
        self._mc_into(B, self.test_mc_samples, self.seed, 1, pvar=True)
        return self._pvar[:B].clone()

    # ---- training ----
    def step_seed(self, step):
        """The noise seed of training step `step` (0-based): fresh draws every step."""
        return _hash32(self.seed ^ ((step * 0x85EBCA6B + 1) & 0xFFFFFFFF))

    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        """One step on the three layers, as LinearProbe.train_step: per-row draws (share = 0) under step_seed(step_count), the
        smoothed cross-entropy on z, the Monte-Carlo backward, one head-gradient call.  Returns (loss, grad_norm) as device scalars."""
        B = self._features(self._train_images(images))
        labels = self._labels(labels, B)
        K, Cd, R, L, s = self.num_classes, self.embed_dim, self.num_factors, lib(), cur_stream()
        seed = self.step_seed(self.step_count)
        self._mc_into(B, self.train_mc_samples, seed, 0)
        self._criterion(labels, B)
        check(L.uvit_op_het_mc_backward(ptr(self._lin), ptr(self._p), ptr(self._dlogits), ptr(self._dlin), ptr(self._het_scratch), B,
                                        self.train_mc_samples, K, R, f32(self.temperature), f32(EPS), seed, 0, s), "uvit_op_het_mc_backward")
        check(L.uvit_op_probe_head_grad(ptr(self._dlin), ptr(self._feat), ptr(self._grad_arena), self._bias_ptr(self._grad_arena), B, self._rows,
                                        Cd, s), "uvit_op_probe_head_grad")
        return self._clip_and_update(lr, weight_decay, max_norm)

    # ---- evaluation ----
    DETECT_COLUMNS = LinearProbe.DETECT_COLUMNS + ("het_var",)

    def evaluate(self, loader, calibration=False, variance=False, detection=False, ood_loader=None, temperature=None):
        """LinearProbe.evaluate on z.  `variance`: the result gains `het_var_mean`, the mean over the set of the predictive variance at
        each sample's predicted class, from per-batch device slabs read once after the last batch.  `detection`, `ood_loader`: as
        LinearProbe.evaluate, with that variance as the column `het_var` whatever `variance` says.  `temperature`: as
        LinearProbe.evaluate, the post-hoc temperature on z (not the softmax temperature of the samples); `het_var` and `het_var_mean`
        are variances of probabilities formed before it and do not change."""
        return self._evaluate_with_mean("het_var_mean", variance, loader, calibration=calibration, detection=detection, ood_loader=ood_loader,
                                        temperature=temperature)
