"""Random-feature Gaussian-process probe head on the frozen encoder: the reference's `modeling_finetune.SNGP` (:525-638), the head
`run_class_finetuning.py --gp_layer` names, behind the pooled features of the linear probe.

    pooled features f (linear_probe.py) -> LayerNorm(gamma, beta; eps 1e-12) -> u = g . W_rf^T + b_rf (frozen) -> phi = s cos(u)
    -> z = phi . W_out^T        P <- m P + (1 - m) phi^T phi / B on training steps        var[b] = ridge phi_b^T inv(P) phi_b

gamma, beta and W_out train; W_rf, b_rf and the precision matrix P do not.  Everything runs as the HIP kernels of csrc/gp.hip and
csrc/probe.hip on the stream of the encoder forward; the update is uvit_op_adamw on one arena [W_out (K D) | gamma (C) | beta (C) |
pad to 4] whose decay group (W_out) comes first.  inv(P) is formed on the host in float64 once per change of P and uploaded as
double: plumbing, not the hot path, and no device solver is needed.  The class is the specification: the reference's
VisionTransformer overwrites this head with an nn.Linear (modeling_finetune.py:416-421) and never uses it.
"""
import contextlib
import ctypes as C
import math

import torch
import torch.nn as nn

from . import native
from .linear_probe import LinearProbe
from .modeling_cyclical import _Holder
from .native import check, cur_stream, f32, lib, ptr
from .probe_util import ws_size

__all__ = ["GPProbe"]

LN_EPS = 1e-12               # SNGP.__init__: layer_norm_eps
MAX_INDUCING = 2048          # csrc/gp.hip: D % 4 == 0, 4 <= D <= 2048


class GPProbe(LinearProbe):
    """state_dict() holds the reference's keys: head._gp_input_normalize_layer.{weight, bias} (C), head._gp_output_layer.weight
    (K, D), head._random_feature.{weight (D, C), bias (D)} and head.precision_matrix (D, D).  `num_inducing` D defaults to the embed
    dim (what the reference passes); the cosine is multiplied by 1 / sqrt(kernel_scale) as in the reference (edward2 has
    sqrt(2 / D) there; the op takes either).  cov_momentum <= 0: the precision matrix is the exact sum over the training steps
    since the last reset_cov()."""

    def __init__(self, encoder, num_classes, smoothing=0.1, num_inducing=None, kernel_scale=1.0, cov_momentum=0.999,
                 cov_ridge_penalty=1e-3):
        D = int(encoder.embed_dim if num_inducing is None else num_inducing)
        if D < 4 or D % 4 or D > MAX_INDUCING:
            raise ValueError(f"num_inducing must be a multiple of 4 in [4, {MAX_INDUCING}], got {num_inducing}")
        if not float(kernel_scale) > 0.0:
            raise ValueError(f"kernel_scale must be positive, got {kernel_scale}")
        if not float(cov_ridge_penalty) > 0.0:
            raise ValueError(f"cov_ridge_penalty must be positive, got {cov_ridge_penalty}")
        if not float(cov_momentum) < 1.0:
            raise ValueError(f"cov_momentum must be below 1, got {cov_momentum}")
        self.num_inducing, self.ridge, self.cov_momentum = D, float(cov_ridge_penalty), float(cov_momentum)
        self.feature_scale = 1.0 / math.sqrt(float(kernel_scale))        # gp_input_scale (:549)
        super().__init__(encoder, num_classes, smoothing=smoothing)

    # ---- arena plumbing ----
    def _views(self):
        K, Cd, D = self.num_classes, self.embed_dim, self.num_inducing
        h = self.head
        return ((h._gp_output_layer.weight, 0, K * D, (K, D)), (h._gp_input_normalize_layer.weight, K * D, K * D + Cd, (Cd,)),
                (h._gp_input_normalize_layer.bias, K * D + Cd, K * D + 2 * Cd, (Cd,)))

    def _setup_head(self, init_scale):
        K, Cd, D = self.num_classes, self.embed_dim, self.num_inducing
        self._n_decay = K * D                    # optim_factory.get_parameter_groups: one-dimensional parameters do not decay
        n = K * D + 2 * Cd
        n = (n + 3) // 4 * 4
        dev = self.encoder._arena.device
        self._arena, self._grad_arena, self.exp_avg, self.exp_avg_sq = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(4))
        self.step_count = 0
        self._w_rf = torch.zeros(D, Cd, dtype=torch.float32, device=dev)
        self._b_rf = torch.zeros(D, dtype=torch.float32, device=dev)
        self._P = torch.zeros(D, D, dtype=torch.float32, device=dev)
        self.head = h = _Holder()
        h.register_parameter("precision_matrix", nn.Parameter(self._P, requires_grad=False))
        h._gp_input_normalize_layer, h._gp_output_layer, h._random_feature = _Holder(), _Holder(), _Holder()
        h._gp_input_normalize_layer.register_parameter("weight", nn.Parameter(self._arena[K * D:K * D + Cd]))
        h._gp_input_normalize_layer.register_parameter("bias", nn.Parameter(self._arena[K * D + Cd:K * D + 2 * Cd]))
        h._gp_output_layer.register_parameter("weight", nn.Parameter(self._arena[:K * D].view(K, D)))
        h._random_feature.register_parameter("weight", nn.Parameter(self._w_rf, requires_grad=False))
        h._random_feature.register_parameter("bias", nn.Parameter(self._b_rf, requires_grad=False))
        self._rebind()
        # the class's own initial values, drawn on the host under the caller's seed: LayerNorm (1, 0); nn.Linear's default for the
        # output layer (:556); N(0, 0.05^2) and U(0, 2 pi) for the frozen random features (modeling_finetune.py:36-46)
        w_out, w_rf, b_rf = torch.empty(K, D), torch.empty(D, Cd), torch.empty(D)
        nn.init.kaiming_uniform_(w_out, a=math.sqrt(5))
        nn.init.normal_(w_rf, mean=0.0, std=0.05)
        nn.init.uniform_(b_rf, a=0.0, b=2.0 * math.pi)
        with torch.no_grad():
            h._gp_output_layer.weight.copy_(w_out)
            h._gp_input_normalize_layer.weight.fill_(1.0)
            h._gp_input_normalize_layer.bias.zero_()
            self._w_rf.copy_(w_rf)
            self._b_rf.copy_(b_rf)
        self._cov_tick, self._sigma_key, self._mf = 0, None, 0.0
        self.reset_cov()

    def _rebind(self):
        super()._rebind()
        self.head._random_feature.weight.data, self.head._random_feature.bias.data = self._w_rf, self._b_rf
        self.head.precision_matrix.data = self._P

    def _apply(self, fn, recurse=True):
        self._w_rf, self._b_rf, self._P = (fn(t).contiguous() for t in (self._w_rf, self._b_rf, self._P))
        if self._P.dtype != torch.float32:
            raise NotImplementedError("the head stays fp32")
        self._sigma_key = None
        self._cov_tick += 1
        return super()._apply(fn, recurse)

    def _vim_head(self):
        self._vim_not_affine("the GP head passes the feature through random Fourier features")

    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._cov_tick += 1                      # the precision matrix may have changed: inv(P) is formed again
        return out

    def _head_buffers_for(self, B):
        K, Cd, D, dev = self.num_classes, self.embed_dim, self.num_inducing, self._arena.device
        ws = ws_size(lib().uvit_op_gp_ln_grad_ws_bytes, B, Cd, D)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
        self._phi, self._u, self._ghat, self._gp_scratch = z(B, D), z(B, D), z(B, Cd), z(ws // 4)
        self._var = z(B, dt=torch.float64)
        self._zero_bias, self._dbias = z(K), z(K)      # the output layer has no bias: gp_output_bias is the constant 0 (:561, :590)

    # ---- forward ----
    def _phi_into(self, B, keep=False):
        """phi of self._feat[:B] into self._phi; with `keep`, ghat and u of the rows as well (the backward reads them)."""
        Cd, D = self.embed_dim, self.num_inducing
        check(lib().uvit_op_gp_features(ptr(self._feat), ptr(self.head._gp_input_normalize_layer.weight), ptr(self.head._gp_input_normalize_layer.bias),
                                        ptr(self._w_rf), ptr(self._b_rf), f32(self.feature_scale), f32(LN_EPS), ptr(self._ghat if keep else None),
                                        ptr(self._u if keep else None), ptr(self._phi), B, Cd, D, cur_stream()), "uvit_op_gp_features")

    def _sigma(self):
        """inv(P) as a (D, D) double device tensor: float64 on the host, cached until P changes."""
        key = (self._cov_tick, self._P._version, self._P.data_ptr())
        if self._sigma_key != key:
            self._sigma_dev = torch.linalg.inv(self._P.detach().cpu().double()).contiguous().to(self._P.device)
            self._sigma_key = key
        return self._sigma_dev

    def _variance_into(self, B, out):
        """var of self._phi[:B] into the double tensor `out`."""
        check(lib().uvit_op_gp_variance(ptr(self._phi), ptr(self._sigma()), C.c_double(self.ridge), ptr(out), B, self.num_inducing,
                                        cur_stream()), "uvit_op_gp_variance")

    def _logits_into(self, B, keep=False):
        K, D = self.num_classes, self.num_inducing
        self._phi_into(B, keep)
        check(lib().uvit_op_probe_logits(ptr(self._phi), ptr(self._arena), ptr(self._zero_bias), ptr(self._logits), B, K, D, cur_stream()),
              "uvit_op_probe_logits")
        if keep:
            return
        # evaluate(variance=True) keeps the batch's variances on the device until the last batch: they get a tensor of their own
        keep_var = self._var_slabs is not None and not self._in_ood
        var = torch.empty(B, dtype=torch.float64, device=self._arena.device) if keep_var else self._var
        if keep_var or self._mf > 0.0 or self._det is not None:
            self._variance_into(B, var)
            self._own_column("gp_var", var, B, self._var_slabs, fresh=keep_var)     # evaluate(detection=True): a column of the store
        if self._mf > 0.0:
            check(lib().uvit_op_gp_mean_field(ptr(self._logits), ptr(var), C.c_double(self._mf), ptr(self._logits), B, K, cur_stream()),
                  "uvit_op_gp_mean_field")

    def predictive_variance(self, images):
        """(B,) float64: ridge phi_b^T inv(P) phi_b, the diagonal of the reference's compute_predictive_covariance (:618-626)."""
        B = self._features(images)
        self._phi_into(B)
        self._variance_into(B, self._var)
        return self._var[:B].clone()

    def reset_cov(self):
        """P <- ridge * I (the reference's reset_cov, :596-597)."""
        with torch.no_grad():
            self._P.zero_()
            self._P.diagonal().fill_(self.ridge)
        self._cov_tick += 1

    # ---- training ----
    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        """One step on gamma, beta and W_out, as LinearProbe.train_step; the precision matrix takes this batch's phi (training steps
        only: the reference also updates it on every evaluation forward through a default argument, a side effect that is not
        reproduced).  Returns (loss, grad_norm) as device scalars."""
        B = self._features(self._train_images(images))
        labels = self._labels(labels, B)
        K, Cd, D, L, s = self.num_classes, self.embed_dim, self.num_inducing, lib(), cur_stream()
        self._logits_into(B, keep=True)
        check(L.uvit_op_gp_precision_update(ptr(self._phi), ptr(self._P), B, D, C.c_double(self.cov_momentum), s), "uvit_op_gp_precision_update")
        self._cov_tick += 1
        self._criterion(labels, B)
        g = self._grad_arena.data_ptr()
        check(L.uvit_op_probe_head_grad(ptr(self._dlogits), ptr(self._phi), C.c_void_p(g), ptr(self._dbias), B, K, D, s),
              "uvit_op_probe_head_grad")
        check(L.uvit_op_gp_ln_grad(ptr(self._dlogits), ptr(self._arena), ptr(self._u), ptr(self._w_rf), ptr(self._ghat), f32(self.feature_scale),
                                   C.c_void_p(g + 4 * K * D), C.c_void_p(g + 4 * (K * D + Cd)), ptr(self._gp_scratch), B, K, Cd, D, s),
              "uvit_op_gp_ln_grad")
        return self._clip_and_update(lr, weight_decay, max_norm)

    # ---- evaluation ----
    @contextlib.contextmanager
    def _mean_field(self, mean_field):
        """`mean_field` in force (self._mf) for the _logits_into calls of one loop."""
        mf = float(mean_field)
        if not mf >= 0.0:
            raise native.UvitError(f"mean_field must be >= 0, got {mean_field}")
        self._mf = mf
        try:
            yield
        finally:
            self._mf = 0.0

    DETECT_COLUMNS = LinearProbe.DETECT_COLUMNS + ("gp_var",)

    def fit_temperature(self, loader, mean_field=0.0, **kw):
        """LinearProbe.fit_temperature on the GP logits, on the mean-field logits with `mean_field` > 0: give the factor of the
        evaluation the temperature is meant for, so that the fit sees the logits that evaluation sees."""
        with self._mean_field(mean_field):
            return super().fit_temperature(loader, **kw)

    def fit_conformal(self, loader, alpha=0.1, mean_field=0.0, **kw):
        """LinearProbe.fit_conformal on the GP logits, on the mean-field logits with `mean_field` > 0 (as fit_temperature)."""
        with self._mean_field(mean_field):
            return super().fit_conformal(loader, alpha, **kw)

    def evaluate_conformal(self, loader, sizes=False, temperature=None, mean_field=0.0):
        """LinearProbe.evaluate_conformal on the GP logits, on the mean-field logits with `mean_field` > 0."""
        with self._mean_field(mean_field):
            return super().evaluate_conformal(loader, sizes=sizes, temperature=temperature)

    def evaluate(self, loader, calibration=False, variance=False, mean_field=0.0, detection=False, ood_loader=None, temperature=None):
        """LinearProbe.evaluate on the GP logits; the precision matrix is not touched.  `variance`: the result gains `gp_var_mean`, the
        mean predictive variance over the set, from per-batch device slabs read after the last batch.  `mean_field` > 0: loss,
        accuracy, calibration and the detection scores are computed from edward2's mean-field logits z / sqrt(1 + mean_field * var)
        (an addition: the reference has no such step); 0 leaves the logits as they are.  `detection`, `ood_loader`: as
        LinearProbe.evaluate, with the predictive variance as the column `gp_var` whatever `variance` says.  `temperature`: as
        LinearProbe.evaluate, applied behind the mean-field step; `gp_var` and `gp_var_mean` do not depend on it."""
        with self._mean_field(mean_field):
            return self._evaluate_with_mean("gp_var_mean", variance, loader, calibration=calibration, detection=detection,
                                            ood_loader=ood_loader, temperature=temperature)

    def evaluate_stability(self, loader, frames, noise, n_sequences=None, mean_field=0.0):
        """LinearProbe.evaluate_stability on the GP logits, on the mean-field logits with `mean_field` > 0."""
        with self._mean_field(mean_field):
            return super().evaluate_stability(loader, frames, noise, n_sequences=n_sequences)

    _OPT_KEYS = ("head._gp_output_layer.weight", "head._gp_input_normalize_layer.weight", "head._gp_input_normalize_layer.bias")
