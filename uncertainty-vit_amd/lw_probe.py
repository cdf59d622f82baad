"""Linear probe with learned layer weights: the reference's `run_class_finetuning.py --linear_classifier --learn_layer_weights`
(modeling_finetune.py:433-436, 499-510), DESIGN.md section 9.15.

    frozen encoder (eval forward, native, full depth) -> every block's residual stream pooled: the mean over ALL tokens, cls included
    (`use_cls`: token 0) -> (`layernorm_before_combine`: F.layer_norm without affine, eps 1e-5) -> feat = sum_l softmax(layer_log_weights)_l p_l
    -> one nn.Linear -> (label-smoothing) cross-entropy

`head.weight`, `head.bias` and `layer_log_weights` (depth scalars, zeros at the start) train; no fc_norm follows the mix.  The
engine's forward already leaves every block's residual stream in its workspace, so nothing of the encoder changes: one
uvit_op_lw_pool call reads all of them, uvit_op_lw_combine writes the mixed feature into the buffer a LinearProbe keeps its feature
in, and everything behind it -- the head, the criterion, the evaluation, every post-hoc family -- is a LinearProbe's.  The step adds
the head's third contraction (uvit_op_probe_input_grad) and uvit_op_lw_grad; `layer_log_weights` lies behind the bias in the
no-decay part of the one arena, so the global-norm clip and the AdamW update are the LinearProbe's calls over a longer arena.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import native
from .linear_probe import LinearProbe, _timm_trunc_normal_
from .modeling_cyclical import _Holder
from .native import check, cur_stream, f32, lib, ptr
from .probe_util import ws_size

__all__ = ["LayerWeightedProbe"]

LW_LN_EPS = 1e-5             # F.layer_norm's default (modeling_finetune.py:505), not the encoder's ln_eps


class LayerWeightedProbe(LinearProbe):
    """state_dict() holds `head.weight` (K, C), `head.bias` (K,) and `layer_log_weights` (depth,), the reference's keys.  `use_cls`:
    token 0 of every block instead of the mean over its tokens.  `layernorm_before_combine`: every block's pooled vector is
    normalised (no affine, eps 1e-5) before the mix."""

    _OPT_KEYS = LinearProbe._OPT_KEYS + ("layer_log_weights",)

    def __init__(self, encoder, num_classes, smoothing=0.1, init_scale=0.001, use_cls=False, layernorm_before_combine=False):
        depth = int(getattr(encoder, "depth", 0))
        if not 1 <= depth <= native.MAX_DEPTH:
            raise ValueError(f"the encoder's depth must be in [1, {native.MAX_DEPTH}], got {depth}")
        self.depth, self.use_cls, self.layernorm_before_combine = depth, bool(use_cls), bool(layernorm_before_combine)
        super().__init__(encoder, num_classes, smoothing=smoothing, init_scale=init_scale)

    # ---- arena: [W (K C) | bias (K, padded to 4) | layer_log_weights (L, padded to 4)], the decay group (W) first ----
    def _lw_offset(self):
        return self.num_classes * self.embed_dim + (self.num_classes + 3) // 4 * 4

    def _setup_head(self, init_scale):
        K, Cd, L = self.num_classes, self.embed_dim, self.depth
        self._n_decay = K * Cd
        n = self._lw_offset() + (L + 3) // 4 * 4
        dev = self.encoder._arena.device
        self._arena = torch.zeros(n, dtype=torch.float32, device=dev)
        self._grad_arena = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_count = 0
        lo = self._lw_offset()
        self.head = _Holder()
        self.head.register_parameter("weight", nn.Parameter(self._arena[:K * Cd].view(K, Cd)))
        self.head.register_parameter("bias", nn.Parameter(self._arena[K * Cd:K * Cd + K]))
        self.register_parameter("layer_log_weights", nn.Parameter(self._arena[lo:lo + L]))     # zeros: modeling_finetune.py:436
        self._rebind()
        _timm_trunc_normal_(self.head.weight.data, std=0.02).mul_(init_scale)     # modeling_finetune.py:439-441
        self.head.bias.data.zero_()

    def _views(self):
        lo = self._lw_offset()
        return super()._views() + ((self.layer_log_weights, lo, lo + self.depth, (self.depth,)),)

    def _lw_ptr(self, arena):
        """layer_log_weights (or its gradient) inside an arena laid out as the head's."""
        return C.c_void_p(arena.data_ptr() + 4 * self._lw_offset())

    def load_state_dict(self, state_dict, strict=True, **kw):
        """A LinearProbe's checkpoint has no layer weights and one of another encoder has another number of them: both are refused."""
        if "layer_log_weights" not in state_dict:
            raise KeyError("the checkpoint has no `layer_log_weights`: it is not a --learn_layer_weights probe (a linear probe's head.* alone "
                           "does not resume here)")
        got = tuple(state_dict["layer_log_weights"].shape)
        if got != (self.depth,):
            raise ValueError(f"the checkpoint's `layer_log_weights` has shape {got}: it was trained on an encoder of another depth, this one "
                             f"has {self.depth} blocks")
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _head_buffers_for(self, B):
        Cd, L, dev = self.embed_dim, self.depth, self._arena.device
        N = self.encoder.patch_embed.num_patches + 1
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
        self._pooled, self._dfeat = z(B, L, Cd), z(B, Cd)
        self._lw_scratch = z(ws_size(lib().uvit_op_lw_pool_ws_bytes, B, L, N, Cd) // 4)
        self._lw_rows = z(B, L, dt=torch.float64)          # uvit_op_lw_grad's per-row partials
        self._lw_w = z(L)                                  # softmax(layer_log_weights) of the last forward

    # ---- forward ----
    def _features(self, images):
        """Encoder eval forward, every block pooled, the mix into self._feat[:B] on the current stream; returns B."""
        self._check_images(images)
        B = images.shape[0]
        self._buffers_for(B)
        enc, L, Cd, dl, s = self.encoder, self.depth, self.embed_dim, lib(), cur_stream()
        e = enc.forward_features(images, bool_masked_pos=None, layer_results=None)
        layers = (C.c_void_p * L)(*[dl.uvit_engine_ws_ptr(e.h, b"x", l + 1) for l in range(L)])
        if not all(layers):
            raise native.UvitError("a block's residual stream is missing from the engine workspace")
        N = enc.patch_embed.num_patches + 1
        check(dl.uvit_op_lw_pool(layers, L, ptr(self._pooled), ptr(self._lw_scratch), B, N, Cd, 1 if self.use_cls else 0,
                                 1 if self.layernorm_before_combine else 0, f32(LW_LN_EPS), s), "uvit_op_lw_pool")
        check(dl.uvit_op_lw_combine(ptr(self._pooled), self._lw_ptr(self._arena), ptr(self._feat), ptr(self._lw_w), B, L, Cd, s),
              "uvit_op_lw_combine")
        return B

    def layer_weights(self):
        """softmax(layer_log_weights) as a device tensor (L,) fp32, in block order: the kernel's own softmax, on the current stream."""
        self._need_gpu("the layer weights are formed")
        w = torch.zeros(self.depth, dtype=torch.float32, device=self._arena.device)
        one = torch.zeros(4, dtype=torch.float32, device=self._arena.device)
        # one row of C = 4 columns whose mix nobody reads: the call is made for w_out
        pooled = torch.zeros(self.depth * 4, dtype=torch.float32, device=self._arena.device)
        check(lib().uvit_op_lw_combine(ptr(pooled), self._lw_ptr(self._arena), ptr(one), ptr(w), 1, self.depth, 4, cur_stream()),
              "uvit_op_lw_combine")
        return w

    # ---- training ----
    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        """LinearProbe.train_step plus the gradient of `layer_log_weights`: dfeat = dlogits . W, g_l = <dfeat, p_l>,
        dlog_w_l = w_l (g_l - sum_j w_j g_j), written into the gradient arena before the one clip + AdamW over the whole arena."""
        B = self._features(self._train_images(images))
        labels = self._labels(labels, B)
        K, Cd, L, dl, s = self.num_classes, self.embed_dim, self.depth, lib(), cur_stream()
        self._logits_into(B)
        self._criterion(labels, B)
        check(dl.uvit_op_probe_head_grad(ptr(self._dlogits), ptr(self._feat), ptr(self._grad_arena), self._bias_ptr(self._grad_arena), B, K,
                                         Cd, s), "uvit_op_probe_head_grad")
        check(dl.uvit_op_probe_input_grad(ptr(self._dlogits), ptr(self._arena), ptr(self._dfeat), B, K, Cd, s), "uvit_op_probe_input_grad")
        check(dl.uvit_op_lw_grad(ptr(self._dfeat), ptr(self._pooled), self._lw_ptr(self._arena), self._lw_ptr(self._grad_arena),
                                 ptr(self._lw_rows), B, L, Cd, s), "uvit_op_lw_grad")
        return self._clip_and_update(lr, weight_decay, max_norm)
