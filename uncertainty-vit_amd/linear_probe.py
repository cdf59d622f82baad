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
from .probe_conformal import CP_KINDS, CP_MAX_A, CP_MAX_K, CP_MAX_N, CP_TABLE, ConformalMixin                               # noqa: F401
from .probe_density import MAHA_COLUMNS, MAHA_MAX_C, MAHA_MAX_K, MAHA_SHRINKAGE, DensityMethods, FeatureDensity           # noqa: F401
from .probe_detect import DETECT_KEYS, DETECT_MAX_N, DETECT_MAX_S, DetectionMixin                                         # noqa: F401
from .probe_neighbours import KNN_COLUMNS, KNN_K, KNN_MAX_C, KNN_MAX_K, KNN_MAX_N, KNN_TEMPERATURE, NeighbourBank, NeighbourMethods  # noqa: F401
from .probe_setcalib import SCAL_CLASS_KEYS, SCAL_DEFAULTS, SCAL_KEYS, SCAL_MAX_BINS, SCAL_MAX_N, SCAL_MAX_NK, SetCalibrationMixin  # noqa: F401
from .probe_stability import STABILITY_MAX_FRAMES, StabilityMixin                                                         # noqa: F401
from .probe_temperature import TS_MAX_ITER, TS_MAX_N, TS_STATUS, TS_T_MAX, TS_T_MIN, TS_TOL, TemperatureMixin             # noqa: F401
from .probe_util import column_mean, labelled_batches, ws_size
from .probe_vim import VIM_COLUMNS, VimMethods, VimScore, vim_default_dim                                                # noqa: F401

__all__ = ["LinearProbe", "build_probe_encoder", "load_encoder_checkpoint"]

CALIB_MAX_BINS = 64          # csrc/calib.hip: 1 <= n_bins <= 64, 1 <= B <= 1024
ECE_BINS, TACE_BINS, TACE_THRESHOLD = 15, 30, 0.01      # the reference's defaults (uncertainty_evaluations.py:200,243)


def _timm_trunc_normal_(t, std):
    """timm's trunc_normal_(t, std=std) as modeling_finetune.py:439 calls it: bounds a = -2, b = 2."""
    lo = (1.0 + math.erf(-2.0 / std / math.sqrt(2.0))) / 2.0
    hi = (1.0 + math.erf(2.0 / std / math.sqrt(2.0))) / 2.0
    with torch.no_grad():
        t.uniform_(2 * lo - 1, 2 * hi - 1).erfinv_().mul_(std * math.sqrt(2.0)).clamp_(-2.0, 2.0)
    return t


class LinearProbe(DetectionMixin, SetCalibrationMixin, DensityMethods, NeighbourMethods, VimMethods, TemperatureMixin, ConformalMixin, StabilityMixin, nn.Module):
    """`encoder`: a VisionTransformerForCyclicalTraining in .eval() (it is NOT a sub-module: state_dict() holds `head.weight`
    (K, C) and `head.bias` (K,), the reference's keys).  Owns the head, gradient and Adam moment arenas.  The post-hoc families are
    the mixins of probe_detect.py, probe_setcalib.py, probe_temperature.py, probe_conformal.py and probe_stability.py; the three feature-side scores
    are objects (probe_density.py, probe_neighbours.py, probe_vim.py) that `_scores` holds in the order of their detection columns."""

    BETAS, EPS = (0.9, 0.999), 1e-8          # create_optimizer's adamw defaults (optim_factory.py:133-134)
    # per-sample uncertainty columns of evaluate(detection=True), larger = more uncertain: the three of uvit_op_detect_rows on the
    # logits; a head with an uncertainty of its own appends its columns
    DETECT_COLUMNS = ("msp", "entropy", "energy")
    TWO_STREAM = False                       # the encoder family the class reads: True in DistProbe (dist_probe.py) alone
    # training-time mixing (enable_mix): the mixer, and (partner, lam) on the device while the running train_step's batch is mixed
    _mixer, _mix, _mix_bufs = None, None, None
    # training-time RandAugment (enable_randaug): the augmenter and the buffers of uvit_op_randaug_batch
    _augmenter, _ra_bufs = None, None

    def __init__(self, encoder, num_classes, smoothing=0.1, init_scale=0.001):
        super().__init__()
        if getattr(encoder, "_two_stream", False) and not self.TWO_STREAM:
            raise NotImplementedError("the linear probe reads the base model; the two-stream (mean, covariance) model is not supported")
        if self.TWO_STREAM and not getattr(encoder, "_two_stream", False):
            raise TypeError("encoder must be a DistVisionTransformerForCyclicalTraining: the two-stream probe reads the covariance stream")
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
        # set-level calibration: the settings while it is enabled, the store of the running evaluation, the metrics' workspace
        self._scal, self._scal_eval, self._scal_ws = None, None, None
        # post-hoc temperature: host (T, s) of the fitted or set value, its device table, the table of the running evaluation, the
        # fit's workspace.  Plain attributes: state_dict() does not see them
        self._ts, self._ts_table, self._ts_on, self._ts_ws = None, None, None, None
        # conformal sets: the fitted or set state (settings and the device table of uvit_op_cp_quantile) and the quantile's workspace
        self._cp, self._cp_ws = None, None
        # the feature-side scores, and those of them that the running evaluate(detection=True) stores: (score, {"correct", "slabs"})
        self._density, self._bank, self._vim_score = FeatureDensity(self), NeighbourBank(self), VimScore(self)
        self._scores, self._score_eval = (self._density, self._bank, self._vim_score), ()
        self._var_slabs = None                   # a head's own column, kept for its mean by _evaluate_with_mean
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

    _OPT_KEYS = ("head.weight", "head.bias")     # the names of _views() in a checkpoint's optimizer state

    def _views(self):
        """(parameter, lo, hi, shape) of every trained parameter, in arena order."""
        K, Cd = self.num_classes, self.embed_dim
        return ((self.head.weight, 0, K * Cd, (K, Cd)), (self.head.bias, K * Cd, K * Cd + K, (K,)))

    def _rebind(self):
        for p, lo, hi, shape in self._views():
            p.data = self._arena[lo:hi].view(shape)
            p.grad = self._grad_arena[lo:hi].view(shape)

    def _apply(self, fn, recurse=True):
        new = fn(self._arena)
        if new.dtype != torch.float32:
            raise NotImplementedError("the head stays fp32")
        self._arena = new.contiguous()
        self._grad_arena, self.exp_avg, self.exp_avg_sq = (fn(t).contiguous() for t in (self._grad_arena, self.exp_avg, self.exp_avg_sq))
        self._buf_batch = self._calib_batch = self._rank_rows = self._seq_rows = 0
        self._det_ws = self._scal_ws = self._ts_table = self._ts_ws = self._cp = self._cp_ws = None
        for score in self._scores:                   # a density and a ViM fit stay float64 (their host parts stay on the host), a bank bf16
            score.moved(new.device)
        self._rebind()
        return self

    def _need_gpu(self, what):
        if self._arena.device.type != "cuda":
            raise native.UvitError(f"{what} as HIP kernels: move the encoder and the probe to a GPU (no CPU fallback)")

    def _check_logits(self, logits, rows):
        """Caller-supplied logits (`rows`, K) fp32 on the GPU; returns the number of rows."""
        if not torch.is_tensor(logits) or not logits.is_cuda:
            raise native.UvitError("logits must be a GPU tensor: the HIP path has no CPU fallback")
        if logits.dtype != torch.float32 or logits.ndim != 2 or logits.shape[1] != self.num_classes or not logits.is_contiguous():
            raise native.UvitError(f"logits must be a contiguous float32 tensor of shape ({rows}, {self.num_classes})")
        return logits.shape[0]

    def _check_feat(self, feat):
        """Caller-supplied features (B, C) fp32 on the GPU, B >= 1; returns B."""
        if not torch.is_tensor(feat) or not feat.is_cuda:
            raise native.UvitError("feat must be a GPU tensor: the HIP path has no CPU fallback")
        if feat.dtype != torch.float32 or feat.ndim != 2 or feat.shape[1] != self.embed_dim or not feat.is_contiguous() or not feat.shape[0]:
            raise native.UvitError(f"feat must be a contiguous float32 tensor of shape (B, {self.embed_dim})")
        return feat.shape[0]

    def _head_buffers_for(self, B):
        """The buffers of a subclass's head for batches of up to B rows (allocated with the probe's own, forgotten with them)."""

    def _buffers_for(self, B, calibration=False):
        """Caller-allocated device buffers of the probe's launches, grown to the largest batch seen; with `calibration`, those of the
        calibration ops (csrc/calib.hip) as well."""
        self._need_gpu("the linear probe runs")
        dev = self._arena.device
        if B > self._buf_batch:
            K, Cd, N = self.num_classes, self.embed_dim, self.encoder.patch_embed.num_patches + 1
            ws = ws_size(lib().uvit_op_probe_pool_ws_bytes, B, N, Cd)
            z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)      # noqa: E731
            self._scratch, self._feat, self._logits, self._dlogits = z(ws // 4), z(B, Cd), z(B, K), z(B, K)
            self._row_loss = z(B)
            self._stats = z(2)                       # {loss, grad norm} of the last train_step
            self._sumsq = z(1, dt=torch.float64)
            self._head_buffers_for(B)
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

    def _bias_ptr(self, arena):
        """The biases of an arena laid out as the head's: behind the decay group, the weights."""
        return C.c_void_p(arena.data_ptr() + 4 * self._n_decay)

    def _logits_into(self, B):
        K, Cd = self.num_classes, self.embed_dim
        check(lib().uvit_op_probe_logits(ptr(self._feat), ptr(self._arena), self._bias_ptr(self._arena), ptr(self._logits), B, K, Cd,
                                         cur_stream()), "uvit_op_probe_logits")

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
    def enable_mix(self, mixer):
        """Random erasing, mixup and cutmix of every training batch (probe_mix.BatchMixer; None switches it off): train_step draws
        with iteration = step_count, runs uvit_op_mix_batch into a buffer of the probe's in front of the encoder and takes
        uvit_op_probe_ce_mix for its loss.  A step whose draw is not active makes the calls of a probe without a mixer and gives
        its bits.  Evaluation is untouched."""
        if mixer is not None and not callable(getattr(mixer, "draw", None)):
            raise TypeError("enable_mix takes a probe_mix.BatchMixer or None")
        self._mixer, self._mix = mixer, None

    def mix_images(self, images, draw):
        """uvit_op_mix_batch on `images` (B, 3, S, S) fp32 on the GPU under a probe_mix.MixDraw, seeded with the mixer's seed and
        iteration = step_count: the mixed batch, a buffer of the probe's that the next call overwrites.  Leaves (partner, lam) of the
        draw on the device for the criterion of the running step."""
        self._check_images(images)
        if images.dtype != torch.float32 or images.ndim != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3] or \
                not images.is_contiguous():
            raise native.UvitError("mixing needs contiguous float32 images of shape (B, 3, S, S)")
        B, S, R = images.shape[0], images.shape[2], draw.boxes.shape[1]
        L, dev = lib(), images.device
        need = L.uvit_op_mix_ws_bytes(B, R)
        if need < 0:
            check(need, "uvit_op_mix_ws_bytes")
        bufs = self._mix_bufs
        if bufs is None or bufs["out"].shape != images.shape or bufs["out"].device != dev or bufs["ws"].numel() < need:
            # the host arrays are read by asynchronous copies: four pinned slots, each guarded by the event of the step that used it
            bufs = self._mix_bufs = {"out": torch.empty_like(images), "ws": torch.empty(need, dtype=torch.uint8, device=dev),
                                     "labels": torch.empty(8 * B, dtype=torch.uint8, device=dev), "slots": [], "at": 0}
        if len(bufs["slots"]) < 4:
            bufs["slots"].append({"event": torch.cuda.Event(), "host": None})
        slot = bufs["slots"][bufs["at"] % len(bufs["slots"])]
        bufs["at"] += 1
        slot["event"].synchronize()                  # returns at once unless the stream is four steps behind
        # [descriptors | erase boxes | partner int32[B] | lam float32[B]]: the first two are the op's host arguments, the last two
        # the device arguments of uvit_op_probe_ce_mix
        parts = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in (draw.desc, draw.boxes, draw.partner, draw.lam)]
        pack = np.concatenate(parts)
        if slot["host"] is None or slot["host"].numel() < pack.size:
            slot["host"] = torch.empty(pack.size, dtype=torch.uint8).pin_memory()
        slot["host"].numpy()[:pack.size] = pack
        host, off = slot["host"].data_ptr(), parts[0].size + parts[1].size
        seed = int(getattr(self._mixer, "seed", 0)) & 0xFFFFFFFF
        check(L.uvit_op_mix_batch(ptr(images), ptr(bufs["out"]), C.c_void_p(host), C.c_void_p(host + parts[0].size) if R else None, B, S, R,
                                  int(draw.erase_mode), seed, self.step_count & 0xFFFFFFFF, ptr(bufs["ws"]), bufs["ws"].numel(), cur_stream()),
              "uvit_op_mix_batch")
        bufs["labels"].copy_(slot["host"][off:off + 8 * B], non_blocking=True)
        slot["event"].record()
        self._mix = (bufs["labels"][:4 * B].view(torch.int32), bufs["labels"][4 * B:].view(torch.float32))
        return bufs["out"]

    def enable_randaug(self, aug):
        """RandAugment of every training batch (probe_randaug.RandAugmenter; None switches it off): train_step draws with iteration =
        step_count and runs uvit_op_randaug_batch into a buffer of the probe's in front of the mixer and the encoder -- timm's order,
        auto-augment in front of RandomErasing and Mixup.  It changes no label, so every head takes it.  A step whose draw is not
        active makes the calls of a probe without an augmenter and gives its bits.  Evaluation is untouched."""
        if aug is not None and not (callable(getattr(aug, "draw", None)) and hasattr(aug, "mean") and hasattr(aug, "std")):
            raise TypeError("enable_randaug takes a probe_randaug.RandAugmenter or None")
        self._augmenter = aug

    def randaug_images(self, images, draw):
        """uvit_op_randaug_batch on `images` (B, 3, S, S) fp32 on the GPU under a probe_randaug.RandAugDraw, with the augmenter's mean
        and std: the augmented batch, a buffer of the probe's that the next call overwrites."""
        self._check_images(images)
        if images.dtype != torch.float32 or images.ndim != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3] or \
                not images.is_contiguous():
            raise native.UvitError("RandAugment needs contiguous float32 images of shape (B, 3, S, S)")
        if self._augmenter is None:
            raise native.UvitError("randaug_images needs an augmenter for its mean and std: call enable_randaug first")
        B, S = images.shape[0], images.shape[2]
        L, dev = lib(), images.device
        need = L.uvit_op_randaug_ws_bytes(B, S)
        if need < 0:
            check(need, "uvit_op_randaug_ws_bytes")
        bufs = self._ra_bufs
        if bufs is None or bufs["out"].shape != images.shape or bufs["out"].device != dev or bufs["ws"].numel() < need:
            # the descriptors are read by an asynchronous copy: four pinned slots, each guarded by the event of the step that used it
            bufs = self._ra_bufs = {"out": torch.empty_like(images), "ws": torch.empty(need, dtype=torch.uint8, device=dev), "slots": [], "at": 0}
        if len(bufs["slots"]) < 4:
            bufs["slots"].append({"event": torch.cuda.Event(), "host": None})
        slot = bufs["slots"][bufs["at"] % len(bufs["slots"])]
        bufs["at"] += 1
        slot["event"].synchronize()                  # returns at once unless the stream is four steps behind
        pack = np.ascontiguousarray(draw.desc).view(np.uint8).reshape(-1)
        if slot["host"] is None or slot["host"].numel() < pack.size:
            slot["host"] = torch.empty(pack.size, dtype=torch.uint8).pin_memory()
        slot["host"].numpy()[:pack.size] = pack
        mean, std = (C.c_float * 3)(*self._augmenter.mean), (C.c_float * 3)(*self._augmenter.std)
        check(L.uvit_op_randaug_batch(ptr(images), ptr(bufs["out"]), C.c_void_p(slot["host"].data_ptr()), B, S, mean, std, ptr(bufs["ws"]),
                                      bufs["ws"].numel(), cur_stream()), "uvit_op_randaug_batch")
        slot["event"].record()
        return bufs["out"]

    def _train_images(self, images):
        """The batch a train_step feeds the encoder: `images`, behind RandAugment where an augmenter's draw of this step is active,
        then, with a mixer whose draw of this step is active, their mix."""
        self._mix = None
        if self._augmenter is not None:
            self._check_images(images)
            draw = self._augmenter.draw(images.shape[0], images.shape[-1], self.step_count)
            if draw.active:
                images = self.randaug_images(images, draw)
        if self._mixer is None:
            return images
        self._check_images(images)
        draw = self._mixer.draw(images.shape[0], images.shape[-1], self.step_count)
        return self.mix_images(images, draw) if draw.active else images

    def _criterion(self, labels, B):
        """The training loss of self._logits[:B] into self._dlogits, self._row_loss and self._stats[0]: the smoothed cross-entropy,
        or, while the step's batch is mixed, the soft-target one of the two labels of every row."""
        L, K, s = lib(), self.num_classes, cur_stream()
        if self._mix is None:
            check(L.uvit_op_probe_ce(ptr(self._logits), ptr(labels), f32(self.smoothing), ptr(self._dlogits), ptr(self._row_loss),
                                     ptr(self._stats), None, B, K, s), "uvit_op_probe_ce")
            return
        partner, lam = self._mix
        self._mix = None
        check(L.uvit_op_probe_ce_mix(ptr(self._logits), ptr(labels), ptr(partner), ptr(lam), f32(self.smoothing), ptr(self._dlogits),
                                     ptr(self._row_loss), ptr(self._stats), B, K, s), "uvit_op_probe_ce_mix")

    def train_step(self, images, labels, lr, weight_decay, max_norm=None):
        """One step on the head: forward, smoothed cross-entropy, head gradients, global-norm clip (max_norm) + AdamW.  Returns
        (loss, grad_norm) as device scalars, valid until the next step; nothing synchronises with the host.  A non-finite loss
        (an out-of-range label) makes the gradients non-finite and uvit_op_adamw then leaves the head untouched.  `step_count`
        (Adam's bias correction) counts calls: the host cannot know of a skipped update without reading the loss, so a caller that
        sees a non-finite loss stops, as the reference and run_linear_probe.py do, or takes the call back with `step_count -= 1`.
        With a mixer (enable_mix) the batch is erased and mixed first and the loss is the soft-target one."""
        B = self._features(self._train_images(images))
        labels = self._labels(labels, B)
        K, Cd, L, s = self.num_classes, self.embed_dim, lib(), cur_stream()
        self._logits_into(B)
        self._criterion(labels, B)
        check(L.uvit_op_probe_head_grad(ptr(self._dlogits), ptr(self._feat), ptr(self._grad_arena), self._bias_ptr(self._grad_arena), B, K, Cd,
                                        s), "uvit_op_probe_head_grad")
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
        B = self._check_logits(logits, "B")
        labels = self._labels(labels, B)
        self._buffers_for(B, calibration=True)
        self._calibration_into(logits, labels, B, self._calib_out.data_ptr(), ece_bins, tace_bins, tace_threshold, reference_bin_accuracy)
        o = self._calib_out
        return o[0], o[2], o[1], o[3] / o[4]

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
        While a ViM fit is set (fit_vim, load_vim_state), detection also stores the columns `vim` and `residual` of every batch's
        features, the OOD images' included, behind those, and stats gains "vim_mean" (the mean of `vim` over the evaluation rows that
        are not NaN) and "vim_acc1" (the accuracy in percent of the head the fit took its snapshot of, counted on the device: it
        differs from acc1 when the head was trained on after the fit).  The post-hoc temperature does not reach `vim`.
        `temperature`: None launches and returns exactly the above.  True applies the fitted or set post-hoc temperature
        (fit_temperature, set_temperature; an error when there is none), a number applies that T: uvit_op_ts_scale then runs in place
        on the logits directly behind every _logits_into of the evaluation, the OOD images included, with 1 / T read from a device
        table, so loss, accuracy counters, the calibration ops and the three detection columns of the logits (msp, entropy, energy)
        see z / T, and stats gains "temperature".  Not scaled, because they are formed before the combination or do not depend on the
        scale of the logits: the members' own lines and the ens_* columns of an ensemble, gp_var, het_var, and everything
        evaluate_stability reports (ranks do not depend on T).
        While set-level calibration is enabled (enable_set_calibration), every labelled batch also writes softmax of its logits --
        behind the temperature and a head's own link -- and its labels into a device store, one uvit_op_scal_metrics call runs behind
        the last batch, and stats gains "set_calibration" = {ECE, MCE, OE, NLL, Brier, SCE, ACE, TACE, AUROC, auroc_classes, acc,
        mean_conf, n, n_bad, "reliability": [[prop, acc, conf], ...], "per_class": {SCE, ACE, TACE, AUROC, n_pos,
        n_over_threshold}}: the values of the evaluation set itself, textbook bin accuracies.  OOD images take no part."""
        detection = bool(detection) or ood_loader is not None
        with self._ts_scope(temperature) as ts_value:
            self._det = {"scores": None, "flags": None, "cap": 0, "n": 0} if detection else None
            self._score_eval = [(score, {"correct": None, "slabs": []}) for score in self._scores if detection and score.state is not None]
            self._scal_eval = {"probs": None, "labels": None, "cap": 0, "n": 0} if self._scal is not None else None
            try:
                stats = self._evaluate(loader, calibration, ood_loader)
                if ts_value is not None:
                    stats["temperature"] = ts_value
                return stats
            finally:
                self._det, self._in_ood, self._score_eval, self._scal_eval = None, False, (), None

    def _evaluate_with_mean(self, key, want, loader, **kw):
        """LinearProbe.evaluate for a head with a per-sample column of its own (_own_column(..., self._var_slabs)): with `want`, the
        evaluation rows of the column are kept on the device and stats gains `key`, their mean, read after the last batch."""
        self._var_slabs = [] if want else None
        try:
            stats = LinearProbe.evaluate(self, loader, **kw)
            if want:
                stats[key] = column_mean(self._var_slabs)
            return stats
        finally:
            self._var_slabs = None

    def _evaluate(self, loader, calibration, ood_loader):
        detection = self._det is not None
        losses, sizes, counters = [], [], None
        calib = []
        for images, labels, B in labelled_batches(self, loader):
            if counters is None:
                counters = torch.zeros(2, dtype=torch.int32, device=images.device)
            if len(losses) % 256 == 0:
                slab = torch.zeros(256, dtype=torch.float32, device=images.device)
            if detection:
                self._det_reserve(B)
                for score, ev in self._score_eval:
                    if ev["correct"] is None:
                        ev["correct"] = torch.zeros(1, dtype=torch.int32, device=images.device)
                    score.eval_batch(B, labels, ev)
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
            if self._scal_eval is not None:
                self._scal_rows(B, labels)
            losses.append((slab, len(losses) % 256))
            sizes.append(B)
        scal = self._scal_launch() if self._scal_eval is not None else None       # before the OOD images reuse self._logits
        if detection:
            mis, ood, n_ood = self._det_launch(sum(sizes), ood_loader)
        if not sizes:
            empty = {"loss": float("nan"), "acc1": float("nan"), "acc5": float("nan"), "n": 0}
            if calibration:
                empty.update({k: float("nan") for k in ("ECE", "TACE", "NLL", "AUROC", "AUROC_zero_absent")})
            if detection:
                empty["detection"] = self._det_stats(mis, ood, 0, 0, n_ood, ood_loader is not None)
            for score, ev in self._score_eval:
                empty.update(score.eval_stats(ev, 0))
            if self._scal_eval is not None:
                empty["set_calibration"] = self._scal_stats(None)
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
        for score, ev in self._score_eval:                                  # read with the counters, after the last batch
            stats.update(score.eval_stats(ev, n))
        if self._scal_eval is not None:
            stats["set_calibration"] = self._scal_stats(scal)
        return stats

    # ---- optimizer state beside the head's parameters in a checkpoint ----
    def optimizer_state_dict(self):
        cut = lambda t: {k: t[lo:hi].view(shape).cpu().clone() for k, (_, lo, hi, shape) in zip(self._OPT_KEYS, self._views())}  # noqa: E731
        return {"step": self.step_count, "exp_avg": cut(self.exp_avg), "exp_avg_sq": cut(self.exp_avg_sq)}

    def load_optimizer_state_dict(self, sd):
        self.step_count = int(sd["step"])
        for arena, key in ((self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq")):
            for k, (_, lo, hi, shape) in zip(self._OPT_KEYS, self._views()):
                arena[lo:hi].view(shape).copy_(sd[key][k])


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
