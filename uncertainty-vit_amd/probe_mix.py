"""Host side of the probe's training-time mixing: what one step draws for uvit_op_mix_batch and uvit_op_probe_ce_mix (include/uvit.h,
csrc/mixup.hip).  Pure numpy: no device, no torch.

The definitions are timm 0.3 / 0.4's `Mixup` and `RandomErasing` (run_class_finetuning.py:128-149 passes the flags on) AS REMEMBERED:
timm is not available where this was written, so the formulas below are the definition here and DESIGN.md states them in full.
The generator is numpy.random.Generator(PCG64) seeded from (seed, iteration, stream), stream 0 for the mixing and 1 for the erasing:
a draw is a function of (seed, iteration) alone, so a resumed run draws what the uninterrupted run would have drawn.  It is NOT timm's
global np.random / random / torch stream; no run of the reference is reproduced draw for draw.
"""
import math
from collections import namedtuple

import numpy as np

__all__ = ["BatchMixer", "MixDraw", "MIX_DESC", "MIX_KINDS", "ERASE_MODES", "MIX_MODES", "MAX_BOXES"]

MIX_KINDS = {"none": 0, "mixup": 1, "cutmix": 2}                 # UVIT_MIX_{NONE, MIXUP, CUTMIX}
ERASE_MODES = {"const": 0, "rand": 1, "pixel": 2}                # UVIT_MIX_ERASE_*
MIX_MODES = ("batch", "pair", "elem")
MAX_BOXES = 8                                                    # UVIT_MIX_MAX_BOXES
ERASE_ATTEMPTS, ERASE_MIN_AREA, ERASE_MAX_AREA, ERASE_MIN_ASPECT = 10, 0.02, 1.0 / 3.0, 0.3      # timm RandomErasing's defaults
# uvit_mix_desc, field for field
MIX_DESC = np.dtype([("kind", "<i4"), ("lam", "<f4"), ("partner", "<i4"), ("yl", "<i4"), ("yh", "<i4"), ("xl", "<i4"), ("xh", "<i4"),
                     ("reserved", "<i4")])

# desc: MIX_DESC[B]; boxes: int32 (B, R, 4) = (top, left, h, w), h == 0: none; partner int32[B] and lam float32[B]: the arguments of
# uvit_op_probe_ce_mix (a kind-0 row has lam 1); erase_mode: UVIT_MIX_ERASE_*; active: False when every row is kind 0 without a box
MixDraw = namedtuple("MixDraw", ("desc", "boxes", "partner", "lam", "erase_mode", "active"))

_NONE = (0, 1.0, (0, 0, 0, 0))


class BatchMixer:
    """What timm's Mixup(mixup_alpha, cutmix_alpha, cutmix_minmax, prob, switch_prob, mode) and RandomErasing(reprob, mode=remode,
    max_count=recount) draw for a batch, with label smoothing left to the loss.  `draw(B, S, iteration)` returns a MixDraw."""

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch", reprob=0.0,
                 remode="pixel", recount=1, seed=0):
        if not (mixup_alpha >= 0.0 and cutmix_alpha >= 0.0):
            raise ValueError(f"mixup and cutmix alphas must be >= 0, got {mixup_alpha} and {cutmix_alpha}")
        for name, v in (("prob", prob), ("switch_prob", switch_prob), ("reprob", reprob)):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"{name} must be in [0, 1], got {v}")
        if mode not in MIX_MODES:
            raise ValueError(f"mode must be one of {MIX_MODES}, got {mode!r}")
        if remode not in ERASE_MODES:
            raise ValueError(f"remode must be one of {tuple(ERASE_MODES)}, got {remode!r}")
        if not 1 <= int(recount) <= MAX_BOXES or int(recount) != recount:
            raise ValueError(f"recount must be in [1, {MAX_BOXES}], got {recount}")
        if cutmix_minmax is not None:
            cutmix_minmax = tuple(float(v) for v in cutmix_minmax)
            if len(cutmix_minmax) != 2 or not 0.0 < cutmix_minmax[0] <= cutmix_minmax[1] <= 1.0:
                raise ValueError(f"cutmix_minmax must be two values in (0, 1], ascending, got {cutmix_minmax}")
            cutmix_alpha = 1.0                                   # timm: the min / max form overrides the alpha
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = float(mixup_alpha), float(cutmix_alpha), cutmix_minmax
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode
        self.reprob, self.remode, self.recount, self.seed = float(reprob), remode, int(recount), int(seed)

    @property
    def mixes(self):
        return (self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0) and self.prob > 0.0

    @property
    def enabled(self):
        """False when no draw can ever be active."""
        return self.mixes or self.reprob > 0.0

    def _rng(self, iteration, stream):
        return np.random.Generator(np.random.PCG64([self.seed & 0xFFFFFFFFFFFFFFFF, int(iteration), stream]))

    # ---- mixing ----
    def _cut_box(self, rng, S, lam):
        """(yl, yh, xl, xh) of timm's rand_bbox (or rand_bbox_minmax), rows first."""
        if self.cutmix_minmax is not None:
            lo, hi = int(S * self.cutmix_minmax[0]), int(S * self.cutmix_minmax[1])
            cut_h, cut_w = (int(rng.integers(lo, hi)) if hi > lo else lo for _ in range(2))
            yl = int(rng.integers(0, S - cut_h)) if S > cut_h else 0
            xl = int(rng.integers(0, S - cut_w)) if S > cut_w else 0
            return yl, yl + cut_h, xl, xl + cut_w
        ratio = math.sqrt(1.0 - lam)
        cut_h = cut_w = int(S * ratio)
        cy, cx = int(rng.integers(0, S)), int(rng.integers(0, S))
        clip = lambda v: min(max(v, 0), S)                       # noqa: E731
        return clip(cy - cut_h // 2), clip(cy + cut_h // 2), clip(cx - cut_w // 2), clip(cx + cut_w // 2)

    def _draw_mix(self, rng, S):
        """One (kind, lam, box): timm's _params_per_batch / _params_per_elem for one element.  lam is a double here; a cutmix row's is
        1 - area / S^2 (correct_lam), and a lam that is 1 as a float32 gives kind 0."""
        if not rng.random() < self.prob:
            return _NONE
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = bool(rng.random() < self.switch_prob)
        else:
            cut = self.cutmix_alpha > 0.0
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(rng.beta(alpha, alpha))
        box = (0, 0, 0, 0)
        if cut:
            box = self._cut_box(rng, S, lam)
            lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(S * S)
        if np.float32(lam) == np.float32(1.0):
            return _NONE
        return (MIX_KINDS["cutmix"] if cut else MIX_KINDS["mixup"]), lam, box

    # ---- erasing ----
    def _draw_boxes(self, rng, S, out):
        """timm RandomErasing._erase for one sample: `recount` boxes, each the first of up to ten attempts that fits."""
        if not rng.random() < self.reprob:
            return
        for r in range(self.recount):
            for _ in range(ERASE_ATTEMPTS):
                area = rng.uniform(ERASE_MIN_AREA, ERASE_MAX_AREA) * S * S / self.recount
                aspect = math.exp(rng.uniform(math.log(ERASE_MIN_ASPECT), math.log(1.0 / ERASE_MIN_ASPECT)))
                h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if h < S and w < S:
                    if h > 0 and w > 0:
                        out[r] = (int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w)
                    break

    def draw(self, B, S, iteration):
        B, S = int(B), int(S)
        if B < 1 or S < 1:
            raise ValueError(f"B and S must be >= 1, got {B} and {S}")
        desc = np.zeros(B, dtype=MIX_DESC)
        desc["partner"] = B - 1 - np.arange(B)                   # x.flip(0)
        desc["lam"] = 1.0
        if self.mixes:
            rng = self._rng(iteration, 0)
            if self.mode == "batch":
                rows = [self._draw_mix(rng, S)] * B
            elif self.mode == "elem":
                rows = [self._draw_mix(rng, S) for _ in range(B)]
            else:                                                # pair: the first half draws, the partners mirror; an odd middle row is left alone
                half = [self._draw_mix(rng, S) for _ in range(B // 2)]
                rows = half + [_NONE] * (B % 2) + half[::-1]
            for b, (kind, lam, box) in enumerate(rows):
                desc[b]["kind"], desc[b]["lam"] = kind, lam      # rounded to float32 once, here
                desc[b]["yl"], desc[b]["yh"], desc[b]["xl"], desc[b]["xh"] = box
        R = self.recount if self.reprob > 0.0 else 0
        boxes = np.zeros((B, R, 4), dtype=np.int32)
        if R:
            rng = self._rng(iteration, 1)
            for b in range(B):
                self._draw_boxes(rng, S, boxes[b])
        active = bool((desc["kind"] != 0).any() or (R and (boxes[:, :, 2] > 0).any()))
        return MixDraw(desc, boxes, desc["partner"].astype(np.int32), desc["lam"].astype(np.float32), ERASE_MODES[self.remode], active)
