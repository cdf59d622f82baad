"""Host side of the probe's RandAugment: what one step draws for uvit_op_randaug_batch (include/uvit.h, csrc/randaug.hip; DESIGN.md
section 9.21).  Pure numpy and math: no device, no torch.

The rules are timm 0.3 / 0.4's `rand_augment_transform` / `RandAugment` / `AugmentOp` (auto_augment.py), which
run_class_finetuning.py:117 reaches through create_transform with `--aa rand-m9-mstd0.5-inc1`, AS REMEMBERED: timm is not available
where this was written, so the rules below are the definition here and DESIGN.md states them in full.  What an op does to the pixels is
Pillow's and is reproduced bit for bit on the device; which ops an image gets is drawn here.
The generator is numpy.random.Generator(PCG64) seeded from (seed, iteration, 2) -- streams 0 and 1 are probe_mix.py's -- so a draw is a
function of (seed, iteration) alone and a resumed run draws what the uninterrupted run would have drawn.  It is NOT timm's global
random / np.random stream; no run of the reference is reproduced draw for draw.
"""
import math
import re
from collections import namedtuple

import numpy as np

__all__ = ["RandAugmenter", "RandAugDraw", "RANDAUG_DESC", "RANDAUG_LAYER", "RANDAUG_OPS", "RANDAUG_FILTERS", "MAX_LAYERS", "parse_config"]

# UVIT_RA_*: 0 is "not applied", 1 .. 15 are timm's _RAND_TRANSFORMS in its order
RANDAUG_OPS = ("None", "AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
               "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
RANDAUG_FILTERS = {"nearest": 0, "bilinear": 2, "bicubic": 3}    # UVIT_RA_{NEAREST, BILINEAR, BICUBIC} = PIL.Image.Resampling
INTERPOLATIONS = tuple(RANDAUG_FILTERS) + ("random",)
MAX_LAYERS = 4                                                   # UVIT_RANDAUG_MAX_LAYERS
MAX_LEVEL = 10.0                                                 # timm's _MAX_LEVEL
# uvit_randaug_layer and uvit_randaug_desc, field for field
RANDAUG_LAYER = np.dtype([("op", "<i4"), ("filter", "<i4"), ("arg0", "<i4"), ("arg1", "<i4"), ("factor", "<f4"), ("fill", "<u4"),
                          ("matrix", "<f8", (6,))])
RANDAUG_DESC = np.dtype([("n_layers", "<i4"), ("reserved", "<i4"), ("layers", RANDAUG_LAYER, (MAX_LAYERS,))])

# desc: RANDAUG_DESC[B]; active: False when no image has an op
RandAugDraw = namedtuple("RandAugDraw", ("desc", "active"))

_OP = {name: i for i, name in enumerate(RANDAUG_OPS)}
_ENHANCE = ("Color", "Contrast", "Brightness", "Sharpness")


def parse_config(config):
    """timm's config string `rand[-m<float>][-n<int>][-mstd<float>][-inc<0|1>]` -> {"m", "n", "mstd", "inc"} with timm's defaults
    (m 10, n 2, mstd 0, inc 0).  `w` (weighted op choice) and every policy that is not `rand` are refused as not built."""
    if not isinstance(config, str) or not config:
        raise ValueError("the RandAugment config is a string such as 'rand-m9-mstd0.5-inc1'")
    sections = config.split("-")
    if sections[0] != "rand":
        raise NotImplementedError(f"--aa {config!r}: only RandAugment ('rand-...') is built; 'original', 'v0' and 'augmix' policies are not")
    out = {"m": MAX_LEVEL, "n": 2, "mstd": 0.0, "inc": False}
    for sec in sections[1:]:
        m = re.fullmatch(r"(mstd|inc|m|n|w)(\d+(?:\.\d*)?|\.\d+)", sec)
        if not m:
            raise ValueError(f"--aa {config!r}: cannot read the section {sec!r}")
        key, val = m.group(1), m.group(2)
        if key == "w":
            raise NotImplementedError(f"--aa {config!r}: weighted op choice ('w') is not built")
        if key == "inc":
            if val not in ("0", "1"):
                raise ValueError(f"--aa {config!r}: inc takes 0 or 1")
            out["inc"] = val == "1"
        elif key == "n":
            if not val.isdigit() or not 1 <= int(val) <= MAX_LAYERS:
                raise ValueError(f"--aa {config!r}: n must be a whole number in [1, {MAX_LAYERS}]")
            out["n"] = int(val)
        else:
            out[key] = float(val)
    if not 0.0 <= out["m"] <= MAX_LEVEL:
        raise ValueError(f"--aa {config!r}: m must be in [0, {MAX_LEVEL:g}]")
    return out


def rotate_matrix(degrees, size):
    """Image.rotate(degrees) of a size x size image: its matrix, with Pillow's round(..., 15) of the sine and cosine and the centre
    (size / 2, size / 2); None where Image.rotate returns a copy (a multiple of 360 degrees)."""
    angle = degrees % 360.0
    if angle == 0:
        return None
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    c = size / 2
    m[2], m[5] = m[0] * -c + m[1] * -c + m[2], m[3] * -c + m[4] * -c + m[5]
    m[2] += c
    m[5] += c
    return m


class RandAugmenter:
    """What timm's rand_augment_transform(config, {translate_pct 0.45, img_mean, interpolation}) draws for a batch.
    `mean` and `std` are the normalisation of the images the op will see.  `draw(B, S, iteration)` returns a RandAugDraw."""

    def __init__(self, config, mean, interpolation="bicubic", seed=0, std=(0.5, 0.5, 0.5)):
        cfg = parse_config(config)
        if interpolation not in INTERPOLATIONS:
            raise ValueError(f"interpolation must be one of {INTERPOLATIONS}, got {interpolation!r}")
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(mean) != 3 or len(std) != 3 or not all(math.isfinite(v) for v in mean + std) or not all(std):
            raise ValueError(f"mean and std must be three finite values each and no std 0, got {mean} and {std}")
        self.mean, self.std = mean, std              # the normalisation of the batch: the op quantises with it, the fill colour comes from the mean
        self.config, self.magnitude, self.num_layers, self.magnitude_std, self.increasing = config, cfg["m"], cfg["n"], cfg["mstd"], cfg["inc"]
        self.interpolation, self.seed = interpolation, int(seed)
        self.fill = tuple(max(0, min(255, round(255 * v))) for v in mean)          # timm: min(255, round(255 * x))
        self.prob = 0.5                                                            # of every op, timm's AugmentOp default
        self.translate_pct = 0.45

    def __repr__(self):
        return (f"RandAugment(n={self.num_layers}, m={self.magnitude:g}, mstd={self.magnitude_std:g}, inc={int(self.increasing)}, "
                f"interpolation={self.interpolation}, fill={self.fill})")

    def _rng(self, iteration):
        return np.random.Generator(np.random.PCG64([self.seed & 0xFFFFFFFFFFFFFFFF, int(iteration), 2]))

    @staticmethod
    def _negate(rng, v):
        return -v if rng.random() > 0.5 else v

    def _layer(self, rng, name, level, S, out):
        """Fill `out` (one RANDAUG_LAYER) with op `name` at `level` in [0, 10]: timm's level functions."""
        frac = level / MAX_LEVEL
        out["op"] = _OP[name]
        out["matrix"] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        if name in ("AutoContrast", "Equalize", "Invert"):
            return
        if name in _ENHANCE:
            out["factor"] = 1.0 + self._negate(rng, frac * 0.9) if self.increasing else frac * 1.8 + 0.1
        elif name == "Posterize":
            out["arg0"] = 4 - int(frac * 4) if self.increasing else int(frac * 4)
        elif name == "Solarize":
            out["arg0"] = 256 - int(frac * 256) if self.increasing else int(frac * 256)
        elif name == "SolarizeAdd":
            out["arg0"], out["arg1"] = int(frac * 110), 128
        else:
            if name == "Rotate":
                m = rotate_matrix(self._negate(rng, frac * 30.0), S)
            elif name in ("ShearX", "ShearY"):
                v = self._negate(rng, frac * 0.3)
                m = (1.0, v, 0.0, 0.0, 1.0, 0.0) if name == "ShearX" else (1.0, 0.0, 0.0, v, 1.0, 0.0)
            else:
                v = self._negate(rng, frac * self.translate_pct) * S
                m = (1.0, 0.0, v, 0.0, 1.0, 0.0) if name == "TranslateXRel" else (1.0, 0.0, 0.0, 0.0, 1.0, v)
            flt = self.interpolation
            if flt == "random":
                flt = ("bilinear", "bicubic")[int(rng.integers(0, 2))]
            if m is None:                                        # Image.rotate(0) is a copy
                out["op"], out["matrix"] = 0, 0.0
                return
            out["matrix"], out["filter"] = m, RANDAUG_FILTERS[flt]
            out["fill"] = self.fill[0] | self.fill[1] << 8 | self.fill[2] << 16

    def draw(self, B, S, iteration):
        B, S = int(B), int(S)
        if B < 1 or S < 1:
            raise ValueError(f"B and S must be >= 1, got {B} and {S}")
        desc = np.zeros(B, dtype=RANDAUG_DESC)
        desc["n_layers"] = self.num_layers
        rng = self._rng(iteration)
        for b in range(B):
            ops = rng.integers(1, len(RANDAUG_OPS), size=self.num_layers)          # uniform, with replacement
            for i, op in enumerate(ops):
                if not rng.random() < self.prob:
                    continue                                     # the layer stays "None"
                level = self.magnitude
                if self.magnitude_std > 0.0:
                    level = float(rng.normal(level, self.magnitude_std))
                level = min(MAX_LEVEL, max(0.0, level))
                self._layer(rng, RANDAUG_OPS[int(op)], level, S, desc[b]["layers"][i])
        return RandAugDraw(desc, bool((desc["layers"]["op"] != 0).any()))
