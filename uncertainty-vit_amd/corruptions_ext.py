"""Four more ImageNet-C-style corruptions generated on the device (csrc/corrupt_ext.hip): pixelate,
jpeg_compression, motion_blur and zoom_blur, the second family beside the nine of corruptions.py, whose CorruptedSet dispatches here.

Every kind reads a table of 4-byte words that is formed here once per set, in double or in integers, and cast once (include/uvit.h
lists the layouts); the device adds no transcendental function and nothing per batch.  As in corruptions.py the severity constants are
those of Hendrycks & Dietterich's generator for 224-pixel images as remembered, NOT verified against it, and jpeg_compression,
motion_blur and zoom_blur are this project's definitions of those distortions, not libjpeg's, ImageMagick's or scipy's bytes; pixelate
is Pillow's two BOX resizes bit for bit.  There is no host fallback."""
import math
from typing import NamedTuple

import numpy as np
import torch

from . import native, probe_util
from .corruptions import CORRUPTIONS, SEVERITIES, _check_f32, _check_u8, _f3
from .native import check, cur_stream, lib, ptr

# the kinds in the order of include/uvit.h (UVIT_CORRUPT_EXT_*): the position is the id
CORRUPTIONS_EXT = ("pixelate", "jpeg_compression", "motion_blur", "zoom_blur")
# c of severity 1 .. 5 (section 9.18's table): the share of the side kept, the quality, (R, sigma), (step, n)
CONSTANTS_EXT = {
    "pixelate": (0.6, 0.5, 0.4, 0.3, 0.25),
    "jpeg_compression": (25, 18, 15, 10, 7),
    "motion_blur": ((10, 3), (15, 5), (15, 8), (15, 12), (20, 15)),
    "zoom_blur": ((0.01, 11), (0.01, 16), (0.02, 11), (0.02, 13), (0.03, 11)),
}
ANGLES = 91                     # motion_blur: whole degrees, theta = a - 45
MAX_MOTION_RADIUS = 24
PRECISION_BITS = 22             # Pillow's Resample.c
# the example tables of the JPEG standard (annex K) that libjpeg scales by the quality, in natural order
IJG_LUMINANCE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
IJG_CHROMINANCE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                   99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99)


class ExtTable(NamedTuple):
    """What uvit_op_corrupt_ext_batch reads for one set: the table's words (a numpy array from ext_params; on the device for
    corrupt_ext) and the kind's integer argument, which fixes the table's length."""
    words: object
    arg: int

    def to(self, device):
        return ExtTable(torch.from_numpy(self.words).to(device) if isinstance(self.words, np.ndarray) else self.words.to(device), self.arg)


def ext_kind_id(kind):
    if kind not in CORRUPTIONS_EXT:
        raise ValueError(f"unknown corruption {kind!r}: one of {', '.join(CORRUPTIONS + CORRUPTIONS_EXT)}")
    return CORRUPTIONS_EXT.index(kind)


def ext_constant(kind, severity):
    ext_kind_id(kind)
    if severity not in SEVERITIES:
        raise ValueError(f"severity {severity!r} outside 1 .. 5")
    return CONSTANTS_EXT[kind][severity - 1]


def box_coefficients(in_size, out_size):
    """Resample.c's precompute_coeffs and normalize_coeffs_8bpc for the BOX filter over a whole axis: per output the first input and
    the count, (out_size, 2), and the coefficients as 22-bit fixed point, (out_size, ksize), zero past the count."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 0.5 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, coefs = np.zeros((out_size, 2), dtype=np.int32), np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        k = np.array([1.0 if -0.5 < (x + xmin - center + 0.5) * ss <= 0.5 else 0.0 for x in range(count)])
        if k.sum() != 0.0:
            k = k / k.sum()
        bounds[xx] = xmin, count
        coefs[xx, :count] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in k]
    return bounds, coefs


def jpeg_quantisation(quality):
    """libjpeg's tables for a quality in 1 .. 100: clamp((base s + 50) / 100, 1, 255) in integers, s = 5000 / q below 50, else 200 - 2 q."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.array([min(max((b * s + 50) // 100, 1), 255) for b in base], dtype=np.float64) for base in (IJG_LUMINANCE, IJG_CHROMINANCE))


def dct_basis():
    """T[u][x] = c(u) / 2 cos((2 x + 1) u pi / 16), c(0) = 1 / sqrt 2, c(u > 0) = 1, in double: the orthonormal 8-point DCT-II."""
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    return np.where(u == 0, math.sqrt(0.5), 1.0) / 2.0 * np.cos((2.0 * x + 1.0) * u * math.pi / 16.0)


def motion_rows(radius, sigma):
    """[w, then (ox, oy) of the 91 directions]: w_i = exp(-i^2 / 2 sigma^2) normalised, the offsets rint(i cos), rint(i sin), in double."""
    i = np.arange(radius + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * sigma * sigma))
    rows = [w / w.sum()]
    for a in range(ANGLES):
        theta = math.radians(a - 45)
        rows += [np.rint(i * math.cos(theta)), np.rint(i * math.sin(theta))]
    return rows


def ext_params(kind, severity, S):
    """The ExtTable of (kind, severity) at image size S, its words a numpy array (int32 for pixelate, else float32).  A motion_blur
    whose radius does not fit (R >= S) is refused here as it is by the op."""
    c = ext_constant(kind, severity)
    S = int(S)
    if not 8 <= S <= 1024:
        raise ValueError(f"image size {S} outside [8, 1024]")
    if kind == "pixelate":
        n = int(S * c)
        down, up = box_coefficients(S, n), box_coefficients(n, S)
        return ExtTable(np.concatenate([t.ravel() for t in down + up]).astype(np.int32), n)
    if kind == "jpeg_compression":
        return ExtTable(np.concatenate([dct_basis().ravel(), *jpeg_quantisation(c)]).astype(np.float32), 0)
    if kind == "motion_blur":
        R, sigma = c
        if R >= S or R > MAX_MOTION_RADIUS:
            raise ValueError(f"motion_blur severity {severity}: radius {R} does not fit an image of {S} pixels (R < S, R <= {MAX_MOTION_RADIUS})")
        return ExtTable(np.concatenate(motion_rows(R, sigma)).astype(np.float32), R)
    step, n = c
    return ExtTable((1.0 / (1.0 + np.arange(n, dtype=np.float64) * step)).astype(np.float32), n)


# ---- the library call (the ext family's calls live here and nowhere else) ----
def corrupt_ext(owner, images_u8, kind, table, seed, index0, mean, std, out=None):
    """uvit_op_corrupt_ext_batch on the current stream; `table` is ext_params(...).to(device), `seed` the set's (corruptions.set_seed),
    `owner` keeps the workspace (`_corrupt_ext_ws`, grown on demand)."""
    _check_u8(images_u8, "images_u8")
    B, _, S, _ = images_u8.shape
    k = ext_kind_id(kind)
    words = table.words if isinstance(table, ExtTable) else None
    want = torch.int32 if kind == "pixelate" else torch.float32
    if not torch.is_tensor(words) or not words.is_cuda or words.dtype != want or not words.is_contiguous():
        raise native.UvitError(f"table must be an ExtTable whose words are a contiguous {want} GPU tensor (ext_params(...).to(device))")
    if out is None:
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=images_u8.device)
    _check_f32(out, "out")
    if out.shape != images_u8.shape:
        raise native.UvitError("corrupt_ext: out must have the shape of images_u8")
    ws = probe_util.workspace(owner, "_corrupt_ext_ws", images_u8.device, lib().uvit_op_corrupt_ext_ws_bytes, k, B, S, int(table.arg),
                              name="uvit_op_corrupt_ext_ws_bytes")
    check(lib().uvit_op_corrupt_ext_batch(ptr(images_u8), ptr(out), B, S, k, ptr(words), words.numel(), int(table.arg), int(seed) & 0xFFFFFFFF,
                                          int(index0), _f3(mean), _f3(std), ptr(ws) if ws.numel() else None, ws.numel(), cur_stream()),
          "uvit_op_corrupt_ext_batch")
    return out
