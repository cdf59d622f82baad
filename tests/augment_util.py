"""NumPy restatement of the arithmetic of csrc/augment.hip: the BEiT augmentation as Pillow computes it
(ImageEnhance on RGB, then the 8-bit separable resampler of Resample.c), then ToTensor + Normalize.

This is the oracle of the GPU tests.  It is itself pinned to Pillow by tests/golden/augment_pil.npz (written by
tools/gen_golden_augment.py from live PIL) and, where PIL is importable, by random cases against PIL directly.

A sample is described by the same fields as uvit_augment_desc (include/uvit.h); `augment(img, d, S, mean, std)` takes the
decoded HWC uint8 image and a mapping with those field names.
"""
import math

import numpy as np

# filter ids = PIL.Image.Resampling values
LANCZOS, BILINEAR, BICUBIC, HAMMING = 1, 2, 3, 5
# jitter op ids = torchvision ColorJitter fn_idx values
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
PRECISION_BITS = 22


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_F054, _F046 = float(np.float32(0.54)), float(np.float32(0.46))     # Resample.c writes 0.54f + 0.46f * cos(x)


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_F054 + _F046 * math.cos(x))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


FILTERS = {BILINEAR: (_bilinear, 1.0), HAMMING: (_hamming, 1.0), BICUBIC: (_bicubic, 2.0), LANCZOS: (_lanczos, 3.0)}


def coeffs(in_size, out_size, flt, first=0, count=None):
    """precompute_coeffs + normalize_coeffs_8bpc of Resample.c for output positions first..first+count-1 of a resize
    in_size -> out_size: (xmin (n,), xlen (n,), k (n, ksize) int32)."""
    fn, support = FILTERS[flt]
    count = out_size if count is None else count
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmins, xlens = np.zeros(count, np.int64), np.zeros(count, np.int64)
    k = np.zeros((count, ksize), np.int32)
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[i, :xmax] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        xmins[i], xlens[i] = xmin, xmax
    return xmins, xlens, k


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass(src, xmins, xlens, k, axis):
    """One 8-bit pass along `axis` (1 = horizontal, 0 = vertical) of an (H, W, 3) uint8 image."""
    src = np.moveaxis(src, axis, 0).astype(np.int32)
    out = np.empty((len(xmins),) + src.shape[1:], np.uint8)
    for i, (x0, n) in enumerate(zip(xmins, xlens)):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
        for t in range(n):
            acc += src[x0 + t] * k[i, t]
        out[i] = _clip8(acc)
    return np.moveaxis(out, 0, axis)


def luma(img):
    """RGB -> L of Pillow's Convert.c (rgb2l)."""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, img, factor):
    """Image.blend(degenerate, img, factor) of Blend.c: float32 d + f * (x - d), clipped, truncated."""
    d = degenerate.astype(np.int32)
    t = d.astype(np.float32) + np.float32(factor) * (img.astype(np.int32) - d).astype(np.float32)
    return np.clip(t, 0, 255).astype(np.uint8)          # t in (0, 255): truncation toward zero = astype


def jitter(img, ops, factors):
    """torchvision ColorJitter on a PIL RGB image, in the given order: ImageEnhance.Brightness / Contrast / Color."""
    for op, f in zip(ops, factors):
        if op == BRIGHTNESS:
            img = blend(np.zeros_like(img), img, f)
        elif op == CONTRAST:
            L = luma(img)
            mean = int(float(L.astype(np.int64).sum()) / L.size + 0.5)
            img = blend(np.full_like(img, mean), img, f)
        elif op == SATURATION:
            img = blend(np.repeat(luma(img)[..., None], 3, axis=2), img, f)
        else:
            raise ValueError(op)
    return img


def resample_window(img, rw, rh, flt, wx, wy, S):
    """img.resize((rw, rh), flt) evaluated on the window [wx, wx+S) x [wy, wy+S) of the result; positions outside the
    resized image are 0 (CenterCrop's padding).  Each pass is skipped when its size is unchanged (ImagingResampleInner)."""
    H, W = img.shape[:2]
    out = np.zeros((S, S, 3), np.uint8)
    x0, x1 = max(wx, 0), min(wx + S, rw)
    y0, y1 = max(wy, 0), min(wy + S, rh)
    if x0 >= x1 or y0 >= y1:
        return out
    if rh != H:
        ymins, ylens, ky = coeffs(H, rh, flt, y0, y1 - y0)
        r0, r1 = int(ymins[0]), int(ymins[-1] + ylens[-1])
    else:
        r0, r1 = y0, y1
    rows = img[r0:r1]
    if rw != W:
        xmins, xlens, kx = coeffs(W, rw, flt, x0, x1 - x0)
        rows = _pass(rows, xmins, xlens, kx, 1)
    else:
        rows = rows[:, x0:x1]
    if rh != H:
        rows = _pass(rows, ymins - r0, ylens, ky, 0)
    out[y0 - wy:y1 - wy, x0 - wx:x1 - wx] = rows
    return out


def to_tensor_normalize(u8, mean, std):
    """ToTensor + Normalize: ((u8 / 255) - mean) / std in float32, (3, S, S)."""
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    m = np.asarray(mean, np.float32).reshape(3, 1, 1)
    s = np.asarray(std, np.float32).reshape(3, 1, 1)
    return (x - m) / s


def augment_u8(img, d, S):
    """Jitter -> flip -> crop -> resize (window) of one HWC uint8 image: the (S, S, 3) uint8 result."""
    n = int(d["n_jitter"])
    img = jitter(img, [int(v) for v in d["jitter_op"][:n]], [float(v) for v in d["jitter_factor"][:n]])
    if d["flip"]:
        img = img[:, ::-1]
    cx, cy, cw, ch = (int(d[k]) for k in ("crop_x", "crop_y", "crop_w", "crop_h"))
    img = np.ascontiguousarray(img[cy:cy + ch, cx:cx + cw])
    return resample_window(img, int(d["resize_w"]), int(d["resize_h"]), int(d["filter"]), int(d["win_x"]), int(d["win_y"]), S)


def augment(img, d, S, mean, std):
    return to_tensor_normalize(augment_u8(img, d, S), mean, std)
