"""Test helper: the four corruptions of csrc/corrupt_ext.hip restated on the host (include/uvit.h), numpy only.

`corrupt(u8, kind, severity, seed, index0, dt)` follows the op's operation order: with dt=np.float32 every + - * / is numpy's IEEE
float32 one, evaluated as the kernels write it (one accumulator per output, taps ascending), so the levels are the kernels' byte for
byte; with dt=np.float64 the same formulas run in double on the same fp32 tables (the tables are the definition): the yardstick the
float32 form is measured against.  `pixelate` is integer arithmetic and has one form.  The tables are restated here from their
definitions, independently of uncertainty_vit_amd.corruptions_ext (tests/test_host_corrupt_ext.py compares the two)."""
import math

import numpy as np

from corrupt_ref import M32, hash32, normalise, set_seed  # noqa: F401  (normalise: the op's last step, for the tests)

KINDS = ("pixelate", "jpeg_compression", "motion_blur", "zoom_blur")
CONSTANTS = {
    "pixelate": (0.6, 0.5, 0.4, 0.3, 0.25),
    "jpeg_compression": (25, 18, 15, 10, 7),
    "motion_blur": ((10, 3), (15, 5), (15, 8), (15, 12), (20, 15)),
    "zoom_blur": ((0.01, 11), (0.01, 16), (0.02, 11), (0.02, 13), (0.03, 11)),
}
BASE_KINDS = 9                      # the ext kinds continue the numbering of the nine in the image key
ANGLES = 91                         # whole degrees, theta = a - 45
PRECISION_BITS = 22                 # Pillow's Resample.c: 32 - 8 - 2
# the IJG tables of the JPEG standard's annex K, natural (row-major) order
IJG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
IJG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def smooth_noise_image(S, seed=7):
    """The tests' fixed image (3, S, S) uint8: three smooth planes (two sinusoids and a ramp) plus Gaussian noise of 12 levels."""
    yy, xx = np.mgrid[0:S, 0:S] / S
    base = np.stack([128 + 100 * np.sin(5 * xx + 2 * yy), 128 + 100 * np.cos(4 * yy - xx), 255 * (xx + yy) / 2])
    return np.clip(base + np.random.default_rng(seed).normal(0, 12, (3, S, S)), 0, 255).astype(np.uint8)


# ---- the tables ----
def box_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BOX filter over the whole axis: (bounds (out, 2) = first input and
    count, coefficients (out, ksize) as 22-bit fixed point, zero past the count)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 0.5 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kk = np.zeros((out_size, 2), dtype=np.int32), np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [1.0 if -0.5 < (x + xmin - center + 0.5) * ss <= 0.5 else 0.0 for x in range(xmax)]
        ww = sum(w)
        w = [k / ww if ww != 0.0 else k for k in w]
        bounds[xx] = xmin, xmax
        kk[xx, :xmax] = [int(0.5 + k * (1 << PRECISION_BITS)) for k in w]
    return bounds, kk


def pixelate_size(severity, S):
    return int(S * CONSTANTS["pixelate"][severity - 1])


def pixelate_table(severity, S):
    n = pixelate_size(severity, S)
    (bd, kd), (bu, ku) = box_coeffs(S, n), box_coeffs(n, S)
    return np.concatenate([bd.ravel(), kd.ravel(), bu.ravel(), ku.ravel()]).astype(np.int32), n


def jpeg_quant_tables(quality):
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (force_baseline): (luma, chroma), 64 integers each."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.array([min(max((b * s + 50) // 100, 1), 255) for b in base], dtype=np.int64) for base in (IJG_LUMA, IJG_CHROMA))


def dct_basis():
    """T[u][x] = c(u) / 2 cos((2 x + 1) u pi / 16), c(0) = 1 / sqrt 2, else 1: in double."""
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    return np.where(u == 0, math.sqrt(0.5), 1.0) / 2.0 * np.cos((2.0 * x + 1.0) * u * math.pi / 16.0)


def jpeg_table(severity):
    ql, qc = jpeg_quant_tables(CONSTANTS["jpeg_compression"][severity - 1])
    return np.concatenate([dct_basis().ravel(), ql.astype(np.float64), qc.astype(np.float64)]).astype(np.float32)


def motion_table(severity):
    """[w_0 .. w_R, then per angle a = 0 .. 90: ox_0 .. ox_R, oy_0 .. oy_R] as fp32 (the offsets are whole numbers)."""
    R, sigma = CONSTANTS["motion_blur"][severity - 1]
    i = np.arange(R + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * sigma * sigma))
    w /= w.sum()
    rows = [w]
    for a in range(ANGLES):
        th = math.radians(a - 45)
        rows += [np.rint(i * math.cos(th)), np.rint(i * math.sin(th))]
    return np.concatenate(rows).astype(np.float32), R


def zoom_table(severity):
    step, n = CONSTANTS["zoom_blur"][severity - 1]
    return (1.0 / (1.0 + np.arange(n, dtype=np.float64) * step)).astype(np.float32), n


def table(kind, severity, S):
    """(the op's table of 4-byte words, the op's integer argument)."""
    if kind == "pixelate":
        return pixelate_table(severity, S)
    if kind == "jpeg_compression":
        return jpeg_table(severity), 0
    if kind == "motion_blur":
        return motion_table(severity)
    if kind == "zoom_blur":
        return zoom_table(severity)
    raise ValueError(kind)


def motion_angle(seed, severity, index):
    """a of image `index` of the set: ((h(key ^ 0x1B873593) >> 8) 91) >> 24."""
    kseed = int(hash32(set_seed(seed, severity) ^ (((BASE_KINDS + KINDS.index("motion_blur") + 1) * 0x9E3779B9) & M32)))
    ikey = int(hash32(kseed ^ (((index + 1) * 0x85EBCA6B) & M32)))
    return ((int(hash32(ikey ^ 0x1B873593)) >> 8) * ANGLES) >> 24


# ---- the kinds ----
def box_pass(img, bounds, kk, axis):
    """One pass of Pillow's ImagingResample on a uint8 plane along `axis`: clip8((2^21 + sum pix k) >> 22)."""
    x = np.moveaxis(img.astype(np.int64), axis, -1)
    out = np.empty(x.shape[:-1] + (len(bounds),), dtype=np.int64)
    for o, (xmin, cnt) in enumerate(bounds):
        out[..., o] = ((1 << (PRECISION_BITS - 1)) + (x[..., xmin:xmin + cnt] * kk[o, :cnt].astype(np.int64)).sum(axis=-1)) >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), -1, axis)


def pixelate(u8, severity):
    """(.., S, S) uint8 -> levels: horizontal then vertical, down to n and up again."""
    S = u8.shape[-1]
    n = pixelate_size(severity, S)
    (bd, kd), (bu, ku) = box_coeffs(S, n), box_coeffs(n, S)
    t = box_pass(box_pass(u8, bd, kd, -1), bd, kd, -2)
    return box_pass(box_pass(t, bu, ku, -1), bu, ku, -2)


def _dct_pass(T, blocks, axis, dt):
    """out[.., k, ..] = sum_j T[k, j] in[.., j, ..] along `axis` of (.., 8, 8) blocks, j ascending into one accumulator from 0."""
    x = np.moveaxis(blocks, axis, -1)
    out = np.zeros(x.shape, dtype=dt)
    for k in range(8):
        acc = np.zeros(x.shape[:-1], dtype=dt)
        for j in range(8):
            acc = acc + T[k, j] * x[..., j]
        out[..., k] = acc
    return np.moveaxis(out, -1, axis)


def _codec(plane, T, Q, dt):
    """(P, P) samples -> the reconstructed samples: per 8x8 block the DCT of p - 128 along x then y, rint(F / Q) Q, the inverse along
    y then x, + 128."""
    P = plane.shape[0]
    b = (plane - dt(128)).reshape(P // 8, 8, P // 8, 8).transpose(0, 2, 1, 3)            # (by, bx, y, x)
    F = _dct_pass(T, _dct_pass(T, b, -1, dt), -2, dt)                                    # (by, bx, v, u)
    Fq = np.rint(F / Q) * Q
    r = _dct_pass(T.T, _dct_pass(T.T, Fq, -2, dt), -1, dt) + dt(128)
    return r.transpose(0, 2, 1, 3).reshape(P, P)


def _upsample(c, dt, hc):
    """(h, h) -> (2 h, 2 h): 0.75 near + 0.25 far, the far sample replicated at the edge of the image's hc x hc chroma samples, vertical
    then horizontal."""
    h = c.shape[0]
    fine = np.arange(2 * h)
    near, far = fine >> 1, np.clip((fine >> 1) + np.where(fine & 1, 1, -1), 0, hc - 1)
    v = dt(0.75) * c[near] + dt(0.25) * c[far]
    return dt(0.75) * v[:, near] + dt(0.25) * v[:, far]


def jpeg_image(u8, severity, dt=np.float32, raw=False):
    """(3, S, S) uint8 -> levels (3, S, S); with `raw`, the values the clip and floor are taken of."""
    S = u8.shape[-1]
    P = (S + 15) // 16 * 16
    tab = jpeg_table(severity).astype(dt)
    T, QL, QC = tab[:64].reshape(8, 8), tab[64:128].reshape(8, 8), tab[128:].reshape(8, 8)
    # past the image: columns and luminance rows repeat the last one; chrominance rows repeat the last PAIR, (S - 1) & ~1 and its
    # successor (clamped), so that the subsampled plane repeats its last row -- libjpeg's padding of a subsampled component
    line = np.arange(P)
    edge, pair = np.minimum(line, S - 1), np.where(line < S, line, np.minimum(((S - 1) & ~1) + (line & 1), S - 1))
    r, g, b = u8[:, edge][:, :, edge].astype(dt)
    rc, gc, bc = u8[:, pair][:, :, edge].astype(dt)
    f = lambda c: dt(np.float32(c))                                                      # noqa: E731  the kernels' fp32 constants
    y = (f(0.299) * r + f(0.587) * g) + f(0.114) * b
    cb = ((f(-0.168736) * rc - f(0.331264) * gc) + f(0.5) * bc) + dt(128)
    cr = ((f(0.5) * rc - f(0.418688) * gc) - f(0.081312) * bc) + dt(128)
    # a JPEG sample is an 8-bit level: the three planes are rounded before anything else reads them, and the 2 x 2 mean is libjpeg's
    # integer one, floor((sum + bias) / 4) with bias 1 in the even and 2 in the odd chroma columns (whole numbers: exact in both forms)
    level = lambda c: np.floor(np.minimum(np.maximum(c, dt(0)), dt(255)) + dt(0.5))      # noqa: E731
    y, cb, cr = level(y), level(cb), level(cr)
    bias = np.where(np.arange(P // 2) & 1, dt(2), dt(1)).astype(dt)
    sub = lambda c: np.floor((((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) + bias) * dt(0.25))      # noqa: E731
    hc = (S + 1) // 2
    y, cb, cr = _codec(y, T, QL, dt), _upsample(_codec(sub(cb), T, QC, dt), dt, hc), _upsample(_codec(sub(cr), T, QC, dt), dt, hc)
    cb, cr = cb - dt(128), cr - dt(128)
    x = np.stack([y + f(1.402) * cr, (y - f(0.344136) * cb) - f(0.714136) * cr, y + f(1.772) * cb])[:, :S, :S]
    if raw:
        return x
    return np.floor(np.minimum(np.maximum(x, dt(0)), dt(255)) + dt(0.5)).astype(np.uint8)


def _quantise(v, dt):
    return np.floor(np.minimum(np.maximum(v, dt(0)), dt(1)) * dt(255) + dt(0.5)).astype(np.uint8)


def motion_image(u8, severity, angle, dt=np.float32, raw=False):
    S = u8.shape[-1]
    tab, R = motion_table(severity)
    w = tab[:R + 1].astype(dt)
    ox = tab[(R + 1) * (1 + 2 * angle):][:R + 1].astype(int)
    oy = tab[(R + 1) * (2 + 2 * angle):][:R + 1].astype(int)
    v = u8.astype(dt) / dt(255)
    yy, xx = np.arange(S)[:, None], np.arange(S)[None, :]
    acc = np.zeros(v.shape, dtype=dt)
    for i in range(R + 1):
        acc = acc + w[i] * v[:, np.clip(yy - oy[i], 0, S - 1), np.clip(xx - ox[i], 0, S - 1)]
    return acc if raw else _quantise(acc, dt)


def zoom_image(u8, severity, dt=np.float32, raw=False):
    S = u8.shape[-1]
    tab, n = zoom_table(severity)
    v = u8.astype(dt) / dt(255)
    c = dt(np.float32(S - 1) / np.float32(2))
    p = np.arange(S).astype(dt)
    acc = v.copy()
    for j in range(n):
        s = c + (p - c) * dt(tab[j])
        i0 = np.clip(np.floor(s).astype(int), 0, S - 1)
        i1 = np.minimum(i0 + 1, S - 1)
        fr = s - i0.astype(dt)
        fy, fx = fr[:, None], fr[None, :]
        top = v[:, i0][:, :, i0] + (v[:, i0][:, :, i1] - v[:, i0][:, :, i0]) * fx
        bot = v[:, i1][:, :, i0] + (v[:, i1][:, :, i1] - v[:, i1][:, :, i0]) * fx
        acc = acc + (top + (bot - top) * fy)
    r = acc / dt(np.float32(n + 1))
    return r if raw else _quantise(r, dt)


def corrupt_image(u8, kind, severity, seed, index, dt=np.float32, raw=False):
    if kind == "pixelate":
        return pixelate(u8, severity)
    if kind == "jpeg_compression":
        return jpeg_image(u8, severity, dt, raw)
    if kind == "motion_blur":
        return motion_image(u8, severity, motion_angle(seed, severity, index), dt, raw)
    if kind == "zoom_blur":
        return zoom_image(u8, severity, dt, raw)
    raise ValueError(kind)


def corrupt(u8, kind, severity, seed=0, index0=0, dt=np.float32, raw=False):
    """A batch (B, 3, S, S) uint8 whose first image is image `index0` of the set -> the levels (B, 3, S, S) uint8."""
    return np.stack([corrupt_image(u8[b], kind, severity, seed, index0 + b, dt, raw) for b in range(u8.shape[0])])
