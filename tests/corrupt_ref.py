"""Test helper: the corruptions of csrc/corrupt.hip restated on the host (include/uvit.h).

`corrupt(u8, kind, severity, seed, index0, dtype)` follows the op's operation order; with dtype=np.float32 every + - * / is numpy's
IEEE float32 one, evaluated as the kernel writes it, so the quantised image is the kernel's byte for byte for every kind but the two
Box-Muller ones (numpy's float32 log / cos / sqrt are not the device's).  With dtype=np.float64 the same formulas run in double on the
same fp32 parameter table (the table is the definition; p0 of shot_noise is the double exp(-lambda)): the yardstick the float32 form
and the device's Box-Muller draws are measured against.  The hash and the uniforms are exact integers in both.  The parameter tables
are restated here from their definitions, independently of uncertainty_vit_amd.corruptions (tests/test_host_corrupt.py compares the two)."""
import numpy as np

M32 = 0xFFFFFFFF
KINDS = ("gaussian_noise", "speckle_noise", "impulse_noise", "shot_noise", "brightness", "saturate", "contrast", "gaussian_blur",
         "defocus_blur")
CONSTANTS = {
    "gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38),
    "speckle_noise": (0.15, 0.2, 0.35, 0.45, 0.6),
    "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27),
    "shot_noise": (60.0, 25.0, 12.0, 5.0, 3.0),
    "brightness": (0.1, 0.2, 0.3, 0.4, 0.5),
    "saturate": ((0.3, 0.0), (0.1, 0.0), (2.0, 0.0), (5.0, 0.1), (20.0, 0.2)),
    "contrast": (0.4, 0.3, 0.2, 0.1, 0.05),
    "gaussian_blur": (1.0, 2.0, 3.0, 4.0, 6.0),
    "defocus_blur": ((3, 0.1), (4, 0.5), (6, 0.5), (8, 0.5), (10, 0.5)),
}


def hash32(x):
    """uvit_hash32 of csrc/common.h on numpy uint64 arrays (or ints) holding 32-bit values: exact."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def set_seed(seed, severity):
    return int(hash32((int(seed) ^ (int(severity) * 0x9E3779B9)) & M32))


def draw_keys(seed, kind, severity, index):
    """(k1, k2) of image `index` of the set."""
    kseed = int(hash32(set_seed(seed, severity) ^ (((KINDS.index(kind) + 1) * 0x9E3779B9) & M32)))
    ikey = int(hash32(kseed ^ (((index + 1) * 0x85EBCA6B) & M32)))
    return int(hash32(ikey ^ 0x1B873593)), int(hash32(ikey ^ 0xCC9E2D51))


def hashes(seed, kind, severity, index, S):
    """(h1, h2) of every value of image `index`: uint64 arrays (3, S, S), the counter is (c S + y) S + x."""
    k1, k2 = draw_keys(seed, kind, severity, index)
    ctr = np.arange(3 * S * S, dtype=np.uint64).reshape(3, S, S)
    return hash32(ctr ^ np.uint64(k1)), hash32(ctr ^ np.uint64(k2))


def uniforms(h1, h2, dt):
    """u1 = ((h1 >> 8) + 1) 2^-24 in (0, 1], u2 = (h2 >> 8) 2^-24 in [0, 1): exact in float32 and float64."""
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(dt) * dt(2.0 ** -24)
    u2 = (h2 >> np.uint64(8)).astype(dt) * dt(2.0 ** -24)
    return u1, u2


def normals(h1, h2, dt):
    """The Box-Muller cosine branch; in float32 with the kernel's float32 2 pi."""
    u1, u2 = uniforms(h1, h2, dt)
    two_pi = dt(np.float32(6.2831854820251465)) if dt is np.float32 else dt(2.0 * np.pi)
    return np.sqrt(dt(-2.0) * np.log(u1)) * np.cos(two_pi * u2)


# ---- the parameter tables, from their definitions in double ----
def gaussian_taps(sigma):
    R = int(4.0 * sigma + 0.5)
    w = np.exp(-np.arange(-R, R + 1, dtype=np.float64) ** 2 / (2.0 * sigma ** 2))
    return w / w.sum()


def defocus_taps(radius, alias):
    """Indicator of x^2 + y^2 <= r^2 on [-R, R]^2, R = max(8, r), normalised; a separable 3-tap (r <= 8) or 5-tap Gaussian of sigma =
    alias over it with reflect-101 border (scipy's mode="mirror"); normalised."""
    from scipy import ndimage
    R = max(8, radius)
    y, x = np.mgrid[-R:R + 1, -R:R + 1]
    k = (x * x + y * y <= radius * radius).astype(np.float64)
    k /= k.sum()
    n = 3 if radius <= 8 else 5
    g = np.exp(-(np.arange(n) - (n - 1) / 2.0) ** 2 / (2.0 * alias ** 2))
    g /= g.sum()
    k = ndimage.correlate1d(ndimage.correlate1d(k, g, axis=0, mode="mirror"), g, axis=1, mode="mirror")
    return k / k.sum()


def shot_tables(c):
    """p0 = exp(-lambda) and kmax (the smallest k with P(X <= k) >= 1 - 2^-25) for lambda = fp32(u8 / 255) * fp32(c), in double."""
    from scipy import stats
    lam = ((np.arange(256, dtype=np.float32) / np.float32(255.0)) * np.float32(c)).astype(np.float64)
    return lam, np.exp(-lam), stats.poisson.ppf(1.0 - 2.0 ** -25, lam)


def params(kind, severity):
    """The op's fp32 table of (kind, severity)."""
    c = CONSTANTS[kind][severity - 1]
    if kind == "shot_noise":
        _, p0, kmax = shot_tables(c)
        return np.concatenate([[c], p0, kmax]).astype(np.float32)
    if kind == "gaussian_blur":
        return gaussian_taps(c).astype(np.float32)
    if kind == "defocus_blur":
        return defocus_taps(*c).ravel().astype(np.float32)
    return np.atleast_1d(np.asarray(c, dtype=np.float64)).astype(np.float32)


# ---- the kinds ----
def quantise(v, dt):
    return np.floor(np.minimum(np.maximum(v, dt(0)), dt(1)) * dt(255) + dt(0.5))


def normalise(q, mean, std):
    """((q / 255) - mean[c]) / std[c] in float32, the augmentation's formula: what the op writes for the levels q (.., 3, S, S)."""
    q = np.asarray(q).astype(np.float32)
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    return (q / np.float32(255.0) - m) / s


def convolve(x, taps, reflect, dt):
    """(S, S) -> (S, S): every output adds its taps dy ascending, then dx ascending, into one accumulator, acc = acc + (t x); zero taps
    are skipped.  Border: reflect-101 or replicate."""
    kh, kw = taps.shape
    S = x.shape[0]
    pad = np.pad(x, ((kh // 2, kh // 2), (kw // 2, kw // 2)), mode="reflect" if reflect else "edge")
    acc = np.zeros((S, S), dtype=dt)
    for dy in range(kh):
        for dx in range(kw):
            t = dt(taps[dy, dx])
            if t != 0:
                acc = acc + t * pad[dy:dy + S, dx:dx + S]
    return acc


def poisson_inverse(u, lam, p0, kmax, dt):
    """k = 0, p = F = p0; while u > F and k < kmax: k += 1, p = (p lam) / k, F = F + p -- on arrays, every step in `dt`."""
    k = np.zeros(u.shape, dtype=dt)
    p, F = p0.astype(dt).copy(), p0.astype(dt).copy()
    while True:
        go = (u > F) & (k < kmax)
        if not go.any():
            return k
        k = np.where(go, k + dt(1), k)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(go, (p * lam) / np.where(go, k, dt(1)), p)
        F = np.where(go, F + p, F)


def corrupt_image(u8, kind, severity, seed, index, dt=np.float32, raw=False):
    """One image (3, S, S) uint8, image `index` of the set -> the quantised levels (3, S, S) as uint8; with `raw`, what the floor is taken
    of instead: clip(v', 0, 1) 255 + 0.5 in `dt`."""
    S = u8.shape[-1]
    table = params(kind, severity)
    P = table.astype(dt)                                     # the fp32 table, widened for the float64 form
    v = u8.astype(dt) / dt(255)
    if kind in ("gaussian_noise", "speckle_noise"):
        z = normals(*hashes(seed, kind, severity, index, S), dt)
        r = v + P[0] * z if kind == "gaussian_noise" else v + (v * P[0]) * z
    elif kind == "impulse_noise":
        h, _ = hashes(seed, kind, severity, index, S)
        t = float(np.float32(table[0])) * 4294967296.0       # uvit_drop_threshold: the product in double
        thr = np.uint64(M32 if t >= 4294967295.0 else int(t))
        r = np.where(h < (thr >> np.uint64(1)), dt(1), np.where(h < thr, dt(0), v))
    elif kind == "shot_noise":
        h, _ = hashes(seed, kind, severity, index, S)
        u, _ = uniforms(h, h, dt)
        lam = v * P[0]
        if dt is np.float32:
            p0, kmax = P[1:257][u8], np.minimum(P[257:513], dt(512))[u8]
        else:
            _, p0_d, kmax_d = shot_tables(CONSTANTS[kind][severity - 1])
            p0, kmax = p0_d[u8], np.minimum(kmax_d, 512.0)[u8]
        r = np.minimum(poisson_inverse(u, lam, p0, kmax, dt) / P[0], dt(1))
    elif kind == "brightness":
        m = v.max(axis=0)
        m2 = np.minimum(m + P[0], dt(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(m == 0, m2, v * (m2 / m))
    elif kind == "saturate":
        m, mn = v.max(axis=0), v.min(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(m == 0, dt(0), (m - mn) / m)
            s2 = np.minimum(np.maximum(s * P[0] + P[1], dt(0)), dt(1))
            colour = m - (m - v) * (s2 / s)
        grey = np.stack([m, m * (dt(1) - s2), m * (dt(1) - s2)])
        r = np.where(s > 0, colour, grey)
    elif kind == "contrast":
        total = u8.reshape(3, -1).astype(np.int64).sum(axis=1)
        mu = (total / (255.0 * S * S)).astype(dt).reshape(3, 1, 1)
        r = (v - mu) * P[0] + mu
    elif kind == "gaussian_blur":
        r = np.stack([convolve(convolve(v[c], P.reshape(-1, 1), False, dt), P.reshape(1, -1), False, dt) for c in range(3)])
    elif kind == "defocus_blur":
        side = int(round(np.sqrt(P.size)))
        r = np.stack([convolve(v[c], P.reshape(side, side), True, dt) for c in range(3)])
    else:
        raise ValueError(kind)
    r = r.astype(dt)
    if raw:
        return np.minimum(np.maximum(r, dt(0)), dt(1)) * dt(255) + dt(0.5)
    return quantise(r, dt).astype(np.uint8)


def corrupt(u8, kind, severity, seed=0, index0=0, dt=np.float32, raw=False):
    """A batch (B, 3, S, S) uint8 whose first image is image `index0` of the set."""
    return np.stack([corrupt_image(u8[b], kind, severity, seed, index0 + b, dt, raw) for b in range(u8.shape[0])])
