"""ImageNet-C-style corruptions generated on the device (csrc/corrupt.hip): the host side of the corruption
sweep of run_linear_probe.py (`--eval --corruptions ...`, the reference's c_evaluate()).

The clean evaluation images are decoded and augmented once, packed to planar uint8 on the device (uvit_op_corrupt_pack, 150 KB per
224-pixel image) and kept in a `CleanCache`; every (corruption, severity) set is then a `CorruptedSet`, an iterable of
(images, labels) on the device that `LinearProbe.evaluate` takes as its loader: one uvit_op_corrupt_batch per batch in front of the
encoder forward.  The severity constants are those of Hendrycks & Dietterich's generator for 224-pixel images as remembered, NOT
verified against it: results are ImageNet-C-style, not the published benchmark (section 9.16).  There is no host fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import native, probe_util
from .native import check, cur_stream, lib, ptr

# the kinds in the order of include/uvit.h (UVIT_CORRUPT_*): the position is the id
CORRUPTIONS = ("gaussian_noise", "speckle_noise", "impulse_noise", "shot_noise", "brightness", "saturate", "contrast", "gaussian_blur",
               "defocus_blur")
SEVERITIES = (1, 2, 3, 4, 5)
# c of severity 1 .. 5 (section 9.16's table)
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
MAX_RADIUS = 24
SHOT_TAIL = 2.0 ** -25          # kmax: the smallest k whose double CDF reaches 1 - SHOT_TAIL
DEFAULT_CACHE_IMAGES = 65536


def kind_id(kind):
    if kind not in CORRUPTIONS:
        raise ValueError(f"unknown corruption {kind!r}: one of {', '.join(CORRUPTIONS)}")
    return CORRUPTIONS.index(kind)


def constant(kind, severity):
    """The table's c of (kind, severity): a number or a pair."""
    kind_id(kind)
    if severity not in SEVERITIES:
        raise ValueError(f"severity {severity!r} outside 1 .. 5")
    return CONSTANTS[kind][severity - 1]


def set_seed(seed, severity):
    """The seed uvit_op_corrupt_batch takes for a set: --corruption_seed with the severity mixed in (the op adds the kind and the
    image's index)."""
    x = (int(seed) ^ (int(severity) * 0x9E3779B9)) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def shot_tables(c):
    """(p0[256], kmax[256]) in double for lambda = fp32(u8 / 255) * fp32(c): exp(-lambda), and the smallest k whose CDF, summed in
    double by the recurrence p_k = p_{k-1} lambda / k, reaches 1 - 2^-25."""
    lam = ((np.arange(256, dtype=np.float32) / np.float32(255.0)) * np.float32(c)).astype(np.float64)
    p0 = np.exp(-lam)
    kmax = np.zeros(256, dtype=np.float64)
    for i in range(256):
        k, p, F = 0, p0[i], p0[i]
        while F < 1.0 - SHOT_TAIL:
            k += 1
            p = p * lam[i] / k
            F += p
        kmax[i] = k
    return p0, kmax


def gaussian_taps(sigma):
    """scipy's gaussian_filter(truncate=4): radius int(4 sigma + 0.5), exp(-i^2 / (2 sigma^2)) normalised, in double."""
    R = int(4.0 * sigma + 0.5)
    i = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return w / w.sum()


def defocus_taps(radius, alias):
    """The (2R+1)^2 defocus kernel in double, R = max(8, radius): the normalised indicator of x^2 + y^2 <= radius^2, blurred by a separable
    3-tap (radius <= 8) or 5-tap Gaussian of sigma = alias with reflect-101 border, and normalised again (the reflecting border does not
    keep the sum where the disk touches the edge)."""
    R = max(8, int(radius))
    i = np.arange(-R, R + 1)
    disk = ((i[:, None] ** 2 + i[None, :] ** 2) <= int(radius) ** 2).astype(np.float64)
    disk /= disk.sum()
    n = 3 if radius <= 8 else 5
    j = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    g = np.exp(-(j * j) / (2.0 * alias * alias))
    g /= g.sum()
    h = n // 2
    for axis in (0, 1):
        pad = np.pad(disk, [(h, h) if a == axis else (0, 0) for a in (0, 1)], mode="reflect")
        disk = sum(g[t] * np.take(pad, np.arange(t, t + 2 * R + 1), axis=axis) for t in range(n))
    return disk / disk.sum()


def corruption_params(kind, severity, S):
    """The fp32 table uvit_op_corrupt_batch reads for (kind, severity) at image size S (include/uvit.h lists the layouts), a numpy array.
    Formed in double, cast once.  A blur whose radius does not fit (R >= S or R > 24) is refused here as it is by the op."""
    c = constant(kind, severity)
    if not 8 <= int(S) <= 1024:
        raise ValueError(f"image size {S} outside [8, 1024]")
    if kind == "shot_noise":
        p0, kmax = shot_tables(c)
        table = np.concatenate([[c], p0, kmax])
    elif kind == "gaussian_blur":
        table = gaussian_taps(c)
    elif kind == "defocus_blur":
        table = defocus_taps(*c).ravel()
    else:
        table = np.atleast_1d(np.asarray(c, dtype=np.float64))
    if kind in ("gaussian_blur", "defocus_blur"):
        R = (int(round(math.sqrt(table.size))) if kind == "defocus_blur" else table.size) // 2
        if R >= S or R > MAX_RADIUS:
            raise ValueError(f"{kind} severity {severity}: radius {R} does not fit an image of {S} pixels (R < S, R <= {MAX_RADIUS})")
    return table.astype(np.float32)


# ---- the three library calls (they live here and nowhere else) ----
def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _check_u8(t, name):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != t.shape[3] \
            or not t.is_contiguous():
        raise native.UvitError(f"{name} must be a contiguous uint8 GPU tensor of shape (B, 3, S, S)")


def _check_f32(t, name):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != t.shape[3] \
            or not t.is_contiguous():
        raise native.UvitError(f"{name} must be a contiguous float32 GPU tensor of shape (B, 3, S, S)")


def pack(images, mean, std, out=None):
    """uvit_op_corrupt_pack on the current stream: the normalised fp32 (B, 3, S, S) images as planar uint8."""
    _check_f32(images, "images")
    B, _, S, _ = images.shape
    if out is None:
        out = torch.empty((B, 3, S, S), dtype=torch.uint8, device=images.device)
    _check_u8(out, "out")
    if out.shape != images.shape:
        raise native.UvitError("pack: out must have the shape of images")
    check(lib().uvit_op_corrupt_pack(ptr(images), B, S, _f3(mean), _f3(std), ptr(out), cur_stream()), "uvit_op_corrupt_pack")
    return out


def corrupt(owner, images_u8, kind, params, seed, index0, mean, std, out=None):
    """uvit_op_corrupt_batch on the current stream; `params` is the DEVICE table of corruption_params, `seed` the set's (set_seed),
    `owner` keeps the workspace (`_corrupt_ws`, grown on demand)."""
    _check_u8(images_u8, "images_u8")
    B, _, S, _ = images_u8.shape
    if not torch.is_tensor(params) or not params.is_cuda or params.dtype != torch.float32 or not params.is_contiguous():
        raise native.UvitError("params must be a contiguous float32 GPU tensor (corruption_params(...) on the device)")
    if out is None:
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=images_u8.device)
    _check_f32(out, "out")
    if out.shape != images_u8.shape:
        raise native.UvitError("corrupt: out must have the shape of images_u8")
    k = kind_id(kind)
    ws = probe_util.workspace(owner, "_corrupt_ws", images_u8.device, lib().uvit_op_corrupt_ws_bytes, k, B, S, name="uvit_op_corrupt_ws_bytes")
    check(lib().uvit_op_corrupt_batch(ptr(images_u8), ptr(out), B, S, k, ptr(params), params.numel(), int(seed) & 0xFFFFFFFF, int(index0),
                                      _f3(mean), _f3(std), ptr(ws) if ws.numel() else None, ws.numel(), cur_stream()), "uvit_op_corrupt_batch")
    return out


class CleanCache:
    """The device uint8 images and labels of the evaluation set, filled by the first CorruptedSet that reads the folder and replayed
    by the later ones.  At most `limit` images: a larger folder is dropped (`overflowed`) and every set reads the folder again.
    Iterating a `ready` cache yields (uint8 batch, labels, index0) in batches of `batch_size`, views of the store."""

    def __init__(self, limit=DEFAULT_CACHE_IMAGES, batch_size=64):
        if limit < 0 or batch_size < 1:
            raise ValueError("CleanCache: limit >= 0 and batch_size >= 1")
        self.limit, self.batch_size = int(limit), int(batch_size)
        self.reset()

    def reset(self):
        self._store, self.n, self.ready, self.overflowed = None, 0, False, False

    @property
    def device(self):
        return self._store[0].device if self._store is not None else None

    def append(self, images_u8, labels):
        """A batch behind the ones held; past the limit everything is dropped and the cache stays empty."""
        if self.overflowed:
            return
        if self.ready:
            raise native.UvitError("CleanCache.append: the cache is complete; reset() it first")
        B, _, S, _ = images_u8.shape
        if self.n + B > self.limit:
            self._store, self.n, self.overflowed = None, 0, True
            return
        specs = (((None, 3, S, S), torch.uint8, 0), ((None,), torch.int64, 0))
        self._store = probe_util.grown(self._store, self.n, self.n + B, self.limit, "CleanCache: over its limit", specs, images_u8.device)
        self._store[0][self.n:self.n + B].copy_(images_u8)
        self._store[1][self.n:self.n + B].copy_(labels)
        self.n += B

    def finish(self):
        """The folder has been read to its end: the cache may be replayed (unless it overflowed)."""
        self.ready = not self.overflowed

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        if not self.ready:
            raise native.UvitError("CleanCache: nothing to replay (not filled to the end, or over its limit)")
        for i0 in range(0, self.n, self.batch_size):
            i1 = min(i0 + self.batch_size, self.n)
            yield self._store[0][i0:i1], self._store[1][i0:i1], i0


class CorruptedSet:
    """One (corruption, severity) set as a loader of LinearProbe.evaluate: yields (images, labels), both on the device, the images
    corrupted by uvit_op_corrupt_batch, or by uvit_op_corrupt_ext_batch for a kind of corruptions_ext.CORRUPTIONS_EXT.  `source` is a DevicePrefetcher over the evaluation loader -- each of its batches is packed to
    uint8 (uvit_op_corrupt_pack) and appended to `cache` when one is given, which is marked complete behind the last batch -- or a
    ready CleanCache.  Both launches go on the current stream.  The bytes of a set depend on (kind, severity, seed) and the image's
    position in the set, not on the batch size or on which of the two sources it is read from."""

    def __init__(self, source, kind, severity, seed, mean, std, cache=None):
        from . import corruptions_ext as ext
        self.source, self.kind, self.severity, self.cache = source, kind, int(severity), cache
        self.seed, self.mean, self.std = set_seed(seed, severity), tuple(mean), tuple(std)
        self._params, self._params_size, self._params_device, self._corrupt_ws = None, None, None, None
        # the family: the nine of this module, or the four of corruptions_ext.py (a table object with .to(device), another op)
        self._ext = ext if kind in ext.CORRUPTIONS_EXT else None
        (ext.ext_constant if self._ext else constant)(kind, self.severity)

    def __len__(self):
        return len(self.source)

    def _batches(self):
        if isinstance(self.source, CleanCache):
            yield from self.source
            return
        if self.cache is not None:
            self.cache.reset()
        index0 = 0
        for item in self.source:
            images, labels = item
            if isinstance(images, (tuple, list)):
                images = images[0]
            if not labels.is_cuda:
                labels = labels.to(images.device, non_blocking=True)
            u8 = pack(images, self.mean, self.std)
            if self.cache is not None:
                self.cache.append(u8, labels)
            yield u8, labels, index0
            index0 += u8.shape[0]
        if self.cache is not None:
            self.cache.finish()

    def __iter__(self):
        for u8, labels, index0 in self._batches():
            S = u8.shape[-1]
            if self._params is None or self._params_device != u8.device or self._params_size != S:
                if self._ext:
                    self._params = self._ext.ext_params(self.kind, self.severity, S).to(u8.device)
                else:
                    self._params = torch.from_numpy(corruption_params(self.kind, self.severity, S)).to(u8.device)
                self._params_size, self._params_device = S, u8.device
            op = self._ext.corrupt_ext if self._ext else corrupt
            yield op(self, u8, self.kind, self._params, self.seed, index0, self.mean, self.std), labels
