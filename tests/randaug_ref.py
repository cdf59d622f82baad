"""NumPy restatement of csrc/randaug.hip (uvit_op_randaug_batch, include/uvit.h): timm's fifteen RandAugment
ops as Pillow computes them on an RGB image, the pack in front of them and the ToTensor + Normalize behind them.

This is the oracle of the GPU tests.  It is itself pinned to Pillow by tests/golden/randaug_pil.npz (written by
tools/gen_golden_randaug.py from live PIL) and, where PIL imports, by random cases against PIL directly (tests/test_host_randaug.py).

    table ops    Invert, Posterize, Solarize, SolarizeAdd from their integers; AutoContrast (double) and Equalize (integers) from the
                 histogram of each channel of the image as it stands
    blend ops    Color, Contrast, Brightness (tests/augment_util.py's Blend.c restatement) and Sharpness, whose degenerate image is
                 ImageFilter.SMOOTH in float32
    affine ops   Geometry.c under a host-made matrix: ImagingGenericTransform in float64 for bilinear and bicubic; nearest takes
                 Pillow's own two paths, the 16.16 fixed-point walk (affine_fixed) or, for a pure translation, ImagingScaleAffine

An image is (H, W, 3) uint8; a layer is a mapping with the fields of uvit_randaug_layer.
"""
import math

import numpy as np

import augment_util as au

# op ids = the position in timm's _RAND_TRANSFORMS, plus one (0: the layer was not applied)
NONE, AUTOCONTRAST, EQUALIZE, INVERT, ROTATE, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, SHEAR_X, SHEAR_Y, \
    TRANSLATE_X_REL, TRANSLATE_Y_REL = range(16)
OP_NAMES = ("None", "AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
            "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
AFFINE_OPS = (ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X_REL, TRANSLATE_Y_REL)
NEAREST, BILINEAR, BICUBIC = 0, 2, 3                     # PIL.Image.Resampling values
FILTERS = (NEAREST, BILINEAR, BICUBIC)
MAX_LAYERS = 4
# uvit_randaug_layer and uvit_randaug_desc, field for field
LAYER = np.dtype([("op", "<i4"), ("filter", "<i4"), ("arg0", "<i4"), ("arg1", "<i4"), ("factor", "<f4"), ("fill", "<u4"), ("matrix", "<f8", (6,))])
DESC = np.dtype([("n_layers", "<i4"), ("reserved", "<i4"), ("layers", LAYER, (MAX_LAYERS,))])
assert LAYER.itemsize == 72 and DESC.itemsize == 296


# ---- the host's matrices ----
def rotate_matrix(degrees, w, h):
    """Image.rotate(degrees)'s matrix for a (w, h) image, centre (w / 2, h / 2); None where Image.rotate returns a copy (0 degrees)."""
    angle = degrees % 360.0
    if angle == 0:
        return None
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def op_matrix(op, value, w, h):
    """The six doubles of an affine op: `value` is degrees (Rotate), the shear factor, or the translation in pixels."""
    if op == ROTATE:
        return rotate_matrix(value, w, h)
    return {SHEAR_X: [1.0, value, 0.0, 0.0, 1.0, 0.0], SHEAR_Y: [1.0, 0.0, 0.0, value, 1.0, 0.0],
            TRANSLATE_X_REL: [1.0, 0.0, value, 0.0, 1.0, 0.0], TRANSLATE_Y_REL: [1.0, 0.0, 0.0, 0.0, 1.0, value]}[op]


def pack_fill(rgb):
    return int(rgb[0]) | int(rgb[1]) << 8 | int(rgb[2]) << 16


def unpack_fill(word):
    return (int(word) & 255, (int(word) >> 8) & 255, (int(word) >> 16) & 255)


# ---- table ops ----
def table_invert():
    return 255 - np.arange(256)


def table_posterize(bits):
    """ImageOps.posterize behind timm's `bits >= 8: return img`; 0 bits keep nothing."""
    if bits >= 8:
        return np.arange(256)
    return np.arange(256) & ~(2 ** (8 - bits) - 1)


def table_solarize(thresh):
    i = np.arange(256)
    return np.where(i < thresh, i, 255 - i)


def table_solarize_add(add, thresh=128):
    i = np.arange(256)
    return np.where(i < thresh, np.minimum(255, i + add), i)


def table_autocontrast(h):
    """ImageOps.autocontrast(cutoff=0) of one channel's histogram: double arithmetic, int() truncates, then the clamp."""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(ix * scale + offset), 0), 255) for ix in range(256)])


def table_equalize(h):
    """ImageOps.equalize of one channel's histogram: integers only.  Image.point clamps an entry above 255."""
    histo = [int(v) for v in h if v]
    if len(histo) <= 1:
        return np.arange(256)
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return np.arange(256)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(n // step)
        n += int(h[i])
    return np.array(lut)


def histogram(img):
    return [np.bincount(img[..., c].ravel(), minlength=256) for c in range(3)]


def apply_tables(img, tables):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = np.clip(np.asarray(tables[c]), 0, 255).astype(np.uint8)[img[..., c]]
    return out


# ---- blend ops ----
def smooth(img):
    """ImageFilter.SMOOTH (Filter.c, 3 x 3): float32 weights k / 13, the accumulator starts at 0.5f and takes the nine products in
    row-major order, truncated and clamped; the one-pixel border is copied."""
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float32) / np.float32(13)).astype(np.float32)
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    f = img.astype(np.float32)
    acc = np.full((H - 2, W - 2, 3), 0.5, np.float32)
    for dy in range(3):
        for dx in range(3):
            acc = acc + f[dy:dy + H - 2, dx:dx + W - 2] * k[3 * dy + dx]
    out[1:-1, 1:-1] = np.clip(acc, 0, 255).astype(np.uint8)           # clip8 of a float: <= 0 -> 0, >= 255 -> 255, else truncated
    return out


def contrast_mean(img):
    L = au.luma(img)
    return int(float(L.astype(np.int64).sum()) / L.size + 0.5)


def enhance(img, op, factor):
    if op == BRIGHTNESS:
        deg = np.zeros_like(img)
    elif op == CONTRAST:
        deg = np.full_like(img, contrast_mean(img))
    elif op == COLOR:
        deg = np.repeat(au.luma(img)[..., None], 3, axis=2)
    else:
        deg = smooth(img)
    return au.blend(deg, img, factor)


# ---- affine ops ----
def _floor(v):
    return np.floor(v).astype(np.int64)


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def _fix(v):
    """Geometry.c's FIX: FLOOR(v * 65536.0 + 0.5) as a 32-bit int."""
    return int(math.floor(v * 65536.0 + 0.5))


def _nearest_sources(a, W, H):
    """(x, y, inside) of Pillow's two NEAREST paths, which are not the generic transform: ImagingScaleAffine when a1 == a3 == 0
    (doubles, COORD truncates) and the 16.16 fixed-point walk of affine_fixed otherwise."""
    xi, yi = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    if a[1] == 0.0 and a[3] == 0.0:
        xo = (a[2] + a[0] * 0.5) + a[0] * xi.astype(np.float64)
        yo = (a[5] + a[4] * 0.5) + a[4] * yi.astype(np.float64)
        x = np.where(xo < 0.0, -1, np.trunc(np.maximum(xo, 0.0))).astype(np.int64)
        y = np.where(yo < 0.0, -1, np.trunc(np.maximum(yo, 0.0))).astype(np.int64)
    else:
        a0, a1, a3, a4 = _fix(a[0]), _fix(a[1]), _fix(a[3]), _fix(a[4])
        a2, a5 = _fix(a[2] + a[0] * 0.5 + a[1] * 0.5), _fix(a[5] + a[3] * 0.5 + a[4] * 0.5)
        x, y = (a2 + xi * a0 + yi * a1) >> 16, (a5 + xi * a3 + yi * a4) >> 16
    return x, y, (x >= 0) & (x < W) & (y >= 0) & (y < H)


def affine(img, m, flt, fill):
    """Image.transform(size, AFFINE, m, flt, fillcolor=fill): float64 for bilinear and bicubic, Pillow's own two paths for nearest."""
    H, W = img.shape[:2]
    a = [float(v) for v in m]
    out = np.empty_like(img)
    out[...] = np.array(fill, np.uint8)
    if flt == NEAREST:
        x, y, inside = _nearest_sources(a, W, H)
        out[inside] = img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)][inside]
        return out
    xc, yc = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    xin = a[0] * xc + a[1] * yc + a[2]
    yin = a[3] * xc + a[4] * yc + a[5]
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    src = img.astype(np.float64)
    xs, ys = xin - 0.5, yin - 0.5
    x, y = _floor(xs), _floor(ys)
    dx, dy = (xs - x)[..., None], (ys - y)[..., None]
    taps = 2 if flt == BILINEAR else 4
    if taps == 4:
        x, y = x - 1, y - 1
    cols = [np.clip(x + i, 0, W - 1) for i in range(taps)]
    rows = []
    for j in range(taps):
        yy = y + j
        ok = ((yy >= 0) & (yy < H))[..., None]
        p = [src[np.clip(yy, 0, H - 1), c] for c in cols]
        v = p[0] + (p[1] - p[0]) * dx if taps == 2 else _cubic(p[0], p[1], p[2], p[3], dx)
        rows.append(v if j == 0 else np.where(ok, v, rows[-1]))          # row 0 is clamped, a later row outside repeats the previous value
    if taps == 2:
        v = rows[0] + (rows[1] - rows[0]) * dy
        res = v.astype(np.int64).astype(np.uint8)                          # (UINT8) v: truncated; v stays inside [0, 255]
    else:
        v = _cubic(rows[0], rows[1], rows[2], rows[3], dy)
        res = np.clip(v, 0, 255).astype(np.int64).astype(np.uint8)
    out[inside] = res[inside]
    return out


# ---- one layer, a chain, the whole op ----
def apply_layer(img, layer):
    op = int(layer["op"])
    if op == NONE:
        return img
    if op == INVERT:
        return apply_tables(img, [table_invert()] * 3)
    if op == POSTERIZE:
        return apply_tables(img, [table_posterize(int(layer["arg0"]))] * 3)
    if op == SOLARIZE:
        return apply_tables(img, [table_solarize(int(layer["arg0"]))] * 3)
    if op == SOLARIZE_ADD:
        return apply_tables(img, [table_solarize_add(int(layer["arg0"]), int(layer["arg1"]))] * 3)
    if op == AUTOCONTRAST:
        return apply_tables(img, [table_autocontrast(h) for h in histogram(img)])
    if op == EQUALIZE:
        return apply_tables(img, [table_equalize(h) for h in histogram(img)])
    if op in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
        return enhance(img, op, float(np.float32(layer["factor"])))
    if op in AFFINE_OPS:
        return affine(img, layer["matrix"], int(layer["filter"]), unpack_fill(layer["fill"]))
    raise ValueError(op)


def make_layer(op, flt=NEAREST, arg0=0, arg1=0, factor=0.0, fill=(0, 0, 0), matrix=None):
    """One uvit_randaug_layer; an affine op without a matrix (Image.rotate's copy) becomes None."""
    e = np.zeros((), dtype=LAYER)
    if op in AFFINE_OPS and matrix is None:
        return e
    e["op"], e["filter"], e["arg0"], e["arg1"], e["factor"], e["fill"] = op, flt, arg0, arg1, factor, pack_fill(fill)
    e["matrix"] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] if matrix is None else matrix
    return e


def make_desc(chains):
    """uvit_randaug_desc[B] from B lists of layers."""
    desc = np.zeros(len(chains), dtype=DESC)
    for b, chain in enumerate(chains):
        desc[b]["n_layers"] = len(chain)
        for i, e in enumerate(chain):
            desc[b]["layers"][i] = e
    return desc


def pack(x, mean, std):
    """uvit_op_corrupt_pack: q = floor(clip(x * std + mean, 0, 1) * 255 + 0.5) in float32, (B, 3, S, S) -> (B, S, S, 3) uint8."""
    m, s = (np.asarray(v, np.float32).reshape(1, 3, 1, 1) for v in (mean, std))
    v = x.astype(np.float32) * s + m
    q = np.floor(np.minimum(np.maximum(v, np.float32(0)), np.float32(1)) * np.float32(255) + np.float32(0.5))
    return np.ascontiguousarray(q.astype(np.uint8).transpose(0, 2, 3, 1))


def randaug_batch(x, desc, mean, std):
    """uvit_op_randaug_batch: (B, 3, S, S) float32 -> (B, 3, S, S) float32."""
    u8 = pack(x, mean, std)
    out = np.empty_like(x, dtype=np.float32)
    for b in range(x.shape[0]):
        img = u8[b]
        for i in range(int(desc[b]["n_layers"])):
            img = apply_layer(img, desc[b]["layers"][i])
        out[b] = au.to_tensor_normalize(img, mean, std)
    return out
