"""Generate the RandAugment fixture tests/golden/randaug_pil.npz from live Pillow.  Build-container only (needs PIL); never runs on the
GPU box.

    python tools/gen_golden_randaug.py

For two 40 x 40 images and one 37 x 53 image (height x width): every one of timm's fifteen ops at levels 0, 4.5 and 10, plain and
increasing, with both signs where the op has one, the three filters for the affine ops, and a few two-layer chains.  The Pillow side
makes the calls timm's auto_augment.py makes (ImageOps, ImageEnhance, Image.rotate, Image.transform(AFFINE)); the layer records beside
each output are uvit_randaug_layer records (probe_randaug.RANDAUG_LAYER) with the host's matrices, which the fixture therefore pins too.
    images   uint8, the three images end to end;  shapes (3, 2) = (H, W)
    image    (N,) the image of case n;  n_layers (N,);  layers (N, 2 * 72) uint8 = two RANDAUG_LAYER records
    out      uint8, Pillow's outputs end to end, each the size of its image
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "randaug_pil.npz")
FILL = (124, 116, 104)                                           # min(255, round(255 * mean)) of the ImageNet mean
LEVELS = (0.0, 4.5, 10.0)


def pil_op(im, name, value, flt, arg1=128):
    """One op as timm's auto_augment.py calls Pillow."""
    from PIL import Image, ImageEnhance, ImageOps
    kw = dict(resample=flt, fillcolor=FILL)
    if name == "AutoContrast":
        return ImageOps.autocontrast(im)
    if name == "Equalize":
        return ImageOps.equalize(im)
    if name == "Invert":
        return ImageOps.invert(im)
    if name == "Posterize":
        return im if value >= 8 else ImageOps.posterize(im, value)               # timm: `if bits_to_keep >= 8: return img`
    if name == "Solarize":
        return ImageOps.solarize(im, value)
    if name == "SolarizeAdd":
        return im.point([min(255, i + value) if i < arg1 else i for i in range(256)] * 3)
    if name in ("Color", "Contrast", "Brightness", "Sharpness"):
        return getattr(ImageEnhance, name)(im).enhance(value)
    if name == "Rotate":
        return im.rotate(value, **kw)
    m = {"ShearX": (1, value, 0, 0, 1, 0), "ShearY": (1, 0, 0, value, 1, 0), "TranslateXRel": (1, 0, value, 0, 1, 0),
         "TranslateYRel": (1, 0, 0, 0, 1, value)}[name]
    return im.transform(im.size, Image.AFFINE, m, **kw)


def layer_record(name, value, flt, size, arg1=128):
    """The uvit_randaug_layer of the same call.  `size` = (w, h); the rotation's centre is (w / 2, h / 2) as in Image.rotate."""
    import math
    from uncertainty_vit_amd.probe_randaug import RANDAUG_LAYER, RANDAUG_OPS
    e = np.zeros((), RANDAUG_LAYER)
    e["op"], e["matrix"] = RANDAUG_OPS.index(name), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if name in ("Posterize", "Solarize", "SolarizeAdd"):
        e["arg0"], e["arg1"] = value, arg1 if name == "SolarizeAdd" else 0
    elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
        e["factor"] = value
    elif name in ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"):
        e["filter"], e["fill"] = flt, FILL[0] | FILL[1] << 8 | FILL[2] << 16
        if name == "Rotate":
            w, h = size
            if value % 360.0 == 0:
                e["op"], e["filter"], e["fill"] = 0, 0, 0
                return e
            a = -math.radians(value % 360.0)                     # Image.rotate, for a centre that need not be square
            m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
            m[2], m[5] = m[0] * -(w / 2) + m[1] * -(h / 2) + m[2], m[3] * -(w / 2) + m[4] * -(h / 2) + m[5]
            m[2] += w / 2
            m[5] += h / 2
            e["matrix"] = m
        else:
            e["matrix"] = {"ShearX": (1, value, 0, 0, 1, 0), "ShearY": (1, 0, 0, value, 1, 0), "TranslateXRel": (1, 0, value, 0, 1, 0),
                           "TranslateYRel": (1, 0, 0, 0, 1, value)}[name]
    return e


def single_cases(size):
    """(name, value, filter) of every single-op case for an image of `size` = (w, h)."""
    w, h = size
    cases = [("AutoContrast", 0, 0), ("Equalize", 0, 0), ("Invert", 0, 0)]
    fr = [lv / 10.0 for lv in LEVELS]
    cases += [("Posterize", b, 0) for b in sorted({int(f * 4) for f in fr} | {4 - int(f * 4) for f in fr} | {8})]
    cases += [("Solarize", t, 0) for t in sorted({int(f * 256) for f in fr} | {256 - int(f * 256) for f in fr})]
    cases += [("SolarizeAdd", a, 0) for a in sorted({int(f * 110) for f in fr})]
    factors = sorted({float(np.float32(v)) for f in fr for v in (f * 1.8 + 0.1, 1.0 + f * 0.9, 1.0 - f * 0.9)})
    cases += [(name, v, 0) for name in ("Color", "Contrast", "Brightness", "Sharpness") for v in factors]
    for flt in (0, 2, 3):
        signed = lambda top: sorted({s * f * top for f in fr for s in (1.0, -1.0)})      # noqa: E731
        cases += [("Rotate", v, flt) for v in signed(30.0)]
        cases += [(name, v, flt) for name in ("ShearX", "ShearY") for v in signed(0.3) if v != 0.0] + [("ShearX", 0.0, flt)]
        cases += [("TranslateXRel", v, flt) for v in signed(0.45 * w) if v != 0.0]
        cases += [("TranslateYRel", v, flt) for v in signed(0.45 * h) if v != 0.0]
    return cases


CHAINS = [(("Rotate", 27.3, 3), ("Equalize", 0, 0)), (("Solarize", 141, 0), ("Sharpness", 1.81, 0)), (("ShearY", -0.27, 2), ("Contrast", 0.19, 0)),
          (("AutoContrast", 0, 0), ("TranslateXRel", 7.3, 0)), (("Color", 1.9, 0), ("Posterize", 2, 0))]


def make_images():
    rng = np.random.default_rng(20261021)
    noise = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    # few levels, a narrow range and flat regions: tables that are not the identity, runs of equal pixels under the filters
    yy, xx = np.mgrid[0:40, 0:40]
    flat = np.stack([40 + 4 * ((xx // 5 + yy // 7) % 9), 200 - 3 * (xx // 4), 90 + ((xx * yy) // 64) * 5], axis=2).astype(np.uint8)
    flat[rng.random((40, 40)) < 0.05] = (255, 0, 128)
    # 37 x 53: random colours in 3 x 3 blocks with a fifth of the pixels replaced by noise
    blocks = np.kron(rng.integers(0, 256, (13, 18, 3)), np.ones((3, 3, 1), dtype=np.int64))[:37, :53].astype(np.uint8)
    spots = rng.random((37, 53)) < 0.2
    blocks[spots] = rng.integers(0, 256, (int(spots.sum()), 3), dtype=np.uint8)
    return [noise, flat, blocks]


def main():
    from PIL import Image
    images = make_images()
    which, n_layers, layers, outs = [], [], [], []
    for i, img in enumerate(images):
        im = Image.fromarray(img)
        for chain in [(c,) for c in single_cases(im.size)] + CHAINS:
            p, rec = im, np.zeros(2, dtype=layer_record("Invert", 0, 0, im.size).dtype)
            for k, (name, value, flt) in enumerate(chain):
                p = pil_op(p, name, value, flt)
                rec[k] = layer_record(name, value, flt, im.size)
            which.append(i)
            n_layers.append(len(chain))
            layers.append(rec.view(np.uint8).reshape(-1))
            outs.append(np.asarray(p).reshape(-1))
    np.savez_compressed(OUT, images=np.concatenate([a.reshape(-1) for a in images]), shapes=np.asarray([a.shape[:2] for a in images], np.int64),
                        image=np.asarray(which, np.int64), n_layers=np.asarray(n_layers, np.int64), layers=np.stack(layers),
                        out=np.concatenate(outs))
    print(OUT, len(which), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
