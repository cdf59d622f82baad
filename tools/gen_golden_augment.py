"""Generate the augmentation fixtures tests/golden/augment_*.npz.  Build-container only (needs PIL and the reference); never
runs on the GPU box.

    python tools/gen_golden_augment.py

augment_crop.npz   (a) crop boxes of the UNMODIFIED reference RandomResizedCropAndInterpolationWithTwoPic.get_params
                       (transforms.py, imported through tools/ref_harness.py) over a grid of image sizes and `random` seeds,
                       extreme aspect ratios included (they reach the central-crop fallback).
augment_pil.npz    (b) PIL outputs (uint8, after the resize / center crop, before ToTensor) of small random images for every
                       filter, jitter order, flip, aug level and padding case, with the uvit_augment_desc records that describe
                       them.  The PIL side calls ImageEnhance / transpose / crop / resize / a zero-padded paste exactly as
                       torchvision's PIL functional does.
"""
import itertools
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")


class _Img:          # get_params only reads .size = (width, height)
    def __init__(self, w, h):
        self.size = (w, h)


def crop_fixture():
    import ref_harness
    ref_harness.install()
    from transforms import RandomResizedCropAndInterpolationWithTwoPic as RRC   # the reference's transforms.py
    sizes = [(500, 375), (375, 500), (224, 224), (1000, 20), (20, 1000), (640, 480), (33, 7), (4000, 3000), (5, 5), (300, 299)]
    rows = []
    for (w, h), seed in itertools.product(sizes, range(8)):
        random.seed(seed)
        for k in range(4):
            i, j, ch, cw = RRC.get_params(_Img(w, h), (0.08, 1.0), (3. / 4., 4. / 3.))
            rows.append((w, h, seed, k, i, j, ch, cw))
    return {"rows": np.asarray(rows, np.int64)}


def pil_case(img, d, S):
    """The reference pipeline in PIL for one descriptor: jitter -> flip -> crop -> resize -> window (zero-padded)."""
    from PIL import Image, ImageEnhance
    p = Image.fromarray(img)
    enh = {0: ImageEnhance.Brightness, 1: ImageEnhance.Contrast, 2: ImageEnhance.Color}
    for k in range(int(d["n_jitter"])):
        p = enh[int(d["jitter_op"][k])](p).enhance(float(d["jitter_factor"][k]))
    if d["flip"]:
        p = p.transpose(Image.FLIP_LEFT_RIGHT)
    cx, cy, cw, ch = (int(d[k]) for k in ("crop_x", "crop_y", "crop_w", "crop_h"))
    p = p.crop((cx, cy, cx + cw, cy + ch))
    rw, rh = int(d["resize_w"]), int(d["resize_h"])
    if (rw, rh) != p.size:
        p = p.resize((rw, rh), int(d["filter"]))
    canvas = Image.new("RGB", (S, S), (0, 0, 0))           # torchvision pads with fill=0, then crops
    wx, wy = int(d["win_x"]), int(d["win_y"])
    canvas.paste(p.crop((max(wx, 0), max(wy, 0), min(wx + S, rw), min(wy + S, rh))), (max(-wx, 0), max(-wy, 0)))
    return np.asarray(canvas)


def pil_fixture():
    from uncertainty_vit_amd.datasets import AUG_DESC_DTYPE, BEiTAugment
    rng = np.random.default_rng(20261015)
    torch.manual_seed(0)
    random.seed(0)
    imgs, descs, outs, sizes = [], [], [], []

    def add(img, d, S):
        imgs.append(img.reshape(-1))
        descs.append(d)
        outs.append(pil_case(img, d, S).reshape(-1))
        sizes.append(S)

    orders = list(itertools.permutations(range(3)))
    filters = [1, 2, 3, 5]
    # explicit descriptors: every filter x jitter order, flips, factors at the ends of [0.6, 1.4], 1-px crops, up- and down-scaling
    for n in range(96):
        H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        S = int(rng.choice([8, 16, 24]))
        d = np.zeros((), AUG_DESC_DTYPE)
        d["h"], d["w"], d["flip"], d["filter"] = H, W, n % 2, filters[n % 4]
        ops = orders[(n // 4) % 6][: 3 - (n // 24) % 4]
        d["n_jitter"] = len(ops)
        for k, op in enumerate(ops):
            d["jitter_op"][k] = op
            d["jitter_factor"][k] = [0.6, 1.4, float(rng.uniform(0.6, 1.4))][(n + k) % 3]
        cw = 1 if n % 7 == 0 else int(rng.integers(1, W + 1))
        ch = 1 if n % 11 == 0 else int(rng.integers(1, H + 1))
        d["crop_w"], d["crop_h"] = cw, ch
        d["crop_x"], d["crop_y"] = int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - ch + 1))
        d["resize_w"] = cw if n % 5 == 0 else S
        d["resize_h"] = ch if n % 6 == 0 else S
        add(img, d, S)
    # the aug levels' own parameter draws, small and large images, padding (images smaller than the output)
    for lvl in (-1, 0, 1, 2, 3, 4):
        for interp in (["bicubic", "random", "lanczos", "hamming", "bilinear"] if lvl == -1 else ["bicubic"]):
            for S in (16, 24):
                aug = BEiTAugment(S, lvl, interp)
                for _ in range(3):
                    H, W = int(rng.integers(4, 48)), int(rng.integers(4, 48))
                    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
                    add(img, aug(H, W), S)
    return {"pixels": np.concatenate(imgs), "desc": np.stack(descs).view(np.uint8).reshape(len(descs), -1),
            "out": np.concatenate(outs), "size": np.asarray(sizes, np.int64)}


def main():
    np.savez_compressed(os.path.join(OUT, "augment_crop.npz"), **crop_fixture())
    np.savez_compressed(os.path.join(OUT, "augment_pil.npz"), **pil_fixture())
    for f in ("augment_crop.npz", "augment_pil.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
