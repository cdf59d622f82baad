"""Host side of the image-folder data path (no GPU): crop parameters against the reference, the NumPy restatement of the
augmentation kernel against Pillow, folder scan, descriptor packing, loader construction."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_util as au  # noqa: E402
from uncertainty_vit_amd import datasets as ds  # noqa: E402


def _pil_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "augment_pil.npz"))
    desc = z["desc"].reshape(-1).view(ds.AUG_DESC_DTYPE)
    px_off, out_off = 0, 0
    for d, S in zip(desc, z["size"]):
        n = int(d["h"]) * int(d["w"]) * 3
        img = z["pixels"][px_off:px_off + n].reshape(int(d["h"]), int(d["w"]), 3)
        out = z["out"][out_off:out_off + S * S * 3].reshape(S, S, 3)
        px_off, out_off = px_off + n, out_off + S * S * 3
        yield img, d, int(S), out


def test_crop_params_match_reference(golden_dir):
    rows = np.load(os.path.join(golden_dir, "augment_crop.npz"))["rows"]
    fallback = 0
    for w, h, seed, k, i, j, ch, cw in rows:
        if k == 0:
            random.seed(int(seed))
        got = ds.rrc_params_two_pic(int(h), int(w))
        assert got == (i, j, ch, cw), (w, h, seed, k)
        fallback += (w, h) in ((1000, 20), (20, 1000))
    assert fallback > 0


def test_restatement_equals_pil_fixture(golden_dir):
    n = 0
    for img, d, S, out in _pil_fixture(golden_dir):
        np.testing.assert_array_equal(au.augment_u8(img, d, S), out)
        n += 1
    assert n > 150


def test_restatement_equals_live_pil():
    pytest.importorskip("PIL")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_golden_augment import pil_case
    rng = np.random.default_rng(7)
    torch.manual_seed(7)
    random.seed(7)
    for lvl in (-1, 0, 1, 2, 3, 4):
        for interp in ("bicubic", "lanczos", "hamming", "random"):
            aug = ds.BEiTAugment(int(rng.choice([20, 32])), lvl, interp)
            for _ in range(4):
                H, W = int(rng.integers(3, 70)), int(rng.integers(3, 70))
                img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
                d = aug(H, W)
                np.testing.assert_array_equal(au.augment_u8(img, d, aug.size), pil_case(img, d, aug.size), err_msg=str(d))


def test_descriptor_layout_matches_header():
    from uncertainty_vit_amd import native
    assert ds.AUG_DESC_DTYPE.itemsize == C.sizeof(native.AugmentDesc) == 88
    for name, _ in native.AugmentDesc._fields_:
        assert ds.AUG_DESC_DTYPE.fields[name][1] == getattr(native.AugmentDesc, name).offset, name
    hdr = open(os.path.join(ROOT, "include", "uvit.h")).read()
    for k, v in (("LANCZOS", ds.LANCZOS), ("BILINEAR", ds.BILINEAR), ("BICUBIC", ds.BICUBIC), ("HAMMING", ds.HAMMING),
                 ("BRIGHTNESS", ds.BRIGHTNESS), ("CONTRAST", ds.CONTRAST), ("SATURATION", ds.SATURATION)):
        assert f"#define UVIT_AUG_{k} {v}" in hdr


def _tree(root, files):
    from PIL import Image
    rng = np.random.default_rng(0)
    for rel, (h, w) in files.items():
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)


def test_folder_scan_order(tmp_path):
    pytest.importorskip("PIL")
    _tree(tmp_path, {"b/x2.png": (5, 6), "b/x1.JPG": (6, 5), "a/z/q.png": (4, 4), "a/c.png": (3, 3)})
    (tmp_path / "b" / "notes.txt").write_text("not an image")
    classes, idx = ds.find_classes(str(tmp_path))
    assert classes == ["a", "b"]
    got = [(os.path.relpath(p, tmp_path), c) for p, c in ds.make_dataset(str(tmp_path), idx)]
    assert got == [("a/c.png", 0), ("a/z/q.png", 0), ("b/x1.JPG", 1), ("b/x2.png", 1)]


def test_collate_packs_pixels_and_offsets():
    aug = ds.BEiTAugment(16, -1)
    items = []
    for h, w in ((5, 7), (9, 3), (4, 4)):
        img = np.full((h, w, 3), h, np.uint8)
        items.append(((img, aug(h, w), np.zeros((2, 2), np.int64), aug.size, aug.mean, aug.std), 3))
    b = ds.collate_packed(items)
    rec = b.records()
    assert list(rec["offset"]) == [0, 105, 186] and b.pixels.numel() == 234
    assert list(rec["h"]) == [5, 9, 4] and list(rec["w"]) == [7, 3, 4]
    for r in rec:
        assert b.pixels[r["offset"]].item() == r["h"]
    assert b.mask.shape == (3, 2, 2) and b.labels.tolist() == [3, 3, 3] and b.size == 16


def test_workspace_size_and_bad_descriptors():
    from uncertainty_vit_amd import native
    aug = ds.BEiTAugment(32, -1)
    rec = np.stack([aug(375, 500), aug(20, 1000)]).astype(ds.AUG_DESC_DTYPE)
    desc = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    assert native.augment_ws_bytes(desc, 32) > 2 * 32 * 32 * 4
    for field, val in (("crop_w", 0), ("crop_x", 10_000), ("filter", 4), ("n_jitter", 4), ("resize_h", 0), ("h", 0)):
        bad = rec.copy()
        bad[0][field] = val
        with pytest.raises(native.UvitError):
            native.augment_ws_bytes(torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()), 32)


def _args(tmp_path, data_set):
    import run_cyclical
    a = run_cyclical.get_args(["--data_set", data_set, "--data_path", str(tmp_path), "--input_size", "32", "--num_mask_patches", "3",
                               "--min_mask_patches_per_block", "1", "--max_mask_patches_per_block", "2"])
    a.window_size = (2, 2)
    return a


def test_image_folder_builds_a_loader(tmp_path):
    pytest.importorskip("PIL")
    _tree(tmp_path, {"a/0.png": (40, 30), "a/1.jpg": (20, 50), "b/2.png": (33, 33), "b/3.jpeg": (60, 41)})
    dataset = ds.build_pretraining_dataset(_args(tmp_path, "image_folder"))
    loader = torch.utils.data.DataLoader(dataset, batch_size=2, num_workers=0, collate_fn=ds.collate_packed, drop_last=True)
    batches = list(loader)
    assert len(batches) == 2
    b = batches[0]
    assert isinstance(b, ds.PackedBatch) and len(b) == 2 and b.mask.shape == (2, 2, 2) and b.labels.tolist() == [0, 0]
    rec = b.records()
    assert (rec["resize_w"] == 32).all() and (rec["n_jitter"] == 3).all()
    assert b.pixels.numel() == 40 * 30 * 3 + 20 * 50 * 3
    assert all(0 < int(m.sum()) <= 3 for m in b.mask)


@pytest.mark.parametrize("name", ["CIFAR10", "CIFAR100"])
def test_cifar_still_raises(tmp_path, name):
    with pytest.raises(NotImplementedError, match="torchvision"):
        ds.build_pretraining_dataset(_args(tmp_path, name))
