"""uvit_op_augment_batch on the GPU: bit-identical (torch.equal) to the NumPy restatement (tests/augment_util.py) and to the
PIL fixture; per-sample independence; error codes; `run_cyclical.py --data_set image_folder` end to end."""
import json
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
from uncertainty_vit_amd import native  # noqa: E402

pytestmark = pytest.mark.gpu
MEANS = [(ds.IMAGENET_INCEPTION_MEAN, ds.IMAGENET_INCEPTION_STD), (ds.IMAGENET_DEFAULT_MEAN, ds.IMAGENET_DEFAULT_STD)]


def run_kernel(imgs, recs, S, mean, std):
    """One uvit_op_augment_batch launch over HWC uint8 images with their descriptor records -> (B, 3, S, S) on the CPU."""
    recs = np.stack(recs).astype(ds.AUG_DESC_DTYPE)
    recs["offset"] = np.concatenate([[0], np.cumsum([i.size for i in imgs])[:-1]])
    desc = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).pin_memory()
    pixels = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).cuda()
    out = torch.full((len(imgs), 3, S, S), float("nan"), device="cuda")
    ws = torch.empty(native.augment_ws_bytes(desc, S), dtype=torch.uint8, device="cuda")
    native.augment_batch(pixels, desc, S, mean, std, out, ws, native.cur_stream())
    torch.cuda.synchronize()
    return out.cpu()


def restated(imgs, recs, S, mean, std):
    return torch.from_numpy(np.stack([au.augment(i, r, S, mean, std) for i, r in zip(imgs, recs)]))


def random_case(rng, S, lvl_aug=None):
    """A random image and descriptor: every filter, up to ~20x up- and down-scaling, 1-px crops, all jitter orders, factors at
    0.6 / 1.4, flips, windows reaching outside the resized image."""
    big = rng.random() < 0.15
    H, W = (int(rng.integers(200, 700)), int(rng.integers(200, 700))) if big else (int(rng.integers(1, 90)), int(rng.integers(1, 90)))
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if lvl_aug is not None:
        return img, lvl_aug(H, W)
    d = np.zeros((), ds.AUG_DESC_DTYPE)
    d["h"], d["w"], d["flip"] = H, W, int(rng.integers(0, 2))
    d["filter"] = int(rng.choice([ds.BILINEAR, ds.BICUBIC, ds.HAMMING, ds.LANCZOS]))
    ops = list(rng.permutation(3))[: int(rng.integers(0, 4))]
    d["n_jitter"] = len(ops)
    for k, op in enumerate(ops):
        d["jitter_op"][k] = op
        d["jitter_factor"][k] = float(rng.choice([0.6, 1.4, rng.uniform(0.6, 1.4)]))
    cw = 1 if rng.random() < 0.1 else int(rng.integers(1, W + 1))
    ch = 1 if rng.random() < 0.1 else int(rng.integers(1, H + 1))
    d["crop_w"], d["crop_h"] = cw, ch
    d["crop_x"], d["crop_y"] = int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - ch + 1))
    d["resize_w"] = cw if rng.random() < 0.15 else max(1, int(min(20 * cw, rng.integers(S // 2, 2 * S))))
    d["resize_h"] = ch if rng.random() < 0.15 else max(1, int(min(20 * ch, rng.integers(S // 2, 2 * S))))
    d["win_x"] = int(rng.integers(-S // 2, max(1, d["resize_w"] - S // 2)))
    d["win_y"] = int(rng.integers(-S // 2, max(1, d["resize_h"] - S // 2)))
    return img, d


@pytest.mark.parametrize("S,n,m", [(40, 160, 0), (24, 96, 1), (224, 12, 0)])
def test_kernel_equals_restatement_random(S, n, m):
    rng = np.random.default_rng(S)
    cases = [random_case(rng, S) for _ in range(n)]
    imgs, recs = [c[0] for c in cases], [c[1] for c in cases]
    mean, std = MEANS[m]
    got = run_kernel(imgs, recs, S, mean, std)
    want = restated(imgs, recs, S, mean, std)
    bad = [i for i in range(n) if not torch.equal(got[i], want[i])]
    assert not bad, [(i, recs[i]) for i in bad[:3]]


@pytest.mark.parametrize("lvl", [-1, 0, 1, 2, 3, 4])
def test_kernel_equals_restatement_aug_levels(lvl):
    rng = np.random.default_rng(100 + lvl)
    torch.manual_seed(lvl + 10)
    random.seed(lvl + 10)
    for S, interp in ((224, "bicubic"), (48, "random"), (32, "lanczos"), (32, "hamming")):
        if lvl != -1 and interp != "bicubic":
            continue
        aug = ds.BEiTAugment(S, lvl, interp)
        cases = [random_case(rng, S, aug) for _ in range(12 if S == 224 else 24)]
        imgs, recs = [c[0] for c in cases], [c[1] for c in cases]
        got = run_kernel(imgs, recs, S, aug.mean, aug.std)
        assert torch.equal(got, restated(imgs, recs, S, aug.mean, aug.std)), (lvl, S, interp)


def test_kernel_equals_pil_fixture(golden_dir):
    from test_host_augment import _pil_fixture
    groups = {}
    for img, d, S, out in _pil_fixture(golden_dir):
        groups.setdefault(S, []).append((img, d, out))
    mean, std = MEANS[0]
    for S, cases in groups.items():
        got = run_kernel([c[0] for c in cases], [c[1] for c in cases], S, mean, std)
        want = torch.from_numpy(np.stack([au.to_tensor_normalize(c[2], mean, std) for c in cases]))
        assert torch.equal(got, want), S


def test_sample_independent_of_batch_position():
    rng = np.random.default_rng(5)
    S = 32
    cases = [random_case(rng, S) for _ in range(9)]
    imgs, recs = [c[0] for c in cases], [c[1] for c in cases]
    mean, std = MEANS[0]
    alone = run_kernel(imgs[:1], recs[:1], S, mean, std)[0]
    for perm in ([0, 1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 0, 0, 5]):
        got = run_kernel([imgs[i] for i in perm], [recs[i] for i in perm], S, mean, std)
        for pos, i in enumerate(perm):
            if i == 0:
                assert torch.equal(got[pos], alone)


def test_error_codes():
    rng = np.random.default_rng(1)
    img, d = random_case(rng, 16)
    rec = np.stack([d]).astype(ds.AUG_DESC_DTYPE)
    desc = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
    pixels = torch.from_numpy(img.reshape(-1)).cuda()
    out = torch.empty(1, 3, 16, 16, device="cuda")
    need = native.augment_ws_bytes(desc, 16)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    L, s = native.lib(), native.cur_stream()
    m = (native.C.c_float * 3)(0.5, 0.5, 0.5)

    def call(desc_t, nbytes, ws_bytes):
        return L.uvit_op_augment_batch(native.ptr(pixels), nbytes, native.C.c_void_p(desc_t.data_ptr()), 1, 16, m, m, native.ptr(out),
                                       native.ptr(ws), ws_bytes, s)

    assert call(desc, pixels.numel(), need) == 0
    assert call(desc, pixels.numel() - 1, need) == -2           # image does not fit in the pixel buffer
    assert call(desc, pixels.numel(), need - 1) == -4           # workspace too small
    for field, val, rc in (("offset", -1, -2), ("crop_y", int(d["h"]), -2), ("filter", 0, -1), ("flip", 2, -1), ("resize_w", 0, -2)):
        bad = rec.copy()
        bad[0][field] = val
        assert call(torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()), pixels.numel(), need) == rc, field
    bad = rec.copy()
    bad[0]["n_jitter"], bad[0]["jitter_op"] = 2, [1, 1, 0]       # an op listed twice
    assert call(torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()), pixels.numel(), need) == -1
    torch.cuda.synchronize()


def _image_tree(root):
    from PIL import Image
    rng = np.random.default_rng(11)
    sizes = [(375, 500), (500, 333), (240, 320), (180, 180), (600, 90), (150, 400), (300, 300), (224, 224)]
    for k in range(16):
        h, w = sizes[k % len(sizes)]
        p = os.path.join(root, f"class{k % 3}", f"img{k}.{'png' if k % 2 else 'jpg'}")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)


def test_cli_image_folder_trains_checkpoints_and_resumes(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    import run_cyclical
    from uncertainty_vit_amd import engine_for_cyclical as eng
    data, out = tmp_path / "data", tmp_path / "out"
    _image_tree(str(data))
    out.mkdir()
    seen = {}
    orig_augment, orig_step = eng.DevicePrefetcher._augment, eng.native_step

    def augment(self, item):
        r = orig_augment(self, item)
        seen.setdefault("packed", item)
        return r

    def step(engine, reducer, samples, mask, hp):
        seen.setdefault("samples", samples.clone())
        return orig_step(engine, reducer, samples, mask, hp)

    monkeypatch.setattr(eng.DevicePrefetcher, "_augment", augment)
    monkeypatch.setattr(eng, "native_step", step)

    def argv(epochs, workers):
        return ["--model", "beit_base_patch16_224", "--data_set", "image_folder", "--data_path", str(data), "--batch_size", "8",
                "--epochs", str(epochs), "--warmup_epochs", "0", "--lr", "5e-4", "--target_layers", "[8,9,10,11]",
                "--num_mask_patches", "75", "--num_workers", str(workers), "--output_dir", str(out), "--clip_grad", "3.0",
                "--train_interpolation", "random"]

    run_cyclical.main(run_cyclical.get_args(argv(2, 2)))
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert [l["epoch"] for l in log] == [0, 1]
    assert all(np.isfinite(l["train_loss"]) and 0 < l["train_loss"] < 10 for l in log)
    assert (out / "checkpoint-1.pth").exists()

    # the first batch the step consumed = the restatement of the parameters the loader drew
    pb = seen["packed"]
    recs = pb.records()
    imgs = [pb.pixels[int(r["offset"]):int(r["offset"]) + int(r["h"]) * int(r["w"]) * 3].numpy().reshape(int(r["h"]), int(r["w"]), 3)
            for r in recs]
    assert torch.equal(seen["samples"].cpu(), restated(imgs, recs, 224, pb.mean, pb.std))

    args = run_cyclical.get_args(argv(3, 0))
    run_cyclical.main(args)
    assert args.start_epoch == 2
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert [l["epoch"] for l in log] == [0, 1, 2] and np.isfinite(log[2]["train_loss"])
