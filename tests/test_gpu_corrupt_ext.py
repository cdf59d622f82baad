"""uvit_op_corrupt_ext_batch on the GPU against tests/corrupt_ext_ref.py: all four kinds are the float32 (for
pixelate: the integer) restatement bit for bit -- nothing on the device is inexact, so there is no tolerance -- pixelate is also live
Pillow, a set does not depend on how it is split into batches, and the exact cases.
Shapes: B = 3 images whose first is image 5 of its set; S = 40 (2.5 MCUs a side, a partial 32-tile, R = 20 is half the image), S = 41 (an
odd plane, odd chroma planes, a true centre pixel) and S = 16 (one MCU, pixelate to 4, motion_blur's R = 15 of 16 and the refusal of
R = 20)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corrupt_ext_ref as xr  # noqa: E402
from uncertainty_vit_amd import corruptions as co  # noqa: E402
from uncertainty_vit_amd import corruptions_ext as cx  # noqa: E402
from uncertainty_vit_amd import datasets as ds  # noqa: E402
from uncertainty_vit_amd.native import UvitError  # noqa: E402

pytestmark = pytest.mark.gpu
B, INDEX0, SEED = 3, 5, 3
MEAN, STD = ds.IMAGENET_DEFAULT_MEAN, ds.IMAGENET_DEFAULT_STD


class Owner:
    """Keeps the workspace of cx.corrupt_ext between the calls of a test."""


def image(s, b=B):
    """Smooth-plus-noise images with a plane of uniform noise in between: low and high frequencies for the DCT, every level for the rest."""
    u8 = np.stack([xr.smooth_noise_image(s, seed=7 + i) for i in range(b)])
    u8[1] = np.random.default_rng(23).integers(0, 256, (3, s, s), dtype=np.uint8)
    return u8


def run_table(u8, kind, table, sev, seed=SEED, index0=INDEX0, owner=None, out=None):
    if out is None:
        out = torch.full(u8.shape, float("nan"), dtype=torch.float32, device="cuda")
    cx.corrupt_ext(owner or Owner(), torch.from_numpy(u8).cuda(), kind, table.to("cuda"), co.set_seed(seed, sev), index0, MEAN, STD, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run(u8, kind, sev, **kw):
    """The op's output for a uint8 batch, as a numpy array on the host."""
    return run_table(u8, kind, cx.ext_params(kind, sev, u8.shape[-1]), sev, **kw)


def want(u8, kind, sev, seed=SEED, index0=INDEX0):
    return xr.normalise(xr.corrupt(u8, kind, sev, seed, index0, np.float32), MEAN, STD)


def levels(out):
    """The uint8 levels behind a normalised output (each is ((q / 255) - mean) / std of a whole q: the rounding is exact)."""
    m, s = np.asarray(MEAN, dtype=np.float64).reshape(3, 1, 1), np.asarray(STD, dtype=np.float64).reshape(3, 1, 1)
    q = np.rint((out.astype(np.float64) * s + m) * 255)
    assert np.array_equal(xr.normalise(q, MEAN, STD).view(np.int32), out.view(np.int32))
    return q.astype(int)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def pillow_pixelate(u8, sev):
    from PIL import Image
    s, n = u8.shape[-1], xr.pixelate_size(sev, u8.shape[-1])
    return np.stack([np.asarray(Image.fromarray(i.transpose(1, 2, 0)).resize((n, n), Image.BOX).resize((s, s), Image.BOX)).transpose(2, 0, 1) for i in u8])


@pytest.mark.parametrize("s", [40, 41])
@pytest.mark.parametrize("sev", [1, 5])
@pytest.mark.parametrize("kind", xr.KINDS)
def test_bit_exact(kind, sev, s):
    u8 = image(s)
    got, ref = run(u8, kind, sev), want(u8, kind, sev)
    assert same_bits(got, ref), f"{int((got != ref).sum())} of {got.size} values differ"
    assert (levels(got) != u8).mean() > 0.5
    if kind == "pixelate":
        try:
            import PIL  # noqa: F401
        except ImportError:
            return
        assert np.array_equal(levels(got), pillow_pixelate(u8, sev))


def test_one_mcu_and_the_refusal_of_a_radius_that_does_not_fit():
    u8 = image(16)
    for kind in xr.KINDS:
        for sev in (1, 2, 3, 4, 5):
            if (kind, sev) == ("motion_blur", 5):                           # R = 20 >= S
                continue
            assert same_bits(run(u8, kind, sev), want(u8, kind, sev)), (kind, sev)
    with pytest.raises(ValueError, match="does not fit"):
        cx.ext_params("motion_blur", 5, 16)
    table = cx.ExtTable(*xr.table("motion_blur", 5, 16))
    out = torch.zeros(u8.shape, dtype=torch.float32, device="cuda")
    with pytest.raises(UvitError, match="unsupported shape"):
        run_table(u8, "motion_blur", table, 5, out=out)
    torch.cuda.synchronize()
    assert not out.any()                                                    # nothing was launched


@pytest.mark.parametrize("kind", xr.KINDS)
def test_a_set_does_not_depend_on_its_split(kind):
    u8 = image(40, b=5)
    owner = Owner()
    whole = run(u8, kind, 3, seed=9, index0=0, owner=owner)
    parts = np.concatenate([run(u8[:2], kind, 3, seed=9, index0=0, owner=owner), run(u8[2:], kind, 3, seed=9, index0=2, owner=owner)])
    assert same_bits(whole, parts) and same_bits(whole, want(u8, kind, 3, 9, 0))
    assert same_bits(whole, run(u8, kind, 3, seed=9, index0=0))             # and not on the run
    # another seed, or another place in the set, changes motion_blur (its direction) and nothing else
    assert same_bits(whole, run(u8, kind, 3, seed=10, index0=0)) == (kind != "motion_blur")
    assert same_bits(whole, run(u8, kind, 3, seed=9, index0=1)) == (kind != "motion_blur")


def test_exact_cases():
    grey = np.full((2, 3, 41, 41), 77, dtype=np.uint8)
    grey[1] = 200
    mid = np.full((1, 3, 41, 41), 128, dtype=np.uint8)
    for sev in (1, 5):
        for kind in ("pixelate", "motion_blur", "zoom_blur"):               # a constant image is a fixed point
            assert np.array_equal(levels(run(grey, kind, sev)), grey), (kind, sev)
        # JPEG: mid-grey has no coefficient and stays within one level; another grey keeps its quantised DC; the planes stay constant
        j = levels(run(mid, "jpeg_compression", sev))
        assert np.abs(j - 128).max() <= 1 and (j == j[:, :, :1, :1]).all()
        j, q0 = levels(run(grey, "jpeg_compression", sev)), int(xr.jpeg_quant_tables(xr.CONSTANTS["jpeg_compression"][sev - 1])[0][0])
        dc = 128 + np.rint(8 * (grey.astype(int) - 128) / q0) * q0 / 8
        assert np.abs(j - dc).max() <= 1 and (j == j[:, :, :1, :1]).all()
    # a single white pixel through motion_blur: the quantised taps at the offsets of each image's direction
    dot = np.zeros((B, 3, 40, 40), dtype=np.uint8)
    dot[:, :, 20, 10] = 255                                                 # ox in [0, 20], |oy| <= 14: every tap lands inside
    for sev in (1, 5):
        tab, R = xr.motion_table(sev)
        got = levels(run(dot, "motion_blur", sev))
        for b in range(B):
            a = xr.motion_angle(SEED, sev, INDEX0 + b)
            ox, oy = tab[(R + 1) * (1 + 2 * a):][:R + 1].astype(int), tab[(R + 1) * (2 + 2 * a):][:R + 1].astype(int)
            expect = np.zeros((40, 40), dtype=np.float32)
            for i in range(R + 1):                                          # two taps of a direction may share a pixel: added in order
                expect[20 + oy[i], 10 + ox[i]] = expect[20 + oy[i], 10 + ox[i]] + tab[i] * np.float32(1.0)
            expect = np.floor(expect * np.float32(255) + np.float32(0.5)).astype(int)
            assert all(np.array_equal(got[b, c], expect) for c in range(3)), (sev, b)
    # the centre pixel of an odd image is its own zoom
    u8 = image(41)
    for sev in (1, 5):
        assert np.array_equal(levels(run(u8, "zoom_blur", sev))[:, :, 20, 20], u8[:, :, 20, 20])


def test_corrupted_sets_take_the_ext_kinds():
    """CorruptedSet over a loader's batches (packed and cached on the way) and over the filled CleanCache, at another batch size, yield the
    restatement's images for a kind of either family."""
    u8 = image(40, b=5)
    labels = torch.arange(5, dtype=torch.int64)
    x = torch.from_numpy(xr.normalise(u8, MEAN, STD)).cuda()
    batches = [((x[:2], None), labels[:2]), ((x[2:], None), labels[2:])]
    cache = co.CleanCache(limit=8, batch_size=3)
    first = torch.cat([i for i, _ in co.CorruptedSet(batches, "motion_blur", 2, 4, MEAN, STD, cache=cache)])
    assert cache.ready and cache.n == 5
    for kind in ("motion_blur", "jpeg_compression", "pixelate"):
        again = list(co.CorruptedSet(cache, kind, 2, 4, MEAN, STD))
        assert [i.shape[0] for i, _ in again] == [3, 2] and torch.equal(torch.cat([lab for _, lab in again]).cpu(), labels)
        got = torch.cat([i for i, _ in again])
        assert same_bits(got.cpu().numpy(), want(u8, kind, 2, 4, 0))
        assert kind != "motion_blur" or torch.equal(got, first)
