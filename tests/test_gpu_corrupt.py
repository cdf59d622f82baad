"""uvit_op_corrupt_pack / uvit_op_corrupt_batch on the GPU against tests/corrupt_ref.py: the pack is the exact
inverse of the normalisation, seven kinds are the float32 restatement bit for bit, the two Box-Muller kinds lie within their derived
bound of the float64 one, the draws have the stated moments and do not depend on how a set is split into batches, and the exact cases.
Shapes: B = 3 images whose first is image 5 of its set, S = 40 (two tiles a side, the second one partial; R = 10 reaches past a quarter
of the image), S = 41 (an odd plane: the one-pixel-per-thread path) and S = 16 with R = 10 (reflect-101 folding most of the image)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corrupt_ref as cr  # noqa: E402
from uncertainty_vit_amd import corruptions as co  # noqa: E402
from uncertainty_vit_amd import datasets as ds  # noqa: E402
from uncertainty_vit_amd.native import UvitError  # noqa: E402

pytestmark = pytest.mark.gpu
B, S, INDEX0 = 3, 40, 5
MEAN, STD = ds.IMAGENET_DEFAULT_MEAN, ds.IMAGENET_DEFAULT_STD
EXACT_KINDS = ("impulse_noise", "shot_noise", "brightness", "saturate", "contrast", "gaussian_blur", "defocus_blur")


class Owner:
    """Keeps the workspace of co.corrupt between the calls of a test."""


def image(b=B, s=S, seed=23):
    u8 = np.random.default_rng(seed).integers(0, 256, (b, 3, s, s), dtype=np.uint8)
    u8[0, :, :4, :4] = 0                                  # black, and grey: the branches of brightness and saturate
    u8[-1, :, :4, :4] = u8[-1, :1, :4, :4]
    return u8


def run(u8, kind, sev, seed=3, index0=INDEX0, mean=MEAN, std=STD, owner=None):
    """The op's output for a uint8 batch, as a numpy array on the host."""
    params = torch.from_numpy(co.corruption_params(kind, sev, u8.shape[-1])).cuda()
    out = torch.full(u8.shape, float("nan"), dtype=torch.float32, device="cuda")
    co.corrupt(owner or Owner(), torch.from_numpy(u8).cuda(), kind, params, co.set_seed(seed, sev), index0, mean, std, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def levels(out, mean=MEAN, std=STD):
    """The uint8 levels behind a normalised output (each is ((q / 255) - mean) / std of a whole q: the rounding is exact)."""
    m, s = np.asarray(mean, dtype=np.float64).reshape(3, 1, 1), np.asarray(std, dtype=np.float64).reshape(3, 1, 1)
    q = np.rint((out.astype(np.float64) * s + m) * 255)
    assert np.array_equal(cr.normalise(q, mean, std).view(np.int32), out.view(np.int32))
    return q.astype(int)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("s", [40, 41])
@pytest.mark.parametrize("mean,std", [(ds.IMAGENET_INCEPTION_MEAN, ds.IMAGENET_INCEPTION_STD), (MEAN, STD)])
def test_pack_inverts_the_normalisation(s, mean, std):
    u8 = image(s=s)
    u8[1, 0].reshape(-1)[:256] = np.arange(256)           # every level
    x = torch.from_numpy(cr.normalise(u8, mean, std)).cuda()
    got = co.pack(x, mean, std)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), u8)
    # values that did not come from uint8 are clipped and rounded
    y = torch.tensor([-9.0, 9.0, 0.0], device="cuda").view(1, 3, 1, 1).expand(1, 3, 8, 8).contiguous()
    z = co.pack(y, (0.5,) * 3, (0.5,) * 3).cpu().numpy()
    assert (z[0, 0] == 0).all() and (z[0, 1] == 255).all() and (z[0, 2] == 128).all()


@pytest.mark.parametrize("sev", [1, 5])
@pytest.mark.parametrize("kind", EXACT_KINDS)
def test_bit_exact_kinds(kind, sev):
    u8 = image()
    got = run(u8, kind, sev)
    want = cr.normalise(cr.corrupt(u8, kind, sev, 3, INDEX0, np.float32), MEAN, STD)
    assert same_bits(got, want), f"{int((got != want).sum())} of {got.size} values differ"
    assert not np.array_equal(levels(got), u8)


@pytest.mark.parametrize("kind,sev", [("brightness", 3), ("shot_noise", 2), ("contrast", 4), ("saturate", 4), ("impulse_noise", 3),
                                      ("gaussian_blur", 2), ("defocus_blur", 3)])
def test_bit_exact_on_an_odd_plane(kind, sev):
    u8 = image(s=41, seed=29)
    assert same_bits(run(u8, kind, sev), cr.normalise(cr.corrupt(u8, kind, sev, 3, INDEX0, np.float32), MEAN, STD))


def test_reflect_101_at_its_limit_and_the_refusal_behind_it():
    u8 = image(s=16, seed=31)
    for kind, sev in (("defocus_blur", 5), ("gaussian_blur", 3)):          # R = 10 and R = 12 in 16 pixels
        assert same_bits(run(u8, kind, sev), cr.normalise(cr.corrupt(u8, kind, sev, 3, INDEX0, np.float32), MEAN, STD))
    with pytest.raises(ValueError):
        co.corruption_params("gaussian_blur", 4, 16)                        # R = 16 >= S
    taps = torch.from_numpy(cr.params("gaussian_blur", 4)).cuda()
    out = torch.zeros(u8.shape, dtype=torch.float32, device="cuda")
    with pytest.raises(UvitError, match="unsupported shape"):
        co.corrupt(Owner(), torch.from_numpy(u8).cuda(), "gaussian_blur", taps, 0, 0, MEAN, STD, out=out)
    torch.cuda.synchronize()
    assert not out.any()                                                    # nothing was launched


@pytest.mark.parametrize("sev", [1, 5])
@pytest.mark.parametrize("kind", ["gaussian_noise", "speckle_noise"])
def test_box_muller_kinds(kind, sev):
    """a device z within 4e-6 of the exact one moves 255 c z by at most 6.1e-4 levels at c = 0.6, so only a value
    that close to a rounding boundary flips: every value within one level of the float64 form, at most 2e-3 of them different."""
    u8 = image()
    got, want = levels(run(u8, kind, sev)), cr.corrupt(u8, kind, sev, 3, INDEX0, np.float64).astype(int)
    diff = got != want
    print(f"\n{kind} severity {sev}: {int(diff.sum())} of {diff.size} values differ, largest difference {int(np.abs(got - want).max())}")
    assert np.abs(got - want).max() <= 1 and diff.mean() <= 2e-3
    assert (got != u8).mean() > 0.5


def test_noise_statistics():
    grey = np.full((B, 3, S, S), 128, dtype=np.uint8)                       # v = 128/255: nothing clips at these severities
    v, n = 128 / 255, B * 3 * S * S
    d = levels(run(grey, "gaussian_noise", 1, seed=0)) / 255 - v
    sd = np.sqrt(0.08 ** 2 + 1 / (12 * 255 ** 2))
    print(f"\ngaussian_noise 1: mean {d.mean():.3e} (se {sd / np.sqrt(n):.3e}), std {d.std():.6f} against {sd:.6f} (se {sd / np.sqrt(2 * n):.3e})")
    assert abs(d.mean()) < 5 * sd / np.sqrt(n) and abs(d.std() - sd) < 5 * sd / np.sqrt(2 * n)
    for sev in (1, 3):
        c = cr.CONSTANTS["shot_noise"][sev - 1]
        x = levels(run(grey, "shot_noise", sev, seed=0)) / 255
        se = np.sqrt(v / c + 1 / (12 * 255 ** 2)) / np.sqrt(n)              # Var(k / c) = lambda / c^2 = v / c
        print(f"shot_noise {sev}: mean {x.mean():.6f} against {v:.6f} (se {se:.3e})")
        assert abs(x.mean() - v) < 5 * se


@pytest.mark.parametrize("kind", ["gaussian_noise", "shot_noise"])
def test_a_set_does_not_depend_on_its_split(kind):
    u8 = image(b=5)
    owner = Owner()
    whole = run(u8, kind, 3, seed=9, index0=0, owner=owner)
    parts = np.concatenate([run(u8[:2], kind, 3, seed=9, index0=0, owner=owner), run(u8[2:], kind, 3, seed=9, index0=2, owner=owner)])
    assert same_bits(whole, parts)
    assert same_bits(whole, run(u8, kind, 3, seed=9, index0=0))             # and not on the run
    assert not np.array_equal(whole, run(u8, kind, 3, seed=10, index0=0))   # another seed, other bytes
    assert not np.array_equal(whole[0], run(u8[:1], kind, 3, seed=9, index0=1)[0])
    assert not np.array_equal(whole, run(u8, kind, 4, seed=9, index0=0))


def test_exact_cases():
    grey = np.full((2, 3, S, S), 77, dtype=np.uint8)
    grey[1] = 200
    for sev in (1, 5):
        for kind in ("gaussian_blur", "defocus_blur", "contrast"):          # a constant image is a fixed point
            assert np.array_equal(levels(run(grey, kind, sev)), grey), (kind, sev)
    for sev in (1, 2, 3):                                                   # c1 = 0: grey stays grey
        assert np.array_equal(levels(run(grey, "saturate", sev)), grey), sev
    black = np.zeros((1, 3, S, S), dtype=np.uint8)
    for sev, level in enumerate((26, 51, 77, 102, 128), 1):                 # floor(255 c + 0.5), c = .1 .. .5
        assert (levels(run(black, "brightness", sev)) == level).all(), sev
    dot = np.zeros((1, 3, S, S), dtype=np.uint8)
    dot[0, :, 20, 20] = 255
    for sev, R in ((1, 8), (5, 10)):                                        # a single white pixel gives the quantised kernel
        k = cr.params("defocus_blur", sev).reshape(2 * R + 1, 2 * R + 1)
        want = np.zeros((S, S), dtype=int)
        want[20 - R:21 + R, 20 - R:21 + R] = np.floor(np.float32(255) * k + np.float32(0.5))[::-1, ::-1]
        got = levels(run(dot, "defocus_blur", sev))
        assert all(np.array_equal(got[0, c], want) for c in range(3)), sev


def test_corrupted_sets_replay_the_cache():
    """CorruptedSet over a loader's batches (packed and cached on the way) and over the filled CleanCache, at another batch size, yield the
    same images and labels; a cache over its limit stays empty."""
    u8 = image(b=5)
    labels = torch.arange(5, dtype=torch.int64)
    x = torch.from_numpy(cr.normalise(u8, MEAN, STD)).cuda()
    batches = [((x[:2], None), labels[:2]), ((x[2:], None), labels[2:])]
    for kind in ("gaussian_noise", "gaussian_blur"):
        cache = co.CleanCache(limit=8, batch_size=3)
        first = list(co.CorruptedSet(batches, kind, 2, 4, MEAN, STD, cache=cache))
        assert cache.ready and cache.n == 5 and [tuple(i.shape) for i, _ in first] == [(2, 3, S, S), (3, 3, S, S)]
        assert all(lab.is_cuda for _, lab in first)
        again = list(co.CorruptedSet(cache, kind, 2, 4, MEAN, STD))
        assert [i.shape[0] for i, _ in again] == [3, 2] and len(cache) == 2
        a, b = torch.cat([i for i, _ in first]), torch.cat([i for i, _ in again])
        assert torch.equal(a, b) and torch.equal(torch.cat([lab for _, lab in again]).cpu(), labels)
        want = cr.normalise(cr.corrupt(u8, kind, 2, 4, 0, np.float64 if kind == "gaussian_noise" else np.float32), MEAN, STD)
        assert (levels(a.cpu().numpy()) != levels(want)).mean() <= (2e-3 if kind == "gaussian_noise" else 0)
    small = co.CleanCache(limit=4, batch_size=3)
    list(co.CorruptedSet(batches, "contrast", 1, 0, MEAN, STD, cache=small))
    assert small.overflowed and not small.ready and small.n == 0
