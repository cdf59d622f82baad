"""GPU: csrc/randaug.hip -- uvit_op_randaug_batch against the numpy restatement of tests/randaug_ref.py, bit for bit, and a probe's
training step with an augmenter (uncertainty-vit_amd/probe_randaug.py, linear_probe.enable_randaug) on the tiny encoder of
tests/test_gpu_probe.py.  No tolerance anywhere: every comparison is of bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_util as au
import probe_ref as pr
import randaug_ref as rr
from test_gpu_probe import fixture_probe
from uncertainty_vit_amd.probe_randaug import RANDAUG_DESC, RandAugmenter

pytestmark = pytest.mark.gpu

GUARD = 64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL = (124, 116, 104)


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def STREAM():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_op(L, x, desc, mean=MEAN, std=STD):
    """One uvit_op_randaug_batch call -> out (B, 3, S, S) as numpy.  x, out and the workspace are followed by sentinels that must
    survive, and x must come back as it went in."""
    x = np.ascontiguousarray(x)
    B, _, S, _ = x.shape
    n = x.size
    xg = torch.full((n + GUARD,), 7.5, device="cuda")
    xg[:n] = torch.from_numpy(x).cuda().view(-1)
    og = torch.full((n + GUARD,), -3.25, device="cuda")
    need = L.uvit_op_randaug_ws_bytes(B, S)
    assert need > 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    desc = np.ascontiguousarray(desc)
    assert desc.dtype == RANDAUG_DESC and desc.shape == (B,)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    rc = L.uvit_op_randaug_batch(P(xg), P(og), C.c_void_p(desc.ctypes.data), B, S, m, s, P(ws), need, STREAM())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((og[n:] == -3.25).all()) and bool((xg[n:] == 7.5).all()) and bool((ws[need:] == 0xA5).all())
    assert np.array_equal(xg[:n].cpu().numpy().reshape(x.shape).view(np.uint32), x.view(np.uint32))           # the input is only read
    return og[:n].cpu().numpy().reshape(x.shape)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def images(B, S, seed, from_u8=True):
    """Normalised batches: ToTensor + Normalize of random uint8 images, or plain normals (values between the uint8 levels and
    outside [0, 1], which the pack rounds and clips)."""
    rng = np.random.default_rng(seed)
    if not from_u8:
        return (rng.standard_normal((B, 3, S, S)) * 1.5).astype(np.float32)
    return np.ascontiguousarray(np.stack([au.to_tensor_normalize(rng.integers(0, 256, (S, S, 3), dtype=np.uint8), MEAN, STD) for _ in range(B)]))


def single_layers(S):
    """Every op at levels 0, 4.5 and 10, plain and increasing, both signs, and the three filters for the affine ops."""
    fr = (0.0, 0.45, 1.0)
    out = [rr.make_layer(op) for op in (rr.AUTOCONTRAST, rr.EQUALIZE, rr.INVERT)]
    out += [rr.make_layer(rr.POSTERIZE, arg0=b) for b in (0, 1, 2, 3, 4, 8)]
    out += [rr.make_layer(rr.SOLARIZE, arg0=t) for t in (0, 115, 141, 256)]
    out += [rr.make_layer(rr.SOLARIZE_ADD, arg0=a, arg1=128) for a in (0, 49, 110)]
    factors = sorted({v for f in fr for v in (f * 1.8 + 0.1, 1.0 + f * 0.9, 1.0 - f * 0.9)})
    out += [rr.make_layer(op, factor=v) for op in (rr.COLOR, rr.CONTRAST, rr.BRIGHTNESS, rr.SHARPNESS) for v in factors]
    for flt in rr.FILTERS:
        for op, top in ((rr.ROTATE, 30.0), (rr.SHEAR_X, 0.3), (rr.SHEAR_Y, 0.3), (rr.TRANSLATE_X_REL, 0.45 * S), (rr.TRANSLATE_Y_REL, 0.45 * S)):
            for v in sorted({sgn * f * top for f in fr for sgn in (1.0, -1.0)}):
                out.append(rr.make_layer(op, flt, fill=FILL, matrix=rr.op_matrix(op, v, S, S)))
        out.append(rr.make_layer(rr.TRANSLATE_X_REL, flt, fill=FILL, matrix=rr.op_matrix(rr.TRANSLATE_X_REL, float(S), S, S)))   # a whole image
    return out


@pytest.mark.parametrize("S", [37, 40])
def test_every_op_and_filter(L, S):
    """B = 5, one layer per image, batch after batch until every case has run; the images of every other batch are not uint8 levels.
    S = 37 is odd (the byte paths, row ends, the smooth filter's border), 40 x 40 takes the 16-byte pack and inverse."""
    B = 5
    layers = single_layers(S)
    seen = set()
    for i0 in range(0, len(layers), B):
        chunk = [layers[(i0 + j) % len(layers)] for j in range(B)]
        desc = rr.make_desc([[e] for e in chunk])
        x = images(B, S, seed=S * 1000 + i0, from_u8=(i0 // B) % 2 == 0)
        want, got = rr.randaug_batch(x, desc, MEAN, STD), run_op(L, x, desc)
        for b in range(B):
            assert same_bits(got[b], want[b]), (rr.OP_NAMES[int(chunk[b]["op"])], int(chunk[b]["filter"]), chunk[b]["matrix"].tolist(),
                                                int((got[b] != want[b]).sum()))
            seen.add((int(chunk[b]["op"]), int(chunk[b]["filter"]) if int(chunk[b]["op"]) in rr.AFFINE_OPS else 0))
    assert {op for op, _ in seen} == set(range(16)) and all((op, f) in seen for op in rr.AFFINE_OPS for f in rr.FILTERS)


def degenerate_images(S):
    """A constant image, a two-valued one, a narrow-range one with few levels: the histogram tables' corner cases."""
    rng = np.random.default_rng(5)
    const = np.full((S, S, 3), (17, 200, 255), np.uint8)
    two = np.where(rng.random((S, S, 1)) < 0.3, np.uint8(40), np.uint8(41)).repeat(3, axis=2).astype(np.uint8)
    two[..., 1] = np.where(two[..., 1] == 40, 0, 255)
    narrow = (100 + rng.integers(0, 7, (S, S, 3)) * 3).astype(np.uint8)
    one_off = np.full((S, S, 3), 9, np.uint8)
    one_off[S // 2, S // 3] = (250, 8, 10)
    return [const, two, narrow, one_off, rng.integers(0, 256, (S, S, 3), dtype=np.uint8)]


@pytest.mark.parametrize("op", [rr.AUTOCONTRAST, rr.EQUALIZE, rr.CONTRAST, rr.SHARPNESS])
def test_degenerate_images(L, op):
    S = 37
    x = np.ascontiguousarray(np.stack([au.to_tensor_normalize(a, MEAN, STD) for a in degenerate_images(S)]))
    desc = rr.make_desc([[rr.make_layer(op, factor=1.7)]] * 5)
    assert same_bits(run_op(L, x, desc), rr.randaug_batch(x, desc, MEAN, STD))


def chain_of_four(S):
    return [rr.make_layer(rr.SHARPNESS, factor=1.81), rr.make_layer(rr.ROTATE, rr.BICUBIC, fill=FILL, matrix=rr.rotate_matrix(-27.3, S, S)),
            rr.make_layer(rr.EQUALIZE), rr.make_layer(rr.SOLARIZE_ADD, arg0=77, arg1=128)]


@pytest.mark.parametrize("S", [37, 40])
def test_chains(L, S):
    """Four layers that mix the four mechanisms; chains with None layers in front, between and behind; a contrast that follows an
    affine op (the mean of L of the image as it stands); one image without a layer."""
    none = rr.make_layer(rr.NONE)
    chains = [chain_of_four(S),
              [none, rr.make_layer(rr.SHEAR_X, rr.BILINEAR, fill=FILL, matrix=rr.op_matrix(rr.SHEAR_X, 0.27, S, S)), none, rr.make_layer(rr.CONTRAST, factor=0.19)],
              [rr.make_layer(rr.AUTOCONTRAST), none, none],
              [],
              [rr.make_layer(rr.TRANSLATE_Y_REL, rr.NEAREST, fill=FILL, matrix=rr.op_matrix(rr.TRANSLATE_Y_REL, -7.3, S, S)),
               rr.make_layer(rr.AUTOCONTRAST), rr.make_layer(rr.COLOR, factor=1.9), rr.make_layer(rr.POSTERIZE, arg0=2)]]
    desc = rr.make_desc(chains)
    x = images(5, S, seed=77)
    got, want = run_op(L, x, desc), rr.randaug_batch(x, desc, MEAN, STD)
    for b in range(5):
        assert same_bits(got[b], want[b]), (b, int((got[b] != want[b]).sum()))
    assert same_bits(got[3], x[3]) and not same_bits(got[0], x[0])
    assert same_bits(run_op(L, x, desc), got)                          # two runs, the same bits
    # the first image alone: B = 1 gives the bits of B = 5
    assert same_bits(run_op(L, x[:1], desc[:1])[0], got[0])


def test_all_none_returns_the_input_bits(L):
    for S in (37, 40):
        x = images(5, S, seed=3)
        none = rr.make_layer(rr.NONE)
        desc = rr.make_desc([[], [none], [none] * 4, [], [none, none]])
        assert same_bits(run_op(L, x, desc), x)


def test_default_config_at_224(L):
    """B = 2, S = 224 under draws of rand-m9-mstd0.5-inc1: more than one workgroup per row of the grid, the 16-byte pack and inverse."""
    aug = RandAugmenter("rand-m9-mstd0.5-inc1", MEAN, "bicubic", seed=11, std=STD)
    x = images(2, 224, seed=9)
    ops, it = set(), 0
    for _ in range(3):
        while True:                                                    # the next draw in which both images have an op
            draw = aug.draw(2, 224, it)
            it += 1
            if (draw.desc["layers"]["op"] != 0).any(axis=1).all():
                break
        ops.update(draw.desc["layers"]["op"].ravel().tolist())
        assert same_bits(run_op(L, x, draw.desc), rr.randaug_batch(x, draw.desc, MEAN, STD)), draw.desc
    assert len(ops - {0}) >= 3


def test_refuses_bad_arguments(L):
    """Every error returns its code before anything is launched: out keeps the pattern it held."""
    B, S = 2, 8
    x = torch.from_numpy(images(B, S, seed=1)).cuda()
    out = torch.arange(x.numel(), dtype=torch.float32, device="cuda")
    pattern = out.clone()
    need = L.uvit_op_randaug_ws_bytes(B, S)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    good = rr.make_desc([[rr.make_layer(rr.INVERT)], [rr.make_layer(rr.ROTATE, rr.BICUBIC, matrix=rr.rotate_matrix(10.0, S, S))]])
    m, s = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)

    def call(desc=good, B=B, S=S, ws_bytes=need, std=s):
        rc = L.uvit_op_randaug_batch(P(x), P(out), C.c_void_p(desc.ctypes.data), B, S, m, std, P(ws), ws_bytes, STREAM())
        torch.cuda.synchronize()
        assert torch.equal(out, pattern)
        return rc

    def with_layer(**kw):
        d = good.copy()
        for k, v in kw.items():
            d[1]["layers"][0][k] = v
        return d

    assert call(B=0) == -2 and call(S=0) == -2 and call(S=1025) == -2 and call(ws_bytes=need - 1) == -4
    assert call(std=(C.c_float * 3)(0.2, 0.0, 0.2)) == -1
    assert call(desc=with_layer(op=16)) == -1 and call(desc=with_layer(filter=1)) == -1 and call(desc=with_layer(factor=float("nan"))) == -1
    bad = good.copy()
    bad[0]["n_layers"] = 5
    assert call(desc=bad) == -2
    # and the same arguments untouched are accepted (out is then overwritten: the pattern check is skipped)
    rc = L.uvit_op_randaug_batch(P(x), P(out), C.c_void_p(good.ctypes.data), B, S, m, s, P(ws), need, STREAM())
    torch.cuda.synchronize()
    assert rc == 0 and not torch.equal(out, pattern)


# --------------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


def active_augmenter(B, S, step):
    """An augmenter whose draw of `step` has an op on some image."""
    for seed in range(64):
        aug = RandAugmenter("rand-m9-mstd0.5-inc1", MEAN, "bicubic", seed=seed, std=STD)
        if aug.draw(B, S, step).active:
            return aug
    raise AssertionError("no active draw in 64 seeds")


def test_train_step_with_an_augmenter(case):
    """A step with an augmenter equals, bit for bit, the step of a probe without one on the restatement's augmented images."""
    fx, _, _, _, _, images_, labels = case
    lr, wd = float(fx["lr"]), float(fx["weight_decay"])
    xg, yg = images_.cuda(), labels.cuda()
    B, S = xg.shape[0], xg.shape[-1]
    aug = active_augmenter(B, S, 0)
    want = rr.randaug_batch(images_.numpy(), aug.draw(B, S, 0).desc, MEAN, STD)
    assert not same_bits(want, images_.numpy())
    probe, plain = fixture_probe(case), fixture_probe(case)
    probe.enable_randaug(aug)
    assert same_bits(probe.randaug_images(xg, aug.draw(B, S, 0)).cpu().numpy(), want)
    loss, gnorm = probe.train_step(xg, yg, lr, wd)
    loss0, gnorm0 = plain.train_step(torch.from_numpy(want).cuda(), yg, lr, wd)
    assert float(loss) == float(loss0) and float(gnorm) == float(gnorm0) and np.isfinite(float(loss))
    assert torch.equal(probe._arena, plain._arena) and torch.equal(probe.exp_avg, plain.exp_avg) and torch.equal(probe.exp_avg_sq, plain.exp_avg_sq)
    untouched = fixture_probe(case)
    loss1, _ = untouched.train_step(xg, yg, lr, wd)
    assert float(loss1) != float(loss) and not torch.equal(untouched._arena, probe._arena)


def test_inactive_draws_leave_the_step_as_it_is(case):
    """An augmenter whose ops are never applied (probability 0): three steps give the bits of a probe without one, and no buffer of
    the op is ever allocated."""
    fx, _, _, _, _, images_, labels = case
    lr, wd = float(fx["lr"]), float(fx["weight_decay"])
    xg, yg = images_.cuda(), labels.cuda()
    probes = [fixture_probe(case), fixture_probe(case), fixture_probe(case)]
    off = RandAugmenter("rand-m9-mstd0.5-inc1", MEAN, seed=3, std=STD)
    off.prob = 0.0
    probes[1].enable_randaug(off)
    probes[2].enable_randaug(RandAugmenter("rand-m9", MEAN, std=STD))
    probes[2].enable_randaug(None)
    losses = [[float(p.train_step(xg, yg, lr, wd)[0]) for _ in range(3)] for p in probes]
    assert losses[0] == losses[1] == losses[2]
    for p in probes[1:]:
        assert torch.equal(p._arena, probes[0]._arena) and torch.equal(p.exp_avg, probes[0].exp_avg) and p._ra_bufs is None


def test_augmenter_then_mixer_and_the_ensemble(case):
    """RandAugment runs in front of the mixer: the mixed batch is the mix of the restatement's augmented images.  The ensemble, which
    refuses a mixer, takes an augmenter."""
    import mix_ref as mr
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.probe_mix import BatchMixer
    fx, _, _, W, _, images_, labels = case
    xg, yg = images_.cuda(), labels.cuda()
    B, S = xg.shape[0], xg.shape[-1]
    aug = active_augmenter(B, S, 0)
    mixer = BatchMixer(mixup_alpha=0.8, seed=3)
    probe = fixture_probe(case)
    probe.enable_randaug(aug)
    probe.enable_mix(mixer)
    fed = probe._train_images(xg).clone()
    augmented = rr.randaug_batch(images_.numpy(), aug.draw(B, S, 0).desc, MEAN, STD)
    d = mixer.draw(B, S, 0)
    want, noisy = mr.mix_batch(augmented, d.desc, d.boxes, d.erase_mode, mixer.seed, 0)
    assert d.active and not noisy.any() and same_bits(fed.cpu().numpy(), want)
    probe._mix = None
    ens, ens0 = (EnsembleProbe(probe.encoder, W.shape[0], members=2, seed=1) for _ in range(2))
    ens0.load_state_dict(ens.state_dict())
    ens.enable_randaug(aug)
    loss, _ = ens.train_step(xg, yg, 1e-3, 0.05)
    loss0, _ = ens0.train_step(torch.from_numpy(augmented).cuda(), yg, 1e-3, 0.05)
    assert float(loss) == float(loss0) and torch.equal(ens._arena, ens0._arena)
