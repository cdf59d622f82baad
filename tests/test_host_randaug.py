"""CPU: the numpy restatement of csrc/randaug.hip (tests/randaug_ref.py) against Pillow's recorded bytes (tests/golden/randaug_pil.npz)
and, where PIL imports, against live Pillow; the draws of uncertainty-vit_amd/probe_randaug.py; the command line's flags; the op's
argument checks, which need no device.  Every comparison of pixels is exact."""
import os

import numpy as np
import pytest

import randaug_ref as rr
from uncertainty_vit_amd.probe_mix import BatchMixer
from uncertainty_vit_amd.probe_randaug import MAX_LAYERS, RANDAUG_DESC, RANDAUG_LAYER, RANDAUG_OPS, RandAugmenter, parse_config, rotate_matrix

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL = (124, 116, 104)


# ------------------------------------------------------------------------------------------------------------ layout and formulas
def test_descriptor_layout():
    assert RANDAUG_LAYER == rr.LAYER and RANDAUG_DESC == rr.DESC and RANDAUG_OPS == rr.OP_NAMES and MAX_LAYERS == rr.MAX_LAYERS
    assert RANDAUG_LAYER.itemsize == 72 and RANDAUG_DESC.itemsize == 8 + 4 * 72 and RANDAUG_LAYER.fields["matrix"][1] == 24


def test_host_matrices_agree():
    for deg in (27.3, -13.0, 30.0, 0.0, 360.0, -30.0):
        assert rotate_matrix(deg, 40) == rr.rotate_matrix(deg, 40, 40)
    assert rotate_matrix(0.0, 40) is None and rr.make_layer(rr.ROTATE, rr.BICUBIC, matrix=None)["op"] == rr.NONE


def test_tables():
    assert rr.table_posterize(8).tolist() == list(range(256)) and not rr.table_posterize(0).any()
    assert rr.table_posterize(3).tolist() == [i & 0xE0 for i in range(256)]
    assert rr.table_solarize(256).tolist() == list(range(256)) and rr.table_solarize(0).tolist() == [255 - i for i in range(256)]
    assert rr.table_solarize_add(110).tolist() == [min(255, i + 110) if i < 128 else i for i in range(256)]
    h = np.zeros(256, np.int64)
    h[77] = 1369
    assert rr.table_autocontrast(h).tolist() == list(range(256)) and rr.table_equalize(h).tolist() == list(range(256))      # a constant channel
    h[77], h[80] = 1000, 369
    assert rr.table_autocontrast(h)[77:81].tolist() == [0, 85, 170, 255]
    assert rr.table_equalize(h)[[77, 80]].tolist() == [0, (3 // 2 + 1000) // 3]                                            # step = 1000 // 255 = 3


def test_pack_is_the_inverse_of_to_tensor_normalize():
    import augment_util as au
    rng = np.random.default_rng(0)
    for mean, std in ((MEAN, STD), ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))):
        u8 = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)[:, :, ::-1].copy()
        x = au.to_tensor_normalize(u8, mean, std)[None]
        assert np.array_equal(rr.pack(x, mean, std)[0], u8)
        assert np.array_equal(rr.randaug_batch(x, rr.make_desc([[]]), mean, std).view(np.uint32), x.view(np.uint32))
    wild = (rng.standard_normal((1, 3, 8, 8)) * 3).astype(np.float32)
    assert rr.pack(wild, MEAN, STD).min() == 0 and rr.pack(wild, MEAN, STD).max() == 255


# ------------------------------------------------------------------------------------------------------------ Pillow's recorded bytes
def test_restatement_equals_the_recorded_pillow_bytes(golden_dir):
    fx = np.load(os.path.join(golden_dir, "randaug_pil.npz"))
    shapes = fx["shapes"]
    assert shapes.tolist() == [[40, 40], [40, 40], [37, 53]]
    sizes = [int(h * w * 3) for h, w in shapes]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    imgs = [fx["images"][starts[i]:starts[i + 1]].reshape(int(shapes[i][0]), int(shapes[i][1]), 3) for i in range(3)]
    at, seen, chains = 0, set(), 0
    for i, n, raw in zip(fx["image"], fx["n_layers"], fx["layers"]):
        layers = raw.view(rr.LAYER)
        img = imgs[int(i)]
        want = fx["out"][at:at + img.size].reshape(img.shape)
        at += img.size
        got = img
        for k in range(int(n)):
            got = rr.apply_layer(got, layers[k])
        assert np.array_equal(got, want), (int(i), [(rr.OP_NAMES[int(e["op"])], int(e["filter"]), int(e["arg0"]), float(e["factor"])) for e in layers[:int(n)]],
                                           int((got != want).sum()))
        seen.update((int(i), int(e["op"]), int(e["filter"]) if int(e["op"]) in rr.AFFINE_OPS else 0) for e in layers[:int(n)])
        chains += int(n) > 1
    assert at == fx["out"].size and chains >= 9
    for i in range(3):
        assert {op for j, op, _ in seen if j == i} == set(range(16))
        assert all((i, op, f) in seen for op in rr.AFFINE_OPS for f in rr.FILTERS)


# ------------------------------------------------------------------------------------------------------------------------- live Pillow
def pil_apply(im, e):
    """The Pillow call of one layer record, as timm makes it."""
    from PIL import Image, ImageEnhance, ImageOps
    op = int(e["op"])
    if op == rr.NONE:
        return im
    if op in rr.AFFINE_OPS:
        return im.transform(im.size, Image.AFFINE, tuple(float(v) for v in e["matrix"]), resample=int(e["filter"]), fillcolor=rr.unpack_fill(e["fill"]))
    if op in (rr.COLOR, rr.CONTRAST, rr.BRIGHTNESS, rr.SHARPNESS):
        return getattr(ImageEnhance, rr.OP_NAMES[op])(im).enhance(float(e["factor"]))
    a0, a1 = int(e["arg0"]), int(e["arg1"])
    return {rr.AUTOCONTRAST: lambda: ImageOps.autocontrast(im), rr.EQUALIZE: lambda: ImageOps.equalize(im), rr.INVERT: lambda: ImageOps.invert(im),
            rr.POSTERIZE: lambda: im if a0 >= 8 else ImageOps.posterize(im, a0), rr.SOLARIZE: lambda: ImageOps.solarize(im, a0),
            rr.SOLARIZE_ADD: lambda: im.point([min(255, i + a0) if i < a1 else i for i in range(256)] * 3)}[op]()


def live_images():
    rng = np.random.default_rng(42)
    const = np.full((21, 33, 3), (17, 200, 255), np.uint8)
    two = np.where(rng.random((30, 30, 1)) < 0.3, np.uint8(40), np.uint8(41)).repeat(3, axis=2).astype(np.uint8)
    two[..., 1] = np.where(two[..., 1] == 40, 0, 255)
    return [rng.integers(0, 256, (40, 40, 3), dtype=np.uint8), rng.integers(0, 256, (29, 45, 3), dtype=np.uint8), const, two,
            (100 + rng.integers(0, 7, (37, 37, 3)) * 3).astype(np.uint8), rng.integers(0, 256, (3, 3, 3), dtype=np.uint8),
            rng.integers(0, 256, (2, 5, 3), dtype=np.uint8)]


def live_layers(w, h, rng):
    out = [rr.make_layer(op) for op in (rr.AUTOCONTRAST, rr.EQUALIZE, rr.INVERT)]
    out += [rr.make_layer(rr.POSTERIZE, arg0=b) for b in (0, 1, 4, 7, 8)]                    # posterize to 0 bits among them
    out += [rr.make_layer(rr.SOLARIZE, arg0=t) for t in (0, 1, 128, 255, 256)]              # solarize at 0 and at 256
    out += [rr.make_layer(rr.SOLARIZE_ADD, arg0=a, arg1=t) for a, t in ((0, 128), (110, 128), (255, 256), (30, 0))]
    out += [rr.make_layer(op, factor=f) for op in (rr.COLOR, rr.CONTRAST, rr.BRIGHTNESS, rr.SHARPNESS)
            for f in (0.0, 0.1, 1.0, 1.9, float(rng.uniform(0.1, 1.9)))]
    for flt in rr.FILTERS:
        vals = {rr.ROTATE: (30.0, -30.0, float(rng.uniform(-30, 30))), rr.SHEAR_X: (0.3, -0.3, float(rng.uniform(-0.3, 0.3))),
                rr.SHEAR_Y: (0.3, -0.3, float(rng.uniform(-0.3, 0.3))),
                rr.TRANSLATE_X_REL: (0.45 * w, -0.45 * w, float(w), -float(w), float(rng.uniform(-0.45, 0.45)) * w),     # by a whole image
                rr.TRANSLATE_Y_REL: (0.45 * h, -0.45 * h, float(h), -float(h), float(rng.uniform(-0.45, 0.45)) * h)}
        out += [rr.make_layer(op, flt, fill=FILL, matrix=rr.op_matrix(op, v, w, h)) for op, vs in vals.items() for v in vs]
    return out


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    n = 0
    for img in live_images():
        im = Image.fromarray(img)
        layers = live_layers(im.size[0], im.size[1], rng)
        for e in layers:
            assert np.array_equal(rr.apply_layer(img, e), np.asarray(pil_apply(im, e))), (img.shape, rr.OP_NAMES[int(e["op"])], int(e["filter"]),
                                                                                          int(e["arg0"]), float(e["factor"]), e["matrix"].tolist())
            n += 1
        for _ in range(6):                                             # chains of two to four layers
            chain = [layers[int(k)] for k in rng.integers(0, len(layers), size=int(rng.integers(2, 5)))]
            got, p = img, im
            for e in chain:
                got, p = rr.apply_layer(got, e), pil_apply(p, e)
            assert np.array_equal(got, np.asarray(p)), [rr.OP_NAMES[int(e["op"])] for e in chain]
    assert n > 500


def test_degenerate_tables_are_the_identity():
    const = np.full((9, 9, 3), (3, 3, 250), np.uint8)
    for op in (rr.AUTOCONTRAST, rr.EQUALIZE):
        assert np.array_equal(rr.apply_layer(const, rr.make_layer(op)), const)
    small = np.arange(27, dtype=np.uint8).reshape(3, 3, 3)                   # step = 0: fewer than 255 pixels besides the last level's
    assert np.array_equal(rr.apply_layer(small, rr.make_layer(rr.EQUALIZE)), small)
    moved = rr.apply_layer(small, rr.make_layer(rr.TRANSLATE_X_REL, rr.BICUBIC, fill=FILL, matrix=rr.op_matrix(rr.TRANSLATE_X_REL, 3.0, 3, 3)))
    assert (moved == np.array(FILL, np.uint8)).all()


# ------------------------------------------------------------------------------------------------------------------------- the config
def test_config_parser():
    assert parse_config("rand-m9-mstd0.5-inc1") == {"m": 9.0, "n": 2, "mstd": 0.5, "inc": True}
    assert parse_config("rand") == {"m": 10.0, "n": 2, "mstd": 0.0, "inc": False}
    assert parse_config("rand-n3-m4.5-inc0-mstd0") == {"m": 4.5, "n": 3, "mstd": 0.0, "inc": False}
    a = RandAugmenter("rand-m9-mstd0.5-inc1", MEAN, "random", seed=5, std=STD)
    assert (a.magnitude, a.num_layers, a.magnitude_std, a.increasing, a.interpolation, a.seed, a.fill) == (9.0, 2, 0.5, True, "random", 5, FILL)
    assert RandAugmenter("rand", (0.5, 0.5, 0.5)).fill == (128, 128, 128) and RandAugmenter("rand", (1.2, 0.0, 1.0)).fill == (255, 0, 255)
    assert "m=9" in repr(a) and "mstd=0.5" in repr(a) and "inc=1" in repr(a)


@pytest.mark.parametrize("config,exc", [("original", NotImplementedError), ("v0", NotImplementedError), ("augmix-m5-w4-d2", NotImplementedError),
                                        ("rand-m9-w0", NotImplementedError), ("randm9", NotImplementedError), ("rand-x3", ValueError),
                                        ("rand-m", ValueError), ("rand-n0", ValueError), ("rand-n5", ValueError), ("rand-n2.5", ValueError),
                                        ("rand-inc2", ValueError), ("rand-m11", ValueError), ("rand--m9", ValueError), ("", ValueError)])
def test_config_refusals(config, exc):
    with pytest.raises(exc):
        RandAugmenter(config, MEAN)


def test_augmenter_refusals():
    for kw in (dict(interpolation="lanczos"), dict(mean=(0.5, 0.5)), dict(mean=(0.5, float("nan"), 0.5)), dict(std=(0.5, 0.0, 0.5))):
        with pytest.raises(ValueError):
            RandAugmenter("rand-m9", **{"mean": MEAN, **kw})
    with pytest.raises(ValueError):
        RandAugmenter("rand-m9", MEAN).draw(0, 8, 0)


# --------------------------------------------------------------------------------------------------------------------------- the draws
def test_a_draw_is_a_function_of_seed_and_iteration():
    a, b = (RandAugmenter("rand-m9-mstd0.5-inc1", MEAN, "random", seed=7) for _ in range(2))
    d = a.draw(8, 224, 5)
    a.draw(8, 224, 6)                                                   # drawing something else in between changes nothing
    assert d.desc.tobytes() == a.draw(8, 224, 5).desc.tobytes() == b.draw(8, 224, 5).desc.tobytes()
    assert d.desc.tobytes() != a.draw(8, 224, 6).desc.tobytes()
    assert d.desc.tobytes() != RandAugmenter("rand-m9-mstd0.5-inc1", MEAN, "random", seed=8).draw(8, 224, 5).desc.tobytes()
    # the first rows of a larger batch are the smaller batch's
    assert a.draw(3, 224, 5).desc.tobytes() == d.desc[:3].tobytes()
    # independent of the mixer's streams: streams 0 and 1 of the same (seed, iteration) draw other numbers, and using them moves nothing
    mixer = BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, reprob=0.5, mode="elem", seed=7)
    mixer.draw(8, 224, 5)
    assert a.draw(8, 224, 5).desc.tobytes() == d.desc.tobytes()
    firsts = [float(np.random.Generator(np.random.PCG64([7, 5, s])).random()) for s in (0, 1, 2)]
    assert len(set(firsts)) == 3 and float(a._rng(5).random()) == firsts[2]


@pytest.mark.parametrize("config", ["rand-m9-mstd0.5-inc1", "rand-m10-mstd3-n4", "rand-m0-mstd2-inc1-n1", "rand-m5"])
@pytest.mark.parametrize("interpolation", ["bicubic", "random", "nearest"])
def test_draws_respect_every_range(config, interpolation):
    S = 224
    a = RandAugmenter(config, MEAN, interpolation, seed=1)
    ops, filters, applied, total = set(), set(), 0, 0
    for it in range(40):
        d = a.draw(16, S, it)
        assert d.desc.dtype == RANDAUG_DESC and (d.desc["n_layers"] == a.num_layers).all() and (d.desc["reserved"] == 0).all()
        assert d.active == bool((d.desc["layers"]["op"] != 0).any())
        for row in d.desc:
            assert (row["layers"][a.num_layers:]["op"] == 0).all()
            for e in row["layers"][:a.num_layers]:
                op = int(e["op"])
                total += 1
                applied += op != 0
                ops.add(op)
                assert 0 <= op < 16 and np.isfinite(e["factor"]) and np.isfinite(e["matrix"]).all()
                name = RANDAUG_OPS[op]
                if name == "Posterize":
                    assert 0 <= e["arg0"] <= 4
                elif name == "Solarize":
                    assert 0 <= e["arg0"] <= 256
                elif name == "SolarizeAdd":
                    assert 0 <= e["arg0"] <= 110 and e["arg1"] == 128
                elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
                    assert 0.1 - 1e-6 <= e["factor"] <= 1.9 + 1e-6
                elif op in rr.AFFINE_OPS:
                    filters.add(int(e["filter"]))
                    assert rr.unpack_fill(e["fill"]) == FILL
                    m = e["matrix"]
                    if name == "Rotate":
                        assert abs(m[0] * m[4] - m[1] * m[3] - 1.0) < 1e-12 and m[0] >= np.cos(np.radians(30.0)) - 1e-12
                    elif name.startswith("Shear"):
                        assert abs(m[1] + m[3]) <= 0.3 and (m[1] == 0.0 or m[3] == 0.0) and m[0] == m[4] == 1.0 and m[2] == m[5] == 0.0
                    else:
                        assert abs(m[2] + m[5]) <= 0.45 * S and (m[2] == 0.0 or m[5] == 0.0) and m[0] == m[4] == 1.0 and m[1] == m[3] == 0.0
    assert ops >= set(range(1, 16)) or a.magnitude == 0.0                 # at magnitude 0 a rotation by 0 degrees becomes None
    assert filters == {"bicubic": {3}, "nearest": {0}, "random": {2, 3}}[interpolation]
    assert 0.4 < applied / total < 0.6                                    # every op is applied with probability 0.5


def level_args(config, name, S=200, tries=64):
    """The set of arguments op `name` gets under `config` with every op applied (probability patched to 1)."""
    a = RandAugmenter(config, MEAN, "bilinear", seed=2)
    a.prob = 1.0
    out = set()
    for it in range(tries):
        for e in a.draw(8, S, it).desc["layers"][:, :a.num_layers].ravel():
            if RANDAUG_OPS[int(e["op"])] == name or (name == "Rotate" and int(e["op"]) == 0):
                out.add((int(e["op"]), int(e["arg0"]), int(e["arg1"]), float(e["factor"]), tuple(float(v) for v in e["matrix"])))
    return out


def test_level_functions():
    """mstd 0, probability 1: the tabulated arguments at m = 4.5, plain and increasing."""
    f32 = lambda v: float(np.float32(v))      # noqa: E731
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    S = 200
    for inc, post, sol, factors in ((0, 1, 115, {f32(0.45 * 1.8 + 0.1)}), (1, 3, 141, {f32(1.0 + 0.45 * 0.9), f32(1.0 - 0.45 * 0.9)})):
        cfg = f"rand-m4.5-inc{inc}"
        assert level_args(cfg, "Posterize") == {(5, post, 0, 0.0, ident)}
        assert level_args(cfg, "Solarize") == {(6, sol, 0, 0.0, ident)}
        assert level_args(cfg, "SolarizeAdd") == {(7, 49, 128, 0.0, ident)}
        for op, name in ((8, "Color"), (9, "Contrast"), (10, "Brightness"), (11, "Sharpness")):
            assert level_args(cfg, name) == {(op, 0, 0, f, ident) for f in factors}
        assert level_args(cfg, "AutoContrast") == {(1, 0, 0, 0.0, ident)}
        assert level_args(cfg, "Rotate") == {(4, 0, 0, 0.0, tuple(rr.rotate_matrix(d, S, S))) for d in (13.5, -13.5)}
        assert level_args(cfg, "ShearX") == {(12, 0, 0, 0.0, (1.0, v, 0.0, 0.0, 1.0, 0.0)) for v in (0.135, -0.135)}
        assert level_args(cfg, "ShearY") == {(13, 0, 0, 0.0, (1.0, 0.0, 0.0, v, 1.0, 0.0)) for v in (0.135, -0.135)}
        assert level_args(cfg, "TranslateXRel") == {(14, 0, 0, 0.0, (1.0, 0.0, v, 0.0, 1.0, 0.0)) for v in (0.45 * 0.45 * S, -0.45 * 0.45 * S)}
        assert level_args(cfg, "TranslateYRel") == {(15, 0, 0, 0.0, (1.0, 0.0, 0.0, 0.0, 1.0, v)) for v in (0.45 * 0.45 * S, -0.45 * 0.45 * S)}
    # the ends of the scale
    assert level_args("rand-m10", "Posterize") == {(5, 4, 0, 0.0, ident)} and level_args("rand-m10-inc1", "Posterize") == {(5, 0, 0, 0.0, ident)}
    assert level_args("rand-m10", "Solarize") == {(6, 256, 0, 0.0, ident)} and level_args("rand-m10-inc1", "Solarize") == {(6, 0, 0, 0.0, ident)}
    assert level_args("rand-m0", "Rotate") == {(0, 0, 0, 0.0, (0.0,) * 6)}                  # Image.rotate(0) is a copy: the layer is None
    assert {a[3] for a in level_args("rand-m0-inc1", "Color")} == {1.0} and {a[3] for a in level_args("rand-m10", "Color")} == {f32(1.9)}
    # the magnitude is clamped to [0, 10]
    assert {a[1] for a in level_args("rand-m10-mstd50", "SolarizeAdd")} >= {0, 110} and max(a[1] for a in level_args("rand-m10-mstd50", "SolarizeAdd")) == 110


# ------------------------------------------------------------------------------------------------------------------ the command line
BASE = ["--nb_classes", "3", "--finetune", "c.pth"]


def test_cli_flags_parse():
    import run_linear_probe as rlp
    a = rlp.get_args(BASE + ["--aa", "rand-m9-mstd0.5-inc1", "--aa_interpolation", "random", "--mix_seed", "5"])
    assert (a.aa, a.aa_interpolation, a.mix_seed) == ("rand-m9-mstd0.5-inc1", "random", 5)
    rlp.validate(a)
    aug = rlp.build_augmenter(a)
    assert (aug.magnitude, aug.num_layers, aug.magnitude_std, aug.increasing, aug.interpolation, aug.seed) == (9.0, 2, 0.5, True, "random", 5)
    assert aug.mean == (0.5, 0.5, 0.5) and aug.std == (0.5, 0.5, 0.5) and aug.fill == (128, 128, 128)
    b = rlp.build_augmenter(rlp.get_args(BASE + ["--aa", "rand-m9", "--seed", "9", "--imagenet_default_mean_and_std"]))
    assert b.seed == 9 and b.interpolation == "bicubic" and b.fill == FILL and b.std == STD
    # absent = off: the reference's default rand-m9-mstd0.5-inc1 is not adopted, and the parsed arguments hold nothing new
    assert rlp.build_augmenter(rlp.get_args(BASE)) is None
    assert not any(hasattr(rlp.get_args([]), f) for f in ("aa", "aa_interpolation"))


def test_cli_defaults_still_equal_the_reference():
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()


@pytest.mark.parametrize("extra", [["--aa", "rand-m9", "--eval"], ["--aa", "original"], ["--aa", "augmix-m3"], ["--aa", "rand-m9-w0"],
                                   ["--aa", "rand-q1"], ["--aa", "rand-m9", "--aa_interpolation", "lanczos"], ["--aa_interpolation", "bilinear"]])
def test_cli_refusals(extra):
    import run_linear_probe as rlp
    with pytest.raises((ValueError, NotImplementedError)):
        rlp.validate(rlp.get_args(BASE + extra))


def test_cli_takes_the_ensemble():
    import run_linear_probe as rlp
    rlp.validate(rlp.get_args(BASE + ["--aa", "rand-m9-mstd0.5-inc1", "--ensembles"]))


# ---------------------------------------------------------------------------------------------- the op's argument checks (nothing is launched)
def test_op_refuses_bad_arguments_without_a_device():
    import ctypes as C
    from uncertainty_vit_amd import native
    L = native.lib()
    ARG, SHAPE, WORKSPACE = -1, -2, -4
    B, S = 2, 8
    buf = np.zeros(2 * B * 3 * S * S + 64, dtype=np.float32)          # host memory stands in: every call returns before it touches it
    x, out = buf.ctypes.data, buf.ctypes.data + 4 * B * 3 * S * S
    good = rr.make_desc([[rr.make_layer(rr.INVERT), rr.make_layer(rr.POSTERIZE, arg0=4)],
                         [rr.make_layer(rr.ROTATE, rr.BICUBIC, fill=FILL, matrix=rr.rotate_matrix(10.0, S, S)), rr.make_layer(rr.SOLARIZE_ADD, arg0=9, arg1=128)]])
    need = L.uvit_op_randaug_ws_bytes(B, S)
    assert need == 768 + 2 * 1024 + 2 * 512                           # 2 x 296 bytes of descriptors, a table block per image, two copies of 2 x 3 x 64 bytes
    for b, s in ((0, 8), (65536, 8), (1, 0), (1, 1025), (-1, 8)):
        assert L.uvit_op_randaug_ws_bytes(b, s) == SHAPE
    assert L.uvit_op_randaug_ws_bytes(65535, 1) > 0 and L.uvit_op_randaug_ws_bytes(1, 1024) > 0
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    ws = np.zeros(need + 16, dtype=np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15

    def call(d=good, xp=x, op=out, B=B, S=S, m=mean, s=std, ws=wsp, ws_bytes=need, no_desc=False):
        return L.uvit_op_randaug_batch(C.c_void_p(xp), C.c_void_p(op), None if no_desc else C.c_void_p(d.ctypes.data), B, S, m, s,
                                       C.c_void_p(ws), ws_bytes, None)

    def layer(b, i, **kw):
        d = good.copy()
        for k, v in kw.items():
            d[b]["layers"][i][k] = v
        return d

    assert call(xp=0) == ARG and call(op=0) == ARG and call(ws=0) == ARG and call(no_desc=True) == ARG and call(m=None) == ARG and call(s=None) == ARG
    assert call(xp=x + 2) == ARG
    assert call(B=0) == SHAPE and call(S=0) == SHAPE and call(S=1025) == SHAPE and call(B=65536) == SHAPE
    for n in (-1, 5):
        d = good.copy()
        d[1]["n_layers"] = n
        assert call(d=d) == SHAPE, n
    for bad in ((float("nan"), 0.2, 0.2), (0.2, float("inf"), 0.2)):
        assert call(m=(C.c_float * 3)(*bad)) == ARG and call(s=(C.c_float * 3)(*bad)) == ARG
    assert call(s=(C.c_float * 3)(0.2, 0.2, 0.0)) == ARG
    for kw in (dict(op=16), dict(op=-1), dict(filter=1), dict(filter=4), dict(filter=-1), dict(factor=float("nan")), dict(factor=float("inf"))):
        assert call(d=layer(0, 0, **kw)) == ARG, kw
    assert call(d=layer(0, 1, arg0=-1)) == ARG and call(d=layer(0, 1, arg0=9)) == ARG                       # posterize bits
    assert call(d=layer(1, 1, arg0=256)) == ARG and call(d=layer(1, 1, arg0=-1)) == ARG and call(d=layer(1, 1, arg1=257)) == ARG
    sol = layer(0, 0, op=rr.SOLARIZE, arg0=257)
    assert call(d=sol) == ARG and call(d=layer(0, 0, op=rr.SOLARIZE, arg0=-1)) == ARG
    for i, v in ((0, float("nan")), (2, float("inf")), (1, 4.5), (5, -8193.0)):
        m = np.array(good[1]["layers"][0]["matrix"])
        m[i] = v
        assert call(d=layer(1, 0, matrix=m)) == ARG, (i, v)
    # a layer past n_layers is not read
    d = good.copy()
    d[0]["n_layers"] = 1
    d[0]["layers"][1]["op"] = 99
    assert call(d=d, ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert not buf.any() and not ws.any()
