"""CPU: the host side of the probe's training-time mixing -- the draws of uncertainty-vit_amd/probe_mix.py, the restatement
tests/mix_ref.py checks itself against, and the command line's flags and refusals."""
import numpy as np
import pytest
import torch

import mix_ref as mr
import probe_ref as pr
from uncertainty_vit_amd.probe_mix import MAX_BOXES, MIX_DESC, BatchMixer


# ------------------------------------------------------------------------------------------------------------------------ the draws
def test_descriptor_layout():
    assert MIX_DESC.itemsize == 32 and MIX_DESC.names == ("kind", "lam", "partner", "yl", "yh", "xl", "xh", "reserved")


@pytest.mark.parametrize("B", [1, 2, 5, 8])
@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_partner_is_the_flipped_batch(B, mode):
    d = BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, reprob=0.5, seed=3).draw(B, 32, 7)
    want = B - 1 - np.arange(B)
    assert d.partner.dtype == np.int32 and d.lam.dtype == np.float32
    assert (d.partner == want).all() and (d.desc["partner"] == want).all()
    assert (d.lam == d.desc["lam"]).all() and (d.lam[d.desc["kind"] == 0] == 1.0).all()


@pytest.mark.parametrize("B", [2, 5, 8, 9])
def test_pair_mode_is_mirrored(B):
    seen = set()
    for it in range(20):
        d = BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, mode="pair", seed=1).draw(B, 32, it).desc
        for f in ("kind", "lam", "yl", "yh", "xl", "xh"):
            assert (d[f] == d[f][::-1]).all(), f
        if B % 2:
            assert d["kind"][B // 2] == 0 and d["lam"][B // 2] == 1.0
        seen.update(d["kind"].tolist())
    assert seen == ({0, 1, 2} if B % 2 else {1, 2})     # the middle row apart, a row is mixed at prob 1 (an empty cutmix box is rare at S = 32)


def test_batch_mode_shares_one_draw():
    d = BatchMixer(mixup_alpha=0.8, mode="batch").draw(6, 16, 0).desc
    assert len(set(d["lam"].tolist())) == 1 and (d["kind"] == 1).all()


def test_switched_off_draws_are_inactive():
    for mixer in (BatchMixer(), BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0), BatchMixer(mixup_alpha=0.8, prob=0.0, reprob=0.0)):
        d = mixer.draw(8, 32, 5)
        assert d.active is False and (d.desc["kind"] == 0).all() and d.boxes.shape == (8, 0, 4)
    assert not BatchMixer().enabled and BatchMixer(reprob=0.1).enabled and BatchMixer(cutmix_minmax=(0.2, 0.5)).enabled
    assert BatchMixer(reprob=1.0).draw(4, 32, 0).active


@pytest.mark.parametrize("minmax", [None, (0.2, 0.6), (0.5, 0.5), (1.0, 1.0)])
@pytest.mark.parametrize("S", [1, 7, 32, 224])
def test_cutmix_boxes_lie_in_the_image(S, minmax):
    n = 0
    for it in range(8):
        d = BatchMixer(cutmix_alpha=1.0, cutmix_minmax=minmax, mode="elem", seed=it).draw(64, S, it).desc
        assert ((d["kind"] == 0) | (d["kind"] == 2)).all()
        assert (0 <= d["yl"]).all() and (d["yl"] <= d["yh"]).all() and (d["yh"] <= S).all()
        assert (0 <= d["xl"]).all() and (d["xl"] <= d["xh"]).all() and (d["xh"] <= S).all()
        cut = d[d["kind"] == 2]
        area = (cut["yh"] - cut["yl"]).astype(np.float64) * (cut["xh"] - cut["xl"])
        assert (cut["lam"] == (1.0 - area / float(S * S)).astype(np.float32)).all()        # correct_lam, rounded to float32 once
        assert (area > 0).all()                                                             # an empty box has lam 1: kind 0
        n += len(cut)
    assert n > 0 or S == 1                             # S = 1: a box is empty (lam 1) or the whole image


@pytest.mark.parametrize("recount", [1, 3, MAX_BOXES])
@pytest.mark.parametrize("S", [4, 20, 224])
def test_erase_boxes_lie_in_the_image(S, recount):
    boxes = BatchMixer(reprob=1.0, recount=recount, seed=2).draw(64, S, 1).boxes
    assert boxes.shape == (64, recount, 4) and boxes.dtype == np.int32
    top, left, h, w = (boxes[..., i] for i in range(4))
    on = h > 0
    assert on.any() and (w[on] > 0).all() and (h < S).all() and (w < S).all() and (w[~on] == 0).all()
    assert (top >= 0).all() and (left >= 0).all() and (top + h <= S).all() and (left + w <= S).all()


def test_a_draw_is_a_function_of_seed_and_iteration():
    mk = lambda seed: BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", reprob=0.5, recount=2, seed=seed)      # noqa: E731
    a, b = mk(4).draw(16, 32, 9), mk(4).draw(16, 32, 9)
    assert a.desc.tobytes() == b.desc.tobytes() and a.boxes.tobytes() == b.boxes.tobytes()
    mixer = mk(4)
    mixer.draw(16, 32, 3)                              # a draw in between changes nothing: no state
    c = mixer.draw(16, 32, 9)
    assert a.desc.tobytes() == c.desc.tobytes() and a.boxes.tobytes() == c.boxes.tobytes()
    other_it, other_seed = mk(4).draw(16, 32, 10), mk(5).draw(16, 32, 9)
    for o in (other_it, other_seed):
        assert a.desc.tobytes() != o.desc.tobytes() and a.boxes.tobytes() != o.boxes.tobytes()
    # the erasing stream does not depend on the mixing flags
    assert BatchMixer(reprob=0.5, recount=2, seed=4).draw(16, 32, 9).boxes.tobytes() == a.boxes.tobytes()


def test_draw_statistics():
    """4096 elem rows: mixup's lam ~ Beta(1, 1) = U(0, 1), mean 0.5 and variance 1 / 12; a row is erased with probability reprob."""
    n, reprob = 4096, 0.25
    d = BatchMixer(mixup_alpha=1.0, mode="elem", reprob=reprob, seed=11).draw(n, 32, 0)
    lam = d.lam[d.desc["kind"] == 1].astype(np.float64)
    assert len(lam) >= n - 2
    se = np.sqrt(1.0 / 12.0 / len(lam))
    print(f"\nmean lam {lam.mean():.4f} (se {se:.4f})")
    assert abs(lam.mean() - 0.5) <= 5 * se
    share = float((d.boxes[:, :, 2] > 0).any(1).mean())
    se = np.sqrt(reprob * (1 - reprob) / n)
    print(f"erased share {share:.4f} against {reprob} (se {se:.4f})")
    assert abs(share - reprob) <= 5 * se
    # with both alphas, cutmix is chosen with probability switch_prob
    kinds = BatchMixer(mixup_alpha=1.0, cutmix_alpha=1.0, switch_prob=0.3, mode="elem", seed=12).draw(n, 224, 0).desc["kind"]
    mixed = kinds != 0
    share = float((kinds[mixed] == 2).mean())
    assert abs(share - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / mixed.sum()) + 2.0 / n           # an empty cutmix box falls back to kind 0


@pytest.mark.parametrize("kw", [dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(prob=1.5), dict(prob=-0.1), dict(switch_prob=2.0),
                                dict(reprob=1.01), dict(mode="half"), dict(remode="noise"), dict(recount=0), dict(recount=9),
                                dict(cutmix_minmax=(0.5,)), dict(cutmix_minmax=(0.0, 0.5)), dict(cutmix_minmax=(0.6, 0.5)),
                                dict(cutmix_minmax=(0.5, 1.5)), dict(cutmix_minmax=(0.1, 0.2, 0.3))])
def test_mixer_refuses(kw):
    with pytest.raises(ValueError):
        BatchMixer(**kw)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def test_soft_loss_is_the_mix_of_the_two_hard_losses():
    B, K, s = 6, 11, 0.1
    z, y = rnd(B, K, seed=1, scale=2.0), torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(2))
    partner = torch.arange(B - 1, -1, -1)
    lam = torch.tensor([0.0, 1.0, 0.25, 0.5, 0.7, 1.0], dtype=torch.float64)
    rows, loss, dz = mr.soft_ce(z, y, partner, lam, s)
    La, _, da = pr.smoothed_ce(z, y, s)
    Lb, _, db = pr.smoothed_ce(z, y[partner], s)
    torch.testing.assert_close(rows, lam * La + (1 - lam) * Lb, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(dz, lam.view(-1, 1) * da + (1 - lam.view(-1, 1)) * db, rtol=1e-13, atol=1e-15)
    assert float(loss) == pytest.approx(float(rows.mean()), rel=1e-15)
    # lam = 1 everywhere: probe_ref's smoothed cross-entropy
    rows1, loss1, dz1 = mr.soft_ce(z, y, partner, torch.ones(B), s)
    torch.testing.assert_close(rows1, La, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(dz1, da, rtol=1e-13, atol=1e-15)
    # the target is a distribution
    torch.testing.assert_close(mr.soft_target(y, partner, lam, K, s).sum(1), torch.ones(B, dtype=torch.float64), rtol=1e-14, atol=0)


def test_soft_loss_gradient():
    B, K, s = 4, 7, 0.1
    z, y = rnd(B, K, seed=3).double(), torch.tensor([0, 6, 3, 3])
    partner, lam = torch.tensor([3, 2, 1, 0]), torch.tensor([0.3, 0.0, 1.0, 0.6], dtype=torch.float64)
    _, _, dz = mr.soft_ce(z, y, partner, lam, s)
    assert float(dz.sum(1).abs().max()) <= 1e-15       # softmax and target both sum to 1
    h = 1e-6
    for b in range(B):
        for k in range(K):
            zp, zm = z.clone(), z.clone()
            zp[b, k] += h
            zm[b, k] -= h
            num = (float(mr.soft_ce(zp, y, partner, lam, s)[1]) - float(mr.soft_ce(zm, y, partner, lam, s)[1])) / (2 * h)
            assert abs(num - float(dz[b, k])) <= 1e-9, (b, k)


def test_restated_mix_batch():
    B, S = 3, 6
    x = rnd(B, 3, S, S, seed=5).numpy()
    desc = np.zeros(B, dtype=MIX_DESC)
    desc["partner"], desc["lam"] = [2, 1, 0], 1.0
    boxes = np.zeros((B, 2, 4), dtype=np.int32)
    out, noisy = mr.mix_batch(x, desc, boxes, 2, 1, 0)
    assert out.tobytes() == x.tobytes() and not noisy.any()                 # kind 0, no box: bit for bit
    desc[0]["kind"], desc[0]["lam"] = 1, 0.25
    desc[2]["kind"], desc[2]["yl"], desc[2]["yh"], desc[2]["xl"], desc[2]["xh"] = 2, 1, 3, 0, 6
    boxes[2, 1] = (0, 0, 2, 5)                                              # sample 2 is erased in rows 0..1, columns 0..4
    out, noisy = mr.mix_batch(x, desc, boxes, 0, 1, 0)
    e2 = x[2].copy()
    e2[:, 0:2, 0:5] = 0.0
    assert np.array_equal(out[0], np.float32(0.25) * x[0] + np.float32(0.75) * e2)
    assert np.array_equal(out[1], x[1])
    assert np.array_equal(out[2][:, 1:3, :], x[0][:, 1:3, :]) and np.array_equal(out[2][:, 0, :], e2[:, 0, :]) and np.array_equal(out[2][:, 3:, :], x[2][:, 3:, :])
    assert not noisy.any()
    # pixel noise: keyed by the sample alone -- the same values in out[2] and in the mixup row that reads sample 2
    o2, n2 = mr.mix_batch(x, desc, boxes, 2, 1, 0)
    assert n2[2][:, 0, 0:5].all() and not n2[2][:, 1:3, :].any() and n2[0][:, 0:2, 0:5].all() and not n2[1].any()
    e, _ = mr.erased(x, boxes, 2, 1, 0)
    assert np.array_equal(o2[2][:, 0, 0:5], e[2][:, 0, 0:5])
    o3, _ = mr.mix_batch(x, desc, boxes, 2, 1, 1)
    assert not np.array_equal(o3[2][:, 0, 0:5], o2[2][:, 0, 0:5])           # another iteration, another fill
    # rand: one value per (box, channel)
    o4, _ = mr.mix_batch(x, desc, boxes, 1, 1, 0)
    assert (o4[2][:, 0, 0:5] == o4[2][:, 0, 0:1]).all() and len(set(o4[2][:, 0, 0].tolist())) == 3


def test_restated_normals():
    """The uniforms lie strictly inside (0, 1) on the grid (k + 0.5) 2^-23, and 2^18 normals have mean 0 and variance 1 within 5
    standard errors."""
    q = np.arange(1 << 18, dtype=np.uint64)
    u1, u2 = mr.uniforms(mr.sample_key(7, 3, 0), q)
    for u in (u1, u2):
        assert u.min() > 0 and u.max() < 1 and np.array_equal(u * 2.0 ** 23 - 0.5, np.floor(u * 2.0 ** 23))
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    n = mr.normals(mr.sample_key(7, 3, 0), q)
    assert abs(n.mean()) <= 5 / np.sqrt(n.size) and abs(n.var() - 1.0) <= 5 * np.sqrt(2.0 / n.size)
    assert not np.array_equal(n, mr.normals(mr.sample_key(7, 3, 1), q)) and not np.array_equal(n, mr.normals(mr.sample_key(7, 4, 0), q))


# ------------------------------------------------------------------------------------------------------------------ the command line
BASE = ["--nb_classes", "3", "--finetune", "c.pth"]


def test_cli_flags_parse():
    import run_linear_probe as rlp
    a = rlp.get_args(BASE + ["--mixup", "0.8", "--cutmix", "1.0", "--cutmix_minmax", "0.2", "0.6", "--mixup_prob", "0.9", "--mixup_switch_prob", "0.4",
                             "--mixup_mode", "elem", "--reprob", "0.25", "--remode", "rand", "--recount", "2", "--mix_seed", "5"])
    assert (a.mixup, a.cutmix, a.cutmix_minmax, a.mixup_prob, a.mixup_switch_prob, a.mixup_mode, a.reprob, a.remode, a.recount, a.mix_seed) == \
        (0.8, 1.0, [0.2, 0.6], 0.9, 0.4, "elem", 0.25, "rand", 2, 5)
    rlp.validate(a)
    m = rlp.build_mixer(a)
    assert (m.mixup_alpha, m.cutmix_alpha, m.cutmix_minmax, m.prob, m.switch_prob, m.mode, m.reprob, m.remode, m.recount, m.seed) == \
        (0.8, 1.0, (0.2, 0.6), 0.9, 0.4, "elem", 0.25, "rand", 2, 5)
    # absent = off (the reference's --reprob 0.25 is not adopted); --mix_seed defaults to --seed
    assert rlp.build_mixer(rlp.get_args(BASE)) is None and rlp.build_mixer(rlp.get_args(BASE + ["--mixup_prob", "0.5"])) is None
    assert rlp.build_mixer(rlp.get_args(BASE + ["--seed", "9", "--reprob", "0.1"])).seed == 9
    assert not any(hasattr(rlp.get_args([]), f) for f in list(rlp.MIX_FLAGS) + ["mix_seed"])


def test_cli_defaults_still_equal_the_reference():
    from test_host_probe import test_cli_defaults_equal_the_reference
    test_cli_defaults_equal_the_reference()


@pytest.mark.parametrize("extra", [["--mixup", "0.8", "--eval"], ["--reprob", "0.25", "--eval"], ["--cutmix", "1.0", "--ensembles"],
                                   ["--mixup", "-0.5"], ["--cutmix", "-1"], ["--mixup", "0.8", "--mixup_prob", "1.5"],
                                   ["--mixup", "0.8", "--mixup_switch_prob", "-0.1"], ["--reprob", "1.2"], ["--mixup", "0.8", "--mixup_mode", "half"],
                                   ["--cutmix_minmax", "0.5"], ["--cutmix_minmax", "0.6", "0.5"], ["--cutmix_minmax", "0", "0.5"],
                                   ["--cutmix_minmax", "0.5", "1.1"], ["--reprob", "0.25", "--recount", "0"], ["--reprob", "0.25", "--recount", "9"],
                                   ["--reprob", "0.25", "--remode", "noise"]])
def test_cli_refusals(extra):
    import run_linear_probe as rlp
    with pytest.raises((ValueError, SystemExit)):
        rlp.validate(rlp.get_args(BASE + extra))


def test_cli_ensembles_refusal_names_the_flag():
    import run_linear_probe as rlp
    with pytest.raises(ValueError, match="--ensembles"):
        rlp.validate(rlp.get_args(BASE + ["--mixup", "0.8", "--ensembles"]))


# ---------------------------------------------------------------------------------------------- the ops' argument checks (nothing is launched)
def test_ops_refuse_bad_arguments_without_a_device():
    import ctypes as C
    from uncertainty_vit_amd import native
    L = native.lib()
    ARG, SHAPE, WORKSPACE = -1, -2, -4
    B, S, R = 2, 8, 1
    buf = np.zeros(2 * B * 3 * S * S + 64, dtype=np.float32)          # host memory stands in: every call returns before it touches it
    x, out = buf.ctypes.data, buf.ctypes.data + 4 * B * 3 * S * S
    desc = BatchMixer(mixup_alpha=1.0, seed=1).draw(B, S, 0).desc
    boxes = np.zeros((B, R, 4), dtype=np.int32)
    need = L.uvit_op_mix_ws_bytes(B, R)
    assert need == 512 and L.uvit_op_mix_ws_bytes(0, 0) == SHAPE and L.uvit_op_mix_ws_bytes(1, 9) == SHAPE

    def call(d=desc, bx=boxes, xp=x, op=out, B=B, S=S, R=R, mode=0, ws=x, ws_bytes=need):
        return L.uvit_op_mix_batch(C.c_void_p(xp), C.c_void_p(op), C.c_void_p(d.ctypes.data), C.c_void_p(bx.ctypes.data), B, S, R, mode, 0, 0,
                                   C.c_void_p(ws), ws_bytes, None)

    assert call(xp=0) == ARG and call(op=0) == ARG and call(ws=0) == ARG and call(mode=3) == ARG and call(op=x) == ARG and call(op=x + 4) == ARG
    assert call(B=0) == SHAPE and call(S=0) == SHAPE and call(R=9) == SHAPE and call(ws_bytes=need - 1) == WORKSPACE
    for field, value, code in (("kind", 3, ARG), ("lam", 2.0, ARG), ("lam", float("nan"), ARG), ("partner", B, ARG), ("yh", S + 1, SHAPE), ("xl", -1, SHAPE)):
        d = desc.copy()
        d[1][field] = value
        assert call(d=d) == code, field
    bad = boxes.copy()
    bad[1, 0] = (4, 4, 5, 2)
    assert call(bx=bad) == SHAPE
    P1 = C.c_void_p(x)
    good = [P1, P1, P1, P1, C.c_float(0.1), P1, P1, P1, 4, 10, None]
    for i, v, code in ((0, None, ARG), (2, None, ARG), (3, None, ARG), (7, None, ARG), (4, C.c_float(1.0), ARG), (8, 0, SHAPE), (9, 0, SHAPE)):
        a = list(good)
        a[i] = v
        assert L.uvit_op_probe_ce_mix(*a) == code, i
    assert not buf.any()
