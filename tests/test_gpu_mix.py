"""GPU: csrc/mixup.hip -- uvit_op_mix_batch against the float32 restatement of tests/mix_ref.py (bit for bit outside the Box-Muller
fills, within the derived bound inside them), uvit_op_probe_ce_mix against float64, and a probe's training step with a mixer
(uncertainty-vit_amd/probe_mix.py, linear_probe.enable_mix) against float64 autograd on the tiny encoder of tests/test_gpu_probe.py."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import mix_ref as mr
import probe_ref as pr
from test_gpu_probe import fixture_probe
from uncertainty_vit_amd.probe_mix import MIX_DESC, BatchMixer

pytestmark = pytest.mark.gpu

ARG, SHAPE, WORKSPACE = -1, -2, -4
GUARD = 64
SEED = 0x5EED1234


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def STREAM():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host(a):
    return C.c_void_p(0 if a is None or a.size == 0 else a.ctypes.data)


def run_mix(L, x, desc, boxes, mode, seed=SEED, iteration=0, shift=0):
    """One uvit_op_mix_batch launch -> out (B, 3, S, S) as numpy.  x and out are followed by sentinels that must survive; `shift`
    moves both by that many floats off their 16-byte alignment."""
    B, _, S, _ = x.shape
    R = boxes.shape[1]
    n = x.size
    xg = torch.full((shift + n + GUARD,), 7.5, device="cuda")
    xg[shift:shift + n] = torch.from_numpy(x).cuda().view(-1)
    og = torch.full((shift + n + GUARD,), -3.25, device="cuda")
    need = L.uvit_op_mix_ws_bytes(B, R)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    desc, boxes = np.ascontiguousarray(desc), np.ascontiguousarray(boxes)
    rc = L.uvit_op_mix_batch(C.c_void_p(xg.data_ptr() + 4 * shift), C.c_void_p(og.data_ptr() + 4 * shift), host(desc), host(boxes), B, S, R, mode,
                             seed, iteration, P(ws), need, STREAM())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((og[shift + n:] == -3.25).all()) and bool((og[:shift] == -3.25).all()) and bool((xg[shift + n:] == 7.5).all())
    assert np.array_equal(xg[shift:shift + n].cpu().numpy().reshape(x.shape), x)               # the input is only read
    return og[shift:shift + n].cpu().numpy().reshape(x.shape)


def images(B, S, seed=0):
    return np.random.default_rng(seed).standard_normal((B, 3, S, S)).astype(np.float32)


# ---- the batches: eight row templates, dealt to the rows of as many batches as it takes to use every template at every B ----
def template(t, b, B, S):
    """(kind, lam, partner, yl, yh, xl, xh) of template t on row b."""
    flip = B - 1 - b
    full, empty = (0, S, 0, S), (S // 2, S // 2, 0, S)
    part = (S // 3, S - S // 4, S // 4, max(S // 4, S - S // 3))
    lam_of = lambda bx: 1.0 - (bx[1] - bx[0]) * (bx[3] - bx[2]) / float(S * S)      # noqa: E731
    return [(0, 1.0, flip) + empty, (1, 0.5, flip) + empty, (1, 0.0, flip) + full, (1, 1.0, flip) + full, (2, lam_of(empty), flip) + empty,
            (2, lam_of(full), flip) + full, (2, lam_of(part), flip) + part, (1, 0.25, b) + part][t]


def batches(B, S):
    for v in range((8 + B - 1) // B):
        desc = np.zeros(B, dtype=MIX_DESC)
        for b in range(B):
            desc[b] = template((v * B + b) % 8, b, B, S) + (0,)
        yield desc


def erase_boxes(B, S, R, seed=1):
    """R boxes per sample: the first covers everything but row 0 and column 0 (every other sample), the others are drawn, some absent
    (h = 0), some reaching the last row and column."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((B, R, 4), dtype=np.int32)
    for j, r in itertools.product(range(B), range(R)):
        if r == 0 and j % 2 == 0:
            boxes[j, r] = (1, 1, S - 1, S - 1) if S > 1 else (0, 0, 1, 1)
        elif rng.random() < 0.7:
            h, w = int(rng.integers(1, S + 1)), int(rng.integers(1, S + 1))
            boxes[j, r] = (S - h if rng.random() < 0.3 else int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w)
    return boxes


def compare(got, want, noisy, what):
    exact = ~noisy
    assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32)), (what, int((got[exact] != want[exact]).sum()))
    if noisy.any():
        err, tol = np.abs(got[noisy].astype(np.float64) - want[noisy]), mr.noise_tol(want[noisy].astype(np.float64))
        assert (err <= tol).all(), (what, float((err / tol).max()))
        return float((err / tol).max())
    return 0.0


@pytest.mark.parametrize("S", [1, 7, 20, 32])
@pytest.mark.parametrize("B", [1, 2, 5, 8])
def test_mix_batch_against_the_restatement(L, B, S):
    """Every kind, lam in {0, 0.5, 1}, an empty and a full-image cutmix box and a self-partner row, under R in {0, 1, 8} erase boxes in
    every erase mode: bit for bit outside the fills of `rand` / `pixel`, within mix_ref.noise_tol inside them.  S = 20 and 32 take the
    16-byte path, 1 and 7 the scalar one; 20 x 20 = 400 and 32 x 32 = 1024 pixels span more than one workgroup of 256 threads."""
    x = images(B, S, seed=B * 100 + S)
    worst, n_noisy, kinds = 0.0, 0, set()
    for desc in batches(B, S):
        kinds.update(desc["kind"].tolist())
        for R, mode in itertools.product((0, 1, 8), (0, 1, 2)):
            boxes = erase_boxes(B, S, R)
            want, noisy = mr.mix_batch(x, desc, boxes, mode, SEED, 3)
            got = run_mix(L, x, desc, boxes, mode, iteration=3)
            worst = max(worst, compare(got, want, noisy, (R, mode)))
            n_noisy += int(noisy.sum())
            assert not (mode == 0 and noisy.any())
    print(f"\nmix_batch B {B} S {S}: {n_noisy} noise values, worst error / bound {worst:.3f}")
    assert kinds == {0, 1, 2} and n_noisy > 0


@pytest.mark.parametrize("S", [20, 7])
def test_mix_batch_off_its_alignment(L, S):
    """x and out one float past a 16-byte boundary: the scalar path, the same values."""
    B = 5
    x, boxes = images(B, S, seed=9), erase_boxes(B, S, 8)
    for desc in batches(B, S):
        want, noisy = mr.mix_batch(x, desc, boxes, 2, SEED, 0)
        aligned, shifted = run_mix(L, x, desc, boxes, 2), run_mix(L, x, desc, boxes, 2, shift=1)
        assert np.array_equal(aligned.view(np.uint32), shifted.view(np.uint32))
        compare(shifted, want, noisy, "shifted")


def test_pixel_noise_statistics(L):
    """B = 8, S = 64, a 63 x 63 box per sample: 95,256 fills, mean within 5 / sqrt(n) of 0 and variance within 5 sqrt(2 / n) of 1."""
    B, S = 8, 64
    desc = next(batches(B, S))
    desc["kind"], desc["lam"] = 0, 1.0
    boxes = np.zeros((B, 1, 4), dtype=np.int32)
    boxes[:, 0] = (1, 0, 63, 63)
    out = run_mix(L, images(B, S), desc, boxes, 2)
    z = out[:, :, 1:, :63].astype(np.float64).ravel()
    n = z.size
    print(f"\npixel noise: n {n}, mean {z.mean():.3e} (se {1 / np.sqrt(n):.3e}), variance {z.var():.5f} (se {np.sqrt(2 / n):.3e})")
    assert n == 8 * 3 * 63 * 63 and abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    # `rand`: one value per (sample, channel)
    r = run_mix(L, images(B, S), desc, boxes, 1)[:, :, 1:, :63]
    assert (r == r[:, :, :1, :1]).all() and len(np.unique(r)) == B * 3


def test_noise_belongs_to_the_sample(L):
    """Sample j's fills are the same bits in out[j] and in the cutmix box of the row whose partner is j; two runs give the same bits;
    another iteration and another seed give other fills; a row's fills do not change when B grows from 4 to 8."""
    S = 32
    x8 = images(8, S, seed=4)
    boxes = np.zeros((8, 2, 4), dtype=np.int32)
    boxes[:, 0], boxes[:, 1] = (2, 3, 20, 17), (10, 0, 9, 32)
    desc = np.zeros(8, dtype=MIX_DESC)
    desc["partner"], desc["lam"] = 7 - np.arange(8), 1.0
    for b in range(4):                                     # rows 0..3 paste a window of their partners 7..4, which stay as they are
        desc[b] = (2, 0.5, 7 - b, 0, 32, 4, 28, 0)
    for mode in (1, 2):
        a, again = run_mix(L, x8, desc, boxes, mode), run_mix(L, x8, desc, boxes, mode)
        assert np.array_equal(a.view(np.uint32), again.view(np.uint32))
        for b in range(4):
            assert np.array_equal(a[b][:, :, 4:28], a[7 - b][:, :, 4:28])
        erased = np.zeros((S, S), dtype=bool)
        erased[2:22, 3:20] = erased[10:19, :] = True
        for other in (run_mix(L, x8, desc, boxes, mode, iteration=1), run_mix(L, x8, desc, boxes, mode, seed=SEED + 1)):
            assert not np.array_equal(other[4:][:, :, erased], a[4:][:, :, erased])
            assert np.array_equal(other[4:][:, :, ~erased], a[4:][:, :, ~erased])
        # the first four samples alone, none mixed: their erased values are those of the batch of eight
        plain = np.zeros(8, dtype=MIX_DESC)
        plain["partner"], plain["lam"] = 7 - np.arange(8), 1.0
        small_desc = plain[:4].copy()
        small_desc["partner"] = 3 - np.arange(4)
        small, big = run_mix(L, np.ascontiguousarray(x8[:4]), small_desc, boxes[:4], mode), run_mix(L, x8, plain, boxes, mode)
        assert np.array_equal(small.view(np.uint32), big[:4].view(np.uint32)) and not np.array_equal(big[:4], x8[:4])


def test_mix_batch_refuses_bad_arguments(L):
    """Every error returns its code before anything is launched: out keeps the pattern it held."""
    B, S, R = 4, 8, 2
    n = B * 3 * S * S
    x = torch.from_numpy(images(B, S)).cuda()
    out = torch.arange(n, dtype=torch.float32, device="cuda")
    pattern = out.clone()
    good_desc = np.zeros(B, dtype=MIX_DESC)
    good_desc["partner"], good_desc["lam"], good_desc["kind"] = B - 1 - np.arange(B), 0.5, [0, 1, 2, 2]
    good_desc["yh"], good_desc["xh"] = 4, 4
    good_boxes = np.zeros((B, R, 4), dtype=np.int32)
    good_boxes[:, 0] = (1, 1, 7, 7)
    need = L.uvit_op_mix_ws_bytes(B, R)
    assert need == 256 + 256 and L.uvit_op_mix_ws_bytes(B, 0) == 256 and L.uvit_op_mix_ws_bytes(9, 8) == 512 + 1280
    for b, r in ((0, 0), (65536, 0), (1, -1), (1, 9)):
        assert L.uvit_op_mix_ws_bytes(b, r) == SHAPE
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(desc=good_desc, boxes=good_boxes, xp=None, op=None, B=B, S=S, R=R, mode=2, wsp=None, ws_bytes=need, no_desc=False, no_boxes=False):
        rc = L.uvit_op_mix_batch(P(x) if xp is None else C.c_void_p(xp), P(out) if op is None else C.c_void_p(op), None if no_desc else host(desc),
                                 None if no_boxes else host(boxes), B, S, R, mode, 1, 0, P(ws) if wsp is None else C.c_void_p(wsp), ws_bytes, STREAM())
        torch.cuda.synchronize()
        assert torch.equal(out, pattern)
        return rc

    def desc_with(row, **kw):
        d = good_desc.copy()
        for k, v in kw.items():
            d[row][k] = v
        return d

    def boxes_with(j, r, box):
        b = good_boxes.copy()
        b[j, r] = box
        return b

    assert call(xp=0) == ARG and call(op=0) == ARG and call(no_desc=True) == ARG and call(wsp=0) == ARG and call(no_boxes=True) == ARG
    assert call(mode=3) == ARG and call(mode=-1) == ARG
    for bad in (dict(kind=3), dict(kind=-1), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")), dict(partner=-1), dict(partner=B)):
        assert call(desc=desc_with(1, **bad)) == ARG, bad
    for bad in (dict(yl=5, yh=4), dict(yh=S + 1), dict(xl=-1), dict(xl=3, xh=2), dict(xh=S + 1), dict(yl=-1)):
        assert call(desc=desc_with(0, **bad)) == SHAPE, bad       # a kind-0 row's box is checked too
    for box in ((0, 0, S + 1, 1), (1, 0, S, 1), (0, 1, 1, S), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, -1, 2), (0, 0, 2, 0), (0, 0, 2, -3)):
        assert call(boxes=boxes_with(3, 1, box)) == SHAPE, box
    assert call(B=0) == SHAPE and call(S=0) == SHAPE and call(S=4097) == SHAPE and call(R=9) == SHAPE and call(R=-1) == SHAPE
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    # out == x, and out overlapping x by one image row at either end: rows read their partners
    assert call(op=x.data_ptr()) == ARG
    assert call(op=x.data_ptr() + 4 * (n - S)) == ARG and call(xp=out.data_ptr() + 4 * (n - S)) == ARG
    assert call(op=x.data_ptr() + 2) == ARG                       # not a float pointer
    # and the same arguments untouched are accepted (out is then overwritten: the pattern check is skipped)
    rc = L.uvit_op_mix_batch(P(x), P(out), host(good_desc), host(good_boxes), B, S, R, 2, 1, 0, P(ws), need, STREAM())
    torch.cuda.synchronize()
    assert rc == 0 and not torch.equal(out, pattern)


# ------------------------------------------------------------------------------------------------------------- the soft-target loss
CE_SHAPES = [(1, 1), (2, 3), (5, 10), (8, 1000), (3, 1003)]


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ce_inputs(B, K):
    """Logits of spread 2, row 1 at +-80 as in tests/test_gpu_probe.py (its loss is about 166); labels that hold 0 and K - 1."""
    z = rnd(B, K, seed=21, scale=2.0)
    if B > 1:
        z[1] = rnd(K, seed=22) + 80.0 * (1.0 - 2.0 * (torch.arange(K) % 2))
    y = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(23))
    y[0] = K - 1
    if B > 1:
        y[1] = min(1, K - 1)
    if B > 2:
        y[2] = 0
    return z, y


def run_ce_mix(L, z, y, partner, lam, s, want_grad=True):
    B, K = z.shape
    zg, yg = z.cuda(), y.cuda()
    pg, lg = partner.to(torch.int32).cuda(), lam.to(torch.float32).cuda()
    d = torch.full((B * K + GUARD,), 7.5, device="cuda") if want_grad else None
    rows, loss = torch.full((B + GUARD,), 7.5, device="cuda"), torch.full((1 + GUARD,), 7.5, device="cuda")
    rc = L.uvit_op_probe_ce_mix(P(zg), P(yg), P(pg), P(lg), C.c_float(s), P(d), P(rows), P(loss), B, K, STREAM())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((rows[B:] == 7.5).all()) and bool((loss[1:] == 7.5).all()) and (d is None or bool((d[B * K:] == 7.5).all()))
    return (None if d is None else d[:B * K].view(B, K).cpu()), rows[:B].cpu(), loss[:1].cpu()


def lam_sets(B):
    mixed = torch.rand(B, generator=torch.Generator().manual_seed(31))
    mixed[0] = 0.0
    if B > 1:
        mixed[-1] = 1.0
    return {"zeros": torch.zeros(B), "ones": torch.ones(B), "mixed": mixed}


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("B,K", CE_SHAPES)
def test_soft_cross_entropy(L, B, K, smoothing):
    """Row losses, their mean and dlogits against the float64 dense-target form within mix_ref's bounds, for lam all 0, all 1 and mixed
    (0 and 1 among them), with the flipped batch as partners; two runs give the same bits; without dlogits the losses are the same."""
    z, y = ce_inputs(B, K)
    partner = torch.arange(B - 1, -1, -1)
    for name, lam in lam_sets(B).items():
        lam32 = lam.to(torch.float32)
        rows_ref, loss_ref, d_ref = mr.soft_ce(z, y, partner, lam32.double(), smoothing)
        d, rows, loss = run_ce_mix(L, z, y, partner, lam32, smoothing)
        err = (rows.double() - rows_ref).abs()
        tol = torch.tensor([mr.ce_loss_tol(float(r)) for r in rows_ref])
        print(f"\nce_mix {(B, K, smoothing, name)}: worst row error / bound {float((err / tol).max()):.3f}, dlogits error / bound "
              f"{float((d.double() - d_ref).abs().max()) / mr.ce_grad_tol(B):.3f}")
        assert bool((err <= tol).all())
        assert abs(float(loss) - float(loss_ref)) <= mr.ce_loss_tol(float(rows_ref.abs().max()))
        assert float((d.double() - d_ref).abs().max()) <= mr.ce_grad_tol(B)
        d2, rows2, loss2 = run_ce_mix(L, z, y, partner, lam32, smoothing)
        assert torch.equal(d, d2) and torch.equal(rows, rows2) and torch.equal(loss, loss2)
        d3, rows3, loss3 = run_ce_mix(L, z, y, partner, lam32, smoothing, want_grad=False)
        assert d3 is None and torch.equal(rows3, rows) and torch.equal(loss3, loss)


@pytest.mark.parametrize("B,K", CE_SHAPES)
def test_soft_cross_entropy_at_lam_one_is_the_hard_one(L, B, K):
    """lam = 1 everywhere against uvit_op_probe_ce on the same logits and labels: within the sum of the two ops' bounds."""
    z, y = ce_inputs(B, K)
    zg, yg = z.cuda(), y.cuda()
    d0, rows0, loss0 = torch.zeros(B, K, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(1, device="cuda")
    assert L.uvit_op_probe_ce(P(zg), P(yg), C.c_float(0.1), P(d0), P(rows0), P(loss0), None, B, K, STREAM()) == 0
    d, rows, loss = run_ce_mix(L, z, y, torch.arange(B - 1, -1, -1), torch.ones(B), 0.1)
    rows0, d0, loss0 = rows0.cpu(), d0.cpu(), loss0.cpu()
    for b in range(B):
        assert abs(float(rows[b]) - float(rows0[b])) <= 1e-5 * (1 + abs(float(rows0[b]))) + mr.ce_loss_tol(float(rows0[b]))
    assert abs(float(loss) - float(loss0)) <= 2 * mr.ce_loss_tol(float(rows0.abs().max()))
    assert float((d - d0).abs().max()) <= 1e-5 / B + mr.ce_grad_tol(B)


@pytest.mark.parametrize("what", ["own label", "own label negative", "partner label", "partner index", "partner index negative", "lam above",
                                  "lam below", "lam nan"])
def test_soft_cross_entropy_bad_rows(L, what):
    """One bad input: NaN in exactly the rows that read it and in *loss_out, the other rows as they are without it, nothing read at the
    bad index (a label of 10^9 and a partner of 10^9 would fault)."""
    B, K, s = 5, 10, 0.1
    z, y = ce_inputs(B, K)
    partner, lam = torch.arange(B - 1, -1, -1), torch.tensor([0.3, 0.6, 0.5, 0.2, 0.9])
    rows_ref, _, d_ref = mr.soft_ce(z, y, partner, lam.to(torch.float32).double(), s)
    y, partner, lam = y.clone(), partner.clone(), lam.clone()
    if what.startswith("own label"):
        y[3] = -1 if "negative" in what else K + 10 ** 9
        bad = {3, 1}                                       # row 1's partner is row 3
    elif what == "partner label":
        y[4] = K
        bad = {4, 0}
    elif what.startswith("partner index"):
        partner[2] = -1 if "negative" in what else 10 ** 9
        bad = {2}
    else:
        lam[1] = {"lam above": 1.0001, "lam below": -1e-6, "lam nan": float("nan")}[what]
        bad = {1}
    d, rows, loss = run_ce_mix(L, z, y, partner, lam, s)
    assert bool(torch.isnan(loss).all())
    for b in range(B):
        if b in bad:
            assert bool(torch.isnan(rows[b])) and bool(torch.isnan(d[b]).all()), b
        else:
            assert abs(float(rows[b]) - float(rows_ref[b])) <= mr.ce_loss_tol(float(rows_ref[b])), b
            assert float((d[b].double() - d_ref[b]).abs().max()) <= mr.ce_grad_tol(B), b


def test_soft_cross_entropy_refuses_bad_arguments(L):
    one = torch.zeros(64, device="cuda")
    P1, N = P(one), None
    good = [P1, P1, P1, P1, C.c_float(0.1), P1, P1, P1, 4, 10, STREAM()]
    for i in (0, 1, 2, 3, 6, 7):
        a = list(good)
        a[i] = N
        assert L.uvit_op_probe_ce_mix(*a) == ARG, i
    for s in (-0.1, 1.0, float("nan")):
        a = list(good)
        a[4] = C.c_float(s)
        assert L.uvit_op_probe_ce_mix(*a) == ARG, s
    for B, K in ((0, 10), (4, 0)):
        a = list(good)
        a[8], a[9] = B, K
        assert L.uvit_op_probe_ce_mix(*a) == SHAPE
    torch.cuda.synchronize()
    assert not one.any()


# --------------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


def test_train_step_with_a_mixer(case):
    """One step under an `elem` mixer with erasing against float64 autograd from probe.features(mixed images): the mixed images are the
    restatement's, the loss within tests/test_gpu_probe.py's 5e-3 relative, the head after the step within that file's weight bound
    for one step (lr + 1e-4; within 0.2 lr where the gradient is at least a tenth of the largest)."""
    fx, cfg, enc, W, bias, images_, labels = case
    lr, wd, s = float(fx["lr"]), float(fx["weight_decay"]), float(fx["smoothing"])
    probe = fixture_probe(case)
    mixer = BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", reprob=0.5, recount=2, seed=3)
    probe.enable_mix(mixer)
    xg, yg = images_.cuda(), labels.cuda()
    B, S = xg.shape[0], xg.shape[-1]
    draw = mixer.draw(B, S, probe.step_count)
    assert draw.active and set(draw.desc["kind"].tolist()) - {0}
    mixed = probe.mix_images(xg, draw).clone()
    want, noisy = mr.mix_batch(images_.numpy(), draw.desc, draw.boxes, draw.erase_mode, mixer.seed, probe.step_count)
    compare(mixed.cpu().numpy(), want, noisy, "train step")
    feat = probe.features(mixed).cpu().double()
    Wd, bd = W.double().clone().requires_grad_(True), bias.double().clone().requires_grad_(True)
    t = mr.soft_target(labels, torch.from_numpy(draw.partner), torch.from_numpy(draw.lam), W.shape[0], s)
    loss_ref = -(t * torch.log_softmax(feat @ Wd.t() + bd, dim=-1)).sum(-1).mean()
    loss_ref.backward()
    opt = pr.HeadAdamW(W, bias)
    opt.step([Wd.grad, bd.grad], lr, wd)
    loss, gnorm = probe.train_step(xg, yg, lr, wd)
    assert probe._mix is None and probe.step_count == 1
    assert float(loss) == pytest.approx(float(loss_ref.detach()), rel=5e-3) and np.isfinite(float(gnorm))
    gmax = max(float(Wd.grad.abs().max()), float(bd.grad.abs().max()))
    sd = probe.state_dict()
    for key, ref, g in (("head.weight", opt.p[0], Wd.grad), ("head.bias", opt.p[1], bd.grad)):
        got = sd[key].cpu().double()
        assert float((got - ref).abs().max()) <= lr + 1e-4, key
        big = g.abs() >= 0.1 * gmax
        assert int(big.sum()) > 0 and float((got - ref)[big].abs().max()) <= 0.2 * lr, key
    # the step differs from an unmixed one
    plain = fixture_probe(case)
    loss0, _ = plain.train_step(xg, yg, lr, wd)
    assert float(loss0) != float(loss) and not torch.equal(plain._arena, probe._arena)


def test_inactive_draws_leave_the_step_as_it_is(case):
    """A mixer whose draws are all inactive (prob 0, no erasing): the head after three steps holds the bits of a probe without one."""
    fx, _, _, _, _, images_, labels = case
    lr, wd = float(fx["lr"]), float(fx["weight_decay"])
    xg, yg = images_.cuda(), labels.cuda()
    probes = [fixture_probe(case), fixture_probe(case), fixture_probe(case)]
    probes[1].enable_mix(BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0))
    probes[2].enable_mix(BatchMixer(mixup_alpha=0.8))
    probes[2].enable_mix(None)
    losses = [[float(p.train_step(xg, yg, lr, wd)[0]) for _ in range(3)] for p in probes]
    assert losses[0] == losses[1] == losses[2]
    for p in probes[1:]:
        assert torch.equal(p._arena, probes[0]._arena) and torch.equal(p.exp_avg, probes[0].exp_avg) and p._mix_bufs is None


def test_other_heads_take_the_mixer(case):
    """The ensemble refuses; the layer-weighted and the GP probe take one mixed step each: finite loss, finite and changed heads."""
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    from uncertainty_vit_amd.gp_probe import GPProbe
    from uncertainty_vit_amd.lw_probe import LayerWeightedProbe
    fx, _, _, W, _, images_, labels = case
    enc, K = fixture_probe(case).encoder, W.shape[0]
    mixer = BatchMixer(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", reprob=0.5, seed=3)
    ens = EnsembleProbe(enc, K, members=2)
    with pytest.raises(NotImplementedError, match="ensemble"):
        ens.enable_mix(mixer)
    ens.enable_mix(None)
    xg, yg = images_.cuda(), labels.cuda()
    for cls in (LayerWeightedProbe, GPProbe):
        torch.manual_seed(5)
        probe = cls(enc, K, smoothing=0.1)
        probe.enable_mix(mixer)
        before = probe._arena.clone()
        loss, gnorm = probe.train_step(xg, yg, 1e-3, 0.05)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss)) and np.isfinite(float(gnorm)) and float(gnorm) > 0, cls.__name__
        assert bool(torch.isfinite(probe._arena).all()) and not torch.equal(before, probe._arena), cls.__name__
        assert probe._mix_bufs is not None and probe._mix is None
