"""GPU: the ensemble probe head (csrc/ens.hip, uncertainty-vit_amd/ens_probe.py) against the float64 restatement of tests/ens_ref.py
on the same inputs.

Tolerance: CPU_ERR below is the error of torch's fp32 CPU evaluation of ens_ref's formulas against their float64 form on the inputs
of the test, (max-norm error / max|ref|, relative L2 error), measured once on the CPU (`PYTHONPATH=. python tests/test_gpu_ens.py`
prints the table) and written here; the kernel is allowed 4 x that -- the margin for another summation order and the device's expf /
logf -- as tests/test_gpu_gp.py and tests/test_gpu_het.py do.  An output whose reference is all zeros has to be all zeros.  Two
outputs have derived bounds: the clip's norms (squares of fp32 are exact in double and the double sum is far below float
resolution: |norm - ref| <= 2^-23 |ref|) and the clipped gradient (one rounding of the norm, one of the quotient, one of the product:
2^-21 |ref| per element).  Integer outputs -- weights, counters, the disagreement count -- are compared for equality; the inputs keep
that meaningful: on the float64 reference the two largest values of every z row and of every member row are at least 1e-4 apart and
no logit lies within 1e-4 of the label's (asserted; another seed is the remedy, not a looser test).  Every test prints what it
measures before it asserts."""
import math

import pytest
import torch

import ens_ref as er
import probe_ref as pr
from test_gpu_probe import P, S as STREAM, f32, fixture_probe, frozen_state, guard_intact, guarded, ok, rnd

pytestmark = pytest.mark.gpu

F64 = torch.float64
SEED = 42
GAP = 1e-4

# (B, M, K): the smallest; K at the top-5 edge; one class past a wave with B not a multiple of the rows per workgroup; the largest M;
# the production K
SHAPES = [(1, 1, 1), (3, 2, 5), (5, 3, 67), (2, 16, 130), (2, 5, 1000)]
# (M, K, C): the smallest aligned case; bias segments off 16-byte alignment; a larger unaligned case; the largest M
CLIP_SHAPES = [(1, 4, 8), (3, 3, 8), (5, 10, 128), (16, 7, 64)]
MODEL = dict(K=10, M=3, init_scale=5.0, lr=1e-3, wd=0.05, bag_seed=7)
UNC = ("total", "aleatoric", "mi", "var")

# fp32 CPU error against float64: {op: {case: {output: (max-norm / max|ref|, relative L2)}}}
# BEGIN CPU_ERR
CPU_ERR = {'ce': {((1, 1, 1), False, 0.1): {'row_loss': (0.0, 0.0), 'loss': (0.0, 0.0), 'dlin': (805000000.0, 805000000.0)},
        ((1, 1, 1), False, 0.0): {'row_loss': (0.0, 0.0), 'loss': (0.0, 0.0), 'dlin': (0.0, 0.0)},
        ((1, 1, 1), True, 0.1): {'row_loss': (0.0, 0.0), 'loss': (0.0, 0.0), 'dlin': (805000000.0, 805000000.0)},
        ((1, 1, 1), True, 0.0): {'row_loss': (0.0, 0.0), 'loss': (0.0, 0.0), 'dlin': (0.0, 0.0)},
        ((3, 2, 5), False, 0.1): {'row_loss': (3.78e-08, 4.08e-08), 'loss': (3.98e-08, 4.28e-08), 'dlin': (1.05e-07, 7.54e-08)},
        ((3, 2, 5), False, 0.0): {'row_loss': (2.85e-08, 3.2e-08), 'loss': (5.41e-08, 4.18e-08), 'dlin': (8.35e-08, 5.87e-08)},
        ((3, 2, 5), True, 0.1): {'row_loss': (3.78e-08, 4.08e-08), 'loss': (6.13e-08, 5.24e-08), 'dlin': (1.23e-07, 9.01e-08)},
        ((3, 2, 5), True, 0.0): {'row_loss': (2.85e-08, 3.2e-08), 'loss': (5.41e-08, 4.32e-08), 'dlin': (5.82e-08, 5.31e-08)},
        ((5, 3, 67), False, 0.1): {'row_loss': (9.87e-08, 5.54e-08), 'loss': (3.65e-08, 3.12e-08), 'dlin': (5.86e-08, 4.03e-08)},
        ((5, 3, 67), False, 0.0): {'row_loss': (4.78e-08, 4.25e-08), 'loss': (7.61e-08, 6.48e-08), 'dlin': (4.48e-08, 3.32e-08)},
        ((5, 3, 67), True, 0.1): {'row_loss': (9.87e-08, 5.54e-08), 'loss': (4.35e-08, 4.26e-08), 'dlin': (2.87e-08, 3.64e-08)},
        ((5, 3, 67), True, 0.0): {'row_loss': (4.78e-08, 4.25e-08), 'loss': (4.16e-08, 3.8e-08), 'dlin': (4.92e-08, 4.02e-08)},
        ((2, 16, 130), False, 0.1): {'row_loss': (7.59e-08, 5.03e-08), 'loss': (8.74e-08, 5.22e-08), 'dlin': (5.1e-08, 3.11e-08)},
        ((2, 16, 130), False, 0.0): {'row_loss': (9.37e-08, 3.88e-08), 'loss': (5.38e-08, 3.92e-08), 'dlin': (4.3e-08, 2.71e-08)},
        ((2, 16, 130), True, 0.1): {'row_loss': (7.59e-08, 5.03e-08), 'loss': (5.2e-08, 4.72e-08), 'dlin': (2.76e-08, 3.04e-08)},
        ((2, 16, 130), True, 0.0): {'row_loss': (9.37e-08, 3.88e-08), 'loss': (2.98e-08, 3.14e-08), 'dlin': (2.27e-08, 2.73e-08)},
        ((2, 5, 1000), False, 0.1): {'row_loss': (6.49e-08, 5.59e-08), 'loss': (6.18e-08, 4.05e-08), 'dlin': (3.68e-08, 2.58e-08)},
        ((2, 5, 1000), False, 0.0): {'row_loss': (4.55e-08, 3.06e-08), 'loss': (6.84e-08, 4.25e-08), 'dlin': (2.75e-08, 2.12e-08)},
        ((2, 5, 1000), True, 0.1): {'row_loss': (6.49e-08, 5.59e-08), 'loss': (1.08e-07, 7.58e-08), 'dlin': (5.89e-08, 3.95e-08)},
        ((2, 5, 1000), True, 0.0): {'row_loss': (4.55e-08, 3.06e-08), 'loss': (4.71e-08, 4.95e-08), 'dlin': (4.57e-08, 3.27e-08)}},
 'combine': {((1, 1, 1), 0): {'z': (0.0, 0.0), 'total': (0.0, 0.0), 'aleatoric': (0.0, 0.0), 'mi': (0.0, 0.0), 'var': (0.0, 0.0)},
             ((1, 1, 1), 1): {'z': (0.0, 0.0), 'total': (0.0, 0.0), 'aleatoric': (0.0, 0.0), 'mi': (0.0, 0.0), 'var': (0.0, 0.0)},
             ((3, 2, 5), 0): {'z': (2.91e-08, 3.07e-08),
                              'total': (2.07e-08, 1.95e-08),
                              'aleatoric': (2.79e-08, 2.16e-08),
                              'mi': (3.95e-08, 3.17e-08),
                              'var': (1.91e-07, 2.17e-07)},
             ((3, 2, 5), 1): {'z': (5.91e-08, 6.35e-08),
                              'total': (2.07e-08, 1.95e-08),
                              'aleatoric': (2.79e-08, 2.16e-08),
                              'mi': (3.95e-08, 3.17e-08),
                              'var': (1.91e-07, 2.17e-07)},
             ((5, 3, 67), 0): {'z': (6.95e-08, 4.65e-08),
                               'total': (8.63e-08, 5.57e-08),
                               'aleatoric': (8.11e-08, 5.05e-08),
                               'mi': (9.03e-08, 8.24e-08),
                               'var': (3.35e-07, 3.03e-07)},
             ((5, 3, 67), 1): {'z': (9.3e-08, 4.04e-08),
                               'total': (8.63e-08, 5.57e-08),
                               'aleatoric': (8.11e-08, 5.05e-08),
                               'mi': (9.03e-08, 8.24e-08),
                               'var': (1.63e-07, 2.02e-07)},
             ((2, 16, 130), 0): {'z': (1.24e-07, 7.84e-08),
                                 'total': (3.07e-08, 3.04e-08),
                                 'aleatoric': (2.91e-08, 2.78e-08),
                                 'mi': (3.86e-08, 3.7e-08),
                                 'var': (1.4e-07, 1.64e-07)},
             ((2, 16, 130), 1): {'z': (6.68e-08, 3.69e-08),
                                 'total': (3.07e-08, 3.04e-08),
                                 'aleatoric': (2.91e-08, 2.78e-08),
                                 'mi': (3.86e-08, 3.7e-08),
                                 'var': (4.57e-07, 4.31e-07)},
             ((2, 5, 1000), 0): {'z': (7.54e-08, 5.03e-08),
                                 'total': (1.45e-07, 1.03e-07),
                                 'aleatoric': (1.39e-07, 9.86e-08),
                                 'mi': (1.76e-07, 1.27e-07),
                                 'var': (5.31e-07, 5.33e-07)},
             ((2, 5, 1000), 1): {'z': (1.01e-07, 4.35e-08),
                                 'total': (1.45e-07, 1.03e-07),
                                 'aleatoric': (1.39e-07, 9.86e-08),
                                 'mi': (1.76e-07, 1.27e-07),
                                 'var': (8.72e-07, 8.38e-07)}},
 'model': {'step': {'z': (8e-08, 8.39e-08),
                    'lin': (9.27e-08, 7.58e-08),
                    'loss': (2.65e-08, 2.6e-08),
                    'dW': (9.6e-08, 7.9e-08),
                    'dbias': (1.03e-07, 6.36e-08)},
           'plain': {'W0': (1.19e-07, 5.64e-08),
                     'b0': (1.28e-07, 5.89e-08),
                     'W1': (8.92e-08, 5.69e-08),
                     'b1': (1.37e-07, 6.08e-08),
                     'W2': (1.05e-07, 5.7e-08),
                     'b2': (1.22e-07, 7.82e-08)},
           'bagged': {'W0': (1.75e-07, 6.25e-08),
                      'b0': (1.29e-07, 6.61e-08),
                      'W1': (8.26e-08, 6.11e-08),
                      'b1': (1.04e-07, 6.96e-08),
                      'W2': (1.25e-07, 6.4e-08),
                      'b2': (8.97e-08, 5.06e-08)},
           'eval': {'member_loss': (4.97e-08, 4.41e-08),
                    'total': (8.29e-08, 4.52e-08),
                    'aleatoric': (7.77e-08, 4.35e-08),
                    'mi': (9.04e-08, 5.68e-08),
                    'var': (3.17e-07, 2.64e-07)}}}
# END CPU_ERR


def metrics(got, ref):
    """(max-norm error / max|ref|, relative L2 error) against a float64 reference; a reference of zeros asks for zeros."""
    d = got.detach().cpu().double() - ref
    if float(ref.abs().max()) == 0.0:
        return (0.0, 0.0) if float(d.abs().max()) == 0.0 else (math.inf, math.inf)
    return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())


def assert_within_4x(op, key, name, got, ref):
    m, lit = metrics(got, ref), CPU_ERR[op][key][name]
    print(f"\n{op} {key} {name}: GPU (max-norm, rel L2) = ({m[0]:.3e}, {m[1]:.3e}); fp32 CPU recorded {lit}")
    assert m[0] <= 4 * lit[0] and m[1] <= 4 * lit[1], (op, key, name, m, lit)


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


# ------------------------------------------------------------------------------------------------------------------------ inputs
RANKS = [0, 1, 4, 5, 2, 0]      # the label's rank among the logits of member b % M: 4 is the last top-5 hit, 5 the first miss

_IN = {}


def ens_inputs(B, M, K):
    """(lin (B, M K) fp32 of spread 2, labels (B,), w (B, M) float64 bagging weights), checked once on the float64 reference."""
    if (B, M, K) not in _IN:
        lin = rnd(B, M * K, seed=201, scale=2.0)
        x = lin.view(B, M, K).double()
        labels = torch.stack([x[b, b % M].argsort(descending=True)[min(RANKS[b % len(RANKS)], K - 1)] for b in range(B)])
        if K > 1:
            for mode in (0, 1):
                top = er.combine(lin, M, mode)[0].topk(2, dim=-1).values
                assert float((top[:, 0] - top[:, 1]).min()) >= GAP, "two z too close: choose another seed"
            top = x.topk(2, dim=-1).values
            assert float((top[..., 0] - top[..., 1]).min()) >= GAP, "two member logits too close: choose another seed"
            zy = x.gather(2, labels.view(B, 1, 1).expand(B, M, 1))
            gap = (x - zy).abs().scatter_(2, labels.view(B, 1, 1).expand(B, M, 1), math.inf)
            assert float(gap.min()) >= GAP, "a logit too close to the label's: choose another seed"
        _IN[(B, M, K)] = (lin, labels, er.bag_weights(B, M, SEED))
    return _IN[(B, M, K)]


_REF = {}


def ce_reference(shape, weighted, s, dtype=F64):
    key = ("ce", shape, weighted, s, dtype)
    if key not in _REF:
        B, M, K = shape
        lin, labels, w = ens_inputs(*shape)
        _REF[key] = er.ce(lin.view(B, M, K), labels, w if weighted else None, s, dtype)
    return _REF[key]


def combine_reference(shape, mode, dtype=F64):
    key = ("combine", shape, mode, dtype)
    if key not in _REF:
        _REF[key] = er.combine(ens_inputs(*shape)[0], shape[1], mode, dtype)
    return _REF[key]


# ----------------------------------------------------------------------------------------------------------------- bagging weights
@pytest.mark.parametrize("B,M", [(1, 1), (5, 3), (130, 16)])
def test_bag_weights(L, B, M):
    """The device's weights equal the restatement's exactly; nothing is written behind them; two runs and two seeds."""
    def run(seed):
        w = guarded(B * M)
        ok(L.uvit_op_ens_bag_weights(P(w), B, M, seed, STREAM()))
        torch.cuda.synchronize()
        assert guard_intact(w, B * M)
        return w[:B * M].view(B, M).cpu()

    a = run(SEED)
    print(f"\nbag weights ({B}, {M}): mean {float(a.mean()):.3f}, max {float(a.max())}")
    assert torch.equal(a.double(), er.bag_weights(B, M, SEED)) and torch.equal(run(SEED), a)
    assert torch.equal(run(er.step_seed(0, 3)).double(), er.bag_weights(B, M, er.step_seed(0, 3)))
    if B * M > 8:
        assert not torch.equal(run(SEED + 1), a)


# --------------------------------------------------------------------------------------------------------------------- criterion
def run_ce(L, lin_g, y_g, w_g, s, B, M, K, want_grad=True, counters=None):
    d = guarded(B * M * K, 5.0) if want_grad else None
    rows, loss = guarded(B * M), guarded(M + 1)
    ok(L.uvit_op_ens_ce(P(lin_g), P(y_g), P(w_g), f32(s), P(d), P(rows), P(loss), P(counters), B, M, K, STREAM()))
    torch.cuda.synchronize()
    assert guard_intact(rows, B * M) and guard_intact(loss, M + 1) and (d is None or guard_intact(d, B * M * K, 5.0))
    return (None if d is None else d[:B * M * K].view(B, M, K).cpu()), rows[:B * M].view(B, M).cpu(), loss[:M + 1].cpu()


def counters_for(M):
    """(M, 2) int32 counters followed by sentinels."""
    c = torch.full((2 * M + 16,), -7, dtype=torch.int32, device="cuda")
    c[:2 * M] = 0
    return c


@pytest.mark.parametrize("s", [0.1, 0.0])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_ens_ce(L, shape, weighted, s):
    """Row losses, the M + 1 losses and dlin within 4 x the fp32 CPU error; the counters equal the restatement's and accumulate; the
    call without dlin and without counters gives the same loss bits; two runs give the same bits; guards intact."""
    B, M, K = shape
    lin, labels, w = ens_inputs(*shape)
    rows_ref, loss_ref, d_ref, c_ref = ce_reference(shape, weighted, s)
    lin_g, y_g, w_g = lin.cuda(), labels.cuda(), (w.float().cuda() if weighted else None)
    cnt = counters_for(M)
    d, rows, loss = run_ce(L, lin_g, y_g, w_g, s, B, M, K, counters=cnt)
    d2, rows2, loss2 = run_ce(L, lin_g, y_g, w_g, s, B, M, K, counters=cnt)
    assert torch.equal(d, d2) and torch.equal(rows, rows2) and torch.equal(loss, loss2)
    print(f"\nce {shape} weighted {weighted} s {s}: counters {cnt[:2 * M].tolist()}, float64 {c_ref.flatten().tolist()}")
    assert cnt[:2 * M].view(M, 2).cpu().tolist() == (2 * c_ref).tolist() and bool((cnt[2 * M:] == -7).all())
    assert int(c_ref.sum()) > 0
    d3, rows3, loss3 = run_ce(L, lin_g, y_g, w_g, s, B, M, K, want_grad=False)
    assert d3 is None and torch.equal(rows3, rows) and torch.equal(loss3, loss)
    key = (shape, weighted, s)
    assert_within_4x("ce", key, "row_loss", rows, rows_ref)
    assert_within_4x("ce", key, "loss", loss, loss_ref)
    assert_within_4x("ce", key, "dlin", d, d_ref)


@pytest.mark.parametrize("weighted", [False, True])
def test_member_outputs_do_not_depend_on_the_other_members(L, weighted):
    """Member m's row_loss, loss and dlin bits from an M = 3 call equal those of an M = 1 call on that member's slice."""
    B, M, K = 5, 3, 67
    lin, labels, w = ens_inputs(B, M, K)
    lin_g, y_g, w_g = lin.cuda(), labels.cuda(), w.float().cuda()
    d, rows, loss = run_ce(L, lin_g, y_g, w_g if weighted else None, 0.1, B, M, K)
    for m in range(M):
        one = lin_g.view(B, M, K)[:, m].contiguous()
        wm = w_g[:, m].contiguous() if weighted else None
        d1, rows1, loss1 = run_ce(L, one, y_g, wm, 0.1, B, 1, K)
        assert torch.equal(d1[:, 0], d[:, m]) and torch.equal(rows1[:, 0], rows[:, m]) and torch.equal(loss1[0], loss[m])


@pytest.mark.parametrize("bad", [-1, 0, 5])
def test_ens_ce_label_out_of_range(L, bad):
    """A label outside [0, K): that row's loss and gradient are NaN for every member, so is every loss of the call; the other rows
    keep their bits, the counters skip the row, and nothing is read at the label."""
    B, M, K = 5, 3, 67
    lin, labels, _ = ens_inputs(B, M, K)
    lin_g = lin.cuda()
    good_d, good_rows, _ = run_ce(L, lin_g, labels.cuda(), None, 0.1, B, M, K)
    yb = labels.clone()
    yb[3] = -1 if bad < 0 else K + bad * 10 ** 9
    cnt = counters_for(M)
    d, rows, loss = run_ce(L, lin_g, yb.cuda(), None, 0.1, B, M, K, counters=cnt)
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(rows[3]).all()) and bool(torch.isnan(d[3]).all())
    keep = [i for i in range(B) if i != 3]
    assert torch.equal(rows[keep], good_rows[keep]) and torch.equal(d[keep], good_d[keep])
    c_ref = er.ce(lin.view(B, M, K)[keep], labels[keep], None, 0.1)[3]
    assert cnt[:2 * M].view(M, 2).cpu().tolist() == c_ref.tolist()
    assert torch.equal(c_ref, er.ce(lin.view(B, M, K), yb, None, 0.1)[3])


# -------------------------------------------------------------------------------------------------------------------------- clip
def clip_inputs(M, K, Cd):
    """A gradient arena whose members have different norms (member m is scaled by m + 1), without the arena's padding."""
    n = M * K * Cd + M * K
    g = rnd(n, seed=301, scale=0.01)
    for m, (wl, wh, bl, bh) in enumerate(er.segments(M, K, Cd)):
        g[wl:wh] *= m + 1
        g[bl:bh] *= m + 1
    return g


@pytest.mark.parametrize("which", ["zero", "below", "between", "above"])
@pytest.mark.parametrize("shape", CLIP_SHAPES)
def test_ens_clip(L, shape, which):
    """max_norm = 0, below every member's norm, between the norms and above every norm: the norms within 2^-23 relative, every
    element of the clipped gradient within 2^-21 relative, members under max_norm (and everything at max_norm <= 0) keep their bits;
    nothing is written behind the arena or the norms; two runs, and a run on an arena off 16-byte alignment, give the same bits."""
    M, K, Cd = shape
    g = clip_inputs(*shape)
    n = g.numel()
    norms0, _ = er.clip(g, M, K, Cd, 0.0)
    srt = norms0.sort().values
    max_norm = {"zero": 0.0, "below": 0.5 * float(srt[0]), "between": float(srt[0] + srt[-1]) / 2 if M > 1 else 0.999 * float(srt[0]),
                "above": 2.0 * float(srt[-1])}[which]
    norms_ref, g_ref = er.clip(g, M, K, Cd, max_norm)

    def run():
        ga, no = guarded(n), guarded(M)
        ga[:n] = g.cuda()
        ok(L.uvit_op_ens_clip(P(ga), P(no), M, K, Cd, f32(max_norm), STREAM()))
        torch.cuda.synchronize()
        assert guard_intact(ga, n) and guard_intact(no, M)
        return ga[:n].cpu(), no[:M].cpu()

    (out, norms), (out2, norms2) = run(), run()
    assert torch.equal(out, out2) and torch.equal(norms, norms2)
    # an arena that is not 16-byte aligned is read with 4-byte loads in the same order: the same bits
    off = guarded(n + 1)
    off[1:n + 1] = g.cuda()
    no = guarded(M)
    assert off[1:].data_ptr() % 16 == 4
    ok(L.uvit_op_ens_clip(P(off[1:]), P(no), M, K, Cd, f32(max_norm), STREAM()))
    torch.cuda.synchronize()
    assert float(off[0]) == 7.5 and guard_intact(off, n + 1) and torch.equal(off[1:n + 1].cpu(), out) and torch.equal(no[:M].cpu(), norms)
    nerr = float(((norms.double() - norms_ref).abs() / norms_ref).max())
    gerr = float(((out.double() - g_ref).abs() / g_ref.abs().clamp_min(1e-300)).max())
    clipped = [m for m in range(M) if max_norm > 0 and float(norms_ref[m]) + 1e-6 > max_norm]
    print(f"\nclip {shape} {which} (max_norm {max_norm:.4g}): norm error {nerr:.2e} (2^-23 = {2 ** -23:.2e}), gradient error {gerr:.2e} "
          f"(2^-21 = {2 ** -21:.2e}), members clipped {clipped}")
    assert nerr <= 2.0 ** -23 and gerr <= 2.0 ** -21
    if which == "between":
        assert 0 < len(clipped) < M or M == 1 and len(clipped) == 1
    else:
        assert len(clipped) == {"zero": 0, "below": M, "above": 0}[which]
    for m, (wl, wh, bl, bh) in enumerate(er.segments(M, K, Cd)):
        if m not in clipped:
            assert torch.equal(out[wl:wh], g[wl:wh]) and torch.equal(out[bl:bh], g[bl:bh])
        else:
            after = math.sqrt(float((out[wl:wh].double() ** 2).sum() + (out[bl:bh].double() ** 2).sum()))
            assert abs(after - max_norm) <= 1e-5 * max_norm + 1e-6


def test_ens_clip_leaves_a_poisoned_member(L):
    """A member with an infinite entry: its norm is inf, its entries keep their bits; the other members are clipped as usual."""
    M, K, Cd = 3, 3, 8
    g = clip_inputs(M, K, Cd)
    g[K * Cd + 5] = float("inf")
    norms_ref, g_ref = er.clip(g, M, K, Cd, 1e-3)
    ga, no = g.cuda(), torch.zeros(M, device="cuda")
    ok(L.uvit_op_ens_clip(P(ga), P(no), M, K, Cd, f32(1e-3), STREAM()))
    out, norms = ga.cpu(), no.cpu()
    assert math.isinf(float(norms[1])) and torch.equal(out[K * Cd:2 * K * Cd], g[K * Cd:2 * K * Cd])
    keep = torch.isfinite(g_ref)
    assert float(((out.double() - g_ref)[keep].abs() / g_ref[keep].abs().clamp_min(1e-300)).max()) <= 2.0 ** -21
    assert float(out[:K * Cd].abs().max()) < float(g[:K * Cd].abs().max())


# ------------------------------------------------------------------------------------------------------------------- combination
def run_combine(L, lin_g, mode, B, M, K, want_unc=True):
    z = guarded(B * K)
    unc = torch.full((5 * B + 16,), 7.5, dtype=F64, device="cuda")
    ok(L.uvit_op_ens_combine(P(lin_g), mode, P(z), P(unc if want_unc else None), B, M, K, STREAM()))
    torch.cuda.synchronize()
    assert guard_intact(z, B * K) and bool((unc[5 * B:] == 7.5).all())
    if not want_unc:
        assert bool((unc == 7.5).all())
    return z[:B * K].view(B, K).cpu(), unc[:5 * B].view(B, 5).cpu()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_ens_combine(L, shape, mode):
    """z and the four floating columns of unc within 4 x the fp32 CPU error; the prediction and the disagreement equal the
    restatement's; the call without unc gives the same z bits; two runs give the same bits; guards intact."""
    B, M, K = shape
    lin = ens_inputs(*shape)[0]
    z_ref, unc_ref, kstar, _ = combine_reference(shape, mode)
    lin_g = lin.cuda()
    (z, unc), (z2, unc2) = run_combine(L, lin_g, mode, B, M, K), run_combine(L, lin_g, mode, B, M, K)
    assert torch.equal(z, z2) and torch.equal(unc, unc2)
    assert torch.equal(run_combine(L, lin_g, mode, B, M, K, want_unc=False)[0], z)
    print(f"\ncombine {shape} mode {mode}: unc row 0 {unc[0].tolist()}; float64 {unc_ref[0].tolist()}")
    assert torch.equal(z.argmax(-1), kstar) and torch.equal(unc[:, 4], unc_ref[:, 4])
    assert bool((unc[:, 2] >= 0).all()) and bool((unc[:, 0] <= math.log(K) + 1e-6).all())
    assert_within_4x("combine", (shape, mode), "z", z, z_ref)
    for col, name in enumerate(UNC):
        assert_within_4x("combine", (shape, mode), name, unc[:, col], unc_ref[:, col])


def test_ens_combine_nan_row(L):
    """A NaN logit: five NaNs in that row's unc; the other rows keep their bits."""
    B, M, K = 5, 3, 67
    lin = ens_inputs(B, M, K)[0]
    lin_g = lin.cuda()
    _, good = run_combine(L, lin_g, 0, B, M, K)
    bad = lin.clone()
    bad[2, K + 7] = float("nan")
    for mode in (0, 1):
        z, unc = run_combine(L, bad.cuda(), mode, B, M, K)
        assert bool(torch.isnan(unc[2]).all()) and bool(torch.isnan(z[2, 7]))
        assert torch.equal(unc[[0, 1, 3, 4], :3], good[[0, 1, 3, 4], :3])


def test_ens_combine_extremes(L):
    """Identical members: no disagreement, mi below 1e-12, var_pred below 1e-24 (every member forms the same fp32 probabilities);
    members with all their mass on different classes: mi within 1e-6 of log M, the tie of z goes to the lowest index."""
    B, M, K = 4, 5, 11
    one = rnd(B, K, seed=205, scale=2.0)
    for mode in (0, 1):
        _, unc = run_combine(L, one.repeat(1, M).cuda(), mode, B, M, K)
        print(f"\nidentical members, mode {mode}: mi {float(unc[:, 2].max()):.2e}, var {float(unc[:, 3].max()):.2e}")
        assert float(unc[:, 2].max()) <= 1e-12 and float(unc[:, 3].max()) <= 1e-24 and float(unc[:, 4].max()) == 0.0
    lin = torch.zeros(2, 4, 6)
    for m in range(4):
        lin[:, m, m] = 40.0
    z, unc = run_combine(L, lin.view(2, 24).cuda(), 1, 2, 4, 6)
    print(f"disjoint members: mi {float(unc[0, 2]):.9f}, log M {math.log(4):.9f}")
    assert abs(float(unc[0, 2]) - math.log(4)) <= 1e-6 and float(unc[0, 4]) == 0.75 and int(z[0].argmax()) == 0


# --------------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


def ens_probe(case, members=MODEL["M"], **kw):
    """EnsembleProbe on the encoder of probe_t48.npz, its heads drawn under seed 5 with logits of spread about 1."""
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    enc = fixture_probe(case).encoder
    torch.manual_seed(5)
    return EnsembleProbe(enc, MODEL["K"], members=members, smoothing=float(case[0]["smoothing"]), init_scale=MODEL["init_scale"], **kw)


def head_of(probe):
    """(W (M K, C), bias (M K)) of the arena, on the host."""
    n, rows = probe._n_decay, probe._rows
    return probe._arena[:n].view(rows, probe.embed_dim).cpu().clone(), probe._arena[n:n + rows].cpu().clone()


def model_gaps(lin, labels, M):
    """The model-level inputs keep the integer outputs meaningful (see the module docstring)."""
    B = lin.shape[0]
    x = lin.view(B, M, -1)
    top = x.topk(2, dim=-1).values
    ztop = er.combine(lin, M, 0)[0].topk(2, dim=-1).values
    idx = labels.view(B, 1, 1).expand(B, M, 1)
    gap = (x - x.gather(2, idx)).abs().scatter_(2, idx, math.inf)
    return min(float((top[..., 0] - top[..., 1]).min()), float((ztop[:, 0] - ztop[:, 1]).min()), float(gap.min()))


def test_ensemble_step_against_ens_ref(case):
    """z, the M + 1 losses and the gradient arena of one train_step against ens_ref on the features the probe itself pooled, within
    4 x the fp32 CPU error recorded for this head on the float64 oracle's features of the same images."""
    fx, cfg, enc, _, _, images, labels = case
    M, s = MODEL["M"], float(fx["smoothing"])
    probe = ens_probe(case)
    xg, yg = images.cuda(), labels.cuda()
    feats = probe.features(xg).cpu()
    W, bias = head_of(probe)
    loss_ref, dW, db, lin_ref = er.grads(feats, W, bias, labels, M, s)
    assert_within_4x("model", "step", "z", probe.logits(xg), er.combine(lin_ref, M, 0)[0])
    assert_within_4x("model", "step", "lin", probe.member_logits(xg).flatten(1), lin_ref)
    loss, gnorm = probe.train_step(xg, yg, MODEL["lr"], MODEL["wd"])
    n, rows = probe._n_decay, probe._rows
    assert_within_4x("model", "step", "loss", probe._member_loss, loss_ref)
    assert float(loss) == float(probe._member_loss[M])
    assert_within_4x("model", "step", "dW", probe._grad_arena[:n].view(rows, -1), dW)
    assert_within_4x("model", "step", "dbias", probe._grad_arena[n:n + rows], db)
    norms_ref, _ = er.clip(torch.cat([dW.flatten(), db]), M, MODEL["K"], cfg.embed_dim, 0.0)
    lit = CPU_ERR["model"]["step"]
    bound = 4 * max(lit["dW"][1], lit["dbias"][1]) + 2.0 ** -23          # | ||g + e|| - ||g|| | <= ||e||
    nerr = float(((probe.member_norms.cpu().double() - norms_ref).abs() / norms_ref).max())
    total = float(norms_ref.pow(2).sum().sqrt())
    print(f"\nmember norms {probe.member_norms.tolist()}, error {nerr:.2e} (bound {bound:.2e}); arena norm {float(gnorm):.6f}, float64 {total:.6f}")
    assert nerr <= bound and abs(float(gnorm) - total) <= bound * total
    assert probe.step_count == 1


@pytest.mark.parametrize("bagging", [False, True])
def test_three_steps_against_ens_ref(case, bagging):
    """Three AdamW steps on the fixture's batch.  Without bagging and clip: every member's head, and a LinearProbe trained alone from
    the same initial bits on the same batches, are within 4 x the fp32 CPU error of the float64 restatement (the direct difference
    between the two is printed: the members train as if alone).  With bagging and a max_norm below every member's norm: the members
    against the restatement.  The encoder's parameters and bf16 shadows keep their bits."""
    from uncertainty_vit_amd.linear_probe import LinearProbe
    fx, cfg, enc, _, _, images, labels = case
    M, K, s, lr, wd = MODEL["M"], MODEL["K"], float(fx["smoothing"]), MODEL["lr"], MODEL["wd"]
    probe = ens_probe(case, bagging=bagging, seed=MODEL["bag_seed"])
    xg, yg = images.cuda(), labels.cuda()
    feats = probe.features(xg).cpu()
    W, bias = head_of(probe)
    max_norm = None
    if bagging:
        _, n0, _ = er.train_steps(feats, W, bias, labels, M, s, lr, wd, 1, MODEL["bag_seed"])
        max_norm = 0.5 * min(n0[0])
    _, norms_ref, (Wp, bp) = er.train_steps(feats, W, bias, labels, M, s, lr, wd, 3, MODEL["bag_seed"] if bagging else None, max_norm)
    alone = []
    if not bagging:
        for m in range(M):
            lp = LinearProbe(probe.encoder, K, smoothing=s)
            lp.load_state_dict(probe.member_state_dict(m))
            alone.append(lp)
    before = frozen_state(probe)
    for _ in range(3):
        probe.train_step(xg, yg, lr, wd, max_norm)
        for lp in alone:
            lp.train_step(xg, yg, lr, wd)
    for a, b in zip(before, frozen_state(probe)):
        assert torch.equal(a, b)
    W3, b3 = head_of(probe)
    key = "bagged" if bagging else "plain"
    if bagging:
        print(f"\nmax_norm {max_norm:.5f}; member norms of step 2 {probe.member_norms.tolist()}, float64 {norms_ref[2]}")
        assert all(n > max_norm for step in norms_ref for n in step)
    for m in range(M):
        assert_within_4x("model", key, f"W{m}", W3[m * K:(m + 1) * K], Wp[m * K:(m + 1) * K])
        assert_within_4x("model", key, f"b{m}", b3[m * K:(m + 1) * K], bp[m * K:(m + 1) * K])
        if not bagging:
            lw, lb = alone[m].head.weight.data.cpu(), alone[m].head.bias.data.cpu()
            print(f"member {m} against a LinearProbe trained alone: max |dW| {float((lw - W3[m * K:(m + 1) * K]).abs().max()):.2e}, "
                  f"max |db| {float((lb - b3[m * K:(m + 1) * K]).abs().max()):.2e}")
            assert_within_4x("model", key, f"W{m}", lw, Wp[m * K:(m + 1) * K])
            assert_within_4x("model", key, f"b{m}", lb, bp[m * K:(m + 1) * K])
    assert probe.step_count == 3


def test_evaluate_members_and_uncertainty(case):
    """evaluate(members=True, uncertainty=True) over two batches: the base keys equal the plain evaluation's; the members' counts equal
    the restatement's, their losses are within 4 x the fp32 CPU error; uncertainty() is within it column by column with the
    disagreement exact, and the set means are the means of its rows; evaluate twice gives identical numbers."""
    fx, cfg, _, _, _, images, labels = case
    M, K = MODEL["M"], MODEL["K"]
    probe = ens_probe(case)
    xg = images.cuda()
    batches = [((xg, None), labels), ((xg[:3], None), labels[:3])]
    e1, e2 = probe.evaluate(batches, members=True, uncertainty=True), probe.evaluate(batches, members=True, uncertainty=True)
    plain = probe.evaluate(batches)
    print(f"\nevaluate: {e1}")
    assert e1 == e2 and "member_loss" not in plain and "ens_mi" not in plain and {k: e1[k] for k in plain} == plain
    feats = probe.features(xg).cpu()
    W, bias = head_of(probe)
    lin = er.head_lin(feats, W, bias)
    print(f"smallest gap of the float64 logits {model_gaps(lin, labels, M):.2e}")
    assert model_gaps(lin, labels, M) >= GAP
    both, y = torch.cat([lin, lin[:3]]), torch.cat([labels, labels[:3]])
    _, loss_ref, _, c_ref = er.ce(both.view(-1, M, K), y, None, 0.0)
    n = xg.shape[0] + 3
    assert e1["n"] == n and e1["member_correct1"] == c_ref[:, 0].tolist() and e1["member_correct5"] == c_ref[:, 1].tolist()
    assert e1["member_acc1"] == [100.0 * c / n for c in c_ref[:, 0].tolist()]
    assert_within_4x("model", "eval", "member_loss", torch.tensor(e1["member_loss"], dtype=F64), loss_ref[:M])
    z_ref, unc_ref, _, _ = er.combine(lin, M, 0)
    c1, c5 = pr.topk_counts(torch.cat([z_ref, z_ref[:3]]), y)
    assert (e1["correct1"], e1["correct5"]) == (c1, c5)
    unc = probe.uncertainty(xg).cpu()
    assert unc.dtype == F64 and tuple(unc.shape) == (xg.shape[0], 5) and torch.equal(unc[:, 4], unc_ref[:, 4])
    for col, name in enumerate(UNC):
        assert_within_4x("model", "eval", name, unc[:, col], unc_ref[:, col])
    assert torch.equal(probe.uncertainty(xg[:3]).cpu(), unc[:3])
    rows = unc.tolist() + unc[:3].tolist()
    for col, k in enumerate(("ens_total", "ens_aleatoric", "ens_mi", "ens_var", "ens_disagreement")):
        assert e1[k] == math.fsum(r[col] for r in rows) / len(rows), k
    assert e1["ens_nan_rows"] == 0 and e1["ens_mi"] > 0


def test_one_member_is_the_linear_probe(case):
    """combine = "logits" with one member built from the fixture's head: evaluate returns LinearProbe.evaluate's counts exactly (and
    its loss: z = lin / 1)."""
    from uncertainty_vit_amd.ens_probe import EnsembleProbe
    fx, cfg, _, W, bias, images, labels = case
    lp = fixture_probe(case)
    ens = EnsembleProbe.from_heads(lp.encoder, [{"head.weight": W, "head.bias": bias}], smoothing=float(fx["smoothing"]))
    xg = images.cuda()
    batches = [((xg, None), labels), ((xg[:3], None), labels[:3])]
    a, b = lp.evaluate(batches), ens.evaluate(batches, members=True, uncertainty=True)
    print(f"\nlinear {a}\nensemble of one {b}")
    assert (a["n"], a["correct1"], a["correct5"]) == (b["n"], b["correct1"], b["correct5"]) and a["loss"] == b["loss"]
    assert b["member_correct1"] == [a["correct1"]] and b["member_correct5"] == [a["correct5"]]
    assert b["ens_mi"] == 0.0 and b["ens_disagreement"] == 0.0 and b["ens_var"] == 0.0
    assert torch.equal(ens.logits(xg), lp.logits(xg))


@pytest.mark.parametrize("combine", ["logits", "probs"])
def test_ensemble_is_a_function_of_the_image(case, combine):
    """A row's z is bit-equal in two batch positions; calibration_batch and stability_batch accept z; the state dict into a new
    ensemble gives equal logits; the optimizer state round-trips; "probs" gives normalised log-probabilities."""
    fx, cfg, _, _, _, images, labels = case
    probe = ens_probe(case, combine=combine)
    xg = images.cuda()
    z = probe.logits(xg)
    perm = torch.arange(xg.shape[0] - 1, -1, -1, device="cuda")
    assert torch.equal(probe.logits(xg[perm]), z[perm]) and torch.equal(probe.logits(xg[1:3]), z[1:3])
    ml = probe.member_logits(xg)
    assert tuple(ml.shape) == (xg.shape[0], MODEL["M"], MODEL["K"])
    if combine == "probs":
        torch.testing.assert_close(z.exp().sum(-1), torch.ones(xg.shape[0], device="cuda"), rtol=0, atol=1e-5)
    else:
        torch.testing.assert_close(z, ml.mean(1), rtol=1e-6, atol=1e-6)
    ece, tace, nll, auroc = probe.calibration_batch(z, labels.cuda())
    assert all(math.isfinite(float(v)) for v in (ece, tace, nll))
    seq = probe.stability_batch(z, 2, False)
    assert tuple(seq.shape) == (xg.shape[0] // 2, 3) and bool(torch.isfinite(seq).all())
    ev = probe.evaluate([((xg, None), labels)], calibration=True, members=True, uncertainty=True)
    assert all(math.isfinite(ev[k]) for k in ("ECE", "TACE", "NLL", "ens_total"))
    twin = ens_probe(case, combine=combine)
    twin.load_state_dict({k: v.cpu() + 0 for k, v in probe.state_dict().items()})
    assert torch.equal(twin.logits(xg), z)
    probe.train_step(xg, labels.cuda(), 1e-3, 0.05, 1.0)
    osd = probe.optimizer_state_dict()
    m0 = probe.exp_avg.clone()
    probe.exp_avg.zero_()
    probe.load_optimizer_state_dict(osd)
    assert osd["step"] == 1 and torch.equal(m0, probe.exp_avg) and float(m0.abs().max()) > 0
    assert not torch.equal(probe.logits(xg), z)


def test_ensemble_step_skips_a_poisoned_batch(case):
    """An out-of-range label: the loss is NaN and every head, its moments included, keeps its bits."""
    _, _, _, _, _, images, labels = case
    probe = ens_probe(case)
    bad = labels.clone()
    bad[2] = MODEL["K"]
    before = [t.clone() for t in (probe._arena, probe.exp_avg, probe.exp_avg_sq)]
    loss, _ = probe.train_step(images.cuda(), bad.cuda(), 1e-3, 0.05, 1.0)
    assert bool(torch.isnan(loss))
    for a, b in zip(before, (probe._arena, probe.exp_avg, probe.exp_avg_sq)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- the table above, measured on the CPU
def measure_cpu_err():
    """CPU_ERR: torch's fp32 CPU evaluation of ens_ref against its float64 form on the inputs of the tests above."""
    import os
    import pprint
    from uncertainty_vit_amd.linear_probe import _timm_trunc_normal_
    r3 = lambda m: tuple(float(f"{v:.2e}") for v in m)      # noqa: E731
    f32t = torch.float32
    out = {"ce": {}, "combine": {}, "model": {}}
    for shape in SHAPES:
        for weighted in (False, True):
            for s in (0.1, 0.0):
                ref, cpu = ce_reference(shape, weighted, s), ce_reference(shape, weighted, s, f32t)
                out["ce"][(shape, weighted, s)] = {n: r3(metrics(cpu[i], ref[i])) for i, n in ((0, "row_loss"), (1, "loss"), (2, "dlin"))}
        for mode in (0, 1):
            ref, cpu = combine_reference(shape, mode), combine_reference(shape, mode, f32t)
            entry = {"z": r3(metrics(cpu[0], ref[0]))}
            entry.update({n: r3(metrics(cpu[1][:, c], ref[1][:, c])) for c, n in enumerate(UNC)})
            assert torch.equal(cpu[1][:, 4], ref[1][:, 4])
            out["combine"][(shape, mode)] = entry
    # the module's step on the float64 oracle's features of the fixture's images, the heads EnsembleProbe draws under seed 5
    fx, cfg, enc, _, _, images, labels = pr.load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    M, K, s, lr, wd = MODEL["M"], MODEL["K"], float(fx["smoothing"]), MODEL["lr"], MODEL["wd"]
    feats = pr.features(enc, cfg, images).float()
    torch.manual_seed(5)
    W = torch.cat([_timm_trunc_normal_(torch.empty(K, cfg.embed_dim), std=0.02).mul_(MODEL["init_scale"]) for _ in range(M)])
    bias = torch.zeros(M * K)
    ref, cpu = er.grads(feats, W, bias, labels, M, s), er.grads(feats, W, bias, labels, M, s, None, f32t)
    assert model_gaps(ref[3], labels, M) >= GAP
    out["model"]["step"] = {"z": r3(metrics(er.combine(cpu[3], M, 0, f32t)[0], er.combine(ref[3], M, 0)[0])), "lin": r3(metrics(cpu[3], ref[3])),
                            "loss": r3(metrics(cpu[0], ref[0])), "dW": r3(metrics(cpu[1], ref[1])), "dbias": r3(metrics(cpu[2], ref[2]))}
    for key, seed in (("plain", None), ("bagged", MODEL["bag_seed"])):
        max_norm = None
        if seed is not None:
            max_norm = 0.5 * min(er.train_steps(feats, W, bias, labels, M, s, lr, wd, 1, seed)[1][0])
        (_, _, (Wp, bp)), (_, _, (Wc, bc)) = (er.train_steps(feats, W, bias, labels, M, s, lr, wd, 3, seed, max_norm, dt) for dt in (F64, f32t))
        out["model"][key] = {}
        for m in range(M):
            out["model"][key][f"W{m}"] = r3(metrics(Wc[m * K:(m + 1) * K], Wp[m * K:(m + 1) * K]))
            out["model"][key][f"b{m}"] = r3(metrics(bc[m * K:(m + 1) * K], bp[m * K:(m + 1) * K]))
    both, y = torch.cat([ref[3], ref[3][:3]]), torch.cat([labels, labels[:3]])
    both32 = torch.cat([cpu[3], cpu[3][:3]])
    entry = {"member_loss": r3(metrics(er.ce(both32.view(-1, M, K), y, None, 0.0, f32t)[1][:M], er.ce(both.view(-1, M, K), y, None, 0.0)[1][:M]))}
    u64, u32 = er.combine(ref[3], M, 0)[1], er.combine(cpu[3], M, 0, f32t)[1]
    entry.update({n: r3(metrics(u32[:, c], u64[:, c])) for c, n in enumerate(UNC)})
    out["model"]["eval"] = entry
    return "CPU_ERR = " + pprint.pformat(out, width=150, sort_dicts=False)


if __name__ == "__main__":
    print(measure_cpu_err())
