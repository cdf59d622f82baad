"""GPU: the linear probe (csrc/probe.hip, uncertainty-vit_amd/linear_probe.py) against float64 torch on the same inputs
(tests/probe_ref.py) and against what the reference classifier computed (tests/golden/probe_t48.npz)."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import probe_ref as pr
from oracle.closed_form import closed_form_images

pytestmark = pytest.mark.gpu

ACT_RT, ACT_AT = 2e-2, 2e-2      # tests/test_gpu_model.py: activations O(1) behind the bf16 encoder


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    assert rc == 0, f"libuvit returned {rc}"


def f32(v):
    return C.c_float(v)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def metrics(got, ref):
    """(max-norm error / max|ref|, relative L2 error) against a float64 reference."""
    d = got.detach().cpu().double() - ref
    return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())


GUARD = 64


def guarded(n, fill=7.5):
    """n floats on the device followed by GUARD sentinels that no kernel may touch."""
    return torch.full((n + GUARD,), fill, device="cuda")


def guard_intact(t, n, fill=7.5):
    return bool((t[n:] == fill).all())


# ------------------------------------------------------------------------------------------------------------------- pool + norm
POOL_CASES = [(1, 2, 64, None), (3, 10, 128, None), (2, 197, 768, None), (1, 197, 1280, None), (5, 197, 1024, "cls"),
              (2, 197, 768, "offset"), (3, 10, 128, "offset")]


@pytest.mark.parametrize("B,N,Cd,variant", POOL_CASES)
def test_pool_norm(L, B, N, Cd, variant):
    """feat = LayerNorm_no_affine(mean of tokens 1..N-1) against float64.  Inputs: unit noise plus a per-(sample, channel) pattern of
    unit variance, so that the pooled row has a spread of about 1 as real features do.  "cls": token 0 is 1e4 (pooling it in moves
    every feature); "offset": 100 on every element (a one-pass E[x^2] - E[x]^2 variance loses 1e4 * 2^-24 = 6e-4 of a variance of 1).
    Bound: the one tests/test_gpu_ops.py::test_layernorm_production_rows has for ln_fwd's statistics -- the mean within 1e-4 of the
    row's standard deviation, rstd within 1e-4 relative -- which for the normalised output (t - mean) * rstd is
    |feat - ref| <= 1e-4 + 1e-4 |ref|.  One token row of 1,280 columns past the last, one slice with a single token (N = 2), a
    short last slice (196 = 7 x 25 + 21) and empty slices (N - 1 < 8) are all in the list.  Two runs give the same bits."""
    x = rnd(B, N, Cd, seed=11) + rnd(B, 1, Cd, seed=12)
    if variant == "cls":
        x[:, 0, :] = 1e4
    if variant == "offset":
        x = x + 100.0
    ref = pr.pool_norm(x, 1e-6)
    ws = L.uvit_op_probe_pool_ws_bytes(B, N, Cd)
    assert ws == B * 8 * Cd * 4
    xg = x.cuda()
    outs = []
    for _ in range(2):
        feat, scratch = guarded(B * Cd), guarded(ws // 4)
        ok(L.uvit_op_probe_pool_norm(P(xg), P(feat), P(scratch), B, N, Cd, f32(1e-6), S()))
        torch.cuda.synchronize()
        assert guard_intact(feat, B * Cd) and guard_intact(scratch, ws // 4)
        outs.append(feat[:B * Cd].view(B, Cd).clone())
    assert torch.equal(outs[0], outs[1])
    err = (outs[0].cpu().double() - ref).abs()
    tol = 1e-4 * (1.0 + ref.abs())
    print(f"\npool_norm {(B, N, Cd, variant)}: worst error / bound {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), (int((err / tol).argmax()), float((err / tol).max()))


# ------------------------------------------------------------------------------------------------------------- the two contractions
HEAD_SHAPES = [(1, 10, 64), (7, 200, 768), (128, 1000, 768), (3, 1003, 128)]
# torch's own fp32 CPU result against float64 on the inputs of contraction_inputs(): (max-norm error / max|ref|, relative L2 error)
CPU_ERR = {
    "logits": {(1, 10, 64): (7.97e-8, 8.30e-8), (7, 200, 768): (1.60e-7, 1.37e-7), (128, 1000, 768): (6.33e-7, 3.50e-7),
               (3, 1003, 128): (8.83e-8, 8.23e-8)},
    "dW": {(1, 10, 64): (2.98e-8, 2.60e-8), (7, 200, 768): (1.08e-7, 5.16e-8), (128, 1000, 768): (4.15e-7, 2.04e-7),
           (3, 1003, 128): (6.81e-8, 3.58e-8)},
    "dbias": {(1, 10, 64): (0.0, 0.0), (7, 200, 768): (4.96e-8, 5.23e-8), (128, 1000, 768): (1.11e-7, 1.04e-7),
              (3, 1003, 128): (4.99e-8, 3.50e-8)},
}


def contraction_inputs(B, K, Cd):
    return rnd(B, Cd, seed=1), rnd(K, Cd, seed=2, scale=0.05), rnd(K, seed=3, scale=0.1), rnd(B, K, seed=4, scale=1.0 / B)


def assert_within_4x(name, shape, got, ref, cpu):
    m = metrics(got, ref)
    now = metrics(cpu, ref)
    lit = CPU_ERR[name][shape]
    print(f"\n{name} {shape}: GPU (max-norm, rel L2) = ({m[0]:.3e}, {m[1]:.3e}); fp32 CPU here ({now[0]:.3e}, {now[1]:.3e}), recorded {lit}")
    assert m[0] <= 4 * lit[0] and m[1] <= 4 * lit[1], (name, shape, m, lit)


@pytest.mark.parametrize("B,K,Cd", HEAD_SHAPES)
def test_logits(L, B, K, Cd):
    """logits = feat . W^T + bias against float64.  Bound: 4 x the error of torch's own fp32 CPU result against float64 on the same
    inputs (the margin for another summation order), in the max norm and in relative L2.  Measured fp32 CPU errors
    (max-norm / max|ref|, relative L2): (1, 10, 64): 7.97e-8, 8.30e-8; (7, 200, 768): 1.60e-7, 1.37e-7; (128, 1000, 768): 6.33e-7,
    3.50e-7; (3, 1003, 128): 8.83e-8, 8.23e-8 (CPU_ERR above; the test prints what the CPU it runs on gives)."""
    feat, W, bias, _ = contraction_inputs(B, K, Cd)
    ref = pr.head_logits(feat, W, bias)
    out = guarded(B * K)
    fg, Wg, bg = feat.cuda(), W.cuda(), bias.cuda()
    ok(L.uvit_op_probe_logits(P(fg), P(Wg), P(bg), P(out), B, K, Cd, S()))
    torch.cuda.synchronize()
    assert guard_intact(out, B * K)
    assert_within_4x("logits", (B, K, Cd), out[:B * K].view(B, K), ref, feat @ W.t() + bias)


@pytest.mark.parametrize("B,K,Cd", HEAD_SHAPES)
def test_head_grad(L, B, K, Cd):
    """dW = dlogits^T . feat and dbias = column sums of dlogits against float64; the outputs held 5.0 before (they are overwritten,
    not added to) and two runs give the same bits.  Bound: 4 x torch's fp32 CPU error against float64 on the same inputs.  Measured
    (max-norm / max|ref|, relative L2), dW: (1, 10, 64): 2.98e-8, 2.60e-8; (7, 200, 768): 1.08e-7, 5.16e-8; (128, 1000, 768):
    4.15e-7, 2.04e-7; (3, 1003, 128): 6.81e-8, 3.58e-8.  dbias: (1, 10, 64): 0, 0 (one term: exact); (7, 200, 768): 4.96e-8,
    5.23e-8; (128, 1000, 768): 1.11e-7, 1.04e-7; (3, 1003, 128): 4.99e-8, 3.50e-8."""
    feat, _, _, dl = contraction_inputs(B, K, Cd)
    refW, refb = pr.head_grads(dl, feat)
    fg, dg = feat.cuda(), dl.cuda()
    runs = []
    for _ in range(2):
        dW, db = guarded(K * Cd, 5.0), guarded(K, 5.0)
        ok(L.uvit_op_probe_head_grad(P(dg), P(fg), P(dW), P(db), B, K, Cd, S()))
        torch.cuda.synchronize()
        assert guard_intact(dW, K * Cd, 5.0) and guard_intact(db, K, 5.0)
        runs.append((dW[:K * Cd].view(K, Cd).clone(), db[:K].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert_within_4x("dW", (B, K, Cd), runs[0][0], refW, dl.t() @ feat)
    assert_within_4x("dbias", (B, K, Cd), runs[0][1], refb, dl.sum(0))


# ------------------------------------------------------------------------------------------------------------------- cross-entropy
def run_ce(L, z, y, s, want_grad=True, counters=None):
    B, K = z.shape
    zg, yg = z.cuda(), y.cuda()
    d = guarded(B * K) if want_grad else None
    rows, loss = guarded(B), guarded(1)
    ok(L.uvit_op_probe_ce(P(zg), P(yg), f32(s), P(d), P(rows), P(loss), P(counters), B, K, S()))
    torch.cuda.synchronize()
    assert guard_intact(rows, B) and guard_intact(loss, 1) and (d is None or guard_intact(d, B * K))
    return (None if d is None else d[:B * K].view(B, K).cpu()), rows[:B].cpu(), loss[:1].cpu()


def ce_logits(B, K):
    """Continuous logits of spread 2; with more than one row, row 1 is +-80 (alternating, plus unit noise): its largest exponent
    overflows fp32 without the max shift and its loss is about 166."""
    z = rnd(B, K, seed=21, scale=2.0)
    if B > 1:
        z[1] = rnd(K, seed=22) + 80.0 * (1.0 - 2.0 * (torch.arange(K) % 2))
    return z


def ce_labels(B, K):
    """Label sets that contain 0 and K - 1 (one row: one set for each)."""
    if B == 1:
        return [torch.tensor([0]), torch.tensor([K - 1])]
    y = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(23))
    y[0], y[1], y[2] = K - 1, 1, 0                 # row 1 is the +-80 row and class 1 holds -80 there: its loss is about 166
    return [y]


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("B,K", [(b, k) for b, k, _ in HEAD_SHAPES])
def test_cross_entropy(L, B, K, smoothing):
    """Row losses, their mean and dlogits against float64, top-1 / top-5 counters against torch.topk.  Bounds from the arithmetic: the
    exponentials are exp2(x log2 e), whose argument rounding costs |x| 2^-24 <= 1.2e-6 relative for the terms within e^-20 of the
    row maximum, the logarithm a few ulp, and the loss takes at most four roundings at its own magnitude (166 on the +-80 row:
    2^-23 x 166 = 2e-5): |loss - ref| <= 1e-5 (1 + |ref|), five times that estimate.  dlogits = (p - target) / B with p in [0, 1]:
    |d - ref| <= 1e-5 / B."""
    z = ce_logits(B, K)
    assert pr.no_ties_among_top(z)                # the six largest of every row differ: top-k is unambiguous
    for y in ce_labels(B, K):
        assert 0 in y.tolist() or K - 1 in y.tolist()
        rows_ref, loss_ref, d_ref = pr.smoothed_ce(z, y, smoothing)
        counters = torch.zeros(2, dtype=torch.int32, device="cuda")
        d, rows, loss = run_ce(L, z, y, smoothing, counters=counters)
        err = (rows.double() - rows_ref).abs() / (1.0 + rows_ref.abs())
        print(f"\nce {(B, K, smoothing)}: row loss error / (1 + |ref|) {float(err.max()):.2e}, dlogits error x B "
              f"{float((d.double() - d_ref).abs().max()) * B:.2e}, +-80 row loss {float(rows_ref[1]) if B > 1 else float('nan'):.2f}")
        assert float(err.max()) <= 1e-5
        assert abs(float(loss) - float(loss_ref)) <= 1e-5 * (1.0 + abs(float(loss_ref)))
        assert float((d.double() - d_ref).abs().max()) <= 1e-5 / B
        c1, c5 = pr.topk_counts(z, y)
        assert counters.tolist() == [c1, c5]
        # no gradient wanted, no counters wanted; the counters accumulate over calls
        d2, rows2, loss2 = run_ce(L, z, y, smoothing, want_grad=False, counters=counters)
        assert d2 is None and torch.equal(rows2, rows) and torch.equal(loss2, loss)
        assert counters.tolist() == [2 * c1, 2 * c5]
        _, rows3, _ = run_ce(L, z, y, smoothing, counters=None)
        assert torch.equal(rows3, rows)


RANKS = [0, 1, 4, 5, 5, 4, 1, 0]      # per row: the label's rank among the row's logits; 4 is the last top-5 hit, 5 the first miss


@pytest.mark.parametrize("B,K", [(8, k) for _, k, _ in HEAD_SHAPES])
def test_cross_entropy_counters_at_chosen_ranks(L, K, B):
    """Labels placed at ranks 0, 1, 4 and 5 of each row's logits (random labels at K >= 200 almost never hit, and a counter that
    never moves would pass there): top-1 counts the two rank-0 rows, top-5 the six rows of rank 0, 1 and 4, and a second call adds
    the same again.  Integer counts: exact."""
    z = ce_logits(B, K)
    assert pr.no_ties_among_top(z)
    y = torch.stack([z[b].argsort(descending=True)[RANKS[b]] for b in range(B)])
    assert pr.topk_counts(z, y) == (2, 6)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    run_ce(L, z, y, 0.0, want_grad=False, counters=counters)
    assert counters.tolist() == [2, 6]
    run_ce(L, z, y, 0.1, counters=counters)
    assert counters.tolist() == [4, 12]


@pytest.mark.parametrize("bad", [-1, 0, 5])
def test_cross_entropy_label_out_of_range(L, bad):
    """A label outside [0, K) (K + bad or -1): the loss of the call is NaN, so are that row's loss and gradient; the other rows are
    what they are without it, the counters skip the row, and nothing is read at the label."""
    B, K = 7, 200
    z = ce_logits(B, K)
    y = ce_labels(B, K)[0]
    good_rows, _, _ = pr.smoothed_ce(z, y, 0.1)
    yb = y.clone()
    yb[3] = -1 if bad < 0 else K + bad * 10 ** 9
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    d, rows, loss = run_ce(L, z, yb, 0.1, counters=counters)
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(rows[3])) and bool(torch.isnan(d[3]).all())
    keep = [i for i in range(B) if i != 3]
    assert bool(torch.isfinite(rows[keep]).all()) and bool(torch.isfinite(d[keep]).all())
    assert float(((rows[keep].double() - good_rows[keep]).abs() / (1 + good_rows[keep].abs())).max()) <= 1e-5
    c1, c5 = pr.topk_counts(z[keep], y[keep])
    assert counters.tolist() == [c1, c5]


# --------------------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


def fixture_probe(case, smoothing=None):
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    fx, cfg, enc, W, bias, _, _ = case
    model = VisionTransformerForCyclicalTraining(img_size=cfg.img_size, patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth,
                                                 num_heads=cfg.num_heads, norm_layer=partial(torch.nn.LayerNorm, eps=cfg.ln_eps),
                                                 init_values=cfg.init_values, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    missing, unexpected = model.load_state_dict(enc, strict=False)       # mask_token, norm.*, lm_head.*: not part of the classifier
    assert not unexpected and all(k.split(".")[0] in ("mask_token", "norm", "lm_head", "rel_pos_bias") for k in missing), missing
    probe = LinearProbe(model.cuda().eval(), W.shape[0], smoothing=float(fx["smoothing"]) if smoothing is None else smoothing)
    probe.load_state_dict({"head.weight": W, "head.bias": bias})
    return probe


def frozen_state(probe):
    e = probe.encoder._engine
    return [t.clone() for t in (probe.encoder._arena, e.params_bf16, e.params_bf16_t, e.ema_bf16, e.ema)]


def test_probe_against_reference_fixture(case):
    """Features, logits, loss, head gradients and the head after three steps against what the reference classifier computed.
    Features and logits: the activation bound of tests/test_gpu_model.py (the encoder's GEMM operands are bf16); loss: that file's
    5e-3 relative; gradients: its gradient bound, 5e-2 relative plus 2e-2 of the largest gradient; the head after three AdamW steps of
    lr: its weight bound, 3 lr + 1e-4 -- and, where the gradient is at least a tenth of the largest (the gradient bound cannot
    flip its sign, the same batch thrice moves such a weight by about 3 lr), within 0.2 x 3 lr.  The encoder's parameters and bf16
    shadows hold the same bits afterwards."""
    fx, cfg, enc, W, bias, images, labels = case
    lr, wd = float(fx["lr"]), float(fx["weight_decay"])
    probe = fixture_probe(case)
    xg, yg = images.cuda(), labels.cuda()
    feat = probe.features(xg)
    torch.testing.assert_close(feat.cpu(), torch.from_numpy(fx["features"]), rtol=ACT_RT, atol=ACT_AT)
    logits = probe.logits(xg)
    torch.testing.assert_close(logits.cpu(), torch.from_numpy(fx["logits"]), rtol=ACT_RT, atol=ACT_AT)
    print(f"\nfeatures max error {float((feat.cpu() - torch.from_numpy(fx['features'])).abs().max()):.2e}, "
          f"logits max error {float((logits.cpu() - torch.from_numpy(fx['logits'])).abs().max()):.2e}")
    before = frozen_state(probe)
    ref_losses, ref_norms, _, _ = pr.train_steps(torch.from_numpy(fx["features"]), W, bias, labels, float(fx["smoothing"]), lr, wd, 3)
    for s in range(3):
        loss, gnorm = probe.train_step(xg, yg, lr, wd)
        assert float(loss) == pytest.approx(float(fx["step_loss"][s]), rel=5e-3)
        assert float(gnorm) == pytest.approx(ref_norms[s], rel=3e-2)
        if s == 0:
            assert float(loss) == pytest.approx(float(fx["loss"]), rel=5e-3)
            gmax = max(float(np.abs(fx["grad/weight"]).max()), float(np.abs(fx["grad/bias"]).max()))
            for p, key in ((probe.head.weight, "grad/weight"), (probe.head.bias, "grad/bias")):
                torch.testing.assert_close(p.grad.cpu(), torch.from_numpy(fx[key]), rtol=5e-2, atol=2e-2 * gmax)
    sd = probe.state_dict()
    for key, ref, g in (("head.weight", fx["post/weight"], fx["grad/weight"]), ("head.bias", fx["post/bias"], fx["grad/bias"])):
        got, ref = sd[key].cpu(), torch.from_numpy(ref)
        torch.testing.assert_close(got, ref, rtol=0, atol=3 * lr + 1e-4)
        big = torch.from_numpy(np.abs(g) >= 0.1 * gmax)
        assert int(big.sum()) > 0 and float((got - ref)[big].abs().max()) <= 0.2 * 3 * lr, key
    for a, b in zip(before, frozen_state(probe)):
        assert torch.equal(a, b)
    assert probe.encoder._grad_arena is None or float(probe.encoder._grad_arena.abs().max()) == 0.0     # no gradient into the encoder


def test_train_step_skips_a_poisoned_batch(case):
    """An out-of-range label: the loss is NaN and the head, its moments included, keeps its bits."""
    _, _, _, _, _, images, labels = case
    probe = fixture_probe(case)
    bad = labels.clone()
    bad[2] = 10
    before = [t.clone() for t in (probe._arena, probe.exp_avg, probe.exp_avg_sq)]
    loss, _ = probe.train_step(images.cuda(), bad.cuda(), 1e-3, 0.05)
    assert bool(torch.isnan(loss))
    for a, b in zip(before, (probe._arena, probe.exp_avg, probe.exp_avg_sq)):
        assert torch.equal(a, b)


EVAL_RANKS = [0, 2, 7, 0, 5, 4, 3, 9, 0, 4, 6, 0]       # rank of each sample's label among its float64 logits: 4 top-1, 8 top-5 (rank 4: the last hit)


def test_evaluate_three_batches(case):
    """evaluate() over 3 batches of 4 images: plain cross-entropy and top-1 / top-5 counts of probe_ref.  The labels are placed at
    fixed ranks of the float64 logits; the test first checks that every label's logit is at least 0.02 away from every other
    logit of its row -- ten times the error the bf16 encoder leaves on these logits (test_probe_against_reference_fixture prints
    it) -- so the counts cannot depend on that error.  Loss: 5e-3 relative (tests/test_gpu_model.py)."""
    fx, cfg, enc, W, bias, _, _ = case
    probe = fixture_probe(case)
    batches, z_all, y_all = [], [], []
    for i in range(3):
        x = closed_form_images(f"probe-eval/{i}", 4, cfg.img_size)
        z = pr.head_logits(pr.features(enc, cfg, x), W, bias)
        y = torch.stack([z[j].argsort(descending=True)[EVAL_RANKS[4 * i + j]] for j in range(4)])
        batches.append(((x.cuda(), None), y))                     # the prefetcher's item: ((images, mask), labels on the host)
        z_all.append(z)
        y_all.append(y)
    z, y = torch.cat(z_all), torch.cat(y_all)
    gap = (z - z.gather(1, y.view(-1, 1))).abs()
    gap.scatter_(1, y.view(-1, 1), float("inf"))
    assert float(gap.min()) > 0.02, float(gap.min())
    _, loss_ref, _ = pr.smoothed_ce(z, y, 0.0)
    c1, c5 = pr.topk_counts(z, y)
    assert (c1, c5) == (4, 8)
    out = probe.evaluate(batches)
    assert out["n"] == 12 and (out["correct1"], out["correct5"]) == (c1, c5)
    assert out["acc1"] == pytest.approx(100.0 * c1 / 12) and out["acc5"] == pytest.approx(100.0 * c5 / 12)
    assert out["loss"] == pytest.approx(float(loss_ref), rel=5e-3)
