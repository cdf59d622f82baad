"""GPU: the two-stream probe (csrc/dprobe.hip, uncertainty-vit_amd/dist_probe.py) against uvit_op_probe_pool_norm (bit for bit),
against the float64 restatement of tests/dprobe_ref.py with its derived bounds, and against what the reference model computed
(tests/golden/dist_d48.npz)."""
import ctypes as C
import math
import os
from functools import partial

import numpy as np
import pytest
import torch

import dprobe_ref as dp
import probe_ref as pr
from oracle import vit_oracle as vo
from oracle import vit_oracle_dist as vd
from oracle.closed_form import closed_form_images, closed_form_state

pytestmark = pytest.mark.gpu

GUARD = 64
EPS = C.c_float(1e-6)


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    lib = native.lib()
    for what, got, want in dp.bad_calls(lib):              # every error code, before anything is launched
        assert got == want, (what, got, want)
    return lib


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    assert rc == 0, f"libuvit returned {rc}"


def guarded(n, fill=7.5, dtype=torch.float32):
    """n elements on the device followed by GUARD sentinels that no kernel may touch."""
    return torch.full((n + GUARD,), fill, device="cuda", dtype=dtype)


def guard_intact(t, n, fill=7.5):
    return bool((t[n:] == fill).all())


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# -------------------------------------------------------------------------------------------------------------- op 1: pool + norm
@pytest.mark.parametrize("Cd", [4, 128, 768, 2048])
@pytest.mark.parametrize("N", [2, 10, 197])
@pytest.mark.parametrize("B", [1, 3])
def test_pair_equals_two_single_calls(L, B, N, Cd):
    """Each output of the pair op equals uvit_op_probe_pool_norm on that stream alone, bit for bit: with the two streams adjacent in
    one buffer (the engine's layout) and with them far apart, the covariance stream at the lower address.  N = 2 is one patch token
    (seven empty slices), N = 10 leaves empty trailing slices, 197 = 7 x 25 + 21 a short last one; C = 4 is one float4, 2048 the
    widest row.  Sentinels behind both outputs and the scratch stay."""
    xm = rnd(B, N, Cd, seed=1) + rnd(B, 1, Cd, seed=2)
    xc = rnd(B, N, Cd, seed=3) * 0.5 - 1.0 + rnd(B, 1, Cd, seed=4)
    n, ws1 = B * N * Cd, L.uvit_op_probe_pool_ws_bytes(B, N, Cd)
    ws = L.uvit_op_dprobe_pool_ws_bytes(B, N, Cd)
    assert ws == 2 * ws1 == 2 * B * 8 * Cd * 4
    single = []
    for x in (xm, xc):
        feat, scratch, xg = guarded(B * Cd), guarded(ws1 // 4), x.cuda()
        ok(L.uvit_op_probe_pool_norm(P(xg), P(feat), P(scratch), B, N, Cd, EPS, S()))
        torch.cuda.synchronize()
        assert guard_intact(feat, B * Cd) and guard_intact(scratch, ws1 // 4)
        single.append(feat[:B * Cd].clone())
    gap = 1 << 20
    adjacent = torch.cat([xm.flatten(), xc.flatten()]).cuda()
    apart = torch.zeros(n + gap + n, device="cuda")
    apart[:n], apart[n + gap:] = xc.flatten().cuda(), xm.flatten().cuda()
    for buf, off_m, off_c in ((adjacent, 0, n), (apart, n + gap, 0)):
        fm, fc, scratch = guarded(B * Cd), guarded(B * Cd), guarded(ws // 4)
        ok(L.uvit_op_dprobe_pool_norm(C.c_void_p(buf.data_ptr() + 4 * off_m), C.c_void_p(buf.data_ptr() + 4 * off_c), P(fm), P(fc), P(scratch),
                                      B, N, Cd, EPS, S()))
        torch.cuda.synchronize()
        assert guard_intact(fm, B * Cd) and guard_intact(fc, B * Cd) and guard_intact(scratch, ws // 4)
        assert torch.equal(fm[:B * Cd], single[0]) and torch.equal(fc[:B * Cd], single[1]), (off_m, off_c)
    ref = dp.pool_norm(xm.numpy())
    assert (np.abs(single[0].view(B, Cd).cpu().numpy() - ref) <= dp.pool_norm_bound(xm.numpy())).all()


# ------------------------------------------------------------------------------------------------------------------ op 2: variance
def cov_features(B, Cd, seed=5):
    """Covariance features of spread 2 around -0.5 with a 0, a -100 and a +50 in every row."""
    c = rnd(B, Cd, seed=seed) * 2.0 - 0.5
    c[:, 0], c[:, 1], c[:, 2] = 0.0, -100.0, 50.0
    return c


def run_variance(L, c, W, scale, want_trace=True):
    B, Cd = c.shape
    K = W.shape[0]
    var, trace = guarded(B * K, -1.0, torch.float64), guarded(B, -1.0) if want_trace else None
    cg, Wg = c.cuda(), W.cuda()
    ok(L.uvit_op_dprobe_variance(P(cg), P(Wg), C.c_double(scale), P(var), P(trace), B, K, Cd, S()))
    torch.cuda.synchronize()
    assert guard_intact(var, B * K, -1.0) and (trace is None or guard_intact(trace, B, -1.0))
    return var[:B * K].view(B, K).cpu().numpy(), None if trace is None else trace[:B].cpu().numpy()


@pytest.mark.parametrize("Cd", [4, 128, 768])
@pytest.mark.parametrize("K", [1, 5, 1000])
@pytest.mark.parametrize("B", [1, 3, 130])
def test_variance_against_float64(L, B, K, Cd):
    """var and trace against the restatement: |got - ref| <= 2 (C + 4) 2^-53 ref (tests/dprobe_ref.py; trace + 2^-24 for its one
    fp32 rounding).  B = 130 crosses the edge of the ninth 16-row tile, K = 1000 = 31 x 32 + 8 that of the column tiles, K = 1 and
    B = 1 leave most of a tile empty.  Two runs give the same bits; without a trace pointer var is the same."""
    c, W = cov_features(B, Cd), rnd(K, Cd, seed=6) * 0.05
    scale = 0.75
    ref, tref = dp.variance(c.numpy(), W.numpy(), scale), dp.trace(c.numpy(), scale)
    var, trace = run_variance(L, c, W, scale)
    var2, _ = run_variance(L, c, W, scale, want_trace=False)
    assert np.array_equal(var, var2)
    err, terr = np.abs(var - ref) / dp.variance_bound(ref, Cd), np.abs(trace - tref) / dp.trace_bound(tref, Cd)
    print(f"\nvariance {(B, K, Cd)}: worst error / bound {err.max():.3f}, trace {terr.max():.3f}")
    assert (ref > 0).all() and err.max() <= 1.0 and terr.max() <= 1.0


def test_variance_exact_cases(L):
    """c = 0: v = s exp(0) = s, and for s a power of two every product s w^2 is exact, so the fma chain is the sequential sum:
    var_k = s sum_c W_kc^2 bit for bit, trace = s.  A one-hot row of W: var_k = v_c, bit for bit where c >= 0 (c + 1 and the product
    with s are single IEEE roundings on both sides) and within 8 x 2^-53 where c < 0 (with u = 2^-53, half an ulp: an exp within
    1 ulp = 2 u and the product's rounding u, on either side: 6 u)."""
    Cd, K, B = 128, 37, 5
    W = rnd(K, Cd, seed=7)
    for s in (1.0, 0.5):
        var, trace = run_variance(L, torch.zeros(B, Cd), W, s)
        assert np.array_equal(var, dp.variance_chain(np.zeros((B, Cd), np.float32), W.numpy(), s))
        assert np.array_equal(trace, np.full(B, s, np.float32))
    c = cov_features(B, Cd)
    eye = torch.eye(Cd)
    eye[3, 3] = -1.0
    v = dp.feature_variance(c.numpy(), 0.75)
    var, _ = run_variance(L, c, eye, 0.75)
    pos = c.numpy() >= 0
    assert pos.any() and (~pos).any()
    assert np.array_equal(var[pos], v[pos])
    assert (np.abs(var - v)[~pos] <= 8 * dp.U64 * v[~pos]).all()


def test_variance_nan_stays_in_its_row(L):
    B, K, Cd = 35, 70, 128
    c, W = cov_features(B, Cd), rnd(K, Cd, seed=8)
    W[:, 9] = 0.0                                        # the NaN meets a zero weight in every class: NaN all the same
    good, tgood = run_variance(L, c, W, 1.0)
    bad = c.clone()
    bad[17, 9] = float("nan")
    var, trace = run_variance(L, bad, W, 1.0)
    keep = np.arange(B) != 17
    assert np.isnan(var[17]).all() and np.isnan(trace[17])
    assert np.array_equal(var[keep], good[keep]) and np.array_equal(trace[keep], tgood[keep])


# --------------------------------------------------------------------------------------------------------------------- model level
K_ = 10


@pytest.fixture(scope="module")
def case(golden_dir):
    """The d48 two-stream configuration with closed-form weights, its images, a DistProbe with a fixed head, and once for all
    tests: the engine's own last-block streams and the probe's features, logits and variances of the batch."""
    from uncertainty_vit_amd.dist_probe import DistProbe
    from uncertainty_vit_amd.modeling_cyclical import DistVisionTransformerForCyclicalTraining
    fx = np.load(os.path.join(golden_dir, "dist_d48.npz"))
    img, dim, depth, heads, B, _, _ = [int(v) for v in fx["cfg"]]
    cfg = vo.VitConfig(img_size=img, embed_dim=dim, depth=depth, num_heads=heads, init_values=float(fx["init_values"]))
    model = DistVisionTransformerForCyclicalTraining(img_size=img, patch_size=16, embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=4,
                                                     qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                                                     init_values=cfg.init_values, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    model.load_state_dict(closed_form_state(vd.param_shapes(cfg), gamma=cfg.init_values), strict=False)
    model = model.cuda().eval()
    x = closed_form_images("d48/0", B, img).cuda()
    em, ec = model(x, None, True, layer_results="end")
    probe = DistProbe(model, K_, smoothing=0.1)
    W, bias = rnd(K_, dim, seed=9) * 0.3, rnd(K_, seed=10) * 0.1
    probe.load_state_dict({"head.weight": W, "head.bias": bias})
    with_cls = lambda t: np.concatenate([np.zeros((B, 1, dim), np.float32), np.asarray(t, np.float32)], 1)      # noqa: E731
    own = dict(mean=with_cls(em[-1].cpu().numpy()), cov=with_cls(ec[-1].cpu().numpy()))
    gold = dict(mean=with_cls(fx[f"fwd/mean_end{depth - 1}/full"]), cov=with_cls(fx[f"fwd/cov_end{depth - 1}/full"]))
    got = dict(feat=probe.features(x).cpu().numpy(), cfeat=probe.cov_features(x).cpu().numpy(), v=probe.feature_variance(x).cpu().numpy(),
               var=probe.predictive_variance(x).cpu().numpy(), logits=probe.logits(x).cpu().numpy())
    return dict(probe=probe, x=x, W=W, bias=bias, own=own, gold=gold, got=got, B=B, dim=dim)


def test_features_against_the_engine_s_own_streams(case):
    """features / cov_features equal the restatement applied to the engine's own last-block streams (fp32 tensors: no bf16 tolerance
    enters) within the row-wise bound of a mean and a LayerNorm (tests/dprobe_ref.py, from tests/rowwise_ref.py)."""
    for key, name in (("feat", "mean"), ("cfeat", "cov")):
        ref, bound = dp.pool_norm(case["own"][name]), dp.pool_norm_bound(case["own"][name])
        err = np.abs(case["got"][key] - ref) / bound
        print(f"\n{key}: worst error / bound {err.max():.3f} (bound up to {bound.max():.2e})")
        assert err.max() <= 1.0


def test_features_against_the_reference_fixture(case):
    """Against the reference model's numbers: the restatement of the golden's last-block streams.  The entry bound 2e-2 + 2e-2 |x|
    of tests/test_gpu_dist.py::test_two_stream_forward_vs_golden goes through the mean and the normalisation (pool_norm_bound's
    e_in): the pooled vectors have a per-sample standard deviation of 0.26 - 0.30 here, so the bound grows by about 1 / sigma."""
    for key, name in (("feat", "mean"), ("cfeat", "cov")):
        g = case["gold"][name]
        sigma = g[:, 1:].mean(1).std(-1)
        bound = dp.pool_norm_bound(g, e_in=2e-2 + 2e-2 * np.abs(g))
        err = np.abs(case["got"][key] - dp.pool_norm(g)) / bound
        print(f"\n{key} vs golden: sigma {sigma.round(3)}, worst error / bound {err.max():.3f} (max |diff| {np.abs(case['got'][key] - dp.pool_norm(g)).max():.2e})")
        assert (sigma > 0.2).all() and (sigma < 0.4).all() and err.max() <= 1.0


def test_variances_and_link(L, case):
    """feature_variance and predictive_variance against the restatement on the probe's own covariance feature (the bound of op 2);
    logits at mean_field = 0 equal uvit_op_probe_logits on the mean feature bit for bit; at pi / 8 they equal the float64 link of the
    restatement on those logits and the device's own variance, rounded once."""
    probe, x, B, Cd = case["probe"], case["x"], case["B"], case["dim"]
    cf, W = case["got"]["cfeat"], case["W"].numpy()
    v, var = dp.feature_variance(cf), dp.variance(cf, W)
    assert (np.abs(case["got"]["v"] - v) <= 8 * dp.U64 * v).all()          # test_variance_exact_cases: 6 u
    assert (np.abs(case["got"]["var"] - var) <= dp.variance_bound(var, Cd)).all()
    plain = torch.zeros(B, K_, device="cuda")
    fg, Wg, bg = torch.from_numpy(case["got"]["feat"]).cuda(), case["W"].cuda(), case["bias"].cuda()
    ok(L.uvit_op_probe_logits(P(fg), P(Wg), P(bg), P(plain), B, K_, Cd, S()))
    assert torch.equal(torch.from_numpy(case["got"]["logits"]).cuda(), plain)
    probe.mean_field = math.pi / 8
    try:
        scaled = probe.logits(x).cpu().numpy()
    finally:
        probe.mean_field = 0.0
    want = dp.link(plain.cpu().numpy(), case["got"]["var"], math.pi / 8).astype(np.float32)
    assert np.array_equal(scaled, want) and (np.abs(scaled) < np.abs(plain.cpu().numpy())).all()


def test_train_steps_are_the_linear_probe_s(case):
    """Three train_steps on the fixed batch lower the loss and match the float64 head update on the probe's own mean feature within
    the tolerances tests/test_gpu_probe.py holds the linear probe to: loss 5e-3 relative, gradient norm 3e-2 relative, the head
    after three AdamW steps of lr within 3 lr + 1e-4.  mean_field is pi / 8 meanwhile: the loss must not see it."""
    from uncertainty_vit_amd.dist_probe import DistProbe
    lr, wd = 1e-3, 0.05
    probe = DistProbe(case["probe"].encoder, K_, smoothing=0.1, mean_field=math.pi / 8)
    probe.load_state_dict({"head.weight": case["W"], "head.bias": case["bias"]})
    labels = torch.tensor([1, 7, 4])[:case["B"]]
    ref_losses, ref_norms, _, ref_head = pr.train_steps(torch.from_numpy(case["got"]["feat"]), case["W"], case["bias"], labels, 0.1, lr, wd, 3)
    losses = []
    for s in range(3):
        loss, gnorm = probe.train_step(case["x"], labels.cuda(), lr, wd)
        losses.append(float(loss))
        assert float(loss) == pytest.approx(ref_losses[s], rel=5e-3) and float(gnorm) == pytest.approx(ref_norms[s], rel=3e-2)
    assert losses[2] < losses[1] < losses[0]
    sd = probe.state_dict()
    for key, ref in (("head.weight", ref_head[0]), ("head.bias", ref_head[1])):
        assert float((sd[key].cpu().double() - ref).abs().max()) <= 3 * lr + 1e-4
        assert float((sd[key].cpu().double() - ref).abs().max()) < 0.2 * float((ref - (case["W"] if key == "head.weight" else case["bias"]).double()).abs().max())


def test_evaluate_returns_the_two_columns_and_their_means(case):
    """evaluate(detection=True) over the batch twice (two batches): the columns are there, each mean equals the mean of the
    per-batch values (predictive_variance at the predicted class; the trace of feature_variance) and accuracy and loss are the linear
    head's at mean_field = 0."""
    probe, x, B = case["probe"], case["x"], case["B"]
    z, var, v = case["got"]["logits"], case["got"]["var"], case["got"]["v"]
    labels = torch.from_numpy(z.argmax(-1)).clone()
    labels[0] = (labels[0] + 1) % K_                    # one wrong prediction per batch: the detection has both kinds of rows
    stats = probe.evaluate([((x, None), labels), ((x, None), labels)], detection=True)
    det = stats["detection"]
    assert det["columns"] == ["msp", "entropy", "energy", "dist_var", "dist_trace"] and det["n"] == 2 * B and det["n_wrong"] == 2
    assert all(0.0 <= det["misclassification"][c]["AUROC"] <= 1.0 for c in ("dist_var", "dist_trace"))
    col = dp.predicted_variance(z, var).astype(np.float32).astype(np.float64)
    tr = v.mean(-1).astype(np.float32).astype(np.float64)
    assert stats["dist_var_mean"] == pytest.approx(col.mean(), rel=1e-12)
    assert stats["dist_trace_mean"] == pytest.approx(tr.mean(), rel=1e-6)
    assert stats["n"] == 2 * B and stats["correct1"] == 2 * (B - 1)
    plain = probe.evaluate([((x, None), labels)], variance=False)
    assert "dist_var_mean" not in plain and "detection" not in plain and plain["acc1"] == stats["acc1"]
    scaled = probe.evaluate([((x, None), labels)], mean_field=math.pi / 8)
    assert scaled["loss"] != plain["loss"] and scaled["dist_var_mean"] == stats["dist_var_mean"] and probe.mean_field == 0.0
