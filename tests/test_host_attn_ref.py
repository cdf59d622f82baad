"""CPU (no GPU): pins tests/attn_ref.py, the float64 restatements of the attention core and the comparator tests/test_gpu_attn_bounds.py
judges the kernels by.

  * with o_fwd and lse set to the exact float64 values the restatement equals float64 autograd of the reference formula
    (modeling_finetune.py:152-185) to 1e-12 relative: head dims 64 and 80, with and without bias and dropout;
  * an emulation -- the same arithmetic in another summation order, fp32 intermediates, bf16 roundings at the cited points -- PASSES
    every bound with worst ratio < 1: the bounds are not too tight;
  * mutations FAIL: one P element zeroed on a row's top key, one keep bit flipped, K and V rows swapped in one key pair, delta taken
    from the exact output instead of o_fwd in one query tile;
  * the ladder: one block of the float64 reference scaled by 1.005 .. 1.10; the comparator rejects at <= 1.02 on flat data and <= 1.01 on
    peaked data, and never later than today's criteria (restated in attn_ref.todays_criteria_reject);
  * the read-out decode recovers attn_keep_mask exactly from the float64 reference, forward and backward;
  * both permutation generators give a one-hot P; so does the bias-selected one in the two-stream core's reference arithmetic
    (oracle.vit_oracle_dist), whose read-out inputs give a uniform P;
  * the two-stream core: without the bf16 operand images the restatement equals float64 autograd of oracle.vit_oracle_dist's formula
    (the covariance gradients times min(y, 1), ELU' at the stored value y) to 1e-12; with them, an fp32 / bf16 emulation passes every bound, and the same mutations fail.

The ladder as measured here (B = 2, H = 2, N = 197, head_dim 64, the inputs of test_attention_fwd / bwd; smallest rejected factor,
today's criteria | this comparator; `-`: not rejected up to 1.10):
                                        flat              peaked
  out, query tile 4 (rows 64..79)      1.050 | 1.020     1.030 | 1.010
  out, last tile (rows 192..196)       1.050 | 1.020     1.030 | 1.010
  dQ, query tile 4                     1.050 | 1.020     1.100 | 1.010
  dV, last key tile                    1.100 | 1.020     1.100 | 1.010
  dV, d-tile 3                         1.020 | 1.020     1.020 | 1.010
"""
import pytest
import torch

import attn_ref as A
from attn_ref import BF16, F32, F64

FACTORS = (1.005, 1.01, 1.02, 1.03, 1.05, 1.10)


def keep_of(B, H, N, p, seed=1234, layer=3):
    from oracle.vit_oracle import attn_keep_mask
    return attn_keep_mask(seed, layer, B, H, N, p) if p > 0 else None


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-300)).item()


def autograd64(qkv, bias, scale, keep, d_o, B, H, N, hd):
    x = qkv.double().requires_grad_(True)
    # the bias the kernel is handed is fp32(bias log2 e): differentiate at that point
    bq = None if bias is None else ((bias.float() * A.LOG2E).double() / A.LOG2E).requires_grad_(True)
    q, k, v = A.split(x, B, H, N, hd)
    s = (q * A.scale32(scale)) @ k.transpose(-2, -1)
    if bq is not None:
        s = s + bq
    a = s.softmax(-1)
    lse = torch.logsumexp(s, -1)
    if keep is not None:
        a = a * keep.double()
    out = a @ v
    out.backward(A.heads(d_o.double(), B, H, N, hd))
    return out.detach(), lse.detach() * A.LOG2E, A.split(x.grad, B, H, N, hd), None if bq is None else bq.grad


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_restatement_is_autograd(hd, with_bias, p):
    B, H, N, scale = 2, 3, 37, hd ** -0.5
    qkv, bias, d_o = A.regime_inputs("flat", B, H, N, hd)
    bias = bias if with_bias else None
    keep = keep_of(B, H, N, p)
    out, lse, (gq, gk, gv), gb = autograd64(qkv, bias, scale, keep, d_o, B, H, N, hd)
    f = A.base_fwd(qkv, bias, scale, keep, B, H, N, hd)
    assert rel(f["out"].ref, out) < 1e-12 and rel(f["lse"].ref, lse) < 1e-12
    b = A.base_bwd(qkv, bias, scale, keep, A.unheads(out), lse, d_o, B, H, N, hd)
    for name, g in (("dq", gq), ("dk", gk), ("dv", gv)):
        assert rel(b[name].ref, g) < 1e-12, name
    assert rel(b["delta"].ref, (A.heads(d_o.double(), B, H, N, hd) * out).sum(-1)) < 1e-12
    if with_bias:
        assert rel(b["dbias"].ref, gb) < 1e-12
        s0 = A._rnd(H, N, N, seed=9)
        b2 = A.base_bwd(qkv, bias, scale, keep, A.unheads(out), lse, d_o, B, H, N, hd, slab0=s0)
        assert rel(b2["dbias"].ref, s0.double() + gb) < 1e-12


def run_emulation(regime, hd, N, with_bias, p, B=2, H=2, slab0=None, **mut):
    """The comparator on the emulation's buffers; mut: p_hook_fwd, p_hook_bwd, keep_emul, qkv_emul, delta.  -> dict name -> worst ratio"""
    scale = hd ** -0.5
    qkv, bias, d_o = A.regime_inputs(regime, B, H, N, hd)
    bias = bias if with_bias else None
    keep = keep_of(B, H, N, p)
    ke, qe = mut.get("keep_emul", keep), mut.get("qkv_emul", qkv)
    o16, lse32 = A.emulate_fwd(qe, bias, scale, ke, B, H, N, hd, p_hook=mut.get("p_hook_fwd"))
    f = A.base_fwd(qkv, bias, scale, keep, B, H, N, hd)
    worst = {"out": A.compare("emul", "out", A.heads(o16, B, H, N, hd), f["out"], check=False)[0],
             "lse": A.compare("emul", "lse", lse32, f["lse"], check=False)[0]}
    assert f["lse"].bound.max().item() <= 3e-3                       # no larger than what the existing tests allow
    # the backward is a function of the GIVEN o_fwd and lse: the emulated forward's own buffers
    o_g, lse_g = A.emulate_fwd(qkv, bias, scale, keep, B, H, N, hd)
    dl, dqkv, db = A.emulate_bwd(qe, bias, scale, ke, o_g, lse_g, d_o, B, H, N, hd, slab0=slab0, p_hook=mut.get("p_hook_bwd"),
                                 delta=mut.get("delta", lambda *_: None)(f, d_o, o_g))
    r = A.base_bwd(qkv, bias, scale, keep, o_g, lse_g, d_o, B, H, N, hd, slab0=slab0)
    gq, gk, gv = A.split(dqkv, B, H, N, hd)
    for name, got in (("delta", dl), ("dq", gq), ("dk", gk), ("dv", gv)) + ((("dbias", db),) if with_bias else ()):
        worst[name] = A.compare("emul", name, got, r[name], check=False)[0]
    return worst


@pytest.mark.parametrize("regime,hd", [("flat", 64), ("flat", 80), ("peaked", 64), ("peaked", 80), ("peaked_tail", 80)])
@pytest.mark.parametrize("N", [33, 197])
@pytest.mark.parametrize("with_bias,p", [(True, 0.1), (False, 0.0)])
def test_emulation_passes_every_bound(regime, hd, N, with_bias, p):
    slab0 = A._rnd(2, N, N, seed=5) if with_bias and N == 33 else None
    worst = run_emulation(regime, hd, N, with_bias, p, slab0=slab0)
    print(f"\nemulation {regime} hd {hd} N {N} bias {with_bias} p {p}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0, worst


def test_peaked_regime_is_peaked():
    qkv, bias, _ = A.regime_inputs("peaked", 2, 2, 197, 64)
    Pm = A.base_fwd(qkv, bias, 0.125, None, 2, 2, 197, 64)["P"]
    med = Pm.amax(-1).median().item()
    print(f"\npeaked: median row maximum of P {med:.2f}")
    assert med > 0.7


# ---- mutations -------------------------------------------------------------------------------------------------------------------
def zero_top(p):
    p = p.clone()
    p[1, 1, 70, p[1, 1, 70].argmax()] = 0
    return p


def flip_keep(regime, B, H, N, hd, p):
    """One keep bit flipped, on its row's top key (on a key that carries no probability a flipped bit cannot show in any output: the
    read-out cases compare those)"""
    qkv, bias, _ = A.regime_inputs(regime, B, H, N, hd)
    top = int(A.base_fwd(qkv, bias, hd ** -0.5, None, B, H, N, hd)["P"][1, 0, 40].argmax())
    k = keep_of(B, H, N, p).clone()
    k[1, 0, 40, top] = k.max() - k[1, 0, 40, top]
    return k


def swap_kv_pair(qkv, B, H, N, hd, k0=100):
    t = qkv.clone().view(B, N, 3, H, hd)
    t[:, [k0, k0 + 1], 1:] = t[:, [k0 + 1, k0], 1:]
    return t.view(B * N, -1)


def exact_delta_in_tile(f, d_o, o_g, tile=4):
    """delta from the EXACT output in one query tile, from o_fwd elsewhere"""
    B, H, N, hd = f["out"].ref.shape
    do = A.heads(d_o, B, H, N, hd).double()
    dl = (do * A.heads(o_g, B, H, N, hd).double()).sum(-1)
    dl[:, :, 16 * tile:16 * tile + 16] = (do * f["out"].ref).sum(-1)[:, :, 16 * tile:16 * tile + 16]
    return dl


@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_mutations_fail(regime):
    B, H, N, hd, p = 2, 2, 197, 64, 0.1
    base = run_emulation(regime, hd, N, True, p)
    assert max(base.values()) < 1.0
    qkv = A.regime_inputs(regime, B, H, N, hd)[0]
    for what, mut, must in (("P zeroed on a row's top key (forward)", dict(p_hook_fwd=zero_top), ("out",)),
                            ("P zeroed on a row's top key (backward)", dict(p_hook_bwd=zero_top), ("dq", "dv")),
                            ("one keep bit flipped", dict(keep_emul=flip_keep(regime, B, H, N, hd, p)), ("out", "dv")),
                            ("K and V rows swapped in one key pair", dict(qkv_emul=swap_kv_pair(qkv, B, H, N, hd)), ("out", "dk", "dv")),
                            ("delta from the exact output in one query tile", dict(delta=exact_delta_in_tile), ("delta",))):
        worst = run_emulation(regime, hd, N, True, p, **mut)
        print(f"\n{regime}: {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        for name in must:
            assert worst[name] > 1.0, (what, name, worst[name])


# ---- the ladder ------------------------------------------------------------------------------------------------------------------
BLOCKS = (("out, query tile 4 (rows 64..79)", "out", lambda t: t[:, :, 64:80]),
          ("out, last tile (rows 192..196)", "out", lambda t: t[:, :, 192:]),
          ("dQ, query tile 4", "dq", lambda t: t[:, :, 64:80]),
          ("dV, last key tile", "dv", lambda t: t[:, :, 192:]),
          ("dV, d-tile 3", "dv", lambda t: t[..., 48:64]))


def ladder(regime):
    B, H, N, hd = 2, 2, 197, 64
    qkv, bias, d_o = A.regime_inputs(regime, B, H, N, hd)
    f = A.base_fwd(qkv, bias, 0.125, None, B, H, N, hd)
    b = A.base_bwd(qkv, bias, 0.125, None, A.unheads(f["out"].ref).to(BF16), f["lse"].ref.to(F32), d_o, B, H, N, hd)
    vals = {"out": f["out"], "dq": b["dq"], "dk": b["dk"], "dv": b["dv"]}
    refs = {k: v.ref for k, v in vals.items()}
    rows = []
    for what, name, block in BLOCKS:
        first = {"today": None, "bound": None}
        for fac in FACTORS:
            got = refs[name].clone()
            block(got).mul_(fac)
            if first["today"] is None and A.todays_criteria_reject(name, got, refs):
                first["today"] = fac
            if first["bound"] is None and A.compare("ladder", name, got, vals[name], check=False)[0] > 1.0:
                first["bound"] = fac
        rows.append((what, first["today"], first["bound"]))
    return rows


@pytest.mark.parametrize("regime,limit", [("flat", 1.02), ("peaked", 1.01)])
def test_ladder(regime, limit):
    rows = ladder(regime)
    fmt = lambda v: "-" if v is None else f"{v:.3f}"      # noqa: E731
    print(f"\n{regime}:")
    for what, today, bound in rows:
        print(f"  {what:34s} {fmt(today):>6s} | {fmt(bound):>6s}")
    for what, today, bound in rows:
        assert bound is not None and bound <= limit, (regime, what, bound)
        assert today is None or bound <= today, (regime, what, today, bound)


# ---- exact cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("N", [33, 197, 208])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_readout_decode_recovers_the_keep_mask(hd, N, p):
    B, H, seed, layer = 3, 3, 77, 4
    keep = keep_of(B, H, N, p, seed, layer)
    want = A.keep_bits(seed, layer, B, H, N, p)
    outs, dvs = [], []
    for c in range(A.readout_chunks(N, hd)):
        qkv = A.readout_qkv(B, H, N, hd, c)
        f = A.base_fwd(qkv, None, hd ** -0.5, keep, B, H, N, hd)
        assert torch.equal(f["P"], torch.full_like(f["P"], 1.0 / N))
        outs.append(f["out"].ref)
        d_o = A.unheads(A.readout_onehot(B, H, N, hd, c)).to(BF16)
        b = A.base_bwd(qkv, None, hd ** -0.5, keep, A.unheads(f["out"].ref).to(BF16), f["lse"].ref.to(F32), d_o, B, H, N, hd)
        dvs.append(b["dv"].ref)
        assert b["dq"].ref.abs().max() == 0 and b["dk"].ref.abs().max() == 0
    got, off = A.readout_decode(outs, N, hd, p)
    assert torch.equal(got, want) and off <= 1.0
    got_b, off_b = A.readout_decode(dvs, N, hd, p)              # dV[k, d] = Pd[q = hd chunk + d, k]: the transposed mask
    assert torch.equal(got_b.transpose(-1, -2), want) and off_b <= 1.0
    flipped = [o.clone() for o in outs]
    flipped[0][2, 1, 5, 7] = 0 if want[2, 1, 5, 7] else outs[0].max()
    assert not torch.equal(A.readout_decode(flipped, N, hd, p)[0], want)


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("N", [5, 33, 197, 208])
def test_bias_selected_permutation_is_one_hot(hd, N):
    B, H = 2, 4
    c = A.bias_selected(B, N, hd)
    f = A.base_fwd(c["qkv"], c["bias"], hd ** -0.5, None, B, H, N, hd)
    mass, peaks = A.off_peak_mass(f["P"], c["pi"])
    assert mass == 0.0 and peaks
    assert torch.equal(f["out"].ref, c["out"])
    b = A.base_bwd(c["qkv"], c["bias"], hd ** -0.5, None, A.unheads(c["out"]).to(BF16), f["lse"].ref.to(F32), c["d_o"], B, H, N, hd)
    assert rel(b["dv"].ref, c["dv"]) < 1e-6              # P = 2^(x - fp32(lse)) is 1 to fp32 rounding; the kernel's bf16(P) is 1
    for name in ("dq", "dk", "dbias"):                   # true value 0: dP and delta are the same sum, written twice
        assert b[name].ref.abs().max() < 1e-9 and (b[name].bound > 0).all(), name


@pytest.mark.parametrize("hd,tail_only", [(64, False), (80, False), (80, True)])
@pytest.mark.parametrize("N", [5, 33, 197, 208])
def test_score_selected_permutation_is_one_hot(hd, tail_only, N):
    B, H = 2, 4
    c = A.score_selected(B, N, hd, tail_only=tail_only)
    assert torch.equal(c["qkv"].float().to(BF16), c["qkv"]) and (A.split(c["qkv"], B, H, N, hd)[2] != 0).all()
    for bias in (None, torch.zeros(H, N, N)):
        f = A.base_fwd(c["qkv"], bias, hd ** -0.5, None, B, H, N, hd)
        mass, peaks = A.off_peak_mass(f["P"], c["pi"])
        assert mass < 2.0 ** -40 and peaks, mass
        assert rel(f["out"].ref, c["out"]) < 2.0 ** -38


# ---- the two-stream core: the premises of its exact cases, in the reference's arithmetic -------------------------------------------
def two_stream_P(qkv_m, qkv_c, bias, B, H, N):
    from oracle.vit_oracle_dist import wasserstein_distance_matmul
    q, k, _ = A.split(qkv_m.double(), B, H, N, 64)
    cq, ck, _ = A.split(qkv_c.double(), B, H, N, 64)
    a = torch.sigmoid(-wasserstein_distance_matmul(q * 0.125, cq, k, ck) + 1e-24)
    return (a if bias is None else a + bias.double()).softmax(-1)


@pytest.mark.parametrize("N", [1, 33, 197])
def test_two_stream_exact_case_premises(N):
    B, H = 2, 4
    c = A.two_stream_selected(B, N)
    Pm = two_stream_P(c["qkv_m"], c["qkv_c"], c["bias"], B, H, N)
    mass, peaks = A.off_peak_mass(Pm, c["pi"])
    assert mass == 0.0 and peaks
    assert torch.equal(Pm @ A.split(c["qkv_m"], B, H, N, 64)[2].double(), c["out_m"])
    assert torch.equal(Pm ** 2 @ A.split(c["qkv_c"], B, H, N, 64)[2].double(), c["out_c"])
    Pm = two_stream_P(A.readout_qkv(B, H, N, 64, 0), torch.ones(B * N, 3 * H * 64, dtype=BF16), None, B, H, N)
    assert torch.equal(Pm, torch.full_like(Pm, 1.0 / N))


# ---- the two-stream core: restatement, emulation, mutations -----------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_two_stream_restatement_is_autograd(with_bias, p):
    from oracle.vit_oracle_dist import wasserstein_distance_matmul
    B, H, N = 2, 3, 37
    qkv_m, qkv_c, pre_c, bias, d_m, d_c = A.ws_inputs("flat", B, H, N)
    keep = keep_of(B, H, N, p)
    xm = qkv_m.double().requires_grad_(True)
    bq = ((bias.float() * A.LOG2E).double() / A.LOG2E).requires_grad_(True) if with_bias else None
    # the call receives y = bf16(ELU(pre) + 1), never pre: the gradient wrt y, times ELU'(pre) = min(y, 1) as include/uvit.h folds it in
    xc = qkv_c.double().requires_grad_(True)
    q, k, v = A.split(xm, B, H, N, 64)
    cq, ck, cv = A.split(xc, B, H, N, 64)
    a = torch.sigmoid(-wasserstein_distance_matmul(q * 0.125, cq, k, ck) + 1e-24)
    lse = torch.logsumexp(a if bq is None else a + bq, -1)
    a = (a if bq is None else a + bq).softmax(-1)
    if keep is not None:
        a = a * keep.double()
    om, oc = a @ v, (a ** 2) @ cv
    ((om * A.heads(d_m.double(), B, H, N, 64)).sum() + (oc * A.heads(d_c.double(), B, H, N, 64)).sum()).backward()
    f = A.ws_fwd(qkv_m, qkv_c, bias if with_bias else None, 0.125, keep, B, H, N, images=False)
    assert rel(f["out_m"].ref, om.detach()) < 1e-12 and rel(f["out_c"].ref, oc.detach()) < 1e-12
    assert rel(f["lse"].ref, lse.detach() * A.LOG2E) < 1e-12
    r = A.ws_bwd(qkv_m, qkv_c, bias if with_bias else None, 0.125, keep, A.unheads(om.detach()), A.unheads(oc.detach()), d_m, d_c,
                 lse.detach() * A.LOG2E, B, H, N, images=False)
    gm, gc = A.split(xm.grad, B, H, N, 64), A.split(xc.grad * xc.detach().clamp(max=1.0), B, H, N, 64)
    for name, g in (("dq_m", gm[0]), ("dk_m", gm[1]), ("dv_m", gm[2]), ("dq_c", gc[0]), ("dk_c", gc[1]), ("dv_c", gc[2])):
        assert rel(r[name].ref, g) < 1e-12, (name, rel(r[name].ref, g))
    if with_bias:
        assert rel(r["dbias"].ref, bq.grad) < 1e-12


def run_ws_emulation(regime, N, with_bias, p, B=2, H=2, slab0=None, keep_emul=None, **hooks):
    qkv_m, qkv_c, _, bias, d_m, d_c = A.ws_inputs(regime, B, H, N)
    bias = bias if with_bias else None
    keep = keep_of(B, H, N, p)
    qm_e = swap_kv_pair(qkv_m, B, H, N, 64) if hooks.pop("swap_kv", False) else qkv_m
    e = A.emulate_ws(qm_e, qkv_c, bias, 0.125, keep if keep_emul is None else keep_emul, d_m, d_c, B, H, N, slab0=slab0, **hooks)
    g = A.emulate_ws(qkv_m, qkv_c, bias, 0.125, keep, d_m, d_c, B, H, N)           # the GIVEN o_m, o_c, lse: the unmutated forward's
    f = A.ws_fwd(qkv_m, qkv_c, bias, 0.125, keep, B, H, N)
    assert f["lse"].bound.max().item() <= 3e-3
    r = A.ws_bwd(qkv_m, qkv_c, bias, 0.125, keep, A.unheads(g["out_m"]), A.unheads(g["out_c"]), d_m, d_c, g["lse"], B, H, N, slab0=slab0)
    worst = {n: A.compare("emul2", n, e[n], f[n], check=False)[0] for n in ("out_m", "out_c", "lse")}
    worst.update({n: A.compare("emul2", n, e[n], r[n], check=False)[0] for n in A.WS_OUTPUTS + (("dbias",) if with_bias else ())})
    return worst, f


@pytest.mark.parametrize("regime", ["flat", "peaked"])
@pytest.mark.parametrize("N", [1, 33, 197])
@pytest.mark.parametrize("with_bias,p", [(True, 0.1), (False, 0.0)])
def test_two_stream_emulation_passes_every_bound(regime, N, with_bias, p):
    slab0 = A._rnd(2, N, N, seed=5) if with_bias and N == 33 else None
    worst, _ = run_ws_emulation(regime, N, with_bias, p, slab0=slab0)
    print(f"\ntwo-stream emulation {regime} N {N} bias {with_bias} p {p}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0, worst


@pytest.mark.parametrize("regime", ["flat", "peaked"])
def test_two_stream_mutations_fail(regime):
    B, H, N, p = 2, 2, 197, 0.1
    _, f = run_ws_emulation(regime, N, True, p)
    top = int(f["P"][1, 0, 40].argmax())
    kf = keep_of(B, H, N, p).clone()
    kf[1, 0, 40, top] = kf.max() - kf[1, 0, 40, top]

    def zero_top_ws(t):
        t = t.clone()
        t[1, 1, 70, int(f["P"][1, 1, 70].argmax())] = 0
        return t

    def exact_delta_in_tile_ws(dl, tile=4):          # delta from the EXACT out_m, out_c in one query tile, from the given ones elsewhere
        _, _, _, _, d_m, d_c = A.ws_inputs(regime, B, H, N)
        dm, dc = A.heads(d_m, B, H, N, 64).double(), A.heads(d_c, B, H, N, 64).double()
        dl = dl.clone()
        dl[:, :, 16 * tile:16 * tile + 16] = ((dm * f["out_m"].ref).sum(-1) + 2 * (dc * f["out_c"].ref).sum(-1))[:, :, 16 * tile:16 * tile + 16]
        return dl

    for what, kw, must in (("P zeroed on a row's top key", dict(p_hook=zero_top_ws), ("out_m", "out_c", "dv_m", "dq_m")),
                           ("one keep bit flipped", dict(keep_emul=kf), ("out_m", "dv_m")),
                           ("K and V rows swapped in one key pair (mean stream)", dict(swap_kv=True), ("out_m", "dk_m", "dbias")),      # (dV reads P alone: flat columns are alike)
                           ("delta from the exact outputs in one query tile", dict(delta_hook=exact_delta_in_tile_ws), ("delta",))):
        worst, _ = run_ws_emulation(regime, N, True, p, **kw)
        print(f"\ntwo-stream {regime}: {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        for name in must:
            assert worst[name] > 1.0, (what, name, worst[name])
