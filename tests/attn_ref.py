"""float64 restatements (torch, device-agnostic) of the base attention core and of the two-stream Wasserstein core, forward and
backward, as functions of exactly what the C ABI call receives, with an absolute error bound per element; the comparator that holds
those bounds and names the tile of the worst element; and the generators of the exact cases (permutations selected by the bias or by
the scores, the uniform read-out of the dropout mask).  Written from the reference's arithmetic (Attention.forward,
modeling_finetune.py:152-185: softmax(q scale k^T + bias) -> dropout -> @ v; oracle/vit_oracle_dist.py for the two-stream core), not
from the kernels: the kernels are only read for WHERE they round.  tests/test_host_attn_ref.py pins this file on the CPU;
tests/test_gpu_attn_bounds.py applies it to the kernels.

What a call receives: bf16 qkv (B N, 3 H hd); the bias (H, N, N) in natural units (the test hands the kernel
padded_bias(bias) = fp32(bias log2 e)); scale (as the fp32 the ABI passes); the keep multipliers of oracle.vit_oracle.attn_keep_mask
(0 or fp32(1 / (1 - p))); for the backward the GIVEN o_fwd (bf16), the GIVEN lse (fp32, log2 units) and d_o (bf16).  The backward
reference computes delta = rowsum(dO o o_fwd) from the given o_fwd, P = 2^(x - lse_given), dS = Pd dP - P delta: the function the
kernel is specified to compute (include/uvit.h), so what remains is the kernel's own error.  Scores x and lse are in log2 units.

Bounds are derived, not tuned.  The rule: every bf16 rounding point of the kernel contributes u8 = 2^-8 (the unit round-off of bf16,
rowwise_ref.BF_ULP) times the sum of |terms| that pass through it; what the kernel forms in fp32 contributes terms in u = 2^-24 that
are two orders smaller.  Each bound is written where it is computed, in a comment that cites the kernel line it comes from
(csrc/attention.hip for the base core, csrc/attention2.hip for the two-stream core).  Padded slab rows and columns are zero bit for
bit (accumulate 0: uvit_zero_launch, attention.hip:809) or untouched (accumulate 1).
"""
import math

import numpy as np
import torch

from rowwise_ref import BF16, BF_ULP, F32, F64, SENT16, SENT32, U, WORST, bits  # noqa: F401

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
TINY = 2.0 ** -100                 # absolute floor on a probability: the hardware exp2 flushes p < 2^-126 to zero
TILE = 16


def g_dot(n):
    """Relative to the sum of |products|: an fp32 MFMA contraction of n exact bf16 x bf16 products (no assumption on the rounding mode of
    the adds inside v_mfma_f32_16x16x32_bf16, hence the 2), or a lane's serial fp32 sum plus the shuffle tree"""
    return 2 * (n + 8) * U


class Val:
    """One output: float64 value, absolute bound per element, and the meaning of each axis ('b', 'h', 'q', 'k', 'd')."""

    def __init__(self, ref, bound, axes):
        assert ref.dim() == len(axes) and (bound is None or bound.shape == ref.shape)
        self.ref, self.bound, self.axes = ref, bound, axes


def where(axes, shape, flat):
    idx = np.unravel_index(int(flat), tuple(shape))
    names = {"b": "b", "h": "h", "q": "query tile", "k": "key tile", "d": "d-tile"}
    return ", ".join(f"{names[a]} {int(i) // TILE if a in 'qkd' else int(i)}" + (f" ({a} {int(i)})" if a in "qkd" else "")
                     for a, i in zip(axes, idx))


def compare(op, name, got, val, exact=False, check=True):
    """got: tensor shaped like val.ref.  Returns (worst |got - ref| / bound, where); asserts worst <= 1 (exact: equality of values)."""
    g, r = got.to(F64).cpu(), val.ref.to(F64).cpu()
    assert g.shape == r.shape, (op, name, tuple(g.shape), tuple(r.shape))
    assert torch.isfinite(g).all(), f"{op}: {name}: non-finite value"
    d = (g - r).abs()
    if exact:
        bad = int(d.argmax())
        assert torch.equal(g, r), f"{op}: {name}: not equal at {where(val.axes, r.shape, bad)}: got {g.flatten()[bad].item()!r}, " \
                                  f"expected {r.flatten()[bad].item()!r} ({int((d != 0).sum())} elements differ)"
        return 0.0, ""
    ratio = torch.where(d == 0, torch.zeros_like(d), d / val.bound.to(F64).cpu())
    worst, at = (ratio.max().item(), int(ratio.argmax())) if ratio.numel() else (0.0, 0)
    loc = where(val.axes, r.shape, at)
    key = f"{op} {name}"
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if check:
        assert worst <= 1.0, f"{op}: {name}: |got - ref| is {worst:.3g} x its bound at {loc} (|diff| {d.flatten()[at].item():.3e})"
    return worst, loc


# ---- layouts -------------------------------------------------------------------------------------------------------------------
def heads(buf, B, H, N, hd):
    """(B N, H hd) -> (B, H, N, hd)"""
    return buf.reshape(B, N, H, hd).permute(0, 2, 1, 3)


def unheads(t):
    """(B, H, N, hd) -> (B N, H hd)"""
    B, H, N, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * hd)


def split(qkv, B, H, N, hd):
    """(B N, 3 H hd) -> q, k, v (B, H, N, hd)"""
    return qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)


def join(q, k, v):
    B, H, N, hd = q.shape
    return torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * hd)


def slab_dbias(slab, N):
    """The kernels' [h][key][q] slab -> dbias (H, q, k)"""
    return slab[:, :N, :N].transpose(1, 2)


def scale32(scale):
    return float(np.float32(scale))


# ---- the base core -------------------------------------------------------------------------------------------------------------
def _scores(qkv, bias, scale, B, H, N, hd, dt=F64):
    """-> q, k, v, the scores x (log2 units) and dx, the bound on the error of the kernel's fp32 score"""
    q, k, v = (t.to(dt) for t in split(qkv, B, H, N, hd))
    c = scale32(scale) * LOG2E
    x = (q @ k.transpose(-1, -2)) * c
    b2 = None
    if bias is not None:
        b2 = (bias.to(F32) * LOG2E).to(dt)[None]              # padded_bias: the product is rounded to fp32; the reference adds that number
        x = x + b2
    # the dot in fp32 MFMAs (:164-166, :459-466): g_dot(hd) c sum |q| |k|;  dot * c + bias, fused or not (:171, :499): u |dot c| + u |x|,
    # and |dot c| <= |x| + |bias log2 e|
    dx = g_dot(hd) * c * (q.abs() @ k.abs().transpose(-1, -2)) + 2 * U * x.abs() + (U * b2.abs() if b2 is not None else 0.0)
    return q, k, v, x, dx


def _keep(keep, x):
    return torch.ones_like(x) if keep is None else keep.to(x.dtype).to(x.device)


def _e_p(x, dx, lse):
    """Relative error of a probability formed in fp32: the score, the subtraction of mx or lse (:187, :499; |mx| <= |lse| + 8), the
    hardware exp2 (1 ulp), * inv_keep (:500) and inv_keep = 1 / (1 - p) itself.  ~1e-5 here: two orders below u8"""
    return LN2 * (dx + 2 * U * (x.abs() + lse.abs()[..., None] + 8)) + 5 * U


def _softmax(x, dx, N):
    """-> P, lse, mx, log2 of the row sum, e_p, and e_row: the relative error of the forward's row sum (:189, :193) and of
    inv_keep / sum (:233)"""
    mx = x.amax(-1, keepdim=True)
    p = torch.exp2(x - mx)
    s = p.sum(-1, keepdim=True)
    Pm = p / s
    lse = (mx + torch.log2(s)).squeeze(-1)
    e_p = _e_p(x, dx, lse)
    e_row = (e_p * Pm).sum(-1, keepdim=True) + g_dot(N) + 4 * U
    return Pm, lse, mx, torch.log2(s).squeeze(-1), e_p, e_row


def _lse_bound(Pm, x, dx, mx, log2s, lse, N):
    """fp32 only (:194): the P-weighted score error (mx itself cancels), the row sum, the hardware log (1 ulp, with an absolute floor
    near sum = 1), the last add"""
    return (Pm * (dx + U * (x - mx).abs())).sum(-1) + (g_dot(N) + 4 * U) / LN2 + 4 * U * (log2s.abs() + 1) + U * lse.abs()


def base_fwd(qkv, bias, scale, keep, B, H, N, hd):
    """-> dict out (B, H, N, hd), lse (B, H, N; log2 units) as Vals, and the float64 P, Pd, x the host pins look at."""
    q, k, v, x, dx = _scores(qkv, bias, scale, B, H, N, hd)
    Pm, lse, mx, log2s, e_p, e_row = _softmax(x, dx, N)
    Pd = Pm * _keep(keep, x)
    out = Pd @ v
    # out: p -> bf16 when packed (:217) and * f -> bf16 (:237): 2 u8;  the fp32 MFMA over the keys (:221): g_dot(N);  each p's and the row
    # sum's fp32 error: e_p + e_row;  all on sum_k Pd |V|.  TINY: a p < 2^-126 the hardware exp2 flushes to zero
    b_out = (2 * BF_ULP + g_dot(N)) * (Pd @ v.abs()) + ((e_p + e_row) * Pd + TINY) @ v.abs()
    return {"out": Val(out, b_out, "bhqd"), "lse": Val(lse, _lse_bound(Pm, x, dx, mx, log2s, lse, N), "bhq"), "P": Pm, "Pd": Pd, "x": x}


def base_bwd(qkv, bias, scale, keep, o_fwd, lse, d_o, B, H, N, hd, slab0=None):
    """-> dict delta (B, H, N), dq, dk, dv (B, H, N, hd), dbias (H, q, k) as Vals; dS, P in float64.  slab0: what the (H, q, k) part of
    the slab held before an accumulating call (None: the call overwrites)."""
    q, k, v, x, dx = _scores(qkv, bias, scale, B, H, N, hd)
    do, o = heads(d_o, B, H, N, hd).to(F64), heads(o_fwd, B, H, N, hd).to(F64)
    lse = lse.to(F64).reshape(B, H, N)
    delta = (do * o).sum(-1)
    b_delta = (hd + 8) * U * (do.abs() * o.abs()).sum(-1)           # serial fp32 per lane, two shuffles (:381-389)
    Pm = torch.exp2(x - lse[..., None])
    Pd = Pm * _keep(keep, x)
    dP = do @ v.transpose(-1, -2)
    b_dP = g_dot(hd) * (do.abs() @ v.abs().transpose(-1, -2))       # fp32 MFMAs (:476-483)
    t1, t2 = Pd * dP, Pm * delta[..., None]
    dS = t1 - t2
    e_p = _e_p(x, dx, lse)
    # dS in fp32 (:499-502): both products carry e_p and their factors' errors, the subtraction (fused or not) 4 u on the |terms|
    r32 = (e_p + 4 * U) * (t1.abs() + t2.abs()) + (Pd + TINY) * b_dP + (Pm + TINY) * b_delta[..., None] + TINY
    # stored ONCE as bf16 (:511 step buffer, :516 pack8): dQ, dK and the streamed dS (:609) all read that one rounded value
    r_dS = BF_ULP * (dS.abs() + r32) + r32
    sc = scale32(scale)

    def contracted(ds, r, other):
        """scale sum ds other: the stored dS's error against |other|, the fp32 MFMA over N (:522, :549), the bf16 store (:578, :655-660)"""
        val = sc * (ds @ other)
        rest = sc * (r @ other.abs()) + g_dot(N) * sc * (ds.abs() @ other.abs())
        return val, rest + BF_ULP * (val.abs() + rest)

    dq, b_dq = contracted(dS, r_dS, k)
    dk, b_dk = contracted(dS.transpose(-1, -2), r_dS.transpose(-1, -2), q)
    PdT = Pd.transpose(-1, -2)
    dv = PdT @ do
    # dV: pd -> bf16 (:510) and the result -> bf16 (:578): 2 u8;  pd's own e_p;  the fp32 MFMA over the queries (:549)
    b_dv = (((2 * BF_ULP + e_p) * Pd).transpose(-1, -2) + TINY) @ do.abs() + g_dot(N) * (PdT @ do.abs())
    res = {"delta": Val(delta, b_delta, "bhq"), "dq": Val(dq, b_dq, "bhqd"), "dk": Val(dk, b_dk, "bhkd"), "dv": Val(dv, b_dv, "bhkd"),
           "dS": dS, "P": Pm, "Pd": Pd}
    s0 = torch.zeros_like(dS[0]) if slab0 is None else slab0.to(F64)
    # attn_dbias_reduce_kernel sums the STORED bf16 dS (:695-697: it reads the step-buffer images stream_ds copied out, :609) in fp32,
    # then one atomic per element on top of what the slab held (:712)
    res["dbias"] = Val(s0 + dS.sum(0), r_dS.sum(0) + (B + 9) * U * (s0.abs() + dS.abs().sum(0)), "hqk")
    return res


# ---- the same arithmetic in another summation order, fp32 intermediates, bf16 roundings at the cited points ------------------------
def _r16(t):
    return t.to(BF16).to(F32)


def _mm32(a, b):
    """fp32 a @ b with the contraction index walked backwards"""
    return a.to(F32).flip(-1) @ b.to(F32).flip(-2)


def _x32(qkv, bias, scale, B, H, N, hd):
    q, k, v = (t.to(F32) for t in split(qkv, B, H, N, hd))
    c = torch.tensor(scale32(scale), dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    x = _mm32(q, k.transpose(-1, -2)) * c
    if bias is not None:
        x = x + (bias.to(F32) * LOG2E)[None]
    return q, k, v, x


def emulate_fwd(qkv, bias, scale, keep, B, H, N, hd, p_hook=None):
    """-> out (B N, H hd) bf16, lse (B, H, N) fp32, as the kernel's buffers"""
    q, k, v, x = _x32(qkv, bias, scale, B, H, N, hd)
    mx = x.amax(-1, keepdim=True)
    p = torch.exp2(x - mx)
    s = p.flip(-1).sum(-1, keepdim=True)
    lse = (mx + torch.log2(s)).squeeze(-1)
    kp = _keep(keep, x)
    pk = _r16(torch.where(kp != 0, p, torch.zeros_like(p)))          # :217
    if p_hook is not None:
        pk = p_hook(pk)
    inv_keep = kp.amax() if keep is not None else torch.tensor(1.0)
    o = _mm32(pk, v) * (inv_keep.to(F32) / s)
    return unheads(o.to(BF16)), lse                                  # :237


def emulate_bwd(qkv, bias, scale, keep, o_fwd, lse, d_o, B, H, N, hd, slab0=None, p_hook=None, delta=None):
    """-> delta (B, H, N) fp32, dqkv (B N, 3 H hd) bf16, dbias (H, q, k) fp32"""
    q, k, v, x = _x32(qkv, bias, scale, B, H, N, hd)
    do, o = heads(d_o, B, H, N, hd).to(F32), heads(o_fwd, B, H, N, hd).to(F32)
    dl = (do * o).flip(-1).sum(-1) if delta is None else delta.to(F32)
    p = torch.exp2(x - lse.to(F32).reshape(B, H, N)[..., None])
    if p_hook is not None:
        p = p_hook(p)
    pd = p * _keep(keep, x)
    dp = _mm32(do, v.transpose(-1, -2))
    ds = _r16(pd * dp - p * dl[..., None])                            # :511, :516
    pd = _r16(pd)                                                    # :510
    sc = torch.tensor(scale32(scale), dtype=F32)
    dq = (_mm32(ds, k) * sc).to(BF16)
    dk = (_mm32(ds.transpose(-1, -2), q) * sc).to(BF16)
    dv = _mm32(pd.transpose(-1, -2), do).to(BF16)
    db = ds.flip(0).sum(0)
    if slab0 is not None:
        db = slab0.to(F32) + db
    return dl, join(dq, dk, dv), db


# ---- the two-stream core -------------------------------------------------------------------------------------------------------
# Reference arithmetic: oracle.vit_oracle_dist.wasserstein_distance_matmul / attention (modeling_finetune_dist.py:111-179):
#   m1 = sig(q scale), m2 = sig(k), c1 = sig(cov_q), c2 = sig(cov_k) (cov_* as stored: ELU(.) + 1);  W = r_i + c_j - 2 (m1.m2 + sqrt c1.sqrt c2),
#   r_i = sum m1^2 + c1;  P = softmax(sig(-W) + bias);  PD = keep P;  out_m = PD v;  out_c = PD^2 cov_v.
# csrc/attention2.hip (the lines cited below) contracts the bf16 IMAGES of m1, sqrt c1, m2, sqrt c2 (:42-43, :59).  As unknown roundings
# they would move W by up to 4 u8 sum(m1 m2 + sqrt(c1 c2)), about 1.  The rounding is deterministic, so the restatement forms the images
# itself from the float64 values (images=True) and an image costs an error term only where the kernel's can differ from it (_image).
def _sig_err(x):
    """Relative error of the kernel's fp32 sigm(x) = rcp(1 + __expf(-x)): the exponent's product, the hardware exp2, the add, the
    hardware rcp.  (sqrtf of it: half of this + 2 u)"""
    return (x.abs() + 16) * U


def _image(v, e, images):
    """The bf16 image of v > 0 and the bound on its distance from the image of any v (1 +- e): one bf16 ulp where those two round
    differently (v lies within e of a rounding tie), else 0"""
    if not images:
        return v, torch.zeros_like(v)
    risk = (v * (1 - e)).to(BF16) != (v * (1 + e)).to(BF16)
    return v.to(BF16).to(F64), risk.to(F64) * torch.exp2(torch.floor(torch.log2(v)) - 7)


def _ws_scores(qkv_m, qkv_c, bias, scale, B, H, N, images):
    q, k, v = split(qkv_m.to(F64), B, H, N, 64)
    cq, ck, cv = split(qkv_c.to(F64), B, H, N, 64)
    sc = scale32(scale)
    o = dict(v=v, cv=cv, cq=cq, ck=ck, sc=sc)
    for n, xx in (("m1", q * sc), ("m2", k), ("c1", cq), ("c2", ck)):
        o[n], o["e_" + n] = torch.sigmoid(xx), _sig_err(xx)
    for n, val, e in (("Am", o["m1"], o["e_m1"]), ("Bm", o["m2"], o["e_m2"]), ("Ac", o["c1"].sqrt(), o["e_c1"] / 2 + 2 * U),
                      ("Bc", o["c2"].sqrt(), o["e_c2"] / 2 + 2 * U)):
        o[n], o["d" + n] = _image(val, e, images)                  # the operand images (:42-43, :59)
    T = lambda t: t.transpose(-1, -2)      # noqa: E731
    dot = o["Am"] @ T(o["Bm"]) + o["Ac"] @ T(o["Bc"])
    # the K = 128 contraction (:157-158, :463-470): the at-risk ulps against the other operand, the fp32 MFMA
    ddot = o["dAm"] @ T(o["Bm"]) + o["Am"] @ T(o["dBm"]) + o["dAc"] @ T(o["Bc"]) + o["Ac"] @ T(o["dBc"]) + g_dot(128) * dot
    ri = (o["m1"] ** 2 + o["c1"]).sum(-1, keepdim=True)
    cj = T((o["m2"] ** 2 + o["c2"]).sum(-1, keepdim=True))
    # the row / column terms are fp32 sums of the UNROUNDED values (:41; :57-58, :134, :356-360): the sigmoids' errors, 128 adds
    dri = (2 * o["e_m1"] * o["m1"] ** 2 + o["e_c1"] * o["c1"]).sum(-1, keepdim=True) + 136 * U * ri
    dcj = T((2 * o["e_m2"] * o["m2"] ** 2 + o["e_c2"] * o["c2"]).sum(-1, keepdim=True)) + 136 * U * cj
    arg = 2 * dot - ri - cj + 1e-24
    dW = 2 * ddot + dri + dcj + 4 * U * (2 * dot + ri + cj)       # 2 a - r_i - c_j (:166, :494)
    sg = torch.sigmoid(arg)
    # sigmoid' <= min(1/4, sg e^dW) on the interval, and the fp32 sigm's own error
    dsg = dW * torch.minimum(torch.full_like(sg, 0.25), sg * torch.exp(dW)) + _sig_err(arg) * sg
    x = sg * LOG2E
    b2 = None
    if bias is not None:
        b2 = (bias.to(F32) * LOG2E).to(F64)[None]
        x = x + b2
    dx = LOG2E * dsg + 2 * U * x.abs() + (U * b2.abs() if b2 is not None else 0.0)      # sg * log2 e + bias (:166, :495)
    o.update(x=x, dx=dx, sg=sg, dsg=dsg)
    return o


def ws_fwd(qkv_m, qkv_c, bias, scale, keep, B, H, N, images=True):
    """-> dict out_m, out_c (B, H, N, 64), lse (B, H, N) as Vals, P, Pd.  images=False: the reference formula itself (no bf16 images)."""
    o = _ws_scores(qkv_m, qkv_c, bias, scale, B, H, N, images)
    x, dx, v, cv = o["x"], o["dx"], o["v"], o["cv"]
    Pm, lse, mx, log2s, e_p, e_row = _softmax(x, dx, N)            # (:175-184, as the base core)
    Pd = Pm * _keep(keep, x)
    rel = e_p + e_row + 2 * U                                       # of pa = p * f (:196)
    P2 = Pd * Pd
    # out_m: pa -> bf16 (:208) and the result -> bf16 (:222): 2 u8;  the fp32 MFMA over the keys (:212);  pa's own error
    b_m = (2 * BF_ULP + g_dot(N)) * (Pd @ v.abs()) + (rel * Pd + TINY) @ v.abs()
    # out_c: the same through pa^2 (:207-208, :213, :223), whose relative error is twice pa's
    b_c = (2 * BF_ULP + g_dot(N)) * (P2 @ cv.abs()) + ((2 * rel + 2 * U) * P2 + TINY) @ cv.abs()
    return {"out_m": Val(Pd @ v, b_m, "bhqd"), "out_c": Val(P2 @ cv, b_c, "bhqd"),
            "lse": Val(lse, _lse_bound(Pm, x, dx, mx, log2s, lse, N), "bhq"), "P": Pm, "Pd": Pd}


def ws_bwd(qkv_m, qkv_c, bias, scale, keep, o_m, o_c, d_m, d_c, lse, B, H, N, slab0=None, images=True):
    """-> dict delta, dq_m, dk_m, dv_m, dq_c, dk_c, dv_c (the cov gradients are those of the PRE-ELU values), dbias as Vals."""
    o = _ws_scores(qkv_m, qkv_c, bias, scale, B, H, N, images)
    x, dx, v, cv, sg, dsg = o["x"], o["dx"], o["v"], o["cv"], o["sg"], o["dsg"]
    T = lambda t: t.transpose(-1, -2)      # noqa: E731
    dm, dc, om, oc = (heads(t, B, H, N, 64).to(F64) for t in (d_m, d_c, o_m, o_c))
    lse = lse.to(F64).reshape(B, H, N)
    delta = (dm * om).sum(-1) + 2 * (dc * oc).sum(-1)
    b_delta = 136 * U * ((dm * om).abs().sum(-1) + 2 * (dc * oc).abs().sum(-1))       # 128 products, serial fp32 + shuffles (:415)
    Pm = torch.exp2(x - lse[..., None])
    K = _keep(keep, x)
    Pd = Pm * K
    e_p = _e_p(x, dx, lse)
    pm, pc = dm @ T(v), dc @ T(cv)                                                     # fp32 MFMAs (:478-486)
    b_pm, b_pc = g_dot(64) * (dm.abs() @ T(v.abs())), g_dot(64) * (dc.abs() @ T(cv.abs()))
    # dS = P (K (pm + 2 PD pc) - delta) (:495-499), as the sum of three terms
    a1, a2, a3 = Pd * pm, 2 * Pd * Pd * pc, Pm * delta[..., None]
    dS = a1 + a2 - a3
    # in fp32: every term carries e_p (a2 twice: P and PD) and 6 u of products and adds, plus its factors' own errors
    r32 = ((e_p + 6 * U) * (a1.abs() + a2.abs() + a3.abs()) + e_p * a2.abs() + (Pd + TINY) * (b_pm + 2 * Pd * b_pc)
           + (Pm + TINY) * b_delta[..., None] + TINY)
    r_dS = BF_ULP * (dS.abs() + r32) + r32              # stored as bf16 for the slab (:511-512)
    t = sg * (1 - sg)
    gv = -dS * t                                        # gW = dL/dW (:500)
    r_gv = r32 * t + dS.abs() * (dsg + 4 * U * t)       # in fp32: dS's error, and sg (1 - sg)'s (<= dsg)
    r_gw = BF_ULP * (gv.abs() + r_gv) + r_gv            # stored ONCE as bf16 (:506): every product below reads that value
    # d r_i adds the fp32 values over the keys (:502, :647), d c_j the stored ones through an all-ones MFMA (:558)
    side_q, e_side_q = gv.sum(-1, keepdim=True), r_gv.sum(-1, keepdim=True) + g_dot(N) * gv.abs().sum(-1, keepdim=True)
    side_k, e_side_k = T(gv.sum(-2, keepdim=True)), T(r_gw.sum(-2, keepdim=True) + g_dot(N) * gv.abs().sum(-2, keepdim=True))

    def contr(g, r, img, dimg):
        """sum gW16 x operand image (dA over the keys :519-520, dB over the queries :552): gW's error against the image, |gW| against the
        image's at-risk ulp, the fp32 MFMA"""
        return g @ img, r @ img + g.abs() @ dimg + g_dot(N) * (g.abs() @ img)

    def back_mean(dA, side, m, e_m, pre):
        """(-2 dA + 2 m dside) m (1 - m) pre (:230-233), stored as bf16 (:576, :656): each term's error times the factor; the factor's
        relative error (1 - m is formed from the rounded m: e_m m / (1 - m)) on the sum of |terms|; u8 on the store"""
        (a, e_a), (sd, e_sd) = dA, side
        f = m * (1 - m) * pre
        val = (-2 * a + 2 * m * sd) * f
        S = 2 * a.abs() + 2 * m * sd.abs()
        err = (2 * e_a + 2 * m * e_sd) * f + (e_m * (2 + m / (1 - m)) + 8 * U) * S * f
        return val, err + BF_ULP * (val.abs() + err)

    def back_cov(dA, side, c, e_c, y):
        """(-dA / sqrt c + dside) c (1 - c) min(y, 1) (:234-238; ELU' of the pre-activation is min(y, 1)), stored as bf16 (:580, :657):
        as back_mean, with the hardware rsq (e_c / 2 + 4 u)"""
        (a, e_a), (sd, e_sd) = dA, side
        rs = c.rsqrt()
        f = c * (1 - c) * y.clamp(max=1.0)
        val = (-a * rs + sd) * f
        S = a.abs() * rs + sd.abs()
        err = (e_a * rs + e_sd + (e_c / 2 + 4 * U) * a.abs() * rs) * f + (e_c * (1 + c / (1 - c)) + 8 * U) * S * f
        return val, err + BF_ULP * (val.abs() + err)

    res = {"delta": Val(delta, b_delta, "bhq")}
    for name, axes, got in (
            ("dq_m", "bhqd", back_mean(contr(gv, r_gw, o["Bm"], o["dBm"]), (side_q, e_side_q), o["m1"], o["e_m1"], o["sc"])),
            ("dk_m", "bhkd", back_mean(contr(T(gv), T(r_gw), o["Am"], o["dAm"]), (side_k, e_side_k), o["m2"], o["e_m2"], 1.0)),
            ("dq_c", "bhqd", back_cov(contr(gv, r_gw, o["Bc"], o["dBc"]), (side_q, e_side_q), o["c1"], o["e_c1"], o["cq"])),
            ("dk_c", "bhkd", back_cov(contr(T(gv), T(r_gw), o["Ac"], o["dAc"]), (side_k, e_side_k), o["c2"], o["e_c2"], o["ck"]))):
        res[name] = Val(got[0], got[1], axes)
    P2 = Pd * Pd
    # dV_m: PD -> bf16 (:504) and the result -> bf16 (:585): 2 u8;  PD's e_p;  the fp32 MFMA over the queries (:552)
    res["dv_m"] = Val(T(Pd) @ dm, (T((2 * BF_ULP + e_p) * Pd) + TINY) @ dm.abs() + g_dot(N) * (T(Pd) @ dm.abs()), "bhkd")
    # dV_c: the same through PD^2 (:505, :556) with twice the e_p, times ELU' = min(cov_v, 1) (:586)
    el = cv.clamp(max=1.0)
    res["dv_c"] = Val((T(P2) @ dc) * el, ((T((2 * BF_ULP + 2 * e_p + 4 * U) * P2) + TINY) @ dc.abs() + g_dot(N) * (T(P2) @ dc.abs())) * el, "bhkd")
    s0 = torch.zeros_like(dS[0]) if slab0 is None else slab0.to(F64)
    # attn2_dbias_reduce_kernel sums the stored bf16 dS in fp32 (:687-689), one atomic per element on top of the slab (:699)
    res["dbias"] = Val(s0 + dS.sum(0), r_dS.sum(0) + (B + 9) * U * (s0.abs() + dS.abs().sum(0)), "hqk")
    res.update(dS=dS, P=Pm, Pd=Pd)
    return res


def ws_inputs(regime, B, H, N, seed=1):
    """qkv_m, qkv_c (= ELU(.) + 1 of the bf16 pre-activation, as the QKV epilogue stores it), pre_c, bias, d_m, d_c: the inputs of
    test_wasserstein_attention_fwd_bwd (flat: bias scale 0.5); peaked: bias scale 4, the only handle that peaks this core."""
    Cd = H * 64
    qkv_m = _rnd(B * N, 3 * Cd, seed=seed).to(BF16)
    pre_c = _rnd(B * N, 3 * Cd, seed=seed + 1).to(BF16)
    qkv_c = (torch.nn.functional.elu(pre_c.float()) + 1).to(BF16)
    bias = _rnd(H, N, N, scale=0.5 if regime == "flat" else 4.0, seed=seed + 2)
    d_m, d_c = _rnd(B * N, Cd, scale=0.5, seed=seed + 3).to(BF16), _rnd(B * N, Cd, scale=0.5, seed=seed + 4).to(BF16)
    return qkv_m, qkv_c, pre_c, bias, d_m, d_c


def emulate_ws(qkv_m, qkv_c, bias, scale, keep, d_m, d_c, B, H, N, slab0=None, p_hook=None, delta_hook=None):
    """The two-stream core in fp32, another summation order, bf16 at the cited points; the backward is given the emulated forward's
    own out_m, out_c, lse.  -> dict of buffers shaped like the Vals of ws_fwd / ws_bwd"""
    q, k, v = (t.to(F32) for t in split(qkv_m, B, H, N, 64))
    cq, ck, cv = (t.to(F32) for t in split(qkv_c, B, H, N, 64))
    T = lambda t: t.transpose(-1, -2)      # noqa: E731
    m1, m2, c1, c2 = torch.sigmoid(q * torch.tensor(scale32(scale))), torch.sigmoid(k), torch.sigmoid(cq), torch.sigmoid(ck)
    Am, Bm, Ac, Bc = _r16(m1), _r16(m2), _r16(c1.sqrt()), _r16(c2.sqrt())
    dot = _mm32(Am, T(Bm)) + _mm32(Ac, T(Bc))
    ri, cj = (m1 * m1 + c1).flip(-1).sum(-1, keepdim=True), T((m2 * m2 + c2).flip(-1).sum(-1, keepdim=True))
    sg = torch.sigmoid(2 * dot - ri - cj)
    x = sg * LOG2E + ((bias.to(F32) * LOG2E)[None] if bias is not None else 0.0)
    mx = x.amax(-1, keepdim=True)
    p = torch.exp2(x - mx)
    s = p.flip(-1).sum(-1, keepdim=True)
    lse = (mx + torch.log2(s)).squeeze(-1)
    K = _keep(keep, x)
    pa = p * (1.0 / s) * K
    if p_hook is not None:
        pa = p_hook(pa)
    out_m, out_c = _mm32(_r16(pa), v).to(BF16), _mm32(_r16(pa * pa), cv).to(BF16)
    dm, dc = heads(d_m, B, H, N, 64).to(F32), heads(d_c, B, H, N, 64).to(F32)
    dl = (dm * out_m.float() + 2 * dc * out_c.float()).flip(-1).sum(-1)
    if delta_hook is not None:
        dl = delta_hook(dl)
    pb = torch.exp2(x - lse[..., None])
    if p_hook is not None:
        pb = p_hook(pb)
    pd = pb * K
    ds = pb * (K * (_mm32(dm, T(v)) + 2 * pd * _mm32(dc, T(cv))) - dl[..., None])
    gv = -ds * sg * (1 - sg)
    gw = _r16(gv)
    side_q, side_k = gv.flip(-1).sum(-1, keepdim=True), T(gw.flip(-2).sum(-2, keepdim=True))
    bm = lambda a, sd, m, pre: ((-2 * a + 2 * m * sd) * m * (1 - m) * pre).to(BF16)                          # noqa: E731
    bc = lambda a, sd, c, y: ((-a * c.rsqrt() + sd) * c * (1 - c) * y.clamp(max=1.0)).to(BF16)               # noqa: E731
    db = _r16(ds).flip(0).sum(0)
    return dict(out_m=out_m, out_c=out_c, lse=lse, delta=dl, dq_m=bm(_mm32(gw, Bm), side_q, m1, scale32(scale)),
                dk_m=bm(_mm32(T(gw), Am), side_k, m2, 1.0), dq_c=bc(_mm32(gw, Bc), side_q, c1, cq), dk_c=bc(_mm32(T(gw), Ac), side_k, c2, ck),
                dv_m=_mm32(T(_r16(pd)), dm).to(BF16), dv_c=(_mm32(T(_r16(pd * pd)), dc) * cv.clamp(max=1.0)).to(BF16),
                dbias=db if slab0 is None else slab0.to(F32) + db)


WS_OUTPUTS = ("delta", "dq_m", "dk_m", "dv_m", "dq_c", "dk_c", "dv_c")


# ---- inputs of the bound tests ---------------------------------------------------------------------------------------------------
def _rnd(*shape, scale=1.0, seed=0):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed)) * scale


def regime_inputs(regime, B, H, N, hd, seed=30):
    """qkv (bf16), bias (fp32, natural units), d_o (bf16), on the CPU.  flat: the N(0, 1) inputs of test_attention_fwd / bwd (seeds 30, 31,
    32; bias scale 0.5, d_o scale 0.5).  peaked: q and k scaled by 3, bias scale 2, two V channels offset by +8, one d_o row scaled by 16
    (what a trained ViT looks like: median row maximum of P about 0.85).  peaked_tail (hd 80): the q / k energy in dims 64..79."""
    Cd = H * hd
    qkv = _rnd(B * N, 3 * Cd, seed=seed)
    d_o = _rnd(B * N, Cd, scale=0.5, seed=seed + 2)
    if regime == "flat":
        bias = _rnd(H, N, N, scale=0.5, seed=seed + 1)
    else:
        assert regime in ("peaked", "peaked_tail")
        bias = _rnd(H, N, N, scale=2.0, seed=seed + 1)
        t = qkv.view(B * N, 3, H, hd)
        if regime == "peaked":
            t[:, :2] *= 3
        else:
            assert hd == 80
            t[:, :2, :, :64] *= 0.25
            t[:, :2, :, 64:] *= 6          # 16 dims carry what 80 carried at scale 3: 16 * 36 ~ 80 * 9
        t[:, 2, :, 5] += 8
        t[:, 2, :, hd - 3] += 8
        d_o.view(B, N, Cd)[:, N // 2] *= 16
    return qkv.to(BF16).contiguous(), bias, d_o.to(BF16).contiguous()


# ---- exact cases -----------------------------------------------------------------------------------------------------------------
PERMS = ("identity", "reversal", "last", "random")


def perms(N, seed=0):
    """(4, N) int64: pi_h(q) per head -- identity, reversal, everything on key N - 1, a seeded random permutation"""
    r = torch.arange(N)
    return torch.stack([r, r.flip(0), torch.full((N,), N - 1), torch.randperm(N, generator=torch.Generator().manual_seed(seed))])


def _ints(*shape, lo=-4, hi=4, seed=0):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F32)


def grid_v(*shape, seed=0):
    """A bf16-exact grid without zero: +-(1 + j / 8) 2^e, j = 0..7, e = -1, 0, 1"""
    g = torch.Generator().manual_seed(seed)
    j, e = torch.randint(0, 8, shape, generator=g), torch.randint(-1, 2, shape, generator=g)
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return sgn * (1 + j / 8.0) * torch.exp2(e.to(F32))


def bias_selected(B, N, hd, seed=0):
    """H = 4 heads, one permutation each.  The bias is 0 at k = pi_h(q) and -1e4 elsewhere, so P is one-hot exactly (2^-14427 is 0 in
    fp32, and in fp64); q, k, v are random, d_o small integers (so that the fp32 sum of the N rows that land on key N - 1 is exact).
    -> qkv, bias, d_o, pi, and the expected out (B, H, N, hd) = V[pi] and dv = sum_{q: pi(q) = k} dO[q], both bf16-exact."""
    H = len(PERMS)
    pi = perms(N, seed)
    qkv = _rnd(B * N, 3 * H * hd, seed=seed + 1).to(BF16)
    d_o = _ints(B * N, H * hd, seed=seed + 2).to(BF16)
    bias = torch.full((H, N, N), -1e4)
    bias.scatter_(2, pi[:, :, None], 0.0)
    return dict(qkv=qkv, bias=bias, d_o=d_o, pi=pi, **selected_expect(qkv, d_o, pi, B, N, hd))


def selected_expect(qkv, d_o, pi, B, N, hd):
    H = pi.shape[0]
    v = split(qkv, B, H, N, hd)[2].to(F64)
    do = heads(d_o, B, H, N, hd).to(F64)
    idx = pi[None, :, :, None].expand(B, H, N, hd)
    out = torch.gather(v, 2, idx)
    dv = torch.zeros_like(v).scatter_add_(2, idx, do).to(BF16).to(F64)         # the kernel rounds the (exact) fp32 sum once, RNE
    return dict(out=out, dv=dv)


def two_stream_selected(B, N, seed=0):
    """The bias-selected permutation for the two-stream core (head dim 64): qkv_c is ELU(.) + 1 of random values, d_m and d_c small
    integers.  With P one-hot, PD = PD^2 = 1 on the selected key: out_m = V_m[pi], out_c = V_c[pi], dV_m = sum_{q: pi(q) = k} dM[q] and the
    pre-ELU gradient dV_c = (sum dC[q]) min(cv, 1) (ELU' folded in, attention2.hip:586; the fp32 product of an integer below 2^10 and a
    bf16 is exact, so it is rounded once); delta = rowsum(dM o o_m) + 2 rowsum(dC o o_c), bound (2 hd + 8) u sum |terms| (:415)."""
    c = bias_selected(B, N, 64, seed)
    H = len(PERMS)
    qkv_c = (torch.nn.functional.elu(_rnd(B * N, 3 * H * 64, seed=seed + 8)) + 1).to(BF16)
    d_c = _ints(B * N, H * 64, seed=seed + 9).to(BF16)
    ec = selected_expect(qkv_c, d_c, c["pi"], B, N, 64)
    cv = split(qkv_c, B, H, N, 64)[2].to(F64)
    dv_c = (ec["dv"] * cv.clamp(max=1.0)).to(BF16).to(F64)
    dm, dc = heads(c["d_o"], B, H, N, 64).to(F64), heads(d_c, B, H, N, 64).to(F64)
    delta = (dm * c["out"]).sum(-1) + 2 * (dc * ec["out"]).sum(-1)
    b_delta = (2 * 64 + 8) * U * ((dm * c["out"]).abs().sum(-1) + 2 * (dc * ec["out"]).abs().sum(-1))
    return dict(qkv_m=c["qkv"], qkv_c=qkv_c, bias=c["bias"], d_m=c["d_o"], d_c=d_c, pi=c["pi"], out_m=c["out"], out_c=ec["out"],
                dv_m=c["dv"], dv_c=dv_c, delta=Val(delta, b_delta, "bhq"))


def score_selected(B, N, hd, seed=0, tail_only=False):
    """H = 4 heads, one permutation each.  k rows are +-1 codes, q = A x the code of pi(q), v sits on grid_v, d_o small integers.  The peak
    score exceeds every other by A c times the gap between hd and the largest off-diagonal code dot; A (16; 256 for the codes that live in
    dims 64..79 only, where distinct codes differ by at least 2) is chosen so that the off-peak mass of the float64 reference is below
    2^-40 (the host test asserts it): an fp32 product sum then returns V[pi] bit for bit."""
    H = len(PERMS)
    pi = perms(N, seed)
    g = torch.Generator().manual_seed(seed + 5)
    if tail_only:
        assert hd == 80
        codes = torch.zeros(B, H, N, hd)
        for b in range(B):
            for h in range(H):
                w = torch.randperm(1 << 16, generator=g)[:N]                     # distinct 16-bit words
                codes[b, h, :, 64:] = ((w[:, None] >> torch.arange(16)[None]) & 1).to(F32) * 2 - 1
        A = 256.0
    else:
        codes = torch.randint(0, 2, (B, H, N, hd), generator=g).to(F32) * 2 - 1
        A = 16.0
    q = A * torch.gather(codes, 2, pi[None, :, :, None].expand(B, H, N, hd))
    qkv = join(q, codes, grid_v(B, H, N, hd, seed=seed + 6)).to(BF16)
    d_o = _ints(B * N, H * hd, seed=seed + 2).to(BF16)
    return dict(qkv=qkv, d_o=d_o, pi=pi, **selected_expect(qkv, d_o, pi, B, N, hd))


def off_peak_mass(P, pi):
    """The largest per-row probability mass outside k = pi_h(q), and whether every row peaks there"""
    B, H, N, _ = P.shape
    idx = pi[None, :, :, None].expand(B, H, N, 1).to(P.device)
    peak = torch.gather(P, 3, idx)
    return (P.sum(-1, keepdim=True) - peak).abs().max().item(), bool((P.argmax(-1, keepdim=True) == idx).all())


# ---- uniform read-out of the dropout mask -----------------------------------------------------------------------------------------
def readout_chunks(N, hd):
    return (N + hd - 1) // hd


def readout_onehot(B, H, N, hd, chunk):
    """(B, H, N, hd): row r is one-hot in d = r - hd chunk (zero outside the chunk)"""
    t = torch.zeros(B, H, N, hd)
    r = torch.arange(hd * chunk, min(N, hd * (chunk + 1)))
    t[:, :, r, r - hd * chunk] = 1.0
    return t


def readout_qkv(B, H, N, hd, chunk):
    """q = k = 0 (every un-normalised p is exactly 1), V one-hot in d = k - hd chunk: out[q, d] = Pd[q, hd chunk + d]"""
    z = torch.zeros(B, H, N, hd)
    return join(z, z, readout_onehot(B, H, N, hd, chunk)).to(BF16)


def readout_decode(rows, N, hd, p_drop):
    """rows: per chunk a (B, H, N, hd) tensor whose [.., r, d] holds Pd[r, hd chunk + d] (forward: out; transposed use for the backward).
    -> (keep bits (B, H, N, N) bool, the largest distance of an element from {0, bf16(inv_keep / N)} in bf16 ulps of the latter)"""
    full = torch.cat([t.to(F64) for t in rows], -1)[..., :N]
    one = float(np.float32(1.0) / np.float32(1.0 - p_drop)) / N if p_drop > 0 else 1.0 / N
    one16 = torch.tensor(one, dtype=F64).to(BF16).to(F64).item()
    ulp = 2.0 ** (math.floor(math.log2(one16)) - 7)
    bitsK = full > 0.5 * one
    off = torch.where(bitsK, (full - one16).abs(), full.abs()).max().item() / ulp
    return bitsK, off


def keep_bits(seed, layer, B, H, N, p_drop):
    from oracle.vit_oracle import attn_keep_mask
    return attn_keep_mask(seed, layer, B, H, N, p_drop) != 0


# ---- today's criteria, restated (tests/test_gpu_ops.py: test_attention_fwd / test_attention_bwd) -----------------------------------
def todays_criteria_reject(name, got, ref):
    """True when the existing assertions on `name` ('out': rtol 2e-2, atol 1e-2; 'dq' / 'dk' / 'dv': rtol 3e-2, atol 2e-2 max |dqkv| and a
    relative L2 of the whole part below 1e-2) would reject got.  ref: dict of the float64 references (dq, dk, dv all needed for max |dqkv|)."""
    r, g = ref[name], got
    err = (g - r).abs()
    if name == "out":
        return bool((err > 1e-2 + 2e-2 * r.abs()).any())
    big = max(ref[n].abs().max().item() for n in ("dq", "dk", "dv"))
    return bool((err > 2e-2 * big + 3e-2 * r.abs()).any()) or ((g - r).norm() / r.norm()).item() >= 1e-2
