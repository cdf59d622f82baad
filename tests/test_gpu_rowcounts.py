"""GPU: the operators of the step over the row counts a training run produces.

With the drop-path sample lists and the masked-row last block the row count of almost every launch changes from step to
step: a Block branch runs on k x 197 compact rows (k = the samples its DropPath kept), the last block's MLP on a multiple of
64 rows.  uvit_gemm_nt_launch picks its kernel, its tile height, the persistent form and the row split from M; the wgrads
reduce over roundup(rows, 64) and the grouped launcher re-plans its chunks from M / 64.  Here every such M is launched.

Rows of a GEMM are independent, so each launch shape has ONE set of bf16 operands at the largest M and ONE float64 reference
(on the device); the launch at a smaller M is compared with the first M rows of it.  Every output buffer is allocated for the
largest M plus SLACK rows and holds a sentinel bit pattern before each launch: afterwards no element of rows [0, M) may still
be the sentinel and every row from M on must be the sentinel bit for bit (a row tile that stores past M).

Measured on an MI355X (256 CUs): the file takes 19 s (2,803 NT launches in 3 s; the rest is references and start-up).  M per
shape / of them split / kernels reached by the rule (128x128, 256-row, 256-row persistent, 320-row):
  ViT-B  qkv 156 / 13 / 7 35 79 35    proj 136 / 0 / 7 109 0 20    fc1 391 / 20 / 15 93 194 89   fc2 367 / 0 / 15 332 0 20
         dgrad_fc2 164 / 20 / 7 128 0 29    dgrad_fc1 136 / 0 / 7 109 0 20
  ViT-L  qkv 80 / 0 / 7 26 24 23      proj, fc2, dgrad_fc1 68 / 0 / 7 61 0 0    fc1 87 / 4 / 7 19 38 23    dgrad_fc2 87 / 4 / 7 57 0 23
  ViT-H  qkv 172 / 27 / 7 21 120 24   proj, fc2, dgrad_fc1 146 / 5 / 7 70 48 21    fc1 193 / 37 / 7 19 138 29    dgrad_fc2 192 / 37 / 7 156 0 29
(the residual launches never split at ViT-B, where the 320-row tiles win wherever a round would overflow, nor at ViT-L, whose tiles never
fill a round: the row offset of a split residual launch is checked at ViT-H's N = 1280)."""
import ctypes as C
import math
import time

import pytest
import torch

from gpu_util import BF16, GELU_DG, MODELS, MULAUX, QKV, RESID, TOKENS, launches, nt_auto_plan, nt_boundary_rows  # noqa: F401
from test_gpu_ops import LOG2E, L, P, S, bf, close, epi, nt, ok, padded_bias, rnd, rows_rel, tn  # noqa: F401  (L is a fixture)

pytestmark = pytest.mark.gpu

SLACK = 320                                      # rows behind the largest M: one row tile of the tallest kernel
SENT16, SENT32 = 0x7B7B, 0x7B7B7B7B              # bf16 / fp32 1.3e36: finite, and no result of these operands


def sentinel(rows, cols, dtype):
    t = torch.empty(rows, cols, dtype=dtype, device="cuda")
    bits = t.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
    return t, bits, (SENT16 if dtype == torch.bfloat16 else SENT32)


def gelu64(h):
    """gelu(h) and gelu'(h) (the erf form of nn.GELU) in float64."""
    cdf = 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return h * cdf, cdf + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


class NtCase:
    """Operands, epilogue and float64 references of one launch shape at m_max rows; run(M) launches the first M rows."""

    def __init__(self, L, N, K, mode, m_max):
        self.L, self.N, self.K, self.mode, self.m_max = L, N, K, mode, m_max
        rows = m_max + SLACK
        self.a, self.w = bf(rnd(m_max, K, seed=1)), bf(rnd(N, K, scale=0.05, seed=2))
        y = self.a.double() @ self.w.double().t()
        kw = dict(ldo=N)
        if mode == QKV:                          # bias = cat(q_bias, 0, v_bias)
            Cd = N // 3
            self.qb, self.vb = rnd(Cd, seed=6), rnd(Cd, seed=7)
            kw.update(bias=self.qb, bias2=self.vb)
            refs = [("qkv", torch.bfloat16, y + torch.cat([self.qb, torch.zeros_like(self.vb), self.vb]).double(), 2e-2, 2e-2)]
        elif mode == GELU_DG:                    # out = gelu(h), out2 = gelu'(h), h = a W^T + b
            self.b = rnd(N, seed=9)
            kw.update(bias=self.b)
            g, dg = gelu64(y + self.b.double())
            refs = [("gelu", torch.bfloat16, g, 2e-2, 2e-2), ("gelu'", torch.bfloat16, dg, 2e-2, 2e-2)]
        elif mode == RESID:                      # out = resid + dp[sample] * gamma * (a W^T + b), out2 = a W^T + b
            nb = (rows + TOKENS - 1) // TOKENS
            self.b, self.gam, self.res = rnd(N, seed=3), rnd(N, scale=0.1, seed=4), rnd(rows, N, seed=5)
            self.dp = 0.25 + 1.5 * torch.arange(nb, device="cuda").float() / nb          # another scale for every sample
            kw.update(bias=self.b, gamma=self.gam, resid=self.res, rowscale=self.dp, tokens=TOKENS)
            y = y + self.b.double()
            scale = self.dp.double().repeat_interleave(TOKENS)[:m_max, None] * self.gam.double()
            refs = [("resid out", torch.float32, self.res[:m_max].double() + scale * y, 5e-3, 5e-3),
                    ("resid branch", torch.bfloat16, y, 2e-2, 2e-2)]
        elif mode == MULAUX:                     # out = (dY W) * aux, aux = the stored gelu'(h)
            self.aux = bf(rnd(rows, N, scale=0.5, seed=8) + 0.5)
            kw.update(aux=self.aux)
            refs = [("mul-aux", torch.bfloat16, y * self.aux[:m_max].double(), 2e-2, 2e-2)]
        else:                                    # BF16 without a bias: the fc1 dgrad
            refs = [("bf16", torch.bfloat16, y, 2e-2, 2e-2)]
        self.outs = []                           # (name, tensor, bit view, sentinel, float64 reference, rtol, atol)
        for name, dtype, ref, rtol, atol in refs:
            t, bits, sent = sentinel(rows, N, dtype)
            self.outs.append((name, t, bits, sent, ref, rtol, atol))
        kw["out"] = self.outs[0][1]
        if len(self.outs) > 1:
            kw["out2"] = self.outs[1][1]
        self.epi = epi(**kw)

    def run(self, M):
        for _, _, bits, sent, _, _, _ in self.outs:
            bits.fill_(sent)
        tail = C.c_int(-1)
        ok(nt(self.L, self.mode, P(self.a), P(self.w), M, self.N, self.K, self.K, self.K, C.byref(self.epi), S(), tail=tail))
        for name, t, bits, sent, ref, rtol, atol in self.outs:
            what = f"{name} at M={M} (N={self.N} K={self.K}, tail {tail.value})"
            past = bits[M:] != sent
            assert not bool(past.any()), f"{what}: {int(past.sum())} elements stored past row M, first in row {M + int(past.any(1).nonzero()[0])}"
            left = bits[:M] == sent
            assert not bool(left.any()), f"{what}: {int(left.sum())} elements of rows [0, M) not written, first in row {int(left.any(1).nonzero()[0])}"
            close(t[:M], ref[:M], rtol=rtol, atol=atol, what=what)
        return tail.value


def sweep_rows(model, name):
    """The M of one launch shape: every k x 197, the dispatch boundaries (256 CUs), and for ViT-B's fc1 / fc2 the masked-row block's
    multiples of 64."""
    N, K, mode = launches(model)[name]
    kmax = MODELS[model][2]
    ms = {k * TOKENS for k in range(1, kmax + 1)}
    bnd = nt_boundary_rows(N, K, mode, kmax * TOKENS)
    ms.update(bnd)
    if model == "vitb" and name in ("fc1", "fc2"):
        ms.update(range(512, 15360 + 1, 64))
    return sorted(ms), bnd


@pytest.mark.parametrize("name", ["qkv", "proj", "fc1", "fc2", "dgrad_fc2", "dgrad_fc1"])
@pytest.mark.parametrize("model", list(MODELS))
def test_gemm_nt_over_run_row_counts(L, model, name):
    """Auto dispatch (nt_variant 3, what the engine uses) of one forward / dgrad launch shape of ViT-B, ViT-L or ViT-H at every M of
    sweep_rows.  The residual launches carry a per-sample drop-path scale that differs for every sample, so that a wrong row offset
    of the split-off tail launch shows; tail_rows_out must be what the dispatch rule (tests/gpu_util.py::nt_auto_plan, restated
    from the comments of uvit_gemm_nt_launch) gives for this device's CU count, and what uvit_op_gemm_nt_plan reports for it; a shape
    that can split must have run both ways."""
    from uncertainty_vit_amd.native import GemmNtPlanInfo, Tuning
    N, K, mode = launches(model)[name]
    ms, bnd = sweep_rows(model, name)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    persist = bool(Tuning.default().nt_persist)
    info = GemmNtPlanInfo()
    case = NtCase(L, N, K, mode, ms[-1])
    torch.cuda.synchronize()
    t0 = time.time()
    kernels, split = {}, 0
    for M in ms:
        kern, want_tail = nt_auto_plan(M, N, K, mode, cu, persist)
        got_tail = case.run(M)
        assert got_tail == want_tail, f"M={M}: tail_rows_out {got_tail}, the dispatch rule gives {want_tail}"
        ok(L.uvit_op_gemm_nt_plan(mode, M, N, K, K, K, N, 0, None, cu, C.byref(info)))
        assert info.tail_rows == got_tail, f"M={M}: tail_rows_out {got_tail}, uvit_op_gemm_nt_plan at {cu} CUs reports {info.tail_rows}"
        kernels[kern] = kernels.get(kern, 0) + 1
        split += got_tail > 0
    torch.cuda.synchronize()
    print(f"\n[{model} {name} N={N} K={K} mode={mode}] {len(ms)} M ({len(bnd)} at dispatch boundaries), {split} split, kernels by the rule "
          f"{dict(sorted(kernels.items()))}, {time.time() - t0:.1f} s")
    if any(nt_auto_plan(M, N, K, mode, cu, persist)[1] > 0 for M in range(1024, ms[-1] + 1)):
        assert 0 < split < len(ms), "a shape that can split must have run split and unsplit launches"


def wgrad_ks(model):
    kmax = MODELS[model][2]
    return list(range(1, kmax + 1)) if model == "vitb" else sorted(set(range(1, kmax + 1, 4)) | {kmax})


@pytest.mark.parametrize("model", list(MODELS))
def test_wgrad_over_run_row_counts(L, model):
    """uvit_op_gemm_tn (per Linear) and uvit_op_wgrad_group (one launch for the layer's four Linears, bias sums fused) at the reduction
    lengths roundup(k x 197, 64) of a Block branch that kept k samples: operands whose rows from k x 197 on are zero (the engine's
    contract), outputs zero before the launch (the engine zeroes the gradient arena once per step), against the float64
    y[:k x 197]^T x[:k x 197].  k = 1..128 for ViT-B; for ViT-L (k <= 64) and ViT-H (k <= 128) every 4th k from 1 plus the largest.
    The sweep runs k downwards and zeroes the rows it leaves, and takes their product off the float64 reference, so there is one
    reference GEMM per Linear.  Bounds: those of test_wgrad_group_production_layer.  Below 512 reduction rows (k = 1, 2) the grouped
    launcher refuses the group, as the engine expects (it then launches Linear by Linear)."""
    from uncertainty_vit_amd.native import WgradProblem
    Cd, Hd, kmax = MODELS[model]
    specs = [(3 * Cd, Cd, "qkv"), (Cd, Cd, "full"), (Hd, Cd, "full"), (Cd, Hd, "full")]
    rows = (kmax * TOKENS + 63) // 64 * 64
    ops = []
    for i, (n, k, bias) in enumerate(specs):
        y, x = bf(rnd(rows, n, scale=0.1, seed=30 + i)), bf(rnd(rows, k, seed=40 + i))
        y[kmax * TOKENS:] = 0
        x[kmax * TOKENS:] = 0
        ops.append([y, x, y.double().t() @ x.double(), y.double().sum(0)])
    ks = wgrad_ks(model)
    t0, prev, grouped = time.time(), kmax, 0
    for kk in reversed(ks):
        m = kk * TOKENS
        red = (m + 63) // 64 * 64
        if prev > kk:                                # leave samples kk .. prev - 1
            for o in ops:
                yd, xd = o[0][m:prev * TOKENS].double(), o[1][m:prev * TOKENS].double()
                o[2] -= yd.t() @ xd
                o[3] -= yd.sum(0)
                o[0][m:prev * TOKENS] = 0
                o[1][m:prev * TOKENS] = 0
        prev = kk
        probs = (WgradProblem * len(specs))()
        keep = []
        for i, ((n, k, bias), (y, x, ref, colsum)) in enumerate(zip(specs, ops)):
            out_tn = torch.zeros(n, k, device="cuda")
            ok(tn(L, P(y), P(x), red, n, k, n, k, P(out_tn), k, S()))
            out = torch.zeros(n, k, device="cuda")
            b1 = torch.zeros(n if bias == "full" else Cd, device="cuda")
            b2 = torch.zeros(Cd, device="cuda") if bias == "qkv" else None
            keep.append((out_tn, out, b1, b2))
            q = probs[i]
            q.Y, q.X, q.C = y.data_ptr(), x.data_ptr(), out.data_ptr()
            q.bias, q.bias2 = b1.data_ptr(), (b2.data_ptr() if b2 is not None else None)
            q.bias_end, q.bias2_begin = (n if bias == "full" else Cd), 2 * Cd
            q.M, q.N, q.K, q.ldy, q.ldx, q.ldc = red, n, k, n, k, k
        rc = L.uvit_op_wgrad_group(probs, len(specs), None, S())
        if red < 512:
            assert rc == -2, f"k={kk}: a group with {red} reduction rows must be refused, got {rc}"
        else:
            ok(rc)
            grouped += 1
        for (n, k, bias), (y, x, ref, colsum), (out_tn, out, b1, b2) in zip(specs, ops, keep):
            for kind, got in (("wgrad", out_tn),) + ((("grouped wgrad", out),) if rc == 0 else ()):
                what = f"{kind} {n}x{k} at k={kk} ({m} rows, reduction {red})"
                close(got, ref, rtol=2e-3, atol=2e-3 * math.sqrt(red / 64), what=what)
                r = rows_rel(got, ref)
                assert float(r.max()) < 1e-3, (what, int(r.argmax()), float(r.max()))
            if rc == 0:
                if bias == "full":
                    close(b1, colsum, rtol=2e-3, atol=2e-2, what=f"bias sums {n} at k={kk}")
                else:
                    close(b1, colsum[:Cd], rtol=2e-3, atol=2e-2, what=f"q bias sums at k={kk}")
                    close(b2, colsum[2 * Cd:], rtol=2e-3, atol=2e-2, what=f"v bias sums at k={kk}")
    torch.cuda.synchronize()
    print(f"\n[{model} wgrad] {len(ks)} k, {grouped} grouped launches, {time.time() - t0:.1f} s")


def attn_ref64(qkv, bias, B, H, N, hd, keep):
    q, k, v = qkv.view(B, N, 3, H, hd).double().permute(2, 0, 3, 1, 4)
    s = (q * hd ** -0.5) @ k.transpose(-2, -1) + bias
    lse = torch.logsumexp(s, -1)
    a = s.softmax(-1) * keep.double()
    return (a @ v).transpose(1, 2).reshape(B, N, H * hd), lse


@pytest.mark.parametrize("hd,H", [(64, 12), (80, 16)])
def test_attention_on_the_first_k_samples(L, hd, H):
    """A Block branch that kept K of 128 samples launches the attention forward and backward on K samples of buffers sized for 128:
    K = 1, 85, 127 at N = 197, head_dim 64 (ViT-B) and 80 (ViT-H), with the bias and dropout.  out, lse, delta and dqkv of the first
    K samples against float64 (the bounds of test_attention_fwd_bwd_production_batch), the bias gradient against the sum over those K
    samples, and everything of the samples past K still the sentinel."""
    from oracle.vit_oracle import attn_keep_mask
    B, N, Cd, p_drop, seed, layer = 128, TOKENS, H * hd, 0.05, 2468, 7
    scale = hd ** -0.5
    qkv = bf(rnd(B * N, 3 * Cd, seed=30))
    bias = rnd(H, N, N, scale=0.5, seed=31)
    biasP = padded_bias(bias)
    d_o = bf(rnd(B * N, Cd, scale=0.5, seed=32))
    keep = attn_keep_mask(seed, layer, B, H, N, p_drop)
    ref_out, ref_lse, ref_dq, ref_db = [], [], [], []
    for b0 in range(0, B, 16):                      # float64 reference, 16 samples at a time; the bias gradient per sample
        qf = qkv.view(B, N, 3 * Cd)[b0:b0 + 16].double().requires_grad_(True)
        bq = bias.double().unsqueeze(0).repeat(16, 1, 1, 1).requires_grad_(True)
        o, l_ = attn_ref64(qf, bq, 16, H, N, hd, keep[b0:b0 + 16].cuda())
        o.backward(d_o.view(B, N, Cd)[b0:b0 + 16].double())
        ref_out.append(o.detach()); ref_lse.append(l_.detach()); ref_dq.append(qf.grad); ref_db.append(bq.grad)
        del qf, bq, o, l_
    ref_out, ref_lse, ref_dq, ref_db = torch.cat(ref_out), torch.cat(ref_lse), torch.cat(ref_dq), torch.cat(ref_db)
    out, out_b, s16 = sentinel(B * N, Cd, torch.bfloat16)
    dqkv, dqkv_b, _ = sentinel(B * N, 3 * Cd, torch.bfloat16)
    lse, lse_b, s32 = sentinel(B * H, N, torch.float32)
    delta, delta_b, _ = sentinel(B * H, N, torch.float32)
    heads = lambda t, parts: t.reshape(-1, N, parts, H, hd).permute(0, 2, 3, 1, 4).reshape(-1, N * hd)        # noqa: E731
    for K in (1, 85, 127):
        for bits, sent in ((out_b, s16), (dqkv_b, s16), (lse_b, s32), (delta_b, s32)):
            bits.fill_(sent)
        ws = torch.empty(L.uvit_op_attn_bwd_ws_bytes(K, H, N), dtype=torch.uint8, device="cuda")
        slab = torch.zeros(H, 208, 208, device="cuda")
        ok(L.uvit_op_attn_fwd_hd(P(qkv), P(biasP), P(out), P(lse), K, H, N, 208, hd, C.c_float(scale), C.c_float(p_drop), seed, layer, S()))
        ok(L.uvit_op_attn_bwd_hd(P(qkv), P(out), P(d_o), P(biasP), P(lse), P(delta), P(dqkv), P(slab), 0, P(ws), K, H, N, 208, hd,
                                 C.c_float(scale), C.c_float(p_drop), seed, layer, S()))
        torch.cuda.synchronize()
        for name, bits, sent, r in (("out", out_b, s16, K * N), ("dqkv", dqkv_b, s16, K * N), ("lse", lse_b, s32, K * H), ("delta", delta_b, s32, K * H)):
            assert not bool((bits[r:] != sent).any()), f"{name}: the K={K} launch wrote past sample K"
            assert not bool((bits[:r] == sent).any()), f"{name}: the K={K} launch left elements of the first K samples unwritten"
        e_out = rows_rel(heads(out[:K * N], 1), heads(ref_out[:K], 1))
        e_dq = rows_rel(heads(dqkv[:K * N], 3), heads(ref_dq[:K], 3))
        e_lse = (lse[:K * H].double() - ref_lse[:K].reshape(K * H, N) * LOG2E).abs().amax(-1)
        print(f"\nhd{hd} K={K}: worst (b, h) out {float(e_out.max()):.2e}, lse {float(e_lse.max()):.2e}, dqkv {float(e_dq.max()):.2e}")
        assert float(e_out.max()) < 2e-2, divmod(int(e_out.argmax()), H)
        assert float(e_lse.max()) < 3e-3 + 1e-3 * float(lse[:K * H].abs().max())
        assert float(e_dq.max()) < 2e-2, int(e_dq.argmax())
        dref = (d_o[:K * N].double() * out[:K * N].double()).view(K, N, H, hd).sum(-1).transpose(1, 2).reshape(K * H, N)
        torch.testing.assert_close(delta[:K * H].double(), dref, rtol=1e-3, atol=1e-3)
        rel = rows_rel(slab[:, :N, :N].transpose(1, 2).reshape(H, -1), ref_db[:K].sum(0).reshape(H, -1))
        assert float(rel.max()) < 1e-2, (K, int(rel.argmax()), float(rel.max()))
        assert slab[:, N:, :].abs().sum() == 0 and slab[:, :, N:].abs().sum() == 0
