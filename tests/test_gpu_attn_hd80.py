"""GPU: the head_dim-80 attention kernels (ViT-H/16: 16 heads of 80) through uvit_op_attn_fwd_hd / uvit_op_attn_bwd_hd, against
autograd of the reference attention (modeling_finetune.py:152-185) in float64 on the device, with the kernels' dropout replayed
(oracle.vit_oracle.attn_keep_mask, which does not depend on the head dim)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_ops import LOG2E, L, P, S, bf, ok, padded_bias, rnd, rows_rel  # noqa: F401  (L is a fixture)

pytestmark = pytest.mark.gpu
HD = 80
SCALE = HD ** -0.5


def attn_ref64(qkv, bias, B, H, N, keep=None):
    """float64: out (B, N, H * 80), lse (natural log)."""
    q, k, v = qkv.view(B, N, 3, H, HD).double().permute(2, 0, 3, 1, 4)
    s = (q * SCALE) @ k.transpose(-2, -1)
    if bias is not None:
        s = s + bias
    a = s.softmax(-1)
    lse = torch.logsumexp(s, -1)
    if keep is not None:
        a = a * keep.double()
    return (a @ v).transpose(1, 2).reshape(B, N, H * HD), lse


def run_case(L, B, H, N, with_bias, p_drop, chunk=16):
    from oracle.vit_oracle import attn_keep_mask
    Cd = H * HD
    seed, layer = 97531, 9
    qkv = bf(rnd(B * N, 3 * Cd, seed=60))
    bias = rnd(H, N, N, scale=0.5, seed=61)
    biasP = padded_bias(bias) if with_bias else None
    keep = attn_keep_mask(seed, layer, B, H, N, p_drop) if p_drop > 0 else None
    out = torch.zeros(B * N, Cd, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(B, H, N, device="cuda")
    ok(L.uvit_op_attn_fwd_hd(P(qkv), P(biasP), P(out), P(lse), B, H, N, 208, HD, C.c_float(SCALE), C.c_float(p_drop), seed, layer, S()))
    d_o = bf(rnd(B * N, Cd, scale=0.5, seed=62))
    delta = torch.zeros(B, H, N, device="cuda")
    dqkv = torch.full((B * N, 3 * Cd), 7.0, dtype=torch.bfloat16, device="cuda")        # every element must be overwritten
    ws = torch.empty(L.uvit_op_attn_bwd_ws_bytes(B, H, N), dtype=torch.uint8, device="cuda")
    slab = torch.full((H, 208, 208), 3.0, device="cuda")
    args = lambda acc, sl: (P(qkv), P(out), P(d_o), P(biasP), P(lse), P(delta), P(dqkv), P(sl), acc, P(ws if sl is not None else None),  # noqa: E731
                            B, H, N, 208, HD, C.c_float(SCALE), C.c_float(p_drop), seed, layer, S())
    ok(L.uvit_op_attn_bwd_hd(*args(0, slab if with_bias else None)))
    torch.cuda.synchronize()
    bq = bias.double().requires_grad_(True) if with_bias else None
    e_out, e_lse, e_dq = [], [], []
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        qf = qkv.view(B, N, 3 * Cd)[b0:b1].double().requires_grad_(True)
        o, l_ = attn_ref64(qf, bq, b1 - b0, H, N, None if keep is None else keep[b0:b1].cuda())
        o.backward(d_o.view(B, N, Cd)[b0:b1].double())
        e_out.append(rows_rel(out.view(B, N, H, HD)[b0:b1].permute(0, 2, 1, 3).reshape((b1 - b0) * H, -1),
                              o.detach().view(-1, N, H, HD).permute(0, 2, 1, 3).reshape((b1 - b0) * H, -1)))
        e_lse.append((lse[b0:b1].double() - l_.detach() * LOG2E).abs().amax(-1).view(-1))
        gq = dqkv.view(B, N, 3, H, HD)[b0:b1].permute(0, 2, 3, 1, 4).reshape((b1 - b0) * 3 * H, -1)
        rq = qf.grad.view(-1, N, 3, H, HD).permute(0, 2, 3, 1, 4).reshape((b1 - b0) * 3 * H, -1)
        e_dq.append(rows_rel(gq, rq))
        del qf, o, l_
    e_out, e_lse, e_dq = torch.cat(e_out), torch.cat(e_lse), torch.cat(e_dq)
    print(f"\nhd80 B={B} H={H} N={N} bias={with_bias} p={p_drop}: worst (b, h) out {float(e_out.max()):.2e}, lse {float(e_lse.max()):.2e}, "
          f"dqkv {float(e_dq.max()):.2e} at (b, part, h) {np.unravel_index(int(e_dq.argmax()), (B, 3, H))}")
    assert float(e_out.max()) < 2e-2, divmod(int(e_out.argmax()), H)
    assert float(e_lse.max()) < 3e-3 + 1e-3 * float(lse.abs().max())
    assert float(e_dq.max()) < 2e-2, np.unravel_index(int(e_dq.argmax()), (B, 3, H))
    dref = (d_o.double() * out.double()).view(B, N, H, HD).sum(-1).transpose(1, 2)
    torch.testing.assert_close(delta.double(), dref, rtol=1e-3, atol=1e-3)
    if with_bias:
        dbias = slab[:, :N, :N].transpose(1, 2).double()
        rel = rows_rel(dbias.reshape(H, -1), bq.grad.reshape(H, -1))
        print(f"  dbias (sum over {B} samples): worst head {int(rel.argmax())} relative L2 {float(rel.max()):.2e}")
        assert float(rel.max()) < 1e-2
        assert slab[:, N:, :].abs().sum() == 0 and slab[:, :, N:].abs().sum() == 0
        ok(L.uvit_op_attn_bwd_hd(*args(1, slab)))            # accumulate: adds on top
        rel2 = rows_rel(slab[:, :N, :N].transpose(1, 2).double().reshape(H, -1), 2 * bq.grad.reshape(H, -1))
        assert float(rel2.max()) < 1e-2


@pytest.mark.parametrize("N", [197, 50, 10])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("p_drop", [0.0, 0.05])
def test_attn_hd80_b2(L, N, with_bias, p_drop):
    """N = 197: the 13-tile kernels; N = 50, 10: the generic ones."""
    run_case(L, 2, 16, N, with_bias, p_drop)


@pytest.mark.parametrize("N,with_bias,p_drop", [(197, True, 0.05), (197, False, 0.0), (50, True, 0.05)])
def test_attn_hd80_b128(L, N, with_bias, p_drop):
    """The ViT-H/16 step's batch: every (sample, head) and the bias gradient summed over 128 samples."""
    run_case(L, 128, 16, N, with_bias, p_drop)


@pytest.mark.parametrize("N", [197, 50])
def test_hd_entry_points_at_64_equal_the_old_ones(L, N):
    B, H, Cd, p_drop, seed, layer = 3, 12, 768, 0.05, 11, 2
    qkv = bf(rnd(B * N, 3 * Cd, seed=70))
    biasP = padded_bias(rnd(H, N, N, scale=0.5, seed=71))
    d_o = bf(rnd(B * N, Cd, scale=0.5, seed=72))
    res = []
    for hd in (None, 64):
        out = torch.zeros(B * N, Cd, dtype=torch.bfloat16, device="cuda")
        lse = torch.zeros(B, H, N, device="cuda")
        delta = torch.zeros(B, H, N, device="cuda")
        dqkv = torch.zeros(B * N, 3 * Cd, dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(L.uvit_op_attn_bwd_ws_bytes(B, H, N), dtype=torch.uint8, device="cuda")
        slab = torch.zeros(H, 208, 208, device="cuda")
        if hd is None:
            ok(L.uvit_op_attn_fwd(P(qkv), P(biasP), P(out), P(lse), B, H, N, 208, C.c_float(0.125), C.c_float(p_drop), seed, layer, S()))
            ok(L.uvit_op_attn_bwd(P(qkv), P(out), P(d_o), P(biasP), P(lse), P(delta), P(dqkv), P(slab), 0, P(ws), B, H, N, 208,
                                  C.c_float(0.125), C.c_float(p_drop), seed, layer, S()))
        else:
            ok(L.uvit_op_attn_fwd_hd(P(qkv), P(biasP), P(out), P(lse), B, H, N, 208, hd, C.c_float(0.125), C.c_float(p_drop), seed, layer, S()))
            ok(L.uvit_op_attn_bwd_hd(P(qkv), P(out), P(d_o), P(biasP), P(lse), P(delta), P(dqkv), P(slab), 0, P(ws), B, H, N, 208, hd,
                                     C.c_float(0.125), C.c_float(p_drop), seed, layer, S()))
        torch.cuda.synchronize()
        res.append((out, lse, delta, dqkv, slab))
    for a, b in zip(res[0][:4], res[1][:4]):                # out, lse, delta, dqkv: the same kernels, bit for bit
        assert torch.equal(a, b)
    # the bias gradient is summed over the batch with fp32 atomics: equal up to the order of the additions
    torch.testing.assert_close(res[0][4], res[1][4], rtol=1e-5, atol=1e-6)


def test_hd_entry_points_reject_other_head_dims(L):
    t = torch.zeros(16, device="cuda")
    for hd in (48, 96, 0):
        assert L.uvit_op_attn_fwd_hd(P(t), P(None), P(t), P(t), 1, 1, 10, 208, hd, C.c_float(0.1), C.c_float(0.0), 1, 0, S()) == -2
        assert L.uvit_op_attn_bwd_hd(P(t), P(t), P(t), P(None), P(t), P(t), P(t), P(None), 0, P(None), 1, 1, 10, 208, hd,
                                     C.c_float(0.1), C.c_float(0.0), 1, 0, S()) == -2
