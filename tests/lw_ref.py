"""Test helper: the layer-weighted probe (csrc/layerweights.hip, uncertainty-vit_amd/lw_probe.py) restated in
float64 on the host, from the reference's arithmetic (modeling_finetune.py:499-510 and the autograd of those lines), with the error
bounds of the kernels.  tests/test_host_lw.py pins it to torch's own expressions and autograd and to tests/golden/probe_lw_t48.npz,
which the reference wrote; tests/test_gpu_lw.py applies it to the kernels.

Bounds, with u = 2^-24 and ud = 2^-53, first order in u, times SLACK = 1.01 for the higher orders; derived from the kernels'
summation lengths, none comes from running them.  S always stands for the sum of the |terms| an element is formed from.

  pool, mode 0      a token's value goes through at most ceil(ceil(N / 8) / 4) - 1 serial adds of its wave, 3 adds over the four waves, 7
                    over the eight slices and one division: |got - ref| <= (ceil(ceil(N / 8) / 4) + 10) u mean_t |x_t|
  pool, mode 1      a copy: bit equality
  layernorm         first-order propagation through y = (p - mu) / sqrt(var + eps) of the pool's bound e_p and of the row sums (a lane's
                    4 ceil(C / 256) serial adds, the 6 levels of the xor tree: n = 4 ceil(C / 256) + 6):
                      d_mu  = (n + 1) u mean|p| + mean(e_p)
                      e_d   = e_p + d_mu + u |p - mu|                           each centred value
                      d_var = (sum 2 |p - mu| e_d + (n + 2) u q) / C + 3 u (var + eps)      q = sum (p - mu)^2; the division, the
                                                                                           fp32 eps, the addition
                      |got - ref| <= e_d / sigma + |y| (d_var / (2 sigma^2) + 2 u) + 2 u |y|      (rsqrtf within 2 u)
  softmax           v - m is one rounding, expf within one ulp: e_l carries (|v_l - m| + 2) u; the xor tree 6 u, the division u:
                      r_l = (|v_l - m| + 2) u + sum_j w_j (|v_j - m| + 2) u + 7 u         relative error of w_l
  combine           an fma chain of L terms: |got - ref| <= sum_l w_l |p_l| (r_l + L u)
  input gradient    16 fmas inside a tile, ceil(K / 16) adds of the tiles: |got - ref| <= (16 + ceil(K / 16)) u sum_k |d_k| |W_kc|
  layer gradient    relative to S = max_l sum_{b, c} |dfeat| |p_l|, not to the result -- g_l - sum_j w_j g_j cancels when the layers
                    resemble each other.  The products are exact in double, a row's sum is n adds, the rows B more, the mix L + 6:
                      |got - ref| <= w_l (3 max_j r_j + 2 (n + B + L + 8) ud) S + u |ref|
"""
import math

import torch

import probe_ref as pr
from oracle import vit_oracle as vo

F64 = torch.float64
U, UD, SLACK = 2.0 ** -24, 2.0 ** -53, 1.01
LN_EPS = 1e-5                # F.layer_norm's default (modeling_finetune.py:505)
SLICES, WAVES = 8, 4         # csrc/layerweights.hip: LW_SLICES, LW_WAVES
CE_TOL = 1e-5                # uvit_op_probe_ce: tests/test_gpu_probe.py::test_cross_entropy derives |loss - ref| <= 1e-5 (1 + |ref|), |d - ref| <= 1e-5 / B


def row_adds(C):
    """Additions a value of a C-column row goes through in a one-wave row sum."""
    return 4 * math.ceil(C / 256) + 6


# ---- the four ops ----
def pool(xs, mode, layernorm, eps=LN_EPS):
    """xs: L tensors (B, N, C), the residual streams behind blocks 0 .. L-1 -> pooled (B, L, C) float64.  mode 0: x.mean(1) over ALL
    tokens; mode 1: x[:, 0]; layernorm: F.layer_norm(p, (C,)) without affine."""
    rows = []
    for x in xs:
        x = x.to(F64)
        p = x.mean(1) if mode == 0 else x[:, 0]
        if layernorm:
            mu = p.mean(-1, keepdim=True)
            var = ((p - mu) ** 2).mean(-1, keepdim=True)
            p = (p - mu) / torch.sqrt(var + eps)
        rows.append(p)
    return torch.stack(rows, 1)


def softmax_w(log_w):
    v = log_w.to(F64)
    e = torch.exp(v - v.max())
    return e / e.sum()


def combine(pooled, log_w):
    """feat (B, C) = sum_l softmax(log_w)_l pooled[:, l]   (F.linear(torch.stack(layer_xs, -1), weights))."""
    return torch.einsum("blc,l->bc", pooled.to(F64), softmax_w(log_w))


def input_grad(dlogits, W):
    """dfeat (B, C) = dlogits (B, K) . W (K, C): autograd of the nn.Linear with respect to its input."""
    return dlogits.to(F64) @ W.to(F64)


def lw_grad(dfeat, pooled, log_w):
    """(dlog_w (L), g (L)): g_l = <dfeat, pooled[:, l]>, dlog_w_l = w_l (g_l - sum_j w_j g_j), the softmax's Jacobian applied to g."""
    w = softmax_w(log_w)
    g = torch.einsum("bc,blc->l", dfeat.to(F64), pooled.to(F64))
    return w * (g - (w * g).sum()), g


# ---- their bounds ----
def pool_bound(xs, mode, layernorm, eps=LN_EPS):
    """|got - ref| per element of pool(); zeros where the op is a copy."""
    B, N, C = xs[0].shape
    n = row_adds(C)
    out = []
    for x in xs:
        x = x.to(F64)
        if mode == 0:
            p, e_p = x.mean(1), (math.ceil(math.ceil(N / SLICES) / WAVES) + 10) * U * x.abs().mean(1)
        else:
            p, e_p = x[:, 0], torch.zeros(B, C, dtype=F64)
        if layernorm:
            mu = p.mean(-1, keepdim=True)
            d = p - mu
            q = (d * d).sum(-1, keepdim=True)
            var = q / C
            sigma = torch.sqrt(var + eps)
            d_mu = (n + 1) * U * p.abs().mean(-1, keepdim=True) + e_p.mean(-1, keepdim=True)
            e_d = e_p + d_mu + U * d.abs()
            d_var = ((2 * d.abs() * e_d).sum(-1, keepdim=True) + (n + 2) * U * q) / C + 3 * U * (var + eps)
            y = d / sigma
            e_p = e_d / sigma + y.abs() * (d_var / (2 * sigma * sigma) + 2 * U) + 2 * U * y.abs()
        out.append(SLACK * e_p)
    return torch.stack(out, 1)


def softmax_rel(log_w):
    """r_l: the relative error of the fp32 w_l."""
    v = log_w.to(F64)
    a = ((v - v.max()).abs() + 2) * U
    return a + (softmax_w(log_w) * a).sum() + 7 * U


def combine_bound(pooled, log_w):
    L = pooled.shape[1]
    return SLACK * torch.einsum("blc,l->bc", pooled.to(F64).abs(), softmax_w(log_w) * (softmax_rel(log_w) + L * U))


def input_grad_bound(dlogits, W):
    K = W.shape[0]
    return SLACK * (16 + math.ceil(K / 16)) * U * (dlogits.to(F64).abs() @ W.to(F64).abs())


def lw_grad_scale(dfeat, pooled):
    """S = max_l sum_{b, c} |dfeat| |pooled[:, l]|: what the layer gradient's bound is relative to."""
    return float(torch.einsum("bc,blc->l", dfeat.to(F64).abs(), pooled.to(F64).abs()).max())


def lw_grad_bound(dfeat, pooled, log_w):
    B, L, C = pooled.shape
    ref, _ = lw_grad(dfeat, pooled, log_w)
    S = lw_grad_scale(dfeat, pooled)
    return SLACK * (softmax_w(log_w) * (3 * float(softmax_rel(log_w).max()) + 2 * (row_adds(C) + B + L + 8) * UD) * S + U * ref.abs())


# ---- the model ----
def layer_streams(enc, cfg, images):
    """The residual stream behind every block, float64: the oracle's block stack (modeling_finetune.py:494-497)."""
    p = {k: v.to(F64) for k, v in enc.items()}
    return vo.forward_features(p, cfg, images.to(F64), None, "end")


def features(enc, cfg, images, log_w, use_cls, layernorm):
    """forward_features of the classifier with learn_layer_weights (modeling_finetune.py:499-510)."""
    return combine(pool(layer_streams(enc, cfg, images), 1 if use_cls else 0, layernorm), log_w)


def step(pooled, W, bias, log_w, labels, smoothing):
    """One forward + backward on pooled features: a dict of feat, logits, loss, dlogits, dW, dbias, dfeat, dlog_w."""
    feat = combine(pooled, log_w)
    logits = pr.head_logits(feat, W, bias)
    _, loss, dz = pr.smoothed_ce(logits, labels, smoothing)
    dW, db = pr.head_grads(dz, feat)
    dfeat = input_grad(dz, W)
    dlw, _ = lw_grad(dfeat, pooled, log_w)
    return dict(feat=feat, logits=logits, loss=loss, dlogits=dz, dW=dW, dbias=db, dfeat=dfeat, dlog_w=dlw)


def step_bounds(pooled, W, bias, log_w, labels, smoothing):
    """Bounds of step()'s entries for the kernels fed the same fp32 pooled, W, bias and log_w: each op's own bound plus, to first
    order, what it inherits from its inputs.  Logits: uvit_op_probe_logits adds C / 16 tile sums of 16 fmas and the bias.  The
    criterion: uvit_op_probe_ce's own CE_TOL, and the softmax moves by at most 2 max_k |dz_k| per element, the loss by as much.
    dW, dbias: uvit_op_probe_head_grad, a chain of B fmas."""
    r = step(pooled, W, bias, log_w, labels, smoothing)
    B, L, C = pooled.shape
    K = W.shape[0]
    Wa, f, d = W.to(F64).abs(), r["feat"].abs(), r["dlogits"].abs()
    e_f = combine_bound(pooled, log_w)
    e_z = e_f @ Wa.t() + SLACK * (math.ceil(C / 16) + 18) * U * (f @ Wa.t() + bias.to(F64).abs())
    zmax = e_z.max(-1, keepdim=True).values
    e_loss = 2 * float(zmax.max()) + CE_TOL * (1 + abs(float(r["loss"])))
    e_d = (CE_TOL + 2 * zmax) / B * torch.ones_like(d)
    e_dW = e_d.t() @ f + d.t() @ e_f + SLACK * (B + 1) * U * (d.t() @ f)
    e_db = e_d.sum(0) + SLACK * (B + 1) * U * d.sum(0)
    e_df = e_d @ Wa + input_grad_bound(r["dlogits"], W)
    w = softmax_w(log_w)
    e_g = torch.einsum("bc,blc->l", e_df, pooled.to(F64).abs())                  # what g_l inherits from dfeat
    e_dlw = lw_grad_bound(r["dfeat"], pooled, log_w) + SLACK * w * (e_g + (w * e_g).sum())
    return r, dict(feat=e_f, logits=e_z, loss=e_loss, dlogits=e_d, dW=e_dW, dbias=e_db, dfeat=e_df, dlog_w=e_dlw)


class LwAdamW(pr.HeadAdamW):
    """torch.optim.AdamW over {head.weight: weight_decay; head.bias, layer_log_weights: 0}: a one-dimensional parameter does not decay
    (optim_factory.get_parameter_groups) and its lr scale is 1."""

    def __init__(self, W, bias, log_w, **kw):
        super().__init__(W, bias, **kw)
        self.p.append(log_w.to(F64).clone())
        self.m.append(torch.zeros_like(self.p[2]))
        self.v.append(torch.zeros_like(self.p[2]))


def train_steps(pooled, W, bias, log_w, labels, smoothing, lr, wd, steps, max_norm=None):
    """`steps` steps on one batch of (frozen) pooled features: per-step losses and grad norms, the first step's results, the
    parameters [W, bias, log_w]."""
    opt = LwAdamW(W, bias, log_w)
    losses, norms, first = [], [], None
    for _ in range(steps):
        r = step(pooled, opt.p[0], opt.p[1], opt.p[2], labels, smoothing)
        first = first if first is not None else r
        norms.append(opt.step([r["dW"], r["dbias"], r["dlog_w"]], lr, wd, max_norm))
        losses.append(float(r["loss"]))
    return losses, norms, first, opt.p


# ---- inputs of the op tests: computed once per shape by the tests' caches ----
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


POOL_SHAPES = [(1, 1, 1, 4), (5, 2, 10, 128), (3, 12, 197, 768), (2, 3, 197, 1280), (2, 64, 7, 2048)]      # (B, L, N, C)
INPUT_GRAD_SHAPES = [(1, 1, 4), (5, 10, 128), (67, 130, 260), (128, 1000, 768)]                                # (B, K, C)


def stream_case(shape):
    """L residual streams (B, N, C) fp32: unit noise plus a per-(layer, sample, channel) pattern of unit variance and a per-layer
    offset, so that a pooled row has a spread of about 1 and the layers differ."""
    B, L, N, C = shape
    return [rnd(B, N, C, seed=100 + l) + rnd(B, 1, C, seed=200 + l) + 0.25 * l for l in range(L)]


def log_w_case(L, seed=7):
    """Log-weights of spread 1, none zero."""
    return rnd(L, seed=seed) + 0.1
