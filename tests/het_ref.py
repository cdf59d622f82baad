"""Test helper: the heteroscedastic probe head restated on the host -- Monte-Carlo softmax over logits with a
low-rank-plus-diagonal Gaussian noise, what the docstrings of the reference's modeling_finetune.MCSoftmaxDenseFA (:904-1217) describe
(edward2's MCSoftmaxDenseFA, non-parameter-efficient form; the diagonal scale is the reference's: a plain Linear plus
MIN_SCALE_MONTE_CARLO = 1e-3, no softplus).  The counter-based noise is restated in exact integer arithmetic (hash, uniforms) and
float64 (Box-Muller); forward, predictive variance, backward and AdamW steps in float64.  Every function takes a `dtype`: float32 gives
torch's fp32 CPU evaluation of the same formulas, whose distance to the float64 form is the yardstick of tests/test_gpu_het.py.
No golden file: the reference's class cannot be the specification (section 9.4, three facts); tests/test_host_het.py pins this file
to autograd and to the literal einsum of :1158."""
import math

import numpy as np
import torch

import probe_ref as pr

F64 = torch.float64
MIN_SCALE = 1e-3             # MIN_SCALE_MONTE_CARLO
EPS = 1e-7                   # the clamp under the logarithm
M32 = 0xFFFFFFFF


def hash32(x):
    """uvit_hash32 of csrc/common.h on numpy uint64 arrays (or ints) holding 32-bit values: exact."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def stream_key(seed, t):
    return int(hash32((int(seed) & M32) ^ (((t + 1) * 0x9E3779B9) & M32)))


def step_seed(seed, step):
    """The seed of training step `step` (0-based): fresh noise every step."""
    return int(hash32((int(seed) & M32) ^ ((step * 0x85EBCA6B + 1) & M32)))


def uniform_bits(seed, t, B, S, n, share):
    """(h1 >> 9, h2 >> 9) of every pair: two uint64 arrays (B, S, ceil(n / 2)) of 23-bit integers."""
    rows = np.zeros(B, dtype=np.uint64) if share else np.arange(B, dtype=np.uint64)
    ctr = (rows[:, None] * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, :]) & np.uint64(M32)
    key = hash32(ctr ^ np.uint64(stream_key(seed, t)))[:, :, None]
    q = np.arange((n + 1) // 2, dtype=np.uint64)[None, None, :]
    h1, h2 = hash32((np.uint64(2) * q) ^ key), hash32((np.uint64(2) * q + np.uint64(1)) ^ key)
    return h1 >> np.uint64(9), h2 >> np.uint64(9)


def uniforms(seed, t, B, S, n, share, dtype=F64):
    """(u1, u2) = ((h >> 9) + 0.5) * 2^-23, exact in float32 and in float64."""
    a, b = uniform_bits(seed, t, B, S, n, share)
    f = lambda v: ((torch.from_numpy(v.astype(np.int64)).to(dtype) + 0.5) * 2.0 ** -23)      # noqa: E731
    return f(a), f(b)


def normals(seed, t, B, S, n, share, dtype=F64):
    """(B, S, n): Box-Muller, both values of a pair used; the last pair is half used when n is odd."""
    u1, u2 = uniforms(seed, t, B, S, n, share, dtype)
    r = torch.sqrt(-2.0 * torch.log(u1))
    ang = (2.0 * math.pi) * u2
    out = torch.stack([r * torch.cos(ang), r * torch.sin(ang)], dim=-1).reshape(B, S, -1)
    return out[:, :, :n].contiguous()


def noise(B, S, K, R, seed, share, dtype=F64):
    """(epsR (B, S, R), epsK (B, S, K)): streams 0 and 1."""
    return normals(seed, 0, B, S, R, share, dtype), normals(seed, 1, B, S, K, share, dtype)


def split(lin, K, R):
    """lin (B, K (R + 2)) -> loc (B, K), d = draw + 1e-3 (B, K), V (B, K, R)."""
    B = lin.shape[0]
    return lin[:, :K], lin[:, K:2 * K] + MIN_SCALE, lin[:, 2 * K:].reshape(B, K, R)


def latents(lin, epsR, epsK, K, R):
    """u (B, S, K) = loc + V . epsR_s + d * epsK_s."""
    loc, d, V = split(lin, K, R)
    return loc[:, None, :] + torch.einsum("bkr,bsr->bsk", V, epsR) + d[:, None, :] * epsK


def forward(lin, epsR, epsK, K, R, temperature=1.0, eps=EPS, dtype=F64):
    """(z, p, pvar, y): y_s = softmax(u_s / T) over the classes, p = mean_s y_s, z = log(clamp(p, eps, 1)),
    pvar = max(mean_s y_s^2 - p^2, 0)."""
    lin, epsR, epsK = (t.to(dtype) for t in (lin, epsR, epsK))
    y = torch.softmax(latents(lin, epsR, epsK, K, R) / temperature, dim=-1)
    p = y.mean(1)
    pvar = ((y * y).mean(1) - p * p).clamp_min(0.0)
    return torch.log(p.clamp(eps, 1.0)), p, pvar, y


def backward(lin, p, dz, epsR, epsK, K, R, temperature=1.0, eps=EPS, dtype=F64):
    """dlin (B, K (R + 2)) in the layout of lin from dz, the gradient at z, and the forward's p."""
    lin, p, dz, epsR, epsK = (t.to(dtype) for t in (lin, p, dz, epsR, epsK))
    S = epsR.shape[1]
    y = torch.softmax(latents(lin, epsR, epsK, K, R) / temperature, dim=-1)
    dp = torch.where((p >= eps) & (p <= 1.0), dz / p, torch.zeros_like(p))            # the clamp's gradient
    a = (y * dp[:, None, :]).sum(-1, keepdim=True)
    du = y * (dp[:, None, :] - a) / (S * temperature)
    dV = torch.einsum("bsk,bsr->bkr", du, epsR)
    return torch.cat([du.sum(1), (du * epsK).sum(1), dV.reshape(lin.shape[0], K * R)], dim=1)


def head_lin(feat, W, bias, dtype=F64):
    """The three layers as one: lin = f . W^T + bias, W (K (R + 2), C) = [W_loc | W_diag | W_scale]."""
    return feat.to(dtype) @ W.to(dtype).t() + bias.to(dtype)


def grads(feat, W, bias, labels, K, R, S, seed, share, smoothing, temperature=1.0, dtype=F64):
    """(loss, dW, dbias, z, p) of the mean smoothed cross-entropy on z."""
    B = feat.shape[0]
    lin = head_lin(feat, W, bias, dtype)
    epsR, epsK = noise(B, S, K, R, seed, share, dtype)
    z, p, _, _ = forward(lin, epsR, epsK, K, R, temperature, EPS, dtype)
    _, loss, dz = pr.smoothed_ce(z, labels, smoothing)
    dlin = backward(lin, p, dz, epsR, epsK, K, R, temperature, EPS, dtype)
    return loss, dlin.t() @ feat.to(dtype), dlin.sum(0), z, p


def train_steps(feat, W, bias, labels, K, R, S, seed, smoothing, lr, wd, steps, temperature=1.0, max_norm=None, first_step=0):
    """`steps` training steps on one batch of (frozen) features in float64: share = 0, the seed of step t is step_seed(seed, t);
    AdamW over {W: weight_decay, bias: 0}.  Returns the per-step losses, gradient norms, the first step's gradients, (W, bias)."""
    opt = pr.HeadAdamW(W, bias)
    losses, norms, first = [], [], None
    for t in range(steps):
        loss, dW, db, _, _ = grads(feat, opt.p[0], opt.p[1], labels, K, R, S, step_seed(seed, first_step + t), 0, smoothing, temperature)
        first = first if first is not None else (dW, db)
        norms.append(opt.step((dW, db), lr, wd, max_norm))
        losses.append(float(loss))
    return losses, norms, first, opt.p


def chunk_size(S):
    """Samples per chunk of the kernels' partition (csrc/het.hip: het_chunk_size): 64 ceil(S / 512)."""
    return 64 * ((S + 511) // 512)
