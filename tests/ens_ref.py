"""Test helper: the ensemble probe head restated on the host -- M linear heads on one feature vector, their
smoothed cross-entropies with optional online-bagging weights, the per-member gradient clip, the combination of the members (the mean
of their logits, engine_for_finetuning.py:288-290, or the logarithm of the mean of their softmaxes) and the split of the predictive
entropy.  The bagging weights are exact integer arithmetic; everything else is float64.  Functions that take a `dtype` give, with
float32, torch's fp32 CPU evaluation of the same formulas, whose distance to the float64 form is the yardstick of
tests/test_gpu_ens.py.  torch and numpy only."""
import math

import numpy as np
import torch

import probe_ref as pr
from het_ref import M32, hash32  # noqa: F401  (uvit_hash32 on numpy uint64 arrays, exact)

F64 = torch.float64
# ceil(2^23 e^-1 sum_{i <= n} 1 / i!): the Poisson(1) CDF on the 23-bit uniform
T = (3085997, 6171993, 7714992, 8229324, 8357907, 8383624, 8387910, 8388523)


def step_seed(seed, step):
    """The bagging seed of training step `step` (0-based)."""
    return int(hash32((int(seed) & M32) ^ ((step * 0x85EBCA6B + 1) & M32)))


def bag_uniforms(B, M, seed):
    """The 23-bit uniforms (B, M) the weights are read from, as int64."""
    key = np.uint64(int(hash32((int(seed) & M32) ^ 0x9E3779B9)))
    idx = np.arange(B * M, dtype=np.uint64) & np.uint64(M32)
    return (hash32(idx ^ key) >> np.uint64(9)).astype(np.int64).reshape(B, M)


def bag_weights(B, M, seed):
    """w (B, M) float64 with integer values 0..8: #{n : u >= T[n]}."""
    u = bag_uniforms(B, M, seed)
    return torch.from_numpy(sum((u >= t).astype(np.int64) for t in T)).to(F64)


def ce(lin, labels, w, s, dtype=F64):
    """lin (B, M, K), labels (B,) int64, w (B, M) or None -> (row_loss (B, M) unweighted, loss (M + 1): the members' weighted means then
    their mean, dlin (B, M, K) = the gradient of sum_m loss_m, counters (M, 2) int: uvit_op_probe_ce's two rules per member).  A label
    outside [0, K) makes its row NaN for every member and moves no counter."""
    z = lin.to(dtype)
    B, M, K = z.shape
    valid = (labels >= 0) & (labels < K)
    y = torch.where(valid, labels, torch.zeros_like(labels)).view(B, 1, 1).expand(B, M, 1)
    logp = torch.log_softmax(z, dim=-1)
    rows = (1.0 - s) * -logp.gather(2, y).squeeze(2) + s * -logp.mean(-1)
    onehot = torch.zeros_like(z).scatter_(2, y, 1.0)
    d = (logp.exp() - (1.0 - s) * onehot - s / K) / B
    wt = torch.ones(B, M, dtype=dtype) if w is None else w.to(dtype)
    d = d * wt[:, :, None]
    nan = torch.full((), float("nan"), dtype=dtype)
    rows = torch.where(valid[:, None], rows, nan)
    d = torch.where(valid[:, None, None], d, nan)
    loss_m = (wt * rows).sum(0) / B
    loss = torch.cat([loss_m, loss_m.mean().view(1)])
    zy = z.gather(2, y)
    notself = torch.ones_like(z, dtype=torch.bool).scatter_(2, y, False)
    top1 = ((z >= zy) & notself).sum(-1) == 0
    top5 = (z > zy).sum(-1) < 5
    counters = torch.stack([(top1 & valid[:, None]).sum(0), (top5 & valid[:, None]).sum(0)], dim=1)
    return rows, loss, d, counters


def segments(M, K, C):
    """[(weight lo, weight hi, bias lo, bias hi)] of the members in the arena [W (M K, C) | bias (M K) | pad]."""
    w0 = M * K * C
    return [(m * K * C, (m + 1) * K * C, w0 + m * K, w0 + (m + 1) * K) for m in range(M)]


def clip(grad, M, K, C, max_norm):
    """grad: the flat gradient arena.  (norms (M) float64, the arena after the per-member clip in float64).  A member whose sum of
    squares is not finite is left as it is; max_norm <= 0 leaves everything."""
    g = grad.to(F64).clone()
    norms = []
    for wl, wh, bl, bh in segments(M, K, C):
        ss = float((g[wl:wh] ** 2).sum() + (g[bl:bh] ** 2).sum())
        norm = math.sqrt(ss) if math.isfinite(ss) else ss
        norms.append(norm)
        if max_norm > 0 and math.isfinite(ss):
            coef = min(max_norm / (norm + 1e-6), 1.0)
            g[wl:wh] *= coef
            g[bl:bh] *= coef
    return torch.tensor(norms, dtype=F64), g


def xlogx(p):
    return torch.where(p > 0, p * torch.log(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p))


def combine(lin, M, mode, dtype=F64):
    """lin (B, M K) or (B, M, K) -> (z (B, K) in `dtype`, unc (B, 5) float64 {total, aleatoric, mi, var_pred, disagreement}, k* (B),
    k_m (B, M)).  The member probabilities are formed in `dtype` and widened; every sum and logarithm of unc is float64."""
    B = lin.shape[0]
    x = lin.reshape(B, M, -1).to(dtype)
    lse = torch.logsumexp(x, dim=-1, keepdim=True)
    if mode == 0:
        z = torch.mean(torch.stack([x[:, m] for m in range(M)]), 0)               # engine_for_finetuning.py:288-290
    else:
        z = torch.logsumexp(x - lse, dim=1) - math.log(M)
    p = torch.exp(x - lse).to(F64)
    pbar = p.mean(1)
    total = -xlogx(pbar).sum(-1)
    aleatoric = -xlogx(p).sum(-1).mean(1)
    kstar, km = z.argmax(-1), x.argmax(-1)
    pk = p.gather(2, kstar.view(B, 1, 1).expand(B, M, 1)).squeeze(2)
    var = ((pk - pbar.gather(1, kstar.view(B, 1))) ** 2).mean(1)
    dis = (km != kstar[:, None]).to(F64).sum(1) / M
    unc = torch.stack([total, aleatoric, (total - aleatoric).clamp_min(0.0), var, dis], dim=1)
    unc[torch.isnan(x).flatten(1).any(1)] = float("nan")
    return z, unc, kstar, km


def head_lin(feat, W, bias, dtype=F64):
    """The M heads as one: lin = f . W^T + bias, W (M K, C)."""
    return feat.to(dtype) @ W.to(dtype).t() + bias.to(dtype)


def grads(feat, W, bias, labels, M, s, w=None, dtype=F64):
    """(loss (M + 1), dW (M K, C), dbias (M K), lin (B, M K)) of sum_m loss_m."""
    B = feat.shape[0]
    lin = head_lin(feat, W, bias, dtype)
    _, loss, d, _ = ce(lin.view(B, M, -1), labels, w, s, dtype)
    d = d.reshape(B, -1)
    return loss, d.t() @ feat.to(dtype), d.sum(0), lin


class HeadAdamW(pr.HeadAdamW):
    """probe_ref.HeadAdamW (float64) with a `dtype`: float32 gives torch's fp32 CPU evaluation of the same update."""

    def __init__(self, W, bias, dtype=F64):
        super().__init__(W, bias)
        self.dtype = dtype
        self.p = [t.to(dtype) for t in self.p]
        self.m, self.v = [torch.zeros_like(t) for t in self.p], [torch.zeros_like(t) for t in self.p]

    def step(self, grads, lr, wd, max_norm=None):
        if self.dtype == F64:
            return super().step(grads, lr, wd, max_norm)
        g = [x.to(self.dtype).clone() for x in grads]
        norm = torch.sqrt(sum((x.double() ** 2).sum() for x in g)).to(self.dtype)      # the clip's sum of squares is double on the device
        if max_norm is not None and max_norm > 0:
            coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
            g = [x * coef for x in g]
        self.t += 1
        b1, b2 = self.betas
        for i, (p, gi) in enumerate(zip(self.p, g)):
            if i == 0:
                p.mul_(1.0 - lr * wd)
            self.m[i].mul_(b1).add_(gi, alpha=1.0 - b1)
            self.v[i].mul_(b2).addcmul_(gi, gi, value=1.0 - b2)
            denom = self.v[i].sqrt() / math.sqrt(1.0 - b2 ** self.t) + self.eps
            p.addcdiv_(self.m[i], denom, value=-lr / (1.0 - b1 ** self.t))
        return float(norm)


def step(feat, opts, labels, s, lr, wd, w=None, max_norm=None, dtype=F64):
    """One training step on frozen features: `opts` is a list of HeadAdamW, one per member (AdamW is elementwise and HeadAdamW's clip
    is over its own head: the per-member clip).  Returns (loss (M + 1), the members' gradient norms, (dW, dbias))."""
    M = len(opts)
    W, bias = torch.cat([o.p[0] for o in opts]), torch.cat([o.p[1] for o in opts])
    K = opts[0].p[1].shape[0]
    loss, dW, db, _ = grads(feat, W, bias, labels, M, s, w, dtype)
    norms = [o.step((dW[m * K:(m + 1) * K], db[m * K:(m + 1) * K]), lr, wd, max_norm) for m, o in enumerate(opts)]
    return loss, norms, (dW, db)


def train_steps(feat, W, bias, labels, M, s, lr, wd, steps, bagging_seed=None, max_norm=None, dtype=F64):
    """`steps` steps on one batch: W (M K, C), bias (M K).  With `bagging_seed` the weights of step t are
    bag_weights(B, M, step_seed(bagging_seed, t)).  Returns (per-step losses (M + 1), per-step member norms, (W, bias))."""
    K, B = W.shape[0] // M, feat.shape[0]
    opts = [HeadAdamW(W[m * K:(m + 1) * K], bias[m * K:(m + 1) * K], dtype) for m in range(M)]
    losses, norms = [], []
    for t in range(steps):
        w = None if bagging_seed is None else bag_weights(B, M, step_seed(bagging_seed, t))
        loss, n, _ = step(feat, opts, labels, s, lr, wd, w, max_norm, dtype)
        losses.append(loss)
        norms.append(n)
    return losses, norms, (torch.cat([o.p[0] for o in opts]), torch.cat([o.p[1] for o in opts]))
