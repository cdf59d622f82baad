"""Test helper: the linear probe restated in float64 torch on the host -- pool -> LayerNorm without affine -> head -> smoothed
cross-entropy -> head gradients -> AdamW -- on top of the oracle's encoder forward (oracle/vit_oracle.py).  Each function cites
the reference lines it follows; tests/test_host_probe.py pins it to tests/golden/probe_t48.npz, which the reference wrote."""
import math
import os

import numpy as np
import torch

from oracle import vit_oracle as vo

F64 = torch.float64


def load_fixture(golden_dir):
    """tests/golden/probe_t48.npz -> (fx, cfg, encoder params {name: fp32 tensor}, head weight, head bias, images, labels)."""
    fx = np.load(os.path.join(golden_dir, "probe_t48.npz"))
    img, dim, depth, heads, K, B, steps = [int(v) for v in fx["cfg"]]
    cfg = vo.VitConfig(img_size=img, embed_dim=dim, depth=depth, num_heads=heads, init_values=float(fx["init_values"]))
    enc = {}
    for k in fx.files:
        if k.startswith("enc/"):
            enc[k[4:]] = torch.from_numpy(fx[k])
        elif k.startswith("encq/"):       # 8-bit grid: value = float32(q) * scale (tools/gen_golden_probe.py)
            enc[k[5:]] = torch.from_numpy(fx[k].astype(np.float32) * np.float32(fx["encs/" + k[5:]]))
    images = torch.from_numpy(fx["images"].astype(np.float32))
    return fx, cfg, enc, torch.from_numpy(fx["head/weight"]), torch.from_numpy(fx["head/bias"]), images, torch.from_numpy(fx["labels"])


def pool_norm(x, eps):
    """fc_norm(x[:, 1:].mean(1)) with elementwise_affine = False: modeling_finetune.py:410-412,512-515.  x (B, N, C)."""
    t = x.to(F64)[:, 1:, :].mean(1)
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return (t - mu) / torch.sqrt(var + eps)


def features(enc, cfg, images):
    """forward_features of the classifier (modeling_finetune.py:476-517; self.norm is Identity with mean pooling): the oracle's
    block stack in float64, then pool_norm."""
    p = {k: v.to(F64) for k, v in enc.items()}
    x = vo.forward_features(p, cfg, images.to(F64), None, "end")[-1]
    return pool_norm(x, cfg.ln_eps)


def head_logits(feat, W, bias):
    """nn.Linear head, modeling_finetune.py:421,522."""
    return feat.to(F64) @ W.to(F64).t() + bias.to(F64)


def smoothed_ce(logits, labels, smoothing):
    """timm LabelSmoothingCrossEntropy (run_class_finetuning.py:620-621; smoothing 0 = nn.CrossEntropyLoss, :623):
    row losses (B,), their mean, and d mean / d logits."""
    z = logits.to(F64)
    B, K = z.shape
    logp = torch.log_softmax(z, dim=-1)
    nll = -logp.gather(1, labels.view(-1, 1)).squeeze(1)
    smooth = -logp.mean(-1)
    rows = (1.0 - smoothing) * nll + smoothing * smooth
    onehot = torch.zeros_like(z).scatter_(1, labels.view(-1, 1), 1.0)
    dz = (logp.exp() - (1.0 - smoothing) * onehot - smoothing / K) / B
    return rows, rows.mean(), dz


def head_grads(dlogits, feat):
    """autograd of the nn.Linear: dW = dlogits^T feat, dbias = column sums."""
    return dlogits.to(F64).t() @ feat.to(F64), dlogits.to(F64).sum(0)


def topk_counts(logits, labels):
    """(top-1, top-5) correct counts as timm.utils.accuracy counts them (torch.topk)."""
    k = min(5, logits.shape[1])
    top = logits.topk(k, dim=1).indices
    hit = top == labels.view(-1, 1)
    return int(hit[:, :1].sum()), int(hit.sum())


def no_ties_among_top(logits, n=6):
    """True when the n largest values of every row are pairwise different (top-k is then unambiguous)."""
    v = logits.topk(min(n, logits.shape[1]), dim=1).values
    return bool((v[:, :-1] > v[:, 1:]).all()) if v.shape[1] > 1 else True


class HeadAdamW:
    """torch.optim.AdamW over {head.weight: weight_decay, head.bias: 0} (optim_factory.py:58-97, 133-134), float64, with
    clip_grad_norm_ (utils.py:375-376) when max_norm is given."""

    def __init__(self, W, bias, betas=(0.9, 0.999), eps=1e-8):
        self.p = [W.to(F64).clone(), bias.to(F64).clone()]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.betas, self.eps, self.t = betas, eps, 0

    def step(self, grads, lr, wd, max_norm=None):
        g = [x.to(F64).clone() for x in grads]
        norm = math.sqrt(sum(float((x ** 2).sum()) for x in g))
        if max_norm is not None and max_norm > 0:
            coef = min(1.0, max_norm / (norm + 1e-6))
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
        return norm


def train_steps(feat, W, bias, labels, smoothing, lr, wd, steps, max_norm=None):
    """`steps` probe steps on one batch of (frozen) features: per-step losses and grad norms, the first step's gradients, the head."""
    opt = HeadAdamW(W, bias)
    losses, norms, first = [], [], None
    for _ in range(steps):
        _, loss, dz = smoothed_ce(head_logits(feat, opt.p[0], opt.p[1]), labels, smoothing)
        g = head_grads(dz, feat)
        first = first if first is not None else g
        norms.append(opt.step(g, lr, wd, max_norm))
        losses.append(float(loss))
    return losses, norms, first, opt.p
