"""Test helper: the random-feature Gaussian-process head restated in float64 torch on the host -- LayerNorm
with affine -> frozen random Fourier features with a cosine -> output layer without bias -> smoothed cross-entropy -> the three
gradients -> AdamW; the Laplace precision matrix and the predictive variance.  Each function cites the lines of the reference's
modeling_finetune.SNGP it follows; tests/test_host_gp.py pins it to tests/golden/gp_head.npz, which the reference class wrote
(tools/gen_golden_gp.py)."""
import math
import os

import numpy as np
import torch

import probe_ref as pr

F64 = torch.float64
LN_EPS, RIDGE, MOMENTUM = 1e-12, 1e-3, 0.999          # SNGP.__init__ defaults: layer_norm_eps, gp_cov_ridge_penalty, gp_cov_momentum
HEAD_KEYS = ("gamma", "beta", "W_rf", "b_rf", "W_out")


def load_fixture(golden_dir):
    """tests/golden/gp_head.npz -> (fx, head {name: fp32 tensor}, features (B, C) fp32, labels)."""
    fx = np.load(os.path.join(golden_dir, "gp_head.npz"))
    head = {k: torch.from_numpy(fx["head/" + k]) for k in HEAD_KEYS if "head/" + k in fx.files}
    head["W_rf"] = torch.from_numpy(fx["headq/W_rf"].astype(np.float32) * np.float32(fx["heads/W_rf"]))      # 8-bit grid, exact
    return fx, head, torch.from_numpy(fx["features"]), torch.from_numpy(fx["labels"])


def layer_norm(f, eps=LN_EPS):
    """(ghat, mean, var): the LayerNorm's normalised rows, biased variance (:555, :580)."""
    f = f.to(F64)
    mu = f.mean(-1, keepdim=True)
    var = ((f - mu) ** 2).mean(-1, keepdim=True)
    return (f - mu) / torch.sqrt(var + eps), mu, var


def features(f, gamma, beta, W_rf, b_rf, scale=1.0, eps=LN_EPS):
    """(ghat, u, phi): g = ghat gamma + beta; u = g W_rf^T + b_rf; phi = scale cos(u)   (:579-587)."""
    ghat, _, _ = layer_norm(f, eps)
    g = ghat * gamma.to(F64) + beta.to(F64)
    u = g @ W_rf.to(F64).t() + b_rf.to(F64)
    return ghat, u, scale * torch.cos(u)


def logits(phi, W_out):
    """The output layer: no bias of its own, plus the constant gp_output_bias = 0 (:556, :590)."""
    return phi.to(F64) @ W_out.to(F64).t()


def precision_update(P, phi, momentum=MOMENTUM):
    """update_cov (:599-616)."""
    phi, P = phi.to(F64), P.to(F64)
    M = phi.t() @ phi
    if momentum > 0:
        return momentum * P + (1.0 - momentum) * (M / phi.shape[0])
    return P + M


def initial_precision(D, ridge=RIDGE):
    return ridge * torch.eye(D, dtype=F64)


def variance(phi, P, ridge=RIDGE):
    """The diagonal of compute_predictive_covariance (:618-626): ridge phi_b^T inv(P) phi_b."""
    phi = phi.to(F64)
    S = torch.linalg.inv(P.to(F64))
    return ridge * ((phi @ S) * phi).sum(-1)


def variance_magnitude(phi, Sigma, ridge=RIDGE):
    """ridge sum_ij |phi_bi Sigma_ij phi_bj|: the sum of magnitudes a double evaluation's round-off is bounded by."""
    a = phi.to(F64).abs()
    return ridge * ((a @ Sigma.to(F64).abs()) * a).sum(-1)


def mean_field(z, var, factor):
    """edward2's mean_field_logits (not in the reference)."""
    return z.to(F64) / torch.sqrt(1.0 + factor * var.to(F64)).view(-1, 1)


def ln_grads(dz, W_out, u, W_rf, ghat, scale=1.0):
    """(dgamma, dbeta) and dW_out's companion chain: dphi = dz W_out; du = -scale sin(u) dphi; dg = du W_rf."""
    dphi = dz.to(F64) @ W_out.to(F64)
    du = -scale * torch.sin(u.to(F64)) * dphi
    dg = du @ W_rf.to(F64)
    return (dg * ghat.to(F64)).sum(0), dg.sum(0)


def grads(f, head, labels, smoothing, scale=1.0):
    """(loss, dW_out, dgamma, dbeta, phi, z) of the mean smoothed cross-entropy."""
    ghat, u, phi = features(f, head["gamma"], head["beta"], head["W_rf"], head["b_rf"], scale)
    z = logits(phi, head["W_out"])
    _, loss, dz = pr.smoothed_ce(z, labels, smoothing)
    dW = dz.t() @ phi
    dgamma, dbeta = ln_grads(dz, head["W_out"], u, head["W_rf"], ghat, scale)
    return loss, dW, dgamma, dbeta, phi, z


class GPAdamW:
    """torch.optim.AdamW over {W_out: weight_decay, gamma: 0, beta: 0} (optim_factory.get_parameter_groups: one-dimensional
    parameters do not decay), float64, with clip_grad_norm_ when max_norm is given."""

    def __init__(self, W_out, gamma, beta, betas=(0.9, 0.999), eps=1e-8):
        self.p = [t.to(F64).clone() for t in (W_out, gamma, beta)]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.betas, self.eps, self.t = betas, eps, 0

    def step(self, grads_, lr, wd, max_norm=None):
        g = [x.to(F64).clone() for x in grads_]
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


def train_steps(f, head, labels, smoothing, lr, wd, steps, scale=1.0, momentum=MOMENTUM, ridge=RIDGE, P=None, max_norm=None):
    """`steps` training steps on one batch of (frozen) features.  Each step: forward with the parameters as they are, precision update
    with that forward's phi (the reference updates inside the forward, :591-593), gradients, AdamW.  Returns per-step losses and
    gradient norms, the precision matrices after each step, and the head afterwards."""
    opt = GPAdamW(head["W_out"], head["gamma"], head["beta"])
    P = initial_precision(head["W_rf"].shape[0], ridge) if P is None else P.to(F64)
    losses, norms, Ps = [], [], []
    h = dict(head)
    for _ in range(steps):
        h["W_out"], h["gamma"], h["beta"] = opt.p
        loss, dW, dgamma, dbeta, phi, _ = grads(f, h, labels, smoothing, scale)
        P = precision_update(P, phi, momentum)
        Ps.append(P)
        norms.append(opt.step((dW, dgamma, dbeta), lr, wd, max_norm))
        losses.append(float(loss))
    h["W_out"], h["gamma"], h["beta"] = opt.p
    return losses, norms, Ps, h
