"""Generate tests/golden/gp_head.npz by running the UNMODIFIED reference head modeling_finetune.SNGP (imported from the reference
checkout through tools/ref_harness.py) on the pooled features of tests/golden/probe_t48.npz.  Build-container only; never runs on
the GPU box.

    python tools/gen_golden_gp.py

The class is the specification, not VisionTransformer(gp_layer=True): modeling_finetune.py:416-421 overwrites the SNGP head with an
nn.Linear, so the reference model never uses it.  SNGP.__init__ hard-codes torch.device('cuda') (:560); while
the constructor runs, the name `torch` in the reference module's namespace is a shim whose device() returns the CPU.  Forward,
backward, update_cov and compute_predictive_covariance then run on the CPU unchanged.

The fixture is data only: the seeded head (W_rf on an 8-bit grid: int8 plus one fp32 scale, exactly what the class was given), and what
the class computes from `features` and `labels` -- logits, the smoothing-0.1 loss, the three gradients, the precision matrix after
one and three training forwards, the three trainable parameters after three torch.optim.AdamW steps and the diagonal of
compute_predictive_covariance after those steps.  Beside each, `dev/<name>`: the class's own deviation from the float64 evaluation
of the same formulas (tests/gp_ref.py), max |fp32 - float64| / max |float64|.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gp_head.npz")
C, D, K = 128, 128, 10
SMOOTHING, LR, WD, STEPS = 0.1, 1e-3, 0.05, 3


class _CpuTorch:
    """Stands in for the name `torch` inside the reference module while SNGP.__init__ runs: device(...) is the CPU."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*a, **k):
        return torch.device("cpu")


def build_head(mf):
    real = mf.torch
    mf.torch = _CpuTorch()
    try:
        return mf.SNGP(C, D, num_classes=K)
    finally:
        mf.torch = real


def smoothed_ce(logits, target, smoothing):
    """timm.loss.LabelSmoothingCrossEntropy.forward, restated (timm is not installed)."""
    logprobs = torch.nn.functional.log_softmax(logits, dim=-1)
    nll_loss = -logprobs.gather(dim=-1, index=target.unsqueeze(1)).squeeze(1)
    smooth_loss = -logprobs.mean(dim=-1)
    return ((1.0 - smoothing) * nll_loss + smoothing * smooth_loss).mean()


def dev(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return np.float64(float((got - ref).abs().max() / ref.abs().max()))


def main():
    ref_harness.install()
    import modeling_finetune as mf
    import gp_ref as gr
    probe = np.load(os.path.join(ROOT, "tests", "golden", "probe_t48.npz"))
    feats, labels = torch.from_numpy(probe["features"]), torch.from_numpy(probe["labels"])
    assert feats.shape == (4, C)
    gen = torch.Generator().manual_seed(20241)
    torch.manual_seed(20241)
    head = build_head(mf)
    assert head.gp_input_scale == 1.0 and head.gp_cov_momentum == 0.999 and head.gp_cov_ridge_penalty == 1e-3
    # seeded away from the initial values (gamma = 1, beta = 0), so that a dropped factor cannot hide
    q = torch.clamp(torch.round(torch.randn(D, C, generator=gen) * 40.0), -127, 127).to(torch.int8)
    scale = np.float32(0.05 / 40.0)
    w = {"gamma": 1.0 + 0.1 * torch.randn(C, generator=gen), "beta": 0.05 * torch.randn(C, generator=gen),
         "W_rf": q.float() * float(scale), "b_rf": 2.0 * np.pi * torch.rand(D, generator=gen), "W_out": 0.05 * torch.randn(K, D, generator=gen)}
    with torch.no_grad():
        head._gp_input_normalize_layer.weight.copy_(w["gamma"])
        head._gp_input_normalize_layer.bias.copy_(w["beta"])
        head._random_feature.weight.copy_(w["W_rf"])
        head._random_feature.bias.copy_(w["b_rf"])
        head._gp_output_layer.weight.copy_(w["W_out"])
    trainable = [n for n, p in head.named_parameters() if p.requires_grad]
    assert trainable == ["_gp_input_normalize_layer.weight", "_gp_input_normalize_layer.bias", "_gp_output_layer.weight"], trainable
    out = {"cfg": np.array([C, D, K, feats.shape[0], STEPS], dtype=np.int64), "smoothing": np.float64(SMOOTHING), "lr": np.float64(LR),
           "weight_decay": np.float64(WD), "ridge": np.float64(head.gp_cov_ridge_penalty), "momentum": np.float64(head.gp_cov_momentum),
           "scale": np.float64(head.gp_input_scale), "features": feats.numpy(), "labels": labels.numpy(),
           "state_dict_keys": np.array(sorted(head.state_dict().keys()))}
    for k in ("gamma", "beta", "b_rf", "W_out"):
        out["head/" + k] = w[k].numpy()
    out["headq/W_rf"], out["heads/W_rf"] = q.numpy(), scale
    assert np.array_equal(q.numpy().astype(np.float32) * scale, w["W_rf"].numpy())

    # one training forward (it updates the precision matrix, :591-593) and backward
    head.train()
    z = head(feats)
    loss = smoothed_ce(z, labels, SMOOTHING)
    loss.backward()
    rl, rdW, rdg, rdb, rphi, rz = gr.grads(feats, w, labels, SMOOTHING)
    rP1 = gr.precision_update(gr.initial_precision(D), rphi)
    got = {"logits": z.detach(), "loss": loss.detach(), "grad/W_out": head._gp_output_layer.weight.grad,
           "grad/gamma": head._gp_input_normalize_layer.weight.grad, "grad/beta": head._gp_input_normalize_layer.bias.grad,
           "P1": head.precision_matrix.detach()}
    want = {"logits": rz, "loss": rl, "grad/W_out": rdW, "grad/gamma": rdg, "grad/beta": rdb, "P1": rP1}
    assert torch.equal(got["P1"], got["P1"].t())

    # three AdamW steps from the same start, the precision matrix from ridge * I again
    head.reset_cov()
    params = [head._gp_output_layer.weight, head._gp_input_normalize_layer.weight, head._gp_input_normalize_layer.bias]
    opt = torch.optim.AdamW([{"params": params[:1], "weight_decay": WD}, {"params": params[1:], "weight_decay": 0.0}], lr=LR,
                            betas=(0.9, 0.999), eps=1e-8)
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        step_loss = smoothed_ce(head(feats), labels, SMOOTHING)
        step_loss.backward()
        opt.step()
        losses.append(step_loss.item())
    rlosses, _, rPs, rh = gr.train_steps(feats, w, labels, SMOOTHING, LR, WD, STEPS)
    got.update({"step_loss": torch.tensor(losses, dtype=torch.float64), "P3": head.precision_matrix.detach(),
                "post/W_out": params[0].detach(), "post/gamma": params[1].detach(), "post/beta": params[2].detach()})
    want.update({"step_loss": torch.tensor(rlosses), "P3": rPs[-1], "post/W_out": rh["W_out"], "post/gamma": rh["gamma"],
                 "post/beta": rh["beta"]})
    # the predictive variance of the batch under the stepped head and the three-update precision matrix (no further update)
    head.eval()
    with torch.no_grad():
        phi, _ = head.gp_layer(feats, update_cov=False)
        cov = head.compute_predictive_covariance(phi)
    assert torch.equal(head.precision_matrix.detach(), got["P3"])
    _, _, rphi3 = gr.features(feats, rh["gamma"], rh["beta"], w["W_rf"], w["b_rf"])
    got["var"], want["var"] = torch.diagonal(cov).clone(), gr.variance(rphi3, rPs[-1])
    out["cond_P3"] = np.float64(float(torch.linalg.cond(rPs[-1])))
    for k, v in got.items():
        out[k] = v.numpy() if v.ndim else np.float64(v.item())
        out["dev/" + k] = dev(v, want[k])
        print(f"{k:12s} reference fp32 vs float64: {out['dev/' + k]:.3e}")
    assert torch.equal(head._random_feature.weight.detach(), w["W_rf"]) and torch.equal(head._random_feature.bias.detach(), w["b_rf"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; loss", loss.item(), "step losses", losses, "cond(P3)", out["cond_P3"])


if __name__ == "__main__":
    main()
