"""Generate tests/golden/probe_t48.npz by running the UNMODIFIED reference classifier (modeling_finetune.VisionTransformer with
linear_classifier=True, imported from the reference checkout through tools/ref_harness.py).  Build-container only; never runs on
the GPU box.

    python tools/gen_golden_probe.py

The fixture is data only: seeded weights, 4 images and labels, and what the reference computes from them -- forward_features,
logits, the smoothing-0.1 loss, the head gradients and the head after three torch.optim.AdamW steps.  The encoder weights carry the
pre-training model's key names (the classifier shares them).  To stay small, the large tensors lie on an 8-bit grid and are stored
as int8 plus one fp32 scale (`encq/<name>`, `encs/<name>`: value = float32(q) * scale, exactly what the reference model was given);
the images lie on a 1/64 grid and are stored as float16, exactly.
"""
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "probe_t48.npz")
IMG, DIM, DEPTH, HEADS, K, B = 48, 128, 2, 2, 10, 4
SMOOTHING, LR, WD, STEPS = 0.1, 1e-3, 0.05, 3


def seeded_weights(model, gen):
    """name -> (fp32 tensor, int8 grid or None, scale) for every encoder parameter of the classifier."""
    out = {}
    for name, p in model.named_parameters():
        if name.startswith("head."):
            continue
        r = torch.randn(p.shape, generator=gen)
        if p.ndim >= 2 and p.numel() > 4096:
            q = torch.clamp(torch.round(r * 40.0), -127, 127).to(torch.int8)
            scale = np.float32(0.03 / 40.0)
            out[name] = (q.float() * float(scale), q, scale)
            continue
        if "norm" in name and name.endswith("weight"):
            t = 1.0 + 0.1 * r
        elif "gamma" in name:
            t = 0.1 * (1.0 + 0.5 * torch.tanh(r))
        elif name.endswith("relative_position_bias_table"):
            t = 0.05 * r                                 # non-zero, so that a bias bug cannot hide
        elif name.endswith("bias"):
            t = 0.01 * r
        else:
            t = 0.03 * r
        out[name] = (t.float(), None, None)
    return out


def smoothed_ce(logits, target, smoothing):
    """timm.loss.LabelSmoothingCrossEntropy.forward, restated (timm is not installed): three lines."""
    logprobs = torch.nn.functional.log_softmax(logits, dim=-1)
    nll_loss = -logprobs.gather(dim=-1, index=target.unsqueeze(1)).squeeze(1)
    smooth_loss = -logprobs.mean(dim=-1)
    return ((1.0 - smoothing) * nll_loss + smoothing * smooth_loss).mean()


def main():
    ref_harness.install()
    import modeling_finetune as mf
    gen = torch.Generator().manual_seed(20240)
    torch.manual_seed(20240)
    model = mf.VisionTransformer(img_size=IMG, patch_size=16, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, mlp_ratio=4, qkv_bias=True,
                                 norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1, use_shared_rel_pos_bias=True,
                                 use_abs_pos_emb=False, use_mean_pooling=True, linear_classifier=True, num_classes=K)
    enc = seeded_weights(model, gen)
    head_w = 0.05 * torch.randn(K, DIM, generator=gen)
    head_b = 0.01 * torch.randn(K, generator=gen)
    sd = {n: v[0] for n, v in enc.items()}
    sd["head.weight"], sd["head.bias"] = head_w.clone(), head_b.clone()
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("relative_position_index") for k in missing), (missing, unexpected)
    # run_class_finetuning.py:529-538: with --linear_classifier every weight the checkpoint provides is frozen
    for n, p in model.named_parameters():
        if n in enc:
            p.requires_grad_(False)
    assert [n for n, p in model.named_parameters() if p.requires_grad] == ["head.weight", "head.bias"]
    model.eval()

    images = (torch.clamp(torch.round(torch.randn(B, 3, IMG, IMG, generator=gen) * 64.0), -256, 256) / 64.0).float()
    labels = torch.tensor([0, K - 1, 3, 6], dtype=torch.int64)
    out = {"cfg": np.array([IMG, DIM, DEPTH, HEADS, K, B, STEPS], dtype=np.int64), "init_values": np.float64(0.1),
           "smoothing": np.float64(SMOOTHING), "lr": np.float64(LR), "weight_decay": np.float64(WD),
           "images": images.numpy().astype(np.float16), "labels": labels.numpy()}
    assert np.array_equal(out["images"].astype(np.float32), images.numpy())
    for n, (t, q, scale) in enc.items():
        if q is None:
            out["enc/" + n] = t.numpy()
        else:
            out["encq/" + n], out["encs/" + n] = q.numpy(), scale
            assert np.array_equal(q.numpy().astype(np.float32) * scale, t.numpy())
    out["head/weight"], out["head/bias"] = head_w.numpy(), head_b.numpy()

    feats = model.forward_features(images)
    logits = model(images)
    loss = smoothed_ce(logits, labels, SMOOTHING)
    loss.backward()
    out["features"], out["logits"], out["loss"] = feats.detach().numpy(), logits.detach().numpy(), np.float64(loss.item())
    out["grad/weight"], out["grad/bias"] = model.head.weight.grad.numpy().copy(), model.head.bias.grad.numpy().copy()
    enc_grads = [n for n, p in model.named_parameters() if n in enc and p.grad is not None]
    out["encoder_grads_none"] = np.bool_(not enc_grads)
    assert not enc_grads, enc_grads

    opt = torch.optim.AdamW([{"params": [model.head.weight], "weight_decay": WD}, {"params": [model.head.bias], "weight_decay": 0.0}],
                            lr=LR, betas=(0.9, 0.999), eps=1e-8)
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        step_loss = smoothed_ce(model(images), labels, SMOOTHING)
        step_loss.backward()
        opt.step()
        losses.append(step_loss.item())
    out["step_loss"] = np.array(losses, dtype=np.float64)
    out["post/weight"], out["post/bias"] = model.head.weight.detach().numpy(), model.head.bias.detach().numpy()
    for n, (t, _, _) in enc.items():
        assert torch.equal(dict(model.named_parameters())[n].detach(), t), n       # the frozen encoder did not move
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; loss", loss.item(), "step losses", losses)


if __name__ == "__main__":
    main()
