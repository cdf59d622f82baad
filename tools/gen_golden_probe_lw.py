"""Generate tests/golden/probe_lw_t48.npz by running the UNMODIFIED reference classifier (modeling_finetune.VisionTransformer with
linear_classifier=True, learn_layer_weights=True, imported from the reference checkout through tools/ref_harness.py).  Build-container
only; never runs on the GPU box.

    python tools/gen_golden_probe_lw.py

The fixture is data only and stores no encoder weight: the encoder, the head, the images and the labels are those of
tests/golden/probe_t48.npz, taken from it by name.  Per combination c = 2 use_cls + layernorm_before_combine it holds, under `c<c>/`, what
the reference computes from them with `layer_log_weights` seeded away from zero: forward_features, logits, the smoothing-0.1 loss, the
three gradients, and the three parameters after three torch.optim.AdamW steps with `layer_log_weights` in the no-decay group (a
one-dimensional parameter: optim_factory.get_parameter_groups).
"""
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness  # noqa: E402
from gen_golden_probe import smoothed_ce  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "probe_lw_t48.npz")
LOG_W = [0.7, -0.4]          # depth 2: softmax = (0.750, 0.250)
COMBOS = [(False, False), (False, True), (True, False), (True, True)]      # (use_cls, layernorm_before_combine)
STEPS = 3


def main():
    import probe_ref as pr
    ref_harness.install()
    import modeling_finetune as mf
    fx, cfg, enc, W, bias, images, labels = pr.load_fixture(os.path.join(ROOT, "tests", "golden"))
    smoothing, lr, wd = float(fx["smoothing"]), float(fx["lr"]), float(fx["weight_decay"])
    assert cfg.depth == len(LOG_W)
    out = {"layer_log_weights": np.array(LOG_W, dtype=np.float32), "combos": np.array(COMBOS, dtype=np.int64), "steps": np.int64(STEPS)}
    for c, (use_cls, ln) in enumerate(COMBOS):
        torch.manual_seed(20240 + c)
        model = mf.VisionTransformer(img_size=cfg.img_size, patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                                     mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                                     init_values=float(fx["init_values"]), use_shared_rel_pos_bias=True, use_abs_pos_emb=False,
                                     use_mean_pooling=not use_cls, linear_classifier=True, num_classes=W.shape[0],
                                     learn_layer_weights=True, layernorm_before_combine=ln)
        sd = {n: v.clone() for n, v in enc.items()}
        sd["head.weight"], sd["head.bias"] = W.clone(), bias.clone()
        sd["layer_log_weights"] = torch.tensor(LOG_W, dtype=torch.float32)
        missing, unexpected = model.load_state_dict(sd, strict=False)
        # without mean pooling the classifier owns a final `norm` that the layer-weight path never calls (modeling_finetune.py:499-510)
        assert not unexpected and all(k.endswith("relative_position_index") or k.startswith("norm.") for k in missing), (missing, unexpected)
        trained = ["head.weight", "head.bias", "layer_log_weights"]
        params = dict(model.named_parameters())
        for n, p in params.items():
            p.requires_grad_(n in trained)
        model.eval()

        feats = model.forward_features(images)
        logits = model(images)
        loss = smoothed_ce(logits, labels, smoothing)
        loss.backward()
        key = f"c{c}/"
        out[key + "features"], out[key + "logits"], out[key + "loss"] = feats.detach().numpy(), logits.detach().numpy(), np.float64(loss.item())
        out[key + "grad/weight"], out[key + "grad/bias"] = model.head.weight.grad.numpy().copy(), model.head.bias.grad.numpy().copy()
        out[key + "grad/layer_log_weights"] = model.layer_log_weights.grad.numpy().copy()

        opt = torch.optim.AdamW([{"params": [model.head.weight], "weight_decay": wd},
                                 {"params": [model.head.bias, model.layer_log_weights], "weight_decay": 0.0}],
                                lr=lr, betas=(0.9, 0.999), eps=1e-8)
        losses = []
        for _ in range(STEPS):
            opt.zero_grad()
            step_loss = smoothed_ce(model(images), labels, smoothing)
            step_loss.backward()
            opt.step()
            losses.append(step_loss.item())
        out[key + "step_loss"] = np.array(losses, dtype=np.float64)
        out[key + "post/weight"], out[key + "post/bias"] = model.head.weight.detach().numpy().copy(), model.head.bias.detach().numpy().copy()
        out[key + "post/layer_log_weights"] = model.layer_log_weights.detach().numpy().copy()
        for n, t in enc.items():
            assert torch.equal(params[n].detach(), t), n       # the frozen encoder did not move
        print(f"combo {c} use_cls={use_cls} layernorm={ln}: loss {loss.item():.6f}, step losses {losses}, "
              f"dlog_w {out[key + 'grad/layer_log_weights']}, log_w after {out[key + 'post/layer_log_weights']}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
