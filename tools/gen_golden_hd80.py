"""Generate the head_dim-80 (ViT-H) fixtures by running the UNMODIFIED reference through tools/ref_harness.py, as
tools/gen_golden.py does (whose fixtures this leaves alone).  Build-container only; never runs on the GPU box.

    python tools/gen_golden_hd80.py

  tests/golden/model_hd80.npz    a head_dim-80 model (img 48, embed 320, 4 heads, depth 2, shared relative-position bias) with
                                 closed-form weights: forward return modes and three training steps, in model_t48.npz's format.
                                 (embed 320 rather than 160: the engine needs embed_dim % 64 == 0.)
  tests/golden/huge_layout.json  names, shapes and order of the reference ViT-H/16 state dict (built with the arguments of
                                 modeling_cyclical.py:346-363 -- the entry point itself raises under create_model), its
                                 parameter count and its optimizer weight-decay groups (optim_factory.py:58-97)
"""
import json
import os
import sys
from functools import partial
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402
import ref_harness  # noqa: E402


def gen_huge_layout(mc):
    model = mc.VisionTransformerForCyclicalTraining(
        patch_size=16, embed_dim=1280, depth=32, num_heads=16, mlp_ratio=4, qkv_bias=True,
        norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1, use_shared_rel_pos_bias=True,
        use_abs_pos_emb=False, drop_path_rate=0.25, attn_drop_rate=0.05)
    import optim_factory
    args = SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=(0.9, 0.999), momentum=0.9)
    opt = optim_factory.create_optimizer(args, model)
    names = {id(p): n for n, p in model.named_parameters()}
    groups = {("decay" if g["weight_decay"] > 0 else "no_decay"): [names[id(p)] for p in g["params"]] for g in opt.param_groups}
    out = {"state_dict": [[k, list(v.shape)] for k, v in model.state_dict().items()],
           "n_params": sum(p.numel() for p in model.parameters()),
           "groups": groups}
    with open(os.path.join(gen_golden.OUT, "huge_layout.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("wrote huge_layout.json", out["n_params"], "params")


def main():
    torch.set_num_threads(8)
    mc, eng = ref_harness.import_reference()
    gen_huge_layout(mc)
    gen_golden.gen_model_case(mc, eng, "hd80", img=48, dim=320, depth=2, heads=4, init_values=0.1, B=3, n_mask=4, seed=5)


if __name__ == "__main__":
    main()
