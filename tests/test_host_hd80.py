"""CPU (no GPU): the head_dim-80 / ViT-H/16 surface -- registry entry, arena layout and optimizer groups against the reference's
ViT-H state dict (tests/golden/huge_layout.json), the shapes the engine refuses, and the oracle's head_dim-80 arithmetic against
the reference itself (tests/golden/model_hd80.npz; both written by tools/gen_golden_hd80.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from golden_util import check_entry, entries
from oracle import vit_oracle as vo
from oracle.closed_form import closed_form_images, closed_form_state, exact_masks

RT, AT = 2e-4, 1e-5   # as test_oracle_golden.py


@pytest.fixture(scope="module")
def native():
    from uncertainty_vit_amd import native as n
    n.build()
    return n


def huge_cfg(native, two_stream=0, embed=1280, heads=16):
    cfg = native.Config(224, 16, 3, embed, 32, heads, 4 * embed, 1, 0, 128, 1e-6, 0.05, 0.25, 0)
    cfg.two_stream = two_stream
    return cfg


def test_create_model_beit_huge(native):
    from uncertainty_vit_amd import modeling_cyclical as mc
    assert "beit_huge_patch16_224" in mc.__all__
    m = mc.create_model("beit_huge_patch16_224", drop_path_rate=0.25, attn_drop_rate=0.05, init_values=0.1,
                        use_shared_rel_pos_bias=True, use_abs_pos_emb=False, num_classes=0)
    assert (m.embed_dim, m.depth, m.num_heads, m.mlp_hidden) == (1280, 32, 16, 5120)
    ref = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "huge_layout.json")))
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref["state_dict"]
    assert sum(p.numel() for p in m.parameters()) == ref["n_params"] == 632_359_872
    from uncertainty_vit_amd.optim_factory import ArenaAdamW
    opt = ArenaAdamW(m, lr=1e-3, weight_decay=0.05)
    assert opt.group_names["decay"] == ref["groups"]["decay"]
    assert opt.group_names["no_decay"] == ref["groups"]["no_decay"]


def test_huge_arena_layout_matches_reference(native, golden_dir):
    L = native.lib()
    cfg = huge_cfg(native)
    ref = json.load(open(os.path.join(golden_dir, "huge_layout.json")))
    # the reference's float tensors, in state-dict order (the int64 relative_position_index buffer is not in the arena)
    want = [(n, tuple(s)) for n, s in ref["state_dict"] if not n.endswith("relative_position_index")]
    got = []
    for i in range(L.uvit_layout_count(C.byref(cfg))):
        e = native.LayoutEntry()
        assert L.uvit_layout_get(C.byref(cfg), i, C.byref(e)) == 0
        got.append((e.name.decode(), tuple(e.shape[: e.ndim]), e.decay))
    assert sorted((n, s) for n, s, _ in got) == sorted(want)
    assert sum(int(np.prod(s)) for _, s, _ in got) == ref["n_params"]
    assert {n for n, _, d in got if d == 1} == set(ref["groups"]["decay"])
    assert {n for n, _, d in got if d == 0} == set(ref["groups"]["no_decay"])
    nd = C.c_int64()
    assert L.uvit_arena_numel(C.byref(cfg), C.byref(nd)) >= ref["n_params"]


def test_head_dim_80_limits(native):
    L = native.lib()
    # head_dim 80 is the base model's only; the two-stream kernels are specialised for 64
    assert L.uvit_layout_count(C.byref(huge_cfg(native))) > 0
    assert L.uvit_layout_count(C.byref(huge_cfg(native, two_stream=1))) == -2          # UVIT_ERR_SHAPE
    for embed, heads in ((768, 16), (1536, 16)):          # head_dim 48, 96
        assert L.uvit_layout_count(C.byref(huge_cfg(native, embed=embed, heads=heads))) == -2
    from functools import partial
    from uncertainty_vit_amd.modeling_cyclical import DistVisionTransformerForCyclicalTraining, VisionTransformerForCyclicalTraining
    args = dict(img_size=48, patch_size=16, depth=2, mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    m = VisionTransformerForCyclicalTraining(embed_dim=320, num_heads=4, **args)
    assert m.embed_dim // m.num_heads == 80
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        DistVisionTransformerForCyclicalTraining(embed_dim=320, num_heads=4, **args)
    for embed, heads in ((96, 2), (192, 2)):              # head_dim 48, 96
        with pytest.raises(NotImplementedError, match="head_dim 64 or 80"):
            VisionTransformerForCyclicalTraining(embed_dim=embed, num_heads=heads, **args)


def load_hd80(golden_dir):
    fx = np.load(os.path.join(golden_dir, "model_hd80.npz"))
    img, dim, depth, heads, B, n_mask, steps = [int(v) for v in fx["cfg"]]
    cfg = vo.VitConfig(img_size=img, embed_dim=dim, depth=depth, num_heads=heads, init_values=float(fx["init_values"]))
    assert cfg.head_dim == 80
    params = closed_form_state(vo.param_shapes(cfg), gamma=cfg.init_values)
    return fx, cfg, params, B, n_mask, steps


def test_oracle_hd80_forward_modes(golden_dir):
    fx, cfg, p, B, n_mask, _ = load_hd80(golden_dir)
    x = closed_form_images("hd80/0", B, cfg.img_size)
    mask = torch.from_numpy(fx["mask0"])
    assert torch.equal(mask, exact_masks(B, cfg.num_patches, n_mask, int(fx["mask_seed"])))
    ends = vo.forward(p, cfg, x, None, True, "end")
    fcs = vo.forward(p, cfg, x, None, True, "fc")
    for i in range(cfg.depth):
        check_entry(fx, f"fwd/end{i}", ends[i], RT, AT)
        check_entry(fx, f"fwd/fc{i}", fcs[i], RT, AT)
    check_entry(fx, "fwd/student_masked", vo.forward(p, cfg, x, mask, False), RT, AT)
    check_entry(fx, "fwd/student_all", vo.forward(p, cfg, x, mask, True), RT, AT)


def test_oracle_hd80_train_steps(golden_dir):
    fx, cfg, p, B, n_mask, steps = load_hd80(golden_dir)
    hp = vo.StepHParams(target_layers=tuple(int(v) for v in fx["target_layers"]))
    ema = {k: v.clone() for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(t) for k, t in p.items()}
    for s in range(steps):
        x = closed_form_images(f"hd80/{s}", B, cfg.img_size)
        res = vo.train_step(p, ema, m, v, cfg, hp, x, torch.from_numpy(fx[f"mask{s}"]), s + 1)
        assert res.loss == pytest.approx(float(fx["step/loss"][s]), rel=2e-4)
        assert res.grad_norm == pytest.approx(float(fx["step/grad_norm"][s]), rel=2e-3)
        if s == 0:
            names = entries(fx, "grad0")
            assert set(names) == set(res.grads.keys())
            for n in names:
                check_entry(fx, "grad0/" + n, res.grads[n], 2e-3, 2e-7)
    for n in entries(fx, "post"):
        check_entry(fx, "post/" + n, p[n], 1e-3, 2e-5)
    for n in entries(fx, "ema"):
        check_entry(fx, "ema/" + n, ema[n], 1e-5, 1e-7)
