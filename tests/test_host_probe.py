"""CPU: the linear probe's host-side pieces -- the float64 restatement (tests/probe_ref.py) against what the reference classifier
computed (tests/golden/probe_t48.npz, written by tools/gen_golden_probe.py), the argument checks of every uvit_op_probe_* entry
point (they return before anything touches a device), the LinearProbe module's state dict, and the command line's defaults."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import probe_ref as pr

RT, AT = 2e-4, 1e-5      # fp32 round-off between two eager CPU formulations (tests/test_oracle_golden.py: activations)


@pytest.fixture(scope="module")
def case(golden_dir):
    return pr.load_fixture(golden_dir)


def close(got, ref, rtol, atol, what):
    torch.testing.assert_close(got.float(), torch.from_numpy(np.asarray(ref)).float(), rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def test_probe_ref_reproduces_reference(case):
    fx, cfg, enc, W, bias, images, labels = case
    assert bool(fx["encoder_grads_none"])                       # the reference left every encoder gradient None
    assert set(labels.tolist()) >= {0, W.shape[0] - 1}
    feat = pr.features(enc, cfg, images)
    close(feat, fx["features"], RT, AT, "features")
    logits = pr.head_logits(feat, W, bias)
    close(logits, fx["logits"], RT, AT, "logits")
    s, lr, wd = float(fx["smoothing"]), float(fx["lr"]), float(fx["weight_decay"])
    _, loss, dz = pr.smoothed_ce(logits, labels, s)
    assert float(loss) == pytest.approx(float(fx["loss"]), rel=2e-4)
    dW, db = pr.head_grads(dz, feat)
    close(dW, fx["grad/weight"], 2e-3, 2e-7, "head.weight gradient")
    close(db, fx["grad/bias"], 2e-3, 2e-7, "head.bias gradient")
    losses, _, _, (Wn, bn) = pr.train_steps(feat, W, bias, labels, s, lr, wd, int(fx["cfg"][6]))
    np.testing.assert_allclose(losses, fx["step_loss"], rtol=2e-4)
    close(Wn, fx["post/weight"], 1e-3, 2e-5, "head.weight after 3 steps")
    close(bn, fx["post/bias"], 1e-3, 2e-5, "head.bias after 3 steps")
    assert float((Wn.float() - W).abs().max()) > 1e-3           # three steps of lr 1e-3 did move the head


def test_smoothed_ce_gradient_is_the_autograd_gradient():
    g = torch.Generator().manual_seed(5)
    z = torch.randn(6, 11, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.tensor([0, 10, 3, 3, 7, 1])
    for s in (0.0, 0.1):
        _, loss, dz = pr.smoothed_ce(z, y, s)
        (auto,) = torch.autograd.grad(loss, z)
        torch.testing.assert_close(dz, auto, rtol=1e-12, atol=1e-14)
        if s == 0.0:
            assert float(loss) == pytest.approx(float(torch.nn.functional.cross_entropy(z, y)), rel=1e-12)


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE = -1, -2


def f(v):
    return C.c_float(v)


def test_pool_norm_rejects_bad_arguments(L):
    assert L.uvit_op_probe_pool_ws_bytes(128, 197, 768) == 128 * 8 * 768 * 4
    for B, N, Cd in ((0, 197, 768), (4, 1, 768), (4, 197, 770), (4, 197, 0), (4, 197, 2052), (-1, 2, 64), (65536, 2, 64)):
        assert L.uvit_op_probe_pool_ws_bytes(B, N, Cd) == SHAPE, (B, N, Cd)
        assert L.uvit_op_probe_pool_norm(P1, P1, P1, B, N, Cd, f(1e-6), NUL) == SHAPE, (B, N, Cd)
    for x, feat, scratch in ((NUL, P1, P1), (P1, NUL, P1), (P1, P1, NUL)):
        assert L.uvit_op_probe_pool_norm(x, feat, scratch, 4, 197, 768, f(1e-6), NUL) == ARG


def test_logits_rejects_bad_arguments(L):
    for B, K, Cd in ((0, 10, 64), (4, 0, 64), (4, 10, 66), (4, 10, 0), (-3, 10, 64), (4, -1, 64)):
        assert L.uvit_op_probe_logits(P1, P1, P1, P1, B, K, Cd, NUL) == SHAPE, (B, K, Cd)
    for i in range(4):
        a = [P1] * 4
        a[i] = NUL
        assert L.uvit_op_probe_logits(*a, 4, 10, 64, NUL) == ARG, i


def test_ce_rejects_bad_arguments(L):
    for B, K in ((0, 10), (4, 0), (-1, 10), (4, -5)):
        assert L.uvit_op_probe_ce(P1, P1, f(0.1), P1, P1, P1, P1, B, K, NUL) == SHAPE, (B, K)
    # logits, labels, row_loss and loss_out are required; dlogits and the counters may be NULL (tested on the GPU)
    for i in (0, 1, 3, 4):
        a = [P1, P1, P1, P1, P1, P1]                # logits, labels, dlogits, row_loss, loss_out, counters
        a[i] = NUL
        assert L.uvit_op_probe_ce(a[0], a[1], f(0.1), a[2], a[3], a[4], a[5], 4, 10, NUL) == ARG, i
    for s in (-0.1, 1.0, float("nan")):
        assert L.uvit_op_probe_ce(P1, P1, f(s), P1, P1, P1, P1, 4, 10, NUL) == ARG, s


def test_head_grad_rejects_bad_arguments(L):
    for B, K, Cd in ((0, 10, 64), (4, 0, 64), (4, 10, 62), (4, 10, 0), (-2, 10, 64)):
        assert L.uvit_op_probe_head_grad(P1, P1, P1, P1, B, K, Cd, NUL) == SHAPE, (B, K, Cd)
    for i in range(4):
        a = [P1] * 4
        a[i] = NUL
        assert L.uvit_op_probe_head_grad(*a, 4, 10, 64, NUL) == ARG, i


# ---- the module ----
def tiny_encoder(two_stream=False):
    from uncertainty_vit_amd.modeling_cyclical import DistVisionTransformerForCyclicalTraining, VisionTransformerForCyclicalTraining
    cls = DistVisionTransformerForCyclicalTraining if two_stream else VisionTransformerForCyclicalTraining
    return cls(img_size=48, patch_size=16, embed_dim=128, depth=2, num_heads=2, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
               init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)


def test_linear_probe_state_dict_and_init():
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    torch.manual_seed(3)
    probe = LinearProbe(tiny_encoder().eval(), 10)
    sd = probe.state_dict()
    assert list(sd) == ["head.weight", "head.bias"]
    assert tuple(sd["head.weight"].shape) == (10, 128) and tuple(sd["head.bias"].shape) == (10,)
    assert [n for n, _ in probe.named_parameters()] == ["head.weight", "head.bias"]
    # modeling_finetune.py:439-441: trunc-normal std 0.02 times init_scale 0.001, bias zero
    w = sd["head.weight"]
    assert float(sd["head.bias"].abs().max()) == 0.0
    assert 0.5 * 2e-5 < float(w.std()) < 1.5 * 2e-5 and float(w.abs().max()) < 2e-3
    # the parameters are views of one arena laid out [W | bias | pad to 4] whose decay group is W
    assert probe._arena.numel() == 10 * 128 + 12 and probe._n_decay == 10 * 128
    assert sd["head.weight"].data_ptr() == probe._arena.data_ptr()
    assert sd["head.bias"].data_ptr() == probe._arena.data_ptr() + 4 * 10 * 128
    # loading the reference's keys goes through the views
    probe.load_state_dict({"head.weight": torch.full((10, 128), 0.5), "head.bias": torch.arange(10.0)})
    assert float(probe._arena[:1280].min()) == 0.5 and probe._arena[1280:1290].tolist() == list(range(10))
    # no CPU fallback
    with pytest.raises(UvitError):
        probe.logits(torch.zeros(2, 3, 48, 48))
    with pytest.raises(UvitError):
        probe.train_step(torch.zeros(2, 3, 48, 48), torch.zeros(2, dtype=torch.int64), 1e-3, 0.05)


def test_linear_probe_rejects_what_is_not_built():
    from uncertainty_vit_amd.linear_probe import LinearProbe
    with pytest.raises(NotImplementedError):
        LinearProbe(tiny_encoder(two_stream=True).eval(), 10)
    with pytest.raises(ValueError):
        LinearProbe(tiny_encoder().train(), 10)             # the encoder must be frozen in eval mode
    with pytest.raises(ValueError):
        LinearProbe(tiny_encoder().eval(), 0)


def test_truncated_encoder_loads_only_its_blocks():
    """--target_layer L: the encoder has L + 1 blocks and takes only their entries of the checkpoint."""
    from uncertainty_vit_amd.linear_probe import load_encoder_checkpoint
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    full = tiny_encoder()
    cut = VisionTransformerForCyclicalTraining(**{**full._ctor, "depth": 1}).eval()
    left = load_encoder_checkpoint(cut, {"model": full.state_dict(), "epoch": 3}, "model|module", "")
    assert left and all(k.startswith("blocks.1.") for k in left)
    for k, v in cut.state_dict().items():
        assert torch.equal(v, full.state_dict()[k]), k
    with pytest.raises(KeyError):
        load_encoder_checkpoint(full, {"model": cut.state_dict()}, "model|module", "")     # a shallower checkpoint lacks blocks.1


def test_cli_defaults_equal_the_reference():
    """Defaults of the flags run_linear_probe.py shares with the reference's run_class_finetuning.py:51-204, as literals."""
    import run_linear_probe
    ref = dict(batch_size=64, epochs=30, model="deit_base_patch16_224", input_size=224, clip_grad=None, weight_decay=0.05, lr=5e-4,
               min_lr=1e-6, warmup_epochs=5, smoothing=0.1, finetune="", model_key="model|module", model_prefix="", target_layer=-1,
               data_path="/datasets01/imagenet_full_size/061417/", eval_data_path=None, nb_classes=0,
               imagenet_default_mean_and_std=False, data_set="IMNET", output_dir="", seed=0, resume="", eval=False, num_workers=0)
    got = vars(run_linear_probe.get_args([]))
    assert got == ref
    a = run_linear_probe.get_args(["--model", "beit_base_patch16_224", "--finetune", "c.pth", "--data_set", "image_folder", "--data_path",
                                   "d", "--nb_classes", "100", "--target_layer", "7", "--eval", "--clip_grad", "1.0"])
    assert (a.nb_classes, a.target_layer, a.eval, a.clip_grad, a.data_set) == (100, 7, True, 1.0, "image_folder")
