"""GPU: a model and its native engine form no reference cycle.  The model owns the engine (`model._engine`) and the engine points
back at its model only weakly, so dropping the last reference to a model frees the engine -- parameter shadows and workspace, tens
of GB at ViT-H bs=128 -- at once, not when Python's cycle collector next runs.  The linear probe builds frozen encoders beside the
pre-training models of a process (and its tests beside the full-size step tests of the suite); with a cycle, every dropped model kept
its engine's buffers until the collector happened to run."""
import gc
import weakref
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu


def tiny_model():
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    return VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=128, depth=2, num_heads=2,
                                                norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1,
                                                use_shared_rel_pos_bias=True, use_abs_pos_emb=False).cuda().eval()


def test_dropping_the_model_frees_its_engine_without_the_cycle_collector():
    gc.collect()
    gc.disable()
    try:
        model = tiny_model()
        engine = model.forward_features(torch.zeros(2, 3, 48, 48, device="cuda"), None, None)
        assert engine is model._engine and engine.model is model      # the back reference still resolves while the model lives
        torch.cuda.synchronize()
        dead, workspace = weakref.ref(engine), weakref.ref(engine.workspace)
        del engine
        assert dead() is not None                                      # the model keeps its engine alive
        del model
        assert dead() is None and workspace() is None                  # reference counting alone let go of engine and workspace
    finally:
        gc.enable()


def test_probe_keeps_its_encoder_and_engine_alive():
    from uncertainty_vit_amd.linear_probe import LinearProbe
    probe = LinearProbe(tiny_model(), 10)             # the probe holds the only reference to the encoder
    gc.collect()
    a = probe.logits(torch.zeros(2, 3, 48, 48, device="cuda"))
    gc.collect()
    assert probe.encoder._engine.model is probe.encoder
    assert torch.equal(a, probe.logits(torch.zeros(2, 3, 48, 48, device="cuda")))
