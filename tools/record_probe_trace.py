"""The libuvit calls of the probe's entry points, by name and in order: the guard of tests/test_gpu_probe_trace.py.

    python tools/record_probe_trace.py            # writes tests/golden/probe_call_trace.json (needs the GPU)

`native.lib()` returns `native._lib` when it is set, so a proxy installed there sees every symbol the Python side of the probe looks
up, the `*_ws_bytes` queries and the encoder forward included, without touching product code.  Names only: pointers, sizes and
values are what the numeric tests pin.  Every scenario runs on a fresh probe over the tiny encoder of the host tests (48 px, C = 128,
K = 10) with two batches of 3 and then 5 images, so that every buffer and store grows once (evaluate_stability: 4 and then 6 images,
whole sequences of 2 frames); the OOD loader holds one batch of 4 images.  A refactor of the Python side must leave the file as it is.
"""
import gc
import json
import os
import sys
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "probe_call_trace.json")
HEADS = ("linear", "gp", "het", "ens", "lap", "lap_fitted")
K = 10


class Recorder:
    """Forwards every attribute to the library and keeps the names asked for."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def tiny_encoder():
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    return VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=128, depth=2, num_heads=2,
                                                norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1,
                                                use_shared_rel_pos_bias=True, use_abs_pos_emb=False)


def make_probe(enc, head):
    torch.manual_seed(5)
    if head == "linear":
        from uncertainty_vit_amd.linear_probe import LinearProbe
        return LinearProbe(enc, K, init_scale=5.0)
    if head == "gp":
        from uncertainty_vit_amd.gp_probe import GPProbe
        return GPProbe(enc, K, num_inducing=64)
    if head == "het":
        from uncertainty_vit_amd.het_probe import HetProbe
        return HetProbe(enc, K, num_factors=4, test_mc_samples=16)
    if head == "ens":
        from uncertainty_vit_amd.ens_probe import EnsembleProbe
        return EnsembleProbe(enc, K, members=3, init_scale=5.0)
    from uncertainty_vit_amd.lap_probe import LaplaceProbe
    return LaplaceProbe(enc, K, init_scale=5.0)


def images(n, seed):
    return torch.randn(n, 3, 48, 48, generator=torch.Generator().manual_seed(seed)).cuda()


def labelled(sizes, seed=0):
    """The prefetcher's items: ((images, mask), labels), the labels on the host."""
    g = torch.Generator().manual_seed(100 + seed)
    return [((images(n, seed + i), None), torch.randint(0, K, (n,), generator=g)) for i, n in enumerate(sizes)]


OWN_FLAGS = {"linear": {}, "gp": {"variance": True, "mean_field": 0.5}, "het": {"variance": True}, "ens": {"members": True, "uncertainty": True},
             "lap": {"variance": True}, "lap_fitted": {"variance": True}}


def with_scores(p):
    """A density and a bank from one batch of two images of one class: the buffers of the batches that follow still grow."""
    small = [((images(2, 40), None), torch.zeros(2, dtype=torch.int64))]
    p.fit_density(small)
    p.fit_neighbours(small, k=2)


def train_steps(p):
    for (x, _), y in labelled((3, 5)):
        p.train_step(x, y.cuda(), 1e-3, 0.05, max_norm=1.0)


def conformal(p):
    p.fit_conformal(labelled((3, 5)), randomized=True)
    p.evaluate_conformal(labelled((3, 5), 7), sizes=True)


# name -> (set-up that is not recorded or None, the recorded call)
SCENARIOS = {
    "evaluate": (None, lambda p, h: p.evaluate(labelled((3, 5)))),
    "evaluate_calibration": (None, lambda p, h: p.evaluate(labelled((3, 5)), calibration=True)),
    "evaluate_detection": (with_scores, lambda p, h: p.evaluate(labelled((3, 5)), detection=True, ood_loader=[images(4, 30)], temperature=True,
                                                                calibration=True, **OWN_FLAGS[h])),
    "fit_temperature": (None, lambda p, h: p.fit_temperature(labelled((3, 5)))),
    "conformal": (None, lambda p, h: conformal(p)),
    "evaluate_stability": (None, lambda p, h: p.evaluate_stability([images(4, 20), (images(6, 21), None)], frames=2, noise=False, n_sequences=5)),
    "fit_density": (None, lambda p, h: p.fit_density(labelled((3, 5)))),
    "fit_neighbours": (None, lambda p, h: p.fit_neighbours(labelled((3, 5)), k=2)),
    "feature_scores": (with_scores, lambda p, h: [p.feature_scores(images(n, 50), distances=True) for n in (3, 5)]),
    "neighbour_scores": (with_scores, lambda p, h: [p.neighbour_scores(images(n, 50), neighbours=True) for n in (3, 5)]),
    "train_step": (None, lambda p, h: train_steps(p)),
    "fit_laplace": (None, lambda p, h: p.fit_laplace(labelled((3, 5)))),                 # the two Laplace heads only
}


def record():
    """{"head/scenario": [symbol names in call order]} on the current device."""
    from uncertainty_vit_amd import native
    torch.manual_seed(1)
    enc = tiny_encoder().cuda().eval()
    real, out = native.lib(), {}
    # an engine that an earlier caller left to the cycle collector would put its uvit_engine_destroy into whichever trace is being
    # recorded when the collector runs: collect now, and keep the collector out of the recording
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        for head in HEADS:
            for name, (setup, run) in SCENARIOS.items():
                if name == "fit_laplace" and not head.startswith("lap"):
                    continue
                p = make_probe(enc, head)
                if head == "lap_fitted":
                    p.fit_laplace(labelled((2,), 60))
                if name == "evaluate_detection":
                    p.set_temperature(1.5)
                if setup is not None:
                    setup(p)
                native._lib = rec = Recorder(real)
                try:
                    run(p, head)
                finally:
                    native._lib = real
                torch.cuda.synchronize()
                out[f"{head}/{name}"] = rec.names
    finally:
        if gc_was_on:
            gc.enable()
    return out


if __name__ == "__main__":
    trace = record()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(trace.items())) + "\n}\n")     # a scenario per line
    print(f"{len(trace)} scenarios, {sum(len(v) for v in trace.values())} calls -> {GOLDEN}")
