"""What run_linear_probe.main prints, writes and calls, per command line: the guard of tests/test_gpu_probe_cli_transcript.py.

    python tools/record_probe_cli.py                       # writes tests/golden/probe_cli_transcript.json (masked; needs the GPU)
    python tools/record_probe_cli.py --raw FILE [--timing] # the unmasked record, for a digit-for-digit comparison of two commits

A scenario is one or two `main()` calls on generated data.  Per call the record holds the printed lines, the keys of every line of
log.txt in their order (`key` for a number, else `key: kind`), the sorted file names of --output_dir, the keys of the returned stats
(one level into its dicts) and the libuvit calls as tools/record_probe_trace.py's Recorder sees them: the count per name and a SHA-256
of the sequence.  The `Namespace(...)` line, MetricLogger's progress lines and `Training time` are dropped, the temporary root reads
`<root>` and the augmentation's repr in a loader's line `<augment>`; in the committed form every whitespace-separated token that
float() accepts once `()[],:` are stripped from its ends reads `#`, so that the golden pins the lines, their order and their wording,
not the digits.  A refactor of the command line must leave the file as it is.

The base encoder is the one tests/test_gpu_lw_cli.py registers (embed 128, depth 3, 2 heads, 48 px: three blocks are the fewest at
which --learn_layer_weights and --mc_dropout_layers 2 differ from the other heads) on the 10-class folder of 200 images of
tests/test_gpu_lap_cli.py in batches of 50; the two-stream head runs on the model and folders of tests/test_gpu_dist_probe_cli.py.
--knn_k 2 and --vim_dim 8 keep the two fits small; nothing had to be left out of a scenario because the command line refused it.
"""
import argparse
import contextlib
import gc
import hashlib
import io
import json
import os
import re
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "probe_cli_transcript.json")
MODEL = "lw_cli_tiny_patch16_48"
AUGMENT = re.compile(r"BEiTAugment\(.*\)\)")
HEAD_FLAGS = {
    "linear": [],
    "gp": ["--gp_layer", "--gp_cov_momentum", "-1"],
    "het": ["--het_layer", "--het_num_factors", "4"],
    "ens": ["--ensembles", "--ens_members", "3", "--ens_bagging"],
    "lap": ["--laplace", "--lap_data_path", "{data}"],
    "mcd": ["--mc_dropout_forwards", "3", "--attn_drop_rate", "0.1", "--mc_dropout_layers", "2"],
    "lw": ["--learn_layer_weights", "--use_cls"],
    "dist": [],
}
BASE = ["--model", MODEL, "--input_size", "48", "--finetune", "{pre}", "--data_set", "image_folder", "--data_path", "{data}",
        "--eval_data_path", "{data}", "--nb_classes", "10", "--batch_size", "50"]
DIST_BASE = ["--model", "dist_beit_base_patch16_224", "--finetune", "{dist_pre}", "--data_set", "image_folder", "--data_path", "{dist_train}",
             "--eval_data_path", "{dist_val}", "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--clip_grad", "1.0"]
TRAIN = ["--epochs", "1", "--warmup_epochs", "0", "--lr", "0.01", "--calibration", "--set_calibration", "--output_dir", "{out}"]
FAMILIES = ["--eval", "--resume", "{head}", "--calibration", "--set_calibration", "--detection", "--ood_data_path", "{ood}",
            "--cp_data_path", "{data}", "--cp_alpha", "0.1", "0.2"]


def _head(name):
    base = DIST_BASE if name == "dist" else BASE
    return [base + HEAD_FLAGS[name] + TRAIN,
            base + HEAD_FLAGS[name] + ["--resume", "{out}/probe-0.pth", "--eval", "--calibration", "--detection", "--output_dir", "{out}/eval"]]


def _corruptions(head_flags, resume):
    return ["--eval", "--resume", resume, "--corruptions", "brightness", "gaussian_noise", "--corruption_severities", "1", "3",
            "--calibration", "--set_calibration", "--detection", "--output_dir", "{out}/eval"] + head_flags


# name -> the argv of its main() calls; {out} is the scenario's own empty folder, {out}/eval a second one
FITS = ["--ts_data_path", "{data}", "--maha_data_path", "{data}", "--knn_data_path", "{data}", "--knn_k", "2", "--vim_data_path", "{data}",
        "--vim_dim", "8"]
SCENARIOS = {f"head_{name}": _head(name) for name in HEAD_FLAGS}
SCENARIOS.update({
    "all_families_linear": [BASE + FAMILIES + FITS + ["--output_dir", "{out}"]],
    # the saved fits come from a first call that also fits the Laplace factors: laplace.pth belongs to the head it was fitted on
    "all_families_saved": [
        BASE + FAMILIES + FITS + ["--laplace", "--lap_data_path", "{data}", "--output_dir", "{out}"],
        BASE + FAMILIES + ["--ts_temperature", "1.5", "--maha_state", "{out}/density.pth", "--knn_state", "{out}/neighbours.pth",
                           "--vim_state", "{out}/vim.pth", "--laplace", "--lap_state", "{out}/laplace.pth", "--output_dir", "{out}/eval"]],
    "gp_mean_field": [
        BASE + ["--gp_layer"] + TRAIN,
        BASE + ["--gp_layer", "--gp_mean_field", "0.5", "--eval", "--resume", "{out}/probe-0.pth", "--ts_data_path", "{data}",
                "--cp_data_path", "{data}", "--perturbation_path", "{pert}", "--output_dir", "{out}/eval"]],
    "corruptions_linear": [BASE + _corruptions([], "{head}")],
    "corruptions_gp": [BASE + ["--gp_layer"] + TRAIN, BASE + _corruptions(["--gp_layer"], "{out}/probe-0.pth")],
})
TIMED = {"eval_all_families": ("all_families_linear", 0), "train_epoch_linear": ("head_linear", 0)}


def _tiny(pretrained=False, **kwargs):
    from uncertainty_vit_amd.modeling_cyclical import _build
    return _build(pretrained, kwargs, embed_dim=128, depth=3, num_heads=2)


def make_inputs(root, make=True):
    """The folders and checkpoints every scenario reads, drawn from fixed seeds: {placeholder: path}."""
    from test_gpu_dist_probe_cli import _two_stream_checkpoint
    from test_gpu_lap_cli import _image_tree
    from test_gpu_probe_cli import _image_tree as _small_tree
    p = {k: os.path.join(root, v) for k, v in dict(data="data", ood="ood", pert="pert", pre="checkpoint-0.pth", head="head-0.pth",
                                                   dist_train="dist_train", dist_val="dist_val", dist_pre="dist-checkpoint-0.pth").items()}
    if not make:
        return p
    _image_tree(p["data"])
    _small_tree(p["ood"], 8)
    _small_tree(p["dist_train"], 12)
    _small_tree(p["dist_val"], 6)
    _two_stream_checkpoint(p["dist_pre"])
    os.makedirs(p["pert"])
    rng = np.random.default_rng(29)
    for name in ("gaussian_noise", "shift"):
        np.save(os.path.join(p["pert"], name + ".npy"), rng.integers(0, 256, (4, 3, 48, 48, 3), dtype=np.uint8))
    torch.manual_seed(5)
    m = _tiny(img_size=48, init_values=0.1, use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    args = SimpleNamespace(rel_pos_bias=True, abs_pos_emb=False, layer_scale_init_value=0.1)
    torch.save({"model": m.state_dict(), "optimizer": {}, "epoch": 0, "scaler": {}, "args": args}, p["pre"])
    w, b = 0.05 * torch.randn(10, 128), 0.1 * torch.randn(10)
    zeros = {"head.weight": torch.zeros(10, 128), "head.bias": torch.zeros(10)}
    torch.save({"model": {"head.weight": w, "head.bias": b}, "optimizer": {"step": 0, "exp_avg": zeros, "exp_avg_sq": zeros}, "epoch": 0}, p["head"])
    return p


def _kind(v):
    if isinstance(v, bool) or v is None:
        return repr(v)
    if isinstance(v, (int, float)):
        return "number"
    if isinstance(v, str):
        return "string"
    if isinstance(v, (list, tuple)):
        return f"list of {len(v)}"
    return type(v).__name__


def _stats_keys(stats):
    return {str(k): sorted(str(i) for i in v) if isinstance(v, dict) else None for k, v in stats.items()}


def run_call(rlp, argv, root):
    """One main() call under the recorder: its record, unmasked, and its wall time."""
    from record_probe_trace import Recorder
    from uncertainty_vit_amd import native
    args = rlp.get_args(argv)
    if args.output_dir:
        os.makedirs(args.output_dir, exist_ok=True)
    log = os.path.join(args.output_dir, "log.txt") if args.output_dir else None
    before = sum(1 for _ in open(log)) if log and os.path.exists(log) else 0
    real, text = native.lib(), io.StringIO()
    gc.collect()                   # as record_probe_trace.py: no engine of an earlier call is destroyed inside this one's trace
    gc.disable()
    native._lib = rec = Recorder(real)
    t0 = time.perf_counter()
    try:
        with contextlib.redirect_stdout(text):
            stats = rlp.main(args)
        torch.cuda.synchronize()
    finally:
        native._lib = real
        gc.enable()
    seconds = time.perf_counter() - t0
    lines = [AUGMENT.sub("<augment>", ln.replace(root, "<root>")) for ln in text.getvalue().splitlines()
             if not ln.startswith(("Namespace(", "Epoch: [", "Training time"))]
    entries = [json.loads(ln) for ln in list(open(log))[before:]] if log and os.path.exists(log) else []
    counts = {}
    for n in rec.names:
        counts[n] = counts.get(n, 0) + 1
    return {"argv": [a.replace(root, "<root>") for a in argv], "stdout": lines, "log_values": [list(map(list, e.items())) for e in entries],
            "files": sorted(os.listdir(args.output_dir)) if args.output_dir else [],
            "stats": _stats_keys(stats), "calls": dict(sorted(counts.items())),
            "calls_sha256": hashlib.sha256("\n".join(rec.names).encode()).hexdigest()}, seconds


def _is_number(token):
    try:
        float(token.strip("()[],:"))
        return True
    except ValueError:
        return False


def mask(call):
    """The committed form of a call's record: no digits, of log.txt the keys and the kinds of their values, no command line."""
    out = {k: v for k, v in call.items() if k not in ("argv", "log", "log_values")}
    out["stdout"] = [" ".join("#" if _is_number(t) else t for t in ln.split()) for ln in call["stdout"]]
    out["log"] = [[k if _kind(v) == "number" else f"{k}: {_kind(v)}" for k, v in e] for e in call["log_values"]]
    return out


@contextlib.contextmanager
def _session(root):
    """The tiny model registered, the inputs under `root`/inputs (made on first use; a temporary root without one): (root, paths)."""
    from uncertainty_vit_amd import modeling_cyclical
    had = modeling_cyclical._REGISTRY.get(MODEL)
    modeling_cyclical._REGISTRY[MODEL] = _tiny
    try:
        with contextlib.ExitStack() as stack:
            root = os.path.realpath(root or stack.enter_context(tempfile.TemporaryDirectory()))
            inputs = os.path.join(root, "inputs")
            yield root, make_inputs(inputs, make=not os.path.exists(inputs))
    finally:
        if had is None:
            del modeling_cyclical._REGISTRY[MODEL]
        else:
            modeling_cyclical._REGISTRY[MODEL] = had


def record(names=None, root=None, masked=True):
    """{scenario: [a record per main() call]} on the current device; every scenario writes into the new folder `root`/<scenario>."""
    import run_linear_probe as rlp
    out = {}
    with _session(root) as (root, paths):
        for name in names or SCENARIOS:
            fill = dict(paths, out=os.path.join(root, name))
            calls = [run_call(rlp, [a.format(**fill) for a in argv], root)[0] for argv in SCENARIOS[name]]
            out[name] = [mask(c) for c in calls] if masked else calls
    return out


def timing(repeats=3):
    """{label: [seconds of each repeat]} of the two calls of TIMED."""
    import run_linear_probe as rlp
    out = {}
    with _session(None) as (root, paths):
        for label, (name, index) in TIMED.items():
            seconds = []
            for r in range(repeats + 1):                   # the first repeat warms the library up and is dropped
                fill = dict(paths, out=os.path.join(root, f"{label}_{r}"))
                seconds.append(run_call(rlp, [a.format(**fill) for a in SCENARIOS[name][index]], root)[1])
            out[label] = seconds[1:]
    return out


def dump(rec, path):
    with open(path, "w") as f:      # a call per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: [\n" + ",\n".join(json.dumps(c, sort_keys=True) for c in v) + "]"
                                  for k, v in sorted(rec.items()) if k != "_timing"))
        f.write((",\n" + json.dumps("_timing") + ": " + json.dumps(rec["_timing"]) if "_timing" in rec else "") + "\n}\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw", metavar="FILE", help="write the unmasked record here instead of the golden")
    ap.add_argument("--timing", action="store_true", help="also time the two calls of TIMED three times each (with --raw)")
    opts = ap.parse_args()
    rec = record(masked=not opts.raw)
    if opts.raw and opts.timing:
        rec["_timing"] = timing()
    dump(rec, opts.raw or GOLDEN)
    print(f"{len(SCENARIOS)} scenarios, {sum(len(v) for k, v in rec.items() if k != '_timing')} calls -> {opts.raw or GOLDEN}")
