"""GPU, end to end: run_linear_probe.main --eval --mc_dropout_forwards ... on a generated 10-class folder of 48 px images, 20 per
class: beit_base_patch16_224 at 48 px cut after block 1, a two-block checkpoint, a head drawn by the other CLI test's helper."""
import json
import re

import pytest

from test_gpu_lap_cli import _image_tree

pytestmark = pytest.mark.gpu

MCD_LINE = re.compile(r"^\* MC-dropout passes (\d+) layers (\d+) of (\d+) rate (\S+) entropy (\d+\.\d{5}) expected (\d+\.\d{5}) MI (\d+\.\d{5}) "
                      r"variance (\d+\.\d{6}) disagreement (\d+\.\d{5})$", re.M)
DET_LINE = re.compile(r"^\* Deterministic Acc@1 (\d+\.\d{3})$", re.M)


def _checkpoints(pre, head):
    """What run_cyclical.py leaves behind for a two-block ViT-B/16 at 48 px (trained without dropout), and a linear probe-0.pth."""
    from functools import partial
    from types import SimpleNamespace

    import torch
    from uncertainty_vit_amd.modeling_cyclical import VisionTransformerForCyclicalTraining
    torch.manual_seed(5)
    m = VisionTransformerForCyclicalTraining(img_size=48, patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                             norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), init_values=0.1,
                                             use_shared_rel_pos_bias=True, use_abs_pos_emb=False)
    args = SimpleNamespace(rel_pos_bias=True, abs_pos_emb=False, layer_scale_init_value=0.1)
    torch.save({"model": m.state_dict(), "optimizer": {}, "epoch": 0, "scaler": {}, "args": args}, pre)
    w, b = 0.05 * torch.randn(10, 768), 0.1 * torch.randn(10)
    zeros = {"head.weight": torch.zeros(10, 768), "head.bias": torch.zeros(10)}
    torch.save({"model": {"head.weight": w, "head.bias": b}, "optimizer": {"step": 0, "exp_avg": zeros, "exp_avg_sq": zeros}, "epoch": 0}, head)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("mcd_cli")
    data, pre, head = root / "data", root / "checkpoint-0.pth", root / "probe-0.pth"
    _image_tree(str(data))
    _checkpoints(pre, head)
    return data, pre, head


def test_cli_eval_under_mc_dropout_and_without(tree, tmp_path, capsys):
    import run_linear_probe as rlp
    data, pre, head = tree
    out = tmp_path / "out"
    out.mkdir()
    argv = ["--model", "beit_base_patch16_224", "--input_size", "48", "--finetune", str(pre), "--resume", str(head), "--data_set", "image_folder",
            "--data_path", str(data), "--eval_data_path", str(data), "--nb_classes", "10", "--target_layer", "1", "--batch_size", "64",
            "--eval"]
    plain = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "MC-dropout" not in text and "Deterministic" not in text and set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"}

    mc = ["--mc_dropout_forwards", "4", "--attn_drop_rate", "0.2", "--mc_dropout_layers", "1", "--mc_seed", "3"]
    stats = rlp.main(rlp.get_args(argv + mc + ["--output_dir", str(out), "--detection", "--calibration"]))
    text = capsys.readouterr().out
    lines = text.splitlines()
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    m, d = MCD_LINE.search(text), DET_LINE.search(text)
    assert m and d and len(acc) == 1 and lines[acc[0] + 1] == m.group(0) and lines[acc[0] + 2] == d.group(0)      # directly behind * Acc@1
    assert m.groups()[:4] == ("4", "1", "2", "0.2")
    assert m.groups()[4:] == tuple(f"{stats[k]:.5f}" if k != "mcd_var" else f"{stats[k]:.6f}" for k in rlp.MCD_KEYS)
    assert d.group(1) == f"{stats['det_acc1']:.3f}" == f"{plain['acc1']:.3f}"             # the deterministic pass is the plain run's
    assert (stats["mcd_passes"], stats["mcd_layers"], stats["n"]) == (4, 1, 200)
    assert stats["mcd_mi"] > 0 and stats["mcd_total"] >= stats["mcd_aleatoric"] and abs(stats["loss"] - plain["loss"]) > 1e-7
    assert stats["detection"]["columns"] == ["msp", "entropy", "energy"] + list(rlp.MCD_KEYS) and "ECE" in stats
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1 and {"test_loss", "test_acc1", "test_mcd_total", "test_mcd_aleatoric", "test_mcd_mi", "test_mcd_var",
                              "test_mcd_disagreement", "test_mcd_det_acc1", "test_mcd_passes", "test_mis_mcd_mi_AUROC", "test_ECE"} <= set(log[0])
    assert log[0]["test_mcd_passes"] == 4 and log[0]["test_mcd_mi"] == stats["mcd_mi"] and log[0]["test_mcd_det_acc1"] == stats["det_acc1"]

    again = rlp.main(rlp.get_args(argv + mc))                                              # the same seed: the same numbers
    capsys.readouterr()
    assert again["loss"] == stats["loss"] and all(again[k] == stats[k] for k in rlp.MCD_KEYS)
    other = rlp.main(rlp.get_args(argv + mc[:-1] + ["4"]))                                  # another seed: other masks
    capsys.readouterr()
    assert other["mcd_mi"] != stats["mcd_mi"] and other["det_acc1"] == stats["det_acc1"]
