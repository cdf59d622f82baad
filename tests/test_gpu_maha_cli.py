"""GPU, end to end: run_linear_probe.main --eval --maha_data_path ... --ood_data_path ... on a generated 10-class folder of 48 px
images, 20 per class, and a folder of noise images: beit_base_patch16_224 at 48 px cut after block 0, a one-block checkpoint, a head
drawn here and saved as probe-0.pth."""
import json
import os
import re

import numpy as np
import pytest
import torch

from test_gpu_lap_cli import _checkpoints, _image_tree

pytestmark = pytest.mark.gpu

FIT_LINE = re.compile(r"^\* Mahalanobis fit on (\d+) images \((\d+) skipped\), (\d+) classes \((\d+) empty\), shrinkage (\S+), "
                      r"log-det (-?\d+\.\d{5}) background (-?\d+\.\d{5})$", re.M)
ACC_LINE = re.compile(r"^\* Mahalanobis Acc@1 (\d+\.\d{3}) mean (\d+\.\d{5})$", re.M)


def _noise_tree(root, n=30, size=48):
    from PIL import Image
    rng = np.random.default_rng(29)
    os.makedirs(os.path.join(root, "other"), exist_ok=True)
    for i in range(n):
        px = rng.integers(0, 256, (size, size, 3)).astype(np.uint8)          # uniform noise: no class's brightness, no class's spread
        Image.fromarray(px).save(os.path.join(root, "other", f"img{i}.png"))


def _shown(text):
    lines = text.splitlines()
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    m, v = FIT_LINE.search(text), ACC_LINE.search(text)
    assert m and v and len(acc) == 1 and len(FIT_LINE.findall(text)) == 1
    assert lines[acc[0] - 2] == m.group(0) and lines[acc[0] - 1] == v.group(0)            # the two lines, directly in front of * Acc@1
    detect = [ln for ln in lines if ln.startswith("* Detect")]
    return m.groups(), v.groups(), lines[acc[0]], detect


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The two image folders and the two checkpoints, made once for the module."""
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("maha_cli")
    data, other, pre, head = root / "data", root / "other", root / "checkpoint-0.pth", root / "probe-0.pth"
    _image_tree(str(data))
    _noise_tree(str(other))
    _checkpoints(pre, head)
    return data, other, pre, head


def test_cli_eval_with_a_density_fit_and_a_saved_fit(tree, tmp_path, capsys):
    import run_linear_probe as rlp
    data, other, pre, head = tree
    out = tmp_path / "out"
    out.mkdir()
    argv = ["--model", "beit_base_patch16_224", "--input_size", "48", "--finetune", str(pre), "--resume", str(head), "--data_set", "image_folder",
            "--data_path", str(data), "--eval_data_path", str(data), "--nb_classes", "10", "--target_layer", "0", "--batch_size", "64",
            "--eval"]
    stats = rlp.main(rlp.get_args(argv + ["--maha_data_path", str(data), "--ood_data_path", str(other), "--output_dir", str(out)]))
    first = _shown(capsys.readouterr().out)
    fit, det = stats["density_fit"], stats["detection"]
    assert first[0] == ("200", "0", "10", "0", "0.001", f"{fit['logdet']:.5f}", f"{fit['logdet0']:.5f}")
    assert first[1] == (f"{stats['maha_acc1']:.3f}", f"{stats['maha_mean']:.5f}") and stats["n"] == 200 and det["n_ood"] == 30
    assert det["columns"] == ["msp", "entropy", "energy", "maha", "rmaha"]                # --maha_data_path implies --detection
    for col in ("maha", "rmaha"):
        assert sum(ln.startswith(f"* Detect misclassification {col} AUROC ") for ln in first[3]) == 1
        assert sum(ln.startswith(f"* Detect OOD {col} AUROC ") for ln in first[3]) == 1
    print(f"\nOOD AUROC maha {det['ood']['maha']['AUROC']:.4f} rmaha {det['ood']['rmaha']['AUROC']:.4f} msp {det['ood']['msp']['AUROC']:.4f}; "
          f"nearest-class-mean Acc@1 {stats['maha_acc1']:.1f}")
    assert 0.0 <= det["ood"]["maha"]["AUROC"] <= 1.0 and 0.0 <= stats["maha_acc1"] <= 100.0 and stats["maha_mean"] > 0
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1 and {"test_loss", "test_acc1", "test_acc5", "test_maha_acc1", "test_maha_mean", "test_maha_shrinkage", "test_mis_maha_AUROC",
                              "test_mis_rmaha_AURC", "test_ood_maha_AUROC", "test_ood_rmaha_FPR95", "test_ood_msp_AUROC"} <= set(log[0])
    assert (log[0]["test_maha_acc1"], log[0]["test_maha_mean"], log[0]["test_maha_shrinkage"]) == (stats["maha_acc1"], stats["maha_mean"], 1e-3)
    saved = torch.load(out / "density.pth", map_location="cpu", weights_only=False)
    assert set(saved) == {"S", "class_sum", "total_sum", "class_count", "sums", "shrinkage"} and tuple(saved["S"].shape) == (768, 768)
    assert tuple(saved["class_sum"].shape) == (10, 768) and saved["sums"].tolist() == [200.0, 0.0] and saved["class_count"].tolist() == [20.0] * 10

    again = rlp.main(rlp.get_args(argv + ["--maha_state", str(out / "density.pth"), "--ood_data_path", str(other)]))
    second = _shown(capsys.readouterr().out)
    assert second == first and again["maha_mean"] == stats["maha_mean"] and str(again["detection"]) == str(det)      # the same numbers

    looser = rlp.main(rlp.get_args(argv + ["--maha_state", str(out / "density.pth"), "--maha_shrinkage", "0.1"]))
    third = _shown(capsys.readouterr().out)
    assert third[0][4] == "0.1" and looser["density_fit"]["logdet"] > fit["logdet"] and "ood" not in looser["detection"]

    plain = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "Mahalanobis" not in text and "* Detect" not in text and set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"}
    assert (plain["loss"], plain["acc1"]) == (stats["loss"], stats["acc1"])               # the density does not touch the logits
