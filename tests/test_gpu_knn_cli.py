"""GPU, end to end: run_linear_probe.main --eval --knn_data_path ... --ood_data_path ... on a generated 10-class folder of 48 px
images, 20 per class, and a folder of noise images: beit_base_patch16_224 at 48 px cut after block 0, a one-block checkpoint, a head
drawn here and saved as probe-0.pth."""
import json
import re

import pytest
import torch

from test_gpu_lap_cli import _checkpoints, _image_tree
from test_gpu_maha_cli import _noise_tree

pytestmark = pytest.mark.gpu

BANK_LINE = re.compile(r"^\* kNN bank of (\d+) images \((\d+) skipped\), (\d+) classes, k (\d+), temperature (\S+)$", re.M)
ACC_LINE = re.compile(r"^\* kNN Acc@1 (\d+\.\d{3}) mean (-?\d+\.\d{5})$", re.M)


def _shown(text):
    lines = text.splitlines()
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    m, v = BANK_LINE.search(text), ACC_LINE.search(text)
    assert m and v and len(acc) == 1 and len(BANK_LINE.findall(text)) == 1
    assert lines[acc[0] - 2] == m.group(0) and lines[acc[0] - 1] == v.group(0)            # the two lines, directly in front of * Acc@1
    detect = [ln for ln in lines if ln.startswith("* Detect")]
    return m.groups(), v.groups(), lines[acc[0]], detect


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The two image folders and the two checkpoints, made once for the module."""
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("knn_cli")
    data, other, pre, head = root / "data", root / "other", root / "checkpoint-0.pth", root / "probe-0.pth"
    _image_tree(str(data))
    _noise_tree(str(other))
    _checkpoints(pre, head)
    return data, other, pre, head


def test_cli_eval_with_a_neighbour_bank_and_a_saved_bank(tree, tmp_path, capsys):
    import run_linear_probe as rlp
    data, other, pre, head = tree
    out = tmp_path / "out"
    out.mkdir()
    argv = ["--model", "beit_base_patch16_224", "--input_size", "48", "--finetune", str(pre), "--resume", str(head), "--data_set", "image_folder",
            "--data_path", str(data), "--eval_data_path", str(data), "--nb_classes", "10", "--target_layer", "0", "--batch_size", "64",
            "--eval"]
    stats = rlp.main(rlp.get_args(argv + ["--knn_data_path", str(data), "--ood_data_path", str(other), "--output_dir", str(out)]))
    first = _shown(capsys.readouterr().out)
    fit, det = stats["neighbour_fit"], stats["detection"]
    assert fit == {"n": 200, "skipped": 0, "classes": 10, "k": 20, "temperature": 0.07} and first[0] == ("200", "0", "10", "20", "0.07")
    assert first[1] == (f"{stats['knn_acc1']:.3f}", f"{stats['knn_mean']:.5f}") and stats["n"] == 200 and det["n_ood"] == 30
    assert det["columns"] == ["msp", "entropy", "energy", "knn"]                          # --knn_data_path implies --detection
    assert sum(ln.startswith("* Detect misclassification knn AUROC ") for ln in first[3]) == 1
    assert sum(ln.startswith("* Detect OOD knn AUROC ") for ln in first[3]) == 1
    print(f"\nOOD AUROC knn {det['ood']['knn']['AUROC']:.4f} msp {det['ood']['msp']['AUROC']:.4f}; k-NN Acc@1 {stats['knn_acc1']:.1f}, "
          f"mean knn {stats['knn_mean']:.5f}")
    # the evaluation set is the bank: the 20th neighbour of an image is one of 19 others of its folder or nearer, the vote sees itself
    assert 0.0 <= det["ood"]["knn"]["AUROC"] <= 1.0 and 0.0 <= stats["knn_acc1"] <= 100.0 and stats["knn_mean"] >= 0
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1 and {"test_loss", "test_acc1", "test_acc5", "test_knn_acc1", "test_knn_mean", "test_knn_k", "test_mis_knn_AUROC",
                              "test_mis_knn_AURC", "test_ood_knn_AUROC", "test_ood_knn_FPR95", "test_ood_msp_AUROC"} <= set(log[0])
    assert (log[0]["test_knn_acc1"], log[0]["test_knn_mean"], log[0]["test_knn_k"]) == (stats["knn_acc1"], stats["knn_mean"], 20)
    saved = torch.load(out / "neighbours.pth", map_location="cpu", weights_only=False)
    assert set(saved) == {"bank", "labels", "sums", "k", "temperature"} and tuple(saved["bank"].shape) == (200, 768)
    assert saved["bank"].dtype == torch.bfloat16 and saved["labels"].dtype == torch.int32 and saved["sums"].tolist() == [200.0, 0.0]
    assert torch.bincount(saved["labels"].long(), minlength=10).tolist() == [20] * 10 and (saved["k"], saved["temperature"]) == (20, 0.07)

    again = rlp.main(rlp.get_args(argv + ["--knn_state", str(out / "neighbours.pth"), "--ood_data_path", str(other)]))
    second = _shown(capsys.readouterr().out)
    assert second == first and again["knn_mean"] == stats["knn_mean"] and str(again["detection"]) == str(det)      # the same numbers

    one = rlp.main(rlp.get_args(argv + ["--knn_state", str(out / "neighbours.pth"), "--knn_k", "1", "--maha_data_path", str(data)]))
    third = _shown(capsys.readouterr().out)
    assert third[0][3] == "1" and one["neighbour_fit"]["k"] == 1 and "ood" not in one["detection"]
    assert one["detection"]["columns"] == ["msp", "entropy", "energy", "maha", "rmaha", "knn"]
    assert one["knn_mean"] <= stats["knn_mean"] and 0.0 <= one["knn_acc1"] <= 100.0       # s_1 >= s_20 row for row

    plain = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "kNN" not in text and "* Detect" not in text and set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"}
    assert (plain["loss"], plain["acc1"]) == (stats["loss"], stats["acc1"])               # the bank does not touch the logits
