"""GPU, end to end: run_linear_probe.main --eval --vim_data_path ... --ood_data_path ... on a generated 10-class folder of 48 px
images, 20 per class, and a folder of noise images: beit_base_patch16_224 at 48 px cut after block 0, a one-block checkpoint, a head
drawn here and saved as probe-0.pth.  200 images span at most 200 directions of the 768, so the runs take --vim_dim 64."""
import json
import re

import pytest
import torch

from test_gpu_lap_cli import _checkpoints, _image_tree
from test_gpu_maha_cli import _noise_tree

pytestmark = pytest.mark.gpu

FIT_LINE = re.compile(r"^\* ViM fit on (\d+) images \((\d+) skipped\), dim (\d+) of (\d+), alpha (-?\d+\.\d{5}), explained (\d\.\d{5})$", re.M)
ACC_LINE = re.compile(r"^\* ViM Acc@1 (\d+\.\d{3}) mean (-?\d+\.\d{5})$", re.M)


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
    root = tmp_path_factory.mktemp("vim_cli")
    data, other, pre, head = root / "data", root / "other", root / "checkpoint-0.pth", root / "probe-0.pth"
    _image_tree(str(data))
    _noise_tree(str(other))
    _checkpoints(pre, head)
    return data, other, pre, head


def test_cli_eval_with_a_vim_fit_and_a_saved_fit(tree, tmp_path, capsys):
    import run_linear_probe as rlp
    data, other, pre, head = tree
    out = tmp_path / "out"
    out.mkdir()
    argv = ["--model", "beit_base_patch16_224", "--input_size", "48", "--finetune", str(pre), "--resume", str(head), "--data_set", "image_folder",
            "--data_path", str(data), "--eval_data_path", str(data), "--nb_classes", "10", "--target_layer", "0", "--batch_size", "64",
            "--eval"]
    stats = rlp.main(rlp.get_args(argv + ["--vim_data_path", str(data), "--vim_dim", "64", "--ood_data_path", str(other), "--output_dir", str(out)]))
    first = _shown(capsys.readouterr().out)
    fit, det = stats["vim_fit"], stats["detection"]
    assert set(fit) == {"n", "skipped", "classes", "dim", "alpha", "explained"} and (fit["n"], fit["skipped"], fit["classes"], fit["dim"]) == (200, 0, 10, 64)
    assert first[0] == ("200", "0", "64", "768", f"{fit['alpha']:.5f}", f"{fit['explained']:.5f}") and 0.0 < fit["explained"] <= 1.0
    assert first[1] == (f"{stats['vim_acc1']:.3f}", f"{stats['vim_mean']:.5f}") and stats["n"] == 200 and det["n_ood"] == 30
    assert det["columns"] == ["msp", "entropy", "energy", "vim", "residual"]              # --vim_data_path implies --detection
    for col in ("vim", "residual"):
        assert sum(ln.startswith(f"* Detect misclassification {col} AUROC ") for ln in first[3]) == 1
        assert sum(ln.startswith(f"* Detect OOD {col} AUROC ") for ln in first[3]) == 1
    print(f"\nOOD AUROC vim {det['ood']['vim']['AUROC']:.4f} residual {det['ood']['residual']['AUROC']:.4f} energy {det['ood']['energy']['AUROC']:.4f}; "
          f"alpha {fit['alpha']:.4f}, explained {fit['explained']:.5f}, ViM Acc@1 {stats['vim_acc1']:.1f}")
    assert stats["vim_acc1"] == stats["acc1"]                                             # the snapshot is the head in use
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 1 and {"test_loss", "test_acc1", "test_acc5", "test_vim_acc1", "test_vim_mean", "test_vim_dim", "test_vim_alpha",
                              "test_mis_vim_AUROC", "test_mis_residual_AURC", "test_ood_vim_AUROC", "test_ood_residual_FPR95",
                              "test_ood_msp_AUROC"} <= set(log[0])
    assert (log[0]["test_vim_acc1"], log[0]["test_vim_mean"], log[0]["test_vim_dim"], log[0]["test_vim_alpha"]) == \
        (stats["vim_acc1"], stats["vim_mean"], 64, fit["alpha"])
    saved = torch.load(out / "vim.pth", map_location="cpu", weights_only=False)
    assert set(saved) == {"R", "origin", "weight", "bias", "alpha", "dim", "eigenvalues", "sums"} and tuple(saved["R"].shape) == (704, 768)
    assert all(saved[k].dtype == torch.float64 for k in ("R", "origin", "weight", "bias", "eigenvalues", "sums"))
    assert saved["sums"][2:].tolist() == [200.0, 0.0] and (saved["alpha"], saved["dim"]) == (fit["alpha"], 64)

    again = rlp.main(rlp.get_args(argv + ["--vim_state", str(out / "vim.pth"), "--ood_data_path", str(other)]))
    second = _shown(capsys.readouterr().out)
    assert second == first and again["vim_mean"] == stats["vim_mean"] and str(again["detection"]) == str(det)      # the same numbers

    # the density on the same folder: its moments serve the fit (one pass fewer), and the fit has the same bits
    both = rlp.main(rlp.get_args(argv + ["--vim_data_path", str(data), "--vim_dim", "64", "--maha_data_path", str(data)]))
    third = _shown(capsys.readouterr().out)
    assert third[0] == first[0] and both["vim_fit"] == fit and both["vim_mean"] == stats["vim_mean"] and "ood" not in both["detection"]
    assert both["detection"]["columns"] == ["msp", "entropy", "energy", "maha", "rmaha", "vim", "residual"]

    for bad in (["--vim_data_path", str(data), "--vim_state", str(out / "vim.pth")], ["--vim_dim", "64"], ["--gp_layer", "--vim_data_path", str(data)],
                ["--het_layer", "--vim_data_path", str(data)], ["--ensembles", "--ens_combine", "probs", "--vim_data_path", str(data)]):
        with pytest.raises(ValueError):
            rlp.main(rlp.get_args(argv + bad))
    capsys.readouterr()

    plain = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "ViM" not in text and "* Detect" not in text and set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"}
    assert (plain["loss"], plain["acc1"]) == (stats["loss"], stats["acc1"])               # the fit does not touch the logits
