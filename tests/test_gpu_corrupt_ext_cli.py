"""GPU, end to end: run_linear_probe.main --eval --corruptions with the kinds of DESIGN.md section 9.18, in the manner of
tests/test_gpu_corrupt_cli.py (beit_base_patch16_224 cut after block 0, a checkpoint of two blocks, 6 validation images in 3 classes):
the reference's lines in its order, the log.txt keys, losses that differ from the clean run's, and the same numbers on a second run."""
import json

import numpy as np
import pytest

from test_gpu_calib_cli import CALIB_LINE, _image_tree, _pretraining_checkpoint
from test_gpu_corrupt_cli import MCE_LINE, SET_LINE, SEV_LINE, sweep_lines

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("corrupt_ext_cli")
    val, ckpt = root / "val", root / "checkpoint-0.pth"
    _image_tree(str(val), 6)
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(val),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--eval"]
    return root, argv


def test_cli_sweep_of_the_ext_kinds(setup, capsys):
    import run_linear_probe as rlp
    root, argv = setup
    out = root / "out"
    out.mkdir()
    sweep = ["--corruptions", "pixelate", "jpeg_compression", "--corruption_severities", "1", "5", "--calibration"]
    stats = rlp.main(rlp.get_args(argv + ["--output_dir", str(out)] + sweep))
    lines = sweep_lines(capsys.readouterr().out)
    # header, then per distortion its name and per severity the reference's line followed by the calibration line
    assert lines[1] == "Distortion : pixelate" and lines[6] == "Distortion : jpeg_compression"
    ces = []
    for i in (2, 4, 7, 9):
        m = SET_LINE.match(lines[i])
        assert m and CALIB_LINE.match(lines[i + 1]), lines[i:i + 2]
        ces.append(float(m.group(2)))
    m = MCE_LINE.match(lines[11])
    assert m and abs(float(m.group(1)) - np.mean(ces)) < 1e-4
    sev = [SEV_LINE.match(ln) for ln in lines[12:14]]
    assert all(sev) and [s.group(1) for s in sev] == ["1", "5"] and len(lines) == 14
    sets = stats["corruptions"]["sets"]
    assert list(sets) == [("pixelate", 1), ("pixelate", 5), ("jpeg_compression", 1), ("jpeg_compression", 5)]
    assert all(s["n"] == 6 and np.isfinite(s["NLL"]) for s in sets.values())
    # the images differ from the clean ones, and from severity to severity: so does the loss
    assert all(s["loss"] != stats["loss"] for s in sets.values())
    assert sets[("pixelate", 1)]["loss"] != sets[("pixelate", 5)]["loss"] and sets[("jpeg_compression", 1)]["loss"] != sets[("jpeg_compression", 5)]["loss"]
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 6                                           # the main evaluation, four sets, the summary
    for entry, ((name, s), st) in zip(log[1:5], sets.items()):
        assert entry[f"test_c_{name}_{s}_acc1"] == st["acc1"] and entry[f"test_c_{name}_{s}_ECE"] == st["ECE"]
        assert set(entry) == {f"test_c_{name}_{s}_{k}" for k in ("acc1", "acc5", "loss", "ce", "ECE", "TACE", "NLL", "AUROC")}
    assert log[5]["test_c_mce"] == stats["corruptions"]["summary"]["mce"]

    # a second run, the two families mixed and nothing cached: the same numbers for the sets both runs have
    again = rlp.main(rlp.get_args(argv + ["--corruptions", "contrast", "jpeg_compression", "pixelate", "--corruption_severities", "1", "5",
                                          "--calibration", "--corruption_cache_images", "0"]))
    capsys.readouterr()
    assert list(again["corruptions"]["sets"])[:2] == [("contrast", 1), ("contrast", 5)]
    for key, st in sets.items():
        np.testing.assert_equal(again["corruptions"]["sets"][key], st)
