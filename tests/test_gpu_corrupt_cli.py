"""GPU, end to end: run_linear_probe.main --eval --corruptions / --corruption_path with the helpers of tests/test_gpu_calib_cli.py
(beit_base_patch16_224 cut after block 0, a checkpoint of two blocks, 6 validation images in 3 classes): the reference's lines in its
order, the mCE line from the four sets, the log.txt keys, the cached against the re-read path, and a pre-made tree."""
import json
import re
import shutil

import numpy as np
import pytest

from test_gpu_calib_cli import CALIB_LINE, _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

SET_LINE = re.compile(r"^\* Acc@1 (\d+\.\d{4}) CE (\d+\.\d{4}) $")
MCE_LINE = re.compile(r"^mCE \(unnormalized\) \(%\): (\d+\.\d{4}), acc :(\d+\.\d{4})$")
SEV_LINE = re.compile(r"^\* Severity (\d) Acc@1 (\S+) CE (\S+) rel-CE (\S+) ECE (\S+) NLL (\S+)$")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("corrupt_cli")
    val, ckpt = root / "val", root / "checkpoint-0.pth"
    _image_tree(str(val), 6)
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(val),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--eval"]
    return root, val, argv


def sweep_lines(text):
    """The lines from the reference's header on."""
    lines = text.splitlines()
    return lines[lines.index("Corrupted dataset evaluation :"):]


def test_cli_sweep_on_the_device(setup, capsys):
    import run_linear_probe as rlp
    root, val, argv = setup
    out = root / "out"
    out.mkdir()
    sweep = ["--corruptions", "gaussian_noise", "contrast", "--corruption_severities", "1", "5", "--calibration"]
    stats = rlp.main(rlp.get_args(argv + ["--output_dir", str(out)] + sweep))
    text = capsys.readouterr().out
    lines = sweep_lines(text)
    assert text.splitlines().index("Corrupted dataset evaluation :") > [i for i, ln in enumerate(text.splitlines()) if ln.startswith("* Acc@1")][0]
    # header, then per distortion its name and per severity the reference's line followed by the calibration line
    assert lines[1] == "Distortion : gaussian_noise" and lines[6] == "Distortion : contrast"
    ces = []
    for i in (2, 4, 7, 9):
        m = SET_LINE.match(lines[i])
        assert m and CALIB_LINE.match(lines[i + 1]), lines[i:i + 2]
        assert abs(float(m.group(2)) - (100 - float(m.group(1))) / 100) < 1e-4
        ces.append(float(m.group(2)))
    m = MCE_LINE.match(lines[11])
    assert m and len(ces) == 4 and abs(float(m.group(1)) - np.mean(ces)) < 1e-4
    sev = [SEV_LINE.match(ln) for ln in lines[12:14]]
    assert all(sev) and [s.group(1) for s in sev] == ["1", "5"] and len(lines) == 14
    sets = stats["corruptions"]["sets"]
    assert list(sets) == [("gaussian_noise", 1), ("gaussian_noise", 5), ("contrast", 1), ("contrast", 5)]
    assert all(s["n"] == 6 and np.isfinite(s["NLL"]) for s in sets.values())
    summ = stats["corruptions"]["summary"]
    assert summ["mce"] == np.mean([(100 - s["acc1"]) / 100 for s in sets.values()]) and f"{summ['mce']:.4f}" == m.group(1)
    assert summ["rel_ce"][0] == summ["ce"][0] - (100 - stats["acc1"]) / 100
    # the images differ from the clean ones: so does the loss
    assert all(s["loss"] != stats["loss"] for s in sets.values())
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 6                                           # the main evaluation, four sets, the summary
    for entry, ((name, s), st) in zip(log[1:5], sets.items()):
        assert entry[f"test_c_{name}_{s}_acc1"] == st["acc1"] and entry[f"test_c_{name}_{s}_ECE"] == st["ECE"]
        assert set(entry) == {f"test_c_{name}_{s}_{k}" for k in ("acc1", "acc5", "loss", "ce", "ECE", "TACE", "NLL", "AUROC")}
    assert log[5]["test_c_mce"] == summ["mce"] and log[5]["test_c_acc"] == summ["acc"] and log[5]["test_c_severity_ce"] == summ["ce"]
    assert len(log[5]["test_c_severity_ECE"]) == 2

    # nothing cached: every set reads the folder again, and gives the same figures
    again = rlp.main(rlp.get_args(argv + sweep + ["--corruption_cache_images", "0"]))
    capsys.readouterr()
    np.testing.assert_equal(again["corruptions"], stats["corruptions"])


def test_cli_sweep_over_a_tree(setup, capsys):
    import run_linear_probe as rlp
    root, val, argv = setup
    tree = root / "val-c"
    for name in ("fog", "contrast"):
        for s in (1, 2):
            shutil.copytree(val, tree / name / str(s))
    stats = rlp.main(rlp.get_args(argv + ["--corruption_path", str(tree), "--corruption_severities", "1", "2"]))
    lines = sweep_lines(capsys.readouterr().out)
    assert lines[1] == "Distortion : contrast" and lines[4] == "Distortion : fog"      # the reference's order, then the others
    assert all(SET_LINE.match(lines[i]) for i in (2, 3, 5, 6)) and MCE_LINE.match(lines[7]) and len(lines) == 10
    sets = stats["corruptions"]["sets"]
    assert list(sets) == [("contrast", 1), ("contrast", 2), ("fog", 1), ("fog", 2)]
    # the same images as the clean folder: the same figures
    assert all(s["acc1"] == stats["acc1"] and s["loss"] == stats["loss"] for s in sets.values())
    assert stats["corruptions"]["summary"]["rel_ce"] == [0.0, 0.0]
    with pytest.raises(FileNotFoundError, match="contrast/3"):
        rlp.main(rlp.get_args(argv + ["--corruption_path", str(tree), "--corruption_severities", "1", "3"]))
