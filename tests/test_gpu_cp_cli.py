"""GPU, end to end: run_linear_probe.main --eval --cp_data_path ... on the small image folders and the checkpoint of
tests/test_gpu_calib_cli.py: beit_base_patch16_224 cut after block 0, 6 images in 3 classes that serve as calibration and as
evaluation folder."""
import json
import re

import pytest

from test_gpu_calib_cli import _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

CP_LINE = re.compile(r"^\* Conformal (lac|aps|raps) alpha (\S+) qhat (\S+) coverage (\d\.\d{5}) size (\d+\.\d{3}) empty (\d\.\d{5}) "
                     r"singleton (\d\.\d{5}) SSCV (\d\.\d{5}) worst-class (\d\.\d{5}) on (\d+) calibration images$", re.M)
CP_KEYS = {"test_cp_alpha", "test_cp_qhat", "test_cp_coverage", "test_cp_size", "test_cp_empty", "test_cp_singleton", "test_cp_sscv",
           "test_cp_worst_class", "test_cp_n_cal"}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("cp_cli")
    val, out, ckpt = root / "val", root / "out", root / "checkpoint-0.pth"
    _image_tree(str(val), 6)
    out.mkdir()
    _pretraining_checkpoint(ckpt)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(val),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "4", "--output_dir", str(out), "--eval"]
    return argv, val, out


def last_log(out):
    return json.loads(open(out / "log.txt").readlines()[-1])


def test_cli_eval_with_conformal_sets(setup, capsys):
    """The calibration folder is the evaluation folder and nothing is randomised: coverage is at least 1 - alpha."""
    import run_linear_probe as rlp
    argv, val, out = setup
    entries = lambda: len(open(out / "log.txt").readlines()) if (out / "log.txt").exists() else 0      # noqa: E731
    before = entries()
    plain = rlp.main(rlp.get_args(argv))
    plain_text = capsys.readouterr().out
    assert "Conformal" not in plain_text and "conformal" not in plain and entries() == before                # today's output

    stats = rlp.main(rlp.get_args(argv + ["--cp_data_path", str(val), "--cp_alpha", "0.1", "0.3"]))
    text = capsys.readouterr().out
    lines = text.splitlines()
    found = CP_LINE.findall(text)
    acc = [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")]
    cp = [i for i, ln in enumerate(lines) if ln.startswith("* Conformal")]
    assert len(found) == 2 and len(acc) == 1 and cp == [acc[0] + 1, acc[0] + 2]
    assert lines[acc[0]] == [ln for ln in plain_text.splitlines() if ln.startswith("* Acc@1")][0]
    fit, conf = stats["conformal_fit"], stats["conformal"]
    assert fit["alpha"] == [0.1, 0.3] and fit["score"] == "aps" and fit["n"] == 6 and fit["status"] == [1, 0]     # k = ceil(7 * 0.9) = 7 > 6
    assert lines[cp[0]:cp[1] + 1] == rlp.conformal_lines(fit, conf)
    for alpha in (0.1, 0.3):
        assert conf[alpha]["coverage"] >= 1.0 - alpha and conf[alpha]["n"] == 6
    assert conf[0.1]["size"] == 3.0 and conf[0.1]["coverage"] == 1.0 and conf[0.1]["size"] >= conf[0.3]["size"]
    log = last_log(out)
    assert set(log) == {"test_loss", "test_acc1", "test_acc5"} | CP_KEYS
    assert log["test_cp_alpha"] == [0.1, 0.3] and log["test_cp_n_cal"] == 6 and log["test_cp_qhat"][1] == fit["qhat"][1]
    assert log["test_cp_coverage"] == [conf[0.1]["coverage"], conf[0.3]["coverage"]]
    assert (stats["correct1"], stats["n"]) == (plain["correct1"], plain["n"])


@pytest.mark.parametrize("head", [["--gp_layer"], ["--het_layer", "--het_num_factors", "2", "--het_test_mc_samples", "32"], ["--ensembles", "--ens_members", "2"]])
def test_cli_conformal_sets_with_the_other_heads(setup, capsys, head):
    import run_linear_probe as rlp
    argv, val, out = setup
    stats = rlp.main(rlp.get_args(argv + head + ["--cp_data_path", str(val), "--cp_alpha", "0.3", "--cp_score", "raps", "--calibration"]))
    text = capsys.readouterr().out
    assert len(CP_LINE.findall(text)) == 1 and stats["conformal_fit"]["score"] == "raps" and stats["conformal_fit"]["lam"] == 0.01
    c = stats["conformal"][0.3]
    assert c["n"] == 6 and 0.0 <= c["coverage"] <= 1.0 and 0.0 <= c["size"] <= 3.0
    if head[0] != "--het_layer":                         # the heteroscedastic head draws its Monte-Carlo noise anew in every pass
        assert c["coverage"] >= 0.7
    assert CP_KEYS <= set(last_log(out))


def test_cli_temperature_reaches_the_conformal_scores(setup, capsys):
    import run_linear_probe as rlp
    argv, val, out = setup
    cp = ["--cp_data_path", str(val), "--cp_alpha", "0.3", "--cp_score", "lac"]
    one = rlp.main(rlp.get_args(argv + cp))
    a = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("* Acc@1")]
    two = rlp.main(rlp.get_args(argv + cp + ["--ts_temperature", "2"]))
    b = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("* Acc@1")]
    assert one["conformal_fit"]["qhat"] != two["conformal_fit"]["qhat"] and two["temperature"] == 2.0
    assert (one["acc1"], one["acc5"], one["n"]) == (two["acc1"], two["acc5"], two["n"]) and a[0].split(" loss ")[0] == b[0].split(" loss ")[0]
    fitted = rlp.main(rlp.get_args(argv + cp + ["--ts_data_path", str(val)]))
    text = capsys.readouterr().out
    assert "* Temperature" in text and len(CP_LINE.findall(text)) == 1 and fitted["conformal"][0.3]["coverage"] >= 0.7
    assert {"test_ts_temperature", "test_cp_qhat"} <= set(last_log(out))
