"""GPU, end to end: run_linear_probe.main --eval --perturbation_path on two small synthetic perturbation files, one with `noise` in
its name, behind the evaluation of tests/test_gpu_calib_cli.py (its image folder and checkpoint helpers are used here):
beit_base_patch16_224 cut after block 0, 6 validation images in 3 classes."""
import json
import re

import numpy as np
import pytest

from test_gpu_calib_cli import _image_tree, _pretraining_checkpoint

pytestmark = pytest.mark.gpu

TOP5 = re.compile(r"^Top5 Distance\t(\S+)$", re.M)
ZIPF = re.compile(r"^Zipf Distance\t(\S+)$", re.M)
MEAN = re.compile(r"^Mean Flipping Prob\t(\S+)$", re.M)


def _sequences(path, n, frames, seed):
    """(n, frames, 32, 32, 3) uint8: frame t = frame 0 plus noise that grows with t."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, 1, 32, 32, 3)).astype(np.float64)
    drift = rng.standard_normal((n, frames, 32, 32, 3)) * 40.0 * np.arange(frames).reshape(1, frames, 1, 1, 1)
    np.save(path, np.clip(base + drift, 0, 255).astype(np.uint8))


def test_cli_eval_with_and_without_perturbations(tmp_path, capsys, monkeypatch):
    pytest.importorskip("PIL")
    import run_linear_probe as rlp
    from uncertainty_vit_amd.linear_probe import LinearProbe
    val, out, ckpt, pdir = tmp_path / "val", tmp_path / "out", tmp_path / "checkpoint-0.pth", tmp_path / "p"
    _image_tree(str(val), 6)
    out.mkdir()
    pdir.mkdir()
    _pretraining_checkpoint(ckpt)
    _sequences(pdir / "gaussian_noise.npy", 3, 4, 1)
    _sequences(pdir / "brightness.npy", 5, 3, 2)
    argv = ["--model", "beit_base_patch16_224", "--finetune", str(ckpt), "--data_set", "image_folder", "--data_path", str(val),
            "--eval_data_path", str(val), "--nb_classes", "3", "--target_layer", "0", "--batch_size", "8", "--output_dir", str(out),
            "--eval"]
    plain = rlp.main(rlp.get_args(argv))
    text = capsys.readouterr().out
    assert "* Acc@1" in text and "Flipping Prob" not in text and "Perturbed dataset" not in text and "Distance" not in text
    assert not (out / "log.txt").exists() and set(plain) == {"loss", "acc1", "acc5", "n", "correct1", "correct5"}

    calls = []
    inner = LinearProbe.evaluate_stability

    def spy(self, loader, frames, noise, **kw):
        sizes = []

        def counted():
            for item in loader:
                sizes.append(item[0][0].shape[0])
                yield item
        r = inner(self, counted(), frames, noise, **kw)
        calls.append((frames, bool(noise), sizes, r))
        return r
    monkeypatch.setattr(LinearProbe, "evaluate_stability", spy)
    stats = rlp.main(rlp.get_args(argv + ["--perturbation_path", str(pdir)]))
    text = capsys.readouterr().out
    assert all(stats[k] == plain[k] for k in plain) and list(stats["stability"]) == ["brightness", "gaussian_noise"]       # sorted
    # V = max(1, 8 // F) sequences per forward: F = 3 -> 2, 2, 1 sequences; F = 4 -> 2, 1; `noise` in the name picks the fixed reference
    assert [(c[0], c[1], c[2]) for c in calls] == [(3, False, [6, 6, 3]), (4, True, [8, 4])]
    assert [c[3] for c in calls] == [stats["stability"]["brightness"], stats["stability"]["gaussian_noise"]]
    lines = text.splitlines()
    assert lines.index("Perturbed dataset evaluation :") > [i for i, ln in enumerate(lines) if ln.startswith("* Acc@1")][0]
    top5, zipf = TOP5.findall(text), ZIPF.findall(text)
    assert len(top5) == 2 and len(zipf) == 2
    for i, name in enumerate(("brightness", "gaussian_noise")):
        r = stats["stability"][name]
        assert r["n_sequences"] == (5, 3)[i] and r["frames"] == (3, 4)[i] and r["nan_sequences"] == 0
        assert 0.0 <= r["flip_prob"] <= 1.0 and 0.0 <= r["top5_dist"] <= 25.0 and r["zipf_dist"] >= 0.0
        at = lines.index(name + " Flipping Prob")
        assert lines[at - 1] == "" and lines[at + 1] == str(r["flip_prob"])                # the reference prints the bare float
        assert lines[at + 2] == "Top5 Distance\t{:.5f}".format(r["top5_dist"]) and lines[at + 3] == "Zipf Distance\t{:.5f}".format(r["zipf_dist"])
        assert "Perturbation : " + name in lines
    flips = [stats["stability"][n]["flip_prob"] for n in ("brightness", "gaussian_noise")]
    assert str(flips) in lines and MEAN.search(text).group(1) == "{:.5f}".format(np.mean(flips))
    log = [json.loads(line) for line in open(out / "log.txt")]
    assert len(log) == 2
    for entry, name in zip(log, ("brightness", "gaussian_noise")):
        r = stats["stability"][name]
        assert entry == {f"test_flip_{name}": r["flip_prob"], f"test_top5_{name}": r["top5_dist"], f"test_zipf_{name}": r["zipf_dist"]}

    monkeypatch.setattr(LinearProbe, "evaluate_stability", inner)
    only = rlp.main(rlp.get_args(argv + ["--perturbation_path", str(pdir), "--perturbations", "gaussian_noise"]))
    capsys.readouterr()
    assert only["stability"] == {"gaussian_noise": stats["stability"]["gaussian_noise"]}      # the same numbers on a second run
    with pytest.raises(ValueError):
        rlp.main(rlp.get_args([a for a in argv if a != "--eval"] + ["--perturbation_path", str(pdir)]))
