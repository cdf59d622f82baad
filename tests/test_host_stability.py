"""CPU: the host-side pieces of the stability metrics -- the numpy restatement (tests/stability_ref.py) against what the reference's
functions computed (tests/golden/stability.npz, written by tools/gen_golden_stability.py), its per-class form against the
reference's permutation form, the sequence data set and its collate function, the argument checks of the two uvit_op_stability_*
entry points (they return before anything touches a device), and the command line's new flags."""
import ctypes as C
import os

import numpy as np
import pytest

import stability_ref as sr


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "stability.npz"))


# ---- the restatement against the fixture ----
def test_fixture_holds_the_crafted_cases(fx):
    z = fx["logits"]
    assert z.shape == (6, 5, 100) and z.dtype == np.float32 and fx["ranks"].dtype == np.uint16
    assert np.array_equal(z * 2, np.round(z * 2))                                      # the half-integer grid
    assert np.array_equal(z[1, 2], z[1, 1]) and bool((z[2] == 1.5).all())              # a pair without change; an all-equal sequence
    zeros = z[3][z[3] == 0]
    assert bool(np.signbit(zeros).any()) and not bool(np.signbit(zeros).all())         # both zeros
    assert all(len(np.unique(z[v, t])) < 40 for v in range(6) for t in range(5))       # heavy ties everywhere


def test_ranks_against_reference_fixture(fx):
    """Both restatements of the definition return rankdata(-z, method='ordinal') as the reference calls it, exactly."""
    z = fx["logits"].reshape(-1, 100)
    want = fx["ranks"].reshape(-1, 100).astype(np.int32)
    assert np.array_equal(sr.ranks_by_definition(z), want) and np.array_equal(sr.ranks(z), want)
    assert np.array_equal(np.argmin(want, axis=1), fx["predictions"].reshape(-1))      # rank 1 = argmax, first index on ties


@pytest.mark.parametrize("noise", [0, 1])
@pytest.mark.parametrize("pair", [sr.pair_per_class, sr.pair_permutation])
def test_metrics_against_reference_fixture(fx, noise, pair):
    """Flip probability and top-5 distance exactly, Zipf distance within 1e-12 of the reference's flip_prob / ranking_dist, for the
    data set and for every sequence on its own, in both modes and in both forms."""
    V, F, K = fx["logits"].shape
    m = "noise%d" % noise
    sums = sr.sequences(sr.ranks(fx["logits"].reshape(-1, K)), V, F, noise, pair)
    d = sr.dataset_values(sums, F)
    print(f"\n{m} {pair.__name__}: zipf - reference {d['zipf_dist'] - float(fx['zipf/' + m]):+.2e}")
    assert d["flip_prob"] == float(fx["flip/" + m]) and d["top5_dist"] == float(fx["top5/" + m])
    assert abs(d["zipf_dist"] - float(fx["zipf/" + m])) <= 1e-12
    assert np.array_equal(sums[:, 0] / (F - 1), fx["flip_seq/" + m]) and np.array_equal(sums[:, 1] / (F - 1), fx["top5_seq/" + m])
    assert float(np.abs(sums[:, 2] / (F - 1) - fx["zipf_seq/" + m]).max()) <= 1e-12
    assert d["n_sequences"] == V and d["nan_sequences"] == 0
    assert sums[2].tolist() == [0.0, 0.0, 0.0]                                         # the all-equal sequence never moves


def random_logits(R, K, seed, ties):
    rng = np.random.default_rng(seed)
    return (rng.integers(-6, 7, (R, K)).astype(np.float32) / 2) if ties else rng.standard_normal((R, K)).astype(np.float32)


@pytest.mark.parametrize("K", [1, 2, 5, 6, 7, 100, 1003])
def test_per_class_form_equals_permutation_form(K):
    """On random logits (with and without ties): the sort-based ranks equal the literal count; for K >= 6 the per-class form of the
    three metrics equals the reference's permutation form (integers exactly, Zipf to 1e-12); for K < 6, where the permutation form is not defined,
    the per-class form is checked by hand-countable properties: a pair with itself gives zeros, top-5 <= 25, flip in {0, 1}."""
    for ties in (False, True):
        z = random_logits(8, K, 7 + K, ties)
        rk = sr.ranks(z)
        assert np.array_equal(rk, sr.ranks_by_definition(z))
        assert all(sorted(r.tolist()) == list(range(1, K + 1)) for r in rk)
        for i in range(7):
            a, b = rk[i], rk[i + 1]
            pc = sr.pair_per_class(a, b)
            assert sr.pair_per_class(a, a) == (0, 0, 0.0) and pc[0] in (0, 1) and 0 <= pc[1] <= 25
            if K >= 6:
                pp = sr.pair_permutation(a, b)
                assert pc[:2] == pp[:2] and abs(pc[2] - pp[2]) <= 1e-12, (K, i, pc, pp)
    if K == 1:
        assert sr.sequences(np.ones((4, 1), dtype=np.int32), 2, 2, 0).tolist() == [[0.0, 0.0, 0.0]] * 2


def test_known_answers_by_hand():
    """K = 7.  a = identity; b swaps the first two classes: the prediction flips, top-5 = |0 - 1| + |1 - 0| = 2, Zipf =
    |1 - 1/2| / 1 + |1/2 - 1| / 2 = 0.75.  b sends class 0 to rank 7: top-5 = |0 - min(6, 5)| + four classes that move up by one = 9."""
    a = np.arange(1, 8)
    assert sr.pair_per_class(a, np.array([2, 1, 3, 4, 5, 6, 7])) == (1, 2, 0.75)
    last = sr.pair_per_class(a, np.array([7, 1, 2, 3, 4, 5, 6]))
    assert last[:2] == (1, 9)
    # ties go to the lower index; -0 == +0; infinities order; a NaN row has no ranks and the sequence no values
    z = np.array([[1.0, 1.0, 2.0], [0.0, -0.0, -1.0], [-np.inf, np.inf, 0.0], [np.nan, 1.0, 2.0]], dtype=np.float32)
    assert sr.ranks(z).tolist() == [[2, 3, 1], [1, 2, 3], [3, 1, 2], [0, 0, 0]]
    s = sr.sequences(sr.ranks(z), 2, 2, 0)
    # a = (2, 3, 1), b = (1, 2, 3): top-5 = |1 - 0| + |2 - 1| + |0 - 2| = 4, Zipf = |1/2 - 1| / 2 + |1/3 - 1/2| / 3 + |1 - 1/3| / 1
    assert s[0, :2].tolist() == [1.0, 4.0] and s[0, 2] == pytest.approx(0.25 + 1 / 18 + 2 / 3, abs=1e-15)
    assert bool(np.isnan(s[1]).all())
    d = sr.dataset_values(s, 2)
    assert d["nan_sequences"] == 1 and d["n_sequences"] == 2 and d["flip_prob"] == 1.0


# ---- the data set and its collate function ----
def test_perturbation_sequences_and_collate(tmp_path):
    """A (5, 3, 40, 32, 3) file, V = 2 sequences per batch: batches of 6, 6 and 3 images; the frames of a sequence adjacent and in
    frame order, every descriptor the level-1 pipeline's (resize the short side to int(S / .875), centre crop), labels 0, nothing
    masked."""
    import torch
    from uncertainty_vit_amd.datasets import BICUBIC, BEiTAugment, PackedBatch, PerturbationSequences, collate_sequences
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, (5, 3, 40, 32, 3), dtype=np.uint8)
    path = tmp_path / "gaussian_noise.npy"
    np.save(path, data)
    aug = BEiTAugment(48, 1, "bicubic", True)
    ds = PerturbationSequences(str(path), aug)
    assert len(ds) == 5 and ds.frames == 3 and isinstance(ds.data, np.memmap)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=collate_sequences)
    batches = list(loader)
    assert [len(b) for b in batches] == [6, 6, 3] and all(isinstance(b, PackedBatch) for b in batches)
    seen = 0
    for b in batches:
        rec, n = b.records(), len(b)
        frame_bytes = 40 * 32 * 3
        assert rec["offset"].tolist() == [i * frame_bytes for i in range(n)] and b.pixels.numel() == n * frame_bytes
        px = b.pixels.numpy().reshape(n // 3, 3, 40, 32, 3)
        assert np.array_equal(px, data[seen:seen + n // 3])                            # sequence-major, frames adjacent
        seen += n // 3
        assert bool((rec["h"] == 40).all()) and bool((rec["w"] == 32).all()) and bool((rec["filter"] == BICUBIC).all())
        assert bool((rec["flip"] == 0).all()) and bool((rec["n_jitter"] == 0).all())
        assert bool((rec["crop_w"] == 32).all()) and bool((rec["crop_h"] == 40).all())
        assert bool((rec["resize_w"] == 54).all()) and bool((rec["resize_h"] == 67).all())        # int(48 / .875) = 54, int(54 * 40 / 32) = 67
        assert bool((rec["win_x"] == 3).all()) and bool((rec["win_y"] == int(round((67 - 48) / 2.0))).all())
        assert b.labels.tolist() == [0] * n and int(b.mask.sum()) == 0 and b.mask.shape[0] == n
        assert (b.size, b.mean, b.std) == (48, aug.mean, aug.std)
    assert seen == 5
    with pytest.raises(ValueError):
        np.save(tmp_path / "bad.npy", np.zeros((2, 3, 8, 8), dtype=np.uint8))
        PerturbationSequences(str(tmp_path / "bad.npy"), aug)


# ---- argument checks of the C entry points: no GPU needed, nothing is launched ----
@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    return native.lib()


P1 = C.c_void_p(4096)      # any non-NULL pointer: the checks return before it is used
NUL = C.c_void_p(0)
ARG, SHAPE = -1, -2


def test_symbols_resolve(L):
    from uncertainty_vit_amd import native
    assert {"uvit_op_stability_ranks", "uvit_op_stability_sequences"} <= set(native.SYMBOLS)
    assert L.uvit_op_stability_ranks is not None and L.uvit_op_stability_sequences is not None
    assert L.uvit_version() == 100


def test_ranks_rejects_bad_arguments(L):
    for R, K in [(0, 10), (-1, 10), (65535 * 256 + 1, 10), (4, 0), (4, -3), (4, 4097)]:
        assert L.uvit_op_stability_ranks(P1, P1, R, K, NUL) == SHAPE, (R, K)
    assert L.uvit_op_stability_ranks(NUL, P1, 4, 10, NUL) == ARG and L.uvit_op_stability_ranks(P1, NUL, 4, 10, NUL) == ARG


def test_sequences_rejects_bad_arguments(L):
    for V, F, K in [(0, 5, 10), (-1, 5, 10), (65536, 5, 10), (2, 1, 10), (2, 0, 10), (2, 257, 10), (2, 5, 0), (2, 5, 4097)]:
        assert L.uvit_op_stability_sequences(P1, P1, V, F, K, 0, NUL) == SHAPE, (V, F, K)
    assert L.uvit_op_stability_sequences(NUL, P1, 2, 5, 10, 0, NUL) == ARG and L.uvit_op_stability_sequences(P1, NUL, 2, 5, 10, 1, NUL) == ARG
    for noise in (2, -1):
        assert L.uvit_op_stability_sequences(P1, P1, 2, 5, 10, noise, NUL) == ARG, noise


# ---- the module and the command line ----
def test_stability_needs_a_gpu():
    """No CPU fallback: stability_batch refuses host tensors."""
    import torch
    from test_host_probe import tiny_encoder
    from uncertainty_vit_amd.linear_probe import LinearProbe
    from uncertainty_vit_amd.native import UvitError
    probe = LinearProbe(tiny_encoder().eval(), 10)
    with pytest.raises(UvitError):
        probe.stability_batch(torch.zeros(8, 10), 4, False)


def test_cli_flags_are_absent_unless_given():
    """--perturbation_path / --perturbations are absent by default and leave the parsed arguments (the first line run_linear_probe
    prints) as they were: a run without them parses to today's names and values."""
    import run_linear_probe as rlp
    base = vars(rlp.get_args([]))
    assert base == {"batch_size": 64, "epochs": 30, "model": "deit_base_patch16_224", "input_size": 224, "clip_grad": None,
                    "weight_decay": 0.05, "lr": 5e-4, "min_lr": 1e-6, "warmup_epochs": 5, "smoothing": 0.1, "finetune": "",
                    "model_key": "model|module", "model_prefix": "", "target_layer": -1,
                    "data_path": "/datasets01/imagenet_full_size/061417/", "eval_data_path": None, "nb_classes": 0,
                    "imagenet_default_mean_and_std": False, "data_set": "IMNET", "output_dir": "", "seed": 0, "resume": "",
                    "eval": False, "num_workers": 0}
    a = rlp.get_args(["--eval", "--perturbation_path", "p", "--perturbations", "snow", "shot_noise"])
    assert a.perturbation_path == "p" and a.perturbations == ["snow", "shot_noise"]
    assert rlp.perturbation_files(a) == [("snow", os.path.join("p", "snow.npy")), ("shot_noise", os.path.join("p", "shot_noise.npy"))]


def test_cli_lists_the_directory_sorted(tmp_path):
    import run_linear_probe as rlp
    for n in ("zoom_blur.npy", "brightness.npy", "notes.txt", "gaussian_noise.npy"):
        (tmp_path / n).write_bytes(b"")
    a = rlp.get_args(["--eval", "--perturbation_path", str(tmp_path)])
    assert [n for n, _ in rlp.perturbation_files(a)] == ["brightness", "gaussian_noise", "zoom_blur"]
