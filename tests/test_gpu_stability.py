"""GPU: the stability ops (csrc/stability.hip) against the numpy restatement (tests/stability_ref.py): ranks exactly, per-sequence
flips and top-5 distances exactly, Zipf distances within 1e-9; through LinearProbe against the reference's stored numbers
(tests/golden/stability.npz) and end to end through the tiny encoder.  Every output sits in front of guard elements that no kernel
may touch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stability_ref as sr
from oracle.closed_form import closed_form_images

pytestmark = pytest.mark.gpu

RANK_SHAPES = [(1, 1), (3, 2), (5, 5), (5, 6), (4, 63), (4, 64), (4, 65), (31, 100), (8, 1000), (8, 1003), (64, 4096), (2, 4095)]
SEQ_SHAPES = [(1, 2, 1), (1, 2, 7), (3, 5, 100), (6, 31, 100), (2, 256, 10), (5, 3, 1003)]
ATOL = 1e-9            # fp64 sums of at most 4096 terms in [0, 1] per pair (the bound of tests/test_gpu_calib.py): round-off near 1e-13
GUARD = 64
FILL = {torch.float32: 7.5, torch.float64: 7.5, torch.int32: 7777}
ARG, SHAPE = -1, -2


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "stability.npz"))


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(n, dtype):
    return torch.full((n + GUARD,), FILL[dtype], dtype=dtype, device="cuda")


def intact(t, n):
    return bool((t[n:] == FILL[t.dtype]).all())


def untouched(t):
    return bool((t == FILL[t.dtype]).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


# ---- the ops, each on its own; every call checks the guards ----
def run_ranks(L, z, misalign=False):
    """z: (R, K) fp32 numpy.  misalign: the device copy starts 4 bytes past a 16-byte boundary (no vector loads)."""
    R, K = z.shape
    buf = torch.zeros(R * K + 4, dtype=torch.float32, device="cuda")
    zg = buf[1:1 + R * K] if misalign else buf[:R * K]
    zg.copy_(torch.from_numpy(np.ascontiguousarray(z)).reshape(-1))
    assert (zg.data_ptr() % 16 == 4) if misalign else (zg.data_ptr() % 16 == 0)
    out = guarded(R * K, torch.int32)
    rc = L.uvit_op_stability_ranks(P(zg), P(out), R, K, S())
    torch.cuda.synchronize()
    assert intact(out, R * K)
    return rc, out


def run_sequences(L, rk, V, F, K, noise):
    """rk: device int32 tensor holding (V F, K) ranks."""
    out = guarded(3 * V, torch.float64)
    rc = L.uvit_op_stability_sequences(P(rk), P(out), V, F, K, noise, S())
    torch.cuda.synchronize()
    assert intact(out, 3 * V)
    return rc, out


# ---- inputs ----
def rank_inputs(R, K):
    """{name: (R, K) fp32}: random values; a half-integer grid with many ties; and `special`, rows that cycle through an all-equal
    row, the two zeros mixed, +inf / -inf / denormals among ordinary values, an ascending and a descending row.  `special` has
    max(R, 5) rows, so that every shape's K meets all five kinds."""
    rng = np.random.default_rng(1000 * R + K)
    special = np.empty((max(R, 5), K), dtype=np.float32)
    for r in range(special.shape[0]):
        kind = r % 5
        if kind == 0:
            special[r] = -2.25
        elif kind == 1:
            special[r] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32), K)
        elif kind == 2:
            special[r] = rng.choice(np.array([np.inf, -np.inf, 1e-45, -1e-45, 3e-39, 0.0, -0.0, 1.0, -3.5, 3e38], dtype=np.float32), K)
        elif kind == 3:
            special[r] = np.arange(K, dtype=np.float32) - K / 2
        else:
            special[r] = K / 2 - np.arange(K, dtype=np.float32)
    return {"random": rng.standard_normal((R, K)).astype(np.float32) * 3,
            "grid": rng.integers(-6, 7, (R, K)).astype(np.float32) / 2,
            "special": special}


def seq_logits(V, F, K, seed):
    """Frames that drift: frame t = frame t - 1 with a tenth of the classes redrawn, on a half-integer grid (ties and flips)."""
    rng = np.random.default_rng(seed)
    z = np.empty((V, F, K), dtype=np.float32)
    z[:, 0] = rng.integers(-8, 9, (V, K)) / 2
    for t in range(1, F):
        z[:, t] = z[:, t - 1]
        moved = rng.random((V, K)) < 0.1
        z[:, t][moved] = (rng.integers(-8, 11, (V, K)) / 2)[moved]
    return z.reshape(V * F, K)


# ---- ranks ----
@pytest.mark.parametrize("R,K", RANK_SHAPES)
def test_ranks(L, R, K):
    """Exact integer equality with the restatement on every kind of input, from a 16-byte aligned base and (K % 4 == 0: the other
    load path) from one that is not; two calls give the same bits."""
    for name, z in rank_inputs(R, K).items():
        R = z.shape[0]                                                     # `special` has at least five rows
        want = sr.ranks(z)
        if K <= 128:
            assert np.array_equal(want, sr.ranks_by_definition(z))
        for misalign in ((False, True) if K % 4 == 0 else (False,)):
            rc, out = run_ranks(L, z, misalign)
            assert rc == 0
            got = out[:R * K].view(R, K).cpu().numpy()
            wrong = int((got != want).sum())
            print(f"\nranks {(R, K)} {name} misaligned {misalign}: {wrong} of {R * K} differ")
            assert wrong == 0, (name, misalign, np.argwhere(got != want)[:8].tolist())
        rc2, out2 = run_ranks(L, z)
        assert rc2 == 0 and torch.equal(bits(out[:R * K]), bits(out2[:R * K]))


def test_ranks_with_more_row_groups_than_workgroups(L):
    """20000 rows of 2 classes and 9000 rows of 130 (four and two rows per workgroup): 5000 and 4500 row groups for the 4096
    workgroups of a launch, so some workgroups walk on to a second group; ties everywhere."""
    for R, K in ((20000, 2), (9000, 130)):
        z = np.random.default_rng(R + K).integers(-3, 4, (R, K)).astype(np.float32) / 2
        rc, out = run_ranks(L, z)
        assert rc == 0 and np.array_equal(out[:R * K].view(R, K).cpu().numpy(), sr.ranks(z))


def test_ranks_of_a_nan_row(L):
    """One row with a NaN among clean ones (K = 100 and K = 1003: a wave per row and a workgroup per row): its ranks are all 0,
    the rows beside it are right; a row of nothing but NaN as well."""
    for R, K in ((6, 100), (3, 1003)):
        z = rank_inputs(R, K)["grid"]
        z[1, K // 3] = np.nan
        z[R - 1] = np.nan
        rc, out = run_ranks(L, z)
        assert rc == 0
        got = out[:R * K].view(R, K).cpu().numpy()
        assert np.array_equal(got, sr.ranks(z)) and not got[1].any() and not got[R - 1].any() and bool((got[0] > 0).all())


# ---- sequences ----
@pytest.mark.parametrize("noise", [0, 1])
@pytest.mark.parametrize("V,F,K", SEQ_SHAPES)
def test_sequences(L, V, F, K, noise):
    """On the op's own ranks (which are the restatement's): flips and top-5 sums exactly, Zipf sums within 1e-9; two calls give the
    same bits."""
    z = seq_logits(V, F, K, 17 * V + F + K)
    rc, rk = run_ranks(L, z)
    assert rc == 0
    rk_host = rk[:V * F * K].view(V * F, K).cpu().numpy()
    assert np.array_equal(rk_host, sr.ranks(z))
    want = sr.sequences(rk_host, V, F, noise)
    rc, out = run_sequences(L, rk, V, F, K, noise)
    rc2, out2 = run_sequences(L, rk, V, F, K, noise)
    assert rc == 0 and rc2 == 0 and torch.equal(bits(out[:3 * V]), bits(out2[:3 * V]))
    got = out[:3 * V].view(V, 3).cpu().numpy()
    err = float(np.abs(got[:, 2] - want[:, 2]).max())
    print(f"\nsequences {(V, F, K)} noise {noise}: flips {got[:, 0].tolist()[:6]} top5 {got[:, 1].tolist()[:6]} Zipf error {err:.1e}")
    assert np.array_equal(got[:, :2], want[:, :2]) and err <= ATOL
    if K >= 6:
        perm = sr.sequences(rk_host, V, F, noise, sr.pair_permutation)
        assert np.array_equal(got[:, :2], perm[:, :2]) and float(np.abs(got[:, 2] - perm[:, 2]).max()) <= ATOL
    if K > 1 and F > 2:
        assert got[:, 0].sum() > 0                                          # the input does flip


@pytest.mark.parametrize("noise", [0, 1])
def test_nan_in_a_sequence(L, noise):
    """A NaN logit in the last frame of sequence 1 of 3: its three values are NaN, its neighbours are what they are without it."""
    V, F, K = 3, 4, 10
    z = seq_logits(V, F, K, 5)
    z[1 * F + 3, 7] = np.nan
    rc, rk = run_ranks(L, z)
    assert rc == 0
    rc, out = run_sequences(L, rk, V, F, K, noise)
    assert rc == 0
    got = out[:3 * V].view(V, 3).cpu().numpy()
    want = sr.sequences(sr.ranks(z), V, F, noise)
    assert bool(np.isnan(got[1]).all()) and bool(np.isnan(want[1]).all())
    assert np.array_equal(got[[0, 2], :2], want[[0, 2], :2]) and float(np.abs(got[[0, 2], 2] - want[[0, 2], 2]).max()) <= ATOL


# ---- errors ----
def test_every_error_return_leaves_the_outputs_untouched(L):
    z = torch.zeros(8 * 16, dtype=torch.float32, device="cuda")
    rk_in = torch.ones(8 * 16, dtype=torch.int32, device="cuda")
    ranks, seq = guarded(8 * 16, torch.int32), guarded(3 * 8, torch.float64)
    for R, K in [(0, 16), (-1, 16), (65535 * 256 + 1, 16), (8, 0), (8, -1), (8, 4097)]:
        assert L.uvit_op_stability_ranks(P(z), P(ranks), R, K, S()) == SHAPE, (R, K)
    assert L.uvit_op_stability_ranks(None, P(ranks), 8, 16, S()) == ARG and L.uvit_op_stability_ranks(P(z), None, 8, 16, S()) == ARG
    for V, F, K in [(0, 4, 16), (-1, 4, 16), (65536, 4, 16), (2, 1, 16), (2, 0, 16), (2, 257, 16), (2, 4, 0), (2, 4, 4097)]:
        assert L.uvit_op_stability_sequences(P(rk_in), P(seq), V, F, K, 0, S()) == SHAPE, (V, F, K)
    assert L.uvit_op_stability_sequences(None, P(seq), 2, 4, 16, 0, S()) == ARG
    assert L.uvit_op_stability_sequences(P(rk_in), None, 2, 4, 16, 0, S()) == ARG
    for noise in (2, -1):
        assert L.uvit_op_stability_sequences(P(rk_in), P(seq), 2, 4, 16, noise, S()) == ARG, noise
    torch.cuda.synchronize()
    assert untouched(ranks) and untouched(seq)


# ---- LinearProbe ----
@pytest.fixture(scope="module")
def case(golden_dir):
    import probe_ref as pr
    return pr.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def probe10(case):
    from test_gpu_probe import fixture_probe
    return fixture_probe(case)


@pytest.fixture(scope="module")
def probe100(probe10):
    from uncertainty_vit_amd.linear_probe import LinearProbe
    return LinearProbe(probe10.encoder, 100)


@pytest.mark.parametrize("noise", [False, True])
def test_stability_batch_against_reference_fixture(probe100, fx, noise):
    """The fixture's logits through stability_batch: the reference's ranks exactly, its flip probability and top-5 distance exactly
    and its Zipf distance within 1e-9, per sequence and for the data set."""
    z = fx["logits"]
    V, F, K = z.shape
    m = "noise%d" % int(noise)
    sums = probe100.stability_batch(torch.from_numpy(z.reshape(V * F, K)).cuda(), F, noise).cpu().numpy()
    assert np.array_equal(probe100._ranks[:V * F].cpu().numpy(), fx["ranks"].reshape(V * F, K).astype(np.int32))
    assert np.array_equal(sums[:, 0] / (F - 1), fx["flip_seq/" + m]) and np.array_equal(sums[:, 1] / (F - 1), fx["top5_seq/" + m])
    d = sr.dataset_values(sums, F)
    e_seq, e_all = float(np.abs(sums[:, 2] / (F - 1) - fx["zipf_seq/" + m]).max()), abs(d["zipf_dist"] - float(fx["zipf/" + m]))
    print(f"\nfixture {m}: flip {d['flip_prob']:.6f} top5 {d['top5_dist']:.6f} zipf {d['zipf_dist']:.9f}; Zipf error per sequence {e_seq:.1e}, "
          f"data set {e_all:.1e}")
    assert d["flip_prob"] == float(fx["flip/" + m]) and d["top5_dist"] == float(fx["top5/" + m])
    assert e_seq <= ATOL and e_all <= ATOL


@pytest.mark.parametrize("noise", [False, True])
def test_stability_batch_is_deterministic_and_independent_of_batching(probe100, noise):
    """Two calls on the same input give identical bits; V sequences in one call equal V calls on one sequence each, bit for bit."""
    V, F, K = 5, 7, 100
    z = torch.from_numpy(seq_logits(V, F, K, 23)).cuda()
    one = probe100.stability_batch(z, F, noise).clone()
    two = probe100.stability_batch(z, F, noise).clone()
    assert torch.equal(bits(one), bits(two))
    single = torch.cat([probe100.stability_batch(z[v * F:(v + 1) * F].contiguous(), F, noise).clone() for v in range(V)])
    assert torch.equal(bits(one), bits(single))
    assert float(one[:, 0].sum()) > 0


def test_stability_batch_refuses_what_it_cannot_run(probe10):
    from uncertainty_vit_amd.native import UvitError
    for z, F in ((torch.zeros(8, 11, device="cuda"), 4),            # K of the head is 10
                 (torch.zeros(9, 10, device="cuda"), 4),            # not whole sequences
                 (torch.zeros(8, 10, device="cuda"), 1),            # a sequence needs two frames
                 (torch.zeros(514, 10, device="cuda"), 257),
                 (torch.zeros(8, 10, device="cuda", dtype=torch.float64), 4)):
        with pytest.raises(UvitError):
            probe10.stability_batch(z, F, False)


@pytest.mark.parametrize("noise", [False, True])
def test_evaluate_stability_end_to_end(probe10, case, noise):
    """8 synthetic sequences of 4 frames through the tiny encoder (48 px, embed 128, 2 blocks, 10 classes) in batches of 3, 3 and 2
    sequences, handed over in the three item forms a loader may use: the result is the restatement applied to probe.logits() of the
    same batches in the same process -- flip probability and top-5 distance exactly, Zipf distance within 1e-9."""
    _, cfg, _, _, _, _, _ = case
    V, F = 8, 4
    base = closed_form_images("stability/base", V, cfg.img_size)
    other = closed_form_images("stability/other", V * F, cfg.img_size).view(V, F, 3, cfg.img_size, cfg.img_size)
    w = torch.tensor([0.0, 0.5, 1.0, 1.5]).view(1, F, 1, 1, 1)
    frames = ((1 - w) * base[:, None] + w * other).contiguous()                    # frame 0 = the base image, later frames drift away
    chunks = [frames[0:3], frames[3:6], frames[6:8]]
    batches = [c.reshape(-1, 3, cfg.img_size, cfg.img_size).cuda() for c in chunks]
    logits = np.concatenate([probe10.logits(b).cpu().numpy() for b in batches])
    want = sr.evaluate(logits, V, F, noise)
    items = [batches[0], (batches[1], torch.zeros(12, dtype=torch.int64)), ((batches[2], None), torch.zeros(8, dtype=torch.int64))]
    got = probe10.evaluate_stability(items, F, noise, n_sequences=V)
    print(f"\nend to end noise {noise}: {got}; restatement {want}")
    assert set(got) == {"flip_prob", "top5_dist", "zipf_dist", "n_sequences", "frames", "nan_sequences"}
    assert got["n_sequences"] == V and got["frames"] == F and got["nan_sequences"] == 0
    assert got["flip_prob"] == want["flip_prob"] and got["top5_dist"] == want["top5_dist"]
    assert abs(got["zipf_dist"] - want["zipf_dist"]) <= ATOL
    assert probe10.evaluate_stability(items, F, noise, n_sequences=V + 3) == got    # a slab with room to spare
    from uncertainty_vit_amd.native import UvitError
    with pytest.raises(UvitError):
        probe10.evaluate_stability(items, F, noise, n_sequences=4)                  # the second batch does not fit
    with pytest.raises(UvitError):
        probe10.evaluate_stability(items, F, noise)                                 # a plain list does not say how many sequences
    empty = probe10.evaluate_stability([], F, noise, n_sequences=0)
    assert empty["n_sequences"] == 0 and np.isnan(empty["flip_prob"])
