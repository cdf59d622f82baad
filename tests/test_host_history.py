"""Host: the schedules of tests/test_gpu_history.py (tests/gpu_util.py::HISTORY) really have the properties that test relies on.
The kept-sample counts come from uvit_drop_path_kept_counts, the host function the engine sizes its compact launches with, and must
agree with the oracle's replay of the draws, from which the GPU test takes them."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import HISTORY, HISTORY_SEED, history_batch, history_cfg, history_kept_counts


@pytest.fixture(scope="module")
def lib():
    from uncertainty_vit_amd import native
    native.build()
    return native.lib()


def counts(lib, name):
    """Per training step of a schedule: (iteration, options, kept samples [layer][draw])."""
    h, cfg = HISTORY[name], history_cfg(name)
    draws = 4 if h["two_stream"] else 2
    out = []
    for kind, arg, *opt in h["steps"]:
        if kind != "step":
            continue
        buf = (C.c_int32 * (draws * cfg.depth))()
        assert lib.uvit_drop_path_kept_counts(cfg.depth, C.c_float(cfg.drop_path_rate), draws, h["B"], C.c_uint32(HISTORY_SEED),
                                              C.c_uint32(arg), buf) == 0
        k = np.array(buf[:]).reshape(cfg.depth, draws)
        assert k.tolist() == history_kept_counts(name, arg), (name, arg)
        out.append((arg, opt[0] if opt else {}, k))
    return out


def test_tiny_schedule_visits_empty_shrinking_and_growing_lists(lib):
    B, tokens = HISTORY["tiny"]["B"], history_cfg("tiny").num_tokens
    steps = counts(lib, "tiny")
    assert 6 <= len(steps) <= 10
    ks = [k for _, _, k in steps]
    on = [o.get("lists", True) for _, o, _ in steps]
    # (nearly) everybody kept, then a step with an empty list on one branch and a partial list on another
    assert any(a.min() >= B - 1 and (b == 0).any() and ((b > 0) & (b < B)).any() for a, b in zip(ks, ks[1:]))
    # one (layer, branch) whose list shrinks between two consecutive steps and grows between two others
    d = np.diff(np.stack(ks), axis=0)
    assert ((d < 0).any(0) & (d > 0).any(0)).any()
    # the top layer's MLP list shrinks from a step whose rows reach past the shorter list's rows, to rows that are no multiple of 64:
    # the pad rows of its dY up to the wgrad's reduction length then hold the earlier step's data unless they are zero-filled
    top = [int(k[-1, 1]) for k in ks]
    assert any(0 < b < a and on[i] and on[i + 1] and (b * tokens) % 64 for i, (a, b) in enumerate(zip(top, top[1:])))
    # the lists are switched off for exactly one step, between steps that run them
    assert on.count(False) == 1 and on[0] and on[-1]
    i = on.index(False)
    assert ((ks[i] > 0) & (ks[i] < B)).any(), "the step without lists must be one that would have run them"
    # the steps compared with the oracle are the ones with an empty list
    assert [bool((k == 0).any()) for _, o, k in steps if o.get("oracle")] == [True, True]


def test_vitb_schedule_changes_the_masked_row_count(lib):
    h, cfg = HISTORY["vitb32"], history_cfg("vitb32")
    B, M = h["B"], h["B"] * cfg.num_tokens
    R, kinds = [], [s[0] for s in h["steps"]]
    for i, (kind, arg, *opt) in enumerate(h["steps"]):
        x, mask, host = history_batch("vitb32", i)
        assert x.shape[0] == mask.shape[0] == (B if kind == "step" else arg)
        if kind != "step":
            assert arg < B                                   # the eval forward runs on the training engine, at another batch size
            continue
        n = int(mask.sum())
        r = (n + 63) // 64 * 64 if host else 0               # uvit_step_begin: R = roundup(n_rows_hint, 64), taken when 512 <= R < B x tokens
        assert r == 0 or 512 <= r < M
        if host:
            assert n == opt[0]["masked"] and len(set(mask.flatten(1).sum(1).tolist())) > 4       # ragged
        R.append(r)
    assert len(set(R) - {0}) >= 3
    assert any(0 < b < a for a, b in zip(R, R[1:])), "no shrink of the compact row count between consecutive steps"
    assert any(a > 0 and b == 0 and c > 0 for a, b, c in zip(R, R[1:], R[2:])), "no dense step between two compact ones"
    e = kinds.index("eval")
    assert 0 < e < len(kinds) - 1 and kinds[e - 1] == kinds[e + 1] == "step"
    ks = np.stack([k for _, _, k in counts(lib, "vitb32")])
    assert ((ks > 0) & (ks < B)).any(2).any(1).all(), "every step runs sample lists"
    assert (np.diff(ks[:, -1, 0]) != 0).any() and (np.diff(ks[:, -2, 1]) != 0).any()


def test_two_stream_schedule_moves_the_stream_offset(lib):
    B = HISTORY["tiny2"]["B"]
    ks = [k for _, _, k in counts(lib, "tiny2")]
    lists = lambda m, c: m > 0 and c > 0 and (m < B or c < B)                       # noqa: E731  (both streams' lists run: ROWS_LIST2)
    # on one layer the mean stream's MLP list shrinks while the covariance stream's grows, both steps running the stacked lists
    assert any(lists(a[l, 1], a[l, 3]) and lists(b[l, 1], b[l, 3]) and b[l, 1] < a[l, 1] and b[l, 3] > a[l, 3]
               for a, b in zip(ks, ks[1:]) for l in range(a.shape[0]))
    assert any((k[:, [1, 3]] == 0).any() for k in ks), "no step with an empty MLP list"


def test_hd80_schedule_changes_k(lib):
    ks = [k for _, _, k in counts(lib, "hd80")]
    assert len(ks) == 3 and history_cfg("hd80").head_dim == 80
    att = [int(k[-1, 0]) for k in ks]
    assert len(set(att)) == 3 and all(0 < a for a in att) and att[1] < att[0] and att[2] < att[1]
