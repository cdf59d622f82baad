"""CPU: what tests/test_gpu_epoch.py trusts -- the float64 update it compares the device with, the properties of the epoch it runs, and
the oracle's losses over that epoch."""
import ctypes

import pytest
import torch

from gpu_util import EPOCH, epoch_batch, epoch_cfg, epoch_table, expected_update, oracle_epoch

f32 = lambda v: ctypes.c_float(float(v)).value  # noqa: E731


def test_expected_update_against_torch_adamw_and_clip():
    """expected_update = clip_grad_norm_ + torch.optim.AdamW over the (decay, no-decay) groups + the EMA formula, three steps with another
    lr / weight decay / gradient each; bounds of test_ema_adamw_sumsq_against_torch (rtol 1e-5, atol 1e-6).  torch runs in float64 and is
    given the scalars as the C ABI carries them, rounded to float32 (with an unrounded beta2, 1 - beta2 and so exp_avg_sq differ by 1.3e-5):
    what is left is the order of float64 operations (measured: params 4.4e-16 max abs, moments 1.7e-16 of their maximum)."""
    n, n_decay, betas, eps = 64 * 1000, 64 * 600, (f32(0.9), f32(0.999)), f32(1e-8)
    gen = torch.Generator().manual_seed(60)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    g0 = torch.randn(n, generator=gen, dtype=torch.float64) * 3
    e0 = torch.randn(n, generator=gen, dtype=torch.float64)
    refd, refn = p0[:n_decay].clone().requires_grad_(True), p0[n_decay:].clone().requires_grad_(True)
    opt = torch.optim.AdamW([{"params": [refd], "weight_decay": 0.05}, {"params": [refn], "weight_decay": 0.0}], lr=2e-3, betas=betas, eps=eps)
    P, M, V, E = p0, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), e0
    for step, (lr, wd, d, gs) in enumerate([(2e-3, 0.05, 0.9998, 1.0), (5e-4, 0.2, None, 1e-3), (1.5e-3, 0.01, 0.99, 2.0)], 1):
        g = g0 * gs                                       # step 2: a norm below the clip threshold (coefficient 1)
        refd.grad, refn.grad = g[:n_decay].clone(), g[n_decay:].clone()
        norm = torch.nn.utils.clip_grad_norm_([refd, refn], 3.0)
        for grp in opt.param_groups:
            grp["lr"] = f32(lr)
        opt.param_groups[0]["weight_decay"] = f32(wd)
        opt.step()
        E_before = E
        P, M, V, E, gn = expected_update(P, M, V, E, g, lr, wd, d, step, n_decay, 3.0, betas, eps)
        assert gn == pytest.approx(float(norm), rel=1e-12)
        assert (gn > 3.0) == (step != 2)
        ref = torch.cat([refd, refn]).detach()
        print(f"step {step}: params max abs error {float((P - ref).abs().max()):.2e}")
        torch.testing.assert_close(P, ref, rtol=1e-5, atol=1e-6)
        st = [opt.state[refd], opt.state[refn]]
        for mine, key in ((M, "exp_avg"), (V, "exp_avg_sq")):
            r = torch.cat([s[key] for s in st])
            print(f"step {step}: {key} max error / max {float((mine - r).abs().max() / r.abs().max()):.2e}")
            torch.testing.assert_close(mine / r.abs().max(), r / r.abs().max(), rtol=1e-5, atol=1e-6)
        if d is None:
            assert E is E_before or torch.equal(E, E_before)
        else:
            torch.testing.assert_close(E, f32(d) * E_before + (1 - f32(d)) * P, rtol=1e-12, atol=0)
    assert not torch.equal(P[n_decay:], p0[n_decay:])


def test_epoch_definition_has_the_properties_the_gpu_test_relies_on():
    E = EPOCH
    ring = 4                                              # slots of train_one_epoch's pinned metrics ring
    assert E["start_steps"] == 3 and E["n_iters"] == 9 and E["n_iters"] > 2 * ring          # step != it; more than two laps
    assert (E["ema_start_at"], E["decay_init"], E["decay"], E["start_lr_decay_at_step"]) == (7, 0.99, 0.9998, 9)
    its = range(E["start_steps"], E["start_steps"] + E["n_iters"])
    assert len(E["lr"]) >= its[-1] + 1 and len(E["wd"]) >= its[-1] + 1
    for name in ("lr", "wd"):
        t = E[name]
        ratios = [max(a, b) / min(a, b) for a, b in zip(t, t[1:])]
        assert min(t) > 0 and min(ratios) >= 2.0, (name, ratios)
        ups = [b > a for a, b in zip(t, t[1:])]
        assert any(ups) and not all(ups), name + " is monotone"
        assert len(set(t[its[0]:its[-1] + 1])) == E["n_iters"], name + ": two iterations of the epoch share a value"
    sc = epoch_table()
    assert len(sc) == E["n_iters"]
    assert [s[0] for s in sc] == [f32(E["lr"][it]) for it in its], "lr is indexed by the global iteration"
    assert [s[1] for s in sc] == [f32(E["wd"][it]) for it in its], "weight decay is indexed by the global iteration"
    decays = {s[2] for s in sc if s[2] >= 0}
    assert not ({s[0] for s in sc} & ({s[1] for s in sc} | decays)) and not ({s[1] for s in sc} & decays), "a value occurs in two rows"
    anneal = lambda it: f32(E["decay_init"] + it * (E["decay"] - E["decay_init"]) / E["ema_start_at"])  # noqa: E731
    regimes = {"annealed (it 3..6)": [s[2] for s in sc[0:4]] == [anneal(it) for it in (3, 4, 5, 6)] and len({s[2] for s in sc[0:4]}) == 4,
               "frozen at the value of it 6 (it 7..9)": [s[2] for s in sc[4:7]] == [anneal(6)] * 3,
               "skipped (it 10..11)": [s[2] for s in sc[7:9]] == [-1.0, -1.0]}
    assert all(regimes.values()), regimes
    # the batches: (B, 3, 48, 48) images and (B, 3, 3) masks with the listed masked patches per image
    cfg = epoch_cfg()
    assert (cfg.img_size, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.init_values) == (48, 128, 2, 2, 0.1) and E["B"] == 3
    assert cfg.drop_path_rate == 0 and cfg.attn_drop_rate == 0 and E["target_layers"] == [1]
    for i in range(E["n_iters"]):
        x, m = epoch_batch(i)
        assert x.shape == (3, 3, 48, 48) and m.shape == (3, 3, 3) and m.sum(dim=(1, 2)).tolist() == [E["n_mask"][i]] * 3


def test_oracle_epoch_losses_are_far_apart():
    """Consecutive losses of the oracle's epoch differ by >= 10 % (five times the 2e-2 the GPU test holds later-step losses to): a loss
    attributed to a neighbouring iteration cannot pass.  Measured: 0.281 0.214 0.289 0.192 0.285 0.192 0.280 0.183 0.276, the closest
    pair 24 % apart."""
    loss, gnorm = oracle_epoch()
    print("oracle epoch losses", [f"{v:.4f}" for v in loss], "grad norms", [f"{v:.3f}" for v in gnorm])
    assert len(loss) == EPOCH["n_iters"] and all(0 < v < 10 for v in loss)
    gaps = [abs(a - b) / max(a, b) for a, b in zip(loss, loss[1:])]
    print("relative gaps", [f"{g:.3f}" for g in gaps])
    assert min(gaps) >= 0.10, gaps
