"""GPU: the LayerScale gradient from the weight gradient (uvit_op_ls_dgamma, uvit_engine_set_ls_saved_y).

  * the kernel against the float64 evaluation of the same formula from the same inputs (tests/lsgrad_ref.py), under the derived bound
    |err_j| <= (K + NREP + 2) 2^-23 (sum_k |W_jk dW_jk| + |b_j| sum |db|) / |gamma_j|;
  * the launches the engine now makes with a NULL pointer -- the residual epilogue without its bf16 branch output, the LayerScale rider
    without y / dgamma -- give bit for bit what the launches with the pointer give;
  * one step, and a second one behind it, with the saved-y path on and off in the four walks the engine has: the gamma gradients of both
    paths meet the bound tests/test_gpu_model.py / tests/test_gpu_dist.py put on them against the oracle, every other gradient agrees
    between the paths to the tolerance those files use for "same computation, different launch" (1e-4, max-norm and relative L2).

The step set-ups use the tiny fixture shapes (tests/golden/model_t48.npz, dist_d48.npz: 48 px, C = 128, depth 2, B = 3).  The masked-row
last block needs at least 512 compact rows (uvit_step_begin), which those shapes cannot have: that set-up runs the same two blocks at
224 px with B = 4 (788 token rows, 480 masked -> 512 compact rows), the smallest shape that takes the path.

Measured on an MI355X (the file runs in 4 s; `pytest -s` prints the figures): kernel, worst |err| / bound 1.6e-3 (K = 256) and 3.1e-4
(K = 1024); gamma gradients against the oracle, relative L2 over the four set-ups: 4.2e-3 .. 7.4e-3 from the weight gradient,
4.3e-3 .. 7.2e-3 from the saved branch outputs (bound 2e-2; two-stream 4e-2).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lsgrad_ref as G
from gpu_util import assert_grads_close, grad_errors, native_model, native_steps, native_trainer, oracle_state
from oracle import vit_oracle as vo
from oracle import vit_oracle_dist as vd
from oracle.closed_form import closed_form_images, exact_masks

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NREP = 32


@pytest.fixture(scope="module")
def L():
    from uncertainty_vit_amd import native
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return native.lib()


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    assert rc == 0, f"libuvit returned {rc}"


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
def _dgamma_set(Cd, K, seed):
    """(W bf16 values, dW, b, db [NREP, C]) on the CPU: every replica holds something else."""
    return ((rnd(Cd, K, seed=seed) * K ** -0.5).to(BF16).to(F32), rnd(Cd, K, seed=seed + 1), rnd(Cd, seed=seed + 2),
            rnd(NREP, Cd, seed=seed + 3) * torch.arange(1, NREP + 1)[:, None] / NREP)


@pytest.mark.parametrize("zero_col", [None, 77])
@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("K", [256, 1024])
def test_ls_dgamma_against_float64(L, K, nsets, zero_col):
    from uncertainty_vit_amd.native import LsDgammaSet
    Cd, stride = 256, 256 + 12
    sets = [_dgamma_set(Cd, K, 1000 * K + 10 * q) for q in range(nsets)]
    gamma = torch.tensor([1e-4, 1.0, -3.0, 1e-20])[torch.randint(0, 4, (Cd,), generator=torch.Generator().manual_seed(K + nsets))]
    if zero_col is not None:
        gamma[zero_col] = 0.0
    want, Sabs = G.dgamma_from_wgrad(sets, gamma)
    bound = G.dgamma_bound(Sabs, gamma, K, NREP)
    # accumulate call: the destination already holds something, no larger than S / |gamma| (lsgrad_ref.dgamma_bound)
    live = gamma != 0
    dest0 = torch.where(live, (rnd(Cd, seed=5).clamp(-1, 1) * 0.5).double() * Sabs / gamma.double().abs().clamp_min(1e-30), torch.ones(Cd, dtype=torch.float64)).float()
    assert torch.isfinite(dest0).all() and (dest0 != 0).all()
    keep = []                                                              # device operands stay alive until the launch has run
    arr = (LsDgammaSet * nsets)()
    for q, (W, dW, b, db) in enumerate(sets):
        dbd = torch.full((NREP, stride), 7.0)
        dbd[:, :Cd] = db
        ts = [W.to(BF16).cuda(), dW.cuda(), b.cuda(), dbd.cuda()]
        keep += ts
        arr[q].W, arr[q].dW, arr[q].b, arr[q].db = (t.data_ptr() for t in ts)
    dest = torch.full((Cd + 4,), 3.5)
    dest[:Cd] = dest0
    dest, g, flag = dest.cuda(), gamma.cuda(), torch.zeros(2, dtype=torch.int32, device="cuda")
    ok(L.uvit_op_ls_dgamma(C.byref(arr), nsets, P(g), P(dest), P(flag), Cd, K, NREP, stride, S()))
    got = dest.cpu().double()
    assert (got[Cd:] == 3.5).all() and flag[1].item() == 0
    err = (got[:Cd] - (want + dest0.double())).abs()
    ratio = (err[live] / bound[live]).max().item()
    print(f"ls_dgamma K={K} sets={nsets}: worst |err| / bound = {ratio:.2e}")
    assert (err[live] <= bound[live]).all(), ratio
    if zero_col is None:
        assert flag[0].item() == 0
    else:
        assert got[zero_col] == 0.0 and flag[0].item() == 1               # 0 / 0: the column gets 0 and the flag is raised
    del keep


def test_ls_dgamma_refuses(L):
    from uncertainty_vit_amd.native import LsDgammaSet
    t = torch.zeros(64, device="cuda")
    arr = (LsDgammaSet * 2)()
    for q in range(2):
        arr[q].W = arr[q].dW = arr[q].b = arr[q].db = t.data_ptr()
    assert L.uvit_op_ls_dgamma(C.byref(arr), 3, P(t), P(t), P(t), 8, 8, 1, 8, S()) == -1
    assert L.uvit_op_ls_dgamma(C.byref(arr), 1, P(t), P(t), None, 8, 8, 1, 8, S()) == -1
    assert L.uvit_op_ls_dgamma(C.byref(arr), 1, P(t), P(t), P(t), 8, 12, 1, 8, S()) == -2          # K % 8
    assert L.uvit_op_ls_dgamma(C.byref(arr), 1, P(t), P(t), P(t), 8, 8, 65, 8, S()) == -2          # more replicas than lanes
    arr[1].db = 0
    assert L.uvit_op_ls_dgamma(C.byref(arr), 2, P(t), P(t), P(t), 8, 8, 1, 8, S()) == -1


# ---- NULL-pointer variants: bit for bit --------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# (nt_variant, kernel the plan must name: 0 = 128x128, 1 = 256-row, 3 = 320-row, M, N, row list)
RESID_CASES = [(0, 0, 200, 256, False), (1, 1, 1024 + 72, 256, False), (1, 1, 1024 + 72, 768, False), (5, 3, 1024 + 72, 256, False),
               (5, 3, 1024 + 72, 768, False), (5, 3, 1024 + 72, 768, True)]


@pytest.mark.parametrize("variant,kernel,M,N,row_list", RESID_CASES)
def test_resid_epilogue_without_out2_is_bit_identical(L, variant, kernel, M, N, row_list):
    from uncertainty_vit_amd.native import GemmEpilogue, GemmNtPlanInfo, Tuning
    K, tokens = 128, 7
    Rs = (M // tokens + 20) * tokens
    a, wt = rnd(M, K, seed=1).to(BF16).cuda(), (rnd(N, K, seed=2) * K ** -0.5).to(BF16).cuda()
    bias, gamma, resid = (rnd(N, seed=3) * 0.1).cuda(), (rnd(N, seed=4) * 0.1 + 0.5).cuda(), rnd(Rs, N, seed=5).cuda()
    scale = torch.tensor([0.0 if i % 3 == 1 else 1.25 for i in range(Rs // tokens)]).cuda()
    rowcount = M - 37
    rowmap = torch.randperm(Rs, generator=torch.Generator().manual_seed(4))[:M]
    rowmap[rowcount:] = -1
    rm, rc = rowmap.to(torch.int32).cuda(), torch.tensor([rowcount], dtype=torch.int32).cuda()
    tu, info = Tuning.default(nt_variant=variant), GemmNtPlanInfo()
    ok(L.uvit_op_gemm_nt_plan(3, M, N, K, K, K, N, int(row_list), C.byref(tu), torch.cuda.get_device_properties(0).multi_processor_count,
                              C.byref(info)))
    assert info.kernel == kernel and info.tail_rows == 0
    outs = []
    for with_out2 in (True, False):
        out, out2 = torch.full((Rs, N), 7.0, device="cuda"), torch.full((Rs, N), 7.0, dtype=BF16, device="cuda")
        ep = GemmEpilogue()
        ep.out, ep.bias, ep.gamma, ep.resid, ep.rowscale = (t.data_ptr() for t in (out, bias, gamma, resid, scale))
        ep.out2 = out2.data_ptr() if with_out2 else 0
        ep.ldo, ep.tokens = N, tokens
        if row_list:
            ok(L.uvit_op_gemm_nt_rows(3, P(a), P(wt), M, N, K, K, K, C.byref(ep), P(rm), P(rc), C.byref(tu), S()))
        else:
            ok(L.uvit_op_gemm_nt_tuned(3, P(a), P(wt), M, N, K, K, K, C.byref(ep), C.byref(tu), None, S()))
        torch.cuda.synchronize()
        outs.append((out, out2))
    (o1, y1), (o0, y0) = outs
    assert same_bits(o1, o0)
    written = rowmap[:rowcount] if row_list else torch.arange(M)
    assert (o1[written.cuda()] != 7.0).any(1).all() and (y1[written.cuda()].float() != 7.0).any(1).all()
    assert (y0.float() == 7.0).all()                                       # nothing was stored through the NULL pointer's neighbours


def _rider(y, gamma, rowscale, dy, dgamma, dbias, tokens, pos=None, cnt=None):
    from uncertainty_vit_amd.native import LsRider
    r = LsRider()
    for k, v in dict(y=y, gamma=gamma, rowscale=rowscale, dy=dy, dgamma=dgamma, dbias=dbias, pos=pos, cnt=cnt).items():
        setattr(r, k, 0 if v is None else v.data_ptr())
    r.tokens = tokens
    return r


@pytest.mark.parametrize("walk", ["dense", "samples", "rows", "ls_bwd", "ls_bwd_rows"])
def test_rider_without_y_is_bit_identical(L, walk):
    """dy, dx, dw, db and dbias of the rider launched with y = dgamma = NULL equal those of the launch with y, bit for bit: the dense walk, the
    drop-path sample lists (own list and rider list differ, pad rows filled) and the row list of the masked-row last block (rider compact by its
    sample list), then the rider on its own (dense and over a row list).  C = 256, 3 samples of 5 tokens; NREP replicas, so that no two
    workgroups add into one word and the column sums have one summation order."""
    Cd, tokens, B = 256, 5, 3
    M = B * tokens
    dy_in, x = rnd(M, Cd, seed=11).to(BF16).cuda(), rnd(M, Cd, seed=12).cuda()
    xd = x.double()
    mean, rstd = xd.mean(-1).float().contiguous(), ((xd.var(-1, unbiased=False) + 1e-6) ** -0.5).float().contiguous()
    w, dres, y = (1 + 0.1 * rnd(Cd, seed=13)).cuda(), rnd(M, Cd, seed=14).cuda(), rnd(M, Cd, seed=15).to(BF16).cuda()
    gamma, scale = (0.1 + 0.05 * rnd(Cd, seed=16)).cuda(), torch.tensor([1.25, 0.0, 1.25]).cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()             # noqa: E731
    own_pos, rid_pos = i32([0, 1, -1]), i32([0, -1, 1])                    # the LayerNorm's branch kept samples 0, 1; the rider's 0, 2
    rid_cnt = i32([2 * tokens])
    rowidx, count = i32([14, 3, 0, 7, 10, 11, 2, 5]), i32([6])
    stride = Cd + 12
    res = []
    for with_y in (True, False):
        dx, dyn = torch.full((M, Cd), 7.0, device="cuda"), torch.full((64, Cd), 7.0, dtype=BF16, device="cuda")
        acc = {k: torch.zeros(NREP, stride, device="cuda") for k in ("dw", "db", "dgamma", "dbias")}
        yy, dg = (y, acc["dgamma"]) if with_y else (None, None)
        if walk in ("ls_bwd", "ls_bwd_rows"):
            r = _rider(yy, gamma, scale, dyn, dg, acc["dbias"], tokens)
            if walk == "ls_bwd":
                ok(L.uvit_op_ls_bwd(P(dres), C.byref(r), M, Cd, NREP, stride, None, None, S()))
            else:
                ok(L.uvit_op_ls_bwd(P(dres), C.byref(r), 64, Cd, NREP, stride, P(rowidx), P(count), S()))
        else:
            if walk == "dense":
                r, args = _rider(yy, gamma, scale, dyn, dg, acc["dbias"], tokens), (None, None, None)
                d, mu, rs, rows = dy_in, mean, rstd, M
            elif walk == "samples":
                r, args = _rider(yy, gamma, scale, dyn, dg, acc["dbias"], tokens, rid_pos, rid_cnt), (None, None, P(own_pos))
                d, mu, rs, rows = dy_in[:2 * tokens], mean[:2 * tokens].contiguous(), rstd[:2 * tokens].contiguous(), M
            else:
                r, args = _rider(yy, gamma, scale, dyn, dg, acc["dbias"], tokens, rid_pos), (P(rowidx), P(count), None)
                ri = rowidx.long()
                d, mu, rs, rows = dy_in[:8], mean[ri].contiguous(), rstd[ri].contiguous(), 8
            ok(L.uvit_op_ln_bwd_walk(P(d), P(x), P(mu), P(rs), P(w), P(dres), P(dx), P(acc["dw"]), P(acc["db"]), rows, Cd, NREP, stride,
                                     args[0], args[1], args[2], C.byref(r), S()))
        torch.cuda.synchronize()
        res.append(dict(dx=dx, dy=dyn, dw=acc["dw"], db=acc["db"], dbias=acc["dbias"], dgamma=acc["dgamma"]))
    a, b = res
    for k in ("dx", "dy", "dw", "db", "dbias"):
        assert same_bits(a[k], b[k]), k
    assert (a["dy"].float() != 7.0).any() and a["dbias"].abs().sum() > 0 and a["dgamma"].abs().sum() > 0
    assert b["dgamma"].abs().sum() == 0
    if walk not in ("ls_bwd", "ls_bwd_rows"):
        assert (a["dx"] != 7.0).any() and a["dw"].abs().sum() > 0
    # y without dgamma (or the reverse) is refused before the device is touched
    bad = _rider(y, gamma, scale, res[0]["dy"], None, res[0]["dbias"], tokens)
    assert L.uvit_op_ls_bwd(P(dres), C.byref(bad), M, Cd, NREP, stride, None, None, S()) == -1


# ---- the step --------------------------------------------------------------------------------------------------------------------
def _tiny(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name))
    img, dim, depth, heads, B, n_mask, _ = [int(v) for v in fx["cfg"]]
    return dict(img_size=img, embed_dim=dim, depth=depth, num_heads=heads, init_values=float(fx["init_values"])), B, n_mask, \
        [int(v) for v in fx["target_layers"]]


SEED, IT = 1234, 3      # kept samples of layer 1 at B = 3, drop_path 0.5: base (attn 1, mlp 1), two-stream MLP lists (mean 2, cov 2)
SETUPS = ["lists", "no_lists", "masked_rows", "two_stream"]


@pytest.mark.parametrize("setup", SETUPS)
def test_step_with_and_without_saved_branch_outputs(golden_dir, setup):
    two = setup == "two_stream"
    kw, B, n_mask, tl = _tiny(golden_dir, "dist_d48.npz" if two else "model_t48.npz")
    kw.update(drop_path_rate=0.5, attn_drop_rate=0.1)
    host_mask = False
    if setup == "masked_rows":
        kw.update(img_size=224)
        B, n_mask, host_mask = 4, 120, True
    cfg = vo.VitConfig(**kw)
    P_ = cfg.num_patches
    x, mask = closed_form_images("lsgrad/" + setup, B, cfg.img_size), exact_masks(B, P_, n_mask, 61)
    extra = dict(stochastic=True, lam=1e-2) if two else {}
    res = {}
    for saved in (False, True):
        model, sd = native_model(cfg, two_stream=two)
        model.ls_saved_y = saved
        model.drop_path_rows = setup != "no_lists"
        ema, opt = native_trainer(model)
        model.train()
        torch.manual_seed(SEED)
        batch = (x, mask) if host_mask else (x.cuda(), mask.cuda())
        st = native_steps(model, ema, opt, [batch], tl, start=IT, **extra)
        e = model._engine
        assert e.ls_saved_y == saved and e.drop_path_rows == (setup != "no_lists")
        assert (e.compact_rows() > 0) == (setup == "masked_rows")
        grads = {n: q.grad.detach().float().cpu().clone() for n, q in model.named_parameters() if q.grad is not None}
        st += native_steps(model, ema, opt, [batch], tl, start=IT + 1, **extra)      # a second step behind the first, other draws
        assert all(np.isfinite(s["loss"]) and np.isfinite(s["grad_norm"]) for s in st)
        assert e.ws_tensor("poisoned", 0, (1,), torch.int32).item() == 0
        res[saved] = (st, grads, sd)
    (s_new, g_new, sd), (s_old, g_old, _) = res[False], res[True]
    assert s_new[0]["loss"] == pytest.approx(s_old[0]["loss"], rel=1e-6)
    # the oracle with the kernels' counter-based masks replayed
    aseed = int(vo._mix32(np.uint32(SEED) ^ np.uint32((IT * 0x85EBCA6B + 0x1234567) & 0xFFFFFFFF)))
    attn = [vo.attn_keep_mask(aseed, l, B, cfg.num_heads, P_ + 1, 0.1) for l in range(cfg.depth)]
    p, em, m1, v1 = oracle_state(sd)
    if two:
        drop = vd.DistDropState(path=vd.drop_path_scales(SEED, IT, cfg, B), attn=attn)
        ref, _, _, _ = vd.train_step(p, em, m1, v1, cfg, vo.StepHParams(target_layers=tuple(tl)), x, mask, 1, lam=1e-2, drop=drop)
        dropped = any(t is not None and (t == 0).any() for row in drop.path for t in row)
    else:
        p1, p2 = vo.drop_path_scales(SEED, IT, cfg, B)
        ref = vo.train_step(p, em, m1, v1, cfg, vo.StepHParams(target_layers=tuple(tl)), x, mask, 1, drop=vo.DropState(path1=p1, path2=p2, attn=attn))
        dropped = any(t is not None and (t == 0).any() for t in p1 + p2)
    assert dropped, "the set-up should drop a sample"
    gammas = [n for n in ref.grads if n.endswith("gamma_1") or n.endswith("gamma_2")]
    assert len(gammas) == 2 * cfg.depth
    for tag, g in (("from wgrad", g_new), ("saved y  ", g_old)):
        errs = grad_errors(g, ref.grads, gammas)
        print(f"[{setup}] gamma gradients {tag} vs oracle (max-norm ratio, relative L2):", {n: (f"{a:.2e}", f"{b:.2e}") for n, (a, b) in errs.items()})
    # the bound of the existing step tests on these tensors (test_gpu_model.py: 5e-2 / 2e-2; test_gpu_dist.py, non-bias tensors: 5e-2 / 4e-2)
    l2 = 4e-2 if two else 2e-2
    assert_grads_close(g_new, ref.grads, names=gammas, max_tol=5e-2, l2_tol=l2, what=f"[{setup}, gamma from wgrad] ")
    assert_grads_close(g_old, ref.grads, names=gammas, max_tol=5e-2, l2_tol=l2, what=f"[{setup}, gamma from saved y] ")
    # every other gradient: the same launches on the same operands, atomics in another order
    others = [n for n in g_old if n not in gammas and float(g_old[n].abs().max()) > 0]
    assert len(others) > 10
    assert_grads_close(g_new, g_old, names=others, max_tol=1e-4, l2_tol=1e-4, what=f"[{setup}, other gradients, new vs saved y] ")
    for n in g_old:
        if n not in gammas and float(g_old[n].abs().max()) == 0:
            assert float(g_new[n].abs().max()) == 0, n


def test_zero_gamma_poisons_the_step_and_the_switch_serves_it(golden_dir):
    """gamma_j == 0: the default path writes 0 for that entry and raises the engine's poisoned flag (the weights stay where they were);
    with the saved branch outputs the step runs and that entry gets its gradient."""
    kw, B, n_mask, tl = _tiny(golden_dir, "model_t48.npz")
    cfg = vo.VitConfig(**kw)
    x, mask = closed_form_images("lsgrad/zero", B, cfg.img_size).cuda(), exact_masks(B, cfg.num_patches, n_mask, 62).cuda()
    out = {}
    for saved in (False, True):
        model, _ = native_model(cfg)
        with torch.no_grad():
            model.blocks[1].gamma_2[5] = 0.0
        model.ls_saved_y = saved
        ema, opt = native_trainer(model)
        before = model._arena.clone()
        native_steps(model, ema, opt, [(x, mask)], tl)
        g = model.blocks[1].gamma_2.grad.detach().float().cpu()
        out[saved] = (g, model._engine.ws_tensor("poisoned", 0, (1,), torch.int32).item(), torch.equal(model._arena, before))
    (g_new, flag_new, frozen_new), (g_old, flag_old, frozen_old) = out[False], out[True]
    assert flag_new == 1 and frozen_new and g_new[5] == 0.0
    assert flag_old == 0 and not frozen_old and g_old[5] != 0.0
    live = torch.arange(g_old.numel()) != 5
    assert (g_new[live] - g_old[live]).norm() <= 2e-2 * g_old[live].norm()
