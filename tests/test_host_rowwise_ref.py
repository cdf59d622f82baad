"""CPU (no GPU): pins tests/rowwise_ref.py, the float64 restatements and the comparator tests/test_gpu_rowwise.py judges the kernels by.

  * every restatement equals float64 autograd on the same inputs to 1e-12 relative (F.layer_norm for the LayerNorm, the explicit
    x + dp gamma y for the LayerScale + DropPath rider);
  * for every (operator, shape) of the GPU file a float32 restatement, evaluated in another order, PASSES the comparator against
    the float64 reference: the bounds are not too tight;
  * a mutated result FAILS the same comparator: the last kept row dropped from a column sum, one sample's pos shifted by one, the last
    pad row left non-zero, one 64-row chunk of a bias sum moved to the other stream.  The any-order bound of a column sum grows
    like R^2 u, so at the 197-token shapes (R = 4531: bound ~ 1 against a dropped term ~ 1) it cannot tell a dropped row apart on
    random inputs; there the column-sum mutation runs on the exact family (where the comparison is equality), at the 7-token
    shapes (R = 77: bound ~ 3e-4) on both families;
  * the new entry points refuse what the launchers refuse, without a device.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import rowwise_ref as R
from rowwise_ref import BF16, F32, F64, Out

EPS = 1e-6
SHAPES = [(c, 7, 11) for c in (128, 260, 768, 1024, 1280, 1536, 2048)] + [(128, 197, 23), (768, 197, 23)]
FAMILIES = ("random", "exact")


def stats_of(x, family):
    if family == "exact":
        return torch.zeros(x.shape[0]), torch.ones(x.shape[0])
    xd = x.double()
    return xd.mean(-1).float(), ((xd.var(-1, unbiased=False) + EPS) ** -0.5).float()


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-300)).item()


def passes(op, ref, got):
    """The float32 results `got` (a dict of Outs whose .ref are the values), laid out as buffers, pass the comparator."""
    for k, o in ref.items():
        if isinstance(o, Out):
            R.compare(op, k, R.materialize(o, None if o.exact and k in ("xcopy", "pad2") else got[k].ref), o)


def fails(op, name, buf, out):
    with pytest.raises(AssertionError):
        R.compare(op, name, buf, out)


def drop_last_term(out, terms_last):
    """A column sum that missed its last row."""
    return (out.ref - terms_last.reshape(1, -1).double()).float()


# ---- the restatements against float64 autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Cd", [128, 260, 1280])
def test_layernorm_restatement_is_autograd(Cd):
    M = 21
    i = R.ln_inputs(M, Cd, "random", seed=1)
    x = i["x"].double().requires_grad_(True); w = i["w"].double().requires_grad_(True); b = i["b"].double().requires_grad_(True)
    y = F.layer_norm(x, (Cd,), w, b, EPS)
    y.backward(i["dy"].double())
    f = R.ln_fwd(i["x"], i["w"], i["b"], EPS, M)
    assert rel(f["y"].ref, y.detach()) < 1e-12 and rel(f["mean"].ref[:, 0], x.detach().mean(-1)) < 1e-12
    mean, rstd = f["mean"].ref[:, 0], f["rstd"].ref[:, 0]
    g = R.ln_bwd(i["dy"], i["x"], mean, rstd, i["w"], i["dres"], M)
    assert rel(g["dx"].ref, x.grad + i["dres"].double()) < 1e-12
    assert rel(g["dw"].ref[0], w.grad) < 1e-12 and rel(g["db"].ref[0], b.grad) < 1e-12
    g0 = R.ln_bwd(i["dy"], i["x"], mean, rstd, i["w"], None, M)
    assert rel(g0["dx"].ref, x.grad) < 1e-12


def test_dropped_sample_passes_dres_through_and_rider_is_autograd():
    """Two branches on a stream: x2 = x1 + dpb gamma_b y_b with x1 = x0 + dpa LN-branch(x0).  A sample the LayerNorm's branch dropped
    (dpa = 0, not in its compact list) gets dx = dres; the rider's dy, dgamma, dbias are the autograd gradients of the explicit
    x + dp gamma (y + bias) with the rider's own kept set."""
    Cd, tokens, B = 128, 7, 6
    M = B * tokens
    i = R.ln_inputs(M, Cd, "random", seed=2)
    ka, kb = R.kept_set("alternating", B), R.kept_set("first_dropped", B)
    dpb = R.rowscale_of(kb).double().repeat_interleave(tokens)[:, None]
    x = i["x"].double().requires_grad_(True); w = i["w"].double().requires_grad_(True); b = i["b"].double().requires_grad_(True)
    yb = i["y"].double().requires_grad_(True); gm = i["gamma"].double().requires_grad_(True); bias = torch.zeros(Cd, dtype=F64, requires_grad=True)
    ln = F.layer_norm(x, (Cd,), w, b, EPS)
    rows = torch.nonzero(ka.repeat_interleave(tokens)).flatten()
    # loss = <dy, ln rows of the kept samples> + <dres, x> (the gradient already on the stream); the rider's branch sees d = dx
    dres = i["dres"].double()
    loss = (ln[rows] * i["dy"].double()[rows]).sum() + (dres * x).sum()
    loss.backward()
    f = R.ln_fwd(i["x"], i["w"], i["b"], EPS, M, pos=R.pos_of(ka), tokens=tokens)
    out = R.ln_bwd(i["dy"][rows], i["x"], f["mean"].ref[:, 0], f["rstd"].ref[:, 0], i["w"], i["dres"], M, pos=R.pos_of(ka),
                   rider=dict(tokens=tokens, rowscale=R.rowscale_of(kb), pos=R.pos_of(kb), y=i["y"], gamma=i["gamma"]),
                   dy_next_rows=int(kb.sum()) * tokens)
    assert rel(out["dx"].ref, x.grad) < 1e-12 and rel(out["dw"].ref[0], w.grad) < 1e-12 and rel(out["db"].ref[0], b.grad) < 1e-12
    dropped = torch.nonzero(~ka.repeat_interleave(tokens)).flatten()
    assert torch.equal(out["passthrough_rows"], dropped) and torch.equal(out["dx"].ref[dropped], dres[dropped])
    d = x.grad.detach()
    (d * (dpb * gm * (yb + bias))).sum().backward()
    kept_b = torch.nonzero(kb.repeat_interleave(tokens)).flatten()
    assert rel(out["dy_next"].ref, yb.grad[kept_b]) < 1e-12
    assert rel(out["dgamma"].ref[0], gm.grad) < 1e-12 and rel(out["dbias_unrounded"], bias.grad) < 1e-12
    ls = R.ls_bwd(d.float(), i["y"], i["gamma"], R.rowscale_of(kb), tokens, M)
    d32 = d.float().double()
    gm.grad = None; bias.grad = None
    (d32 * (dpb * gm * (i["y"].double() + bias))).sum().backward()
    assert rel(ls["dgamma"].ref[0], gm.grad) < 1e-12 and rel(ls["dbias_unrounded"], bias.grad) < 1e-12


# ---- float32 passes, mutations fail --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cd,tokens,B", SHAPES)
def test_ln_fwd_float32_passes_and_mutations_fail(Cd, tokens, B):
    M, Rs = B * tokens, B * tokens + 40
    i = R.ln_inputs(Rs, Cd, "random", seed=100)
    rowidx = torch.randperm(Rs, generator=torch.Generator().manual_seed(1))[:M]
    for kw in (dict(), dict(rowidx=rowidx, count=M - 5), dict(rowidx=rowidx, count=M - 5, stats=False)):
        f = lambda dt: R.ln_fwd(i["x"], i["w"], i["b"], EPS, M, dt=dt, **kw)      # noqa: E731
        ref = f(F64)
        passes("ln_fwd", ref, f(F32))
    buf = R.materialize(ref["y"]); buf[M - 1] = 1.0                          # the last pad row left non-zero
    fails("ln_fwd", "y", buf, ref["y"])
    for kept in R.KEPT_SETS:
        pos = R.pos_of(R.kept_set(kept, B))
        f = lambda dt, p=pos: R.ln_fwd(i["x"][:M], i["w"], i["b"], EPS, M, pos=p, tokens=tokens, dt=dt)      # noqa: E731
        ref = f(F64)
        passes("ln_fwd", ref, f(F32))
        bad = pos.clone(); last = int(torch.nonzero(pos >= 0)[-1]); bad[last] += 1      # one sample's pos shifted by one
        mut = f(F64, bad)
        fails("ln_fwd", "y", R.materialize(mut["y"]), ref["y"])
        fails("ln_fwd", "mean", R.materialize(mut["mean"]), ref["mean"])
        if kept != "all":                                                   # a dropped sample not copied to xcopy
            buf = R.materialize(ref["xcopy"])
            R.bits(buf)[int(torch.nonzero(pos < 0)[0]) * tokens] = R.SENT32
            fails("ln_fwd", "xcopy", buf, ref["xcopy"])


def ln_bwd_variants(Cd, tokens, B, family):
    """(name, stream rows, kwargs of rowwise_ref.ln_bwd minus the operands) of the launches of tests/test_gpu_rowwise.py."""
    M, ex = B * tokens, family == "exact"
    rowidx = torch.randperm((B + 5) * tokens, generator=torch.Generator().manual_seed(2))[:M]
    keep5 = R.kept_set("alternating", B + 5)
    sc5 = R.rowscale_of(keep5, exact=ex)
    dense = torch.arange(M)
    yield "rows dense", dense, dict()
    yield "rows dense, no dres", dense, dict(dres=None)
    yield "rows list", rowidx, dict(rowidx=rowidx, count=M - 9)
    yield "rows dense + rider", dense, dict(rider=dict(tokens=tokens, rowscale=sc5), dy_next_rows=(B + 5) * tokens)
    yield "rows dense + rider without rowscale", dense, dict(rider=dict(tokens=tokens, rowscale=None), dy_next_rows=(B + 5) * tokens)
    yield "rows list + compact rider", rowidx, dict(rowidx=rowidx, count=M - 9, rider=dict(tokens=tokens, rowscale=sc5, pos=R.pos_of(keep5)),
                                                    dy_next_rows=int(keep5.sum()) * tokens)
    rows_of = lambda k: torch.nonzero(k.repeat_interleave(tokens)).flatten()      # noqa: E731
    for kept in R.KEPT_SETS:
        k = R.kept_set(kept, B)
        yield f"samples {kept}, no rider", rows_of(k), dict(pos=R.pos_of(k), rider=dict(tokens=tokens))
    for own, rid, pad_base in (("alternating", "first_dropped", 0), ("all", "last_dropped", 3 * tokens), ("one", "alternating", 0),
                               ("first_dropped", "all", 0)):
        ko, kr = R.kept_set(own, B), R.kept_set(rid, B)
        cnt = int(kr.sum()) * tokens
        yield f"samples {own} + rider {rid}", rows_of(ko), dict(
            pos=None if own == "all" else R.pos_of(ko), dy_next_rows=(pad_base + cnt + 63) // 64 * 64 - pad_base,
            rider=dict(tokens=tokens, rowscale=R.rowscale_of(kr, exact=ex), pos=R.pos_of(kr), cnt=cnt, pad_base=pad_base, pad2_cols=3 * Cd))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Cd,tokens,B", SHAPES)
def test_ln_bwd_float32_passes_and_mutations_fail(Cd, tokens, B, family):
    M, Rs, ex = B * tokens, (B + 5) * tokens, family == "exact"
    i = R.ln_inputs(Rs, Cd, family, seed=200)
    mean, rstd = stats_of(i["x"], family)
    sums_tell = ex or tokens == 7                                           # see the module docstring
    for name, a_rows, kw in ln_bwd_variants(Cd, tokens, B, family):
        kw = dict(kw)
        samples = name.startswith("samples")
        x, dres = (i["x"][:M], i["dres"][:M]) if samples else (i["x"], i["dres"])
        if "dres" in kw:
            dres = kw.pop("dres")
        rider = kw.pop("rider", None)
        if rider is not None and "rowscale" in rider:
            rider = dict(rider, y=i["y"][:len(x)], gamma=i["gamma"])

        def f(dt, rider=rider, **over):
            a = dict(kw, **over)
            return R.ln_bwd(i["dy"][a_rows], x, mean[a_rows], rstd[a_rows], i["w"], dres, M, rider=rider, exact=ex, dt=dt, **a)

        ref, got = f(F64), f(F32)
        passes(f"ln_bwd {name}", ref, got)
        # a LayerNorm gradient that misses the last kept row
        last = a_rows[(kw.get("count") or len(a_rows)) - 1]
        if sums_tell:
            fails(name, "db", drop_last_term(ref["db"], i["dy"][last]), ref["db"])
        if "dy_next" in ref:
            stored = R.materialize(ref["dy_next"], got["dy_next"].ref)
            R.compare(name, "dbias", stored[ref["dy_next_idx"]].float().sum(0), R.stored_colsum(stored, ref["dy_next_idx"], ex))
            idx = ref["dy_next_idx"]
            if sums_tell and len(idx):                                      # a LayerScale gradient that misses the last kept row
                fails(name, "dbias", (stored[idx[:-1]].double().sum(0)).float(), R.stored_colsum(stored, idx, ex))
                e_last = ref["dy_next"].ref[idx[-1]] / i["gamma"].double()
                fails(name, "dgamma", drop_last_term(ref["dgamma"], e_last * i["y"][int(ref["dy_next_src"][-1])].double()), ref["dgamma"])
            if rider.get("pos") is not None and samples:                     # one sample's pos shifted by one
                bad = rider["pos"].clone(); bad[int(torch.nonzero(bad >= 0)[-1])] += 1
                mut = f(F64, rider=dict(rider, pos=bad), dy_next_rows=kw["dy_next_rows"] + rider["tokens"])
                fails(name, "dy_next", R.materialize(mut["dy_next"]), ref["dy_next"])
            if "pad2" in ref and (ref["dy_next"].state == R.ZERO).any():     # the last pad row left non-zero
                for k in ("dy_next", "pad2"):
                    buf = R.materialize(ref[k])
                    buf[int(torch.nonzero(ref[k].state == R.ZERO)[-1])] = 1.0
                    fails(name, k, buf, ref[k])
        if samples and kw.get("pos") is not None and len(ref["passthrough_rows"]):
            buf = R.materialize(ref["dx"], got["dx"].ref)                    # a dropped sample whose dres did not pass through exactly
            r0 = int(ref["passthrough_rows"][0])
            buf[r0] = buf[r0] * (1 + 2.0 ** -20) + 2.0 ** -20
            fails(name, "dx", buf, ref["dx"])


@pytest.mark.parametrize("tokens,B,pad_base,K", [(7, 66, 0, 64), (7, 66, 0, 55), (7, 66, 0, 9), (7, 66, 21, 61), (7, 66, 21, 52),
                                                 (7, 66, 21, 6), (197, 14, 0, 13), (197, 14, 591, 10)])
def test_pad_fill_mutation_fails(tokens, B, pad_base, K):
    Cd, M = 128, B * tokens
    i = R.ln_inputs(M, Cd, "exact", seed=400)
    kr = torch.zeros(B, dtype=torch.bool)
    kr[torch.randperm(B, generator=torch.Generator().manual_seed(K))[:K]] = True
    cnt = K * tokens
    npad = (pad_base + cnt + 63) // 64 * 64 - pad_base
    assert (pad_base + cnt) % 64 in (0, 1, 63)
    ref = R.ln_bwd(i["dy"], i["x"], torch.zeros(M), torch.ones(M), i["w"], i["dres"], M, dy_next_rows=npad, exact=True,
                   rider=dict(tokens=tokens, rowscale=R.rowscale_of(kr, exact=True), pos=R.pos_of(kr), cnt=cnt, pad_base=pad_base,
                              pad2_cols=3 * Cd, y=i["y"], gamma=i["gamma"]))
    for k in ("dy_next", "pad2"):
        assert int((ref[k].state == R.ZERO).sum()) == npad - cnt and ref[k].ref.shape[0] == npad
        R.compare("pad", k, R.materialize(ref[k]), ref[k])
        buf = R.materialize(ref[k])
        if npad > cnt:
            buf[npad - 1, -1] = 1.0                                          # the last pad row left non-zero
        else:
            buf[npad] = 0                                                    # no pad rows: the row behind the kept ones must stay untouched
        fails("pad", k, buf, ref[k])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Cd,tokens,B", SHAPES)
def test_ls_bwd_float32_passes_and_mutations_fail(Cd, tokens, B, family):
    Rs, ex = B * tokens, family == "exact"
    i = R.ln_inputs(Rs, Cd, family, seed=500)
    scale = R.rowscale_of(R.kept_set("alternating", B), exact=ex)
    count = Rs - 2 * tokens - 3
    rowidx = torch.randperm(Rs, generator=torch.Generator().manual_seed(3))[:count]
    Mpad = (count + 63) // 64 * 64
    lists = torch.cat([rowidx, torch.zeros(Mpad - count, dtype=torch.long)])
    for M, ri, cn in ((Rs, None, None), (Mpad, lists, count)):
        f = lambda dt: R.ls_bwd(i["dres"], i["y"], i["gamma"], scale, tokens, M, ri, cn, exact=ex, dt=dt)      # noqa: E731
        ref, got = f(F64), f(F32)
        passes("ls_bwd", ref, got)
        n = len(ref["dy_idx"])
        last = int(ri[n - 1]) if ri is not None else n - 1
        if last // tokens % 2 == 1:                                         # the last row belongs to a dropped sample: its term is 0
            continue
        if ex or tokens == 7:
            e_last = i["dres"][last].double() * scale[last // tokens].double()
            fails("ls_bwd", "dgamma", drop_last_term(ref["dgamma"], e_last * i["y"][last].double()), ref["dgamma"])
        if cn is not None:
            buf = R.materialize(ref["dy"]); buf[M - 1, 0] = 1.0              # the last pad row left non-zero
            fails("ls_bwd", "dy", buf, ref["dy"])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("ncols", [8, 512, 520, 768])
def test_colsum_float32_passes_and_a_dropped_row_fails(ncols, family):
    ld, col0, ex = 3 * ncols, 2 * ncols, family == "exact"
    y = R.ints(1000, ld, seed=600) if ex else R.rnd(1000, ld, seed=600).to(BF16).to(F32)
    for M in (1, 255, 256, 257, 1000):
        ref = R.colsum(y, col0, ncols, M, exact=ex)
        passes("colsum", ref, R.colsum(y, col0, ncols, M, exact=ex, dt=F32))
        if ex or M <= 257:                                                  # (R = 1000, random: bound ~ 0.05, a term can be as small in every column)
            fails("colsum", "out", drop_last_term(ref["out"], y[M - 1, col0:col0 + ncols]), ref["out"])
        fails("colsum", "out", (y[:M, col0 - 8:col0 - 8 + ncols].double().sum(0)).float(), ref["out"])      # the wrong column block


def test_reduce_replicas_float32_passes_and_a_missing_replica_fails():
    rep, out0 = R.rnd(32, 768, seed=7), R.rnd(768, seed=9)
    ref = R.reduce_replicas(rep, out0)
    passes("reduce_replicas", ref, R.reduce_replicas(rep, out0, dt=F32))
    fails("reduce_replicas", "out", (out0.double() + rep[:-1].double().sum(0)).float(), ref["out"])      # a replica that is never summed


@pytest.mark.parametrize("B,Pn,Cd", [(3, 9, 128), (3, 196, 768), (130, 9, 768), (130, 196, 128)])
def test_token_bwd_float32_passes_and_mutations_fail(B, Pn, Cd):
    M = B * (Pn + 1)
    mask = (torch.rand(B, Pn, generator=torch.Generator().manual_seed(5)) < 0.4).long()
    mask[0] = 0; mask[-1, 1:] = 1
    c0, m0 = R.ints(Cd, seed=1101), R.ints(Cd, seed=1102)
    for family in FAMILIES:
        ex = family == "exact"
        dx = R.ints(M, Cd, seed=1100) if ex else R.rnd(M, Cd, seed=1100)
        ref = R.token_bwd(dx, mask, B, Pn, c0, m0, exact=ex)
        passes("token_bwd", ref, R.token_bwd(dx, mask, B, Pn, c0, m0, exact=ex, dt=F32))
        if ex or B == 3:
            fails("token_bwd", "dcls", drop_last_term(ref["dcls"], dx[(B - 1) * (Pn + 1)]), ref["dcls"])
            fails("token_bwd", "dmask_token", drop_last_term(ref["dmask_token"], dx[M - 1]), ref["dmask_token"])
        buf = R.materialize(ref["dpatch"])
        buf[B * Pn - 1] = dx[M - 1].to(BF16)                                # a masked row that is not zero
        fails("token_bwd", "dpatch", buf, ref["dpatch"])


def test_droppath_lists_builder():
    keep = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1], dtype=torch.bool)
    o = R.droppath_lists(keep, 7, 192)
    assert o["pos"].tolist() == [0, -1, 1, 2, -1, -1, 3, -1, 4, 5, 6] and o["bmap"].tolist() == [0, 2, 3, 6, 8, 9, 10, 0, 0, 0, 0]
    assert o["cnt"] == 49 and o["rows_written"] == 64 and o["rows"][:8].tolist() == [0, 1, 2, 3, 4, 5, 6, 14]
    assert o["rows"][48].item() == 76 and (o["rows"][49:] == -1).all()


@pytest.mark.parametrize("M", [64, 192, 1100])
def test_resid_rows_float32_passes_and_mutations_fail(M):
    N, K, tokens = 256, 128, 7
    Rs = (M // tokens + 20) * tokens
    a, wt = R.rnd(M, K, seed=900).to(BF16).to(F32), (R.rnd(N, K, seed=901) * K ** -0.5).to(BF16).to(F32)
    bias, gamma, resid = R.rnd(N, seed=902) * 0.1, R.rnd(N, seed=903) * 0.1 + 0.5, R.rnd(Rs, N, seed=904)
    scale = R.rowscale_of(R.kept_set("alternating", Rs // tokens))
    rowcount = M - 37
    rowmap = torch.randperm(Rs, generator=torch.Generator().manual_seed(4))[:M]
    rowmap[rowcount:] = -1
    f = lambda dt, rc=rowcount, sc=scale: R.resid_rows(a, wt, bias, gamma, resid, sc, tokens, rowmap, rc, M, dt=dt)      # noqa: E731
    ref = f(F64)
    passes("resid_rows", ref, f(F32))
    fails("resid_rows", "out", R.materialize(f(F64, rc=rowcount - 1)["out"]), ref["out"])            # the last listed row not written
    shifted = torch.roll(scale, 1)                                                                   # rowscale taken at the wrong sample
    fails("resid_rows", "out", R.materialize(ref["out"], f(F64, sc=shifted)["out"].ref), ref["out"])


@pytest.mark.parametrize("M,s1_row", [(1024, 512), (1088, 576)])
def test_wgrad_split_chunk_in_the_wrong_stream_fails(M, s1_row):
    Y, X = R.ints(M, 512, lo=-2, hi=2, seed=1001), R.ints(M, 256, lo=-2, hi=2, seed=1011)
    ref = R.wgrad_split(Y, X, s1_row, 256, 256)
    for k in ("bias", "bias2", "bias_s1", "bias2_s1", "C"):
        R.compare("wgrad_split", k, ref[k].ref.float(), ref[k])
    chunk = Y[s1_row:s1_row + 64, :256].double().sum(0)                     # the first 64-row chunk of the second stream
    fails("wgrad_split", "bias", (ref["bias"].ref[0] + chunk).float(), ref["bias"])
    fails("wgrad_split", "bias_s1", (ref["bias_s1"].ref[0] - chunk).float(), ref["bias_s1"])


def test_transpose_restatement():
    src = R.rnd(70, 100, seed=3).to(BF16)
    ref = R.transpose(src)["dst"]
    R.compare("transpose", "dst", R.materialize(ref), ref)
    buf = R.materialize(ref); buf[99, 69] = buf[98, 69]
    fails("transpose", "dst", buf, ref)


def test_struct_mirrors_follow_the_header():
    """uvit_ls_rider, uvit_wgrad_split and uvit_transpose_desc cross the C ABI by pointer: the ctypes mirrors carry the header's fields in
    the header's order."""
    import os
    import re
    from uncertainty_vit_amd import native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uvit.h")).read()
    for name, mirror in (("uvit_ls_rider", native.LsRider), ("uvit_wgrad_split", native.WgradSplit), ("uvit_transpose_desc", native.TransposeDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = re.findall(r"\*?\s*([a-z_0-9]+)\s*[,;]", body)
        assert fields == [n for n, _ in mirror._fields_], (name, fields)
    assert (C.sizeof(native.LsRider), C.sizeof(native.WgradSplit), C.sizeof(native.TransposeDesc)) == (96, 24, 32)


# ---- refused without a device --------------------------------------------------------------------------------------------------
def test_entry_points_refuse_without_a_device():
    from uncertainty_vit_amd import native
    native.build()
    host = (C.c_char * 4096)()
    calls = R.refused_calls(native.lib(), C.addressof(host))
    assert len(calls) > 50
    for what, rc, want in calls:
        assert rc == want, f"{what}: returned {rc}, expected {want}"
    assert bytes(host) == bytes(4096)
