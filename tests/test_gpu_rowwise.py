"""GPU: the step's row-wise kernels, through the operator entry points, in every walk the engine launches them in, against the
float64 restatements and derived bounds of tests/rowwise_ref.py.

Operands are seeded on the CPU.  Every output buffer is over-allocated and filled with the sentinel bit patterns of
tests/test_gpu_rowcounts.py before the launch; rowwise_ref.compare then demands a value in every row the walk must write, zero bits
in every row it must zero and the sentinel in every other row.  Column-sum accumulators are zero inside their span and sentinel
between the replicas.  Two input families per column-sum case: random, and exact (integers and powers of two: every product and
partial sum is exact in fp32, so dw, db, dgamma, dbias and the column sums must equal the reference in any summation order).

Field -> case (LnFwd, LnBwd, LsNext of csrc/uvit_internal.h and what the other entry points carry):
  LnFwd.x w b y M C eps          test_ln_fwd_rows_walk (dense)
  LnFwd.mean rstd                test_ln_fwd_rows_walk (dense: written; row list: rows >= count untouched; NULL)
  LnFwd.rowidx count             test_ln_fwd_rows_walk (row list)
  LnFwd.pos xcopy tokens         test_ln_fwd_samples_walk, test_lists_feed_layernorm_chain
  LnBwd.dy x mean rstd w dx dw db M C   test_ln_bwd_rows_walk (dense)
  LnBwd.dres                     test_ln_bwd_rows_walk (with / without), test_ln_bwd_samples_walk (pass-through of a dropped sample)
  LnBwd.rowidx count             test_ln_bwd_rows_walk (row list, row list + compact rider)
  LnBwd.pos                      test_ln_bwd_samples_walk
  LnBwd.nrep rep_stride          test_ln_bwd_samples_walk[nrep=32], test_ls_bwd, test_colsum, then uvit_op_reduce_replicas
  LsNext.y gamma rowscale dy dgamma dbias   test_ln_bwd_rows_walk (dense rider, with rowscale and with NULL = 1), test_ls_bwd
  LsNext.tokens                  test_ln_bwd_samples_walk (no rider: layer 0's form; riders)
  LsNext.pos                     test_ln_bwd_rows_walk (row list + compact rider), test_ln_bwd_samples_walk (own pos != rider pos)
  LsNext.cnt pad_base pad2 pad2_cols    test_ln_bwd_pad_fill, test_ln_bwd_samples_walk
  ls_bwd rowidx count            test_ls_bwd (row list to the reduction length)
  colsum ld col0 ncols M         test_colsum
  droppath_lists (all)           test_droppath_lists, test_lists_feed_layernorm_chain
  gemm_nt_rows rowmap rowcount   test_resid_over_a_row_list
  wgrad split bias_s1 bias2_s1 s1_row   test_wgrad_group_stream_split
  token_bwd (all)                test_token_bwd
  transpose_batch descs ndesc total_tiles   test_transpose_batch
  refused combinations           test_refused_with_device_pointers (the list of rowwise_ref.refused_calls, also run on the CPU)

Measured on an MI355X (256 CUs), worst |got - ref| / bound per operator and output (test_zz_report_worst_ratios prints them; the
file runs in 10-14 s).  bf16 outputs sit just below 1 by construction: 2^-8 |ref| IS the rounding of a bf16 store.  The column sums move in
the second digit from run to run with the order of the atomics.
  ln_fwd       y 0.995   mean 0.041   rstd 0.092
  ln_bwd       dx 0.117   dw 0.181   db 0.006   dy_next 0.996   dgamma 0.035   dbias 0.010
  ls_bwd       dy 0.996   dgamma 0.023   dbias 0.004
  chain        y 0.987   mean 0.014   rstd 0.075   dx 0.066   dw 0.018   db 0.000   dy_next 0.985   dgamma 0.011   dbias 0.002
  colsum 0.0007   reduce_replicas 0.100   resid_rows out 0.013, out2 0.986   token_bwd dpatch 0.996, dcls 0.156, dmask_token 0.079
  exact family, wgrad split, transposes, lists: equality.
"""
import ctypes as C

import pytest
import torch

import rowwise_ref as R
from rowwise_ref import BF16, F32

pytestmark = pytest.mark.gpu

EPS = 1e-6
# (C, tokens, B): M = 77 is one row per wave and workgroups without work; M = 4531 is three rows per wave on 256 CUs (rows_per_block 24),
# the next-row prefetch and a ragged last workgroup
SHAPES = [(c, 7, 11) for c in (128, 260, 768, 1024, 1280, 1536, 2048)] + [(128, 197, 23), (768, 197, 23)]
FAMILIES = ("random", "exact")


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


def dev(t, dtype=None):
    return None if t is None else t.to(dtype or t.dtype).contiguous().cuda()


def i32(t):
    return None if t is None else (torch.tensor([t]) if isinstance(t, int) else t).to(torch.int32).cuda()


def sent(rows, cols, dtype):
    return R.sentinel(rows, cols, dtype, "cuda")


class Acc:
    """A replicated column-sum accumulator: nrep spans of n zeros, rep_stride apart, sentinel words between them."""

    def __init__(self, n, nrep):
        self.n, self.nrep, self.stride = n, nrep, n + (12 if nrep > 1 else 4)
        self.t = sent(nrep, self.stride, F32)
        self.t[:, :n] = 0

    def total(self):
        assert (R.bits(self.t[:, self.n:]) == R.SENT32).all(), "a word between the replica spans was written"
        return self.t[:, :self.n].double().sum(0).cpu()


def check(op, outs, **got):
    for name, t in got.items():
        R.compare(op, name, t.total() if isinstance(t, Acc) else t.cpu(), outs[name])


def rider_struct(y=None, gamma=None, rowscale=None, dy=None, dgamma=None, dbias=None, tokens=0, pos=None, cnt=None, pad_base=0, pad2=None,
                 pad2_cols=0):
    from uncertainty_vit_amd.native import LsRider
    r = LsRider()
    for k, v in dict(y=y, gamma=gamma, rowscale=rowscale, dy=dy, dgamma=dgamma, dbias=dbias, pos=pos, cnt=cnt, pad2=pad2).items():
        setattr(r, k, 0 if v is None else (v.t if isinstance(v, Acc) else v).data_ptr())
    r.tokens, r.pad_base, r.pad2_cols = tokens, pad_base, pad2_cols
    return r


def stats_of(x, family):
    """The saved statistics a LayerNorm forward would hand to the backward, as fp32 inputs (exact family: mean 0, rstd 1)."""
    if family == "exact":
        return torch.zeros(x.shape[0]), torch.ones(x.shape[0])
    xd = x.double()
    return xd.mean(-1).float(), ((xd.var(-1, unbiased=False) + EPS) ** -0.5).float()


# ---- LayerNorm forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cd,tokens,B", SHAPES)
def test_ln_fwd_rows_walk(L, Cd, tokens, B):
    M, Rs = B * tokens, B * tokens + 40
    inp = R.ln_inputs(Rs, Cd, "random", seed=100)
    x, w, b = dev(inp["x"]), dev(inp["w"]), dev(inp["b"])

    def run(rowidx, count, stats):
        y, mean, rstd = sent(M + 2, Cd, BF16), sent(M + 2, 1, F32), sent(M + 2, 1, F32)
        ri, cn = i32(rowidx), i32(count)
        ok(L.uvit_op_ln_fwd_walk(P(x), P(w), P(b), P(y), P(mean) if stats else None, P(rstd) if stats else None, M, Cd, C.c_float(EPS),
                                 P(ri), P(cn), None, None, 0, S()))
        ref = R.ln_fwd(inp["x"], inp["w"], inp["b"], EPS, M, rowidx, count, stats=stats)
        check("ln_fwd", ref, y=y, **(dict(mean=mean, rstd=rstd) if stats else {}))
        if not stats:
            assert (R.bits(mean) == R.SENT32).all() and (R.bits(rstd) == R.SENT32).all()

    run(None, None, True)                                                   # dense
    rowidx = torch.randperm(Rs, generator=torch.Generator().manual_seed(1))[:M]
    run(rowidx, M - 5, True)                                                # row list, count < M: rows >= count zero, their statistics untouched
    run(rowidx, M - 5, False)                                               # mean / rstd NULL


@pytest.mark.parametrize("Cd,tokens,B", SHAPES)
def test_ln_fwd_samples_walk(L, Cd, tokens, B):
    M = B * tokens
    inp = R.ln_inputs(M, Cd, "random", seed=110)
    x, w, b = dev(inp["x"]), dev(inp["w"]), dev(inp["b"])
    for kept in R.KEPT_SETS:
        pos = R.pos_of(R.kept_set(kept, B))
        ref = R.ln_fwd(inp["x"], inp["w"], inp["b"], EPS, M, pos=pos, tokens=tokens)
        rows = ref["y"].ref.shape[0]
        y, mean, rstd, xcopy = sent(rows + 2, Cd, BF16), sent(rows + 2, 1, F32), sent(rows + 2, 1, F32), sent(M + 2, Cd, F32)
        pd = i32(pos)
        ok(L.uvit_op_ln_fwd_walk(P(x), P(w), P(b), P(y), P(mean), P(rstd), M, Cd, C.c_float(EPS), None, None, P(pd), P(xcopy), tokens, S()))
        check("ln_fwd", ref, y=y, mean=mean, rstd=rstd, xcopy=xcopy)


# ---- LayerNorm backward --------------------------------------------------------------------------------------------------------
class LnBwdCase:
    """Operands of one LayerNorm backward over a residual stream of Rs rows, dense by stream row; the launches gather what they need."""

    def __init__(self, Rs, Cd, family, seed):
        self.Rs, self.C, self.family, self.exact = Rs, Cd, family, family == "exact"
        self.inp = R.ln_inputs(Rs, Cd, family, seed)
        self.mean, self.rstd = stats_of(self.inp["x"], family)
        i = self.inp
        self.d = {k: dev(i[k]) for k in ("x", "w", "dres", "gamma")}
        self.d["y"] = dev(i["y"], BF16)

    def run(self, L, M, a_rows, nrep=1, rowidx=None, count=None, pos=None, dres=True, rider=None, dy_next_rows=0, pad2_rows=0):
        """a_rows: the stream row of each row of dy / mean / rstd.  rider: None, or the reference's rider dict."""
        i, Cd = self.inp, self.C
        dy, mean, rstd = i["dy"][a_rows], self.mean[a_rows], self.rstd[a_rows]
        dx, dw, db = sent(self.Rs + 2, Cd, F32), Acc(Cd, nrep), Acc(Cd, nrep)
        got = dict(dx=dx, dw=dw, db=db)
        rs = None
        rd = dict(rider or {})
        if rider is not None:
            kw = dict(tokens=rider["tokens"])
            if rider.get("y") is not None:
                dyn, dg, dbi = sent(dy_next_rows + 2, Cd, BF16), Acc(Cd, nrep), Acc(Cd, nrep)
                got.update(dy_next=dyn, dgamma=dg)
                kw.update(y=self.d["y"], gamma=self.d["gamma"], rowscale=dev(rider.get("rowscale")), dy=dyn, dgamma=dg, dbias=dbi,
                          pos=i32(rider.get("pos")), cnt=i32(rider.get("cnt")), pad_base=rider.get("pad_base", 0))
                if rider.get("pad2_cols"):
                    got["pad2"] = sent(pad2_rows + 2, rider["pad2_cols"], BF16)
                    kw.update(pad2=got["pad2"], pad2_cols=rider["pad2_cols"])
                rd.update(y=i["y"], gamma=i["gamma"])
            rs = rider_struct(**kw)
        ops = [dev(dy, BF16), dev(mean), dev(rstd), i32(rowidx), i32(count), i32(pos)]
        ok(L.uvit_op_ln_bwd_walk(P(ops[0]), P(self.d["x"]), P(ops[1]), P(ops[2]), P(self.d["w"]), P(self.d["dres"]) if dres else None,
                                 P(dx), P(dw.t), P(db.t), M, Cd, nrep, dw.stride, P(ops[3]), P(ops[4]), P(ops[5]),
                                 None if rs is None else C.byref(rs), S()))
        ref = R.ln_bwd(dy, i["x"], mean, rstd, i["w"], i["dres"] if dres else None, M, rowidx, count, pos, rd if rider is not None else None,
                       dy_next_rows, exact=self.exact)
        check("ln_bwd", ref, **got)
        pt = ref["passthrough_rows"]
        assert torch.equal(R.bits(dx.cpu()[pt]), R.bits(i["dres"][pt])), "a dropped sample's dx is not dres bit for bit"
        if "dy_next" in got:
            R.compare("ln_bwd", "dbias", dbi.total(), R.stored_colsum(got["dy_next"].cpu(), ref["dy_next_idx"], self.exact))
        return got


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Cd,tokens,B", SHAPES)
def test_ln_bwd_rows_walk(L, Cd, tokens, B, family):
    M, Rs = B * tokens, (B + 5) * tokens
    case = LnBwdCase(Rs, Cd, family, seed=200)
    dense = torch.arange(M)
    case.run(L, M, dense)                                                    # dense, with dres
    case.run(L, M, dense, dres=False)
    rowidx = torch.randperm(Rs, generator=torch.Generator().manual_seed(2))[:M]
    case.run(L, M, rowidx, rowidx=rowidx, count=M - 9)                       # row list: dx rows >= count keep the sentinel
    case.run(L, M, rowidx, rowidx=rowidx, count=M - 9, dres=False)
    keep = R.kept_set("alternating", B + 5)
    scale = R.rowscale_of(keep, exact=case.exact)
    case.run(L, M, dense, rider=dict(tokens=tokens, rowscale=scale, y=True), dy_next_rows=Rs)           # dense rider
    case.run(L, M, dense, rider=dict(tokens=tokens, y=True), dy_next_rows=Rs)                           # rowscale NULL: every multiplier 1
    # the masked-row last block: a row list whose rider is compact by the MLP branch's sample list
    pos = R.pos_of(keep)
    case.run(L, M, rowidx, rowidx=rowidx, count=M - 9, rider=dict(tokens=tokens, rowscale=scale, pos=pos, y=True),
             dy_next_rows=int(keep.sum()) * tokens)


@pytest.mark.parametrize("nrep", [1, 32])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Cd,tokens,B", SHAPES)
def test_ln_bwd_samples_walk(L, Cd, tokens, B, family, nrep):
    M = B * tokens
    case = LnBwdCase(M, Cd, family, seed=300)
    rows_of = lambda pos: torch.nonzero((pos >= 0).repeat_interleave(tokens)).flatten()      # noqa: E731
    for kept in R.KEPT_SETS if nrep == 1 else ("alternating",):                   # no rider: layer 0's form, next.tokens alone
        pos = R.pos_of(R.kept_set(kept, B))
        case.run(L, M, rows_of(pos), nrep=nrep, pos=pos, rider=dict(tokens=tokens))
    # own list and rider list differ: a sample dropped by the LayerNorm's branch passes dres through and adds nothing to dw / db,
    # one dropped by the rider writes no dy row and adds nothing to dgamma / dbias
    for own, rid, pad_base in (("alternating", "first_dropped", 0), ("all", "last_dropped", 3 * tokens), ("one", "alternating", 0),
                               ("first_dropped", "all", 0)):
        ko, kr = R.kept_set(own, B), R.kept_set(rid, B)
        pos, rpos = (None if own == "all" else R.pos_of(ko)), R.pos_of(kr)
        cnt = int(kr.sum()) * tokens
        npad = (pad_base + cnt + 63) // 64 * 64 - pad_base
        got = case.run(L, M, rows_of(R.pos_of(ko)), nrep=nrep, pos=pos,
                       rider=dict(tokens=tokens, rowscale=R.rowscale_of(kr, exact=case.exact), pos=rpos, cnt=cnt, pad_base=pad_base,
                                  pad2_cols=3 * Cd, y=True), dy_next_rows=npad, pad2_rows=npad)
    # the replicas are then added onto a gradient that already holds something
    dw = got["dw"]
    out0 = R.rnd(Cd, seed=9)
    out = sent(1, Cd + 4, F32); out[0, :Cd] = dev(out0)
    ok(L.uvit_op_reduce_replicas(P(dw.t), P(out), Cd, nrep, dw.stride, S()))
    R.compare("reduce_replicas", "out", out[0, :Cd].cpu(), R.reduce_replicas(dw.t[:, :Cd].cpu(), out0)["out"])
    assert (R.bits(out[0, Cd:]) == R.SENT32).all() and dw.total() is not None


# (pad_base + cnt) % 64 in {0, 1, 63} at pad_base 0 and 3 tokens: kept samples K of the rider with cnt = K tokens
PAD_CASES = [(7, 66, 0, 64), (7, 66, 0, 55), (7, 66, 0, 9), (7, 66, 21, 61), (7, 66, 21, 52), (7, 66, 21, 6),
             (197, 14, 0, 13), (197, 14, 591, 10)]


@pytest.mark.parametrize("tokens,B,pad_base,K", PAD_CASES)
def test_ln_bwd_pad_fill(L, tokens, B, pad_base, K):
    """Rows cnt .. roundup(pad_base + cnt, 64) - pad_base of the rider's dy and of pad2 (3 C columns) are zero, the row behind them is
    untouched (and row cnt itself when pad_base + cnt is a multiple of 64)."""
    Cd, M = 128, B * tokens
    assert (pad_base + K * tokens) % 64 in (0, 1, 63)
    case = LnBwdCase(M, Cd, "exact", seed=400)
    kr = torch.zeros(B, dtype=torch.bool)
    kr[torch.randperm(B, generator=torch.Generator().manual_seed(K))[:K]] = True
    cnt = K * tokens
    npad = (pad_base + cnt + 63) // 64 * 64 - pad_base
    case.run(L, M, torch.arange(M), rider=dict(tokens=tokens, rowscale=R.rowscale_of(kr, exact=True), pos=R.pos_of(kr), cnt=cnt,
                                               pad_base=pad_base, pad2_cols=3 * Cd, y=True), dy_next_rows=npad, pad2_rows=npad)


# ---- LayerScale + DropPath backward on its own ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nrep", [1, 32])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Cd,tokens,B", SHAPES)
def test_ls_bwd(L, Cd, tokens, B, family, nrep):
    Rs = B * tokens
    exact = family == "exact"
    inp = R.ln_inputs(Rs, Cd, family, seed=500)
    d_in = inp["dres"]                                                     # the residual-stream gradient
    scale = R.rowscale_of(R.kept_set("alternating", B), exact=exact)
    dx, y, gamma, sc = dev(d_in), dev(inp["y"], BF16), dev(inp["gamma"]), dev(scale)
    count = Rs - 2 * tokens - 3
    rowidx = torch.randperm(Rs, generator=torch.Generator().manual_seed(3))[:count]
    Mpad = (count + 63) // 64 * 64                                         # the wgrad's reduction length: rows count .. Mpad are zeroed
    lists = torch.cat([rowidx, torch.zeros(Mpad - count, dtype=torch.long)])
    for M, ri, cn in ((Rs, None, None), (Mpad, lists, count)):
        dy, dg, dbi = sent(M + 2, Cd, BF16), Acc(Cd, nrep), Acc(Cd, nrep)
        rs = rider_struct(y=y, gamma=gamma, rowscale=sc, dy=dy, dgamma=dg, dbias=dbi, tokens=tokens)
        rid, cnd = i32(ri), i32(cn)
        ok(L.uvit_op_ls_bwd(P(dx), C.byref(rs), M, Cd, nrep, dg.stride, P(rid), P(cnd), S()))
        ref = R.ls_bwd(d_in, inp["y"], inp["gamma"], scale, tokens, M, ri, cn, exact=exact)
        check("ls_bwd", ref, dy=dy, dgamma=dg)
        R.compare("ls_bwd", "dbias", dbi.total(), R.stored_colsum(dy.cpu(), ref["dy_idx"], exact))


# ---- column sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("ncols", [8, 512, 520, 768])
def test_colsum(L, ncols, family):
    """The qkv form (ld = 3 ncols, col0 = 2 ncols) at row counts around the 16-row unroll, its remainder loop and the 256-row
    workgroup seam, into 1 and 32 replicas."""
    ld, col0, Mmax = 3 * ncols, 2 * ncols, 1000
    y = R.ints(Mmax, ld, seed=600) if family == "exact" else R.rnd(Mmax, ld, seed=600).to(BF16).to(F32)
    yd = dev(y, BF16)
    for M in (1, 255, 256, 257, 1000):
        for nrep in (1, 32):
            acc = Acc(ncols, nrep)
            ok(L.uvit_op_colsum(P(yd), ld, col0, ncols, M, P(acc.t), nrep, acc.stride, S()))
            check("colsum", R.colsum(y, col0, ncols, M, exact=family == "exact"), out=acc)


# ---- drop-path sample lists ----------------------------------------------------------------------------------------------------
def lists_case(nlists, B, seed):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(nlists, B, generator=g) < 0.7
    keep[0] = True                                                         # all kept
    if nlists > 1:
        keep[1] = R.kept_set("one", B)
        keep[2] = R.kept_set("alternating", B)
    return keep


def run_lists(L, keep, tokens, host_counts=None):
    nlists, B = keep.shape
    stride = (B * tokens + 63) // 64 * 64 + 64
    scales = dev(torch.stack([R.rowscale_of(k) for k in keep]))
    mk = lambda n: torch.full((n,), R.SENT32, dtype=torch.int32, device="cuda")        # noqa: E731
    pos, bmap, rows, cnt = mk(nlists * B), mk(nlists * B), mk(nlists * stride), mk(2 * nlists + 2)
    hc = (C.c_int32 * nlists)(*(host_counts if host_counts is not None else [int(k.sum()) for k in keep]))
    ok(L.uvit_op_droppath_lists(P(scales), P(pos), P(bmap), P(rows), P(cnt), nlists, B, tokens, stride, hc, S()))
    return pos.view(nlists, B), bmap.view(nlists, B), rows.view(nlists, stride), cnt


@pytest.mark.parametrize("tokens", [7, 197])
@pytest.mark.parametrize("B", [11, 256, 300])
@pytest.mark.parametrize("nlists", [1, 6])
def test_droppath_lists(L, nlists, B, tokens):
    keep = lists_case(nlists, B, seed=700 + B)
    counts = [int(k.sum()) for k in keep]
    wrong = list(counts); wrong[nlists - 1] += 1
    for hc in (counts, wrong):
        pos, bmap, rows, cnt = (t.cpu() for t in run_lists(L, keep, tokens, hc))
        for l in range(nlists):
            ref = R.droppath_lists(keep[l], tokens, rows.shape[1])
            assert torch.equal(pos[l].long(), ref["pos"]) and torch.equal(bmap[l].long(), ref["bmap"]), l
            n = ref["rows_written"]
            assert torch.equal(rows[l, :n].long(), ref["rows"][:n]), l
            assert (rows[l, n:] == R.SENT32).all(), "written behind the pad rows"
            assert cnt[l].item() == ref["cnt"]
            assert cnt[nlists + l].item() == int(hc[l] != counts[l]), "mismatch flag"
        assert (cnt[2 * nlists:] == R.SENT32).all()


def test_lists_feed_layernorm_chain(L):
    """lists -> LayerNorm forward samples walk -> LayerNorm backward samples walk, the index arrays staying on the device: the
    attention branch's list drives the LayerNorm, the MLP branch's list its rider."""
    Cd, tokens, B = 128, 7, 11
    M = B * tokens
    keep = torch.stack([R.kept_set("alternating", B), R.kept_set("first_dropped", B)])
    pos, bmap, rows, cnt = run_lists(L, keep, tokens)
    case = LnBwdCase(M, Cd, "random", seed=800)
    i = case.inp
    fref = R.ln_fwd(i["x"], i["w"], i["b"], EPS, M, pos=R.pos_of(keep[0]), tokens=tokens)
    ka = fref["y"].ref.shape[0]
    y, mean, rstd, xcopy = sent(ka + 2, Cd, BF16), sent(ka + 2, 1, F32), sent(ka + 2, 1, F32), sent(M + 2, Cd, F32)
    ok(L.uvit_op_ln_fwd_walk(P(case.d["x"]), P(case.d["w"]), P(dev(i["b"])), P(y), P(mean), P(rstd), M, Cd, C.c_float(EPS), None, None,
                             P(pos[0]), P(xcopy), tokens, S()))
    check("chain", fref, y=y, mean=mean, rstd=rstd, xcopy=xcopy)
    # backward with the statistics the forward left on the device, and the rider's count from the lists
    a_rows = torch.nonzero(keep[0].repeat_interleave(tokens)).flatten()
    dy = i["dy"][a_rows]
    kb = int(keep[1].sum()) * tokens
    npad = (kb + 63) // 64 * 64
    dx, dw, db, dyn, dg, dbi = sent(M + 2, Cd, F32), Acc(Cd, 1), Acc(Cd, 1), sent(npad + 2, Cd, BF16), Acc(Cd, 1), Acc(Cd, 1)
    scale = R.rowscale_of(keep[1])
    sc, dyd = dev(scale), dev(dy, BF16)
    rs = rider_struct(y=case.d["y"], gamma=case.d["gamma"], rowscale=sc, dy=dyn, dgamma=dg, dbias=dbi, tokens=tokens, pos=pos[1],
                      cnt=cnt[1:2])
    ok(L.uvit_op_ln_bwd_walk(P(dyd), P(case.d["x"]), P(mean), P(rstd), P(case.d["w"]), P(case.d["dres"]), P(dx), P(dw.t), P(db.t), M, Cd, 1,
                             dw.stride, None, None, P(pos[0]), C.byref(rs), S()))
    m_, r_ = mean[:ka, 0].cpu(), rstd[:ka, 0].cpu()
    ref = R.ln_bwd(dy, i["x"], m_, r_, i["w"], i["dres"], M, pos=R.pos_of(keep[0]),
                   rider=dict(tokens=tokens, rowscale=scale, pos=R.pos_of(keep[1]), cnt=kb, y=i["y"], gamma=i["gamma"]), dy_next_rows=npad)
    check("chain", ref, dx=dx, dw=dw, db=db, dy_next=dyn, dgamma=dg)
    R.compare("chain", "dbias", dbi.total(), R.stored_colsum(dyn.cpu(), ref["dy_next_idx"]))


# ---- RESID epilogue over a row list --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 3])
@pytest.mark.parametrize("M", [64, 192, 1100])
def test_resid_over_a_row_list(L, M, variant):
    from uncertainty_vit_amd.native import GemmEpilogue, GemmNtPlanInfo, Tuning
    N, K, tokens = 256, 128, 7
    Rs = (M // tokens + 20) * tokens                                        # the residual stream is larger than the list
    a, wt = R.rnd(M, K, seed=900).to(BF16).to(F32), (R.rnd(N, K, seed=901) * K ** -0.5).to(BF16).to(F32)
    bias, gamma, resid = R.rnd(N, seed=902) * 0.1, R.rnd(N, seed=903) * 0.1 + 0.5, R.rnd(Rs, N, seed=904)
    scale = R.rowscale_of(R.kept_set("alternating", Rs // tokens))
    rowcount = M - 37
    rowmap = torch.randperm(Rs, generator=torch.Generator().manual_seed(4))[:M]
    rowmap[rowcount:] = -1                                                  # the pad of the list
    out, out2 = sent(Rs + 2, N, F32), sent(Rs + 2, N, BF16)
    ops = [dev(a, BF16), dev(wt, BF16), dev(bias), dev(gamma), dev(resid), dev(scale), i32(rowmap), i32(rowcount)]
    ep = GemmEpilogue()
    ep.out, ep.out2, ep.bias, ep.gamma, ep.resid, ep.rowscale = (t.data_ptr() for t in (out, out2, ops[2], ops[3], ops[4], ops[5]))
    ep.ldo, ep.tokens = N, tokens
    tu, info = Tuning.default(nt_variant=variant), GemmNtPlanInfo()
    ok(L.uvit_op_gemm_nt_plan(3, M, N, K, K, K, N, 1, C.byref(tu), torch.cuda.get_device_properties(0).multi_processor_count, C.byref(info)))
    assert info.tail_rows == 0 and info.rows == M, "a row-list launch must not split its rows"
    ok(L.uvit_op_gemm_nt_rows(3, P(ops[0]), P(ops[1]), M, N, K, K, K, C.byref(ep), P(ops[6]), P(ops[7]), C.byref(tu), S()))
    check("resid_rows", R.resid_rows(a, wt, bias, gamma, resid, scale, tokens, rowmap, rowcount, M), out=out, out2=out2)
    assert L.uvit_op_gemm_nt_rows(0, P(ops[0]), P(ops[1]), M, N, K, K, K, C.byref(ep), P(ops[6]), P(ops[7]), C.byref(tu), S()) == -1


# ---- grouped wgrad with a stream split -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [0, 1, 4])
@pytest.mark.parametrize("M,s1_row", [(1024, 512), (1088, 576)])
def test_wgrad_group_stream_split(L, M, s1_row, chunks):
    """Two stacked two-stream problems in one launch (N = K = 256 with one bias; N = 512 with bias and bias2, the qkv form): the column
    sums of rows [0, s1_row) go to bias / bias2, the rest to bias_s1 / bias2_s1.  Exact family: dW and every bias sum bit for bit."""
    from uncertainty_vit_amd.native import Tuning, WgradProblem, WgradSplit
    specs = [(256, 256, 256, 256), (512, 256, 256, 256)]                    # N, K, bias_end, bias2_begin
    probs, split, held, refs = (WgradProblem * 2)(), (WgradSplit * 2)(), [], []
    for j, (N, K, be, b2) in enumerate(specs):
        Y, X = R.ints(M, N, lo=-2, hi=2, seed=1000 + j), R.ints(M, K, lo=-2, hi=2, seed=1010 + j)
        Yd, Xd, Cw = dev(Y, BF16), dev(X, BF16), torch.zeros(N, K, device="cuda")
        accs = {n: Acc(be, 1) for n in ("bias", "bias_s1")}
        if N > be:
            accs.update({n: Acc(N - b2, 1) for n in ("bias2", "bias2_s1")})
        q = probs[j]
        q.Y, q.X, q.C, q.bias = Yd.data_ptr(), Xd.data_ptr(), Cw.data_ptr(), accs["bias"].t.data_ptr()
        q.bias2 = accs["bias2"].t.data_ptr() if "bias2" in accs else None
        q.bias_end, q.bias2_begin, q.M, q.N, q.K, q.ldy, q.ldx, q.ldc = be, b2, M, N, K, N, K, K
        split[j].bias_s1 = accs["bias_s1"].t.data_ptr()
        split[j].bias2_s1 = accs["bias2_s1"].t.data_ptr() if "bias2_s1" in accs else None
        split[j].s1_row = s1_row
        held.append((Yd, Xd, Cw, accs))
        refs.append(R.wgrad_split(Y, X, s1_row, be, b2))
    tu = Tuning.default(wgrad_group_chunks=chunks)
    ok(L.uvit_op_wgrad_group_split(probs, split, 2, C.byref(tu), S()))
    for (Yd, Xd, Cw, accs), ref in zip(held, refs):
        R.compare("wgrad_split", "C", Cw.cpu(), ref["C"])
        for n, acc in accs.items():
            R.compare("wgrad_split", n, acc.total(), ref[n])
    split[0].s1_row = s1_row - 64                                           # not half of the K-tiles: refused, nothing launched
    assert L.uvit_op_wgrad_group_split(probs, split, 2, C.byref(tu), S()) == -2
    split[0].s1_row = s1_row + 8                                            # not a multiple of 64
    assert L.uvit_op_wgrad_group_split(probs, split, 2, C.byref(tu), S()) == -2


# ---- token-assembly backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cd", [128, 768])
@pytest.mark.parametrize("Pn", [9, 196])
@pytest.mark.parametrize("B", [3, 130])
def test_token_bwd(L, B, Pn, Cd):
    M = B * (Pn + 1)
    masks = {"none": torch.zeros(B, Pn, dtype=torch.int64), "all": torch.ones(B, Pn, dtype=torch.int64),
             "ragged": (torch.rand(B, Pn, generator=torch.Generator().manual_seed(5)) < 0.4).long()}
    masks["ragged"][0] = 0; masks["ragged"][-1, 1:] = 1
    for family in FAMILIES:
        dx = R.ints(M, Cd, seed=1100) if family == "exact" else R.rnd(M, Cd, seed=1100)
        dxd = dev(dx)
        for name, mask in masks.items():
            c0, m0 = R.ints(Cd, seed=1101), R.ints(Cd, seed=1102)           # the accumulators already hold something
            dpatch, dcls, dmt = sent(B * Pn + 2, Cd, BF16), sent(1, Cd + 4, F32), sent(1, Cd + 4, F32)
            dcls[0, :Cd], dmt[0, :Cd] = dev(c0), dev(m0)
            md = dev(mask)
            ok(L.uvit_op_token_bwd(P(dxd), P(md), P(dpatch), P(dcls), P(dmt), B, Pn, Cd, S()))
            ref = R.token_bwd(dx, mask, B, Pn, c0, m0, exact=family == "exact")
            assert (R.bits(dcls[0, Cd:]) == R.SENT32).all() and (R.bits(dmt[0, Cd:]) == R.SENT32).all()
            R.compare("token_bwd", f"dpatch[{name}]", dpatch.cpu(), ref["dpatch"])
            R.compare("token_bwd", f"dcls[{name}]", dcls[0, :Cd].cpu(), ref["dcls"])
            R.compare("token_bwd", f"dmask_token[{name}]", dmt[0, :Cd].cpu(), ref["dmask_token"])


# ---- batched transposes --------------------------------------------------------------------------------------------------------
def test_transpose_batch(L):
    from uncertainty_vit_amd.native import TransposeDesc
    shapes = [(256, 128), (64, 192), (70, 100)]                             # the last one is ragged: the element-wise path
    descs, held, tile0 = (TransposeDesc * len(shapes))(), [], 0
    for j, (r, c) in enumerate(shapes):
        src = R.rnd(r, c, seed=1200 + j).to(BF16)
        sd, dst = dev(src), sent(c + 2, r, BF16)
        descs[j].src, descs[j].dst, descs[j].rows, descs[j].cols, descs[j].tile0 = sd.data_ptr(), dst.data_ptr(), r, c, tile0
        tile0 += ((r + 63) // 64) * ((c + 63) // 64)
        held.append((src, sd, dst))
    dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    ok(L.uvit_op_transpose_batch(P(dd), len(shapes), tile0, S()))
    for src, _, dst in held:
        R.compare("transpose", "dst", dst.cpu(), R.transpose(src)["dst"])


# ---- refused ---------------------------------------------------------------------------------------------------------------------
def test_refused_with_device_pointers(L):
    buf = torch.zeros(1 << 16, device="cuda")
    for what, rc, want in R.refused_calls(L, buf.data_ptr()):
        assert rc == want, f"{what}: returned {rc}, expected {want}"
    torch.cuda.synchronize()
    assert not buf.any(), "a refused call wrote to the device"


def test_zz_report_worst_ratios():
    print("\nworst |got - ref| / bound per operator:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
