"""float64 restatements (torch, CPU) of the step's row-wise operators in every walk the engine launches, and the comparator
that holds their error bounds.  Written from the reference's arithmetic (nn.LayerNorm, modeling_finetune.py:290-299; LayerScale +
DropPath, :295-298; token assembly, modeling_cyclical.py:179-192), not from the kernels.

Every restatement returns a dict name -> Out.  An Out is the float64 value of one output buffer, an absolute error bound per
element, and per row what the operator must do with it: WRITTEN (a value: no sentinel may remain), ZERO (zero bit for bit) or KEEP
(untouched: still the sentinel the buffer was filled with, as is every row behind the Out's rows).  `compare` checks all of it
and returns the worst |got - ref| / bound.  tests/test_host_rowwise_ref.py pins this file on the CPU (autograd, a float32
restatement in another order that must pass, mutations that must fail); tests/test_gpu_rowwise.py applies it to the kernels.

Bounds, with u = 2^-24 (derived, not tuned):
  bf16 outputs      |got - ref| <= 2^-8 |ref| + g_row S      S = sum of |terms| the element is formed from (reference intermediates)
  fp32 row outputs  |got - ref| <= g_row S                    g_row = (4 ceil(C / 256) + 16) u: a lane's serial adds, the wave shuffle
                                                              tree, slack for the products
  fp32 column sums  |got - ref| <= (R + 8) u sum_r |t_r|      any summation order of R terms (atomics, replicas), 8 u for the terms' own
                                                              rounding; plus what the terms inherit when they are computed values (the
                                                              rider on a LayerNorm backward sums e = dx * dp of a dx that carries g_row S_dx)
  GEMM epilogue     g_gemm = (K + 16) u in place of g_row: an fp32 dot of K products in any order
  exact cases       value equality (bit equality up to the sign of zero)
dbias is the sum of the STORED bf16 dy (the kernel re-reads what it rounded): a reference that rounds its own e * gamma can land one
bf16 ulp (2^-8) away in an element, which no summation bound covers, so `stored_colsum` sums the dy buffer under test -- whose
elements are checked against the reference separately.
"""
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
BF_ULP = 2.0 ** -8
SENT16, SENT32 = 0x7B7B, 0x7B7B7B7B              # the sentinels of tests/test_gpu_rowcounts.py
WRITTEN, ZERO, KEEP = 1, 0, -1
WORST = {}                                       # "operator output" -> worst |got - ref| / bound seen by compare()


def gamma_row(C):
    return (4 * math.ceil(C / 256) + 16) * U


def gamma_gemm(K):
    return (K + 16) * U


class Out:
    def __init__(self, ref, bound, dtype, state=None, exact=False):
        self.ref = ref if ref.dim() == 2 else ref.reshape(-1, 1) if state is not None else ref.reshape(1, -1)
        self.bound = None if bound is None else bound.reshape(self.ref.shape).to(F64)
        self.dtype, self.exact = dtype, exact
        self.state = torch.full((self.ref.shape[0],), WRITTEN, dtype=torch.int8) if state is None else state.to(torch.int8)


def bf16_out(ref, S, C, state=None, g=None):
    return Out(ref, BF_ULP * ref.abs().to(F64) + (gamma_row(C) if g is None else g) * S.to(F64), BF16, state)


def f32_out(ref, S, C, state=None, g=None):
    return Out(ref, (gamma_row(C) if g is None else g) * S.to(F64), F32, state)


def colsum_out(terms, extra=None, exact=False):
    """The sum over the rows of terms [R, C]."""
    R = terms.shape[0]
    bound = (R + 8) * U * terms.abs().to(F64).sum(0)
    if extra is not None:
        bound = bound + extra.to(F64)
    return Out(terms.sum(0), bound, F32, exact=exact)


def exact_out(ref, dtype, state=None):
    return Out(ref, None, dtype, state, exact=True)


def stored_colsum(stored, rows, exact=False):
    """dbias: the column sums of the rows `rows` of a stored bf16 buffer."""
    return colsum_out(stored[rows].to(F64), exact=exact)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def sentinel(rows, cols, dtype, device="cpu"):
    t = torch.empty(rows, cols, dtype=dtype, device=device)
    bits(t).fill_(SENT16 if dtype == BF16 else SENT32)
    return t


def materialize(out, values=None, slack=2):
    """The buffer an operator that computed `values` (default: the Out's own) would leave behind, `slack` untouched rows after it."""
    v = out.ref if values is None else values.reshape(out.ref.shape)
    t = sentinel(out.ref.shape[0] + slack, out.ref.shape[1], out.dtype)
    w, z = out.state == WRITTEN, out.state == ZERO
    t[:out.ref.shape[0]][w] = v[w].to(out.dtype)
    t[:out.ref.shape[0]][z] = 0
    return t


def compare(op, name, got, out):
    """got: CPU tensor of out.dtype, [rows >= out's rows, cols] (1-D: one column per row for a per-row Out, else one row)."""
    n, cols = out.ref.shape
    got = got.reshape(-1, cols)
    w, z, k = out.state == WRITTEN, out.state == ZERO, out.state == KEEP
    what = f"{op}: {name}"
    if got.dtype == F64 and out.dtype == F32:      # the float64 total of fp32 replicas: values only
        assert got.shape[0] == n and w.all()
    else:
        assert got.dtype == out.dtype and got.shape[0] >= n, (op, name, got.dtype, tuple(got.shape), n)
        b, sent = bits(got), (SENT16 if out.dtype == BF16 else SENT32)
        assert not (b[:n][w] == sent).any(), f"{what}: a row the operator must write still holds the sentinel"
        assert (b[:n][z] == 0).all(), f"{what}: a row the operator must zero is not zero"
        assert (b[:n][k] == sent).all() and (b[n:] == sent).all(), f"{what}: a row the operator must not touch was written"
    g, r = got[:n][w].to(F64), out.ref[w].to(F64)
    if out.exact:
        assert torch.equal(g, out.ref[w].to(out.dtype).to(F64)), f"{what}: not exact, max |diff| {(g - r).abs().max().item():.3e}"
        return 0.0
    assert torch.isfinite(g).all(), f"{what}: non-finite value"
    d, bd = (g - r).abs(), out.bound[w]
    ratio = torch.where(d == 0, torch.zeros_like(d), d / bd)
    worst = ratio.max().item() if ratio.numel() else 0.0
    key = f"{op} {name.split('[')[0]}"
    WORST[key] = max(WORST.get(key, 0.0), worst)
    assert worst <= 1.0, f"{what}: |got - ref| is {worst:.3g} x its bound (max |diff| {d.max().item():.3e})"
    return worst


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F32)


def ints(*shape, lo=-3, hi=3, seed=0):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F32)


def pow2(*shape, exps=(-1, 0, 1), seed=0):
    e = torch.tensor(exps, dtype=F32)[torch.randint(0, len(exps), shape, generator=torch.Generator().manual_seed(seed))]
    return torch.exp2(e)


def pairs(t):
    """Columns 2j and 2j + 1 made equal."""
    t = t.clone(); t[..., 1::2] = t[..., 0::2]
    return t


KEPT_SETS = ("all", "first_dropped", "last_dropped", "alternating", "one")


def kept_set(name, B):
    k = torch.ones(B, dtype=torch.bool)
    if name == "first_dropped": k[0] = False
    elif name == "last_dropped": k[-1] = False
    elif name == "alternating": k[1::2] = False
    elif name == "one": k[:] = False; k[B // 2] = True
    else: assert name == "all"
    return k


def pos_of(keep):
    """sample -> compact slot (-1: dropped), int64."""
    return torch.where(keep, torch.cumsum(keep.long(), 0) - 1, torch.full_like(keep, -1, dtype=torch.long))


def rowscale_of(keep, rate=0.2, exact=False):
    """DropPath multiplier per sample: 0 for a dropped one, 1 / (1 - rate) for a kept one (exact: rate 0.5, a power of two)."""
    return keep.to(F32) * (2.0 if exact else 1.0 / (1.0 - rate))


def ln_inputs(R, C, family, seed):
    """x, w, b, dy (bf16-exact fp32), dres, rider y (bf16-exact), gamma for R stream rows.  exact: integers and powers of two, the
    columns in equal pairs with dy antisymmetric inside a pair, so that with mean = 0, rstd = 1 the row sums of dy w and dy w xhat
    are exactly 0 and dx = dres + dy w is exact, like every product and partial sum behind it."""
    if family == "exact":
        x, w = pairs(ints(R, C, seed=seed)), pairs(pow2(C, seed=seed + 1))
        dy = ints(R, C, seed=seed + 3); dy[:, 1::2] = -dy[:, 0::2]
        return dict(x=x, w=w, b=ints(C, seed=seed + 2), dy=dy, dres=ints(R, C, seed=seed + 4), y=ints(R, C, seed=seed + 5),
                    gamma=pow2(C, exps=(-2, -1, 0), seed=seed + 6))
    q = lambda t: t.to(BF16).to(F32)      # noqa: E731
    return dict(x=rnd(R, C, seed=seed) * 2 + 0.3, w=rnd(C, seed=seed + 1) * 0.2 + 1, b=rnd(C, seed=seed + 2) * 0.1,
                dy=q(rnd(R, C, seed=seed + 3)), dres=rnd(R, C, seed=seed + 4), y=q(rnd(R, C, seed=seed + 5)),
                gamma=rnd(C, seed=seed + 6) * 0.1 + 0.5)


# ---- restatements --------------------------------------------------------------------------------------------------------------
def _rsum(t, dt):
    """Row sums; the float32 restatement adds the columns in the opposite order."""
    return (t if dt == F64 else t.flip(-1)).sum(-1, keepdim=True)


def _csum_terms(t, dt):
    return t if dt == F64 else t.flip(0)


def _scatter(rows, idx, val, cols, dt):
    o = torch.zeros(rows, cols, dtype=dt)
    o[idx] = val
    return o


def _state(rows, written=None, zero=None, default=KEEP):
    s = torch.full((rows,), default, dtype=torch.int8)
    if zero is not None: s[zero] = ZERO
    if written is not None: s[written] = WRITTEN
    return s


def ln_fwd(x, w, b, eps, M, rowidx=None, count=None, pos=None, tokens=0, stats=True, dt=F64):
    """LayerNorm forward.  rows walk: y / mean / rstd row r <- x row rowidx[r], rows >= count zero in y and untouched in the statistics.
    samples walk (pos): compact y / mean / rstd, a dropped sample's rows copied to xcopy."""
    C = x.shape[1]
    xd, wd, bd = x.to(dt), w.to(dt), b.to(dt)
    out = {}
    if pos is None:
        n = M if count is None else min(count, M)
        src = torch.arange(n) if rowidx is None else rowidx[:n].long()
        dst, rows = torch.arange(n), M
        st_y, st_s = _state(M, dst, torch.arange(n, M)), _state(M, dst)
    else:
        r = torch.arange(M); smp = r // tokens; slot = pos.long()[smp]; kept = slot >= 0
        src, dst, rows = r[kept], slot[kept] * tokens + (r[kept] - smp[kept] * tokens), (int(pos.max()) + 1) * tokens
        st_y = st_s = _state(rows, dst)
        out["xcopy"] = exact_out(x.clone(), F32, _state(M, r[~kept]))
    xs = xd[src]
    mean = _rsum(xs, dt) / C
    d = xs - mean
    rstd = (_rsum(d * d, dt) / C + eps) ** -0.5
    y = d * rstd * wd + bd
    mabs = xs.abs().sum(-1, keepdim=True) / C
    out["y"] = bf16_out(_scatter(rows, dst, y, C, dt), _scatter(rows, dst, (xs.abs() + mabs) * rstd * wd.abs() + bd.abs(), C, dt), C, st_y)
    if stats:
        out["mean"] = f32_out(_scatter(rows, dst, mean, 1, dt), _scatter(rows, dst, mabs, 1, dt), C, st_s)
        out["rstd"] = f32_out(_scatter(rows, dst, rstd, 1, dt), _scatter(rows, dst, rstd, 1, dt), C, st_s)
    return out


def ln_bwd(dy, x, mean, rstd, w, dres, M, rowidx=None, count=None, pos=None, rider=None, dy_next_rows=0, exact=False, dt=F64):
    """LayerNorm backward, dx = dres + rstd (g - mean(g) - xhat mean(g xhat)), g = dy w; dw = sum dy xhat; db = sum dy; mean / rstd are
    the saved statistics, indexed like dy.  rows walk: dy row r belongs to stream row rowidx[r], rows >= count are skipped.  samples
    walk (pos, rider cnt, or rider pos without a row list): dy compact by pos, a dropped sample passes dres through and adds nothing.
    rider (dict y, gamma, rowscale, tokens, pos, cnt, pad_base, pad2_cols; y None: no rider, only `tokens` is read): LayerScale +
    DropPath backward of the computed dx, dy_next dense or compact by its own pos; with cnt the pad rows of dy_next and pad2 are zero.
    `exact`: the column sums are exact cases."""
    C, R = x.shape[1], x.shape[0]
    rider = rider or {}
    tokens, rpos, cnt = rider.get("tokens", 0), rider.get("pos"), rider.get("cnt")
    has_ls = rider.get("y") is not None
    samples = pos is not None or cnt is not None or (rpos is not None and rowidx is None)
    if not samples:
        n = M if count is None else min(count, M)
        xr = torch.arange(n) if rowidx is None else rowidx[:n].long()
        ar = torch.arange(n)
        smp = xr // tokens if tokens else torch.zeros(n, dtype=torch.long)
    else:
        xr = torch.arange(M); smp = xr // tokens
        sa = smp if pos is None else pos.long()[smp]
        ar = torch.where(sa < 0, torch.full_like(sa, -1), sa * tokens + (xr - smp * tokens))
    t = xr - smp * tokens if tokens else xr
    own, a = ar >= 0, ar.clamp(min=0)
    o1 = own[:, None]
    wd = w.to(dt)
    g = dy.to(dt)[a] * wd
    rs = rstd.to(dt)[a][:, None]
    h = (x.to(dt)[xr] - mean.to(dt)[a][:, None]) * rs
    s1, s2 = _rsum(g, dt) / C, _rsum(g * h, dt) / C
    dr = dres.to(dt)[xr] if dres is not None else torch.zeros(len(xr), C, dtype=dt)
    dx = torch.where(o1, dr + rs * (g - s1 - h * s2), dr)
    S_dx = torch.where(o1, dr.abs() + rs * (g.abs() + g.abs().sum(-1, keepdim=True) / C + h.abs() * (g * h).abs().sum(-1, keepdim=True) / C),
                       torch.zeros_like(dr))
    out = {"dx": f32_out(_scatter(R, xr, dx, C, dt), _scatter(R, xr, S_dx, C, dt), C, _state(R, xr)),
           "dw": colsum_out(_csum_terms((dy.to(dt)[a] * h)[own], dt), exact=exact),
           "db": colsum_out(_csum_terms(dy.to(dt)[a][own], dt), exact=exact),
           "passthrough_rows": xr[~own]}
    if has_ls:
        dp = rider["rowscale"].to(dt)[smp][:, None] if rider.get("rowscale") is not None else torch.ones(len(xr), 1, dtype=dt)
        if rpos is None:
            yr = xr
        else:
            sb = rpos.long()[smp]
            yr = torch.where(sb < 0, torch.full_like(sb, -1), sb * tokens + t)
        act = yr >= 0
        e = (dx * dp)[act]
        S_e = ((S_dx + torch.where(o1, torch.zeros_like(dr), dr.abs())) * dp.abs())[act]
        gm, yv = rider["gamma"].to(dt), rider["y"].to(dt)[xr][act]
        rows = dy_next_rows or R
        st = _state(rows, yr[act])
        if cnt is not None:
            npad = ((rider.get("pad_base", 0) + cnt + 63) // 64) * 64 - rider.get("pad_base", 0)
            st[cnt:npad] = ZERO
            if rider.get("pad2_cols"):
                out["pad2"] = exact_out(torch.zeros(npad, rider["pad2_cols"], dtype=dt), BF16, _state(npad, zero=torch.arange(cnt, npad)))
        out["dy_next"] = bf16_out(_scatter(rows, yr[act], e * gm, C, dt), _scatter(rows, yr[act], S_e * gm.abs(), C, dt), C, st)
        out["dy_next_idx"], out["dy_next_src"] = yr[act], xr[act]          # the written rows in walk order, and their stream rows
        out["dgamma"] = colsum_out(_csum_terms(e * yv, dt), extra=gamma_row(C) * ((S_dx * dp.abs())[act] * yv.abs()).sum(0), exact=exact)
        out["dbias_unrounded"] = (e * gm).sum(0)
    return out


def ls_bwd(d, y, gamma, rowscale, tokens, M, rowidx=None, count=None, exact=False, dt=F64):
    """LayerScale + DropPath backward on its own over the residual-stream gradient d: e = d dp, dy = bf16(e gamma), dgamma = sum e y.
    Row list: dy is compact, row r reads stream row rowidx[r]; rows count .. M of dy are zero."""
    C = d.shape[1]
    n = M if rowidx is None else min(count, M)
    xr = torch.arange(n) if rowidx is None else rowidx[:n].long()
    dp = rowscale.to(dt)[xr // tokens][:, None] if rowscale is not None else 1.0
    e = d.to(dt)[xr] * dp
    dyn = e * gamma.to(dt)
    return {"dy": bf16_out(_scatter(M, torch.arange(n), dyn, C, dt), _scatter(M, torch.arange(n), dyn.abs(), C, dt), C,
                           _state(M, torch.arange(n), torch.arange(n, M))),
            "dy_idx": torch.arange(n),
            "dgamma": colsum_out(_csum_terms(e * y.to(dt)[xr], dt), exact=exact),
            "dbias_unrounded": dyn.sum(0)}


def colsum(y, col0, ncols, M, exact=False, dt=F64):
    return {"out": colsum_out(_csum_terms(y[:M, col0:col0 + ncols].to(dt), dt), exact=exact)}


def reduce_replicas(rep, out0, dt=F64):
    """out0 + the sum of the replicas rep [nrep, n]."""
    return {"out": colsum_out(_csum_terms(torch.cat([out0.reshape(1, -1), rep]).to(dt), dt))}


def token_bwd(dx, mask, B, P, dcls0, dmask0, exact=False, dt=F64):
    """Token-assembly backward: dpatch = dx[:, 1:] with the masked rows zero, dcls = dcls0 + sum_b dx[b, 0], dmask_token = dmask0 + the
    sum of the masked rows (what the accumulators held is one more term of the sum)."""
    C = dx.shape[-1]
    d = dx.to(dt).reshape(B, P + 1, C)
    m = mask.reshape(B, P).bool()
    patch = d[:, 1:].reshape(B * P, C)
    dpatch = torch.where(m.reshape(-1, 1), torch.zeros_like(patch), patch)
    return {"dpatch": Out(dpatch, BF_ULP * dpatch.abs().to(F64), BF16),
            "dcls": colsum_out(_csum_terms(torch.cat([dcls0.to(dt)[None], d[:, 0]]), dt), exact=exact),
            "dmask_token": colsum_out(_csum_terms(torch.cat([dmask0.to(dt)[None], patch[m.reshape(-1)]]), dt), exact=exact)}


def transpose(src):
    return {"dst": exact_out(src.t().contiguous(), BF16)}


def droppath_lists(keep, tokens, rows_stride):
    """The lists of one (layer, branch): keep [B] bool -> pos [B], bmap [B] (0 behind the kept samples), rows [rows_stride] (-1 on the
    pad rows up to the next multiple of 64, untouched behind them), cnt = kept rows.  int32 Outs, all exact."""
    B = keep.numel()
    pos = pos_of(keep)
    kept = torch.nonzero(keep).flatten()
    bmap = torch.zeros(B, dtype=torch.long); bmap[:len(kept)] = kept
    n = len(kept) * tokens
    npad = (n + 63) // 64 * 64
    rows = torch.full((rows_stride,), -1, dtype=torch.long)
    rows[:n] = (kept[:, None] * tokens + torch.arange(tokens)[None]).flatten()
    return dict(pos=pos, bmap=bmap, rows=rows, rows_written=npad, cnt=n)


def resid_rows(a, wt, bias, gamma, resid, rowscale, tokens, rowmap, rowcount, M, dt=F64):
    """RESID epilogue over a row list: GEMM row m < rowcount stands for stream row rowmap[m]: out2 = bf16(a w^T + bias) and
    out = resid + rowscale[row / tokens] gamma (a w^T + bias) are written THERE, every other stream row is untouched."""
    R, N, K = resid.shape[0], wt.shape[0], a.shape[1]
    n = min(rowcount, M)
    xr = rowmap[:n].long()
    ad, wd = a.to(dt)[:n], wt.to(dt)
    yv = ad @ wd.t() + bias.to(dt)
    S_y = ad.abs() @ wd.abs().t() + bias.to(dt).abs()
    dp = rowscale.to(dt)[xr // tokens][:, None] if rowscale is not None else 1.0
    sc = dp * gamma.to(dt)
    out = resid.to(dt)[xr] + sc * yv
    st = _state(R, xr)
    g = gamma_gemm(K)
    return {"out2": bf16_out(_scatter(R, xr, yv, N, dt), _scatter(R, xr, S_y, N, dt), N, st, g=g),
            "out": f32_out(_scatter(R, xr, out, N, dt), _scatter(R, xr, resid.to(dt)[xr].abs() + abs(sc) * S_y, N, dt), N, st, g=g)}


def wgrad_split(Y, X, s1_row, bias_end, bias2_begin):
    """dW = Y^T X and the per-stream bias sums of the stacked rows: [0, s1_row) and [s1_row, M) (exact family: all exact)."""
    Yd, Xd = Y.to(F64), X.to(F64)
    o = {"C": exact_out(Yd.t() @ Xd, F32)}
    for name, lo, hi in (("", 0, s1_row), ("_s1", s1_row, Y.shape[0])):
        o["bias" + name] = colsum_out(Yd[lo:hi, :bias_end], exact=True)
        o["bias2" + name] = colsum_out(Yd[lo:hi, bias2_begin:], exact=True)
    return o


# ---- what the launchers refuse -------------------------------------------------------------------------------------------------
def refused_calls(L, p):
    """(what, return code, expected code) of calls the entry points must refuse before they touch the device: -1 (UVIT_ERR_ARG) for a
    NULL mandatory pointer, -2 (UVIT_ERR_SHAPE) for what uvit_ln_fwd_launch, uvit_ln_bwd_launch and the other launchers refuse.
    p: any non-NULL address; a refused call neither reads nor writes it."""
    import ctypes as C
    from uncertainty_vit_amd.native import GemmEpilogue, LsRider, TransposeDesc, WgradProblem, WgradSplit
    v, f, N = C.c_void_p(p), C.c_float(1e-6), None
    out = []

    def fwd(what, want, x=v, y=v, mean=v, rstd=v, M=14, Cd=128, rowidx=N, count=N, pos=N, xcopy=N, tokens=0):
        out.append((f"ln_fwd_walk: {what}", L.uvit_op_ln_fwd_walk(x, v, v, y, mean, rstd, M, Cd, f, rowidx, count, pos, xcopy, tokens, N), want))

    fwd("pos without xcopy", -2, pos=v, tokens=7)
    fwd("xcopy without pos", -2, xcopy=v, tokens=7)
    fwd("M % tokens != 0", -2, pos=v, xcopy=v, tokens=5)
    fwd("samples walk without tokens", -2, pos=v, xcopy=v)
    fwd("a row list together with pos", -2, pos=v, xcopy=v, tokens=7, rowidx=v, count=v)
    fwd("samples walk without statistics", -2, pos=v, xcopy=v, tokens=7, mean=N, rstd=N)
    fwd("C = 130", -2, Cd=130)
    fwd("C = 2052", -2, Cd=2052)
    fwd("x NULL", -1, x=N)
    fwd("y NULL", -1, y=N)
    fwd("mean without rstd", -1, rstd=N)

    def rider(**kw):
        r = LsRider()
        for k, val in kw.items():
            setattr(r, k, p if val is v else val)
        return r

    full = dict(y=v, gamma=v, dy=v, dgamma=v, dbias=v, tokens=7)

    def bwd(what, want, dy=v, dres=v, dx=v, M=14, Cd=128, rowidx=N, count=N, pos=N, nxt=None, nrep=1):
        out.append((f"ln_bwd_walk: {what}", L.uvit_op_ln_bwd_walk(dy, v, v, v, v, dres, dx, v, v, M, Cd, nrep, Cd, rowidx, count, pos,
                                                                  N if nxt is None else C.byref(nxt), N), want))

    bwd("a row list without a count", -2, rowidx=v)
    bwd("a samples walk without dres", -2, pos=v, dres=N, nxt=rider(tokens=7))
    bwd("a samples walk without tokens", -2, pos=v)
    bwd("a samples walk with M % tokens != 0", -2, pos=v, nxt=rider(tokens=5))
    bwd("a samples walk with a row list", -2, pos=v, rowidx=v, count=v, nxt=rider(tokens=7))
    bwd("rider pos without a rider dy", -2, nxt=rider(tokens=7, pos=v))
    bwd("rider cnt without a rider dy", -2, nxt=rider(tokens=7, cnt=v))
    bwd("pad2 without cnt", -2, nxt=rider(pad2=v, pad2_cols=384, **full))
    bwd("pad2_cols % 4 != 0", -2, nxt=rider(cnt=v, pad2=v, pad2_cols=386, **full))
    bwd("pad_base < 0", -2, nxt=rider(cnt=v, pad_base=-64, **full))
    bwd("a rider without tokens", -2, nxt=rider(**dict(full, tokens=0)))
    bwd("C = 130", -2, Cd=130)
    bwd("C = 2052", -2, Cd=2052)
    bwd("dy NULL", -1, dy=N)
    bwd("dx NULL", -1, dx=N)
    bwd("a rider dy without its y", -1, nxt=rider(**dict(full, y=0)))
    bwd("nrep = 0", -1, nrep=0)

    r = rider(**full)
    out += [("ls_bwd: rider NULL", L.uvit_op_ls_bwd(v, N, 14, 128, 1, 128, N, N, N), -1),
            ("ls_bwd: dx NULL", L.uvit_op_ls_bwd(N, C.byref(r), 14, 128, 1, 128, N, N, N), -1),
            ("ls_bwd: a row list without a count", L.uvit_op_ls_bwd(v, C.byref(r), 14, 128, 1, 128, v, N, N), -2),
            ("ls_bwd: C = 130", L.uvit_op_ls_bwd(v, C.byref(r), 14, 130, 1, 128, N, N, N), -2),
            ("colsum: y NULL", L.uvit_op_colsum(N, 24, 16, 8, 4, v, 1, 8, N), -1),
            ("colsum: ncols % 8 != 0", L.uvit_op_colsum(v, 24, 16, 4, 4, v, 1, 8, N), -2),
            ("colsum: columns beyond ld", L.uvit_op_colsum(v, 24, 24, 8, 4, v, 1, 8, N), -2),
            ("reduce_replicas: out NULL", L.uvit_op_reduce_replicas(v, N, 8, 2, 8, N), -1),
            ("reduce_replicas: n % 4 != 0", L.uvit_op_reduce_replicas(v, v, 6, 2, 8, N), -2),
            ("reduce_replicas: stride % 4 != 0", L.uvit_op_reduce_replicas(v, v, 8, 2, 10, N), -2)]
    hc = (C.c_int32 * 2)(1, 1)
    out += [("droppath_lists: pos NULL", L.uvit_op_droppath_lists(v, N, v, v, v, 2, 11, 7, 128, hc, N), -1),
            ("droppath_lists: host_counts NULL", L.uvit_op_droppath_lists(v, v, v, v, v, 2, 11, 7, 128, N, N), -1),
            ("droppath_lists: no list", L.uvit_op_droppath_lists(v, v, v, v, v, 0, 11, 7, 128, hc, N), -1),
            ("droppath_lists: rows_stride below the padded rows", L.uvit_op_droppath_lists(v, v, v, v, v, 2, 11, 7, 77, hc, N), -1)]
    ep = GemmEpilogue()
    ep.out, ep.resid, ep.ldo, ep.tokens = p, p, 256, 7
    out += [("gemm_nt_rows: a mode other than RESID", L.uvit_op_gemm_nt_rows(0, v, v, 64, 256, 128, 128, 128, C.byref(ep), v, v, N, N), -1),
            ("gemm_nt_rows: rowmap NULL", L.uvit_op_gemm_nt_rows(3, v, v, 64, 256, 128, 128, 128, C.byref(ep), N, v, N, N), -1),
            ("gemm_nt_rows: rowcount NULL", L.uvit_op_gemm_nt_rows(3, v, v, 64, 256, 128, 128, 128, C.byref(ep), v, N, N, N), -1),
            ("gemm_nt_rows: K % 64 != 0", L.uvit_op_gemm_nt_rows(3, v, v, 64, 256, 120, 120, 120, C.byref(ep), v, v, N, N), -2)]
    q, sp = WgradProblem(), WgradSplit()
    q.Y, q.X, q.C, q.bias, q.bias_end, q.M, q.N, q.K, q.ldy, q.ldx, q.ldc = p, p, p, p, 256, 1024, 256, 256, 256, 256, 256
    sp.bias_s1, sp.s1_row = p, 448
    out += [("wgrad_group_split: split NULL", L.uvit_op_wgrad_group_split(C.byref(q), N, 1, N, N), -1),
            ("wgrad_group_split: s1_row not half of the 64-row tiles", L.uvit_op_wgrad_group_split(C.byref(q), C.byref(sp), 1, N, N), -2)]
    sp.s1_row = 520
    out.append(("wgrad_group_split: s1_row % 64 != 0", L.uvit_op_wgrad_group_split(C.byref(q), C.byref(sp), 1, N, N), -2))
    sp.s1_row, sp.bias_s1 = 512, None
    out.append(("wgrad_group_split: a split without bias_s1", L.uvit_op_wgrad_group_split(C.byref(q), C.byref(sp), 1, N, N), -2))
    sp.bias_s1, q.M = p, 960
    out.append(("wgrad_group_split: a split below 1024 rows", L.uvit_op_wgrad_group_split(C.byref(q), C.byref(sp), 1, N, N), -2))
    out += [("token_bwd: mask NULL", L.uvit_op_token_bwd(v, N, v, v, v, 3, 9, 128, N), -1),
            ("token_bwd: C % 4 != 0", L.uvit_op_token_bwd(v, v, v, v, v, 3, 9, 130, N), -2),
            ("token_bwd: C = 2052", L.uvit_op_token_bwd(v, v, v, v, v, 3, 9, 2052, N), -2),
            ("transpose_batch: descs NULL", L.uvit_op_transpose_batch(N, 1, 1, N), -1),
            ("transpose_batch: no tiles", L.uvit_op_transpose_batch(v, 1, 0, N), -1)]
    assert C.sizeof(TransposeDesc) == 32 and C.sizeof(LsRider) == 96 and C.sizeof(WgradSplit) == 24
    return out
