// LayerNorm forward/backward and the data2vec target builder, gfx950.  HBM-bound: one wave per
// row, float4 loads of the fp32 residual stream, row statistics by wave shuffles, bf16x4 stores.
//
// Reference: nn.LayerNorm(eps=1e-6) inside Block (modeling_finetune.py:290-299); target builder
// = affine-free F.layer_norm(eps=1e-5) per layer, mean over layers, optional post layer_norm,
// masked-row gather (engine_for_cyclical.py:92-122).
#include "common.h"
#include "uvit_internal.h"
#include "rowwise.h"

#define LN_WAVES 4

// How a kernel's row index becomes addresses (LnFwd / LnBwd in uvit_internal.h): WALK_ROWS = dense or through a row list, WALK_SAMPLES =
// dense walk of the residual stream with COMPACT branch buffers, by the per-sample maps of the drop-path sample lists (round 4).
enum LnWalk { WALK_ROWS, WALK_SAMPLES };

template <int NV, LnWalk WALK>
__global__ __launch_bounds__(LN_WAVES * 64)
void ln_fwd_kernel(const float* __restrict__ x, const int* __restrict__ rowidx, const int* __restrict__ count,
                   const int* __restrict__ pos, const float* __restrict__ w, const float* __restrict__ b, bf16* __restrict__ y,
                   float* __restrict__ mean_o, float* __restrict__ rstd_o, float* __restrict__ xcopy, int M, int C, float eps, int tokens) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nv = C >> 2;
    int src = row;
    size_t dst = row;
    if constexpr (WALK == WALK_ROWS) {
        if (row >= (count ? *count : M)) { store_zero_row<NV>(y + (size_t)row * C, nv, lane); return; }    // padded compact rows stay zero
        if (rowidx) src = rowidx[row];
    }
    RowVec<NV> r;
    load_row(r, x + (size_t)src * C, C, lane);
    if constexpr (WALK == WALK_SAMPLES) {
        const int smp = row / tokens, slot = pos[smp];
        if (slot < 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) if (lane + 64 * k < nv) ((float4*)(xcopy + (size_t)row * C))[lane + 64 * k] = r.v[k];
            return;
        }
        dst = (size_t)slot * tokens + (row - smp * tokens);
    }
    float mean, rstd;
    row_stats(r, C, lane, eps, mean, rstd);
    if (lane == 0 && (WALK == WALK_SAMPLES || mean_o)) { mean_o[dst] = mean; rstd_o[dst] = rstd; }
    normalize_store(r, mean, rstd, w, b, y + dst * C, nv, lane);
}

// Backward (LnBwd): LS = a branch's LayerScale + DropPath backward rides along on dx (LsNext), so the fp32 residual gradient is not read
// a second time by a separate pass.
//
// Shape of the launch (round 2): ONE 8-wave workgroup per CU walks a contiguous slab of rows.
//   * every operand row of a wave's NEXT row (x, dy, dres, y_next: 9 KB) is requested before the current row's two wave
//     reductions, so 2 rows x 8 waves = 144 KB are in flight per CU and the reductions / stores of one row hide under the
//     loads of the next (the old kernel asked for dres / y_next only after the reductions);
//   * the column sums (dw, db, dgamma, dbias) are reduced across the 8 waves in LDS and leave as ONE atomic per column
//     per workgroup: ~250 x 4 x C atomics per launch instead of ~900 x 4 x C (the old 4-wave blocks), 8 adders per
//     replica address instead of 28 -- same-address float atomics run at a fraction of the streaming rate
//     (MI355X_MICROARCH.md, Global float atomics), and they were a large part of this kernel's 108 us.
#define LNB_WAVES 8

// LSY: the rider also reads the branch output y and sums dgamma (false: LsNext::y is null, neither the load nor the sum exists)
template <int NV, bool LS, bool LSY>
struct LnbRow {                      // operands of one row, as loaded
    float4 x[NV], dres[NV];
    bf16x4 dy[NV], y[LSY ? NV : 1];
    float mean, rstd, dp;
    int xr;                          // residual-stream row
    int ar;                          // row of dy / mean / rstd (-1: the LayerNorm's own branch dropped the sample, dres passes through)
    int yr;                          // row of dy_next (-1: its branch dropped the sample)
};

template <int NV, LnWalk WALK, bool LS, bool LSY>
__device__ __forceinline__ void lnb_load(LnbRow<NV, LS, LSY>& r, int row, const bf16* dy, const float* x, const int* map,
                                         const float* mean_i, const float* rstd_i, const float* dres, const LsNext& ls,
                                         int C, int nv, int lane) {
    const int tokens = ls.tokens;
    r.dp = 1.0f;
    if constexpr (WALK == WALK_ROWS) {
        const int xr = map ? map[row] : row;
        r.xr = xr; r.ar = row; r.yr = xr;
        r.mean = mean_i[row]; r.rstd = rstd_i[row];
        if constexpr (LS) {
            if (ls.rowscale) r.dp = ls.rowscale[xr / tokens];
            if (ls.pos) { const int smp = xr / tokens, sl = ls.pos[smp]; r.yr = sl < 0 ? -1 : sl * tokens + (xr - smp * tokens); }
        }
    } else {
        const int smp = row / tokens, t = row - smp * tokens;
        const int sa = map ? map[smp] : smp, sb = LS ? (ls.pos ? ls.pos[smp] : smp) : -1;
        r.xr = row;
        r.ar = sa < 0 ? -1 : sa * tokens + t;
        r.yr = sb < 0 ? -1 : sb * tokens + t;
        r.mean = 0.f; r.rstd = 0.f;
        if (r.ar >= 0) { r.mean = mean_i[r.ar]; r.rstd = rstd_i[r.ar]; }
        if (r.yr >= 0 && ls.rowscale) r.dp = ls.rowscale[smp];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = lane + 64 * k;
        if (i < nv) {
            if (WALK == WALK_ROWS || r.ar >= 0) {
                r.x[k] = ((const float4*)(x + (size_t)r.xr * C))[i];
                r.dy[k] = ((const bf16x4*)(dy + (size_t)r.ar * C))[i];
            }
            r.dres[k] = WALK == WALK_SAMPLES || dres ? ((const float4*)(dres + (size_t)r.xr * C))[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (LSY) if (WALK == WALK_ROWS || r.yr >= 0) r.y[k] = ((const bf16x4*)(ls.y + (size_t)r.xr * C))[i];
        }
    }
}

// samples walk: the pad rows of dy_next (and of pad2) <- 0, see LsNext
template <int NV>
__device__ __forceinline__ void lnb_pad_fill(const LsNext& ls, int C, int nv, int lane, int wave) {
    const int n = *ls.cnt, npad = ((ls.pad_base + n + 63) & ~63) - ls.pad_base;
    for (int r = n + wave; r < npad; r += LNB_WAVES) {
        store_zero_row<NV>(ls.dy + (size_t)r * C, nv, lane);
        if (ls.pad2) for (int c = lane * 4; c < ls.pad2_cols; c += 256) *(bf16x4*)(ls.pad2 + (size_t)r * ls.pad2_cols + c) = bf16x4_zero();
    }
}

template <int NV, LnWalk WALK, bool LS, bool LSY>
__global__ __launch_bounds__(LNB_WAVES * 64)
void ln_bwd_kernel(const bf16* __restrict__ dy, const float* __restrict__ x, const int* __restrict__ map /* rowidx | pos */,
                   const int* __restrict__ count, const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                   const float* __restrict__ w, const float* __restrict__ dres, float* __restrict__ dx,
                   float* __restrict__ dw, float* __restrict__ db, int M, int C, int nrep, size_t rep_stride, LsNext ls,
                   int rows_per_block) {
    __shared__ float red[LNB_WAVES][64 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = C >> 2;
    int n_valid = M;
    if constexpr (WALK == WALK_ROWS) { if (count) n_valid = min(*count, M); }
    if constexpr (WALK == WALK_SAMPLES && LS) { if (ls.cnt && blockIdx.x == gridDim.x - 1) lnb_pad_fill<NV>(ls, C, nv, lane, wave); }
    float4 ww[NV], gm[LS ? NV : 1];
    RowVec<NV> aw, ab;
    RowVec<LSY ? NV : 1> ag;
    RowVec<LS ? NV : 1> ay;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        aw.v[k] = make_float4(0.f, 0.f, 0.f, 0.f); ab.v[k] = aw.v[k];
        ww[k] = lane + 64 * k < nv ? ((const float4*)w)[lane + 64 * k] : aw.v[k];
    }
#pragma unroll
    for (int k = 0; k < (LS ? NV : 1); ++k) {
        ay.v[k] = make_float4(0.f, 0.f, 0.f, 0.f); gm[k] = ay.v[k];
        if constexpr (LS) { if (lane + 64 * k < nv) gm[k] = ((const float4*)ls.gamma)[lane + 64 * k]; }
    }
#pragma unroll
    for (int k = 0; k < (LSY ? NV : 1); ++k) ag.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int row_end = min((int)(blockIdx.x + 1) * rows_per_block, n_valid);
    int row = blockIdx.x * rows_per_block + wave;
    LnbRow<NV, LS, LSY> cur, nxt;
    if (row < row_end) lnb_load<NV, WALK, LS, LSY>(cur, row, dy, x, map, mean_i, rstd_i, dres, ls, C, nv, lane);
    for (; row < row_end; row += LNB_WAVES) {
        const bool more = row + LNB_WAVES < row_end;
        if (more) lnb_load<NV, WALK, LS, LSY>(nxt, row + LNB_WAVES, dy, x, map, mean_i, rstd_i, dres, ls, C, nv, lane);
        const bool own = WALK == WALK_ROWS || cur.ar >= 0;      // false: the row passes dres through
        const float mean = cur.mean, rstd = cur.rstd;
        float4 g[NV], h[NV];
        float s1 = 0.f, s2 = 0.f;
        if (own) {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                if (lane + 64 * k < nv) {
                    const float d0 = bf2f(cur.dy[k][0]), d1 = bf2f(cur.dy[k][1]), d2 = bf2f(cur.dy[k][2]), d3 = bf2f(cur.dy[k][3]);
                    h[k] = normalize4(cur.x[k], mean, rstd);
                    aw.v[k].x += d0 * h[k].x; aw.v[k].y += d1 * h[k].y; aw.v[k].z += d2 * h[k].z; aw.v[k].w += d3 * h[k].w;
                    ab.v[k].x += d0; ab.v[k].y += d1; ab.v[k].z += d2; ab.v[k].w += d3;
                    g[k] = make_float4(d0 * ww[k].x, d1 * ww[k].y, d2 * ww[k].z, d3 * ww[k].w);
                    s1 += g[k].x + g[k].y + g[k].z + g[k].w;
                    s2 += g[k].x * h[k].x + g[k].y * h[k].y + g[k].z * h[k].z + g[k].w * h[k].w;
                } else {
                    g[k] = make_float4(0.f, 0.f, 0.f, 0.f); h[k] = g[k];
                }
            }
            s1 = wave_sum(s1) / C;
            s2 = wave_sum(s2) / C;
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = lane + 64 * k;
            if (i < nv) {
                float4 o = cur.dres[k];
                if (own) o = make_float4(o.x + rstd * (g[k].x - s1 - h[k].x * s2), o.y + rstd * (g[k].y - s1 - h[k].y * s2),
                                         o.z + rstd * (g[k].z - s1 - h[k].z * s2), o.w + rstd * (g[k].w - s1 - h[k].w * s2));
                ((float4*)(dx + (size_t)cur.xr * C))[i] = o;
                if constexpr (LS) if (cur.yr >= 0) {
                    bf16x4* dyn = (bf16x4*)(ls.dy + (size_t)cur.yr * C) + i;
                    if constexpr (LSY) ls_apply(o, cur.dp, cur.y[k], gm[k], dyn, ag.v[k], ay.v[k]);
                    else ls_apply(o, cur.dp, gm[k], dyn, ay.v[k]);
                }
            }
        }
        if (more) cur = nxt;
    }
    // cross-wave reduction of the column partials in LDS, then one atomic per column per workgroup, into replica
    // (block % nrep) of the accumulators (summed once per step)
    const size_t rep = (size_t)(blockIdx.x % nrep) * rep_stride;
    auto fold = [&](const float4& part, float* dst, int k) {
        __syncthreads();
        ((float4*)red[wave])[lane] = part;
        __syncthreads();
        // 8 waves x 256 floats -> wave q folds floats [32 q, 32 q + 32) of the 256 (lanes 0..31), 8 partial rows each
        if (lane < 32) {
            const int col = wave * 32 + lane;
            float sum = 0.f;
#pragma unroll
            for (int q = 0; q < LNB_WAVES; ++q) sum += red[q][col];
            const int c = 256 * k + col;                 // column of the row: float4 index (lane' + 64 k) * 4 + component
            if (c < C) atomicAdd(dst + rep + c, sum);
        }
    };
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        if (64 * k < nv) {
            fold(aw.v[k], dw, k);
            fold(ab.v[k], db, k);
            if constexpr (LSY) fold(ag.v[k], ls.dgamma, k);
            if constexpr (LS) fold(ay.v[k], ls.dbias, k);
        }
    }
}

// acc[i] (+)= layer_norm(x[rowidx[i]] - sub[rowidx[i]])  (no affine; sub == nullptr: 0).  `sub` = the stream before the
// MLP branch: x - sub is the block's `fc` output, the `--layer_results fc` target (modeling_cyclical.py:199-205).
template <int NV>
__global__ __launch_bounds__(LN_WAVES * 64)
void target_accum_kernel(const float* __restrict__ x, const float* __restrict__ sub, const int* __restrict__ rowidx,
                         const int* __restrict__ count, float* __restrict__ acc, int first, int Mmax, int C, float eps, int ln) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    if (row >= Mmax) return;
    const int nv = C >> 2;
    float4* dst = (float4*)(acc + (size_t)row * C);
    if (row >= *count) {
        if (first)
#pragma unroll
            for (int k = 0; k < NV; ++k) if (lane + 64 * k < nv) dst[lane + 64 * k] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    RowVec<NV> r;
    load_row(r, x + (size_t)rowidx[row] * C, C, lane);
    if (sub) {
        RowVec<NV> q;
        load_row(q, sub + (size_t)rowidx[row] * C, C, lane);
#pragma unroll
        for (int k = 0; k < NV; ++k) { r.v[k].x -= q.v[k].x; r.v[k].y -= q.v[k].y; r.v[k].z -= q.v[k].z; r.v[k].w -= q.v[k].w; }
    }
    float mean = 0.f, rstd = 1.f;
    if (ln) row_stats(r, C, lane, eps, mean, rstd);          // ln == 0 (--no_target_layer_norm_last): the rows are summed as they are
    normalize_store(r, mean, rstd, (float*)dst, !first, nv, lane);
}

template <int NV>
__global__ __launch_bounds__(LN_WAVES * 64)
void target_finalize_kernel(float* __restrict__ acc, const int* __restrict__ count, float inv_layers, int post_ln,
                            int Mmax, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    if (row >= Mmax || row >= *count) return;
    const int nv = C >> 2;
    RowVec<NV> r;
    load_row(r, acc + (size_t)row * C, C, lane);
#pragma unroll
    for (int k = 0; k < NV; ++k) { r.v[k].x *= inv_layers; r.v[k].y *= inv_layers; r.v[k].z *= inv_layers; r.v[k].w *= inv_layers; }
    float mean = 0.f, rstd = 1.f;
    if (post_ln) row_stats(r, C, lane, eps, mean, rstd);
    normalize_store(r, mean, rstd, acc + (size_t)row * C, false, nv, lane);
}

// Slabs per CU.  Round 3 tried 2 (512 workgroups that could rebalance when some CUs are held by RCCL channel workgroups): the step was
// slower with all CUs (25.4 -> 25.7 ms) AND with 240 / 224 CUs masked in (28.2 -> 28.8, 28.7 -> 29.5 ms; tools/cu_mask_bench.sh), so 1 stays.
#define LNB_BLOCKS_PER_CU 1
static int lnb_rows(int M, int resident_blocks_per_cu) {
    // rows per workgroup so that the grid is `resident_blocks_per_cu` balanced workgroups per CU
    static int ncu = 0;
    if (!ncu) {
        int dev = 0; hipDeviceProp_t prop;
        ncu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                  ? prop.multiProcessorCount : 256;
    }
    const int target = ncu * resident_blocks_per_cu;
    int rows = (M + target - 1) / target;
    rows = ((rows + LNB_WAVES - 1) / LNB_WAVES) * LNB_WAVES;      // every wave of a block walks the same number of rows
    return rows < LNB_WAVES ? LNB_WAVES : rows;
}

static int ln_shape_ok(int M, int C) { return (M > 0 && C > 0 && (C % 4) == 0 && C <= ROW_MAXV * 256) ? UVIT_OK : UVIT_ERR_SHAPE; }
static dim3 ln_grid(int M) { return dim3((M + LN_WAVES - 1) / LN_WAVES); }      // one wave per row

int uvit_ln_fwd_launch(const LnFwd& p, hipStream_t s) {
    const bool samples = p.pos || p.xcopy;
    if (ln_shape_ok(p.M, p.C) || (samples && (p.rowidx || p.count))) return UVIT_ERR_SHAPE;
    if (samples && (p.tokens <= 0 || (p.M % p.tokens) || !p.pos || !p.xcopy || !p.mean || !p.rstd)) return UVIT_ERR_SHAPE;
    dispatch_nv(p.C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((samples ? ln_fwd_kernel<NV, WALK_SAMPLES> : ln_fwd_kernel<NV, WALK_ROWS>), ln_grid(p.M), dim3(LN_WAVES * 64), 0, s,
                           p.x, p.rowidx, p.count, p.pos, p.w, p.b, p.y, p.mean, p.rstd, p.xcopy, p.M, p.C, p.eps, p.tokens);
    });
    return uvit_check_launch();
}
int uvit_ln_bwd_launch(const LnBwd& p, hipStream_t s) {
    const LsNext& n = p.next;
    const bool ls = n.dy != nullptr, lsy = ls && n.y != nullptr, samples = p.pos || n.cnt || (n.pos && !p.rowidx);
    if (ln_shape_ok(p.M, p.C) || (p.rowidx && !p.count) || (samples && (p.rowidx || p.count))) return UVIT_ERR_SHAPE;
    if ((ls || samples) && n.tokens <= 0) return UVIT_ERR_SHAPE;
    if (lsy && !n.dgamma) return UVIT_ERR_SHAPE;
    if (samples && ((p.M % n.tokens) || !p.dres)) return UVIT_ERR_SHAPE;
    if (((n.pos || n.cnt) && !ls) || n.pad_base < 0 || (n.pad2 && (!n.cnt || n.pad2_cols <= 0 || (n.pad2_cols % 4)))) return UVIT_ERR_SHAPE;
    const int rpb = lnb_rows(p.M, LNB_BLOCKS_PER_CU);
    dispatch_nv(p.C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        // samples walk: LS is instantiated both ways, like the rows walk (the parent tested ls.dy at run time there)
        // ... and a rider without the branch output (next.y null) is its own instantiation: no y load, no dgamma sum
        auto kernel = samples ? (lsy ? ln_bwd_kernel<NV, WALK_SAMPLES, true, true> : ls ? ln_bwd_kernel<NV, WALK_SAMPLES, true, false>
                                                                                         : ln_bwd_kernel<NV, WALK_SAMPLES, false, false>)
                              : (lsy ? ln_bwd_kernel<NV, WALK_ROWS, true, true> : ls ? ln_bwd_kernel<NV, WALK_ROWS, true, false>
                                                                                      : ln_bwd_kernel<NV, WALK_ROWS, false, false>);
        hipLaunchKernelGGL(kernel, dim3((p.M + rpb - 1) / rpb), dim3(LNB_WAVES * 64), 0, s, p.dy, p.x, samples ? p.pos : p.rowidx, p.count,
                           p.mean, p.rstd, p.w, p.dres, p.dx, p.dw, p.db, p.M, p.C, p.nrep > 0 ? p.nrep : 1, p.rep_stride, n, rpb);
    });
    return uvit_check_launch();
}
int uvit_target_accum_launch(const float* x, const int* rowidx, const int* count, float* acc, int first, int Mmax,
                             int C, float eps, hipStream_t s, const float* sub, int ln) {
    if (ln_shape_ok(Mmax, C)) return UVIT_ERR_SHAPE;
    dispatch_nv(C, [&](auto nv) {
        hipLaunchKernelGGL(target_accum_kernel<decltype(nv)::value>, ln_grid(Mmax), dim3(LN_WAVES * 64), 0, s, x, sub, rowidx, count, acc, first,
                           Mmax, C, eps, ln);
    });
    return uvit_check_launch();
}
int uvit_target_finalize_launch(float* acc, const int* count, int n_layers, int post_ln, int Mmax, int C, float eps,
                                hipStream_t s) {
    if (ln_shape_ok(Mmax, C) || n_layers <= 0) return UVIT_ERR_SHAPE;
    dispatch_nv(C, [&](auto nv) {
        hipLaunchKernelGGL(target_finalize_kernel<decltype(nv)::value>, ln_grid(Mmax), dim3(LN_WAVES * 64), 0, s, acc, count, 1.0f / n_layers,
                           post_ln, Mmax, C, eps);
    });
    return uvit_check_launch();
}

// grads[i] += sum_r rep[r][i]  (replicated column-sum accumulators -> gradient arena), once per step
__global__ __launch_bounds__(256)
void reduce_replicas_kernel(const float* __restrict__ rep, float* __restrict__ out, size_t n4, int nrep, size_t stride4) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 a = ((const float4*)out)[i];
        for (int r = 0; r < nrep; ++r) {
            const float4 b = ((const float4*)rep)[(size_t)r * stride4 + i];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        ((float4*)out)[i] = a;
    }
}
int uvit_reduce_replicas_launch(const float* rep, float* out, size_t n, int nrep, size_t stride, hipStream_t s) {
    if (n % 4 || stride % 4) return UVIT_ERR_SHAPE;
    size_t g = (n / 4 + 255) / 256;
    hipLaunchKernelGGL(reduce_replicas_kernel, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(256), 0, s, rep, out, n / 4, nrep, stride / 4);
    return uvit_check_launch();
}

// ------------------------------------------------------------------------------------------
// Dense target builder for the batch- / instance-norm target variants (engine_for_cyclical.py:94-118; flags off in every
// BASELINE config).  Those normalise over ALL tokens, so the masked-rows-only builder above cannot serve them: each
// target layer is gathered into a dense [B*P, C] buffer (cls dropped), normalised per channel over (B, T) ("batch") and /
// or per (sample, channel) over T ("instance"; both affine-free, biased variance, eps 1e-5), then accumulated.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void gather_patch_rows_kernel(const float* __restrict__ x, const float* __restrict__ sub, float* __restrict__ v, int B, int P, int C4) {
    const size_t total = (size_t)B * P * C4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / C4; const int c = (int)(i - row * C4);
        const int b = (int)(row / P), p_ = (int)(row - (size_t)b * P);
        const size_t src = ((size_t)b * (P + 1) + 1 + p_) * C4 + c;
        float4 a = ((const float4*)x)[src];
        if (sub) { const float4 q = ((const float4*)sub)[src]; a.x -= q.x; a.y -= q.y; a.z -= q.z; a.w -= q.w; }
        ((float4*)v)[i] = a;
    }
}

// one workgroup per (group of `rows` consecutive rows, 64 channels): v <- (v - mean_c) * rsqrt(var_c + eps), statistics over
// the group's rows (biased variance, accumulated in fp64)
__global__ __launch_bounds__(256)
void colnorm_kernel(float* __restrict__ v, int rows, int C, float eps) {
    __shared__ double red[2][4][64];
    __shared__ float stat[2][64];
    const int ch = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    float* base = v + (size_t)blockIdx.y * rows * C;
    double s1 = 0.0, s2 = 0.0;
    if (ch < C)
        for (int r = ph; r < rows; r += 4) { const double a = base[(size_t)r * C + ch]; s1 += a; s2 += a * a; }
    red[0][ph][threadIdx.x & 63] = s1; red[1][ph][threadIdx.x & 63] = s2;
    __syncthreads();
    if (ph == 0) {
        const int l = threadIdx.x;
        const double a = red[0][0][l] + red[0][1][l] + red[0][2][l] + red[0][3][l];
        const double q = red[1][0][l] + red[1][1][l] + red[1][2][l] + red[1][3][l];
        const double mean = a / rows, var = q / rows - mean * mean;
        stat[0][l] = (float)mean; stat[1][l] = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + (double)eps));
    }
    __syncthreads();
    if (ch < C) {
        const float mean = stat[0][threadIdx.x & 63], rstd = stat[1][threadIdx.x & 63];
        for (int r = ph; r < rows; r += 4) { float* q = base + (size_t)r * C + ch; *q = (*q - mean) * rstd; }
    }
}

__global__ __launch_bounds__(256)
void axpy_rows_kernel(float* __restrict__ acc, const float* __restrict__ v, int first, size_t n4) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 a = ((const float4*)v)[i];
        if (!first) { const float4 b = ((const float4*)acc)[i]; a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
        ((float4*)acc)[i] = a;
    }
}

// out[i] = dense[patch row of token row rowidx[i]]  (rowidx holds b * (P + 1) + 1 + p in mask order)
__global__ __launch_bounds__(256)
void gather_masked_rows_kernel(const float* __restrict__ dense, const int* __restrict__ rowidx, const int* __restrict__ count,
                               float* __restrict__ out, int Mmax, int P, int C4) {
    const int n = min(*count, Mmax);
    const size_t total = (size_t)n * C4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / C4; const int c = (int)(i - r * C4);
        const int tok = rowidx[r], b = tok / (P + 1), p_ = tok - b * (P + 1) - 1;
        ((float4*)out)[i] = ((const float4*)dense)[((size_t)b * P + p_) * C4 + c];
    }
}

static unsigned dense_grid(size_t n) { size_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

int uvit_gather_patch_rows_launch(const float* x, const float* sub, float* v, int B, int P, int C, hipStream_t s) {
    if (C % 4) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(gather_patch_rows_kernel, dim3(dense_grid((size_t)B * P * (C / 4))), dim3(256), 0, s, x, sub, v, B, P, C / 4);
    return uvit_check_launch();
}
int uvit_colnorm_launch(float* v, int groups, int rows, int C, float eps, hipStream_t s) {
    if (groups < 1 || rows < 1) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(colnorm_kernel, dim3((C + 63) / 64, groups), dim3(256), 0, s, v, rows, C, eps);
    return uvit_check_launch();
}
int uvit_axpy_rows_launch(float* acc, const float* v, int first, size_t n, hipStream_t s) {
    if (n % 4) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(axpy_rows_kernel, dim3(dense_grid(n / 4)), dim3(256), 0, s, acc, v, first, n / 4);
    return uvit_check_launch();
}
int uvit_gather_masked_rows_launch(const float* dense, const int* rowidx, const int* count, float* out, int Mmax, int P, int C,
                                   hipStream_t s) {
    if (C % 4) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(gather_masked_rows_kernel, dim3(dense_grid((size_t)Mmax * (C / 4))), dim3(256), 0, s, dense, rowidx, count, out,
                       Mmax, P, C / 4);
    return uvit_check_launch();
}
