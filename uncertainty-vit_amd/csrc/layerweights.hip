// Learned layer weights over every block's pooled output (gfx950): the reference's `--learn_layer_weights`
//   pool             modeling_finetune.py:499-508   p_l = x_l.mean(1) over ALL tokens (x_l[:, 0] with --use_cls), optionally
//                                                    F.layer_norm(p_l, (C,)) without affine (--layernorm_before_combine)
//   combine          modeling_finetune.py:509-510   feat = sum_l softmax(layer_log_weights)_l p_l
//   input gradient   autograd of the nn.Linear      dfeat = dlogits . W
//   weight gradient  autograd of the softmax mix    g_l = <dfeat, p_l>, dlog_w_l = w_l (g_l - sum_j w_j g_j)
// All fp32 in memory; g_l and what follows it are double.  No float atomics: every sum has one owner and a fixed order, so the same
// input gives the same bits on every run.  The pool is the one op here that moves data (L x B x N x C floats per batch); it is the
// walk of probe.hip's pool with the layer as a second grid dimension, the layers' pointers travelling by value in the kernel's
// argument struct.  DESIGN.md section 9.15.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums is part of the contract, the softmax's expf is the accurate one and
// the divisions are IEEE divisions (a mean of equal values is that value, equal log-weights at L = 2^k are exactly 1 / L).
#ifdef __FAST_MATH__
#error "layerweights.hip fixes the order of its sums and relies on IEEE division: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"
#include "rowwise.h"

#define LW_SLICES 8          // token slices per (sample, layer): B x L x 8 workgroups stream the residual streams
#define LW_WAVES 4
#define LW_MAX_B 65535       // samples ride on grid.z
#define LW_PT 64             // the contraction: 64 x 64 output tile, 16 reduction steps per LDS tile (probe.hip's scheme)
#define LW_PK 16

struct LwLayers { const float* x[UVIT_MAX_DEPTH]; };

// ---- pool, mode 0: partial column sums of tokens 0..N-1, one workgroup per (slice, layer, sample); wave w takes the slice's tokens
// w, w + 4, ...  A slice past the last token writes zeros. ----
template <int NV>
__global__ __launch_bounds__(64 * LW_WAVES)
void lw_pool_partial_kernel(const LwLayers layers, float* __restrict__ scratch, int L, int N, int C) {
    __shared__ float4 red[LW_WAVES - 1][NV * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slice = blockIdx.x, l = blockIdx.y, b = blockIdx.z, nv = C >> 2;
    const float* __restrict__ x = layers.x[l];
    const int per = (N + LW_SLICES - 1) / LW_SLICES;
    const int t0 = slice * per, t1 = min(N, t0 + per);
    RowVec<NV> acc, r;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = t0 + wave; t < t1; t += LW_WAVES) {
        load_row(r, x + ((size_t)b * N + t) * C, C, lane);
#pragma unroll
        for (int k = 0; k < NV; ++k) { acc.v[k].x += r.v[k].x; acc.v[k].y += r.v[k].y; acc.v[k].z += r.v[k].z; acc.v[k].w += r.v[k].w; }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave - 1][lane + 64 * k] = acc.v[k];
    }
    __syncthreads();
    if (wave == 0) {
        float* dst = scratch + (((size_t)b * L + l) * LW_SLICES + slice) * C;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = lane + 64 * k;
            if (i < nv) {
                float4 a = acc.v[k];
                for (int w = 0; w < LW_WAVES - 1; ++w) { const float4 o = red[w][i]; a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w; }
                ((float4*)dst)[i] = a;
            }
        }
    }
}

// ---- finish: one wave per (sample, layer) row.  mode 0: the slices added in slice order, divided by N; mode 1: token 0 of the layer,
// nothing else of it is read.  Then, with layernorm, the affine-free LayerNorm of the row (two-pass variance). ----
template <int NV>
__global__ __launch_bounds__(256)
void lw_pool_finish_kernel(const LwLayers layers, const float* __restrict__ scratch, float* __restrict__ pooled, int rows, int L, int N,
                           int C, int mode, int layernorm, float eps) {
    const int lane = WavePerRow::lane(), row = WavePerRow::row(), nv = C >> 2;
    if (row >= rows) return;
    const int b = row / L, l = row - b * L;
    RowVec<NV> acc, r;
    if (mode == 1) {
        load_row(acc, layers.x[l] + (size_t)b * N * C, C, lane);
    } else {
        const float* src = scratch + (size_t)row * LW_SLICES * C;
        load_row(acc, src, C, lane);
        for (int s = 1; s < LW_SLICES; ++s) {
            load_row(r, src + (size_t)s * C, C, lane);
#pragma unroll
            for (int k = 0; k < NV; ++k) { acc.v[k].x += r.v[k].x; acc.v[k].y += r.v[k].y; acc.v[k].z += r.v[k].z; acc.v[k].w += r.v[k].w; }
        }
        const float n = (float)N;
#pragma unroll
        for (int k = 0; k < NV; ++k) { acc.v[k].x /= n; acc.v[k].y /= n; acc.v[k].z /= n; acc.v[k].w /= n; }
    }
    float mean = 0.f, rstd = 1.f;
    if (layernorm) row_stats(acc, C, lane, eps, mean, rstd);
    float* dst = pooled + (size_t)row * C;
    if (layernorm) {
        normalize_store(acc, mean, rstd, dst, false, nv, lane);
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (lane + 64 * k < nv) ((float4*)dst)[lane + 64 * k] = acc.v[k];
    }
}

// w = softmax(log_w) of L <= 64 values, lane l holding w_l (0 in the lanes from L on): the maximum subtracted, the exponentials added by
// the xor tree, one IEEE division per lane.  The same instructions in the forward and in the gradient: the same bits.
__device__ __forceinline__ float lw_softmax(const float* __restrict__ log_w, int L, int lane) {
    const float v = lane < L ? log_w[lane] : -INFINITY;
    const float m = wave_max(v);
    const float e = lane < L ? expf(v - m) : 0.f;
    return e / wave_sum(e);
}

// ---- combine: feat[b] = sum_l w_l pooled[b, l], an fma chain in layer order from 0; one wave per sample ----
template <int NV>
__global__ __launch_bounds__(256)
void lw_combine_kernel(const float* __restrict__ pooled, const float* __restrict__ log_w, float* __restrict__ feat,
                       float* __restrict__ w_out, int B, int L, int C) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row(), nv = C >> 2;
    if (b >= B) return;
    const float w = lw_softmax(log_w, L, lane);
    if (w_out && b == 0 && lane < L) w_out[lane] = w;
    RowVec<NV> acc, r;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < L; ++l) {
        const float wl = __shfl(w, l, 64);
        load_row(r, pooled + ((size_t)b * L + l) * C, C, lane);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            acc.v[k].x = fmaf(wl, r.v[k].x, acc.v[k].x); acc.v[k].y = fmaf(wl, r.v[k].y, acc.v[k].y);
            acc.v[k].z = fmaf(wl, r.v[k].z, acc.v[k].z); acc.v[k].w = fmaf(wl, r.v[k].w, acc.v[k].w);
        }
    }
    float* dst = feat + (size_t)b * C;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (lane + 64 * k < nv) ((float4*)dst)[lane + 64 * k] = acc.v[k];
}

// ---- dfeat[B, C] = dlogits[B, K] . W[K, C]: the reduction runs over k in ascending order, the 16 products of a tile summed on their
// own and then added to the running sum (probe_logits_kernel's order); every output element has one owner ----
__global__ __launch_bounds__(256)
void probe_input_grad_kernel(const float* __restrict__ dlogits, const float* __restrict__ W, float* __restrict__ dfeat, int B, int K, int C) {
    __shared__ __attribute__((aligned(16))) float Ds[LW_PK][LW_PT + 4], Ws[LW_PK][LW_PT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int c0 = blockIdx.x * LW_PT, b0 = blockIdx.y * LW_PT;
    const int wr = tid >> 4, wc = (tid & 15) * 4;         // W staging: class row of the tile, first of four columns
    const int dk = tid & 15, dr = tid >> 4;               // dlogits staging: one class column, batch rows dr, dr + 16, ... (K need not be a multiple of 4)
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += LW_PK) {
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + wr < K && c0 + wc < C) w = *(const float4*)(W + (size_t)(k0 + wr) * C + c0 + wc);     // C % 4 == 0: inside the row or outside it
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + dr + 16 * i;
            d[i] = (b < B && k0 + dk < K) ? dlogits[(size_t)b * K + k0 + dk] : 0.f;
        }
        __syncthreads();
        *(float4*)&Ws[wr][wc] = w;
#pragma unroll
        for (int i = 0; i < 4; ++i) Ds[dk][dr + 16 * i] = d[i];
        __syncthreads();
        float t[4][4] = {};
#pragma unroll
        for (int k = 0; k < LW_PK; ++k) {
            const float4 dv = *(const float4*)&Ds[k][ty * 4], wv = *(const float4*)&Ws[k][tx * 4];
            const float dd[4] = {dv.x, dv.y, dv.z, dv.w}, ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) t[i][j] = fmaf(dd[i], ww[j], t[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += t[i][j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + ty * 4 + i, c = c0 + tx * 4;
        if (b < B && c < C) *(float4*)(dfeat + (size_t)b * C + c) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
    }
}

// ---- layer-weight gradient, per-row partials: part[b, l] = sum_c dfeat[b, c] pooled[b, l, c] in double (the products of two floats are
// exact there); per lane over its columns in ascending order, then the xor tree; one wave per sample ----
template <int NV>
__global__ __launch_bounds__(256)
void lw_grad_rows_kernel(const float* __restrict__ dfeat, const float* __restrict__ pooled, double* __restrict__ part, int B, int L, int C) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    RowVec<NV> d, r;
    load_row(d, dfeat + (size_t)b * C, C, lane);           // columns past the row are zeros: they add +0
    for (int l = 0; l < L; ++l) {
        load_row(r, pooled + ((size_t)b * L + l) * C, C, lane);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            s += (double)d.v[k].x * (double)r.v[k].x; s += (double)d.v[k].y * (double)r.v[k].y;
            s += (double)d.v[k].z * (double)r.v[k].z; s += (double)d.v[k].w * (double)r.v[k].w;
        }
        s = wave_sum(s);
        if (lane == 0) part[(size_t)b * L + l] = s;
    }
}

// ---- finish: lane l owns g_l = the rows' partials added in row order, then dlog_w_l = w_l (g_l - sum_j w_j g_j); one wave ----
__global__ __launch_bounds__(64)
void lw_grad_finish_kernel(const double* __restrict__ part, const float* __restrict__ log_w, float* __restrict__ dlog_w, int B, int L) {
    const int lane = threadIdx.x;
    const double w = (double)lw_softmax(log_w, L, lane);
    double g = 0.0;
    if (lane < L)
        for (int b = 0; b < B; ++b) g += part[(size_t)b * L + lane];
    const double mix = wave_sum(w * g);                    // the lanes from L on hold w = 0, g = 0
    if (lane < L) dlog_w[lane] = (float)(w * (g - mix));
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool lw_shape_ok(int B, int L, int C) {
    return B >= 1 && B <= LW_MAX_B && L >= 1 && L <= UVIT_MAX_DEPTH && C >= 4 && (C % 4) == 0 && C <= ROW_MAXV * 256;
}

extern "C" int64_t uvit_op_lw_pool_ws_bytes(int B, int L, int N, int C) {
    if (!lw_shape_ok(B, L, C) || N < 1) return UVIT_ERR_SHAPE;
    return (int64_t)B * L * LW_SLICES * C * (int64_t)sizeof(float);
}

extern "C" int uvit_op_lw_pool(const float* const* x_layers, int L, float* pooled, float* scratch, int B, int N, int C, int mode,
                               int layernorm, float eps, uvit_stream stream) {
    if (!x_layers || !pooled || !scratch || (mode != 0 && mode != 1) || (layernorm != 0 && layernorm != 1) || !(eps >= 0.f)) return UVIT_ERR_ARG;
    if (!lw_shape_ok(B, L, C) || N < 1) return UVIT_ERR_SHAPE;
    LwLayers layers = {};
    for (int l = 0; l < L; ++l) {
        if (!x_layers[l]) return UVIT_ERR_ARG;
        layers.x[l] = x_layers[l];
    }
    hipStream_t s = (hipStream_t)stream;
    const int rows = B * L;
    dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        if (mode == 0)
            hipLaunchKernelGGL((lw_pool_partial_kernel<NV>), dim3(LW_SLICES, L, B), dim3(64 * LW_WAVES), 0, s, layers, scratch, L, N, C);
        hipLaunchKernelGGL((lw_pool_finish_kernel<NV>), WavePerRow::grid(rows), WavePerRow::block(), 0, s, layers, (const float*)scratch, pooled,
                           rows, L, N, C, mode, layernorm, eps);
    });
    return uvit_check_launch();
}

extern "C" int uvit_op_lw_combine(const float* pooled, const float* log_w, float* feat, float* w_out, int B, int L, int C, uvit_stream stream) {
    if (!pooled || !log_w || !feat) return UVIT_ERR_ARG;
    if (!lw_shape_ok(B, L, C)) return UVIT_ERR_SHAPE;
    dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((lw_combine_kernel<NV>), WavePerRow::grid(B), WavePerRow::block(), 0, (hipStream_t)stream, pooled, log_w, feat, w_out,
                           B, L, C);
    });
    return uvit_check_launch();
}

extern "C" int uvit_op_probe_input_grad(const float* dlogits, const float* W, float* dfeat, int B, int K, int C, uvit_stream stream) {
    if (!dlogits || !W || !dfeat) return UVIT_ERR_ARG;
    if (B < 1 || K < 1 || C < 4 || (C % 4) || (B + LW_PT - 1) / LW_PT > 65535) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(probe_input_grad_kernel, dim3((C + LW_PT - 1) / LW_PT, (B + LW_PT - 1) / LW_PT), dim3(256), 0, (hipStream_t)stream,
                       dlogits, W, dfeat, B, K, C);
    return uvit_check_launch();
}

extern "C" int uvit_op_lw_grad(const float* dfeat, const float* pooled, const float* log_w, float* dlog_w, double* scratch, int B, int L,
                               int C, uvit_stream stream) {
    if (!dfeat || !pooled || !log_w || !dlog_w || !scratch || misaligned(scratch, 8)) return UVIT_ERR_ARG;
    if (!lw_shape_ok(B, L, C)) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((lw_grad_rows_kernel<NV>), WavePerRow::grid(B), WavePerRow::block(), 0, s, dfeat, pooled, scratch, B, L, C);
    });
    hipLaunchKernelGGL(lw_grad_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)scratch, log_w, dlog_w, B, L);
    return uvit_check_launch();
}
