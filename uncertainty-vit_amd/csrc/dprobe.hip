// Probe of the two-stream (mean, covariance) model (gfx950), DESIGN.md section 9.17:
//   pool + norm      modeling_finetune_dist.py:280-326   both streams of the last block through fc_norm(x[:, 1:].mean(1)), no affine
//   variance         this project's definition           v = s (ELU(c) + 1) of the covariance stream's feature c, read as f ~ N(m, diag(v));
//                                                        the linear head carries it to var[b, k] = sum_c W[k, c]^2 v[b, c]
// The pair op runs the kernels of probe_pool.h with the stream index on grid.z: each output equals uvit_op_probe_pool_norm on that
// stream alone bit for bit.  The variance is double on fp32 inputs widened: (double) w * (double) w is exact (48 bits), every var[b, k]
// is one fma chain over c in ascending order, trace[b] is a fixed-order double sum rounded once.  No atomics.  The link behind it
// is uvit_op_lap_probit (laplace.hip).
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums below is part of the contract.
#ifdef __FAST_MATH__
#error "dprobe.hip fixes the order of its sums: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"
#include "probe_pool.h"

#define DPROBE_MAX_K 65535   // classes: K / 32 column tiles on grid.x

// v = s (ELU(c) + 1), the map the model applies to its covariances (modeling_finetune_dist.py:127), in double.  A NaN c gives NaN.
__device__ __forceinline__ double dprobe_v(float c, double scale) {
    const double cd = (double)c;
    const double e = cd > 0.0 ? cd + 1.0 : exp(cd);          // NaN > 0 is false: exp(NaN) = NaN
    return scale * e;
}

// ---- variance: var (B, K) = V (B, C) . (W o W)^T with V = v(cfeat); uvit_op_lap_variance's output tiles ----
// A workgroup of 128 threads owns 16 rows x 32 classes, a thread 2 x 2 of them; a tile holds 16 reduction steps; the next tile's
// global loads are issued before the current tile's arithmetic.  Every element is one fma chain over c in ascending order; rows and
// classes past the edge and columns past C hold zeros, and fma(0, 0, acc) = acc.  A NaN v reaches every class of its own row (NaN
// times a zero weight is NaN) and no other row: a row's chain reads that row's v alone.
#define DM 16
#define DN 32
#define DK 16
#define DXQ (DM * DK / 128)  // staged elements of V per thread
#define DWQ (DN * DK / 128)  // staged elements of W per thread
__global__ __launch_bounds__(128)
void dprobe_variance_kernel(const float* __restrict__ cfeat, const float* __restrict__ W, double scale, double* __restrict__ var, int B,
                            int K, int C) {
    __shared__ __attribute__((aligned(16))) double Vs[DK][DM + 2], Ws[DK][DN + 2];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int k0 = blockIdx.x * DN, b0 = blockIdx.y * DM;
    double xv[DXQ], wv[DWQ];
    auto load = [&](int c0) {                                 // element tid + 128 q of a (rows, DK) tile: adjacent lanes, adjacent c
#pragma unroll
        for (int q = 0; q < DXQ; ++q) {
            const int b = b0 + (tid + 128 * q) / DK, c = c0 + (tid + 128 * q) % DK;
            xv[q] = (b < B && c < C) ? dprobe_v(cfeat[(size_t)b * C + c], scale) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < DWQ; ++q) {
            const int k = k0 + (tid + 128 * q) / DK, c = c0 + (tid + 128 * q) % DK;
            const double w = (k < K && c < C) ? (double)W[(size_t)k * C + c] : 0.0;
            wv[q] = w * w;                                    // exact: two 24-bit significands
        }
    };
    double acc[2][2] = {};
    load(0);
    for (int c0 = 0; c0 < C; c0 += DK) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < DXQ; ++q) Vs[(tid + 128 * q) % DK][(tid + 128 * q) / DK] = xv[q];
#pragma unroll
        for (int q = 0; q < DWQ; ++q) Ws[(tid + 128 * q) % DK][(tid + 128 * q) / DK] = wv[q];
        __syncthreads();
        if (c0 + DK < C) load(c0 + DK);
#pragma unroll
        for (int c = 0; c < DK; ++c) {
            const double2 x = *(const double2*)&Vs[c][ty * 2], w = *(const double2*)&Ws[c][tx * 2];
            acc[0][0] = fma(x.x, w.x, acc[0][0]); acc[0][1] = fma(x.x, w.y, acc[0][1]);
            acc[1][0] = fma(x.y, w.x, acc[1][0]); acc[1][1] = fma(x.y, w.y, acc[1][1]);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int b = b0 + ty * 2 + i;
        if (b >= B) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + tx * 2 + j;
            if (k < K) var[(size_t)b * K + k] = acc[i][j];
        }
    }
}

// ---- trace[b] = mean_c v[b, c]: one wave per row; lane l adds its columns l, l + 64, ... in ascending order, then the xor tree ----
__global__ __launch_bounds__(256)
void dprobe_trace_kernel(const float* __restrict__ cfeat, double scale, float* __restrict__ trace, int B, int C) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    double acc = 0.0;
    for (int c = lane; c < C; c += 64) acc += dprobe_v(cfeat[(size_t)b * C + c], scale);
    acc = wave_sum(acc);
    if (lane == 0) trace[b] = (float)(acc / (double)C);
}

// ---- launchers: arguments are validated before anything touches the device ----
extern "C" int64_t uvit_op_dprobe_pool_ws_bytes(int B, int N, int C) {
    if (probe_pool_bad_shape(B, N, C)) return UVIT_ERR_SHAPE;
    return POOL_MAX_STREAMS * probe_pool_stream_bytes(B, C);
}

extern "C" int uvit_op_dprobe_pool_norm(const float* x_mean, const float* x_cov, float* feat_mean, float* feat_cov, float* scratch, int B,
                                        int N, int C, float eps, uvit_stream stream) {
    if (!x_mean || !x_cov || !feat_mean || !feat_cov || !scratch) return UVIT_ERR_ARG;
    if (probe_pool_bad_shape(B, N, C)) return UVIT_ERR_SHAPE;
    probe_pool_launch(PoolStreams{{x_mean, x_cov}, {feat_mean, feat_cov}}, POOL_MAX_STREAMS, scratch, B, N, C, eps, (hipStream_t)stream);
    return uvit_check_launch();
}

extern "C" int uvit_op_dprobe_variance(const float* cfeat, const float* W, double scale, double* var, float* trace, int B, int K, int C,
                                       uvit_stream stream) {
    if (!cfeat || !W || !var || !(scale > 0.0) || !(scale < INFINITY)) return UVIT_ERR_ARG;
    if (B < 1 || B > POOL_MAX_B || K < 1 || K > DPROBE_MAX_K || C < 4 || (C % 4) || C > ROW_MAXV * 256) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dprobe_variance_kernel, dim3((K + DN - 1) / DN, (B + DM - 1) / DM), dim3(128), 0, s, cfeat, W, scale, var, B, K, C);
    if (trace) hipLaunchKernelGGL(dprobe_trace_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, cfeat, scale, trace, B, C);
    return uvit_check_launch();
}
