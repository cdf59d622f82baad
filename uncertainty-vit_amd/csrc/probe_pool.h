// Pool + norm of the probe (modeling_finetune.py:410-412,512-515): t = x[:, 1:].mean(1); fc_norm(t) with elementwise_affine = False.
// The two kernels and their launch, shared by probe.hip (one residual stream) and dprobe.hip (the two streams of the two-stream
// model in one launch pair): the stream index rides on grid.z, and every (stream, sample) is summed by the same workgroups in the
// same order whatever the number of streams, so a stream's output does not depend on what travels beside it.
// For strict translation units only (no -ffast-math): the order of the sums below is part of the contract.
#pragma once
#include "probe_common.h"
#include "rowwise.h"

#define POOL_SLICES 8        // token slices per sample: B x 8 workgroups stream the residual stream (1024 at B = 128 for 256 CUs)
#define POOL_WAVES 4
#define POOL_MAX_B 65535     // samples ride on grid.y
#define POOL_MAX_STREAMS 2

// the residual streams of one launch and their outputs; stream s uses scratch + s * B * POOL_SLICES * C
struct PoolStreams {
    const float* x[POOL_MAX_STREAMS];
    float* feat[POOL_MAX_STREAMS];
};

// ---- pool: partial column sums of tokens 1..N-1, one workgroup per (slice, sample, stream); wave w takes the slice's tokens w, w + 4, ... ----
template <int NV>
__global__ __launch_bounds__(64 * POOL_WAVES)
void probe_pool_partial_kernel(PoolStreams ps, float* __restrict__ scratch, int N, int C) {
    __shared__ float4 red[POOL_WAVES - 1][NV * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slice = blockIdx.x, b = blockIdx.y, nv = C >> 2;
    const float* __restrict__ x = blockIdx.z ? ps.x[1] : ps.x[0];
    scratch += (size_t)blockIdx.z * gridDim.y * POOL_SLICES * C;
    const int per = (N - 1 + POOL_SLICES - 1) / POOL_SLICES;
    const int t0 = 1 + slice * per, t1 = min(N, t0 + per);
    RowVec<NV> acc, r;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = t0 + wave; t < t1; t += POOL_WAVES) {
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
        float* dst = scratch + ((size_t)b * POOL_SLICES + slice) * C;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = lane + 64 * k;
            if (i < nv) {
                float4 a = acc.v[k];
                for (int w = 0; w < POOL_WAVES - 1; ++w) { const float4 o = red[w][i]; a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w; }
                ((float4*)dst)[i] = a;
            }
        }
    }
}

// ---- finish: slices added in slice order, mean over the N - 1 patch tokens, affine-free LayerNorm; one wave per (sample, stream) ----
template <int NV>
__global__ __launch_bounds__(256)
void probe_pool_norm_kernel(const float* __restrict__ scratch, PoolStreams ps, int B, int N, int C, float eps) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row(), nv = C >> 2;
    if (b >= B) return;
    float* __restrict__ feat = blockIdx.z ? ps.feat[1] : ps.feat[0];
    scratch += (size_t)blockIdx.z * B * POOL_SLICES * C;
    RowVec<NV> acc, r;
    load_row(acc, scratch + (size_t)b * POOL_SLICES * C, C, lane);
    for (int s = 1; s < POOL_SLICES; ++s) {
        load_row(r, scratch + ((size_t)b * POOL_SLICES + s) * C, C, lane);
#pragma unroll
        for (int k = 0; k < NV; ++k) { acc.v[k].x += r.v[k].x; acc.v[k].y += r.v[k].y; acc.v[k].z += r.v[k].z; acc.v[k].w += r.v[k].w; }
    }
    const float inv = 1.0f / (float)(N - 1);
#pragma unroll
    for (int k = 0; k < NV; ++k) { acc.v[k].x *= inv; acc.v[k].y *= inv; acc.v[k].z *= inv; acc.v[k].w *= inv; }
    float mean, rstd;
    row_stats(acc, C, lane, eps, mean, rstd);
    normalize_store(acc, mean, rstd, feat + (size_t)b * C, false, nv, lane);
}

// ---- the limits and the launch pair; the callers have checked their pointers ----
static inline bool probe_pool_bad_shape(int B, int N, int C) {
    return B < 1 || B > POOL_MAX_B || N < 2 || C < 4 || (C % 4) || C > ROW_MAXV * 256;
}

static inline int64_t probe_pool_stream_bytes(int B, int C) { return (int64_t)B * POOL_SLICES * C * (int64_t)sizeof(float); }

static inline void probe_pool_launch(const PoolStreams& ps, int streams, float* scratch, int B, int N, int C, float eps, hipStream_t s) {
    dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((probe_pool_partial_kernel<NV>), dim3(POOL_SLICES, B, streams), dim3(64 * POOL_WAVES), 0, s, ps, scratch, N, C);
        dim3 grid = WavePerRow::grid(B);
        grid.z = streams;
        hipLaunchKernelGGL((probe_pool_norm_kernel<NV>), grid, WavePerRow::block(), 0, s, (const float*)scratch, ps, B, N, C, eps);
    });
}
