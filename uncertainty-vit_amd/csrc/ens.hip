// Ensemble probe head on the frozen encoder (gfx950): M linear heads behind one pooled feature vector, the deep-ensemble baseline
// the reference evaluates with `--ensembles` (engine_for_finetuning.ensembles_evaluate, :225-343), here with the encoder forward
// shared by the members
//   lin (B, M K)       one uvit_op_probe_logits call with K := M K; member m owns columns m K .. (m + 1) K - 1
//   row_loss[b, m]   = (1 - s)(lse - z_y) + s (lse - mean_k z_k),  z = lin[b, m K : (m + 1) K]        (probe.hip's row body)
//   loss_m           = (1 / B) sum_b w[b, m] row_loss[b, m];   dlin[b, m, k] = w[b, m] (softmax(z)_k - (1 - s)[k == y] - s / K) / B
//   w[b, m]          = Poisson(1) online-bagging weight (Oza & Russell), counter-based on uvit_hash32, or 1
//   clip             = per member: norm_m over its K C weights and K biases, its gradient scaled by min(max_norm / (norm_m + 1e-6), 1)
//   combine          = mode 0: z = mean_m lin (the reference's mean of logits); mode 1: z = log mean_m softmax(lin_m); and the split
//                      of the predictive entropy of pbar = mean_m softmax(lin_m) into expected member entropy and mutual information
// One wave per (row, member) in the criterion and per row in the combination; one workgroup per member in the clip.  No float
// atomics: every floating sum has one owner and a fixed order that does not depend on the launch shape or on M, so the same input
// gives the same bits on every run and member m's outputs are those of a one-member call on its slice.  The ops are launch-bound
// (lin is 2.5 MB at B = 128, M = 5, K = 1000): coalesced lane-strided reads, nothing else is tuned.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums is part of the contract, NaN rows are found with v != v and expf /
// logf are the accurate ones.
#ifdef __FAST_MATH__
#error "ens.hip fixes the order of its sums and tests for NaN: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define ENS_MAX_M 16             // the combination keeps (max, lse) and the running argmax of every member in registers
#define ENS_CLIP_THREADS 1024

// ---- online bagging: w = #{n : u >= T[n]} with u the 23-bit uniform and T[n] = ceil(2^23 e^-1 sum_{i <= n} 1 / i!), the Poisson(1)
// CDF; an integer comparison, so host and device agree exactly.  The law is cut at 8 (P(w > 8) = 1.1e-6). ----
__host__ __device__ __forceinline__ uint32_t ens_bag_key(uint32_t seed) { return uvit_hash32(seed ^ 0x9E3779B9u); }
__host__ __device__ __forceinline__ float ens_bag_weight(uint32_t key, uint32_t idx) {
    const uint32_t u = uvit_hash32(idx ^ key) >> 9;
    const int w = (u >= 3085997u) + (u >= 6171993u) + (u >= 7714992u) + (u >= 8229324u) + (u >= 8357907u) + (u >= 8383624u) +
                  (u >= 8387910u) + (u >= 8388523u);
    return (float)w;
}

__global__ __launch_bounds__(256)
void ens_bag_weights_kernel(float* __restrict__ w, size_t n, uint32_t key) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) w[i] = ens_bag_weight(key, (uint32_t)i);
}

// ---- criterion: one wave per (row, member) pair r = b M + m, whose K logits start at lin + r K; probe_ce_kernel's row
// body, except that lse - v is formed as log(sum) - (v - max).
// row_loss holds the unweighted loss; the weight enters dlin here and the member's mean in the kernel below. ----
__global__ __launch_bounds__(256)
void ens_ce_kernel(const float* __restrict__ lin, const int64_t* __restrict__ labels, const float* __restrict__ weights, float smoothing,
                   float* __restrict__ dlin, float* __restrict__ row_loss, int* __restrict__ counters, int B, int M, int K) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (size_t)B * M) return;
    const int b = (int)(r / M), m = (int)(r % M);
    const float* z = lin + r * K;
    const int64_t y = labels[b];
    const bool valid = y >= 0 && y < (int64_t)K;     // spelled out, as in probe_ce_kernel
    float mx = -INFINITY;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, z[k]);
    mx = wave_max(mx);
    const float zy = valid ? z[y] : 0.f;
    float se = 0.f, sz = 0.f;
    int gt = 0, ge = 0;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        se += expf(v - mx);
        sz += v;
        gt += v > zy;
        ge += (v >= zy) && k != (int)y;
    }
    se = wave_sum(se); sz = wave_sum(sz);
    gt = wave_sum(gt); ge = wave_sum(ge);
    // lse - v is formed as log(se) - (v - mx): the row maximum cancels exactly instead of costing an ulp of lse
    const float lg = logf(se);
    const float nan = __uint_as_float(0x7FC00000u);
    if (lane == 0) {
        row_loss[r] = valid ? (1.f - smoothing) * (lg - (zy - mx)) + smoothing * (lg - (sz / (float)K - mx)) : nan;
        if (counters && valid) {
            if (ge == 0) atomicAdd(counters + 2 * m, 1);
            if (gt < 5) atomicAdd(counters + 2 * m + 1, 1);
        }
    }
    if (dlin) {
        const float invB = 1.0f / (float)B, uni = smoothing / (float)K, w = weights ? weights[r] : 1.0f;
        float* d = dlin + r * K;
        for (int k = lane; k < K; k += 64) {
            const float p = expf((z[k] - mx) - lg);
            d[k] = valid ? w * ((p - (k == (int)y ? 1.f - smoothing : 0.f) - uni) * invB) : nan;
        }
    }
}

// loss_out[m] = (1 / B) sum_b w[b, m] row_loss[b, m]: wave m walks its member's rows in order, 64 at a time; loss_out[M] = their mean,
// added in member order by one thread
__global__ __launch_bounds__(64 * ENS_MAX_M)
void ens_loss_mean_kernel(const float* __restrict__ row_loss, const float* __restrict__ weights, float* __restrict__ loss_out, int B, int M) {
    __shared__ float member[ENS_MAX_M];
    const int lane = threadIdx.x & 63, m = threadIdx.x >> 6;
    float acc = 0.f;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + lane;
        float v = 0.f;
        if (b < B) {
            v = row_loss[(size_t)b * M + m];
            if (weights) v *= weights[(size_t)b * M + m];
        }
        acc += wave_sum(v);
    }
    acc /= (float)B;
    if (lane == 0) { member[m] = acc; loss_out[m] = acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < M; ++i) s += member[i];
        loss_out[M] = s / (float)M;
    }
}

// ---- per-member clip: workgroup m sums the squares of its K C weights and K biases in double, norm_m = (float)sqrt, and scales its
// two segments in place.  Thread t takes the weight quads t, t + 1024, ... (K C is a multiple of 4; the four squares of a quad are
// added in element order), then the biases t, t + 1024, ...; the 1024 partial sums meet in a fixed tree through LDS.  One workgroup
// streams 3 MB at K = 1000, C = 768: 16 waves with 16-byte loads, four in flight per lane, because 256 lanes with 4-byte loads took
// 0.3 ms for it.  A gradient that is not 16-byte aligned is read by the same lanes in the same order with
// 4-byte loads, so the bits do not depend on the alignment.  The bias segment starts at M K C + m K floats, which is not 16-byte
// aligned in general: scalar accesses. ----
template <bool VEC>
__device__ __forceinline__ float4 ens_load_quad(const float* g, size_t q) {
    if (VEC) return ((const float4*)g)[q];
    return make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
}
template <bool VEC>
__device__ __forceinline__ void ens_store_quad(float* g, size_t q, float4 v) {
    if (VEC) { ((float4*)g)[q] = v; return; }
    g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
}

template <bool VEC>
__global__ __launch_bounds__(ENS_CLIP_THREADS)
void ens_clip_kernel(float* __restrict__ grad, float* __restrict__ norms, int M, int K, int C, float max_norm) {
    __shared__ double red[ENS_CLIP_THREADS];
    const int t = threadIdx.x, m = blockIdx.x;
    const size_t nw = (size_t)K * C, nq = nw / 4;
    float* gw = grad + (size_t)m * nw;
    float* gb = grad + (size_t)M * nw + (size_t)m * K;
    double acc = 0.0;
#pragma unroll 4
    for (size_t q = t; q < nq; q += ENS_CLIP_THREADS) {
        const float4 v = ens_load_quad<VEC>(gw, q);
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    for (int i = t; i < K; i += ENS_CLIP_THREADS) { const double v = (double)gb[i]; acc += v * v; }
    red[t] = acc;
    __syncthreads();
    for (int s = ENS_CLIP_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double sumsq = red[0];
    const float norm = (float)sqrt(sumsq);
    if (t == 0) norms[m] = norm;
    if (!(max_norm > 0.f) || !(sumsq - sumsq == 0.0)) return;         // norms only; a non-finite member is left to uvit_op_adamw's guard
    const float coef = fminf(max_norm / (norm + 1e-6f), 1.0f);
    if (coef == 1.0f) return;                                         // under max_norm: the member keeps its bits
#pragma unroll 4
    for (size_t q = t; q < nq; q += ENS_CLIP_THREADS) {
        float4 v = ens_load_quad<VEC>(gw, q);
        v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
        ens_store_quad<VEC>(gw, q, v);
    }
    for (int i = t; i < K; i += ENS_CLIP_THREADS) gb[i] *= coef;
}

// ---- combination: one wave per row.  Pass 1: (max, log of the shifted exp sum) of every member's K logits, kept in registers.  Pass 2, one walk over the
// classes: z[k], the running argmax of z and of every member, and in double the entropy terms of pbar and of the members.  Then
// var_pred and disagreement at k*.  p_m[k] = expf((lin - max_m) - log sum_m) in fp32, widened; every sum and logarithm of unc in double. ----
__global__ __launch_bounds__(256)
void ens_combine_kernel(const float* __restrict__ lin, int mode, float* __restrict__ z, double* __restrict__ unc, int B, int M, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* row = lin + (size_t)b * M * K;
    float mxs[ENS_MAX_M], lse[ENS_MAX_M];          // lse_m = mxs[m] + lse[m]; x - lse_m is formed as (x - mxs[m]) - lse[m]
    bool has_nan = false;
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) {
        mxs[m] = lse[m] = 0.f;
        if (m < M) {
            const float* v = row + (size_t)m * K;
            float mx = -INFINITY;
            for (int k = lane; k < K; k += 64) { const float x = v[k]; mx = fmaxf(mx, x); has_nan |= x != x; }
            mx = wave_max(mx);
            float se = 0.f;
            for (int k = lane; k < K; k += 64) se += expf(v[k] - mx);
            mxs[m] = mx;
            lse[m] = logf(wave_sum(se));
        }
    }
    has_nan = __any(has_nan);
    const float fM = (float)M, logM = logf(fM);
    const double dM = (double)M;
    float best = -INFINITY, mbest[ENS_MAX_M];
    int besti = 0x7FFFFFFF, mbesti[ENS_MAX_M];
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) { mbest[m] = -INFINITY; mbesti[m] = 0x7FFFFFFF; }
    double h_total = 0.0, h_member = 0.0;
    for (int k = lane; k < K; k += 64) {
        float x[ENS_MAX_M], zsum = 0.f, amax = -INFINITY;
        double pbar = 0.0;
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) {
            x[m] = 0.f;
            if (m < M) {
                const float v = row[(size_t)m * K + k];
                x[m] = (v - mxs[m]) - lse[m];
                zsum += v;
                amax = fmaxf(amax, x[m]);
                if (v > mbest[m]) { mbest[m] = v; mbesti[m] = k; }
                if (unc) {
                    const double p = (double)expf(x[m]);
                    pbar += p;
                    if (p > 0.0) h_member += p * log(p);
                }
            }
        }
        float zk;
        if (mode == 0) {
            zk = zsum / fM;
        } else {
            float se = 0.f;
#pragma unroll
            for (int m = 0; m < ENS_MAX_M; ++m)
                if (m < M) se += expf(x[m] - amax);
            zk = amax + logf(se) - logM;
        }
        z[(size_t)b * K + k] = zk;
        if (zk > best) { best = zk; besti = k; }
        if (unc) {
            pbar /= dM;
            if (pbar > 0.0) h_total += pbar * log(pbar);
        }
    }
    if (!unc) return;
    // argmax across the lanes: the larger value, the lower index on ties (a lane without a class holds -inf and the largest index)
    WAVE_ARGMAX(best, besti);
    int differ = 0;
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) {
        if (m < M) {
            float v = mbest[m];
            int i = mbesti[m];
            WAVE_ARGMAX(v, i);
            differ += i != besti;
        }
    }
    h_total = wave_sum(h_total);
    h_member = wave_sum(h_member);
    if (lane != 0) return;
    double* out = unc + (size_t)b * 5;
    if (has_nan || besti >= K) {
        for (int i = 0; i < 5; ++i) out[i] = quiet_nan();
        return;
    }
    double pk[ENS_MAX_M], pbar = 0.0, var = 0.0;
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) {
        pk[m] = 0.0;
        if (m < M) { pk[m] = (double)expf((row[(size_t)m * K + besti] - mxs[m]) - lse[m]); pbar += pk[m]; }
    }
    pbar /= dM;
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m)
        if (m < M) var += (pk[m] - pbar) * (pk[m] - pbar);
    const double total = -h_total, aleatoric = -h_member / dM;
    out[0] = total;
    out[1] = aleatoric;
    out[2] = fmax(total - aleatoric, 0.0);
    out[3] = var / dM;
    out[4] = (double)differ / dM;
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool ens_bad_shape(int B, int M, int K) {
    return B < 1 || K < 1 || M < 1 || M > ENS_MAX_M || ((size_t)B * M + 3) / 4 > 0x7FFFFFFFu;
}

extern "C" int uvit_op_ens_bag_weights(float* w, int B, int M, uint32_t seed, uvit_stream stream) {
    if (!w) return UVIT_ERR_ARG;
    if (ens_bad_shape(B, M, 1)) return UVIT_ERR_SHAPE;
    const size_t n = (size_t)B * M;
    hipLaunchKernelGGL(ens_bag_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, n, ens_bag_key(seed));
    return uvit_check_launch();
}

extern "C" int uvit_op_ens_ce(const float* lin, const int64_t* labels, const float* weights, float smoothing, float* dlin, float* row_loss,
                              float* loss_out, int32_t* top1_top5, int B, int M, int K, uvit_stream stream) {
    if (!lin || !labels || !row_loss || !loss_out || !(smoothing >= 0.f && smoothing < 1.f)) return UVIT_ERR_ARG;
    if (ens_bad_shape(B, M, K)) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * M;
    hipLaunchKernelGGL(ens_ce_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, lin, labels, weights, smoothing, dlin, row_loss,
                       (int*)top1_top5, B, M, K);
    hipLaunchKernelGGL(ens_loss_mean_kernel, dim3(1), dim3(64 * M), 0, s, (const float*)row_loss, weights, loss_out, B, M);
    return uvit_check_launch();
}

extern "C" int uvit_op_ens_clip(float* grad, float* norms, int M, int K, int C, float max_norm, uvit_stream stream) {
    if (!grad || !norms) return UVIT_ERR_ARG;
    if (K < 1 || M < 1 || M > ENS_MAX_M || C < 4 || (C % 4)) return UVIT_ERR_SHAPE;
    if (!misaligned(grad, 16))
        hipLaunchKernelGGL(ens_clip_kernel<true>, dim3(M), dim3(ENS_CLIP_THREADS), 0, (hipStream_t)stream, grad, norms, M, K, C, max_norm);
    else
        hipLaunchKernelGGL(ens_clip_kernel<false>, dim3(M), dim3(ENS_CLIP_THREADS), 0, (hipStream_t)stream, grad, norms, M, K, C, max_norm);
    return uvit_check_launch();
}

extern "C" int uvit_op_ens_combine(const float* lin, int mode, float* z, double* unc, int B, int M, int K, uvit_stream stream) {
    if (!lin || !z || (mode != 0 && mode != 1)) return UVIT_ERR_ARG;
    if (ens_bad_shape(B, M, K)) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(ens_combine_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, (hipStream_t)stream, lin, mode, z, unc, B, M, K);
    return uvit_check_launch();
}
