// Heteroscedastic probe head on the frozen encoder (gfx950): Monte-Carlo softmax with low-rank-plus-diagonal logit noise, the layer
// the reference names modeling_finetune.MCSoftmaxDenseFA (:904-1217; Collier et al., CVPR 2021; edward2's class of that name, the
// non-parameter-efficient form), behind the probe's pooled features
//   lin[b] = [ loc (K) | draw (K) | V (K, R) row-major ]    one uvit_op_probe_logits call;   d = draw + 1e-3
//   u_s    = loc + V . epsR_s + d * epsK_s                  epsR_s (R), epsK_s (K) standard normal, s = 0 .. S-1
//   y_s    = softmax(u_s / T);   p = mean_s y_s;   z = log(clamp(p, eps, 1));   pvar = mean_s y_s^2 - p^2, clamped at 0
//   dp     = eps <= p <= 1 ? dz / p : 0;   a_s = <y_s, dp>;   du_s = y_s (dp - a_s) / (S T)
//   dlin[b] = [ sum_s du_s | sum_s du_s epsK_s | sum_s du_s (x) epsR_s ]
// The draws are counter-based on uvit_hash32 (common.h), so forward and backward regenerate them and the (B, S, K) latents never
// exist in memory.  One wave handles one sample at a time with the K classes spread over its lanes in pairs (a Box-Muller pair
// serves two adjacent classes); the row maximum, the exp sum and a_s are wave reductions.  The samples of a row are split into
// at most HET_MAX_CHUNKS chunks of het_chunk_size(S) samples, a function of S alone, one workgroup (one wave) per (row, chunk);
// the chunk sums go to `scratch` and a second kernel adds them in chunk order.  No float atomics: every sum has one owner and a fixed
// order that does not depend on the launch shape, so the same input gives the same bits on every run.  No MFMA: the rank-R product is
// R FMAs per term beside a Gaussian draw and an exp.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums is part of the contract and logf / sincosf / expf are the accurate ones.
#ifdef __FAST_MATH__
#error "het.hip fixes the order of its sums and needs accurate logf / sincosf / expf: build it without -ffast-math"
#endif
#include <math.h>

#include <type_traits>

#include "../../include/uvit.h"
#include "probe_common.h"

#define HET_MAX_B 65535
#define HET_MIN_K 3
#define HET_MAX_K 4096
#define HET_MAX_R 32
#define HET_MAX_S 65535
#define HET_MAX_CHUNKS 8         // chunks of samples per row: the partial sums in scratch are HET_MAX_CHUNKS x the output at most
#define HET_CHUNK_UNIT 64        // a chunk is a multiple of this many samples
#define HET_LDS_FLOATS 16384     // 64 KiB: V stays in LDS when K R fits; the backward's dV tile holds min(R, 16384 / K) factors
#define HET_MIN_SCALE 1e-3f      // MIN_SCALE_MONTE_CARLO: d = draw + 1e-3, no softplus (the reference's diagonal)

// samples per chunk: the smallest multiple of 64 that covers S in 8 chunks.  A function of S alone.
static inline int het_chunk_size(int S) {
    const int span = HET_MAX_CHUNKS * HET_CHUNK_UNIT;
    return HET_CHUNK_UNIT * ((S + span - 1) / span);
}
static inline int het_chunks(int S) { const int cs = het_chunk_size(S); return (S + cs - 1) / cs; }

// ---- the noise: stream t in {0: factors, 1: diagonal}, sample counter ctr = row * S + s, pair q -> values 2 q and 2 q + 1 ----
__host__ __device__ __forceinline__ uint32_t het_stream_key(uint32_t seed, uint32_t t) {
    return uvit_hash32(seed ^ ((t + 1u) * 0x9E3779B9u));
}
// (h >> 9) < 2^23, so (h >> 9) + 0.5 has 24 significant bits and the product with 2^-23 is exact: u in (0, 1)
__device__ __forceinline__ float het_uniform(uint32_t h) { return ((float)(h >> 9) + 0.5f) * 0x1p-23f; }
__device__ __forceinline__ void het_pair(uint32_t key, uint32_t q, float& n0, float& n1) {
    const float u1 = het_uniform(uvit_hash32((2u * q) ^ key)), u2 = het_uniform(uvit_hash32((2u * q + 1u) ^ key));
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);       // the accurate sinf and cosf of one argument
    n0 = r * cs;
    n1 = r * sn;
}

// one wave per (row, sample): the draws as the two kernels below form them
__global__ __launch_bounds__(64)
void het_noise_kernel(float* __restrict__ epsR, float* __restrict__ epsK, int S, int K, int R, uint32_t keyR, uint32_t keyK, int share) {
    const int lane = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const uint32_t ctr = (share ? 0u : (uint32_t)b) * (uint32_t)S + (uint32_t)s;      // mod 2^32
    const uint32_t kR = uvit_hash32(ctr ^ keyR), kK = uvit_hash32(ctr ^ keyK);
    const size_t at = (size_t)b * S + s;
    float n0, n1;
    if (epsR) {
        float* o = epsR + at * R;
        for (int q = lane; 2 * q < R; q += 64) {
            het_pair(kR, (uint32_t)q, n0, n1);
            o[2 * q] = n0;
            if (2 * q + 1 < R) o[2 * q + 1] = n1;
        }
    }
    if (epsK) {
        float* o = epsK + at * K;
        for (int q = lane; 2 * q < K; q += 64) {
            het_pair(kK, (uint32_t)q, n0, n1);
            o[2 * q] = n0;
            if (2 * q + 1 < K) o[2 * q + 1] = n1;
        }
    }
}

// ---- one sample by one wave.  Lane l owns the class pairs q = l + 64 j (classes 2 q, 2 q + 1), j < NP: NV = 2 NP values per lane ----
// Classes past K carry loc = -inf and d = 0 and read V at class K - 1: their u is -inf and their y is 0.
template <int NP, bool VLDS>
struct HetRow {
    static constexpr int NV = 2 * NP;
    float loc[NV], d[NV];
    int kc[NV];                  // the class, clamped to K - 1 (what V is read at)
    const float* Vg;             // V (K, R) row-major in global memory
    const float* Vs;             // V as [r][K] in LDS (VLDS)
    int K, R;

    __device__ __forceinline__ void load(const float* __restrict__ row, float* vs, int K_, int R_, int lane) {
        K = K_; R = R_;
        Vg = row + 2 * (size_t)K;
        Vs = vs;
        if (VLDS) {
            for (int i = lane; i < K * R; i += 64) {
                const int k = i / R, r = i - k * R;
                vs[r * K + k] = Vg[i];
            }
            __syncthreads();
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int k = 2 * (lane + 64 * (v >> 1)) + (v & 1);
            const bool in = k < K;
            kc[v] = in ? k : K - 1;
            loc[v] = in ? row[k] : -INFINITY;
            d[v] = in ? row[K + k] + HET_MIN_SCALE : 0.f;
        }
    }

    // y = softmax(u / T) of sample `ctr`; nK = the diagonal draws; eR = the factor draw r in lane r (r < R <= 32)
    __device__ __forceinline__ void sample(uint32_t ctr, uint32_t keyR, uint32_t keyK, float invT, int lane, float (&y)[NV], float (&nK)[NV],
                                           float& eR) const {
        const uint32_t kR = uvit_hash32(ctr ^ keyR), kK = uvit_hash32(ctr ^ keyK);
        float n0, n1;
        het_pair(kR, (uint32_t)(lane >> 1) & 15u, n0, n1);      // the R factor draws of the sample, formed once: lane r holds draw r
        eR = (lane & 1) ? n1 : n0;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            het_pair(kK, (uint32_t)(lane + 64 * j), nK[2 * j], nK[2 * j + 1]);
            y[2 * j] = fmaf(d[2 * j], nK[2 * j], loc[2 * j]);
            y[2 * j + 1] = fmaf(d[2 * j + 1], nK[2 * j + 1], loc[2 * j + 1]);
        }
        for (int r = 0; r < R; ++r) {
            const float er = __shfl(eR, r, 64);
#pragma unroll
            for (int v = 0; v < NV; ++v) y[v] = fmaf(VLDS ? Vs[r * K + kc[v]] : Vg[(size_t)kc[v] * R + r], er, y[v]);
        }
        float m = -INFINITY;
#pragma unroll
        for (int v = 0; v < NV; ++v) { y[v] *= invT; m = fmaxf(m, y[v]); }
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) { y[v] = expf(y[v] - m); sum += y[v]; }
        const float inv = 1.0f / wave_sum(sum);
#pragma unroll
        for (int v = 0; v < NV; ++v) y[v] *= inv;
    }
};

// ---- forward: part[(b, chunk)] = [ sum_s y_s (K) | sum_s y_s^2 (K) ] over the samples of the chunk, in sample order ----
template <int NP, bool VLDS>
__global__ __launch_bounds__(64)
void het_fwd_kernel(const float* __restrict__ lin, float* __restrict__ part, int S, int K, int R, float invT, uint32_t keyR, uint32_t keyK,
                    int share, int chunk) {
    extern __shared__ __attribute__((aligned(16))) float het_lds[];
    constexpr int NV = 2 * NP;
    const int lane = threadIdx.x, c = blockIdx.x, b = blockIdx.y;
    HetRow<NP, VLDS> row;
    row.load(lin + (size_t)b * K * (R + 2), het_lds, K, R, lane);
    float sp[NV] = {}, sp2[NV] = {}, y[NV], nK[NV], eR;
    const int s0 = c * chunk, s1 = min(S, s0 + chunk);
    const uint32_t base = (share ? 0u : (uint32_t)b) * (uint32_t)S;
    for (int s = s0; s < s1; ++s) {
        row.sample(base + (uint32_t)s, keyR, keyK, invT, lane, y, nK, eR);
#pragma unroll
        for (int v = 0; v < NV; ++v) { sp[v] += y[v]; sp2[v] = fmaf(y[v], y[v], sp2[v]); }
    }
    float* o = part + ((size_t)b * gridDim.x + c) * 2 * K;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int k = 2 * (lane + 64 * (v >> 1)) + (v & 1);
        if (k < K) { o[k] = sp[v]; o[K + k] = sp2[v]; }
    }
}

// p = (sum over the chunks in chunk order) / S; z = log(clamp(p, eps, 1)); pvar = max(mean y^2 - p^2, 0)
__global__ __launch_bounds__(256)
void het_fwd_finish_kernel(const float* __restrict__ part, float* __restrict__ z, float* __restrict__ p, float* __restrict__ pvar, int S,
                           int K, int nch, float eps) {
    const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (k >= K) return;
    const float* in = part + (size_t)b * nch * 2 * K;
    float a = 0.f, a2 = 0.f;
    for (int c = 0; c < nch; ++c) { a += in[(size_t)c * 2 * K + k]; a2 += in[(size_t)c * 2 * K + K + k]; }
    const float fS = (float)S, pk = a / fS;
    const size_t at = (size_t)b * K + k;
    p[at] = pk;
    // the logarithm in double, rounded once: B K values, and log(eps) = -16.1 is then the fp32 number next to it (logf is within 1 ulp)
    if (z) z[at] = (float)log((double)fminf(fmaxf(pk, eps), 1.0f));
    if (pvar) pvar[at] = fmaxf(a2 / fS - pk * pk, 0.f);
}

// ---- backward: part[(b, chunk)] = [ dloc (K) | ddraw (K) | dV (K, R) ] of the chunk's samples, in sample order.  blockIdx.z is a tile
// of RT factors whose dV sums live in LDS as [r][K]; tile 0 also owns dloc and ddraw (registers). ----
template <int NP, bool VLDS>
__global__ __launch_bounds__(64)
void het_bwd_kernel(const float* __restrict__ lin, const float* __restrict__ p, const float* __restrict__ dz, float* __restrict__ part, int S,
                    int K, int R, float invT, float eps, uint32_t keyR, uint32_t keyK, int share, int chunk, int RT) {
    extern __shared__ __attribute__((aligned(16))) float het_lds[];
    constexpr int NV = 2 * NP;
    const int lane = threadIdx.x, c = blockIdx.x, b = blockIdx.y, r0 = blockIdx.z * RT, nr = min(R, r0 + RT) - r0;
    float* acc = het_lds + (VLDS ? K * R : 0);            // [nr][K]
    for (int i = lane; i < nr * K; i += 64) acc[i] = 0.f;
    HetRow<NP, VLDS> row;
    row.load(lin + (size_t)b * K * (R + 2), het_lds, K, R, lane);
    __syncthreads();
    float dps[NV], gl[NV] = {}, gd[NV] = {}, y[NV], nK[NV], eR;
    const float sc = invT / (float)S;                     // du = y (dp - a) / (S T): the factor goes into dp once
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int k = 2 * (lane + 64 * (v >> 1)) + (v & 1);
        float g = 0.f;
        if (k < K) {
            const float pk = p[(size_t)b * K + k];
            if (pk >= eps && pk <= 1.0f) g = dz[(size_t)b * K + k] / pk * sc;          // the clamp's gradient
        }
        dps[v] = g;
    }
    const bool first = blockIdx.z == 0;
    const int s0 = c * chunk, s1 = min(S, s0 + chunk);
    const uint32_t base = (share ? 0u : (uint32_t)b) * (uint32_t)S;
    for (int s = s0; s < s1; ++s) {
        row.sample(base + (uint32_t)s, keyR, keyK, invT, lane, y, nK, eR);
        float a = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) a = fmaf(y[v], dps[v], a);
        a = wave_sum(a);
#pragma unroll
        for (int v = 0; v < NV; ++v) y[v] *= dps[v] - a;                               // y now holds du
        if (first) {
#pragma unroll
            for (int v = 0; v < NV; ++v) { gl[v] += y[v]; gd[v] = fmaf(y[v], nK[v], gd[v]); }
        }
        for (int r = 0; r < nr; ++r) {
            const float er = __shfl(eR, r0 + r, 64);
            float* ar = acc + r * K;
            float t[NV];                                  // one owner: class k belongs to this lane.  All reads, then all writes: the
#pragma unroll                                            // reads do not wait for one another behind a store that cannot alias them
            for (int v = 0; v < NV; ++v) t[v] = ar[row.kc[v]];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int k = 2 * (lane + 64 * (v >> 1)) + (v & 1);
                if (k < K) ar[k] = fmaf(y[v], er, t[v]);
            }
        }
    }
    __syncthreads();
    float* o = part + ((size_t)b * gridDim.x + c) * K * (R + 2);
    if (first) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int k = 2 * (lane + 64 * (v >> 1)) + (v & 1);
            if (k < K) { o[k] = gl[v]; o[K + k] = gd[v]; }
        }
    }
    for (int i = lane; i < nr * K; i += 64) {             // out in the row-major (K, R) layout of lin
        const int k = i / nr, r = i - k * nr;
        o[2 * (size_t)K + (size_t)k * R + r0 + r] = acc[r * K + k];
    }
}

// dlin[b, j] = the chunk sums added in chunk order; n = K (R + 2)
__global__ __launch_bounds__(256)
void het_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ dlin, int n, int nch) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= n) return;
    const float* in = part + (size_t)b * nch * n + j;
    float a = 0.f;
    for (int c = 0; c < nch; ++c) a += in[(size_t)c * n];
    dlin[(size_t)b * n + j] = a;
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool het_bad_shape(int B, int S, int K, int R) {
    return B < 1 || B > HET_MAX_B || S < 1 || S > HET_MAX_S || K < HET_MIN_K || K > HET_MAX_K || R < 1 || R > HET_MAX_R || R > K;
}
static inline bool het_bad_scalars(float temperature, float eps, int share) {
    return !(temperature > 0.f) || !(temperature < INFINITY) || !(eps >= 0.f) || !(eps < 1.f) || (share != 0 && share != 1);
}

template <typename F>
static inline void het_dispatch(int K, int R, F&& f) {
    const bool vlds = K * R <= HET_LDS_FLOATS;
#define HET_CASE(NP_)                                                                               \
    if (K <= 128 * NP_) {                                                                           \
        if (vlds) f(std::integral_constant<int, NP_>{}, std::true_type{});                          \
        else f(std::integral_constant<int, NP_>{}, std::false_type{});                              \
        return;                                                                                     \
    }
    HET_CASE(1) HET_CASE(4) HET_CASE(8) HET_CASE(32)
#undef HET_CASE
}

extern "C" int uvit_op_het_noise(float* epsR, float* epsK, int B, int S, int K, int R, uint32_t seed, int share, uvit_stream stream) {
    if (share != 0 && share != 1) return UVIT_ERR_ARG;
    if (het_bad_shape(B, S, K, R)) return UVIT_ERR_SHAPE;
    if (!epsR && !epsK) return UVIT_OK;
    hipLaunchKernelGGL(het_noise_kernel, dim3(S, B), dim3(64), 0, (hipStream_t)stream, epsR, epsK, S, K, R, het_stream_key(seed, 0),
                       het_stream_key(seed, 1), share);
    return uvit_check_launch();
}

extern "C" int64_t uvit_op_het_mc_ws_bytes(int B, int S, int K, int R) {
    if (het_bad_shape(B, S, K, R)) return UVIT_ERR_SHAPE;
    return (int64_t)het_chunks(S) * B * K * (R + 2) * (int64_t)sizeof(float);
}

extern "C" int uvit_op_het_mc_forward(const float* lin, float* z, float* p, float* pvar, float* scratch, int B, int S, int K, int R,
                                      float temperature, float eps, uint32_t seed, int share, uvit_stream stream) {
    if (!lin || !p || !scratch || het_bad_scalars(temperature, eps, share)) return UVIT_ERR_ARG;
    if (het_bad_shape(B, S, K, R)) return UVIT_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int nch = het_chunks(S), chunk = het_chunk_size(S);
    const float invT = 1.0f / temperature;
    const uint32_t keyR = het_stream_key(seed, 0), keyK = het_stream_key(seed, 1);
    het_dispatch(K, R, [&](auto np, auto vl) {
        constexpr int NP = decltype(np)::value;
        constexpr bool VLDS = decltype(vl)::value;
        const size_t lds = VLDS ? (size_t)K * R * sizeof(float) : 0;
        hipLaunchKernelGGL((het_fwd_kernel<NP, VLDS>), dim3(nch, B), dim3(64), lds, st, lin, scratch, S, K, R, invT, keyR, keyK, share, chunk);
    });
    hipLaunchKernelGGL(het_fwd_finish_kernel, dim3((K + 255) / 256, B), dim3(256), 0, st, (const float*)scratch, z, p, pvar, S, K, nch, eps);
    return uvit_check_launch();
}

extern "C" int uvit_op_het_mc_backward(const float* lin, const float* p, const float* dz, float* dlin, float* scratch, int B, int S, int K,
                                       int R, float temperature, float eps, uint32_t seed, int share, uvit_stream stream) {
    if (!lin || !p || !dz || !dlin || !scratch || het_bad_scalars(temperature, eps, share)) return UVIT_ERR_ARG;
    if (het_bad_shape(B, S, K, R)) return UVIT_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int nch = het_chunks(S), chunk = het_chunk_size(S);
    const int RT = R < HET_LDS_FLOATS / K ? R : HET_LDS_FLOATS / K, ntile = (R + RT - 1) / RT;      // K <= 4096: RT >= 4
    const float invT = 1.0f / temperature;
    const uint32_t keyR = het_stream_key(seed, 0), keyK = het_stream_key(seed, 1);
    int rc = UVIT_OK;
    het_dispatch(K, R, [&](auto np, auto vl) {
        constexpr int NP = decltype(np)::value;
        constexpr bool VLDS = decltype(vl)::value;
        const size_t lds = ((VLDS ? (size_t)K * R : 0) + (size_t)K * RT) * sizeof(float);        // <= 128 KiB
        auto kern = het_bwd_kernel<NP, VLDS>;
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            rc = UVIT_ERR_LAUNCH;
            return;
        }
        hipLaunchKernelGGL(kern, dim3(nch, B, ntile), dim3(64), lds, st, lin, p, dz, scratch, S, K, R, invT, eps, keyR, keyK, share, chunk, RT);
    });
    if (rc != UVIT_OK) return rc;
    const int n = K * (R + 2);
    hipLaunchKernelGGL(het_bwd_finish_kernel, dim3((n + 255) / 256, B), dim3(256), 0, st, (const float*)scratch, dlin, n, nch);
    return uvit_check_launch();
}
