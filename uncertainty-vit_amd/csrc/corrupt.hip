// ImageNet-C-style corruptions of a batch of clean uint8 images on gfx950 (include/uvit.h, uvit_op_corrupt_*; DESIGN.md section 9.16;
// numpy restatement: tests/corrupt_ref.py).  The clean evaluation images stay on the device as planar uint8 (uvit_op_corrupt_pack,
// the inverse of the augmentation's ToTensor + Normalize) and every (corruption, severity) set is one launch sequence per batch in
// front of the encoder forward:
//   gaussian_noise, speckle_noise, impulse_noise, shot_noise, brightness, saturate    one pointwise launch
//   contrast                                                                         plane means (exact integer sums), one pointwise launch
//   gaussian_blur                                                                    vertical pass into the workspace, horizontal pass
//   defocus_blur                                                                     one dense (2R+1)^2 pass
// The working value is v = float(u8) / 255.0f, every kind ends with q = floor(clip(v', 0, 1) * 255 + 0.5) and writes
// ((q / 255) - mean[c]) / std[c], the augmentation's formula.
// This file relies on IEEE fp32 + - * / WITHOUT contraction (build.sh: no -ffast-math, -ffp-contract=off): every expression below is
// evaluated operation by operation as it is written, so a float32 numpy restatement reproduces its bytes.  Only logf, cosf and sqrtf of
// the Box-Muller draw (gaussian_noise, speckle_noise) are not reproducible off the device; DESIGN.md bounds their effect.
// No float atomics, no atomics at all: every output value has one owner, and a convolution adds its taps in row-major order into ONE
// accumulator, acc = acc + (t * x).  The noise is counter-based on common.h's hash: the key of an image comes from the seed, the kind
// and the image's index in the SET, the counter is the value's index inside the image, so a set has the same bytes for every batch
// size and every split.
#ifdef __FAST_MATH__
#error "corrupt.hip relies on IEEE fp32 arithmetic evaluated as written: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE = 32;               // a convolution workgroup owns TILE x TILE outputs, four per thread
constexpr int MAX_RADIUS = 24;         // gaussian_blur at sigma 6
constexpr int MAX_BATCH = 21845;       // 3 B planes in gridDim.z
constexpr int SHOT_LEVELS = 256;       // params of shot_noise: c, p0[256], kmax[256]
constexpr float SHOT_KMAX_CAP = 512.f; // the inversion loop ends whatever the table holds

struct Norm { float m[3], s[3]; };

__device__ __forceinline__ float quantise(float v) { return floorf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); }
__device__ __forceinline__ float normalise(float q, float m, float s) { return (q / 255.0f - m) / s; }

// ---- counter-based draws ----
__device__ __forceinline__ uint32_t draw_key1(uint32_t ikey) { return uvit_hash32(ikey ^ 0x1B873593u); }
__device__ __forceinline__ uint32_t draw_key2(uint32_t ikey) { return uvit_hash32(ikey ^ 0xCC9E2D51u); }
__device__ __forceinline__ float uniform_open(uint32_t h) { return (float)((h >> 8) + 1u) * 5.9604644775390625e-08f; }    // (0, 1], exact
__device__ __forceinline__ float uniform_half(uint32_t h) { return (float)(h >> 8) * 5.9604644775390625e-08f; }           // [0, 1), exact
__device__ __forceinline__ float box_muller(uint32_t h1, uint32_t h2) {
    return sqrtf(-2.0f * logf(uniform_open(h1))) * cosf(6.2831854820251465f * uniform_half(h2));
}

// k ~ Poisson(lambda) by inversion of the fp32 CDF: p0 = exp(-lambda) and kmax come from the host's table
__device__ __forceinline__ float poisson(float u, float lambda, float p0, float kmax) {
    float k = 0.0f, p = p0, F = p0;
    while (u > F && k < kmax) {
        k = k + 1.0f;
        p = (p * lambda) / k;
        F = F + p;
    }
    return k;
}

// ---- the pointwise kinds: one thread owns VEC neighbouring pixels of one image, all three channels ----
template <int KIND>
__device__ __forceinline__ void corrupt_pixel(const float v[3], float r[3], uint32_t ctr, uint32_t plane, uint32_t k1, uint32_t k2,
                                              const float* __restrict__ params, const float* __restrict__ mu, const uint8_t u[3]) {
    if (KIND == UVIT_CORRUPT_GAUSSIAN_NOISE || KIND == UVIT_CORRUPT_SPECKLE_NOISE) {
        const float c = params[0];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t i = ctr + (uint32_t)ch * plane;
            const float z = box_muller(uvit_hash32(i ^ k1), uvit_hash32(i ^ k2));
            r[ch] = KIND == UVIT_CORRUPT_GAUSSIAN_NOISE ? v[ch] + c * z : v[ch] + (v[ch] * c) * z;
        }
    } else if (KIND == UVIT_CORRUPT_IMPULSE_NOISE) {
        const uint32_t thr = uvit_drop_threshold(params[0]), half = thr >> 1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t h = uvit_hash32((ctr + (uint32_t)ch * plane) ^ k1);
            r[ch] = h < half ? 1.0f : h < thr ? 0.0f : v[ch];
        }
    } else if (KIND == UVIT_CORRUPT_SHOT_NOISE) {
        const float c = params[0];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float uu = uniform_open(uvit_hash32((ctr + (uint32_t)ch * plane) ^ k1));
            const float k = poisson(uu, v[ch] * c, params[1 + u[ch]], fminf(params[1 + SHOT_LEVELS + u[ch]], SHOT_KMAX_CAP));
            r[ch] = fminf(k / c, 1.0f);
        }
    } else if (KIND == UVIT_CORRUPT_BRIGHTNESS) {
        const float m = fmaxf(fmaxf(v[0], v[1]), v[2]), m2 = fminf(m + params[0], 1.0f);
        if (m == 0.0f) {
            r[0] = r[1] = r[2] = m2;
        } else {
            const float ratio = m2 / m;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) r[ch] = v[ch] * ratio;
        }
    } else if (KIND == UVIT_CORRUPT_SATURATE) {
        const float m = fmaxf(fmaxf(v[0], v[1]), v[2]), mn = fminf(fminf(v[0], v[1]), v[2]);
        const float s = m == 0.0f ? 0.0f : (m - mn) / m;
        const float s2 = fminf(fmaxf(s * params[0] + params[1], 0.0f), 1.0f);
        if (s > 0.0f) {
            const float ratio = s2 / s;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) r[ch] = m - (m - v[ch]) * ratio;
        } else {                                        // grey: hue 0
            r[0] = m;
            r[1] = r[2] = m * (1.0f - s2);
        }
    } else {                                            // UVIT_CORRUPT_CONTRAST
        const float c = params[0];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) r[ch] = (v[ch] - mu[ch]) * c + mu[ch];
    }
}

template <int KIND, int VEC>
__global__ __launch_bounds__(THREADS)
void corrupt_point_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int S, const float* __restrict__ params,
                          const float* __restrict__ mu, uint32_t kseed, uint32_t index0, Norm nm) {
    const uint32_t plane = (uint32_t)S * (uint32_t)S;
    const uint32_t p0 = (blockIdx.x * THREADS + threadIdx.x) * VEC;
    if (p0 >= plane) return;
    const int b = blockIdx.y;
    const uint8_t* src = in + (size_t)b * 3 * plane + p0;
    float* dst = out + (size_t)b * 3 * plane + p0;
    const uint32_t ikey = corrupt_image_key(kseed, index0 + (uint32_t)b),k1 = draw_key1(ikey), k2 = draw_key2(ikey);
    uint8_t u[3][VEC];
    float res[3][VEC];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (VEC == 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(src + (size_t)ch * plane);
#pragma unroll
            for (int j = 0; j < VEC; ++j) u[ch][j] = (uint8_t)(w >> (8 * j));
        } else {
            u[ch][0] = src[(size_t)ch * plane];
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const uint8_t uj[3] = {u[0][j], u[1][j], u[2][j]};
        const float v[3] = {(float)uj[0] / 255.0f, (float)uj[1] / 255.0f, (float)uj[2] / 255.0f};
        float r[3];
        corrupt_pixel<KIND>(v, r, p0 + j, plane, k1, k2, params, mu ? mu + b * 3 : nullptr, uj);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) res[ch][j] = normalise(quantise(r[ch]), nm.m[ch], nm.s[ch]);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (VEC == 4) {
            *reinterpret_cast<float4*>(dst + (size_t)ch * plane) = make_float4(res[ch][0], res[ch][1], res[ch][2], res[ch][3]);
        } else {
            dst[(size_t)ch * plane] = res[ch][0];
        }
    }
}

// mu[b * 3 + c] = float(sum / (255.0 S S)) of plane (b, c): an exact integer sum (at most 255 * 2^20), the division in double
__global__ __launch_bounds__(THREADS)
void corrupt_plane_mean_kernel(const uint8_t* __restrict__ in, float* __restrict__ mu, int S) {
    const int plane = S * S;
    const uint8_t* p = in + (size_t)blockIdx.x * plane;
    int s = 0;
    for (int i = threadIdx.x; i < plane; i += THREADS) s += p[i];
    s = wave_sum(s);
    __shared__ int part[THREADS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < THREADS / 64; ++w) total += part[w];
        mu[blockIdx.x] = (float)((double)total / (255.0 * (double)S * (double)S));
    }
}

// ---- the convolution: one body for the dense kernel and both separable passes ----
// A workgroup stages the (TILE + kh - 1) x (TILE + kw - 1) inputs of its TILE x TILE outputs in LDS (the border resolved while
// loading); thread (tx, ty) owns the outputs (ty + 8 i, tx), i = 0 .. 3: four independent chains, each ONE accumulator that takes its
// taps dy ascending, then dx ascending.  The taps are read through a wave-uniform pointer; a zero tap adds an exact 0 and is skipped.
__device__ __forceinline__ int border_index(int i, int S, int reflect) {
    if (reflect) i = i < 0 ? -i : i >= S ? 2 * (S - 1) - i : i;      // reflect-101; one fold is enough for a radius < S
    return min(max(i, 0), S - 1);                                    // replicate (and the in-bounds guard of outputs outside the image)
}

template <bool IN_U8, bool FINAL>
__global__ __launch_bounds__(THREADS)
void corrupt_conv_kernel(const void* __restrict__ in, float* __restrict__ out, int S, const float* __restrict__ taps, int kh, int kw,
                         int reflect, Norm nm) {
    extern __shared__ float tile[];
    const int ry = kh >> 1, rx = kw >> 1, tw = TILE + 2 * rx, th = TILE + 2 * ry;
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    const size_t base = (size_t)blockIdx.z * S * S;
    for (int i = threadIdx.x; i < th * tw; i += THREADS) {
        const int ly = i / tw, lx = i - ly * tw;
        const size_t g = base + (size_t)border_index(y0 + ly - ry, S, reflect) * S + border_index(x0 + lx - rx, S, reflect);
        tile[i] = IN_U8 ? (float)static_cast<const uint8_t*>(in)[g] / 255.0f : static_cast<const float*>(in)[g];
    }
    __syncthreads();
    const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x / TILE;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int dy = 0; dy < kh; ++dy) {
        const float* row = tile + (ty + dy) * tw + tx;
        for (int dx = 0; dx < kw; ++dx) {
            const float t = taps[dy * kw + dx];
            if (t == 0.0f) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = acc[i] + t * row[i * 8 * tw + dx];
        }
    }
    const int ch = blockIdx.z % 3, x = x0 + tx;
    if (x >= S) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = y0 + ty + 8 * i;
        if (y < S) out[base + (size_t)y * S + x] = FINAL ? normalise(quantise(acc[i]), nm.m[ch], nm.s[ch]) : acc[i];
    }
}

// (B, 3, S, S) fp32 normalised -> planar uint8: q = floor(clip(x * std + mean, 0, 1) * 255 + 0.5)
template <int VEC>
__global__ __launch_bounds__(THREADS)
void corrupt_pack_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int64_t n, int64_t plane, Norm nm) {
    const int64_t i = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * VEC;
    if (i >= n) return;
    const int ch = (int)((i / plane) % 3);
    if (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4*>(x + i);
        const uint32_t q0 = (uint32_t)quantise(v.x * nm.s[ch] + nm.m[ch]), q1 = (uint32_t)quantise(v.y * nm.s[ch] + nm.m[ch]),
                       q2 = (uint32_t)quantise(v.z * nm.s[ch] + nm.m[ch]), q3 = (uint32_t)quantise(v.w * nm.s[ch] + nm.m[ch]);
        *reinterpret_cast<uint32_t*>(out + i) = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
    } else {
        out[i] = (uint8_t)quantise(x[i] * nm.s[ch] + nm.m[ch]);
    }
}

// ---- host side: validation and launches ----
inline bool bad_kind(int kind) { return kind < 0 || kind >= UVIT_CORRUPT_KINDS; }
inline int check_shape(int B, int S) { return (B < 1 || B > MAX_BATCH || S < 8 || S > 1024) ? UVIT_ERR_SHAPE : UVIT_OK; }
inline bool make_norm(const float* mean, const float* stdv, Norm* nm) {
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(mean[c]) || !std::isfinite(stdv[c]) || stdv[c] == 0.0f) return false;
        nm->m[c] = mean[c];
        nm->s[c] = stdv[c];
    }
    return true;
}
inline int64_t ws_need(int kind, int B, int S) {
    if (kind == UVIT_CORRUPT_CONTRAST) return (int64_t)align16((size_t)B * 3 * sizeof(float));
    if (kind == UVIT_CORRUPT_GAUSSIAN_BLUR) return (int64_t)B * 3 * S * S * (int64_t)sizeof(float);
    return 0;
}
// The radius a blur's tap count stands for, or -1: 2 R + 1 taps (gaussian_blur), (2 R + 1)^2 taps (defocus_blur).
inline int blur_radius(int kind, int n_params) {
    if (n_params < 1) return -1;
    int side = n_params;
    if (kind == UVIT_CORRUPT_DEFOCUS_BLUR) {
        side = (int)lround(sqrt((double)n_params));
        if (side * side != n_params) return -1;
    }
    return (side & 1) ? side >> 1 : -1;
}
inline int param_count(int kind) {          // of the kinds whose table has a fixed length
    switch (kind) {
        case UVIT_CORRUPT_SATURATE: return 2;
        case UVIT_CORRUPT_SHOT_NOISE: return 1 + 2 * SHOT_LEVELS;
        default: return 1;
    }
}

template <int KIND>
void launch_point(bool vec, dim3 grid1, dim3 grid4, hipStream_t s, const uint8_t* in, float* out, int S, const float* params, const float* mu,
                  uint32_t kseed, uint32_t index0, const Norm& nm) {
    if (vec) hipLaunchKernelGGL((corrupt_point_kernel<KIND, 4>), grid4, dim3(THREADS), 0, s, in, out, S, params, mu, kseed, index0, nm);
    else hipLaunchKernelGGL((corrupt_point_kernel<KIND, 1>), grid1, dim3(THREADS), 0, s, in, out, S, params, mu, kseed, index0, nm);
}

}  // namespace

extern "C" int uvit_op_corrupt_pack(const float* x, int B, int S, const float* mean, const float* stdv, uint8_t* out_u8, uvit_stream stream) {
    if (!x || !mean || !stdv || !out_u8) return UVIT_ERR_ARG;
    Norm nm;
    if (!make_norm(mean, stdv, &nm)) return UVIT_ERR_ARG;
    if (check_shape(B, S)) return UVIT_ERR_SHAPE;
    const int64_t plane = (int64_t)S * S, n = (int64_t)B * 3 * plane;
    if (plane % 4 == 0 && !misaligned(x, 16) && !misaligned(out_u8, 4)) {
        const int64_t blocks = (n / 4 + THREADS - 1) / THREADS;
        hipLaunchKernelGGL(corrupt_pack_kernel<4>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, x, out_u8, n, plane, nm);
    } else {
        const int64_t blocks = (n + THREADS - 1) / THREADS;
        hipLaunchKernelGGL(corrupt_pack_kernel<1>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, x, out_u8, n, plane, nm);
    }
    return uvit_check_launch();
}

extern "C" int64_t uvit_op_corrupt_ws_bytes(int kind, int B, int S) {
    if (bad_kind(kind)) return UVIT_ERR_ARG;
    if (check_shape(B, S)) return UVIT_ERR_SHAPE;
    return ws_need(kind, B, S);
}

extern "C" int uvit_op_corrupt_batch(const uint8_t* in_u8, float* out, int B, int S, int kind, const float* params, int n_params,
                                     uint32_t seed, int64_t index0, const float* mean, const float* stdv, void* ws, int64_t ws_bytes,
                                     uvit_stream stream) {
    if (!in_u8 || !out || !params || !mean || !stdv || bad_kind(kind)) return UVIT_ERR_ARG;
    Norm nm;
    if (!make_norm(mean, stdv, &nm)) return UVIT_ERR_ARG;
    if (index0 < 0 || index0 > (int64_t)0xFFFFFFFFll - MAX_BATCH) return UVIT_ERR_ARG;
    if (check_shape(B, S)) return UVIT_ERR_SHAPE;
    const bool blur = kind == UVIT_CORRUPT_GAUSSIAN_BLUR || kind == UVIT_CORRUPT_DEFOCUS_BLUR;
    int R = 0;
    if (blur) {
        R = blur_radius(kind, n_params);
        if (R < 0) return UVIT_ERR_ARG;
        if (R >= S || R > MAX_RADIUS) return UVIT_ERR_SHAPE;
    } else if (n_params != param_count(kind)) {
        return UVIT_ERR_ARG;
    }
    const int64_t need = ws_need(kind, B, S);
    if (need > 0 && !ws) return UVIT_ERR_ARG;
    if (ws_bytes < need) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (blur) {
        const dim3 grid((S + TILE - 1) / TILE, (S + TILE - 1) / TILE, 3 * B);
        const int side = 2 * R + 1;
        const size_t lds_sep = (size_t)(TILE + 2 * R) * TILE * sizeof(float), lds_dense = (size_t)(TILE + 2 * R) * (TILE + 2 * R) * sizeof(float);
        if (kind == UVIT_CORRUPT_GAUSSIAN_BLUR) {
            float* mid = (float*)ws;
            hipLaunchKernelGGL((corrupt_conv_kernel<true, false>), grid, dim3(THREADS), lds_sep, s, (const void*)in_u8, mid, S, params, side, 1, 0, nm);
            hipLaunchKernelGGL((corrupt_conv_kernel<false, true>), grid, dim3(THREADS), lds_sep, s, (const void*)mid, out, S, params, 1, side, 0, nm);
        } else {
            hipLaunchKernelGGL((corrupt_conv_kernel<true, true>), grid, dim3(THREADS), lds_dense, s, (const void*)in_u8, out, S, params, side, side, 1, nm);
        }
        return uvit_check_launch();
    }
    // the key of the set and the kind; the image's index joins it on the device
    const uint32_t kseed = uvit_hash32(seed ^ ((uint32_t)(kind + 1) * 0x9E3779B9u)), i0 = (uint32_t)index0;
    const int plane = S * S;
    const bool vec = plane % 4 == 0 && !misaligned(in_u8, 4) && !misaligned(out, 16);
    const dim3 grid1((plane + THREADS - 1) / THREADS, B), grid4((plane / 4 + THREADS - 1) / THREADS, B);
    float* mu = nullptr;
    if (kind == UVIT_CORRUPT_CONTRAST) {
        mu = (float*)ws;
        hipLaunchKernelGGL(corrupt_plane_mean_kernel, dim3(3 * B), dim3(THREADS), 0, s, in_u8, mu, S);
    }
    switch (kind) {
        case UVIT_CORRUPT_GAUSSIAN_NOISE: launch_point<UVIT_CORRUPT_GAUSSIAN_NOISE>(vec, grid1, grid4, s, in_u8, out, S, params, mu, kseed, i0, nm); break;
        case UVIT_CORRUPT_SPECKLE_NOISE: launch_point<UVIT_CORRUPT_SPECKLE_NOISE>(vec, grid1, grid4, s, in_u8, out, S, params, mu, kseed, i0, nm); break;
        case UVIT_CORRUPT_IMPULSE_NOISE: launch_point<UVIT_CORRUPT_IMPULSE_NOISE>(vec, grid1, grid4, s, in_u8, out, S, params, mu, kseed, i0, nm); break;
        case UVIT_CORRUPT_SHOT_NOISE: launch_point<UVIT_CORRUPT_SHOT_NOISE>(vec, grid1, grid4, s, in_u8, out, S, params, mu, kseed, i0, nm); break;
        case UVIT_CORRUPT_BRIGHTNESS: launch_point<UVIT_CORRUPT_BRIGHTNESS>(vec, grid1, grid4, s, in_u8, out, S, params, mu, kseed, i0, nm); break;
        case UVIT_CORRUPT_SATURATE: launch_point<UVIT_CORRUPT_SATURATE>(vec, grid1, grid4, s, in_u8, out, S, params, mu, kseed, i0, nm); break;
        default: launch_point<UVIT_CORRUPT_CONTRAST>(vec, grid1, grid4, s, in_u8, out, S, params, mu, kseed, i0, nm); break;
    }
    return uvit_check_launch();
}
