// Shared helpers of the probe translation units (probe, calib, setcalib, stability, gp, het, ens, detect, tscale, conformal, laplace, maha, knn, vim, mcd, layerweights, corrupt, corrupt_ext, dprobe, mixup, randaug),
// on top of common.h.  These files are built WITHOUT -ffast-math: each states in its own header which IEEE property it relies on and
// refuses to compile under __FAST_MATH__.  Nothing here reorders a sum: a wave sum is the xor tree from distance 32 down to 1.
#pragma once
#include "common.h"

// ---- wave (64 lanes) reductions beside common.h's float pair; every lane gets the result ----
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {                // the two words travel as two 32-bit shuffles
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int lo = __shfl_xor((int)(v & 0xFFFFFFFFll), o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
        v += (long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned long long)(unsigned int)lo);
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// (value, index) arg max over the wave, in place: the larger value wins, the lower index among equal values.  A lane without a
// candidate holds -inf and the largest index.  A macro and not a function: as an inlined function the same tree came out of the
// compiler with other registers and another schedule in three of its four kernels.
#define WAVE_ARGMAX(best, bi)                                                         \
    _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) {                           \
        const float ov_ = __shfl_xor(best, o_, 64);                                   \
        const int oi_ = __shfl_xor(bi, o_, 64);                                       \
        if (ov_ > best || (ov_ == best && oi_ < bi)) { best = ov_; bi = oi_; }        \
    }

// ---- small predicates ----
#define QUIET_NAN_BITS 0x7FF8000000000000ULL
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double((long long)QUIET_NAN_BITS); }
__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < INFINITY; }      // false for NaN and for +-inf
__device__ __forceinline__ bool label_ok(int64_t y, int K) { return y >= 0 && y < (int64_t)K; }

// ---- sort keys: the image of an fp32 value as an unsigned word whose unsigned order is the numeric order of the value (-0 below +0;
// a caller that wants the zeros equal folds them first), and its inverse ----
__device__ __forceinline__ unsigned int key32(float v) {
    const unsigned int u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key32_value(unsigned int u) { return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
__device__ __forceinline__ float fold_zero(float v) { return v == 0.f ? 0.f : v; }     // -0 -> +0

// ---- bitonic network on 64-bit keys: pair q of the step at distance j is (i, i | j), i = q with a zero inserted at bit log2(j);
// the loops, the key layout and the direction of a step belong to the kernel.  BITONIC_LO and BITONIC_CMPX_AT are macros for the
// reason given at WAVE_ARGMAX; cmpx() serves keys that are already in registers. ----
#define BITONIC_LO(q, j) ((((q) & ~((j) - 1)) << 1) | ((q) & ((j) - 1)))
#define BITONIC_CMPX_AT(keys, i, l, asc)                                              \
    {                                                                                 \
        const unsigned long long a_ = (keys)[i], b_ = (keys)[l];                      \
        if ((a_ > b_) == (asc)) { (keys)[i] = b_; (keys)[l] = a_; }                   \
    }
__device__ __forceinline__ void cmpx(unsigned long long& a, unsigned long long& b, bool asc) {
    if ((a > b) == asc) { const unsigned long long t = a; a = b; b = t; }
}

// ---- the corruption ops' key of image `index` of a set (corrupt.hip, corrupt_ext.hip): kseed carries the set's seed and the kind ----
__host__ __device__ __forceinline__ uint32_t corrupt_image_key(uint32_t kseed, uint32_t index) {
    return uvit_hash32(kseed ^ ((index + 1u) * 0x85EBCA6Bu));
}

// ---- one wave per row: workgroups of four waves, wave w of workgroup g owns row 4 g + w ----
struct WavePerRow {
    static __device__ __forceinline__ int lane() { return threadIdx.x & 63; }
    static __device__ __forceinline__ int row() { return blockIdx.x * 4 + (threadIdx.x >> 6); }
    static inline dim3 grid(int rows) { return dim3((rows + 3) / 4); }
    static inline dim3 block() { return dim3(256); }
};

// ---- launcher checks ----
static inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
template <class T> static inline T align16(T n) { return (n + 15) & ~(T)15; }
