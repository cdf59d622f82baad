// Row-wise device helpers shared by norm.hip and elementwise.hip (gfx950): one wave per row, lane l owns the float4 column groups
// l, l + 64, ... of the row; NV = groups per lane actually needed (ceil(C / 256)) is a template parameter, so register use and hence
// occupancy follow the real row length (NV = 3 for C = 768) instead of the maximum.
#pragma once
#include <type_traits>
#include "common.h"

#define ROW_MAXV 8          // float4 per lane: C <= 2048

// The one NV ladder: f(std::integral_constant<int, NV>) for the smallest instantiated NV that holds a row of C columns.  Further template
// arguments (LS, the walk, the wave count) are the caller's; the argument list of the launch is written once, inside f.
template <class F>
static inline void dispatch_nv(int C, F&& f) {
    const int nv = (C + 255) / 256;
    if (nv <= 1) f(std::integral_constant<int, 1>{}); else if (nv == 2) f(std::integral_constant<int, 2>{});
    else if (nv == 3) f(std::integral_constant<int, 3>{}); else if (nv == 4) f(std::integral_constant<int, 4>{});
    else if (nv == 5) f(std::integral_constant<int, 5>{}); else f(std::integral_constant<int, ROW_MAXV>{});
}

template <int NV> struct RowVec { float4 v[NV]; };

template <int NV>
__device__ __forceinline__ void load_row(RowVec<NV>& r, const float* x, int C, int lane) {
    const int nv = C >> 2;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = lane + 64 * k;
        r.v[k] = i < nv ? ((const float4*)x)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

template <int NV>
__device__ __forceinline__ void row_stats(const RowVec<NV>& r, int C, int lane, float eps, float& mean, float& rstd) {
    const int nv = C >> 2;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) s += r.v[k].x + r.v[k].y + r.v[k].z + r.v[k].w;
    mean = wave_sum(s) / C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        if (lane + 64 * k < nv) {
            const float a = r.v[k].x - mean, b = r.v[k].y - mean, c = r.v[k].z - mean, d = r.v[k].w - mean;
            q += a * a + b * b + c * c + d * d;
        }
    }
    rstd = rsqrtf(wave_sum(q) / C + eps);
}

__device__ __forceinline__ float4 normalize4(const float4& v, float mean, float rstd) {
    return make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd);
}

// y = (x - mean) * rstd * w + b  ->  bf16
template <int NV>
__device__ __forceinline__ void normalize_store(const RowVec<NV>& r, float mean, float rstd, const float* w, const float* b, bf16* y,
                                                int nv, int lane) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = lane + 64 * k;
        if (i < nv) {
            const float4 h = normalize4(r.v[k], mean, rstd), ww = ((const float4*)w)[i], bb = ((const float4*)b)[i];
            ((bf16x4*)y)[i] = bf16x4{f2bf(h.x * ww.x + bb.x), f2bf(h.y * ww.y + bb.y), f2bf(h.z * ww.z + bb.z), f2bf(h.w * ww.w + bb.w)};
        }
    }
}
// no affine: dst (+)= (x - mean) * rstd  (fp32)
template <int NV>
__device__ __forceinline__ void normalize_store(const RowVec<NV>& r, float mean, float rstd, float* dst, bool accumulate, int nv, int lane) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = lane + 64 * k;
        if (i < nv) {
            float4 o = normalize4(r.v[k], mean, rstd);
            if (accumulate) { const float4 a = ((const float4*)dst)[i]; o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w; }
            ((float4*)dst)[i] = o;
        }
    }
}

__device__ __forceinline__ bf16x4 bf16x4_zero() { return bf16x4{f2bf(0.f), f2bf(0.f), f2bf(0.f), f2bf(0.f)}; }

// one bf16 row of C = 4 nv columns <- 0 (pad rows of compact buffers)
template <int NV>
__device__ __forceinline__ void store_zero_row(bf16* y, int nv, int lane) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (lane + 64 * k < nv) ((bf16x4*)y)[lane + 64 * k] = bf16x4_zero();
}

// LayerScale + DropPath backward of four columns of one row (modeling_finetune.py:295-298): with e = d * dp,
//   *dy = bf16(e * gamma),  dgamma partial ag += e * y,  dbias partial ab += dy (the stored bf16, re-read)
__device__ __forceinline__ void ls_apply(const float4& d, float dp, const bf16x4& y, const float4& gamma, bf16x4* dy, float4& ag, float4& ab) {
    const float e0 = d.x * dp, e1 = d.y * dp, e2 = d.z * dp, e3 = d.w * dp;
    ag.x += e0 * bf2f(y[0]); ag.y += e1 * bf2f(y[1]); ag.z += e2 * bf2f(y[2]); ag.w += e3 * bf2f(y[3]);
    const bf16x4 o = {f2bf(e0 * gamma.x), f2bf(e1 * gamma.y), f2bf(e2 * gamma.z), f2bf(e3 * gamma.w)};
    *dy = o;
    ab.x += bf2f(o[0]); ab.y += bf2f(o[1]); ab.z += bf2f(o[2]); ab.w += bf2f(o[3]);
}
// the same without the branch output: dy and the dbias partial only (dgamma then comes from the weight gradient, ls_dgamma_kernel)
__device__ __forceinline__ void ls_apply(const float4& d, float dp, const float4& gamma, bf16x4* dy, float4& ab) {
    const float e0 = d.x * dp, e1 = d.y * dp, e2 = d.z * dp, e3 = d.w * dp;
    const bf16x4 o = {f2bf(e0 * gamma.x), f2bf(e1 * gamma.y), f2bf(e2 * gamma.z), f2bf(e3 * gamma.w)};
    *dy = o;
    ab.x += bf2f(o[0]); ab.y += bf2f(o[1]); ab.z += bf2f(o[2]); ab.w += bf2f(o[3]);
}
