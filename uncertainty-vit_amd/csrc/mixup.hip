// Training-time mixing of a batch of normalised images on gfx950 and the soft-target cross-entropy that goes with it (include/uvit.h,
// uvit_op_mix_batch / uvit_op_probe_ce_mix; numpy restatement: tests/mix_ref.py).
//   uvit_op_mix_batch      random erasing, then mixup / cutmix with a partner row, one launch: out[b] from e(b) and e(partner(b)),
//                          e(j) = sample j behind its erase boxes.  Every output value has one owner; a thread owns VEC neighbouring
//                          pixels of one image row, all three channels, and reads the partner only where the row's kind needs it.
//   uvit_op_probe_ce_mix   the cross-entropy of the two-label target lam oh(y_b) + (1 - lam) oh(y_partner(b)), one wave per row with
//                          probe_ce_kernel's sums, and the mean over rows by one wave in row order.
// This file relies on IEEE fp32 + - * / WITHOUT contraction (build.sh: no -ffast-math, -ffp-contract=off): lam * e(b) + (1 - lam) * e(p)
// is two products and one sum, each rounded, so a float32 numpy restatement reproduces its bytes.  Only logf, cosf and sqrtf of the
// Box-Muller fill of an erased pixel are not reproducible off the device; tests/mix_ref.py bounds their effect.
// No atomics.  The fill is counter-based on common.h's hash: the key of a sample comes from the seed, the iteration and the sample's
// index in the batch, the counter from the box and the channel (rand) or from the pixel (pixel), so an erased pixel of sample j has one
// value wherever j appears, for every batch size and every launch shape.
#ifdef __FAST_MATH__
#error "mixup.hip relies on IEEE fp32 arithmetic evaluated as written: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BATCH = 65535;       // B rows in gridDim.y
constexpr int MAX_SIZE = 4096;         // 3 S S < 2^26: the pixel counter fits a word with room to spare
constexpr int MAX_BOXES = UVIT_MIX_MAX_BOXES;

// ---- the fill of an erased pixel ----
__host__ __device__ __forceinline__ uint32_t mix_iter_key(uint32_t seed, uint32_t iteration) {
    return uvit_hash32(seed ^ (iteration * 0x9E3779B9u + 0x7F4A7C15u));
}
__device__ __forceinline__ uint32_t mix_sample_key(uint32_t kit, uint32_t j) { return uvit_hash32(kit ^ ((j + 1u) * 0x85EBCA6Bu)); }
// (h >> 9) < 2^23, so (h >> 9) + 0.5 has 24 significant bits and the product with 2^-23 is exact: u in (0, 1)
__device__ __forceinline__ float mix_uniform(uint32_t h) { return ((float)(h >> 9) + 0.5f) * 0x1p-23f; }
__device__ __forceinline__ float mix_normal(uint32_t kj, uint32_t q) {
    const uint32_t k1 = uvit_hash32(kj ^ 0x1B873593u), k2 = uvit_hash32(kj ^ 0xCC9E2D51u);
    const float u1 = mix_uniform(uvit_hash32(q ^ k1)), u2 = mix_uniform(uvit_hash32(q ^ k2));
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831854820251465f * u2);
}

// Nibble i of the result = 1 + the last box of sample j that holds pixel (y, x0 + i) (a later box overwrites an earlier one), 0: none.
// One word and not an array: indexed by the pixel loop, an array went to scratch memory.
template <int VEC>
__device__ __forceinline__ uint32_t covering(const uvit_mix_box* __restrict__ boxes, int R, int j, int y, int x0) {
    uint32_t hits = 0;
    for (int r = 0; r < R; ++r) {
        const uvit_mix_box bx = boxes[(size_t)j * R + r];
        if (bx.h > 0 && y >= bx.top && y < bx.top + bx.h) {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (x0 + i >= bx.left && x0 + i < bx.left + bx.w) hits = (hits & ~(15u << (4 * i))) | ((uint32_t)(r + 1) << (4 * i));
        }
    }
    return hits;
}
__device__ __forceinline__ float fill_value(int mode, uint32_t kj, int box, int c, int y, int x, int S) {
    if (mode == UVIT_MIX_ERASE_CONST) return 0.0f;
    const uint32_t q = mode == UVIT_MIX_ERASE_RAND ? (uint32_t)(box * 3 + c) : ((uint32_t)c * (uint32_t)S + (uint32_t)y) * (uint32_t)S + (uint32_t)x;
    return mix_normal(kj, q);
}

template <int VEC>
__global__ __launch_bounds__(THREADS)
void mix_batch_kernel(const float* __restrict__ x, float* __restrict__ out, const uvit_mix_desc* __restrict__ desc,
                      const uvit_mix_box* __restrict__ boxes, int S, int R, int mode, uint32_t kit) {
    const uint32_t plane = (uint32_t)S * (uint32_t)S;
    const uint32_t p0 = (blockIdx.x * THREADS + threadIdx.x) * VEC;
    if (p0 >= plane) return;
    const int b = blockIdx.y;
    const int y = (int)(p0 / (uint32_t)S), x0 = (int)(p0 - (uint32_t)y * (uint32_t)S);      // VEC == 4: S % 4 == 0, the pixels share a row
    const uvit_mix_desc d = desc[b];
    const int p = d.partner;
    const bool in_rows = d.kind == UVIT_MIX_CUTMIX && y >= d.yl && y < d.yh;
    uint32_t par_mask = 0;                                 // bit j: pixel j reads the partner
    bool any_own = false;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const bool inbox = in_rows && x0 + j >= d.xl && x0 + j < d.xh;
        if (d.kind == UVIT_MIX_MIXUP || inbox) par_mask |= 1u << j;
        any_own |= d.kind != UVIT_MIX_CUTMIX || !inbox;
    }
    const bool any_par = par_mask != 0;
    const uint32_t ho = covering<VEC>(boxes, any_own ? R : 0, b, y, x0), hp = covering<VEC>(boxes, any_par ? R : 0, p, y, x0);
    const uint32_t ko = mix_sample_key(kit, (uint32_t)b), kp = mix_sample_key(kit, (uint32_t)p);
    const float lam = d.lam, oml = 1.0f - d.lam;
    const float* so = x + (size_t)b * 3 * plane + p0;
    const float* sp = x + (size_t)p * 3 * plane + p0;
    float* dst = out + (size_t)b * 3 * plane + p0;
    // pixel j of channel c from its own value and its partner's; called with constant j (a loop over an array of four went to scratch)
    auto pixel = [&](int c, int j, float eo, float ep) -> float {
        const int xx = x0 + j;
        const bool use_par = (par_mask >> j) & 1u, own = d.kind != UVIT_MIX_CUTMIX || !use_par;
        const int bo = (int)((ho >> (4 * j)) & 15u) - 1, bp = (int)((hp >> (4 * j)) & 15u) - 1;
        if (own && bo >= 0) eo = fill_value(mode, ko, bo, c, y, xx, S);
        if (use_par && bp >= 0) ep = fill_value(mode, kp, bp, c, y, xx, S);
        return d.kind == UVIT_MIX_MIXUP ? lam * eo + oml * ep : use_par ? ep : eo;
    };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (VEC == 4) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), q = a;      // a row that is not needed is not read
            if (any_own) a = *reinterpret_cast<const float4*>(so + (size_t)c * plane);
            if (any_par) q = *reinterpret_cast<const float4*>(sp + (size_t)c * plane);
            *reinterpret_cast<float4*>(dst + (size_t)c * plane) = make_float4(pixel(c, 0, a.x, q.x), pixel(c, 1, a.y, q.y), pixel(c, 2, a.z, q.z),
                                                                              pixel(c, 3, a.w, q.w));
        } else {
            dst[(size_t)c * plane] = pixel(c, 0, any_own ? so[(size_t)c * plane] : 0.f, any_par ? sp[(size_t)c * plane] : 0.f);
        }
    }
}

// ---- criterion of the two-label target: one wave per row, probe_ce_kernel's sums ----
// t = lam oh(ya) + (1 - lam) oh(yb), oh(y)_k = s / K + (1 - s) [k == y];  loss = lam L(ya) + (1 - lam) L(yb),
// L(y) = (1 - s) (lse - z_y) + s (lse - mean_k z_k);  dlogits = (softmax - t) / B.
// A label (own or partner's) outside [0, K), a partner outside [0, B) or a lam outside [0, 1]: the row's loss and gradient are NaN and
// nothing is read at the bad index.
__global__ __launch_bounds__(256)
void probe_ce_mix_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const int* __restrict__ partner,
                         const float* __restrict__ lam, float smoothing, float* __restrict__ dlogits, float* __restrict__ row_loss, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* z = logits + (size_t)b * K;
    const int p = partner[b];
    const bool p_ok = p >= 0 && p < B;
    const int64_t ya = labels[b], yb = p_ok ? labels[p] : (int64_t)-1;
    const float l = lam[b];
    const bool valid = p_ok && label_ok(ya, K) && label_ok(yb, K) && l >= 0.0f && l <= 1.0f;      // a NaN lam fails both comparisons
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, z[k]);
    m = wave_max(m);
    const float za = valid ? z[ya] : 0.f, zb = valid ? z[yb] : 0.f;
    float se = 0.f, sz = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        se += expf(v - m);
        sz += v;
    }
    se = wave_sum(se); sz = wave_sum(sz);
    const float lse = m + logf(se);
    const float nan = __uint_as_float(0x7FC00000u);
    const float oml = 1.0f - l;
    if (lane == 0) {
        const float uni = smoothing * (lse - sz / (float)K);
        const float La = (1.f - smoothing) * (lse - za) + uni, Lb = (1.f - smoothing) * (lse - zb) + uni;
        row_loss[b] = valid ? l * La + oml * Lb : nan;
    }
    if (dlogits) {
        const float invB = 1.0f / (float)B, uni = smoothing / (float)K;
        float* d = dlogits + (size_t)b * K;
        for (int k = lane; k < K; k += 64) {
            const float pk = expf(z[k] - lse);
            const float on = (k == (int)ya ? l : 0.f) + (k == (int)yb ? oml : 0.f);
            d[k] = valid ? (pk - (1.f - smoothing) * on - uni) * invB : nan;
        }
    }
}

// mean of row_loss: one wave walks the rows in order, 64 at a time (probe.hip's probe_loss_mean_kernel)
__global__ __launch_bounds__(64)
void mix_loss_mean_kernel(const float* __restrict__ row_loss, float* __restrict__ loss_out, int B) {
    float acc = 0.f;
    for (int b0 = 0; b0 < B; b0 += 64) acc += wave_sum(b0 + (int)threadIdx.x < B ? row_loss[b0 + threadIdx.x] : 0.f);
    if (threadIdx.x == 0) *loss_out = acc / (float)B;
}

// ---- host side ----
inline int check_shape(int B, int S, int R) {
    return (B < 1 || B > MAX_BATCH || S < 1 || S > MAX_SIZE || R < 0 || R > MAX_BOXES) ? UVIT_ERR_SHAPE : UVIT_OK;
}
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
inline size_t off_boxes(int B) { return align256((size_t)B * sizeof(uvit_mix_desc)); }
inline int64_t ws_need(int B, int R) { return (int64_t)(off_boxes(B) + align256((size_t)B * R * sizeof(uvit_mix_box))); }

}  // namespace

extern "C" int64_t uvit_op_mix_ws_bytes(int B, int R) {
    if (check_shape(B, 1, R)) return UVIT_ERR_SHAPE;
    return ws_need(B, R);
}

extern "C" int uvit_op_mix_batch(const float* x, float* out, const uvit_mix_desc* desc, const uvit_mix_box* boxes, int B, int S, int R,
                                 int erase_mode, uint32_t seed, uint32_t iteration, void* workspace, int64_t ws_bytes, uvit_stream stream) {
    if (!x || !out || !desc || !workspace) return UVIT_ERR_ARG;
    if (check_shape(B, S, R)) return UVIT_ERR_SHAPE;
    if (R > 0 && !boxes) return UVIT_ERR_ARG;
    if (erase_mode != UVIT_MIX_ERASE_CONST && erase_mode != UVIT_MIX_ERASE_RAND && erase_mode != UVIT_MIX_ERASE_PIXEL) return UVIT_ERR_ARG;
    if (misaligned(x, 4) || misaligned(out, 4)) return UVIT_ERR_ARG;
    const size_t plane = (size_t)S * S, bytes = (size_t)B * 3 * plane * sizeof(float);
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
    if (xa < oa + bytes && oa < xa + bytes) return UVIT_ERR_ARG;          // rows read their partners: no overlap at all
    for (int b = 0; b < B; ++b) {
        const uvit_mix_desc& d = desc[b];
        if (d.kind != UVIT_MIX_NONE && d.kind != UVIT_MIX_MIXUP && d.kind != UVIT_MIX_CUTMIX) return UVIT_ERR_ARG;
        if (!(d.lam >= 0.0f && d.lam <= 1.0f)) return UVIT_ERR_ARG;
        if (d.partner < 0 || d.partner >= B) return UVIT_ERR_ARG;
        if (d.yl < 0 || d.yl > d.yh || d.yh > S || d.xl < 0 || d.xl > d.xh || d.xh > S) return UVIT_ERR_SHAPE;
        for (int r = 0; r < R; ++r) {
            const uvit_mix_box& e = boxes[(size_t)b * R + r];
            if (e.h == 0) continue;
            if (e.h < 0 || e.w < 1 || e.top < 0 || e.left < 0 || e.h > S - e.top || e.w > S - e.left) return UVIT_ERR_SHAPE;
        }
    }
    if (ws_bytes < ws_need(B, R)) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uvit_mix_desc* ddesc = (uvit_mix_desc*)ws;
    uvit_mix_box* dboxes = (uvit_mix_box*)(ws + off_boxes(B));
    if (hipMemcpyAsync(ddesc, desc, (size_t)B * sizeof(uvit_mix_desc), hipMemcpyHostToDevice, s) != hipSuccess) return UVIT_ERR_LAUNCH;
    if (R > 0 && hipMemcpyAsync(dboxes, boxes, (size_t)B * R * sizeof(uvit_mix_box), hipMemcpyHostToDevice, s) != hipSuccess) return UVIT_ERR_LAUNCH;
    const uint32_t kit = mix_iter_key(seed, iteration);
    const bool vec = S % 4 == 0 && !misaligned(x, 16) && !misaligned(out, 16);
    if (vec) {
        const dim3 grid((unsigned)((plane / 4 + THREADS - 1) / THREADS), B);
        hipLaunchKernelGGL(mix_batch_kernel<4>, grid, dim3(THREADS), 0, s, x, out, (const uvit_mix_desc*)ddesc, (const uvit_mix_box*)dboxes, S, R, erase_mode, kit);
    } else {
        const dim3 grid((unsigned)((plane + THREADS - 1) / THREADS), B);
        hipLaunchKernelGGL(mix_batch_kernel<1>, grid, dim3(THREADS), 0, s, x, out, (const uvit_mix_desc*)ddesc, (const uvit_mix_box*)dboxes, S, R, erase_mode, kit);
    }
    return uvit_check_launch();
}

extern "C" int uvit_op_probe_ce_mix(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam, float smoothing,
                                    float* dlogits, float* row_loss, float* loss_out, int B, int K, uvit_stream stream) {
    if (!logits || !labels || !partner || !lam || !row_loss || !loss_out || !(smoothing >= 0.f && smoothing < 1.f)) return UVIT_ERR_ARG;
    if (B < 1 || K < 1) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(probe_ce_mix_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, logits, labels, (const int*)partner, lam, smoothing, dlogits,
                       row_loss, B, K);
    hipLaunchKernelGGL(mix_loss_mean_kernel, dim3(1), dim3(64), 0, s, (const float*)row_loss, loss_out, B);
    return uvit_check_launch();
}
