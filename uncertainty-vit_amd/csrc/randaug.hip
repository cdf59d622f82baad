// RandAugment of a batch of normalised images on gfx950 with Pillow's arithmetic bit for bit (include/uvit.h, uvit_op_randaug_batch;
// DESIGN.md section 9.21; numpy restatement: tests/randaug_ref.py).  The batch is quantised into planar uint8, every layer reads the
// planes the previous one wrote and writes the other copy, and the last stage is the augmentation's ToTensor + Normalize:
//   ra_pack     x -> uint8, corrupt.hip's quantisation
//   ra_stats    layer l, one workgroup per image whose op needs them: the three histograms by integer LDS atomics and from them the
//               AutoContrast (double) or Equalize (integer) tables, or the rounded mean of L for Contrast
//   ra_apply    layer l, one thread per pixel and all three channels: table, blend or affine op of the image's descriptor
//   ra_unpack   uint8 -> ((u8 / 255) - mean) / std
// An image's current copy is the parity of the ops it has had, so a NONE layer moves no bytes.  Every output value has one owner.
// This file relies on IEEE fp32 and fp64 + - * / WITHOUT contraction (build.sh: no -ffast-math, -ffp-contract=off): Blend.c's
// d + f * (x - d), Filter.c's float accumulator and Geometry.c's double polynomials are evaluated operation by operation as written.
#ifdef __FAST_MATH__
#error "randaug.hip relies on IEEE arithmetic evaluated as written: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"
#include "pil_pixel.h"

namespace {

constexpr int THREADS = 256;
constexpr int STAT_THREADS = 1024;
constexpr int MAX_BATCH = 65535;       // B rows in gridDim.y
constexpr int MAX_SIZE = 1024;         // the sum of L fits 32 bits, the fixed-point walk of NEAREST stays inside 32 bits
constexpr int MAX_LAYERS = UVIT_RANDAUG_MAX_LAYERS;
constexpr int TABLE_BYTES = 1024;      // per image: three 256-byte tables, then the mean of L as an int
constexpr double MAX_LINEAR = 4.0, MAX_SHIFT = 8192.0;

struct Norm { float m[3], s[3]; };

__device__ __forceinline__ float quantise(float v) { return floorf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); }   // corrupt.hip's
__device__ __forceinline__ float normalise(float q, float m, float s) { return (q / 255.0f - m) / s; }

__host__ __device__ inline bool is_affine(int op) { return op == UVIT_RA_ROTATE || (op >= UVIT_RA_SHEAR_X && op <= UVIT_RA_TRANSLATE_Y_REL); }
__host__ __device__ inline bool needs_stats(int op) { return op == UVIT_RA_AUTOCONTRAST || op == UVIT_RA_EQUALIZE || op == UVIT_RA_CONTRAST; }
// which of the two copies holds image b in front of layer l: the parity of the ops it has had
__device__ inline int copy_in_front_of(const uvit_randaug_desc& d, int l) {
    int n = 0;
    for (int i = 0; i < MAX_LAYERS; ++i) n += (i < l && i < d.n_layers && d.layers[i].op != UVIT_RA_NONE) ? 1 : 0;
    return n & 1;
}

// ---- pack and its inverse ----
template <int VEC>
__global__ __launch_bounds__(THREADS)
void ra_pack_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int64_t n, int64_t plane, Norm nm) {
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

template <int VEC>
__global__ __launch_bounds__(THREADS)
void ra_unpack_kernel(const uvit_randaug_desc* __restrict__ desc, const uint8_t* __restrict__ buf0, const uint8_t* __restrict__ buf1,
                      float* __restrict__ out, int64_t image, int64_t plane, Norm nm) {
    const int64_t i = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * VEC;      // inside the image: plane % VEC == 0, one channel per thread
    if (i >= image) return;
    const int b = blockIdx.y;
    const int ch = (int)(i / plane);
    const uint8_t* src = (copy_in_front_of(desc[b], MAX_LAYERS) ? buf1 : buf0) + (int64_t)b * image + i;
    float* dst = out + (int64_t)b * image + i;
    const float m = nm.m[ch], s = nm.s[ch];
    if (VEC == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(src);
        *reinterpret_cast<float4*>(dst) = make_float4(normalise((float)(w & 255u), m, s), normalise((float)((w >> 8) & 255u), m, s),
                                                      normalise((float)((w >> 16) & 255u), m, s), normalise((float)(w >> 24), m, s));
    } else {
        dst[0] = normalise((float)src[0], m, s);
    }
}

// ---- statistics of layer l: the tables of AutoContrast and Equalize, the mean of L of Contrast ----
__global__ __launch_bounds__(STAT_THREADS)
void ra_stats_kernel(const uvit_randaug_desc* __restrict__ desc, const uint8_t* __restrict__ buf0, const uint8_t* __restrict__ buf1,
                     uint8_t* __restrict__ tables, int S, int layer) {
    const int b = blockIdx.x;
    const uvit_randaug_desc& d = desc[b];
    if (layer >= d.n_layers) return;
    const int op = d.layers[layer].op;
    if (!needs_stats(op)) return;
    __shared__ unsigned int hist[3][256];
    __shared__ unsigned int lsum;
    __shared__ int lo[3], hi[3], levels[3];
    const int t = threadIdx.x;
    const int plane = S * S;
    const uint8_t* src = (copy_in_front_of(d, layer) ? buf1 : buf0) + (size_t)b * 3 * plane;
    uint8_t* table = tables + (size_t)b * TABLE_BYTES;
    if (t < 768) hist[t >> 8][t & 255] = 0u;
    if (t == 0) lsum = 0u;
    __syncthreads();
    if (op == UVIT_RA_CONTRAST) {
        unsigned int acc = 0u;                               // at most 255 * 1024 per thread
        for (int p = t; p < plane; p += STAT_THREADS) acc += (unsigned int)luma(src[p], src[plane + p], src[2 * plane + p]);
        atomicAdd(&lsum, acc);                               // integer: the order does not matter; at most 255 * 2^20
        __syncthreads();
        if (t == 0) {
            const double mean = (double)lsum / (double)plane;            // ImageStat: sum / count
            *reinterpret_cast<int*>(table + 768) = (int)(mean + 0.5);
        }
        return;
    }
    for (int p = t; p < plane; p += STAT_THREADS) {
        atomicAdd(&hist[0][src[p]], 1u);
        atomicAdd(&hist[1][src[plane + p]], 1u);
        atomicAdd(&hist[2][src[2 * plane + p]], 1u);
    }
    __syncthreads();
    if (t < 3) {
        int l = 256, h = -1, n = 0;
        for (int i = 0; i < 256; ++i)
            if (hist[t][i]) {
                if (l == 256) l = i;
                h = i;
                ++n;
            }
        lo[t] = l;
        hi[t] = h;
        levels[t] = n;
    }
    __syncthreads();
    if (t >= 768) return;
    const int c = t >> 8, v = t & 255;
    int r = v;
    if (op == UVIT_RA_AUTOCONTRAST) {
        if (hi[c] > lo[c]) {
            const double scale = 255.0 / (double)(hi[c] - lo[c]);
            const double offset = (double)(-lo[c]) * scale;
            r = (int)((double)v * scale + offset);
            r = r < 0 ? 0 : r > 255 ? 255 : r;
        }
    } else {                                                 // equalize
        const int step = (plane - (int)hist[c][hi[c]]) / 255;
        if (levels[c] > 1 && step > 0) {
            int n = step / 2;
            for (int j = 0; j < v; ++j) n += (int)hist[c][j];
            r = n / step;
            r = r > 255 ? 255 : r;
        }
    }
    table[t] = (uint8_t)r;
}

// ---- the ops of layer l ----
__device__ __forceinline__ int floor_int(double v) { return v >= 0.0 ? (int)v : (int)floor(v); }      // Geometry.c's FLOOR
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

// bilinear (TAPS 2) or bicubic (TAPS 4) sample of one channel plane at the source position (xs, ys) = (xin - 0.5, yin - 0.5)
template <int TAPS>
__device__ __forceinline__ int sample(const uint8_t* __restrict__ ch, int S, double xs, double ys) {
    int x = floor_int(xs), y = floor_int(ys);
    const double dx = xs - x, dy = ys - y;
    if (TAPS == 4) { --x; --y; }
    int col[TAPS];
#pragma unroll
    for (int i = 0; i < TAPS; ++i) col[i] = clampi(x + i, S - 1);
    double row[TAPS];
#pragma unroll
    for (int j = 0; j < TAPS; ++j) {
        const int yy = y + j;
        if (j == 0 || (yy >= 0 && yy < S)) {
            const uint8_t* in = ch + (size_t)clampi(yy, S - 1) * S;
            if (TAPS == 2) {
                const double a = in[col[0]], bb = in[col[1]];
                row[j] = a + (bb - a) * dx;
            } else {
                row[j] = cubic((double)in[col[0]], (double)in[col[1]], (double)in[col[2]], (double)in[col[3]], dx);
            }
        } else {
            row[j] = row[j - 1];
        }
    }
    if (TAPS == 2) return (int)(row[0] + (row[1] - row[0]) * dy);             // (UINT8) v: inside [0, 255], truncated
    const double v = cubic(row[0], row[1], row[2], row[3], dy);
    return v <= 0.0 ? 0 : v >= 255.0 ? 255 : (int)v;
}

__device__ __forceinline__ int fix16(double v) { return floor_int(v * 65536.0 + 0.5); }
__device__ __forceinline__ int coord(double v) { return v < 0.0 ? -1 : (int)v; }

__global__ __launch_bounds__(THREADS)
void ra_apply_kernel(const uvit_randaug_desc* __restrict__ desc, const uint8_t* __restrict__ tables, uint8_t* __restrict__ buf0,
                     uint8_t* __restrict__ buf1, int S, int layer) {
    const int b = blockIdx.y;
    const uvit_randaug_desc& d = desc[b];
    if (layer >= d.n_layers) return;
    const uvit_randaug_layer& e = d.layers[layer];
    const int op = e.op;
    if (op == UVIT_RA_NONE) return;
    const int plane = S * S;
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= plane) return;
    const int cur = copy_in_front_of(d, layer);
    const uint8_t* src = (cur ? buf1 : buf0) + (size_t)b * 3 * plane;
    uint8_t* dst = (cur ? buf0 : buf1) + (size_t)b * 3 * plane;
    const int y = p / S, x = p - y * S;
    int v[3] = {src[p], src[plane + p], src[2 * plane + p]};
    if (is_affine(op)) {
        const double m0 = e.matrix[0], m1 = e.matrix[1], m2 = e.matrix[2], m3 = e.matrix[3], m4 = e.matrix[4], m5 = e.matrix[5];
        v[0] = (int)(e.fill & 255u);
        v[1] = (int)((e.fill >> 8) & 255u);
        v[2] = (int)((e.fill >> 16) & 255u);
        if (e.filter == UVIT_RA_NEAREST) {
            int sx, sy;
            if (m1 == 0.0 && m3 == 0.0) {                    // ImagingScaleAffine
                sx = coord((m2 + m0 * 0.5) + m0 * (double)x);
                sy = coord((m5 + m4 * 0.5) + m4 * (double)y);
            } else {                                         // affine_fixed
                sx = (fix16(m2 + m0 * 0.5 + m1 * 0.5) + x * fix16(m0) + y * fix16(m1)) >> 16;
                sy = (fix16(m5 + m3 * 0.5 + m4 * 0.5) + x * fix16(m3) + y * fix16(m4)) >> 16;
            }
            if (sx >= 0 && sx < S && sy >= 0 && sy < S) {
                const int q = sy * S + sx;
                v[0] = src[q];
                v[1] = src[plane + q];
                v[2] = src[2 * plane + q];
            }
        } else {
            const double xc = (double)x + 0.5, yc = (double)y + 0.5;
            const double xin = m0 * xc + m1 * yc + m2, yin = m3 * xc + m4 * yc + m5;
            if (xin >= 0.0 && xin < (double)S && yin >= 0.0 && yin < (double)S) {
                const double xs = xin - 0.5, ys = yin - 0.5;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    v[c] = e.filter == UVIT_RA_BILINEAR ? sample<2>(src + (size_t)c * plane, S, xs, ys) : sample<4>(src + (size_t)c * plane, S, xs, ys);
            }
        }
    } else if (op == UVIT_RA_INVERT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = 255 - v[c];
    } else if (op == UVIT_RA_POSTERIZE) {
        const int mask = e.arg0 >= 8 ? 255 : ~((1 << (8 - e.arg0)) - 1) & 255;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] &= mask;
    } else if (op == UVIT_RA_SOLARIZE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] < e.arg0 ? v[c] : 255 - v[c];
    } else if (op == UVIT_RA_SOLARIZE_ADD) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] < e.arg1 ? min(255, v[c] + e.arg0) : v[c];
    } else if (op == UVIT_RA_AUTOCONTRAST || op == UVIT_RA_EQUALIZE) {
        const uint8_t* table = tables + (size_t)b * TABLE_BYTES;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = table[c * 256 + v[c]];
    } else {                                                 // the four ImageEnhance ops
        int deg[3] = {0, 0, 0};                              // brightness: black
        if (op == UVIT_RA_COLOR) {
            deg[0] = deg[1] = deg[2] = luma(v[0], v[1], v[2]);
        } else if (op == UVIT_RA_CONTRAST) {
            deg[0] = deg[1] = deg[2] = *reinterpret_cast<const int*>(tables + (size_t)b * TABLE_BYTES + 768);
        } else if (op == UVIT_RA_SHARPNESS) {
            if (x == 0 || y == 0 || x == S - 1 || y == S - 1) {
                deg[0] = v[0]; deg[1] = v[1]; deg[2] = v[2];
            } else {
                const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint8_t* in = src + (size_t)c * plane + p;
                    float acc = 0.5f;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) acc = acc + (float)in[dy * S + dx] * ((dy == 0 && dx == 0) ? k5 : k1);
                    deg[c] = acc <= 0.0f ? 0 : acc >= 255.0f ? 255 : (int)acc;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = blend(deg[c], v[c], e.factor);
    }
    dst[p] = (uint8_t)v[0];
    dst[plane + p] = (uint8_t)v[1];
    dst[2 * plane + p] = (uint8_t)v[2];
}

// ---- host side ----
inline int check_shape(int B, int S) { return (B < 1 || B > MAX_BATCH || S < 1 || S > MAX_SIZE) ? UVIT_ERR_SHAPE : UVIT_OK; }
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
inline size_t off_tables(int B) { return align256((size_t)B * sizeof(uvit_randaug_desc)); }
inline size_t off_buf0(int B) { return off_tables(B) + (size_t)B * TABLE_BYTES; }
inline size_t buf_bytes(int B, int S) { return align256((size_t)B * 3 * S * S); }
inline int64_t ws_need(int B, int S) { return (int64_t)(off_buf0(B) + 2 * buf_bytes(B, S)); }

int check_layer(const uvit_randaug_layer& e) {
    if (e.op < 0 || e.op >= UVIT_RA_OPS) return UVIT_ERR_ARG;
    if (e.filter != UVIT_RA_NEAREST && e.filter != UVIT_RA_BILINEAR && e.filter != UVIT_RA_BICUBIC) return UVIT_ERR_ARG;
    if (!std::isfinite(e.factor)) return UVIT_ERR_ARG;
    for (int i = 0; i < 6; ++i) {
        if (!std::isfinite(e.matrix[i])) return UVIT_ERR_ARG;
        if (is_affine(e.op) && fabs(e.matrix[i]) > (i % 3 == 2 ? MAX_SHIFT : MAX_LINEAR)) return UVIT_ERR_ARG;
    }
    if (e.op == UVIT_RA_POSTERIZE && (e.arg0 < 0 || e.arg0 > 8)) return UVIT_ERR_ARG;
    if (e.op == UVIT_RA_SOLARIZE && (e.arg0 < 0 || e.arg0 > 256)) return UVIT_ERR_ARG;
    if (e.op == UVIT_RA_SOLARIZE_ADD && (e.arg0 < 0 || e.arg0 > 255 || e.arg1 < 0 || e.arg1 > 256)) return UVIT_ERR_ARG;
    return UVIT_OK;
}

}  // namespace

extern "C" int64_t uvit_op_randaug_ws_bytes(int B, int S) {
    if (check_shape(B, S)) return UVIT_ERR_SHAPE;
    return ws_need(B, S);
}

extern "C" int uvit_op_randaug_batch(const float* x, float* out, const uvit_randaug_desc* desc, int B, int S, const float* mean,
                                     const float* stdv, void* workspace, int64_t ws_bytes, uvit_stream stream) {
    if (!x || !out || !desc || !mean || !stdv || !workspace) return UVIT_ERR_ARG;
    if (check_shape(B, S)) return UVIT_ERR_SHAPE;
    if (misaligned(x, 4) || misaligned(out, 4) || misaligned(workspace, 16)) return UVIT_ERR_ARG;
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(mean[c]) || !std::isfinite(stdv[c]) || stdv[c] == 0.0f) return UVIT_ERR_ARG;
        nm.m[c] = mean[c];
        nm.s[c] = stdv[c];
    }
    bool stats[MAX_LAYERS] = {}, apply[MAX_LAYERS] = {};
    for (int b = 0; b < B; ++b) {
        const uvit_randaug_desc& d = desc[b];
        if (d.n_layers < 0 || d.n_layers > MAX_LAYERS) return UVIT_ERR_SHAPE;
        for (int l = 0; l < d.n_layers; ++l) {
            const int rc = check_layer(d.layers[l]);
            if (rc) return rc;
            stats[l] |= needs_stats(d.layers[l].op);
            apply[l] |= d.layers[l].op != UVIT_RA_NONE;
        }
    }
    if (ws_bytes < ws_need(B, S)) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uvit_randaug_desc* ddesc = (uvit_randaug_desc*)ws;
    uint8_t* tables = (uint8_t*)(ws + off_tables(B));
    uint8_t* buf0 = (uint8_t*)(ws + off_buf0(B));
    uint8_t* buf1 = buf0 + buf_bytes(B, S);
    if (hipMemcpyAsync(ddesc, desc, (size_t)B * sizeof(uvit_randaug_desc), hipMemcpyHostToDevice, s) != hipSuccess) return UVIT_ERR_LAUNCH;
    const int64_t plane = (int64_t)S * S, image = 3 * plane, n = (int64_t)B * image;
    const bool vec = plane % 4 == 0 && !misaligned(x, 16) && !misaligned(out, 16);
    if (vec) hipLaunchKernelGGL(ra_pack_kernel<4>, dim3((unsigned)((n / 4 + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, x, buf0, n, plane, nm);
    else hipLaunchKernelGGL(ra_pack_kernel<1>, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, x, buf0, n, plane, nm);
    for (int l = 0; l < MAX_LAYERS; ++l) {
        if (stats[l])
            hipLaunchKernelGGL(ra_stats_kernel, dim3(B), dim3(STAT_THREADS), 0, s, (const uvit_randaug_desc*)ddesc, (const uint8_t*)buf0,
                               (const uint8_t*)buf1, tables, S, l);
        if (apply[l])
            hipLaunchKernelGGL(ra_apply_kernel, dim3((unsigned)((plane + THREADS - 1) / THREADS), B), dim3(THREADS), 0, s,
                               (const uvit_randaug_desc*)ddesc, (const uint8_t*)tables, buf0, buf1, S, l);
    }
    if (vec)
        hipLaunchKernelGGL(ra_unpack_kernel<4>, dim3((unsigned)((image / 4 + THREADS - 1) / THREADS), B), dim3(THREADS), 0, s,
                           (const uvit_randaug_desc*)ddesc, (const uint8_t*)buf0, (const uint8_t*)buf1, out, image, plane, nm);
    else
        hipLaunchKernelGGL(ra_unpack_kernel<1>, dim3((unsigned)((image + THREADS - 1) / THREADS), B), dim3(THREADS), 0, s,
                           (const uvit_randaug_desc*)ddesc, (const uint8_t*)buf0, (const uint8_t*)buf1, out, image, plane, nm);
    return uvit_check_launch();
}
