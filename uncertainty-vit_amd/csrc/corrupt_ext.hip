// Four more ImageNet-C-style corruptions of a batch of clean uint8 images on gfx950 (include/uvit.h, uvit_op_corrupt_ext_*; DESIGN.md
// section 9.18; numpy restatement: tests/corrupt_ext_ref.py), beside the nine of corrupt.hip:
//   pixelate           Pillow's resize((n, n), BOX) then resize((S, S), BOX): four integer passes, uint8 intermediates in the workspace
//   jpeg_compression   a JPEG-style round trip without the entropy coder: one workgroup per 16 x 16 MCU (colour conversion, 4:2:0
//                      subsampling, 8 x 8 DCT, quantisation, inverse DCT) into fp32 Y / Cb / Cr planes in the workspace, then one
//                      pointwise launch (triangle chroma upsampling, colour conversion, crop)
//   motion_blur        a one-sided line kernel along one of 91 directions drawn per image, gathered from an LDS tile
//   zoom_blur          the mean of the image and n bilinear zooms about its centre
// Every kind ends with a whole level q in [0, 255] and writes ((q / 255) - mean[c]) / std[c], corrupt.hip's expression.
// This file relies on IEEE fp32 + - * / and rintf / floorf WITHOUT contraction (build.sh: no -ffast-math, -ffp-contract=off): every
// expression below is evaluated operation by operation as it is written, so the float32 numpy restatement reproduces its bytes for
// all four kinds.  No transcendental function runs on the device (the taps, the 91 directions' offsets, the DCT basis and the
// reciprocal zoom factors come from the host's table), no atomics, one owner per output value, every sum in ONE accumulator with its
// taps ascending, acc = acc + (t * x).  The only draw, motion_blur's direction, is counter-based on the image's index in the SET.
#ifdef __FAST_MATH__
#error "corrupt_ext.hip relies on IEEE fp32 arithmetic evaluated as written: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE = 32;               // a motion_blur workgroup owns TILE x TILE outputs, four per thread
constexpr int MAX_BATCH = 21845;       // 3 B planes in a grid dimension
constexpr int MAX_MOTION_R = 24;       // the LDS tile is (TILE + 2 R)^2 floats
constexpr int MAX_ZOOMS = 32;
constexpr int ANGLES = 91;             // motion_blur: whole degrees, theta = a - 45
constexpr int PRECISION_BITS = 22;     // Pillow's Resample.c: 32 - 8 - 2
constexpr int UP_KSIZE = 3;            // the BOX filter's coefficient slots when enlarging
constexpr int JPEG_WORDS = 192;        // DCT basis, luminance and chrominance quantisation tables

struct Norm { float m[3], s[3]; };

__device__ __forceinline__ float quantise(float v) { return floorf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); }
__device__ __forceinline__ float normalise(float q, float m, float s) { return (q / 255.0f - m) / s; }
__device__ __forceinline__ int clampi(int i, int lo, int hi) { return min(max(i, lo), hi); }

// ---- pixelate: one pass of Pillow's ImagingResample along x (HORIZ) or along y ----
// out[o] = clip8((2^21 + sum_k in[first_o + k] coef[o][k]) >> 22) for k < count_o; bounds holds (first, count) per output index of the
// resampled axis, coefs `ksize` slots per output.  One thread per output value; `axis_in` is the input's length along the resampled
// axis, the other axis has the output's length.  The table is clamped to the axis, whatever it holds.
template <bool HORIZ, bool FINAL>
__global__ __launch_bounds__(THREADS)
void pixelate_pass_kernel(const uint8_t* __restrict__ in, void* __restrict__ out, int out_w, int out_h, int axis_in,
                          const int* __restrict__ bounds, const int* __restrict__ coefs, int ksize, Norm nm) {
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= out_w * out_h) return;
    const int y = idx / out_w, x = idx - y * out_w, o = HORIZ ? x : y;
    const int first = clampi(bounds[2 * o], 0, axis_in - 1), count = clampi(bounds[2 * o + 1], 0, min(ksize, axis_in - first));
    const int in_w = HORIZ ? axis_in : out_w, in_h = HORIZ ? out_h : axis_in;
    const uint8_t* src = in + (size_t)blockIdx.y * in_w * in_h + (HORIZ ? (size_t)y * in_w + first : (size_t)first * in_w + x);
    const int* k = coefs + (size_t)o * ksize;
    int ss = 1 << (PRECISION_BITS - 1);
    for (int i = 0; i < count; ++i) ss += (int)src[HORIZ ? i : (size_t)i * in_w] * k[i];
    const int q = clampi(ss >> PRECISION_BITS, 0, 255);
    const size_t dst = (size_t)blockIdx.y * out_w * out_h + idx;
    if (FINAL) {
        const int ch = blockIdx.y % 3;
        static_cast<float*>(out)[dst] = normalise((float)q, nm.m[ch], nm.s[ch]);
    } else {
        static_cast<uint8_t*>(out)[dst] = (uint8_t)q;
    }
}

__device__ __forceinline__ float sample_level(float v) { return floorf(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f); }

// ---- jpeg_compression, first launch: one workgroup per MCU of 16 x 16 pixels, thread (ty, tx) loads pixel (ty, tx) ----
// The planes of image b in the workspace: Y (P x P), Cb and Cr (P/2 x P/2), P = S rounded up to a multiple of 16; the pixels past the
// image repeat its last row and column (for the chrominance: its last pair of rows).  A JPEG sample is an 8-bit level: Y, Cb and Cr are
// rounded to whole levels before anything else reads them, and the 2 x 2 mean of the chrominance is libjpeg's integer one,
// floor((sum + bias) / 4) with bias 1 in the even and 2 in the odd columns (whole numbers below 2^24: exact in fp32).
// Six 8 x 8 blocks per MCU (Y at (by, bx) = 0 .. 3, Cb = 4, Cr = 5) go through
//   F = T (p - 128) T^t along x, then along y;  F' = rintf(F / Q) * Q;  p' = T^t F' T along y, then along x;  p' + 128
// with T[u][x] the host's basis: 384 values per pass on 256 threads, each value one 8-tap sum, taps ascending.
__global__ __launch_bounds__(THREADS)
void jpeg_codec_kernel(const uint8_t* __restrict__ in, float* __restrict__ planes, int S, int P, const float* __restrict__ table) {
    __shared__ float T[64], Q[2][64];
    __shared__ float blk_a[6][64], blk_b[6][64];
    __shared__ float chroma[2][16][16];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < 64) T[tid] = table[tid];
    else if (tid < JPEG_WORDS) Q[(tid - 64) >> 6][(tid - 64) & 63] = table[tid];
    const size_t plane = (size_t)S * S;
    // past the image: columns and luminance rows repeat the last one; chrominance rows repeat the last PAIR of rows, so that the
    // subsampled plane repeats its last row (libjpeg pads a subsampled component after subsampling)
    const int y = blockIdx.y * 16 + ty, x = min((int)blockIdx.x * 16 + tx, S - 1);
    const int yc = y < S ? y : min(((S - 1) & ~1) + (y & 1), S - 1);
    const uint8_t* img_in = in + (size_t)blockIdx.z * 3 * plane + x;
    const uint8_t* src = img_in + (size_t)min(y, S - 1) * S;
    float r = (float)src[0], g = (float)src[plane], b = (float)src[2 * plane];
    blk_a[(ty >> 3) * 2 + (tx >> 3)][(ty & 7) * 8 + (tx & 7)] = sample_level((0.299f * r + 0.587f * g) + 0.114f * b) - 128.0f;
    if (y >= S) {
        src = img_in + (size_t)yc * S;
        r = (float)src[0], g = (float)src[plane], b = (float)src[2 * plane];
    }
    chroma[0][ty][tx] = sample_level(((-0.168736f * r - 0.331264f * g) + 0.5f * b) + 128.0f);
    chroma[1][ty][tx] = sample_level(((0.5f * r - 0.418688f * g) - 0.081312f * b) + 128.0f);
    __syncthreads();
    if (tid < 128) {                                        // 4:2:0: the integer mean of 2 x 2 (an MCU starts at an even chroma column)
        const int c = tid >> 6, j = tid & 63, cy = 2 * (j >> 3), cx = 2 * (j & 7);
        const float sum = (chroma[c][cy][cx] + chroma[c][cy][cx + 1]) + (chroma[c][cy + 1][cx] + chroma[c][cy + 1][cx + 1]);
        const float mean = floorf((sum + ((j & 1) ? 2.0f : 1.0f)) * 0.25f);
        blk_a[4 + c][j] = mean - 128.0f;
    }
    __syncthreads();
    for (int i = tid; i < 6 * 64; i += THREADS) {           // along x: row y, frequency u
        const int k = i >> 6, y = (i >> 3) & 7, u = i & 7;
        float acc = 0.0f;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc = acc + T[u * 8 + x] * blk_a[k][y * 8 + x];
        blk_b[k][y * 8 + u] = acc;
    }
    __syncthreads();
    for (int i = tid; i < 6 * 64; i += THREADS) {           // along y: frequency (v, u); quantised
        const int k = i >> 6, v = (i >> 3) & 7, u = i & 7;
        float acc = 0.0f;
#pragma unroll
        for (int y = 0; y < 8; ++y) acc = acc + T[v * 8 + y] * blk_b[k][y * 8 + u];
        const float q = Q[k >= 4][v * 8 + u];
        blk_a[k][v * 8 + u] = rintf(acc / q) * q;
    }
    __syncthreads();
    for (int i = tid; i < 6 * 64; i += THREADS) {           // the inverse along y
        const int k = i >> 6, y = (i >> 3) & 7, u = i & 7;
        float acc = 0.0f;
#pragma unroll
        for (int v = 0; v < 8; ++v) acc = acc + T[v * 8 + y] * blk_a[k][v * 8 + u];
        blk_b[k][y * 8 + u] = acc;
    }
    __syncthreads();
    float* img = planes + (size_t)blockIdx.z * ((size_t)P * P * 3 / 2);
    const int h = P / 2;
    for (int i = tid; i < 6 * 64; i += THREADS) {           // the inverse along x, + 128
        const int k = i >> 6, y = (i >> 3) & 7, x = i & 7;
        float acc = 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + T[u * 8 + x] * blk_b[k][y * 8 + u];
        acc = acc + 128.0f;
        if (k < 4) img[(size_t)(blockIdx.y * 16 + (k >> 1) * 8 + y) * P + blockIdx.x * 16 + (k & 1) * 8 + x] = acc;
        else img[(size_t)P * P + (size_t)(k - 4) * h * h + (size_t)(blockIdx.y * 8 + y) * h + blockIdx.x * 8 + x] = acc;
    }
}

// ---- jpeg_compression, second launch: one thread per pixel of the image ----
// Chroma by the triangle filter, 0.75 near + 0.25 far per axis, vertical then horizontal, the far sample clamped to the image's samples.
__device__ __forceinline__ float chroma_up(const float* __restrict__ c, int h, int ny, int fy, int nx, int fx) {
    const float vn = 0.75f * c[(size_t)ny * h + nx] + 0.25f * c[(size_t)fy * h + nx];
    const float vf = 0.75f * c[(size_t)ny * h + fx] + 0.25f * c[(size_t)fy * h + fx];
    return 0.75f * vn + 0.25f * vf;
}

__global__ __launch_bounds__(THREADS)
void jpeg_finish_kernel(const float* __restrict__ planes, float* __restrict__ out, int S, int P, Norm nm) {
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= S * S) return;
    const int y = idx / S, x = idx - y * S, h = P / 2, hc = (S + 1) / 2;      // the image has hc x hc chroma samples of the plane's h x h
    const float* img = planes + (size_t)blockIdx.y * ((size_t)P * P * 3 / 2);
    const int ny = y >> 1, fy = clampi(ny + ((y & 1) ? 1 : -1), 0, hc - 1), nx = x >> 1, fx = clampi(nx + ((x & 1) ? 1 : -1), 0, hc - 1);
    const float Y = img[(size_t)y * P + x];
    const float cb = chroma_up(img + (size_t)P * P, h, ny, fy, nx, fx) - 128.0f;
    const float cr = chroma_up(img + (size_t)P * P + (size_t)h * h, h, ny, fy, nx, fx) - 128.0f;
    const float rgb[3] = {Y + 1.402f * cr, (Y - 0.344136f * cb) - 0.714136f * cr, Y + 1.772f * cb};
    float* dst = out + (size_t)blockIdx.y * 3 * S * S + idx;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        dst[(size_t)ch * S * S] = normalise(floorf(fminf(fmaxf(rgb[ch], 0.0f), 255.0f) + 0.5f), nm.m[ch], nm.s[ch]);
}

// ---- motion_blur ----
// table: w[R + 1], then per direction a: ox[R + 1], oy[R + 1] (whole numbers).  A workgroup stages the (TILE + 2 R)^2 inputs of its
// TILE x TILE outputs in LDS, the border replicated while loading; thread (tx, ty) owns the outputs (ty + 8 i, tx), i = 0 .. 3.
__global__ __launch_bounds__(THREADS)
void motion_blur_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int S, int R, const float* __restrict__ table, uint32_t kseed,
                        uint32_t index0, Norm nm) {
    extern __shared__ float tile[];
    const int tw = TILE + 2 * R, x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    const size_t base = (size_t)blockIdx.z * S * S;
    for (int i = threadIdx.x; i < tw * tw; i += THREADS) {
        const int ly = i / tw, lx = i - ly * tw;
        tile[i] = (float)in[base + (size_t)clampi(y0 + ly - R, 0, S - 1) * S + clampi(x0 + lx - R, 0, S - 1)] / 255.0f;
    }
    __syncthreads();
    const uint32_t ikey = corrupt_image_key(kseed, index0 + blockIdx.z / 3);
    const uint32_t a = ((uvit_hash32(ikey ^ 0x1B873593u) >> 8) * (uint32_t)ANGLES) >> 24;
    const float* ox = table + (size_t)(R + 1) * (1 + 2 * a);
    const float* oy = ox + (R + 1);
    const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x / TILE;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i <= R; ++i) {
        const float w = table[i];
        const float* p = tile + (ty + R - clampi((int)oy[i], -R, R)) * tw + tx + R - clampi((int)ox[i], -R, R);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + w * p[j * 8 * tw];
    }
    const int ch = blockIdx.z % 3, x = x0 + tx;
    if (x >= S) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = y0 + ty + 8 * j;
        if (y < S) out[base + (size_t)y * S + x] = normalise(quantise(acc[j]), nm.m[ch], nm.s[ch]);
    }
}

// ---- zoom_blur: one thread per output value; table: 1 / z_j, j < n ----
// zoom_j samples the plane bilinearly at c + (p - c) (1 / z_j), c = (S - 1) / 2: z_j >= 1 keeps every sample between the pixel and the
// centre, the clamps only guard a table that holds something else.  Horizontal interpolation first, then vertical.
__global__ __launch_bounds__(THREADS)
void zoom_blur_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int S, int n, const float* __restrict__ table, Norm nm) {
    __shared__ float unit[256];                             // float(u8) / 255.0f of every level: one division per level, not per sample
    unit[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= S * S) return;
    const int y = idx / S, x = idx - y * S;
    const uint8_t* p = in + (size_t)blockIdx.y * S * S;
    const float c = (float)(S - 1) / 2.0f, dx = (float)x - c, dy = (float)y - c;
    float acc = unit[p[idx]];
    for (int j = 0; j < n; ++j) {
        const float iz = table[j], sx = c + dx * iz, sy = c + dy * iz;
        const int xa = clampi((int)floorf(sx), 0, S - 1), ya = clampi((int)floorf(sy), 0, S - 1), xb = min(xa + 1, S - 1), yb = min(ya + 1, S - 1);
        const float fx = sx - (float)xa, fy = sy - (float)ya;
        const float v00 = unit[p[(size_t)ya * S + xa]], v01 = unit[p[(size_t)ya * S + xb]];
        const float v10 = unit[p[(size_t)yb * S + xa]], v11 = unit[p[(size_t)yb * S + xb]];
        const float top = v00 + (v01 - v00) * fx, bot = v10 + (v11 - v10) * fx;
        acc = acc + (top + (bot - top) * fy);
    }
    const int ch = blockIdx.y % 3;
    out[(size_t)blockIdx.y * S * S + idx] = normalise(quantise(acc / (float)(n + 1)), nm.m[ch], nm.s[ch]);
}

// ---- host side: validation and launches ----
inline bool bad_kind(int kind) { return kind < 0 || kind >= UVIT_CORRUPT_EXT_KINDS; }
inline int check_shape(int B, int S) { return (B < 1 || B > MAX_BATCH || S < 8 || S > 1024) ? UVIT_ERR_SHAPE : UVIT_OK; }
inline bool make_norm(const float* mean, const float* stdv, Norm* nm) {
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(mean[c]) || !std::isfinite(stdv[c]) || stdv[c] == 0.0f) return false;
        nm->m[c] = mean[c];
        nm->s[c] = stdv[c];
    }
    return true;
}
inline int down_ksize(int S, int n) { return 2 * ((S + 2 * n - 1) / (2 * n)) + 1; }      // 2 ceil(0.5 S / n) + 1
inline int padded(int S) { return (S + 15) / 16 * 16; }
// The kind's integer argument: UVIT_OK, or the error of a value outside the kind's range (S has been checked).
inline int check_arg(int kind, int S, int arg) {
    switch (kind) {
        case UVIT_CORRUPT_EXT_PIXELATE: return (arg < 1 || arg > S) ? UVIT_ERR_ARG : UVIT_OK;
        case UVIT_CORRUPT_EXT_JPEG_COMPRESSION: return arg != 0 ? UVIT_ERR_ARG : UVIT_OK;
        case UVIT_CORRUPT_EXT_MOTION_BLUR: return arg < 1 ? UVIT_ERR_ARG : (arg >= S || arg > MAX_MOTION_R) ? UVIT_ERR_SHAPE : UVIT_OK;
        default: return (arg < 1 || arg > MAX_ZOOMS) ? UVIT_ERR_ARG : UVIT_OK;
    }
}
inline int64_t table_words(int kind, int S, int arg) {
    switch (kind) {
        case UVIT_CORRUPT_EXT_PIXELATE: return (int64_t)arg * (2 + down_ksize(S, arg)) + (int64_t)S * (2 + UP_KSIZE);
        case UVIT_CORRUPT_EXT_JPEG_COMPRESSION: return JPEG_WORDS;
        case UVIT_CORRUPT_EXT_MOTION_BLUR: return (int64_t)(arg + 1) * (1 + 2 * ANGLES);
        default: return arg;
    }
}
inline int64_t ws_need(int kind, int B, int S, int arg) {
    if (kind == UVIT_CORRUPT_EXT_PIXELATE) return align16((int64_t)B * 3 * ((int64_t)2 * S * arg + (int64_t)arg * arg));
    if (kind == UVIT_CORRUPT_EXT_JPEG_COMPRESSION) return (int64_t)B * padded(S) * padded(S) * 3 / 2 * (int64_t)sizeof(float);
    return 0;
}
inline dim3 flat_grid(int64_t values, int planes) { return dim3((unsigned)((values + THREADS - 1) / THREADS), (unsigned)planes); }

}  // namespace

extern "C" int64_t uvit_op_corrupt_ext_ws_bytes(int kind, int B, int S, int arg) {
    if (bad_kind(kind)) return UVIT_ERR_ARG;
    if (check_shape(B, S)) return UVIT_ERR_SHAPE;
    if (const int e = check_arg(kind, S, arg)) return e;
    return ws_need(kind, B, S, arg);
}

extern "C" int uvit_op_corrupt_ext_batch(const uint8_t* in_u8, float* out, int B, int S, int kind, const void* table, int n_table, int arg,
                                         uint32_t seed, int64_t index0, const float* mean, const float* stdv, void* ws, int64_t ws_bytes,
                                         uvit_stream stream) {
    if (!in_u8 || !out || !table || !mean || !stdv || bad_kind(kind)) return UVIT_ERR_ARG;
    Norm nm;
    if (!make_norm(mean, stdv, &nm)) return UVIT_ERR_ARG;
    if (index0 < 0 || index0 > (int64_t)0xFFFFFFFFll - MAX_BATCH) return UVIT_ERR_ARG;
    if (check_shape(B, S)) return UVIT_ERR_SHAPE;
    if (const int e = check_arg(kind, S, arg)) return e;
    if ((int64_t)n_table != table_words(kind, S, arg)) return UVIT_ERR_ARG;
    const int64_t need = ws_need(kind, B, S, arg);
    if (need > 0 && !ws) return UVIT_ERR_ARG;
    if (ws_bytes < need) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int planes = 3 * B;
    if (kind == UVIT_CORRUPT_EXT_PIXELATE) {
        const int n = arg, kd = down_ksize(S, n);
        const int* bd = (const int*)table;                  // (n, 2), then (n, kd), then (S, 2), then (S, 3)
        const int *cd = bd + 2 * n, *bu = cd + (size_t)n * kd, *cu = bu + 2 * S;
        uint8_t* t1 = (uint8_t*)ws;                         // (planes, S, n), (planes, n, n), (planes, n, S)
        uint8_t *t2 = t1 + (size_t)planes * S * n, *t3 = t2 + (size_t)planes * n * n;
        hipLaunchKernelGGL((pixelate_pass_kernel<true, false>), flat_grid((int64_t)S * n, planes), dim3(THREADS), 0, s, in_u8, (void*)t1, n, S, S, bd, cd, kd, nm);
        hipLaunchKernelGGL((pixelate_pass_kernel<false, false>), flat_grid((int64_t)n * n, planes), dim3(THREADS), 0, s, (const uint8_t*)t1, (void*)t2, n, n, S, bd, cd, kd, nm);
        hipLaunchKernelGGL((pixelate_pass_kernel<true, false>), flat_grid((int64_t)n * S, planes), dim3(THREADS), 0, s, (const uint8_t*)t2, (void*)t3, S, n, n, bu, cu, UP_KSIZE, nm);
        hipLaunchKernelGGL((pixelate_pass_kernel<false, true>), flat_grid((int64_t)S * S, planes), dim3(THREADS), 0, s, (const uint8_t*)t3, (void*)out, S, S, n, bu, cu, UP_KSIZE, nm);
    } else if (kind == UVIT_CORRUPT_EXT_JPEG_COMPRESSION) {
        const int P = padded(S);
        hipLaunchKernelGGL(jpeg_codec_kernel, dim3(P / 16, P / 16, B), dim3(THREADS), 0, s, in_u8, (float*)ws, S, P, (const float*)table);
        hipLaunchKernelGGL(jpeg_finish_kernel, flat_grid((int64_t)S * S, B), dim3(THREADS), 0, s, (const float*)ws, out, S, P, nm);
    } else if (kind == UVIT_CORRUPT_EXT_MOTION_BLUR) {
        // the key of the set and the kind, numbered behind the nine of corrupt.hip; the image's index joins it on the device
        const uint32_t kseed = uvit_hash32(seed ^ ((uint32_t)(UVIT_CORRUPT_KINDS + kind + 1) * 0x9E3779B9u));
        const int tw = TILE + 2 * arg;
        hipLaunchKernelGGL(motion_blur_kernel, dim3((S + TILE - 1) / TILE, (S + TILE - 1) / TILE, planes), dim3(THREADS), (size_t)tw * tw * sizeof(float), s,
                           in_u8, out, S, arg, (const float*)table, kseed, (uint32_t)index0, nm);
    } else {
        hipLaunchKernelGGL(zoom_blur_kernel, flat_grid((int64_t)S * S, planes), dim3(THREADS), 0, s, in_u8, out, S, arg, (const float*)table, nm);
    }
    return uvit_check_launch();
}
