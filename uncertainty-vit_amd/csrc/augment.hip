// BEiT augmentation of a batch of decoded images on gfx950, with Pillow's arithmetic bit for bit
// (include/uvit.h, uvit_op_augment_batch; numpy restatement: tests/augment_util.py).
//
//   ColorJitter (ImageEnhance Brightness / Contrast / Color = Image.blend, Blend.c)
//   -> horizontal flip -> crop -> resize with the 8-bit separable resampler of Resample.c
//   -> ToTensor + Normalize into fp32 NCHW
//
// Four launches per batch, all on the caller's stream:
//   aug_contrast_sum  exact integer sum of L over the whole image, for samples whose jitter has a contrast step
//                     (the only non-pointwise step; L of the image as it stands when contrast runs)
//   aug_coeffs        per sample and axis: the filter taps of every output position in the window (fp64, then 22-bit fixed point)
//   aug_hpass         horizontal pass over the source rows the vertical pass reads; the jitter is applied to each pixel loaded
//   aug_vpass         vertical pass, ToTensor + Normalize, zero padding outside the resized image
//
// IEEE semantics are required: build.sh compiles this file WITHOUT -ffast-math and with -ffp-contract=off, so
// d + f * (x - d) is a float multiply then a float add (as Blend.c), the divisions are correctly rounded, and the fp64
// coefficient arithmetic is evaluated operation by operation as Resample.c writes it.
#include <algorithm>
#include <cmath>
#include <math.h>

#include "common.h"
#include "pil_pixel.h"
#include "../../include/uvit.h"

#if defined(__FAST_MATH__) || __FINITE_MATH_ONLY__
#error "augment.hip must be compiled without -ffast-math (bit-exact Pillow arithmetic)"
#endif

namespace {

constexpr int PRECISION_BITS = 22;   // Resample.c: 32 - 8 - 2
constexpr int AUG_THREADS = 256;
constexpr int MAX_SIDE = 1 << 15;    // bound on every image / resize / output side

// ---- Resample.c filters (double, evaluated as written) ----
__host__ __device__ inline double filt_bilinear(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}
__host__ __device__ inline double filt_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
__host__ __device__ inline double filt_hamming(double x) {
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * M_PI;
    return sin(x) / x * (0.54f + 0.46f * cos(x));
}
__host__ __device__ inline double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
__host__ __device__ inline double filt_lanczos(double x) {
    if (-3.0 <= x && x < 3.0) return sinc(x) * sinc(x / 3);
    return 0.0;
}
__host__ __device__ inline double filt_support(int f) {
    return f == UVIT_AUG_BICUBIC ? 2.0 : f == UVIT_AUG_LANCZOS ? 3.0 : 1.0;
}
__host__ __device__ inline double filt_eval(int f, double x) {
    switch (f) {
        case UVIT_AUG_BILINEAR: return filt_bilinear(x);
        case UVIT_AUG_BICUBIC: return filt_bicubic(x);
        case UVIT_AUG_HAMMING: return filt_hamming(x);
        default: return filt_lanczos(x);
    }
}

// One axis of a resize in_size -> out_size, as precompute_coeffs (Resample.c) sets it up.
struct Axis {
    double scale, support, ss;
    int in_size, ksize;
};
__host__ __device__ inline Axis make_axis(int in_size, int out_size, int f) {
    Axis a;
    a.in_size = in_size;
    a.scale = (double)in_size / out_size;
    const double filterscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = filt_support(f) * filterscale;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    a.ss = 1.0 / filterscale;
    return a;
}
// taps [xmin, xmin + xlen) of output position xx, and its centre
__host__ __device__ inline void axis_bounds(const Axis& a, int xx, int* xmin, int* xlen, double* center) {
    const double c = (xx + 0.5) * a.scale;
    int lo = (int)(c - a.support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(c + a.support + 0.5);
    if (hi > a.in_size) hi = a.in_size;
    *xmin = lo;
    *xlen = hi - lo;
    *center = c;
}

__host__ __device__ inline bool need_h(const uvit_augment_desc& d) { return d.resize_w != d.crop_w; }
__host__ __device__ inline bool need_v(const uvit_augment_desc& d) { return d.resize_h != d.crop_h; }

// Rows [r0, r1) of the crop the horizontal pass produces: the rows the vertical pass reads for the window's rows inside
// the resized image (ImagingResampleInner's ybox_first / ybox_last, restricted to the window).  r1 <= r0: nothing.
__host__ __device__ inline void row_range(const uvit_augment_desc& d, int S, int* r0, int* r1) {
    const int y0 = d.win_y > 0 ? d.win_y : 0;
    const int y1 = d.win_y + S < d.resize_h ? d.win_y + S : d.resize_h;
    const int x0 = d.win_x > 0 ? d.win_x : 0;
    const int x1 = d.win_x + S < d.resize_w ? d.win_x + S : d.resize_w;
    if (y0 >= y1 || x0 >= x1) { *r0 = *r1 = 0; return; }
    if (!need_v(d)) { *r0 = y0; *r1 = y1; return; }
    const Axis a = make_axis(d.crop_h, d.resize_h, d.filter);
    int lo, n;
    double c;
    axis_bounds(a, y0, &lo, &n, &c);
    *r0 = lo;
    axis_bounds(a, y1 - 1, &lo, &n, &c);
    *r1 = lo + n;
}

// ---- Pillow's pixel arithmetic: luma() and blend() of pil_pixel.h ----
// jitter steps [0, n) of the sample's order; contrast blends towards `cmean`
__device__ inline void jitter(const uvit_augment_desc& d, int n, int cmean, int& r, int& g, int& b) {
    for (int i = 0; i < n; ++i) {
        const float f = d.jitter_factor[i];
        int dr = 0, dg = 0, db = 0;                                       // brightness: black
        if (d.jitter_op[i] == UVIT_AUG_CONTRAST) {
            dr = dg = db = cmean;
        } else if (d.jitter_op[i] == UVIT_AUG_SATURATION) {
            dr = dg = db = luma(r, g, b);
        }
        r = blend(dr, r, f);
        g = blend(dg, g, f);
        b = blend(db, b, f);
    }
}

__device__ inline int contrast_pos(const uvit_augment_desc& d) {
    for (int i = 0; i < d.n_jitter; ++i)
        if (d.jitter_op[i] == UVIT_AUG_CONTRAST) return i;
    return -1;
}

__device__ inline int clip8(int acc) {
    acc >>= PRECISION_BITS;
    return acc < 0 ? 0 : acc > 255 ? 255 : acc;
}

// ---- kernels ----
__global__ void __launch_bounds__(AUG_THREADS) aug_contrast_sum(const uint8_t* __restrict__ px, const uvit_augment_desc* __restrict__ desc,
                                                                unsigned long long* __restrict__ sums) {
    const uvit_augment_desc& d = desc[blockIdx.y];
    const int cpos = contrast_pos(d);
    if (cpos < 0) return;
    const int64_t n = (int64_t)d.h * d.w;
    const uint8_t* img = px + d.offset;
    unsigned long long s = 0;
    for (int64_t p = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * AUG_THREADS) {
        int r = img[3 * p], g = img[3 * p + 1], b = img[3 * p + 2];
        jitter(d, cpos, 0, r, g, b);
        s += (unsigned long long)luma(r, g, b);
    }
    __shared__ unsigned long long red[AUG_THREADS];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = AUG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicAdd(&sums[blockIdx.y], red[0]);
}

// table[b][axis][o] = {xmin, xlen, k[0..kmax)}: taps of window position o (axis 0: columns, 1: rows; xmin in crop coordinates).
// xlen = 0 where the position lies outside the resized image or the axis is not resampled.
__global__ void __launch_bounds__(AUG_THREADS) aug_coeffs(const uvit_augment_desc* __restrict__ desc, int32_t* __restrict__ table, int S,
                                                          int kmax) {
    const int o = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (o >= S) return;
    const int b = blockIdx.y, axis = blockIdx.z;
    const uvit_augment_desc& d = desc[b];
    int32_t* e = table + (((int64_t)b * 2 + axis) * S + o) * (2 + kmax);
    const int in_size = axis ? d.crop_h : d.crop_w, out_size = axis ? d.resize_h : d.resize_w;
    const int pos = (axis ? d.win_y : d.win_x) + o;
    e[0] = 0;
    e[1] = 0;
    if (in_size == out_size || pos < 0 || pos >= out_size) return;
    const Axis a = make_axis(in_size, out_size, d.filter);
    int xmin, xlen;
    double center;
    axis_bounds(a, pos, &xmin, &xlen, &center);
    if (xlen > kmax) xlen = kmax;    // never: kmax >= ksize >= xlen (host-side sizing); keeps the table write in bounds
    double ww = 0.0;
    for (int x = 0; x < xlen; ++x) ww += filt_eval(d.filter, (x + xmin - center + 0.5) * a.ss);
    for (int x = 0; x < xlen; ++x) {
        double k = filt_eval(d.filter, (x + xmin - center + 0.5) * a.ss);
        if (ww != 0.0) k /= ww;
        e[2 + x] = k < 0 ? (int)(-0.5 + k * (1 << PRECISION_BITS)) : (int)(0.5 + k * (1 << PRECISION_BITS));
    }
    e[0] = xmin;
    e[1] = xlen;
}

// temp[b][r][o] (RGB packed in 32 bits) = horizontal pass of crop row r0 + r at window column o, jitter applied on load.
__global__ void __launch_bounds__(AUG_THREADS) aug_hpass(const uint8_t* __restrict__ px, const uvit_augment_desc* __restrict__ desc,
                                                         const unsigned long long* __restrict__ sums, const int32_t* __restrict__ table,
                                                         uint32_t* __restrict__ temp, int S, int kmax, int rows_cap) {
    const int b = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x;
    const int r = (int)(t / S), o = (int)(t % S);
    const uvit_augment_desc& d = desc[b];
    int r0, r1;
    row_range(d, S, &r0, &r1);
    if (r1 - r0 > rows_cap) r1 = r0 + rows_cap;
    const int pos = d.win_x + o;
    if (r >= r1 - r0 || pos < 0 || pos >= d.resize_w) return;
    int cmean = 0;
    if (contrast_pos(d) >= 0) {
        const double mean = (double)sums[b] / (double)((int64_t)d.h * d.w);      // ImageStat: sum / count
        cmean = (int)(mean + 0.5);
    }
    const uint8_t* row = px + d.offset + ((int64_t)(d.crop_y + r0 + r) * d.w) * 3;
    auto load = [&](int x, int& R, int& G, int& B) {   // x: column of the crop
        int sx = d.crop_x + x;
        if (d.flip) sx = d.w - 1 - sx;
        R = row[3 * sx];
        G = row[3 * sx + 1];
        B = row[3 * sx + 2];
        jitter(d, d.n_jitter, cmean, R, G, B);
    };
    int R, G, B;
    if (need_h(d)) {
        const int32_t* e = table + ((int64_t)b * 2 * S + o) * (2 + kmax);
        const int xmin = e[0], xlen = e[1];
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int x = 0; x < xlen; ++x) {
            int pr, pg, pb;
            load(xmin + x, pr, pg, pb);
            const int k = e[2 + x];
            s0 += pr * k;
            s1 += pg * k;
            s2 += pb * k;
        }
        R = clip8(s0);
        G = clip8(s1);
        B = clip8(s2);
    } else {
        load(pos, R, G, B);
    }
    temp[((int64_t)b * rows_cap + r) * S + o] = (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
}

__global__ void __launch_bounds__(AUG_THREADS) aug_vpass(const uvit_augment_desc* __restrict__ desc, const int32_t* __restrict__ table,
                                                         const uint32_t* __restrict__ temp, float* __restrict__ out, int S, int kmax,
                                                         int rows_cap, float m0, float m1, float m2, float sd0, float sd1, float sd2) {
    const int b = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * AUG_THREADS + threadIdx.x;
    if (t >= (int64_t)S * S) return;
    const int oy = (int)(t / S), ox = (int)(t % S);
    const uvit_augment_desc& d = desc[b];
    const int py = d.win_y + oy, pxx = d.win_x + ox;
    int R = 0, G = 0, B = 0;                                            // CenterCrop's padding
    if (py >= 0 && py < d.resize_h && pxx >= 0 && pxx < d.resize_w) {
        int r0, r1;
        row_range(d, S, &r0, &r1);
        const int rows = r1 - r0 < rows_cap ? r1 - r0 : rows_cap;
        const uint32_t* col = temp + (int64_t)b * rows_cap * S + ox;
        if (need_v(d)) {
            const int32_t* e = table + (((int64_t)b * 2 + 1) * S + oy) * (2 + kmax);
            const int ymin = e[0] - r0, ylen = e[1];
            int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
            for (int y = 0; y < ylen; ++y) {
                const int ri = ymin + y;
                if (ri < 0 || ri >= rows) continue;   // never: [r0, r1) covers every tap (row_range)
                const uint32_t v = col[(int64_t)ri * S];
                const int k = e[2 + y];
                s0 += (int)(v & 255) * k;
                s1 += (int)((v >> 8) & 255) * k;
                s2 += (int)((v >> 16) & 255) * k;
            }
            R = clip8(s0);
            G = clip8(s1);
            B = clip8(s2);
        } else {
            const int ri = py - r0;
            if (ri >= 0 && ri < rows) {
                const uint32_t v = col[(int64_t)ri * S];
                R = v & 255;
                G = (v >> 8) & 255;
                B = (v >> 16) & 255;
            }
        }
    }
    // ToTensor: u8 / 255; Normalize: (x - mean) / std -- float32, IEEE division
    const int64_t plane = (int64_t)S * S;
    float* o = out + (int64_t)b * 3 * plane + (int64_t)oy * S + ox;
    o[0] = ((float)R / 255.0f - m0) / sd0;
    o[plane] = ((float)G / 255.0f - m1) / sd1;
    o[2 * plane] = ((float)B / 255.0f - m2) / sd2;
}

// ---- host side: validation and workspace plan ----
struct Plan {
    int kmax, rows_cap;
    int64_t max_pixels;
    size_t off_sums, off_table, off_temp, bytes;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int check_desc(const uvit_augment_desc& d, int S) {
    if (d.h < 1 || d.w < 1 || d.h > MAX_SIDE || d.w > MAX_SIDE || d.offset < 0) return UVIT_ERR_SHAPE;
    if (d.crop_w < 1 || d.crop_h < 1 || d.crop_x < 0 || d.crop_y < 0 || d.crop_x > d.w - d.crop_w || d.crop_y > d.h - d.crop_h)
        return UVIT_ERR_SHAPE;
    if (d.resize_w < 1 || d.resize_h < 1 || d.resize_w > MAX_SIDE || d.resize_h > MAX_SIDE) return UVIT_ERR_SHAPE;
    if (d.win_x < -MAX_SIDE || d.win_y < -MAX_SIDE || d.win_x > MAX_SIDE || d.win_y > MAX_SIDE) return UVIT_ERR_SHAPE;
    if (d.flip != 0 && d.flip != 1) return UVIT_ERR_ARG;
    if (d.filter != UVIT_AUG_BILINEAR && d.filter != UVIT_AUG_BICUBIC && d.filter != UVIT_AUG_HAMMING && d.filter != UVIT_AUG_LANCZOS)
        return UVIT_ERR_ARG;
    if (d.n_jitter < 0 || d.n_jitter > 3) return UVIT_ERR_ARG;
    for (int i = 0; i < d.n_jitter; ++i) {
        if (d.jitter_op[i] < UVIT_AUG_BRIGHTNESS || d.jitter_op[i] > UVIT_AUG_SATURATION || !std::isfinite(d.jitter_factor[i])) return UVIT_ERR_ARG;
        for (int j = 0; j < i; ++j)
            if (d.jitter_op[j] == d.jitter_op[i]) return UVIT_ERR_ARG;
    }
    (void)S;
    return UVIT_OK;
}

int make_plan(const uvit_augment_desc* desc, int B, int S, Plan* p) {
    if (!desc || B < 1 || S < 1 || S > 4096) return UVIT_ERR_ARG;
    p->kmax = 1;
    p->rows_cap = 1;
    p->max_pixels = 1;
    for (int b = 0; b < B; ++b) {
        const uvit_augment_desc& d = desc[b];
        const int rc = check_desc(d, S);
        if (rc) return rc;
        if (need_h(d)) p->kmax = std::max(p->kmax, make_axis(d.crop_w, d.resize_w, d.filter).ksize);
        if (need_v(d)) p->kmax = std::max(p->kmax, make_axis(d.crop_h, d.resize_h, d.filter).ksize);
        int r0, r1;
        row_range(d, S, &r0, &r1);
        p->rows_cap = std::max(p->rows_cap, r1 - r0);
        p->max_pixels = std::max(p->max_pixels, (int64_t)d.h * d.w);
    }
    p->off_sums = align256((size_t)B * sizeof(uvit_augment_desc));
    p->off_table = p->off_sums + align256((size_t)B * sizeof(unsigned long long));
    p->off_temp = p->off_table + align256((size_t)B * 2 * S * (2 + p->kmax) * sizeof(int32_t));
    p->bytes = p->off_temp + align256((size_t)B * p->rows_cap * S * sizeof(uint32_t));
    return UVIT_OK;
}

}  // namespace

extern "C" int64_t uvit_op_augment_ws_bytes(const uvit_augment_desc* desc, int B, int S) {
    Plan p;
    const int rc = make_plan(desc, B, S, &p);
    return rc ? rc : (int64_t)p.bytes;
}

extern "C" int uvit_op_augment_batch(const uint8_t* pixels, int64_t pixel_bytes, const uvit_augment_desc* desc, int B, int S,
                                     const float* mean, const float* stdv, float* out, void* workspace, int64_t ws_bytes,
                                     uvit_stream stream) {
    if (!pixels || !mean || !stdv || !out || !workspace || pixel_bytes < 0) return UVIT_ERR_ARG;
    Plan p;
    const int rc = make_plan(desc, B, S, &p);
    if (rc) return rc;
    for (int b = 0; b < B; ++b)
        if (desc[b].offset > pixel_bytes - (int64_t)desc[b].h * desc[b].w * 3) return UVIT_ERR_SHAPE;
    if (ws_bytes < (int64_t)p.bytes) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uvit_augment_desc* ddesc = (uvit_augment_desc*)ws;
    unsigned long long* sums = (unsigned long long*)(ws + p.off_sums);
    int32_t* table = (int32_t*)(ws + p.off_table);
    uint32_t* temp = (uint32_t*)(ws + p.off_temp);
    if (hipMemcpyAsync(ddesc, desc, (size_t)B * sizeof(uvit_augment_desc), hipMemcpyHostToDevice, s) != hipSuccess) return UVIT_ERR_LAUNCH;
    if (hipMemsetAsync(sums, 0, (size_t)B * sizeof(unsigned long long), s) != hipSuccess) return UVIT_ERR_LAUNCH;
    const int64_t sum_blocks = std::min<int64_t>((p.max_pixels + AUG_THREADS * 16 - 1) / (AUG_THREADS * 16), 256);
    aug_contrast_sum<<<dim3((unsigned)sum_blocks, B), AUG_THREADS, 0, s>>>(pixels, ddesc, sums);
    aug_coeffs<<<dim3((S + AUG_THREADS - 1) / AUG_THREADS, B, 2), AUG_THREADS, 0, s>>>(ddesc, table, S, p.kmax);
    const int64_t hthreads = (int64_t)p.rows_cap * S;
    aug_hpass<<<dim3((unsigned)((hthreads + AUG_THREADS - 1) / AUG_THREADS), B), AUG_THREADS, 0, s>>>(pixels, ddesc, sums, table, temp, S,
                                                                                                      p.kmax, p.rows_cap);
    const int64_t vthreads = (int64_t)S * S;
    aug_vpass<<<dim3((unsigned)((vthreads + AUG_THREADS - 1) / AUG_THREADS), B), AUG_THREADS, 0, s>>>(
        ddesc, table, temp, out, S, p.kmax, p.rows_cap, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
    return uvit_check_launch();
}
