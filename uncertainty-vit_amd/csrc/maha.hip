// Mahalanobis and relative Mahalanobis out-of-distribution scores of the probe's pooled feature f (gfx950), DESIGN.md section 9.10.
//   accumulate   S += sum_b f_b f_b^T (C, C)   class_sum[y_b] += f_b (K, C)   total_sum += f_b (C)   class_count[y_b] += 1
//                sums += {rows used, rows skipped}                                         over the usable rows of one batch
//   scores       g = W f, g0 = W0 f   (W = L^-1, W0 = L0^-1 of the host's Cholesky factors: lower triangular)
//                d_k = sum_c (g_c - Wmu[k, c])^2      maha = min_k d_k over the classes with a row, pred = its index
//                d_0 = sum_c (g0_c - Wmu0[c])^2       rmaha = maha - d_0
// All arithmetic is double on fp32 inputs widened.  No float atomics: every sum has one owner and a fixed order (ascending index, then
// the xor tree where a wave meets), so the same sequence of batches gives the same bits.  Plain v_fma_f64 tiles, as laplace.hip's: the
// part's vector and matrix fp64 rates are equal, and the distance is a sum of squared differences, which no matrix instruction forms
// (the expanded |g|^2 - 2 g.m + |m|^2 cancels), so v_mfma_f64_16x16x4_f64 could serve the whitening alone.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums is part of the contract and rows are screened with isfinite.
#ifdef __FAST_MATH__
#error "maha.hip fixes the order of its sums and tests for non-finite values: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"
#include "gram.h"

#define MAHA_MAX_B 65535
#define MAHA_MAX_C 2048
#define MAHA_MAX_K 4096

// ---- accumulate, launch 1: eff[b] = the label of a usable row, -1 for a row with a non-finite feature or a label outside [0, K) ----
__global__ __launch_bounds__(256)
void maha_screen_kernel(const float* __restrict__ feat, const int64_t* __restrict__ labels, int* __restrict__ eff, int B, int C, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* f = feat + (size_t)b * C;
    const int64_t y = labels[b];
    int bad = label_ok(y, K) ? 0 : 1;
    for (int c = lane; c < C; c += 64)
        if (!isfinite(f[c])) bad = 1;
    bad = __any(bad);
    if (lane == 0) eff[b] = bad ? -1 : (int)y;
}

// ---- accumulate, launch 2: S += X^T X with X = the usable rows of feat (zero rows otherwise) ----
// The reduction of laplace.hip's A factor without its column of ones (gram.h): S_ij is one fma chain over b in ascending order, (i, j)
// and (j, i) are formed from the same products in the same order and added to the old value by the same expression, so S stays
// symmetric bit for bit.
__global__ __launch_bounds__(256)
void maha_gram_kernel(const float* __restrict__ feat, const int* __restrict__ eff, double* __restrict__ out, int B, int C) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int j0 = blockIdx.x * GRAM_T, i0 = blockIdx.y * GRAM_T;
    double acc[4][4] = {}, none[4] = {};
    gram_tile<false>([&](int b, int col) { return (b >= B || col >= C || eff[b] < 0) ? 0.0 : (double)feat[(size_t)b * C + col]; }, B, i0, j0,
                     acc, none);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = i0 + ty * 4 + i;
        if (r >= C) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = j0 + tx * 4 + j;
            if (c >= C) continue;
            double* dst = out + (size_t)r * C + c;
            *dst = *dst + acc[i][j];
        }
    }
}

// ---- accumulate, launch 3: the class sums, the total, the counts; one owner per (k, c) walking b in ascending order ----
// blockIdx.y = k < K owns class k, blockIdx.y = K the total over every usable row and the two counters of `sums`.  eff[b] is the same
// for the whole workgroup (a scalar load), and a row of feat is read only by the workgroups of its class and of the total.
__global__ __launch_bounds__(256)
void maha_class_kernel(const float* __restrict__ feat, const int* __restrict__ eff, double* __restrict__ class_sum,
                       double* __restrict__ total_sum, double* __restrict__ class_count, double* __restrict__ sums, int B, int C, int K) {
    const int c = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    double s = 0.0;
    int n = 0;
    for (int b = 0; b < B; ++b) {
        const int e = eff[b];
        if (k < K ? e != k : e < 0) continue;
        ++n;
        if (c < C) s += (double)feat[(size_t)b * C + c];
    }
    if (c == 0) {
        if (k < K) class_count[k] = class_count[k] + (double)n;          // whole numbers below 2^53: exact
        else { sums[0] = sums[0] + (double)n; sums[1] = sums[1] + (double)(B - n); }
    }
    if (n == 0 || c >= C) return;                         // nothing of this class in the batch: its sums keep their bits
    double* dst = (k < K ? class_sum + (size_t)k * C : total_sum) + c;
    *dst = *dst + s;
}

// ---- scores, launches 1 and 2: out (M, N) from X (M, R) and Bm (N, R), both with the reduction index contiguous ----
// MODE 0 (whitening): X = feat fp32, Bm = W (blockIdx.z = 0) or W0 (1), out[m, n] = sum_r X[m, r] Bm[n, r] = (W f)_n.  W is lower
//         triangular with exact zeros above the diagonal, so the chain of column n ends behind r = n: a tile walks r < n0 + VN only
//         (inside the diagonal tile the zeros are read and add exact zeros), and the tiles with the longest chains start first.
// MODE 1 (distances): X = the whitened rows (double), Bm = Wmu, out[m, n] = sum_r (X[m, r] - Bm[n, r])^2.
// A workgroup of 256 threads owns 16 rows x 32 columns, a thread 1 x 2 of them: at B = 128, C = 768, K = 1000 that is 2 x 192 and 256
// workgroups of four waves.  The launch is bound by latency, not by arithmetic: the same tile with 128 threads and 2 x 2 outputs per
// thread (8 instead of 12 bytes of LDS reads per FMA, half the waves) measured 19 % slower, and 16 to 128 reduction steps per LDS tile measured
// alike (profiles/maha_tile_ab.json).  Every element is one chain over r in ascending order; rows, columns and steps past the edges
// are staged as zeros and add exact zeros.  The next tile's global loads are issued before the current tile's arithmetic, and all
// LDS fragments of a tile are requested before the first is used.
#define VM 16
#define VN 32
#define VK 16                // reduction steps per LDS tile
#define VT 256               // threads: 16 rows x 16 column pairs
#define VBQ (VN * VK / VT)   // staged elements of Bm per thread (X: one)
template <int MODE>
__global__ __launch_bounds__(VT)
void maha_mm_kernel(const float* __restrict__ feat, const double* __restrict__ X0, const double* B0, const double* B1,
                    double* out0, double* out1, int64_t ld, int M, int R, int N) {
    __shared__ __attribute__((aligned(16))) double Xs[VK][VM + 2], Bs[VK][VN + 2];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = (gridDim.x - 1 - blockIdx.x) * VN, m0 = blockIdx.y * VM;
    const double* __restrict__ Bm = blockIdx.z ? B1 : B0;
    double* __restrict__ out = blockIdx.z ? out1 : out0;
    const int rend = MODE == 0 ? min(R, n0 + VN) : R;
    const int sr = tid % VK, sq = tid / VK;               // staging: reduction step (adjacent lanes, adjacent r), row or column
    double xv, bv[VBQ];
    auto load = [&](int r0) {
        const int m = m0 + sq, r = r0 + sr;
        xv = (m < M && r < R) ? (MODE == 0 ? (double)feat[(size_t)m * R + r] : X0[(size_t)m * R + r]) : 0.0;
#pragma unroll
        for (int q = 0; q < VBQ; ++q) {
            const int n = n0 + sq + VM * q;
            bv[q] = (n < N && r < R) ? Bm[(size_t)n * R + r] : 0.0;
        }
    };
    double acc[2] = {};
    load(0);
    for (int r0 = 0; r0 < rend; r0 += VK) {
        __syncthreads();
        Xs[sr][sq] = xv;
#pragma unroll
        for (int q = 0; q < VBQ; ++q) Bs[sr][sq + VM * q] = bv[q];
        __syncthreads();
        if (r0 + VK < rend) load(r0 + VK);
        double xf[VK];
        double2 wf[VK];
#pragma unroll
        for (int r = 0; r < VK; ++r) { xf[r] = Xs[r][ty]; wf[r] = *(const double2*)&Bs[r][tx * 2]; }
#pragma unroll
        for (int r = 0; r < VK; ++r) {
            if (MODE == 0) {
                acc[0] = fma(xf[r], wf[r].x, acc[0]); acc[1] = fma(xf[r], wf[r].y, acc[1]);
            } else {
                const double d0 = xf[r] - wf[r].x, d1 = xf[r] - wf[r].y;
                acc[0] = fma(d0, d0, acc[0]); acc[1] = fma(d1, d1, acc[1]);
            }
        }
    }
    const int m = m0 + ty;
    if (m >= M) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + tx * 2 + j;
        if (n < N) out[(size_t)m * ld + n] = acc[j];
    }
}

// ---- scores, launch 3: one wave per row ----
// d_0 from the background's whitened row (lane partial sums over ascending c, the xor tree), the minimum of the row's d_k over the
// classes with a row (the lowest index on ties; a NaN distance never wins) and the three outputs, each rounded to its type once.  A
// row with a non-finite feature gets NaN, NaN, -1 and a row of NaN in `dist`.  With labels and `correct`, the rows whose pred equals
// their label are counted (an integer atomic: whole numbers, any order).
__global__ __launch_bounds__(256)
void maha_rows_kernel(const float* __restrict__ feat, const double* __restrict__ g0, const double* __restrict__ Wmu0,
                      const double* __restrict__ class_count, double* d, int64_t ld, int write_nan, float* __restrict__ maha,
                      float* __restrict__ rmaha, int* __restrict__ pred, const int64_t* __restrict__ labels, int* __restrict__ correct,
                      int B, int C, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* f = feat + (size_t)b * C;
    int bad = 0;
#pragma unroll 4                                          // four loads in flight per lane: a wave per row has nothing else to hide them
    for (int c = lane; c < C; c += 64) bad |= !isfinite(f[c]);
    bad = __any(bad);
    double* dr = d + (size_t)b * ld;
    if (bad) {
        if (write_nan)
            for (int k = lane; k < K; k += 64) dr[k] = NAN;
        if (lane == 0) { maha[b] = NAN; rmaha[b] = NAN; pred[b] = -1; }
        return;
    }
    const double* g = g0 + (size_t)b * C;
    double s0 = 0.0;
#pragma unroll 4
    for (int c = lane; c < C; c += 64) {
        const double t = g[c] - Wmu0[c];
        s0 = fma(t, t, s0);
    }
    s0 = wave_sum(s0);
    double best = INFINITY;
    int at = K;                                           // K: no class with a row and a comparable distance seen yet
#pragma unroll 4
    for (int k = lane; k < K; k += 64) {
        const double n = class_count[k], v = dr[k];
        if (n > 0.0 && (v < best || (at == K && v == best))) { best = v; at = k; }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double ob = __shfl_xor(best, s, 64);
        const int oa = __shfl_xor(at, s, 64);
        if (oa < K && (at == K || ob < best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    if (lane == 0) {
        if (at == K) { maha[b] = NAN; rmaha[b] = NAN; pred[b] = -1; return; }
        maha[b] = (float)best;
        rmaha[b] = (float)(best - s0);
        pred[b] = at;
        if (labels && correct && labels[b] == (int64_t)at) atomicAdd(correct, 1);
    }
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool maha_bad_ck(int C, int K) { return C < 4 || (C % 4) || C > MAHA_MAX_C || K < 2 || K > MAHA_MAX_K; }
static inline bool maha_bad_b(int B) { return B < 1 || B > MAHA_MAX_B; }

// workspace of uvit_op_maha_accumulate: the rows' effective labels (B) int32, padded to 16 bytes
extern "C" int64_t uvit_op_maha_accumulate_ws_bytes(int B, int C, int K) {
    if (maha_bad_b(B) || maha_bad_ck(C, K)) return UVIT_ERR_SHAPE;
    return align16((int64_t)B * 4);
}

extern "C" int uvit_op_maha_accumulate(const float* feat, const int64_t* labels, double* S, double* class_sum, double* total_sum,
                                       double* class_count, double* sums, void* ws, int64_t ws_bytes, int B, int C, int K,
                                       uvit_stream stream) {
    if (!feat || !labels || !S || !class_sum || !total_sum || !class_count || !sums || !ws) return UVIT_ERR_ARG;
    if (misaligned(feat, 4) || misaligned(labels, 8) || misaligned(S, 8) || misaligned(class_sum, 8) || misaligned(total_sum, 8) ||
        misaligned(class_count, 8) || misaligned(sums, 8) || misaligned(ws, 16))
        return UVIT_ERR_ARG;
    if (maha_bad_b(B) || maha_bad_ck(C, K)) return UVIT_ERR_SHAPE;
    if (ws_bytes < uvit_op_maha_accumulate_ws_bytes(B, C, K)) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int* eff = (int*)ws;
    const int tg = (C + GRAM_T - 1) / GRAM_T;
    hipLaunchKernelGGL(maha_screen_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, feat, labels, eff, B, C, K);
    hipLaunchKernelGGL(maha_gram_kernel, dim3(tg, tg), dim3(256), 0, s, feat, (const int*)eff, S, B, C);
    hipLaunchKernelGGL(maha_class_kernel, dim3((C + 255) / 256, K + 1), dim3(256), 0, s, feat, (const int*)eff, class_sum, total_sum,
                       class_count, sums, B, C, K);
    return uvit_check_launch();
}

// workspace of uvit_op_maha_scores: W f (B, C) double | W0 f (B, C) double | the distances (B, K) double (used when dist is NULL)
extern "C" int64_t uvit_op_maha_scores_ws_bytes(int B, int C, int K) {
    if (maha_bad_b(B) || maha_bad_ck(C, K)) return UVIT_ERR_SHAPE;
    return ((int64_t)B * C * 2 + (int64_t)B * K) * 8;
}

extern "C" int uvit_op_maha_scores(const float* feat, const double* W, const double* W0, const double* Wmu, const double* Wmu0,
                                   const double* class_count, float* maha, float* rmaha, int32_t* pred, double* dist, int64_t ld,
                                   const int64_t* labels, int32_t* correct, void* ws, int64_t ws_bytes, int B, int C, int K,
                                   uvit_stream stream) {
    if (!feat || !W || !W0 || !Wmu || !Wmu0 || !class_count || !maha || !rmaha || !pred || !ws) return UVIT_ERR_ARG;
    if (misaligned(feat, 4) || misaligned(W, 8) || misaligned(W0, 8) || misaligned(Wmu, 8) || misaligned(Wmu0, 8) || misaligned(class_count, 8) ||
        misaligned(maha, 4) || misaligned(rmaha, 4) || misaligned(pred, 4) || misaligned(dist, 8) || misaligned(labels, 8) || misaligned(correct, 4) ||
        misaligned(ws, 16))
        return UVIT_ERR_ARG;
    if (maha_bad_b(B) || maha_bad_ck(C, K) || (dist && ld < K)) return UVIT_ERR_SHAPE;
    if (ws_bytes < uvit_op_maha_scores_ws_bytes(B, C, K)) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* g = (double*)ws;
    double* g0 = g + (size_t)B * C;
    double* d = dist ? dist : g0 + (size_t)B * C;
    const int64_t ldd = dist ? ld : K;
    const int tm = (B + VM - 1) / VM;
    hipLaunchKernelGGL((maha_mm_kernel<0>), dim3((C + VN - 1) / VN, tm, 2), dim3(VT), 0, s, feat, (const double*)nullptr, W, W0, g, g0,
                       (int64_t)C, B, C, C);
    hipLaunchKernelGGL((maha_mm_kernel<1>), dim3((K + VN - 1) / VN, tm, 1), dim3(VT), 0, s, (const float*)nullptr, (const double*)g, Wmu,
                       Wmu, d, d, ldd, B, C, K);
    hipLaunchKernelGGL(maha_rows_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, feat, (const double*)g0, Wmu0, class_count, d, ldd,
                       dist ? 1 : 0, maha, rmaha, pred, labels, correct, B, C, K);
    return uvit_check_launch();
}
