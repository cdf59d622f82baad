// ViM (virtual-logit matching, Wang et al., CVPR 2022) and residual out-of-distribution scores of the probe's pooled feature f (gfx950),
// DESIGN.md section 9.13.  The host stacks the null-space basis R (Cn, C) of the centred training features and the affine head (W, b)
// into one matrix and one vector, A = [R ; W] (Cn + K, C) and a = [-R o ; b] (Cn + K), so that one product serves both halves:
//   product      y = A f + a (B, Cn + K)          y[:, :Cn] = R (f - o), y[:, Cn:] = the logits z = W f + b
//   rows         residual = sqrt(sum_{j < Cn} y_j^2)      lse = max_k z_k + log(sum_k exp(z_k - max))      pred = arg max_k z_k
//                vim = fma(alpha, residual, -lse)
//   sums         {sum max_k z, sum residual, rows used, rows skipped} += over the usable rows of the batch (the fit's alpha)
// All arithmetic is double on fp32 features widened.  No float atomics: every sum has one owner and a fixed order (ascending index,
// then the xor tree where a wave meets), so the same batch gives the same bits and a row's outputs do not depend on its neighbours.
// Compiled WITHOUT -ffast-math (build.sh).  The IEEE properties this file relies on: the order of every sum is part of the contract
// (no reassociation), rows are screened with isfinite and answered with NaN (finite-math-only would fold both away), the arg max's
// tie rule compares doubles for equality, and exp / log / sqrt are the correctly specified library functions, not their approximate
// forms, because the tests hold the outputs to bounds of a few units in the last place.
#ifdef __FAST_MATH__
#error "vim.hip fixes the order of its sums, tests for non-finite values and answers them with NaN: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define VIM_MAX_B 65535
#define VIM_MAX_C 2048
#define VIM_MAX_K 4096

// ---- launch 1: y (M, N) = A f + a from feat (M, R) fp32 and A (N, R) double, both with the reduction index contiguous ----
// maha.hip's whitening tile without its triangular cut: a workgroup of 256 threads owns 16 rows x 32 columns, a thread 1 x 2 of them.
// At B = 128, C = 768, Cn + K = 1256 that is 8 x 40 = 320 workgroups of four waves, and the launch is bound by latency as maha's is
// (profiles/maha_tile_ab.json measured the alternatives of this tile on the same reduction length).  Every element is one fma chain
// over c in ascending order from zero, then one addition of a_n; rows, columns and steps past the edges are staged as zeros and add
// exact zeros.  The next tile's global loads are issued before the current tile's arithmetic, and all LDS fragments of a tile are
// requested before the first is used.
#define VM 16
#define VN 32
#define VK 16                // reduction steps per LDS tile
#define VT 256               // threads: 16 rows x 16 column pairs
#define VBQ (VN * VK / VT)   // staged elements of A per thread (feat: one)
__global__ __launch_bounds__(VT)
void vim_mm_kernel(const float* __restrict__ feat, const double* __restrict__ A, const double* __restrict__ a, double* __restrict__ y,
                   int M, int R, int N) {
    __shared__ __attribute__((aligned(16))) double Xs[VK][VM + 2], Bs[VK][VN + 2];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * VN, m0 = blockIdx.y * VM;
    const int sr = tid % VK, sq = tid / VK;               // staging: reduction step (adjacent lanes, adjacent r), row or column
    double xv, bv[VBQ];
    auto load = [&](int r0) {
        const int m = m0 + sq, r = r0 + sr;
        xv = (m < M && r < R) ? (double)feat[(size_t)m * R + r] : 0.0;
#pragma unroll
        for (int q = 0; q < VBQ; ++q) {
            const int n = n0 + sq + VM * q;
            bv[q] = (n < N && r < R) ? A[(size_t)n * R + r] : 0.0;
        }
    };
    double acc[2] = {};
    load(0);
    for (int r0 = 0; r0 < R; r0 += VK) {
        __syncthreads();
        Xs[sr][sq] = xv;
#pragma unroll
        for (int q = 0; q < VBQ; ++q) Bs[sr][sq + VM * q] = bv[q];
        __syncthreads();
        if (r0 + VK < R) load(r0 + VK);
        double xf[VK];
        double2 wf[VK];
#pragma unroll
        for (int r = 0; r < VK; ++r) { xf[r] = Xs[r][ty]; wf[r] = *(const double2*)&Bs[r][tx * 2]; }
#pragma unroll
        for (int r = 0; r < VK; ++r) { acc[0] = fma(xf[r], wf[r].x, acc[0]); acc[1] = fma(xf[r], wf[r].y, acc[1]); }
    }
    const int m = m0 + ty;
    if (m >= M) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + tx * 2 + j;
        if (n < N) y[(size_t)m * N + n] = acc[j] + a[n];
    }
}

// ---- launch 2: one wave per row ----
// residual from the first Cn entries of the row of y (lane partial sums over ascending j, the xor tree, one square root), then the
// arg max of the K logits behind them (the lowest class on ties; a NaN logit never wins), the sum of exp(z - max) in the same order
// and the three outputs, each rounded to its type once.  A row with a non-finite feature gets NaN, NaN, -1.  With labels and
// `correct`, the rows whose pred equals their label are counted (an integer atomic: whole numbers, any order).  With `rowmax`, the
// row's max_k z and residual are kept in double for launch 3 (pred < 0 marks a skipped row there).
__global__ __launch_bounds__(256)
void vim_rows_kernel(const float* __restrict__ feat, const double* __restrict__ y, double alpha, float* __restrict__ vim,
                     float* __restrict__ residual, int* __restrict__ pred, const int64_t* __restrict__ labels, int* __restrict__ correct,
                     double* __restrict__ rowmax, double* __restrict__ rowres, int B, int C, int Cn, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* f = feat + (size_t)b * C;
    int bad = 0;
#pragma unroll 4                                          // four loads in flight per lane: a wave per row has nothing else to hide them
    for (int c = lane; c < C; c += 64) bad |= !isfinite(f[c]);
    bad = __any(bad);
    if (bad) {
        if (lane == 0) { vim[b] = NAN; residual[b] = NAN; pred[b] = -1; }
        return;
    }
    const double* yr = y + (size_t)b * (Cn + K);
    const double* z = yr + Cn;
    double s = 0.0;
#pragma unroll 4
    for (int j = lane; j < Cn; j += 64) {
        const double t = yr[j];
        s = fma(t, t, s);
    }
    const double res = sqrt(wave_sum(s));
    double best = -INFINITY;
    int at = K;                                           // K: no comparable logit seen yet
#pragma unroll 4
    for (int k = lane; k < K; k += 64) {
        const double v = z[k];
        if (v > best || (at == K && v == best)) { best = v; at = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (oa < K && (at == K || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    double e = 0.0;
#pragma unroll 4
    for (int k = lane; k < K; k += 64) e += exp(z[k] - best);
    const double lse = best + log(wave_sum(e));
    if (lane == 0) {
        if (at == K) { vim[b] = NAN; residual[b] = NAN; pred[b] = -1; return; }      // every logit NaN: a non-finite A
        vim[b] = (float)fma(alpha, res, -lse);
        residual[b] = (float)res;
        pred[b] = at;
        if (rowmax) { rowmax[b] = best; rowres[b] = res; }
        if (labels && correct && labels[b] == (int64_t)at) atomicAdd(correct, 1);
    }
}

// ---- launch 3 (with `sums` only): one workgroup owns the four sums ----
// Thread t walks the rows t, t + 256, ... in ascending order, a wave adds its lanes by the xor tree, and thread 0 adds the four waves'
// values in wave order to the old value: a fixed order for every B.  The two counters are whole numbers below 2^53: exact.
__global__ __launch_bounds__(256)
void vim_sums_kernel(const int* __restrict__ pred, const double* __restrict__ rowmax, const double* __restrict__ rowres,
                     double* __restrict__ sums, int B) {
    __shared__ double part[4][3];
    const int tid = threadIdx.x;
    double sm = 0.0, sr = 0.0;
    int used = 0;
    for (int b = tid; b < B; b += 256) {
        if (pred[b] < 0) continue;
        sm += rowmax[b];
        sr += rowres[b];
        ++used;
    }
    sm = wave_sum(sm);
    sr = wave_sum(sr);
    used = wave_sum(used);
    if ((tid & 63) == 0) { part[tid >> 6][0] = sm; part[tid >> 6][1] = sr; part[tid >> 6][2] = (double)used; }
    __syncthreads();
    if (tid == 0) {
        double tm = part[0][0], tr = part[0][1], tu = part[0][2];
        for (int w = 1; w < 4; ++w) { tm += part[w][0]; tr += part[w][1]; tu += part[w][2]; }
        sums[0] = sums[0] + tm;
        sums[1] = sums[1] + tr;
        sums[2] = sums[2] + tu;
        sums[3] = sums[3] + ((double)B - tu);
    }
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool vim_bad_shape(int B, int C, int Cn, int K) {
    return B < 1 || B > VIM_MAX_B || C < 4 || (C % 4) || C > VIM_MAX_C || Cn < 1 || Cn > C - 1 || K < 2 || K > VIM_MAX_K;
}

// workspace of uvit_op_vim_scores: y (B, Cn + K) double | the rows' max logit (B) double | the rows' residual (B) double
extern "C" int64_t uvit_op_vim_scores_ws_bytes(int B, int C, int Cn, int K) {
    if (vim_bad_shape(B, C, Cn, K)) return UVIT_ERR_SHAPE;
    return align16(((int64_t)B * (Cn + K) + 2 * (int64_t)B) * 8);
}

extern "C" int uvit_op_vim_scores(const float* feat, const double* A, const double* a, double alpha, float* vim, float* residual,
                                  int32_t* pred, const int64_t* labels, int32_t* correct, double* sums, void* ws, int64_t ws_bytes,
                                  int B, int C, int Cn, int K, uvit_stream stream) {
    if (!feat || !A || !a || !vim || !residual || !pred || !ws) return UVIT_ERR_ARG;
    if (misaligned(feat, 4) || misaligned(A, 8) || misaligned(a, 8) || misaligned(vim, 4) || misaligned(residual, 4) || misaligned(pred, 4) ||
        misaligned(labels, 8) || misaligned(correct, 4) || misaligned(sums, 8) || misaligned(ws, 16))
        return UVIT_ERR_ARG;
    if (!(fabs(alpha) < INFINITY)) return UVIT_ERR_ARG;   // false for NaN and for +-inf
    if (vim_bad_shape(B, C, Cn, K)) return UVIT_ERR_SHAPE;
    if (ws_bytes < uvit_op_vim_scores_ws_bytes(B, C, Cn, K)) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int N = Cn + K;
    double* y = (double*)ws;
    double* rowmax = y + (size_t)B * N;
    double* rowres = rowmax + B;
    hipLaunchKernelGGL(vim_mm_kernel, dim3((N + VN - 1) / VN, (B + VM - 1) / VM), dim3(VT), 0, s, feat, A, a, y, B, C, N);
    hipLaunchKernelGGL(vim_rows_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, feat, (const double*)y, alpha, vim, residual, pred,
                       labels, correct, sums ? rowmax : (double*)nullptr, rowres, B, C, Cn, K);
    if (sums) hipLaunchKernelGGL(vim_sums_kernel, dim3(1), dim3(256), 0, s, (const int*)pred, (const double*)rowmax, (const double*)rowres, sums, B);
    return uvit_check_launch();
}
