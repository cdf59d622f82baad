// Post-hoc last-layer K-FAC Laplace approximation of the linear probe head (gfx950), DESIGN.md section 9.9.  With phi = [f, 1]
// (D = C + 1 entries), z = W f + b, p = softmax(z):
//   factors    A += sum_b phi_b phi_b^T (D, D)   G_sum += sum_b (diag(p_b) - p_b p_b^T) (K, K)   sums += {nll, rows used, rows skipped}
//   prepare    T[i, k] = sum_j U_G[k, j]^2 / (lam_A[i] lam_G[j] + tau) (D, K)      from the host's eigen-decompositions of A and G
//   variance   a = phi U_A;  var[b, k] = sum_i a_bi^2 T[i, k]                      = diag(J (G (x) A + tau I)^-1 J^T), J = I_K (x) phi^T
//   probit     out[b, k] = z[b, k] / sqrt(1 + factor var[b, k]);  lap_var[b] = var[b, argmax_k z[b, k]]
// All arithmetic is double on fp32 inputs widened.  No float atomics: every sum has one owner and a fixed order (ascending index, then
// the xor tree where a wave meets), so the same input gives the same bits on every run.  These are LDS-tiled v_fma_f64 kernels: the
// part's vector and matrix fp64 rates are equal, and small output tiles keep all compute units busy at a batch of 128 rows.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums is part of the contract, rows are screened with isfinite and the
// softmax needs the accurate double exp / log.
#ifdef __FAST_MATH__
#error "laplace.hip fixes the order of its sums, tests for non-finite values and needs the accurate exp / log: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"
#include "gram.h"

#define LAP_MAX_B 65535
#define LAP_MAX_C 2048
#define LAP_MAX_K 4096

// ---- factors, launch 1: the double max-shifted softmax of every row, its NLL and whether the row is used; one wave per row ----
// A row with a non-finite logit or a label outside [0, K) gets p = 0, nll = 0 and used = 0: it then adds exact zeros to every sum.
__global__ __launch_bounds__(256)
void lap_softmax_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, double* __restrict__ p,
                        double* __restrict__ row_nll, int* __restrict__ used, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* z = logits + (size_t)b * ld;
    double* pr = p + (size_t)b * K;
    const int64_t y = labels[b];
    int bad = label_ok(y, K) ? 0 : 1;
    double m = -INFINITY;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        if (!isfinite(v)) bad = 1;
        m = fmax(m, (double)v);
    }
    bad = __any(bad);
    if (bad) {
        for (int k = lane; k < K; k += 64) pr[k] = 0.0;
        if (lane == 0) { row_nll[b] = 0.0; used[b] = 0; }
        return;
    }
    m = wave_max(m);
    double s = 0.0;
    for (int k = lane; k < K; k += 64) {
        const double e = exp((double)z[k] - m);
        pr[k] = e;
        s += e;
    }
    s = wave_sum(s);                                  // every lane holds the same bits: a + b == b + a at every level
    for (int k = lane; k < K; k += 64) pr[k] = pr[k] / s;  // a lane reads back what it wrote
    if (lane == 0) { row_nll[b] = log(s) - ((double)z[y] - m); used[b] = 1; }
}

// ---- factors, launches 2 and 3: X^T X over the batch, added into a (N, N) double matrix in place ----
// MODE 0: X = phi = [f, 1] of the used rows (zero rows otherwise), N = C + 1, out = A:      A_ij += S_ij
// MODE 1: X = p (zero in the rows left out), N = K, out = G_sum:                             G_kl += delta_kl sum_b p_bk - S_kl
// S_ij = one fma chain over b in ascending order.  (i, j) and (j, i) are formed from the same products (a * b == b * a) in the same
// order and combined with the old value by the same expression, so a symmetric matrix stays symmetric bit for bit.
#define FT GRAM_T            // output tile edge: 256 threads with a 4 x 4 micro-tile each (gram.h)
template <int MODE>
__device__ __forceinline__ double lap_x(const float* __restrict__ feat, const double* __restrict__ p, const int* __restrict__ used,
                                        int b, int col, int B, int C, int N) {
    if (b >= B || col >= N) return 0.0;
    if (MODE == 1) return p[(size_t)b * N + col];
    if (!used[b]) return 0.0;
    return col < C ? (double)feat[(size_t)b * C + col] : 1.0;
}

template <int MODE>
__global__ __launch_bounds__(256)
void lap_gram_kernel(const float* __restrict__ feat, const double* __restrict__ p, const int* __restrict__ used, double* __restrict__ out,
                     int B, int C, int N) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int j0 = blockIdx.x * FT, i0 = blockIdx.y * FT;
    double acc[4][4] = {}, si[4] = {};
    gram_tile<MODE == 1>([&](int b, int col) { return lap_x<MODE>(feat, p, used, b, col, B, C, N); }, B, i0, j0, acc, si);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = i0 + ty * 4 + i;
        if (r >= N) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = j0 + tx * 4 + j;
            if (c >= N) continue;
            double* dst = out + (size_t)r * N + c;
            if (MODE == 0) *dst = *dst + acc[i][j];
            else *dst = *dst + ((r == c ? si[i] : 0.0) - acc[i][j]);
        }
    }
}

// ---- factors, launch 4: sums += {sum of the rows' NLL, rows used, rows skipped}; one wave, lane partial sums over ascending b ----
__global__ __launch_bounds__(64)
void lap_sums_kernel(const double* __restrict__ row_nll, const int* __restrict__ used, double* __restrict__ sums, int B) {
    const int lane = threadIdx.x;
    double s = 0.0, n = 0.0;
    for (int b = lane; b < B; b += 64) {
        s += row_nll[b];
        n += (double)used[b];
    }
    s = wave_sum(s);
    n = wave_sum(n);                                  // whole numbers below 2^53: exact
    if (lane == 0) {
        sums[0] = sums[0] + s;
        sums[1] = sums[1] + n;
        sums[2] = sums[2] + ((double)B - n);
    }
}

// ---- prepare: T[i, k] = sum_j U_G[k, j]^2 / (lam_A[i] lam_G[j] + tau), j ascending, one owner per element ----
// A workgroup owns 16 rows i x 16 columns k and walks j in tiles of 64: U_G[k, j]^2 and lam_G[j] are staged in LDS.
#define PJ 64
__global__ __launch_bounds__(256)
void lap_prepare_kernel(const double* __restrict__ UG, const double* __restrict__ lamA, const double* __restrict__ lamG, double tau,
                        double* __restrict__ T, int D, int K) {
    __shared__ double u2[16][PJ + 1], lg[PJ];
    const int tid = threadIdx.x, tk = tid & 15, ti = tid >> 4;
    const int k0 = blockIdx.x * 16, i = blockIdx.y * 16 + ti;
    const double la = i < D ? lamA[i] : 0.0;
    double acc = 0.0;
    for (int j0 = 0; j0 < K; j0 += PJ) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {                     // 16 x 64 squares: row tid / 64 + 4 q, column tid % 64 (adjacent lanes, adjacent j)
            const int kk = (tid >> 6) + 4 * q, jj = tid & 63;
            const double u = (k0 + kk < K && j0 + jj < K) ? UG[(size_t)(k0 + kk) * K + j0 + jj] : 0.0;
            u2[kk][jj] = u * u;
        }
        if (tid < PJ) lg[tid] = j0 + tid < K ? lamG[j0 + tid] : 0.0;
        __syncthreads();
        const int nj = min(PJ, K - j0);
        for (int j = 0; j < nj; ++j) acc += u2[tk][j] / (la * lg[j] + tau);
    }
    if (i < D && k0 + tk < K) T[(size_t)i * K + k0 + tk] = acc;
}

// ---- variance: two small double GEMMs, out (M, N) = X (M, R) . Bm (R, N) with Bm row-major ----
// MODE 0: X = phi = [f, 1] (R = C + 1), Bm = U_A, out[b, i] = a_bi^2 (the square is taken once, here)
// MODE 1: X = the squares (R = D), Bm = T, out = var
// A workgroup of 128 threads owns 16 rows x 32 columns, a thread 2 x 2 of them: at B = 128, C = 768, K = 1000 that is 200 and 256
// workgroups, against the 26 and 32 of a 64 x 64 tile.  Every element is one fma chain over r in ascending order.  The next tile's
// global loads are issued before the current tile's arithmetic.  A tile holds 16 reduction steps: 32 and 64 steps per tile (fewer
// round trips to memory, 134 VGPRs) measured 8 % and 5 % slower (profiles/lap_variance_tile_ab.json), so the launch does not wait
// on its loads; what it pays is 8 bytes of LDS reads per FMA with two waves on a compute unit.
#define VM 16
#define VN 32
#ifndef LAP_VK
#define LAP_VK 16            // reduction steps per LDS tile; a multiple of 8 (-DLAP_VK=64 through UVIT_EXTRA_FLAGS for the A/B)
#endif
#define VK LAP_VK
#define VXQ (VM * VK / 128)  // staged elements of X per thread
#define VBQ (VN * VK / 128)  // staged elements of Bm per thread
template <int MODE>
__device__ __forceinline__ double lap_vx(const float* __restrict__ feat, const double* __restrict__ X, int m, int r, int M, int R) {
    if (m >= M || r >= R) return 0.0;
    if (MODE == 1) return X[(size_t)m * R + r];
    return r < R - 1 ? (double)feat[(size_t)m * (R - 1) + r] : 1.0;
}

template <int MODE>
__global__ __launch_bounds__(128)
void lap_mm_kernel(const float* __restrict__ feat, const double* __restrict__ X, const double* __restrict__ Bm, double* __restrict__ out,
                   int M, int R, int N) {
    __shared__ __attribute__((aligned(16))) double Xs[VK][VM + 2], Bs[VK][VN + 2];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * VN, m0 = blockIdx.y * VM;
    const int bn = tid & 31, br = tid >> 5;               // Bm staging: column, reduction row (and + 4, + 8, ...)
    double xv[VXQ], bv[VBQ];
    auto load = [&](int r0) {                             // X staging: element tid + 128 q of the (VM, VK) tile, adjacent lanes adjacent r
#pragma unroll
        for (int q = 0; q < VXQ; ++q) xv[q] = lap_vx<MODE>(feat, X, m0 + (tid + 128 * q) / VK, r0 + (tid + 128 * q) % VK, M, R);
#pragma unroll
        for (int q = 0; q < VBQ; ++q) {
            const int r = r0 + br + 4 * q;
            bv[q] = (r < R && n0 + bn < N) ? Bm[(size_t)r * N + n0 + bn] : 0.0;
        }
    };
    double acc[2][2] = {};
    load(0);
    for (int r0 = 0; r0 < R; r0 += VK) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < VXQ; ++q) Xs[(tid + 128 * q) % VK][(tid + 128 * q) / VK] = xv[q];
#pragma unroll
        for (int q = 0; q < VBQ; ++q) Bs[br + 4 * q][bn] = bv[q];
        __syncthreads();
        if (r0 + VK < R) load(r0 + VK);
#pragma unroll
        for (int r = 0; r < VK; ++r) {                    // rows past R hold zeros: fma(0, 0, acc) = acc
            const double2 x = *(const double2*)&Xs[r][ty * 2], w = *(const double2*)&Bs[r][tx * 2];
            acc[0][0] = fma(x.x, w.x, acc[0][0]); acc[0][1] = fma(x.x, w.y, acc[0][1]);
            acc[1][0] = fma(x.y, w.x, acc[1][0]); acc[1][1] = fma(x.y, w.y, acc[1][1]);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + ty * 2 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + tx * 2 + j;
            if (n < N) out[(size_t)m * N + n] = MODE == 0 ? acc[i][j] * acc[i][j] : acc[i][j];
        }
    }
}

// ---- probit: one wave per row; the arg-max of the unscaled logits (lowest index on ties) is taken before anything is written ----
__global__ __launch_bounds__(256)
void lap_probit_kernel(const float* logits, int64_t ld, const double* __restrict__ var, double factor, float* out, int64_t ld_out,
                       float* __restrict__ lap_var, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* z = logits + (size_t)b * ld;
    const double* v = var + (size_t)b * K;
    float* o = out + (size_t)b * ld_out;
    if (lap_var) {
        float best = -INFINITY;
        int at = K;                                       // K: no comparable logit seen yet
        for (int k = lane; k < K; k += 64) {
            const float x = z[k];
            if (x > best || (at == K && x == best)) { best = x; at = k; }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const float ob = __shfl_xor(best, s, 64);
            const int oa = __shfl_xor(at, s, 64);
            if (oa < K && (at == K || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
        }
        if (lane == 0) lap_var[b] = (float)v[at < K ? at : 0];
    }
    for (int k = lane; k < K; k += 64) {
        const double vk = v[k];
        const double den = vk >= 0.0 ? sqrt(1.0 + factor * vk) : NAN;      // a NaN or negative variance: NaN in this entry
        o[k] = (float)((double)z[k] / den);
    }
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool lap_bad_ck(int C, int K) { return C < 4 || (C % 4) || C > LAP_MAX_C || K < 2 || K > LAP_MAX_K; }
static inline bool lap_bad_b(int B) { return B < 1 || B > LAP_MAX_B; }

// workspace of uvit_op_lap_factors: p (B, K) double | row NLL (B) double | row used (B) int32, padded to 16 bytes
extern "C" int64_t uvit_op_lap_factors_ws_bytes(int B, int C, int K) {
    if (lap_bad_b(B) || lap_bad_ck(C, K)) return UVIT_ERR_SHAPE;
    return ((int64_t)B * K + B) * 8 + align16((int64_t)B * 4);
}

extern "C" int uvit_op_lap_factors(const float* feat, const float* logits, int64_t ld, const int64_t* labels, double* A, double* G,
                                   double* sums, void* ws, int64_t ws_bytes, int B, int C, int K, uvit_stream stream) {
    if (!feat || !logits || !labels || !A || !G || !sums || !ws) return UVIT_ERR_ARG;
    if (misaligned(feat, 4) || misaligned(logits, 4) || misaligned(labels, 8) || misaligned(A, 8) || misaligned(G, 8) || misaligned(sums, 8) || misaligned(ws, 16))
        return UVIT_ERR_ARG;
    if (lap_bad_b(B) || lap_bad_ck(C, K) || ld < K) return UVIT_ERR_SHAPE;
    if (ws_bytes < uvit_op_lap_factors_ws_bytes(B, C, K)) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* p = (double*)ws;
    double* row_nll = p + (size_t)B * K;
    int* used = (int*)(row_nll + B);
    const int D = C + 1, ta = (D + FT - 1) / FT, tg = (K + FT - 1) / FT;
    hipLaunchKernelGGL(lap_softmax_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, logits, ld, labels, p, row_nll, used, B, K);
    hipLaunchKernelGGL((lap_gram_kernel<0>), dim3(ta, ta), dim3(256), 0, s, feat, (const double*)nullptr, (const int*)used, A, B, C, D);
    hipLaunchKernelGGL((lap_gram_kernel<1>), dim3(tg, tg), dim3(256), 0, s, (const float*)nullptr, (const double*)p, (const int*)used, G, B,
                       C, K);
    hipLaunchKernelGGL(lap_sums_kernel, dim3(1), dim3(64), 0, s, (const double*)row_nll, (const int*)used, sums, B);
    return uvit_check_launch();
}

extern "C" int uvit_op_lap_prepare(const double* UG, const double* lamA, const double* lamG, double tau, double* T, int C, int K,
                                   uvit_stream stream) {
    if (!UG || !lamA || !lamG || !T || !(tau > 0.0) || !(tau < INFINITY)) return UVIT_ERR_ARG;
    if (misaligned(UG, 8) || misaligned(lamA, 8) || misaligned(lamG, 8) || misaligned(T, 8)) return UVIT_ERR_ARG;
    if (lap_bad_ck(C, K)) return UVIT_ERR_SHAPE;
    const int D = C + 1;
    hipLaunchKernelGGL(lap_prepare_kernel, dim3((K + 15) / 16, (D + 15) / 16), dim3(256), 0, (hipStream_t)stream, UG, lamA, lamG, tau, T,
                       D, K);
    return uvit_check_launch();
}

// workspace of uvit_op_lap_variance: the squares a^2 (B, C + 1) double
extern "C" int64_t uvit_op_lap_variance_ws_bytes(int B, int C, int K) {
    if (lap_bad_b(B) || lap_bad_ck(C, K)) return UVIT_ERR_SHAPE;
    return align16((int64_t)B * (C + 1) * 8);
}

extern "C" int uvit_op_lap_variance(const float* feat, const double* UA, const double* T, double* var, void* ws, int64_t ws_bytes, int B,
                                    int C, int K, uvit_stream stream) {
    if (!feat || !UA || !T || !var || !ws) return UVIT_ERR_ARG;
    if (misaligned(feat, 4) || misaligned(UA, 8) || misaligned(T, 8) || misaligned(var, 8) || misaligned(ws, 16)) return UVIT_ERR_ARG;
    if (lap_bad_b(B) || lap_bad_ck(C, K)) return UVIT_ERR_SHAPE;
    if (ws_bytes < uvit_op_lap_variance_ws_bytes(B, C, K)) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int D = C + 1, tm = (B + VM - 1) / VM;
    double* a2 = (double*)ws;
    hipLaunchKernelGGL((lap_mm_kernel<0>), dim3((D + VN - 1) / VN, tm), dim3(128), 0, s, feat, (const double*)nullptr, UA, a2, B, D, D);
    hipLaunchKernelGGL((lap_mm_kernel<1>), dim3((K + VN - 1) / VN, tm), dim3(128), 0, s, (const float*)nullptr, (const double*)a2, T, var, B,
                       D, K);
    return uvit_check_launch();
}

extern "C" int uvit_op_lap_probit(const float* logits, int64_t ld, const double* var, double factor, float* out, int64_t ld_out,
                                  float* lap_var, int B, int K, uvit_stream stream) {
    if (!logits || !var || !out || !(factor >= 0.0) || !(factor < INFINITY)) return UVIT_ERR_ARG;
    if (misaligned(logits, 4) || misaligned(var, 8) || misaligned(out, 4) || misaligned(lap_var, 4)) return UVIT_ERR_ARG;
    if (lap_bad_b(B) || K < 2 || K > LAP_MAX_K || ld < K || ld_out < K) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(lap_probit_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, (hipStream_t)stream, logits, ld, var, factor, out, ld_out, lap_var,
                       B, K);
    return uvit_check_launch();
}
