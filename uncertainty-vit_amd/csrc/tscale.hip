// Post-hoc temperature scaling (Guo et al., 2017) fitted and applied on the device (gfx950).  DESIGN.md section 9.7.
//   uvit_op_ts_fit    the scalar s = 1 / T that minimises the mean NLL of softmax(s z) over a stored set of logits (N, K), by a
//                     bracketed Newton iteration that is enqueued whole and never reads back to the host
//   uvit_op_ts_scale  dst = (float)((double) src * s) with s read from the fit's device table
// With d_k = z_k - max_k z_k, at the point s:
//   f(s) = (1 / n) sum_i [ log sum_k exp(s d_ik) - s d_i,y ]     g = f' = (1 / n) sum_i [ sum_k p_ik d_ik - d_i,y ]
//   h = f'' = (1 / n) sum_i [ sum_k p_ik d_ik^2 - (sum_k p_ik d_ik)^2 ] >= 0,   p_ik = exp(s d_ik) / sum_k exp(s d_ik)
// Arithmetic of a row pass (the test bounds of tests/ts_ref.py are derived from these steps).  One wave per row; lane l owns the
// columns l, l + 64, ... .  m = max_k z_k and d_k = z_k - m in fp32; a_k = (float)(s (double) d_k), one rounding of the double product;
// e_k = expf(a_k), the accurate fp32 exponential; from there on double: S = sum e_k, T1 = sum e_k d_k, T2 = sum e_k d_k^2 (d_k is kept
// finite, so a term with e_k = 0 adds 0), each as per-lane partial sums over ascending k, then the xor tree over the lanes.  Row values
//   f_i = log S - s d_y,   g_i = T1 / S - d_y,   h_i = T2 / S - (T1 / S)^2,   d_y = (double)(z_y - m), the difference formed in fp32.
// A workgroup of four waves owns 16 rows, wave w the four consecutive rows 4 w .. 4 w + 3; the row values go to LDS, one thread per
// quantity adds the 16 rows in ascending order, and each workgroup writes ONE partial per quantity; a single workgroup then adds the partials (thread t those at t, t + 256, ... in ascending
// order, the xor tree, the four waves in order) and takes the step.  No atomics, every sum has one owner, no workgroup waits for
// another: every dependency between workgroups is a kernel boundary.  The sums depend on N and K alone (not on ld, not on the device),
// so two calls give the same bits.
// A label outside [0, K) is counted, nothing is read at it, and the whole table becomes NaN.  A row (with a label in range) that holds
// a non-finite logit is left out and counted.
// The iteration:  pass 1 evaluates s_max = 1 / t_min, s_min = 1 / t_max, s_0 = clamp(1) and 1 (one point when s_0 = 1) in one read.
// g(s_max) <= 0: the result is s_max (status 2, clamped at t_min); g(s_min) >= 0: s_min (status 1, clamped at t_max).  Otherwise
// [lo, hi] = [s_min, s_max] brackets the root and every pass at s moves lo or hi to s by the sign of g(s), forms the candidate
// s - g / h, replaces it by sqrt(lo hi) when h is not positive and finite or the candidate is not inside (lo, hi), and stops with
// status 0 when |candidate - s| <= tol s or g == 0; the result is s, the point where f and g were evaluated.  After max_iter passes:
// status 3.  2 max_iter launches are enqueued; those behind the end read the state's `done` word and return at once.
// Compiled WITHOUT -ffast-math (build.sh): non-finite logits are found by comparison, the accurate expf / log / sqrt are part of the
// bounds and the order of the sums is part of the contract.
#ifdef __FAST_MATH__
#error "tscale.hip finds non-finite logits by comparison and fixes the order of its sums: build it without -ffast-math"
#endif
#include <float.h>
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define TS_MAX_N (1 << 20)
#define TS_ROWS 16               // rows per workgroup of a pass: four waves, four consecutive rows each (small workgroups: a compute
                                 // unit takes the next one as soon as one ends, so the grid has no long last round)
#define TS_THREADS 256
#define TS_WAVES (TS_THREADS / 64)
#define TS_WAVE_ROWS (TS_ROWS / TS_WAVES)
#define TS_STEP_THREADS 256      // the summing step: one workgroup, thread t adds the partials t, t + 256, ...
#define TS_CACHE 16              // a lane keeps up to 16 columns of its row in registers: K <= 1024 is read once per pass
#define TS_MAX_POINTS 4
#define TS_STATE 8               // doubles: s | lo | hi | done | passes | 3 spare
#define TS_MAX_ITER 64

struct TsPoints { double s[TS_MAX_POINTS]; };


// S, T1, T2 of one column at NP points.  The difference is kept finite (a spread beyond the fp32 range ends at -FLT_MAX), so that a
// term with e = 0 adds 0 and not 0 * inf.
template <int NP>
__device__ __forceinline__ void ts_add(float z, float m, const double* s, double* S, double* T1, double* T2) {
    const double dd = (double)fmaxf(z - m, -FLT_MAX);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const float e = expf((float)(s[p] * dd));
        const double ed = (double)e * dd;
        S[p] += (double)e;
        T1[p] += ed;
        T2[p] += ed * dd;
    }
}

// ---- one pass over the rows.  NP points: 3 or 4 in the first pass (pts), 1 afterwards (state[0]).  NR > 0: K <= 64 NR and the rows
// stay in registers, RPI rows of the wave in flight at once (their loads are issued together and their reductions interleave; a row
// past the end re-reads row N - 1 and counts for nothing); NR = 0: a longer row is read twice, one row at a time.  The code between
// the loads and the row values has no branch.  The row values (a logarithm and two divisions in double) of the RPI rows are formed
// at once, row r in lane r, and go to LDS; one thread per quantity adds the workgroup's 16 rows in ascending order.
// part (gridDim.x, 3 NP + 2) = per point {sum f, sum g, sum h}, rows used, bad labels ----
template <int NP, int NR, int RPI>
__global__ __launch_bounds__(TS_THREADS)
void ts_pass_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int N, int K, TsPoints pts,
                    const double* __restrict__ state, double* __restrict__ part) {
    constexpr int Q = 3 * NP + 2, NC = NR > 0 ? NR : 1;
    __shared__ double rv[TS_ROWS][Q];
    double s[NP];
    if (NP == 1) {
        if (state[3] != 0.0) return;                         // the fit has ended: nothing to do (uniform over the grid)
        s[0] = state[0];
    } else {
#pragma unroll
        for (int p = 0; p < NP; ++p) s[p] = pts.s[p];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * TS_ROWS + wave * TS_WAVE_ROWS;
    for (int it = 0; it < TS_WAVE_ROWS; it += RPI) {
        double* mine = rv[wave * TS_WAVE_ROWS + it + (lane < RPI ? lane : 0)];
        if (row0 + it >= (int64_t)N) {                       // uniform over the wave: rows past the end add zeros
            if (lane < RPI)
#pragma unroll
                for (int q = 0; q < Q; ++q) mine[q] = 0.0;
            continue;
        }
        const float* z[RPI];
        float c[RPI][NC];
        double S[RPI][NP], T1[RPI][NP], T2[RPI][NP], dy[RPI];
        bool use[RPI], badl[RPI];
#pragma unroll
        for (int r = 0; r < RPI; ++r) {
            const int64_t row = row0 + it + r;
            z[r] = logits + (size_t)(row < (int64_t)N ? row : (int64_t)N - 1) * (size_t)ld;
            if (NR > 0) {
#pragma unroll
                for (int j = 0; j < NC; ++j) c[r][j] = lane + 64 * j < K ? z[r][lane + 64 * j] : -INFINITY;
            }
        }
#pragma unroll
        for (int r = 0; r < RPI; ++r) {
            const int64_t row = row0 + it + r;
            const bool valid = row < (int64_t)N;
            float m = -INFINITY;
            bool ok = true;
            if (NR > 0) {
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    ok = ok && (lane + 64 * j >= K || finite32(c[r][j]));
                    m = fmaxf(m, c[r][j]);
                }
            } else {
                for (int k = lane; k < K; k += 64) {
                    const float v = z[r][k];
                    ok = ok && finite32(v);
                    m = fmaxf(m, v);
                }
            }
            const int64_t y = labels[valid ? row : (int64_t)N - 1];
            const bool inside = label_ok(y, K);
            use[r] = valid && inside && !__any(!ok);
            badl[r] = valid && !inside;
            m = wave_max(m);
            double a0[NP], a1[NP], a2[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) a0[p] = a1[p] = a2[p] = 0.0;
            if (NR > 0) {
#pragma unroll
                for (int j = 0; j < NC; ++j)
                    if (lane + 64 * j < K) ts_add<NP>(c[r][j], m, s, a0, a1, a2);
            } else {
                for (int k = lane; k < K; k += 64) ts_add<NP>(z[r][k], m, s, a0, a1, a2);
            }
            dy[r] = (double)(z[r][inside ? y : 0] - m);      // nothing is read at a label outside [0, K)
#pragma unroll
            for (int p = 0; p < NP; ++p) { S[r][p] = wave_sum(a0[p]); T1[r][p] = wave_sum(a1[p]); T2[r][p] = wave_sum(a2[p]); }
        }
        // every lane holds the sums of all RPI rows: lane r takes row r's
        double Sx[NP], T1x[NP], T2x[NP], dyx = dy[0];
        bool usex = use[0], badx = badl[0];
#pragma unroll
        for (int p = 0; p < NP; ++p) { Sx[p] = S[0][p]; T1x[p] = T1[0][p]; T2x[p] = T2[0][p]; }
#pragma unroll
        for (int r = 1; r < RPI; ++r) {
            const bool me = lane == r;
            dyx = me ? dy[r] : dyx; usex = me ? use[r] : usex; badx = me ? badl[r] : badx;
#pragma unroll
            for (int p = 0; p < NP; ++p) { Sx[p] = me ? S[r][p] : Sx[p]; T1x[p] = me ? T1[r][p] : T1x[p]; T2x[p] = me ? T2[r][p] : T2x[p]; }
        }
        double val[Q];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double mu = T1x[p] / Sx[p], q = T2x[p] / Sx[p];
            val[3 * p] = usex ? log(Sx[p]) - s[p] * dyx : 0.0;
            val[3 * p + 1] = usex ? mu - dyx : 0.0;
            val[3 * p + 2] = usex ? q - mu * mu : 0.0;
        }
        val[3 * NP] = usex ? 1.0 : 0.0;
        val[3 * NP + 1] = badx ? 1.0 : 0.0;
        if (lane < RPI)
#pragma unroll
            for (int q = 0; q < Q; ++q) mine[q] = val[q];
    }
    __syncthreads();
    if (threadIdx.x < Q) {
        const int q = threadIdx.x;
        double t = 0.0;
        for (int i = 0; i < TS_ROWS; ++i) t += rv[i][q];     // the rows in ascending order
        part[(size_t)blockIdx.x * Q + q] = t;
    }
}

struct TsFit { double s_min, s_max, t_lo, t_hi, tol; int max_iter, N; };

// out = {T, s, NLL at s = 1, NLL at the result, g at the result, passes, status, rows left out}
__device__ __forceinline__ void ts_finish(double* __restrict__ state, double* __restrict__ out, const TsFit& fit, double s, double f, double g,
                                          double passes, double status, double nll1, bool first) {
    const double t = 1.0 / s;
    out[0] = t < fit.t_lo ? fit.t_lo : (t > fit.t_hi ? fit.t_hi : t);
    out[1] = s;
    if (first) out[2] = nll1;
    out[3] = f;
    out[4] = g;
    out[5] = passes;
    out[6] = status;
    state[3] = 1.0;
}

// ---- the step behind a pass: one workgroup adds the partials in a fixed order, one thread moves the state ----
template <int NP>
__global__ __launch_bounds__(TS_STEP_THREADS)
void ts_step_kernel(const double* __restrict__ part, int nblk, double* __restrict__ state, double* __restrict__ out, TsFit fit, TsPoints pts) {
    constexpr int Q = 3 * NP + 2;
    __shared__ double red[TS_STEP_THREADS / 64][Q];
    if (NP == 1 && state[3] != 0.0) return;
    const int tid = threadIdx.x;
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    for (int b = tid; b < nblk; b += TS_STEP_THREADS)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] += part[(size_t)b * Q + q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = wave_sum(acc[q]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int q = 0; q < Q; ++q) red[tid >> 6][q] = acc[q];
    __syncthreads();
    if (tid != 0) return;
    double tot[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) tot[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    const double n = tot[3 * NP], bad = tot[3 * NP + 1];
    double s, f, g, h, passes;
    if (NP == 1) {
        s = state[0];
        passes = state[4] + 1.0;
        f = tot[0] / n; g = tot[1] / n; h = tot[2] / n;
    } else {
        // points of the first pass: 0 = s_max, 1 = s_min, 2 = s_0, 3 = 1 (NP = 3: s_0 is 1 and serves as both)
        passes = 1.0;
        state[4] = 1.0;
        out[7] = (double)fit.N - n - bad;
        if (bad > 0.0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) out[q] = quiet_nan();
            state[3] = 1.0;
            return;
        }
        if (!(n > 0.0)) {
            out[0] = out[1] = out[2] = out[3] = out[4] = quiet_nan();
            out[5] = 1.0; out[6] = 0.0;
            state[3] = 1.0;
            return;
        }
        const double nll1 = tot[3 * (NP - 1)] / n;
        if (tot[1] / n <= 0.0) { ts_finish(state, out, fit, pts.s[0], tot[0] / n, tot[1] / n, 1.0, 2.0, nll1, true); return; }
        if (tot[3 + 1] / n >= 0.0) { ts_finish(state, out, fit, pts.s[1], tot[3] / n, tot[3 + 1] / n, 1.0, 1.0, nll1, true); return; }
        out[2] = nll1;
        state[1] = fit.s_min;
        state[2] = fit.s_max;
        s = pts.s[2];
        f = tot[6] / n; g = tot[7] / n; h = tot[8] / n;
    }
    double lo = state[1], hi = state[2];
    if (g < 0.0) lo = s; else hi = s;
    double cand = s - g / h;
    if (!(h > 0.0 && h < INFINITY) || !(cand > lo && cand < hi)) cand = sqrt(lo * hi);
    state[1] = lo; state[2] = hi; state[4] = passes;
    if (fabs(cand - s) <= fit.tol * s || g == 0.0) { ts_finish(state, out, fit, s, f, g, passes, 0.0, 0.0, false); return; }
    if (passes >= (double)fit.max_iter) { ts_finish(state, out, fit, s, f, g, passes, 3.0, 0.0, false); return; }
    state[0] = cand;
}

// ---- dst = (float)((double) src * s), s = table[1] ----
__global__ __launch_bounds__(256)
void ts_scale_kernel(const float* src, float* dst, int64_t ld_src, int64_t ld_dst, const double* __restrict__ table, int B, int K) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const double s = table[1];
    for (int b = blockIdx.y; b < B; b += gridDim.y)
        dst[(size_t)b * (size_t)ld_dst + k] = (float)((double)src[(size_t)b * (size_t)ld_src + k] * s);
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool ts_set_ok(int N, int K) { return N >= 1 && N <= TS_MAX_N && K >= 2; }
static inline int ts_blocks(int N) { return (N + TS_ROWS - 1) / TS_ROWS; }
static inline size_t ts_ws_total(int N) { return (TS_STATE + (size_t)ts_blocks(N) * (3 * TS_MAX_POINTS + 2)) * sizeof(double); }

extern "C" int64_t uvit_op_ts_ws_bytes(int N, int K) {
    if (!ts_set_ok(N, K)) return UVIT_ERR_SHAPE;
    return (int64_t)ts_ws_total(N);
}

// rows of a wave in flight at once: all four in the one-point passes, two in the first pass (its sums at 3 or 4 points take the registers)
template <int NP>
static inline void ts_launch_pass(hipStream_t st, const float* logits, int64_t ld, const int64_t* labels, int N, int K, const TsPoints& pts,
                                  const double* state, double* part) {
    constexpr int RPI = NP == 1 ? TS_WAVE_ROWS : 2;
    const dim3 grid(ts_blocks(N)), block(TS_THREADS);
    if (K <= 64) hipLaunchKernelGGL((ts_pass_kernel<NP, 1, RPI>), grid, block, 0, st, logits, ld, labels, N, K, pts, state, part);
    else if (K <= 256) hipLaunchKernelGGL((ts_pass_kernel<NP, 4, RPI>), grid, block, 0, st, logits, ld, labels, N, K, pts, state, part);
    else if (K <= 64 * TS_CACHE) hipLaunchKernelGGL((ts_pass_kernel<NP, TS_CACHE, RPI>), grid, block, 0, st, logits, ld, labels, N, K, pts, state, part);
    else hipLaunchKernelGGL((ts_pass_kernel<NP, 0, 1>), grid, block, 0, st, logits, ld, labels, N, K, pts, state, part);
}

extern "C" int uvit_op_ts_fit(const float* logits, int64_t ld, const int64_t* labels, int N, int K, double t_min, double t_max, double tol,
                              int max_iter, double* out, void* ws, int64_t ws_bytes, uvit_stream stream) {
    if (!logits || !labels || !out || !ws || misaligned(ws, 16)) return UVIT_ERR_ARG;
    if (!ts_set_ok(N, K) || ld < (int64_t)K) return UVIT_ERR_SHAPE;
    if (!(t_min > 0.0) || !(t_max > t_min) || !(t_max < INFINITY) || !(tol > 0.0) || max_iter < 1 || max_iter > TS_MAX_ITER) return UVIT_ERR_SHAPE;
    if (ws_bytes < (int64_t)ts_ws_total(N)) return UVIT_ERR_WORKSPACE;
    TsFit fit;
    fit.s_min = 1.0 / t_max; fit.s_max = 1.0 / t_min;
    fit.t_lo = fmax(t_min, 1.0 / fit.s_max); fit.t_hi = fmin(t_max, 1.0 / fit.s_min);
    fit.tol = tol; fit.max_iter = max_iter; fit.N = N;
    TsPoints pts;
    pts.s[0] = fit.s_max; pts.s[1] = fit.s_min;
    pts.s[2] = 1.0 < fit.s_min ? fit.s_min : (1.0 > fit.s_max ? fit.s_max : 1.0);
    pts.s[3] = 1.0;
    double *state = (double*)ws, *part = state + TS_STATE;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = ts_blocks(N);
    if (hipMemsetAsync(state, 0, TS_STATE * sizeof(double), st) != hipSuccess) return UVIT_ERR_LAUNCH;
    if (pts.s[2] == 1.0) {                                    // 1 lies inside the range: s_0 and the point of `NLL at s = 1` are one
        ts_launch_pass<3>(st, logits, ld, labels, N, K, pts, state, part);
        hipLaunchKernelGGL((ts_step_kernel<3>), dim3(1), dim3(TS_STEP_THREADS), 0, st, (const double*)part, nblk, state, out, fit, pts);
    } else {
        ts_launch_pass<TS_MAX_POINTS>(st, logits, ld, labels, N, K, pts, state, part);
        hipLaunchKernelGGL((ts_step_kernel<TS_MAX_POINTS>), dim3(1), dim3(TS_STEP_THREADS), 0, st, (const double*)part, nblk, state, out, fit, pts);
    }
    for (int it = 1; it < max_iter; ++it) {
        ts_launch_pass<1>(st, logits, ld, labels, N, K, pts, state, part);
        hipLaunchKernelGGL((ts_step_kernel<1>), dim3(1), dim3(TS_STEP_THREADS), 0, st, (const double*)part, nblk, state, out, fit, pts);
    }
    return uvit_check_launch();
}

extern "C" int uvit_op_ts_scale(const float* src, float* dst, int64_t ld_src, int64_t ld_dst, const double* table, int B, int K,
                                uvit_stream stream) {
    if (!src || !dst || !table) return UVIT_ERR_ARG;
    if (B < 1 || K < 1 || ld_src < (int64_t)K || ld_dst < (int64_t)K) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(ts_scale_kernel, dim3((K + 255) / 256, B < 1024 ? B : 1024), dim3(256), 0, (hipStream_t)stream, src, dst, ld_src, ld_dst,
                       table, B, K);
    return uvit_check_launch();
}
