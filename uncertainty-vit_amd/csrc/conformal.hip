// Split conformal prediction sets (LAC, APS, RAPS) calibrated and evaluated on the device (gfx950).  DESIGN.md section 9.8.
//   uvit_op_cp_scores    the conformal score of each row's label into a float64 device column
//   uvit_op_cp_quantile  the exact order statistic q_a = k_a-th smallest score, k_a = ceil((n + 1)(1 - alpha_a)), for up to 8 levels
//   uvit_op_cp_sets      per evaluation row and level: the size of {j : s_j <= q_a} and the flag s_y <= q_a, added to integer counters
//   uvit_op_cp_finish    the counters turned into coverage, mean size, SSCV, worst-class coverage, ... in the table's remaining slots
// Arithmetic of a row (the bound delta of tests/cp_ref.py is derived from these steps).  m = max_k z_k and d_k = z_k - m in fp32;
// e_k = expf(d_k), the accurate fp32 exponential; from there on double: S = sum_k e_k.  The ordinal rank o_j of class j is exact
// integer arithmetic on the fp32 logits, 1 + #{i : z_i > z_j} + #{i < j : z_i == z_j} (uvit_op_stability_ranks' rule; softmax is
// monotone, so this is the rank by descending p with ties to the smaller index), and
//   lac   s_j = 1 - e_j / S
//   aps   s_j = (sum_{i : o_i < o_j} e_i + u e_j) / S          raps   the same + lam * max(0, o_j - kreg)
// with u = 1 when there is no u vector.  cp_row() forms the label's score by streaming the row once more: one wave per row, lane l
// owns the columns l, l + 64, ..., per-lane partial sums over ascending k, the xor tree over the lanes.  uvit_op_cp_sets calls the
// SAME function for the covered flag, so covered == (the score uvit_op_cp_scores writes for that row <= q) bit for bit; the set
// size is the count of s_j <= q over the row in rank order: 64-bit keys (order-preserving image of -z, class index) sorted in LDS by
// a bitonic network over K padded to a power of two, thread t then owns PER consecutive ranks, the threads' totals are added in
// ascending order, and every s_j is compared with all levels' q.  lac needs no order and skips the sort.
// The sums depend on K alone (not on ld, not on the batch a row arrives in), so two calls give the same bits, and the counters are
// integers added by atomics, which is exact: consecutive batches give the counters of their concatenation.
// A row that holds a non-finite logit gets a NaN score (uvit_op_cp_quantile counts and leaves it out; uvit_op_cp_sets counts it as
// skipped).  A label outside [0, K) gets a NaN with the payload CP_BAD_BITS, nothing is read at it, and the table becomes NaN.
// Compiled WITHOUT -ffast-math and with -ffp-contract=off (build.sh): non-finite logits are found by comparison, the accurate
// expf is part of the bound, and the score expression must round the same way wherever it is inlined.
#ifdef __FAST_MATH__
#error "conformal.hip finds non-finite logits by comparison and fixes the rounding of its scores: build it without -ffast-math"
#endif
#include <float.h>
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define CP_MAX_N (1 << 20)
#define CP_MAX_K 4096
#define CP_MAX_A 8
#define CP_TABLE 16              // doubles per level: alpha | q | k | n | rows left out | status | coverage | mean size | empty | singleton |
                                 // max size | SSCV | worst-class coverage | evaluation rows used | evaluation rows skipped | 0
#define CP_LAC 0
#define CP_APS 1
#define CP_RAPS 2
#define CP_BAD_BITS 0x7FF8000000000BADULL       // the score of a row whose label is outside [0, K); a non-finite logit: quiet_nan()
#define CP_PASSES 8              // radix select: eight bits per pass, from the top byte down
#define CP_GLOBAL 4              // counters: rows used | rows skipped | bad labels | 0, then CP_LEVEL per level, then the classes
#define CP_LEVEL 20              // covered | size sum | empty | singleton | max size | 7 bins: rows | 7 bins: covered | 0
#define CP_BINS 7
#ifndef CP_WAVE_MAX_KP
#define CP_WAVE_MAX_KP 128       // the sets kernel: one wave per row up to this padded K, four waves above (measured: DESIGN.md 9.8)
#endif

typedef unsigned long long u64;

__device__ __forceinline__ double cp_bits(u64 b) { return __longlong_as_double((long long)b); }

// The score of the class with rank o: `before` = sum of the e_i ranked before it, e its own exponential, S the row's sum.
__device__ __forceinline__ double cp_score_of(int kind, double before, double e, double u, double S, int o, double lam, int kreg) {
    if (kind == CP_LAC) return 1.0 - e / S;
    const double pen = o > kreg ? lam * (double)(o - kreg) : 0.0;         // lam = 0 (aps): + 0.0, the aps score bit for bit
    return (before + u * e) / S + pen;
}

struct CpRow { double score, S; float m; int state; };                    // state: 0 usable, 1 a non-finite logit, 2 a bad label

// The label's score of one row, by the 64 lanes of one wave.
__device__ __forceinline__ CpRow cp_row(const float* __restrict__ z, int K, int64_t y, float u, int kind, double lam, int kreg, int lane) {
    CpRow r;
    float m = -INFINITY;
    bool ok = true;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        ok = ok && finite32(v);
        m = fmaxf(m, v);
    }
    m = wave_max(m);
    const bool inside = label_ok(y, K);
    r.m = m;
    r.state = !inside ? 2 : (__any(!ok) ? 1 : 0);                         // uniform over the wave
    if (r.state) {
        r.S = quiet_nan();
        r.score = cp_bits(r.state == 2 ? CP_BAD_BITS : QUIET_NAN_BITS);
        return r;
    }
    const float zy = z[y];
    double S = 0.0, before = 0.0;
    int ahead = 0;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        const double e = (double)expf(v - m);
        S += e;
        if (v > zy || (v == zy && k < (int)y)) { before += e; ++ahead; }
    }
    S = wave_sum(S);
    before = wave_sum(before);
    ahead = wave_sum(ahead);
    r.S = S;
    r.score = cp_score_of(kind, before, (double)expf(zy - m), (double)u, S, ahead + 1, lam, kreg);
    return r;
}

// ---- scores: one wave per row, four rows per workgroup ----
__global__ __launch_bounds__(256)
void cp_scores_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, const float* __restrict__ u, int N,
                      int K, int kind, double lam, int kreg, double* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)N) return;
    const CpRow r = cp_row(logits + (size_t)row * (size_t)ld, K, labels[row], u ? u[row] : 1.0f, kind, lam, kreg, lane);
    if (lane == 0) scores[row] = r.score;
}

// ---- the order statistic: a radix select on the bit patterns (non-negative doubles order as unsigned integers) ----
// ws: u64 state[CP_MAX_A][4] = prefix | k remaining | stopped | 0;  u64 glob[4] = NaN rows | bad labels | 0 | 0;
//     uint32 hist[CP_PASSES][CP_MAX_A][256] (pass 0 uses level 0's for every level)
struct CpLevels { double alpha[CP_MAX_A], one_minus[CP_MAX_A]; };
static inline size_t cp_ws_total() { return (CP_MAX_A * 4 + 4) * sizeof(u64) + (size_t)CP_PASSES * CP_MAX_A * 256 * sizeof(uint32_t); }

__global__ __launch_bounds__(256)
void cp_hist_kernel(const double* __restrict__ scores, int N, int A, int pass, const u64* __restrict__ state, u64* __restrict__ glob,
                    uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[CP_MAX_A * 256];
    const int tid = threadIdx.x, nh = (pass == 0 ? 1 : A) * 256, shift = 56 - 8 * pass;
    for (int i = tid; i < nh; i += 256) h[i] = 0;
    u64 pre[CP_MAX_A];
    bool act[CP_MAX_A];
#pragma unroll
    for (int a = 0; a < CP_MAX_A; ++a) {
        act[a] = pass > 0 && a < A && state[a * 4 + 2] == 0;
        pre[a] = act[a] ? state[a * 4] >> (shift + 8) : 0;
    }
    __syncthreads();
    u64 n_nan = 0, n_bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < (int64_t)N; i += (int64_t)gridDim.x * 256) {
        u64 b = (u64)__double_as_longlong(scores[i]);
        if ((b & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL) {       // a NaN: left out
            if (b == CP_BAD_BITS) ++n_bad; else ++n_nan;
            continue;
        }
        if (b >> 63) b = 0;                                               // -0 (the scores are non-negative)
        const int byte = (int)((b >> shift) & 255);
        if (pass == 0) {
            atomicAdd(&h[byte], 1u);
        } else {
            const u64 top = b >> (shift + 8);
#pragma unroll
            for (int a = 0; a < CP_MAX_A; ++a)
                if (act[a] && top == pre[a]) atomicAdd(&h[a * 256 + byte], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < nh; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
    if (pass == 0) {
        if (n_nan) atomicAdd(&glob[0], n_nan);
        if (n_bad) atomicAdd(&glob[1], n_bad);
    }
}

__global__ __launch_bounds__(64)
void cp_select_kernel(const uint32_t* __restrict__ hist, int N, int A, int pass, u64* __restrict__ state, const u64* __restrict__ glob,
                      CpLevels lv, double* __restrict__ table) {
    const int a = threadIdx.x;
    if (a >= A) return;
    const uint32_t* h = hist + (pass == 0 ? 0 : a * 256);
    double* t = table + a * CP_TABLE;
    u64 prefix = 0;
    int64_t krem;
    if (pass == 0) {
        int64_t n = 0;
        for (int b = 0; b < 256; ++b) n += h[b];
        const int64_t bad = (int64_t)glob[1];
        const double kd = ceil((double)(n + 1) * lv.one_minus[a]);
        if (bad > 0) {
            for (int q = 0; q < CP_TABLE; ++q) t[q] = quiet_nan();
            state[a * 4 + 2] = 2;
            return;
        }
        for (int q = 0; q < CP_TABLE; ++q) t[q] = 0.0;
        t[0] = lv.alpha[a]; t[2] = kd; t[3] = (double)n; t[4] = (double)((int64_t)N - n);
        if (kd > (double)n) {                                             // fewer rows than the level needs: every set is full
            t[1] = INFINITY; t[5] = 1.0;
            state[a * 4 + 2] = 1;
            return;
        }
        krem = (int64_t)kd;
    } else {
        if (state[a * 4 + 2] != 0) return;
        prefix = state[a * 4];
        krem = (int64_t)state[a * 4 + 1];
    }
    int64_t cum = 0;
    int sel = 255;
    for (int b = 0; b < 256; ++b) {
        const int64_t c = h[b];
        if (cum + c >= krem) { sel = b; break; }
        cum += c;
    }
    prefix |= (u64)sel << (56 - 8 * pass);
    state[a * 4] = prefix;
    state[a * 4 + 1] = (u64)(krem - cum);
    if (pass == CP_PASSES - 1) t[1] = cp_bits(prefix);
}

// ---- sets: one workgroup of T threads per row, K padded to KP ----
__device__ __forceinline__ int cp_bin(int size) {
    return size <= 1 ? 0 : size <= 3 ? 1 : size <= 6 ? 2 : size <= 10 ? 3 : size <= 100 ? 4 : size <= 1000 ? 5 : 6;
}

template <int KP, int T>
__global__ __launch_bounds__(T)
void cp_sets_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, const float* __restrict__ u, int B, int K,
                    int kind, double lam, int kreg, const double* __restrict__ table, int A, u64* __restrict__ counters,
                    int32_t* __restrict__ sizes, uint8_t* __restrict__ covered, int64_t ld_out) {
    constexpr int PER = KP / T;
    __shared__ u64 key[KP];
    __shared__ double tsum[T];
    __shared__ double r_score, r_S;
    __shared__ float r_m;
    __shared__ int r_state, cnt[CP_MAX_A];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t row = blockIdx.x;
    const float* z = logits + (size_t)row * (size_t)ld;
    const int64_t y = labels[row];
    const float uf = u ? u[row] : 1.0f;
    if (tid < 64) {                                                       // the first wave: the label's score, as uvit_op_cp_scores forms it
        const CpRow r = cp_row(z, K, y, uf, kind, lam, kreg, lane);
        if (lane == 0) { r_score = r.score; r_S = r.S; r_m = r.m; r_state = r.state; }
    }
    if (tid < CP_MAX_A) cnt[tid] = 0;
    __syncthreads();
    const int state = r_state;                                            // uniform over the workgroup
    if (state != 0) {
        if (tid == 0) atomicAdd(&counters[state == 2 ? 2 : 1], 1ULL);
        if (tid < A) {
            if (sizes) sizes[(size_t)tid * (size_t)ld_out + row] = -1;
            if (covered) covered[(size_t)tid * (size_t)ld_out + row] = 0;
        }
        return;
    }
    const float m = r_m;
    const double S = r_S, uu = (double)uf;
    double q[CP_MAX_A];
#pragma unroll
    for (int a = 0; a < CP_MAX_A; ++a) q[a] = a < A ? table[a * CP_TABLE + 1] : 0.0;
    int c[CP_MAX_A];
#pragma unroll
    for (int a = 0; a < CP_MAX_A; ++a) c[a] = 0;
    if (kind == CP_LAC) {
        for (int k = tid; k < K; k += T) {
            const double s = cp_score_of(CP_LAC, 0.0, (double)expf(z[k] - m), uu, S, 0, 0.0, 0);
#pragma unroll
            for (int a = 0; a < CP_MAX_A; ++a) c[a] += a < A && s <= q[a] ? 1 : 0;
        }
    } else {
        for (int i = tid; i < KP; i += T) {
            u64 kk = ~0ULL;                                               // padding sorts behind every class
            if (i < K) {
                const uint32_t b = __float_as_uint(z[i] + 0.0f);          // -0 -> +0
                const uint32_t img = (b & 0x80000000u) ? ~b : (b | 0x80000000u);      // ascending in z
                kk = ((u64)(~img) << 32) | (u64)i;                        // descending z, then ascending index
            }
            key[i] = kk;
        }
        __syncthreads();
        for (int k = 2; k <= KP; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int p = tid; p < KP / 2; p += T) {
                    const int i = BITONIC_LO(p, j), l = i | j;
                    BITONIC_CMPX_AT(key, i, l, (i & k) == 0);
                }
                __syncthreads();
            }
        // thread t owns the ranks t PER + 1 .. (t + 1) PER
        double e[PER], tot = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = tid * PER + i;
            e[i] = 0.0;
            if (r < K) {
                const uint32_t img = ~(uint32_t)(key[r] >> 32);
                const uint32_t b = (img & 0x80000000u) ? (img & 0x7FFFFFFFu) : ~img;
                e[i] = (double)expf(__uint_as_float(b) - m);
            }
            tot += e[i];
        }
        tsum[tid] = tot;
        __syncthreads();
        double run = 0.0;
        for (int t = 0; t < tid; ++t) run += tsum[t];                     // the threads in front, in ascending order
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int r = tid * PER + i;
            if (r < K) {
                const double s = cp_score_of(kind, run, e[i], uu, S, r + 1, lam, kreg);
#pragma unroll
                for (int a = 0; a < CP_MAX_A; ++a) c[a] += a < A && s <= q[a] ? 1 : 0;
            }
            run += e[i];
        }
    }
#pragma unroll
    for (int a = 0; a < CP_MAX_A; ++a) {
        const int w = wave_sum(c[a]);
        if (lane == 0 && a < A && w) atomicAdd(&cnt[a], w);
    }
    __syncthreads();
    u64* cls = counters + CP_GLOBAL + (size_t)CP_LEVEL * A;               // totals (K), then covered (A, K)
    if (tid == 0) {
        atomicAdd(&counters[0], 1ULL);
        atomicAdd(&cls[y], 1ULL);
    }
    if (tid < A) {
        const int a = tid, size = cnt[a], bin = cp_bin(size);
        const bool cov = r_score <= table[a * CP_TABLE + 1];
        u64* L = counters + CP_GLOBAL + (size_t)CP_LEVEL * a;
        if (cov) atomicAdd(&L[0], 1ULL);
        atomicAdd(&L[1], (u64)size);
        if (size == 0) atomicAdd(&L[2], 1ULL);
        if (size == 1) atomicAdd(&L[3], 1ULL);
        atomicMax(&L[4], (u64)size);
        atomicAdd(&L[5 + bin], 1ULL);
        if (cov) {
            atomicAdd(&L[5 + CP_BINS + bin], 1ULL);
            atomicAdd(&cls[(size_t)K * (a + 1) + y], 1ULL);
        }
        if (sizes) sizes[(size_t)a * (size_t)ld_out + row] = size;
        if (covered) covered[(size_t)a * (size_t)ld_out + row] = cov ? 1 : 0;
    }
}

// ---- finish: one workgroup per level ----
__global__ __launch_bounds__(256)
void cp_finish_kernel(const u64* __restrict__ counters, double* __restrict__ table, int K, int A) {
    __shared__ double red[256];
    const int a = blockIdx.x, tid = threadIdx.x;
    const u64* L = counters + CP_GLOBAL + (size_t)CP_LEVEL * a;
    const u64* tot = counters + CP_GLOBAL + (size_t)CP_LEVEL * A;
    const u64* cov = tot + (size_t)K * (a + 1);
    double w = INFINITY;
    for (int c = tid; c < K; c += 256)
        if (tot[c]) w = fmin(w, (double)cov[c] / (double)tot[c]);
    red[tid] = w;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmin(red[tid], red[tid + o]);
        __syncthreads();
    }
    if (tid != 0) return;
    double* t = table + a * CP_TABLE;
    const double n = (double)counters[0], nan = quiet_nan(), target = 1.0 - t[0];
    const bool good = counters[2] == 0 && counters[0] > 0 && t[1] == t[1];
    double sscv = 0.0;
    for (int b = 0; b < CP_BINS; ++b)
        if (L[5 + b]) sscv = fmax(sscv, fabs((double)L[5 + CP_BINS + b] / (double)L[5 + b] - target));
    t[6] = good ? (double)L[0] / n : nan;
    t[7] = good ? (double)L[1] / n : nan;
    t[8] = good ? (double)L[2] / n : nan;
    t[9] = good ? (double)L[3] / n : nan;
    t[10] = good ? (double)L[4] : nan;
    t[11] = good ? sscv : nan;
    t[12] = good ? red[0] : nan;
    t[13] = (double)counters[0];
    t[14] = (double)counters[1];
    t[15] = 0.0;
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool cp_kind_ok(int kind, double lam, int kreg) {
    return kind >= CP_LAC && kind <= CP_RAPS && lam >= 0.0 && lam < INFINITY && kreg >= 0;          // lam >= 0 is false for NaN
}
static inline bool cp_k_ok(int K) { return K >= 2 && K <= CP_MAX_K; }

extern "C" int uvit_op_cp_scores(const float* logits, int64_t ld, const int64_t* labels, const float* u, int N, int K, int kind, double lam,
                                 int kreg, double* scores, uvit_stream stream) {
    if (!logits || !labels || !scores) return UVIT_ERR_ARG;
    if (N < 1 || N > CP_MAX_N || !cp_k_ok(K) || ld < (int64_t)K || !cp_kind_ok(kind, lam, kreg)) return UVIT_ERR_SHAPE;
    if (kind != CP_RAPS) { lam = 0.0; kreg = 0; }
    hipLaunchKernelGGL(cp_scores_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, labels, u, N, K, kind, lam, kreg, scores);
    return uvit_check_launch();
}

extern "C" int64_t uvit_op_cp_ws_bytes(int N, int A) {
    if (N < 1 || N > CP_MAX_N || A < 1 || A > CP_MAX_A) return UVIT_ERR_SHAPE;
    return (int64_t)cp_ws_total();
}

extern "C" int uvit_op_cp_quantile(const double* scores, int N, const double* alphas, int A, double* table, void* ws, int64_t ws_bytes,
                                   uvit_stream stream) {
    if (!scores || !alphas || !table || !ws || misaligned(ws, 16)) return UVIT_ERR_ARG;
    if (N < 1 || N > CP_MAX_N || A < 1 || A > CP_MAX_A) return UVIT_ERR_SHAPE;
    CpLevels lv;
    for (int a = 0; a < CP_MAX_A; ++a) {
        const double al = a < A ? alphas[a] : 0.5;
        if (!(al > 0.0 && al < 1.0)) return UVIT_ERR_SHAPE;
        lv.alpha[a] = al;
        lv.one_minus[a] = 1.0 - al;
    }
    if (ws_bytes < (int64_t)cp_ws_total()) return UVIT_ERR_WORKSPACE;
    u64 *state = (u64*)ws, *glob = state + CP_MAX_A * 4;
    uint32_t* hist = (uint32_t*)(glob + 4);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, cp_ws_total(), st) != hipSuccess) return UVIT_ERR_LAUNCH;
    const int blocks = (N + 255) / 256 < 1024 ? (N + 255) / 256 : 1024;
    for (int pass = 0; pass < CP_PASSES; ++pass) {
        uint32_t* h = hist + (size_t)pass * CP_MAX_A * 256;
        hipLaunchKernelGGL(cp_hist_kernel, dim3(blocks), dim3(256), 0, st, scores, N, A, pass, (const u64*)state, glob, h);
        hipLaunchKernelGGL(cp_select_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)h, N, A, pass, state, (const u64*)glob, lv, table);
    }
    return uvit_check_launch();
}

extern "C" int64_t uvit_op_cp_counter_count(int K, int A) {
    if (!cp_k_ok(K) || A < 1 || A > CP_MAX_A) return UVIT_ERR_SHAPE;
    return (int64_t)CP_GLOBAL + (int64_t)CP_LEVEL * A + (int64_t)K * (A + 1);
}

template <int KP, int T>
static inline void cp_launch_sets(hipStream_t st, const float* logits, int64_t ld, const int64_t* labels, const float* u, int B, int K, int kind,
                                  double lam, int kreg, const double* table, int A, u64* counters, int32_t* sizes, uint8_t* covered,
                                  int64_t ld_out) {
    hipLaunchKernelGGL((cp_sets_kernel<KP, T>), dim3(B), dim3(T), 0, st, logits, ld, labels, u, B, K, kind, lam, kreg, table, A, counters, sizes,
                       covered, ld_out);
}

extern "C" int uvit_op_cp_sets(const float* logits, int64_t ld, const int64_t* labels, const float* u, int B, int K, int kind, double lam,
                               int kreg, const double* table, int A, int64_t* counters, int32_t* sizes, uint8_t* covered, int64_t ld_out,
                               uvit_stream stream) {
    if (!logits || !labels || !table || !counters) return UVIT_ERR_ARG;
    if (B < 1 || B > CP_MAX_N || !cp_k_ok(K) || ld < (int64_t)K || A < 1 || A > CP_MAX_A || !cp_kind_ok(kind, lam, kreg)) return UVIT_ERR_SHAPE;
    if ((sizes || covered) && ld_out < (int64_t)B) return UVIT_ERR_SHAPE;
    if (kind != CP_RAPS) { lam = 0.0; kreg = 0; }
    hipStream_t st = (hipStream_t)stream;
    u64* cn = (u64*)counters;
#define CP_GO(KP, T) cp_launch_sets<KP, T>(st, logits, ld, labels, u, B, K, kind, lam, kreg, table, A, cn, sizes, covered, ld_out)
    if (K <= 64) CP_GO(64, 64);
    else if (K <= 128) CP_GO(128, 64);
    else if (K <= 256) { if (256 <= CP_WAVE_MAX_KP) CP_GO(256, 64); else CP_GO(256, 256); }
    else if (K <= 512) { if (512 <= CP_WAVE_MAX_KP) CP_GO(512, 64); else CP_GO(512, 256); }
    else if (K <= 1024) { if (1024 <= CP_WAVE_MAX_KP) CP_GO(1024, 64); else CP_GO(1024, 256); }
    else if (K <= 2048) CP_GO(2048, 256);
    else CP_GO(4096, 256);
#undef CP_GO
    return uvit_check_launch();
}

extern "C" int uvit_op_cp_finish(const int64_t* counters, double* table, int K, int A, uvit_stream stream) {
    if (!counters || !table) return UVIT_ERR_ARG;
    if (!cp_k_ok(K) || A < 1 || A > CP_MAX_A) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(cp_finish_kernel, dim3(A), dim3(256), 0, (hipStream_t)stream, (const u64*)counters, table, K, A);
    return uvit_check_launch();
}
