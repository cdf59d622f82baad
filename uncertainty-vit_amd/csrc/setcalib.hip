// Set-level calibration of a classifier's evaluation set on the device (gfx950): DESIGN.md section 9.19.
//   uvit_op_scal_probs     per batch, one wave per row: the softmax of calib_softmax_kernel (calib.hip), written at the batch's rows of
//                          the set's row-major store (row stride ld >= K); no 1024-row limit
//   uvit_op_scal_metrics   per evaluation: top-label ECE / MCE / OE with the reliability table, NLL, Brier, and per class SCE_c, ACE_c,
//                          TACE_c, AUROC_c, all from ONE sort of every column: the K class columns p[:, c] and the confidence column
// Keys are 32-bit: a probability in [0, 1] has the bit pattern of a non-negative float <= 0x3F800000 < 2^30, whose unsigned order is
// the numeric order, so key = bits << 1 | hit ([y == c] for a class column, [pred == y] for the confidence column) is ordered by
// (value, hit) and stays below the padding 0xFFFFFFFF.  Equal keys are the same (value, hit): the sorted column is a function of the
// input alone, whatever network produced it.  For the key only, a value is clamped to [0, 1] (NaN and negatives -> 0, above 1 -> 1):
// a set that holds such a value reports it as a bad row and NaN metrics, and no input can make an index leave its array.
// Every bin of every metric is a contiguous run [a, b) of the sorted column, found by bisection with the comparison of calib.hip (the
// fp32 value widened to double against a double bound); in a tie group the negatives stand in front of the positives, so AUROC's pair
// counts come from one prefix count of the positives.  No float atomics and no atomics at all: a run's sum is formed from its own
// elements by one wave (lane l adds a + l, a + l + 64, ... ascending, then the xor tree), a class is owned by one workgroup, the set's
// means by one workgroup; the order depends on (N, K, the bin counts) and the values, never on ld, timing or the batches that filled
// the store.  No workgroup waits for another: every dependency between workgroups is a kernel boundary.
// Compiled WITHOUT -ffast-math (build.sh): the accurate expf, the IEEE comparisons, NaN found by its comparisons and the order of
// the sums are part of the contract.
#ifdef __FAST_MATH__
#error "setcalib.hip fixes the order of its sums and compares in IEEE double: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define SCAL_MAX_N (1 << 20)
#define SCAL_MAX_NK (1ll << 30)
#define SCAL_MAX_BINS 64
#define SCAL_CHUNK 8192            // 32-bit keys a workgroup sorts in LDS: 32 KB
#define SCAL_SORT_THREADS 1024     // 16 waves: the network is a chain of LDS round trips, hidden by waves and by nothing else
#define SCAL_GROUP_KEYS (1ll << 26)   // keys of one group of columns: 256 MB, the bound of the workspace's large part
#define SCAL_CLS_THREADS 1024      // the workgroup that owns a sorted column
#define SCAL_CLS_WAVES (SCAL_CLS_THREADS / 64)
#define SCAL_PER_THREAD 8          // consecutive sorted positions per thread of the prefix count
#define SCAL_SEG (SCAL_CLS_THREADS * SCAL_PER_THREAD)
#define SCAL_TILE 64               // rows x columns of the transposing key builder
#define SCAL_PAD 0xFFFFFFFFu

typedef unsigned int scal_key;

__device__ __forceinline__ scal_key scal_make_key(float v, bool hit) {
    const float c = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;                      // NaN, -0 and negatives -> +0
    return (__float_as_uint(c) << 1) | (hit ? 1u : 0u);
}
__device__ __forceinline__ double scal_value(scal_key k) { return (double)__uint_as_float(k >> 1); }

// ---- softmax into the store: calib_softmax_kernel's arithmetic, row n at probs + n ld ----
__global__ __launch_bounds__(256)
void scal_probs_kernel(const float* __restrict__ logits, float* __restrict__ probs, int64_t ld, int N, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= N) return;
    const float* z = logits + (size_t)b * K;
    float* p = probs + (size_t)b * (size_t)ld;
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, z[k]);
    m = wave_max(m);
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += expf(z[k] - m);
    s = wave_sum(s);
    for (int k = lane; k < K; k += 64) p[k] = expf(z[k] - m) / s;
}

// ---- rows: one wave per row.  conf, pred, correct and nll exactly as calib_conf_rows_kernel; brier = sum_k (p_k - [k == y])^2 in
// double (lane partial sums over k = l, l + 64, ... ascending, then the xor tree).  rowkey = the confidence column's key, rowflag =
// correct | bad << 1 with bad = a label outside [0, K) (nothing is read at it) or a probability that is not finite. ----
__global__ __launch_bounds__(256)
void scal_rows_kernel(const float* __restrict__ probs, int64_t ld, const int64_t* __restrict__ labels, scal_key* __restrict__ rowkey,
                      uint8_t* __restrict__ rowflag, double* __restrict__ row_nll, double* __restrict__ row_brier, int N, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= N) return;
    const float* p = probs + (size_t)b * (size_t)ld;
    const int64_t y = labels[b];
    const bool valid = label_ok(y, K);
    float best = -INFINITY;
    int bi = 0x7FFFFFFF, bad = 0;
    double s = 0.0, br = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float v = p[k];
        const double d = (double)v - ((int64_t)k == y ? 1.0 : 0.0);
        s += (double)v;
        br += d * d;
        bad |= !finite32(v);
        if (v > best) { best = v; bi = k; }
    }
    WAVE_ARGMAX(best, bi);
    s = wave_sum(s);
    br = wave_sum(br);
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) {
        const double eps = 1.1920928955078125e-07;       // torch.finfo(torch.float32).eps
        double q = (valid ? (double)p[y] : 0.0) / s;
        q = q < eps ? eps : (q > 1.0 - eps ? 1.0 - eps : q);
        const bool correct = valid && (int64_t)bi == y;
        row_nll[b] = valid ? -log(q) : quiet_nan();
        row_brier[b] = br;
        rowkey[b] = scal_make_key(best, correct);
        rowflag[b] = (uint8_t)((correct ? 1 : 0) | ((bad || !valid) ? 2 : 0));
    }
}

// ---- keys of a group of columns t0 .. t0 + cols: a 64 x 64 tile of the row-major store is read row by row (64 adjacent classes per
// row segment, 256 bytes) and written column by column, so that column t of the group is the contiguous array keys + (t - t0) P.
// Column K is the confidence column (rowkey).  Positions N .. P hold the padding. ----
__global__ __launch_bounds__(256)
void scal_build_kernel(const float* __restrict__ probs, int64_t ld, const int64_t* __restrict__ labels, const scal_key* __restrict__ rowkey,
                       scal_key* __restrict__ keys, int N, int K, int P, int t0, int cols, int tiles_r) {
    __shared__ scal_key tile[SCAL_TILE][SCAL_TILE + 1];
    const int r0 = (blockIdx.x % tiles_r) * SCAL_TILE, c0 = (blockIdx.x / tiles_r) * SCAL_TILE;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int r = ly; r < SCAL_TILE; r += 4) {
        const int row = r0 + r, cl = c0 + lx, t = t0 + cl;
        scal_key key = SCAL_PAD;
        if (row < N && cl < cols)
            key = t < K ? scal_make_key(probs[(size_t)row * (size_t)ld + t], labels[row] == (int64_t)t) : rowkey[row];
        tile[r][lx] = key;
    }
    __syncthreads();
    for (int c = ly; c < SCAL_TILE; c += 4) {
        const int cl = c0 + c, row = r0 + lx;
        if (cl < cols && row < P) keys[(size_t)cl * P + row] = tile[lx][c];
    }
}

// ---- the bitonic network on 32-bit keys (probe_common.h has the 64-bit one) ----
#define SCAL_CMPX_AT(keys, i, l, asc)                                                 \
    {                                                                                 \
        const scal_key a_ = (keys)[i], b_ = (keys)[l];                                \
        if ((a_ > b_) == (asc)) { (keys)[i] = b_; (keys)[l] = a_; }                   \
    }
__device__ __forceinline__ void scal_cmpx(scal_key& a, scal_key& b, bool asc) {
    if ((a > b) == asc) { const scal_key t = a; a = b; b = t; }
}

// ---- sort, in LDS: workgroup (chunk, column) owns the Lc = min(P, 8192) keys behind chunk * Lc and runs the levels k_lo .. k_hi of
// the network on them, every level from distance min(k, Lc) / 2 down to 1 (larger distances of a level were global passes).  The
// direction of a compare-exchange comes from the key's position in the column; the last two steps of a level (j = 2, 1) run in
// registers on four consecutive keys. ----
__global__ __launch_bounds__(SCAL_SORT_THREADS)
void scal_sort_local_kernel(scal_key* __restrict__ keys, int P, int Lc, int nchunk, int k_lo, int k_hi) {
    __shared__ scal_key sk[SCAL_CHUNK];
    const int tid = threadIdx.x, base = (blockIdx.x % nchunk) * Lc;
    scal_key* kcol = keys + (size_t)(blockIdx.x / nchunk) * P;
    for (int i = tid; i < Lc; i += SCAL_SORT_THREADS) sk[i] = kcol[base + i];
    __syncthreads();
    for (int k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (k >> 1) < (Lc >> 1) ? (k >> 1) : (Lc >> 1); j > 0; j >>= 1) {
            if (j == 2) {
                for (int t = tid; t < (Lc >> 2); t += SCAL_SORT_THREADS) {
                    const bool asc = ((base + 4 * t) & k) == 0;
                    scal_key x0 = sk[4 * t], x1 = sk[4 * t + 1], x2 = sk[4 * t + 2], x3 = sk[4 * t + 3];
                    scal_cmpx(x0, x2, asc); scal_cmpx(x1, x3, asc); scal_cmpx(x0, x1, asc); scal_cmpx(x2, x3, asc);
                    sk[4 * t] = x0; sk[4 * t + 1] = x1; sk[4 * t + 2] = x2; sk[4 * t + 3] = x3;
                }
                __syncthreads();
                break;
            }
            for (int q = tid; q < (Lc >> 1); q += SCAL_SORT_THREADS) {
                const int i = BITONIC_LO(q, j), l = i | j;
                SCAL_CMPX_AT(sk, i, l, ((base + i) & k) == 0);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < Lc; i += SCAL_SORT_THREADS) kcol[base + i] = sk[i];
}

// ---- sort, one global pass: the compare-exchange of level k at distance j >= 8192, one pair per thread, every column of the group ----
__global__ __launch_bounds__(256)
void scal_sort_global_kernel(scal_key* __restrict__ keys, int P, int cols, int k, int j) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const int half = P >> 1;
    if (g >= (long long)cols * half) return;
    scal_key* kcol = keys + (size_t)(g / half) * P;
    const int q = (int)(g % half), i = BITONIC_LO(q, j), l = i | j;
    SCAL_CMPX_AT(kcol, i, l, (i & k) == 0);
}

// ---- a sorted column: positions [0, N) ascending, the padding behind ----
struct ScalBounds { double v[SCAL_MAX_BINS + 1]; };
struct ScalParams {
    ScalBounds ece, cw;
    double thr;
    int ece_bins, cw_bins, ace_bins, tace_bins;
};

// first position in [0, N] whose value, widened, is > x (above == 1) or is not < x (above == 0)
__device__ __forceinline__ int scal_first(const scal_key* __restrict__ kcol, int N, double x, int above) {
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double v = scal_value(kcol[mid]);
        if (above ? (v > x) : !(v < x)) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// first position in [0, hi] whose key is >= key
__device__ __forceinline__ int scal_first_key(const scal_key* __restrict__ kcol, int hi, scal_key key) {
    int lo = 0;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (kcol[mid] >= key) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// one past the last position of the run of `key` that starts at a: gallop, then bisect
__device__ __forceinline__ int scal_run_end(const scal_key* __restrict__ kcol, int a, int N, scal_key key) {
    int lo = a, step = 1;
    while (lo + step < N && kcol[lo + step] == key) { lo += step; step <<= 1; }
    int hi = lo + step < N ? lo + step : N;                  // the key at hi differs, or hi == N
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (kcol[mid] == key) lo = mid; else hi = mid;
    }
    return lo + 1;
}

// ---- one workgroup per sorted column t = t0 + blockIdx.x.
// Class column (t < K).  AUROC: the first positive r of a tie group owns the group's positives [r, e).  With q the group's first
// position, [q, r) are its negatives, so negatives below = q - (positives before r), ties = r - q, and the group adds
// (e - r) (2 (q - pos_before) + (r - q)) to the int64 numerator of 2 #{pos > neg} + #{pos == neg}.  pos_before is the exclusive prefix
// count of the positives: 8192 positions per round, 8 consecutive positions per thread.
// Runs: SCE's bin i is [first > cw_i, first > cw_{i+1}); an adaptive family (ACE: threshold 0, TACE) has z = #{v < threshold}, the
// thresholded sorted value sv(j) = j < z ? 0 : v(j), bounds lo_i = sv(i (N / bins)), up_i = lo_{i+1} or 1.0, and bin i is
// [max(z, first > lo_i), max(z, first > up_i)).  Wave w takes the runs w, w + 16, ...; a bin's score is count / N |sum / count - hits /
// count|, a class value the sum of the scores in bin order by one thread.  per_class (K, 6) = SCE_c, ACE_c, TACE_c, AUROC_c, n_pos,
// N - z of TACE.
// Confidence column (t == K): the runs of the ece bounds give top_table (bins, 3) = (count / N, hits / count, sum / count). ----
__global__ __launch_bounds__(SCAL_CLS_THREADS)
void scal_class_kernel(const scal_key* __restrict__ keys, ScalParams pr, double* __restrict__ per_class, double* __restrict__ top_table,
                       int N, int K, int P, int t0) {
    __shared__ int wtot[SCAL_CLS_WAVES];
    __shared__ long long wnum[SCAL_CLS_WAVES];
    __shared__ double score[3][SCAL_MAX_BINS];
    __shared__ int zt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = t0 + (int)blockIdx.x;
    const scal_key* kcol = keys + (size_t)blockIdx.x * P;
    const bool top = t >= K;
    long long num = 0;
    int n_pos = 0;
    if (!top) {
        for (int s0 = 0; s0 < N; s0 += SCAL_SEG) {
            const int p0 = s0 + tid * SCAL_PER_THREAD;
            scal_key k[SCAL_PER_THREAD];
            int mine = 0;
#pragma unroll
            for (int r = 0; r < SCAL_PER_THREAD; ++r) {
                k[r] = p0 + r < N ? kcol[p0 + r] : SCAL_PAD;
                mine += (p0 + r < N) ? (int)(k[r] & 1u) : 0;
            }
            int incl = mine;                                 // inclusive scan over the wave's threads
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            int run = n_pos + incl - mine, seg_total = 0;
            for (int w = 0; w < SCAL_CLS_WAVES; ++w) {
                if (w < wave) run += wtot[w];
                seg_total += wtot[w];
            }
            scal_key prev = (p0 > 0 && p0 - 1 < N) ? kcol[p0 - 1] : SCAL_PAD;
#pragma unroll
            for (int r = 0; r < SCAL_PER_THREAD; ++r) {
                const int p = p0 + r;
                if (p < N) {
                    const scal_key key = k[r];
                    if ((key & 1u) && (p == 0 || key != prev)) {
                        const int q = (p > 0 && (prev >> 1) == (key >> 1)) ? scal_first_key(kcol, p, key & ~1u) : p;
                        const int e = scal_run_end(kcol, p, N, key);
                        num += (long long)(e - p) * (2ll * (long long)(q - run) + (long long)(p - q));
                    }
                    run += (int)(key & 1u);
                    prev = key;
                }
            }
            n_pos += seg_total;
            __syncthreads();                                 // wtot is written again in the next round
        }
        num = wave_sum(num);
        if (lane == 0) wnum[wave] = num;
    }
    // runs
    const int nb0 = top ? pr.ece_bins : pr.cw_bins, nb1 = top ? 0 : pr.ace_bins, nb2 = top ? 0 : pr.tace_bins;
    for (int r = wave; r < nb0 + nb1 + nb2; r += SCAL_CLS_WAVES) {
        const int f = r < nb0 ? 0 : (r < nb0 + nb1 ? 1 : 2), i = r - (f == 0 ? 0 : (f == 1 ? nb0 : nb0 + nb1));
        int a, b;
        if (f == 0) {
            const ScalBounds& bd = top ? pr.ece : pr.cw;
            a = scal_first(kcol, N, bd.v[i], 1);
            b = scal_first(kcol, N, bd.v[i + 1], 1);
        } else {
            const int bins = f == 1 ? nb1 : nb2, bin_n = N / bins;       // 0 when N < bins: every lower bound is the column minimum
            const int z = scal_first(kcol, N, f == 1 ? 0.0 : pr.thr, 0);
            const int jl = i * bin_n, ju = (i + 1) * bin_n;
            const double lo = jl < z ? 0.0 : scal_value(kcol[jl]);
            const double up = i + 1 < bins ? (ju < z ? 0.0 : scal_value(kcol[ju])) : 1.0;
            a = scal_first(kcol, N, lo, 1);
            b = scal_first(kcol, N, up, 1);
            a = a < z ? z : a;
            b = b < z ? z : b;
            if (f == 2 && i == 0 && lane == 0) zt = z;
        }
        if (b < a) b = a;
        double sum = 0.0;
        int hits = 0;
        for (int j = a + lane; j < b; j += 64) {
            const scal_key key = kcol[j];
            sum += scal_value(key);
            hits += (int)(key & 1u);
        }
        sum = wave_sum(sum);
        hits = wave_sum(hits);
        if (lane == 0) {
            const int cnt = b - a;
            const double prop = (double)cnt / (double)N, acc = cnt ? (double)hits / (double)cnt : 0.0, conf = cnt ? sum / (double)cnt : 0.0;
            if (top) {
                top_table[3 * i] = prop; top_table[3 * i + 1] = acc; top_table[3 * i + 2] = conf;
            } else {
                score[f][i] = cnt ? prop * fabs(conf - acc) : 0.0;
            }
        }
    }
    __syncthreads();
    if (top) return;
    double* o = per_class + 6 * (size_t)t;
    if (tid < 3) {
        const int bins = tid == 0 ? nb0 : (tid == 1 ? nb1 : nb2);
        double acc = 0.0;
        for (int i = 0; i < bins; ++i) acc += score[tid][i];
        o[tid] = acc;
    } else if (tid == 3) {
        long long u2 = 0;
        for (int w = 0; w < SCAL_CLS_WAVES; ++w) u2 += wnum[w];
        const int n_neg = N - n_pos;
        o[3] = (n_pos > 0 && n_neg > 0) ? (double)u2 / (2.0 * (double)n_pos * (double)n_neg) : quiet_nan();
        o[4] = (double)n_pos;
        o[5] = (double)(N - zt);
    }
}

// ---- the set's numbers: one workgroup.  A sum over rows or classes: thread t adds the elements t, t + 1024, ... ascending, the xor
// tree adds a wave's threads and every thread adds the 16 waves in order. ----
__device__ __forceinline__ double scal_block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < SCAL_CLS_WAVES; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ int scal_block_sum(int v, double* red) { return (int)scal_block_sum((double)v, red); }   // counts <= 2^30: exact

__global__ __launch_bounds__(SCAL_CLS_THREADS)
void scal_finish_kernel(const scal_key* __restrict__ rowkey, const uint8_t* __restrict__ rowflag, const double* __restrict__ row_nll,
                        const double* __restrict__ row_brier, const double* __restrict__ per_class, const double* __restrict__ top_table,
                        int ece_bins, double* __restrict__ out, int N, int K) {
    __shared__ double red[SCAL_CLS_WAVES];
    const int tid = threadIdx.x;
    double nll = 0.0, br = 0.0, cf = 0.0;
    int corr = 0, bad = 0;
    for (int n = tid; n < N; n += SCAL_CLS_THREADS) {
        const unsigned int f = rowflag[n];
        nll += row_nll[n];
        br += row_brier[n];
        cf += scal_value(rowkey[n]);
        corr += (int)(f & 1u);
        bad += (int)((f >> 1) & 1u);
    }
    nll = scal_block_sum(nll, red); br = scal_block_sum(br, red); cf = scal_block_sum(cf, red);
    corr = scal_block_sum(corr, red); bad = scal_block_sum(bad, red);
    double sce = 0.0, ace = 0.0, tace = 0.0, auc = 0.0;
    int have = 0;
    for (int c = tid; c < K; c += SCAL_CLS_THREADS) {
        const double* p = per_class + 6 * (size_t)c;
        sce += p[0]; ace += p[1]; tace += p[2];
        if (p[3] == p[3]) { auc += p[3]; ++have; }
    }
    sce = scal_block_sum(sce, red); ace = scal_block_sum(ace, red); tace = scal_block_sum(tace, red); auc = scal_block_sum(auc, red);
    have = scal_block_sum(have, red);
    if (tid == 0) {
        double ece = 0.0, mce = 0.0, oe = 0.0;
        for (int i = 0; i < ece_bins; ++i) {
            const double prop = top_table[3 * i], acc = top_table[3 * i + 1], conf = top_table[3 * i + 2], gap = fabs(conf - acc);
            ece += prop * gap;
            mce = gap > mce ? gap : mce;
            oe += prop * (conf * (conf - acc > 0.0 ? conf - acc : 0.0));
        }
        const double n = (double)N, k = (double)K, nan = quiet_nan();
        const double v[12] = {ece, mce, oe, nll / n, br / n, sce / k, ace / k, tace / k, have ? auc / (double)have : nan, (double)have,
                              (double)corr / n, cf / n};
        for (int i = 0; i < 12; ++i) out[i] = bad ? nan : v[i];
        out[12] = n; out[13] = (double)bad; out[14] = 0.0; out[15] = 0.0;
    }
}

// ---- launchers: arguments are validated before anything touches the device ----
struct ScalLayout { int P, Lc, G; size_t row_nll, row_brier, rowkey, rowflag, keys, fixed, total; };

static inline bool scal_set_ok(int N, int K) { return N >= 1 && N <= SCAL_MAX_N && K >= 1 && (long long)N * (long long)K <= SCAL_MAX_NK; }

// G = columns per group: all K + 1 when they fit SCAL_GROUP_KEYS keys (at least 64 columns do: P <= 2^20)
static inline ScalLayout scal_layout(int N, int K) {
    ScalLayout d;
    d.P = 1;
    while (d.P < N) d.P <<= 1;
    d.Lc = d.P < SCAL_CHUNK ? d.P : SCAL_CHUNK;
    const long long T = (long long)K + 1, fit = SCAL_GROUP_KEYS / d.P;
    d.G = (int)(T < fit ? T : fit);
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align16(bytes); return here; };
    d.row_nll = take((size_t)N * sizeof(double));
    d.row_brier = take((size_t)N * sizeof(double));
    d.rowkey = take((size_t)N * sizeof(scal_key));
    d.rowflag = take((size_t)N);
    d.fixed = at;
    d.keys = take((size_t)d.G * d.P * sizeof(scal_key));
    d.total = at;
    return d;
}

// launches of one group of columns: the key builder, the sort, the column owner
static inline int scal_group_launches(const ScalLayout& d) {
    int n = 3;
    for (int k = d.Lc << 1; k <= d.P; k <<= 1) {
        for (int j = k >> 1; j >= d.Lc; j >>= 1) ++n;
        ++n;
    }
    return n;
}

extern "C" int uvit_op_scal_probs(const float* logits, float* probs, int64_t ld, int N, int K, uvit_stream stream) {
    if (!logits || !probs) return UVIT_ERR_ARG;
    if (N < 1 || K < 1 || ld < (int64_t)K) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(scal_probs_kernel, WavePerRow::grid(N), WavePerRow::block(), 0, (hipStream_t)stream, logits, probs, ld, N, K);
    return uvit_check_launch();
}

extern "C" int64_t uvit_op_scal_ws_bytes(int N, int K) {
    if (!scal_set_ok(N, K)) return UVIT_ERR_SHAPE;
    return (int64_t)scal_layout(N, K).total;
}

extern "C" int64_t uvit_op_scal_launches(int N, int K, int64_t ws_bytes) {
    if (!scal_set_ok(N, K)) return UVIT_ERR_SHAPE;
    ScalLayout d = scal_layout(N, K);
    const long long room = (ws_bytes - (long long)d.fixed) / ((long long)d.P * (long long)sizeof(scal_key));
    if (room < 1) return UVIT_ERR_WORKSPACE;
    const long long G = room < d.G ? room : d.G, T = (long long)K + 1;
    return 2 + (T + G - 1) / G * scal_group_launches(d);
}

extern "C" int uvit_op_scal_metrics(const float* probs, int64_t ld, const int64_t* labels, int N, int K, const double* ece_bounds, int ece_bins,
                                    const double* cw_bounds, int cw_bins, int ace_bins, int tace_bins, double tace_threshold, double* out,
                                    double* top_table, double* per_class, void* ws, int64_t ws_bytes, uvit_stream stream) {
    if (!probs || !labels || !ece_bounds || !cw_bounds || !out || !top_table || !per_class || !ws || misaligned(ws, 16)) return UVIT_ERR_ARG;
    if (!(tace_threshold == tace_threshold)) return UVIT_ERR_ARG;
    if (!scal_set_ok(N, K) || ld < (int64_t)K) return UVIT_ERR_SHAPE;
    const int bins[4] = {ece_bins, cw_bins, ace_bins, tace_bins};
    for (int i = 0; i < 4; ++i)
        if (bins[i] < 1 || bins[i] > SCAL_MAX_BINS) return UVIT_ERR_SHAPE;
    const ScalLayout d = scal_layout(N, K);
    const long long room = (ws_bytes - (long long)d.fixed) / ((long long)d.P * (long long)sizeof(scal_key));
    if (room < 1) return UVIT_ERR_WORKSPACE;
    const int G = (int)(room < d.G ? room : d.G), T = K + 1;
    ScalParams pr;                                           // travels by value: the call stays asynchronous
    for (int i = 0; i <= SCAL_MAX_BINS; ++i) {
        pr.ece.v[i] = i <= ece_bins ? ece_bounds[i] : 0.0;
        pr.cw.v[i] = i <= cw_bins ? cw_bounds[i] : 0.0;
    }
    pr.thr = tace_threshold; pr.ece_bins = ece_bins; pr.cw_bins = cw_bins; pr.ace_bins = ace_bins; pr.tace_bins = tace_bins;
    char* w = (char*)ws;
    double *row_nll = (double*)(w + d.row_nll), *row_brier = (double*)(w + d.row_brier);
    scal_key *rowkey = (scal_key*)(w + d.rowkey), *keys = (scal_key*)(w + d.keys);
    uint8_t* rowflag = (uint8_t*)(w + d.rowflag);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(scal_rows_kernel, WavePerRow::grid(N), WavePerRow::block(), 0, st, probs, ld, labels, rowkey, rowflag, row_nll, row_brier, N, K);
    const int tiles_r = (d.P + SCAL_TILE - 1) / SCAL_TILE, nchunk = d.P / d.Lc;
    for (int t0 = 0; t0 < T; t0 += G) {
        const int cols = T - t0 < G ? T - t0 : G;
        const unsigned int pair_blocks = (unsigned int)(((long long)cols * (d.P / 2) + 255) / 256);
        hipLaunchKernelGGL(scal_build_kernel, dim3((unsigned int)tiles_r * (unsigned int)((cols + SCAL_TILE - 1) / SCAL_TILE)), dim3(256), 0, st,
                           probs, ld, labels, (const scal_key*)rowkey, keys, N, K, d.P, t0, cols, tiles_r);
        // 1 launch sorts every chunk; then per level k > chunk: log2(k / chunk) global passes and 1 launch that finishes the level in LDS
        hipLaunchKernelGGL(scal_sort_local_kernel, dim3((unsigned int)nchunk * (unsigned int)cols), dim3(SCAL_SORT_THREADS), 0, st, keys, d.P, d.Lc,
                           nchunk, 2, d.Lc);
        for (int k = d.Lc << 1; k <= d.P; k <<= 1) {
            for (int j = k >> 1; j >= d.Lc; j >>= 1)
                hipLaunchKernelGGL(scal_sort_global_kernel, dim3(pair_blocks), dim3(256), 0, st, keys, d.P, cols, k, j);
            hipLaunchKernelGGL(scal_sort_local_kernel, dim3((unsigned int)nchunk * (unsigned int)cols), dim3(SCAL_SORT_THREADS), 0, st, keys, d.P,
                               d.Lc, nchunk, k, k);
        }
        hipLaunchKernelGGL(scal_class_kernel, dim3(cols), dim3(SCAL_CLS_THREADS), 0, st, (const scal_key*)keys, pr, per_class, top_table, N, K, d.P, t0);
    }
    hipLaunchKernelGGL(scal_finish_kernel, dim3(1), dim3(SCAL_CLS_THREADS), 0, st, (const scal_key*)rowkey, (const uint8_t*)rowflag,
                       (const double*)row_nll, (const double*)row_brier, (const double*)per_class, (const double*)top_table, ece_bins, out, N, K);
    return uvit_check_launch();
}
