// Calibration metrics of a classifier's batch on the device (gfx950): what the reference's evaluate() reports beside Acc@1 / Acc@5
//   ECE, bin table   uncertainty_evaluations.py:134-202      MaxProbCELoss / ECELoss: 15 equal-width confidence bins
//   TACE             uncertainty_evaluations.py:112-132,159-186,241-261   per class: threshold, adaptive bins of B / n_bins sorted values
//   NLL              uncertainty_evaluations.py:270-272      -Categorical(softmax).log_prob(target).mean()
//   AUROC            one-vs-rest over the classes present in the batch (DESIGN.md section 9 on torchmetrics' convention)
// uvit_op_calib_softmax is the only place where logits become probabilities; the three metric ops take probs (B, K) fp32.
// Comparisons: an fp32 probability is widened to double and compared with a double bound (the host's np.linspace values for ECE, the
// threshold for TACE, elements of the column itself for TACE's adaptive bins), so bin membership is exactly what a float64
// restatement finds on the same fp32 values; only the sums carry round-off.  No float atomics: every floating sum has one owner and
// a fixed order (stated at each kernel), so the same input gives the same bits on every run.  The kernels are launch-bound (< 1 MB of
// input), hence double arithmetic wherever a sum is formed.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums and the IEEE comparisons are part of the contract.
#ifdef __FAST_MATH__
#error "calib.hip fixes the order of its sums and compares in IEEE double: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define CALIB_MAX_B 1024
#define CALIB_MAX_BINS 64
#define TACE_THREADS 1024    // 16 waves: the sorting network is a chain of LDS round trips, hidden by waves and by nothing else


// 1 when any label lies outside [0, K); every lane of the wave gets the answer
__device__ __forceinline__ int any_bad_label(const int64_t* __restrict__ labels, int B, int K, int lane) {
    int bad = 0;
    for (int b = lane; b < B; b += 64) {
        const int64_t y = labels[b];
        bad |= !label_ok(y, K);
    }
    return __any(bad) ? 1 : 0;
}

// ---- softmax: fp32, max-shifted, one wave per row; lane l adds its terms k = l, l + 64, ... in ascending order, then the xor tree ----
__global__ __launch_bounds__(256)
void calib_softmax_kernel(const float* __restrict__ logits, float* __restrict__ probs, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* z = logits + (size_t)b * K;
    float* p = probs + (size_t)b * K;
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, z[k]);
    m = wave_max(m);
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += expf(z[k] - m);
    s = wave_sum(s);
    for (int k = lane; k < K; k += 64) p[k] = expf(z[k] - m) / s;
}

// ---- confidence, rows: one wave per row.  conf = max_k p, pred = the lowest index attaining it, correct = (pred == y);
// nll = -log(clamp(p_y / sum_k p_k, eps, 1 - eps)), eps = 2^-23, sum and quotient in double (lane partial sums over k = l, l + 64, ...
// ascending, then the xor tree).  A label outside [0, K): nll is NaN, correct 0, nothing is read at the label. ----
__global__ __launch_bounds__(256)
void calib_conf_rows_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels, float* __restrict__ row_conf,
                            int* __restrict__ row_pred_correct, double* __restrict__ row_nll, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* p = probs + (size_t)b * K;
    const int64_t y = labels[b];
    const bool valid = label_ok(y, K);
    float best = -INFINITY;
    int bi = 0x7FFFFFFF;
    double s = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float v = p[k];
        s += (double)v;
        if (v > best) { best = v; bi = k; }
    }
    WAVE_ARGMAX(best, bi);
    s = wave_sum(s);
    if (lane == 0) {
        const double eps = 1.1920928955078125e-07;       // torch.finfo(torch.float32).eps
        double q = (valid ? (double)p[y] : 0.0) / s;
        q = q < eps ? eps : (q > 1.0 - eps ? 1.0 - eps : q);
        row_nll[b] = valid ? -log(q) : quiet_nan();
        row_conf[b] = best;
        row_pred_correct[b] = bi;
        row_pred_correct[B + b] = (valid && (int64_t)bi == y) ? 1 : 0;
    }
}

static_assert(TACE_THREADS >= CALIB_MAX_BINS * 16, "calib_tace_kernel: one thread per (bin, class) of a group of up to 16 classes");

struct CalibBounds { double v[CALIB_MAX_BINS + 1]; };

// Bin accuracy as the reference computes it (uncertainty_evaluations.py:184): its `in_bin` is a uint8 0/1 array and `accuracies` a
// numpy array, so `accuracies[in_bin]` picks rows 0 and 1 BY POSITION and the mean runs over all B rows:
// (count a[1] + (B - count) a[0]) / B, with a[b] the hit flag of row b.  At B = 1 the reference cannot index row 1; a1 is then a0.
__device__ __forceinline__ double positional_bin_acc(int cnt, int B, int a0, int a1) {
    return ((double)cnt * (double)a1 + (double)(B - cnt) * (double)a0) / (double)B;
}

// ---- confidence, bins: one wave.  Lane i < n_bins owns bin i and walks the rows in row order; ECE is added in bin order by lane 0;
// NLL is the mean of row_nll in row order, 64 rows at a time through the xor tree. ----
__global__ __launch_bounds__(64)
void calib_conf_bins_kernel(const float* __restrict__ row_conf, const int* __restrict__ row_pred_correct, const double* __restrict__ row_nll,
                            const int64_t* __restrict__ labels, CalibBounds bd, int n_bins, int positional_acc,
                            double* __restrict__ table, double* __restrict__ ece_nll, int B, int K) {
    __shared__ double score[CALIB_MAX_BINS];
    const int lane = threadIdx.x;
    if (lane < n_bins) {
        const double lo = bd.v[lane], up = bd.v[lane + 1];
        int cnt = 0, hit = 0;
        double sum = 0.0;
        for (int b = 0; b < B; ++b) {
            const double c = (double)row_conf[b];
            if (c > lo && c <= up) { ++cnt; hit += row_pred_correct[B + b]; sum += c; }
        }
        const double prop = (double)cnt / (double)B;
        const double conf = cnt ? sum / (double)cnt : 0.0;
        const double acc = !cnt ? 0.0 : positional_acc ? positional_bin_acc(cnt, B, row_pred_correct[B], row_pred_correct[B + (B > 1)])
                                                       : (double)hit / (double)cnt;
        table[3 * lane] = prop; table[3 * lane + 1] = acc; table[3 * lane + 2] = conf;
        score[lane] = cnt ? prop * fabs(conf - acc) : 0.0;
    }
    const int bad = any_bad_label(labels, B, K, lane);
    double nll = 0.0;
    for (int b0 = 0; b0 < B; b0 += 64) nll += wave_sum(b0 + lane < B ? row_nll[b0 + lane] : 0.0);
    __syncthreads();
    if (lane == 0) {
        double ece = 0.0;
        for (int i = 0; i < n_bins; ++i) ece += score[i];
        ece_nll[0] = bad ? quiet_nan() : ece;
        ece_nll[1] = nll / (double)B;
    }
}

// ---- TACE: one workgroup per group of CG = 2^cg_shift adjacent classes, so that every row of the row-major matrix is read as one
// CG x 4-byte segment.  The thresholded columns are sorted in LDS as 64-bit keys (order-preserving image of the fp32 value << 32 |
// [y_b == c]) by a bitonic network over P = B rounded up to a power of two, padded with all-ones keys; the layout is keys[row][class],
// class fastest, so a 32-lane group touches 32 consecutive keys in the load, in both sides of every compare-exchange and in no step
// more than two rows of one bank.  In sorted order bin i = {lo_i < v <= up_i} is the contiguous run behind the copies of lo_i that
// starts at or after i * bin_n, so the owner of (class, bin) walks it once, ascending: equal values commute exactly, hence the sum
// does not depend on how the network ordered ties.  Class value = sum over bins in bin order, one owner thread per class. ----
__device__ __forceinline__ double tace_key_value(unsigned long long key) {
    return (double)key32_value((unsigned int)(key >> 32));
}

__global__ __launch_bounds__(TACE_THREADS)
void calib_tace_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels, double thr, int n_bins, int positional_acc,
                       double* __restrict__ per_class, int B, int K, int P, int cg_shift) {
    extern __shared__ unsigned long long keys[];          // max(P, n_bins) << cg_shift entries (the launcher sizes it)
    const int CG = 1 << cg_shift, cmask = CG - 1, c0 = blockIdx.x * CG, tid = threadIdx.x;
    for (int idx = tid; idx < (P << cg_shift); idx += TACE_THREADS) {
        const int j = idx >> cg_shift, c = c0 + (idx & cmask);
        unsigned long long key = ~0ull;
        if (j < B && c < K) {
            const float p = probs[(size_t)j * K + c];
            const float v = ((double)p < thr) ? 0.f : p;
            key = ((unsigned long long)key32(v) << 32) | (unsigned long long)(labels[j] == (int64_t)c);
        }
        keys[idx] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < ((P >> 1) << cg_shift); idx += TACE_THREADS) {
                const int q = idx >> cg_shift, cc = idx & cmask;
                const int i = BITONIC_LO(q, j), l = i | j;
                BITONIC_CMPX_AT(keys, (i << cg_shift) + cc, (l << cg_shift) + cc, (i & k) == 0);
            }
            __syncthreads();
        }
    }
    const int bin_n = B / n_bins;                         // 0 when B < n_bins: every lower bound is the column minimum, as in the reference
    double r = 0.0;                                       // thread tid owns (bin, class) = (tid / CG, tid % CG): n_bins * CG <= 64 * 16
    const int i = tid >> cg_shift, cc = tid & cmask;
    if (i < n_bins && c0 + cc < K) {
        const double lo = tace_key_value(keys[((i * bin_n) << cg_shift) + cc]);
        const double up = i + 1 < n_bins ? tace_key_value(keys[(((i + 1) * bin_n) << cg_shift) + cc]) : 1.0;
        int j = i * bin_n, cnt = 0, pos = 0;
        double sum = 0.0;
        while (j < B && tace_key_value(keys[(j << cg_shift) + cc]) <= lo) ++j;
        while (j < B) {
            const unsigned long long key = keys[(j << cg_shift) + cc];
            const double v = tace_key_value(key);
            if (!(v <= up)) break;
            ++cnt; pos += (int)(key & 1ull); sum += v;
            ++j;
        }
        if (cnt) {
            const int64_t c = (int64_t)(c0 + cc);
            const double acc = positional_acc ? positional_bin_acc(cnt, B, labels[0] == c, labels[B > 1] == c) : (double)pos / (double)cnt;
            r = ((double)cnt / (double)B) * fabs(sum / (double)cnt - acc);
        }
    }
    __syncthreads();                                      // every walk is over: the key array becomes the (bin, class) score table
    double* score = (double*)keys;
    if (tid < (n_bins << cg_shift)) score[tid] = r;
    __syncthreads();
    if (tid < CG && c0 + tid < K) {
        double acc = 0.0;
        for (int bin = 0; bin < n_bins; ++bin) acc += score[(bin << cg_shift) + tid];
        per_class[c0 + tid] = acc;
    }
}

// TACE = (sum_c per_class[c]) / K: one wave, class order, 64 classes at a time through the xor tree
__global__ __launch_bounds__(64)
void calib_tace_mean_kernel(const double* __restrict__ per_class, const int64_t* __restrict__ labels, double* __restrict__ tace, int B, int K) {
    const int lane = threadIdx.x;
    const int bad = any_bad_label(labels, B, K, lane);
    double acc = 0.0;
    for (int c0 = 0; c0 < K; c0 += 64) acc += wave_sum(c0 + lane < K ? per_class[c0 + lane] : 0.0);
    if (lane == 0) *tace = bad ? quiet_nan() : acc / (double)K;
}

// ---- AUROC, rows: one wave per sample i walks column y_i.  u2_i = sum over j with y_j != y_i of 2 [p_i > p_j] + [p_i == p_j]
// (integers: 2 B^2 <= 2^21), n_pos = the number of rows that carry y_i, first = no earlier row carries it.  rows = int32[3 B]:
// u2 | n_pos | first.  A row with a label outside [0, K) writes zeros and reads no probability. ----
__global__ __launch_bounds__(256)
void calib_auroc_rows_kernel(const float* __restrict__ probs, const int64_t* __restrict__ labels, int* __restrict__ rows, int B, int K) {
    const int lane = WavePerRow::lane(), i = WavePerRow::row();
    if (i >= B) return;
    const int64_t y = labels[i];
    const bool valid = label_ok(y, K);
    int u2 = 0, npos = 0, earlier = 0;
    if (valid) {
        const double pi = (double)probs[(size_t)i * K + y];
        for (int j = lane; j < B; j += 64) {
            if (labels[j] == y) {
                ++npos;
                earlier += j < i;
            } else {
                const double pj = (double)probs[(size_t)j * K + y];
                u2 += 2 * (pi > pj) + (pi == pj);
            }
        }
    }
    u2 = wave_sum(u2); npos = wave_sum(npos); earlier = wave_sum(earlier);
    if (lane == 0) {
        rows[i] = u2;
        rows[B + i] = npos;
        rows[2 * B + i] = (valid && earlier == 0) ? 1 : 0;
    }
}

// out[0] = sum over samples, in sample order (64 at a time through the xor tree), of u2_i / (2 n_pos n_neg) = sum_c AUC_c over the
// classes with a positive and a negative row; out[1] = how many such classes, each counted at the first sample that carries it
__global__ __launch_bounds__(64)
void calib_auroc_finish_kernel(const int* __restrict__ rows, const int64_t* __restrict__ labels, double* __restrict__ out, int B, int K) {
    const int lane = threadIdx.x;
    const int bad = any_bad_label(labels, B, K, lane);
    double sum = 0.0;
    int count = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int i = b0 + lane;
        double term = 0.0;
        int first = 0;
        if (i < B) {
            const int npos = rows[B + i], nneg = B - npos;
            if (npos >= 1 && nneg >= 1) {
                term = (double)rows[i] / (2.0 * (double)npos * (double)nneg);
                first = rows[2 * B + i];
            }
        }
        sum += wave_sum(term);
        count += wave_sum(first);
    }
    if (lane == 0) {
        out[0] = bad ? quiet_nan() : sum;
        out[1] = (double)count;
    }
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool calib_shape_ok(int B, int K) { return B >= 1 && B <= CALIB_MAX_B && K >= 1; }

extern "C" int uvit_op_calib_softmax(const float* logits, float* probs, int B, int K, uvit_stream stream) {
    if (!logits || !probs) return UVIT_ERR_ARG;
    if (!calib_shape_ok(B, K)) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(calib_softmax_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, (hipStream_t)stream, logits, probs, B, K);
    return uvit_check_launch();
}

extern "C" int uvit_op_calib_confidence(const float* probs, const int64_t* labels, const double* bounds, int n_bins, int positional_acc, float* row_conf,
                                        int32_t* row_pred_correct, double* row_nll, double* bin_table, double* ece_nll, int B, int K,
                                        uvit_stream stream) {
    if (!probs || !labels || !bounds || !row_conf || !row_pred_correct || !row_nll || !bin_table || !ece_nll || (positional_acc & ~1)) return UVIT_ERR_ARG;
    if (!calib_shape_ok(B, K) || n_bins < 1 || n_bins > CALIB_MAX_BINS) return UVIT_ERR_SHAPE;
    CalibBounds bd;
    for (int i = 0; i <= CALIB_MAX_BINS; ++i) bd.v[i] = i <= n_bins ? bounds[i] : 0.0;      // travels by value: the call stays asynchronous
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(calib_conf_rows_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, probs, labels, row_conf, (int*)row_pred_correct, row_nll, B, K);
    hipLaunchKernelGGL(calib_conf_bins_kernel, dim3(1), dim3(64), 0, s, (const float*)row_conf, (const int*)row_pred_correct,
                       (const double*)row_nll, labels, bd, n_bins, positional_acc, bin_table, ece_nll, B, K);
    return uvit_check_launch();
}

extern "C" int uvit_op_calib_tace(const float* probs, const int64_t* labels, double threshold, int n_bins, int positional_acc, double* per_class, double* tace,
                                  int B, int K, uvit_stream stream) {
    if (!probs || !labels || !per_class || !tace || (positional_acc & ~1)) return UVIT_ERR_ARG;
    if (!calib_shape_ok(B, K) || n_bins < 1 || n_bins > CALIB_MAX_BINS) return UVIT_ERR_SHAPE;
    int P = 1;
    while (P < B) P <<= 1;
    const int cg_shift = P <= 256 ? 4 : (P == 512 ? 3 : 2);                                  // at most 4096 keys = 32 KB of LDS
    const int CG = 1 << cg_shift;
    const size_t lds = (size_t)(P > n_bins ? P : n_bins) * CG * sizeof(unsigned long long);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(calib_tace_kernel, dim3((K + CG - 1) / CG), dim3(TACE_THREADS), lds, s, probs, labels, threshold, n_bins, positional_acc, per_class, B, K, P, cg_shift);
    hipLaunchKernelGGL(calib_tace_mean_kernel, dim3(1), dim3(64), 0, s, (const double*)per_class, labels, tace, B, K);
    return uvit_check_launch();
}

extern "C" int uvit_op_calib_auroc(const float* probs, const int64_t* labels, int32_t* rows, double* out, int B, int K, uvit_stream stream) {
    if (!probs || !labels || !rows || !out) return UVIT_ERR_ARG;
    if (!calib_shape_ok(B, K)) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(calib_auroc_rows_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, probs, labels, (int*)rows, B, K);
    hipLaunchKernelGGL(calib_auroc_finish_kernel, dim3(1), dim3(64), 0, s, (const int*)rows, labels, out, B, K);
    return uvit_check_launch();
}
