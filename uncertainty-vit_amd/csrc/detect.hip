// Set-level detection metrics of per-sample uncertainty scores on the device (gfx950): does a score rank the wrong predictions (or
// the images of another data set) above the rest?  DESIGN.md section 9.6.
//   uvit_op_detect_rows     per batch, one wave per row of the logits: 1 - max softmax, softmax entropy, -logsumexp and the
//                           wrong-prediction flag, written at the batch's offset of the set-level store
//   uvit_op_detect_column   per batch: a head's own per-sample column (float or double, strided) into the store as fp32
//   uvit_op_detect_metrics  per evaluation: every column sorted over the whole set (a bitonic network that spans workgroups), a
//                           prefix count of the positives in sorted order, then AUROC, AUPR (average precision), FPR at 95 % TPR
//                           and AURC (area under the risk-coverage curve) with ties grouped
// Keys are 64-bit and strictly ordered: order-preserving image of the fp32 score << 32 | sample index << 2 | bad-label bit << 1 |
// positive bit.  No two keys are equal, so the sorted array is a function of the input alone, whatever network or launch shape
// produced it.  -0 is ranked as +0 (equal scores are one tie group, as a comparison of the values finds them); a NaN score gets
// the image 0xFFFFFFFF, above +inf, and sorts behind every number in index order, in front of the padding (all ones).
// No float atomics and no atomics at all: integer counts and floating sums alike have one owner per segment and are added in segment
// order by one thread, so two calls give the same bits.  No workgroup waits for another: every dependency between workgroups is a
// kernel boundary.  Compiled WITHOUT -ffast-math (build.sh): NaN is found with v != v, the row scores need the accurate expf and
// the order of the sums is part of the contract.
#ifdef __FAST_MATH__
#error "detect.hip finds NaN scores with v != v and fixes the order of its sums: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define DET_MAX_N (1 << 20)
#define DET_MAX_S 16
#define DET_CHUNK 4096           // keys a workgroup sorts in LDS: 32 KB
#define DET_SORT_THREADS 1024    // 16 waves: the network is a chain of LDS round trips, hidden by waves and by nothing else
#define DET_SEG 4096             // sorted positions per workgroup of the scan and metric kernels
#define DET_SEG_THREADS 256      // 16 consecutive positions per thread
#define DET_PER_THREAD (DET_SEG / DET_SEG_THREADS)
#define DET_NAN_IMAGE 0xFFFFFFFFu

typedef unsigned long long det_key;

__device__ __forceinline__ unsigned int det_image(det_key k) { return (unsigned int)(k >> 32); }

// ---- rows: one wave per row of z (B, K).  m = max z (lowest index on ties), e_k = expf(z_k - m) in fp32, S = sum e_k and
// T = sum e_k (z_k - m) in double (lane partial sums over k = l, l + 64, ... ascending, then the xor tree).  msp = 1 - 1 / S,
// entropy = log S - T / S (a term with e_k = 0 adds 0: 0 log 0 = 0; clamped at 0), energy = -(m + log S). ----
__global__ __launch_bounds__(256)
void det_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, float* __restrict__ scores, int64_t ld, int64_t n0,
                     uint8_t* __restrict__ flags, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* z = logits + (size_t)b * K;
    float best = -INFINITY;
    int bi = 0x7FFFFFFF;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        if (v > best) { best = v; bi = k; }
    }
    WAVE_ARGMAX(best, bi);
    double s = 0.0, t = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float d = z[k] - best;
        const float e = expf(d);
        s += (double)e;
        if (e != 0.f) t += (double)e * (double)d;
    }
    s = wave_sum(s);
    t = wave_sum(t);
    if (lane == 0) {
        const double ls = log(s);
        double ent = ls - t / s;
        if (ent < 0.0) ent = 0.0;
        const size_t at = (size_t)(n0 + b);
        scores[at] = (float)(1.0 - 1.0 / s);
        scores[(size_t)ld + at] = (float)ent;
        scores[2 * (size_t)ld + at] = (float)(-((double)best + ls));
        if (labels) {
            const int64_t y = labels[b];
            flags[at] = !label_ok(y, K) ? 2 : ((int64_t)bi != y ? 1 : 0);
        }
    }
}

// dst[b] = (float) src[b * stride]: a head's own column (float or double) into the store
__global__ __launch_bounds__(256)
void det_column_kernel(const void* __restrict__ src, int is_double, int64_t stride, float* __restrict__ dst, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    dst[b] = is_double ? (float)((const double*)src)[(size_t)b * stride] : ((const float*)src)[(size_t)b * stride];
}

// ---- keys ----
__device__ __forceinline__ det_key det_make_key(const float* __restrict__ col, const uint8_t* __restrict__ flags, int gi, int N) {
    if (gi >= N) return ~0ull;
    const float v = col[gi];
    const unsigned int f = flags[gi];
    const bool nan = v != v;
    const unsigned int u = nan ? DET_NAN_IMAGE : key32(fold_zero(v));                 // -0 ranks as +0
    const unsigned int low = ((unsigned int)gi << 2) | (f >= 2u ? 2u : 0u) | ((f == 1u && !nan) ? 1u : 0u);
    return ((det_key)u << 32) | (det_key)low;
}

// ---- sort, in LDS: workgroup x of column y owns the Lc = min(P, 4096) keys behind x * Lc and runs the levels k_lo .. k_hi of the
// network on them, every level from distance min(k, Lc) / 2 down to 1 (larger distances of a level were global passes).  The
// direction of a compare-exchange comes from the key's global position.  Pair q of a step touches i = q with a zero inserted at bit
// log2(j) and i | j, so a half-wave reads 32 consecutive keys on both sides at j >= 32 and runs of j keys below; the last two steps
// of a level (j = 2, 1) run in registers on four consecutive keys.  With `build` the keys are formed from the column and the flags
// instead of being read back. ----
__global__ __launch_bounds__(DET_SORT_THREADS)
void det_sort_local_kernel(const float* __restrict__ scores, int64_t ld, const uint8_t* __restrict__ flags, det_key* __restrict__ keys,
                           int N, int P, int Lc, int k_lo, int k_hi, int build) {
    __shared__ det_key sk[DET_CHUNK];
    const int tid = threadIdx.x, base = blockIdx.x * Lc;
    det_key* kcol = keys + (size_t)blockIdx.y * P;
    const float* col = scores + (size_t)blockIdx.y * (size_t)ld;
    for (int i = tid; i < Lc; i += DET_SORT_THREADS) sk[i] = build ? det_make_key(col, flags, base + i, N) : kcol[base + i];
    __syncthreads();
    for (int k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (k >> 1) < (Lc >> 1) ? (k >> 1) : (Lc >> 1); j > 0; j >>= 1) {
            if (j == 2) {
                for (int t = tid; t < (Lc >> 2); t += DET_SORT_THREADS) {
                    const bool asc = ((base + 4 * t) & k) == 0;
                    det_key x0 = sk[4 * t], x1 = sk[4 * t + 1], x2 = sk[4 * t + 2], x3 = sk[4 * t + 3];
                    cmpx(x0, x2, asc); cmpx(x1, x3, asc); cmpx(x0, x1, asc); cmpx(x2, x3, asc);
                    sk[4 * t] = x0; sk[4 * t + 1] = x1; sk[4 * t + 2] = x2; sk[4 * t + 3] = x3;
                }
                __syncthreads();
                break;
            }
            for (int q = tid; q < (Lc >> 1); q += DET_SORT_THREADS) {
                const int i = BITONIC_LO(q, j), l = i | j;
                BITONIC_CMPX_AT(sk, i, l, ((base + i) & k) == 0);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < Lc; i += DET_SORT_THREADS) kcol[base + i] = sk[i];
}

// ---- sort, one global pass: the compare-exchange of level k at distance j >= 4096, one pair per thread ----
__global__ __launch_bounds__(256)
void det_sort_global_kernel(det_key* __restrict__ keys, int P, int k, int j) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= (P >> 1)) return;
    det_key* kcol = keys + (size_t)blockIdx.y * P;
    const int i = BITONIC_LO(q, j), l = i | j;
    BITONIC_CMPX_AT(kcol, i, l, (i & k) == 0);
}

// ---- the sorted set: positions [0, n) hold the numbers ascending, [n, N) the NaN rows by index, [N, P) the padding.  A segment is
// DET_SEG consecutive positions, thread t of its workgroup owns the 16 behind t * 16. ----
// meta (int32[4] per column): n | positives among the n | bad-label flags among the N | FP of the FPR95 group
// scan 1 of 3: per segment, the number of positive keys and of bad-label keys at positions < N
__global__ __launch_bounds__(DET_SEG_THREADS)
void det_seg_sums_kernel(const det_key* __restrict__ keys, int* __restrict__ segsum, int N, int P, int nseg) {
    __shared__ int red[2][DET_SEG_THREADS / 64];
    const int tid = threadIdx.x, seg = blockIdx.x;
    const det_key* kcol = keys + (size_t)blockIdx.y * P;
    int pos = 0, bad = 0;
    for (int r = 0; r < DET_PER_THREAD; ++r) {
        const int p = seg * DET_SEG + tid * DET_PER_THREAD + r;
        if (p < N) {
            const unsigned int low = (unsigned int)kcol[p];
            pos += low & 1u;
            bad += (low >> 1) & 1u;
        }
    }
    pos = wave_sum(pos);
    bad = wave_sum(bad);
    if ((tid & 63) == 0) { red[0][tid >> 6] = pos; red[1][tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        int* o = segsum + 2 * ((size_t)blockIdx.y * nseg + seg);
        o[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        o[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// scan 2 of 3: one thread per column adds the (at most 256) segment sums in order; n is the first position whose image is the NaN
// image, found by bisection of the sorted positions [0, N)
__global__ __launch_bounds__(64)
void det_scan_sums_kernel(const det_key* __restrict__ keys, const int* __restrict__ segsum, int* __restrict__ segoff, int* __restrict__ meta,
                          int N, int P, int nseg, int S) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const det_key* kcol = keys + (size_t)s * P;
    int run = 0, bad = 0;
    for (int g = 0; g < nseg; ++g) {
        segoff[(size_t)s * nseg + g] = run;
        run += segsum[2 * ((size_t)s * nseg + g)];
        bad += segsum[2 * ((size_t)s * nseg + g) + 1];
    }
    int lo = 0, hi = N;                                      // first position in [0, N] with the NaN image
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (det_image(kcol[mid]) == DET_NAN_IMAGE) hi = mid; else lo = mid + 1;
    }
    meta[4 * s] = lo; meta[4 * s + 1] = run; meta[4 * s + 2] = bad; meta[4 * s + 3] = 0;
}

// scan 3 of 3: prefix[p] = the number of positive keys at positions <= p; the sample indices in sorted order when asked for
__global__ __launch_bounds__(DET_SEG_THREADS)
void det_scan_apply_kernel(const det_key* __restrict__ keys, const int* __restrict__ segoff, int* __restrict__ prefix, int32_t* __restrict__ order,
                           int N, int P, int nseg) {
    __shared__ int wtot[DET_SEG_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, seg = blockIdx.x, p0 = seg * DET_SEG + tid * DET_PER_THREAD;
    const det_key* kcol = keys + (size_t)blockIdx.y * P;
    unsigned int low[DET_PER_THREAD];
    int mine = 0;
#pragma unroll
    for (int r = 0; r < DET_PER_THREAD; ++r) {
        low[r] = p0 + r < P ? (unsigned int)kcol[p0 + r] : 0u;
        mine += (p0 + r < N) ? (int)(low[r] & 1u) : 0;
    }
    int incl = mine;                                         // inclusive scan over the wave's threads
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wtot[tid >> 6] = incl;
    __syncthreads();
    int run = segoff[(size_t)blockIdx.y * nseg + seg] + incl - mine;
    for (int w = 0; w < (tid >> 6); ++w) run += wtot[w];
#pragma unroll
    for (int r = 0; r < DET_PER_THREAD; ++r) {
        const int p = p0 + r;
        if (p < N) {
            run += (int)(low[r] & 1u);
            prefix[(size_t)blockIdx.y * P + p] = run;
            if (order) order[(size_t)blockIdx.y * N + p] = (int32_t)(low[r] >> 2);
        }
    }
}

// last position of the tie group that starts at a: positions are sorted, so the group is a run; gallop, then bisect
__device__ __forceinline__ int det_group_end(const det_key* __restrict__ kcol, int a, int n, unsigned int u) {
    int lo = a, step = 1;
    while (lo + step < n && det_image(kcol[lo + step]) == u) { lo += step; step <<= 1; }
    int hi = lo + step < n ? lo + step : n;                  // the image at hi differs, or hi == n
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (det_image(kcol[mid]) == u) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- metrics, per segment.  A tie group [a, b] (ascending positions) is owned by the thread that owns position a.  Seen from the
// most uncertain end, the counts at the end of the group are TP = P - prefix[a - 1], FP = (n - a) - TP, at the end of the group
// before it TP' = P - prefix[b], FP' = (n - b - 1) - TP'.  The owner adds (FP - FP')(TP + TP') to the AUROC numerator (int64),
// ((TP - TP') / P) TP / (TP + FP) to the average precision, and writes FP when TP' < ceil(0.95 P) <= TP (exactly one group).  Every
// position p < n adds prefix[p] / (p + 1) to the AURC sum.  A thread adds its 16 positions in ascending order, the workgroup's
// threads are added by the xor tree and the four waves in order: part = {int64 numerator, double AP, double AURC} per segment. ----
__global__ __launch_bounds__(DET_SEG_THREADS)
void det_metric_parts_kernel(const det_key* __restrict__ keys, const int* __restrict__ prefix, int* __restrict__ meta, double* __restrict__ part,
                             int P, int nseg) {
    __shared__ double redd[2][DET_SEG_THREADS / 64];
    __shared__ long long redl[DET_SEG_THREADS / 64];
    const int tid = threadIdx.x, seg = blockIdx.x, s = blockIdx.y, p0 = seg * DET_SEG + tid * DET_PER_THREAD;
    const det_key* kcol = keys + (size_t)s * P;
    const int* pre = prefix + (size_t)s * P;
    const int n = meta[4 * s], Ptot = meta[4 * s + 1];
    const int need = (int)((19ll * Ptot + 19ll) / 20ll);      // ceil(0.95 P) in integers
    long long num = 0;
    double ap = 0.0, rc = 0.0;
    unsigned int before = (p0 > 0 && p0 - 1 < n) ? det_image(kcol[p0 - 1]) : 0u;
    for (int r = 0; r < DET_PER_THREAD; ++r) {
        const int a = p0 + r;
        if (a >= n) break;
        const unsigned int u = det_image(kcol[a]);
        rc += (double)pre[a] / (double)(a + 1);
        if (a == 0 || u != before) {
            const int b = det_group_end(kcol, a, n, u);
            const int tp = Ptot - (a > 0 ? pre[a - 1] : 0), tpp = Ptot - pre[b];
            const int fp = (n - a) - tp, fpp = (n - b - 1) - tpp;
            num += (long long)(fp - fpp) * (long long)(tp + tpp);
            if (Ptot > 0) {
                ap += ((double)(tp - tpp) / (double)Ptot) * ((double)tp / (double)(tp + fp));
                if (tpp < need && tp >= need) meta[4 * s + 3] = fp;
            }
        }
        before = u;
    }
    num = wave_sum(num);
    ap = wave_sum(ap);
    rc = wave_sum(rc);
    if ((tid & 63) == 0) { redl[tid >> 6] = num; redd[0][tid >> 6] = ap; redd[1][tid >> 6] = rc; }
    __syncthreads();
    if (tid == 0) {
        double* o = part + 3 * ((size_t)s * nseg + seg);
        o[0] = __longlong_as_double(redl[0] + redl[1] + redl[2] + redl[3]);
        o[1] = ((redd[0][0] + redd[0][1]) + redd[0][2]) + redd[0][3];
        o[2] = ((redd[1][0] + redd[1][1]) + redd[1][2]) + redd[1][3];
    }
}

// ---- metrics, finish: one thread per column adds the segments in order.  out[s] = {AUROC, AUPR, FPR95, AURC, n, P, NaN scores, 0} ----
__global__ __launch_bounds__(64)
void det_metric_finish_kernel(const int* __restrict__ meta, const double* __restrict__ part, double* __restrict__ out, int N, int nseg, int S) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const int n = meta[4 * s], Ptot = meta[4 * s + 1], bad = meta[4 * s + 2], Nn = n - Ptot;
    long long num = 0;
    double ap = 0.0, rc = 0.0;
    for (int g = 0; g < nseg; ++g) {
        const double* p = part + 3 * ((size_t)s * nseg + g);
        num += __double_as_longlong(p[0]);
        ap += p[1];
        rc += p[2];
    }
    const bool ranked = Ptot > 0 && Nn > 0 && !bad;
    double* o = out + 8 * (size_t)s;
    o[0] = ranked ? (double)num / (2.0 * (double)Ptot * (double)Nn) : quiet_nan();
    o[1] = (Ptot > 0 && !bad) ? ap : quiet_nan();
    o[2] = ranked ? (double)meta[4 * s + 3] / (double)Nn : quiet_nan();
    o[3] = (n > 0 && !bad) ? rc / (double)n : quiet_nan();
    o[4] = (double)n; o[5] = (double)Ptot; o[6] = (double)(N - n); o[7] = 0.0;
}

// ---- launchers: arguments are validated before anything touches the device ----
struct DetLayout { int P, Lc, nseg; size_t keys, prefix, segsum, segoff, meta, part, total; };

static inline DetLayout det_layout(int N, int S) {
    DetLayout d;
    d.P = 1;
    while (d.P < N) d.P <<= 1;
    d.Lc = d.P < DET_CHUNK ? d.P : DET_CHUNK;
    d.nseg = (d.P + DET_SEG - 1) / DET_SEG;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t here = at; at += align16(bytes); return here; };
    d.keys = take((size_t)S * d.P * sizeof(det_key));
    d.prefix = take((size_t)S * d.P * sizeof(int));
    d.segsum = take((size_t)S * d.nseg * 2 * sizeof(int));
    d.segoff = take((size_t)S * d.nseg * sizeof(int));
    d.meta = take((size_t)S * 4 * sizeof(int));
    d.part = take((size_t)S * d.nseg * 3 * sizeof(double));
    d.total = at;
    return d;
}

static inline bool det_set_ok(int N, int S) { return N >= 1 && N <= DET_MAX_N && S >= 1 && S <= DET_MAX_S; }

extern "C" int uvit_op_detect_rows(const float* logits, const int64_t* labels, float* scores, int64_t ld, int64_t n0, uint8_t* flags, int B, int K,
                                   uvit_stream stream) {
    if (!logits || !scores || (labels && !flags)) return UVIT_ERR_ARG;
    if (B < 1 || K < 1 || n0 < 0 || ld < n0 + (int64_t)B) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(det_rows_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, (hipStream_t)stream, logits, labels, scores, ld, n0, flags, B, K);
    return uvit_check_launch();
}

extern "C" int uvit_op_detect_column(const void* src, int src_is_double, int64_t stride, float* dst, int B, uvit_stream stream) {
    if (!src || !dst || (src_is_double & ~1)) return UVIT_ERR_ARG;
    if (B < 1 || stride < 1) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(det_column_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, src_is_double, stride, dst, B);
    return uvit_check_launch();
}

extern "C" int64_t uvit_op_detect_ws_bytes(int N, int S) {
    if (!det_set_ok(N, S)) return UVIT_ERR_SHAPE;
    return (int64_t)det_layout(N, S).total;
}

extern "C" int uvit_op_detect_metrics(const float* scores, int64_t ld, const uint8_t* flags, int N, int S, int32_t* order, double* out, void* ws,
                                      int64_t ws_bytes, uvit_stream stream) {
    if (!scores || !flags || !out || !ws || misaligned(ws, 16)) return UVIT_ERR_ARG;
    if (!det_set_ok(N, S) || ld < (int64_t)N) return UVIT_ERR_SHAPE;
    const DetLayout d = det_layout(N, S);
    if (ws_bytes < (int64_t)d.total) return UVIT_ERR_WORKSPACE;
    char* w = (char*)ws;
    det_key* keys = (det_key*)(w + d.keys);
    int *prefix = (int*)(w + d.prefix), *segsum = (int*)(w + d.segsum), *segoff = (int*)(w + d.segoff), *meta = (int*)(w + d.meta);
    double* part = (double*)(w + d.part);
    hipStream_t st = (hipStream_t)stream;
    const dim3 chunks(d.P / d.Lc, S), segs(d.nseg, S);
    // 1 launch sorts every chunk; then per level k > chunk: log2(k / chunk) global passes and 1 launch that finishes the level in LDS
    hipLaunchKernelGGL(det_sort_local_kernel, chunks, dim3(DET_SORT_THREADS), 0, st, scores, ld, flags, keys, N, d.P, d.Lc, 2, d.Lc, 1);
    for (int k = d.Lc << 1; k <= d.P; k <<= 1) {
        for (int j = k >> 1; j >= d.Lc; j >>= 1)
            hipLaunchKernelGGL(det_sort_global_kernel, dim3((d.P / 2 + 255) / 256, S), dim3(256), 0, st, keys, d.P, k, j);
        hipLaunchKernelGGL(det_sort_local_kernel, chunks, dim3(DET_SORT_THREADS), 0, st, scores, ld, flags, keys, N, d.P, d.Lc, k, k, 0);
    }
    hipLaunchKernelGGL(det_seg_sums_kernel, segs, dim3(DET_SEG_THREADS), 0, st, (const det_key*)keys, segsum, N, d.P, d.nseg);
    hipLaunchKernelGGL(det_scan_sums_kernel, dim3((S + 63) / 64), dim3(64), 0, st, (const det_key*)keys, (const int*)segsum, segoff, meta, N, d.P, d.nseg, S);
    hipLaunchKernelGGL(det_scan_apply_kernel, segs, dim3(DET_SEG_THREADS), 0, st, (const det_key*)keys, (const int*)segoff, prefix, order, N, d.P, d.nseg);
    hipLaunchKernelGGL(det_metric_parts_kernel, segs, dim3(DET_SEG_THREADS), 0, st, (const det_key*)keys, (const int*)prefix, meta, part, d.P, d.nseg);
    hipLaunchKernelGGL(det_metric_finish_kernel, dim3((S + 63) / 64), dim3(64), 0, st, (const int*)meta, (const double*)part, out, N, d.nseg, S);
    return uvit_check_launch();
}
