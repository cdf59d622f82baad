// Stability of a classifier under perturbation sequences on the device (gfx950): what the reference's p_evaluate() reports
//   ranks            uncertainty_evaluations.py:641      np.uint16(rankdata(-frame, method='ordinal')) per frame
//   flip probability uncertainty_evaluations.py:766-782  flip_prob: [pred_ref != pred_t] over the F - 1 pairs of a sequence
//   top-5 / Zipf     uncertainty_evaluations.py:743-763,829-837   ranking_dist / dist(perm2[argsort(perm1)], mode)
// Ordinal rank of class k in a logit row z: r[k] = 1 + #{j : z_j > z_k} + #{j < k : z_j == z_k}; rank 1 is the largest logit, ties
// go to the lower index, +0 and -0 are equal, +-inf order like any other value.  A row with a NaN has no ranks: they are all 0, and a
// sequence that holds such a row has no values (NaN); nothing is ever indexed by a rank.
// The distances are taken per class instead of per rank position (a = ranks of the reference frame, b = ranks of frame t):
//   flip   = #{c : a[c] == 1 and b[c] != 1}                     (0 or 1 on permutations: the class ranked first lost its place)
//   top-5  = sum over c with a[c] <= 5 of |(a[c] - 1) - min(b[c] - 1, 5)|
//   Zipf   = sum over c of |1 / a[c] - 1 / b[c]| / a[c]
// which is dist(sigma) with sigma[a[c] - 1] = b[c], so no inverse permutation is formed.
// No atomics: every sum has one owner and a fixed order (stated at the kernel), so the same input gives the same bits on every run.
// Compiled WITHOUT -ffast-math (build.sh): z != z finds the NaN rows, the comparisons are IEEE and the order of the sums is part of
// the contract.
#ifdef __FAST_MATH__
#error "stability.hip tests for NaN, compares in IEEE and fixes the order of its sums: build it without -ffast-math"
#endif
#include <math.h>
#include <stdint.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define STAB_MAX_K 4096
#define STAB_MAX_F 256
#define STAB_MAX_V 65535
#define STAB_MAX_R (65535 * 256)
#define STAB_MAX_GRID 4096

// 64-bit sort key of class k with logit z: high word = an unsigned image of -z whose order is the numeric order of -z (the two zeros
// folded into one), low word = k.  Ascending keys = descending logits, lower index first among equals.  The largest high word of a
// number is that of -z = +inf, 0xFF800000, so the padding key (all ones) sorts strictly behind every real key, a logit of -inf
// included; in a row with a NaN (whose ranks are not used) the low word, k < 4096, still keeps every real key in front of the padding.
__device__ __forceinline__ unsigned long long stab_key(float z, int k) {
    return ((unsigned long long)key32(fold_zero(-z)) << 32) | (unsigned long long)(unsigned int)k;
}

// ---- ranks: each row is sorted in LDS by a bitonic network over P = K rounded up to a power of two.  A row belongs to TPR =
// 2^tpr_shift threads, TPR = clamp(P / 2, 64, 1024), and a workgroup has at least 256 threads: four rows per workgroup up to
// K = 128 (one wave each), two up to K = 256, one workgroup of 256 .. 1024 threads per row above.  Every row of the launch runs the
// same number of steps, so the barriers are uniform; a workgroup's rows past R sort padding and write nothing.  A launch has at most
// STAB_MAX_GRID workgroups (several per CU at any shape), each walking the row groups blockIdx.x, blockIdx.x + gridDim.x, ...: the
// grid stays launchable up to the largest R.  vec: K % 4 == 0 and a 16-byte aligned base, the row is read as float4. ----
__global__ __launch_bounds__(1024)
void stability_ranks_kernel(const float* __restrict__ logits, int* __restrict__ ranks, int R, int K, int P, int tpr_shift, int rpb, int vec) {
    extern __shared__ unsigned long long stab_lds[];      // rpb * P keys, then rpb NaN flags
    int* nan_flag = (int*)(stab_lds + (size_t)rpb * P);
    const int TPR = 1 << tpr_shift, tid = threadIdx.x, lr = tid >> tpr_shift, t = tid & (TPR - 1);
    unsigned long long* kr = stab_lds + (size_t)lr * P;
    const long long groups = ((long long)R + rpb - 1) / rpb;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {          // g is the same in the whole workgroup: uniform barriers
        const long long row = g * rpb + lr;
        const bool live = row < (long long)R;
        if (t == 0) nan_flag[lr] = 0;
        __syncthreads();
        if (live) {
            const float* z = logits + (size_t)row * K;
            bool bad = false;
            if (vec) {
                const float4* z4 = (const float4*)z;
                for (int i = t; i < (K >> 2); i += TPR) {
                    const float4 v = z4[i];
                    bad |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
                    kr[4 * i] = stab_key(v.x, 4 * i);
                    kr[4 * i + 1] = stab_key(v.y, 4 * i + 1);
                    kr[4 * i + 2] = stab_key(v.z, 4 * i + 2);
                    kr[4 * i + 3] = stab_key(v.w, 4 * i + 3);
                }
            } else {
                for (int k = t; k < K; k += TPR) {
                    const float v = z[k];
                    bad |= v != v;
                    kr[k] = stab_key(v, k);
                }
            }
            for (int k = K + t; k < P; k += TPR) kr[k] = ~0ull;
            if (bad) nan_flag[lr] = 1;                    // every writer stores the same value
        } else {
            for (int k = t; k < P; k += TPR) kr[k] = ~0ull;
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int q = t; q < (P >> 1); q += TPR) {
                    const int i = BITONIC_LO(q, j), l = i | j;
                    BITONIC_CMPX_AT(kr, i, l, (i & k) == 0);
                }
                __syncthreads();
            }
        }
        if (live) {
            int* out = ranks + (size_t)row * K;
            if (nan_flag[lr]) {
                for (int p = t; p < K; p += TPR) out[p] = 0;
            } else {
                for (int p = t; p < K; p += TPR) {                                  // positions 0 .. K - 1 hold the K real keys
                    const unsigned int c = (unsigned int)kr[p];
                    if (c < (unsigned int)K) out[c] = p + 1;
                }
            }
        }
        __syncthreads();                                  // the keys and the flag are read out before the next group overwrites them
    }
}

// the double that lane i (uniform) holds as the words (lo, hi), in every lane
__device__ __forceinline__ double stab_lane_double(int lo, int hi, int i) {
    const unsigned long long l = (unsigned int)__builtin_amdgcn_readlane(lo, i), h = (unsigned int)__builtin_amdgcn_readlane(hi, i);
    return __longlong_as_double((long long)((h << 32) | l));
}

// ---- sequences: one workgroup per sequence, one wave per pair (wave w takes pairs w, w + n_waves, ...).  Within a pair the 64 lanes
// form the terms of 64 adjacent classes at a time and the Zipf terms are then added one by one in class order (every lane keeps the
// same running sum); the pair's three values land in LDS at the pair's index, and thread 0 adds them in frame order.  Neither order
// depends on the number of waves.  The integers are summed as integers (top-5 of a pair <= 5 * 5, of a sequence <= 255 * 25).  A rank
// below 1 (a NaN row's 0) makes all three values NaN. ----
__global__ __launch_bounds__(1024)
void stability_sequences_kernel(const int* __restrict__ ranks, double* __restrict__ seq, int F, int K, int noise) {
    __shared__ double pair_zipf[STAB_MAX_F];
    __shared__ int pair_flip[STAB_MAX_F], pair_top5[STAB_MAX_F], pair_bad[STAB_MAX_F];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int* base = ranks + (size_t)blockIdx.x * F * K;
    for (int t = 1 + wave; t < F; t += n_waves) {
        const int* a = base + (size_t)(noise ? 0 : t - 1) * K;
        const int* b = base + (size_t)t * K;
        int flip = 0, top5 = 0, bad = 0;
        double zipf = 0.0;
        for (int c0 = 0; c0 < K; c0 += 64) {
            const int c = c0 + lane;
            double term = 0.0;
            if (c < K) {
                const int ai = a[c], bi = b[c];
                if (ai < 1 || bi < 1) {
                    bad = 1;
                } else {
                    flip += (ai == 1 && bi != 1);
                    if (ai <= 5) {
                        const int d = (ai - 1) - (bi - 1 < 5 ? bi - 1 : 5);
                        top5 += d < 0 ? -d : d;
                    }
                    const double da = (double)ai;
                    term = fabs(1.0 / da - 1.0 / (double)bi) / da;
                }
            }
            const int n = K - c0 < 64 ? K - c0 : 64;
            const long long tb = __double_as_longlong(term);
            const int lo = (int)tb, hi = (int)(tb >> 32);
            if (n == 64) {                                                    // class c0 + i, ascending, by v_readlane: no LDS round trip
#pragma unroll
                for (int i = 0; i < 64; ++i) zipf += stab_lane_double(lo, hi, i);
            } else {
                for (int i = 0; i < n; ++i) zipf += stab_lane_double(lo, hi, i);
            }
        }
        flip = wave_sum(flip); top5 = wave_sum(top5); bad = wave_sum(bad);
        if (lane == 0) { pair_flip[t - 1] = flip; pair_top5[t - 1] = top5; pair_bad[t - 1] = bad; pair_zipf[t - 1] = zipf; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int flip = 0, top5 = 0, bad = 0;
        double zipf = 0.0;
        for (int p = 0; p < F - 1; ++p) { flip += pair_flip[p]; top5 += pair_top5[p]; bad |= pair_bad[p]; zipf += pair_zipf[p]; }
        const double nan = quiet_nan();
        double* o = seq + (size_t)blockIdx.x * 3;
        o[0] = bad ? nan : (double)flip;
        o[1] = bad ? nan : (double)top5;
        o[2] = bad ? nan : zipf;
    }
}

// ---- launchers: arguments are validated before anything touches the device ----
extern "C" int uvit_op_stability_ranks(const float* logits, int32_t* ranks, int R, int K, uvit_stream stream) {
    if (!logits || !ranks) return UVIT_ERR_ARG;
    if (K < 1 || K > STAB_MAX_K || R < 1 || R > STAB_MAX_R) return UVIT_ERR_SHAPE;
    int P = 1;
    while (P < K) P <<= 1;
    int tpr_shift = 6;                                                                  // clamp(P / 2, 64, 1024) threads per row
    while ((1 << tpr_shift) < (P >> 1) && tpr_shift < 10) ++tpr_shift;
    const int TPR = 1 << tpr_shift, threads = TPR > 256 ? TPR : 256, rpb = threads / TPR;
    const size_t lds = (size_t)rpb * P * sizeof(unsigned long long) + (size_t)rpb * sizeof(int);   // at most 32 KB + 4
    const int vec = (K % 4 == 0) && !misaligned(logits, 16);
    const int groups = (R + rpb - 1) / rpb;
    hipLaunchKernelGGL(stability_ranks_kernel, dim3(groups < STAB_MAX_GRID ? groups : STAB_MAX_GRID), dim3(threads), lds, (hipStream_t)stream, logits, (int*)ranks, R, K, P,
                       tpr_shift, rpb, vec);
    return uvit_check_launch();
}

extern "C" int uvit_op_stability_sequences(const int32_t* ranks, double* seq, int V, int F, int K, int noise, uvit_stream stream) {
    if (!ranks || !seq || (noise & ~1)) return UVIT_ERR_ARG;
    if (K < 1 || K > STAB_MAX_K || F < 2 || F > STAB_MAX_F || V < 1 || V > STAB_MAX_V) return UVIT_ERR_SHAPE;
    const int waves = F - 1 < 16 ? F - 1 : 16;
    hipLaunchKernelGGL(stability_sequences_kernel, dim3(V), dim3(64 * waves), 0, (hipStream_t)stream, (const int*)ranks, seq, F, K, noise);
    return uvit_check_launch();
}
