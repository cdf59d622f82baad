// MC-dropout on the frozen encoder (gfx950): the streaming combination of T stochastic passes, the method the reference evaluates
// with `--mc_dropout_forwards` (uncertainty_evaluations.evaluate_MC_dropout, :42-89: T passes over the whole loader, every pass's
// logits kept, torch.mean(outputs, 0)); DESIGN.md section 9.14.  Here each pass's logits (B, K) are added to a caller-owned per-row state and one
// call behind the last pass forms the combined logits and the five uncertainty columns: nothing of size (T, B, K) is stored.
//   accumulate   p = softmax(z) in fp32 (ens.hip's formula), widened; sum_z += z, sum_p += p, sum_p2 += p p, sum_h += H(p),
//                votes[argmax z] += 1, all per row
//   finalize     mode 0: z = sum_z / T; mode 1: z = log(sum_p / T); pbar = sum_p / T, k* = argmax z:
//                total = H(pbar), aleatoric = sum_h / T, mi = max(total - aleatoric, 0),
//                var_pred = max(sum_p2[k*] / T - pbar[k*]^2, 0), disagreement = 1 - votes[k*] / T
// One wave per row; lane i owns the classes i, i + 64, ... of its row's state, lane 0 the row's sum_h and flag.  No float atomics:
// every sum has one owner and a fixed order (per-lane partial sums over ascending k, then the xor tree), so the bits do not depend on
// the launch shape -- a batch split into two calls gives the bits of one call -- and are the same on every run.  The ops are
// launch-bound (the state is 3.6 MB at B = 128, K = 1000): coalesced lane-strided accesses, nothing else is tuned.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums is part of the contract, NaN rows are found with v != v and expf /
// logf / log are the accurate ones.
#ifdef __FAST_MATH__
#error "mcd.hip fixes the order of its sums and tests for NaN: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

// ---- the state of one row: [sum_z K | sum_p K | sum_p2 K | sum_h] double, [votes K | flag] int32, padded to 16 bytes ----
static inline __host__ __device__ size_t mcd_row_bytes(int K) {
    return ((size_t)(3 * (size_t)K + 1) * 8 + ((size_t)K + 1) * 4 + 15) & ~(size_t)15;
}
struct McdRow {
    double *sum_z, *sum_p, *sum_p2, *sum_h;
    int *votes, *flag;
    __device__ __forceinline__ McdRow(void* state, int b, int K) {
        char* base = (char*)state + (size_t)b * mcd_row_bytes(K);
        sum_z = (double*)base; sum_p = sum_z + K; sum_p2 = sum_p + K; sum_h = sum_p2 + K;
        votes = (int*)(sum_h + 1); flag = votes + K;
    }
};

__global__ __launch_bounds__(256)
void mcd_accumulate_kernel(const float* __restrict__ logits, void* __restrict__ state, int first, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* z = logits + (size_t)b * K;
    const McdRow st(state, b, K);
    // the row's maximum and its first position; a NaN never wins (v > best is false)
    float best = -INFINITY;
    int besti = 0x7FFFFFFF;
    bool has_nan = false;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        has_nan |= v != v;
        if (v > best) { best = v; besti = k; }
    }
    WAVE_ARGMAX(best, besti);
    has_nan = __any(has_nan);
    const float mx = best;
    float se = 0.f;
    for (int k = lane; k < K; k += 64) se += expf(z[k] - mx);
    const float lg = logf(wave_sum(se));          // common.h's wave_sum(float): the fp32 xor tree, as in ens.hip (se is a float: no widening)
    double h = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        const double p = (double)expf((v - mx) - lg);
        if (p > 0.0) h += p * log(p);
        const int vote = k == besti ? 1 : 0;
        if (first) {
            st.sum_z[k] = (double)v; st.sum_p[k] = p; st.sum_p2[k] = p * p; st.votes[k] = vote;
        } else {
            st.sum_z[k] += (double)v; st.sum_p[k] += p; st.sum_p2[k] += p * p; st.votes[k] += vote;
        }
    }
    h = -wave_sum(h);
    if (lane != 0) return;
    const int bad = (has_nan || !finite32(mx)) ? 1 : 0;      // a NaN, a +inf (inf - inf), or nothing above -inf: no softmax
    if (first) { *st.sum_h = h; *st.flag = bad; }
    else { *st.sum_h += h; *st.flag |= bad; }
}

__global__ __launch_bounds__(256)
void mcd_finalize_kernel(const void* __restrict__ state, int T, int mode, float* __restrict__ z, double* __restrict__ unc, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const McdRow st((void*)state, b, K);
    const double dT = (double)T;
    float best = -INFINITY;
    int besti = 0x7FFFFFFF;
    double h_total = 0.0;
    for (int k = lane; k < K; k += 64) {
        const double pbar = st.sum_p[k] / dT;
        const float zk = mode == 0 ? (float)(st.sum_z[k] / dT) : (float)log(pbar);
        z[(size_t)b * K + k] = zk;
        if (zk > best) { best = zk; besti = k; }
        if (unc && pbar > 0.0) h_total += pbar * log(pbar);
    }
    if (!unc) return;
    WAVE_ARGMAX(best, besti);
    h_total = wave_sum(h_total);
    if (lane != 0) return;
    double* out = unc + (size_t)b * 5;
    if (*st.flag || besti >= K) {
        for (int i = 0; i < 5; ++i) out[i] = quiet_nan();
        return;
    }
    const double total = -h_total, aleatoric = *st.sum_h / dT, pk = st.sum_p[besti] / dT;
    out[0] = total;
    out[1] = aleatoric;
    out[2] = fmax(total - aleatoric, 0.0);
    out[3] = fmax(st.sum_p2[besti] / dT - pk * pk, 0.0);
    out[4] = 1.0 - (double)st.votes[besti] / dT;
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool mcd_bad_shape(int B, int K) { return B < 1 || K < 1; }

extern "C" int64_t uvit_op_mcd_state_bytes(int B, int K) {
    if (mcd_bad_shape(B, K)) return UVIT_ERR_SHAPE;
    return (int64_t)((size_t)B * mcd_row_bytes(K));
}

extern "C" int uvit_op_mcd_accumulate(const float* logits, void* state, int first, int B, int K, uvit_stream stream) {
    if (!logits || !state || (first != 0 && first != 1) || misaligned(state, 16)) return UVIT_ERR_ARG;
    if (mcd_bad_shape(B, K)) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(mcd_accumulate_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, (hipStream_t)stream, logits, state, first, B, K);
    return uvit_check_launch();
}

extern "C" int uvit_op_mcd_finalize(const void* state, int T, int mode, float* z, double* unc, int B, int K, uvit_stream stream) {
    if (!state || !z || (mode != 0 && mode != 1) || misaligned(state, 16)) return UVIT_ERR_ARG;
    if (mcd_bad_shape(B, K) || T < 1) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(mcd_finalize_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, (hipStream_t)stream, state, T, mode, z, unc, B, K);
    return uvit_check_launch();
}
