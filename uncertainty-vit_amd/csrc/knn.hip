// k-nearest-neighbour search of the probe's pooled feature in a bank of training features (gfx950), DESIGN.md section 9.11.
//   rows      feat (B, C) fp32 -> unit rows in bf16 (the norm summed in double), an int32 label per row, -1 for an unusable row
//   search    sim, idx (B, k): the k bank rows with the largest dot product per query row, sorted by (similarity descending, index
//             ascending).  Q . Bank^T as v_mfma_f32_16x16x32_bf16 tiles that are never stored: every workgroup streams one contiguous
//             slab of the bank for 64 query rows and keeps a running top-k per row in LDS; a merge kernel forms the final sorted k.
//   scores    knn = 2 - 2 s_k, the weighted k-NN vote of DINO / iBOT and its arg max
// Every similarity is one accumulator chain over C in ascending 32-element MFMA steps, whichever tile, wave or slab forms it, and the
// selection compares 64-bit keys (order-preserving bits of the similarity, inverted index) that are distinct for distinct bank rows.
// The k largest keys of a set do not depend on the order in which the set is walked, so the result is a function of the inputs
// alone: the same bits for every slab count and on every run.  No atomics on floating data.
// Compiled WITHOUT -ffast-math (build.sh): rows are screened with isfinite, NaN similarities are found with s == s and -0 is folded
// into +0 by an addition that fast-math would remove.
#ifdef __FAST_MATH__
#error "knn.hip screens non-finite values and canonicalises the sign of zero: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"

#define KNN_MAX_B 65535
#define KNN_MAX_ROWS (1 << 22)
#define KNN_MAX_C 2048
#define KNN_MAX_K 256        // neighbours
#define KNN_MAX_N (1 << 22)
#define KNN_MAX_SLABS 1024
#define KNN_MAX_CLASSES 4096

#define KNN_QM 64            // query rows per workgroup: 4 waves x 16
#define KNN_BN 64            // bank rows per tile
#define KNN_BK 64            // reduction elements per LDS tile: two MFMA steps of 32
#define KNN_LD 144           // bytes per LDS tile row: 128 + 16, so the 16 rows of a fragment read fall into 16 distinct bank groups
#define KNN_TILE (KNN_QM * KNN_LD)

// ---- rows ----
// One wave per row: |f|^2 in double (lane partial sums over ascending c, the xor tree), then (float)(f_c / sqrt(|f|^2)) to bf16 RNE.
__global__ __launch_bounds__(256)
void knn_rows_kernel(const float* __restrict__ feat, const int64_t* __restrict__ labels, bf16* __restrict__ out,
                     int* __restrict__ out_labels, int B, int C, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* f = feat + (size_t)b * C;
    double s = 0.0;
    int bad = 0;
#pragma unroll 4
    for (int c = lane; c < C; c += 64) {
        const float v = f[c];
        bad |= !isfinite(v);
        s = fma((double)v, (double)v, s);
    }
    s = wave_sum(s);
    bad = __any(bad);
    int64_t y = 0;
    if (labels) {
        y = labels[b];
        bad |= label_ok(y, K) ? 0 : 1;
    }
    bad |= !(s > 0.0);
    const double inv = 1.0 / sqrt(s);
    bf16* o = out + (size_t)b * C;
    for (int c = lane; c < C; c += 64) o[c] = bad ? f2bf(0.0f) : f2bf((float)((double)f[c] * inv));
    if (lane == 0) out_labels[b] = bad ? -1 : (int)y;
}

// sums += {rows used, rows skipped}: one workgroup counts the labels just written (whole numbers below 2^53: exact, any order)
__global__ __launch_bounds__(256)
void knn_count_kernel(const int* __restrict__ out_labels, double* __restrict__ sums, int B) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int n = 0;
    for (int b = threadIdx.x; b < B; b += 256) n += out_labels[b] < 0 ? 1 : 0;
    if (n) atomicAdd(&bad, n);
    __syncthreads();
    if (threadIdx.x == 0) { sums[0] = sums[0] + (double)(B - bad); sums[1] = sums[1] + (double)bad; }
}

// ---- search ----
__device__ __forceinline__ uint64_t knn_key(float s, int idx) {
    uint32_t u = __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint32_t)(~idx);
}
__device__ __forceinline__ float knn_key_sim(uint64_t key) {
    uint32_t u = (uint32_t)(key >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ int knn_key_idx(uint64_t key) { return (int)(~(uint32_t)key); }

// The smallest of the 64 lanes' keys, wave-uniform.  All lanes active.  Four DPP steps inside each row of 16 lanes (swap within pairs,
// swap the pairs of a quad, mirror a half row, mirror the row) leave the row's minimum in all of its lanes; the four rows meet in
// scalar registers.  A tenth of the latency of six ds_bpermute rounds, which an insertion would otherwise wait for.
template <int CTRL>
__device__ __forceinline__ uint64_t knn_dpp_min(uint64_t v) {
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    const uint64_t o = ((uint64_t)ohi << 32) | olo;
    return o < v ? o : v;
}
__device__ __forceinline__ uint64_t knn_readlane(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t knn_wave_min(uint64_t v) {
    v = knn_dpp_min<0xB1>(v);                            // quad_perm [1, 0, 3, 2]
    v = knn_dpp_min<0x4E>(v);                            // quad_perm [2, 3, 0, 1]
    v = knn_dpp_min<0x141>(v);                           // row_half_mirror
    v = knn_dpp_min<0x140>(v);                           // row_mirror
    const uint64_t a = knn_readlane(v, 0), b = knn_readlane(v, 16), c = knn_readlane(v, 32), d = knn_readlane(v, 48);
    const uint64_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// A wave's running top-k of one row: `list` holds kpad = 64 E keys, the first k live (0 = empty, below every key of a bank row), the
// rest all-ones.  *thr is the smallest live key and *pos a place where it is.  A candidate above *thr replaces it; then one pass
// finds the new smallest.  Called by the whole wave with a wave-uniform candidate.
__device__ __forceinline__ void knn_insert(volatile uint64_t* list, int E, uint64_t cand, volatile uint64_t* thr, volatile int* pos,
                                           int lane) {
    if (lane == 0) list[*pos] = cand;
    uint64_t m = ~0ull;
    int at = 0;
    for (int e = 0; e < E; ++e) {
        const uint64_t v = list[lane + 64 * e];
        if (v < m) { m = v; at = lane + 64 * e; }
    }
    const uint64_t w = knn_wave_min(m);
    const int p = __builtin_amdgcn_readlane(at, __builtin_ctzll(__ballot(m == w)));
    if (lane == 0) { *thr = w; *pos = p; }
}

__device__ __forceinline__ void knn_list_init(uint64_t* list, uint64_t* thr, int* pos, int rows, int kpad, int k, int tid, int nt) {
    for (int i = tid; i < rows * kpad; i += nt) list[i] = (i % kpad) < k ? 0ull : ~0ull;
    for (int i = tid; i < rows; i += nt) { thr[i] = 0ull; pos[i] = 0; }
}

// Workgroup (qt, slab): query rows [64 qt, 64 qt + 64) against bank rows [slab * per, min(N, (slab + 1) * per)), per % 64 == 0.
// Wave w owns rows 16 w .. 16 w + 15 of the tile: 4 accumulators (16 query rows x 4 x 16 bank rows) per bank tile, lane l holding
// query row 4 (l >> 4) + reg and bank row 16 nb + (l & 15).  Rows past B, bank rows past the slab and reduction elements past C are
// staged as zeros (one code path; a zero step adds an exact zero to every chain alike) and masked out of the selection.
// Block ids are laid out so that the query tiles of one slab are 8 apart: they run on the same XCD at the same time and share its L2.
__global__ __launch_bounds__(256)
void knn_search_kernel(const bf16* __restrict__ query, const bf16* __restrict__ bank, const int* __restrict__ bank_labels,
                       uint64_t* __restrict__ ws, int B, int C, int N, int k, int kpad, int slabs, int per, int nq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;
    char* Bs = smem + KNN_TILE;
    uint64_t* lists = (uint64_t*)(smem + 2 * KNN_TILE);
    uint64_t* thr = lists + (size_t)KNN_QM * kpad;
    int* pos = (int*)(thr + KNN_QM);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = blockIdx.x / (8 * nq), rem = blockIdx.x % (8 * nq);
    const int qt = rem >> 3, slab = grp * 8 + (rem & 7);
    if (slab >= slabs) return;
    const int q0 = qt * KNN_QM;
    const int nbeg = min(N, slab * per), nend = min(N, nbeg + per);
    knn_list_init(lists, thr, pos, KNN_QM, kpad, k, tid, 256);
    __syncthreads();
    const int nkc = (C + KNN_BK - 1) / KNN_BK, ntile = (nend - nbeg + KNN_BN - 1) / KNN_BN, nstep = nkc * ntile;
    const int lr = tid >> 2, lc = tid & 3;                 // staging: tile row, 16-byte chunk (and chunk + 4)
    uint4 ra[2], rb[2];
    auto load = [&](int step) {
        const int n0 = nbeg + (step / nkc) * KNN_BN, kc = (step % nkc) * KNN_BK;
        const int q = q0 + lr, n = n0 + lr;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = kc + (lc + 4 * h) * 8;
            ra[h] = (q < B && c < C) ? *(const uint4*)(query + (size_t)q * C + c) : make_uint4(0, 0, 0, 0);
            rb[h] = (n < nend && c < C) ? *(const uint4*)(bank + (size_t)n * C + c) : make_uint4(0, 0, 0, 0);
        }
    };
    const bool active = q0 + wave * 16 < B;               // a wave whose rows are all past B only stages
    const int E = kpad >> 6;
    volatile uint64_t* wthr = thr + wave * 16;
    volatile int* wpos = pos + wave * 16;
    volatile uint64_t* wlist = lists + (size_t)wave * 16 * kpad;
    f32x4 acc[4];
    int lab[4];
    if (nstep) load(0);
    for (int step = 0; step < nstep; ++step) {
        const int kci = step % nkc, n0 = nbeg + (step / nkc) * KNN_BN;
        if (kci == 0) {
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int n = n0 + nb * 16 + (lane & 15);
                lab[nb] = n < nend ? bank_labels[n] : -1;
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *(uint4*)(As + lr * KNN_LD + (lc + 4 * h) * 16) = ra[h];
            *(uint4*)(Bs + lr * KNN_LD + (lc + 4 * h) * 16) = rb[h];
        }
        __syncthreads();
        if (step + 1 < nstep) load(step + 1);
        if (!active) continue;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int off = kk * 64 + (lane >> 4) * 16;
            const bf16x8 a = *(const bf16x8*)(As + (wave * 16 + (lane & 15)) * KNN_LD + off);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const bf16x8 b = *(const bf16x8*)(Bs + (nb * 16 + (lane & 15)) * KNN_LD + off);
                acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nb], 0, 0, 0);
            }
        }
        if (kci != nkc - 1) continue;
        // selection: the tile's 16 x 64 candidates against the rows' thresholds, 64 per comparison
        uint64_t t[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] = wthr[(lane >> 4) * 4 + r];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int n = n0 + nb * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = acc[nb][r] + 0.0f;                       // -0 -> +0: equal similarities get equal keys
                const uint64_t key = knn_key(s, n);
                uint64_t mask = __ballot(lab[nb] >= 0 && s == s && key > t[r]);
                while (mask) {
                    const int L = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const int row = (L >> 4) * 4 + r;
                    const uint64_t cand = knn_readlane(key, L);
                    if (cand > wthr[row]) knn_insert(wlist + (size_t)row * kpad, E, cand, wthr + row, wpos + row, lane);
                }
            }
        }
    }
    if (!active) return;
    for (int row = 0; row < 16; ++row) {
        const int b = q0 + wave * 16 + row;
        if (b >= B) break;
        uint64_t* dst = ws + ((size_t)b * slabs + slab) * k;
        for (int j = lane; j < k; j += 64) dst[j] = wlist[(size_t)row * kpad + j];
    }
}

// One wave per query row: the slabs' lists (slabs * k keys) through the same running top-k, then each live key's rank by counting
// (keys of bank rows are distinct; empties rank by position behind them) and sim, idx written at the rank.
__global__ __launch_bounds__(64)
void knn_merge_kernel(const uint64_t* __restrict__ ws, const int* __restrict__ query_valid, float* __restrict__ sim,
                      int* __restrict__ idx, int64_t ld, int k, int kpad, int slabs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* list = (uint64_t*)smem;
    uint64_t* thr = list + kpad;
    int* pos = (int*)(thr + 1);
    const int lane = threadIdx.x, b = blockIdx.x;
    float* so = sim + (size_t)b * ld;
    int* io = idx + (size_t)b * ld;
    if (query_valid[b] < 0) {
        for (int j = lane; j < k; j += 64) { so[j] = NAN; io[j] = -1; }
        return;
    }
    knn_list_init(list, thr, pos, 1, kpad, k, lane, 64);
    __syncthreads();
    volatile uint64_t* vlist = list;
    volatile uint64_t* vthr = thr;
    volatile int* vpos = pos;
    const int E = kpad >> 6;
    const size_t total = (size_t)slabs * k;
    const uint64_t* src = ws + (size_t)b * total;
    for (size_t i0 = 0; i0 < total; i0 += 64) {
        const uint64_t key = i0 + lane < total ? src[i0 + lane] : 0ull;
        uint64_t mask = __ballot(key > *vthr);
        while (mask) {
            const int L = __builtin_ctzll(mask);
            mask &= mask - 1;
            const uint64_t cand = knn_readlane(key, L);
            if (cand > *vthr) knn_insert(vlist, E, cand, vthr, vpos, lane);
        }
    }
    __syncthreads();
    for (int p = lane; p < k; p += 64) {
        const uint64_t v = list[p];
        int rank = 0;
        for (int q = 0; q < k; ++q) {
            const uint64_t o = list[q];
            rank += (o > v || (o == v && q < p)) ? 1 : 0;
        }
        so[rank] = v ? knn_key_sim(v) : -INFINITY;
        io[rank] = v ? knn_key_idx(v) : -1;
    }
}

// ---- scores: one wave per row ----
// w_j = exp((s_j - s_1) / T) in double; the vote of neighbour j's class is the sum of w_i over the neighbours i of that class in
// ascending i, formed by every lane that holds a neighbour of the class (the same chain, the same bits); the arg max takes the
// largest vote and the lowest class among equals.  A neighbour whose bank label is outside [0, K) does not vote.
__global__ __launch_bounds__(64)
void knn_scores_kernel(const float* __restrict__ sim, const int* __restrict__ idx, int64_t ld, const int* __restrict__ bank_labels, int N,
                       float* __restrict__ knn, int* __restrict__ pred, double* __restrict__ votes, int64_t ldv,
                       const int64_t* __restrict__ labels, int* __restrict__ correct, int k, int K, double T) {
    __shared__ double w[KNN_MAX_K];
    __shared__ int cls[KNN_MAX_K];
    const int lane = threadIdx.x, b = blockIdx.x;
    const float* s = sim + (size_t)b * ld;
    const int* ix = idx + (size_t)b * ld;
    const float sk = s[k - 1], s1 = s[0];
    const int ik = ix[k - 1];
    double* vr = votes ? votes + (size_t)b * ldv : nullptr;
    if (!(sk == sk) || sk == -INFINITY || ik < 0 || ik >= N) {
        if (vr)
            for (int c = lane; c < K; c += 64) vr[c] = NAN;
        if (lane == 0) { knn[b] = NAN; pred[b] = -1; }
        return;
    }
    for (int j = lane; j < k; j += 64) {
        const int i = ix[j];
        const int c = (i >= 0 && i < N) ? bank_labels[i] : -1;
        cls[j] = (c >= 0 && c < K) ? c : -1;
        w[j] = exp(((double)s[j] - (double)s1) / T);
    }
    if (vr)
        for (int c = lane; c < K; c += 64) vr[c] = 0.0;
    __syncthreads();
    double best = -1.0;
    int at = K;                                           // K: no vote seen
    for (int j = lane; j < k; j += 64) {
        const int c = cls[j];
        if (c < 0) continue;
        double v = 0.0;
        for (int i = 0; i < k; ++i)
            if (cls[i] == c) v += w[i];
        if (vr) vr[c] = v;
        if (v > best || (v == best && c < at)) { best = v; at = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (lane == 0) {
        knn[b] = fmaf(-2.0f, sk, 2.0f);
        pred[b] = at < K ? at : -1;
        if (labels && correct && at < K && labels[b] == (int64_t)at) atomicAdd(correct, 1);
    }
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool knn_bad_c(int C) { return C < 32 || (C % 32) || C > KNN_MAX_C; }
static inline bool knn_bad_search(int B, int C, int N, int k, int slabs) {
    return B < 1 || B > KNN_MAX_B || knn_bad_c(C) || N < 1 || N > KNN_MAX_N || k < 1 || k > KNN_MAX_K || slabs < 0 || slabs > KNN_MAX_SLABS;
}

static int knn_num_cu() {
    static int ncu = 0;
    if (!ncu) {
        int dev = 0;
        hipDeviceProp_t prop;
        ncu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                  ? prop.multiProcessorCount : 256;
    }
    return ncu;
}

// slabs = 0: three workgroups per CU over the query tiles (what the LDS holds at k <= 64; the loop hides its load latency by
// occupancy), at least 1024 bank rows per slab
static int knn_slabs(int B, int N, int slabs) {
    if (slabs > 0) return slabs;
    const int nq = (B + KNN_QM - 1) / KNN_QM;
    int s = (3 * knn_num_cu() + nq - 1) / nq;
    const int lim = (N + 1023) / 1024;
    s = s < lim ? s : lim;
    return s < 1 ? 1 : (s > KNN_MAX_SLABS ? KNN_MAX_SLABS : s);
}

extern "C" int uvit_op_knn_rows(const float* feat, const int64_t* labels, void* out, int32_t* out_labels, double* sums, int B, int C,
                                int K, uvit_stream stream) {
    if (!feat || !out || !out_labels) return UVIT_ERR_ARG;
    if (misaligned(feat, 4) || misaligned(labels, 8) || misaligned(out, 16) || misaligned(out_labels, 4) || misaligned(sums, 8)) return UVIT_ERR_ARG;
    if (B < 1 || B > KNN_MAX_ROWS || knn_bad_c(C) || (labels && (K < 2 || K > KNN_MAX_CLASSES))) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(knn_rows_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, feat, labels, (bf16*)out, out_labels, B, C, K);
    if (sums) hipLaunchKernelGGL(knn_count_kernel, dim3(1), dim3(256), 0, s, (const int*)out_labels, sums, B);
    return uvit_check_launch();
}

// workspace of uvit_op_knn_search: the slabs' unsorted lists, (B, slabs, k) 64-bit keys
extern "C" int64_t uvit_op_knn_search_ws_bytes(int B, int C, int N, int k, int slabs) {
    if (knn_bad_search(B, C, N, k, slabs)) return UVIT_ERR_SHAPE;
    return align16((int64_t)B * knn_slabs(B, N, slabs) * k * 8);
}

extern "C" int uvit_op_knn_search(const void* query, const int32_t* query_valid, const void* bank, const int32_t* bank_labels, float* sim,
                                  int32_t* idx, int64_t ld, void* ws, int64_t ws_bytes, int B, int C, int N, int k, int slabs,
                                  uvit_stream stream) {
    if (!query || !query_valid || !bank || !bank_labels || !sim || !idx || !ws) return UVIT_ERR_ARG;
    if (misaligned(query, 16) || misaligned(query_valid, 4) || misaligned(bank, 16) || misaligned(bank_labels, 4) || misaligned(sim, 4) ||
        misaligned(idx, 4) || misaligned(ws, 16))
        return UVIT_ERR_ARG;
    if (knn_bad_search(B, C, N, k, slabs) || ld < k) return UVIT_ERR_SHAPE;
    if (ws_bytes < uvit_op_knn_search_ws_bytes(B, C, N, k, slabs)) return UVIT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int ns = knn_slabs(B, N, slabs), nq = (B + KNN_QM - 1) / KNN_QM, kpad = (k + 63) & ~63;
    const int per = (((N + ns - 1) / ns) + KNN_BN - 1) / KNN_BN * KNN_BN;
    const size_t lds = 2 * KNN_TILE + (size_t)KNN_QM * kpad * 8 + KNN_QM * 12;                     // <= 146 KiB at k = 256
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)knn_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return UVIT_ERR_LAUNCH;
    hipLaunchKernelGGL(knn_search_kernel, dim3(((ns + 7) / 8) * 8 * nq), dim3(256), lds, s, (const bf16*)query, (const bf16*)bank,
                       (const int*)bank_labels, (uint64_t*)ws, B, C, N, k, kpad, ns, per, nq);
    hipLaunchKernelGGL(knn_merge_kernel, dim3(B), dim3(64), (size_t)kpad * 8 + 16, s, (const uint64_t*)ws, (const int*)query_valid, sim, idx,
                       ld, k, kpad, ns);
    return uvit_check_launch();
}

extern "C" int uvit_op_knn_scores(const float* sim, const int32_t* idx, int64_t ld, const int32_t* bank_labels, int N, float* knn,
                                  int32_t* pred, double* votes, int64_t ldv, const int64_t* labels, int32_t* correct, int B, int k,
                                  int K, double temperature, uvit_stream stream) {
    if (!sim || !idx || !bank_labels || !knn || !pred) return UVIT_ERR_ARG;
    if (misaligned(sim, 4) || misaligned(idx, 4) || misaligned(bank_labels, 4) || misaligned(knn, 4) || misaligned(pred, 4) || misaligned(votes, 8) ||
        misaligned(labels, 8) || misaligned(correct, 4))
        return UVIT_ERR_ARG;
    if (!(temperature > 0.0) || !(temperature < INFINITY)) return UVIT_ERR_ARG;
    if (B < 1 || B > KNN_MAX_B || N < 1 || N > KNN_MAX_N || k < 1 || k > KNN_MAX_K || ld < k || K < 2 || K > KNN_MAX_CLASSES ||
        (votes && ldv < K))
        return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(knn_scores_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, sim, idx, ld, (const int*)bank_labels, N, knn, pred,
                       votes, ldv, labels, correct, k, K, temperature);
    return uvit_check_launch();
}
