// Linear probe on the frozen encoder (gfx950): everything behind the last block of `run_class_finetuning.py --linear_classifier`
//   pool + norm      modeling_finetune.py:410-412,512-515   t = x[:, 1:].mean(1); fc_norm(t) with elementwise_affine = False
//   head             modeling_finetune.py:421,522            logits = feat . W^T + bias
//   criterion        run_class_finetuning.py:617-623         timm LabelSmoothingCrossEntropy / nn.CrossEntropyLoss, + its gradient
//   head gradient    autograd of the nn.Linear               dW = dlogits^T . feat, dbias = column sums of dlogits
// All fp32.  No float atomics: every sum has one owner and a fixed order, so the same input gives the same bits on every run.  The head
// is 0.2 GFLOP at B = 128, K = 1000, C = 768 beside an encoder forward of several milliseconds, so the two contractions are LDS-tiled
// FMA kernels and not MFMA ones.  None of the entry points needs the engine.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums below is part of the contract.
#ifdef __FAST_MATH__
#error "probe.hip fixes the order of its fp32 sums: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"
#include "probe_pool.h"      // pool + norm: the kernels and their launch, shared with dprobe.hip
#include "rowwise.h"

// ---- the two contractions: 64 x 64 output tile, 256 threads with a 4 x 4 micro-tile each, 16 reduction steps per LDS tile ----
#define PT 64
#define PK 16

// logits[B, K] = feat[B, C] . W[K, C]^T + bias: both operands are read along C (float4) and stored transposed, [c][row]
__global__ __launch_bounds__(256)
void probe_logits_kernel(const float* __restrict__ feat, const float* __restrict__ W, const float* __restrict__ bias,
                         float* __restrict__ logits, int B, int K, int C) {
    __shared__ __attribute__((aligned(16))) float As[PK][PT + 4], Ws[PK][PT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int k0 = blockIdx.x * PT, b0 = blockIdx.y * PT;
    const int lr = tid >> 2, lc = (tid & 3) * 4;          // staging: tile row, first of four reduction columns
    float acc[4][4] = {};
    for (int c0 = 0; c0 < C; c0 += PK) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), w = a;
        if (c0 + lc < C) {                                // C % 4 == 0: a float4 is inside the row or outside it
            if (b0 + lr < B) a = *(const float4*)(feat + (size_t)(b0 + lr) * C + c0 + lc);
            if (k0 + lr < K) w = *(const float4*)(W + (size_t)(k0 + lr) * C + c0 + lc);
        }
        __syncthreads();
        As[lc][lr] = a.x; As[lc + 1][lr] = a.y; As[lc + 2][lr] = a.z; As[lc + 3][lr] = a.w;
        Ws[lc][lr] = w.x; Ws[lc + 1][lr] = w.y; Ws[lc + 2][lr] = w.z; Ws[lc + 3][lr] = w.w;
        __syncthreads();
        // the 16 products of a tile are summed on their own and then added to the running sum: C / 16 additions at full magnitude
        // instead of C (a single C-term chain was seen to exceed the 4 x margin over a blocked CPU sgemm's round-off that
        // tests/test_gpu_probe.py allows at C = 768; an observation during development, no recorded profile)
        float t[4][4] = {};
#pragma unroll
        for (int c = 0; c < PK; ++c) {
            const float4 av = *(const float4*)&As[c][ty * 4], wv = *(const float4*)&Ws[c][tx * 4];
            const float ar[4] = {av.x, av.y, av.z, av.w}, wr[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) t[i][j] = fmaf(ar[i], wr[j], t[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += t[i][j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + ty * 4 + i;
        if (b >= B) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + tx * 4 + j;
            if (k < K) logits[(size_t)b * K + k] = acc[i][j] + bias[k];
        }
    }
}

// dW[K, C] = dlogits[B, K]^T . feat[B, C], dbias[K] = column sums of dlogits: the reduction runs over b in ascending order and every
// output element has one owner (dbias: the first 64 threads of the workgroups of the first column tile).  Outputs are overwritten.
__global__ __launch_bounds__(256)
void probe_head_grad_kernel(const float* __restrict__ dlogits, const float* __restrict__ feat, float* __restrict__ dW,
                            float* __restrict__ dbias, int B, int K, int C) {
    __shared__ __attribute__((aligned(16))) float Ds[PK][PT + 4], Fs[PK][PT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int c0 = blockIdx.x * PT, k0 = blockIdx.y * PT;
    const int fr = tid >> 4, fc = (tid & 15) * 4;         // feat staging: batch row, first of four columns
    const int dr = tid >> 6, dc = tid & 63;               // dlogits staging: batch rows dr, dr + 4, ..., one class column (K need not be a multiple of 4)
    float acc[4][4] = {};
    float bsum = 0.f;
    for (int b0 = 0; b0 < B; b0 += PK) {
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b0 + fr < B && c0 + fc < C) f = *(const float4*)(feat + (size_t)(b0 + fr) * C + c0 + fc);
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + dr + 4 * i;
            d[i] = (b < B && k0 + dc < K) ? dlogits[(size_t)b * K + k0 + dc] : 0.f;
        }
        __syncthreads();
        *(float4*)&Fs[fr][fc] = f;
#pragma unroll
        for (int i = 0; i < 4; ++i) Ds[dr + 4 * i][dc] = d[i];
        __syncthreads();
#pragma unroll
        for (int b = 0; b < PK; ++b) {
            const float4 dv = *(const float4*)&Ds[b][ty * 4], fv = *(const float4*)&Fs[b][tx * 4];
            const float dd[4] = {dv.x, dv.y, dv.z, dv.w}, ff[4] = {fv.x, fv.y, fv.z, fv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(dd[i], ff[j], acc[i][j]);
        }
        if (blockIdx.x == 0 && tid < PT) {
#pragma unroll
            for (int b = 0; b < PK; ++b) bsum += Ds[b][tid];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + ty * 4 + i, c = c0 + tx * 4;
        if (k < K && c < C) *(float4*)(dW + (size_t)k * C + c) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
    }
    if (blockIdx.x == 0 && tid < PT && k0 + tid < K) dbias[k0 + tid] = bsum;
}

// ---- criterion: one wave per row ----
// loss_b = (1 - s) (lse - z_y) + s (lse - mean_k z_k);  dlogits = (softmax - (1 - s) onehot - s / K) / B.
// counters[0] += z_y is the strict row maximum, counters[1] += fewer than five logits are greater than z_y.
// A label outside [0, K): the row's loss and gradient are NaN, nothing is read at the label, no counter moves.
__global__ __launch_bounds__(256)
void probe_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, float smoothing, float* __restrict__ dlogits,
                     float* __restrict__ row_loss, int* __restrict__ counters, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const float* z = logits + (size_t)b * K;
    const int64_t y = labels[b];
    const bool valid = y >= 0 && y < (int64_t)K;     // spelled out: through label_ok() the compiler orders two operands differently
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, z[k]);
    m = wave_max(m);
    const float zy = valid ? z[y] : 0.f;
    float se = 0.f, sz = 0.f;
    int gt = 0, ge = 0;
    for (int k = lane; k < K; k += 64) {
        const float v = z[k];
        se += expf(v - m);
        sz += v;
        gt += v > zy;
        ge += (v >= zy) && k != (int)y;
    }
    se = wave_sum(se); sz = wave_sum(sz);
    gt = wave_sum(gt); ge = wave_sum(ge);
    const float lse = m + logf(se);
    const float nan = __uint_as_float(0x7FC00000u);
    if (lane == 0) {
        row_loss[b] = valid ? (1.f - smoothing) * (lse - zy) + smoothing * (lse - sz / (float)K) : nan;
        if (counters && valid) {
            if (ge == 0) atomicAdd(counters, 1);
            if (gt < 5) atomicAdd(counters + 1, 1);
        }
    }
    if (dlogits) {
        const float invB = 1.0f / (float)B, uni = smoothing / (float)K;
        float* d = dlogits + (size_t)b * K;
        for (int k = lane; k < K; k += 64) {
            const float p = expf(z[k] - lse);
            d[k] = valid ? (p - (k == (int)y ? 1.f - smoothing : 0.f) - uni) * invB : nan;
        }
    }
}

// mean of row_loss: one wave walks the rows in order, 64 at a time
__global__ __launch_bounds__(64)
void probe_loss_mean_kernel(const float* __restrict__ row_loss, float* __restrict__ loss_out, int B) {
    float acc = 0.f;
    for (int b0 = 0; b0 < B; b0 += 64) acc += wave_sum(b0 + (int)threadIdx.x < B ? row_loss[b0 + threadIdx.x] : 0.f);
    if (threadIdx.x == 0) *loss_out = acc / (float)B;
}

// ---- launchers: arguments are validated before anything touches the device ----
extern "C" int64_t uvit_op_probe_pool_ws_bytes(int B, int N, int C) {
    if (probe_pool_bad_shape(B, N, C)) return UVIT_ERR_SHAPE;
    return probe_pool_stream_bytes(B, C);
}

extern "C" int uvit_op_probe_pool_norm(const float* x, float* feat, float* scratch, int B, int N, int C, float eps, uvit_stream stream) {
    if (!x || !feat || !scratch) return UVIT_ERR_ARG;
    if (probe_pool_bad_shape(B, N, C)) return UVIT_ERR_SHAPE;
    probe_pool_launch(PoolStreams{{x, nullptr}, {feat, nullptr}}, 1, scratch, B, N, C, eps, (hipStream_t)stream);
    return uvit_check_launch();
}

extern "C" int uvit_op_probe_logits(const float* feat, const float* W, const float* bias, float* logits, int B, int K, int C,
                                    uvit_stream stream) {
    if (!feat || !W || !bias || !logits) return UVIT_ERR_ARG;
    if (B < 1 || K < 1 || C < 4 || (C % 4) || (B + PT - 1) / PT > 65535) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(probe_logits_kernel, dim3((K + PT - 1) / PT, (B + PT - 1) / PT), dim3(256), 0, (hipStream_t)stream, feat, W, bias,
                       logits, B, K, C);
    return uvit_check_launch();
}

extern "C" int uvit_op_probe_ce(const float* logits, const int64_t* labels, float smoothing, float* dlogits, float* row_loss,
                                float* loss_out, int32_t* top1_top5, int B, int K, uvit_stream stream) {
    if (!logits || !labels || !row_loss || !loss_out || !(smoothing >= 0.f && smoothing < 1.f)) return UVIT_ERR_ARG;
    if (B < 1 || K < 1) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(probe_ce_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, s, logits, labels, smoothing, dlogits, row_loss, (int*)top1_top5, B, K);
    hipLaunchKernelGGL(probe_loss_mean_kernel, dim3(1), dim3(64), 0, s, (const float*)row_loss, loss_out, B);
    return uvit_check_launch();
}

extern "C" int uvit_op_probe_head_grad(const float* dlogits, const float* feat, float* dW, float* dbias, int B, int K, int C,
                                       uvit_stream stream) {
    if (!dlogits || !feat || !dW || !dbias) return UVIT_ERR_ARG;
    if (B < 1 || K < 1 || C < 4 || (C % 4) || (K + PT - 1) / PT > 65535) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(probe_head_grad_kernel, dim3((C + PT - 1) / PT, (K + PT - 1) / PT), dim3(256), 0, (hipStream_t)stream, dlogits, feat,
                       dW, dbias, B, K, C);
    return uvit_check_launch();
}
