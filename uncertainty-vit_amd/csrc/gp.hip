// Random-feature Gaussian-process head on the frozen encoder (gfx950): the reference's modeling_finetune.SNGP (:525-638) behind the
// probe's pooled features
//   features         :579-587   g = LayerNorm(f; gamma, beta, eps); u = g . W_rf^T + b_rf; phi = scale * cos(u)
//   precision        :599-616   P <- m P + (1 - m) phi^T phi / B   (m > 0),   P <- P + phi^T phi   (m <= 0)
//   LayerNorm grads  autograd   dphi = dz . W_out; du = -scale sin(u) dphi; dg = du . W_rf; dgamma = sum_b dg ghat; dbeta = sum_b dg
//   variance         :618-626   var[b] = ridge phi_b^T Sigma phi_b, the diagonal of compute_predictive_covariance, in double
//   mean field       edward2    out = z / sqrt(1 + factor var)   (an addition: the reference has no such step)
// The output layer and its gradient are uvit_op_probe_logits / uvit_op_probe_head_grad on phi.  fp32 except where stated.  No float
// atomics: every sum has one owner and a fixed order, so the same input gives the same bits on every run.  These are 0.1-0.2 GFLOP
// per launch beside an encoder forward of several milliseconds: LDS-tiled FMA kernels, not MFMA ones.
// Compiled WITHOUT -ffast-math (build.sh): the order of the sums below is part of the contract and cosf / sinf are the accurate ones.
#ifdef __FAST_MATH__
#error "gp.hip fixes the order of its sums and needs accurate cosf / sinf: build it without -ffast-math"
#endif
#include <math.h>

#include "../../include/uvit.h"
#include "probe_common.h"
#include "rowwise.h"

#define GT 64                // output tile edge: 256 threads with a 4 x 4 micro-tile each
#define GK 16                // reduction steps per LDS tile
#define GP_MAX_B 65535
#define GP_MAX_D 2048

// ---- features: row statistics by one wave per row, then the (B, C) x (C, D) contraction with the + b_rf, cos, * scale epilogue ----
// Every workgroup recomputes the statistics of its 64 rows (the same arithmetic in every column tile, so the same bits); the
// workgroups of column tile 0 write ghat.  The LayerNorm is applied while the tile of f is staged: g never goes to memory.
template <int NV>
__global__ __launch_bounds__(256)
void gp_features_kernel(const float* __restrict__ feat, const float* __restrict__ gamma, const float* __restrict__ beta,
                        const float* __restrict__ W, const float* __restrict__ brf, float scale, float eps, float* __restrict__ ghat,
                        float* __restrict__ u, float* __restrict__ phi, int B, int C, int D) {
    __shared__ __attribute__((aligned(16))) float As[GK][GT + 4], Ws[GK][GT + 4];
    __shared__ float smean[GT], srstd[GT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wave = tid >> 6;
    const int d0 = blockIdx.x * GT, b0 = blockIdx.y * GT;
    for (int r = wave; r < GT; r += 4) {                  // wave-uniform: a row belongs to one wave
        const int b = b0 + r;
        float mean = 0.f, rstd = 0.f;
        if (b < B) {
            RowVec<NV> row;
            load_row(row, feat + (size_t)b * C, C, lane);
            row_stats(row, C, lane, eps, mean, rstd);
            if (ghat && blockIdx.x == 0) normalize_store(row, mean, rstd, ghat + (size_t)b * C, false, C >> 2, lane);
        }
        if (lane == 0) { smean[r] = mean; srstd[r] = rstd; }
    }
    __syncthreads();
    const int lr = tid >> 2, lc = (tid & 3) * 4;          // staging: tile row, first of four reduction columns
    const float mean = smean[lr], rstd = srstd[lr];
    float acc[4][4] = {};
    for (int c0 = 0; c0 < C; c0 += GK) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), w = a;
        if (c0 + lc < C) {                                // C % 4 == 0: a float4 is inside the row or outside it
            if (b0 + lr < B) {
                const float4 f = *(const float4*)(feat + (size_t)(b0 + lr) * C + c0 + lc);
                const float4 h = normalize4(f, mean, rstd), gm = *(const float4*)(gamma + c0 + lc), bt = *(const float4*)(beta + c0 + lc);
                a = make_float4(h.x * gm.x + bt.x, h.y * gm.y + bt.y, h.z * gm.z + bt.z, h.w * gm.w + bt.w);
            }
            if (d0 + lr < D) w = *(const float4*)(W + (size_t)(d0 + lr) * C + c0 + lc);
        }
        __syncthreads();
        As[lc][lr] = a.x; As[lc + 1][lr] = a.y; As[lc + 2][lr] = a.z; As[lc + 3][lr] = a.w;
        Ws[lc][lr] = w.x; Ws[lc + 1][lr] = w.y; Ws[lc + 2][lr] = w.z; Ws[lc + 3][lr] = w.w;
        __syncthreads();
        // tile-wise sums, as probe_logits_kernel: C / 16 additions at full magnitude instead of C
        float t[4][4] = {};
#pragma unroll
        for (int c = 0; c < GK; ++c) {
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
    const int d = d0 + tx * 4;
    if (d >= D) return;                                   // D % 4 == 0: the four columns are inside the row or outside it
    const float4 bb = *(const float4*)(brf + d);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + ty * 4 + i;
        if (b >= B) continue;
        const float4 uu = make_float4(acc[i][0] + bb.x, acc[i][1] + bb.y, acc[i][2] + bb.z, acc[i][3] + bb.w);
        if (u) *(float4*)(u + (size_t)b * D + d) = uu;
        *(float4*)(phi + (size_t)b * D + d) = make_float4(scale * cosf(uu.x), scale * cosf(uu.y), scale * cosf(uu.z), scale * cosf(uu.w));
    }
}

// ---- precision: P (D, D) in place; element (i, j) = one fma chain over b in ascending order, then the blend with the old value.
// (i, j) and (j, i) are formed from the same products (a * b == b * a) in the same order and blended with the same old value when
// P came in symmetric, so they come out with identical bits.
__global__ __launch_bounds__(256)
void gp_precision_kernel(const float* __restrict__ phi, float* __restrict__ P, int B, int D, float m, float om) {
    __shared__ __attribute__((aligned(16))) float Is[GK][GT + 4], Js[GK][GT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int j0 = blockIdx.x * GT, i0 = blockIdx.y * GT;
    const int fr = tid >> 4, fc = (tid & 15) * 4;         // staging: batch row, first of four columns
    float acc[4][4] = {};
    for (int b0 = 0; b0 < B; b0 += GK) {
        float4 vi = make_float4(0.f, 0.f, 0.f, 0.f), vj = vi;
        if (b0 + fr < B) {
            if (i0 + fc < D) vi = *(const float4*)(phi + (size_t)(b0 + fr) * D + i0 + fc);
            if (j0 + fc < D) vj = *(const float4*)(phi + (size_t)(b0 + fr) * D + j0 + fc);
        }
        __syncthreads();
        *(float4*)&Is[fr][fc] = vi;
        *(float4*)&Js[fr][fc] = vj;
        __syncthreads();
#pragma unroll
        for (int b = 0; b < GK; ++b) {                    // rows past B hold zeros: fma(0, 0, acc) = acc
            const float4 iv = *(const float4*)&Is[b][ty * 4], jv = *(const float4*)&Js[b][tx * 4];
            const float ii[4] = {iv.x, iv.y, iv.z, iv.w}, jj[4] = {jv.x, jv.y, jv.z, jv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ii[i], jj[j], acc[i][j]);
        }
    }
    const int j = j0 + tx * 4;
    if (j >= D) return;
    const float fB = (float)B;                            // the reference divides the batch sum by the batch size
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = i0 + ty * 4 + i;
        if (r >= D) continue;
        float4* dst = (float4*)(P + (size_t)r * D + j);
        const float4 o = *dst;
        float4 n;
        if (m > 0.f) {                                    // one explicit form for every element: no contraction may tell (i, j) from (j, i)
            n.x = fmaf(m, o.x, om * (acc[i][0] / fB)); n.y = fmaf(m, o.y, om * (acc[i][1] / fB));
            n.z = fmaf(m, o.z, om * (acc[i][2] / fB)); n.w = fmaf(m, o.w, om * (acc[i][3] / fB));
        } else {
            n.x = o.x + acc[i][0]; n.y = o.y + acc[i][1]; n.z = o.z + acc[i][2]; n.w = o.w + acc[i][3];
        }
        *dst = n;
    }
}

// ---- out (M, N) = A (M, R) . Bm (R, N), both row-major, R arbitrary, N % 4 == 0; tile-wise sums over R in ascending order.
// EPI 0: out = acc.  EPI 1: out = -scale * sinf(u) * acc (the derivative of scale * cos(u), u (M, N)).
template <int EPI>
__global__ __launch_bounds__(256)
void gp_nn_kernel(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ u, float scale,
                  float* __restrict__ out, int M, int R, int N) {
    __shared__ __attribute__((aligned(16))) float As[GK][GT + 4], Bs[GK][GT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * GT, m0 = blockIdx.y * GT;
    const int ar = tid >> 2, ac = (tid & 3) * 4;          // A staging: tile row, first of four reduction columns (scalar loads: R % 4 != 0 is allowed)
    const int br = tid >> 4, bc = (tid & 15) * 4;         // Bm staging: reduction row, first of four columns
    float acc[4][4] = {};
    for (int r0 = 0; r0 < R; r0 += GK) {
        float a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = (m0 + ar < M && r0 + ac + q < R) ? A[(size_t)(m0 + ar) * R + r0 + ac + q] : 0.f;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + br < R && n0 + bc < N) w = *(const float4*)(Bm + (size_t)(r0 + br) * N + n0 + bc);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) As[ac + q][ar] = a[q];
        *(float4*)&Bs[br][bc] = w;
        __syncthreads();
        float t[4][4] = {};
#pragma unroll
        for (int r = 0; r < GK; ++r) {
            const float4 av = *(const float4*)&As[r][ty * 4], wv = *(const float4*)&Bs[r][tx * 4];
            const float aa[4] = {av.x, av.y, av.z, av.w}, ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) t[i][j] = fmaf(aa[i], ww[j], t[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += t[i][j];
    }
    const int n = n0 + tx * 4;
    if (n >= N) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int mrow = m0 + ty * 4 + i;
        if (mrow >= M) continue;
        float4 o = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        if (EPI == 1) {
            const float4 uu = *(const float4*)(u + (size_t)mrow * N + n);
            o.x *= -scale * sinf(uu.x); o.y *= -scale * sinf(uu.y); o.z *= -scale * sinf(uu.z); o.w *= -scale * sinf(uu.w);
        }
        *(float4*)(out + (size_t)mrow * N + n) = o;
    }
}

// dgamma[c] = sum_b dg[b, c] ghat[b, c], dbeta[c] = sum_b dg[b, c]: one thread per column walks b in ascending order
__global__ __launch_bounds__(64)
void gp_ln_colsum_kernel(const float* __restrict__ dg, const float* __restrict__ ghat, float* __restrict__ dgamma,
                         float* __restrict__ dbeta, int B, int C) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    float sg = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
        const float d = dg[(size_t)b * C + c];
        sg = fmaf(d, ghat[(size_t)b * C + c], sg);
        sb += d;
    }
    dgamma[c] = sg;
    dbeta[c] = sb;
}

// ---- variance: var[b] = ridge * sum_j (sum_i phi_bi Sigma_ij) phi_bj, all in double.  One workgroup of 1024 threads per VB samples;
// thread t owns the columns j = t, t + 1024: it walks the rows i in ascending order (the loads of a wave are adjacent and do not
// depend on one another), multiplies by phi_bj and adds its columns in ascending order; the 64 lanes of a wave meet in a fixed
// shuffle tree and the sixteen waves are added in wave order.
#define VB 4
#define VT 1024

__global__ __launch_bounds__(VT)
void gp_variance_kernel(const float* __restrict__ phi, const double* __restrict__ Sigma, double ridge, double* __restrict__ var,
                        int B, int D) {
    __shared__ float ph[VB][GP_MAX_D];
    __shared__ double red[VT / 64][VB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b0 = blockIdx.x * VB;
    for (int v = 0; v < VB; ++v)
        for (int j = tid; j < D; j += VT) ph[v][j] = b0 + v < B ? phi[(size_t)(b0 + v) * D + j] : 0.f;
    __syncthreads();
    double s[VB] = {};
    for (int j = tid; j < D; j += VT) {
        double t[VB] = {};
#pragma unroll 8
        for (int i = 0; i < D; ++i) {
            const double sg = Sigma[(size_t)i * D + j];
#pragma unroll
            for (int v = 0; v < VB; ++v) t[v] = fma((double)ph[v][i], sg, t[v]);
        }
#pragma unroll
        for (int v = 0; v < VB; ++v) s[v] = fma(t[v], (double)ph[v][j], s[v]);
    }
#pragma unroll
    for (int v = 0; v < VB; ++v) s[v] = wave_sum(s[v]);     // every wave takes part: threads without a column carry zeros
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < VB; ++v) red[wave][v] = s[v];
    }
    __syncthreads();
    if (tid < VB && b0 + tid < B) {
        double a = red[0][tid];
        for (int w = 1; w < VT / 64; ++w) a += red[w][tid];
        var[b0 + tid] = ridge * a;
    }
}

// ---- mean field: out[b, k] = z[b, k] / sqrt(1 + factor var[b]) in double, rounded once to fp32; one wave per row; out may be z ----
__global__ __launch_bounds__(256)
void gp_mean_field_kernel(const float* logits, const double* __restrict__ var, double factor, float* out, int B, int K) {
    const int lane = WavePerRow::lane(), b = WavePerRow::row();
    if (b >= B) return;
    const double den = sqrt(1.0 + factor * var[b]);
    const float* z = logits + (size_t)b * K;
    float* o = out + (size_t)b * K;
    for (int k = lane; k < K; k += 64) o[k] = (float)((double)z[k] / den);
}

// ---- launchers: arguments are validated before anything touches the device ----
static inline bool gp_bad_bcd(int B, int C, int D) {
    return B < 1 || B > GP_MAX_B || C < 4 || (C % 4) || C > ROW_MAXV * 256 || D < 4 || (D % 4) || D > GP_MAX_D;
}

extern "C" int uvit_op_gp_features(const float* feat, const float* gamma, const float* beta, const float* W_rf, const float* b_rf,
                                   float scale, float ln_eps, float* ghat, float* u, float* phi, int B, int C, int D,
                                   uvit_stream stream) {
    if (!feat || !gamma || !beta || !W_rf || !b_rf || !phi || !(ln_eps >= 0.f) || !(scale == scale)) return UVIT_ERR_ARG;
    if (gp_bad_bcd(B, C, D)) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    dispatch_nv(C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((gp_features_kernel<NV>), dim3((D + GT - 1) / GT, (B + GT - 1) / GT), dim3(256), 0, s, feat, gamma, beta, W_rf,
                           b_rf, scale, ln_eps, ghat, u, phi, B, C, D);
    });
    return uvit_check_launch();
}

extern "C" int uvit_op_gp_precision_update(const float* phi, float* P, int B, int D, double momentum, uvit_stream stream) {
    if (!phi || !P || !(momentum == momentum) || momentum >= 1.0) return UVIT_ERR_ARG;
    if (gp_bad_bcd(B, 4, D)) return UVIT_ERR_SHAPE;
    // the reference multiplies by the Python doubles m and 1 - m, each rounded to fp32 on its own (modeling_finetune.py:608-610)
    const int nt = (D + GT - 1) / GT;
    hipLaunchKernelGGL(gp_precision_kernel, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, phi, P, B, D, (float)momentum,
                       (float)(1.0 - momentum));
    return uvit_check_launch();
}

extern "C" int64_t uvit_op_gp_ln_grad_ws_bytes(int B, int C, int D) {
    if (gp_bad_bcd(B, C, D)) return UVIT_ERR_SHAPE;
    return ((int64_t)B * D + (int64_t)B * C) * (int64_t)sizeof(float);
}

extern "C" int uvit_op_gp_ln_grad(const float* dlogits, const float* W_out, const float* u, const float* W_rf, const float* ghat,
                                  float scale, float* dgamma, float* dbeta, float* scratch, int B, int K, int C, int D,
                                  uvit_stream stream) {
    if (!dlogits || !W_out || !u || !W_rf || !ghat || !dgamma || !dbeta || !scratch || !(scale == scale)) return UVIT_ERR_ARG;
    if (gp_bad_bcd(B, C, D) || K < 1) return UVIT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    float* du = scratch;
    float* dg = scratch + (size_t)B * D;
    const int bt = (B + GT - 1) / GT;
    hipLaunchKernelGGL((gp_nn_kernel<1>), dim3((D + GT - 1) / GT, bt), dim3(256), 0, s, dlogits, W_out, u, scale, du, B, K, D);
    hipLaunchKernelGGL((gp_nn_kernel<0>), dim3((C + GT - 1) / GT, bt), dim3(256), 0, s, (const float*)du, W_rf, (const float*)nullptr, 0.f,
                       dg, B, D, C);
    hipLaunchKernelGGL(gp_ln_colsum_kernel, dim3((C + 63) / 64), dim3(64), 0, s, (const float*)dg, ghat, dgamma, dbeta, B, C);
    return uvit_check_launch();
}

extern "C" int uvit_op_gp_variance(const float* phi, const double* Sigma, double ridge, double* var, int B, int D, uvit_stream stream) {
    if (!phi || !Sigma || !var || !(ridge >= 0.0)) return UVIT_ERR_ARG;
    if (gp_bad_bcd(B, 4, D)) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(gp_variance_kernel, dim3((B + VB - 1) / VB), dim3(VT), 0, (hipStream_t)stream, phi, Sigma, ridge, var, B, D);
    return uvit_check_launch();
}

extern "C" int uvit_op_gp_mean_field(const float* logits, const double* var, double factor, float* out, int B, int K,
                                     uvit_stream stream) {
    if (!logits || !var || !out || !(factor >= 0.0)) return UVIT_ERR_ARG;
    if (B < 1 || B > GP_MAX_B || K < 1) return UVIT_ERR_SHAPE;
    hipLaunchKernelGGL(gp_mean_field_kernel, WavePerRow::grid(B), WavePerRow::block(), 0, (hipStream_t)stream, logits, var, factor, out, B, K);
    return uvit_check_launch();
}
