// Internal launch interfaces shared by the .hip translation units of libuvit (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

enum { EPI_BF16 = 0, EPI_QKV = 1, EPI_GELU = 2, EPI_RESID = 3, EPI_F32 = 4, EPI_PATCH = 5, EPI_DGELU = 6, EPI_QKV_ELU = 7,
       EPI_GELU_DG = 8,    // out = gelu(h), out2 = gelu'(h) (bf16): what backward needs of h, computed beside gelu (shared erf / exp)
       EPI_MULAUX = 9 };   // out = acc * aux (bf16): GELU backward against the stored gelu'(h), no transcendental work

struct GemmEpi {
    void* out = nullptr;             // bf16 or f32 [M, ldo]
    void* out2 = nullptr;            // GELU: pre-activation h (bf16); RESID: branch output before gamma (bf16)
    const float* bias = nullptr;     // [N]   (QKV: q_bias [N/3])
    const float* bias2 = nullptr;    // QKV: v_bias [N/3]
    const float* gamma = nullptr;    // RESID: LayerScale [N]
    const float* resid = nullptr;    // RESID: residual stream [M, ldo] f32
    const float* rowscale = nullptr; // RESID: per-sample drop-path multiplier [B] (null = 1)
    const void* aux = nullptr;       // DGELU: h [M, ldo] bf16
    const int64_t* mask = nullptr;   // PATCH: bool_masked_pos flattened [B*P] (null = teacher)
    const float* mask_token = nullptr;
    int ldo = 0;
    int tokens = 1;                  // RESID: rows per sample
    int patches = 1;                 // PATCH: rows per sample in the GEMM
    int row0 = 0;                    // RESID: sample index of GEMM row m is (m + row0) / tokens (row-split launches)
    int ngroup = 0;                  // 256x256 kernel: column tiles per row-tile group of the XCD-aware tile order (0 = 6)
    // RESID over a COMPACT row list (the student's last MLP on the masked rows only): GEMM row m stands for residual-stream row
    // rowmap[m] -- resid is read and out / out2 are written THERE, the drop-path sample is rowmap[m] / tokens; rows m >= *rowcount
    // are padding and write nothing
    const int* rowmap = nullptr;
    const int* rowcount = nullptr;
    // persistent 256x256 kernel: 16 zero-initialised counters (8 per-XCD tile counters, 1 exit counter) in device memory -> the workgroups
    // take their tiles from the counters instead of by a fixed stride (nullptr: fixed stride); the last workgroup to leave zeroes them again
    unsigned* tile_counter = nullptr;
};

// gemm.hip
// Launch tuning (mirrors uvit_tuning in include/uvit.h).  Passed by the caller on every launch: the launchers keep no
// mutable process-wide state, so host threads launching on different streams do not interact.
struct GemmTune {
    int nt_variant = 3;      // 0: 128x128, 1: 256x256 staggered (1 WG/CU), 5: 320x256, 3: auto by shape
    int tn_variant = 3;      // 0: 128x128 kernel, 1: 256x256 staggered kernel, 3: auto
    int tn_target = 512;     // workgroups the wgrad split-K aims for (MI355X sweep: 512 beats 256..1536 on all four wgrad shapes)
    int group_chunks = 0;    // grouped wgrad: 0 = cost model, > 0 = forced token-chunk count
    int nt_group = 0;        // 256x256 NT kernel: column tiles per row-tile group of the tile order (0 = default 6)
    int nt_persist = 1;      // 256x256 NT kernel, more tiles than CUs: persistent workgroups, operand pipeline across tiles
};
// What one NT launch runs (the dispatch of uvit_gemm_nt_launch): kind = the kernel of the first `rows` rows on `grid` workgroups,
// tail_rows = the remaining rows, which go to a second launch of the 128x128 kernel (0: none).
enum { NT_128 = 0, NT_256 = 1, NT_256P = 2, NT_320 = 3, NT_RING128 = 4, NT_RING160 = 5, NT_KINDS = 6 };
struct NtPlan { int kind; int rows; int grid; int tail_rows; };
// The plan of a launch on a device with num_cu CUs: host arithmetic only, no device is touched.  Returns the launcher's error codes.
int uvit_gemm_nt_plan(int mode, int M, int N, int K, int lda, int ldw, int ldo, bool row_list, const GemmTune* tune, int num_cu,
                      NtPlan* out);
// tune == nullptr: defaults.  tail_rows_out (nullable) receives the rows that went to the row-split tail launch.
int uvit_gemm_nt_launch(int mode, const void* A, const void* W, int M, int N, int K, int lda, int ldw,
                        const GemmEpi* epi, hipStream_t s, const GemmTune* tune = nullptr, int* tail_rows_out = nullptr);
// allow_split: partial sums are combined with fp32 atomics -> C must be zero (or hold a value to add to)
int uvit_gemm_tn_launch(const void* Y, const void* X, int M, int Nn, int Kk, int ldy, int ldx, float* C,
                        int ldc, int allow_split, hipStream_t s, const GemmTune* tune = nullptr);

// grouped wgrad (all Linear weight gradients of one layer in one launch, bias column sums fused)
#define UVIT_TN_GROUP_MAX 6
struct TnProb {
    const void* Y = nullptr;         // dY [M, ldy] bf16 (rows beyond the real tokens are zero)
    const void* X = nullptr;         // layer input [M, ldx] bf16
    float* C = nullptr;              // dW [Nn, ldc] fp32, accumulated into (zeroed arena)
    float* bias = nullptr;           // column sums of Y[:, 0:bias_end) (null: none)
    float* bias2 = nullptr;          // column sums of Y[:, bias2_begin:Nn) (qkv: v_bias; null: none)
    int bias_end = 0, bias2_begin = 0;
    // stacked two-stream operands (rows [0, s1_row) = mean stream, [s1_row, M) = covariance stream) whose bias differs per stream: the
    // column sums of the rows from s1_row on go to bias_s1 / bias2_s1 (s1_row = 0: one stream); every token chunk must lie in ONE stream
    float* bias_s1 = nullptr; float* bias2_s1 = nullptr; int s1_row = 0;
    int M = 0, Nn = 0, Kk = 0, ldy = 0, ldx = 0, ldc = 0;
    // filled by the launcher
    int nm = 0, tiles_n = 0, tiles_k = 0, chunk_steps = 0, chunks = 0;
};
struct TnGroup { TnProb p[UVIT_TN_GROUP_MAX]; int nprob = 0; int max_chunks = 0; };
bool uvit_gemm_tn_group_ok(const TnProb* probs, int n, const GemmTune* tune = nullptr);
int uvit_gemm_tn_group_launch(const TnProb* probs, int n, hipStream_t s, const GemmTune* tune = nullptr);

// attention.hip
// bmap != nullptr: the launch runs a COMPACT batch (drop-path sample list); sample slot b draws the dropout of sample bmap[b]
int uvit_attn_fwd_launch(const void* qkv, const float* biasP, void* out, float* lse, int B, int H, int N, int NP,
                         float scale, float p_drop, uint32_t seed, uint32_t layer, hipStream_t s, const int* bmap = nullptr,
                         int head_dim = 64);     // head_dim: 64 or 80 (qkv (B, N, 3, H, head_dim))
// fused backward (one recomputation of P; dS leaves as bf16 for the bias gradient): ds_ws holds uvit_attn_bwd_fused_ws_bytes()
// bytes and is written when want_ds != 0; uvit_attn_dbias_reduce_launch sums it over the batch into ONE [H][NP][NP] slab laid out
// [h][key][q] (accumulate = 0: the slab is zero-filled first).  Two launches so that the reduction can run on another stream.
size_t uvit_attn_bwd_fused_ws_bytes(int B, int H, int N);
int uvit_attn_bwd_fused_launch(const void* qkv, const void* o_fwd, const void* d_o, const float* biasP, const float* lse,
                               float* delta, void* dqkv, void* ds_ws, int want_ds, int B, int H, int N, int NP, float scale,
                               float p_drop, uint32_t seed, uint32_t layer, hipStream_t s, const int* bmap = nullptr,
                               int head_dim = 64);
int uvit_attn_dbias_reduce_launch(const void* ds_ws, float* dbias_slab, int accumulate, int B, int H, int N, int NP, hipStream_t s);

// attention2.hip (two-stream Wasserstein attention)
int uvit_attn2_fwd_launch(const void* qkv_m, const void* qkv_c, const float* biasP, void* out_m, void* out_c, float* lse,
                          int B, int H, int N, int NP, float scale, float p_drop, uint32_t seed, uint32_t layer, hipStream_t s);
// fused backward (round 4; same contract as the base model's): dS tiles (bf16) go to ds_ws when want_ds != 0 and
// uvit_attn2_dbias_reduce_launch sums them over the batch into ONE [H][NP][NP] slab laid out [h][key][q]
size_t uvit_attn2_bwd_ws_bytes(int B, int H, int N);
int uvit_attn2_bwd_launch(const void* qkv_m, const void* qkv_c, const void* o_m, const void* o_c, const void* d_m, const void* d_c,
                          const float* biasP, const float* lse, float* delta, void* dqkv_m, void* dqkv_c, void* ds_ws, int want_ds,
                          int B, int H, int N, int NP, float scale, float p_drop, uint32_t seed, uint32_t layer, hipStream_t s);
int uvit_attn2_dbias_reduce_launch(const void* ds_ws, float* dbias_slab, int accumulate, int B, int H, int N, int NP, hipStream_t s);

// norm.hip
// LayerNorm forward, y = bf16((x - mean) * rstd * w + b), one wave per row.  The walk follows from the fields that are set:
//   rows     (default) y / mean / rstd row r <- x row rowidx[r] (null: r); rows r >= *count (null: M) are padding and get zeros;
//   samples  (pos) dense walk of x with a COMPACT y: sample b's rows go to slot pos[b] of y / mean / rstd, a dropped sample's (pos[b] < 0)
//            rows are copied to xcopy -- the branch's output stream, x + 0 * branch, which its residual epilogue then does not touch.
struct LnFwd {
    const float* x = nullptr;        // [.., C] f32 residual stream
    const float* w = nullptr;        // [C]
    const float* b = nullptr;        // [C]
    bf16* y = nullptr;               // [M, C] (samples: compact)
    float* mean = nullptr;           // [M] saved statistics, indexed like y (rows walk: both nullable)
    float* rstd = nullptr;
    int M = 0, C = 0;                // rows walked
    float eps = 0.f;
    const int* rowidx = nullptr;     // rows walk
    const int* count = nullptr;
    const int* pos = nullptr;        // samples walk: [M / tokens]
    float* xcopy = nullptr;          // samples walk: [M, C]
    int tokens = 0;                  // samples walk: rows per sample
};
int uvit_ln_fwd_launch(const LnFwd& p, hipStream_t s);

// The branch whose LayerScale + DropPath backward rides along in a row-wise backward pass over the residual-stream gradient d
// (modeling_finetune.py:295-298): with e = d * rowscale[sample]:  dy = bf16(e * gamma),  dgamma += e * y,  dbias += dy.
struct LsNext {
    const bf16* y = nullptr;         // branch output before gamma, dense-indexed
    const float* gamma = nullptr;    // [C]
    const float* rowscale = nullptr; // per-sample drop-path multiplier (null = 1)
    bf16* dy = nullptr;              // null: no branch rides along
    float* dgamma = nullptr;         // replicated column-sum accumulators
    float* dbias = nullptr;
    int tokens = 0;                  // rows per sample of the residual stream (a samples-walk LayerNorm backward reads it without a rider, too)
    // LayerNorm backward only -- dy is COMPACT by the branch's drop-path sample list:
    const int* pos = nullptr;        // sample -> compact slot, -1 = dropped: writes nothing, adds nothing (null: dense)
    const int* cnt = nullptr;        // samples walk: kept rows; the last workgroup zero-fills the pad rows of dy, cnt .. the next multiple of 64 of
    int pad_base = 0;                //   pad_base + cnt (the wgrad's reduction length; pad_base = rows in front of dy in a stacked buffer)
    bf16* pad2 = nullptr;            //   and the same rows of a second buffer [rows][pad2_cols] (the attention branch's dqkv, which the attention
    int pad2_cols = 0;               //   backward writes for the kept samples only)
};
// LayerNorm backward: dx = dres + rstd * (dy*w - mean(dy*w) - xhat * mean(dy*w*xhat));  dw += dy*xhat;  db += dy, with `next` fused on dx.
//   rows     (default) dy / mean / rstd row r belongs to residual-stream row rowidx[r] (null: r), where x, dres, dx and next.y live; rows
//            r >= *count are skipped (dx keeps what it held); next.dy is indexed like dx, or compact by next.pos;
//   samples  (pos, next.cnt, or next.pos without a row list) dense walk of the residual stream: dy / mean / rstd compact by pos (null: every
//            sample kept) -- a dropped sample's rows pass dres through (dx = dres) and add nothing to dw / db; next.dy compact by next.pos.
struct LnBwd {
    const bf16* dy = nullptr;
    const float* x = nullptr;
    const float* mean = nullptr;
    const float* rstd = nullptr;
    const float* w = nullptr;
    const float* dres = nullptr;     // gradient already on the residual stream (rows walk: null = 0)
    float* dx = nullptr;
    float* dw = nullptr;             // replicated column-sum accumulators: workgroup g adds into replica g % nrep
    float* db = nullptr;
    int M = 0, C = 0;                // rows walked
    int nrep = 1;
    size_t rep_stride = 0;
    const int* rowidx = nullptr;     // rows walk; a row list needs its count
    const int* count = nullptr;
    const int* pos = nullptr;        // samples walk
    LsNext next;
};
int uvit_ln_bwd_launch(const LnBwd& p, hipStream_t s);
int uvit_reduce_replicas_launch(const float* rep, float* out, size_t n, int nrep, size_t stride, hipStream_t s);
int uvit_target_accum_launch(const float* x, const int* rowidx, const int* count, float* acc, int first, int Mmax,
                             int C, float eps, hipStream_t s, const float* sub = nullptr,     // sub: rows subtracted before the LayerNorm
                             int ln = 1);                                                   // ln = 0: no LayerNorm, the rows are summed as they are
int uvit_variance_loss_launch(const float* out, const int* count, float w, float margin, float loss_scale, float* scratch,
                              float* loss, float* std_loss0_out, void* dout_bf16, int Mmax, int C, hipStream_t s);
int uvit_gather_patch_rows_launch(const float* x, const float* sub, float* v, int B, int P, int C, hipStream_t s);
int uvit_colnorm_launch(float* v, int groups, int rows, int C, float eps, hipStream_t s);
int uvit_axpy_rows_launch(float* acc, const float* v, int first, size_t n, hipStream_t s);
int uvit_gather_masked_rows_launch(const float* dense, const int* rowidx, const int* count, float* out, int Mmax, int P, int C,
                                   hipStream_t s);
int uvit_target_finalize_launch(float* acc, const int* count, int n_layers, int post_ln, int Mmax, int C, float eps,
                                hipStream_t s);

// elementwise.hip
int uvit_im2col_launch(const float* img, void* cols_bf16, int B, int Cin, int img_size, int patch, hipStream_t s);
int uvit_mask_compact_launch(const int64_t* mask, int* rowidx, int* count, int B, int P, hipStream_t s);
int uvit_set_cls_launch(float* x, const float* cls, const float* pos, int B, int N, int C, hipStream_t s);
int uvit_relpos_gather_launch(const float* table, const int* index, float* biasP, int H, int N, int NP, hipStream_t s);
int uvit_relpos_scatter_launch(const float* slab, int nslab, const int* index, float* dtable, int H, int N, int NP,
                               hipStream_t s);
// LayerScale + DropPath backward on its own (ls.pos / cnt / pad unused); row list: ls.dy is compact, dx / ls.y live at rowidx[row], rows >= *count get zeros
int uvit_ls_bwd_launch(const float* dx, const LsNext& ls, int M, int C, int nrep, size_t rep_stride, hipStream_t s,
                       const int* rowidx = nullptr, const int* count = nullptr);
// LayerScale gradient from the weight gradient (elementwise.hip): dgamma[j] += sum over the sets of (sum_k W[j][k] dW[j][k] + b[j] *
// sum_r db[r * rep_stride + j]) / gamma[j]; W / dW are [C][K] row-major, K % 8 == 0, nrep <= 64, one or two sets.  gamma[j] == 0:
// dgamma[j] <- 0 and *flag <- 1.
struct LsDgammaSet { const bf16* W; const float* dW; const float* b; const float* db; };
int uvit_ls_dgamma_launch(const LsDgammaSet* sets, int nsets, const float* gamma, float* dgamma, int* flag, int C, int K, int nrep,
                          size_t rep_stride, hipStream_t s);
int uvit_rows_guard_launch(const int* count, int limit, float* loss, hipStream_t s);   // *count > limit: loss <- NaN (the step is then skipped like any non-finite one)
int uvit_colsum_launch(const void* y_bf16, int ld, int col0, int ncols, int M, float* out, int nrep, size_t rep_stride,
                       hipStream_t s);
int uvit_smooth_l1_launch(const float* out, const float* target, const int* count, float beta, int l2, float loss_scale,
                          float* loss, void* dout_bf16, int Mmax, int C, hipStream_t s);
int uvit_token_bwd_launch(const float* dx, const int64_t* mask, void* dpatch_bf16, float* dcls, float* dmask_token,
                          int B, int P, int C, hipStream_t s);
int uvit_transpose_batch_launch(const void* descs_dev, int ndesc, int max_tiles, hipStream_t s);
int uvit_droppath_launch(float* scales, const float* rates_dev, int depth, int nbr, int B, uint32_t seed, uint32_t step,
                         hipStream_t s);
// drop-path sample lists of a step (elementwise.hip): per (layer, branch) list lb: pos[lb][b], bmap[lb][slot], rows[lb][r] (stride rows_stride,
// pad rows -1), cnt[lb] = kept rows, cnt[nlists + lb] = 1 when the kept SAMPLES differ from host_counts[lb], what the host sized the launches
// with; uvit_droppath_lists_guard_launch turns any such flag into a NaN loss
int uvit_droppath_lists_launch(const float* scales, int* pos, int* bmap, int* rows, int* cnt, int nlists, int B, int tokens,
                               int rows_stride, const int* host_counts, hipStream_t s);
int uvit_droppath_lists_guard_launch(const int* cnt, int nlists, float* loss, hipStream_t s);
int uvit_add_pos_launch(float* x, const float* pos, int B, int N, int C, hipStream_t s);
int uvit_pos_bwd_launch(const float* dx, float* dpos, int B, int N, int C, hipStream_t s);
int uvit_synth_batch_launch(float* images, int64_t* mask, int B, int chans, int img_size, int patches, int n_mask, uint32_t seed,
                            uint32_t it, hipStream_t s);
int uvit_poison_if_nonfinite_launch(const float* loss, float* dst, int* sticky, hipStream_t s);
int uvit_wasserstein_loss_launch(const float* out_m, const float* out_c, const float* tgt_m, const float* tgt_c, const int* count,
                                 float lam, float loss_scale, float* scratch, float* loss, void* dout_m_bf16, void* dout_c_bf16,
                                 int Mmax, int C, hipStream_t s);

// optim.hip
// guard_loss / guard_sumsq (nullable, device): the update is skipped when either holds a non-finite value
int uvit_ema_launch(float* ema, const float* p, void* ema_bf16, size_t n, float decay, hipStream_t s, const float* guard_loss = nullptr,
                    const double* guard_sumsq = nullptr);
int uvit_sumsq_launch(const float* g, size_t n, double* out, hipStream_t s);
int uvit_adamw_launch(float* p, const float* g, float* m, float* v, void* p_bf16, size_t n, size_t n_decay, float lr,
                      float wd, float b1, float b2, float eps, int step, const double* sumsq, float max_norm,
                      float grad_scale, float* gnorm_out, hipStream_t s, const float* guard_loss = nullptr,
                      float* ema = nullptr, void* ema_bf16 = nullptr, float ema_decay = 0.f,    // ema: fused EMA teacher update
                      int* sticky_poison = nullptr,    // set (and honoured) once a step's loss / norm was not finite
                      const float* sched_dev = nullptr, int sched_len = 0, int sched_idx = 0);   // device-resident {lr, wd, ema decay} tables
int uvit_zero_launch(void* dst, size_t bytes, hipStream_t s);
int uvit_cast_bf16_launch(const float* src, void* dst_bf16, size_t n, hipStream_t s);

struct TransposeDesc { const void* src; void* dst; int rows; int cols; int tile0; int pad; };
