/* libuvit -- C ABI of the MI355X-native data2vec ViT pre-training step.
 *
 * The reference (fx-erick/uncertainty-vit) is pure Python: it has no FFI / plugin boundary of
 * its own.  This header is therefore the NEW native boundary the build
 * defines; each entry point names the reference code it replaces.  Conventions:
 *   - plain pointers and sizes, no torch types; every pointer is DEVICE memory unless noted;
 *   - the caller allocates all buffers (arenas, workspace); nothing is allocated per call;
 *   - every call is asynchronous and ordered on the `stream` argument (a hipStream_t);
 *   - return value 0 = ok, negative = UVIT_ERR_*; nothing throws;
 *   - no global state besides the engine object.
 * Host-side mirror of the reference's Python API lives in uncertainty-vit_amd/ (ctypes).
 */
#ifndef UVIT_H
#define UVIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVIT_VERSION 100
#define UVIT_MAX_DEPTH 64

typedef struct uvit_engine uvit_engine;
typedef void* uvit_stream;   /* hipStream_t */

/* Constructor arguments of VisionTransformerForCyclicalTraining (modeling_cyclical.py:34-60)
 * plus the per-GPU batch the workspace is sized for. */
typedef struct uvit_config {
    int32_t img_size, patch_size, in_chans, embed_dim, depth, num_heads, mlp_hidden;
    int32_t use_shared_rel_pos_bias;  /* modeling_cyclical.py:84-89 */
    int32_t use_abs_pos_emb;          /* --abs_pos_emb (run_cyclical.py:55, default off): pos_embed (1, N, C) added after the cls concat */
    int32_t batch;
    float ln_eps;                     /* 1e-6, modeling_cyclical.py:294 */
    float attn_drop_rate;             /* --attn_drop_rate */
    float drop_path_rate;             /* --drop_path; per-layer linspace(0, rate, depth) */
    int32_t bias_chunk;               /* ignored (it sized the retired dQ kernels); kept for the struct layout */
    int32_t two_stream;               /* 1: DistVisionTransformerForCyclicalTraining (mean, cov) model, modeling_cyclical_dist.py:14-165 */
} uvit_config;

/* One tensor of the flat parameter arena; `name` is the reference state-dict key. */
typedef struct uvit_layout_entry {
    char name[96];
    int64_t offset;   /* in floats, multiple of 64 */
    int64_t numel;
    int32_t ndim;
    int32_t decay;    /* 1 = weight-decay group (optim_factory.py:58-97); 2 = never receives a gradient in the reference (kept constant) */
    int64_t shape[4];
} uvit_layout_entry;

/* Buffers owned by the caller.  fp32 arenas hold `uvit_arena_numel` floats; bf16 shadows the
 * same number of 2-byte elements.  Layout = [decay tensors | no-decay tensors]. */
typedef struct uvit_buffers {
    float* params;        /* student fp32 master weights */
    float* grads;         /* student gradients */
    float* adam_m;
    float* adam_v;
    float* ema;           /* EMA teacher fp32 (timm ModelEmaV2 at run_cyclical.py:503) */
    void* params_bf16;    /* bf16 shadow of params (GEMM operands) */
    void* params_bf16_t;  /* transposed bf16 copies of the 2-D Linear weights (dgrad operands) */
    void* ema_bf16;       /* bf16 shadow of the teacher */
    const int32_t* rel_index;  /* (N*N) relative_position_index as int32 (modeling_finetune.py:339-353) */
    void* workspace;
    int64_t workspace_bytes;
} uvit_buffers;

/* Per-step knobs of train_one_epoch (engine_for_cyclical.py:24-32, 47-56, 88-186). */
typedef struct uvit_step_params {
    int32_t target_layers[UVIT_MAX_DEPTH];
    int32_t n_target_layers;
    int32_t target_layer_norm_last;   /* not --no_target_layer_norm_last */
    int32_t post_target_layer_norm;
    int32_t l2_loss;
    float l1_beta;
    float loss_scale;                 /* -1 = off */
    float clip_grad;                  /* <= 0: no clipping (norm still reported) */
    float lr, weight_decay, beta1, beta2, eps;
    int32_t opt_step;                 /* 1-based AdamW step count */
    float ema_decay;                  /* cur_decay; EMA skipped when do_ema == 0 */
    int32_t do_ema;
    float grad_scale;                 /* multiplies gradients before clipping (1/world after a SUM all-reduce) */
    uint32_t seed;                    /* dropout / drop-path stream */
    uint32_t it;                      /* global iteration, decorrelates masks between steps */
    int32_t train_dropout;            /* 1: apply attn_drop_rate and drop_path_rate in the student */
    float lambda_pretraining;         /* WassersteinLoss weight (two-stream model only; --lambda_pretraining) */
    /* Device-resident schedules (utils.py:408-459 tables + the EMA decay anneal / tri-phase cut-off of
     * engine_for_cyclical.py:55-56,182-185): sched_dev = float[3][sched_len] = {lr, weight_decay, ema_decay} per iteration,
     * ema_decay < 0 meaning "skip EMA".  When non-NULL the optimizer kernels read entry `sched_index` on the device and the
     * scalar fields lr / weight_decay / ema_decay / do_ema above are ignored: the step's launch arguments then do not
     * depend on the iteration (a captured step can be replayed). */
    const float* sched_dev;
    int32_t sched_len, sched_index;
    /* flag-gated arithmetic of the step (no BASELINE config switches it on): */
    int32_t layer_results_fc;         /* --layer_results fc: targets from the teacher's MLP-branch outputs (modeling_cyclical.py:199-205) */
    float var_w0, var_margin0;        /* variance term, engine_for_cyclical.py:130-139,161 (var_w0 <= 0: off) */
    /* target-builder variants (engine_for_cyclical.py:94-118): affine-free batch norm over (B, T) per channel, instance norm
     * over T per (sample, channel) on every target layer; instance norm of the layer average.  Both models: with the two-stream model they act
     * on the MEAN targets (the covariance targets, :73-86, only know the two layer-norm flags). */
    int32_t target_batch_norm, target_instance_norm, post_target_instance_norm;
    /* Upper bound on the number of masked patches of this batch (the loader has bool_masked_pos on the host before the upload), 0 = not
     * given.  The loss reads the student at the masked rows only (modeling_cyclical.py:207,215-225), so with a bound the base model's last
     * block runs its MLP -- forward, dgrads and wgrads -- on those rows alone; results equal the all-rows step.  A bound BELOW the true count
     * makes the loss NaN (the step is then skipped like any non-finite one); the two-stream model ignores it (measured at the end of round 4:
     * the per-stream launches and the larger zero fills cost what the skipped rows save). */
    int32_t n_rows_hint;
} uvit_step_params;

int uvit_version(void);
/* First 16 hex digits of the SHA-256 over csrc/{*.hip,*.h} (sorted by name) + include/uvit.h that the library was built
 * from; the host side compares it with the sources on disk and refuses a stale build. */
const char* uvit_source_hash(void);

/* ---- arena layout (single source of truth for the host-side state-dict views) ---- */
int uvit_layout_count(const uvit_config* cfg);
int uvit_layout_get(const uvit_config* cfg, int index, uvit_layout_entry* out);
int64_t uvit_arena_numel(const uvit_config* cfg, int64_t* n_decay_out);
int64_t uvit_workspace_bytes(const uvit_config* cfg);

/* ---- engine ----
 * Calls on ONE engine must be stream-ordered with respect to one another: issue them on one stream, or order the streams with events, so
 * that no two of them can be in flight at once (a uvit_engine_forward_features on a second stream while a step is still running is not
 * allowed).  They share the workspace and the tile counters of the persistent GEMMs: the engine keeps 2 x 16 counters, the second block
 * for the teacher pass of a step (which it runs beside the student pass itself), the first for every other pass -- chosen by the role of
 * the call, never by the stream it is given.  Different engines are independent. */
uvit_engine* uvit_engine_create(const uvit_config* cfg, const uvit_buffers* bufs, uvit_stream stream, int* err_out);
void uvit_engine_destroy(uvit_engine* e);

/* Refresh bf16 shadows (+ transposes) from the fp32 arenas: which = 1 student, 2 teacher, 3 both.
 * Needed after load_state_dict / init (replaces nothing in the reference; precision plumbing). */
int uvit_engine_sync_shadows(uvit_engine* e, int which, uvit_stream stream);

/* VisionTransformerForCyclicalTraining.forward_features (modeling_cyclical.py:170-207) for
 * `which` = 0 student / 1 teacher weights.  images (B,Cin,S,S) f32; mask (B,P) int64 or NULL.
 * Leaves every layer's residual stream in the workspace (see uvit_engine_ws_ptr). Batch may be
 * <= cfg.batch.  train_dropout applies attention dropout / drop-path with (seed, it). */
int uvit_engine_forward_features(uvit_engine* e, int which, const float* images, const int64_t* mask, int batch,
                                 int train_dropout, uint32_t seed, uint32_t it, uvit_stream stream);
/* Blocks first_layer .. depth-1 once more, from the residual stream X[first_layer] that the preceding uvit_engine_forward_features
 * (same `which`, same `batch`) left in the workspace: the stochastic passes of MC-dropout.  No images: im2col
 * and the embedding are skipped.  With train_dropout (student weights), block l draws the attention-dropout masks it draws in a full
 * forward at (seed, it); drop-path is never applied (the reference's enable_dropout leaves DropPath in eval mode).  Overwrites
 * X[first_layer+1 .. depth], the "xm" of those blocks and their activations; X[0 .. first_layer] are only read, so any number of tails
 * from the same or a lower block may follow one forward, and a tail changes nothing that a later forward or training step computes.
 * A tail from a HIGHER block than an earlier tail since the forward would continue that tail's stream, not the forward's: it is refused
 * (run uvit_engine_forward_features again first).
 * Refused before any launch: UVIT_ERR_SHAPE for the two-stream model; UVIT_ERR_ARG for a NULL engine, first_layer outside [0, depth) or
 * above the lowest first_layer of a tail since the forward, and a `which` or `batch` other than that of the last
 * uvit_engine_forward_features -- which includes the case that there is none, or that a training step, or a tail whose launch failed,
 * has come since (the engine keeps this "tail valid" record). */
int uvit_engine_forward_tail(uvit_engine* e, int which, int batch, int first_layer, int train_dropout, uint32_t seed, uint32_t it,
                             uvit_stream stream);
/* norm + drop cls + (masked-row gather) + lm_head (modeling_cyclical.py:207,215-225) on the last
 * forward_features result.  all_tokens=1: out (B*P, C); else out (count, C) rows in mask order.
 * out must hold B*P*C floats; *count_dev (device int) receives the number of valid rows.
 * which: bit 0 = teacher weights, bit 1 = covariance stream (two-stream model: cov_lm_head). */
int uvit_engine_head(uvit_engine* e, int which, int all_tokens, float* out, int32_t* count_dev, uvit_stream stream);

/* Device pointers into the workspace after a forward: name in {"x" (layer 0..depth residual stream
 * (B,N,C) f32), "xm" (after the attention branch), "loss", "grad_norm", "targets", "outputs", "count"};
 * two-stream model: also "x_cov", "xm_cov", "targets_cov", "outputs_cov"; "poisoned" (one int32: the sticky flag of a skipped step). */
void* uvit_engine_ws_ptr(uvit_engine* e, const char* name, int layer);
/* Rows the last training step ran its last block's MLP on (uvit_step_params.n_rows_hint): 0 = every token row. */
int uvit_engine_compact_rows(uvit_engine* e);

/* ---- the training step, engine_for_cyclical.py:58-186 ---- */
/* teacher forward (no grad) -> targets; student forward; loss; backward through lm_head + final norm */
int uvit_step_begin(uvit_engine* e, const float* images, const int64_t* mask, const uvit_step_params* hp,
                    uvit_stream stream);
/* backward of block `layer` (call depth-1 .. 0); its gradients are complete afterwards */
int uvit_step_backward_layer(uvit_engine* e, int layer, const uvit_step_params* hp, uvit_stream stream);
/* make `stream` wait until block `layer`'s weight gradients (computed on the engine's second stream) are final:
 * call on the communication stream before all-reducing that block's bucket */
int uvit_step_wait_layer_grads(uvit_engine* e, int layer, uvit_stream stream);
/* token assembly + patch embedding + relative-position table gradients */
int uvit_step_backward_embed(uvit_engine* e, uvit_stream stream);
/* clip_grad_norm_ + AdamW (utils.py:375-381) + EMA (engine_for_cyclical.py:182-185) + shadow refresh */
int uvit_step_update(uvit_engine* e, const uvit_step_params* hp, uvit_stream stream);
/* all of the above on one stream (single-GPU fast path) */
int uvit_train_step(uvit_engine* e, const float* images, const int64_t* mask, const uvit_step_params* hp,
                    uvit_stream stream);
/* Launch tuning.  It is an ARGUMENT (engine member / operator-call parameter), never process-wide state, so host
 * threads that launch on different streams cannot disturb one another.
 *   nt_variant: NT GEMM kernel for large shapes: 3 = auto by shape (default), 1 = 256x256 tile with staggered wave
 *               groups (one workgroup per CU), 5 = the same kernel with 320x256 tiles, 0 = 128x128 generic kernel,
 *               6 / 7 = ring kernel (two workgroups per CU, 3-deep 32-k ring) with 128- / 160-row tiles (where it runs, N % 256 == 0
 *               and M >= 128, K may be any multiple of 32 from 64 on; every other kernel needs K % 64 == 0);
 *   tn_variant: wgrad (TN) GEMM: 3 = auto (default), 1 = 256x256 staggered kernel, 0 = 128x128;
 *   tn_split_target: workgroups the wgrad token split aims for (default 512);
 *   wgrad_group_chunks: token chunks per output tile of uvit_op_wgrad_group (0 = cost model, default);
 *   nt_group: 256x256 NT kernel: column tiles walked per row tile in the XCD-aware tile order (0 = default).
 *   nt_persist: 256x256 NT kernel with more tiles than CUs: 1 = one persistent workgroup per CU with the operand pipeline
 *               running across its tiles (default), 0 = one workgroup per tile. */
typedef struct uvit_tuning { int32_t nt_variant, tn_variant, tn_split_target, wgrad_group_chunks, nt_group, nt_persist; } uvit_tuning;
void uvit_tuning_default(uvit_tuning* out);
/* Replace the engine's tuning (values outside the lists above are refused with UVIT_ERR_ARG). */
int uvit_engine_set_tuning(uvit_engine* e, const uvit_tuning* t);
/* dual = 1 (default): teacher forward and the wgrad GEMMs run on an internal second HIP stream beside the
 * caller's stream; dual = 2: the same on a second stream of LOWER priority than the caller's (the critical chain of the
 * step gets free CUs first: faster with the whole GPU to itself, slower when other kernels -- RCCL -- hold CUs, so the
 * host mirror selects it for single-GPU runs only); dual = 0: everything on the caller's stream (used to time one
 * kernel in isolation).  Environment UVIT_SINGLE_STREAM=1 selects 0 at engine creation. */
int uvit_engine_set_streams(uvit_engine* e, int dual);
/* on = 1 (default): a training step of the base model runs every Block branch on the samples its DropPath KEPT (timm drop_path,
 * modeling_finetune.py:51-62: a dropped sample's branch is multiplied by 0 in the forward and receives no gradient), in compact rows
 * sized by the host from the same counter-based hash the device draws with; on = 0: every branch runs all samples and the dropped ones
 * are multiplied by 0, as the reference does.  Same results either way (bench.py reports both rates).  Environment UVIT_DP_ROWS=0
 * selects 0 at engine creation. */
int uvit_engine_set_drop_path_rows(uvit_engine* e, int on);
/* on = 0 (default): the LayerScale gradients of a training step come from the block's weight gradients,
 *   dgamma_j = (sum_k W_jk dW_jk + b_j db_j) / gamma_j        (W: the bf16 weight the forward multiplied by; see uvit_op_ls_dgamma)
 * so the student forward does not store the Block branches' pre-LayerScale outputs and backward does not read them back.  A gamma entry
 * that is exactly 0 makes the quotient 0 / 0: that entry's gradient is set to 0 and the engine's sticky `poisoned` flag is raised, so the
 * step (and every later one) leaves the weights untouched instead of training on a wrong gradient.  on = 1: the forward saves the branch
 * outputs and the LayerScale backward sums dgamma += e * y from them, which also serves gamma == 0.  Takes effect at the next
 * uvit_step_begin; every other gradient is computed by the same launches either way.  Environment UVIT_LS_SAVED_Y=1 selects 1 at engine
 * creation. */
int uvit_engine_set_ls_saved_y(uvit_engine* e, int on);
/* The host side of those lists, callable without a GPU: kept samples per (layer, draw) for one step -- out[draws_per_block * layer + k],
 * draws_per_block = 2 (base: attn, mlp) or 4 (two-stream: mean attn, mean mlp, cov attn, cov mlp) -- from the counter-based hash the device
 * draws its DropPath multipliers with (rates linspace(0, drop_path_rate, depth), modeling_cyclical.py:94-96).  Pure host arithmetic. */
int uvit_drop_path_kept_counts(int depth, float drop_path_rate, int draws_per_block, int batch, uint32_t seed, uint32_t it, int32_t* out);
/* Measurement aid for bench.py: bracket every launch of the dominant kernel (the fc1 GEMM with
 * fused bias+GELU, gemm_nt256_kernel<EPI_GELU / EPI_GELU_DG>) with HIP events on the stream it runs on.
 * profile_read: sum of the event-bracketed durations (ms), launch count, algorithmic FLOPs per launch. */
int uvit_engine_profile(uvit_engine* e, int enable, int max_launches);
int uvit_engine_profile_read(uvit_engine* e, double* total_ms, int* launches, double* flops_per_launch);
/* The brackets by kind: 0 = fc1 of the teacher (bias + GELU), 1 = fc1 of the student (also stores GELU'), 2 = attention proj and
 * 3 = fc2 (both: bias, LayerScale, DropPath, fp32 residual epilogue), -1 = kinds 0 and 1 together.  bytes_per_launch (nullable) =
 * the launch's algorithmic HBM bytes (operands read once, results written once).  Every launch of a kind is bracketed, compact ones
 * included (drop-path sample lists, the masked-row last block): FLOPs and bytes are those of the MEAN row count of the kind's launches. */
int uvit_engine_profile_read_kind(uvit_engine* e, int kind, double* total_ms, int* launches, double* flops_per_launch,
                                  double* bytes_per_launch);
/* enqueues the copy of 8 floats {loss, grad_norm, -, -, std_loss0 (the `loss_var0` meter), ...} of the last step into (pinned) host memory behind the step's kernels and returns:
 * the caller reads them after an event it records on `stream` has completed (engine_for_cyclical.py:164,186
 * sync twice per step instead).  A step whose loss or gradient norm is not finite leaves the weights untouched, and so
 * does every later step of that engine. */
int uvit_engine_read_stats_async(uvit_engine* e, float* host_out2, uvit_stream stream);
/* copies {loss, grad_norm} to host memory; synchronises the stream */
int uvit_engine_read_stats(uvit_engine* e, float* host_out2, uvit_stream stream);

/* ---- individual operators (tests, autograd wrappers) ---- */
typedef struct uvit_gemm_epilogue {
    void* out; void* out2; const float* bias; const float* bias2; const float* gamma; const float* resid;
    const float* rowscale; const void* aux; const int64_t* mask; const float* mask_token;
    int32_t ldo, tokens, patches;
    int32_t row0;   /* RESID: sample index of row m is (m + row0) / tokens */
} uvit_gemm_epilogue;
enum { UVIT_EPI_BF16 = 0, UVIT_EPI_QKV = 1, UVIT_EPI_GELU = 2, UVIT_EPI_RESID = 3, UVIT_EPI_F32 = 4,
       UVIT_EPI_PATCH = 5, UVIT_EPI_DGELU = 6, UVIT_EPI_QKV_ELU = 7,
       UVIT_EPI_GELU_DG = 8,   /* out = gelu(h), out2 = gelu'(h) (bf16), h = bf16(acc + bias): the training forward of Mlp.fc1 */
       UVIT_EPI_MULAUX = 9 };  /* out = bf16(acc * aux): GELU backward against the gelu'(h) stored by mode 8 */

/* C[M,N] = A[M,K] . W[N,K]^T with a fused epilogue: nn.Linear / F.linear sites of
 * modeling_finetune.py:75-82,151,186 and the Conv2d-as-GEMM at :317 */
int uvit_op_gemm_nt(int mode, const void* A_bf16, const void* W_bf16, int M, int N, int K, int lda, int ldw,
                    const uvit_gemm_epilogue* epi, uvit_stream stream);
/* The same with explicit tuning (NULL = defaults); *tail_rows (nullable, host) receives the number of rows the
 * launcher handed to its row-split tail launch (0 = single launch). */
int uvit_op_gemm_nt_tuned(int mode, const void* A_bf16, const void* W_bf16, int M, int N, int K, int lda, int ldw,
                          const uvit_gemm_epilogue* epi, const uvit_tuning* tune, int* tail_rows, uvit_stream stream);
/* What that call would launch on a device with num_cu compute units (num_cu <= 0: UVIT_ERR_ARG), and the same error codes for the
 * shapes and modes it refuses: host arithmetic only, no device is touched.  kernel: 0 = 128x128, 1 = 256-row, 2 = 256-row persistent,
 * 3 = 320-row, 4 = ring 128-row, 5 = ring 160-row; it runs the first `rows` rows on `grid` workgroups, and tail_rows more rows (0: none)
 * go to a second, 128x128 launch.  ldo = the epilogue's ldo; row_list != 0: the launch walks a row list (which never splits). */
typedef struct uvit_gemm_nt_plan_info { int32_t kernel, rows, grid, tail_rows; } uvit_gemm_nt_plan_info;
int uvit_op_gemm_nt_plan(int mode, int M, int N, int K, int lda, int ldw, int ldo, int row_list,
                         const uvit_tuning* tuning, int num_cu, uvit_gemm_nt_plan_info* out);
/* The same with DYNAMIC tile assignment for the persistent 256x256 kernel (round 4): tile_counters = 16 uint32 in device memory, zero
 * before the first launch (every launch leaves them zero again; launches that may run concurrently need their own 16).  The workgroups
 * then take tiles from per-XCD counters instead of by a fixed stride, so a launch that finds CUs occupied by other work (RCCL's channel
 * workgroups in a data-parallel run) takes tiles / free CUs longer instead of twice as long.  NULL = fixed stride. */
int uvit_op_gemm_nt_sched(int mode, const void* A_bf16, const void* W_bf16, int M, int N, int K, int lda, int ldw,
                          const uvit_gemm_epilogue* epi, const uvit_tuning* tune, uint32_t* tile_counters, uvit_stream stream);
/* C[N,K] (f32) = Y[M,N]^T . X[M,K]: weight gradients; M must be a multiple of 64.  tune: NULL = defaults */
int uvit_op_gemm_tn(const void* Y_bf16, const void* X_bf16, int M, int N, int K, int ldy, int ldx, float* C, int ldc,
                    const uvit_tuning* tune, uvit_stream stream);
/* All weight gradients of one layer's Linears in one launch (256x256 tiles, token-chunked, fp32 atomics into C).
 * Every problem: M % 64 == 0 and M >= 512, N % 256 == 0, K % 256 == 0; C (and the bias outputs) must hold zeros or a
 * value to add to.  bias (nullable) receives the column sums of Y[:, 0:bias_end) -- the Linear's bias gradient,
 * modeling_finetune.py:149-151 for the qkv split -- and bias2 (nullable) those of Y[:, bias2_begin:N); both bounds
 * are multiples of 256.  Returns UVIT_ERR_SHAPE (nothing launched) when a problem does not qualify. */
typedef struct uvit_wgrad_problem {
    const void* Y_bf16; const void* X_bf16; float* C; float* bias; float* bias2;
    int32_t bias_end, bias2_begin, M, N, K, ldy, ldx, ldc;
} uvit_wgrad_problem;
int uvit_op_wgrad_group(const uvit_wgrad_problem* problems, int count, const uvit_tuning* tune, uvit_stream stream);
/* Attention core, modeling_finetune.py:152-185. qkv (B,N,3,H,64) bf16; biasP (H,NP,NP) f32 or NULL in the kernels'
 * private layout built by uvit_op_relpos_gather: bias * log2(e), -1e30 in padded key columns; lse is in log2 units */
int uvit_op_attn_fwd(const void* qkv, const float* biasP, void* out, float* lse, int B, int H, int N, int NP,
                     float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream stream);
/* Backward of the same core (autograd of modeling_finetune.py:152-185), fused since round 3: dQ, dK, dV from ONE recomputation of
 * the probabilities; delta (B,H,N) = rowsum(dO o O) is an output; the score gradients leave the kernel once, as bf16, into
 * ds_workspace (uvit_op_attn_bwd_ws_bytes(B, H, N) bytes; only needed with dbias_slab) and a second kernel sums them over the
 * batch into dbias_slab = ONE (H, NP, NP) slab laid out [h][key][q] (accumulate_slab: add; NULL: no bias gradient). */
int64_t uvit_op_attn_bwd_ws_bytes(int B, int H, int N);
int uvit_op_attn_bwd(const void* qkv, const void* o_fwd, const void* d_o, const float* biasP, const float* lse,
                           float* delta, void* dqkv, float* dbias_slab, int accumulate_slab, void* ds_workspace, int B, int H,
                           int N, int NP, float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream stream);
/* The same two calls with an explicit head_dim: qkv (B,N,3,H,head_dim), out / d_o / o_fwd (B,N,H,head_dim).  head_dim 64 runs the
 * kernels of uvit_op_attn_fwd / uvit_op_attn_bwd; 80 (ViT-H) runs their head_dim-80 variants; anything else returns
 * UVIT_ERR_SHAPE.  The workspace size (uvit_op_attn_bwd_ws_bytes) does not depend on head_dim. */
int uvit_op_attn_fwd_hd(const void* qkv, const float* biasP, void* out, float* lse, int B, int H, int N, int NP, int head_dim,
                        float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream stream);
int uvit_op_attn_bwd_hd(const void* qkv, const void* o_fwd, const void* d_o, const float* biasP, const float* lse,
                        float* delta, void* dqkv, float* dbias_slab, int accumulate_slab, void* ds_workspace, int B, int H,
                        int N, int NP, int head_dim, float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream stream);
/* Two-stream Wasserstein attention core (modeling_finetune_dist.py:129-162 + uncertainty_evaluations.py:276-294).
 * qkv_m: mean-stream (B,N,3,H,64) bf16; qkv_c: covariance stream, already ELU(.)+1.  The backward returns the
 * gradient of the PRE-ELU covariance QKV (ELU' folded in).  biasP / lse units as for uvit_op_attn_fwd. */
int uvit_op_attn2_fwd(const void* qkv_m, const void* qkv_c, const float* biasP, void* out_m, void* out_c, float* lse, int B, int H,
                      int N, int NP, float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream stream);
/* Backward, fused since round 4 (one recomputation of P for all six gradients), same contract as uvit_op_attn_bwd: the score
 * gradients leave once, as bf16, into ds_workspace (uvit_op_attn2_bwd_ws_bytes(B, H, N) bytes; only needed with dbias_slab) and a
 * second kernel sums them over the batch into dbias_slab = ONE (H, NP, NP) slab laid out [h][key][q]. */
int64_t uvit_op_attn2_bwd_ws_bytes(int B, int H, int N);
int uvit_op_attn2_bwd(const void* qkv_m, const void* qkv_c, const void* o_m, const void* o_c, const void* d_m, const void* d_c,
                      const float* biasP, const float* lse, float* delta, void* dqkv_m, void* dqkv_c, float* dbias_slab,
                      int accumulate_slab, void* ds_workspace, int B, int H, int N, int NP, float scale, float p_drop, uint32_t seed,
                      uint32_t layer, uvit_stream stream);
int uvit_op_relpos_gather(const float* table, const int32_t* index, float* biasP, int H, int N, int NP, uvit_stream stream);
int uvit_op_relpos_scatter(const float* slab, int nslab, const int32_t* index, float* dtable, int H, int N, int NP,
                           uvit_stream stream);
/* nn.LayerNorm forward / backward (modeling_finetune.py:290-299) */
int uvit_op_ln_fwd(const float* x, const float* w, const float* b, void* y_bf16, float* mean, float* rstd, int M, int C,
                   float eps, uvit_stream stream);
int uvit_op_ln_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* w,
                   const float* dres, float* dx, float* dw, float* db, int M, int C, uvit_stream stream);
/* ---- the same row-wise kernels in every walk the engine launches them in (tests).  Each call fills the launcher's descriptor and
 * launches: nothing is allocated.  UVIT_ERR_ARG for a NULL mandatory pointer, before the device is touched; otherwise the launcher's
 * own codes (UVIT_ERR_SHAPE for a combination of fields it refuses).  Column sums (dw, db, dgamma, dbias, colsum) are ADDED into
 * nrep replicas of the accumulator, rep_stride floats apart (workgroup g adds into replica g % nrep): the caller zeroes them. ---- */
/* LayerNorm forward.  rows walk (pos == NULL): y / mean / rstd row r <- x row rowidx[r] (NULL: r); rows r >= *count (NULL: M) get a
 * zero y row and leave mean / rstd alone; mean / rstd may both be NULL.  samples walk (pos, xcopy, tokens; M % tokens == 0; no row
 * list): sample b's rows go to rows pos[b] * tokens + t of y / mean / rstd; a sample with pos[b] < 0 is copied to xcopy instead. */
int uvit_op_ln_fwd_walk(const float* x, const float* w, const float* b, void* y_bf16, float* mean, float* rstd, int M, int C,
                        float eps, const int32_t* rowidx, const int32_t* count, const int32_t* pos, float* xcopy, int tokens,
                        uvit_stream stream);
/* The LayerScale + DropPath backward of the branch behind a row-wise backward pass over the residual-stream gradient d
 * (modeling_finetune.py:295-298): e = d * rowscale[sample], dy = bf16(e * gamma), dgamma += e * y, dbias += dy (the stored bf16).
 * y = NULL together with dgamma = NULL (one without the other: UVIT_ERR_ARG): y is not read and dgamma is not summed
 * (uvit_op_ls_dgamma computes it from the weight gradient); dy and dbias are what the call with y gives, bit for bit.
 * tokens = rows per sample.  LayerNorm backward only: pos (sample -> compact slot of dy, -1 = dropped: writes nothing, adds nothing;
 * NULL = dense); cnt (samples walk: kept rows; the pad rows cnt .. roundup(pad_base + cnt, 64) - pad_base of dy are zero-filled, and the
 * same rows of pad2 [rows][pad2_cols], pad2_cols % 4 == 0). */
typedef struct uvit_ls_rider {
    const void* y; const float* gamma; const float* rowscale; void* dy; float* dgamma; float* dbias;
    int32_t tokens; const int32_t* pos; const int32_t* cnt; int32_t pad_base; void* pad2; int32_t pad2_cols;
} uvit_ls_rider;
/* LayerNorm backward with `next` (nullable) fused on dx.  rows walk: dy / mean / rstd row r belongs to residual-stream row rowidx[r]
 * (NULL: r; a row list needs count), where x, dres (nullable), dx and next->y live; rows r >= *count are skipped.  samples walk (pos, or
 * next->cnt, or next->pos without a row list; needs dres, next->tokens, M % tokens == 0): dy / mean / rstd compact by pos (NULL: all
 * kept); a dropped sample's rows get dx = dres and add nothing to dw / db. */
int uvit_op_ln_bwd_walk(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* w, const float* dres,
                        float* dx, float* dw, float* db, int M, int C, int nrep, int64_t rep_stride, const int32_t* rowidx,
                        const int32_t* count, const int32_t* pos, const uvit_ls_rider* next, uvit_stream stream);
/* The rider on its own over d = dx [.., C] (pos / cnt / pad* unused).  Row list: rider->dy is compact, row r reads dx / y / rowscale at
 * residual-stream row rowidx[r], rows r >= *count (up to M) get zeros. */
int uvit_op_ls_bwd(const float* dx, const uvit_ls_rider* rider, int M, int C, int nrep, int64_t rep_stride, const int32_t* rowidx,
                   const int32_t* count, uvit_stream stream);
/* LayerScale gradient from the weight gradient: dgamma[j] += sum over the nsets (1 or 2) sets of
 * (sum_k W[j][k] * dW[j][k] + b[j] * sum_r db[r * rep_stride + j]) / gamma[j],  j < C, k < K, r < nrep.
 * W (bf16) and dW (f32) are [C][K] row-major, K % 8 == 0, nrep <= 64 (UVIT_ERR_SHAPE otherwise).  fp32 accumulation, one wave per j, no
 * atomics.  gamma[j] == 0: dgamma[j] = 0 and *flag = 1 (flag is never cleared). */
typedef struct uvit_ls_dgamma_set { const void* W_bf16; const float* dW; const float* b; const float* db; } uvit_ls_dgamma_set;
int uvit_op_ls_dgamma(const uvit_ls_dgamma_set* sets, int nsets, const float* gamma, float* dgamma, int32_t* flag, int C, int K,
                      int nrep, int64_t rep_stride, uvit_stream stream);
/* out[c] += sum over the M rows of y[m][col0 + c], c < ncols (ld, col0, ncols multiples of 8) */
int uvit_op_colsum(const void* y_bf16, int ld, int col0, int ncols, int M, float* out, int nrep, int64_t rep_stride, uvit_stream stream);
/* out[i] += sum_r rep[r * stride + i], i < n (n, stride multiples of 4) */
int uvit_op_reduce_replicas(const float* rep, float* out, int64_t n, int nrep, int64_t stride, uvit_stream stream);
/* Drop-path sample lists from the multipliers scales [nlists][B] (0 = dropped): per list pos [B] (slot or -1), bmap [B] (slot -> sample,
 * 0 behind the kept ones), rows [rows_stride] (compact row -> residual-stream row, -1 on the pad rows up to the next multiple of 64,
 * nothing behind them), cnt[l] = kept rows, cnt[nlists + l] = 1 when the kept samples differ from host_counts[l] (HOST array). */
int uvit_op_droppath_lists(const float* scales, int32_t* pos, int32_t* bmap, int32_t* rows, int32_t* cnt, int nlists, int B, int tokens,
                           int rows_stride, const int32_t* host_counts, uvit_stream stream);
/* uvit_op_gemm_nt_tuned in mode UVIT_EPI_RESID (any other: UVIT_ERR_ARG) over a COMPACT row list: GEMM row m stands for residual-stream
 * row rowmap[m] -- resid is read and out / out2 are written there, rowscale is taken at rowmap[m] / tokens; rows m >= *rowcount write
 * nothing.  Such a launch never splits its rows. */
int uvit_op_gemm_nt_rows(int mode, const void* A_bf16, const void* W_bf16, int M, int N, int K, int lda, int ldw,
                         const uvit_gemm_epilogue* epi, const int32_t* rowmap, const int32_t* rowcount, const uvit_tuning* tune,
                         uvit_stream stream);
/* uvit_op_wgrad_group on stacked two-stream operands: split[i] (parallel to problems[i]; s1_row = 0: one stream) sends the column sums
 * of the rows from s1_row on to bias_s1 / bias2_s1.  s1_row % 64 == 0, M >= 1024, s1_row / 64 == (M / 64 + 1) / 2, and bias, bias_s1
 * (bias2_s1 with bias2) set; anything else returns UVIT_ERR_SHAPE. */
typedef struct uvit_wgrad_split { float* bias_s1; float* bias2_s1; int32_t s1_row; } uvit_wgrad_split;
int uvit_op_wgrad_group_split(const uvit_wgrad_problem* problems, const uvit_wgrad_split* split, int count, const uvit_tuning* tune,
                              uvit_stream stream);
/* token-assembly backward (modeling_cyclical.py:179-192) of dx (B, P + 1, C): dpatch (B, P, C) bf16 = dx[:, 1:] with the masked rows
 * zero (mask: int64 (B, P)), dcls [C] += sum_b dx[b, 0], dmask_token [C] += the sum of the masked rows */
int uvit_op_token_bwd(const float* dx, const int64_t* mask, void* dpatch_bf16, float* dcls, float* dmask_token, int B, int P, int C,
                      uvit_stream stream);
/* bf16 transposes in one launch: dst (cols, rows) = src (rows, cols)^T per descriptor; descs in DEVICE memory, tile0 = the first
 * 64 x 64 tile of the descriptor in the launch (ascending; total_tiles = their sum) */
typedef struct uvit_transpose_desc { const void* src; void* dst; int32_t rows, cols, tile0, pad; } uvit_transpose_desc;
int uvit_op_transpose_batch(const uvit_transpose_desc* descs_dev, int ndesc, int total_tiles, uvit_stream stream);
/* ModelEmaV2._update with the lambda of engine_for_cyclical.py:183 */
int uvit_op_ema(float* ema, const float* params, void* ema_bf16, int64_t n, float decay, uvit_stream stream);
int uvit_op_sumsq(const float* g, int64_t n, double* out, uvit_stream stream);
int uvit_op_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t n_decay, float lr,
                  float wd, float b1, float b2, float eps, int step, const double* sumsq, float max_norm,
                  float grad_scale, float* gnorm_out, uvit_stream stream);
/* F.smooth_l1_loss / F.mse_loss forward + gradient (engine_for_cyclical.py:147-150) */
int uvit_op_smooth_l1(const float* out, const float* target, const int32_t* count_dev, float beta, int l2,
                      float loss_scale, float* loss, void* dout_bf16, int Mmax, int C, uvit_stream stream);
/* WassersteinLoss forward + gradient (distloss.py:13-30, 73-79; engine_for_cyclical.py:152-161).  *loss += lam * loss_scale *
 * sum_r softplus(u_r) / max softplus(u); dout_m_bf16 (which already holds the SmoothL1 gradient) is ADDED to, dout_c_bf16 is
 * written.  scratch: 16 + Mmax floats.  Rows >= *count_dev are ignored (their dout_c rows are zeroed). */
int uvit_op_wasserstein_loss(const float* out_m, const float* out_c, const float* tgt_m, const float* tgt_c,
                             const int32_t* count_dev, float lam, float loss_scale, float* scratch, float* loss,
                             void* dout_m_bf16, void* dout_c_bf16, int Mmax, int C, uvit_stream stream);
/* target builder, engine_for_cyclical.py:92-122 */
int uvit_op_target_accum(const float* x, const int32_t* rowidx, const int32_t* count, float* acc, int first, int Mmax,
                         int C, float eps, uvit_stream stream);
/* variance term of the loss (engine_for_cyclical.py:130-139): z0_c = sqrt(var_r(out[r, c]) + 1e-6) over the *count_dev valid rows
 * (unbiased), std_loss0 = sum_c relu(margin - z0_c) / C.  *loss += w * loss_scale * std_loss0, *std_loss0_out = std_loss0, and
 * the gradient is ADDED to dout_bf16 (which already holds the regression gradient).  scratch: 2 * C + 16 floats. */
int uvit_op_variance_loss(const float* out, const int32_t* count_dev, float w, float margin, float loss_scale, float* scratch,
                          float* loss, float* std_loss0_out, void* dout_bf16, int Mmax, int C, uvit_stream stream);
int uvit_op_target_finalize(float* acc, const int32_t* count, int n_layers, int post_ln, int Mmax, int C, float eps,
                            uvit_stream stream);
int uvit_op_mask_compact(const int64_t* mask, int32_t* rowidx, int32_t* count, int B, int P, uvit_stream stream);
/* Synthetic batch built on the device (the loader contract of datasets.py:110-118 / engine_for_cyclical.py:45,58): images
 * (B, chans, S, S) f32 ~ N(0, 1); mask (B, patches) int64 with exactly n_mask ones per image.  Counter-based on (seed, it).
 * Either pointer may be NULL. */
int uvit_op_synth_batch(float* images, int64_t* mask, int B, int chans, int img_size, int patches, int n_mask, uint32_t seed,
                        uint32_t it, uvit_stream stream);
int uvit_op_im2col(const float* img, void* cols_bf16, int B, int Cin, int img_size, int patch, uvit_stream stream);
int uvit_op_droppath(float* scales, const float* rates_dev, int depth, int B, uint32_t seed, uint32_t step,
                     uvit_stream stream);
int uvit_op_cast_bf16(const float* src, void* dst_bf16, int64_t n, uvit_stream stream);

/* BEiT pre-training augmentation of a batch of decoded images (the reference's DataAugmentationForBEiT, datasets.py:31-117,
 * ImageFolder data sets): per sample, in this order and with Pillow's integer / float32 arithmetic bit for bit
 *   1. ColorJitter on the whole image: jitter_op[0..n_jitter) in order, each Image.blend(degenerate, img, factor) (Blend.c) with
 *      degenerate = black (brightness), the constant int(mean(L) + 0.5) of the image as it stands (contrast), per-pixel L
 *      (saturation); L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16;
 *   2. horizontal flip (flip = 1);
 *   3. crop (crop_x, crop_y, crop_w, crop_h) of the flipped image, resize to (resize_w, resize_h) with Resample.c's 8-bit separable
 *      resampler (taps clipped to the crop; a pass whose size is unchanged is skipped), evaluated on the S x S window at
 *      (win_x, win_y) of the resized image; window positions outside it are 0 (CenterCrop's padding);
 *   4. ToTensor + Normalize: ((u8 / 255) - mean[c]) / std[c] in float32 into out (B, 3, S, S).
 * pixels: ONE device buffer of pixel_bytes bytes holding every image as HWC uint8 RGB (rows of w * 3 bytes) at desc[b].offset.
 * desc: HOST memory (B entries), validated here and copied into the workspace by an asynchronous copy on `stream`: keep it
 * unchanged until the stream has passed this call (pinned memory, like any hipMemcpyAsync source).  mean / std: HOST, 3 floats.
 * workspace: uvit_op_augment_ws_bytes(desc, B, S) bytes (depends on the descriptors: filter taps and source rows).
 * Errors (nothing launched): UVIT_ERR_SHAPE for an image, crop, resize or window outside its bounds or an image that does not fit
 * in pixel_bytes; UVIT_ERR_ARG for a bad filter, flip or jitter entry (an op listed twice included); UVIT_ERR_WORKSPACE. */
#define UVIT_AUG_LANCZOS 1      /* filter ids = PIL.Image.Resampling */
#define UVIT_AUG_BILINEAR 2
#define UVIT_AUG_BICUBIC 3
#define UVIT_AUG_HAMMING 5
#define UVIT_AUG_BRIGHTNESS 0   /* jitter op ids = torchvision ColorJitter's fn_idx */
#define UVIT_AUG_CONTRAST 1
#define UVIT_AUG_SATURATION 2
typedef struct uvit_augment_desc {
    int64_t offset;                            /* byte offset of the image in `pixels` */
    int32_t h, w;                              /* decoded size */
    int32_t flip;
    int32_t crop_x, crop_y, crop_w, crop_h;    /* inside [0, w) x [0, h), in flipped coordinates */
    int32_t resize_w, resize_h;
    int32_t win_x, win_y;                      /* origin of the S x S output window in the resized image (may be negative) */
    int32_t filter;                            /* UVIT_AUG_{BILINEAR, BICUBIC, HAMMING, LANCZOS} */
    int32_t n_jitter;                          /* 0..3 */
    int32_t jitter_op[3];                      /* UVIT_AUG_{BRIGHTNESS, CONTRAST, SATURATION}, distinct */
    float jitter_factor[3];
    int32_t reserved;                          /* 0 */
} uvit_augment_desc;
int64_t uvit_op_augment_ws_bytes(const uvit_augment_desc* desc, int B, int S);   /* < 0: the UVIT_ERR_* of the batch call */
int uvit_op_augment_batch(const uint8_t* pixels, int64_t pixel_bytes, const uvit_augment_desc* desc, int B, int S, const float* mean,
                          const float* std, float* out, void* workspace, int64_t ws_bytes, uvit_stream stream);

/* ---- linear probe on the frozen encoder (run_class_finetuning.py --linear_classifier): everything behind the last block ----
 * All fp32, no float atomics (the same input gives the same bits on every run), no engine handle: x is the residual stream the
 * encoder left in its workspace, uvit_engine_ws_ptr(e, "x", depth).  Every call checks its arguments before it touches the device:
 * UVIT_ERR_ARG for a NULL pointer (or a smoothing outside [0, 1)), UVIT_ERR_SHAPE for a size outside the stated conditions. */
/* feat[b] (B, C) = LayerNorm without affine (eps) of the mean over tokens 1..N-1 of x[b] (B, N, C): `fc_norm(x[:, 1:].mean(1))`,
 * modeling_finetune.py:410-412,512-515.  C % 4 == 0, C <= 2048, N >= 2, B <= 65535 (both calls).  scratch: uvit_op_probe_pool_ws_bytes(B, N, C) bytes
 * (< 0: the UVIT_ERR_* of the call); partial column sums per (sample, token slice), added in slice order. */
int64_t uvit_op_probe_pool_ws_bytes(int B, int N, int C);
int uvit_op_probe_pool_norm(const float* x, float* feat, float* scratch, int B, int N, int C, float eps, uvit_stream stream);
/* logits (B, K) = feat (B, C) . W (K, C)^T + bias (K): the nn.Linear head, modeling_finetune.py:421,522.  K >= 1, C % 4 == 0. */
int uvit_op_probe_logits(const float* feat, const float* W, const float* bias, float* logits, int B, int K, int C, uvit_stream stream);
/* timm LabelSmoothingCrossEntropy (smoothing 0: nn.CrossEntropyLoss), run_class_finetuning.py:617-623, one wave per row:
 *   row_loss[b] = (1 - s) (lse - z_y) + s (lse - mean_k z_k);  *loss_out = mean_b row_loss[b], summed by one wave in row order;
 *   dlogits (nullable) = (softmax - (1 - s) onehot - s / K) / B, the gradient of *loss_out;
 *   top1_top5 (nullable, ACCUMULATED int32[2]): [0] += 1 when z_y is the strict row maximum, [1] += 1 when fewer than five logits
 *   are greater than z_y.
 * A label outside [0, K) makes row_loss[b], *loss_out and the row of dlogits NaN; nothing is read at that label. */
int uvit_op_probe_ce(const float* logits, const int64_t* labels, float smoothing, float* dlogits, float* row_loss, float* loss_out,
                     int32_t* top1_top5, int B, int K, uvit_stream stream);
/* dW (K, C) = dlogits (B, K)^T . feat (B, C), dbias (K) = column sums of dlogits.  Overwrites both; every element has one owner and
 * its sum runs over b in ascending order.  The head arena of the update is [W (K C) | bias (K, padded to 4)] with n_decay = K C for
 * uvit_op_adamw (head.weight decays, head.bias does not: optim_factory.py:58-97). */
int uvit_op_probe_head_grad(const float* dlogits, const float* feat, float* dW, float* dbias, int B, int K, int C, uvit_stream stream);

/* ---- calibration metrics of a classifier's batch (uncertainty_evaluations.py: ECELoss, TACELoss, NLL; AUROC one-vs-rest) ----
 * 1 <= B <= 1024, K >= 1, 1 <= n_bins <= 64.  Every call checks its arguments before it touches the device (UVIT_ERR_ARG for a NULL
 * pointer, UVIT_ERR_SHAPE for a size outside these limits, outputs untouched) and is asynchronous on `stream`.  No float atomics;
 * every floating sum has one owner and a fixed order, so the same input gives the same bits on every run.  probs is (B, K) fp32,
 * labels int64[B].  Comparisons widen the fp32 probability to double and compare with a double bound, so bin membership is what a
 * float64 restatement finds on the same fp32 values.  A label outside [0, K) makes ECE, NLL, TACE and the AUROC sum of the call NaN;
 * nothing is read at such a label. */
/* probs = softmax(logits) per row: fp32, max-shifted, one wave per row.  The only place where logits become probabilities. */
int uvit_op_calib_softmax(const float* logits, float* probs, int B, int K, uvit_stream stream);
/* Per row: row_conf[b] = max_k p, row_pred_correct[b] = the lowest index attaining it, row_pred_correct[B + b] = (pred == y),
 * row_nll[b] = -log(clamp(p_y / sum_k p_k, 2^-23, 1 - 2^-23)) (sum and quotient in double: Categorical(probs).log_prob).
 * bounds: HOST array double[n_bins + 1], the values of np.linspace(0, 1, n_bins + 1); it is read during the call and travels by value.
 * Bin i holds the rows with bounds[i] < conf <= bounds[i + 1] (a conf of exactly 0 falls in no bin).  bin_table = double[3 n_bins],
 * (prop, acc, conf) per bin with prop = count / B, zeros for an empty bin, each bin summed in row order.
 * positional_acc (0 or 1, else UVIT_ERR_ARG) chooses the bin accuracy, here and in uvit_op_calib_tace: 0 = the mean of the hit flag
 * a[b] (correct; [y_b == c] for TACE) over the rows of the bin; 1 = what the reference's compute_bins returns, whose
 * `accuracies[in_bin]` indexes rows 0 and 1 by position: (count a[1] + (B - count) a[0]) / B (a[1] := a[0] at B = 1, where the
 * reference cannot run).  The reference's published ECE / TACE are mode 1;
 * ece_nll[0] = sum_i prop_i |conf_i - acc_i| in bin order, ece_nll[1] = mean of row_nll in row order. */
int uvit_op_calib_confidence(const float* probs, const int64_t* labels, const double* bounds, int n_bins, int positional_acc, float* row_conf,
                             int32_t* row_pred_correct, double* row_nll, double* bin_table, double* ece_nll, int B, int K,
                             uvit_stream stream);
/* Thresholded adaptive calibration error.  Per class c: v_b = p[b, c] < threshold ? 0 : p[b, c]; sorted ascending; bin_n = B / n_bins
 * (integer; 0 when B < n_bins); lo_i = sorted[i bin_n], up_i = lo_{i+1}, up_last = 1.0; bin i holds the b with lo_i < v_b <= up_i;
 * per_class[c] (double[K]) = sum_i (count_i / B) |mean v - acc_i| in bin order, acc_i by positional_acc (see above); *tace = (sum_c per_class[c]) / K in class
 * order.  One workgroup per group of adjacent classes sorts its columns in LDS. */
int uvit_op_calib_tace(const float* probs, const int64_t* labels, double threshold, int n_bins, int positional_acc, double* per_class,
                       double* tace, int B, int K, uvit_stream stream);
/* One-vs-rest AUROC over the classes present in the batch.  rows = int32[3 B]: u2_i = sum over j with y_j != y_i of
 * 2 [p_i > p_j] + [p_i == p_j] in column y_i | n_pos_i = rows that carry y_i | first_i = no earlier row carries y_i.
 * out[0] = sum_i u2_i / (2 n_pos_i (B - n_pos_i)) over the samples whose class has a negative row, in sample order = sum_c AUC_c;
 * out[1] = the number of classes counted. */
int uvit_op_calib_auroc(const float* probs, const int64_t* labels, int32_t* rows, double* out, int B, int K, uvit_stream stream);

/* ---- stability under perturbation sequences (uncertainty_evaluations.py: p_evaluate, flip_prob, ranking_dist, dist) ----
 * 1 <= K <= 4096, 1 <= R <= 65535 * 256, 2 <= F <= 256, 1 <= V <= 65535.  Every call checks its arguments before it touches the
 * device (UVIT_ERR_ARG for a NULL pointer or a noise other than 0 / 1, UVIT_ERR_SHAPE for a size outside these limits, outputs
 * untouched) and is asynchronous on `stream`.  No atomics; every sum has one owner and a fixed order, so the same input gives the
 * same bits on every run. */
/* ranks (R, K) int32 = the ordinal ranks of logits (R, K) fp32, row by row: r[k] = 1 + #{j : z_j > z_k} + #{j < k : z_j == z_k},
 * i.e. rankdata(-z, method='ordinal'): rank 1 is the largest logit (the row's prediction: argmax, first index on ties), ties go to the
 * lower index, +0 == -0, +-inf order like any other value.  A row that holds a NaN gets the rank 0 for every class.  Each row is
 * sorted in LDS as 64-bit keys (order-preserving image of -z, class index) by a bitonic network over K padded to a power of two. */
int uvit_op_stability_ranks(const float* logits, int32_t* ranks, int R, int K, uvit_stream stream);
/* ranks (V F, K): the F frames of a sequence adjacent.  The reference frame of frame t >= 1 is frame t - 1 (noise = 0) or frame 0
 * (noise = 1).  With a = ranks of the reference frame and b = ranks of frame t, each of the F - 1 pairs gives
 *   flip = #{c : a[c] == 1 and b[c] != 1} (= [pred_ref != pred_t] on permutations),
 *   top5 = sum over c with a[c] <= 5 of |(a[c] - 1) - min(b[c] - 1, 5)|,   zipf = sum over c of |1 / a[c] - 1 / b[c]| / a[c].
 * seq (V, 3) double = {flip, top5, zipf} summed over the sequence's pairs (the caller divides by F - 1).  flip and top5 are summed
 * as integers; zipf is formed and summed in double, the classes of a pair one by one in ascending order, the pairs in frame order,
 * each sum by one owner.  A rank below 1 anywhere in a sequence (a NaN row) makes its three values NaN; nothing is indexed by a
 * rank. */
int uvit_op_stability_sequences(const int32_t* ranks, double* seq, int V, int F, int K, int noise, uvit_stream stream);

/* ---- random-feature Gaussian-process head on the frozen encoder: modeling_finetune.SNGP (:525-638), DESIGN.md section 9.3 ----
 * 1 <= B <= 65535, C % 4 == 0, 4 <= C <= 2048, D % 4 == 0, 4 <= D <= 2048, K >= 1.  fp32 unless stated otherwise.  Every call checks
 * its arguments before it touches the device (UVIT_ERR_ARG for a NULL pointer or a bad scalar, UVIT_ERR_SHAPE for a size outside these
 * limits, outputs untouched) and is asynchronous on `stream`.  No float atomics; every sum has one owner and a fixed order that does
 * not depend on the launch shape, so the same input gives the same bits on every run.  The output layer z = phi . W_out^T and its
 * gradient dW_out = dz^T phi are uvit_op_probe_logits (with a zero bias) and uvit_op_probe_head_grad on phi with C := D. */
/* ghat (B, C, nullable) = (feat - mean) * rstd per row (two-pass statistics, ln_eps >= 0 inside the root); g = ghat gamma + beta;
 * u (B, D, nullable) = g . W_rf (D, C)^T + b_rf (D), summed in tiles of 16 along C in ascending order; phi (B, D) = scale * cos(u).
 * The reference passes scale = gp_input_scale = 1 / sqrt(gp_kernel_scale) (:586-587); edward2 has sqrt(2 / D) there. */
int uvit_op_gp_features(const float* feat, const float* gamma, const float* beta, const float* W_rf, const float* b_rf, float scale,
                        float ln_eps, float* ghat, float* u, float* phi, int B, int C, int D, uvit_stream stream);
/* P (D, D), in place (:599-616).  S_ij = sum_b phi_bi phi_bj, one fma chain over b in ascending order.  momentum > 0:
 * P_ij <- fma(m, P_ij, om * (S_ij / B)) with m = (float)momentum and om = (float)(1 - momentum) (the reference's two Python
 * doubles, each rounded to fp32 on its own); momentum <= 0: P_ij <- P_ij + S_ij.  A symmetric P stays symmetric bit for bit.
 * momentum >= 1 or NaN: UVIT_ERR_ARG. */
int uvit_op_gp_precision_update(const float* phi, float* P, int B, int D, double momentum, uvit_stream stream);
/* Gradients of the LayerNorm's affine from dlogits (B, K), the gradient of the loss at z: du = -scale sin(u) * (dlogits . W_out (K, D)),
 * dg = du . W_rf (D, C), dgamma[c] = sum_b dg[b, c] ghat[b, c], dbeta[c] = sum_b dg[b, c], b in ascending order.  Three launches;
 * scratch holds du and dg: uvit_op_gp_ln_grad_ws_bytes(B, C, D) bytes (< 0: the UVIT_ERR_* of the call).  dgamma and dbeta (C) are
 * overwritten. */
int64_t uvit_op_gp_ln_grad_ws_bytes(int B, int C, int D);
int uvit_op_gp_ln_grad(const float* dlogits, const float* W_out, const float* u, const float* W_rf, const float* ghat, float scale,
                       float* dgamma, float* dbeta, float* scratch, int B, int K, int C, int D, uvit_stream stream);
/* var[b] (B, double) = ridge * phi_b^T Sigma phi_b, the diagonal of compute_predictive_covariance (:618-626).  Sigma (D, D) is DOUBLE
 * (the host's float64 inverse of P); phi is widened to double, products and sums are double in a fixed order.  ridge >= 0. */
int uvit_op_gp_variance(const float* phi, const double* Sigma, double ridge, double* var, int B, int D, uvit_stream stream);
/* out[b, k] = (float)(logits[b, k] / sqrt(1 + factor var[b])) formed in double: edward2's mean_field_logits, not part of the
 * reference.  factor >= 0; factor = 0 returns the logits bit for bit.  out may alias logits.  One wave per row. */
int uvit_op_gp_mean_field(const float* logits, const double* var, double factor, float* out, int B, int K, uvit_stream stream);

/* ---- heteroscedastic probe head on the frozen encoder: Monte-Carlo softmax with low-rank-plus-diagonal logit noise, the layer
 * modeling_finetune.MCSoftmaxDenseFA (:904-1217) describes (edward2's MCSoftmaxDenseFA, non-parameter-efficient form); DESIGN.md
 * section 9.4 ----
 * 1 <= B <= 65535, 1 <= S <= 65535 Monte-Carlo samples, 3 <= K <= 4096 classes, 1 <= R <= min(32, K) factors.  fp32.
 *   lin[b] (K (R + 2)) = [ loc (K) | draw (K) | V (K, R) row-major ], one uvit_op_probe_logits call with K := K (R + 2); d = draw + 1e-3
 *   u_s = loc + V . epsR_s + d * epsK_s;   y_s = softmax(u_s / T);   p = (1 / S) sum_s y_s,   s = 0 .. S-1
 * Noise: counter-based on the hash of common.h (uvit_hash32, written h below), regenerated by every kernel, never stored.  With
 * row = share ? 0 : b and stream t in {0: factors epsR, 1: diagonal epsK}: key_t = h(seed ^ ((t + 1) * 0x9E3779B9u)),
 * key = h((uint32_t)(row * S + s) ^ key_t); pair q: h1 = h((2 q) ^ key), h2 = h((2 q + 1) ^ key), u_i = ((h_i >> 9) + 0.5) * 2^-23 (exact
 * in fp32, inside (0, 1)), r = sqrt(-2 ln u1), n[2 q] = r cos(2 pi u2), n[2 q + 1] = r sin(2 pi u2); both values are used, |n| <= 5.8.
 * share = 1: the draws do not depend on the row (the reference's share_samples_across_batch), so a row's result does not depend on
 * its place in the batch.
 * Every call checks its arguments before it touches the device (UVIT_ERR_ARG for a NULL required pointer, a temperature that is
 * not a positive finite number, an eps outside [0, 1) or a share outside {0, 1}; UVIT_ERR_SHAPE for a size outside the limits; outputs
 * untouched) and is asynchronous on `stream`.  No float atomics: one wave handles one sample at a time, the samples of a row are split
 * into ceil(S / cs) <= 8 chunks of cs = 64 ceil(S / 512) samples (a function of S alone, not of the launch), each chunk is summed in
 * sample order and the chunk sums are added in chunk order by a second kernel, so the same input gives the same bits on every run. */
/* The draws themselves: epsR (B, S, R) and epsK (B, S, K); either may be NULL and is then left alone.  For tests and debugging: the
 * step never calls it. */
int uvit_op_het_noise(float* epsR, float* epsK, int B, int S, int K, int R, uint32_t seed, int share, uvit_stream stream);
/* scratch of both calls below: ceil(S / cs) * B * K * (R + 2) * 4 bytes, i.e. up to 8 x the size of lin (the backward's chunk sums of
 * dlin; the forward uses the first ceil(S / cs) * B * 2 K floats of it).  49 MB at B = 128, S = 1000, K = 1000, R = 10.  < 0: the
 * UVIT_ERR_* of the call. */
int64_t uvit_op_het_mc_ws_bytes(int B, int S, int K, int R);
/* p (B, K, required: the backward reads it) = the Monte-Carlo mean of the softmax; z (B, K, nullable) = log(clamp(p, eps, 1)), the
 * head's "logits"; pvar (B, K, nullable) = max((1 / S) sum_s y_s^2 - p^2, 0).  p holds the same bits whether or not z and pvar are asked for. */
int uvit_op_het_mc_forward(const float* lin, float* z, float* p, float* pvar, float* scratch, int B, int S, int K, int R,
                           float temperature, float eps, uint32_t seed, int share, uvit_stream stream);
/* dlin (B, K (R + 2)), overwritten, in the layout of lin, from dz (B, K), the gradient of the loss at z, and the forward's p:
 *   dp[k] = eps <= p[k] <= 1 ? dz[k] / p[k] : 0;   a_s = <y_s, dp>;   du_s = y_s * (dp - a_s) / (S T)
 *   dloc = sum_s du_s;   ddraw[k] = sum_s du_s[k] epsK_s[k];   dV[k, r] = sum_s du_s[k] epsR_s[r]
 * with the draws of the same (seed, share).  One uvit_op_probe_head_grad call on dlin then gives the gradients of the three layers. */
int uvit_op_het_mc_backward(const float* lin, const float* p, const float* dz, float* dlin, float* scratch, int B, int S, int K, int R,
                            float temperature, float eps, uint32_t seed, int share, uvit_stream stream);

/* ---- ensemble probe head on the frozen encoder: M linear heads behind one pooled feature vector, the deep ensemble the reference
 * evaluates with --ensembles (engine_for_finetuning.ensembles_evaluate, :225-343); DESIGN.md section 9.5 ----
 * B >= 1, K >= 1 classes, 1 <= M <= 16 members.  fp32 unless stated otherwise.  The head arena is [W (M K, C) | bias (M K) | pad to 4]
 * with n_decay = M K C, member m owning rows m K .. (m + 1) K - 1, so lin (B, M K) is one uvit_op_probe_logits call and the head
 * gradient one uvit_op_probe_head_grad call, both with K := M K.
 * Every call checks its arguments before it touches the device (UVIT_ERR_ARG for a NULL required pointer, a smoothing outside [0, 1)
 * or a mode outside {0, 1}; UVIT_ERR_SHAPE for B < 1, K < 1, M outside [1, 16] or C % 4 != 0; outputs untouched) and is asynchronous
 * on `stream`.  No float atomics; every floating sum has one owner and a fixed order that depends neither on the launch shape nor on
 * M, so the same input gives the same bits on every run and member m's outputs are those of an M = 1 call on its slice. */
/* w (B, M): the online-bagging weights (Oza & Russell), Poisson(1) per (row, member), counter-based on the hash of common.h (uvit_hash32, written h):
 * key = h(seed ^ 0x9E3779B9u), hh = h((uint32_t)(b M + m) ^ key), w[b, m] = #{n in 0..7 : (hh >> 9) >= T[n]} as a float in 0..8,
 * T = {3085997, 6171993, 7714992, 8229324, 8357907, 8383624, 8387910, 8388523} = ceil(2^23 e^-1 sum_{i <= n} 1 / i!): integer
 * comparisons, so a host restatement agrees exactly.  uvit_op_ens_ce takes the weights as an input; nothing is stored between steps. */
int uvit_op_ens_bag_weights(float* w, int B, int M, uint32_t seed, uvit_stream stream);
/* The members' smoothed cross-entropies, one wave per (row, member) with uvit_op_probe_ce's formulas on z = lin[b, m K : (m + 1) K]
 * (lse - v is formed as log(sum_k exp(z_k - max)) - (v - max), so the row maximum cancels exactly):
 *   row_loss[b, m] (B, M) = (1 - s)(lse - z_y) + s (lse - mean_k z_k), unweighted;
 *   loss_out (M + 1): loss_out[m] = (1 / B) sum_b w[b, m] row_loss[b, m], each member summed by one wave in row order, then
 *   loss_out[M] = their mean, added in member order;  weights (B, M, nullable): w = 1;
 *   dlin (B, M K, nullable) = w[b, m] (softmax(z)_k - (1 - s)[k == y] - s / K) / B, the gradient of sum_m loss_out[m]: every member
 *   receives exactly its own gradient;
 *   top1_top5 (nullable, ACCUMULATED int32 (M, 2)): uvit_op_probe_ce's two rules per member.
 * A label outside [0, K) makes that row's losses and gradients NaN for every member (and so every entry of loss_out); nothing is
 * read at that label and no counter moves. */
int uvit_op_ens_ce(const float* lin, const int64_t* labels, const float* weights, float smoothing, float* dlin, float* row_loss,
                   float* loss_out, int32_t* top1_top5, int B, int M, int K, uvit_stream stream);
/* Per-member gradient clip on the gradient arena [dW (M K, C) | dbias (M K) | pad]: member m's segments start at m K C and at
 * M K C + m K floats (the second is not 16-byte aligned in general; C % 4 == 0, C >= 4).  One workgroup per member sums the squares
 * of its K C weights and K biases in double (per-thread strided partial sums over quads of four adjacent elements, a fixed tree; the
 * same order whether or not grad is 16-byte aligned), norms[m] (M) = (float)sqrt of it, and
 * with max_norm > 0 multiplies the member's entries in place by fminf(max_norm / (norms[m] + 1e-6f), 1.0f) (uvit_op_adamw's
 * expression).  max_norm <= 0 only writes the norms.  A member whose sum is not finite is left as it is: uvit_op_adamw's guard then
 * skips the whole update. */
int uvit_op_ens_clip(float* grad, float* norms, int M, int K, int C, float max_norm, uvit_stream stream);
/* z (B, K) from lin (B, M K), one wave per row; lse_m = log-sum-exp of member m's logits, p_m[k] = expf(lin[b, m, k] - lse_m), the
 * difference formed as (lin[b, m, k] - max_m) - log(sum_k exp(lin[b, m, k] - max_m)):
 *   mode 0: z[k] = (sum_m lin[b, m, k]) / M, added in member order: torch.mean(torch.stack(outputs), 0), engine_for_finetuning.py:288-290;
 *   mode 1: z[k] = log((1 / M) sum_m p_m[k]) as a max-shifted log-sum-exp over m of lin[b, m, k] - lse_m, no clamp.
 * unc (B, 5, double, nullable), with pbar = (1 / M) sum_m p_m, k* = argmax z and k_m = argmax lin[b, m, :] (lowest index on ties):
 *   {total = -sum_k pbar log pbar, aleatoric = -(1 / M) sum_m sum_k p_m log p_m, mi = max(total - aleatoric, 0),
 *    var_pred = (1 / M) sum_m (p_m[k*] - pbar[k*])^2, disagreement = #{m : k_m != k*} / M}.
 * p_m is formed in fp32 and widened; every sum and logarithm of unc is double, 0 log 0 = 0.  A row that holds a NaN logit gives five
 * NaNs; z follows IEEE arithmetic.  z holds the same bits whether or not unc is asked for. */
int uvit_op_ens_combine(const float* lin, int mode, float* z, double* unc, int B, int M, int K, uvit_stream stream);

/* ---- set-level detection metrics of per-sample uncertainty scores: misclassification and out-of-distribution detection, DESIGN.md
 * section 9.6 ----
 * The store of an evaluation is S fp32 columns of ld elements each (column s starts at scores + s ld) and one uint8 flag per sample;
 * every column is oriented so that larger means more uncertain.  Every call checks its arguments before it touches the device
 * (UVIT_ERR_ARG for a NULL required pointer, UVIT_ERR_SHAPE for a size outside the stated limits, UVIT_ERR_WORKSPACE, outputs
 * untouched) and is asynchronous on `stream`.  No atomics; every sum has one owner and a fixed order, so the same input gives the
 * same bits on every run, and no workgroup waits for another. */
/* Per batch, one wave per row of logits z (B, K) fp32, B >= 1, K >= 1, 0 <= n0, n0 + B <= ld.  Writes at position n0 + b of columns
 * 0, 1, 2:  msp = 1 - max_k softmax(z)_k,  entropy = -sum_k p_k log p_k (0 log 0 = 0),  energy = -logsumexp(z); expf in fp32, the row
 * sums and everything behind them in double, rounded once to fp32.  flags[n0 + b] = 1 when the lowest index attaining max z differs
 * from labels[b], else 0; 2 for a label outside [0, K), and nothing is read at that label.  labels == NULL (images without labels):
 * no flag is written and flags may be NULL. */
int uvit_op_detect_rows(const float* logits, const int64_t* labels, float* scores, int64_t ld, int64_t n0, uint8_t* flags, int B, int K,
                        uvit_stream stream);
/* dst[b] = (float) src[b stride] for b < B: a head's own per-sample column (float, or double with src_is_double = 1; stride >= 1 in
 * elements) into a column of the store; the caller offsets both pointers. */
int uvit_op_detect_column(const void* src, int src_is_double, int64_t stride, float* dst, int B, uvit_stream stream);
/* Set level, 1 <= N <= 2^20 samples, 1 <= S <= 16 columns, ld >= N; ws: uvit_op_detect_ws_bytes(N, S) bytes (< 0: the UVIT_ERR_* of the
 * call), 16-byte aligned.  positive = flag 1.  Per column, a 64-bit key per sample: order-preserving image of the fp32 score << 32 |
 * sample index << 2 | [flag >= 2] << 1 | [flag == 1].  -0 ranks as +0.  A NaN score gets the image 0xFFFFFFFF: NaN rows sort behind
 * every number by index, are counted and take no part in the metrics.  The keys are sorted ascending by a bitonic network over N
 * padded to a power of two (all-ones padding): 4096-key chunks in LDS, one launch per compare-exchange distance >= 4096; the keys
 * are all different, so the sorted order (ties in score by ascending index) does not depend on the network.  An inclusive prefix
 * count of the positives in sorted order follows (three launches), then the metrics.  Tie groups are runs of equal image; walking
 * from the most uncertain end with TP_i, FP_i the cumulative positives and negatives at the end of group i, P and Nn the totals
 * over the n ranked samples:
 *   AUROC = sum_i (FP_i - FP_{i-1}) (TP_i + TP_{i-1}) / (2 P Nn)           int64 numerator, exact
 *   AUPR  = sum_i ((TP_i - TP_{i-1}) / P) TP_i / (TP_i + FP_i)             average precision, double
 *   FPR95 = FP_i / Nn at the first group with TP_i >= ceil(19 P / 20)       exact integers
 *   AURC  = (1 / n) sum_{k = 1..n} (positives among the k least uncertain) / k, in the ascending order of the keys, double
 * The double sums are formed per 4096 sorted positions (16 consecutive positions per thread in ascending order, a fixed tree over
 * the threads) and the segments are added in order by one thread.  out (S, 8) double = {AUROC, AUPR, FPR95, AURC, n, P, N - n, 0};
 * AUROC and FPR95 are NaN when P = 0 or Nn = 0, AUPR when P = 0, AURC when n = 0; a flag >= 2 anywhere among the N makes all four
 * NaN in every column.  order (S, N) int32, nullable: the sample indices in sorted order, the NaN rows last by index. */
int64_t uvit_op_detect_ws_bytes(int N, int S);
int uvit_op_detect_metrics(const float* scores, int64_t ld, const uint8_t* flags, int N, int S, int32_t* order, double* out, void* ws,
                           int64_t ws_bytes, uvit_stream stream);

/* ---- set-level calibration of an evaluation set: ECE / MCE / OE, NLL, Brier, SCE, ACE, TACE and per-class AUROC, DESIGN.md section
 * 9.19 ----
 * The store of an evaluation is row-major: row n of the fp32 probabilities starts at probs + n ld, ld >= K, beside one int64 label per
 * row.  Every call checks its arguments before it touches the device (UVIT_ERR_ARG for a NULL required pointer, a misaligned
 * workspace or a NaN threshold, UVIT_ERR_SHAPE for a size outside the stated limits, UVIT_ERR_WORKSPACE, outputs untouched), is
 * asynchronous on `stream` and never reads back.  No atomics; every sum has one owner and an order that depends on (N, K, the bin
 * counts) and the values alone -- not on ld, on timing or on the batches that filled the store -- so the same set gives the same bits.
 * All bin accuracies are the mean over the rows of the bin (the reading positional_acc = 0 of the per-batch ops). */
/* Per batch, one wave per row of logits z (N, K) fp32, N >= 1 (no upper limit), K >= 1: row n of softmax(z) to probs + n ld, with the
 * arithmetic of uvit_op_calib_softmax (the same bytes at ld == K).  The caller offsets `probs` to the batch's first row of the store. */
int uvit_op_scal_probs(const float* logits, float* probs, int64_t ld, int N, int K, uvit_stream stream);
/* Set level, 1 <= N <= 2^20 rows, 1 <= K, N K <= 2^30, every bin count in 1 .. 64.  ece_bounds / cw_bounds: host arrays of bins + 1
 * doubles (np.linspace(0, 1, bins + 1)); they travel by value.  Every comparison is the fp32 probability widened to double against a
 * double bound.
 * Per row: conf = max_k p_k, pred = the lowest index attaining it, correct = [pred == y], nll = -log(clamp(p_y / sum_k p_k, eps,
 * 1 - eps)) as uvit_op_calib_confidence, brier = sum_k (p_k - [k == y])^2 in double.
 * Top label, over ece_bins equal-width bins lo < conf <= up: top_table (ece_bins, 3) = (prop, acc, conf) per bin (zeros for an empty
 * bin); ECE = sum prop |conf - acc|, MCE = max |conf - acc|, OE = sum prop conf max(conf - acc, 0); NLL and Brier are row means.
 * Per class c, on the column p[:, c] with hit = [y == c]: SCE_c over cw_bins equal-width bins; ACE_c (threshold 0, ace_bins) and
 * TACE_c (tace_threshold, tace_bins) over adaptive bins -- values under the threshold become 0, the bounds are every (N / bins)-th
 * sorted value plus 1.0, bin i holds lo_i < v <= up_i with weight count / N; AUROC_c = P(p_pos > p_neg) + P(p_pos == p_neg) / 2
 * from int64 pair counts, NaN without a positive or without a negative row.
 * per_class (K, 6) = SCE_c, ACE_c, TACE_c, AUROC_c, n_pos, #{v >= tace_threshold}.
 * out[16] = ECE, MCE, OE, NLL, Brier, SCE, ACE, TACE (means over all K classes), mean AUROC_c over the classes that have one, how
 * many have one, accuracy, mean confidence, N, bad rows, 0, 0.  A row is bad when its label lies outside [0, K) (nothing is read at
 * it) or one of its probabilities is not finite; one bad row makes out[0 .. 11] NaN.  For the sort alone a value is clamped to
 * [0, 1], so no input makes a kernel index out of range.
 * One bitonic sort of 32-bit keys (value bits << 1 | hit) serves every per-class metric and, with the confidence column as column
 * K, the top-label bins: every bin is a contiguous run of a sorted column.  8192-key chunks in LDS, one launch per compare-exchange
 * distance >= 8192, every column of a group in the same launch.  ws: 16-byte aligned; uvit_op_scal_ws_bytes(N, K) (< 0: the
 * UVIT_ERR_* of the call) is 21 N bytes rounded up plus the keys of one group of columns, at most 2^26 keys = 256 MB, all K + 1
 * columns when they fit.  A smaller workspace is accepted down to one column of keys (uvit_op_scal_ws_bytes(N, 1) holds two): the
 * groups get smaller, the launches more, the results keep their bits.  uvit_op_scal_launches: the kernel launches of the call. */
int64_t uvit_op_scal_ws_bytes(int N, int K);
int64_t uvit_op_scal_launches(int N, int K, int64_t ws_bytes);
int uvit_op_scal_metrics(const float* probs, int64_t ld, const int64_t* labels, int N, int K, const double* ece_bounds, int ece_bins,
                         const double* cw_bounds, int cw_bins, int ace_bins, int tace_bins, double tace_threshold, double* out,
                         double* top_table, double* per_class, void* ws, int64_t ws_bytes, uvit_stream stream);

/* ---- post-hoc temperature scaling, fitted and applied on the device, DESIGN.md section 9.7 ----
 * s = 1 / T minimises f(s) = (1 / n) sum_i [ log sum_k exp(s z_ik) - s z_i,y_i ], the mean NLL of softmax(z / T), over
 * [1 / t_max, 1 / t_min]; g = f' = (1 / n) sum_i [ sum_k p_ik z_ik - z_i,y_i ] is non-decreasing and h = f'' = (1 / n) sum_i Var_p_i[z_i].
 * Every call checks its arguments before it touches the device (UVIT_ERR_ARG for a NULL required pointer or a misaligned workspace,
 * UVIT_ERR_SHAPE for a size or a setting outside the stated limits, UVIT_ERR_WORKSPACE, outputs untouched) and is asynchronous on
 * `stream`.  No atomics; every sum has one owner and a fixed order that depends on N and K alone, so the same input gives the same
 * bits on every run and for every ld; no workgroup waits for another and nothing is read back to the host. */
/* Workspace of uvit_op_ts_fit in bytes; UVIT_ERR_SHAPE unless 1 <= N <= 2^20 and K >= 2. */
int64_t uvit_op_ts_ws_bytes(int N, int K);
/* logits (N, ld >= K) fp32, labels (N) int64, out: 8 doubles on the device, ws: uvit_op_ts_ws_bytes(N, K) bytes, 16-byte aligned.
 * UVIT_ERR_SHAPE also for t_min <= 0, t_max <= t_min or not finite, tol <= 0, max_iter outside [1, 64].
 * A row pass: one wave per row, 16 rows per workgroup; m = max_k z_k, d_k = z_k - m in fp32, e_k = expf((float)(s (double) d_k)), then
 * double: S = sum e_k, T1 = sum e_k d_k, T2 = sum e_k d_k^2 (lane partial sums over ascending k, the xor tree), row values
 * log S - s d_y, T1 / S - d_y, T2 / S - (T1 / S)^2 with d_y = z_y - m formed in fp32; a workgroup adds its rows in ascending order and
 * writes one partial per quantity, one workgroup adds the partials in a fixed order and takes the step.
 * Pass 1 evaluates s_max = 1 / t_min, s_min = 1 / t_max, s_0 = 1 clamped to [s_min, s_max], and 1 in one read.  g(s_max) <= 0: the
 * result is s_max, status 2; g(s_min) >= 0: s_min, status 1.  Otherwise a bracketed Newton from s_0: the pass at s moves the bracket
 * [lo, hi] by the sign of g(s); the candidate s - g / h is replaced by sqrt(lo hi) when h is not positive and finite or the candidate
 * is not inside (lo, hi); status 0 when |candidate - s| <= tol s or g == 0, status 3 after max_iter passes.  The result is the last
 * point evaluated.  2 max_iter launches are enqueued up front; those behind the end read the device state and return at once.
 * out = {T = 1 / s clamped to [max(t_min, 1 / s_max), min(t_max, 1 / s_min)], s, NLL at s = 1, NLL at the result, g at the result,
 * passes used, status, rows left out}.  A label outside [0, K) makes all eight NaN and nothing is read at that label.  A row with a
 * non-finite logit is left out and counted; when no row remains T, s, the NLLs and g are NaN (passes 1, status 0). */
int uvit_op_ts_fit(const float* logits, int64_t ld, const int64_t* labels, int N, int K, double t_min, double t_max, double tol,
                   int max_iter, double* out, void* ws, int64_t ws_bytes, uvit_stream stream);
/* dst[b, k] = (float)((double) src[b, k] * s) for b < B, k < K, with s = table[1] read on the device (the table of uvit_op_ts_fit, or
 * any 8 doubles); ld_src, ld_dst >= K; dst == src is allowed.  A NaN s gives NaN logits; s > 0 is a monotone map, ranks are kept. */
int uvit_op_ts_scale(const float* src, float* dst, int64_t ld_src, int64_t ld_dst, const double* table, int B, int K, uvit_stream stream);

/* ---- split conformal prediction sets, calibrated and evaluated on the device, DESIGN.md section 9.8 ----
 * Per row: m = max_k z_k, e_k = expf(z_k - m) in fp32, S = sum_k e_k in double, o_j = 1 + #{i : z_i > z_j} + #{i < j : z_i == z_j} (the
 * ordinal rank by descending softmax, ties to the smaller index), and with a per-row u in [0, 1] (u == NULL: 1)
 *   kind 0 (lac):  s_j = 1 - e_j / S
 *   kind 1 (aps):  s_j = (sum_{i : o_i < o_j} e_i + u e_j) / S        kind 2 (raps): the same + lam * max(0, o_j - kreg)
 * lam and kreg are read for kind 2 only.  Limits: 1 <= N, B <= 2^20 rows, 2 <= K <= 4096 classes, 1 <= A <= 8 levels, ld >= K.  Every
 * call checks its arguments before it touches the device (UVIT_ERR_ARG for a NULL required pointer or a misaligned workspace,
 * UVIT_ERR_SHAPE for a size, a kind, a negative or non-finite lam, a negative kreg or an alpha outside (0, 1), UVIT_ERR_WORKSPACE;
 * outputs untouched) and is asynchronous on `stream`; nothing is read back to the host.  Every double sum has a fixed order that
 * depends on K alone; the only atomics add integers, which is exact: the same input gives the same bits on every run. */
/* scores (N) double = s_y of each row, one wave per row.  A row with a non-finite logit gets a NaN; a label outside [0, K) gets the
 * NaN 0x7FF8000000000BAD, nothing is read at it, and uvit_op_cp_quantile turns its table to NaN. */
int uvit_op_cp_scores(const float* logits, int64_t ld, const int64_t* labels, const float* u, int N, int K, int kind, double lam, int kreg,
                      double* scores, uvit_stream stream);
/* Workspace of uvit_op_cp_quantile in bytes; UVIT_ERR_SHAPE outside the limits. */
int64_t uvit_op_cp_ws_bytes(int N, int A);
/* scores (N) double on the device, non-negative or NaN; alphas: A doubles ON THE HOST, each in (0, 1); table (A, 16) double on the
 * device; ws 16-byte aligned.  With n the number of non-NaN scores and k_a = ceil((n + 1) (1 - alpha_a)) (the product and the ceiling
 * in double), q_a is the k_a-th smallest score, found by a radix select on the bit patterns, eight bits per pass: q_a is one of the
 * input scores bit for bit.  k_a > n: q_a = +inf, status 1.  Row a of the table = {alpha, q, k, n, N - n, status (0 finite, 1 +inf),
 * then ten slots that uvit_op_cp_finish fills (0 here)}.  A bad-label score anywhere makes all 16 slots of every row NaN. */
int uvit_op_cp_quantile(const double* scores, int N, const double* alphas, int A, double* table, void* ws, int64_t ws_bytes,
                        uvit_stream stream);
/* Number of int64 counters of uvit_op_cp_sets: 4 + 20 A + K (A + 1); UVIT_ERR_SHAPE outside the limits.  Layout: rows used | rows
 * skipped (a non-finite logit) | bad labels | 0; per level {covered, size sum, empty sets, singletons, largest set, rows of the 7
 * size bins [0,1] [2,3] [4,6] [7,10] [11,100] [101,1000] [1001,inf), covered rows of the 7 bins, 0}; rows per class (K); covered rows
 * per level and class (A, K).  The caller zeroes them once; calls over consecutive batches add up to the call over their concatenation. */
int64_t uvit_op_cp_counter_count(int K, int A);
/* One evaluation batch against the q of `table` (A, 16): per row and level size = #{j : s_j <= q_a} and covered = [s_y <= q_a], s_y
 * by the very function uvit_op_cp_scores uses.  One workgroup per row; kinds 1 and 2 sort the row in LDS as 64-bit keys (image of
 * -z, class index) by a bitonic network over K padded to a power of two and take a double prefix sum in rank order.  sizes (A, ld_out)
 * int32 and covered (A, ld_out) uint8 are optional (ld_out >= B); a skipped row gets size -1 and covered 0 there.  Rows with a
 * non-finite logit or a bad label are counted and take part in nothing else. */
int uvit_op_cp_sets(const float* logits, int64_t ld, const int64_t* labels, const float* u, int B, int K, int kind, double lam, int kreg,
                    const double* table, int A, int64_t* counters, int32_t* sizes, uint8_t* covered, int64_t ld_out, uvit_stream stream);
/* Slots 6 .. 15 of every table row from the counters: coverage, mean size, share of empty sets, share of singletons, largest set,
 * SSCV = max over the non-empty size bins of |coverage in the bin - (1 - alpha)|, worst-class coverage = min over the classes with a
 * row of covered_c / rows_c, rows used, rows skipped, 0.  The seven metrics are NaN when no row was used, a label was bad or q is NaN. */
int uvit_op_cp_finish(const int64_t* counters, double* table, int K, int A, uvit_stream stream);

/* ---- post-hoc last-layer K-FAC Laplace approximation of the linear head, DESIGN.md section 9.9 ----
 * f (B, C) is the probe's pooled, normalised feature, phi = [f, 1] has D = C + 1 entries, z = W f + b are the head's logits and
 * p = softmax(z).  Over the rows of a labelled set: A = sum phi phi^T (D, D), G = (1 / n) sum (diag(p) - p p^T) (K, K), and the
 * posterior precision of the head's K D parameters is G (x) A + tau I.  With the host's A = U_A diag(lam_A) U_A^T and
 * G = U_G diag(lam_G) U_G^T the variance of logit k at phi is var_k = sum_i a_i^2 T[i, k], a = U_A^T phi,
 * T[i, k] = sum_j U_G[k, j]^2 / (lam_A[i] lam_G[j] + tau).
 * Limits: C % 4 == 0, 4 <= C <= 2048, 2 <= K <= 4096, 1 <= B <= 65535, ld >= K.  Every call checks its arguments before it touches
 * the device (UVIT_ERR_ARG for a NULL required pointer, a pointer that is not aligned to its element -- a workspace: to 16 bytes --
 * or a bad scalar, UVIT_ERR_SHAPE for a size outside these limits, UVIT_ERR_WORKSPACE; outputs untouched) and is asynchronous on
 * `stream`.  All arithmetic is double on fp32 inputs widened.  No atomics; every sum has one owner and a fixed order, so the same
 * input gives the same bits on every run. */
/* Workspace of uvit_op_lap_factors in bytes: the softmax (B, K) double, a double and an int32 per row. */
int64_t uvit_op_lap_factors_ws_bytes(int B, int C, int K);
/* One batch added in place into A (D, D), G_sum (K, K) (NOT divided by n: the host divides) and sums = {nll = -sum log p[y], rows
 * used, rows skipped}, all double and zeroed once by the caller.  feat (B, C) fp32, logits (B, ld) fp32, labels (B) int64.  A first
 * launch writes the max-shifted softmax to ws (lane partial sums over ascending k, the xor tree); then every element of A is one fma
 * chain over b in ascending order, every element of G_sum is delta_kl sum_b p_bk minus such a chain of p_bk p_bl, and both are added
 * to the old value; (i, j) and (j, i) come from the same products in the same order: symmetric inputs stay symmetric bit for bit.
 * A row with a non-finite logit or a label outside [0, K) is left out of everything and counted as skipped. */
int uvit_op_lap_factors(const float* feat, const float* logits, int64_t ld, const int64_t* labels, double* A, double* G, double* sums,
                        void* ws, int64_t ws_bytes, int B, int C, int K, uvit_stream stream);
/* T (D, K) double from UG (K, K; column j the j-th eigenvector), lamA (D) and lamG (K), all double: j in ascending order, one owner
 * per element.  Once per fit and tau; tau must be positive and finite (UVIT_ERR_ARG). */
int uvit_op_lap_prepare(const double* UG, const double* lamA, const double* lamG, double tau, double* T, int C, int K, uvit_stream stream);
/* Workspace of uvit_op_lap_variance in bytes: the squares a^2 (B, D) double. */
int64_t uvit_op_lap_variance_ws_bytes(int B, int C, int K);
/* var (B, K) double = (phi UA)^2 T with UA (D, D; column i the i-th eigenvector) and T (D, K) double: two launches of 16 x 32 output
 * tiles, every element one fma chain over the reduction index in ascending order; a^2 is rounded once, into ws. */
int uvit_op_lap_variance(const float* feat, const double* UA, const double* T, double* var, void* ws, int64_t ws_bytes, int B, int C, int K,
                         uvit_stream stream);
/* The probit link: out[b, k] = (float)((double) logits[b, k] / sqrt(1 + factor var[b, k])), rounded once; ld, ld_out >= K; out may
 * alias logits; factor >= 0 and finite, factor = 0 returns the logits bit for bit (pi / 8 is the literature's value).  A NaN or
 * negative var gives NaN in that entry alone.  lap_var (B) fp32, nullable: var[b, argmax_k logits[b, k]], the arg-max over the
 * unscaled logits with the lowest index on ties (NaN logits never win; index 0 when all are NaN).  One wave per row. */
int uvit_op_lap_probit(const float* logits, int64_t ld, const double* var, double factor, float* out, int64_t ld_out, float* lap_var,
                       int B, int K, uvit_stream stream);

/* ---- probe of the two-stream (mean, covariance) model, DESIGN.md section 9.17 ----
 * m (B, C) and c (B, C) are the pooled, normalised features of the mean and the covariance stream.  v = scale (ELU(c) + 1) =
 * scale (c > 0 ? c + 1 : exp(c)) is read as the variance of a feature f ~ N(m, diag(v)); the linear head z = W f + b carries it to
 * z ~ N(W m + b, W diag(v) W^T), of which the diagonal var[b, k] = sum_c W[k, c]^2 v[b, c] is built.  The link on var is
 * uvit_op_lap_probit above.  Limits: C % 4 == 0, 4 <= C <= 2048, 1 <= B <= 65535, N >= 2, 1 <= K <= 65535.  Every call checks its
 * arguments before it touches the device (UVIT_ERR_ARG for a NULL required pointer or a bad scalar, UVIT_ERR_SHAPE for a size outside
 * these limits; outputs untouched) and is asynchronous on `stream`.  No atomics; every sum has one owner and a fixed order, so the
 * same input gives the same bits on every run. */
/* Workspace of uvit_op_dprobe_pool_norm in bytes: twice uvit_op_probe_pool_ws_bytes(B, N, C) (< 0: the UVIT_ERR_* of the call). */
int64_t uvit_op_dprobe_pool_ws_bytes(int B, int N, int C);
/* uvit_op_probe_pool_norm of two residual streams (B, N, C) in one launch pair, the stream index on a grid dimension: feat_mean from
 * x_mean and feat_cov from x_cov, each bit for bit what uvit_op_probe_pool_norm gives on that stream alone (the same 8 token slices,
 * the same 4 waves, the same order of every sum).  The two inputs, and the two outputs, are independent pointers. */
int uvit_op_dprobe_pool_norm(const float* x_mean, const float* x_cov, float* feat_mean, float* feat_cov, float* scratch, int B, int N, int C,
                             float eps, uvit_stream stream);
/* var (B, K) double and trace (B) fp32, nullable, from cfeat = c (B, C) fp32 and the head's weights W (K, C) fp32.  v is formed in
 * double from the fp32 c, (double) w * (double) w is exact, and every var[b, k] is one fma chain over c in ascending order (16 x 32
 * output tiles, as uvit_op_lap_variance).  trace[b] = (float)(sum_c v[b, c] / C): lane l of one wave adds columns l, l + 64, ... in
 * ascending order, the lanes meet in the xor tree, the quotient is rounded once.  A NaN in cfeat[b] makes row b of var and trace[b]
 * NaN and touches no other row.  scale must be finite and greater than 0 (UVIT_ERR_ARG). */
int uvit_op_dprobe_variance(const float* cfeat, const float* W, double scale, double* var, float* trace, int B, int K, int C,
                            uvit_stream stream);

/* ---- Mahalanobis and relative Mahalanobis out-of-distribution scores of the probe's feature, DESIGN.md section 9.10 ----
 * f (B, C) is the probe's pooled, normalised feature.  Over the usable rows of a labelled set (every feature finite, the label inside
 * [0, K)): S = sum f f^T (C, C), class_sum[k] = the sum of the rows of class k (K, C), total_sum (C), class_count (K).  From these the
 * host forms the class means mu_k, the overall mean mu_0, the tied covariance Sigma = (S - sum_k n_k mu_k mu_k^T) / n and the
 * background covariance Sigma_0 = S / n - mu_0 mu_0^T, shrinks both (+ rho tr / C I), factors them (L L^T, L_0 L_0^T) and uploads
 * W = L^-1, W0 = L_0^-1, Wmu[k] = W mu_k and Wmu0 = W0 mu_0.  Then d_k(f) = |W f - Wmu[k]|^2, maha = min_k d_k over the classes with
 * a row, pred = arg min (the lowest index on ties), d_0 = |W0 f - Wmu0|^2 and rmaha = maha - d_0; larger = more out of distribution.
 * Limits, argument checks, double arithmetic and the fixed order of every sum are those of the Laplace ops above. */
/* Workspace of uvit_op_maha_accumulate in bytes: an int32 per row, padded to 16 bytes. */
int64_t uvit_op_maha_accumulate_ws_bytes(int B, int C, int K);
/* One batch added in place into S (C, C), class_sum (K, C), total_sum (C), class_count (K) and sums = {rows used, rows skipped}, all
 * double and zeroed once by the caller.  feat (B, C) fp32, labels (B) int64.  Every element of S is one fma chain over b in ascending
 * order added to the old value, (i, j) and (j, i) from the same products in the same order: S stays symmetric bit for bit.  Every
 * element of class_sum and total_sum has one owner that walks b in ascending order (K + 1 rows of workgroups read the B screened
 * labels each).  A row with a non-finite feature or a label outside [0, K) is left out of everything and counted as skipped. */
int uvit_op_maha_accumulate(const float* feat, const int64_t* labels, double* S, double* class_sum, double* total_sum, double* class_count,
                            double* sums, void* ws, int64_t ws_bytes, int B, int C, int K, uvit_stream stream);
/* Workspace of uvit_op_maha_scores in bytes: W f and W0 f (B, C) double each and the distances (B, K) double. */
int64_t uvit_op_maha_scores_ws_bytes(int B, int C, int K);
/* maha (B) fp32, rmaha (B) fp32 and pred (B) int32 of feat (B, C) fp32 from W, W0 (C, C) double, row-major and lower triangular with
 * exact zeros above the diagonal, Wmu (K, C), Wmu0 (C) and class_count (K) double.  The whitened rows go to ws (16 x 32 output tiles,
 * every element one fma chain over ascending column index); every d_k is the sum of the squared differences (g_c - Wmu[k, c])^2 in
 * ascending c, never the expanded form; the minimum skips the classes with class_count <= 0 (none left: NaN, NaN, -1) and takes the
 * lowest index on ties; the fp32 outputs are rounded once.  dist (B, ld) double, nullable, ld >= K: every d_k, the padding untouched;
 * NULL gives the same maha, rmaha and pred bits.  A row with a non-finite feature gets NaN, NaN, -1 and NaN in its row of dist.
 * labels (B) int64 and correct (1) int32, both nullable: *correct += the rows whose pred equals their label (an integer atomic). */
int uvit_op_maha_scores(const float* feat, const double* W, const double* W0, const double* Wmu, const double* Wmu0,
                        const double* class_count, float* maha, float* rmaha, int32_t* pred, double* dist, int64_t ld,
                        const int64_t* labels, int32_t* correct, void* ws, int64_t ws_bytes, int B, int C, int K, uvit_stream stream);

/* ---- k-nearest-neighbour OOD score and k-NN classifier of the probe's feature (csrc/knn.hip) ----
 * Deep nearest neighbours (Sun et al., ICML 2022): features are scaled to unit length, the score of a test feature is its distance to
 * the k-th nearest training feature, knn = |q - b_(k)|^2 = 2 - 2 s_k with s the dot product; larger = more out of distribution.  The
 * same neighbours give the weighted k-NN classifier of DINO / iBOT: votes_c = sum_j exp((s_j - s_1) / T) [label_j == c].
 * Arguments are checked before anything touches the device, nothing synchronises with the host, a second run gives the same bits. */
/* feat (B, C) fp32 -> out (B, C) bf16 unit rows, written at the pointer given (bank + row0 * C appends to a bank; 16-byte aligned) and
 * out_labels (B) int32.  |f|^2 is summed in double; an element is (float)(f_c * (1 / sqrt(|f|^2))) rounded to bf16, nearest even.
 * labels (B) int64, nullable: a usable row gets its label (0 without labels).  A row with a non-finite element, a zero norm or a label
 * outside [0, K) becomes a zero row with out_labels = -1.  sums (2) double, nullable: {rows used, rows skipped} added in place.
 * C % 32 == 0, 32 <= C <= 2048, 1 <= B <= 2^22; K (2 .. 4096) is read with labels only. */
int uvit_op_knn_rows(const float* feat, const int64_t* labels, void* out, int32_t* out_labels, double* sums, int B, int C, int K,
                     uvit_stream stream);
/* Workspace of uvit_op_knn_search in bytes: the slabs' running lists, (B, slabs, k) 64-bit keys; O(B slabs k), never (B, N). */
int64_t uvit_op_knn_search_ws_bytes(int B, int C, int N, int k, int slabs);
/* query (B, C) bf16 and query_valid (B) int32 (both from uvit_op_knn_rows; valid = not negative), bank (N, C) bf16, bank_labels (N)
 * int32 -> sim (B, ld) fp32 and idx (B, ld) int32, ld >= k, the padding untouched: per query row the k bank rows with the largest
 * dot product among those with bank_labels >= 0, sorted by (similarity descending, index ascending); fewer than k such rows leave
 * -inf and -1 behind them; an invalid query row gets NaN and -1 throughout.  The products are v_mfma_f32_16x16x32_bf16 with fp32
 * accumulation, one chain over C in ascending 32-element steps for every output element; -0 is reported as +0.  The bank is split into
 * `slabs` contiguous row ranges (0: chosen from N, B and the CU count; 1 .. 1024), a workgroup streams one slab for 64 query rows and
 * keeps a running top-k per row, a second kernel merges.  The order is total (64-bit key: the similarity's bits, then the inverted
 * index), so the result has the same bits for every `slabs` and on every run.  1 <= B <= 65535, 1 <= k <= 256, 1 <= N <= 2^22. */
int uvit_op_knn_search(const void* query, const int32_t* query_valid, const void* bank, const int32_t* bank_labels, float* sim,
                       int32_t* idx, int64_t ld, void* ws, int64_t ws_bytes, int B, int C, int N, int k, int slabs, uvit_stream stream);
/* From sim, idx (B, ld) of uvit_op_knn_search and bank_labels (N): knn (B) fp32 = fmaf(-2, s_k, 2); pred (B) int32 = the arg max over
 * classes of votes_c (double, j ascending, the lowest class on ties; a neighbour whose label is outside [0, K) does not vote);
 * votes (B, ldv) double, nullable, ldv >= K (NULL gives the same knn and pred bits).  A row whose k-th entry is missing or NaN gets
 * knn = NaN, pred = -1 (and NaN votes).  labels (B) int64 and correct (1) int32, both nullable: *correct += the rows whose pred equals
 * their label (an integer atomic).  2 <= K <= 4096, temperature positive and finite, B, k, N as above. */
int uvit_op_knn_scores(const float* sim, const int32_t* idx, int64_t ld, const int32_t* bank_labels, int N, float* knn, int32_t* pred,
                       double* votes, int64_t ldv, const int64_t* labels, int32_t* correct, int B, int k, int K, double temperature,
                       uvit_stream stream);

/* ---- ViM and residual OOD scores of the probe's feature (csrc/vim.hip) ----
 * Virtual-logit matching (Wang et al., CVPR 2022) for a frozen encoder with an affine head z = W f + b.  With o = -pinv(W) b, the
 * rows of R (Cn, C) an orthonormal basis of the Cn = C - D smallest principal directions of the training features centred at o:
 * residual = |R (f - o)|, vim = alpha residual - logsumexp(z), pred = arg max z; larger = more out of distribution.  The host stacks
 * A = [R ; W] (Cn + K, C) and a = [-R o ; b] (Cn + K), both double, row-major.  Arguments are checked before anything touches the
 * device (-1: a NULL or misaligned pointer, a non-finite alpha; -2: a shape; -4: the workspace), nothing synchronises with the host,
 * a second run gives the same bits, and a row's outputs do not depend on the other rows of the batch.
 * C % 4 == 0, 4 <= C <= 2048, 1 <= Cn <= C - 1, 2 <= K <= 4096, 1 <= B <= 65535. */
/* Workspace of uvit_op_vim_scores in bytes: y (B, Cn + K) double and two doubles per row, padded to 16 bytes. */
int64_t uvit_op_vim_scores_ws_bytes(int B, int C, int Cn, int K);
/* vim (B) fp32, residual (B) fp32 and pred (B) int32 of feat (B, C) fp32.  y = A f + a goes to ws (16 x 32 output tiles; every
 * element is one fma chain over ascending c from zero, then one addition of a_j).  Per row, by one wave: residual = sqrt(sum_{j < Cn}
 * y_j^2) (lane partial sums in ascending j, then the xor tree); max and arg max of the K logits behind them (the lowest class on
 * ties); lse = max + log(sum_k exp(z_k - max)) in double, same order; vim = fma(alpha, residual, -lse); each output rounded to its type
 * once.  A row with a non-finite feature gets NaN, NaN, -1.  labels (B) int64 and correct (1) int32, both nullable: *correct += the
 * rows whose pred equals their label (an integer atomic).  sums (4) double, nullable: {sum of max_k z, sum of residual, rows used,
 * rows skipped} over the batch's usable rows, added in place by one owner in a fixed order (a third launch of one workgroup; without
 * sums the call makes two launches). */
int uvit_op_vim_scores(const float* feat, const double* A, const double* a, double alpha, float* vim, float* residual, int32_t* pred,
                       const int64_t* labels, int32_t* correct, double* sums, void* ws, int64_t ws_bytes, int B, int C, int Cn, int K,
                       uvit_stream stream);

/* ---- MC-dropout: streaming combination of T stochastic passes (csrc/mcd.hip) ----
 * The reference keeps the logits of all T passes over the whole loader and takes torch.mean(outputs, 0) (uncertainty_evaluations.py:42-89); here
 * every pass is added to a caller-owned per-row state and nothing of size (T, B, K) exists.  One wave per row, no float atomics, every
 * sum has one owner and a fixed order: the bits do not depend on the launch shape (a batch split into two calls gives the bits of one
 * call) and are the same on every run.  Arguments are checked before anything touches the device: UVIT_ERR_ARG for a NULL required
 * pointer, a mode outside {0, 1}, a `first` outside {0, 1} or a state that is not 16-byte aligned; UVIT_ERR_SHAPE for B < 1, K < 1,
 * T < 1.  Asynchronous on `stream`.
 * State of row b: uvit_op_mcd_state_bytes(1, K) bytes at state + b * uvit_op_mcd_state_bytes(1, K):
 *   double sum_z[K], sum_p[K], sum_p2[K], sum_h | int32 votes[K], nan flag | padding to 16 bytes. */
int64_t uvit_op_mcd_state_bytes(int B, int K);        /* < 0: UVIT_ERR_SHAPE */
/* One pass: logits (B, K) fp32.  p[k] = expf((z[k] - max) - logf(sum_k expf(z[k] - max))) in fp32 (uvit_op_ens_combine's formula),
 * widened; sum_z += z, sum_p += p, sum_p2 += p p (double), sum_h += -sum_k p log p (double, 0 log 0 = 0; per-lane partial sums over
 * ascending k, then the xor tree), votes[argmax z] += 1 (lowest index on ties).  first = 1 overwrites instead of adding: no memset.
 * A row with a NaN or +inf logit, or without any logit above -inf, has no softmax: it raises its flag, which stays up. */
int uvit_op_mcd_accumulate(const float* logits, void* state, int first, int B, int K, uvit_stream stream);
/* After T passes: z (B, K) fp32, mode 0: (float)(sum_z / T), the reference's mean of logits; mode 1: (float)log(sum_p / T).
 * unc (B, 5, double, nullable), with pbar = sum_p / T and k* = argmax z (lowest index on ties):
 *   {total = -sum_k pbar log pbar, aleatoric = sum_h / T, mi = max(total - aleatoric, 0),
 *    var_pred = max(sum_p2[k*] / T - pbar[k*]^2, 0), disagreement = 1 - votes[k*] / T}.
 * A flagged row gives five NaNs; z follows IEEE arithmetic.  z holds the same bits whether or not unc is asked for.  The state is only
 * read. */
int uvit_op_mcd_finalize(const void* state, int T, int mode, float* z, double* unc, int B, int K, uvit_stream stream);

/* ---- Learned layer weights over every block's pooled output (csrc/layerweights.hip) ----
 * The reference's --learn_layer_weights (modeling_finetune.py:433-436, 499-510): every block's residual stream is pooled, and a
 * trained softmax over L scalars mixes the pooled vectors in front of the head.  All fp32 in memory, no float atomics: every sum has
 * one owner and a fixed order, so the same input gives the same bits on every run.  Every call checks its arguments before it touches
 * the device (UVIT_ERR_ARG for a NULL required pointer, a mode or a layernorm outside {0, 1}, a negative or NaN eps, a misaligned
 * scratch; UVIT_ERR_SHAPE for a size outside the stated conditions; outputs untouched) and is asynchronous on `stream`.
 * Conditions of all of them: 1 <= B <= 65535, 1 <= L <= UVIT_MAX_DEPTH, C % 4 == 0, 4 <= C <= 2048; the pool: N >= 1. */
int64_t uvit_op_lw_pool_ws_bytes(int B, int L, int N, int C);     /* < 0: the UVIT_ERR_* of the call */
/* pooled (B, L, C) from the residual streams x_layers[l] (B, N, C), l = 0 .. L-1: x_layers is a HOST array of L device pointers, in any
 * address order, none NULL; they travel to the kernels by value (nothing is allocated or copied, the array may be freed on return).
 *   mode 0: the mean over tokens 0 .. N-1, the cls token included: partial column sums per (token slice, layer, sample) into scratch
 *           (uvit_op_lw_pool_ws_bytes bytes), added in slice order by one wave per (sample, layer) row and divided by N (an IEEE
 *           division); two launches for all layers.
 *   mode 1: token 0 of every layer; no other token is read, scratch is not touched; one launch.
 *   layernorm 1: each (b, l) row becomes (p - mean) / sqrt(var + eps), no affine, two-pass variance (F.layer_norm; the reference passes
 *           eps = 1e-5, not the encoder's). */
int uvit_op_lw_pool(const float* const* x_layers, int L, float* pooled, float* scratch, int B, int N, int C, int mode, int layernorm,
                    float eps, uvit_stream stream);
/* w = softmax(log_w) over L values in fp32 (the maximum subtracted, the exponentials added by the xor tree of one wave, one division
 * each); feat[b] (C) = sum_l w_l pooled[b, l], an fma chain in layer order from 0, one wave per row.  w_out (L, nullable) receives w.
 * A weight of exactly 1 returns its layer's bits; equal log-weights at L = 2^k give exactly 1 / L. */
int uvit_op_lw_combine(const float* pooled, const float* log_w, float* feat, float* w_out, int B, int L, int C, uvit_stream stream);
/* dfeat (B, C) = dlogits (B, K) . W (K, C), the third contraction of the head beside uvit_op_probe_logits and uvit_op_probe_head_grad:
 * 64 x 64 LDS-tiled FMA, the reduction over k ascending in tiles of 16 whose sums are added to the running sum; overwritten.
 * B >= 1, K >= 1, C % 4 == 0, C >= 4. */
int uvit_op_probe_input_grad(const float* dlogits, const float* W, float* dfeat, int B, int K, int C, uvit_stream stream);
/* dlog_w (L) fp32, overwritten: with g_l = sum_{b, c} dfeat[b, c] pooled[b, l, c] in double (per row: one wave, per lane over its
 * columns ascending, then the xor tree; then lane l adds the rows in row order) and w of uvit_op_lw_combine (the same bits),
 * dlog_w_l = (float)(w_l (g_l - sum_j w_j g_j)).  scratch: B L doubles, 8-byte aligned. */
int uvit_op_lw_grad(const float* dfeat, const float* pooled, const float* log_w, float* dlog_w, double* scratch, int B, int L, int C,
                    uvit_stream stream);

/* ---- ImageNet-C-style corruptions generated on the device (csrc/corrupt.hip) ----
 * The reference's c_evaluate() reads pre-made corrupted folders; here the clean evaluation images are kept on the device as planar
 * uint8 and every (corruption, severity) set is generated per batch in front of the encoder forward.  IEEE fp32, no contraction, no
 * atomics: the same input gives the same bits on every run, and tests/corrupt_ref.py restates every kind but the two Box-Muller ones
 * bit for bit.  Every call checks its arguments before it touches the device (nothing launched on an error):
 *   UVIT_ERR_ARG        a NULL pointer, an unknown kind, a parameter count that does not fit the kind, a mean or std that is not finite,
 *                       a std of 0, an index0 outside [0, 2^32 - 1 - 21845]
 *   UVIT_ERR_SHAPE      B outside [1, 21845], S outside [8, 1024], a blur radius R >= S or R > 24
 *   UVIT_ERR_WORKSPACE  ws_bytes below uvit_op_corrupt_ws_bytes(kind, B, S)
 * mean / std: HOST, 3 floats each, as in uvit_op_augment_batch. */
#define UVIT_CORRUPT_GAUSSIAN_NOISE 0
#define UVIT_CORRUPT_SPECKLE_NOISE 1
#define UVIT_CORRUPT_IMPULSE_NOISE 2
#define UVIT_CORRUPT_SHOT_NOISE 3
#define UVIT_CORRUPT_BRIGHTNESS 4
#define UVIT_CORRUPT_SATURATE 5
#define UVIT_CORRUPT_CONTRAST 6
#define UVIT_CORRUPT_GAUSSIAN_BLUR 7
#define UVIT_CORRUPT_DEFOCUS_BLUR 8
#define UVIT_CORRUPT_KINDS 9
/* out_u8 (B, 3, S, S) planar uint8 from the normalised fp32 images x (B, 3, S, S) that uvit_op_augment_batch wrote:
 * q = floor(clip(x * std[c] + mean[c], 0, 1) * 255 + 0.5), the exact inverse of the augmentation's step 4 for values that came from
 * uint8. */
int uvit_op_corrupt_pack(const float* x, int B, int S, const float* mean, const float* std, uint8_t* out_u8, uvit_stream stream);
int64_t uvit_op_corrupt_ws_bytes(int kind, int B, int S);        /* < 0: UVIT_ERR_ARG (kind) or UVIT_ERR_SHAPE; may be 0 (ws may then be NULL) */
/* out (B, 3, S, S) fp32 = the corrupted in_u8 (B, 3, S, S), quantised to uint8 levels and normalised.  With v = float(u8) / 255.0f
 * every kind forms v' as below and writes ((q / 255) - mean[c]) / std[c], q = floor(clip(v', 0, 1) * 255 + 0.5) (ImageNet-C truncates;
 * rounding makes pack followed by an identity exact).  params: DEVICE fp32 table of n_params values, prepared once per set
 * (corruptions.corruption_params); z: a standard normal, u: a uniform, both below.
 *   GAUSSIAN_NOISE  [c]                 v + c z
 *   SPECKLE_NOISE   [c]                 v + (v c) z
 *   IMPULSE_NOISE   [c]                 h < T/2: 1; h < T: 0; else v, with T = floor(c 2^32) (common.h's uvit_drop_threshold)
 *   SHOT_NOISE      [c, p0[256], kmax[256]]   min(k / c, 1), k ~ Poisson(lambda = v c) by inversion: k = 0, p = F = p0[u8]; while u > F and
 *                                       k < kmax[u8]: k = k + 1, p = (p lambda) / k, F = F + p.  p0 = exp(-lambda) and kmax, the smallest k whose
 *                                       CDF reaches 1 - 2^-25, come from the host in double from the fp32 lambda (kmax is capped at 512 here)
 *   BRIGHTNESS      [c]                 m = max(r, g, b), m' = min(m + c, 1): rgb (m' / m), or (m', m', m') when m == 0
 *   SATURATE        [c0, c1]            s = (m - min) / m (0 when m == 0), s' = clip(s c0 + c1, 0, 1): m - (m - x) (s' / s) for s > 0, else
 *                                       (m, m (1 - s'), m (1 - s'))
 *   CONTRAST        [c]                 (v - mu) c + mu, mu = float(sum / (255.0 S S)) of the image's channel plane: exact integer sum, division in double
 *   GAUSSIAN_BLUR   2 R + 1 taps        vertical then horizontal pass, border replicate, the fp32 intermediate in ws
 *   DEFOCUS_BLUR    (2 R + 1)^2 taps    dense, row-major, border reflect-101
 * A convolution adds its taps dy ascending, then dx ascending, into one fp32 accumulator from 0, acc = acc + (t x); zero taps are skipped.
 * Draws: with key = h(h(seed ^ (kind + 1) 0x9E3779B9) ^ (index0 + b + 1) 0x85EBCA6B) of image b (h = uvit_hash32; index0 = the index of
 * the batch's first image in the SET), k1 = h(key ^ 0x1B873593), k2 = h(key ^ 0xCC9E2D51) and the counter i = (c S + y) S + x:
 * h1 = h(i ^ k1), h2 = h(i ^ k2), u = u1 = ((h1 >> 8) + 1) 2^-24, u2 = (h2 >> 8) 2^-24, z = sqrtf(-2 logf(u1)) cosf(2 pi u2); impulse
 * noise compares h1.  `seed` is the set's: the caller mixes the severity into it (corruptions.set_seed).  A set therefore has the same
 * bytes for every batch size and every split. */
int uvit_op_corrupt_batch(const uint8_t* in_u8, float* out, int B, int S, int kind, const float* params, int n_params, uint32_t seed,
                          int64_t index0, const float* mean, const float* std, void* ws, int64_t ws_bytes, uvit_stream stream);

/* ---- four more corruptions: pixelate, jpeg_compression, motion_blur, zoom_blur (csrc/corrupt_ext.hip) ----
 * A second op beside uvit_op_corrupt_batch with the same contract: in_u8 and out as above, every kind forms a whole level q in [0, 255]
 * and writes ((q / 255) - mean[c]) / std[c]; IEEE fp32 or integer arithmetic in a fixed order, no contraction, no atomics, no
 * transcendental function on the device, so tests/corrupt_ext_ref.py restates all four bit for bit.  `table`: DEVICE memory of n_table
 * 4-byte words, int32 or fp32 by kind, prepared once per set (corruptions_ext.ext_params); `arg`: the kind's integer, which fixes
 * n_table.  Nothing is launched on an error:
 *   UVIT_ERR_ARG        a NULL pointer, an unknown kind, an arg outside the kind's range, an n_table that does not fit (kind, S, arg), a
 *                       mean or std that is not finite, a std of 0, an index0 outside [0, 2^32 - 1 - 21845]
 *   UVIT_ERR_SHAPE      B outside [1, 21845], S outside [8, 1024], motion_blur with R >= S or R > 24
 *   UVIT_ERR_WORKSPACE  ws_bytes below uvit_op_corrupt_ext_ws_bytes(kind, B, S, arg)
 * PIXELATE (int32 table, arg = n in [1, S]): Pillow's resize((n, n), BOX) then resize((S, S), BOX), bit for bit.  Each resize is a
 *   horizontal then a vertical pass with a uint8 intermediate (ws); a pass writes clip8((2^21 + sum_k pix[first + k] coef[k]) >> 22).
 *   table = down bounds (n, 2) = (first, count) per output, down coefficients (n, kd), kd = 2 ceil(S / 2n) + 1, up bounds (S, 2), up
 *   coefficients (S, 3): Resample.c's precompute_coeffs for the BOX filter, each coefficient int(0.5 + k 2^22), zero past the count.
 * JPEG_COMPRESSION (fp32 table of 192, arg = 0): T[8][8], T[u][x] = c(u) / 2 cos((2 x + 1) u pi / 16), then the luminance and the
 *   chrominance quantisation table, 64 each in natural order.  With P = S rounded up to a multiple of 16 and pixels past the image
 *   repeating its last column and, for Y, its last row; for Cb and Cr a row y >= S repeats row min(((S - 1) & ~1) + (y & 1), S - 1), the
 *   last pair of rows, so that the subsampled plane repeats its last row as libjpeg's does; r, g, b = float(u8):
 *     Y = ((0.299 r + 0.587 g) + 0.114 b), Cb = ((-0.168736 r - 0.331264 g) + 0.5 b) + 128, Cr = ((0.5 r - 0.418688 g) - 0.081312 b) + 128
 *     each of the three rounded to an 8-bit level, floor(clip(x, 0, 255) + 0.5), as a JPEG sample is
 *     Cb, Cr subsampled 4:2:0 by libjpeg's integer mean: floor((((a00 + a01) + (a10 + a11)) + bias) 0.25), bias 1 in the even and 2 in
 *     the odd chroma columns
 *     per 8 x 8 block of p - 128: t[y][u] = sum_x T[u][x] p[y][x], F[v][u] = sum_y T[v][y] t[y][u], F' = rintf(F / Q[v][u]) Q[v][u],
 *     s[y][u] = sum_v T[v][y] F'[v][u], p'[y][x] = (sum_u T[u][x] s[y][u]) + 128; every sum one accumulator from 0, index ascending
 *     chroma back to P x P: 0.75 near + 0.25 far per axis (far = the other neighbour of the fine pixel, clamped to the image's
 *     ceil(S / 2) samples), first
 *     vertically on both columns, then horizontally; cb = Cb - 128, cr = Cr - 128
 *     R = Y + 1.402 cr, G = (Y - 0.344136 cb) - 0.714136 cr, B = Y + 1.772 cb; q = floor(clip(x, 0, 255) + 0.5), cropped to S
 *   The fp32 planes Y (P, P), Cb, Cr (P/2, P/2) of every image live in ws between the two launches.
 * MOTION_BLUR (fp32 table of (R + 1) 183, arg = R): w[R + 1], then per direction a = 0 .. 90 (theta = a - 45 degrees) ox[R + 1] and
 *   oy[R + 1], the whole numbers rint(i cos theta), rint(i sin theta).  v = float(u8) / 255;
 *   v'(y, x) = sum_i w_i v(clamp(y - oy_i), clamp(x - ox_i)), i ascending, acc = acc + (w x); q as in uvit_op_corrupt_batch.
 *   a = ((h(key ^ 0x1B873593) >> 8) 91) >> 24 with key = h(h(seed ^ (9 + kind + 1) 0x9E3779B9) ^ (index0 + b + 1) 0x85EBCA6B): the image
 *   key of uvit_op_corrupt_batch with the kinds numbered on from its nine.  The only kind that reads seed and index0.
 * ZOOM_BLUR (fp32 table of n, arg = n in [1, 32]): 1 / z_j.  v' = (v + sum_j zoom_j(v)) / float(n + 1), j ascending, one accumulator
 *   that starts at v; zoom_j(v)(y, x) samples at sx = c + (x - c) (1 / z_j), sy likewise, c = (S - 1) / 2: x0 = floor(sx), fx = sx - x0,
 *   x1 = min(x0 + 1, S - 1), top = v00 + (v01 - v00) fx, bot = v10 + (v11 - v10) fx, top + (bot - top) fy. */
#define UVIT_CORRUPT_EXT_PIXELATE 0
#define UVIT_CORRUPT_EXT_JPEG_COMPRESSION 1
#define UVIT_CORRUPT_EXT_MOTION_BLUR 2
#define UVIT_CORRUPT_EXT_ZOOM_BLUR 3
#define UVIT_CORRUPT_EXT_KINDS 4
int64_t uvit_op_corrupt_ext_ws_bytes(int kind, int B, int S, int arg);      /* < 0: UVIT_ERR_ARG (kind, arg) or UVIT_ERR_SHAPE; may be 0 */
int uvit_op_corrupt_ext_batch(const uint8_t* in_u8, float* out, int B, int S, int kind, const void* table, int n_table, int arg,
                              uint32_t seed, int64_t index0, const float* mean, const float* std, void* ws, int64_t ws_bytes,
                              uvit_stream stream);

/* ---- probe training: random erasing, mixup and cutmix of a batch, and the soft-target loss (csrc/mixup.hip) ----
 * timm's RandomErasing (per-sample transform) followed by timm's Mixup (behind the collate), run_class_finetuning.py:128-149, on the
 * normalised fp32 images x (B, 3, S, S) that uvit_op_augment_batch wrote, into out (B, 3, S, S), one launch.  1 <= B <= 65535,
 * 1 <= S <= 4096, 0 <= R <= 8 erase boxes per row.  IEEE fp32 evaluated as written, no contraction, no atomics; the same input gives
 * the same bits on every run.
 * desc[b] (HOST, B entries): kind, lam in [0, 1], partner in [0, B), the cutmix box rows [yl, yh) and columns [xl, xh) with
 * 0 <= yl <= yh <= S and 0 <= xl <= xh <= S (read for every kind, used by CUTMIX).  boxes (HOST, (B, R); NULL when R == 0): the erase
 * boxes of row b, rows [top, top + h), columns [left, left + w) inside the image; h == 0: none.  Both are validated here and copied
 * into the workspace by asynchronous copies on `stream`: keep them unchanged until the stream has passed this call (pinned memory,
 * like any hipMemcpyAsync source).  workspace: uvit_op_mix_ws_bytes(B, R) bytes (< 0: UVIT_ERR_SHAPE).
 * e(j, c, y, x), sample j behind its erasing: x[j, c, y, x] outside every box of j; inside one, the fill of the LAST box that holds
 * the pixel (a later box overwrites an earlier one):
 *   erase_mode CONST   0.0f
 *              RAND    n(j, q) with q = 3 r + c             one standard normal per (sample, box r, channel)
 *              PIXEL   n(j, q) with q = (c S + y) S + x     one per (sample, channel, pixel); does not depend on the box
 * n(j, q), with h = uvit_hash32: kit = h(seed ^ (iteration 0x9E3779B9 + 0x7F4A7C15)), kj = h(kit ^ (j + 1) 0x85EBCA6B),
 *   k1 = h(kj ^ 0x1B873593), k2 = h(kj ^ 0xCC9E2D51), h1 = h(q ^ k1), h2 = h(q ^ k2), u_i = ((h_i >> 9) + 0.5) 2^-23 (exact in fp32,
 *   inside (0, 1)), n = sqrtf(-2.0f logf(u1)) cosf(6.2831854820251465f u2), every product in fp32 (all words mod 2^32).  The key holds
 *   the seed, the iteration and the sample's index j alone: an erased pixel of sample j has the same value as itself and as anybody's
 *   partner, for every B and every launch shape.
 * out[b], with p = desc[b].partner and lam = desc[b].lam:
 *   NONE     e(b)
 *   MIXUP    fl(fl(lam e(b)) + fl(fl(1.0f - lam) e(p)))
 *   CUTMIX   e(p) inside the cutmix box, e(b) outside
 * A row whose partner is itself is legal.  A NONE row does not read its partner, a CUTMIX row reads it inside the box only (16-byte
 * accesses when S % 4 == 0 and both pointers are 16-byte aligned; any S >= 1 is correct).
 * Errors (nothing launched, out untouched): UVIT_ERR_ARG for a NULL pointer (boxes with R > 0 included), an unknown kind or
 * erase_mode, a lam outside [0, 1] (NaN included), a partner outside [0, B), and for out overlapping x anywhere (rows read their
 * partners); UVIT_ERR_SHAPE for B, S or R outside their limits, a cutmix box or an erase box outside the image, h < 0 or h > 0 with
 * w < 1; UVIT_ERR_WORKSPACE. */
#define UVIT_MIX_NONE 0
#define UVIT_MIX_MIXUP 1
#define UVIT_MIX_CUTMIX 2
#define UVIT_MIX_ERASE_CONST 0
#define UVIT_MIX_ERASE_RAND 1
#define UVIT_MIX_ERASE_PIXEL 2
#define UVIT_MIX_MAX_BOXES 8
typedef struct uvit_mix_desc {
    int32_t kind;                              /* UVIT_MIX_{NONE, MIXUP, CUTMIX} */
    float lam;
    int32_t partner;
    int32_t yl, yh, xl, xh;                    /* the cutmix box */
    int32_t reserved;                          /* 0 */
} uvit_mix_desc;
typedef struct uvit_mix_box { int32_t top, left, h, w; } uvit_mix_box;
int64_t uvit_op_mix_ws_bytes(int B, int R);
int uvit_op_mix_batch(const float* x, float* out, const uvit_mix_desc* desc, const uvit_mix_box* boxes, int B, int S, int R,
                      int erase_mode, uint32_t seed, uint32_t iteration, void* workspace, int64_t ws_bytes, uvit_stream stream);
/* timm SoftTargetCrossEntropy on Mixup's two-label target (engine_for_finetuning.py:617-619) without a (B, K) target tensor, one wave
 * per row: with p = partner[b] (int32[B], device), lam_b = lam[b] (float[B], device), s = smoothing and
 *   t = lam_b oh(y_b) + (1 - lam_b) oh(y_p),  oh(y)_k = s / K + (1 - s) [k == y]      (mixup_target: off = s / K, on = 1 - s + off)
 *   row_loss[b] = -sum_k t_k log softmax(z)_k = lam_b L(y_b) + (1 - lam_b) L(y_p),  L(y) = uvit_op_probe_ce's row formula;
 *   *loss_out = mean_b row_loss[b], summed by one wave in row order;  dlogits (nullable) = (softmax - t) / B.
 * No accuracy counters: the reference reports no training accuracy under mixup.  A label, own or partner's, outside [0, K), a partner
 * outside [0, B) or a lam outside [0, 1] makes row_loss[b], the row of dlogits and *loss_out NaN; nothing is read at the bad index.
 * UVIT_ERR_ARG for a NULL required pointer or a smoothing outside [0, 1); UVIT_ERR_SHAPE for B < 1 or K < 1 (K = 1 is legal). */
int uvit_op_probe_ce_mix(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam, float smoothing,
                         float* dlogits, float* row_loss, float* loss_out, int B, int K, uvit_stream stream);

/* ---- probe training: RandAugment of a batch, Pillow's arithmetic bit for bit (csrc/randaug.hip) ----
 * timm's rand_augment_transform (`--aa rand-m9-mstd0.5-inc1`, run_class_finetuning.py:117) on the normalised fp32 images x (B, 3, S, S)
 * that uvit_op_augment_batch wrote, into out (B, 3, S, S); out may be x.  1 <= B <= 65535, 1 <= S <= 1024.  mean, std: HOST, 3 floats.
 * The first stage quantises as uvit_op_corrupt_pack does, q = floor(clip(x * std[c] + mean[c], 0, 1) * 255 + 0.5); the layers of image
 * b then run in order on the uint8 image the previous layer left; the last stage writes ((u8 / 255) - mean[c]) / std[c], the
 * augmentation's step 4.  An image whose layers are all NONE comes out with the bits it went in with (for values that came from uint8).
 * desc (HOST, B entries, validated here and copied into the workspace by an asynchronous copy on `stream`: keep it unchanged until the
 * stream has passed this call): n_layers in [0, UVIT_RANDAUG_MAX_LAYERS] layers {op, filter, arg0, arg1, factor, fill, matrix[6]}:
 *   INVERT                    255 - v
 *   POSTERIZE    arg0 = bits in [0, 8]: v & ~(2^(8 - bits) - 1); 8: the identity, 0: black
 *   SOLARIZE     arg0 = thresh in [0, 256]: v < thresh ? v : 255 - v
 *   SOLARIZE_ADD arg0 = add in [0, 255], arg1 = thresh in [0, 256]: v < thresh ? min(255, v + add) : v
 *   AUTOCONTRAST ImageOps.autocontrast(cutoff 0), per channel from its histogram: lo, hi = the lowest and highest level present;
 *                hi <= lo: identity; else scale = 255.0 / (hi - lo), offset = -lo * scale, clamp((int)(v * scale + offset)) in double
 *   EQUALIZE     ImageOps.equalize, per channel, integers: fewer than two levels present: identity; step = (S S - h[last level present])
 *                / 255; step == 0: identity; else min(255, (step / 2 + sum_{j < v} h[j]) / step)
 *   COLOR, CONTRAST, BRIGHTNESS, SHARPNESS   ImageEnhance.*.enhance(factor) = Blend.c's float32 d + factor * (v - d), clipped and
 *                truncated, with d = L (Convert.c's rgb2l of the pixel), (int)(mean of L over the image + 0.5), 0, and ImageFilter.SMOOTH:
 *                a float32 accumulator that starts at 0.5f and takes the nine products v * (k / 13.0f), k = 1 1 1 1 5 1 1 1 1, in
 *                row-major order, <= 0: 0, >= 255: 255, else truncated; the one-pixel border is the image's own
 *   ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X_REL, TRANSLATE_Y_REL   Image.transform(AFFINE, matrix, filter, fillcolor = fill): the host
 *                forms the matrix (probe_randaug.py), the five ops are one mechanism here.  BILINEAR and BICUBIC are Geometry.c's
 *                ImagingGenericTransform in double: xin = (m0 (x + .5) + m1 (y + .5)) + m2, yin likewise; fill where xin < 0, xin >= S,
 *                yin < 0 or yin >= S; else subtract 0.5, take floor and the fraction; columns clamped to [0, S); the first row clamped, a
 *                later row outside the image repeats the previous row's value; bilinear a + (b - a) d truncated; bicubic p1 = v2,
 *                p2 = -v1 + v3, p3 = 2 (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4, v = p1 + d (p2 + d (p3 + d p4)), clamped to
 *                [0, 255], truncated.  NEAREST is not the generic transform in Pillow and is not here: with m1 == m3 == 0
 *                (ImagingScaleAffine) the source column is trunc((m2 + m0 0.5) + m0 x), -1 below 0, rows likewise; otherwise
 *                (affine_fixed) 16.16 fixed point, FIX(v) = floor(v 65536 + 0.5): xin = (FIX(m2 + m0 0.5 + m1 0.5) + x FIX(m0) + y FIX(m1))
 *                >> 16, yin likewise; fill where the source lies outside the image.  |m0|, |m1|, |m3|, |m4| <= 4 and |m2|, |m5| <= 8192
 *                keep the fixed-point walk inside 32 bits.
 *   fill = r | g << 8 | b << 16.  filter: a PIL.Image.Resampling value, read by the affine ops.
 * workspace: uvit_op_randaug_ws_bytes(B, S) bytes (< 0: UVIT_ERR_SHAPE): the descriptors, a 1 KiB table block per image and two planar
 * uint8 copies of the batch that the layers write in turn.  Launches: the pack, per layer a statistics pass when an image's op needs a
 * histogram or the mean of L and an apply pass when an image has an op, then the inverse.  No float atomics: the histograms and the
 * sum of L are integer LDS atomics; the same input gives the same bits on every run and for every B.
 * Errors (nothing launched): UVIT_ERR_SHAPE for B, S or an n_layers outside their limits; UVIT_ERR_ARG for a NULL pointer, a mean or
 * std that is not finite, a std of 0, an unknown op or filter, a factor or a matrix entry that is not finite or a matrix outside the
 * bounds above, or bits, thresh or add outside their ranges; UVIT_ERR_WORKSPACE. */
#define UVIT_RANDAUG_MAX_LAYERS 4
#define UVIT_RA_NONE 0                         /* the layer was not applied; 1 .. 15: timm's _RAND_TRANSFORMS in its order */
#define UVIT_RA_AUTOCONTRAST 1
#define UVIT_RA_EQUALIZE 2
#define UVIT_RA_INVERT 3
#define UVIT_RA_ROTATE 4
#define UVIT_RA_POSTERIZE 5
#define UVIT_RA_SOLARIZE 6
#define UVIT_RA_SOLARIZE_ADD 7
#define UVIT_RA_COLOR 8
#define UVIT_RA_CONTRAST 9
#define UVIT_RA_BRIGHTNESS 10
#define UVIT_RA_SHARPNESS 11
#define UVIT_RA_SHEAR_X 12
#define UVIT_RA_SHEAR_Y 13
#define UVIT_RA_TRANSLATE_X_REL 14
#define UVIT_RA_TRANSLATE_Y_REL 15
#define UVIT_RA_OPS 16
#define UVIT_RA_NEAREST 0
#define UVIT_RA_BILINEAR 2
#define UVIT_RA_BICUBIC 3
typedef struct uvit_randaug_layer {
    int32_t op;                                /* UVIT_RA_* */
    int32_t filter;                            /* UVIT_RA_{NEAREST, BILINEAR, BICUBIC} */
    int32_t arg0, arg1;
    float factor;
    uint32_t fill;
    double matrix[6];
} uvit_randaug_layer;
typedef struct uvit_randaug_desc {
    int32_t n_layers;
    int32_t reserved;                          /* 0 */
    uvit_randaug_layer layers[UVIT_RANDAUG_MAX_LAYERS];
} uvit_randaug_desc;
int64_t uvit_op_randaug_ws_bytes(int B, int S);
int uvit_op_randaug_batch(const float* x, float* out, const uvit_randaug_desc* desc, int B, int S, const float* mean, const float* std,
                          void* workspace, int64_t ws_bytes, uvit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* UVIT_H */
