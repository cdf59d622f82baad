// Engine: arena layout, workspace plan and the launch sequence of the data2vec ViT step
// (engine_for_cyclical.py:58-186 over modeling_cyclical.py:170-225) on one HIP stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/uvit.h"
#include "common.h"
#include "uvit_internal.h"

#define CHECK(x) do { int _rc = (x); if (_rc) return _rc; } while (0)
#define NREP 32
#define RP(off) (e->grep + ((off) - e->lo.n_decay))   // replica 0 address of a no-decay gradient
#define HIPCHECK(x) do { if ((x) != hipSuccess) return UVIT_ERR_LAUNCH; } while (0)
// every GEMM launch of the engine carries the engine's own tuning (no process-wide launcher state)
#define GEMM_NT(...) uvit_gemm_nt_launch(__VA_ARGS__, &e->tune)
#define GEMM_TN(...) uvit_gemm_tn_launch(__VA_ARGS__, &e->tune)
#define GEMM_TN_GROUP(...) uvit_gemm_tn_group_launch(__VA_ARGS__, &e->tune)

// ------------------------------------------------------------------------------------------
// layout
// ------------------------------------------------------------------------------------------
// x[2]: per stream, 0 = mean (the only one of the base model), 1 = covariance (the "cov_" tensors; filled, like cqkvw, for the two-stream model only)
struct LayerOff { size_t n1w, n1b, qkvw, qb[2], vb[2], projw[2], projb[2], g1, n2w, n2b, fc1w, fc1b, fc2w, fc2b, g2, cqkvw; };
struct Layout {
    size_t cls[2], mask_tok[2], pew[2], peb[2], relt, normw, normb, lmw[2], lmb[2], pos;
    LayerOff L[UVIT_MAX_DEPTH];
    size_t n_total, n_decay, n_live;     // [0, n_decay) decay | [n_decay, n_live) no-decay | [n_live, n_total) frozen
    std::vector<uvit_layout_entry> entries;
};

static size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

static int cfg_ok(const uvit_config* c) {
    if (!c) return UVIT_ERR_ARG;
    if (c->depth < 1 || c->depth > UVIT_MAX_DEPTH || c->num_heads < 1) return UVIT_ERR_SHAPE;
    // head_dim 64 (ViT-B/L) or, base model only, 80 (ViT-H): attention2.hip (two-stream) is specialised for 64
    if (c->embed_dim != c->num_heads * 64 && (c->two_stream || c->embed_dim != c->num_heads * 80)) return UVIT_ERR_SHAPE;
    if (c->embed_dim % 64 || c->mlp_hidden % 64 || c->patch_size % 8 || c->img_size % c->patch_size) return UVIT_ERR_SHAPE;
    if ((c->in_chans * c->patch_size * c->patch_size) % 64) return UVIT_ERR_SHAPE;
    const int g = c->img_size / c->patch_size;
    if (g * g + 1 > 208 || c->batch < 1) return UVIT_ERR_SHAPE;
    if (c->use_abs_pos_emb && c->two_stream) return UVIT_ERR_SHAPE;      // the two-stream model has no position embedding (modeling_cyclical_dist.py:113-130)
    return UVIT_OK;
}

static void build_layout(const uvit_config* c, Layout& lo) {
    const int64_t C = c->embed_dim, Hd = c->mlp_hidden, g = c->img_size / c->patch_size;
    size_t off = 0;
    auto add = [&](const std::string& name, std::vector<int64_t> shape, int decay) -> size_t {
        uvit_layout_entry e;
        memset(&e, 0, sizeof(e));
        snprintf(e.name, sizeof(e.name), "%s", name.c_str());
        e.offset = (int64_t)off; e.ndim = (int)shape.size(); e.decay = decay; e.numel = 1;
        for (size_t i = 0; i < shape.size(); ++i) { e.shape[i] = shape[i]; e.numel *= shape[i]; }
        lo.entries.push_back(e);
        const size_t at = off;
        off = align64(off + (size_t)e.numel);
        return at;
    };
    auto blk = [](int i, const char* s) { return "blocks." + std::to_string(i) + "." + s; };
    // ---- decay group: everything that is not 1-D, not *.bias, not in {pos_embed, cls_token} ----
    const bool two = c->two_stream != 0;
    lo.mask_tok[0] = add("mask_token", {1, 1, C}, 1);
    if (two) lo.mask_tok[1] = add("cov_mask_token", {1, 1, C}, 1);
    // 'cov_cls_token' is not in the no_weight_decay() skip list {'pos_embed','cls_token'} and is 3-D: decay group
    if (two) lo.cls[1] = add("cov_cls_token", {1, 1, C}, 1);
    if (c->use_shared_rel_pos_bias) lo.relt = add("rel_pos_bias.relative_position_bias_table", {(2 * g - 1) * (2 * g - 1) + 3, c->num_heads}, 1);
    else lo.relt = (size_t)-1;
    lo.pew[0] = add("patch_embed.proj.weight", {C, c->in_chans, c->patch_size, c->patch_size}, 1);
    if (two) lo.pew[1] = add("cov_patch_embed.proj.weight", {C, c->in_chans, c->patch_size, c->patch_size}, 1);
    for (int i = 0; i < c->depth; ++i) {
        lo.L[i].qkvw = add(blk(i, "attn.qkv.weight"), {3 * C, C}, 1);
        lo.L[i].projw[0] = add(blk(i, "attn.proj.weight"), {C, C}, 1);
        if (two) lo.L[i].projw[1] = add(blk(i, "attn.cov_proj.weight"), {C, C}, 1);
        lo.L[i].fc1w = add(blk(i, "mlp.fc1.weight"), {Hd, C}, 1);
        lo.L[i].fc2w = add(blk(i, "mlp.fc2.weight"), {C, Hd}, 1);
    }
    lo.lmw[0] = add("lm_head.weight", {C, C}, 1);
    if (two) lo.lmw[1] = add("cov_lm_head.weight", {C, C}, 1);
    lo.n_decay = off;
    // ---- no-decay group ----
    lo.cls[0] = add("cls_token", {1, 1, C}, 0);
    // 'pos_embed' (1, N, C) is 3-D but sits in the no_weight_decay() skip list (modeling_cyclical.py:163-165)
    lo.pos = c->use_abs_pos_emb ? add("pos_embed", {1, g * g + 1, C}, 0) : (size_t)-1;
    lo.peb[0] = add("patch_embed.proj.bias", {C}, 0);
    if (two) lo.peb[1] = add("cov_patch_embed.proj.bias", {C}, 0);
    for (int i = 0; i < c->depth; ++i) {
        lo.L[i].g1 = add(blk(i, "gamma_1"), {C}, 0);
        lo.L[i].g2 = add(blk(i, "gamma_2"), {C}, 0);
        lo.L[i].n1w = add(blk(i, "norm1.weight"), {C}, 0);
        lo.L[i].n1b = add(blk(i, "norm1.bias"), {C}, 0);
        lo.L[i].qb[0] = add(blk(i, "attn.q_bias"), {C}, 0);
        lo.L[i].vb[0] = add(blk(i, "attn.v_bias"), {C}, 0);
        if (two) { lo.L[i].qb[1] = add(blk(i, "attn.cov_q_bias"), {C}, 0); lo.L[i].vb[1] = add(blk(i, "attn.cov_v_bias"), {C}, 0); }
        lo.L[i].projb[0] = add(blk(i, "attn.proj.bias"), {C}, 0);
        if (two) lo.L[i].projb[1] = add(blk(i, "attn.cov_proj.bias"), {C}, 0);
        lo.L[i].n2w = add(blk(i, "norm2.weight"), {C}, 0);
        lo.L[i].n2b = add(blk(i, "norm2.bias"), {C}, 0);
        lo.L[i].fc1b = add(blk(i, "mlp.fc1.bias"), {Hd}, 0);
        lo.L[i].fc2b = add(blk(i, "mlp.fc2.bias"), {C}, 0);
    }
    lo.normw = add("norm.weight", {C}, 0);
    lo.normb = add("norm.bias", {C}, 0);
    lo.lmb[0] = add("lm_head.bias", {C}, 0);
    if (two) lo.lmb[1] = add("cov_lm_head.bias", {C}, 0);
    lo.n_live = off;
    // attn.cov_qkv.weight is never used by the reference's forward (modeling_finetune_dist.py:127 reuses qkv.weight):
    // its .grad stays None, so torch's AdamW never touches it (no weight decay either).  It lives at the END of the
    // no-decay region with a zero gradient, which leaves it exactly constant; flag 2 = "frozen".  Being last keeps its
    // 21 M floats out of the replicated column-sum accumulators (which span [n_decay, n_live) only).
    if (two)
        for (int i = 0; i < c->depth; ++i) lo.L[i].cqkvw = add(blk(i, "attn.cov_qkv.weight"), {3 * C, C}, 2);
    lo.n_total = off;
}

// ------------------------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------------------------
// Activation buffers are STACKED over the S streams of the model (S = 1 base model, S = 2 two-stream
// "stochastic" model: mean rows [0, M), covariance rows [Mpad, Mpad + M)).  Ops whose weights are shared by the
// streams (LayerNorms, fc1, fc2 weight gradient, qkv weight gradient, ...) run ONCE over the stacked rows.
struct LayerActs {
    bf16 *ln1, *qkv, *attn, *projout, *ln2, *h, *a, *mlpout;
    float *mean1, *rstd1, *mean2, *rstd2, *lse;
};

struct uvit_engine {
    uvit_config cfg;
    uvit_buffers buf;
    Layout lo;
    int B, P, N, NP, C, Hd, H, Kpe, M, Mpad, BP, BPpad;     // (Hd: the MLP hidden size)
    int head_dim;          // C / H: 64 or 80
    float attn_scale;      // head_dim ** -0.5 (0.125f for 64)
    int S;                 // streams: 1 or 2
    GemmTune tune;         // launch tuning of this engine's GEMMs (uvit_engine_set_tuning)
    int cur_B;             // batch of the last forward
    // the "tail valid" record: the weight set and batch of the uvit_engine_forward_features whose X[0..depth] are still in the workspace
    // (uvit_engine_forward_tail reads one of them); -1 after a training step, a failed forward or tail, or on a fresh engine.
    // tail_first: the lowest block a tail has started at since that forward (depth: none yet) -- X[l] for l > tail_first is a tail's
    int tail_which = -1, tail_B = 0, tail_first = 0;
    // workspace
    bf16* cols;
    float* X[UVIT_MAX_DEPTH + 1];
    float* XM[UVIT_MAX_DEPTH];
    LayerActs acts[UVIT_MAX_DEPTH];
    LayerActs tacts;       // teacher scratch (nothing saved)
    float *tX[2], *tXM;
    int *rowidx, *count;
    bf16 *normed[2], *dout[2], *dnormed[2], *dpatch[2];
    float *meanF[2], *rstdF[2], *outputs[2], *targets[2];
    float *biasP_s, *biasP_t, *slabs, *delta;
    void* ds_ws[2] = {nullptr, nullptr};   // fused attention backward: dS of one layer (bf16), by layer parity: the batch reduction runs on the second stream
    float *dXa, *dXb;
    bf16 *dY1[2], *dY2[2], *dH[2], *dLN, *dAttn, *dqkv[2];   // [layer parity]: read by the wgrad stream while the next layer runs
    float *dp_scales, *dp_rates;
    // drop-path sample lists (training step): per (layer, draw) list lb = 2 S l + k, k as in dp_draw (base: attn, mlp; two-stream: mean attn,
    // mean mlp, cov attn, cov mlp -- only the two MLP lists are used there: the two-stream attention needs both streams of a sample)
    int *dpl_pos = nullptr, *dpl_bmap = nullptr, *dpl_rows = nullptr, *dpl_cnt = nullptr;
    size_t dpl_stride = 0;                 // ints per rows list
    int dpl_K[128] = {};                   // kept samples per list (2 S lists per layer), from the host's evaluation of the drop-path hash
    bool dpl_enable = true;                // uvit_engine_set_drop_path_rows
    bool dpl_on = false;                   // the current step runs with lists
    // LayerScale gradient: false (default) = from the weight gradient (ls_dgamma_kernel), nothing of the branch outputs is saved; true = the
    // student forward saves every branch's pre-LayerScale output (acts[l].projout / mlpout) and the riders sum dgamma from it
    bool ls_saved_y = false;               // uvit_engine_set_ls_saved_y
    bool ls_saved_step = false;            // ... as latched by uvit_step_begin for the step's forward and backward
    std::vector<float> dp_rates_host;
    float *loss, *gnorm; double* sumsq;
    float* wl_scratch;     // Wasserstein loss: scalars + per-row distances
    float *dense_v, *dense_acc; int *idrows, *idcount;   // dense target builder (batch / instance-norm target variants)
    float* var_scratch;    // variance term: column sums / centred squares (2 C + 16 floats)
    int* poisoned;         // sticky: set by the first step whose loss / gradient norm is not finite; AdamW and EMA then skip every step
    TransposeDesc* tdesc; int n_tdesc, n_ttiles;
    int64_t* mask_copy;
    unsigned* tile_cnt = nullptr;   // 2 x 16 counters (caller's stream, second stream): dynamic tile assignment of the persistent GEMMs
    float* grep;           // [NREP][no-decay region] replicated column-sum accumulators
    size_t n_nd;           // floats in the live (not frozen) part of the no-decay region
    bool slab_started;
    bool last_dropout; uint32_t last_seed;
    int bwd_next = -1;      // the layer uvit_step_backward_layer takes next: depth-1 after uvit_step_begin, then down to 0 (-1: none)
    int compact_R = 0;      // > 0: this step runs the last block's MLP on the masked rows only, in R (multiple of 64) compact rows (uvit_step_params.n_rows_hint)
    // second stream: teacher forward beside student forward; wgrad GEMMs beside the dgrad chain
    bool dual = true;
    hipStream_t aux = nullptr, aux_eq = nullptr, aux_lo = nullptr;     // aux = the one in use (uvit_engine_set_streams)
    hipEvent_t ev_fork = nullptr, ev_teacher = nullptr, ev_x = nullptr;
    hipEvent_t ev_wdone[UVIT_MAX_DEPTH] = {};
    hipEvent_t ev_ds = nullptr;             // dS of the current layer is complete (main stream -> second stream)
    // optional HIP-event bracketing of the dominant kernel (fc1 GEMM, EPI_GELU) for bench.py's roofline
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;   // pairs
    std::vector<int> prof_kind;        // per pair: UVIT_PROF_* (which Linear of the block the bracket holds)
    std::vector<int> prof_rows;        // per pair: rows of the bracketed launch (compact launches run fewer than B x tokens)
    size_t prof_used = 0;
    // stacked-row helpers
    size_t rows_all() const { return (size_t)(S - 1) * Mpad + M; }      // rows a stacked row-wise op covers
    size_t rows_alloc() const { return (size_t)S * Mpad; }
};

struct Bump {
    char* base; size_t off, cap;
    template <typename T> T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? (T*)(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

static size_t roundup(size_t x, size_t m) { return (x + m - 1) / m * m; }
static std::vector<float> dp_rates_linspace(int depth, float rate);

static void plan_workspace(uvit_engine* e, Bump& b) {
    const uvit_config& c = e->cfg;
    const size_t Mp = e->rows_alloc(), C = e->C, Hd = e->Hd, BPp = e->BPpad;
    auto acts = [&](LayerActs& a) {
        a.ln1 = b.take<bf16>(Mp * C); a.qkv = b.take<bf16>(Mp * 3 * C); a.attn = b.take<bf16>(Mp * C);
        a.projout = b.take<bf16>(Mp * C); a.ln2 = b.take<bf16>(Mp * C); a.h = b.take<bf16>(Mp * Hd);
        a.a = b.take<bf16>(Mp * Hd); a.mlpout = b.take<bf16>(Mp * C);
        a.mean1 = b.take<float>(Mp); a.rstd1 = b.take<float>(Mp); a.mean2 = b.take<float>(Mp); a.rstd2 = b.take<float>(Mp);
        a.lse = b.take<float>((size_t)e->B * e->H * e->N);
    };
    e->cols = b.take<bf16>(BPp * e->Kpe);
    for (int i = 0; i <= c.depth; ++i) e->X[i] = b.take<float>(Mp * C);
    for (int i = 0; i < c.depth; ++i) { e->XM[i] = b.take<float>(Mp * C); acts(e->acts[i]); }
    acts(e->tacts);
    e->tX[0] = b.take<float>(Mp * C); e->tX[1] = b.take<float>(Mp * C); e->tXM = b.take<float>(Mp * C);
    e->rowidx = b.take<int>(e->BP + 64); e->count = b.take<int>(64);
    for (int st = 0; st < e->S; ++st) {
        e->normed[st] = b.take<bf16>(BPp * C); e->dout[st] = b.take<bf16>(BPp * C); e->dnormed[st] = b.take<bf16>(BPp * C);
        e->dpatch[st] = b.take<bf16>(BPp * C);
        e->meanF[st] = b.take<float>(BPp); e->rstdF[st] = b.take<float>(BPp);
        e->outputs[st] = b.take<float>(BPp * C); e->targets[st] = b.take<float>(BPp * C);
    }
    const size_t bias_n = (size_t)e->H * e->NP * e->NP;
    e->biasP_s = b.take<float>(bias_n); e->biasP_t = b.take<float>(bias_n);
    e->slabs = b.take<float>(bias_n);       // ONE bias-gradient slab [h][key][q] (both model families since round 4)
    e->delta = b.take<float>((size_t)e->B * e->H * e->N);
    if (e->cfg.use_shared_rel_pos_bias)
        for (int k = 0; k < 2; ++k)
            e->ds_ws[k] = b.take<char>(e->S == 1 ? uvit_attn_bwd_fused_ws_bytes(e->B, e->H, e->N) : uvit_attn2_bwd_ws_bytes(e->B, e->H, e->N));
    e->dXa = b.take<float>(Mp * C); e->dXb = b.take<float>(Mp * C);
    for (int k = 0; k < 2; ++k) {
        e->dY1[k] = b.take<bf16>(Mp * C); e->dY2[k] = b.take<bf16>(Mp * C); e->dH[k] = b.take<bf16>(Mp * Hd);
        e->dqkv[k] = b.take<bf16>(Mp * 3 * C);
    }
    e->dLN = b.take<bf16>(Mp * C); e->dAttn = b.take<bf16>(Mp * C);
    e->dp_scales = b.take<float>((size_t)c.depth * 2 * e->S * e->B); e->dp_rates = b.take<float>(c.depth);
    if ((size_t)c.depth * 2 * e->S <= 128) {
        const size_t nl = (size_t)c.depth * 2 * e->S;
        e->dpl_stride = roundup((size_t)e->B * e->N, 64);
        e->dpl_pos = b.take<int>(nl * e->B); e->dpl_bmap = b.take<int>(nl * e->B);
        e->dpl_rows = b.take<int>(nl * e->dpl_stride); e->dpl_cnt = b.take<int>(2 * nl + 64);    // counts, then the host-mismatch flags
    }
    e->loss = b.take<float>(64); e->gnorm = e->loss + 1; e->sumsq = (double*)(e->loss + 2);
    e->wl_scratch = b.take<float>(16 + BPp);
    e->poisoned = b.take<int>(64);
    e->var_scratch = b.take<float>(2 * C + 16);
    e->dense_v = b.take<float>(BPp * C); e->dense_acc = b.take<float>(BPp * C);
    e->idrows = b.take<int>(e->BP + 64); e->idcount = b.take<int>(64);
    e->tdesc = b.take<TransposeDesc>(7 * c.depth + 4);
    e->mask_copy = b.take<int64_t>(e->BP + 64);
    e->grep = b.take<float>((size_t)NREP * e->n_nd);
    e->tile_cnt = b.take<unsigned>(64);          // zero from the workspace memset; every launch leaves its counters at zero
}

static void fill_dims(uvit_engine* e) {
    const uvit_config& c = e->cfg;
    const int g = c.img_size / c.patch_size;
    e->B = c.batch; e->P = g * g; e->N = e->P + 1; e->NP = 208; e->C = c.embed_dim; e->Hd = c.mlp_hidden;
    e->H = c.num_heads; e->Kpe = c.in_chans * c.patch_size * c.patch_size;
    e->head_dim = c.embed_dim / c.num_heads;
    e->attn_scale = e->head_dim == 64 ? 0.125f : (float)(1.0 / std::sqrt((double)e->head_dim));
    e->S = c.two_stream ? 2 : 1;
    e->M = e->B * e->N; e->Mpad = (int)roundup(e->M, 128); e->BP = e->B * e->P; e->BPpad = (int)roundup(e->BP, 128);
    e->cur_B = e->B;
    Layout tmp_lo; build_layout(&e->cfg, tmp_lo);
    e->n_nd = tmp_lo.n_live - tmp_lo.n_decay;      // span of the replicated accumulators: live no-decay tensors only
}

extern "C" void uvit_engine_destroy(uvit_engine* e);
extern "C" int uvit_version(void) { return UVIT_VERSION; }
#ifndef UVIT_SRC_HASH
#define UVIT_SRC_HASH "unknown"
#endif
extern "C" const char* uvit_source_hash(void) { return UVIT_SRC_HASH; }

extern "C" int uvit_layout_count(const uvit_config* cfg) {
    if (cfg_ok(cfg)) return UVIT_ERR_SHAPE;
    Layout lo; build_layout(cfg, lo);
    return (int)lo.entries.size();
}
extern "C" int uvit_layout_get(const uvit_config* cfg, int index, uvit_layout_entry* out) {
    if (cfg_ok(cfg) || !out) return UVIT_ERR_SHAPE;
    Layout lo; build_layout(cfg, lo);
    if (index < 0 || index >= (int)lo.entries.size()) return UVIT_ERR_ARG;
    *out = lo.entries[index];
    return UVIT_OK;
}
extern "C" int64_t uvit_arena_numel(const uvit_config* cfg, int64_t* n_decay_out) {
    if (cfg_ok(cfg)) return UVIT_ERR_SHAPE;
    Layout lo; build_layout(cfg, lo);
    if (n_decay_out) *n_decay_out = (int64_t)lo.n_decay;
    return (int64_t)lo.n_total;
}
extern "C" int64_t uvit_workspace_bytes(const uvit_config* cfg) {
    if (cfg_ok(cfg)) return UVIT_ERR_SHAPE;
    uvit_engine tmp;
    tmp.cfg = *cfg;
    fill_dims(&tmp);
    Bump b{nullptr, 0, 0};
    plan_workspace(&tmp, b);
    return (int64_t)roundup(b.off, 4096) + 4096;
}

extern "C" uvit_engine* uvit_engine_create(const uvit_config* cfg, const uvit_buffers* bufs, uvit_stream stream, int* err_out) {
    auto fail = [&](int rc) -> uvit_engine* { if (err_out) *err_out = rc; return nullptr; };
    if (cfg_ok(cfg) || !bufs) return fail(UVIT_ERR_SHAPE);
    if (!bufs->params || !bufs->grads || !bufs->adam_m || !bufs->adam_v || !bufs->ema || !bufs->params_bf16 ||
        !bufs->params_bf16_t || !bufs->ema_bf16 || !bufs->workspace) return fail(UVIT_ERR_ARG);
    if (cfg->use_shared_rel_pos_bias && !bufs->rel_index) return fail(UVIT_ERR_ARG);
    if (bufs->workspace_bytes < uvit_workspace_bytes(cfg)) return fail(UVIT_ERR_WORKSPACE);
    uvit_engine* e = new uvit_engine();
    e->cfg = *cfg; e->buf = *bufs;
    fill_dims(e);
    build_layout(cfg, e->lo);
    Bump b{(char*)bufs->workspace, 0, (size_t)bufs->workspace_bytes};
    plan_workspace(e, b);
    hipStream_t s = (hipStream_t)stream;
    // pad rows of every activation buffer must be (and stay) zero: TN GEMMs reduce over them
    if (hipMemsetAsync(bufs->workspace, 0, b.off, s) != hipSuccess) { delete e; return fail(UVIT_ERR_LAUNCH); }
    // drop-path rates linspace(0, rate, depth)  (modeling_cyclical.py:94-96)
    std::vector<float> rates = dp_rates_linspace(cfg->depth, cfg->drop_path_rate);
    e->dp_rates_host = rates;
    if (const char* v = getenv("UVIT_DP_ROWS")) e->dpl_enable = v[0] != '0';     // A/B switch (uvit_engine_set_drop_path_rows)
    if (const char* v = getenv("UVIT_LS_SAVED_Y")) e->ls_saved_y = v[0] == '1';  // A/B switch and fallback (uvit_engine_set_ls_saved_y)
    // transposed-copy descriptors
    std::vector<TransposeDesc> td;
    int tiles = 0;
    const char* src = (const char*)bufs->params_bf16; char* dst = (char*)bufs->params_bf16_t;
    auto addT = [&](size_t off, int rows, int cols) {
        TransposeDesc d; d.src = src + off * 2; d.dst = dst + off * 2; d.rows = rows; d.cols = cols; d.tile0 = tiles; d.pad = 0;
        tiles += ((rows + 63) / 64) * ((cols + 63) / 64);
        td.push_back(d);
    };
    for (int i = 0; i < cfg->depth; ++i) {
        addT(e->lo.L[i].qkvw, 3 * e->C, e->C); addT(e->lo.L[i].projw[0], e->C, e->C);
        addT(e->lo.L[i].fc1w, e->Hd, e->C); addT(e->lo.L[i].fc2w, e->C, e->Hd);
        if (e->S == 2) addT(e->lo.L[i].projw[1], e->C, e->C);
    }
    for (int st = 0; st < e->S; ++st) addT(e->lo.lmw[st], e->C, e->C);
    e->n_tdesc = (int)td.size(); e->n_ttiles = tiles;
    {
        std::vector<int> idr(e->BP);
        for (int i = 0; i < e->BP; ++i) idr[i] = i;
        const int cnt = e->BP;
        if (hipMemcpyAsync(e->idrows, idr.data(), idr.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(e->idcount, &cnt, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { delete e; return fail(UVIT_ERR_LAUNCH); }
    }
    if (hipMemcpyAsync(e->dp_rates, rates.data(), rates.size() * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(e->tdesc, td.data(), td.size() * sizeof(TransposeDesc), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) { delete e; return fail(UVIT_ERR_LAUNCH); }
    e->slab_started = false; e->last_dropout = false; e->last_seed = 0;
    {
        const char* env = getenv("UVIT_SINGLE_STREAM");
        e->dual = !(env && env[0] == '1');
        // Two second streams: one at the caller's priority, one BELOW it (round 4).  What the second stream carries -- teacher forward,
        // weight gradients, bias-gradient reductions -- is off the critical chain of the step (student forward -> loss -> dgrad chain), and
        // with the lower priority the dispatcher hands free CUs to the critical chain first: 25.41 -> 25.03 ms per step on all 256 CUs
        // (tools/ab.sh, 4 alternating pairs).  With CUs taken away it is the other way round (240 CUs: 28.51 -> 29.21 ms: the 216 wgrad
        // workgroups then queue behind the chain and finish late), so the host selects it for single-GPU runs only
        // (uvit_engine_set_streams(e, 2)); data-parallel runs, where RCCL's channel workgroups hold CUs during backward, keep mode 1.
        int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        bool ok = hipStreamCreateWithFlags(&e->aux_eq, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithPriority(&e->aux_lo, hipStreamNonBlocking, lo) == hipSuccess;
        e->aux = e->aux_eq;
        auto mk = [&](hipEvent_t* ev) { ok = ok && hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess; };
        mk(&e->ev_fork); mk(&e->ev_teacher); mk(&e->ev_ds); mk(&e->ev_x);
        for (int i = 0; i < cfg->depth; ++i) mk(&e->ev_wdone[i]);
        if (!ok) { uvit_engine_destroy(e); return fail(UVIT_ERR_LAUNCH); }
    }
    if (err_out) *err_out = UVIT_OK;
    return e;
}

extern "C" void uvit_engine_destroy(uvit_engine* e) {
    if (!e) return;
    for (hipEvent_t ev : e->prof_ev) (void)hipEventDestroy(ev);
    if (e->aux_eq) { (void)hipStreamSynchronize(e->aux_eq); (void)hipStreamDestroy(e->aux_eq); }
    if (e->aux_lo) { (void)hipStreamSynchronize(e->aux_lo); (void)hipStreamDestroy(e->aux_lo); }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_teacher) (void)hipEventDestroy(e->ev_teacher);
    if (e->ev_ds) (void)hipEventDestroy(e->ev_ds);
    if (e->ev_x) (void)hipEventDestroy(e->ev_x);
    for (int i = 0; i < UVIT_MAX_DEPTH; ++i) if (e->ev_wdone[i]) (void)hipEventDestroy(e->ev_wdone[i]);
    delete e;
}

static int tune_from_abi(const uvit_tuning* t, GemmTune& g) {
    if (!t) { g = GemmTune(); return UVIT_OK; }
    if ((t->nt_variant != 0 && t->nt_variant != 1 && t->nt_variant != 3 && t->nt_variant != 5 && t->nt_variant != 6 && t->nt_variant != 7) ||
        (t->tn_variant != 0 && t->tn_variant != 1 && t->tn_variant != 3) || t->tn_split_target < 0 || t->wgrad_group_chunks < 0 || t->nt_group < 0 || t->nt_group > 64 || (t->nt_persist != 0 && t->nt_persist != 1))
        return UVIT_ERR_ARG;
    g.nt_variant = t->nt_variant; g.tn_variant = t->tn_variant;
    g.tn_target = t->tn_split_target > 0 ? t->tn_split_target : 512; g.group_chunks = t->wgrad_group_chunks; g.nt_group = t->nt_group; g.nt_persist = t->nt_persist;
    return UVIT_OK;
}

extern "C" void uvit_tuning_default(uvit_tuning* out) {
    if (!out) return;
    const GemmTune d;
    out->nt_variant = d.nt_variant; out->tn_variant = d.tn_variant; out->tn_split_target = d.tn_target; out->wgrad_group_chunks = d.group_chunks; out->nt_group = d.nt_group; out->nt_persist = d.nt_persist;
}

extern "C" int uvit_engine_set_tuning(uvit_engine* e, const uvit_tuning* t) {
    if (!e) return UVIT_ERR_ARG;
    return tune_from_abi(t, e->tune);
}

extern "C" int uvit_engine_set_streams(uvit_engine* e, int dual) {
    if (!e || dual < 0 || dual > 2) return UVIT_ERR_ARG;
    // switching streams between steps: whatever the old second stream still holds must be ordered before the new one's work
    hipStream_t next = dual == 2 ? e->aux_lo : e->aux_eq;
    if (next != e->aux && e->aux) HIPCHECK(hipStreamSynchronize(e->aux));
    e->aux = next;
    e->dual = dual != 0;
    return UVIT_OK;
}

extern "C" int uvit_engine_set_drop_path_rows(uvit_engine* e, int on) {
    if (!e) return UVIT_ERR_ARG;
    e->dpl_enable = on != 0;
    return UVIT_OK;
}

extern "C" int uvit_engine_set_ls_saved_y(uvit_engine* e, int on) {
    if (!e) return UVIT_ERR_ARG;
    e->ls_saved_y = on != 0;
    return UVIT_OK;
}

extern "C" int uvit_engine_profile(uvit_engine* e, int enable, int max_launches) {
    if (!e) return UVIT_ERR_ARG;
    if (enable && e->prof_ev.empty()) {
        e->prof_ev.resize((size_t)(max_launches > 0 ? max_launches : 4096) * 2);
        e->prof_kind.assign(e->prof_ev.size() / 2, -1);
        e->prof_rows.assign(e->prof_ev.size() / 2, 0);
        for (auto& ev : e->prof_ev) if (hipEventCreate(&ev) != hipSuccess) return UVIT_ERR_LAUNCH;
    }
    e->prof_on = enable != 0;
    if (enable) e->prof_used = 0;
    return UVIT_OK;
}

// kinds of bracketed launches (full-size forward Linears of a block; the bench line's roofline block names them)
enum { UVIT_PROF_FC1_T = 0, UVIT_PROF_FC1_S = 1, UVIT_PROF_PROJ = 2, UVIT_PROF_FC2 = 3, UVIT_PROF_KINDS = 4 };

// kind < 0: the two fc1 kinds together (the round-1 contract of uvit_engine_profile_read)
extern "C" int uvit_engine_profile_read_kind(uvit_engine* e, int kind, double* total_ms, int* launches, double* flops_per_launch,
                                             double* bytes_per_launch) {
    if (!e || !total_ms || !launches || kind >= UVIT_PROF_KINDS) return UVIT_ERR_ARG;
    double t = 0.0, rows = 0.0; int n = 0;
    for (size_t i = 0; i + 1 < e->prof_used; i += 2) {
        const int k = e->prof_kind[i / 2];
        if (kind < 0 ? (k != UVIT_PROF_FC1_T && k != UVIT_PROF_FC1_S) : k != kind) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e->prof_ev[i], e->prof_ev[i + 1]) != hipSuccess) return UVIT_ERR_LAUNCH;
        t += ms; ++n; rows += e->prof_rows[i / 2];
    }
    *total_ms = t; *launches = n;
    // algorithmic work of ONE launch, at the MEAN row count of the bracketed launches (rows of one stream for proj / fc2, the stacked rows
    // for fc1; compact launches -- drop-path sample lists, the masked-row last block -- run fewer rows than B x tokens)
    const double M1 = n ? rows / n : (double)e->cur_B * e->N, Mall = M1, C = e->C, Hd = e->Hd;
    double fl = 0.0, by = 0.0;
    if (kind < 0 || kind == UVIT_PROF_FC1_T || kind == UVIT_PROF_FC1_S) {
        fl = 2.0 * Mall * Hd * C;
        by = 2.0 * (Mall * C + Hd * C + Mall * Hd * (kind == UVIT_PROF_FC1_T ? 1.0 : kind == UVIT_PROF_FC1_S ? 2.0 : 1.5));
    } else if (kind == UVIT_PROF_PROJ) {
        fl = 2.0 * M1 * C * C;            // bf16 A + W, fp32 residual in and stream out (+ the student's saved bf16 branch output: not counted)
        by = 2.0 * (M1 * C + C * C) + 8.0 * M1 * C;
    } else {
        fl = 2.0 * M1 * C * Hd;
        by = 2.0 * (M1 * Hd + C * Hd) + 8.0 * M1 * C;
    }
    if (flops_per_launch) *flops_per_launch = fl;
    if (bytes_per_launch) *bytes_per_launch = by;
    return UVIT_OK;
}
extern "C" int uvit_engine_profile_read(uvit_engine* e, double* total_ms, int* launches, double* flops_per_launch) {
    return uvit_engine_profile_read_kind(e, -1, total_ms, launches, flops_per_launch, nullptr);
}

extern "C" int uvit_engine_sync_shadows(uvit_engine* e, int which, uvit_stream stream) {
    if (!e) return UVIT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (which & 1) {
        CHECK(uvit_cast_bf16_launch(e->buf.params, e->buf.params_bf16, e->lo.n_total, s));
        CHECK(uvit_transpose_batch_launch(e->tdesc, e->n_tdesc, e->n_ttiles, s));
    }
    if (which & 2) CHECK(uvit_cast_bf16_launch(e->buf.ema, e->buf.ema_bf16, e->lo.n_total, s));
    return UVIT_OK;
}

// ---- forward ----
struct Weights { const float* f; const bf16* b; };
static Weights weights_of(const uvit_engine* e, int which) {      // which = 0: the student's weights, 1: the EMA teacher's
    return which ? Weights{e->buf.ema, (const bf16*)e->buf.ema_bf16} : Weights{e->buf.params, (const bf16*)e->buf.params_bf16};
}

// drop-path draw (and sample list) of (layer, stream, branch): 2 draws per block (base) or 4 (two-stream: mean attn, mean mlp, cov attn,
// cov mlp; modeling_finetune_dist.py:51-55)
static int dp_draw(const uvit_engine* e, int l, int st, int branch) { return 2 * e->S * l + 2 * st + branch; }
static const float* dp_ptr(uvit_engine* e, bool on, int l, int st, int branch, int Bc) {      // the draw's multipliers
    return on ? e->dp_scales + (size_t)dp_draw(e, l, st, branch) * Bc : nullptr;
}

// Drop-path sample lists (base model, training step with drop_path > 0; round 4).  A branch that dropped a sample adds exactly 0 for it in the
// forward and sends exactly 0 back (timm drop_path: x / keep * mask, modeling_finetune.py:51-62), so each branch of the student runs on its
// KEPT samples only: the LayerNorm in front gathers them into compact rows (and copies the dropped samples' rows to the branch's output
// stream), the Linears / the attention core run K * tokens rows, the residual epilogue scatters through the row list, and backward mirrors it.
// The host evaluates the same integer hash as droppath_kernel to size the launches; the lists themselves are built on the device.
struct DpList { const int *pos, *bmap, *rows, *cnt; int K; };
static void dp_list_get(const uvit_engine* e, int l, int st, int branch, DpList& d) {
    const int lb = dp_draw(e, l, st, branch);
    d.pos = e->dpl_pos + (size_t)lb * e->B; d.bmap = e->dpl_bmap + (size_t)lb * e->B;
    d.rows = e->dpl_rows + (size_t)lb * e->dpl_stride; d.cnt = e->dpl_cnt + lb; d.K = e->dpl_K[lb];
}
// The host's evaluation of droppath_kernel (elementwise.hip): kept samples per (layer, draw), draws = 2 (base: attn, mlp) or 4 (two-stream).
// Pure host code -- no device call -- so the CPU test suite pins it against the oracle's drop_path_scales.
static void dp_kept_counts(const float* rates, int depth, int nbr, int B, uint32_t seed, uint32_t it, int* out) {
    for (int l = 0; l < depth; ++l)
        for (int br = 0; br < nbr; ++br) {
            const float r = rates[l];
            int K = B;
            if (r > 0.f) {
                const uint32_t key = uvit_hash32(seed ^ ((it * (uint32_t)nbr * depth + (uint32_t)nbr * l + br + 1u) * 0x9E3779B9u));
                const uint32_t thr = uvit_drop_threshold(r);
                K = 0;
                for (int b = 0; b < B; ++b) K += uvit_hash32((uint32_t)b ^ key) >= thr ? 1 : 0;
            }
            out[nbr * l + br] = K;
        }
}
static std::vector<float> dp_rates_linspace(int depth, float rate) {     // drop-path rates linspace(0, rate, depth)  (modeling_cyclical.py:94-96)
    std::vector<float> rates(depth);
    for (int i = 0; i < depth; ++i) rates[i] = depth > 1 ? (float)((double)rate * i / (depth - 1)) : 0.f;
    return rates;
}
extern "C" int uvit_drop_path_kept_counts(int depth, float drop_path_rate, int draws_per_block, int B, uint32_t seed, uint32_t it,
                                          int32_t* out) {
    if (depth < 1 || depth > UVIT_MAX_DEPTH || (draws_per_block != 2 && draws_per_block != 4) || B < 1 || !out) return UVIT_ERR_ARG;
    const std::vector<float> rates = dp_rates_linspace(depth, drop_path_rate);
    dp_kept_counts(rates.data(), depth, draws_per_block, B, seed, it, out);
    return UVIT_OK;
}
static int dp_lists_begin(uvit_engine* e, uint32_t seed, uint32_t it, int Bc, hipStream_t s) {
    const int depth = e->cfg.depth, nbr = 2 * e->S;
    e->dpl_on = false;
    if (!e->dpl_pos) return UVIT_OK;
    dp_kept_counts(e->dp_rates_host.data(), depth, nbr, Bc, seed, it, e->dpl_K);
    bool any = false;
    for (int i = 0; i < nbr * depth; ++i) {
        const int K = e->dpl_K[i], br = i % nbr;
        any = any || (K > 0 && K < Bc && (e->S == 1 || (br & 1)));
    }
    e->dpl_on = any;
    if (!any) return UVIT_OK;
    return uvit_droppath_lists_launch(e->dp_scales, e->dpl_pos, e->dpl_bmap, e->dpl_rows, e->dpl_cnt, nbr * depth, Bc, e->N,
                                      (int)e->dpl_stride, e->dpl_K, s);
}

// Which rows a Block branch runs on -- one answer for the forward and the backward of a pass:
//   ROWS_ALL     every row, stacked over the S streams (stream st from row st * Mpad);
//   ROWS_LIST    base model, student step: the branch's drop-path sample list, K x tokens compact rows (attention: K samples);
//   ROWS_LIST2   two-stream model, student step, MLP branch: the kept rows of the mean stream, then those of the covariance stream, stacked
//                without a gap (fc1 / fc2 share their weights between the streams; the two-stream attention needs both streams of a sample);
//   ROWS_MASKED  the last block's MLP on the R compact rows of the masked-patch list (base model; student step, and the teacher of a step
//                whose targets take the masked rows only): LN2 gathers them, fc1 / fc2 are R-row GEMMs, the residual epilogue of fc2 reads
//                x_mid and writes x_out / the saved branch output at the listed rows (the other rows of x_out are never read: the head and the
//                final-norm backward go through the same list).
// A list runs when it drops somebody and nobody's list drops everybody (nobody dropped: the dense launches; everybody: dense too, 0 x branch).
enum RowMode { ROWS_ALL, ROWS_LIST, ROWS_LIST2, ROWS_MASKED };
enum Pass { PASS_DENSE, PASS_TEACHER, PASS_STUDENT };     // drop-in forward (as rows: also a dense-target teacher) / teacher of a step / student of a step
struct BranchRows {
    RowMode mode = ROWS_ALL;
    int K = 0;                    // samples of the attention core
    int n[2] = {0, 0};            // rows of each stream
    size_t off[2] = {0, 0};       // first row of each stream in the branch's buffers
    int rows = 0;                 // rows of a launch over the stacked streams: off[S-1] + n[S-1]
    int red = 0;                  // reduction length of the wgrads: rows to the next multiple of 64 (pad rows of every dY are zero)
    DpList d[2] = {};             // ROWS_LIST / ROWS_LIST2: each stream's sample list (zero otherwise)
    const int* rowmap[2] = {nullptr, nullptr};    // row list of each stream's residual epilogue / row-list kernels (null: dense)
    const int* rowcnt[2] = {nullptr, nullptr};
};
static BranchRows branch_rows(const uvit_engine* e, int l, int branch, Pass pass, int Bc) {
    const int S = e->S;
    BranchRows r;
    r.K = Bc; r.n[0] = r.n[1] = Bc * e->N; r.off[1] = e->Mpad;
    if (pass != PASS_DENSE && branch == 1 && l == e->cfg.depth - 1 && e->compact_R > 0) {
        r.mode = ROWS_MASKED; r.n[0] = e->compact_R; r.rowmap[0] = e->rowidx; r.rowcnt[0] = e->count;
    } else if (pass == PASS_STUDENT && e->dpl_on && (S == 1 || branch == 1)) {
        DpList d[2] = {};
        bool none = false, some = false;
        for (int st = 0; st < S; ++st) {
            dp_list_get(e, l, st, branch, d[st]);
            none = none || d[st].K == 0; some = some || d[st].K < e->B;
        }
        if (!none && some) {
            r.mode = S == 1 ? ROWS_LIST : ROWS_LIST2;
            r.K = d[0].K;
            for (int st = 0; st < S; ++st) { r.d[st] = d[st]; r.n[st] = d[st].K * e->N; r.rowmap[st] = d[st].rows; r.rowcnt[st] = d[st].cnt; }
            r.off[1] = r.n[0];
        }
    }
    r.rows = (int)(r.off[S - 1] + r.n[S - 1]);
    r.red = (int)roundup(r.rows, 64);
    return r;
}

// One forward pass, as its three callers name it: the drop-in forward (uvit_engine_forward_features: either weight set, every layer kept), the teacher of
// a step (feeds the target builder) and the student of a step (keeps what backward needs).  fwd_pass derives the rest from the call's inputs, once.
struct Draw { bool on; uint32_t seed, it; };      // train-mode dropout / drop-path of a pass and the (seed, iteration) of its draws
struct FwdPass {
    Pass kind;                      // PASS_DENSE: the drop-in forward
    Pass rows;                      // what branch_rows is asked: the kind, but PASS_DENSE for a teacher whose targets take every patch row
    int which;                      // weight set: 0 student, 1 EMA teacher
    Weights w;
    float* biasP;                   // the weight set's relative-position bias in the attention kernels' layout
    unsigned* tile_cnt;             // the pass's 16 counters of the persistent GEMMs' dynamic tile assignment
    Draw draw;
    bool dp_on; float pdrop;        // drop-path multipliers / attention dropout in effect (train mode and student weights)
    uint32_t aseed;                 // attention-dropout seed of (seed, it); no kernel reads it while pdrop is 0
    int Bc; hipStream_t s;
    const uvit_step_params* hp;     // teacher of a step: the target builder's flags (null otherwise)
    bool dense;                     // ... and whether stream 0's targets go through the dense (batch- / instance-norm) builder
};
static FwdPass fwd_pass(uvit_engine* e, Pass kind, int which, int Bc, Draw draw, const uvit_step_params* hp, hipStream_t s) {
    FwdPass p;
    p.kind = kind; p.which = which; p.w = weights_of(e, which); p.biasP = which ? e->biasP_t : e->biasP_s;
    // The teacher of a step runs beside its student (on the second stream, when there is one): it takes the second block of counters, every
    // other pass the first.  By the role of the call, not by the stream it is given: calls on one engine are stream-ordered (include/uvit.h).
    p.tile_cnt = e->tile_cnt + (kind == PASS_TEACHER ? 16 : 0);
    const bool train = draw.on && !which;
    p.dp_on = train && e->cfg.drop_path_rate > 0.f; p.pdrop = train ? e->cfg.attn_drop_rate : 0.f;
    p.aseed = uvit_hash32(draw.seed ^ (draw.it * 0x85EBCA6Bu + 0x1234567u));
    p.draw = draw; p.Bc = Bc; p.s = s; p.hp = hp;
    p.dense = hp && (hp->target_batch_norm || hp->target_instance_norm || hp->post_target_instance_norm || !hp->target_layer_norm_last);
    p.rows = p.dense ? PASS_DENSE : kind;
    return p;
}

static int forward_layer(uvit_engine* e, const FwdPass& p, int l, const float* x_in, float* x_mid, float* x_out, LayerActs& a) {
    const LayerOff& o = e->lo.L[l];
    const Weights& w = p.w; hipStream_t s = p.s;
    const int Bc = p.Bc, M = Bc * e->N, C = e->C, Hd = e->Hd, S = e->S;
    const size_t Mp = e->Mpad;                                   // row offset of stream 1 in the residual stream
    const bool save = p.kind == PASS_STUDENT;                    // keep what backward needs
    const bool save_y = save && e->ls_saved_step;                // ... the branch outputs among it only on the saved-y path
    const BranchRows at = branch_rows(e, l, 0, p.rows, Bc), ml = branch_rows(e, l, 1, p.rows, Bc);
    LnFwd n1; n1.x = x_in; n1.w = w.f + o.n1w; n1.b = w.f + o.n1b; n1.y = a.ln1; n1.mean = a.mean1; n1.rstd = a.rstd1; n1.M = at.rows; n1.C = C;
    n1.eps = e->cfg.ln_eps;
    if (at.mode == ROWS_LIST) { n1.pos = at.d[0].pos; n1.xcopy = x_mid; n1.tokens = e->N; n1.M = M; }      // the dropped rows copied to x_mid
    CHECK(uvit_ln_fwd_launch(n1, s));
    for (int st = 0; st < S; ++st) {     // same qkv.weight for both streams (modeling_finetune_dist.py:121,127)
        GemmEpi q; q.out = a.qkv + at.off[st] * 3 * C; q.bias = w.f + o.qb[st]; q.bias2 = w.f + o.vb[st]; q.ldo = 3 * C;
        q.tile_counter = p.tile_cnt;
        CHECK(GEMM_NT(st ? EPI_QKV_ELU : EPI_QKV, a.ln1 + at.off[st] * C, w.b + o.qkvw, at.n[st], 3 * C, C, C, C, &q, s));
    }
    if (S == 1) {
        CHECK(uvit_attn_fwd_launch(a.qkv, p.biasP, a.attn, a.lse, at.K, e->H, e->N, e->NP, e->attn_scale, p.pdrop, p.aseed, (uint32_t)l, s, at.d[0].bmap,
                                   e->head_dim));
    } else {
        CHECK(uvit_attn2_fwd_launch(a.qkv, a.qkv + Mp * 3 * C, p.biasP, a.attn, a.attn + Mp * C, a.lse, Bc, e->H, e->N, e->NP, 0.125f,
                                    p.pdrop, p.aseed, (uint32_t)l, s));
    }
    // optional HIP-event brackets around the block's forward Linears, each with the rows of its launch (bench.py's roofline block)
    auto prof_begin = [&](int kind, int rows) -> bool {
        if (!(e->prof_on && e->prof_used + 2 <= e->prof_ev.size())) return false;
        e->prof_kind[e->prof_used / 2] = kind; e->prof_rows[e->prof_used / 2] = rows;
        (void)hipEventRecord(e->prof_ev[e->prof_used], s);
        return true;
    };
    auto prof_end = [&](bool on) { if (on) { (void)hipEventRecord(e->prof_ev[e->prof_used + 1], s); e->prof_used += 2; } };
    for (int st = 0; st < S; ++st) {
        GemmEpi pj; pj.out = x_mid + st * Mp * C; pj.out2 = save_y ? a.projout + st * Mp * C : nullptr; pj.bias = w.f + o.projb[st];
        pj.gamma = w.f + o.g1; pj.resid = x_in + st * Mp * C; pj.rowscale = dp_ptr(e, p.dp_on, l, st, 0, Bc); pj.ldo = C; pj.tokens = e->N;
        pj.rowmap = at.rowmap[st]; pj.rowcount = at.rowcnt[st];
        const bool pp = prof_begin(UVIT_PROF_PROJ, at.n[st]);
        CHECK(GEMM_NT(EPI_RESID, a.attn + at.off[st] * C, w.b + o.projw[st], at.n[st], C, C, C, C, &pj, s));
        prof_end(pp);
    }
    LnFwd n2; n2.x = x_mid; n2.w = w.f + o.n2w; n2.b = w.f + o.n2b; n2.y = a.ln2; n2.mean = a.mean2; n2.rstd = a.rstd2; n2.M = ml.rows; n2.C = C;
    n2.eps = e->cfg.ln_eps;
    if (ml.mode == ROWS_LIST || ml.mode == ROWS_LIST2) {     // each stream's kept rows to its compact rows; the dropped rows copied to x_out
        n2.tokens = e->N; n2.M = M;
        for (int st = 0; st < S; ++st) {
            n2.x = x_mid + st * Mp * C; n2.pos = ml.d[st].pos; n2.xcopy = x_out + st * Mp * C;
            n2.y = a.ln2 + ml.off[st] * C; n2.mean = a.mean2 + ml.off[st]; n2.rstd = a.rstd2 + ml.off[st];
            CHECK(uvit_ln_fwd_launch(n2, s));
        }
    } else {                                                 // every row of the stacked streams, or the masked rows gathered (row map null / set)
        n2.rowidx = ml.rowmap[0]; n2.count = ml.rowcnt[0];
        CHECK(uvit_ln_fwd_launch(n2, s));
    }
    GemmEpi f1; f1.out = a.a; f1.out2 = save ? a.h : nullptr; f1.bias = w.f + o.fc1b; f1.ldo = Hd; f1.tile_counter = p.tile_cnt;
    const bool prof = prof_begin(save ? UVIT_PROF_FC1_S : UVIT_PROF_FC1_T, ml.rows);
    // student (save): a.h receives gelu'(h) -- all that backward needs of h -- computed beside gelu(h)
    CHECK(GEMM_NT(save ? EPI_GELU_DG : EPI_GELU, a.ln2, w.b + o.fc1w, ml.rows, Hd, C, C, C, &f1, s));
    prof_end(prof);
    for (int st = 0; st < S; ++st) {
        GemmEpi f2; f2.out = x_out + st * Mp * C; f2.out2 = save_y ? a.mlpout + st * Mp * C : nullptr; f2.bias = w.f + o.fc2b;
        f2.gamma = w.f + o.g2; f2.resid = x_mid + st * Mp * C; f2.rowscale = dp_ptr(e, p.dp_on, l, st, 1, Bc); f2.ldo = C; f2.tokens = e->N;
        f2.rowmap = ml.rowmap[st]; f2.rowcount = ml.rowcnt[st];
        const bool pf2 = prof_begin(UVIT_PROF_FC2, ml.n[st]);
        CHECK(GEMM_NT(EPI_RESID, a.a + ml.off[st] * Hd, w.b + o.fc2w, ml.n[st], C, Hd, Hd, Hd, &f2, s));
        prof_end(pf2);
    }
    return UVIT_OK;
}

// patch embedding + token assembly into x0 (modeling_cyclical.py:171-192; two-stream: modeling_cyclical_dist.py:106-130)
static int embed(uvit_engine* e, const Weights& w, const int64_t* mask, float* x0, int Bc, hipStream_t s) {
    for (int st = 0; st < e->S; ++st) {
        float* x = x0 + (size_t)st * e->Mpad * e->C;
        GemmEpi pe; pe.out = x; pe.bias = w.f + e->lo.peb[st]; pe.mask = mask; pe.mask_token = w.f + e->lo.mask_tok[st]; pe.ldo = e->C; pe.patches = e->P;
        CHECK(GEMM_NT(EPI_PATCH, e->cols, w.b + e->lo.pew[st], Bc * e->P, e->C, e->Kpe, e->Kpe, e->Kpe, &pe, s));
        CHECK(uvit_set_cls_launch(x, w.f + e->lo.cls[st], nullptr, Bc, e->N, e->C, s));
        // x = x + pos_embed (modeling_cyclical.py:193-194; --abs_pos_emb, off in every BASELINE config)
        if (e->cfg.use_abs_pos_emb) CHECK(uvit_add_pos_launch(x, w.f + e->lo.pos, Bc, e->N, e->C, s));
    }
    return UVIT_OK;
}

// Target builder of a step's teacher pass (engine_for_cyclical.py:92-122): what follows teacher layer l, and the finalisation.
struct TargetBuild { bool dense; int n; };      // FwdPass::dense; target layers accumulated so far
static int targets_after_layer(uvit_engine* e, const FwdPass& p, TargetBuild& t, int l, const float* xout) {
    const uvit_step_params* hp = p.hp; const int Bc = p.Bc; hipStream_t s = p.s;
    if (t.dense && Bc != e->B) return UVIT_ERR_ARG;
    // `[targets[i] for i in target_layers]` (engine_for_cyclical.py:92): a layer listed twice is summed twice and the
    // mean divides by len(target_layers); the host has already mapped negative indices and refused out-of-range ones
    for (int k = 0; k < hp->n_target_layers; ++k) {
        if (hp->target_layers[k] != l) continue;
        const float* sub = hp->layer_results_fc ? e->tXM : nullptr;     // --layer_results fc: x_out - x_mid
        // Stream 0 (the only one of the base model; the MEAN targets of a stochastic step, engine_for_cyclical.py:93-118)
        // takes the dense builder when a batch- / instance-norm variant is on; the covariance targets (:73-86) only know
        // `target_layer_norm_last` and `post_target_layer_norm` and always go through the masked-row builder.
        for (int st = t.dense ? 1 : 0; st < e->S; ++st)
            CHECK(uvit_target_accum_launch(xout + (size_t)st * e->Mpad * e->C, e->rowidx, e->count, e->targets[st], t.n == 0,
                                           Bc * e->P, e->C, 1e-5f, s, sub ? sub + (size_t)st * e->Mpad * e->C : nullptr,
                                           hp->target_layer_norm_last ? 1 : 0));
        if (t.dense) {
            // all patch tokens of this layer -> [batch norm] -> [instance norm] -> [LayerNorm] -> accumulate
            CHECK(uvit_gather_patch_rows_launch(xout, sub, e->dense_v, Bc, e->P, e->C, s));
            if (hp->target_batch_norm) CHECK(uvit_colnorm_launch(e->dense_v, 1, Bc * e->P, e->C, 1e-5f, s));
            if (hp->target_instance_norm) CHECK(uvit_colnorm_launch(e->dense_v, Bc, e->P, e->C, 1e-5f, s));
            if (hp->target_layer_norm_last)
                CHECK(uvit_target_accum_launch(e->dense_v, e->idrows, e->idcount, e->dense_acc, t.n == 0, Bc * e->P, e->C, 1e-5f, s));
            else CHECK(uvit_axpy_rows_launch(e->dense_acc, e->dense_v, t.n == 0, (size_t)Bc * e->P * e->C, s));
        }
        ++t.n;
    }
    return UVIT_OK;
}
static int targets_finalize(uvit_engine* e, const FwdPass& p, const TargetBuild& t) {
    const uvit_step_params* hp = p.hp; const int Bc = p.Bc; hipStream_t s = p.s;
    if (t.n != hp->n_target_layers) return UVIT_ERR_ARG;     // an index outside [0, depth) reached the C ABI
    for (int st = t.dense ? 1 : 0; st < e->S; ++st)
        CHECK(uvit_target_finalize_launch(e->targets[st], e->count, t.n, hp->post_target_layer_norm, Bc * e->P, e->C, 1e-5f, s));
    if (t.dense) {
        const bool pin = hp->post_target_instance_norm != 0;
        CHECK(uvit_target_finalize_launch(e->dense_acc, e->idcount, t.n, hp->post_target_layer_norm && !pin, Bc * e->P, e->C, 1e-5f, s));
        if (pin) {
            CHECK(uvit_colnorm_launch(e->dense_acc, Bc, e->P, e->C, 1e-5f, s));
            if (hp->post_target_layer_norm)
                CHECK(uvit_target_finalize_launch(e->dense_acc, e->idcount, 1, 1, Bc * e->P, e->C, 1e-5f, s));
        }
        CHECK(uvit_gather_masked_rows_launch(e->dense_acc, e->rowidx, e->count, e->targets[0], Bc * e->P, e->P, e->C, s));
    }
    return UVIT_OK;
}

static int run_forward(uvit_engine* e, const FwdPass& p, const float* images, const int64_t* mask) {
    const int Bc = p.Bc; hipStream_t s = p.s;
    if (Bc < 1 || Bc > e->B) return UVIT_ERR_SHAPE;
    // (a step builds the patch columns once, for both of its passes)
    if (p.kind == PASS_DENSE) CHECK(uvit_im2col_launch(images, e->cols, Bc, e->cfg.in_chans, e->cfg.img_size, e->cfg.patch_size, s));
    CHECK(uvit_relpos_gather_launch(e->cfg.use_shared_rel_pos_bias ? p.w.f + e->lo.relt : nullptr, e->buf.rel_index, p.biasP,
                                    e->H, e->N, e->NP, s));
    if (p.dp_on) CHECK(uvit_droppath_launch(e->dp_scales, e->dp_rates, e->cfg.depth, 2 * e->S, Bc, p.draw.seed, p.draw.it, s));
    if (!p.which) {
        e->dpl_on = false;
        if (p.dp_on && p.kind == PASS_STUDENT && e->dpl_enable && Bc == e->B) CHECK(dp_lists_begin(e, p.draw.seed, p.draw.it, Bc, s));
        e->last_dropout = p.draw.on; e->last_seed = p.aseed;
    }
    // the teacher of a step alternates between two residual streams and keeps nothing; every other pass keeps every layer
    const bool keep = p.kind != PASS_TEACHER;
    CHECK(embed(e, p.w, mask, keep ? e->X[0] : e->tX[0], Bc, s));
    TargetBuild tb{p.dense, 0};
    for (int l = 0; l < e->cfg.depth; ++l) {
        float* xout = keep ? e->X[l + 1] : e->tX[(l + 1) & 1];
        CHECK(forward_layer(e, p, l, keep ? e->X[l] : e->tX[l & 1], keep ? e->XM[l] : e->tXM, xout, keep ? e->acts[l] : e->tacts));
        if (!keep) CHECK(targets_after_layer(e, p, tb, l, xout));
    }
    if (!keep) CHECK(targets_finalize(e, p, tb));
    e->cur_B = Bc;
    return UVIT_OK;
}

extern "C" int uvit_engine_forward_features(uvit_engine* e, int which, const float* images, const int64_t* mask, int batch,
                                            int train_dropout, uint32_t seed, uint32_t it, uvit_stream stream) {
    if (!e || !images || (which != 0 && which != 1)) return UVIT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    e->tail_which = -1;
    if (mask) CHECK(uvit_mask_compact_launch(mask, e->rowidx, e->count, batch, e->P, s));
    const FwdPass drop_in = fwd_pass(e, PASS_DENSE, which, batch, Draw{train_dropout != 0, seed, it}, nullptr, s);
    CHECK(run_forward(e, drop_in, images, mask));
    e->tail_which = which; e->tail_B = batch; e->tail_first = e->cfg.depth;
    return UVIT_OK;
}

// Blocks first_layer .. depth-1 again, from the X[first_layer] the last uvit_engine_forward_features left: the stochastic passes of
// MC-dropout.  The pass is the drop-in forward's with two differences: no im2col / embed, and never a drop-path
// draw (the reference's enable_dropout switches Dropout modules to train mode and leaves DropPath in eval).  The attention seed and the
// layer index are fwd_pass's and forward_layer's, so layer l draws the masks it draws in a full forward at (seed, it).
extern "C" int uvit_engine_forward_tail(uvit_engine* e, int which, int batch, int first_layer, int train_dropout, uint32_t seed,
                                        uint32_t it, uvit_stream stream) {
    if (!e || (which != 0 && which != 1)) return UVIT_ERR_ARG;
    if (e->S != 1) return UVIT_ERR_SHAPE;                                     // the base model only
    if (first_layer < 0 || first_layer >= e->cfg.depth) return UVIT_ERR_ARG;
    if (e->tail_which != which || e->tail_B != batch || batch < 1 || batch > e->B) return UVIT_ERR_ARG;      // no forward to continue
    if (first_layer > e->tail_first) return UVIT_ERR_ARG;     // X[first_layer] is an earlier tail's by now, not the forward's
    hipStream_t s = (hipStream_t)stream;
    FwdPass p = fwd_pass(e, PASS_DENSE, which, batch, Draw{train_dropout != 0, seed, it}, nullptr, s);
    p.dp_on = false;
    // biasP of this weight set is the forward's (nothing between the two calls writes it); X[first_layer] is only read
    e->tail_which = -1;                                       // a launch that fails midway leaves no stream to continue
    for (int l = first_layer; l < e->cfg.depth; ++l)
        CHECK(forward_layer(e, p, l, e->X[l], e->XM[l], e->X[l + 1], e->acts[l]));
    e->tail_which = which; e->tail_first = first_layer;
    return UVIT_OK;
}

// final norm (shared) + drop cls + masked-row gather + per-stream head (modeling_cyclical.py:207,215-225)
static int head_forward(uvit_engine* e, const Weights& w, int Bc, int st, bool all_tokens, float* out, hipStream_t s, int rows = 0) {
    const int BP = rows > 0 ? rows : Bc * e->P;        // rows > 0: a host-side bound on the masked rows (training step with n_rows_hint)
    const float* x = e->X[e->cfg.depth] + (size_t)st * e->Mpad * e->C;
    const size_t lmw = e->lo.lmw[st], lmb = e->lo.lmb[st];
    LnFwd fn; fn.x = x; fn.w = w.f + e->lo.normw; fn.b = w.f + e->lo.normb; fn.C = e->C; fn.eps = e->cfg.ln_eps;
    if (all_tokens) {
        // normalise all tokens, then run the head on the patch rows of each sample
        fn.y = e->acts[0].ln1; fn.mean = e->acts[0].mean1; fn.rstd = e->acts[0].rstd1; fn.M = Bc * e->N;
        CHECK(uvit_ln_fwd_launch(fn, s));
        for (int b = 0; b < Bc; ++b) {
            GemmEpi h; h.out = out + (size_t)b * e->P * e->C; h.bias = w.f + lmb; h.ldo = e->C;
            CHECK(GEMM_NT(EPI_F32, e->acts[0].ln1 + ((size_t)b * e->N + 1) * e->C, w.b + lmw, e->P, e->C, e->C,
                                      e->C, e->C, &h, s));
        }
        return UVIT_OK;
    }
    fn.rowidx = e->rowidx; fn.count = e->count; fn.y = e->normed[st]; fn.mean = e->meanF[st]; fn.rstd = e->rstdF[st]; fn.M = BP;
    CHECK(uvit_ln_fwd_launch(fn, s));
    GemmEpi h; h.out = out; h.bias = w.f + lmb; h.ldo = e->C;
    CHECK(GEMM_NT(EPI_F32, e->normed[st], w.b + lmw, BP, e->C, e->C, e->C, e->C, &h, s));
    return UVIT_OK;
}

extern "C" int uvit_engine_head(uvit_engine* e, int which, int all_tokens, float* out, int32_t* count_dev, uvit_stream stream) {
    if (!e || !out) return UVIT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int st = (which >> 1) & 1;                     // bit 1 selects the covariance stream of the two-stream model
    if (st >= e->S) return UVIT_ERR_ARG;
    CHECK(head_forward(e, weights_of(e, which & 1), e->cur_B, st, all_tokens != 0, out, s));
    if (count_dev && !all_tokens) HIPCHECK(hipMemcpyAsync(count_dev, e->count, sizeof(int), hipMemcpyDeviceToDevice, s));
    return UVIT_OK;
}

extern "C" int uvit_engine_compact_rows(uvit_engine* e) { return e ? e->compact_R : 0; }

extern "C" void* uvit_engine_ws_ptr(uvit_engine* e, const char* name, int layer) {
    if (!e || !name) return nullptr;
    const std::string n(name);
    const size_t cov = (size_t)e->Mpad * e->C;           // element offset of the covariance stream in stacked buffers
    if (n == "x" && layer >= 0 && layer <= e->cfg.depth) return e->X[layer];
    if (n == "xm" && layer >= 0 && layer < e->cfg.depth) return e->XM[layer];
    if (n == "x_cov" && e->S == 2 && layer >= 0 && layer <= e->cfg.depth) return e->X[layer] + cov;
    if (n == "xm_cov" && e->S == 2 && layer >= 0 && layer < e->cfg.depth) return e->XM[layer] + cov;
    if (n == "loss") return e->loss;
    if (n == "grad_norm") return e->gnorm;
    if (n == "targets") return e->targets[0];
    if (n == "outputs") return e->outputs[0];
    if (n == "targets_cov" && e->S == 2) return e->targets[1];
    if (n == "outputs_cov" && e->S == 2) return e->outputs[1];
    if (n == "count") return e->count;
    if (n == "dx") return e->dXa;
    if (n == "poisoned") return e->poisoned;
    return nullptr;
}

// ---- training step ----
// Weight gradients dW += dY^T X of n Linears with their bias column sums: ONE launch of the grouped wgrad kernel when every problem
// qualifies (uvit_gemm_tn_group_ok: dimensions multiples of 256, >= 512 reduction rows); otherwise, problem by problem in list order,
// the bias column sums (a two-stream problem's rows from s1_row on into the *_s1 biases) and the plain TN GEMM.  Every bias is a
// replicated no-decay accumulator; the rows between the real tokens and the reduction length are zero in dY, so both paths sum the same.
static int wgrad(uvit_engine* e, const TnProb* p, int n, hipStream_t s) {
    if (uvit_gemm_tn_group_ok(p, n, &e->tune)) return GEMM_TN_GROUP(p, n, s);
    for (int i = 0; i < n; ++i) {
        const TnProb& q = p[i];
        const int r0 = q.s1_row ? q.s1_row : q.M;
        const bf16* y1 = (const bf16*)q.Y + (size_t)r0 * q.ldy;
        if (q.bias) CHECK(uvit_colsum_launch(q.Y, q.ldy, 0, q.bias_end, r0, q.bias, NREP, e->n_nd, s));
        if (q.bias2) CHECK(uvit_colsum_launch(q.Y, q.ldy, q.bias2_begin, q.Nn - q.bias2_begin, r0, q.bias2, NREP, e->n_nd, s));
        if (q.s1_row && q.bias_s1) CHECK(uvit_colsum_launch(y1, q.ldy, 0, q.bias_end, q.M - r0, q.bias_s1, NREP, e->n_nd, s));
        if (q.s1_row && q.bias2_s1) CHECK(uvit_colsum_launch(y1, q.ldy, q.bias2_begin, q.Nn - q.bias2_begin, q.M - r0, q.bias2_s1, NREP, e->n_nd, s));
        CHECK(GEMM_TN(q.Y, q.X, q.M, q.Nn, q.Kk, q.ldy, q.ldx, q.C, q.ldc, 1, s));
    }
    return UVIT_OK;
}

extern "C" int uvit_step_begin(uvit_engine* e, const float* images, const int64_t* mask, const uvit_step_params* hp,
                               uvit_stream stream) {
    if (!e || !images || !mask || !hp || hp->n_target_layers < 1 || hp->n_target_layers > UVIT_MAX_DEPTH) return UVIT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int Bc = e->B, BP = e->BP, C = e->C;
    Layout& lo = e->lo;
    e->tail_which = -1;      // the step's passes overwrite the residual streams a tail would continue
    // every gradient is accumulated (split-K wgrad atomics, bias/LN/gamma column sums): zero the arena once per step.
    // With two streams the ~440 MB of memsets ride on the second stream ahead of the teacher forward (which has slack
    // against the student forward); their first consumers run after the ev_teacher join below.
    hipStream_t ts = e->dual ? e->aux : s;
    if (e->dual) { HIPCHECK(hipEventRecord(e->ev_fork, s)); HIPCHECK(hipStreamWaitEvent(ts, e->ev_fork, 0)); }
    CHECK(uvit_zero_launch(e->buf.grads, lo.n_live * sizeof(float), ts));      // frozen tensors never receive a gradient
    CHECK(uvit_zero_launch(e->grep, (size_t)NREP * e->n_nd * sizeof(float), ts));
    CHECK(uvit_zero_launch(e->loss, 64 * sizeof(float), ts));
    CHECK(uvit_zero_launch(e->dXa, e->rows_alloc() * C * sizeof(float), ts));
    e->slab_started = false; e->bwd_next = e->cfg.depth - 1;
    e->ls_saved_step = e->ls_saved_y;
    // the last block's MLP on the masked rows only (see forward_layer): base model, a row bound from the host, and fewer rows than tokens
    e->compact_R = 0;
    if (e->S == 1 && hp->n_rows_hint > 0) {
        const int R = (int)roundup((size_t)(hp->n_rows_hint < BP ? hp->n_rows_hint : BP), 64);
        if (R >= 512 && R < e->M) {
            e->compact_R = R;
            // its LayerNorm backward writes the residual-stream gradient and the proj branch's dY at the listed rows only: the rest is zero
            CHECK(uvit_zero_launch(e->dXb, e->rows_alloc() * C * sizeof(float), ts));
            CHECK(uvit_zero_launch(e->dY2[(e->cfg.depth - 1) & 1], e->rows_alloc() * C * sizeof(bf16), ts));
        }
    }
    HIPCHECK(hipMemcpyAsync(e->mask_copy, mask, (size_t)BP * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    CHECK(uvit_mask_compact_launch(mask, e->rowidx, e->count, Bc, e->P, s));
    CHECK(uvit_im2col_launch(images, e->cols, Bc, e->cfg.in_chans, e->cfg.img_size, e->cfg.patch_size, s));
    // teacher (EMA weights, eval mode, no grad: engine_for_cyclical.py:68-122) runs on the second stream,
    // beside the student forward (engine_for_cyclical.py:124-128); they share only read-only inputs
    if (e->dual) { HIPCHECK(hipEventRecord(e->ev_fork, s)); HIPCHECK(hipStreamWaitEvent(ts, e->ev_fork, 0)); }   // im2col / mask list
    const FwdPass teacher = fwd_pass(e, PASS_TEACHER, 1, Bc, Draw{false, 0, 0}, hp, ts);
    const FwdPass student = fwd_pass(e, PASS_STUDENT, 0, Bc, Draw{hp->train_dropout != 0, hp->seed, hp->it}, nullptr, s);
    CHECK(run_forward(e, teacher, images, nullptr));
    if (e->dual) HIPCHECK(hipEventRecord(e->ev_teacher, ts));
    CHECK(run_forward(e, student, images, mask));
    const int Rh = e->compact_R > 0 ? e->compact_R : BP;      // rows of the head and of its backward (rows beyond the device-side count are zero)
    for (int st = 0; st < e->S; ++st) CHECK(head_forward(e, student.w, Bc, st, false, e->outputs[st], s, e->compact_R));
    if (e->dual) HIPCHECK(hipStreamWaitEvent(s, e->ev_teacher, 0));
    // loss + dLoss/dOutputs: engine_for_cyclical.py:130-163 (+ WassersteinLoss for the two-stream model, :152-161)
    const float ls = hp->loss_scale == -1.0f ? 1.0f : hp->loss_scale;
    CHECK(uvit_smooth_l1_launch(e->outputs[0], e->targets[0], e->count, hp->l1_beta, hp->l2_loss, ls, e->loss, e->dout[0], BP, C, s));
    if (hp->var_w0 > 0.f)      // variance term on the mean-stream outputs (engine_for_cyclical.py:130-139); std_loss0 -> loss[4]
        CHECK(uvit_variance_loss_launch(e->outputs[0], e->count, hp->var_w0, hp->var_margin0, ls, e->var_scratch, e->loss, e->loss + 4,
                                        e->dout[0], BP, C, s));
    if (e->compact_R > 0) CHECK(uvit_rows_guard_launch(e->count, e->compact_R, e->loss, s));     // more masked rows than the host promised
    if (e->dpl_on) CHECK(uvit_droppath_lists_guard_launch(e->dpl_cnt, 2 * e->S * e->cfg.depth, e->loss, s));   // a sample list that is not the host's
    if (e->S == 2)
        CHECK(uvit_wasserstein_loss_launch(e->outputs[0], e->outputs[1], e->targets[0], e->targets[1], e->count, hp->lambda_pretraining,
                                           ls, e->wl_scratch, e->loss, e->dout[0], e->dout[1], BP, C, s));
    // head backward
    float* g = e->buf.grads;
    const bf16* wt = (const bf16*)e->buf.params_bf16_t;
    for (int st = 0; st < e->S; ++st) {
        const size_t lmw = lo.lmw[st], lmb = lo.lmb[st];
        // lm_head weight gradient + bias column sum: one launch of the grouped wgrad kernel when the shapes qualify (was a column-sum launch
        // and the plain TN kernel, 50 us, on the critical chain between the loss and the first dgrad)
        TnProb hw; hw.Y = e->dout[st]; hw.X = e->normed[st]; hw.C = g + lmw; hw.M = e->compact_R > 0 ? e->compact_R : e->BPpad; hw.Nn = C; hw.Kk = C;
        hw.ldy = C; hw.ldx = C; hw.ldc = C; hw.bias = RP(lmb); hw.bias_end = C;
        CHECK(wgrad(e, &hw, 1, s));
        GemmEpi d; d.out = e->dnormed[st]; d.ldo = C;
        CHECK(GEMM_NT(EPI_BF16, e->dout[st], wt + lmw, Rh, C, C, C, C, &d, s));
        // final LayerNorm backward scattered into the (zeroed) residual-stream gradient
        LnBwd fn; fn.dy = e->dnormed[st]; fn.x = e->X[e->cfg.depth] + (size_t)st * e->Mpad * C; fn.rowidx = e->rowidx; fn.count = e->count;
        fn.mean = e->meanF[st]; fn.rstd = e->rstdF[st]; fn.w = e->buf.params + lo.normw; fn.dx = e->dXa + (size_t)st * e->Mpad * C;
        fn.dw = RP(lo.normw); fn.db = RP(lo.normb); fn.M = Rh; fn.C = C; fn.nrep = NREP; fn.rep_stride = e->n_nd;
        CHECK(uvit_ln_bwd_launch(fn, s));
    }
    return UVIT_OK;
}

extern "C" int uvit_step_backward_layer(uvit_engine* e, int l, const uvit_step_params* hp, uvit_stream stream) {
    if (!e || l < 0 || l >= e->cfg.depth || l != e->bwd_next) return UVIT_ERR_ARG;     // depth-1 .. 0 after uvit_step_begin
    (void)hp;
    e->bwd_next = l - 1;
    hipStream_t s = (hipStream_t)stream;
    const LayerOff& o = e->lo.L[l];
    LayerActs& a = e->acts[l];
    const int M = e->M, C = e->C, Hd = e->Hd, S = e->S;
    const size_t Mp = e->Mpad;
    float* g = e->buf.grads;
    const float* pf = e->buf.params;
    const bf16* wt = (const bf16*)e->buf.params_bf16_t;
    const bool dp_on = e->last_dropout && e->cfg.drop_path_rate > 0.f;
    const float pdrop = e->last_dropout ? e->cfg.attn_drop_rate : 0.f;
    // wgrad GEMMs + bias column sums go to the second stream; the dgrad chain stays on `s`.  The
    // gradient buffers they read are double-buffered by layer parity; before reusing a parity the
    // main stream waits for the wgrad work of layer l+2.
    const int par = l & 1;
    hipStream_t ws = e->dual ? e->aux : s;
    if (e->dual && l + 2 < e->cfg.depth) HIPCHECK(hipStreamWaitEvent(s, e->ev_wdone[l + 2], 0));
    bf16 *dY1 = e->dY1[par], *dY2 = e->dY2[par], *dH = e->dH[par], *dqkv = e->dqkv[par];
    // the rows of each branch, as the forward ran them (branch_rows); compact branches run their row-wise launches to the reduction length,
    // so that the pad rows of the compact dY they write are zero.  The layer below's MLP rows: its LayerScale backward rides in this layer's
    // LayerNorm 1 backward
    const BranchRows at = branch_rows(e, l, 0, PASS_STUDENT, e->B), ml = branch_rows(e, l, 1, PASS_STUDENT, e->B);
    const BranchRows nx = l > 0 ? branch_rows(e, l - 1, 1, PASS_STUDENT, e->B) : BranchRows{};
    const int Mmlp = ml.mode == ROWS_ALL ? ml.rows : ml.red;
    // two-stream model, dense MLP branch: the rows between the mean stream's tokens and the covariance stream's first row (M .. Mpad) are pad
    // rows of the stacked dY1, which the dgrads and wgrads walk.  A stacked-list branch (ROWS_LIST2: the layer above of this parity, or an
    // earlier step) puts the covariance stream's compact rows there, so they are zeroed here rather than assumed to have stayed zero
    if (S == 2 && ml.mode == ROWS_ALL && Mp > (size_t)M) CHECK(uvit_zero_launch(dY1 + (size_t)M * C, (Mp - M) * C * sizeof(bf16), s));
    // weight gradients of the block, launched once the dgrad chain has produced every dY (wgrad)
    TnProb wg[UVIT_TN_GROUP_MAX];
    int nwg = 0;
    {
        TnProb& f2 = wg[nwg++]; f2.Y = dY1; f2.X = a.a; f2.C = g + o.fc2w; f2.M = ml.red; f2.Nn = C; f2.Kk = Hd; f2.ldy = C; f2.ldx = Hd; f2.ldc = Hd;
        TnProb& f1 = wg[nwg++]; f1.Y = dH; f1.X = a.ln2; f1.C = g + o.fc1w; f1.M = ml.red; f1.Nn = Hd; f1.Kk = C; f1.ldy = Hd; f1.ldx = C; f1.ldc = C;
        f1.bias = RP(o.fc1b); f1.bias_end = Hd;
        for (int st = 0; st < S; ++st) {
            TnProb& pj = wg[nwg++]; pj.Y = dY2 + at.off[st] * C; pj.X = a.attn + at.off[st] * C; pj.C = g + o.projw[st];
            pj.M = (int)roundup(at.n[st], 64); pj.Nn = C; pj.Kk = C; pj.ldy = C; pj.ldx = C; pj.ldc = C;
        }
        TnProb& qk = wg[nwg++]; qk.Y = dqkv; qk.X = a.ln1; qk.C = g + o.qkvw; qk.M = at.red; qk.Nn = 3 * C; qk.Kk = C; qk.ldy = 3 * C; qk.ldx = C; qk.ldc = C;
        qk.bias = RP(o.qb[0]); qk.bias_end = C; qk.bias2 = RP(o.vb[0]); qk.bias2_begin = 2 * C;
        // two-stream: the q / v biases differ per stream while the stacked wgrad reduces over both: the token chunks of stream 1
        // (rows from Mpad on) sum into the covariance stream's biases (round 4; was 4 colsum launches per layer)
        if (S == 2) { qk.bias_s1 = RP(o.qb[1]); qk.bias2_s1 = RP(o.vb[1]); qk.s1_row = (int)Mp; }
    }
    // --- MLP branch: x_out = x_mid + dp * gamma2 * fc2(gelu(fc1(ln2(x_mid))))   (weights shared by the streams)
    // (the LayerScale backward of a branch rides in the LayerNorm backward that produces its input -- below the top layer, the MLP branch's
    //  rides in the LayerNorm 1 backward of the layer above; in the two-stream model that kernel is launched once per stream, because
    //  drop-path scales and the proj bias differ per stream)
    // the MLP branch of layer `layer` as the rider of a row-wise backward over stream st: its dY1 is compact by the branch's rows `br`
    const bool saved_y = e->ls_saved_step;      // false: the riders leave dgamma to ls_dgamma (below, behind the wgrad)
    auto mlp_rider = [&](int layer, int st, const BranchRows& br, bf16* dY) {
        const LayerOff& L = e->lo.L[layer];
        LsNext n; n.gamma = pf + L.g2; n.rowscale = dp_ptr(e, dp_on, layer, st, 1, e->B);
        n.dy = dY + br.off[st] * C; n.dbias = RP(L.fc2b); n.tokens = e->N;
        if (saved_y) { n.y = e->acts[layer].mlpout + st * Mp * C; n.dgamma = RP(L.g2); }
        return n;
    };
    if (l == e->cfg.depth - 1)
        for (int st = 0; st < S; ++st)      // a compact branch's last stream runs to the reduction length: the kernel zero-fills the pad rows
            CHECK(uvit_ls_bwd_launch(e->dXa + st * Mp * C, mlp_rider(l, st, ml, dY1), (ml.mode == ROWS_ALL || st + 1 < S) ? ml.n[st] : ml.red - (int)ml.off[st],
                                     C, NREP, e->n_nd, s, ml.rowmap[st], ml.rowcnt[st]));
    GemmEpi d1; d1.out = dH; d1.aux = a.h; d1.ldo = Hd;
    CHECK(GEMM_NT(EPI_MULAUX, dY1, wt + o.fc2w, Mmlp, Hd, C, C, C, &d1, s));      // dH = (dY.W2) * gelu'(h)
    GemmEpi d2; d2.out = e->dLN; d2.ldo = C;
    CHECK(GEMM_NT(EPI_BF16, dH, wt + o.fc1w, Mmlp, C, Hd, Hd, Hd, &d2, s));
    // --- attention branch: x_mid = x_in + dp * gamma1 * proj(attn(ln1(x_in)))   (proj differs per stream)
    // LayerNorm 2 backward + the attention branch's LayerScale backward.  Samples walk: dense, with each branch's sample list (it also
    // zero-fills the pad rows of dY2 and of dqkv: the attention backward writes K samples).  Rows walk: dense, or the row list of the masked-row
    // last block -- dLN / mean / rstd compact, the (zeroed) dense dXb / dY2 written at the listed rows, dY2 compact by the attention list if any
    const bool ln2_samples = ml.mode != ROWS_MASKED && (ml.mode != ROWS_ALL || at.mode == ROWS_LIST);
    for (int st = 0; st < S; ++st) {
        const size_t eo = st * Mp * C;
        LnBwd b; b.dy = e->dLN + ml.off[st] * C; b.x = e->XM[l] + eo; b.mean = a.mean2 + ml.off[st]; b.rstd = a.rstd2 + ml.off[st]; b.w = pf + o.n2w;
        b.dres = e->dXa + eo; b.dx = e->dXb + eo; b.dw = RP(o.n2w); b.db = RP(o.n2b); b.C = C; b.nrep = NREP; b.rep_stride = e->n_nd;
        LsNext& n = b.next;
        n.gamma = pf + o.g1; n.rowscale = dp_ptr(e, dp_on, l, st, 0, e->B); n.dy = dY2 + at.off[st] * C;
        n.dbias = RP(o.projb[st]); n.tokens = e->N; n.pos = at.d[st].pos;
        if (saved_y) { n.y = a.projout + eo; n.dgamma = RP(o.g1); }
        if (ln2_samples) { b.M = M; b.pos = ml.d[st].pos; n.cnt = at.d[st].cnt; if (at.mode == ROWS_LIST) { n.pad2 = dqkv; n.pad2_cols = 3 * C; } }
        else { b.M = ml.n[st]; b.rowidx = ml.rowmap[st]; b.count = ml.rowcnt[st]; }
        CHECK(uvit_ln_bwd_launch(b, s));
    }
    for (int st = 0; st < S; ++st) {
        GemmEpi d3; d3.out = e->dAttn + at.off[st] * C; d3.ldo = C;
        CHECK(GEMM_NT(EPI_BF16, dY2 + at.off[st] * C, wt + o.projw[st], at.n[st], C, C, C, C, &d3, s));
    }
    const float* biasP = e->biasP_s;
    float* slabs = e->cfg.use_shared_rel_pos_bias ? e->slabs : nullptr;
    {
        // fused backward (both model families): every gradient from one recomputation of P; dS (bf16) goes to the parity buffer and
        // its batch reduction into the ONE bias-gradient slab runs on the second stream, beside the dgrad chain.  The parity buffer
        // of layer l was last read by the reduction of layer l + 2, which precedes ev_wdone[l + 2] on that stream (waited for above).
        void* dsw = slabs ? e->ds_ws[par] : nullptr;
        if (S == 1) {
            // (a compact launch writes K samples: the rows up to the wgrad's reduction length are zero-filled by the LayerNorm 2 backward above,
            //  or here in the masked-row last block, whose LayerNorm 2 backward is the row-list kernel)
            if (at.mode == ROWS_LIST && ml.mode == ROWS_MASKED && at.red > at.rows)
                CHECK(uvit_zero_launch(dqkv + (size_t)at.rows * 3 * C, (size_t)(at.red - at.rows) * 3 * C * sizeof(bf16), s));
            CHECK(uvit_attn_bwd_fused_launch(a.qkv, a.attn, e->dAttn, biasP, a.lse, e->delta, dqkv, dsw, dsw != nullptr, at.K, e->H,
                                             e->N, e->NP, e->attn_scale, pdrop, e->last_seed, (uint32_t)l, s, at.d[0].bmap, e->head_dim));
        } else {
            CHECK(uvit_attn2_bwd_launch(a.qkv, a.qkv + Mp * 3 * C, a.attn, a.attn + Mp * C, e->dAttn, e->dAttn + Mp * C, biasP, a.lse,
                                        e->delta, dqkv, dqkv + Mp * 3 * C, dsw, dsw != nullptr, e->B, e->H, e->N, e->NP, 0.125f, pdrop,
                                        e->last_seed, (uint32_t)l, s));
        }
        if (dsw) {
            if (e->dual) { HIPCHECK(hipEventRecord(e->ev_ds, s)); HIPCHECK(hipStreamWaitEvent(ws, e->ev_ds, 0)); }
            if (S == 1) CHECK(uvit_attn_dbias_reduce_launch(dsw, slabs, e->slab_started ? 1 : 0, at.K, e->H, e->N, e->NP, ws));
            else CHECK(uvit_attn2_dbias_reduce_launch(dsw, slabs, e->slab_started ? 1 : 0, e->B, e->H, e->N, e->NP, ws));
        }
    }
    e->slab_started = true;
    if (e->dual) { HIPCHECK(hipEventRecord(e->ev_x, s)); HIPCHECK(hipStreamWaitEvent(ws, e->ev_x, 0)); }    // every dY of the block is there
    CHECK(wgrad(e, wg, nwg, ws));
    if (!saved_y) {
        // LayerScale gradients of the block from its weight gradients (ls_dgamma_kernel), into replica 0 of gamma's accumulators (which
        // uvit_reduce_replicas_launch folds with the rest).  Both riders -- the attention branch's in the LayerNorm 2 backward above, the MLP
        // branch's in the layer above's LayerNorm 1 backward / the top layer's ls_bwd -- precede ev_x, so their dbias sums are complete; W is
        // this step's bf16 shadow (AdamW rewrites it in uvit_step_update).  proj differs per stream and gamma_1 is shared: both streams' terms
        // are summed; fc2 and gamma_2 are shared, with one stacked dW.
        const bf16* wb = (const bf16*)e->buf.params_bf16;
        LsDgammaSet aset[2];
        for (int st = 0; st < S; ++st) aset[st] = LsDgammaSet{wb + o.projw[st], g + o.projw[st], pf + o.projb[st], RP(o.projb[st])};
        CHECK(uvit_ls_dgamma_launch(aset, S, pf + o.g1, RP(o.g1), e->poisoned, C, C, NREP, e->n_nd, ws));
        const LsDgammaSet mset{wb + o.fc2w, g + o.fc2w, pf + o.fc2b, RP(o.fc2b)};
        CHECK(uvit_ls_dgamma_launch(&mset, 1, pf + o.g2, RP(o.g2), e->poisoned, C, Hd, NREP, e->n_nd, ws));
    }
    if (e->dual) HIPCHECK(hipEventRecord(e->ev_wdone[l], ws));
    GemmEpi d4; d4.out = e->dLN; d4.ldo = C;
    CHECK(GEMM_NT(EPI_BF16, dqkv, wt + o.qkvw, at.rows, C, 3 * C, 3 * C, 3 * C, &d4, s));
    // LayerNorm 1 backward + the LayerScale backward of layer l-1's MLP branch into its dY1, of parity (l-1) & 1, last read by the wgrad of
    // layer l+1
    if (l > 0 && e->dual && l + 1 < e->cfg.depth) HIPCHECK(hipStreamWaitEvent(s, e->ev_wdone[l + 1], 0));
    // Samples walk: dense, with the attention list and the list of layer l-1's MLP (two-stream: its stacked compact dY1, the last stream's launch
    // zero-fills the pad rows).  Layer 0 has no rider and no per-stream operand: one launch over the stacked streams
    const bool ln1_samples = at.mode == ROWS_LIST || nx.mode != ROWS_ALL;
    for (int st = 0; st < (l > 0 ? S : 1); ++st) {
        const size_t ro = st * Mp, eo = ro * C;
        LnBwd b; b.dy = e->dLN + eo; b.x = e->X[l] + eo; b.mean = a.mean1 + ro; b.rstd = a.rstd1 + ro; b.w = pf + o.n1w; b.dres = e->dXb + eo;
        b.dx = e->dXa + eo; b.dw = RP(o.n1w); b.db = RP(o.n1b); b.M = l > 0 ? M : (int)e->rows_all(); b.C = C; b.nrep = NREP;
        b.rep_stride = e->n_nd;
        if (ln1_samples) { b.pos = at.d[st].pos; b.next.tokens = e->N; }
        if (l > 0) {
            b.next = mlp_rider(l - 1, st, nx, e->dY1[(l - 1) & 1]);
            b.next.pos = nx.d[st].pos;
            if (st + 1 == S && nx.d[st].cnt) { b.next.cnt = nx.d[st].cnt; b.next.pad_base = (int)nx.off[st]; }
        }
        CHECK(uvit_ln_bwd_launch(b, s));
    }
    return UVIT_OK;
}

extern "C" int uvit_step_backward_embed(uvit_engine* e, uvit_stream stream) {
    if (!e) return UVIT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Layout& lo = e->lo;
    float* g = e->buf.grads;
    const int C = e->C, BP = e->BP;
    // token assembly backward: d cls_token, d mask_token, gradient of the patch-embedding output; then the patch-embedding weight gradient and
    // its bias column sum as ONE grouped launch (end of round 4; was a column-sum launch and the plain TN kernel per stream, 137 us each at the
    // very end of backward) when the shapes qualify
    TnProb pe[2];
    for (int st = 0; st < e->S; ++st) {
        CHECK(uvit_token_bwd_launch(e->dXa + (size_t)st * e->Mpad * C, e->mask_copy, e->dpatch[st], g + lo.cls[st], g + lo.mask_tok[st], e->B, e->P, C, s));
        TnProb& q = pe[st]; q.Y = e->dpatch[st]; q.X = e->cols; q.C = g + lo.pew[st]; q.M = (int)roundup(BP, 64); q.Nn = C; q.Kk = e->Kpe;
        q.ldy = C; q.ldx = e->Kpe; q.ldc = e->Kpe; q.bias = RP(lo.peb[st]); q.bias_end = C;
    }
    CHECK(wgrad(e, pe, e->S, s));
    if (e->cfg.use_abs_pos_emb) CHECK(uvit_pos_bwd_launch(e->dXa, g + lo.pos, e->B, e->N, C, s));     // d pos_embed = sum_b dX[b]
    if (e->dual) HIPCHECK(hipStreamWaitEvent(s, e->ev_wdone[0], 0));   // every wgrad / bias sum / bias-gradient reduction has landed
    if (e->cfg.use_shared_rel_pos_bias && e->slab_started)
        CHECK(uvit_relpos_scatter_launch(e->slabs, 1, e->buf.rel_index, g + lo.relt, e->H, e->N, e->NP, s));
    // fold the replicated column-sum accumulators into the no-decay gradients
    CHECK(uvit_reduce_replicas_launch(e->grep, g + lo.n_decay, e->n_nd, NREP, e->n_nd, s));
    CHECK(uvit_poison_if_nonfinite_launch(e->loss, g + lo.n_decay, e->poisoned, s));     // non-finite loss -> every rank's norm is NaN
    return UVIT_OK;
}

extern "C" int uvit_step_wait_layer_grads(uvit_engine* e, int layer, uvit_stream stream) {
    if (!e || layer < 0 || layer >= e->cfg.depth) return UVIT_ERR_ARG;
    if (e->dual) HIPCHECK(hipStreamWaitEvent((hipStream_t)stream, e->ev_wdone[layer], 0));
    return UVIT_OK;
}

extern "C" int uvit_step_update(uvit_engine* e, const uvit_step_params* hp, uvit_stream stream) {
    if (!e || !hp) return UVIT_ERR_ARG;
    if (hp->sched_dev && (hp->sched_len < 1 || hp->sched_index < 0 || hp->sched_index >= hp->sched_len)) return UVIT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Layout& lo = e->lo;
    // (end of round 4, measured and removed: summing each block's share of the clip norm behind its wgrad on the second stream, which leaves
    //  5 MB instead of 345 MB for this pass -- the 12 streaming launches take CUs from the dgrad chain: 23.76 vs 23.54 ms per step, 4 rotated pairs)
    HIPCHECK(hipMemsetAsync(e->sumsq, 0, sizeof(double), s));
    CHECK(uvit_sumsq_launch(e->buf.grads, lo.n_live, e->sumsq, s));
    const float gs = hp->grad_scale > 0.f ? hp->grad_scale : 1.0f;
    CHECK(uvit_adamw_launch(e->buf.params, e->buf.grads, e->buf.adam_m, e->buf.adam_v, e->buf.params_bf16, lo.n_live, lo.n_decay,
                            hp->lr, hp->weight_decay, hp->beta1, hp->beta2, hp->eps, hp->opt_step, e->sumsq, hp->clip_grad, gs,
                            e->gnorm, s, e->loss, (hp->do_ema || hp->sched_dev) ? e->buf.ema : nullptr, e->buf.ema_bf16, hp->ema_decay, e->poisoned,
                            hp->sched_dev, hp->sched_len, hp->sched_index));
    // (round 4 tried these transposed copies on the second stream, beside the next forward: 24.9-25.2 vs 24.7-25.2 ms per step, no gain; again at the
    //  end of the round with the order-rotated A/B, five pairs: 23.47 vs 23.43 ms)
    CHECK(uvit_transpose_batch_launch(e->tdesc, e->n_tdesc, e->n_ttiles, s));
    // frozen tensors (two-stream cov_qkv.weight) sit behind n_live: AdamW never touches them, the reference's EMA does
    // average them (ModelEmaV2 walks every state-dict value) -- a no-op on values that never change, skipped
    return UVIT_OK;
}

extern "C" int uvit_train_step(uvit_engine* e, const float* images, const int64_t* mask, const uvit_step_params* hp,
                               uvit_stream stream) {
    CHECK(uvit_step_begin(e, images, mask, hp, stream));
    for (int l = e->cfg.depth - 1; l >= 0; --l) CHECK(uvit_step_backward_layer(e, l, hp, stream));
    CHECK(uvit_step_backward_embed(e, stream));
    return uvit_step_update(e, hp, stream);
}

extern "C" int uvit_engine_read_stats_async(uvit_engine* e, float* host_out2, uvit_stream stream) {
    if (!e || !host_out2) return UVIT_ERR_ARG;
    HIPCHECK(hipMemcpyAsync(host_out2, e->loss, 8 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return UVIT_OK;
}

extern "C" int uvit_engine_read_stats(uvit_engine* e, float* host_out2, uvit_stream stream) {
    if (!e || !host_out2) return UVIT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    HIPCHECK(hipMemcpyAsync(host_out2, e->loss, 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return UVIT_OK;
}

// ------------------------------------------------------------------------------------------
// operator-level C ABI (thin wrappers over the internal launchers)
// ------------------------------------------------------------------------------------------
#define S(x) ((hipStream_t)(x))
static GemmEpi epi_from_abi(const uvit_gemm_epilogue* ep) {
    GemmEpi g; g.out = ep->out; g.out2 = ep->out2; g.bias = ep->bias; g.bias2 = ep->bias2; g.gamma = ep->gamma;
    g.resid = ep->resid; g.rowscale = ep->rowscale; g.aux = ep->aux; g.mask = ep->mask; g.mask_token = ep->mask_token;
    g.ldo = ep->ldo; g.tokens = ep->tokens > 0 ? ep->tokens : 1; g.patches = ep->patches > 0 ? ep->patches : 1;
    g.row0 = ep->row0;
    return g;
}
extern "C" int uvit_op_gemm_nt_tuned(int mode, const void* A, const void* W, int M, int N, int K, int lda, int ldw,
                                     const uvit_gemm_epilogue* ep, const uvit_tuning* tune, int* tail_rows, uvit_stream st) {
    if (!A || !W || !ep || !ep->out) return UVIT_ERR_ARG;
    GemmTune tu;
    const int trc = tune_from_abi(tune, tu);
    if (trc) return trc;
    GemmEpi g = epi_from_abi(ep);
    return uvit_gemm_nt_launch(mode, A, W, M, N, K, lda, ldw, &g, S(st), &tu, tail_rows);
}
extern "C" int uvit_op_gemm_nt_plan(int mode, int M, int N, int K, int lda, int ldw, int ldo, int row_list, const uvit_tuning* tune,
                                    int num_cu, uvit_gemm_nt_plan_info* out) {
    if (!out || num_cu <= 0) return UVIT_ERR_ARG;
    GemmTune tu;
    const int trc = tune_from_abi(tune, tu);
    if (trc) return trc;
    NtPlan p;
    const int rc = uvit_gemm_nt_plan(mode, M, N, K, lda, ldw, ldo, row_list != 0, &tu, num_cu, &p);
    if (rc == UVIT_OK) { out->kernel = p.kind; out->rows = p.rows; out->grid = p.grid; out->tail_rows = p.tail_rows; }
    return rc;
}
extern "C" int uvit_op_gemm_nt(int mode, const void* A, const void* W, int M, int N, int K, int lda, int ldw,
                               const uvit_gemm_epilogue* ep, uvit_stream st) {
    return uvit_op_gemm_nt_tuned(mode, A, W, M, N, K, lda, ldw, ep, nullptr, nullptr, st);
}
extern "C" int uvit_op_gemm_nt_sched(int mode, const void* A, const void* W, int M, int N, int K, int lda, int ldw,
                                     const uvit_gemm_epilogue* ep, const uvit_tuning* tune, uint32_t* tile_counters, uvit_stream st) {
    if (!ep || !A || !W || !ep->out) return UVIT_ERR_ARG;
    GemmTune tu;
    const int trc = tune_from_abi(tune, tu);
    if (trc) return trc;
    GemmEpi g = epi_from_abi(ep);
    g.tile_counter = tile_counters;
    return uvit_gemm_nt_launch(mode, A, W, M, N, K, lda, ldw, &g, S(st), &tu, nullptr);
}
extern "C" int uvit_op_wgrad_group(const uvit_wgrad_problem* problems, int count, const uvit_tuning* tune, uvit_stream st) {
    if (!problems || count < 1 || count > UVIT_TN_GROUP_MAX) return UVIT_ERR_ARG;
    GemmTune tu;
    const int trc = tune_from_abi(tune, tu);
    if (trc) return trc;
    TnProb pr[UVIT_TN_GROUP_MAX];
    for (int i = 0; i < count; ++i) {
        const uvit_wgrad_problem& q = problems[i];
        if (!q.Y_bf16 || !q.X_bf16 || !q.C) return UVIT_ERR_ARG;
        pr[i].Y = q.Y_bf16; pr[i].X = q.X_bf16; pr[i].C = q.C; pr[i].bias = q.bias; pr[i].bias2 = q.bias2;
        pr[i].bias_end = q.bias_end; pr[i].bias2_begin = q.bias2_begin;
        pr[i].M = q.M; pr[i].Nn = q.N; pr[i].Kk = q.K; pr[i].ldy = q.ldy; pr[i].ldx = q.ldx; pr[i].ldc = q.ldc;
    }
    return uvit_gemm_tn_group_launch(pr, count, S(st), &tu);
}

extern "C" int uvit_op_gemm_tn(const void* Y, const void* X, int M, int N, int K, int ldy, int ldx, float* C, int ldc,
                               const uvit_tuning* tune, uvit_stream st) {
    if (!Y || !X || !C) return UVIT_ERR_ARG;
    GemmTune tu;
    const int trc = tune_from_abi(tune, tu);
    if (trc) return trc;
    if (hipMemsetAsync(C, 0, (size_t)N * ldc * sizeof(float), S(st)) != hipSuccess) return UVIT_ERR_LAUNCH;
    return uvit_gemm_tn_launch(Y, X, M, N, K, ldy, ldx, C, ldc, 1, S(st), &tu);
}
extern "C" int uvit_op_attn_fwd(const void* qkv, const float* biasP, void* out, float* lse, int B, int H, int N, int NP,
                                float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream st) {
    if (!qkv || !out || !lse) return UVIT_ERR_ARG;
    return uvit_attn_fwd_launch(qkv, biasP, out, lse, B, H, N, NP, scale, p_drop, seed, layer, S(st));
}
extern "C" int64_t uvit_op_attn_bwd_ws_bytes(int B, int H, int N) {
    if (B < 1 || H < 1 || N < 1 || N > 208) return UVIT_ERR_SHAPE;
    return (int64_t)uvit_attn_bwd_fused_ws_bytes(B, H, N);
}
extern "C" int uvit_op_attn_bwd(const void* qkv, const void* o_fwd, const void* d_o, const float* biasP, const float* lse,
                                      float* delta, void* dqkv, float* slab, int acc, void* ds_ws, int B, int H, int N, int NP,
                                      float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream st) {
    if (!qkv || !o_fwd || !d_o || !lse || !delta || !dqkv || (slab && !ds_ws)) return UVIT_ERR_ARG;
    CHECK(uvit_attn_bwd_fused_launch(qkv, o_fwd, d_o, biasP, lse, delta, dqkv, ds_ws, slab != nullptr, B, H, N, NP, scale, p_drop, seed, layer, S(st)));
    if (slab) CHECK(uvit_attn_dbias_reduce_launch(ds_ws, slab, acc, B, H, N, NP, S(st)));
    return UVIT_OK;
}
extern "C" int uvit_op_attn_fwd_hd(const void* qkv, const float* biasP, void* out, float* lse, int B, int H, int N, int NP, int head_dim,
                                   float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream st) {
    if (!qkv || !out || !lse) return UVIT_ERR_ARG;
    if (head_dim != 64 && head_dim != 80) return UVIT_ERR_SHAPE;
    return uvit_attn_fwd_launch(qkv, biasP, out, lse, B, H, N, NP, scale, p_drop, seed, layer, S(st), nullptr, head_dim);
}
extern "C" int uvit_op_attn_bwd_hd(const void* qkv, const void* o_fwd, const void* d_o, const float* biasP, const float* lse,
                                   float* delta, void* dqkv, float* slab, int acc, void* ds_ws, int B, int H, int N, int NP, int head_dim,
                                   float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream st) {
    if (!qkv || !o_fwd || !d_o || !lse || !delta || !dqkv || (slab && !ds_ws)) return UVIT_ERR_ARG;
    if (head_dim != 64 && head_dim != 80) return UVIT_ERR_SHAPE;
    CHECK(uvit_attn_bwd_fused_launch(qkv, o_fwd, d_o, biasP, lse, delta, dqkv, ds_ws, slab != nullptr, B, H, N, NP, scale, p_drop, seed, layer,
                                     S(st), nullptr, head_dim));
    if (slab) CHECK(uvit_attn_dbias_reduce_launch(ds_ws, slab, acc, B, H, N, NP, S(st)));
    return UVIT_OK;
}
extern "C" int uvit_op_attn2_fwd(const void* qkv_m, const void* qkv_c, const float* biasP, void* out_m, void* out_c, float* lse, int B,
                                 int H, int N, int NP, float scale, float p_drop, uint32_t seed, uint32_t layer, uvit_stream st) {
    if (!qkv_m || !qkv_c || !out_m || !out_c || !lse) return UVIT_ERR_ARG;
    return uvit_attn2_fwd_launch(qkv_m, qkv_c, biasP, out_m, out_c, lse, B, H, N, NP, scale, p_drop, seed, layer, S(st));
}
extern "C" int64_t uvit_op_attn2_bwd_ws_bytes(int B, int H, int N) {
    if (B <= 0 || H <= 0 || N <= 0) return UVIT_ERR_SHAPE;
    return (int64_t)uvit_attn2_bwd_ws_bytes(B, H, N);
}
extern "C" int uvit_op_attn2_bwd(const void* qkv_m, const void* qkv_c, const void* o_m, const void* o_c, const void* d_m, const void* d_c,
                                 const float* biasP, const float* lse, float* delta, void* dqkv_m, void* dqkv_c, float* slab, int acc,
                                 void* ds_ws, int B, int H, int N, int NP, float scale, float p_drop, uint32_t seed, uint32_t layer,
                                 uvit_stream st) {
    if (!qkv_m || !qkv_c || !o_m || !o_c || !d_m || !d_c || !lse || !delta || !dqkv_m || !dqkv_c || (slab && !ds_ws)) return UVIT_ERR_ARG;
    CHECK(uvit_attn2_bwd_launch(qkv_m, qkv_c, o_m, o_c, d_m, d_c, biasP, lse, delta, dqkv_m, dqkv_c, ds_ws, slab != nullptr, B, H, N, NP,
                                scale, p_drop, seed, layer, S(st)));
    if (slab) CHECK(uvit_attn2_dbias_reduce_launch(ds_ws, slab, acc, B, H, N, NP, S(st)));
    return UVIT_OK;
}
extern "C" int uvit_op_relpos_gather(const float* t, const int32_t* idx, float* biasP, int H, int N, int NP, uvit_stream st) {
    return uvit_relpos_gather_launch(t, idx, biasP, H, N, NP, S(st));
}
extern "C" int uvit_op_relpos_scatter(const float* slab, int nslab, const int32_t* idx, float* dt, int H, int N, int NP, uvit_stream st) {
    return uvit_relpos_scatter_launch(slab, nslab, idx, dt, H, N, NP, S(st));
}
extern "C" int uvit_op_ln_fwd(const float* x, const float* w, const float* b, void* y, float* mean, float* rstd, int M, int C,
                              float eps, uvit_stream st) {
    LnFwd p; p.x = x; p.w = w; p.b = b; p.y = (bf16*)y; p.mean = mean; p.rstd = rstd; p.M = M; p.C = C; p.eps = eps;
    return uvit_ln_fwd_launch(p, S(st));
}
extern "C" int uvit_op_ln_bwd(const void* dy, const float* x, const float* mean, const float* rstd, const float* w,
                              const float* dres, float* dx, float* dw, float* db, int M, int C, uvit_stream st) {
    LnBwd p; p.dy = (const bf16*)dy; p.x = x; p.mean = mean; p.rstd = rstd; p.w = w; p.dres = dres; p.dx = dx; p.dw = dw; p.db = db; p.M = M; p.C = C;
    return uvit_ln_bwd_launch(p, S(st));
}
// the row-wise kernels in the walks the step launches them in: each wrapper fills the launcher's descriptor, nothing else
static LsNext ls_from_abi(const uvit_ls_rider* r) {
    LsNext n;
    if (!r) return n;
    n.y = (const bf16*)r->y; n.gamma = r->gamma; n.rowscale = r->rowscale; n.dy = (bf16*)r->dy; n.dgamma = r->dgamma; n.dbias = r->dbias;
    n.tokens = r->tokens; n.pos = r->pos; n.cnt = r->cnt; n.pad_base = r->pad_base; n.pad2 = (bf16*)r->pad2; n.pad2_cols = r->pad2_cols;
    return n;
}
extern "C" int uvit_op_ln_fwd_walk(const float* x, const float* w, const float* b, void* y, float* mean, float* rstd, int M, int C, float eps,
                                   const int32_t* rowidx, const int32_t* count, const int32_t* pos, float* xcopy, int tokens, uvit_stream st) {
    if (!x || !w || !b || !y || (!mean != !rstd)) return UVIT_ERR_ARG;
    LnFwd p; p.x = x; p.w = w; p.b = b; p.y = (bf16*)y; p.mean = mean; p.rstd = rstd; p.M = M; p.C = C; p.eps = eps;
    p.rowidx = rowidx; p.count = count; p.pos = pos; p.xcopy = xcopy; p.tokens = tokens;
    return uvit_ln_fwd_launch(p, S(st));
}
extern "C" int uvit_op_ln_bwd_walk(const void* dy, const float* x, const float* mean, const float* rstd, const float* w, const float* dres,
                                   float* dx, float* dw, float* db, int M, int C, int nrep, int64_t rep_stride, const int32_t* rowidx,
                                   const int32_t* count, const int32_t* pos, const uvit_ls_rider* next, uvit_stream st) {
    if (!dy || !x || !mean || !rstd || !w || !dx || !dw || !db || nrep < 1 || rep_stride < 0) return UVIT_ERR_ARG;
    // y and dgamma come together or not at all (both NULL: the rider writes dy / dbias only, uvit_op_ls_dgamma supplies dgamma)
    if (next && next->dy && (!next->gamma || !next->dbias || (!next->y != !next->dgamma))) return UVIT_ERR_ARG;
    LnBwd p; p.dy = (const bf16*)dy; p.x = x; p.mean = mean; p.rstd = rstd; p.w = w; p.dres = dres; p.dx = dx; p.dw = dw; p.db = db;
    p.M = M; p.C = C; p.nrep = nrep; p.rep_stride = (size_t)rep_stride; p.rowidx = rowidx; p.count = count; p.pos = pos;
    p.next = ls_from_abi(next);
    return uvit_ln_bwd_launch(p, S(st));
}
extern "C" int uvit_op_ls_bwd(const float* dx, const uvit_ls_rider* r, int M, int C, int nrep, int64_t rep_stride, const int32_t* rowidx,
                              const int32_t* count, uvit_stream st) {
    if (!dx || !r || !r->gamma || !r->dy || !r->dbias || (!r->y != !r->dgamma) || nrep < 1 || rep_stride < 0) return UVIT_ERR_ARG;
    if (M <= 0 || C <= 0 || r->tokens <= 0) return UVIT_ERR_SHAPE;
    return uvit_ls_bwd_launch(dx, ls_from_abi(r), M, C, nrep, (size_t)rep_stride, S(st), rowidx, count);
}
extern "C" int uvit_op_ls_dgamma(const uvit_ls_dgamma_set* sets, int nsets, const float* gamma, float* dgamma, int32_t* flag, int C, int K,
                                 int nrep, int64_t rep_stride, uvit_stream st) {
    if (!sets || nsets < 1 || nsets > 2 || !gamma || !dgamma || !flag || rep_stride < 0) return UVIT_ERR_ARG;
    LsDgammaSet q[2];
    for (int i = 0; i < nsets; ++i) {
        if (!sets[i].W_bf16 || !sets[i].dW || !sets[i].b || !sets[i].db) return UVIT_ERR_ARG;
        q[i] = LsDgammaSet{(const bf16*)sets[i].W_bf16, sets[i].dW, sets[i].b, sets[i].db};
    }
    return uvit_ls_dgamma_launch(q, nsets, gamma, dgamma, flag, C, K, nrep, (size_t)rep_stride, S(st));
}
extern "C" int uvit_op_colsum(const void* y, int ld, int col0, int ncols, int M, float* out, int nrep, int64_t rep_stride, uvit_stream st) {
    if (!y || !out || nrep < 1 || rep_stride < 0) return UVIT_ERR_ARG;
    if (M <= 0 || ncols <= 0 || col0 < 0 || col0 + ncols > ld) return UVIT_ERR_SHAPE;
    return uvit_colsum_launch(y, ld, col0, ncols, M, out, nrep, (size_t)rep_stride, S(st));
}
extern "C" int uvit_op_reduce_replicas(const float* rep, float* out, int64_t n, int nrep, int64_t stride, uvit_stream st) {
    if (!rep || !out || n < 0 || nrep < 0 || stride < 0) return UVIT_ERR_ARG;
    return uvit_reduce_replicas_launch(rep, out, (size_t)n, nrep, (size_t)stride, S(st));
}
extern "C" int uvit_op_droppath_lists(const float* scales, int32_t* pos, int32_t* bmap, int32_t* rows, int32_t* cnt, int nlists, int B,
                                      int tokens, int rows_stride, const int32_t* host_counts, uvit_stream st) {
    if (!scales || !pos || !bmap || !rows || !cnt || !host_counts || B < 1 || tokens < 1) return UVIT_ERR_ARG;
    return uvit_droppath_lists_launch(scales, pos, bmap, rows, cnt, nlists, B, tokens, rows_stride, host_counts, S(st));
}
extern "C" int uvit_op_gemm_nt_rows(int mode, const void* A, const void* W, int M, int N, int K, int lda, int ldw, const uvit_gemm_epilogue* ep,
                                    const int32_t* rowmap, const int32_t* rowcount, const uvit_tuning* tune, uvit_stream st) {
    if (!A || !W || !ep || !ep->out || !ep->resid || !rowmap || !rowcount || mode != UVIT_EPI_RESID) return UVIT_ERR_ARG;
    GemmTune tu;
    const int trc = tune_from_abi(tune, tu);
    if (trc) return trc;
    GemmEpi g = epi_from_abi(ep);
    g.rowmap = rowmap; g.rowcount = rowcount;
    return uvit_gemm_nt_launch(mode, A, W, M, N, K, lda, ldw, &g, S(st), &tu, nullptr);
}
extern "C" int uvit_op_wgrad_group_split(const uvit_wgrad_problem* problems, const uvit_wgrad_split* split, int count, const uvit_tuning* tune,
                                         uvit_stream st) {
    if (!problems || !split || count < 1 || count > UVIT_TN_GROUP_MAX) return UVIT_ERR_ARG;
    GemmTune tu;
    const int trc = tune_from_abi(tune, tu);
    if (trc) return trc;
    TnProb pr[UVIT_TN_GROUP_MAX];
    for (int i = 0; i < count; ++i) {
        const uvit_wgrad_problem& q = problems[i];
        if (!q.Y_bf16 || !q.X_bf16 || !q.C) return UVIT_ERR_ARG;
        pr[i].Y = q.Y_bf16; pr[i].X = q.X_bf16; pr[i].C = q.C; pr[i].bias = q.bias; pr[i].bias2 = q.bias2;
        pr[i].bias_end = q.bias_end; pr[i].bias2_begin = q.bias2_begin;
        pr[i].M = q.M; pr[i].Nn = q.N; pr[i].Kk = q.K; pr[i].ldy = q.ldy; pr[i].ldx = q.ldx; pr[i].ldc = q.ldc;
        pr[i].bias_s1 = split[i].bias_s1; pr[i].bias2_s1 = split[i].bias2_s1; pr[i].s1_row = split[i].s1_row;
    }
    return uvit_gemm_tn_group_launch(pr, count, S(st), &tu);
}
extern "C" int uvit_op_token_bwd(const float* dx, const int64_t* mask, void* dpatch, float* dcls, float* dmask_token, int B, int P, int C,
                                 uvit_stream st) {
    if (!dx || !mask || !dpatch || !dcls || !dmask_token) return UVIT_ERR_ARG;
    if (B < 1 || P < 1 || C < 1) return UVIT_ERR_SHAPE;
    return uvit_token_bwd_launch(dx, mask, dpatch, dcls, dmask_token, B, P, C, S(st));
}
static_assert(sizeof(uvit_transpose_desc) == sizeof(TransposeDesc), "uvit_transpose_desc mirrors TransposeDesc");
extern "C" int uvit_op_transpose_batch(const uvit_transpose_desc* descs_dev, int ndesc, int total_tiles, uvit_stream st) {
    if (!descs_dev || ndesc < 1 || total_tiles < 1) return UVIT_ERR_ARG;
    return uvit_transpose_batch_launch(descs_dev, ndesc, total_tiles, S(st));
}
extern "C" int uvit_op_ema(float* ema, const float* p, void* eb, int64_t n, float d, uvit_stream st) {
    return uvit_ema_launch(ema, p, eb, (size_t)n, d, S(st));
}
extern "C" int uvit_op_sumsq(const float* g, int64_t n, double* out, uvit_stream st) { return uvit_sumsq_launch(g, (size_t)n, out, S(st)); }
extern "C" int uvit_op_adamw(float* p, const float* g, float* m, float* v, void* pb, int64_t n, int64_t nd, float lr, float wd,
                             float b1, float b2, float eps, int step, const double* sumsq, float max_norm, float gs,
                             float* gn, uvit_stream st) {
    return uvit_adamw_launch(p, g, m, v, pb, (size_t)n, (size_t)nd, lr, wd, b1, b2, eps, step, sumsq, max_norm, gs, gn, S(st));
}
extern "C" int uvit_op_smooth_l1(const float* out, const float* target, const int32_t* count, float beta, int l2, float ls,
                                 float* loss, void* dout, int Mmax, int C, uvit_stream st) {
    return uvit_smooth_l1_launch(out, target, count, beta, l2, ls, loss, dout, Mmax, C, S(st));
}
extern "C" int uvit_op_wasserstein_loss(const float* om, const float* oc, const float* tm, const float* tc, const int32_t* count, float lam,
                                        float ls, float* scratch, float* loss, void* dm, void* dc, int Mmax, int C, uvit_stream st) {
    if (!om || !oc || !tm || !tc || !count || !scratch || !loss || !dm || !dc || Mmax < 1 || C < 1) return UVIT_ERR_ARG;
    return uvit_wasserstein_loss_launch(om, oc, tm, tc, count, lam, ls, scratch, loss, dm, dc, Mmax, C, S(st));
}
extern "C" int uvit_op_variance_loss(const float* out, const int32_t* count, float w, float margin, float ls, float* scratch, float* loss,
                                     float* std_out, void* dout, int Mmax, int C, uvit_stream st) {
    if (!out || !count || !scratch || !loss || !dout) return UVIT_ERR_ARG;
    return uvit_variance_loss_launch(out, count, w, margin, ls, scratch, loss, std_out, dout, Mmax, C, S(st));
}
extern "C" int uvit_op_target_accum(const float* x, const int32_t* rowidx, const int32_t* count, float* acc, int first, int Mmax,
                                    int C, float eps, uvit_stream st) {
    return uvit_target_accum_launch(x, rowidx, count, acc, first, Mmax, C, eps, S(st));
}
extern "C" int uvit_op_target_finalize(float* acc, const int32_t* count, int nl, int post_ln, int Mmax, int C, float eps, uvit_stream st) {
    return uvit_target_finalize_launch(acc, count, nl, post_ln, Mmax, C, eps, S(st));
}
extern "C" int uvit_op_mask_compact(const int64_t* mask, int32_t* rowidx, int32_t* count, int B, int P, uvit_stream st) {
    return uvit_mask_compact_launch(mask, rowidx, count, B, P, S(st));
}
extern "C" int uvit_op_synth_batch(float* images, int64_t* mask, int B, int chans, int img_size, int patches, int n_mask, uint32_t seed,
                                   uint32_t it, uvit_stream st) {
    if (!images && !mask) return UVIT_ERR_ARG;
    return uvit_synth_batch_launch(images, mask, B, chans, img_size, patches, n_mask, seed, it, S(st));
}
extern "C" int uvit_op_im2col(const float* img, void* cols, int B, int Cin, int S_, int p, uvit_stream st) {
    return uvit_im2col_launch(img, cols, B, Cin, S_, p, S(st));
}
extern "C" int uvit_op_droppath(float* sc, const float* rates, int depth, int B, uint32_t seed, uint32_t step, uvit_stream st) {
    return uvit_droppath_launch(sc, rates, depth, 2, B, seed, step, S(st));
}
extern "C" int uvit_op_cast_bf16(const float* src, void* dst, int64_t n, uvit_stream st) { return uvit_cast_bf16_launch(src, dst, (size_t)n, S(st)); }
