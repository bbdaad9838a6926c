// session.h -- what the host files of libemmax_hip.so share (model / session / vision / prefill / step / generate / modes / ops .hip): the
// model and session structs, the error helpers, the KV-cache accessors, the way into and out of the session's stream, and the prototypes of
// the functions that cross files.  Internal: not installed, no device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/emmax.h"
#include "common.h"
#include "kernels.h"

// ---- errors (model.hip) --------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)   // what crosses the host files stays out of the library's exported symbols (as does the last section)
extern thread_local std::string g_err;   // what emmax_last_error reports
int fail(int code, const char* fmt, ...);
#pragma GCC visibility pop
#define HIPCHK(x)                                                                                                   \
    do {                                                                                                            \
        hipError_t e_ = (x);                                                                                        \
        if (e_ != hipSuccess) return fail(EMMAX_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define KCHK(x)                                                                                                     \
    do {                                                                                                            \
        int r_ = (x);                                                                                               \
        if (r_ != 0) return fail(r_ == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s failed (%d) (%s:%d)", #x, r_, __FILE__, __LINE__); \
    } while (0)

static inline int pad_to(int x, int m) { return (x + m - 1) / m * m; }
static const int PAGE = 64;   // KV page: 64 tokens x head_dim bf16 per kv head
static const int EMMAX_LM_BLOCKS = 512;   // persistent lm-head grid: one argmax partial per block (the capacity of a session's partial buffers)

typedef uint16_t bf16;

// Bump plan of the weight arenas and the session workspace.  `base == nullptr` only sizes.  Every tensor is 256-byte aligned.
struct Bump {
    char* base;
    int64_t off = 0;
    void* bytes(int64_t n) {
        off = (off + 255) / 256 * 256;
        void* p = base ? (void*)(base + off) : nullptr;
        off += n;
        return p;
    }
    bf16* take(int64_t elems) { return (bf16*)bytes(elems * 2); }
};

// ---- model ---------------------------------------------------------------------------------------------------------
struct Bound {
    const void* ptr;
    int dtype;
    std::vector<int64_t> shape;
    int64_t numel() const {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

struct BlockW {
    bf16 *n1w, *n1b, *qkv_w, *qkv_b, *proj_w, *proj_b, *ls1, *n2w, *n2b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ls2;
    float *ln1_s, *ln1_c, *ln2_s, *ln2_c;   // LayerNorm folded into qkv / fc1 (kernels.h: GemmParams::ln_*): column sums of W' and the constant term
};
struct TowerW {
    int D, Dp, D3p, M, Mp, N, n_prefix, n_patches, hd, Kpe, n_blocks;
    bf16 *patch_w, *patch_b, *pos, *cls, *reg;
    std::vector<BlockW> blk;
};

// the stages of a decoder layer (the unit the profiler times); the step is stages 0..4 of every layer + the lm-head
enum { STAGE_QKV = 0, STAGE_ATTN = 1, STAGE_OPROJ = 2, STAGE_GATEUP = 3, STAGE_DOWN = 4, STAGE_LMHEAD = 5 };
// bits of the tuning switch fp8_gemv (step.hip: fp8_gemv_mask)
enum { F8_QKV = 1, F8_OPROJ = 2, F8_GATEUP = 4, F8_DOWN = 8, F8_LMHEAD = 16 };

// One decode projection: every copy of its matrix, and how the step launches it (step.hip: launch_proj)
struct ProjW {
    bf16 *rm, *fm;   // row-major (prefill GEMMs, batch 1-2 GEMV); MFMA-fragment-major for the B >= 3 decode path (fp8 mode: e4m3 tiles)
    bf16* km;        // ... in the row order of decode_km.hip (qkv: RoPE pairs, gate-up: (gate, up) pairs inside a 16-row tile); o-proj / down /
                     // lm-head: that kernel reads the natural order -- the same pointer as fm
    bf16* r8;        // fp8 mode: the same e4m3 values as rows in the GEMV's span order (batch 1-2)
    float *sc, *km_sc;      // fp8 mode: per-row scales (null otherwise), and those of km in its row order
    void *tiles, *codes;    // block-scaled modes (WFmt::mx): the tiles in km's row order and their e8m0 scale stream (launch_quant_mx); null otherwise.  rm then
                            // holds the de-quantised values: the prefill evaluates the model the decode step streams
    int gemv_mode, f8bit;   // GEMV_QKV / GEMV_RESID / GEMV_GATEUP / GEMV_LMHEAD, and its bit of the tuning switch fp8_gemv
    int wfmt;               // PW_*: the model's decode weight format
    bool wide;              // MXFP4 mode: the model's mx4_wide (the tiles are served at 17-64 rows too)
};
struct LayerW {
    bf16 *ln1, *ln2;
    ProjW proj[STAGE_DOWN + 1];   // by stage: STAGE_QKV, STAGE_OPROJ, STAGE_GATEUP, STAGE_DOWN
};

struct emmax_model {
    emmax_config cfg;
    std::unordered_map<std::string, Bound> bound;
    bool finalized = false;
    // derived dims
    int H, inter, inter_p, q_dim, kv_dim, qkv_dim, vocab, vocab_p, V, Vp, P1, P1p;
    TowerW tw[2];
    bf16 *pj1_w, *pj1_b, *pj2_w, *pj2_b, *pj3_w, *pj3_b;
    bf16 *embed, *final_norm;
    ProjW lm_head_w = {};
    int wfmt = PW_BF16;          // the decode weight format (kernels.h: WFMT), set once from cfg.decode_fp8.  fp8: e4m3 decode copies; MX4 / MX6:
                                 // block-scaled tiles that decode_km.hip alone reads at 1-16 rows, at every batch
    bool is_mx() const { return wfmt_is_mx(wfmt); }
    const char* wfmt_name() const { return WFMT[wfmt].name; }
    bool mx4_wide = false;       // ... and 17-64 rows on decode_kmp.hip's MX4 form: the tuning switch mx4_wide as it stood at emmax_model_create, frozen
    bool ln_folded = false;      // the ViT LayerNorms are folded into the qkv / fc1 weights (tuning switch gemm_lnfuse at finalize)
    bool aux_built = false;      // the batch >= 3 copies exist (fp8 models: always, they are part of the main arena)
    bool aux_ab = false;         // ... including decode_mfma.hip's qkv / gate-up pair
    std::vector<LayerW> layers;
};

// ---- session -------------------------------------------------------------------------------------------------------
// The small pinned host buffer: the done read-back of emmax_generate, and the staging area that every control upload goes through
// (modes.hip: upload_rows) -- UPLOAD_ROWS rows of the widest parameter set, sampling's four 4-byte columns and its 8-byte seed.
enum { UPLOAD_ROWS = 256, PINNED_BYTES = 4096 * 4 };
struct Pinned {
    int32_t done[EMMAX_MAX_DECODE_BATCH];
    alignas(8) char upload[UPLOAD_ROWS * (4 * 4 + 8)];
};
static_assert(sizeof(Pinned) <= PINNED_BYTES, "the pinned buffer's layout outgrew its allocation");

// SAMPLING (emmax_session_set_sampling; the sampled finish, sample.hip): per-row parameters of every row, staging rows included, and the
// log-probability rows beside out_ids.  Off: none of it is touched and a step launches what a greedy session launches
struct Sampling {
    bool on = false;
    float *t, *p, *logprob /* [rows_total][max_out] */;
    int32_t* k;
    uint64_t* seed;
    uint32_t* sub;
};
// LOGITS PROCESSING (emmax_session_set_processing; the processing finish, sample.hip): per-row repetition penalty, n-gram size and
// min-new-tokens of every row, staging rows included, and each row's prompt ids (every prefill fills them while processing is on).
struct Processing {
    bool on = false;
    float* pen;
    int32_t *ng, *mn, *hist /* [rows_total][max_prompt] */, *hist_len;
};
// WARPERS (emmax_session_set_warpers): per-row min_p / typical_p / epsilon_cutoff / eta_cutoff of every row, staging rows included (0 = off;
// the workspace starts zeroed).  TOKEN RULES (emmax_session_set_token_rules): the session's one rule table behind a device count word, and
// a per-row enable word.  Either on: a step ends in the EXT finish (sample.hip).  Both off: none of it is touched
struct Warpers {
    bool on = false;
    float *minp, *typ, *eps, *eta;
};
struct TokenRules {
    bool on = false;
    bool implied_proc = false;   // the rules turned processing on with neutral values (they read the history): clearing them turns it off again
    int32_t *n /* [1] */, *off /* [EMMAX_MAX_RULES + 1] */, *ids /* [EMMAX_MAX_RULE_TOTAL] */, *flags;
    float* bias;
    uint32_t* en;                // [rows_total]
};
// TOKEN AUTOMATON (emmax_session_set_automaton): the session's one automaton over token classes -- cls [EMMAX_SAMPLE_MAX_V] (the tail stays
// zero: a lane reads four class bytes as a dword), allow [EMMAX_MAX_AUT_STATES][8], next [EMMAX_MAX_AUT_STATES][EMMAX_MAX_AUT_CLASSES] -- at full
// size behind stable pointers, so that another table re-captures nothing; per row, staging rows included, the start state (-1: unconstrained)
// and the state, which every prefill that restarts the row sets to its start.  On: a step ends in the CON finish (sample_con.hip).  Off: none of it
// is touched
struct Automaton {
    bool on = false;
    bool implied_proc = false;   // the automaton turned processing on with neutral values: clearing it turns it off again
    int n_states = 0, n_classes = 0;
    uint8_t* cls;
    uint32_t* allow;
    int16_t* next;
    int32_t *start, *state;      // [rows_total]
};
// SCORES (emmax_session_set_scores): device words {scores, logits, max_new, rows} the processing finish stores through.  Processing or scores
// on: the step runs on the logit rows and ends in the processing finish.  Both off: none of it is touched
struct Scores {
    bool on = false, has_scores = false;
    int rows = 0;   // rows of the bound score buffers: the batch of the first prefill after the binding (0: none yet)
    uint64_t* words;
};
// TOP-N / WATCHED-TOKEN LOG-PROBABILITIES (emmax_session_set_top_logprobs; sample.hip: emmax_top_logprobs_kernel): device words {top_ids,
// top_lp, watch_lp, n_top, n_watch, max_new} naming the caller's buffers, and the session's copy of the watch list.  The host keeps the same
// values: the buffers are columns of session_row_cols, so a commit moves a staged request's entry.  Off: none of it is touched and a step launches what it launches without
struct TopLogprobs {
    bool on = false;
    int n_top = 0, n_watch = 0, max_new = 0;
    int32_t* ids_out = nullptr;
    float *lp_out = nullptr, *watch_out = nullptr;
    uint64_t* words;      // [TOPLP_WORDS]
    int32_t* watch_ids;   // [EMMAX_MAX_WATCH_IDS]
};
// BEAM SEARCH (emmax_session_set_beams; beam.hip): K beams per group, 0 = off.  Rows g K + k are the running beams of group g; the per-row
// candidate lists of a step, HF's running / finished state, the groups' words, the page bookkeeping (spare page and copy list per row), the
// trace [max_out][max_batch] and the resolved result.  Beams off: none of it is touched
struct Beams {
    int K = 0, G = 0, es = 0, lp_pos = 0, eos = -1, max_new = 0;
    bool forked = false, ready = false;
    float *cand_acc, *row_lse, *run, *fin_score, *pw, *tr_score, *tr_lse, *tc_acc, *res_score;
    int32_t *cand_tok, *fin_flag, *fin_t, *fin_par, *fin_tok, *grp, *spare, *csrc, *cdst, *cntok, *tr_tok, *tr_par, *tc_idx, *res_bidx, *res_len;
};

// TAPS (emmax_session_set_pass_taps / emmax_session_set_step_taps; taps.hip): caller-owned fp32 buffers the session fills while it runs a pass it
// would run anyway.  hl / al: the selected hidden states (bit i = HF's hidden_states[i], bit n_layers the normed last) and attention layers.
// pass: consumed by the next prefill or emmax_extend over its packed rows, [n_sel][total_rows][H] and [n_sel][total_rows][Hq][ld];  step: filled by
// every decode step that follows, [max_new][n_sel][B][H] and [max_new][n_sel][B][Hq][ld], indexed by the row's n_out.  serial: counts every binding
// and unbinding -- part of the captured graph's key (the buffers are kernel arguments).  Nothing bound: none of it is touched and every pass launches
// what it launches without
struct TapSet {
    bool on = false;
    float *hidden = nullptr, *attn = nullptr;
    uint64_t hl = 0, al = 0;
    int ld = 0;
};
struct Taps {
    TapSet pass, step;
    int step_max_new = 0, step_B = 0;
    int serial = 0;
};

struct emmax_session {
    emmax_model* m;
    int max_batch, max_prompt, max_ctx, max_pages, max_rows /* packed prefill rows */, max_out;
    // STAGING rows (overlapped admission, emmax_slots_prefill_staged): every per-row array and the paged KV region hold
    // rows_total = max_batch + n_stg rows; rows stg0 .. are never part of a decode batch -- a request is prefilled into them on a
    // second stream while the live rows keep decoding, and emmax_slots_commit moves it into its slot between two decode steps
    // (state copied, page-table rows swapped: no K/V moves)
    int rows_total, stg0, n_stg;
    // vision scratch
    bf16 *vA, *vpe, *vtok, *vln, *vqkv, *vatt, *vmlp, *feats, *pj1, *pj2, *patch_embeds;
    float* vstats;              // LayerNorm (mean, rstd) of every token row, f32 [rows][2]
    int32_t* cu_vit[2];
    // a SECOND set of tower scratch for up to vis2_B frames (round 5): the two towers do not depend on each other, and at small batches each
    // is a chain of under-filled, launch-latency-bound kernels (one frame: ~360 launches of ~14 us) -- tower 1 runs on the session's vision
    // stream beside tower 0 (run_vision; tuning switch vis_streams)
    bf16 *v2A, *v2pe, *v2tok, *v2ln, *v2qkv, *v2att, *v2mlp;
    float *v2stats, *v2splitk_ws;
    int64_t v2splitk_bytes;
    int vis2_B = 0;
    hipStream_t vis_stream = nullptr;
    hipEvent_t ev_vfork = nullptr, ev_vjoin = nullptr;
    // prefill scratch
    bf16 *ph, *pxn, *pqkv, *patt, *pact;
    float* ph32;                // the prefill's residual stream in fp32 (tuning switch resid32 = 1), [max_rows][H]
    bool p32 = false;           // the last prefill ran on ph32 (what emmax_prefill_logits normalises)
    int32_t* cu;
    // decode
    bf16 *dh, *dq, *datt, *dact;
    float* dh32;                // the decode step's residual stream in fp32 (tuning switch resid32; GemvParams::h32), [rows_total][H]
    float *part, *part_val, *part_val2 /* lm-head argmax partials of a staged prefill */;
    // the fp32 logit rows of every row an lm-head can emit into (a staged prefill's rows are its own: it runs beside the live step): what the
    // sampled, processing and beam finishes read
    float* logits;              // f32 [rows_total][vocab]
    Sampling samp;
    Processing proc;
    Warpers warp;
    TokenRules rules;
    Automaton aut;
    Scores scores;
    TopLogprobs toplp;
    Taps taps;
    Beams beam;
    // SAMPLE GROUPS (emmax_session_set_sample_groups; step.hip: run_group_fork): N sampled rows per prefilled prompt, 0 = off.  Rows g N + j are
    // the samples of prompt g; the fork's copy list lives in the beams' (csrc / cdst / cntok: beams and groups exclude each other)
    int grp_N = 0;
    // complete prompt pages the rows of group g share, int32 [groups]: written by the fork (sample groups: run_group_fork; beams: the prefill
    // form of the beam merge), read by the grouped decode attention (step.hip: attn_group_rows)
    int32_t* grp_shared = nullptr;
    // GROUPS IN SLOT SERVING (emmax_slots_fork; generate.hip): a prefilled slot forked into idle slots that read its complete prompt pages.
    // hidden: the pages a follower's table row does not name while it names the owner's, int32 [rows_total][max_pages], -1 = none -- table
    // entries that are a row's own plus hidden entries are a permutation of all page ids at every moment.  fork_*: the upload columns of a
    // fork's sampling parameters (one entry per follower; the fork kernel hands them to the followers' rows)
    int32_t* hidden = nullptr;
    float *fork_t = nullptr, *fork_p = nullptr;
    int32_t* fork_k = nullptr;
    uint64_t* fork_seed = nullptr;
    uint32_t* fork_sub = nullptr;
    // ... host side, per slot: the group it belongs to (-1: none), whether it owns the group's shared pages, how many those are; whether its
    // own logit row is still its prompt's (prefilled in place with sampling on, no step since), and the staged request it was committed from
    std::vector<int> sg_gid, sg_own, sg_nfull, slot_fresh, slot_stg_idx, slot_stg_epoch;
    int sg_next = 0, sg_followers = 0 /* rows that hide pages now */;
    int stg_epoch = 0;          // staged batches so far: a staging row's logit row is its request's until the next emmax_slots_prefill_staged
    bool stg_logits = false;    // ... and was written at all (sampling was on at that staged prefill)
    int32_t *part_idx2;
    int32_t *part_idx, *page_table;
    RowState rows;              // the generation state of every row, staging rows included (kernels.h); with the optional arrays above: session_row_cols
    // EXACT NUMERICS (round 6; tuning switch `exact` at emmax_session_create): fp32 activations end to end.  x32a: the fp32 result of the GEMM
    // in flight (qkv rows, SwiGLU product, fc1 output ...); xhla / xhlb: the two-term bf16 ("HL") A operands, ping-pong; xtok32: the ViT's fp32
    // token rows; xfeats32 / xpe32: fp32 tower features / projected patch embeddings; dq32 / dact32: the decode step's fp32 q rows and SwiGLU
    // product.  The paged KV region holds fp32 rows (twice the bytes of the bf16 cache).
    bool exact = false;
    int kv_fmt = 0;             // KV_BF16 / KV_FP8 / KV_F32 / KV_X24 (kv_format_now() at emmax_session_create)
    long long kv24 = 0;         // KV_X24: elements of one operand's plane of a layer (GemvParams::kv24), else 0
    float *x32a = nullptr, *xtok32 = nullptr, *xfeats32 = nullptr, *xpe32 = nullptr, *dq32 = nullptr, *dact32 = nullptr;
    bf16 *xhla = nullptr, *xhlb = nullptr;
    float* splitk_ws;           // fp32 partial tiles of split-K GEMMs (gemm.hip)
    int64_t splitk_bytes;
    unsigned long long* sk_ws = nullptr;     // device: stream-K granules of the MFMA decode projections (decode_mfma.hip), all zero between launches
    unsigned long long* sk_ws2 = nullptr;    // ... of a STAGED prefill's lm-head: it runs on a second stream beside the live decode steps, and the
                                             // granules are indexed by block id only -- two concurrent launches on one workspace would consume or
                                             // clear each other's partial sums
    int32_t *stop_ids /* [EMMAX_MAX_STOP_IDS] */, *stop_cfg /* {n_trigger, n_after} */;
    bool slots_open = false;    // slot serving mode: rows are independent request slots (emmax_slots_open)
    float *cos_t, *sin_t;
    int n_lm_blocks;
    // kv
    bf16* kv;
    int64_t kv_layer_stride;   // BYTES between layers.  bf16 cache: K at +0, V at +stride/2.  fp8 cache (kv8): K bytes, V bytes, K scales, V scales
    bool kv8 = false;          // the cache holds e4m3 rows + one fp32 scale per (token, kv head) row (tuning switch kv_fp8 at emmax_session_create)
    bf16* kv_stage = nullptr;  // kv8: the step's new K / V rows, bf16 [rows_total][Hkv][2][head_dim] (qkv launch -> attention launch)
    // host state
    int cur_B = 0, total_rows = 0, max_seqlen = 0, vision_B = 0;
    int dec_steps = 0;          // decode steps issued since the last full prefill (upper bound of every row's context growth)
    bool prefilled = false;
    std::vector<int> S;         // per-row prefill lengths
    Pinned* pinned = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    hipStream_t graph_stream_cap = nullptr;  // stream the graphs were captured on
    int graph_B = 0;
    int graph_failed = 0;
    int last_step_graph = 0;   // the most recent decode step was a graph replay (what emmax_session_graph_active reports)
    int last_via = 0;          // launcher family of the most recent projection launch (step.hip: launch_proj; EMMAX_VIA_*)
    // emmax_op_decode_stage (ops.hip): a RowState of its own for the rows it runs -- 8 int32 columns of op_rows rows (ctx_len, cur_tok, done,
    // n_out, max_new, stop_m, stop_after, -) and an output row each -- so that a single stage never touches the session's generation state
    int op_rows = 0;
    int32_t *op_state = nullptr, *op_out = nullptr;
    int32_t* ext_base = nullptr;   // emmax_extend / emmax_slot_extend (extend.hip): the extended rows' cached lengths before the call, int32 [max_batch]
    hipEvent_t ev = nullptr;
    int graph_epoch = -1;      // emmax_tune().epoch the graph was captured under (a changed switch re-captures)
    int graph_grp = 0;    // attn_group_rows() the step was captured under (rows per group of the grouped attention route, 0 = today's launch)
    int graph_taps = 0;   // taps.serial the step was captured under (bound step taps are launches of the step: binding or unbinding re-captures)
    int graph_mode = 0;   // finish_mode() the step was captured under (the parameters and score buffers are device words: a change re-captures nothing)
    hipStream_t own_stream = nullptr;   // where a call made on the (uncapturable) legacy stream runs: StreamScope
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    std::string graph_err;
};

// paged KV region: per layer K and V, rows x pages x kv heads x 64 tokens x head_dim elements -- bf16, or (kv8) e4m3 bytes + a 4-byte scale per row
// format of the paged cache: bf16 rows; e4m3 rows + a scale (kv_fp8); exact numerics: 24-bit rows (exact = 1: a bf16 plane + an 8-bit extension plane per
// operand = the top 24 bits of the fp32 value, 2^-16 relative, 1.5 x the bf16 bytes) or fp32 rows (exact = 2: 2 x the bytes -- the A/B partner)
enum { KV_BF16 = 0, KV_FP8 = 1, KV_F32 = 2, KV_X24 = 3 };
static inline int kv_elem_bytes(int fmt) { return fmt == KV_F32 ? 4 : fmt == KV_X24 ? 3 : fmt == KV_FP8 ? 1 : 2; }
static inline int64_t kv_rows_per_layer(const emmax_model* m, int rows, int max_pages) { return (int64_t)rows * max_pages * m->cfg.n_kv_heads * PAGE; }
static inline char* kv_layer(emmax_session* s, int layer) { return (char*)s->kv + (size_t)layer * s->kv_layer_stride; }
static inline int64_t kv_rows(emmax_session* s) { return kv_rows_per_layer(s->m, s->rows_total, s->max_pages); }
static inline bf16* kcache_of(emmax_session* s, int layer) { return (bf16*)kv_layer(s, layer); }
static inline bf16* vcache_of(emmax_session* s, int layer) { return (bf16*)(kv_layer(s, layer) + kv_rows(s) * s->m->cfg.head_dim * kv_elem_bytes(s->kv_fmt)); }
static inline float* kscale_of(emmax_session* s, int layer) { return (float*)(kv_layer(s, layer) + 2 * kv_rows(s) * s->m->cfg.head_dim); }   // kv8 only
static inline float* vscale_of(emmax_session* s, int layer) { return kscale_of(s, layer) + kv_rows(s); }
// the hidden rows of a decode step: the fp32 stream (tuning switch resid32, the default) or the bf16 rows of rounds 1-4
// (resid32: 0 = bf16 rows everywhere, 1 = fp32 stream in the prefill and the decode step, 2 = in the decode step only)
static inline float* h32_of(emmax_session* s, int slot0 = 0) { return emmax_tune().resid32 ? s->dh32 + (size_t)slot0 * s->m->H : nullptr; }

// ---- the way into the session's stream, and the functions that cross files -----------------------------------------
#pragma GCC visibility push(hidden)
// The way into and out of the session's stream.  The legacy / per-thread default streams cannot be captured: a call made on one of them runs on
// the session's own stream, ordered after everything already queued on the caller's stream (the constructor) and before anything queued on it
// afterwards (leave).  A call that returns early with an error never reaches leave(): the destructor re-joins the caller's stream then, so
// that it does not run ahead of what the call had queued (errors ignored)
class StreamScope {
public:
    StreamScope(emmax_session* s, emmax_stream user) : s_(s), user_((hipStream_t)user), st_(user_) { err_ = enter(); }
    StreamScope(const StreamScope&) = delete;   // (one way in, one way out)
    ~StreamScope() { if (st_ != user_ && hipEventRecord(s_->ev_out, st_) == hipSuccess) (void)hipStreamWaitEvent(user_, s_->ev_out, 0); }
    int error() const { return err_; }   // of the way in: nothing was queued, the call returns it
    hipStream_t stream() const { return st_; }
    int leave() {
        const hipStream_t st = st_;
        st_ = user_;   // joined below, or failing: nothing left for the destructor
        if (st != user_) {
            HIPCHK(hipEventRecord(s_->ev_out, st));
            HIPCHK(hipStreamWaitEvent(user_, s_->ev_out, 0));
        }
        return 0;
    }

private:
    int enter() {
        if ((uintptr_t)user_ > 2) return 0;
        HIPCHK(hipEventRecord(s_->ev_in, user_));
        HIPCHK(hipStreamWaitEvent(s_->own_stream, s_->ev_in, 0));
        st_ = s_->own_stream;
        return 0;
    }
    emmax_session* s_;
    hipStream_t user_, st_;
    int err_;
};

// modes.hip: the checks of emmax_session_set_sampling on n host values (rows: the row each is for, named in the message), and the upload
// of a fork's parameters into the session's fork_* columns
int check_sampling_values(const emmax_session* s, const int32_t* rows, int n, const float* T, const int32_t* top_k, const float* top_p);
int upload_fork_sampling(emmax_session* s, int n, const float* T, const int32_t* top_k, const float* top_p, const uint64_t* seed, const uint32_t* subseq,
                         hipStream_t st);
// modes.hip: the taps' hooks.  idx: HF's hidden_states index (0 = behind the embed / patch splice, i = behind layer i's down projection, n_layers = that
// row normed); each returns 0 at once where its buffer or its bit is not bound.  tap_pass_check: the pass taps against the pass's lengths (EMMAX_ERR_INVALID)
int tap_pass_check(emmax_session* s, int max_keys, const char* who);
int tap_pass_hidden(emmax_session* s, int idx, int total, hipStream_t st);
int tap_pass_attn(emmax_session* s, int li, int B, int total, int max_n, int r0, bool ext, hipStream_t st);
int tap_step_hidden(emmax_session* s, int idx, int B, hipStream_t st);
int tap_step_attn(emmax_session* s, int li, int B, hipStream_t st);
// what ends the mode a binding was made for (slot serving, beams, sample groups, another prefill for the step taps) unbinds
static inline void taps_unbind(emmax_session* s, bool pass, bool step) {
    if (step && s->taps.step.on) s->taps.serial += 1;   // (the pass taps are no part of the captured step)
    if (pass) s->taps.pass = TapSet();
    if (step) s->taps.step = TapSet();
}
// session.hip: the session's per-row device arrays whose owner is on (kernels.h: RowCols) -- what a staged commit moves and, of the inherited
// ones, what a slot fork copies.  A new per-row array is one more line there.  EMMAX_ERR_STATE when the list would outgrow its capacity
int session_row_cols(const emmax_session* s, RowCols* out);
// generate.hip: every hidden page back into its row's table (a permutation again), no slot in a group; what ends or restarts slot serving calls it
int slots_restore_pages(emmax_session* s, hipStream_t st);
// vision.hip: GEMM parameters -- plain; of a session stage (with the session's split-K scratch); of an exact-numerics stage (HL rows in, fp32 out)
GemmParams gp(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K);
GemmParams gps(emmax_session* s, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K);
GemmParams gpx(emmax_session* s, const void* A_hl, int Kp, const void* W, int ldw, float* C, int ldc, int M, int N);
// prefill.hip
int run_prefill(emmax_session* s, const int32_t* ids, const int32_t* lens, int B, int P_max, const void* patches, hipStream_t st, int slot0 = -1);
// the decoder layers over the packed rows + the gather of the last rows; ext != nullptr: the rows extend a cached context (extend_attn.hip)
int run_prefill_layers(emmax_session* s, int B, int total, int maxS, int r0, const ExtendAttnPlan* ext, hipStream_t st);
// extend.hip: what a continuation is not served with, each with its own message (verify.hip refuses the same and more)
int extend_refusals(const emmax_session* s, const char* who);
// extend.hip: lens[b] more tokens on top of the cached context of rows r0 .. r0 + B (slot: a request slot, between two steps)
int run_extend(emmax_session* s, int r0, int B, const int32_t* ids, const int32_t* lens, int P_max, int max_new, bool slot, hipStream_t st);
// step.hip
int model_max_decode_batch(const emmax_model* m, bool exact = false, int* first_stage = nullptr, int* first_B = nullptr);   // the planner: the largest batch every stage has a route for
int session_max_rows(const emmax_session* s);                      // ... of the session's model and numerics
int decode_stage_route(const emmax_model* m, int stage, int B, bool exact);   // EMMAX_VIA_* of the stage's last launch, <= 0: no route
bool decode_batch_served(const emmax_model* m, int B, bool exact);             // the serving policy above 8 rows (step.hip)
const char* decode_stage_name(int stage);
int stage_chunk(int stage, bool exact);                            // rows per launch of a stage (exact numerics: 8; down / lm-head: EMMAX_KMP_ROWS)
bool beam_pages_fit(const emmax_session* s, int S, int max_new);
int launch_beam_finish(emmax_session* s, bool is_prefill, hipStream_t st);
int run_group_fork(emmax_session* s, int G, hipStream_t st);
int run_slots_fork(emmax_session* s, int src, int logit_row, const int32_t* dst, int n, hipStream_t st);   // the device side of emmax_slots_fork
int run_lm_head_step(emmax_session* s, int B, bool is_prefill, float* logits_out, bool do_finish, hipStream_t st, int slot0 = 0);
int run_decode_stage(emmax_session* s, int B, int li, int stage, hipStream_t st);
int decode_oproj_form(const emmax_model* m, bool exact, int B, int* nsplit);
int attn_group_rows(const emmax_session* s, int B);                // rows per group when a B-row step takes the grouped attention route, else 0
int run_decode_step(emmax_session* s, int B, hipStream_t st);
int ensure_graph(emmax_session* s, int B, hipStream_t st);
int launch_graph_step(emmax_session* s, int B, hipStream_t st);
void drop_graph(emmax_session* s);

#pragma GCC visibility pop
