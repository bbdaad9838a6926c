// step.hip -- one decode step: the projection dispatch (launch_proj), the stages of a decoder layer, the lm-head step and the four ways
// a step ends (greedy / sampled / processing / beam finish), and the capture and replay of the step as a hipGraph.
#include "session.h"

// tuning switch streamk = 0 gives every MFMA decode block whole tasks (the split before stream-K)
static bool streamk_on() { return emmax_tune().streamk != 0; }

// tuning switch fp8_gemv = bit mask of the batch 1-2 fp8 projections that run as dot-product GEMV over the e4m3 row copy
// (1 qkv, 2 o-proj, 4 gate/up, 8 down, 16 lm-head); the others go through the MFMA kernels like every larger batch.
// Default (round 3, once the K-split MFMA kernels of decode_km.hip existed): the o-proj, and at batch 1 the lm-head.  Per launch
// at B = 1 / B = 2, row GEMV against decode_km.hip (one box, tools/ab_bench.sh): qkv 14.1 / 17.3 against 12.5 / 12.7 us, gate/up
// 17.9 / 20.3 against 17.1 / 17.1, down (always MFMA) 11.9, o-proj 7.7 / 9.8 against 8.4 / 10.7, lm-head 25.0 / 28.7 against
// 25.7 / 24.4: step 1.939 -> 1.886 ms/token at B = 1 with everything on the MFMA kernels, 2.287 -> 2.028 at B = 2.
static int fp8_gemv_mask(int B) {
    const int mask = emmax_tune().fp8_gemv;
    if (mask >= 0) return mask & 31;
    return B == 1 ? (F8_OPROJ | F8_LMHEAD) : F8_OPROJ;
}

// Which copies of a projection's matrix exist -- flags, not pointers: the planner asks before any arena exists.  copies_of: what a
// ProjW holds now (launch_proj); copies_planned: what the model has or, before emmax_model_build_aux, will have.
// tiles: block-scaled tiles exist, of format wfmt (PW_*); wide: MXFP4 tiles that are served at 17-64 rows too (decode_kmp.hip's MX4 form): the model
// was created under the tuning switch mx4_wide
struct ProjCopies { bool rm, r8, sc, km, fm, tiles; int f8bit, wfmt; bool wide; };
static ProjCopies copies_of(const ProjW& w) { return {w.rm != nullptr, w.r8 != nullptr, w.sc != nullptr, w.km != nullptr, w.fm != nullptr, w.tiles != nullptr, w.f8bit, w.wfmt, w.tiles != nullptr && w.wide}; }
static ProjCopies copies_planned(const emmax_model* m, int stage) {
    // decode_mfma.hip's qkv / gate-up pair: fp8 models always, bf16 models when the aux arena was (or would now be) built with the tuning switch km = 0
    const bool pair = stage == STAGE_QKV || stage == STAGE_GATEUP;
    const bool fp8 = m->wfmt == PW_FP8;
    const bool fm = fp8 || (!m->is_mx() && (!pair || (m->aux_built ? m->aux_ab : emmax_tune().km == 0)));
    const int bit = stage == STAGE_QKV ? F8_QKV : stage == STAGE_OPROJ ? F8_OPROJ : stage == STAGE_GATEUP ? F8_GATEUP : stage == STAGE_DOWN ? F8_DOWN : F8_LMHEAD;
    return {true, fp8, fp8, !m->is_mx(), fm, m->is_mx(), bit, m->wfmt, m->mx4_wide};
}

// Which launcher family takes a projection at B rows (EMMAX_VIA_*), EMMAX_VIA_NONE when none does, ROUTE_NO_FM when only decode_mfma.hip's copy
// (not built) could have.  The order of preference: exact numerics -- the two-term forms or nothing (decode_ks.hip at batch 1-2,
// decode_km.hip's EX kernels at 3-8); MXFP4 / MXFP6 tiles -- decode_km.hip at every batch 1-16, for MXFP4 decode_kmp.hip's MX4 form at 17-64 when the model froze mx4_wide, no other kernel reads them; the fp8 row GEMV at batch
// 1-2 under the fp8_gemv mask; batch >= 3 and fp8: the K-split MFMA kernels (decode_km.hip, 17-64 rows decode_kmp.hip), else decode_mfma.hip;
// else (batch 1-2, bf16) decode_ks.hip, else decode.hip's staged GEMV.  Pure: every question goes to a family's own check, and *g is the
// geometry the chosen family's check returned -- its launcher runs from it without asking again.
enum { ROUTE_NO_FM = -1 };
static int proj_route(const ProjCopies& c, ProjShape s, int B, ProjGeom* g) {
    if (s.exact) {
        s.wfmt = PW_BF16;
        if (c.sc || c.tiles) return EMMAX_VIA_NONE;   // (bf16 weights only: check_exact)
        if (B < EMMAX_MFMA_MIN_BATCH) return decode_ks_takes(s, B, g) ? EMMAX_VIA_KS : EMMAX_VIA_NONE;
        // (at most 8 rows per launch, never decode_kmp.hip; tuning switch km = 0 names decode_mfma.hip, which has no two-term form: nothing)
        return c.km && decode_km_enabled() && decode_km_takes(s, B, g) ? EMMAX_VIA_KM : EMMAX_VIA_NONE;
    }
    if (c.tiles) {
        s.wfmt = c.wfmt;   // (MXFP6 tiles: the same routes at 1-16 rows, no wide form)
        // the MXFP4 down projection runs on the phased kernel only: the K-split form would take K <= 4096, but the format's error lines were
        // measured on the phased kernel alone (policy, not a kernel limit -- the same line emmax_model_create draws)
        if (c.f8bit == F8_DOWN && s.K <= 4096) return EMMAX_VIA_NONE;
        // 17-64 rows: decode_kmp.hip's MX4 form, for a model that froze the tuning switch mx4_wide (decode_km_takes hands them on under the shape's flag)
        s.mx4_wide = c.wide && c.wfmt == PW_MX4;
        if (!decode_km_takes(s, B, g)) return EMMAX_VIA_NONE;
        return B > 16 ? EMMAX_VIA_KMP : EMMAX_VIA_KM;
    }
    s.wfmt = c.sc ? PW_FP8 : PW_BF16;
    if (B < EMMAX_MFMA_MIN_BATCH && c.sc && c.r8 && (fp8_gemv_mask(B) & c.f8bit) && decode_gemv_takes(s, B, g)) return EMMAX_VIA_GEMV_FP8;
    if (B >= EMMAX_MFMA_MIN_BATCH || c.sc) {
        if (c.km && decode_km_enabled() && decode_km_takes(s, B, g)) return B > 16 ? EMMAX_VIA_KMP : EMMAX_VIA_KM;   // (decode_km.hip hands 17-64 rows to decode_kmp.hip)
        if (!c.fm) return ROUTE_NO_FM;
        return decode_mfma_takes(s, B, g) ? EMMAX_VIA_MFMA : EMMAX_VIA_NONE;
    }
    if (decode_ks_enabled() && decode_ks_takes(s, B, g)) return EMMAX_VIA_KS;
    return decode_gemv_takes(s, B, g) ? EMMAX_VIA_GEMV : EMMAX_VIA_NONE;
}

// One projection of the step (ProjW, session.h): route once, point p at the chosen family's copy of the matrix, launch from the route's geometry.
// via (optional): which launcher family took the call (include/emmax.h: EMMAX_VIA_*), what emmax_op_decode_stage reports
static int launch_proj(const ProjW& w, GemvParams& p, int B, hipStream_t st, int* grid_out, int* via = nullptr) {
    const int mode = w.gemv_mode;
    ProjGeom g;
    const int route = proj_route(copies_of(w), proj_shape(mode, p), B, &g);
    if (via) *via = route > 0 ? route : EMMAX_VIA_NONE;
    switch (route) {
        case EMMAX_VIA_KS:
            gemv_set_weights(p, PW_BF16, w.rm);
            return launch_decode_ks(mode, p, B, st, grid_out, &g);
        case EMMAX_VIA_GEMV:
            gemv_set_weights(p, PW_BF16, w.rm);
            return launch_decode_gemv_staged(mode, p, B, g, st, grid_out);
        case EMMAX_VIA_GEMV_FP8:
            gemv_set_weights(p, PW_FP8, w.r8, w.sc);
            p.ldw = p.K;   // bytes per row
            return launch_decode_gemv_staged(mode, p, B, g, st, grid_out);
        case EMMAX_VIA_KM:
        case EMMAX_VIA_KMP:
            if (w.tiles) gemv_set_weights(p, w.wfmt, w.tiles, w.codes);
            else gemv_set_weights(p, w.sc ? PW_FP8 : PW_BF16, w.km, w.km_sc);
            return launch_decode_km(mode, p, B, st, grid_out, &g);
        case EMMAX_VIA_MFMA:
            gemv_set_weights(p, w.sc ? PW_FP8 : PW_BF16, w.fm, w.sc);
            return launch_decode_mfma(mode, p, B, st, grid_out, &g);
        case ROUTE_NO_FM:
            return fail(EMMAX_ERR_STATE, "decode_mfma.hip's copy of this matrix was not built (tuning switch km was 1 at emmax_model_build_aux)");
        default: break;
    }
    if (p.exact) return fail(EMMAX_ERR_INVALID, "exact numerics: no two-term kernel for this projection (batch %d, K %d)", B, p.K);
    if (w.tiles) return fail(EMMAX_ERR_INVALID, "%s decode weights: no kernel for this projection (batch %d of 1-%d, K %d)", WFMT[w.wfmt].name, B, (w.wide && w.wfmt == PW_MX4) ? EMMAX_MAX_DECODE_BATCH : 16, p.K);
    return -1;   // no family takes this shape at this batch
}

// How a stage's rows are split into launches: exact numerics -- chunks of 8 for every projection stage and the lm-head (the two-term MFMA kernels
// hold 8 rows: decode_km.hip EX, the two terms of a row in the sixteen batch columns; each chunk streams the weights again, so the conformance mode
// covers every batch the default path serves at ceil(B / 8) times its weight traffic); otherwise the down projection and the lm-head in chunks of
// EMMAX_KMP_ROWS (33-64 rows: K = 11008 does not fit the eight phases of a four-way split; the argmax partials are laid out per launch); every
// other stage whole.  (The attention launch takes any batch.)
int stage_chunk(int stage, bool exact) {
    return exact ? 8 : (stage == STAGE_DOWN || stage == STAGE_LMHEAD) ? EMMAX_KMP_ROWS : EMMAX_MAX_DECODE_BATCH;
}

// one KV split per (row, head) (batch >= 5 at 32 heads): nothing to merge -- the attention launch normalises and writes the bf16 row
// itself and the o-proj is a plain projection; otherwise the o-proj prologue merges the split partials.
bool attn_direct_rule(int B, int Hkv, bool exact) {
    // exact numerics: the fp32 row in place over the q rows, at batch >= 3 (decode_km.hip's EX o-proj takes fp32 rows; decode_ks.hip's merges the partials)
    if (exact && B < EMMAX_MFMA_MIN_BATCH) return false;
    return decode_attn_nsplit(B, Hkv) == 1 && emmax_tune().attn_direct != 0;
}
static bool attn_direct_on(const emmax_model* m, bool exact, int B) { return attn_direct_rule(B, m->cfg.n_kv_heads, exact); }
static bool attn_direct_on(const emmax_session* s, int B) { return attn_direct_on(s->m, s->exact, B); }

// THE route rule of the grouped attention (decode_attn.hip: launch_group_attn): rows per group when a B-row step of the session, as configured
// now, reads each group's shared prompt pages once, else 0 = the launch of a plain batch.  Groups on (sample groups, or beams behind their
// fork), default numerics, a step whose attention is the one-split direct form, B whole groups of a width the launcher takes, and the tuning
// switch attn_group: 0 never, 1 wherever all of that holds, -1 (default) only at the batches where the two launches were MEASURED faster than
// the one (profiles/group_attn_bench.txt; ms per step at context 768, 32 layers, one launch -> two, spread <= 0.02):
//    8 rows 3.093 -> 3.340   16 rows 3.379 -> 3.557   24 rows 3.794 -> 3.959   40 rows 5.911 -> 6.004      slower: out of the rule
//   32 rows 4.124 -> 4.101 (4 x 8), 4.102 -> 4.066 (2 x 16), 4.230 -> 4.187 (8 x 4)   48 rows 6.232 -> 6.117   64 rows 6.965 -> 6.498 (8 x 8),
//   6.922 -> 6.457 (4 x 16), 7.144 -> 6.513 (16 x 4)                                                       faster: in
// (up to 24 rows the caches serve the rows' repeated reads and the second launch boundary costs more than the bytes; 40 rows = 160 span
// blocks x 2 splits on 256 CUs, a round and a quarter.)  The default rule is those measured shapes and no other: SAMPLE groups of 4 .. 16 rows
// at 32, 48 or 64 rows.  Beams were measured as one K = 8 group only (3.249 -> 3.505, slower) and N = 2 / 3 not at all: they take the route
// under attn_group = 1 alone until someone measures them.  run_decode_stage, ensure_graph and emmax_session_attn_grouped all ask here.
int attn_group_rows(const emmax_session* s, int B) {
    const int N = s->grp_N > 0 ? s->grp_N : (s->beam.K >= 2 && s->beam.forked) ? s->beam.K : 0;
    const int sw = emmax_tune().attn_group;
    if (N < 2 || s->exact || sw == 0 || !attn_direct_on(s, B)) return 0;
    if (sw < 0 && !(s->grp_N >= 4 && s->grp_N <= 16 && (B == 32 || B == 48 || B == 64))) return 0;
    return group_attn_takes(B, N, s->m->cfg.n_heads, s->m->cfg.n_kv_heads) ? N : 0;
}

// what the o-proj of a B-row step reads (emmax_op_decode_stage feeds it): 0 = the bf16 attention rows, 1 = split partials (*nsplit of them per
// (row, head)), 2 = exact numerics, the fp32 rows the one-split attention launch left over the q rows
int decode_oproj_form(const emmax_model* m, bool exact, int B, int* nsplit) {
    const bool direct = attn_direct_on(m, exact, B);
    if (nsplit) *nsplit = direct ? 1 : decode_attn_nsplit(B, m->cfg.n_kv_heads);
    return !direct ? 1 : (exact ? 2 : 0);
}

// The shape of a stage's projection in a B-row step, from the model's dimensions alone (what stage_params / lmhead_params put into GemvParams)
static ProjShape stage_shape(const emmax_model* m, int stage, int B, bool exact) {
    ProjShape s = {};
    s.exact = exact; s.h32 = exact || emmax_tune().resid32 != 0; s.ld_ok = true;   // (every K is a multiple of 64: check_config, derive)
    switch (stage) {
        case STAGE_QKV: s.mode = GEMV_QKV; s.K = m->H; s.n_rows = m->qkv_dim; s.head_dim = m->cfg.head_dim; s.Hq = m->cfg.n_heads; break;
        case STAGE_OPROJ:
            s.mode = GEMV_RESID; s.K = m->q_dim; s.n_rows = m->H;
            if (decode_oproj_form(m, exact, B, &s.nsplit) == 1) { s.attn_part = true; s.Hq = m->cfg.n_heads; }
            break;
        case STAGE_GATEUP: s.mode = GEMV_GATEUP; s.K = m->H; s.n_rows = 2 * m->inter_p; break;
        case STAGE_DOWN: s.mode = GEMV_RESID; s.K = m->inter_p; s.n_rows = m->H; break;
        default: s.mode = GEMV_LMHEAD; s.K = m->H; s.n_rows = m->vocab; s.max_parts = EMMAX_LM_BLOCKS;
    }
    return s;
}

// Steps of more than 8 rows are served in the forms they were built and measured in, whatever else the launchers would take: the ONE-split
// direct attention form (judged at nine rows, as ever: with split partials the bf16 and MXFP4 o-proj have no kernel there, and decode_km.hip's
// fp8 one, which has, is not run at those batches anywhere) and an intermediate size above 4096 (the phased down kernels; a shorter K would go
// through the K-split form, which no test runs as a down projection at 9-64 rows).  Policy, not a kernel limit: widening it is a change of its
// own with GPU coverage at the shapes it opens.  Exact numerics runs 8 rows per launch and is not concerned.
bool decode_batch_served(const emmax_model* m, int B, bool exact) {
    if (exact || B <= 8) return true;
    return emmax_tune().attn_direct != 0 && decode_attn_nsplit(9, m->cfg.n_kv_heads) == 1 && m->inter_p > 4096;
}

// The family that takes the LAST launch of a stage of a B-row step (what emmax_op_decode_stage reports), or EMMAX_VIA_NONE / ROUTE_NO_FM when one
// of the stage's launches has no route or the step is not served at B rows (decode_batch_served).  Host only.
int decode_stage_route(const emmax_model* m, int stage, int B, bool exact) {
    if (!decode_batch_served(m, B, exact)) return EMMAX_VIA_NONE;
    const ProjShape s = stage_shape(m, stage, B, exact);
    const ProjCopies c = copies_planned(m, stage);
    const int chunk = stage_chunk(stage, exact);
    int via = EMMAX_VIA_NONE, n_prev = 0;
    for (int r = 0; r < B && via >= 0; r += chunk) {
        const int n = std::min(chunk, B - r);
        ProjGeom g;
        if (n != n_prev && (via = proj_route(c, s, n, &g)) == EMMAX_VIA_NONE) break;   // (n == n_prev: the same launch again)
        n_prev = n;
    }
    return via;
}

static const int kProjStages[] = {STAGE_QKV, STAGE_OPROJ, STAGE_GATEUP, STAGE_DOWN, STAGE_LMHEAD};
const char* decode_stage_name(int stage) {
    return stage == STAGE_QKV ? "qkv" : stage == STAGE_OPROJ ? "o-proj" : stage == STAGE_GATEUP ? "gate/up" : stage == STAGE_DOWN ? "down" : "lm-head";
}

// The largest B <= EMMAX_MAX_DECODE_BATCH such that every launch of every stage of every step of 1 .. B rows has a route.  It reads tuning
// switches (km, km_down, attn_direct, attn_nsplit ...), so the answer can shrink after a session was created: emmax_session_bytes / create
// check it once, run_prefill and emmax_slots_open again.  first_stage / first_B (optional): the first (stage, batch) without a route
int model_max_decode_batch(const emmax_model* m, bool exact, int* first_stage, int* first_B) {
    for (int B = 1; B <= EMMAX_MAX_DECODE_BATCH; ++B)
        for (int stage : kProjStages)
            if (decode_stage_route(m, stage, B, exact) <= 0) {
                if (first_stage) *first_stage = stage;
                if (first_B) *first_B = B;
                return B - 1;
            }
    return EMMAX_MAX_DECODE_BATCH;
}
int session_max_rows(const emmax_session* s) { return model_max_decode_batch(s->m, s->exact); }

// GemvParams of a projection stage of decoder layer `li` (qkv / o-proj / gate-up / down), as every launcher takes them
static void stage_params(emmax_session* s, int B, int li, int stage, GemvParams& p) {
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    const LayerW& L = m->layers[li];
    memset(&p, 0, sizeof(p));
    p.sk_ws = streamk_on() ? s->sk_ws : nullptr;
    if (stage != STAGE_ATTN) { p.h32 = h32_of(s); p.ldh = m->H; }   // qkv / gate-up read the hidden rows, o-proj / down add into them
    if (s->exact) { p.exact = 1; p.h32 = s->dh32; p.ldh = m->H; }
    switch (stage) {
        case STAGE_QKV:
            p.x = s->dh; p.ldx = m->H; p.ldw = m->H; p.K = m->H; p.norm_w = L.ln1; p.eps = c.rms_eps;
            p.y = s->dq; p.ldy = m->q_dim; p.n_rows = m->qkv_dim;
            p.head_dim = c.head_dim; p.Hq = c.n_heads; p.Hkv = c.n_kv_heads; p.page = PAGE; p.max_pages = s->max_pages;
            p.ctx_len = s->rows.ctx_len; p.page_table = s->page_table; p.cos_t = s->cos_t; p.sin_t = s->sin_t;
            p.kcache = kcache_of(s, li); p.vcache = vcache_of(s, li);
            p.kv_stage = s->kv8 ? s->kv_stage : nullptr;   // fp8 KV cache: the new rows wait as bf16 for the attention launch
            if (s->exact) { p.y = s->dq32; p.kv24 = s->kv24; }   // fp32 q rows; kcache / vcache are the 24-bit (or fp32) cache
            break;
        case STAGE_OPROJ:
            p.x = s->datt; p.ldx = m->q_dim; p.ldw = m->q_dim; p.K = m->q_dim; p.y = s->dh; p.ldy = m->H; p.n_rows = m->H;
            if (!attn_direct_on(s, B)) {   // split merge fused into the staging
                p.attn_part = s->part; p.nsplit = decode_attn_nsplit(B, c.n_kv_heads); p.Hq = c.n_heads;
            } else if (s->exact) {
                p.x = s->dq32;             // the attention launch left the normalised fp32 rows in place of the q rows
            }
            break;
        case STAGE_GATEUP:
            p.x = s->dh; p.ldx = m->H; p.ldw = m->H; p.K = m->H; p.norm_w = L.ln2; p.eps = c.rms_eps;
            p.y = s->dact; p.ldy = m->inter_p; p.n_rows = 2 * m->inter_p;
            if (s->exact) p.y = s->dact32;
            break;
        case STAGE_DOWN:
            p.x = s->dact; p.ldx = m->inter_p; p.ldw = m->inter_p; p.K = m->inter_p; p.y = s->dh; p.ldy = m->H; p.n_rows = m->H;
            if (s->exact) p.x = s->dact32;
            break;
        default: break;
    }
}
static void lmhead_params(emmax_session* s, int slot0, float* logits_out, GemvParams& p) {
    emmax_model* m = s->m;
    memset(&p, 0, sizeof(p));
    p.sk_ws = streamk_on() ? (slot0 >= s->stg0 ? s->sk_ws2 : s->sk_ws) : nullptr;
    p.x = s->dh + (size_t)slot0 * m->H; p.ldx = m->H; p.ldw = m->H; p.K = m->H; p.norm_w = m->final_norm; p.eps = m->cfg.rms_eps;
    p.h32 = h32_of(s, slot0); p.ldh = m->H;
    if (s->exact) { p.exact = 1; p.h32 = s->dh32 + (size_t)slot0 * m->H; }
    const bool stg = slot0 >= s->stg0;
    p.n_rows = m->vocab; p.max_parts = s->n_lm_blocks; p.part_val = stg ? s->part_val2 : s->part_val; p.part_idx = stg ? s->part_idx2 : s->part_idx;
    p.logits_out = logits_out;
}

// how a step ends (the captured graph is keyed on it: the finish's parameters differ in each): bit 0 sampling, bit 1 processing, bit 2
// scores.  0: the greedy finish (lm-head argmax partials); 1: the sampled finish; bit 1 or 2 set: the processing finish
// beams on: bit 3, stop_on_eos in bit 4, K and the early-stopping mode above (the beam finish holds them by value)
// warpers or token rules on (bits 13, 14): the EXT finish; top-N / watched log-probabilities bound (bit 15): their launch ahead of the finish
// a token automaton set (bit 16): the CON finish
enum { FINISH_TOPLP = 1 << 15, FINISH_WARP = 1 << 13, FINISH_RULES = 1 << 14, FINISH_AUT = 1 << 16, FINISH_EXT = FINISH_WARP | FINISH_RULES | FINISH_AUT,
       FINISH_ROWS = 6 | FINISH_EXT /* runs on the logit rows */ };
static int finish_mode(const emmax_session* s) {
    return (s->samp.on ? 1 : 0) | (s->proc.on ? 2 : 0) | (s->scores.on ? 4 : 0) |
           (s->beam.K ? (8 | (s->beam.eos >= 0 ? 16 : 0) | (s->beam.K << 5) | (s->beam.es << 10) | (s->beam.lp_pos << 12)) : 0) |
           (s->warp.on ? FINISH_WARP : 0) | (s->rules.on ? FINISH_RULES : 0) | (s->toplp.on ? FINISH_TOPLP : 0) |
           (s->aut.on ? FINISH_AUT : 0);
}

// the per-row state of rows slot0 .. slot0 + B that a finish updates
static void finish_rows(emmax_session* s, int B, bool is_prefill, int slot0, FinishParams& f) {
    emmax_model* m = s->m;
    const RowState r = s->rows.from(slot0, s->max_out);
    f.B = B;
    f.cur_tok = r.cur_tok; f.ctx_len = r.ctx_len; f.done = r.done; f.n_out = r.n_out; f.out_ids = r.out_ids;
    f.max_new_p = r.max_new; f.max_out = s->max_out; f.max_ctx = s->max_ctx;
    f.stop_ids = s->stop_ids; f.stop_cfg = s->stop_cfg; f.stop_m = r.stop_m; f.stop_after = r.stop_after;
    f.eos_id = m->cfg.eos_id; f.pad_id = m->cfg.pad_id; f.is_prefill = is_prefill ? 1 : 0;
}

// finish of a step over rows slot0 .. slot0 + B: argmax over the n_part lm-head partials, EOS / budget / stop rule, next token
static int launch_finish_step(emmax_session* s, int B, bool is_prefill, int n_part, int slot0, hipStream_t st) {
    FinishParams f;
    memset(&f, 0, sizeof(f));
    // the partial count is the grid the launch really used (every launcher reports it): a count modelled separately went
    // stale when a launcher capped its grid (fp8 row GEMV shapes 1/2, EMMAX_GEMV_GRID) and stale partials could win the argmax
    if (n_part <= 0 || n_part > s->n_lm_blocks) return fail(EMMAX_ERR_STATE, "lm-head launch reported no partial count");
    const bool stg = slot0 >= s->stg0;   // a staged prefill runs beside the live batch's decode steps: its own partial buffers
    f.part_val = stg ? s->part_val2 : s->part_val; f.part_idx = stg ? s->part_idx2 : s->part_idx; f.n_part = n_part;
    finish_rows(s, B, is_prefill, slot0, f);
    KCHK(launch_decode_finish(f, st));
    return 0;
}

// the sampling parameters of rows slot0 .. in a finish's parameter struct (SampleFinishParams / ProcFinishParams: the same five fields)
template <class P>
static void sampling_rows(emmax_session* s, int slot0, P& p) {
    p.temperature = s->samp.t + slot0; p.top_k = s->samp.k + slot0; p.top_p = s->samp.p + slot0;
    p.seed = s->samp.seed + slot0; p.subseq = s->samp.sub + slot0;
}

// top-N / watched log-probabilities bound: the rows' entries at their generation index, from the raw logit rows the lm-head just wrote.  Its own
// launch AHEAD of the finish: it reads n_out and done as the step found them (the finish advances both)
static int launch_top_logprobs_step(emmax_session* s, int B, bool is_prefill, int slot0, const float* logits, hipStream_t st) {
    if (!s->toplp.on) return 0;
    TopLogprobParams p;
    memset(&p, 0, sizeof(p));
    p.logits = logits; p.ld = s->m->vocab; p.V = s->m->vocab;
    p.words = s->toplp.words; p.watch_ids = s->toplp.watch_ids; p.row0 = slot0; p.is_prefill = is_prefill ? 1 : 0;
    const RowState r = s->rows.from(slot0, s->max_out);
    p.n_out = r.n_out; p.done = r.done; p.max_new_p = r.max_new;
    KCHK(launch_top_logprobs(p, B, st));
    return 0;
}

// finish of a SAMPLED step over rows slot0 .. slot0 + B: each row's draw from its complete fp32 logit row (the lm-head launch just before
// wrote them, on the same stream), then the same bookkeeping
static int launch_sampled_finish_step(emmax_session* s, int B, bool is_prefill, int slot0, const float* logits, hipStream_t st) {
    if (int r = launch_top_logprobs_step(s, B, is_prefill, slot0, logits, st)) return r;
    SampleFinishParams p;
    memset(&p, 0, sizeof(p));
    finish_rows(s, B, is_prefill, slot0, p.f);
    p.logits = logits; p.ld = s->m->vocab; p.V = s->m->vocab;
    sampling_rows(s, slot0, p);
    p.logprob = s->samp.logprob + (size_t)slot0 * s->max_out;
    KCHK(launch_sample_finish(p, st));
    return 0;
}

// finish of a step with logits processing or scores on: the processors, then the draw (sampling on) or the argmax, then the scores store
static int launch_proc_finish_step(emmax_session* s, int B, bool is_prefill, int slot0, const float* logits, hipStream_t st) {
    if (int r = launch_top_logprobs_step(s, B, is_prefill, slot0, logits, st)) return r;
    ConFinishParams p;   // (no automaton: launched as its ExtFinishParams base; warpers and token rules off too: as its ProcFinishParams base)
    memset(&p, 0, sizeof(p));
    finish_rows(s, B, is_prefill, slot0, p.f);
    p.logits = logits; p.ld = s->m->vocab; p.V = s->m->vocab;
    if (s->samp.on) sampling_rows(s, slot0, p);   // else temperature stays null: every row greedy
    p.logprob = s->samp.logprob + (size_t)slot0 * s->max_out;
    p.row0 = slot0;
    if (s->proc.on) {
        p.penalty = s->proc.pen + slot0; p.ngram = s->proc.ng + slot0; p.min_new = s->proc.mn + slot0;
        p.hist = s->proc.hist + (size_t)slot0 * s->max_prompt; p.hist_len = s->proc.hist_len + slot0; p.max_prompt = s->max_prompt;
    }
    if (s->scores.on) p.score_words = s->scores.words;
    if (!s->warp.on && !s->rules.on && !s->aut.on) {
        KCHK(launch_proc_finish(p, st));
        return 0;
    }
    if (s->warp.on) { p.min_p = s->warp.minp + slot0; p.typical_p = s->warp.typ + slot0; p.eps_cut = s->warp.eps + slot0; p.eta_cut = s->warp.eta + slot0; }
    if (s->rules.on) {
        p.rt.n = s->rules.n; p.rt.off = s->rules.off; p.rt.ids = s->rules.ids; p.rt.flags = s->rules.flags; p.rt.bias = s->rules.bias;
        p.rule_en = s->rules.en + slot0;
    }
    if (s->aut.on) {
        p.cls = s->aut.cls; p.allow = s->aut.allow; p.next = s->aut.next; p.n_states = EMMAX_MAX_AUT_STATES; p.next_ld = EMMAX_MAX_AUT_CLASSES;
        p.state = s->aut.state + slot0;
        KCHK(launch_con_finish(p, st));
        return 0;
    }
    KCHK(launch_ext_finish(p, st));
    return 0;
}

// pages a group of K beams uses for a context of S tokens and max_new generated ones, against the K rows' share (include/emmax.h): the
// prompt's pages, a private page per beam from the prompt's partial page on, one more per beam at every page boundary, K spares
bool beam_pages_fit(const emmax_session* s, int S, int max_new) {
    const int K = s->beam.K, rem = S % PAGE;
    long long need = (S + PAGE - 1) / PAGE + (rem > 0 ? K - 1 : K) + K;
    for (int L = S + 1; L <= S + max_new - 1; ++L)
        if (L % PAGE == 0) need += K;
    return S + max_new <= s->max_ctx && need <= (long long)K * s->max_pages;
}

static int launch_page_copies(emmax_session* s, int rows, hipStream_t st);

// the tail of a step with beams on (beam.hip): per-row candidates, the groups' merge + state + page-table gather, the partial-page copies.
// is_prefill: the first beam step, from the prefill's one logit row per group, and the fork
int launch_beam_finish(emmax_session* s, bool is_prefill, hipStream_t st) {
    emmax_model* m = s->m;
    const int K = s->beam.K, G = s->beam.G, rows = G * K;
    BeamRowParams r;
    memset(&r, 0, sizeof(r));
    r.logits = s->logits; r.ld = m->vocab; r.V = m->vocab; r.K = K; r.is_prefill = is_prefill ? 1 : 0;
    r.run_score = s->beam.run; r.done = s->rows.done; r.n_out = s->rows.n_out;
    r.cand_acc = s->beam.cand_acc; r.cand_tok = s->beam.cand_tok; r.row_lse = s->beam.row_lse;
    r.score_words = s->scores.on ? s->scores.words : nullptr;
    KCHK(launch_beam_rows(r, is_prefill ? G : rows, st));
    BeamMergeParams g;
    memset(&g, 0, sizeof(g));
    g.K = K; g.V = m->vocab; g.is_prefill = r.is_prefill; g.eos_id = s->beam.eos; g.pad_id = m->cfg.pad_id; g.max_pages = s->max_pages;
    g.max_out = s->max_out; g.tr_ld = std::min(s->max_batch, EMMAX_MAX_DECODE_BATCH); g.es_mode = s->beam.es; g.lp_pos = s->beam.lp_pos;
    g.pw = s->beam.pw; g.cand_acc = s->beam.cand_acc; g.cand_tok = s->beam.cand_tok; g.row_lse = s->beam.row_lse;
    g.run_score = s->beam.run; g.fin_score = s->beam.fin_score; g.fin_flag = s->beam.fin_flag; g.fin_t = s->beam.fin_t; g.fin_par = s->beam.fin_par;
    g.fin_tok = s->beam.fin_tok; g.grp_state = s->beam.grp;
    g.cur_tok = s->rows.cur_tok; g.ctx_len = s->rows.ctx_len; g.done = s->rows.done; g.n_out = s->rows.n_out; g.max_new_p = s->rows.max_new;
    g.page_table = s->page_table; g.spare = s->beam.spare; g.copy_src = s->beam.csrc; g.copy_dst = s->beam.cdst; g.copy_ntok = s->beam.cntok;
    g.grp_shared = s->grp_shared;
    g.tr_tok = s->beam.tr_tok; g.tr_par = s->beam.tr_par; g.tr_score = s->beam.tr_score; g.tr_lse = s->beam.tr_lse; g.tc_idx = s->beam.tc_idx;
    g.tc_acc = s->beam.tc_acc;
    if (is_prefill)
        for (int i = 0; i < G; ++i) g.S[i] = s->S[i];
    KCHK(launch_beam_merge(g, G, st));
    return launch_page_copies(s, rows, st);
}

// the partial-page copies of the list in beam.csrc / cdst / cntok (the beam merge or the sample groups' fork wrote it), one entry per row:
// every layer, every plane of the cache format
static int launch_page_copies(emmax_session* s, int rows, hipStream_t st) {
    emmax_model* m = s->m;
    BeamCopyParams c;
    memset(&c, 0, sizeof(c));
    const long long kvr = kv_rows(s), hd = m->cfg.head_dim;
    c.kv = (char*)s->kv; c.layer_stride = s->kv_layer_stride; c.Hkv = m->cfg.n_kv_heads; c.n_pages = s->rows_total * s->max_pages;
    c.copy_src = s->beam.csrc; c.copy_dst = s->beam.cdst; c.copy_ntok = s->beam.cntok;
    auto plane = [&](long long off, int rb) { c.plane_off[c.n_planes] = off; c.plane_rb[c.n_planes] = rb; c.n_planes += 1; };
    switch (s->kv_fmt) {
    case KV_FP8:   // K bytes, V bytes, K scales, V scales
        plane(0, (int)hd); plane(kvr * hd, (int)hd); plane(2 * kvr * hd, 4); plane(2 * kvr * hd + kvr * 4, 4);
        break;
    case KV_X24:   // per operand a bf16 plane and its 8-bit extension plane
        plane(0, (int)hd * 2); plane(kvr * hd * 2, (int)hd); plane(kvr * hd * 3, (int)hd * 2); plane(kvr * hd * 5, (int)hd);
        break;
    case KV_F32:
        plane(0, (int)hd * 4); plane(kvr * hd * 4, (int)hd * 4);
        break;
    default:
        plane(0, (int)hd * 2); plane(kvr * hd * 2, (int)hd * 2);
    }
    KCHK(launch_beam_copy(c, rows, m->cfg.n_layers, st));
    return 0;
}

// The end of a prefill with sample groups on (include/emmax.h): the lm-head of the G prefilled rows, each group's logit row (and prompt history)
// given to its N rows, the fork of the page table with the copies of the prompt's partial page, then token 0 of all G x N rows by the
// sampled or processing finish a G x N batch's prefill ends in -- row g N + j draws with its own parameters.  The finish reads logit rows
// and per-row state only, so it runs behind the fork
int run_group_fork(emmax_session* s, int G, hipStream_t st) {
    emmax_model* m = s->m;
    const int N = s->grp_N, rows = G * N, V = m->vocab;
    if (s->exact) {   // (as with beams: a group's first row must not depend on how many groups were prefilled with it)
        for (int g = 0; g < G; ++g)
            if (int r = run_lm_head_step(s, 1, true, s->logits + (size_t)g * V, false, st, g)) return r;
    } else if (int r = run_lm_head_step(s, G, true, s->logits, false, st, 0)) {
        return r;
    }
    KCHK(launch_group_bcast(s->logits, (long long)V * 4, G, N, st));
    if (s->proc.on) {
        KCHK(launch_group_bcast(s->proc.hist, (long long)s->max_prompt * 4, G, N, st));
        KCHK(launch_group_bcast(s->proc.hist_len, 4, G, N, st));
    }
    GroupForkParams f;
    memset(&f, 0, sizeof(f));
    f.N = N; f.max_pages = s->max_pages; f.page_table = s->page_table; f.st = s->rows;
    f.copy_src = s->beam.csrc; f.copy_dst = s->beam.cdst; f.copy_ntok = s->beam.cntok; f.grp_shared = s->grp_shared;
    bool partial = false;
    for (int g = 0; g < G; ++g) {
        f.S[g] = s->S[g];
        partial = partial || s->S[g] % PAGE != 0;
    }
    KCHK(launch_group_fork(f, G, st));
    if (partial)   // (every prompt ends on a page boundary: all pages are shared by reference, nothing to copy)
        if (int r = launch_page_copies(s, rows, st)) return r;
    for (int g = G - 1; g >= 0; --g)
        for (int j = N - 1; j >= 0; --j) s->S[g * N + j] = s->S[g];
    s->cur_B = rows;
    const int mode = finish_mode(s), chunk = stage_chunk(STAGE_LMHEAD, s->exact);   // one finish per lm-head launch of a G x N step (run_lm_head_step)
    for (int r0 = 0; r0 < rows; r0 += chunk) {
        const int n = std::min(chunk, rows - r0);
        const float* lg = s->logits + (size_t)r0 * V;
        if (int r = (mode & FINISH_ROWS) ? launch_proc_finish_step(s, n, true, r0, lg, st) : launch_sampled_finish_step(s, n, true, r0, lg, st)) return r;
    }
    return 0;
}

// The device side of emmax_slots_fork (include/emmax.h): the fork of slot `src` into the n idle slots dst[] -- page-table rows, hidden pages,
// per-row state and parameters in one launch, the copies of the prompt's partial page, then token 0 of every follower by the finish a one-row
// prefill ends in, reading the prompt's logit row where the source's prefill left it (row `logit_row`: the finishes take it as const)
int run_slots_fork(emmax_session* s, int src, int logit_row, const int32_t* dst, int n, hipStream_t st) {
    SlotForkParams f;
    memset(&f, 0, sizeof(f));
    f.n = n; f.rows = s->cur_B; f.src = src; f.S = s->S[src]; f.max_pages = s->max_pages;
    for (int j = 0; j < n; ++j) f.dst[j] = dst[j];
    f.page_table = s->page_table; f.hidden = s->hidden; f.st = s->rows;
    if (int r = session_row_cols(s, &f.cols)) return r;   // (the kernel copies the inherited ones)
    f.copy_src = s->beam.csrc; f.copy_dst = s->beam.cdst; f.copy_ntok = s->beam.cntok;
    f.in_t = s->fork_t; f.in_p = s->fork_p; f.in_k = s->fork_k; f.in_seed = s->fork_seed; f.in_sub = s->fork_sub;
    f.temperature = s->samp.t; f.top_p = s->samp.p; f.top_k = s->samp.k; f.seed = s->samp.seed; f.subseq = s->samp.sub;
    if (s->aut.on) { f.aut_start = s->aut.start; f.aut_state = s->aut.state; }   // a follower enters at the source's start state
    KCHK(launch_slots_fork(f, st));
    if (f.S % PAGE != 0)   // (else the prompt ends on a page boundary: every page is shared by reference, nothing to copy)
        if (int r = launch_page_copies(s, n, st)) return r;
    const float* lg = s->logits + (size_t)logit_row * s->m->vocab;
    for (int j = 0; j < n; ++j)
        if (int r = (finish_mode(s) & FINISH_ROWS) ? launch_proc_finish_step(s, 1, true, dst[j], lg, st) : launch_sampled_finish_step(s, 1, true, dst[j], lg, st)) return r;
    return 0;
}

// slot0: first row of the B rows this call covers (slot prefill: one row in the middle of a live batch)
int run_lm_head_step(emmax_session* s, int B, bool is_prefill, float* logits_out, bool do_finish, hipStream_t st, int slot0) {
    emmax_model* m = s->m;
    if (do_finish && s->beam.K) {   // beams on: every chunk's lm-head writes its logit rows, then ONE beam finish over all rows (a prefill's
                                    // rows wait for emmax_generate, which knows the token budget the first beam step needs)
        if (is_prefill && s->exact) {   // exact numerics: a group's first row must not depend on how many groups were prefilled with it, and
                                        // lm-heads of 1-2 and of 3-8 rows are different kernels -- one row per launch
            for (int b = 0; b < B; ++b) {
                if (int r = run_lm_head_step(s, 1, true, s->logits + (size_t)(slot0 + b) * m->vocab, false, st, slot0 + b)) return r;
            }
            return 0;
        }
        const int r = run_lm_head_step(s, B, is_prefill, s->logits + (size_t)slot0 * m->vocab, false, st, slot0);
        if (r || is_prefill) return r;
        return launch_beam_finish(s, false, st);
    }
    const int chunk = stage_chunk(STAGE_LMHEAD, s->exact);
    if (B > chunk) {   // one launch per chunk, each with its own finish: the argmax partials are laid out per launch
        for (int r0 = 0; r0 < B; r0 += chunk)
            if (int r = run_lm_head_step(s, std::min(chunk, B - r0), is_prefill, logits_out ? logits_out + (size_t)r0 * m->vocab : nullptr, do_finish, st, slot0 + r0)) return r;
        return 0;
    }
    // sampling, processing or scores on: a step's lm-head also writes the fp32 logit rows of its B rows, and the sampled or processing finish
    // reads them
    const int mode = do_finish ? finish_mode(s) : 0;
    const bool sampled = mode != 0;
    if (sampled) logits_out = s->logits + (size_t)slot0 * m->vocab;
    GemvParams p;
    lmhead_params(s, slot0, logits_out, p);
    int lm_grid = 0;
    KCHK(launch_proj(m->lm_head_w, p, B, st, &lm_grid, &s->last_via));
    if (mode & FINISH_ROWS) return launch_proc_finish_step(s, B, is_prefill, slot0, logits_out, st);
    if (sampled) return launch_sampled_finish_step(s, B, is_prefill, slot0, logits_out, st);
    if (do_finish) return launch_finish_step(s, B, is_prefill, lm_grid, slot0, st);
    return 0;
}

// rows r .. of a projection stage's operands (stage_chunk: which stages run in more than one launch)
static void offset_rows(GemvParams& p, int stage, int r, bool exact) {
    const size_t eb = exact ? 4 : 2;   // bytes of an activation element the stages hand on (exact numerics: fp32)
    if (p.h32) p.h32 += (size_t)r * p.ldh;
    switch (stage) {
        case STAGE_QKV:   // (qkv and gate/up run in chunks in exact numerics only, where the rows are read from the fp32 stream)
            p.y = (char*)p.y + (size_t)r * p.ldy * eb;
            p.ctx_len += r; p.page_table += (size_t)r * p.max_pages;
            break;
        case STAGE_OPROJ:
            if (p.attn_part) p.attn_part += (size_t)r * p.Hq * p.nsplit * EMMAX_PSTRIDE;
            else p.x = (const char*)p.x + (size_t)r * p.ldx * eb;
            p.y = (bf16*)p.y + (size_t)r * p.ldy;
            break;
        case STAGE_GATEUP: p.y = (char*)p.y + (size_t)r * p.ldy * eb; break;
        default:   // STAGE_DOWN
            p.x = (const char*)p.x + (size_t)r * p.ldx * eb;
            p.y = (bf16*)p.y + (size_t)r * p.ldy;
    }
}

// one stage of decoder layer `li` (the unit the profiler times); the step is stages 0..4 of every layer + lm head
int run_decode_stage(emmax_session* s, int B, int li, int stage, hipStream_t st) {
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    if (stage == STAGE_ATTN) {
        DecodeAttnParams a;
        memset(&a, 0, sizeof(a));
        a.q = s->dq; a.ldq = m->q_dim; a.kcache = kcache_of(s, li); a.vcache = vcache_of(s, li);
        if (s->kv8) { a.kv_stage = s->kv_stage; a.kscale = kscale_of(s, li); a.vscale = vscale_of(s, li); }
        a.page_table = s->page_table; a.ctx_len = s->rows.ctx_len; a.done = s->rows.done; a.part = s->part; a.Hkv = c.n_kv_heads; a.page = PAGE;
        a.max_pages = s->max_pages; a.scale = 1.0f / sqrtf((float)c.head_dim);
        a.o_out = attn_direct_on(s, B) ? s->datt : nullptr;
        const int ns = decode_attn_nsplit(B, c.n_kv_heads);
        if (s->exact) {
            a.q = s->dq32; a.kv24 = s->kv24;
            a.o_out = attn_direct_on(s, B) ? (void*)s->dq32 : nullptr;
            KCHK(launch_x_decode_attn(a, B, c.n_heads, c.head_dim, ns, st));
            return 0;
        }
        if (const int N = attn_group_rows(s, B)) {   // the shared prompt pages once per group, then the rows' tails
            a.grp_shared = s->grp_shared;
            KCHK(launch_group_attn(a, B, N, c.n_heads, c.head_dim, st));
            return 0;
        }
        KCHK(launch_decode_attn(a, B, c.n_heads, c.head_dim, ns, st));
        return 0;
    }
    if (stage < STAGE_QKV || stage > STAGE_DOWN) return fail(EMMAX_ERR_INVALID, "unknown decode stage %d", stage);
    const ProjW& w = m->layers[li].proj[stage];
    GemvParams p0;
    stage_params(s, B, li, stage, p0);
    const int chunk = stage_chunk(stage, s->exact);
    for (int r = 0; r < B; r += chunk) {
        GemvParams p = p0;
        int grid = 0;
        offset_rows(p, stage, r, s->exact);
        KCHK(launch_proj(w, p, std::min(chunk, B - r), st, &grid, &s->last_via));
    }
    return 0;
}

// layer 0's qkv with the embedding gather folded in: decode_ks.hip's check is asked with the launch's own parameters (x_tok set); where it
// says no, the embed launch and the plain stage
static int run_qkv0_with_embed(emmax_session* s, int B, hipStream_t st) {
    emmax_model* m = s->m;
    GemvParams p;
    stage_params(s, B, 0, STAGE_QKV, p);
    gemv_set_weights(p, PW_BF16, m->layers[0].proj[STAGE_QKV].rm);
    p.x = m->embed; p.x_tok = s->rows.cur_tok; p.x_copy = s->dh; p.x_vocab = m->vocab;
    const int r = launch_decode_ks(GEMV_QKV, p, B, st, nullptr);
    if (r == -2) {
        KCHK(launch_decode_embed(s->rows.cur_tok, m->embed, s->dh, B, m->H, m->vocab, st, s->exact ? s->dh32 : h32_of(s)));
        return run_decode_stage(s, B, 0, STAGE_QKV, st);
    }
    return r ? fail(EMMAX_ERR_HIP, "qkv launch of layer 0 failed (code %d)", r) : 0;
}

int run_decode_step(emmax_session* s, int B, hipStream_t st) {
    emmax_model* m = s->m;
    // batch 1-2 on bf16 weights: the embedding row is read by layer 0's qkv launch itself (decode_ks.hip, when it takes the launch) -- one launch fewer
    const bool fold_embed = B < EMMAX_MFMA_MIN_BATCH && m->wfmt == PW_BF16 && decode_ks_enabled() && emmax_tune().fold_embed != 0;
    if (!fold_embed) KCHK(launch_decode_embed(s->rows.cur_tok, m->embed, s->dh, B, m->H, m->vocab, st, s->exact ? s->dh32 : h32_of(s)));
    const bool taps = s->taps.step.on;   // (nothing bound: the launches below are all there is)
    if (taps)
        if (int r = tap_step_hidden(s, 0, B, st)) return r;
    for (int li = 0; li < m->cfg.n_layers; ++li)
        for (int stage = STAGE_QKV; stage <= STAGE_DOWN; ++stage) {
            if (int r = (li == 0 && stage == STAGE_QKV && fold_embed) ? run_qkv0_with_embed(s, B, st) : run_decode_stage(s, B, li, stage, st)) return r;
            // the map behind the attention launch (an fp8 cache gets the step's key only there), the stream behind the down projection
            if (taps && stage == STAGE_ATTN)
                if (int r = tap_step_attn(s, li, B, st)) return r;
            if (taps && stage == STAGE_DOWN)
                if (int r = tap_step_hidden(s, li + 1, B, st)) return r;
        }
    return run_lm_head_step(s, B, false, nullptr, true, st);
}

void drop_graph(emmax_session* s) {
    if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    s->graph_exec = nullptr;
    s->graph = nullptr;
    s->graph_B = 0;
}

static int graph_fail(emmax_session* s, const std::string& why) {
    s->graph_failed = 1;
    s->graph_err = why;
    (void)hipGetLastError();
    return 1;
}

// Capture one decode step into a hipGraph.
int ensure_graph(emmax_session* s, int B, hipStream_t st) {
    // Default: eager launch-ahead.  One step is 163 launches for >= 2.6 ms of GPU time, so a single host thread stays far
    // ahead of the device, and measured on MI355X / ROCm 7.2 the replayed graph is the SLOWER option: 3.05 vs 2.95 ms/token
    // at B = 1 (~0.6 us more per kernel node than a same-stream launch; round 3: 2.73 vs 2.62).  What was tried against that,
    // and what each runtime setting did, is recorded in profiles/r05_graph_switches.txt.
    // Tuning switch graph = 1 (EMMAX_GRAPH=1 at start-up, or emmax_tuning_set) selects graph replay (a host whose launch thread
    // cannot be kept free).
    s->last_step_graph = 0;   // set again by launch_graph_step when a replay really runs
    if (!emmax_tune().graph) return 1;   // eager step: a captured graph stays valid for the next caller that wants replay
    if (s->graph_exec && s->graph_B == B && s->graph_stream_cap == st && s->graph_epoch == emmax_tune().epoch && s->graph_mode == finish_mode(s) &&
        s->graph_grp == attn_group_rows(s, B) && s->graph_taps == s->taps.serial)
        return 0;
    drop_graph(s);
    if (s->graph_failed) return 1;
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return graph_fail(s, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e));
    const int r = run_decode_step(s, B, st);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(st, &g);
    if (r != 0 || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        return graph_fail(s, r != 0 ? ("launch during capture: " + g_err) : (std::string("hipStreamEndCapture: ") + hipGetErrorString(e)));
    }
    hipGraphExec_t ge = nullptr;
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        return graph_fail(s, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    }
    s->graph = g; s->graph_exec = ge; s->graph_B = B; s->graph_stream_cap = st; s->graph_epoch = emmax_tune().epoch;
    s->graph_mode = finish_mode(s); s->graph_grp = attn_group_rows(s, B); s->graph_taps = s->taps.serial;
    return 0;
}

int launch_graph_step(emmax_session* s, int B, hipStream_t st) {
    s->last_step_graph = 1;
    HIPCHK(hipGraphLaunch(s->graph_exec, st));
    return 0;
}
