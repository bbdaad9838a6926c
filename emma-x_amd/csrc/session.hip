// session.hip -- the session: its workspace plan (every activation buffer, the per-row state, the mode state), the sizing of the paged KV
// region, and emmax_session_bytes* / create / destroy.
#include "session.h"

static void plan_session(emmax_session* s, Bump& b) {
    emmax_model* m = s->m;
    const int Bv = s->max_batch;
    int maxN = 0, maxDp = 0, maxD3p = 0, maxMp = 0, maxK = 0;
    for (int t = 0; t < 2; ++t) {
        const TowerW& T = m->tw[t];
        maxN = std::max(maxN, T.N); maxDp = std::max(maxDp, T.Dp); maxD3p = std::max(maxD3p, T.D3p);
        maxMp = std::max(maxMp, T.Mp); maxK = std::max(maxK, T.Kpe);
    }
    const int np = m->tw[0].n_patches;
    const int64_t vr = (int64_t)Bv * maxN;
    s->vA = (bf16*)b.bytes((int64_t)Bv * np * maxK * 2);
    s->vpe = (bf16*)b.bytes((int64_t)Bv * np * maxDp * 2);
    s->vtok = (bf16*)b.bytes(vr * maxDp * 2);
    s->vln = (bf16*)b.bytes(vr * maxDp * 2);
    s->vstats = (float*)b.bytes(vr * 2 * 4);
    s->vqkv = (bf16*)b.bytes(vr * maxD3p * 2);
    s->vatt = (bf16*)b.bytes(vr * maxDp * 2);
    s->vmlp = (bf16*)b.bytes(vr * maxMp * 2);
    s->feats = (bf16*)b.bytes((int64_t)Bv * np * m->Vp * 2);
    s->pj1 = (bf16*)b.bytes((int64_t)Bv * np * m->P1p * 2);
    s->pj2 = (bf16*)b.bytes((int64_t)Bv * np * m->H * 2);
    s->patch_embeds = (bf16*)b.bytes((int64_t)Bv * np * m->H * 2);
    for (int t = 0; t < 2; ++t) s->cu_vit[t] = (int32_t*)b.bytes((Bv + 1) * 4);
    {   // tower 1's own scratch for the two-stream form (sized for tower 1 alone, up to 256 frames: ~5 MB per frame)
        const TowerW& T1 = m->tw[1];
        s->vis2_B = std::min(Bv, 256);
        const int64_t B2 = s->vis2_B, r2 = B2 * T1.N;
        s->v2A = (bf16*)b.bytes(B2 * np * T1.Kpe * 2);
        s->v2pe = (bf16*)b.bytes(B2 * np * T1.Dp * 2);
        s->v2tok = (bf16*)b.bytes(r2 * T1.Dp * 2);
        s->v2ln = (bf16*)b.bytes(r2 * T1.Dp * 2);
        s->v2stats = (float*)b.bytes(r2 * 2 * 4);
        s->v2qkv = (bf16*)b.bytes(r2 * T1.D3p * 2);
        s->v2att = (bf16*)b.bytes(r2 * T1.Dp * 2);
        s->v2mlp = (bf16*)b.bytes(r2 * T1.Mp * 2);
        s->v2splitk_bytes = (int64_t)64 << 20;   // the same budget as the session's split-K scratch: the same plans, bit-identical towers
        s->v2splitk_ws = (float*)b.bytes(s->v2splitk_bytes);
    }
    const int64_t R = s->max_rows;
    s->ph = (bf16*)b.bytes(R * m->H * 2);
    s->ph32 = (float*)b.bytes(R * m->H * 4);
    s->pxn = (bf16*)b.bytes(R * m->H * 2);
    s->pqkv = (bf16*)b.bytes(R * m->qkv_dim * 2);
    s->patt = (bf16*)b.bytes(R * m->q_dim * 2);
    s->pact = (bf16*)b.bytes(R * m->inter_p * 2);
    s->cu = (int32_t*)b.bytes((s->max_batch + 1) * 4);
    const int Bd = s->max_batch, Br = s->rows_total;   // decode batch rows / all rows incl. the staging rows
    s->dh = (bf16*)b.bytes((int64_t)Br * m->H * 2);
    s->dh32 = (float*)b.bytes((int64_t)Br * m->H * 4);
    s->kv_stage = (bf16*)b.bytes((int64_t)Br * 2 * m->kv_dim * 2);
    s->dq = (bf16*)b.bytes((int64_t)Bd * m->q_dim * 2);
    s->datt = (bf16*)b.bytes((int64_t)Bd * m->q_dim * 2);
    s->dact = (bf16*)b.bytes((int64_t)Bd * m->inter_p * 2);
    s->part = (float*)b.bytes((int64_t)Bd * m->cfg.n_heads * 16 * 132 * 4);
    s->n_lm_blocks = EMMAX_LM_BLOCKS;
    s->part_val = (float*)b.bytes((int64_t)s->n_lm_blocks * Bd * 4);
    s->part_idx = (int32_t*)b.bytes((int64_t)s->n_lm_blocks * Bd * 4);
    s->part_val2 = (float*)b.bytes((int64_t)s->n_lm_blocks * Bd * 4);
    s->part_idx2 = (int32_t*)b.bytes((int64_t)s->n_lm_blocks * Bd * 4);
    s->logits = (float*)b.bytes((int64_t)Br * m->vocab * 4);
    s->samp.t = (float*)b.bytes(Br * 4);
    s->samp.p = (float*)b.bytes(Br * 4);
    s->samp.k = (int32_t*)b.bytes(Br * 4);
    s->samp.seed = (uint64_t*)b.bytes(Br * 8);
    s->samp.sub = (uint32_t*)b.bytes(Br * 4);
    s->samp.logprob = (float*)b.bytes((int64_t)Br * s->max_out * 4);
    s->proc.pen = (float*)b.bytes(Br * 4);
    s->proc.ng = (int32_t*)b.bytes(Br * 4);
    s->proc.mn = (int32_t*)b.bytes(Br * 4);
    s->proc.hist = (int32_t*)b.bytes((int64_t)Br * s->max_prompt * 4);
    s->proc.hist_len = (int32_t*)b.bytes(Br * 4);
    s->scores.words = (uint64_t*)b.bytes(4 * 8);
    s->warp.minp = (float*)b.bytes(Br * 4);
    s->warp.typ = (float*)b.bytes(Br * 4);
    s->warp.eps = (float*)b.bytes(Br * 4);
    s->warp.eta = (float*)b.bytes(Br * 4);
    s->rules.n = (int32_t*)b.bytes(4);
    s->rules.off = (int32_t*)b.bytes((EMMAX_MAX_RULES + 1) * 4);
    s->rules.ids = (int32_t*)b.bytes(EMMAX_MAX_RULE_TOTAL * 4);
    s->rules.flags = (int32_t*)b.bytes(EMMAX_MAX_RULES * 4);
    s->rules.bias = (float*)b.bytes(EMMAX_MAX_RULES * 4);
    s->rules.en = (uint32_t*)b.bytes(Br * 4);
    s->rows.cur_tok = (int32_t*)b.bytes(Br * 4);
    s->rows.ctx_len = (int32_t*)b.bytes(Br * 4);
    s->rows.done = (int32_t*)b.bytes(Br * 4);
    s->rows.n_out = (int32_t*)b.bytes(Br * 4);
    s->rows.out_ids = (int32_t*)b.bytes((int64_t)Br * s->max_out * 4);
    s->rows.max_new = (int32_t*)b.bytes(Br * 4);
    s->stop_ids = (int32_t*)b.bytes(EMMAX_MAX_STOP_IDS * 4);
    s->stop_cfg = (int32_t*)b.bytes(2 * 4);
    s->rows.stop_m = (int32_t*)b.bytes(Br * 4);
    s->rows.stop_after = (int32_t*)b.bytes(Br * 4);
    s->page_table = (int32_t*)b.bytes((int64_t)Br * s->max_pages * 4);
    s->sk_ws = (unsigned long long*)b.bytes((int64_t)256 * 2 * 256 * 8);
    s->sk_ws2 = (unsigned long long*)b.bytes((int64_t)256 * 2 * 256 * 8);
    s->splitk_bytes = (int64_t)64 << 20;   // e.g. 4 slices of a 768 x 4096 prefill GEMM = 50 MB; smaller budgets just split less
    s->splitk_ws = (float*)b.bytes(s->splitk_bytes);
    s->cos_t = (float*)b.bytes((int64_t)s->max_ctx * (m->cfg.head_dim / 2) * 4);
    s->sin_t = (float*)b.bytes((int64_t)s->max_ctx * (m->cfg.head_dim / 2) * 4);
    {   // beam search: rows are decode rows only (no beams on staging rows)
        const int64_t Rb = std::min(Bd, EMMAX_MAX_DECODE_BATCH), T = s->max_out;
        s->beam.cand_acc = (float*)b.bytes(Rb * 2 * EMMAX_MAX_BEAMS * 4);
        s->beam.cand_tok = (int32_t*)b.bytes(Rb * 2 * EMMAX_MAX_BEAMS * 4);
        s->beam.row_lse = (float*)b.bytes(Rb * 4);
        s->beam.run = (float*)b.bytes(Rb * 4);
        s->beam.fin_score = (float*)b.bytes(Rb * 4);
        s->beam.fin_flag = (int32_t*)b.bytes(Rb * 4);
        s->beam.fin_t = (int32_t*)b.bytes(Rb * 4);
        s->beam.fin_par = (int32_t*)b.bytes(Rb * 4);
        s->beam.fin_tok = (int32_t*)b.bytes(Rb * 4);
        s->beam.grp = (int32_t*)b.bytes(Rb * 4 * 4);
        s->beam.spare = (int32_t*)b.bytes(Rb * 4);
        s->beam.csrc = (int32_t*)b.bytes(Rb * 4);
        s->beam.cdst = (int32_t*)b.bytes(Rb * 4);
        s->beam.cntok = (int32_t*)b.bytes(Rb * 4);
        s->grp_shared = (int32_t*)b.bytes(Rb * 4);
        s->beam.pw = (float*)b.bytes((T + 1) * 4);
        s->beam.tr_tok = (int32_t*)b.bytes(T * Rb * 4);
        s->beam.tr_par = (int32_t*)b.bytes(T * Rb * 4);
        s->beam.tr_score = (float*)b.bytes(T * Rb * 4);
        s->beam.tr_lse = (float*)b.bytes(T * Rb * 4);
        s->beam.tc_idx = (int32_t*)b.bytes(T * Rb * 2 * 4);
        s->beam.tc_acc = (float*)b.bytes(T * Rb * 2 * 4);
        s->beam.res_bidx = (int32_t*)b.bytes(T * Rb * 4);
        s->beam.res_len = (int32_t*)b.bytes(Rb * 4);
        s->beam.res_score = (float*)b.bytes(Rb * 4);
    }
    {   // groups in slot serving: the hidden-page rows, and a fork's parameter upload (followers are decode rows)
        const int64_t Rb = std::min(Bd, EMMAX_MAX_DECODE_BATCH);
        s->hidden = (int32_t*)b.bytes((int64_t)Br * s->max_pages * 4);
        s->fork_t = (float*)b.bytes(Rb * 4);
        s->fork_p = (float*)b.bytes(Rb * 4);
        s->fork_k = (int32_t*)b.bytes(Rb * 4);
        s->fork_seed = (uint64_t*)b.bytes(Rb * 8);
        s->fork_sub = (uint32_t*)b.bytes(Rb * 4);
    }
    s->op_rows = std::min(Bd, EMMAX_MAX_DECODE_BATCH);
    s->op_state = (int32_t*)b.bytes((int64_t)s->op_rows * 8 * 4);
    s->op_out = (int32_t*)b.bytes((int64_t)s->op_rows * s->max_out * 4);
    s->ext_base = (int32_t*)b.bytes((int64_t)Bd * 4);
    if (s->exact) {
        const int64_t npr = (int64_t)Bv * np;
        auto mx = [](int64_t a, int64_t b2) { return a > b2 ? a : b2; };
        const int64_t n32 = mx(mx(vr * mx(maxD3p, maxMp), npr * mx(mx(m->P1p, m->H), maxDp)), R * mx(m->qkv_dim, m->inter_p));
        const int64_t nhla = mx(mx(npr * maxK, vr * maxDp), mx(npr * mx(m->Vp, m->H), R * m->H));
        const int64_t nhlb = mx(mx(vr * mx(maxDp, maxMp), npr * m->P1p), R * mx(m->q_dim, m->inter_p));
        s->x32a = (float*)b.bytes(n32 * 4);
        s->xhla = (bf16*)b.bytes(nhla * 4);   // two bf16 terms per element
        s->xhlb = (bf16*)b.bytes(nhlb * 4);
        s->xtok32 = (float*)b.bytes(vr * maxDp * 4);
        s->xfeats32 = (float*)b.bytes(npr * m->Vp * 4);
        s->xpe32 = (float*)b.bytes(npr * m->H * 4);
        s->dq32 = (float*)b.bytes((int64_t)Bd * m->q_dim * 4);
        s->dact32 = (float*)b.bytes((int64_t)Bd * m->inter_p * 4);
    }
    // top-N / watched log-probabilities: the words that name the caller's buffers and the watch list (last in the plan: every other offset stays)
    s->toplp.words = (uint64_t*)b.bytes(TOPLP_WORDS * 8);
    s->toplp.watch_ids = (int32_t*)b.bytes(EMMAX_MAX_WATCH_IDS * 4);
    // the token automaton (behind them for the same reason)
    s->aut.cls = (uint8_t*)b.bytes(EMMAX_SAMPLE_MAX_V);
    s->aut.allow = (uint32_t*)b.bytes((int64_t)EMMAX_MAX_AUT_STATES * 8 * 4);
    s->aut.next = (int16_t*)b.bytes((int64_t)EMMAX_MAX_AUT_STATES * EMMAX_MAX_AUT_CLASSES * 2);
    s->aut.start = (int32_t*)b.bytes(Br * 4);
    s->aut.state = (int32_t*)b.bytes(Br * 4);
}

// THE per-row device arrays of a session, by {owner is on, owner, inherited by a forked follower, bytes between rows, bytes of a row that move}.
// emmax_slots_commit moves all of them (misc.hip: emmax_slots_commit_kernel), emmax_slots_fork the inherited ones, and
// emmax_session_clear_warpers zeroes its owner's: a per-row array added to plan_session gets its name in here and is served by all three
int session_row_cols(const emmax_session* s, RowCols* out) {
    const RowState& r = s->rows;
    const TopLogprobs& t = s->toplp;
    const uint32_t out_row = (uint32_t)s->max_out * 4, hist_row = (uint32_t)s->max_prompt * 4;
    const uint32_t top_row = (uint32_t)t.n_top * 4, watch_row = (uint32_t)t.n_watch * 4;   // caller-owned [rows][max_new][n]: a staged request has entry 0 only
    bool fits = true;
    out->n = 0;
    auto add = [&](bool on, int owner, int inherit, uint32_t stride, uint32_t move, std::initializer_list<const void*> bases) {
        for (const void* b : bases) {
            fits = fits && (!on || out->n < (int)(sizeof(out->col) / sizeof(out->col[0])));
            if (on && fits) out->col[out->n++] = RowCol{(char*)b, stride, move, (uint8_t)owner, (uint8_t)inherit};
        }
    };
    add(true, ROWS_CORE, 0, 4, 4, {r.cur_tok, r.ctx_len, r.done, r.n_out, r.stop_m, r.stop_after});
    add(true, ROWS_CORE, 1, 4, 4, {r.max_new});
    add(true, ROWS_CORE, 0, out_row, out_row, {r.out_ids});
    add(s->samp.on, ROWS_SAMPLING, 0, 4, 4, {s->samp.t, s->samp.k, s->samp.p, s->samp.sub});
    add(s->samp.on, ROWS_SAMPLING, 0, 8, 8, {s->samp.seed});
    add(s->samp.on, ROWS_SAMPLING, 0, out_row, out_row, {s->samp.logprob});
    add(s->proc.on, ROWS_PROCESSING, 1, 4, 4, {s->proc.pen, s->proc.ng, s->proc.mn, s->proc.hist_len});
    add(s->proc.on, ROWS_PROCESSING, 1, hist_row, hist_row, {s->proc.hist});
    add(s->warp.on, ROWS_WARPERS, 1, 4, 4, {s->warp.minp, s->warp.typ, s->warp.eps, s->warp.eta});
    add(s->rules.on, ROWS_RULES, 1, 4, 4, {s->rules.en});
    add(s->aut.on, ROWS_AUTOMATON, 1, 4, 4, {s->aut.start});
    add(s->aut.on, ROWS_AUTOMATON, 0, 4, 4, {s->aut.state});   // (a follower's state is its source's START: the fork sets it)
    add(t.on && t.n_top > 0, ROWS_TOPLP, 0, (uint32_t)t.max_new * top_row, top_row, {t.ids_out, t.lp_out});
    add(t.on && t.n_watch > 0, ROWS_TOPLP, 0, (uint32_t)t.max_new * watch_row, watch_row, {t.watch_out});
    return fits ? 0 : fail(EMMAX_ERR_STATE, "a session has more per-row arrays than the %d a commit or a fork carries (kernels.h: RowCols)", out->n);
}

static int kv_format_now() { return emmax_tune().exact >= 2 ? KV_F32 : emmax_tune().exact == 1 ? KV_X24 : (emmax_tune().kv_fp8 ? KV_FP8 : KV_BF16); }
static int64_t kv_layer_bytes(const emmax_model* m, int rows, int max_pages, int fmt) {
    return 2 * kv_rows_per_layer(m, rows, max_pages) * (m->cfg.head_dim * kv_elem_bytes(fmt) + (fmt == KV_FP8 ? 4 : 0));
}
static int64_t kv_bytes_for(const emmax_model* m, int max_batch, int max_pages, int fmt) {
    return (int64_t)m->cfg.n_layers * kv_layer_bytes(m, max_batch, max_pages, fmt);
}

static int session_dims(const emmax_model* m, int max_batch, int max_prompt, int max_ctx, int* max_pages, int* max_rows) {
    if (!m) return fail(EMMAX_ERR_INVALID, "null model");
    if (max_batch < 1 || max_batch > 256) return fail(EMMAX_ERR_INVALID, "max_batch outside 1..256");
    const int np = m->tw[0].n_patches;
    if (max_prompt < 1) return fail(EMMAX_ERR_INVALID, "max_prompt < 1");
    if (max_ctx < np + max_prompt + 1) return fail(EMMAX_ERR_INVALID, "max_ctx %d < patches %d + max_prompt %d + 1", max_ctx, np, max_prompt);
    *max_pages = (max_ctx + PAGE - 1) / PAGE;
    *max_rows = max_batch * (np + max_prompt);
    return 0;
}

// stage_rows: staging rows for overlapped admissions (emmax_slots_prefill_staged), 0 .. min(max_batch, EMMAX_MAX_DECODE_BATCH).  They
// cost per-row state AND their share of the paged KV region; a session that never stages (emmax_prefill / emmax_generate, the bench)
// asks for none (round 4 gave every session min(max_batch, 8) of them and doubled the KV region of small sessions).
static int check_stage_rows(int max_batch, int stage_rows) {
    if (stage_rows < 0 || stage_rows > max_batch || stage_rows > EMMAX_MAX_DECODE_BATCH)
        return fail(EMMAX_ERR_INVALID, "stage_rows %d outside 0..min(max_batch=%d, %d)", stage_rows, max_batch, EMMAX_MAX_DECODE_BATCH);
    return 0;
}
// what an exact-numerics session needs of its model and its shape
static int check_exact(const emmax_model* m, int max_batch, int stage_rows) {
    if (m->wfmt != PW_BF16) return fail(EMMAX_ERR_INVALID, "exact numerics (tuning switch exact) runs on bf16 weights: this model streams %s decode weights", m->wfmt_name());
    if (m->finalized && m->ln_folded)
        return fail(EMMAX_ERR_STATE, "exact numerics needs the ViT LayerNorms unfolded: set the tuning switch exact = 1 BEFORE emmax_model_finalize");
    // batch 1-2: decode_ks.hip's two-term dot products; batch 3-8: decode_km.hip's EX kernels (the two terms of a row in the MFMA's sixteen batch
    // columns); batches above 8 rows run their projections in chunks of 8 (stage_chunk).  What shapes those take is their checks' to say: the
    // exact planner must serve min(max_batch, 8) rows
    if (max_batch > EMMAX_MAX_DECODE_BATCH) return fail(EMMAX_ERR_INVALID, "exact numerics serves batches of 1-%d rows; max_batch %d", EMMAX_MAX_DECODE_BATCH, max_batch);
    int stage = 0, B = 0;
    if (model_max_decode_batch(m, true, &stage, &B) < std::min(max_batch, 8))
        return fail(EMMAX_ERR_INVALID, "exact numerics: no two-term kernel takes the %s projection of this model at batch %d (decode_ks.hip at 1-2 rows: widths in multiples of 64; decode_km.hip at 3-8: hidden / q widths in multiples of 256 up to 4096, tuning switch km); max_batch %d",
                    decode_stage_name(stage), B, max_batch);
    return 0;
}

extern "C" {

int emmax_session_bytes(const emmax_model* m, int max_batch, int max_prompt, int max_ctx, int64_t* ws, int64_t* kv) {
    return emmax_session_bytes_ex(m, max_batch, max_prompt, max_ctx, 0, ws, kv);
}
int emmax_session_bytes_ex(const emmax_model* m, int max_batch, int max_prompt, int max_ctx, int stage_rows, int64_t* ws, int64_t* kv) {
    int mp, mr, r;
    if ((r = session_dims(m, max_batch, max_prompt, max_ctx, &mp, &mr))) return r;
    if ((r = check_stage_rows(max_batch, stage_rows))) return r;
    emmax_session tmp;
    tmp.m = const_cast<emmax_model*>(m);
    tmp.max_batch = max_batch; tmp.max_prompt = max_prompt; tmp.max_ctx = max_ctx; tmp.max_pages = mp; tmp.max_rows = mr;
    tmp.max_out = max_ctx;
    tmp.n_stg = stage_rows; tmp.stg0 = max_batch; tmp.rows_total = max_batch + tmp.n_stg;
    tmp.exact = emmax_tune().exact != 0;
    if (tmp.exact && (r = check_exact(m, max_batch, stage_rows))) return r;
    if (m->is_mx() && max_batch > model_max_decode_batch(m))   // no kernel streams the block-scaled tiles for more rows: refused here, not at the first prefill
        return fail(EMMAX_ERR_INVALID, "%s decode weights serve batches of 1-%d rows; max_batch %d", m->wfmt_name(), model_max_decode_batch(m), max_batch);
    Bump b{nullptr};
    plan_session(&tmp, b);
    if (ws) *ws = b.off + 256;
    if (kv) *kv = kv_bytes_for(m, tmp.rows_total, mp, kv_format_now());
    return 0;
}

int emmax_session_create(emmax_model* m, int max_batch, int max_prompt, int max_ctx, void* ws, int64_t ws_bytes, void* kv,
                         int64_t kvb, emmax_session** out) {
    return emmax_session_create_ex(m, max_batch, max_prompt, max_ctx, 0, ws, ws_bytes, kv, kvb, out);
}
int emmax_session_stage_rows(const emmax_session* s) { return s ? s->n_stg : -1; }
int emmax_session_exact(const emmax_session* s) { return s ? (s->exact ? 1 : 0) : -1; }
int emmax_session_create_ex(emmax_model* m, int max_batch, int max_prompt, int max_ctx, int stage_rows, void* ws, int64_t ws_bytes, void* kv,
                            int64_t kvb, emmax_session** out) {
    if (!m || !ws || !kv || !out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(EMMAX_ERR_STATE, "model not finalized");
    int64_t need_ws, need_kv;
    if (int r = emmax_session_bytes_ex(m, max_batch, max_prompt, max_ctx, stage_rows, &need_ws, &need_kv)) return r;
    if (ws_bytes < need_ws || kvb < need_kv)
        return fail(EMMAX_ERR_NOMEM, "session memory too small: workspace %lld/%lld, kv %lld/%lld", (long long)ws_bytes,
                    (long long)need_ws, (long long)kvb, (long long)need_kv);
    if (((uintptr_t)ws % 256) || ((uintptr_t)kv % 256)) return fail(EMMAX_ERR_INVALID, "workspace / kv must be 256-byte aligned");
    if (decode_mfma_init() != 0 || decode_km_init() != 0 || decode_kmp_init() != 0)
        return fail(EMMAX_ERR_HIP, "could not raise the dynamic LDS limit of the MFMA decode kernels");
    emmax_session* s = new emmax_session();
    s->m = m;
    s->max_batch = max_batch; s->max_prompt = max_prompt; s->max_ctx = max_ctx;
    session_dims(m, max_batch, max_prompt, max_ctx, &s->max_pages, &s->max_rows);
    s->max_out = max_ctx;
    s->n_stg = stage_rows; s->stg0 = max_batch; s->rows_total = max_batch + s->n_stg;
    s->exact = emmax_tune().exact != 0;
    Bump b{(char*)ws};
    plan_session(s, b);
    s->sg_gid.assign(s->rows_total, -1); s->sg_own.assign(s->rows_total, 0); s->sg_nfull.assign(s->rows_total, 0);
    s->slot_fresh.assign(s->rows_total, 0); s->slot_stg_idx.assign(s->rows_total, -1); s->slot_stg_epoch.assign(s->rows_total, -1);
    s->kv = (bf16*)kv;
    s->kv8 = !s->exact && emmax_tune().kv_fp8 != 0;
    s->kv_fmt = kv_format_now();
    s->kv_layer_stride = kv_layer_bytes(m, s->rows_total, s->max_pages, s->kv_fmt);
    s->kv24 = s->kv_fmt == KV_X24 ? (long long)kv_rows_per_layer(m, s->rows_total, s->max_pages) * m->cfg.head_dim : 0;
    // Every activation buffer starts as zeros, so its padding columns start finite.  They do NOT stay zero: the towers share scratch set 0 at each
    // tower's own pitch, and the bf16 token assembly writes the real columns only, so a padded tower (the tiny SigLIP: D 144 in rows of 256) reads
    // the other tower's leftovers in its padding columns.  What keeps that harmless is that the padded COLUMNS OF THE WEIGHTS are zero
    // (model.hip) and every leftover is a finite value the encode wrote: 0 x finite = 0 in every GEMM, and the norms and the attention read
    // the real columns only (tests/test_vision_stages_gpu.py: the shared-scratch case pins it bit for bit).
    HIPCHK(hipMemset(ws, 0, need_ws));
    HIPCHK(hipMemset(s->hidden, 0xff, (size_t)s->rows_total * s->max_pages * 4));   // no row hides a page
    HIPCHK(hipMemset(kv, 0, need_kv));
    HIPCHK(hipDeviceSynchronize());
    if (decode_gemv_init() != 0) return fail(EMMAX_ERR_HIP, "could not raise the dynamic LDS limit of the GEMV kernels");
    HIPCHK(hipHostMalloc((void**)&s->pinned, PINNED_BYTES, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s->ev_out, hipEventDisableTiming));
    HIPCHK(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&s->vis_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&s->ev_vfork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s->ev_vjoin, hipEventDisableTiming));
    // static page assignment: row b owns pages [b*max_pages, (b+1)*max_pages)
    {
        std::vector<int32_t> pt((size_t)s->rows_total * s->max_pages);
        for (size_t i = 0; i < pt.size(); ++i) pt[i] = (int32_t)i;
        HIPCHK(hipMemcpy(s->page_table, pt.data(), pt.size() * 4, hipMemcpyHostToDevice));
        for (int t = 0; t < 2; ++t) {
            std::vector<int32_t> cu(max_batch + 1);
            for (int i = 0; i <= max_batch; ++i) cu[i] = i * m->tw[t].N;
            HIPCHK(hipMemcpy(s->cu_vit[t], cu.data(), cu.size() * 4, hipMemcpyHostToDevice));
        }
        // RoPE tables, fp32, HF LlamaRotaryEmbedding order of operations (inv_freq fp32, pos*inv_freq fp32, cos/sin)
        const int half = m->cfg.head_dim / 2;
        std::vector<float> cs((size_t)max_ctx * half), sn((size_t)max_ctx * half);
        for (int i = 0; i < half; ++i) {
            const float inv = 1.0f / powf(m->cfg.rope_theta, (float)(2 * i) / (float)m->cfg.head_dim);
            for (int p = 0; p < max_ctx; ++p) {
                const float f = (float)p * inv;
                cs[(size_t)p * half + i] = (float)cos((double)f);
                sn[(size_t)p * half + i] = (float)sin((double)f);
            }
        }
        HIPCHK(hipMemcpy(s->cos_t, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s->sin_t, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
    }
    *out = s;
    return 0;
}

void emmax_session_destroy(emmax_session* s) {
    if (!s) return;
    drop_graph(s);
    if (s->pinned) (void)hipHostFree(s->pinned);
    if (s->ev) (void)hipEventDestroy(s->ev);
    if (s->ev_in) (void)hipEventDestroy(s->ev_in);
    if (s->ev_out) (void)hipEventDestroy(s->ev_out);
    if (s->own_stream) (void)hipStreamDestroy(s->own_stream);
    if (s->vis_stream) (void)hipStreamDestroy(s->vis_stream);
    if (s->ev_vfork) (void)hipEventDestroy(s->ev_vfork);
    if (s->ev_vjoin) (void)hipEventDestroy(s->ev_vjoin);
    delete s;
}

}  // extern "C"
