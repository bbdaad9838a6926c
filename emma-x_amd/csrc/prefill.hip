// prefill.hip -- the packed prefill (bf16 and exact numerics): per-row state, the decoder layers as GEMMs over all prompt rows, the
// first token through the step's lm-head and finish (step.hip); emmax_prefill* and emmax_prefill_logits.
#include "session.h"

// the prefill in exact numerics: fp32 residual rows (ph32), every GEMM over two-term A operands with fp32 results, fp32 RoPE, fp32 K / V
// into the fp32 cache, fp32-MFMA causal attention; semantics as run_prefill (modeling_prismatic.py:362-415, HF LlamaDecoderLayer)
static int run_prefill_x(emmax_session* s, const int32_t* ids, int B, int P_max, const void* patches, int np, int total, int maxS, int r0, hipStream_t st) {
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    // patch rows: fp32 [B, n_patches, hidden] -- what emmax_vision_encode* hands out in an exact session (the session's own copy when the caller passes none)
    KCHK(launch_x_embed_splice(ids, P_max, s->cu, m->embed, (const float*)patches, nullptr, s->ph32, B, maxS, np, m->H, m->vocab, st));
    s->p32 = true;
    auto into_stream = [&](GemmParams& g) { g.C = s->ph32; g.ldc = m->H; g.residual = s->ph32; g.res_f32 = 1; g.ldr = m->H; };
    for (int li = 0; li < c.n_layers; ++li) {
        const LayerW& L = m->layers[li];
        KCHK(launch_x_rmsnorm(s->ph32, s->xhla, L.ln1, total, m->H, m->H, 2 * m->H, c.rms_eps, st));
        GemmParams g = gpx(s, s->xhla, m->H, L.proj[STAGE_QKV].rm, m->H, s->x32a, m->qkv_dim, total, m->qkv_dim);
        KCHK(launch_gemm(g, st));
        KCHK(launch_x_rope_kv_write(s->x32a, m->qkv_dim, 0, m->q_dim, m->q_dim + m->kv_dim, s->cu, B, total, s->cos_t, s->sin_t, kcache_of(s, li),
                                    vcache_of(s, li), s->kv24, s->page_table + (size_t)r0 * s->max_pages, s->max_pages, c.n_heads, c.n_kv_heads, c.head_dim, PAGE, st));
        AttnParams a;
        a.qkv = s->x32a; a.out = s->xhlb; a.cu_seqlens = s->cu;
        a.ld_qkv = m->qkv_dim; a.q_off = 0; a.k_off = m->q_dim; a.v_off = m->q_dim + m->kv_dim; a.ld_out = 2 * m->q_dim;
        a.B = B; a.max_seqlen = maxS; a.Hq = c.n_heads; a.Hkv = c.n_kv_heads;
        a.scale = 1.0f / sqrtf((float)c.head_dim); a.causal = 1;
        KCHK(launch_x_attention(a, c.head_dim, st));
        g = gpx(s, s->xhlb, m->q_dim, L.proj[STAGE_OPROJ].rm, m->q_dim, nullptr, 0, total, m->H);
        into_stream(g);
        KCHK(launch_gemm(g, st));
        KCHK(launch_x_rmsnorm(s->ph32, s->xhla, L.ln2, total, m->H, m->H, 2 * m->H, c.rms_eps, st));
        g = gpx(s, s->xhla, m->H, L.proj[STAGE_GATEUP].rm, m->H, s->x32a, m->inter_p, total, 2 * m->inter_p);
        g.act = 2;
        KCHK(launch_gemm(g, st));
        KCHK(launch_x_split_rows(s->x32a, s->xhlb, total, m->inter_p, m->inter_p, m->inter_p, 2 * m->inter_p, st));
        g = gpx(s, s->xhlb, m->inter_p, L.proj[STAGE_DOWN].rm, m->inter_p, nullptr, 0, total, m->H);
        into_stream(g);
        KCHK(launch_gemm(g, st));
    }
    KCHK(launch_gather_last_rows(s->ph, s->dh + (size_t)r0 * m->H, s->cu, B, m->H, st, s->dh32 + (size_t)r0 * m->H, s->ph32));
    if (int r = s->grp_N ? run_group_fork(s, B, st) : run_lm_head_step(s, B, true, nullptr, true, st, r0)) return r;
    s->prefilled = true;
    s->beam.ready = s->beam.K != 0;
    return 0;
}

// The decoder layers over the packed rows in s->ph / s->ph32 (embedded by the caller) and the gather of every sequence's last row into the decode
// rows r0 ..: shared by the prefill (ext == nullptr: rows at positions 0 .., causal attention inside the qkv buffer) and by the extension of a cached
// context (extend.hip: ext = the extension attention's plan)
int run_prefill_layers(emmax_session* s, int B, int total, int maxS, int r0, const ExtendAttnPlan* ext, hipStream_t st) {
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    const bool p32 = s->p32;
    auto input_norm = [&](const void* w) {
        return p32 ? launch_rmsnorm_f32(s->ph32, s->pxn, w, total, m->H, m->H, m->H, c.rms_eps, st)
                   : launch_rmsnorm(s->ph, s->pxn, w, total, m->H, m->H, m->H, c.rms_eps, st);
    };
    auto into_stream = [&](GemmParams& g) {   // C = residual stream += A W^T
        if (p32) { g.C = s->ph32; g.out_f32 = 1; g.residual = s->ph32; g.res_f32 = 1; }
        else { g.residual = s->ph; }
        g.ldr = m->H;
    };
    // the RMSNorm behind a projection whose partial tiles meet in a split-K reduce pass (one-frame prefill: o-proj, down) is applied
    // by that pass (gemm_fuses_norm); otherwise it is its own launch
    auto with_norm = [&](GemmParams& g, const void* w) {
        g.norm_w = w; g.norm_out = s->pxn; g.ld_norm = m->H; g.norm_eps = c.rms_eps;
        if (gemm_fuses_norm(g)) return true;
        g.norm_w = nullptr; g.norm_out = nullptr;
        return false;
    };
    bool normed = false;   // s->pxn already holds ln1 of the current layer
    for (int li = 0; li < c.n_layers; ++li) {
        const LayerW& L = m->layers[li];
        if (!normed) KCHK(input_norm(L.ln1));
        GemmParams g = gps(s, s->pxn, m->H, L.proj[STAGE_QKV].rm, m->H, s->pqkv, m->qkv_dim, total, m->qkv_dim, m->H);
        KCHK(launch_gemm(g, st));
        const int32_t* ptab = s->page_table + (size_t)r0 * s->max_pages;
        if (ext) {
            // the rows sit at position ext_base[b] + i: RoPE, the K / V append and the attention take that offset from the device, and the attention
            // reads keys and values from the paged cache alone -- the cached prefix and the rows just appended (extend_attn.hip)
            KCHK(launch_rope_kv_write_at(s->pqkv, m->qkv_dim, 0, m->q_dim, m->q_dim + m->kv_dim, s->cu, s->ext_base, B, total, s->cos_t, s->sin_t,
                                         s->kv8 ? nullptr : kcache_of(s, li), s->kv8 ? nullptr : vcache_of(s, li), ptab, s->max_pages, c.n_heads, c.n_kv_heads,
                                         c.head_dim, PAGE, s->max_ctx, st));
            if (s->kv8)
                KCHK(launch_kv_quant_rows_at(s->pqkv, m->qkv_dim, m->q_dim, m->q_dim + m->kv_dim, s->cu, s->ext_base, B, total, kcache_of(s, li), vcache_of(s, li),
                                             kscale_of(s, li), vscale_of(s, li), ptab, s->max_pages, c.n_kv_heads, c.head_dim, PAGE, st));
            if (int r = tap_pass_attn(s, li, B, total, maxS, r0, true, st)) return r;
            ExtendAttnParams a;
            memset(&a, 0, sizeof(a));
            a.q = s->pqkv; a.ldq = m->qkv_dim; a.q_off = 0; a.out = s->patt; a.ld_out = m->q_dim;
            a.kcache = kcache_of(s, li); a.vcache = vcache_of(s, li);
            if (s->kv8) { a.kscale = kscale_of(s, li); a.vscale = vscale_of(s, li); }
            a.page_table = ptab; a.cu = s->cu; a.base = s->ext_base; a.part = s->splitk_ws;   // (the split-K scratch is idle between two GEMMs)
            a.B = B; a.Hq = c.n_heads; a.Hkv = c.n_kv_heads; a.max_pages = s->max_pages; a.scale = 1.0f / sqrtf((float)c.head_dim);
            KCHK(launch_extend_attn(a, *ext, total, st));
        } else {
            // (fp8 KV cache: the pass rotates q / k in place only, the quantising pass appends K and V as e4m3 rows + scales)
            KCHK(launch_rope_kv_write(s->pqkv, m->qkv_dim, 0, m->q_dim, m->q_dim + m->kv_dim, s->cu, B, total, s->cos_t, s->sin_t,
                                      s->kv8 ? nullptr : kcache_of(s, li), s->kv8 ? nullptr : vcache_of(s, li), s->page_table + (size_t)r0 * s->max_pages,
                                      s->max_pages, c.n_heads, c.n_kv_heads, c.head_dim, PAGE, st));
            if (s->kv8)
                KCHK(launch_kv_quant_rows(s->pqkv, m->qkv_dim, m->q_dim, m->q_dim + m->kv_dim, s->cu, B, total, kcache_of(s, li), vcache_of(s, li),
                                          kscale_of(s, li), vscale_of(s, li), s->page_table + (size_t)r0 * s->max_pages, s->max_pages, c.n_kv_heads,
                                          c.head_dim, PAGE, st));
            if (int r = tap_pass_attn(s, li, B, total, maxS, r0, false, st)) return r;   // (the layer's keys are in the cache: the map reads them there)
            AttnParams a;
            a.qkv = s->pqkv; a.out = s->patt; a.cu_seqlens = s->cu;
            a.ld_qkv = m->qkv_dim; a.q_off = 0; a.k_off = m->q_dim; a.v_off = m->q_dim + m->kv_dim; a.ld_out = m->q_dim;
            a.B = B; a.max_seqlen = maxS; a.Hq = c.n_heads; a.Hkv = c.n_kv_heads;
            a.scale = 1.0f / sqrtf((float)c.head_dim); a.causal = 1;
            KCHK(launch_attention(a, c.head_dim, st));
        }
        g = gps(s, s->patt, m->q_dim, L.proj[STAGE_OPROJ].rm, m->q_dim, s->ph, m->H, total, m->H, m->q_dim);
        into_stream(g);
        normed = with_norm(g, L.ln2);
        KCHK(launch_gemm(g, st));
        if (!normed) KCHK(input_norm(L.ln2));
        g = gps(s, s->pxn, m->H, L.proj[STAGE_GATEUP].rm, m->H, s->pact, m->inter_p, total, 2 * m->inter_p, m->H);
        g.act = 2;
        KCHK(launch_gemm(g, st));
        g = gps(s, s->pact, m->inter_p, L.proj[STAGE_DOWN].rm, m->inter_p, s->ph, m->H, total, m->H, m->inter_p);
        into_stream(g);
        normed = li + 1 < c.n_layers && with_norm(g, m->layers[li + 1].ln1);
        KCHK(launch_gemm(g, st));
        if (int r = tap_pass_hidden(s, li + 1, total, st)) return r;
    }
    taps_unbind(s, true, false);   // consumed by this pass
    KCHK(launch_gather_last_rows(s->ph, s->dh + (size_t)r0 * m->H, s->cu, B, m->H, st, h32_of(s, r0), p32 ? s->ph32 : nullptr));
    return 0;
}

// patches == nullptr: language-only forward (no patch rows are spliced in; modeling_prismatic.py:343-359)
// slot0 >= 0: slot serving -- the B (= 1) rows land in rows slot0.. of the live decode batch, whose other rows are untouched
int run_prefill(emmax_session* s, const int32_t* ids, const int32_t* lens, int B, int P_max, const void* patches, hipStream_t st, int slot0) {
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    if (!m->finalized) return fail(EMMAX_ERR_STATE, "model not finalized");
    // (an exact session was checked against the shapes its two-term kernels take when it was created, and chunks larger batches: check_exact)
    const int max_rows = session_max_rows(s);
    if (B <= 0 || B > s->max_batch || B > max_rows) {
        // (block-scaled tiles: the model's limit binds -- it can move after the session was created, with the attention switches)
        const bool mx_limit = m->is_mx() && B >= 1 && B <= s->max_batch;
        return fail(EMMAX_ERR_INVALID, "prefill batch %d outside 1..min(max_batch=%d, %d) (%s%s%s)", B, s->max_batch, max_rows, mx_limit ? "the limit of a model with " : "",
                    mx_limit ? m->wfmt_name() : "",
                    mx_limit ? " decode weights, re-read at every prefill: emmax_model_max_decode_batch"
                             : "decode batches above 8 need the shapes decode_km.hip takes: emmax_model_max_decode_batch");
    }
    if (B >= EMMAX_MFMA_MIN_BATCH && !m->aux_built)
        return fail(EMMAX_ERR_STATE, "batch %d decodes on the fragment-major weight copies: call emmax_model_build_aux first", B);
    const int np = patches ? m->tw[0].n_patches : 0;
    const bool slot_mode = slot0 >= 0;
    const int r0 = slot_mode ? slot0 : 0;
    if (!slot_mode)   // a plain prefill ends slot serving: the pages that followers of a group hide go back into their rows first
        if (int r = slots_restore_pages(s, st)) return r;
    if (s->beam.K) {   // beams on: B groups, one prefilled row each, forked into B x K rows by emmax_generate
        if (slot_mode) return fail(EMMAX_ERR_STATE, "request slots are not served while beams are on");
        const int rows = B * s->beam.K;
        if (rows > s->max_batch || rows > max_rows)
            return fail(EMMAX_ERR_INVALID, "%d groups x %d beams exceed min(max_batch=%d, %d) rows", B, s->beam.K, s->max_batch, max_rows);
        if (rows >= EMMAX_MFMA_MIN_BATCH && !m->aux_built)
            return fail(EMMAX_ERR_STATE, "%d beam rows decode on the fragment-major weight copies: call emmax_model_build_aux first", rows);
        for (int b = 0; b < B; ++b)
            if (lens[b] >= 1 && !beam_pages_fit(s, np + lens[b], 1))
                return fail(EMMAX_ERR_NOMEM, "group %d: a context of %d tokens leaves its %d beams no spare pages (%d pages per row)", b, np + lens[b], s->beam.K, s->max_pages);
        KCHK(launch_beam_pages(s->page_table, B, s->max_pages, s->beam.K, st));   // row g over the pool of group g: the pages of rows g K ..
        s->beam.G = B; s->beam.forked = false; s->beam.ready = false;
    }
    if (s->grp_N) {   // sample groups on: B prompts, one prefilled row each, forked into B x N sampled rows behind the lm-head (run_group_fork)
        if (slot_mode) return fail(EMMAX_ERR_STATE, "request slots are not served while sample groups are on");
        if (!s->samp.on)
            return fail(EMMAX_ERR_STATE, "sample groups need sampling: %d greedy rows of one prompt would be identical (emmax_session_set_sampling)", s->grp_N);
        const int rows = B * s->grp_N;
        if (rows > s->max_batch || rows > max_rows)
            return fail(EMMAX_ERR_INVALID, "%d groups x %d samples exceed min(max_batch=%d, %d) rows", B, s->grp_N, s->max_batch, max_rows);
        if (rows >= EMMAX_MFMA_MIN_BATCH && !m->aux_built)
            return fail(EMMAX_ERR_STATE, "%d sampled rows decode on the fragment-major weight copies: call emmax_model_build_aux first", rows);
        KCHK(launch_beam_pages(s->page_table, B, s->max_pages, s->grp_N, st));   // row g over the first pages of group g's pool: those of row g N
    }
    if (slot_mode) {
        if (!s->slots_open) return fail(EMMAX_ERR_STATE, "slot prefill before emmax_slots_open");
        if (r0 >= s->stg0) {   // staging rows
            if (r0 + B > s->rows_total) return fail(EMMAX_ERR_INVALID, "%d requests exceed the %d staging rows", B, s->n_stg);
        } else if (r0 + B > s->cur_B) return fail(EMMAX_ERR_INVALID, "slot %d outside the %d open slots", r0, s->cur_B);
        if ((int)s->S.size() < s->rows_total) s->S.resize(s->rows_total, 0);
    } else {
        s->S.assign(s->rows_total, 0);
        s->slots_open = false;
    }
    int total = 0, maxS = 0;
    PrefillState ps;
    ps.B = B;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] > P_max || lens[b] > s->max_prompt)
            return fail(EMMAX_ERR_INVALID, "row %d: prompt length %d outside 1..min(P_max=%d, max_prompt=%d)", b, lens[b], P_max, s->max_prompt);
        const int Sb = np + lens[b];
        if (Sb + 1 > s->max_ctx) return fail(EMMAX_ERR_NOMEM, "row %d: %d prompt+patch tokens do not fit max_ctx %d", b, Sb, s->max_ctx);
        s->S[r0 + b] = Sb;
        ps.S[b] = Sb;
        total += Sb;
        maxS = std::max(maxS, Sb);
    }
    if (total > s->max_rows) return fail(EMMAX_ERR_NOMEM, "packed prefill rows %d exceed capacity %d", total, s->max_rows);
    if (int r = tap_pass_check(s, maxS, "prefill")) return r;
    if (!slot_mode) taps_unbind(s, false, true);   // step taps were bound for the rows of the last pass
    KCHK(launch_prefill_state(ps, s->cu, s->rows.from(r0, s->max_out), st));
    if (s->aut.on) {   // the rows enter the automaton at their start states (sample groups: the B x N rows the prefill forks into)
        const int rows = s->grp_N && !slot_mode ? B * s->grp_N : B;
        HIPCHK(hipMemcpyAsync(s->aut.state + r0, s->aut.start + r0, (size_t)rows * 4, hipMemcpyDeviceToDevice, st));
    }
    if (s->scores.on && !slot_mode && !s->beam.K) {   // the score buffers' rows: the first prefill after the binding's; another batch size unbinds them
        const int rows = s->grp_N ? B * s->grp_N : B;   // (sample groups: the B x N rows the prefill forks into)
        if (s->scores.rows == 0) {
            s->scores.rows = rows;
            KCHK(launch_set_int((int32_t*)(s->scores.words + 3), rows, st));
        } else if (s->scores.rows != rows) {
            s->scores.on = false;
        }
    }
    if (s->proc.on) {   // the rows' prompt ids: the history the processors read
        HistParams h;
        memset(&h, 0, sizeof(h));
        h.ids = ids; h.P_max = P_max; h.B = B; h.max_prompt = s->max_prompt;
        h.dst = s->proc.hist + (size_t)r0 * s->max_prompt; h.dst_len = s->proc.hist_len + r0;
        for (int b = 0; b < B; ++b) h.len[b] = lens[b];
        KCHK(launch_hist_fill(h, st));
    }
    if (!slot_mode) { s->cur_B = B; s->dec_steps = 0; }
    s->total_rows = total; s->max_seqlen = maxS;
    if (s->exact) return run_prefill_x(s, ids, B, P_max, patches, np, total, maxS, r0, st);

    // fp32 residual stream (tuning switch resid32 = 1; 2 = the decode step only): o-proj and down add into fp32 rows -- through the
    // split-K reduce passes of a one-frame prefill, through the direct fp32 epilogue of the big GEMMs otherwise -- and the RMSNorms read
    // them; the stream is rounded to bf16 only where a GEMM consumes the normalised rows
    const bool p32 = emmax_tune().resid32 == 1;
    s->p32 = p32;
    KCHK(launch_embed_splice(ids, P_max, s->cu, m->embed, patches, s->ph, B, maxS, np, m->H, m->vocab, st, p32 ? s->ph32 : nullptr));
    if (int r = tap_pass_hidden(s, 0, total, st)) return r;
    if (int r = run_prefill_layers(s, B, total, maxS, r0, nullptr, st)) return r;
    if (int r = s->grp_N ? run_group_fork(s, B, st) : run_lm_head_step(s, B, true, nullptr, true, st, r0)) return r;
    s->prefilled = true;
    s->beam.ready = s->beam.K != 0;
    return 0;
}

extern "C" {

int emmax_prefill(emmax_session* s, const int32_t* ids, const int32_t* lens, int B, int P_max, const void* patches, emmax_stream st) {
    if (!s || !ids || !lens) return fail(EMMAX_ERR_INVALID, "null argument");
    const void* pe = patches ? patches : (s->exact ? (const void*)s->xpe32 : (const void*)s->patch_embeds);
    if (!patches && s->vision_B != B) return fail(EMMAX_ERR_STATE, "no patch embeddings for batch %d (call emmax_vision_encode first)", B);
    return run_prefill(s, ids, lens, B, P_max, pe, (hipStream_t)st);
}

int emmax_prefill_text(emmax_session* s, const int32_t* ids, const int32_t* lens, int B, int P_max, emmax_stream st) {
    if (!s || !ids || !lens) return fail(EMMAX_ERR_INVALID, "null argument");
    return run_prefill(s, ids, lens, B, P_max, nullptr, (hipStream_t)st);
}

int emmax_prefill_logits(emmax_session* s, float* out, emmax_stream stream) {
    if (!s || !out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "prefill has not run");
    emmax_model* m = s->m;
    hipStream_t st = (hipStream_t)stream;
    if (s->exact) {
        KCHK(launch_x_rmsnorm(s->ph32, s->xhla, m->final_norm, s->total_rows, m->H, m->H, 2 * m->H, m->cfg.rms_eps, st));
        GemmParams gx = gpx(s, s->xhla, m->H, m->lm_head_w.rm, m->H, out, m->vocab, s->total_rows, m->vocab_p);
        gx.N_store = m->vocab;
        KCHK(launch_gemm(gx, st));
        return 0;
    }
    if (s->p32) KCHK(launch_rmsnorm_f32(s->ph32, s->pxn, m->final_norm, s->total_rows, m->H, m->H, m->H, m->cfg.rms_eps, st));
    else KCHK(launch_rmsnorm(s->ph, s->pxn, m->final_norm, s->total_rows, m->H, m->H, m->H, m->cfg.rms_eps, st));
    GemmParams g = gps(s, s->pxn, m->H, m->lm_head_w.rm, m->H, out, m->vocab, s->total_rows, m->vocab_p, m->H);
    g.N_store = m->vocab; g.out_f32 = 1;
    KCHK(launch_gemm(g, st));
    return 0;
}

// the rows emmax_prefill_logits would multiply out, scored in place (score.hip): the same final norm into pxn, then lse / target logit / argmax per
// row through the split-K scratch (idle between two GEMMs).  Nothing a later step or emmax_prefill_logits reads is touched.
int emmax_prefill_score(emmax_session* s, const int32_t* targets, float* lse_out, float* target_logit_out, int32_t* argmax_out, emmax_stream stream) {
    if (!s || !targets || !lse_out || !target_logit_out || !argmax_out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "emmax_prefill_score: prefill has not run");
    if (s->exact) return fail(EMMAX_ERR_STATE, "emmax_prefill_score: exact-numerics sessions are not scored (the scoring kernel has no two-term form)");
    emmax_model* m = s->m;
    hipStream_t st = (hipStream_t)stream;
    ScoreForm f;
    if (!score_form(s->total_rows, m->vocab, m->H, s->splitk_bytes, 0, &f))
        return fail(EMMAX_ERR_INVALID, "emmax_prefill_score: no scoring plan for %d rows x vocab %d x hidden %d (hidden a multiple of 64)", s->total_rows, m->vocab, m->H);
    if (s->p32) KCHK(launch_rmsnorm_f32(s->ph32, s->pxn, m->final_norm, s->total_rows, m->H, m->H, m->H, m->cfg.rms_eps, st));
    else KCHK(launch_rmsnorm(s->ph, s->pxn, m->final_norm, s->total_rows, m->H, m->H, m->H, m->cfg.rms_eps, st));
    ScoreParams p;
    memset(&p, 0, sizeof(p));
    p.X = s->pxn; p.W = m->lm_head_w.rm; p.targets = targets; p.ws = s->splitk_ws; p.lse = lse_out; p.target_logit = target_logit_out; p.argmax = argmax_out;
    p.ldx = m->H; p.ldw = m->H; p.rows = s->total_rows; p.V = m->vocab; p.K = m->H;
    KCHK(launch_score_rows(p, f, st));
    return 0;
}

}  // extern "C"
