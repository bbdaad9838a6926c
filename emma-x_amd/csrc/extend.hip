// extend.hip -- more tokens on top of a cached context: emmax_extend, emmax_slot_extend, emmax_session_context.  The prefill's pipeline
// (prefill.hip: run_prefill_layers, the layer loop both share) over the packed NEW rows alone; RoPE, the K / V append and the attention take
// the rows' cached lengths from the device (extend_attn.hip), so the keys of the new rows are the cached prefix plus the rows themselves.
#include "session.h"

// what a continuation is not served with -- each with its own message.  The session stays as it was
int extend_refusals(const emmax_session* s, const char* who) {
    if (s->exact) return fail(EMMAX_ERR_STATE, "%s: exact-numerics sessions are not extended (their fp32 / 24-bit cache has no extension attention)", who);
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "%s: not served while beams are on (emmax_session_clear_beams)", who);
    if (s->grp_N) return fail(EMMAX_ERR_STATE, "%s: not served while sample groups are on (emmax_session_clear_sample_groups)", who);
    if (s->proc.on && !s->rules.implied_proc && !s->aut.implied_proc)
        return fail(EMMAX_ERR_STATE,
                    "%s: history-reading processors are on (emmax_session_set_processing): the [rows][max_prompt = %d] id history they read has no room "
                    "for the extension's ids (emmax_session_clear_processing)", who, s->max_prompt);
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "%s: no prefill yet: there is no cached context to extend", who);
    return 0;
}

int run_extend(emmax_session* s, int r0, int B, const int32_t* ids, const int32_t* lens, int P_max, int max_new, bool slot, hipStream_t st) {
    const char* who = slot ? "emmax_slot_extend" : "emmax_extend";
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || r0 < 0 || r0 + B > s->cur_B) return fail(EMMAX_ERR_INVALID, "%s: rows %d..%d outside the %d live rows", who, r0, r0 + B - 1, s->cur_B);
    if ((int)s->S.size() < s->rows_total) s->S.resize(s->rows_total, 0);
    // the rows' cached lengths (and, for a slot, whether its request has finished), read back once: the call is not part of a captured step
    int32_t ctx[EMMAX_MAX_DECODE_BATCH], done[EMMAX_MAX_DECODE_BATCH];
    HIPCHK(hipMemcpyAsync(ctx, s->rows.ctx_len + r0, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(done, s->rows.done + r0, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    PrefillState ps;
    ps.B = B;
    int total = 0, max_n = 0, max_L = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] > P_max) return fail(EMMAX_ERR_INVALID, "%s: row %d: %d new ids outside 1..P_max = %d", who, r0 + b, lens[b], P_max);
        if (ctx[b] < 1) return fail(EMMAX_ERR_STATE, "%s: row %d holds no context (an idle or released row)", who, r0 + b);
        if (slot && !done[b]) return fail(EMMAX_ERR_STATE, "%s: slot %d still decodes: a follow-up extends a finished request", who, r0 + b);
        const long need = (long)ctx[b] + lens[b] + std::max(max_new, 1);
        if (need > s->max_ctx || need > (long)s->max_pages * PAGE)
            return fail(EMMAX_ERR_NOMEM, "%s: row %d: context %d + %d new ids + %d tokens to generate exceed max_ctx %d (the row's %d pages)", who, r0 + b, ctx[b], lens[b],
                        std::max(max_new, 1), s->max_ctx, s->max_pages);
        ps.S[b] = lens[b];
        total += lens[b];
        max_n = std::max(max_n, lens[b]);
        max_L = std::max(max_L, ctx[b] + lens[b]);
    }
    if (total > s->max_rows) return fail(EMMAX_ERR_NOMEM, "%s: %d packed new rows exceed the prefill capacity %d", who, total, s->max_rows);
    if (int r = tap_pass_check(s, max_L, who)) return r;
    if (!slot) taps_unbind(s, false, true);   // step taps were bound for the rows as the last pass left them
    // the key-split workspace is the split-K scratch (idle between two GEMMs): fewer splits if the partials would not fit
    ExtendAttnPlan plan;
    if (!extend_attn_plan(B, max_n, max_L, c.n_heads, c.n_kv_heads, 0, s->kv8 ? 1 : 0, &plan) || c.head_dim != 128)
        return fail(EMMAX_ERR_INVALID, "%s: the extension attention takes head_dim 128 and GQA groups of 1 / 2 / 4 / 8 (heads %d / %d, head_dim %d)", who, c.n_heads, c.n_kv_heads, c.head_dim);
    while (plan.nsplit > 1 && (int64_t)total * c.n_heads * plan.nsplit * EMMAX_PSTRIDE * 4 > s->splitk_bytes) plan.nsplit -= 1;
    plan.split = plan.nsplit > 1 ? 1 : 0;

    KCHK(launch_extend_state(ps, s->cu, s->ext_base, s->rows.from(r0, s->max_out), s->aut.on ? s->aut.state + r0 : nullptr,
                             s->aut.on ? s->aut.start + r0 : nullptr, st));
    if (s->scores.on && !slot) {   // the score buffers' rows, as a prefill binds them: the first pass after the binding's; another batch size unbinds them
        if (s->scores.rows == 0) {
            s->scores.rows = B;
            KCHK(launch_set_int((int32_t*)(s->scores.words + 3), B, st));
        } else if (s->scores.rows != B) {
            s->scores.on = false;
        }
    }
    for (int b = 0; b < B; ++b) s->S[r0 + b] = ctx[b] + lens[b];   // (with dec_steps: still an upper bound of the row's context)
    if (!slot && r0 == 0 && B == s->cur_B) s->dec_steps = 0;       // every live row's length is known exactly again
    s->total_rows = total; s->max_seqlen = max_n;

    const bool p32 = emmax_tune().resid32 == 1;
    s->p32 = p32;
    KCHK(launch_embed_splice(ids, P_max, s->cu, m->embed, nullptr, s->ph, B, max_n, 0, m->H, m->vocab, st, p32 ? s->ph32 : nullptr));
    if (int r = tap_pass_hidden(s, 0, total, st)) return r;
    if (int r = run_prefill_layers(s, B, total, max_n, r0, &plan, st)) return r;   // the prefill's layers, their attention over the paged cache
    // the first token of the continuation, as a prefill picks it (greedy, or the session's sampling / warpers / rules / automaton -- a row keeps
    // its automaton state, one outside the automaton entered at its start state above)
    return run_lm_head_step(s, B, true, nullptr, true, st, r0);
}

extern "C" {

int emmax_extend(emmax_session* s, int row0, int B, const int32_t* ids, const int32_t* lens, int P_max, int max_new, emmax_stream stream) {
    if (!s || !ids || !lens) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = extend_refusals(s, "emmax_extend")) return r;
    if (s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_extend: the rows are request slots (emmax_slot_extend extends one of them)");
    if (max_new < 0 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "emmax_extend: max_new_tokens %d outside 0..%d", max_new, s->max_out);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = run_extend(s, row0, B, ids, lens, P_max, max_new, false, sc.stream())) return r;
    return sc.leave();
}

int emmax_slot_extend(emmax_session* s, int slot, const int32_t* ids, int len, int max_new, emmax_stream stream) {
    if (!s || !ids) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = extend_refusals(s, "emmax_slot_extend")) return r;
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slot_extend before emmax_slots_open");
    if (slot < 0 || slot >= s->cur_B) return fail(EMMAX_ERR_INVALID, "emmax_slot_extend: slot %d outside 0..%d", slot, s->cur_B - 1);
    if (max_new < 1 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "emmax_slot_extend: max_new_tokens %d outside 1..%d", max_new, s->max_out);
    if (s->sg_gid[slot] >= 0) return fail(EMMAX_ERR_STATE, "emmax_slot_extend: slot %d belongs to a sample group: its prompt pages are shared (emmax_slot_release it first)", slot);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = run_extend(s, slot, 1, ids, &len, len, max_new, true, sc.stream())) return r;
    KCHK(launch_set_ints(s->rows.max_new + slot, 1, max_new, sc.stream()));
    s->slot_fresh[slot] = s->samp.on ? 1 : 0;   // (sampling on: the extension left its last row's logits in the slot's own row, as a slot prefill does)
    s->slot_stg_idx[slot] = -1;
    return sc.leave();
}

int emmax_session_context(emmax_session* s, int row0, int n, int32_t* ctx_out_host, emmax_stream stream) {
    if (!s || !ctx_out_host) return fail(EMMAX_ERR_INVALID, "null argument");
    if (n < 1 || row0 < 0 || row0 + n > s->rows_total) return fail(EMMAX_ERR_INVALID, "emmax_session_context: rows %d..%d outside 0..%d", row0, row0 + n - 1, s->rows_total - 1);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    HIPCHK(hipMemcpyAsync(ctx_out_host, s->rows.ctx_len + row0, (size_t)n * 4, hipMemcpyDeviceToHost, sc.stream()));
    HIPCHK(hipStreamSynchronize(sc.stream()));
    return sc.leave();
}

}  // extern "C"
