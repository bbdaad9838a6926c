// generate.hip -- the calls that drive decode steps: emmax_decode_step, emmax_generate (greedy / sampled / processing / beams), the last
// logits, and slot serving (continuous batching: open, prefill into slots or staging rows, commit, step, state, output, release).
#include "session.h"

int slots_restore_pages(emmax_session* s, hipStream_t st) {
    if (s->sg_followers) KCHK(launch_slots_unhide(s->page_table, s->hidden, s->rows_total * s->max_pages, st));
    s->sg_followers = 0;
    std::fill(s->sg_gid.begin(), s->sg_gid.end(), -1);
    std::fill(s->sg_own.begin(), s->sg_own.end(), 0);
    return 0;
}

// a slot that a prefill or a commit is about to fill must not be a member of a live group: its table row names pages it does not own
static int check_not_in_group(const emmax_session* s, int slot, const char* what) {
    if (s->sg_gid[slot] >= 0)
        return fail(EMMAX_ERR_STATE, "%s: slot %d still belongs to a sample group (emmax_slot_release it first)", what, slot);
    return 0;
}

extern "C" {

int emmax_last_logits(emmax_session* s, float* out, emmax_stream stream) {
    if (!s || !out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "prefill has not run");
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "emmax_last_logits is not served while beams are on (bind a logits buffer: emmax_session_set_scores)");
    if (s->grp_N && s->dec_steps == 0) {   // no step since the group prefill: the last logits are the groups' rows as the fork handed them out
        HIPCHK(hipMemcpyAsync(out, s->logits, (size_t)s->cur_B * s->m->vocab * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return 0;
    }
    return run_lm_head_step(s, s->cur_B, false, out, false, (hipStream_t)stream);
}

int emmax_decode_step(emmax_session* s, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "decode before prefill");
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "with beams on the decode steps run inside emmax_generate");
    s->dec_steps += 1;
    if (emmax_tune().graph) {   // the step is a replay of the captured hipGraph (as in emmax_generate / emmax_slots_step)
        StreamScope sc(s, stream);
        if (sc.error()) return sc.error();
        const hipStream_t st = sc.stream();
        if (int r = ensure_graph(s, s->cur_B, st) == 0 ? launch_graph_step(s, s->cur_B, st) : run_decode_step(s, s->cur_B, st)) return r;
        return sc.leave();
    }
    s->last_step_graph = 0;   // eager mode: emmax_session_graph_active() reports what the steps really do; the graph is kept
    return run_decode_step(s, s->cur_B, (hipStream_t)stream);
}

int emmax_set_current_tokens(emmax_session* s, const int32_t* toks, emmax_stream st) {
    if (!s || !toks) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "no active sequences");
    if (s->slots_open) return fail(EMMAX_ERR_STATE, "caller-supplied tokens are not supported while request slots are open");
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "caller-supplied tokens are not supported while beams are on");
    if (s->proc.on) return fail(EMMAX_ERR_STATE, "caller-supplied tokens are not supported while logits processing is on (they would be missing from the history)");
    // the rows decode again (done flag cleared): the next step appends at position <= S_b + dec_steps, which must exist
    int maxS = 0;
    for (int b = 0; b < s->cur_B && b < (int)s->S.size(); ++b) maxS = std::max(maxS, s->S[b]);
    if (maxS + s->dec_steps + 1 >= s->max_ctx)
        return fail(EMMAX_ERR_NOMEM, "context %d + 1 reaches max_ctx %d: no room to decode a caller-supplied token", maxS + s->dec_steps, s->max_ctx);
    KCHK(launch_set_tokens(s->rows, toks, s->cur_B, s->max_out, (hipStream_t)st));
    return 0;
}

int emmax_generate(emmax_session* s, int max_new, int stop_on_eos, int32_t* out_ids, int32_t* out_lens, emmax_stream stream) {
    if (!s || !out_ids || !out_lens) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "generate before prefill");
    if (max_new < 1 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "max_new_tokens %d outside 1..%d", max_new, s->max_out);
    if (s->beam.K) {
        if (!s->beam.ready || s->beam.forked) return fail(EMMAX_ERR_STATE, "with beams on emmax_generate runs once per prefill (the prefill must follow emmax_session_set_beams)");
        for (int g = 0; g < s->beam.G; ++g)
            if (!beam_pages_fit(s, s->S[g], max_new))
                return fail(EMMAX_ERR_NOMEM, "group %d: context %d + %d new tokens x %d beams do not fit max_ctx %d / the %d pages of its rows", g, s->S[g], max_new,
                            s->beam.K, s->max_ctx, s->beam.K * s->max_pages);
    }
    StreamScope sc(s, stream);   // (the loop may replay a captured graph)
    if (sc.error()) return sc.error();
    const hipStream_t st = sc.stream();
    if (s->beam.K) {   // the first beam step from the prefill's logit rows, and the fork into G x K rows
        const int rows = s->beam.G * s->beam.K, ld = std::min(s->max_batch, EMMAX_MAX_DECODE_BATCH);
        s->beam.eos = stop_on_eos ? s->m->cfg.eos_id : -1;
        s->beam.max_new = max_new;
        KCHK(launch_set_ints(s->rows.max_new, rows, max_new, st));
        KCHK(launch_beam_reset(rows, s->beam.K, s->beam.run, s->beam.fin_score, s->beam.fin_flag, s->beam.fin_t, s->beam.fin_par, s->beam.fin_tok, s->beam.grp,
                               s->beam.csrc, st));
        const size_t n1 = (size_t)max_new * ld * 4;
        HIPCHK(hipMemsetAsync(s->beam.tr_tok, 0xff, n1, st));
        HIPCHK(hipMemsetAsync(s->beam.tr_par, 0xff, n1, st));
        HIPCHK(hipMemsetAsync(s->beam.tr_score, 0, n1, st));
        HIPCHK(hipMemsetAsync(s->beam.tr_lse, 0, n1, st));
        HIPCHK(hipMemsetAsync(s->beam.tc_idx, 0xff, 2 * n1, st));
        HIPCHK(hipMemsetAsync(s->beam.tc_acc, 0, 2 * n1, st));
        if (s->scores.on) KCHK(launch_set_int((int32_t*)(s->scores.words + 3), rows, st));
        if (int r = launch_beam_finish(s, true, st)) return r;
        for (int g = s->beam.G - 1; g >= 0; --g)
            for (int k = 0; k < s->beam.K; ++k) s->S[g * s->beam.K + k] = s->S[g];
        s->cur_B = rows;
        s->beam.forked = true;
        s->beam.ready = false;
    }
    const int B = s->cur_B;
    if (!s->beam.K) KCHK(launch_set_ints(s->rows.max_new, B, max_new, st));
    const bool use_graph = (max_new > 2) && ensure_graph(s, B, st) == 0;
    const int CHK = 16;
    int32_t* done_host = s->pinned->done;
    bool pending = false;
    for (int i = 1; i < max_new; ++i) {
        s->dec_steps += 1;
        if (int r = use_graph ? launch_graph_step(s, B, st) : run_decode_step(s, B, st)) return r;
        if (stop_on_eos && (i % CHK) == 0) {
            if (pending) {   // the previous read-back is certainly complete once its event fired
                HIPCHK(hipEventSynchronize(s->ev));
                bool all = true;
                for (int b = 0; b < B; ++b) all = all && (done_host[b] != 0);
                if (all) { pending = false; break; }
            }
            HIPCHK(hipMemcpyAsync(done_host, s->rows.done, B * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventRecord(s->ev, st));
            pending = true;
        }
    }
    if (s->beam.K) {   // the kept hypotheses, best first per group, out of the token / parent tables
        BeamResolveParams q;
        memset(&q, 0, sizeof(q));
        q.rows = B; q.K = s->beam.K; q.max_out = s->max_out; q.max_new = max_new; q.tr_ld = std::min(s->max_batch, EMMAX_MAX_DECODE_BATCH);
        q.pad_id = s->m->cfg.pad_id;
        q.fin_t = s->beam.fin_t; q.fin_par = s->beam.fin_par; q.fin_tok = s->beam.fin_tok; q.tr_tok = s->beam.tr_tok; q.tr_par = s->beam.tr_par;
        q.fin_score = s->beam.fin_score; q.seq = s->rows.out_ids; q.bidx = s->beam.res_bidx; q.len = s->beam.res_len; q.score = s->beam.res_score;
        KCHK(launch_beam_resolve(q, st));
    }
    HIPCHK(hipMemcpy2DAsync(out_ids, (size_t)max_new * 4, s->rows.out_ids, (size_t)s->max_out * 4, (size_t)max_new * 4, B,
                            hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(out_lens, s->beam.K ? s->beam.res_len : s->rows.n_out, B * 4, hipMemcpyDeviceToDevice, st));
    return sc.leave();
}

int emmax_slots_open(emmax_session* s, int n_slots, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "request slots are not served while beams are on (emmax_session_clear_beams)");
    if (s->grp_N) return fail(EMMAX_ERR_STATE, "request slots are not served while sample groups are on (emmax_session_clear_sample_groups)");
    const int max_rows = session_max_rows(s);
    if (n_slots < 1 || n_slots > s->max_batch || n_slots > max_rows) {
        const bool mx_limit = s->m->is_mx() && n_slots >= 1 && n_slots <= s->max_batch;
        return fail(EMMAX_ERR_INVALID, "%d slots outside 1..min(max_batch=%d, %d)%s%s%s", n_slots, s->max_batch, max_rows, mx_limit ? ": the limit of a model with " : "",
                    mx_limit ? s->m->wfmt_name() : "", mx_limit ? " decode weights" : "");
    }
    if (n_slots >= EMMAX_MFMA_MIN_BATCH && !s->m->aux_built)
        return fail(EMMAX_ERR_STATE, "%d slots decode on the fragment-major weight copies: call emmax_model_build_aux first", n_slots);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = slots_restore_pages(s, sc.stream())) return r;   // a group still outstanding from the last serve
    KCHK(launch_slots_idle(n_slots, s->rows, s->m->cfg.pad_id, sc.stream()));
    s->cur_B = n_slots;
    s->S.assign(s->rows_total, 0);
    std::fill(s->slot_fresh.begin(), s->slot_fresh.end(), 0);
    std::fill(s->slot_stg_idx.begin(), s->slot_stg_idx.end(), -1);
    s->slots_open = true;
    s->scores.on = false;   // no scores in slot serving (the bound buffers were a generate call's)
    taps_unbind(s, true, true);   // ... and no taps
    s->prefilled = true;   // decode steps are legal: idle slots are rows that are already done
    return sc.leave();
}

int emmax_slot_prefill(emmax_session* s, int slot, const int32_t* ids, int len, const void* patches, int max_new, emmax_stream stream) {
    if (!s || !ids) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slot_prefill before emmax_slots_open");
    if (slot < 0 || slot >= s->cur_B) return fail(EMMAX_ERR_INVALID, "slot %d outside 0..%d", slot, s->cur_B - 1);
    if (max_new < 1 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "max_new_tokens %d outside 1..%d", max_new, s->max_out);
    if (int r = check_not_in_group(s, slot, "emmax_slot_prefill")) return r;
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    s->slot_fresh[slot] = 0; s->slot_stg_idx[slot] = -1;
    if (int r = run_prefill(s, ids, &len, 1, len, patches, sc.stream(), slot)) return r;
    KCHK(launch_set_ints(s->rows.max_new + slot, 1, max_new, sc.stream()));
    s->slot_fresh[slot] = s->samp.on ? 1 : 0;   // (sampling on: the prefill left the prompt's logit row in the slot's own)
    return sc.leave();
}

int emmax_slots_prefill(emmax_session* s, int slot0, int n, const int32_t* ids, int P_max, const int32_t* lens_host, const void* patches,
                        const int32_t* max_new_host, emmax_stream stream) {
    if (!s || !ids || !lens_host || !max_new_host) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slots_prefill before emmax_slots_open");
    if (n < 1 || slot0 < 0 || slot0 + n > s->cur_B) return fail(EMMAX_ERR_INVALID, "slots %d..%d outside 0..%d", slot0, slot0 + n - 1, s->cur_B - 1);
    for (int i = 0; i < n; ++i)
        if (max_new_host[i] < 1 || max_new_host[i] > s->max_out)
            return fail(EMMAX_ERR_INVALID, "slot %d: max_new_tokens %d outside 1..%d", slot0 + i, max_new_host[i], s->max_out);
    for (int i = 0; i < n; ++i)
        if (int r = check_not_in_group(s, slot0 + i, "emmax_slots_prefill")) return r;
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    for (int i = 0; i < n; ++i) { s->slot_fresh[slot0 + i] = 0; s->slot_stg_idx[slot0 + i] = -1; }
    if (int r = run_prefill(s, ids, lens_host, n, P_max, patches, sc.stream(), slot0)) return r;   // one packed pass over the n requests (ragged lengths)
    for (int i = 0; i < n; ++i) KCHK(launch_set_ints(s->rows.max_new + slot0 + i, 1, max_new_host[i], sc.stream()));
    for (int i = 0; i < n; ++i) s->slot_fresh[slot0 + i] = s->samp.on ? 1 : 0;
    return sc.leave();
}

int emmax_slots_prefill_staged(emmax_session* s, int n, const int32_t* ids, int P_max, const int32_t* lens_host, const void* patches,
                               const int32_t* max_new_host, emmax_stream stream) {
    if (!s || !ids || !lens_host || !max_new_host) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slots_prefill_staged before emmax_slots_open");
    if (s->n_stg == 0)
        return fail(EMMAX_ERR_INVALID, "session created without staging rows: use emmax_session_create_ex(..., stage_rows > 0) (a plain emmax_session_create gives none since ABI 4)");
    if (n < 1 || n > s->n_stg)
        return fail(EMMAX_ERR_INVALID, "%d staged requests outside 1..%d (the session's staging rows: emmax_session_create_ex)", n, s->n_stg);
    if ((uintptr_t)stream <= 2) return fail(EMMAX_ERR_INVALID, "a staged prefill needs its own (non-default) stream: it runs beside the decode steps");
    for (int i = 0; i < n; ++i)
        if (max_new_host[i] < 1 || max_new_host[i] > s->max_out)
            return fail(EMMAX_ERR_INVALID, "staged request %d: max_new_tokens %d outside 1..%d", i, max_new_host[i], s->max_out);
    hipStream_t st = (hipStream_t)stream;
    s->stg_epoch += 1;   // the staging rows' logit rows are this batch's from here on
    s->stg_logits = s->samp.on;
    if (int r = run_prefill(s, ids, lens_host, n, P_max, patches, st, s->stg0)) return r;
    for (int i = 0; i < n; ++i) KCHK(launch_set_ints(s->rows.max_new + s->stg0 + i, 1, max_new_host[i], st));
    return 0;
}

int emmax_slots_commit(emmax_session* s, const int32_t* staged_idx_host, const int32_t* slots_host, int n, emmax_stream stream) {
    if (!s || !slots_host || !staged_idx_host) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slots_commit before emmax_slots_open");
    if (n < 1 || n > s->n_stg) return fail(EMMAX_ERR_INVALID, "%d commits outside 1..%d", n, s->n_stg);
    CommitParams c;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < n; ++i) {
        if (slots_host[i] < 0 || slots_host[i] >= s->cur_B) return fail(EMMAX_ERR_INVALID, "slot %d outside 0..%d", slots_host[i], s->cur_B - 1);
        if (staged_idx_host[i] < 0 || staged_idx_host[i] >= s->n_stg) return fail(EMMAX_ERR_INVALID, "staged request %d outside 0..%d", staged_idx_host[i], s->n_stg - 1);
        for (int j = 0; j < i; ++j)
            if (slots_host[j] == slots_host[i] || staged_idx_host[j] == staged_idx_host[i]) return fail(EMMAX_ERR_INVALID, "slot / staged request named twice");
        if (int r = check_not_in_group(s, slots_host[i], "emmax_slots_commit")) return r;
        c.slot[i] = slots_host[i];
        c.src[i] = s->stg0 + staged_idx_host[i];
    }
    c.n = n; c.max_pages = s->max_pages; c.page_table = s->page_table;
    c.done = s->rows.done; c.ctx_len = s->rows.ctx_len;
    if (int r = session_row_cols(s, &c.cols)) return r;   // the top-N entries a staged request has written move with it like everything else
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    KCHK(launch_slots_commit(c, sc.stream()));
    for (int i = 0; i < n; ++i) {
        const int slot = slots_host[i];
        s->S[slot] = s->S[s->stg0 + staged_idx_host[i]];
        s->slot_fresh[slot] = 0;   // (a commit does not move logit rows: the request's stays in its staging row)
        s->slot_stg_idx[slot] = staged_idx_host[i]; s->slot_stg_epoch[slot] = s->stg_epoch;
    }
    return sc.leave();
}

int emmax_slots_step(emmax_session* s, int n_steps, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slots_step before emmax_slots_open");
    if (n_steps < 1) return fail(EMMAX_ERR_INVALID, "n_steps %d < 1", n_steps);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    const hipStream_t st = sc.stream();
    const int B = s->cur_B;
    const bool use_graph = ensure_graph(s, B, st) == 0;
    std::fill(s->slot_fresh.begin(), s->slot_fresh.end(), 0);   // a sampled step overwrites every slot's logit row
    for (int i = 0; i < n_steps; ++i) {
        if (int r = use_graph ? launch_graph_step(s, B, st) : run_decode_step(s, B, st)) return r;
    }
    return sc.leave();
}

int emmax_slots_state(emmax_session* s, int32_t* done_out, int32_t* n_out_out, emmax_stream stream) {
    if (!s || !done_out || !n_out_out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slots_state before emmax_slots_open");
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    HIPCHK(hipMemcpyAsync(done_out, s->rows.done, s->cur_B * 4, hipMemcpyDeviceToDevice, sc.stream()));
    HIPCHK(hipMemcpyAsync(n_out_out, s->rows.n_out, s->cur_B * 4, hipMemcpyDeviceToDevice, sc.stream()));
    return sc.leave();
}

int emmax_slot_output(emmax_session* s, int slot, int32_t* ids_out, int n, emmax_stream stream) {
    if (!s || !ids_out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slot_output before emmax_slots_open");
    if (slot < 0 || slot >= s->cur_B || n < 0 || n > s->max_out) return fail(EMMAX_ERR_INVALID, "slot %d / %d ids out of range", slot, n);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (n > 0) HIPCHK(hipMemcpyAsync(ids_out, s->rows.out_ids + (size_t)slot * s->max_out, (size_t)n * 4, hipMemcpyDeviceToDevice, sc.stream()));
    return sc.leave();
}

int emmax_slot_release(emmax_session* s, int slot, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slot_release before emmax_slots_open");
    if (slot < 0 || slot >= s->cur_B) return fail(EMMAX_ERR_INVALID, "slot %d outside 0..%d", slot, s->cur_B - 1);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    KCHK(launch_slots_idle(1, s->rows.from(slot, s->max_out), s->m->cfg.pad_id, sc.stream()));
    s->S[slot] = 0;
    s->slot_fresh[slot] = 0; s->slot_stg_idx[slot] = -1;
    if (s->sg_gid[slot] >= 0) {   // a member of a group: a follower takes its hidden pages back; the owner takes its heir's and the heir owns the shared ones
        const int gid = s->sg_gid[slot], nfull = s->sg_nfull[slot], mp = s->max_pages;
        int from = slot;
        if (s->sg_own[slot]) {
            from = -1;
            for (int h = 0; h < s->cur_B && from < 0; ++h)
                if (h != slot && s->sg_gid[h] == gid) from = h;   // the heir: the lowest-numbered live follower
            if (from >= 0) s->sg_own[from] = 1;
        }
        if (from >= 0) {
            if (nfull > 0) KCHK(launch_slots_unhide(s->page_table + (size_t)slot * mp, s->hidden + (size_t)from * mp, nfull, sc.stream()));
            s->sg_followers -= 1;
        }
        s->sg_gid[slot] = -1; s->sg_own[slot] = 0;
    }
    return sc.leave();
}

int emmax_slots_fork(emmax_session* s, int src_slot, int staged_idx, const int32_t* dst_slots_host, int n, const float* temperature_host,
                     const int32_t* top_k_host, const float* top_p_host, const uint64_t* seed_host, const uint32_t* subseq_host, emmax_stream stream) {
    if (!s || !dst_slots_host || !temperature_host || !top_k_host || !top_p_host || !seed_host || !subseq_host) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slots_fork before emmax_slots_open");
    if (n < 1) return fail(EMMAX_ERR_INVALID, "%d followers < 1", n);
    if (!s->samp.on)
        return fail(EMMAX_ERR_STATE, "a fork needs sampling: %d greedy rows of one prompt would be identical (emmax_session_set_sampling)", n + 1);
    if (src_slot < 0 || src_slot >= s->cur_B) return fail(EMMAX_ERR_INVALID, "source slot %d outside 0..%d", src_slot, s->cur_B - 1);
    if (staged_idx < -1 || staged_idx >= s->n_stg) return fail(EMMAX_ERR_INVALID, "staged request %d outside -1..%d", staged_idx, s->n_stg - 1);
    for (int i = 0; i < n; ++i) {
        const int d = dst_slots_host[i];
        if (d < 0 || d >= s->cur_B) return fail(EMMAX_ERR_INVALID, "destination slot %d outside 0..%d", d, s->cur_B - 1);
        if (d == src_slot) return fail(EMMAX_ERR_INVALID, "destination slot %d is the source", d);
        for (int j = 0; j < i; ++j)
            if (dst_slots_host[j] == d) return fail(EMMAX_ERR_INVALID, "destination slot %d named twice", d);
        if (s->S[d] != 0 || s->sg_gid[d] >= 0) return fail(EMMAX_ERR_INVALID, "destination slot %d is not idle (emmax_slot_release it first)", d);
    }
    if (int r = check_sampling_values(s, dst_slots_host, n, temperature_host, top_k_host, top_p_host)) return r;
    if (s->S[src_slot] == 0) return fail(EMMAX_ERR_STATE, "source slot %d holds no request", src_slot);
    if (s->sg_gid[src_slot] >= 0) return fail(EMMAX_ERR_STATE, "source slot %d already belongs to a sample group", src_slot);
    int logit_row = src_slot;
    if (staged_idx < 0) {
        if (s->slot_stg_idx[src_slot] >= 0)
            return fail(EMMAX_ERR_STATE, "source slot %d was committed from staged request %d: its logit row is that staging row's (pass staged_idx)", src_slot,
                        s->slot_stg_idx[src_slot]);
        if (!s->slot_fresh[src_slot])
            return fail(EMMAX_ERR_STATE, "source slot %d: a decode step ran since its prefill (or it was prefilled with sampling off), the prompt's logit row is gone",
                        src_slot);
    } else {
        if (s->slot_stg_idx[src_slot] != staged_idx || s->slot_stg_epoch[src_slot] != s->stg_epoch)
            return fail(EMMAX_ERR_STATE, "staged request %d of source slot %d is not of the current staged batch: an older batch's logit row is gone", staged_idx,
                        src_slot);
        if (!s->stg_logits) return fail(EMMAX_ERR_STATE, "the staged batch was prefilled with sampling off: it left no logit rows");
        logit_row = s->stg0 + staged_idx;
    }
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = upload_fork_sampling(s, n, temperature_host, top_k_host, top_p_host, seed_host, subseq_host, sc.stream())) return r;
    if (int r = run_slots_fork(s, src_slot, logit_row, dst_slots_host, n, sc.stream())) return r;
    const int gid = s->sg_next++;
    s->sg_gid[src_slot] = gid; s->sg_own[src_slot] = 1; s->sg_nfull[src_slot] = s->S[src_slot] / PAGE;
    for (int i = 0; i < n; ++i) {
        const int d = dst_slots_host[i];
        s->S[d] = s->S[src_slot];
        s->sg_gid[d] = gid; s->sg_own[d] = 0; s->sg_nfull[d] = s->S[src_slot] / PAGE;
        s->slot_fresh[d] = 0; s->slot_stg_idx[d] = -1;
    }
    s->sg_followers += n;
    return sc.leave();
}

int emmax_slots_page_state(emmax_session* s, int32_t* table_out_dev, int32_t* hidden_out_dev, emmax_stream stream) {
    if (!s || !table_out_dev || !hidden_out_dev) return fail(EMMAX_ERR_INVALID, "null argument");
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    const size_t bytes = (size_t)s->rows_total * s->max_pages * 4;
    HIPCHK(hipMemcpyAsync(table_out_dev, s->page_table, bytes, hipMemcpyDeviceToDevice, sc.stream()));
    HIPCHK(hipMemcpyAsync(hidden_out_dev, s->hidden, bytes, hipMemcpyDeviceToDevice, sc.stream()));
    return sc.leave();
}

int emmax_session_graph_active(emmax_session* s) {
    if (s && !s->graph_exec && !s->graph_err.empty()) g_err = s->graph_err;   // why the capture was refused
    return s && s->graph_exec && s->last_step_graph ? 1 : 0;
}

}  // extern "C"
