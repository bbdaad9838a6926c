// modes.hip -- how a session's steps end, configured: the stop rule, sampling, logits processing, scores and beam search -- the host checks,
// the upload of the per-row parameters, and the calls that hand the results back (log-probabilities, beam result and trace).
#include <initializer_list>

#include "session.h"

// One column of a per-row upload: elements of `esize` bytes, from a host array to rows r0 .. of a device array
struct Column { void* dev; const void* host; int esize; };

// rows r0 .. r0 + n of every column: the caller's arrays are pageable, so they go through the pinned upload area, UPLOAD_ROWS rows at a time
static int upload_rows(emmax_session* s, int r0, int n, hipStream_t st, std::initializer_list<Column> cols) {
    char* const h = s->pinned->upload;
    const int chunk = std::min(n, (int)UPLOAD_ROWS);
    auto span = [&](const Column& k) { return ((size_t)chunk * k.esize + 7) / 8 * 8; };   // a column's share of the area
    size_t need = 0;
    for (const Column& k : cols) need += span(k);
    if (need > sizeof(s->pinned->upload)) return fail(EMMAX_ERR_STATE, "an upload of %zu bytes per chunk exceeds the pinned area", need);
    HIPCHK(hipStreamSynchronize(st));   // the pinned staging words may still feed an earlier upload
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int c = std::min(chunk, n - c0);
        size_t off = 0;
        for (const Column& k : cols) {
            const size_t bytes = (size_t)c * k.esize;
            if (bytes) {   // (the stop rule may name no trigger ids)
                memcpy(h + off, (const char*)k.host + (size_t)c0 * k.esize, bytes);
                HIPCHK(hipMemcpyAsync((char*)k.dev + (size_t)(r0 + c0) * k.esize, h + off, bytes, hipMemcpyHostToDevice, st));
            }
            off += span(k);
        }
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}

// the rows a per-row configuration call names: n decode rows from row0 (emmax_session_set_*), or the first n staging rows (emmax_slots_set_*_staged)
static int check_rows(const emmax_session* s, int row0, int n, bool staged) {
    if (staged) return n < 1 || n > s->n_stg ? fail(EMMAX_ERR_INVALID, "%d staged requests outside 1..%d (the session's staging rows)", n, s->n_stg) : 0;
    return n < 1 || row0 < 0 || row0 + n > s->max_batch ? fail(EMMAX_ERR_INVALID, "rows %d..%d outside 0..%d", row0, row0 + n - 1, s->max_batch - 1) : 0;
}

// ---- sampling in the decode step (ABI 7) ------------------------------------------------------------------------------
int check_sampling_values(const emmax_session* s, const int32_t* rows, int n, const float* T, const int32_t* top_k, const float* top_p) {
    if (s->m->vocab > EMMAX_SAMPLE_MAX_V) return fail(EMMAX_ERR_INVALID, "sampling takes vocabularies of up to %d entries (%d)", EMMAX_SAMPLE_MAX_V, s->m->vocab);
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(T[i]) || T[i] < 0.f) return fail(EMMAX_ERR_INVALID, "row %d: temperature %g (finite and >= 0)", rows[i], (double)T[i]);
        if (top_k[i] < 0) return fail(EMMAX_ERR_INVALID, "row %d: top_k %d (>= 0)", rows[i], top_k[i]);
        if (!(top_p[i] > 0.f && top_p[i] <= 1.f)) return fail(EMMAX_ERR_INVALID, "row %d: top_p %g (0 < top_p <= 1)", rows[i], (double)top_p[i]);
    }
    return 0;
}

int upload_fork_sampling(emmax_session* s, int n, const float* T, const int32_t* top_k, const float* top_p, const uint64_t* seed, const uint32_t* subseq,
                         hipStream_t st) {
    return upload_rows(s, 0, n, st, {{s->fork_t, T, 4}, {s->fork_k, top_k, 4}, {s->fork_p, top_p, 4}, {s->fork_sub, subseq, 4}, {s->fork_seed, seed, 8}});
}

static int set_sampling_rows(emmax_session* s, int row0, int n, bool staged, const float* T, const int32_t* top_k, const float* top_p, const uint64_t* seed,
                             const uint32_t* subseq, emmax_stream stream) {
    if (!s || !T || !top_k || !top_p || !seed || !subseq) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = check_rows(s, row0, n, staged)) return r;
    if (!staged && s->beam.K) return fail(EMMAX_ERR_STATE, "sampling is not available while beams are on");
    const int r0 = staged ? s->stg0 : row0;
    std::vector<int32_t> rows(n);
    for (int i = 0; i < n; ++i) rows[i] = r0 + i;
    if (int r = check_sampling_values(s, rows.data(), n, T, top_k, top_p)) return r;
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = upload_rows(s, r0, n, sc.stream(), {{s->samp.t, T, 4}, {s->samp.k, top_k, 4}, {s->samp.p, top_p, 4}, {s->samp.sub, subseq, 4}, {s->samp.seed, seed, 8}})) return r;
    s->samp.on = true;
    return sc.leave();
}

// ---- logits processing and scores in the decode step (ABI 8) --------------------------------------------------------------
static int set_processing_rows(emmax_session* s, int row0, int n, bool staged, const float* pen, const int32_t* ng, const int32_t* mn, emmax_stream stream) {
    if (!s || !pen || !ng || !mn) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = check_rows(s, row0, n, staged)) return r;
    if (!staged && s->beam.K) return fail(EMMAX_ERR_STATE, "logits processing is not available while beams are on");
    const int r0 = staged ? s->stg0 : row0;
    if (s->m->vocab > EMMAX_SAMPLE_MAX_V) return fail(EMMAX_ERR_INVALID, "logits processing takes vocabularies of up to %d entries (%d)", EMMAX_SAMPLE_MAX_V, s->m->vocab);
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(pen[i]) || !(pen[i] > 0.f)) return fail(EMMAX_ERR_INVALID, "row %d: repetition penalty %g (finite and > 0)", r0 + i, (double)pen[i]);
        if (ng[i] < 0 || ng[i] > EMMAX_MAX_NGRAM) return fail(EMMAX_ERR_INVALID, "row %d: no_repeat_ngram_size %d outside 0..%d", r0 + i, ng[i], EMMAX_MAX_NGRAM);
        if (mn[i] < 0) return fail(EMMAX_ERR_INVALID, "row %d: min_new_tokens %d (>= 0)", r0 + i, mn[i]);
    }
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = upload_rows(s, r0, n, sc.stream(), {{s->proc.pen, pen, 4}, {s->proc.ng, ng, 4}, {s->proc.mn, mn, 4}})) return r;
    s->proc.on = true;
    if (!staged) s->rules.implied_proc = s->aut.implied_proc = false;   // the caller's own processing now: clearing the token rules or the automaton leaves it on
    return sc.leave();
}

// ---- the further warpers and the token rules (new symbols, same ABI) -------------------------------------------------------------
int check_warper_values(int row0, int n, const float* minp, const float* typ, const float* eps, const float* eta) {
    for (int i = 0; i < n; ++i) {
        if (!(minp[i] >= 0.f && minp[i] <= 1.f)) return fail(EMMAX_ERR_INVALID, "row %d: min_p %g (0 = off, else 0 < min_p <= 1)", row0 + i, (double)minp[i]);
        if (!(typ[i] >= 0.f && typ[i] <= 1.f)) return fail(EMMAX_ERR_INVALID, "row %d: typical_p %g (0 or 1 = off, else 0 < typical_p < 1)", row0 + i, (double)typ[i]);
        if (!(eps[i] >= 0.f && eps[i] < 1.f)) return fail(EMMAX_ERR_INVALID, "row %d: epsilon_cutoff %g (0 = off, else 0 < epsilon_cutoff < 1)", row0 + i, (double)eps[i]);
        if (!(eta[i] >= 0.f && eta[i] < 1.f)) return fail(EMMAX_ERR_INVALID, "row %d: eta_cutoff %g (0 = off, else 0 < eta_cutoff < 1)", row0 + i, (double)eta[i]);
    }
    return 0;
}

static int set_warper_rows(emmax_session* s, int row0, int n, bool staged, const float* minp, const float* typ, const float* eps, const float* eta, emmax_stream stream) {
    if (!s || !minp || !typ || !eps || !eta) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = check_rows(s, row0, n, staged)) return r;
    if (!staged && s->beam.K) return fail(EMMAX_ERR_STATE, "warpers are not available while beams are on");
    if (s->m->vocab > EMMAX_SAMPLE_MAX_V) return fail(EMMAX_ERR_INVALID, "warpers take vocabularies of up to %d entries (%d)", EMMAX_SAMPLE_MAX_V, s->m->vocab);
    const int r0 = staged ? s->stg0 : row0;
    if (int r = check_warper_values(r0, n, minp, typ, eps, eta)) return r;
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = upload_rows(s, r0, n, sc.stream(), {{s->warp.minp, minp, 4}, {s->warp.typ, typ, 4}, {s->warp.eps, eps, 4}, {s->warp.eta, eta, 4}})) return r;
    s->warp.on = true;
    return sc.leave();
}

// a rule table as the host hands it over: n rules, rule r = ids[off[r] .. off[r + 1]), within the caps, flags and biases in range
int check_rule_table(int n, const int32_t* off, const int32_t* ids, const int32_t* flags, const float* bias) {
    if (n < 1 || n > EMMAX_MAX_RULES) return fail(EMMAX_ERR_INVALID, "%d token rules outside 1..%d", n, EMMAX_MAX_RULES);
    if (!off || !ids || !flags || !bias) return fail(EMMAX_ERR_INVALID, "null argument");
    if (off[0] != 0 || off[n] > EMMAX_MAX_RULE_TOTAL) return fail(EMMAX_ERR_INVALID, "token rules: offsets start at %d and end at %d (0 .. at most %d ids)", off[0], off[n], EMMAX_MAX_RULE_TOTAL);
    for (int r = 0; r < n; ++r) {
        const int len = off[r + 1] - off[r];
        if (len < 1 || len > EMMAX_MAX_RULE_IDS) return fail(EMMAX_ERR_INVALID, "token rule %d: %d ids outside 1..%d", r, len, EMMAX_MAX_RULE_IDS);
        if (flags[r] < 0 || flags[r] > 7) return fail(EMMAX_ERR_INVALID, "token rule %d: flags %d outside 0..7", r, flags[r]);
        if ((flags[r] & 3) == 0 && std::isnan(bias[r])) return fail(EMMAX_ERR_INVALID, "token rule %d: bias is NaN", r);
        for (int k = off[r]; k < off[r + 1]; ++k)
            if (ids[k] < 0) return fail(EMMAX_ERR_INVALID, "token rule %d: negative id %d", r, ids[k]);
    }
    return 0;
}

static int set_rule_enable_rows(emmax_session* s, int row0, int n, bool staged, const uint32_t* en, emmax_stream stream) {
    if (!s || !en) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = check_rows(s, row0, n, staged)) return r;
    if (!s->rules.on) return fail(EMMAX_ERR_STATE, "no token rules are set (emmax_session_set_token_rules)");
    const int r0 = staged ? s->stg0 : row0;
    for (int i = 0; i < n; ++i)
        if (en[i] > 15u) return fail(EMMAX_ERR_INVALID, "row %d: rule enable word %u outside 0..15", r0 + i, en[i]);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = upload_rows(s, r0, n, sc.stream(), {{s->rules.en, en, 4}})) return r;
    return sc.leave();
}

// The token rules and the automaton are processors that read the history: setting either turns processing on, with neutral values on every row,
// where it was off.  *implied: the setter's note that the processing is its own to turn off again
static int neutral_processing_on(emmax_session* s, bool* implied) {
    if (s->proc.on) return 0;
    std::vector<float> one((size_t)s->rows_total, 1.f);
    HIPCHK(hipMemcpy(s->proc.pen, one.data(), one.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(s->proc.ng, 0, (size_t)s->rows_total * 4));
    HIPCHK(hipMemset(s->proc.mn, 0, (size_t)s->rows_total * 4));
    s->proc.on = true;
    *implied = true;
    return 0;
}
// ... and clearing the one whose processing it is (mine) hands it to the other where that is still on -- it is the other's to turn off now --
// and turns it off otherwise
static void hand_over_processing(emmax_session* s, bool mine, bool other_on, bool* other_implied) {
    if (mine) {
        if (other_on) *other_implied = true;
        else s->proc.on = false;
    }
    if (!s->samp.on && !s->proc.on) (void)emmax_session_clear_top_logprobs(s, nullptr);
}

extern "C" {

int emmax_session_set_warpers(emmax_session* s, int row0, int n, const float* min_p_host, const float* typical_p_host, const float* epsilon_cutoff_host,
                              const float* eta_cutoff_host, emmax_stream stream) {
    return set_warper_rows(s, row0, n, false, min_p_host, typical_p_host, epsilon_cutoff_host, eta_cutoff_host, stream);
}

int emmax_slots_set_warpers_staged(emmax_session* s, int n, const float* min_p_host, const float* typical_p_host, const float* epsilon_cutoff_host,
                                   const float* eta_cutoff_host, emmax_stream stream) {
    return set_warper_rows(s, 0, n, true, min_p_host, typical_p_host, epsilon_cutoff_host, eta_cutoff_host, stream);
}

int emmax_session_clear_warpers(emmax_session* s, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->warp.on) return 0;
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    RowCols cols;
    if (int r = session_row_cols(s, &cols)) return r;
    for (int i = 0; i < cols.n; ++i)
        if (cols.col[i].owner == ROWS_WARPERS) HIPCHK(hipMemsetAsync(cols.col[i].base, 0, (size_t)s->rows_total * cols.col[i].stride_bytes, sc.stream()));
    s->warp.on = false;
    return sc.leave();
}

int emmax_session_warpers(const emmax_session* s) { return s ? (s->warp.on ? 1 : 0) : -1; }

int emmax_session_set_token_rules(emmax_session* s, int n_rules, const int32_t* offsets_host, const int32_t* ids_host, const int32_t* flags_host,
                                  const float* bias_host, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = check_rule_table(n_rules, offsets_host, ids_host, flags_host, bias_host)) return r;
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "token rules are not available while beams are on");
    if (s->m->vocab > EMMAX_SAMPLE_MAX_V) return fail(EMMAX_ERR_INVALID, "token rules take vocabularies of up to %d entries (%d)", EMMAX_SAMPLE_MAX_V, s->m->vocab);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    HIPCHK(hipStreamSynchronize(sc.stream()));   // no step reads the table while it changes
    const int32_t n = n_rules;
    HIPCHK(hipMemcpy(s->rules.off, offsets_host, (size_t)(n_rules + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->rules.ids, ids_host, (size_t)offsets_host[n_rules] * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->rules.flags, flags_host, (size_t)n_rules * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->rules.bias, bias_host, (size_t)n_rules * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->rules.n, &n, 4, hipMemcpyHostToDevice));
    if (!s->rules.on) {   // every row starts with every kind enabled; the rules read the history: processing on, neutral where it was off
        std::vector<uint32_t> all((size_t)s->rows_total, 15u);
        HIPCHK(hipMemcpy(s->rules.en, all.data(), all.size() * 4, hipMemcpyHostToDevice));
        if (int r = neutral_processing_on(s, &s->rules.implied_proc)) return r;
    }
    s->rules.on = true;
    return sc.leave();
}

int emmax_session_set_rule_enables(emmax_session* s, int row0, int n, const uint32_t* enable_host, emmax_stream stream) {
    return set_rule_enable_rows(s, row0, n, false, enable_host, stream);
}

int emmax_slots_set_rule_enables_staged(emmax_session* s, int n, const uint32_t* enable_host, emmax_stream stream) {
    return set_rule_enable_rows(s, 0, n, true, enable_host, stream);
}

int emmax_session_clear_token_rules(emmax_session* s, emmax_stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    hand_over_processing(s, s->rules.on && s->rules.implied_proc, s->aut.on, &s->aut.implied_proc);
    s->rules.on = s->rules.implied_proc = false;
    return 0;
}

int emmax_session_token_rules(const emmax_session* s) { return s ? (s->rules.on ? 1 : 0) : -1; }

// ---- the token automaton (new symbols, same ABI) --------------------------------------------------------------------------------
static int set_automaton_start_rows(emmax_session* s, int row0, int n, bool staged, const int32_t* start, emmax_stream stream) {
    if (!s || !start) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = check_rows(s, row0, n, staged)) return r;
    if (!s->aut.on) return fail(EMMAX_ERR_STATE, "no token automaton is set (emmax_session_set_automaton)");
    const int r0 = staged ? s->stg0 : row0;
    for (int i = 0; i < n; ++i)
        if (start[i] < -1 || start[i] >= s->aut.n_states) return fail(EMMAX_ERR_INVALID, "row %d: start state %d outside -1..%d", r0 + i, start[i], s->aut.n_states - 1);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = upload_rows(s, r0, n, sc.stream(), {{s->aut.start, start, 4}})) return r;
    return sc.leave();
}

int emmax_session_set_automaton(emmax_session* s, int n_states, int n_classes, const uint8_t* cls_host, const uint32_t* allow_host, const int16_t* next_host,
                                emmax_stream stream) {
    if (!s || !cls_host || !allow_host || !next_host) return fail(EMMAX_ERR_INVALID, "null argument");
    if (n_states < 1 || n_states > EMMAX_MAX_AUT_STATES) return fail(EMMAX_ERR_INVALID, "%d automaton states outside 1..%d", n_states, EMMAX_MAX_AUT_STATES);
    if (n_classes < 1 || n_classes > EMMAX_MAX_AUT_CLASSES) return fail(EMMAX_ERR_INVALID, "%d token classes outside 1..%d", n_classes, EMMAX_MAX_AUT_CLASSES);
    const int V = s->m->vocab;
    if (V > EMMAX_SAMPLE_MAX_V) return fail(EMMAX_ERR_INVALID, "a token automaton takes vocabularies of up to %d entries (%d)", EMMAX_SAMPLE_MAX_V, V);
    for (int i = 0; i < V; ++i)
        if (cls_host[i] >= n_classes) return fail(EMMAX_ERR_INVALID, "token %d: class %d outside 0..%d", i, (int)cls_host[i], n_classes - 1);
    for (int st = 0; st < n_states; ++st)
        for (int c = 0; c < n_classes; ++c) {
            const int v = next_host[(size_t)st * n_classes + c];
            if (v < -1 || v >= n_states) return fail(EMMAX_ERR_INVALID, "state %d, class %d: next state %d outside -1..%d", st, c, v, n_states - 1);
        }
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "a token automaton is not available while beams are on");
    // the device layout: full-size tables, rows of next at EMMAX_MAX_AUT_CLASSES; what the table does not have allows nothing and ends the row
    std::vector<uint8_t> cls((size_t)EMMAX_SAMPLE_MAX_V, 0);
    std::vector<uint32_t> allow((size_t)EMMAX_MAX_AUT_STATES * 8, 0u);
    std::vector<int16_t> next((size_t)EMMAX_MAX_AUT_STATES * EMMAX_MAX_AUT_CLASSES, (int16_t)-1);
    memcpy(cls.data(), cls_host, (size_t)V);
    for (int st = 0; st < n_states; ++st) {
        for (int c = 0; c < n_classes; ++c) {
            if ((allow_host[(size_t)st * 8 + (c >> 5)] >> (c & 31)) & 1u) allow[(size_t)st * 8 + (c >> 5)] |= 1u << (c & 31);
            next[(size_t)st * EMMAX_MAX_AUT_CLASSES + c] = next_host[(size_t)st * n_classes + c];
        }
    }
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    HIPCHK(hipStreamSynchronize(sc.stream()));   // no step reads the table while it changes
    HIPCHK(hipMemcpy(s->aut.cls, cls.data(), cls.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->aut.allow, allow.data(), allow.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->aut.next, next.data(), next.size() * 2, hipMemcpyHostToDevice));
    if (!s->aut.on) {   // every row starts unconstrained; the mask is a processor: processing on, neutral where it was off
        HIPCHK(hipMemset(s->aut.start, 0xff, (size_t)s->rows_total * 4));
        HIPCHK(hipMemset(s->aut.state, 0xff, (size_t)s->rows_total * 4));
        if (int r = neutral_processing_on(s, &s->aut.implied_proc)) return r;
    }
    s->aut.on = true;
    s->aut.n_states = n_states; s->aut.n_classes = n_classes;
    return sc.leave();
}

int emmax_session_set_automaton_starts(emmax_session* s, int row0, int n, const int32_t* start_host, emmax_stream stream) {
    return set_automaton_start_rows(s, row0, n, false, start_host, stream);
}

int emmax_slots_set_automaton_starts_staged(emmax_session* s, int n, const int32_t* start_host, emmax_stream stream) {
    return set_automaton_start_rows(s, 0, n, true, start_host, stream);
}

int emmax_session_clear_automaton(emmax_session* s, emmax_stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    hand_over_processing(s, s->aut.on && s->aut.implied_proc, s->rules.on, &s->rules.implied_proc);
    s->aut.on = s->aut.implied_proc = false;
    return 0;
}

int emmax_session_automaton(const emmax_session* s) { return s ? (s->aut.on ? 1 : 0) : -1; }

int emmax_session_automaton_state(emmax_session* s, int row0, int n, int32_t* state_out_dev, emmax_stream stream) {
    if (!s || !state_out_dev) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->aut.on) return fail(EMMAX_ERR_STATE, "no token automaton is set (emmax_session_set_automaton)");
    if (n < 1 || row0 < 0 || row0 + n > s->rows_total) return fail(EMMAX_ERR_INVALID, "rows %d..%d outside 0..%d", row0, row0 + n - 1, s->rows_total - 1);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    HIPCHK(hipMemcpyAsync(state_out_dev, s->aut.state + row0, (size_t)n * 4, hipMemcpyDeviceToDevice, sc.stream()));
    return sc.leave();
}

int emmax_session_set_stop(emmax_session* s, const int32_t* trigger_ids, int n_trigger, int n_after, emmax_stream stream) {
    if (!s || (n_trigger > 0 && !trigger_ids)) return fail(EMMAX_ERR_INVALID, "null argument");
    if (n_trigger < 0 || n_trigger > EMMAX_MAX_STOP_IDS || n_after < 0)
        return fail(EMMAX_ERR_INVALID, "stop rule: %d trigger ids (max %d), %d tokens after", n_trigger, EMMAX_MAX_STOP_IDS, n_after);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    const int32_t cfg[2] = {n_trigger, n_after};
    if (int r = upload_rows(s, 0, 1, sc.stream(), {{s->stop_ids, trigger_ids, n_trigger * 4}, {s->stop_cfg, cfg, 8}})) return r;
    return sc.leave();
}

int emmax_session_set_sampling(emmax_session* s, int row0, int n, const float* temperature_host, const int32_t* top_k_host, const float* top_p_host,
                               const uint64_t* seed_host, const uint32_t* subseq_host, emmax_stream stream) {
    return set_sampling_rows(s, row0, n, false, temperature_host, top_k_host, top_p_host, seed_host, subseq_host, stream);
}

int emmax_slots_set_sampling_staged(emmax_session* s, int n, const float* temperature_host, const int32_t* top_k_host, const float* top_p_host,
                                    const uint64_t* seed_host, const uint32_t* subseq_host, emmax_stream stream) {
    return set_sampling_rows(s, 0, n, true, temperature_host, top_k_host, top_p_host, seed_host, subseq_host, stream);
}

int emmax_session_clear_sampling(emmax_session* s, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    s->samp.on = false;
    if (!s->proc.on) (void)emmax_session_clear_top_logprobs(s, stream);   // no logit rows are written any more
    return emmax_session_clear_warpers(s, stream);   // the warpers belong to the draw
}

int emmax_session_sampling(const emmax_session* s) { return s ? (s->samp.on ? 1 : 0) : -1; }

int emmax_session_logprobs(emmax_session* s, int max_new, float* out_dev, emmax_stream stream) {
    if (!s || !out_dev) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->samp.on) return fail(EMMAX_ERR_STATE, "log-probabilities exist in a sampling session only (emmax_session_set_sampling)");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "no generation has run");
    if (max_new < 1 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "max_new_tokens %d outside 1..%d", max_new, s->max_out);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    HIPCHK(hipMemcpy2DAsync(out_dev, (size_t)max_new * 4, s->samp.logprob, (size_t)s->max_out * 4, (size_t)max_new * 4, s->cur_B,
                            hipMemcpyDeviceToDevice, sc.stream()));
    return sc.leave();
}

int emmax_slot_logprobs(emmax_session* s, int slot, float* out_dev, int n, emmax_stream stream) {
    if (!s || !out_dev) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->samp.on) return fail(EMMAX_ERR_STATE, "log-probabilities exist in a sampling session only (emmax_session_set_sampling)");
    if (!s->slots_open) return fail(EMMAX_ERR_STATE, "emmax_slot_logprobs before emmax_slots_open");
    if (slot < 0 || slot >= s->cur_B || n < 0 || n > s->max_out) return fail(EMMAX_ERR_INVALID, "slot %d / %d values out of range", slot, n);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (n > 0) HIPCHK(hipMemcpyAsync(out_dev, s->samp.logprob + (size_t)slot * s->max_out, (size_t)n * 4, hipMemcpyDeviceToDevice, sc.stream()));
    return sc.leave();
}

int emmax_session_set_processing(emmax_session* s, int row0, int n, const float* penalty_host, const int32_t* ngram_host, const int32_t* min_new_host,
                                 emmax_stream stream) {
    return set_processing_rows(s, row0, n, false, penalty_host, ngram_host, min_new_host, stream);
}

int emmax_slots_set_processing_staged(emmax_session* s, int n, const float* penalty_host, const int32_t* ngram_host, const int32_t* min_new_host,
                                      emmax_stream stream) {
    return set_processing_rows(s, 0, n, true, penalty_host, ngram_host, min_new_host, stream);
}

int emmax_session_clear_processing(emmax_session* s, emmax_stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    s->proc.on = false;
    s->rules.on = s->rules.implied_proc = false;   // the token rules are processors (the table stays on the device; set it again to use it)
    s->aut.on = s->aut.implied_proc = false;       // ... and so is the automaton's mask
    if (!s->samp.on) (void)emmax_session_clear_top_logprobs(s, nullptr);   // no logit rows are written any more
    return 0;
}

int emmax_session_processing(const emmax_session* s) { return s ? (s->proc.on ? 1 : 0) : -1; }

int emmax_session_set_scores(emmax_session* s, float* scores_dev, float* logits_dev, int max_new, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (s->slots_open) return fail(EMMAX_ERR_STATE, "scores are not kept in slot serving (emmax_slots_open)");
    if (!scores_dev && !logits_dev) {
        s->scores.on = s->scores.has_scores = false;
        return 0;
    }
    if (s->beam.K && scores_dev) return fail(EMMAX_ERR_STATE, "processed scores are not kept while beams are on (bind the raw logits buffer only)");
    if (s->m->vocab > EMMAX_SAMPLE_MAX_V) return fail(EMMAX_ERR_INVALID, "scores take vocabularies of up to %d entries (%d)", EMMAX_SAMPLE_MAX_V, s->m->vocab);
    if (max_new < 1 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "max_new_tokens %d outside 1..%d", max_new, s->max_out);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    const uint64_t words[4] = {(uint64_t)(uintptr_t)scores_dev, (uint64_t)(uintptr_t)logits_dev, (uint64_t)max_new, 0};   // rows: set by the next prefill
    if (int r = upload_rows(s, 0, 1, sc.stream(), {{s->scores.words, words, 4 * 8}})) return r;
    s->scores.on = true;
    s->scores.has_scores = scores_dev != nullptr;
    s->scores.rows = 0;
    return sc.leave();
}

// ---- top-N and watched-token log-probabilities in the decode step (new symbols, same ABI) -------------------------------------
int emmax_session_set_top_logprobs(emmax_session* s, int n_top, int32_t* top_ids_dev, float* top_lp_dev, int n_watch, const int32_t* watch_ids_host,
                                   float* watch_lp_dev, int max_new, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    const int V = s->m->vocab;
    if (n_top < 0 || n_top > EMMAX_MAX_TOP_LOGPROBS || n_top > V)
        return fail(EMMAX_ERR_INVALID, "n_top %d outside 0..min(%d, the vocabulary's %d)", n_top, EMMAX_MAX_TOP_LOGPROBS, V);
    if (n_watch < 0 || n_watch > EMMAX_MAX_WATCH_IDS) return fail(EMMAX_ERR_INVALID, "n_watch %d outside 0..%d", n_watch, EMMAX_MAX_WATCH_IDS);
    if (n_top == 0 && n_watch == 0) return fail(EMMAX_ERR_INVALID, "neither top log-probabilities nor watched ids asked for (emmax_session_clear_top_logprobs unbinds)");
    if ((n_top > 0 && (!top_ids_dev || !top_lp_dev)) || (n_watch > 0 && (!watch_ids_host || !watch_lp_dev))) return fail(EMMAX_ERR_INVALID, "null argument");
    for (int w = 0; w < n_watch; ++w)
        if (watch_ids_host[w] < 0 || watch_ids_host[w] >= V) return fail(EMMAX_ERR_INVALID, "watch id %d (entry %d) outside 0..%d", watch_ids_host[w], w, V - 1);
    if (max_new < 1 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "max_new_tokens %d outside 1..%d", max_new, s->max_out);
    if (V > EMMAX_SAMPLE_MAX_V) return fail(EMMAX_ERR_INVALID, "top log-probabilities take vocabularies of up to %d entries (%d)", EMMAX_SAMPLE_MAX_V, V);
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "top log-probabilities are not available while beams are on");
    if (!s->samp.on && !s->proc.on)
        return fail(EMMAX_ERR_STATE, "top log-probabilities read the session's logit rows: turn sampling (temperature 0 for greedy rows) or logits processing on first");
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    uint64_t words[TOPLP_WORDS] = {};
    words[TOPLP_W_IDS] = (uint64_t)(uintptr_t)top_ids_dev; words[TOPLP_W_LP] = (uint64_t)(uintptr_t)top_lp_dev; words[TOPLP_W_WATCH] = (uint64_t)(uintptr_t)watch_lp_dev;
    words[TOPLP_W_NTOP] = (uint64_t)n_top; words[TOPLP_W_NWATCH] = (uint64_t)n_watch; words[TOPLP_W_MAXNEW] = (uint64_t)max_new;
    if (int r = upload_rows(s, 0, 1, sc.stream(), {{s->toplp.words, words, (int)sizeof(words)}, {s->toplp.watch_ids, watch_ids_host, n_watch * 4}})) return r;
    s->toplp.on = true;
    s->toplp.n_top = n_top; s->toplp.n_watch = n_watch; s->toplp.max_new = max_new;
    s->toplp.ids_out = top_ids_dev; s->toplp.lp_out = top_lp_dev; s->toplp.watch_out = watch_lp_dev;
    return sc.leave();
}

int emmax_session_clear_top_logprobs(emmax_session* s, emmax_stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    s->toplp = TopLogprobs{false, 0, 0, 0, nullptr, nullptr, nullptr, s->toplp.words, s->toplp.watch_ids};
    return 0;
}

int emmax_session_top_logprobs(const emmax_session* s) { return s ? (s->toplp.on ? 1 : 0) : -1; }

// ---- taps: hidden states and attention maps out of the passes the session runs anyway (new symbols, same ABI; taps.hip) -----------------
static int tap_sel(uint64_t mask, int bit) { return __builtin_popcountll(mask & ((1ull << bit) - 1)); }   // the entry's place among the selected, lowest first

static int taps_args(const emmax_session* s, const char* who, const float* hidden, uint64_t hl, const float* attn, uint64_t al, int ld_keys) {
    const auto& c = s->m->cfg;
    const int nl = c.n_layers;
    if (nl > 62) return fail(EMMAX_ERR_INVALID, "%s: the layer masks hold up to 62 layers (%d)", who, nl);
    if ((hidden != nullptr) != (hl != 0) || (attn != nullptr) != (al != 0))
        return fail(EMMAX_ERR_INVALID, "%s: a buffer and its layer mask go together (hidden %s, mask %llx; attentions %s, mask %llx)", who, hidden ? "set" : "null",
                    (unsigned long long)hl, attn ? "set" : "null", (unsigned long long)al);
    if (hl >> (nl + 1)) return fail(EMMAX_ERR_INVALID, "%s: hidden_layers %llx names an entry above %d (bit i = hidden_states[i], bit %d the normed last)", who, (unsigned long long)hl, nl, nl);
    if (al >> nl) return fail(EMMAX_ERR_INVALID, "%s: attn_layers %llx names a layer above %d", who, (unsigned long long)al, nl - 1);
    if ((((uintptr_t)hidden | (uintptr_t)attn) & 15)) return fail(EMMAX_ERR_INVALID, "%s: the buffers are 16-byte aligned", who);
    if (attn) {
        if (ld_keys < 4 || ld_keys % 4) return fail(EMMAX_ERR_INVALID, "%s: ld_keys %d is not a positive multiple of 4 (16-byte stores)", who, ld_keys);
        const int G = c.n_kv_heads > 0 ? c.n_heads / c.n_kv_heads : 0;
        if (c.head_dim != 128 || c.n_heads % c.n_kv_heads || (G != 1 && G != 2 && G != 4 && G != 8))
            return fail(EMMAX_ERR_INVALID, "%s: the probability kernel takes head_dim 128 and GQA groups of 1 / 2 / 4 / 8 (heads %d / %d, head_dim %d)", who, c.n_heads,
                        c.n_kv_heads, c.head_dim);
    }
    if (s->exact) return fail(EMMAX_ERR_STATE, "%s: exact-numerics sessions serve no taps (their fp32 / 24-bit cache has no probability kernel)", who);
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "%s: not served while beams are on (emmax_session_clear_beams)", who);
    if (s->grp_N) return fail(EMMAX_ERR_STATE, "%s: not served while sample groups are on (emmax_session_clear_sample_groups)", who);
    if (s->slots_open) return fail(EMMAX_ERR_STATE, "%s: not served while request slots are open", who);
    return 0;
}

int emmax_session_set_pass_taps(emmax_session* s, float* hidden_dev, uint64_t hidden_layers, float* attn_dev, uint64_t attn_layers, int ld_keys, emmax_stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!hidden_dev && !attn_dev && !hidden_layers && !attn_layers) {
        taps_unbind(s, true, false);
        return 0;
    }
    if (int r = taps_args(s, "emmax_session_set_pass_taps", hidden_dev, hidden_layers, attn_dev, attn_layers, ld_keys)) return r;
    s->taps.pass.on = true;
    s->taps.pass.hidden = hidden_dev; s->taps.pass.hl = hidden_layers; s->taps.pass.attn = attn_dev; s->taps.pass.al = attn_layers;
    s->taps.pass.ld = attn_dev ? ld_keys : 0;
    return 0;
}

int emmax_session_set_step_taps(emmax_session* s, float* hidden_dev, uint64_t hidden_layers, float* attn_dev, uint64_t attn_layers, int ld_keys, int max_new,
                                emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!hidden_dev && !attn_dev && !hidden_layers && !attn_layers) {
        taps_unbind(s, false, true);
        return 0;
    }
    const char* who = "emmax_session_set_step_taps";
    if (int r = taps_args(s, who, hidden_dev, hidden_layers, attn_dev, attn_layers, ld_keys)) return r;
    if (max_new < 1 || max_new > s->max_ctx) return fail(EMMAX_ERR_INVALID, "%s: max_new %d outside 1..max_ctx = %d", who, max_new, s->max_ctx);
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "%s: no prefill yet: the buffers' batch is that of the live rows", who);
    if (attn_dev) {   // the lengths are known here (read back once: a binding is not part of a captured step): a row sees one key more per step,
                      // max(1, max_new - 1) steps to come
        int32_t ctx[EMMAX_MAX_DECODE_BATCH];
        const int B = std::min(s->cur_B, (int)EMMAX_MAX_DECODE_BATCH);
        StreamScope sc(s, stream);
        if (sc.error()) return sc.error();
        HIPCHK(hipMemcpyAsync(ctx, s->rows.ctx_len, (size_t)B * 4, hipMemcpyDeviceToHost, sc.stream()));
        HIPCHK(hipStreamSynchronize(sc.stream()));
        if (int r = sc.leave()) return r;
        int longest = 0;
        for (int b = 0; b < B; ++b) longest = std::max(longest, ctx[b]);
        const int need = longest + std::max(1, max_new - 1);
        if (ld_keys < need) return fail(EMMAX_ERR_INVALID, "%s: ld_keys %d is smaller than the %d keys a row can see (context %d + the steps to come)", who, ld_keys, need, longest);
    }
    s->taps.step.on = true;
    s->taps.step.hidden = hidden_dev; s->taps.step.hl = hidden_layers; s->taps.step.attn = attn_dev; s->taps.step.al = attn_layers;
    s->taps.step.ld = attn_dev ? ld_keys : 0;
    s->taps.step_max_new = max_new; s->taps.step_B = s->cur_B;
    s->taps.serial += 1;
    return 0;
}

int emmax_session_clear_taps(emmax_session* s, emmax_stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    taps_unbind(s, true, true);
    return 0;
}

int emmax_session_taps(const emmax_session* s) { return s ? ((s->taps.pass.on ? 1 : 0) | (s->taps.step.on ? 2 : 0)) : -1; }

}  // extern "C"

int tap_pass_check(emmax_session* s, int max_keys, const char* who) {
    if (s->taps.pass.on && s->taps.pass.attn && s->taps.pass.ld < max_keys)
        return fail(EMMAX_ERR_INVALID, "%s: the bound attention tap's ld_keys %d is smaller than the %d keys a row of this pass sees (emmax_session_set_pass_taps)", who,
                    s->taps.pass.ld, max_keys);
    return 0;
}

// the stream's rows as the pass / the step holds them now: fp32 where the stream is fp32, else the bf16 rows
static void tap_stream_src(TapRowsParams& p, const float* h32, const bf16* h16, int H) {
    p.src = h32 ? (const void*)h32 : (const void*)h16;
    p.src_f32 = h32 ? 1 : 0;
    p.ld_src = H;
}

int tap_pass_hidden(emmax_session* s, int idx, int total, hipStream_t st) {
    const TapSet& t = s->taps.pass;
    if (!t.on || !t.hidden || !((t.hl >> idx) & 1)) return 0;
    emmax_model* m = s->m;
    TapRowsParams p;
    memset(&p, 0, sizeof(p));
    tap_stream_src(p, s->p32 ? s->ph32 : nullptr, s->ph, m->H);
    p.dst = t.hidden + (size_t)tap_sel(t.hl, idx) * total * m->H;
    p.rows = total; p.H = m->H; p.eps = m->cfg.rms_eps;
    if (idx == m->cfg.n_layers) p.norm_w = m->final_norm;
    KCHK(launch_tap_rows(p, st));
    return 0;
}

int tap_pass_attn(emmax_session* s, int li, int B, int total, int max_n, int r0, bool ext, hipStream_t st) {
    const TapSet& t = s->taps.pass;
    if (!t.on || !t.attn || !((t.al >> li) & 1)) return 0;
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    AttnProbsParams a;
    memset(&a, 0, sizeof(a));
    a.q = s->pqkv; a.ldq = m->qkv_dim; a.q_off = 0; a.kcache = kcache_of(s, li);
    if (s->kv8) a.kscale = kscale_of(s, li);
    a.page_table = s->page_table + (size_t)r0 * s->max_pages; a.cu = s->cu; a.base = ext ? s->ext_base : nullptr;
    a.probs = t.attn + (size_t)tap_sel(t.al, li) * total * c.n_heads * t.ld;
    a.ld_keys = t.ld; a.B = B; a.Hq = c.n_heads; a.Hkv = c.n_kv_heads; a.max_pages = s->max_pages; a.scale = 1.0f / sqrtf((float)c.head_dim);
    KCHK(launch_attn_probs(a, max_n, s->kv8 ? 1 : 0, st));
    return 0;
}

// A decode step's taps.  At every launch of the step before its finish, ctx_len[b] is the row's cached length BEFORE the step = the position of the
// step's token: the qkv epilogue rotates at it and writes K / V there (fp8 cache: into kv_stage, appended by the attention launch), the attention
// covers ctx_len + 1 keys, and only the finish advances it.  So the step's map is the probability kernel at base = ctx_len, one new row
// per sequence, behind the attention launch.  n_out[b] is the index of the token the step is about to emit: the row's slot
int tap_step_hidden(emmax_session* s, int idx, int B, hipStream_t st) {
    const TapSet& t = s->taps.step;
    if (!t.on || !t.hidden || !((t.hl >> idx) & 1) || B != s->taps.step_B) return 0;
    emmax_model* m = s->m;
    const int n_sel = __builtin_popcountll(t.hl);
    TapRowsParams p;
    memset(&p, 0, sizeof(p));
    if (idx == 0) {   // behind the embed: the token's row of the table itself (a step of 1-2 rows folds the gather into layer 0's qkv launch)
        p.src = m->embed; p.src_f32 = 0; p.ld_src = m->H; p.gather = s->rows.cur_tok; p.gather_rows = m->vocab;
    } else {
        tap_stream_src(p, h32_of(s), s->dh, m->H);
    }
    p.dst = t.hidden + (size_t)tap_sel(t.hl, idx) * B * m->H;
    p.rows = B; p.H = m->H; p.eps = m->cfg.rms_eps;
    p.gen_idx = s->rows.n_out; p.done = s->rows.done; p.gen_stride = (long long)n_sel * B * m->H; p.max_new = s->taps.step_max_new;
    if (idx == m->cfg.n_layers) p.norm_w = m->final_norm;
    KCHK(launch_tap_rows(p, st));
    return 0;
}

int tap_step_attn(emmax_session* s, int li, int B, hipStream_t st) {
    const TapSet& t = s->taps.step;
    if (!t.on || !t.attn || !((t.al >> li) & 1) || B != s->taps.step_B) return 0;
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    const int n_sel = __builtin_popcountll(t.al);
    AttnProbsParams a;
    memset(&a, 0, sizeof(a));
    a.q = s->dq; a.ldq = m->q_dim; a.q_off = 0; a.kcache = kcache_of(s, li);
    if (s->kv8) a.kscale = kscale_of(s, li);
    a.page_table = s->page_table; a.cu = nullptr; a.base = s->rows.ctx_len;
    a.probs = t.attn + (size_t)tap_sel(t.al, li) * B * c.n_heads * t.ld;
    a.gen_idx = s->rows.n_out; a.done = s->rows.done; a.gen_stride = (long long)n_sel * B * c.n_heads * t.ld; a.max_new = s->taps.step_max_new;
    a.ld_keys = t.ld; a.B = B; a.Hq = c.n_heads; a.Hkv = c.n_kv_heads; a.max_pages = s->max_pages; a.scale = 1.0f / sqrtf((float)c.head_dim);
    KCHK(launch_attn_probs(a, 1, s->kv8 ? 1 : 0, st));
    return 0;
}

extern "C" {

// ---- beam search in the decode step (ABI 9) ---------------------------------------------------------------------------
int emmax_session_set_beams(emmax_session* s, int num_beams, double length_penalty, int early_stopping, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    const int max_rows = session_max_rows(s);
    if (num_beams < 2 || num_beams > EMMAX_MAX_BEAMS || num_beams > s->max_batch || num_beams > max_rows)
        return fail(EMMAX_ERR_INVALID, "num_beams %d outside 2..min(%d, max_batch=%d, %d)", num_beams, EMMAX_MAX_BEAMS, s->max_batch, max_rows);
    if (!std::isfinite(length_penalty)) return fail(EMMAX_ERR_INVALID, "length_penalty must be finite");
    if (early_stopping < 0 || early_stopping > 2) return fail(EMMAX_ERR_INVALID, "early_stopping %d: 0 False, 1 True, 2 never", early_stopping);
    if (s->m->vocab > EMMAX_SAMPLE_MAX_V || s->m->vocab < 2 * num_beams)
        return fail(EMMAX_ERR_INVALID, "beams take vocabularies of %d..%d entries (%d)", 2 * num_beams, EMMAX_SAMPLE_MAX_V, s->m->vocab);
    if (s->slots_open) return fail(EMMAX_ERR_STATE, "beams cannot be turned on while request slots are open");
    if (s->grp_N) return fail(EMMAX_ERR_STATE, "beams cannot be turned on while sample groups are on (emmax_session_clear_sample_groups)");
    if (s->aut.on) return fail(EMMAX_ERR_STATE, "beams cannot be turned on while a token automaton is set (emmax_session_clear_automaton)");
    if (s->samp.on || s->proc.on || s->warp.on || s->rules.on) return fail(EMMAX_ERR_STATE, "beams cannot be turned on while sampling or logits processing is on");
    if (s->scores.on && s->scores.has_scores) return fail(EMMAX_ERR_STATE, "beams cannot be turned on while a scores buffer is bound");
    if (s->toplp.on) return fail(EMMAX_ERR_STATE, "beams cannot be turned on while top log-probabilities are bound (emmax_session_clear_top_logprobs)");
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = slots_restore_pages(s, sc.stream())) return r;
    std::vector<float> pw((size_t)s->max_out + 1);
    for (size_t n = 0; n < pw.size(); ++n) pw[n] = (float)pow((double)n, length_penalty);
    HIPCHK(hipStreamSynchronize(sc.stream()));
    HIPCHK(hipMemcpy(s->beam.pw, pw.data(), pw.size() * 4, hipMemcpyHostToDevice));
    taps_unbind(s, true, true);   // no taps with beams
    s->beam.K = num_beams; s->beam.es = early_stopping; s->beam.lp_pos = length_penalty > 0.0 ? 1 : 0;
    s->beam.G = 0; s->beam.forked = false; s->beam.ready = false;
    s->prefilled = false;   // rows of an earlier batch do not continue as beams
    return sc.leave();
}

int emmax_session_clear_beams(emmax_session* s, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->beam.K) return 0;
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    KCHK(launch_beam_pages(s->page_table, s->rows_total, s->max_pages, 1, sc.stream()));   // static assignment again: row b owns its own pages
    s->beam.K = 0; s->beam.G = 0; s->beam.forked = false; s->beam.ready = false;
    s->prefilled = false;
    return sc.leave();
}

int emmax_session_beams(const emmax_session* s) { return s ? s->beam.K : -1; }

int emmax_session_beam_result(emmax_session* s, int max_new, int32_t* seq_dev, int32_t* len_dev, float* score_dev, int32_t* bidx_dev, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->beam.K || !s->beam.forked) return fail(EMMAX_ERR_STATE, "no beam generation to report");
    if (max_new < 1 || max_new > s->beam.max_new) return fail(EMMAX_ERR_INVALID, "max_new %d outside 1..%d (the generation's)", max_new, s->beam.max_new);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    const hipStream_t st = sc.stream();
    const int rows = s->beam.G * s->beam.K;
    if (seq_dev) HIPCHK(hipMemcpy2DAsync(seq_dev, (size_t)max_new * 4, s->rows.out_ids, (size_t)s->max_out * 4, (size_t)max_new * 4, rows, hipMemcpyDeviceToDevice, st));
    if (bidx_dev) HIPCHK(hipMemcpy2DAsync(bidx_dev, (size_t)max_new * 4, s->beam.res_bidx, (size_t)s->max_out * 4, (size_t)max_new * 4, rows, hipMemcpyDeviceToDevice, st));
    if (len_dev) HIPCHK(hipMemcpyAsync(len_dev, s->beam.res_len, rows * 4, hipMemcpyDeviceToDevice, st));
    if (score_dev) HIPCHK(hipMemcpyAsync(score_dev, s->beam.res_score, rows * 4, hipMemcpyDeviceToDevice, st));
    return sc.leave();
}

// ---- sample groups: N sampled rows per prefilled prompt (additions to ABI 11) ----------------------------------------------
int emmax_session_set_sample_groups(emmax_session* s, int n, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    const int max_rows = std::min(s->max_batch, session_max_rows(s));
    if (n < 2 || n > max_rows) return fail(EMMAX_ERR_INVALID, "%d samples per group outside 2..min(max_batch=%d, the model's decode batch)=%d", n, s->max_batch, max_rows);
    if (s->beam.K) return fail(EMMAX_ERR_STATE, "sample groups cannot be turned on while beams are on (emmax_session_clear_beams)");
    if (s->slots_open) return fail(EMMAX_ERR_STATE, "sample groups cannot be turned on while request slots are open");
    if (s->sg_followers) {
        StreamScope sc(s, stream);
        if (sc.error()) return sc.error();
        if (int r = slots_restore_pages(s, sc.stream())) return r;
        if (int r = sc.leave()) return r;
    }
    taps_unbind(s, true, true);   // no taps with sample groups
    s->grp_N = n;
    s->prefilled = false;   // rows of an earlier batch do not continue as groups
    return 0;
}

int emmax_session_clear_sample_groups(emmax_session* s, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->grp_N) return 0;
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    KCHK(launch_beam_pages(s->page_table, s->rows_total, s->max_pages, 1, sc.stream()));   // static assignment again: row b owns its own pages
    s->grp_N = 0;
    s->prefilled = false;
    return sc.leave();
}

int emmax_session_sample_groups(const emmax_session* s) { return s ? s->grp_N : -1; }

int emmax_session_attn_grouped(const emmax_session* s, int B) { return !s ? -1 : (B >= 1 && attn_group_rows(s, B)) ? 1 : 0; }

int emmax_session_beam_trace(emmax_session* s, int max_new, int32_t* tok_dev, int32_t* parent_dev, float* score_dev, float* lse_dev, int32_t* cand_idx_dev,
                             float* cand_acc_dev, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->beam.K || !s->beam.forked) return fail(EMMAX_ERR_STATE, "no beam generation to report");
    if (max_new < 1 || max_new > s->beam.max_new) return fail(EMMAX_ERR_INVALID, "max_new %d outside 1..%d (the generation's)", max_new, s->beam.max_new);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    const size_t rows = (size_t)s->beam.G * s->beam.K, ld = (size_t)std::min(s->max_batch, EMMAX_MAX_DECODE_BATCH);
    auto out = [&](void* dst, const void* src, size_t mul) -> hipError_t {
        return dst ? hipMemcpy2DAsync(dst, rows * mul * 4, src, ld * mul * 4, rows * mul * 4, (size_t)max_new, hipMemcpyDeviceToDevice, sc.stream()) : hipSuccess;
    };
    HIPCHK(out(tok_dev, s->beam.tr_tok, 1));
    HIPCHK(out(parent_dev, s->beam.tr_par, 1));
    HIPCHK(out(score_dev, s->beam.tr_score, 1));
    HIPCHK(out(lse_dev, s->beam.tr_lse, 1));
    HIPCHK(out(cand_idx_dev, s->beam.tc_idx, 2));
    HIPCHK(out(cand_acc_dev, s->beam.tc_acc, 2));
    return sc.leave();
}

}  // extern "C"
