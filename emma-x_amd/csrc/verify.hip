// verify.hip -- draft-verified greedy decoding: emmax_verify, emmax_session_set_budget, emmax_session_output, emmax_op_verify_accept.
// A generation in flight takes a WINDOW per row -- its pending token and a guessed continuation -- through the extension pass (extend.hip: the
// prefill's pipeline over the packed new rows, attention over the paged cache), scores every row's argmax (score.hip) and keeps the longest prefix
// of the guess that the model's own argmax agrees with.  Two small kernels around that pass: the pass's state (cu / base / token budget; the rows'
// generation state stays as it is) and the accept walk, which does per emitted token exactly what a decode step's finish does (kernels.h:
// emmax_finish_row).  K / V rows the pass wrote beyond the accepted run are dead: nothing reads past ctx_len and later appends overwrite them.
#include "session.h"

// ---- device ----------------------------------------------------------------------------------------------------------------
// the counterpart of emmax_extend_state_kernel for rows in mid-generation: cu = the packed offsets of the window rows, base = the cached
// lengths, the token budget; ctx_len / done / n_out / stop match / output row untouched.  Pointers already offset to the first row
__global__ void emmax_verify_state_kernel(PrefillState st, int32_t* cu, int32_t* base, const int32_t* ctx_len, int32_t* max_new, int budget) {
    if (threadIdx.x == 0) {
        int acc = 0;
        cu[0] = 0;
        for (int b = 0; b < st.B; ++b) {
            acc += st.S[b];
            cu[b + 1] = acc;
            base[b] = ctx_len[b];
            max_new[b] = budget;
        }
    }
}

// One block per sequence.  Window row i of sequence b is id w[i] = ids[b][i], cached at base + i; p[i] = argmax[cu[b] + i] is the model's token
// behind it.  Row i is reached while the row is not done and p[i - 1] == w[i]: the lanes find the first i with p[i] != w[i + 1], one thread walks
// the run before it (the stop rule's matcher is a state machine) through emmax_finish_row -- a plain decode step's bookkeeping per token.
// A row that is done when the pass starts is left exactly as it is.  emitted[b] = tokens the row emitted (0 .. n), new_ids[cu[b] ..] = those tokens
__global__ __launch_bounds__(64) void emmax_verify_accept_kernel(VerifyAcceptParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    __shared__ int s_first[64];
    const int start = p.cu[b];
    const int n = min(max(p.cu[b + 1] - start, 0), p.P_max);
    const int32_t* w = p.ids + (size_t)b * p.P_max;
    const int32_t* am = p.argmax + start;
    int first = n - 1;   // the last window row reached if every guess matches
    for (int i = lane; i + 1 < n; i += 64)
        if (am[i] != w[i + 1]) { first = i; break; }
    s_first[lane] = first;
    __syncthreads();
    if (lane != 0) return;
    for (int l = 1; l < 64; ++l) first = min(first, s_first[l]);
    int e = 0;
    if (!p.f.done[b]) {
        const int n0 = p.f.n_out[b];
        for (int i = 0; i <= first; ++i) {
            const int tok = am[i];
            emmax_finish_row(p.f, b, tok, nullptr, 0.f, false);
            if (p.f.n_out[b] > n0 + e) {   // (a row whose budget was spent before the pass emits nothing and is done)
                if (p.new_ids) p.new_ids[start + e] = tok;
                e += 1;
            }
            if (p.f.done[b]) break;
        }
    }
    p.emitted[b] = e;
}

int launch_verify_state(const PrefillState& st, int32_t* cu, int32_t* base, const int32_t* ctx_len, int32_t* max_new, int budget, hipStream_t stream) {
    if (st.B < 1 || st.B > EMMAX_MAX_DECODE_BATCH) return -1;
    hipLaunchKernelGGL(emmax_verify_state_kernel, dim3(1), dim3(64), 0, stream, st, cu, base, ctx_len, max_new, budget);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_verify_accept(const VerifyAcceptParams& p, hipStream_t stream) {
    if (p.f.B < 1 || p.f.B > EMMAX_MAX_DECODE_BATCH || p.P_max < 1 || !p.argmax || !p.ids || !p.cu || !p.emitted) return -1;
    hipLaunchKernelGGL(emmax_verify_accept_kernel, dim3(p.f.B), dim3(64), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// what a verify pass is not served with beyond extend_refusals: the accepted ids are argmaxes of RAW rows, and the pass multiplies by the prefill's matrices
static int verify_refusals(const emmax_session* s, const char* who) {
    if (int r = extend_refusals(s, who)) return r;
    if (s->slots_open) return fail(EMMAX_ERR_STATE, "%s: not served while request slots are open", who);
    // (the most specific cause first: token rules and an automaton turn processing on themselves, the log-probabilities need sampling or processing)
    if (s->taps.step.on) return fail(EMMAX_ERR_STATE, "%s: step taps are bound (emmax_session_clear_taps): the pass fills none per generated token", who);
    if (s->toplp.on) return fail(EMMAX_ERR_STATE, "%s: top / watched log-probabilities are bound (emmax_session_clear_top_logprobs): the pass stores none", who);
    if (s->scores.on) return fail(EMMAX_ERR_STATE, "%s: scores are bound (emmax_session_set_scores): the pass stores no logit rows per generated token", who);
    if (s->aut.on) return fail(EMMAX_ERR_STATE, "%s: a token automaton is set (emmax_session_clear_automaton): the accepted ids are argmaxes of raw rows", who);
    if (s->rules.on) return fail(EMMAX_ERR_STATE, "%s: token rules are on (emmax_session_clear_token_rules): the accepted ids are argmaxes of raw rows", who);
    if (s->warp.on) return fail(EMMAX_ERR_STATE, "%s: warpers are on (emmax_session_clear_warpers): the accepted ids are argmaxes of raw rows", who);
    if (s->proc.on) return fail(EMMAX_ERR_STATE, "%s: logits processing is on (emmax_session_clear_processing): the accepted ids are argmaxes of raw rows", who);
    if (s->samp.on) return fail(EMMAX_ERR_STATE, "%s: sampling is on (emmax_session_clear_sampling): a guess is verified against the greedy token", who);
    if (s->m->wfmt == PW_FP8)
        return fail(EMMAX_ERR_STATE, "%s: the model decodes on fp8 weights and prefills on the unquantised matrices: the pass would verify another model", who);
    return 0;
}

static int run_verify(emmax_session* s, int r0, int B, const int32_t* ids, const int32_t* lens, int P_max, int max_new, int32_t* emitted_host,
                      int32_t* new_ids_host, int32_t* done_host, hipStream_t st) {
    const char* who = "emmax_verify";
    emmax_model* m = s->m;
    const auto& c = m->cfg;
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || r0 < 0 || r0 + B > s->cur_B) return fail(EMMAX_ERR_INVALID, "%s: rows %d..%d outside the %d live rows", who, r0, r0 + B - 1, s->cur_B);
    if (P_max < 1) return fail(EMMAX_ERR_INVALID, "%s: P_max %d", who, P_max);
    if ((int)s->S.size() < s->rows_total) s->S.resize(s->rows_total, 0);
    // the rows' cached lengths, done flags and pending tokens, and the windows' first ids, read back once: the call is not part of a captured step
    int32_t ctx[EMMAX_MAX_DECODE_BATCH], done[EMMAX_MAX_DECODE_BATCH], cur[EMMAX_MAX_DECODE_BATCH], w0[EMMAX_MAX_DECODE_BATCH];
    HIPCHK(hipMemcpyAsync(ctx, s->rows.ctx_len + r0, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(done, s->rows.done + r0, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cur, s->rows.cur_tok + r0, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpy2DAsync(w0, 4, ids, (size_t)P_max * 4, 4, B, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    PrefillState ps;
    ps.B = B;
    int total = 0, max_n = 0, max_L = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] > P_max) return fail(EMMAX_ERR_INVALID, "%s: row %d: a window of %d ids outside 1..P_max = %d", who, r0 + b, lens[b], P_max);
        if (ctx[b] < 1) return fail(EMMAX_ERR_STATE, "%s: row %d holds no context (an idle or released row)", who, r0 + b);
        // a live row may emit one token per window row, and the last of them stays pending; a done row only rides along (its rows are never kept)
        const long need = (long)ctx[b] + lens[b] + (done[b] ? 0 : 1);
        if (need > s->max_ctx || need > (long)s->max_pages * PAGE)
            return fail(EMMAX_ERR_NOMEM, "%s: row %d: context %d + a window of %d ids%s exceed max_ctx %d (the row's %d pages)", who, r0 + b, ctx[b], lens[b],
                        done[b] ? "" : " + the pending token", s->max_ctx, s->max_pages);
        if (!done[b] && w0[b] != cur[b])
            return fail(EMMAX_ERR_INVALID, "%s: row %d: the window starts with id %d, the row's pending token is %d", who, r0 + b, w0[b], cur[b]);
        ps.S[b] = lens[b];
        total += lens[b];
        max_n = std::max(max_n, lens[b]);
        max_L = std::max(max_L, ctx[b] + lens[b]);
    }
    if (total > s->max_rows) return fail(EMMAX_ERR_NOMEM, "%s: %d packed window rows exceed the prefill capacity %d", who, total, s->max_rows);
    // the pass's small outputs live in the qkv scratch, idle behind the last layer: targets | lse | target logit | argmax | emitted ids (total each), emitted [B]
    if (((int64_t)5 * total + B) * 4 > (int64_t)s->max_rows * m->qkv_dim * 2)
        return fail(EMMAX_ERR_NOMEM, "%s: the pass's outputs of %d rows do not fit the prefill scratch", who, total);
    ScoreForm sf;
    if (!score_form(total, m->vocab, m->H, s->splitk_bytes, 0, &sf))
        return fail(EMMAX_ERR_INVALID, "%s: no scoring plan for %d rows x vocab %d x hidden %d (hidden a multiple of 64)", who, total, m->vocab, m->H);
    if (int r = tap_pass_check(s, max_L, who)) return r;
    ExtendAttnPlan plan;
    if (!extend_attn_plan(B, max_n, max_L, c.n_heads, c.n_kv_heads, 0, s->kv8 ? 1 : 0, &plan) || c.head_dim != 128)
        return fail(EMMAX_ERR_INVALID, "%s: the extension attention takes head_dim 128 and GQA groups of 1 / 2 / 4 / 8 (heads %d / %d, head_dim %d)", who, c.n_heads, c.n_kv_heads, c.head_dim);
    while (plan.nsplit > 1 && (int64_t)total * c.n_heads * plan.nsplit * EMMAX_PSTRIDE * 4 > s->splitk_bytes) plan.nsplit -= 1;
    plan.split = plan.nsplit > 1 ? 1 : 0;

    const RowState rows = s->rows.from(r0, s->max_out);
    KCHK(launch_verify_state(ps, s->cu, s->ext_base, rows.ctx_len, rows.max_new, max_new, st));
    for (int b = 0; b < B; ++b) s->S[r0 + b] = ctx[b] + lens[b];   // (with dec_steps: an upper bound of the row's context whatever is accepted)
    if (r0 == 0 && B == s->cur_B) s->dec_steps = 0;
    s->total_rows = total; s->max_seqlen = max_n;

    const bool p32 = emmax_tune().resid32 == 1;
    s->p32 = p32;
    KCHK(launch_embed_splice(ids, P_max, s->cu, m->embed, nullptr, s->ph, B, max_n, 0, m->H, m->vocab, st, p32 ? s->ph32 : nullptr));
    if (int r = tap_pass_hidden(s, 0, total, st)) return r;
    if (int r = run_prefill_layers(s, B, total, max_n, r0, &plan, st)) return r;
    // every window row's argmax, as emmax_prefill_score takes it: the final norm into pxn, then the scoring launch through the split-K scratch
    if (p32) KCHK(launch_rmsnorm_f32(s->ph32, s->pxn, m->final_norm, total, m->H, m->H, m->H, c.rms_eps, st));
    else KCHK(launch_rmsnorm(s->ph, s->pxn, m->final_norm, total, m->H, m->H, m->H, c.rms_eps, st));
    int32_t* scr = (int32_t*)s->pqkv;
    int32_t *targets = scr, *argmax = scr + 3 * (size_t)total, *new_ids = scr + 4 * (size_t)total, *emitted = scr + 5 * (size_t)total;
    HIPCHK(hipMemsetAsync(targets, 0x9c, (size_t)total * 4, st));   // 0x9c9c9c9c < 0: no row has a target
    ScoreParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.X = s->pxn; sp.W = m->lm_head_w.rm; sp.targets = targets; sp.ws = s->splitk_ws; sp.lse = (float*)(scr + (size_t)total);
    sp.target_logit = (float*)(scr + 2 * (size_t)total); sp.argmax = argmax;
    sp.ldx = m->H; sp.ldw = m->H; sp.rows = total; sp.V = m->vocab; sp.K = m->H;
    KCHK(launch_score_rows(sp, sf, st));
    VerifyAcceptParams va;
    memset(&va, 0, sizeof(va));
    va.f.B = B;
    va.f.cur_tok = rows.cur_tok; va.f.ctx_len = rows.ctx_len; va.f.done = rows.done; va.f.n_out = rows.n_out; va.f.out_ids = rows.out_ids;
    va.f.max_new_p = rows.max_new; va.f.max_out = s->max_out; va.f.max_ctx = s->max_ctx;
    va.f.stop_ids = s->stop_ids; va.f.stop_cfg = s->stop_cfg; va.f.stop_m = rows.stop_m; va.f.stop_after = rows.stop_after;
    va.f.eos_id = c.eos_id; va.f.pad_id = c.pad_id; va.f.is_prefill = 0;
    va.argmax = argmax; va.ids = ids; va.cu = s->cu; va.P_max = P_max; va.emitted = emitted; va.new_ids = new_ids;
    KCHK(launch_verify_accept(va, st));
    std::vector<int32_t> packed((size_t)total);
    HIPCHK(hipMemcpyAsync(packed.data(), new_ids, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(emitted_host, emitted, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(done_host, rows.done, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int b = 0, off = 0; b < B; off += lens[b], ++b)
        for (int i = 0; i < P_max; ++i) new_ids_host[(size_t)b * P_max + i] = i < emitted_host[b] ? packed[off + i] : c.pad_id;
    return 0;
}

extern "C" {

int emmax_verify(emmax_session* s, int row0, int B, const int32_t* ids_dev, const int32_t* lens_host, int P_max, int max_new, int32_t* emitted_host,
                 int32_t* new_ids_host, int32_t* done_host, emmax_stream stream) {
    if (!s || !ids_dev || !lens_host || !emitted_host || !new_ids_host || !done_host) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = verify_refusals(s, "emmax_verify")) return r;
    if (max_new < 1 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "emmax_verify: max_new_tokens %d outside 1..%d", max_new, s->max_out);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    if (int r = run_verify(s, row0, B, ids_dev, lens_host, P_max, max_new, emitted_host, new_ids_host, done_host, sc.stream())) return r;
    return sc.leave();
}

int emmax_session_set_budget(emmax_session* s, int row0, int B, int max_new, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "emmax_session_set_budget: no prefill yet");
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || row0 < 0 || row0 + B > s->cur_B)
        return fail(EMMAX_ERR_INVALID, "emmax_session_set_budget: rows %d..%d outside the %d live rows", row0, row0 + B - 1, s->cur_B);
    if (max_new < 1 || max_new > s->max_out) return fail(EMMAX_ERR_INVALID, "emmax_session_set_budget: max_new_tokens %d outside 1..%d", max_new, s->max_out);
    KCHK(launch_set_ints(s->rows.max_new + row0, B, max_new, (hipStream_t)stream));
    return 0;
}

int emmax_session_output(emmax_session* s, int row0, int B, int first, int n, int32_t* ids_host, int32_t* n_out_host, int32_t* done_host, emmax_stream stream) {
    if (!s || !ids_host) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "emmax_session_output: no prefill yet");
    if (B < 1 || row0 < 0 || row0 + B > s->cur_B) return fail(EMMAX_ERR_INVALID, "emmax_session_output: rows %d..%d outside the %d live rows", row0, row0 + B - 1, s->cur_B);
    if (first < 0 || n < 1 || first + n > s->max_out)
        return fail(EMMAX_ERR_INVALID, "emmax_session_output: ids %d..%d outside the output row's 0..%d", first, first + n - 1, s->max_out - 1);
    StreamScope sc(s, stream);
    if (sc.error()) return sc.error();
    const hipStream_t st = sc.stream();
    HIPCHK(hipMemcpy2DAsync(ids_host, (size_t)n * 4, s->rows.out_ids + (size_t)row0 * s->max_out + first, (size_t)s->max_out * 4, (size_t)n * 4, B,
                            hipMemcpyDeviceToHost, st));
    if (n_out_host) HIPCHK(hipMemcpyAsync(n_out_host, s->rows.n_out + row0, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    if (done_host) HIPCHK(hipMemcpyAsync(done_host, s->rows.done + row0, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return sc.leave();
}

// the accept kernel as a pure op on caller-owned arrays.  cu and the stop rule's trigger count are read back and checked on the host BEFORE the
// launch (the call synchronises the stream and cannot be captured)
int emmax_op_verify_accept(const int32_t* argmax_dev, const int32_t* ids_dev, int P_max, const int32_t* cu_dev, int B, int32_t* cur_tok_dev, int32_t* ctx_len_dev,
                           int32_t* done_dev, int32_t* n_out_dev, const int32_t* max_new_dev, int32_t* stop_m_dev, int32_t* stop_after_dev, int32_t* out_ids_dev,
                           int max_out, const int32_t* stop_ids_dev, const int32_t* stop_cfg_dev, int eos_id, int pad_id, int max_ctx, int32_t* emitted_dev,
                           int32_t* new_ids_dev, emmax_stream stream) {
    const char* who = "emmax_op_verify_accept";
    if (!argmax_dev || !ids_dev || !cu_dev || !cur_tok_dev || !ctx_len_dev || !done_dev || !n_out_dev || !max_new_dev || !stop_m_dev || !stop_after_dev ||
        !out_ids_dev || !stop_ids_dev || !stop_cfg_dev || !emitted_dev)
        return fail(EMMAX_ERR_INVALID, "%s: null argument", who);
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || P_max < 1 || max_out < 1 || max_ctx < 1)
        return fail(EMMAX_ERR_INVALID, "%s: B %d (1..%d), P_max %d, max_out %d, max_ctx %d", who, B, EMMAX_MAX_DECODE_BATCH, P_max, max_out, max_ctx);
    const hipStream_t st = (hipStream_t)stream;
    int32_t h_cu[EMMAX_MAX_DECODE_BATCH + 1], h_cfg[2], h_m[EMMAX_MAX_DECODE_BATCH];
    HIPCHK(hipMemcpyAsync(h_cu, cu_dev, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_cfg, stop_cfg_dev, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_m, stop_m_dev, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_cu[0] != 0) return fail(EMMAX_ERR_INVALID, "%s: cu_seqlens starts at %d", who, h_cu[0]);
    for (int b = 0; b < B; ++b) {
        const int n = h_cu[b + 1] - h_cu[b];
        if (n < 1 || n > P_max) return fail(EMMAX_ERR_INVALID, "%s: sequence %d has a window of %d rows outside 1..P_max = %d", who, b, n, P_max);
        if (h_m[b] < 0 || h_m[b] >= std::max(h_cfg[0], 1)) return fail(EMMAX_ERR_INVALID, "%s: sequence %d: stop match %d outside the %d trigger ids", who, b, h_m[b], h_cfg[0]);
    }
    if (h_cfg[0] < 0 || h_cfg[0] > EMMAX_MAX_STOP_IDS || h_cfg[1] < 0)
        return fail(EMMAX_ERR_INVALID, "%s: stop rule of %d trigger ids (max %d), %d tokens after", who, h_cfg[0], EMMAX_MAX_STOP_IDS, h_cfg[1]);
    VerifyAcceptParams va;
    memset(&va, 0, sizeof(va));
    va.f.B = B;
    va.f.cur_tok = cur_tok_dev; va.f.ctx_len = ctx_len_dev; va.f.done = done_dev; va.f.n_out = n_out_dev; va.f.out_ids = out_ids_dev;
    va.f.max_new_p = max_new_dev; va.f.max_out = max_out; va.f.max_ctx = max_ctx;
    va.f.stop_ids = stop_ids_dev; va.f.stop_cfg = stop_cfg_dev; va.f.stop_m = stop_m_dev; va.f.stop_after = stop_after_dev;
    va.f.eos_id = eos_id; va.f.pad_id = pad_id; va.f.is_prefill = 0;
    va.argmax = argmax_dev; va.ids = ids_dev; va.cu = cu_dev; va.P_max = P_max; va.emitted = emitted_dev; va.new_ids = new_ids_dev;
    KCHK(launch_verify_accept(va, st));
    return 0;
}

}  // extern "C"
