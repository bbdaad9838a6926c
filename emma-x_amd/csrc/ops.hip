// ops.hip -- the entry points that run one piece on its own: the decode-stage profiler and the single-kernel emmax_op_* calls the tests
// and tools drive.
#include "session.h"

// y[B, N] = x[B, K] . W^T, nothing fused: the parameters of the single-projection entry points
static GemvParams plain_gemv(const void* x, const void* W, void* y, int N, int K, int wfmt = PW_BF16, const void* scales = nullptr) {
    GemvParams p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.ldx = K; p.ldw = K; p.K = K; p.y = y; p.ldy = N; p.n_rows = N;
    gemv_set_weights(p, wfmt, W, scales);
    return p;
}

// the three single-kernel entry points of a block-scaled format (emmax_op_*_mxfp4 / _mxfp6): `op` is the exported name, for the texts
static int op_quant_mx(int wfmt, const char* op, const void* W, int ld, void* tiles, void* scales, int N, int K, int perm, int perm_hd, emmax_stream st) {
    if (!W || !tiles || !scales) return fail(EMMAX_ERR_INVALID, "%s: null argument", op);
    int r = launch_quant_mx(wfmt, W, ld, tiles, scales, N, K, perm, perm_hd, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s: N %% 16, K %% 128, ld %% 8, ld >= K (perm 1: N %% head_dim, head_dim %% 16; perm 2: N %% 32) required", op);
    return 0;
}
static int op_dequant_mx(int wfmt, const char* op, const void* tiles, const void* scales, void* W, int ld, int N, int K, int perm, int perm_hd, emmax_stream st) {
    if (!W || !tiles || !scales) return fail(EMMAX_ERR_INVALID, "%s: null argument", op);
    int r = launch_dequant_mx(wfmt, tiles, scales, W, ld, N, K, perm, perm_hd, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s: N %% 16, K %% 128, ld %% 8, ld >= K (perm 1: N %% head_dim, head_dim %% 16; perm 2: N %% 32) required", op);
    return 0;
}
static int op_gemm_small_mx(int wfmt, const char* op, const void* x, const void* tiles, const void* scales, void* y, int B, int N, int K, emmax_stream st) {
    if (!x || !tiles || !scales || !y) return fail(EMMAX_ERR_INVALID, "%s: null argument", op);
    GemvParams p = plain_gemv(x, tiles, y, N, K, wfmt, scales);
    if (B < 1 || B > 16) return fail(EMMAX_ERR_INVALID, "%s: batch %d outside 1..16", op, B);
    // (the K-split kernel only: the phased kernel of the down projection is reached through emmax_op_decode_stage)
    const int r = launch_decode_km(GEMV_PLAIN, p, B, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s: unsupported shape (N %% 16 and N <= 32768; K %% 1024 and K <= 4096)", op);
    return 0;
}

extern "C" {

int emmax_profile_decode_stage(emmax_session* s, int stage, int reps, float* avg_us, emmax_stream stream) {
    if (!s || !avg_us || reps < 1) return fail(EMMAX_ERR_INVALID, "bad argument");
    if (!s->prefilled) return fail(EMMAX_ERR_STATE, "profile needs an active (prefilled) session");
    hipStream_t st = (hipStream_t)stream;
    emmax_model* m = s->m;
    const int B = s->cur_B, nl = m->cfg.n_layers;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    int launches = 0, r = 0;
    // one untimed sweep (instruction cache, clocks), then `reps` timed sweeps over all layers: every launch streams a
    // different layer's weights, so nothing is served from the 256 MiB Infinity Cache that a real step would not get
    for (int pass = 0; pass < 2 && r == 0; ++pass) {
        if (pass == 1) HIPCHK(hipEventRecord(e0, st));
        const int n = pass == 0 ? 1 : reps;
        for (int i = 0; i < n && r == 0; ++i) {
            if (stage == STAGE_LMHEAD) {
                r = run_lm_head_step(s, B, false, nullptr, false, st);
                launches += pass;
            } else {
                for (int li = 0; li < nl && r == 0; ++li) {
                    r = run_decode_stage(s, B, li, stage, st);
                    launches += pass;
                }
            }
        }
    }
    if (r) return r;
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_us = ms * 1000.0f / (float)launches;
    return 0;
}

// ---- single-kernel entry points --------------------------------------------------------------------------------------
int emmax_op_sample(const float* logits, int ld, int B, int V, const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seed,
                    const uint32_t* subseq, const int32_t* step, int32_t* tok_out, float* logprob_out, emmax_stream stream) {
    if (!logits || !temperature || !top_k || !top_p || !seed || !subseq || !step || !tok_out || !logprob_out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (B < 1 || V < 1 || V > EMMAX_SAMPLE_MAX_V || ld < V)
        return fail(EMMAX_ERR_INVALID, "emmax_op_sample: B %d (>= 1), V %d (1..%d), ld %d (>= V)", B, V, EMMAX_SAMPLE_MAX_V, ld);
    SampleParams p;
    memset(&p, 0, sizeof(p));
    p.logits = logits; p.ld = ld; p.V = V; p.temperature = temperature; p.top_k = top_k; p.top_p = top_p; p.seed = seed; p.subseq = subseq;
    p.step = step; p.tok_out = tok_out; p.logprob_out = logprob_out;
    KCHK(launch_sample(p, B, (hipStream_t)stream));
    return 0;
}
int emmax_op_top_logprobs(const float* logits, int ld, int B, int V, int n_top, int32_t* top_ids_out, float* top_lp_out, int n_watch,
                          const int32_t* watch_ids, float* watch_lp_out, emmax_stream stream) {
    if (!logits) return fail(EMMAX_ERR_INVALID, "null argument");
    if (B < 1 || V < 1 || V > EMMAX_SAMPLE_MAX_V || ld < V)
        return fail(EMMAX_ERR_INVALID, "emmax_op_top_logprobs: B %d (>= 1), V %d (1..%d), ld %d (>= V)", B, V, EMMAX_SAMPLE_MAX_V, ld);
    if (n_top < 0 || n_top > EMMAX_MAX_TOP_LOGPROBS || n_top > V)
        return fail(EMMAX_ERR_INVALID, "emmax_op_top_logprobs: n_top %d outside 0..min(%d, V = %d)", n_top, EMMAX_MAX_TOP_LOGPROBS, V);
    if (n_watch < 0 || n_watch > EMMAX_MAX_WATCH_IDS) return fail(EMMAX_ERR_INVALID, "emmax_op_top_logprobs: n_watch %d outside 0..%d", n_watch, EMMAX_MAX_WATCH_IDS);
    if ((n_top > 0 && (!top_ids_out || !top_lp_out)) || (n_watch > 0 && (!watch_ids || !watch_lp_out))) return fail(EMMAX_ERR_INVALID, "null argument");
    TopLogprobParams p;
    memset(&p, 0, sizeof(p));
    p.logits = logits; p.ld = ld; p.V = V; p.n_top = n_top; p.top_ids = top_ids_out; p.top_lp = top_lp_out;
    p.n_watch = n_watch; p.watch_ids = watch_ids; p.watch_lp = watch_lp_out;
    KCHK(launch_top_logprobs(p, B, (hipStream_t)stream));
    return 0;
}
int emmax_op_sample_ext(const float* logits, int ld, int B, int V, const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seed,
                        const uint32_t* subseq, const int32_t* n_out, const float* min_p, const float* typical_p, const float* epsilon_cutoff,
                        const float* eta_cutoff, const float* penalty, const int32_t* ngram, const int32_t* min_new, const int32_t* hist, const int32_t* hist_len,
                        int max_hist, int n_rules, const int32_t* rule_off, const int32_t* rule_ids, const int32_t* rule_flags, const float* rule_bias,
                        const uint32_t* rule_enable, int eos_id, int pad_id, int32_t* tok_out, float* logprob_out, float* scores_out, emmax_stream stream) {
    if (!logits || !temperature || !top_k || !top_p || !seed || !subseq || !n_out || !tok_out || !logprob_out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (B < 1 || V < 1 || V > EMMAX_SAMPLE_MAX_V || ld < V)
        return fail(EMMAX_ERR_INVALID, "emmax_op_sample_ext: B %d (>= 1), V %d (1..%d), ld %d (>= V)", B, V, EMMAX_SAMPLE_MAX_V, ld);
    const bool warp = min_p || typical_p || epsilon_cutoff || eta_cutoff, proc = penalty || ngram || min_new || hist || hist_len;
    if (warp && (!min_p || !typical_p || !epsilon_cutoff || !eta_cutoff)) return fail(EMMAX_ERR_INVALID, "emmax_op_sample_ext: the four warper arrays come together");
    if (proc && (!penalty || !ngram || !min_new || !hist || !hist_len || max_hist < 1))
        return fail(EMMAX_ERR_INVALID, "emmax_op_sample_ext: the processor arrays and the histories come together (max_hist >= 1)");
    if (n_rules < 0 || n_rules > EMMAX_MAX_RULES) return fail(EMMAX_ERR_INVALID, "%d token rules outside 0..%d", n_rules, EMMAX_MAX_RULES);
    if (n_rules > 0 && (!proc || !rule_off || !rule_ids || !rule_flags || !rule_bias || !rule_enable))
        return fail(EMMAX_ERR_INVALID, "emmax_op_sample_ext: token rules need the table's five arrays and the processor arrays (the histories)");
    ExtFinishParams p;
    memset(&p, 0, sizeof(p));
    p.f.B = B; p.f.n_out = (int32_t*)n_out; p.f.is_prefill = 1; p.f.max_out = 0; p.f.eos_id = eos_id; p.f.pad_id = pad_id;
    p.logits = logits; p.ld = ld; p.V = V; p.temperature = temperature; p.top_k = top_k; p.top_p = top_p; p.seed = seed; p.subseq = subseq;
    p.min_p = min_p; p.typical_p = typical_p; p.eps_cut = epsilon_cutoff; p.eta_cut = eta_cutoff;
    p.penalty = penalty; p.ngram = ngram; p.min_new = min_new; p.hist = hist; p.hist_len = hist_len; p.max_prompt = max_hist;
    if (n_rules > 0) { p.rt.n_host = n_rules; p.rt.off = rule_off; p.rt.ids = rule_ids; p.rt.flags = rule_flags; p.rt.bias = rule_bias; p.rule_en = rule_enable; }
    p.tok_out = tok_out; p.logprob_out = logprob_out; p.scores_out = scores_out;
    KCHK(launch_ext_finish(p, (hipStream_t)stream));
    return 0;
}
int emmax_op_sample_constrained(const float* logits, int ld, int B, int V, const float* temperature, const int32_t* top_k, const float* top_p,
                                const uint64_t* seed, const uint32_t* subseq, const int32_t* n_out, const float* min_p, const float* typical_p,
                                const float* epsilon_cutoff, const float* eta_cutoff, const float* penalty, const int32_t* ngram, const int32_t* min_new,
                                const int32_t* hist, const int32_t* hist_len, int max_hist, int n_rules, const int32_t* rule_off, const int32_t* rule_ids,
                                const int32_t* rule_flags, const float* rule_bias, const uint32_t* rule_enable, int eos_id, int pad_id, int n_states,
                                int n_classes, const uint8_t* cls, const uint32_t* allow, const int16_t* next, const int32_t* state, int32_t* tok_out,
                                float* logprob_out, int32_t* state_out, float* scores_out, emmax_stream stream) {
    if (!logits || !temperature || !top_k || !top_p || !seed || !subseq || !n_out || !tok_out || !logprob_out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!cls || !allow || !next || !state || !state_out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (B < 1 || V < 1 || V > EMMAX_SAMPLE_MAX_V || ld < V)
        return fail(EMMAX_ERR_INVALID, "emmax_op_sample_constrained: B %d (>= 1), V %d (1..%d), ld %d (>= V)", B, V, EMMAX_SAMPLE_MAX_V, ld);
    if (n_states < 1 || n_states > EMMAX_MAX_AUT_STATES || n_classes < 1 || n_classes > EMMAX_MAX_AUT_CLASSES)
        return fail(EMMAX_ERR_INVALID, "emmax_op_sample_constrained: %d states (1..%d), %d classes (1..%d)", n_states, EMMAX_MAX_AUT_STATES, n_classes, EMMAX_MAX_AUT_CLASSES);
    const bool warp = min_p || typical_p || epsilon_cutoff || eta_cutoff;
    if (warp && (!min_p || !typical_p || !epsilon_cutoff || !eta_cutoff)) return fail(EMMAX_ERR_INVALID, "emmax_op_sample_constrained: the four warper arrays come together");
    if (!penalty || !ngram || !min_new || !hist || !hist_len || max_hist < 1)
        return fail(EMMAX_ERR_INVALID, "emmax_op_sample_constrained: the mask is a processor: it needs the processor arrays and the histories (max_hist >= 1)");
    if (n_rules < 0 || n_rules > EMMAX_MAX_RULES) return fail(EMMAX_ERR_INVALID, "%d token rules outside 0..%d", n_rules, EMMAX_MAX_RULES);
    if (n_rules > 0 && (!rule_off || !rule_ids || !rule_flags || !rule_bias || !rule_enable))
        return fail(EMMAX_ERR_INVALID, "emmax_op_sample_constrained: token rules need the table's five arrays");
    ConFinishParams p;
    memset(&p, 0, sizeof(p));
    p.f.B = B; p.f.n_out = (int32_t*)n_out; p.f.is_prefill = 1; p.f.max_out = 0; p.f.eos_id = eos_id; p.f.pad_id = pad_id;
    p.logits = logits; p.ld = ld; p.V = V; p.temperature = temperature; p.top_k = top_k; p.top_p = top_p; p.seed = seed; p.subseq = subseq;
    p.min_p = min_p; p.typical_p = typical_p; p.eps_cut = epsilon_cutoff; p.eta_cut = eta_cutoff;
    p.penalty = penalty; p.ngram = ngram; p.min_new = min_new; p.hist = hist; p.hist_len = hist_len; p.max_prompt = max_hist;
    if (n_rules > 0) { p.rt.n_host = n_rules; p.rt.off = rule_off; p.rt.ids = rule_ids; p.rt.flags = rule_flags; p.rt.bias = rule_bias; p.rule_en = rule_enable; }
    p.tok_out = tok_out; p.logprob_out = logprob_out; p.scores_out = scores_out;
    p.cls = cls; p.allow = allow; p.next = next; p.n_states = n_states; p.next_ld = n_classes; p.state = (int32_t*)state; p.state_out = state_out;
    KCHK(launch_con_finish(p, (hipStream_t)stream));
    return 0;
}
int emmax_op_gemm(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* bias, int act,
                  const void* scale, const void* residual, int ldr, int out_f32, emmax_stream st) {
    GemmParams p = gp(A, lda, W, ldw, C, ldc, M, N, K);
    p.bias = bias; p.act = act; p.scale = scale; p.residual = residual; p.ldr = ldr; p.out_f32 = out_f32;
    int r = launch_gemm(p, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_gemm: unsupported shape (K%%64, N%%128, ld%%8) or launch failure");
    return 0;
}
int emmax_op_gemm_splitk(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* bias, int act,
                         const void* scale, const void* residual, int ldr, int out_f32, int ksplit, void* ws, int64_t ws_bytes,
                         emmax_stream st) {
    GemmParams p = gp(A, lda, W, ldw, C, ldc, M, N, K);
    p.bias = bias; p.act = act; p.scale = scale; p.residual = residual; p.ldr = ldr; p.out_f32 = out_f32;
    p.ws = (float*)ws; p.ws_bytes = ws_bytes;
    // ksplit = 0: the launch plan of a session stage with this scratch (whole tiles, split-K, or a column remainder through split-K)
    int r = ksplit == 0 ? launch_gemm(p, (hipStream_t)st) : launch_gemm_splitk(p, ksplit, (hipStream_t)st, emmax_tune().gemm_sk_big > 0 ? 1 : 0);   // (tools: explicit slices, geometry by switch)
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID,
                       "emmax_op_gemm_splitk: unsupported (ksplit = 0 or 2 <= ksplit <= K/64, ws >= ksplit*M*N*4 bytes, K%%64, N%%128; SwiGLU: bf16 output)");
    return 0;
}
int emmax_gemm_plan(int M, int N, int K, int act, int out_f32, int has_ln, int has_residual, int with_norm, int64_t ws_bytes, char* text_out,
                    int text_len) {
    if (!text_out || text_len < 16) return fail(EMMAX_ERR_INVALID, "emmax_gemm_plan: text buffer of at least 16 bytes");
    void* const any = (void*)(uintptr_t)256;   // the plan looks at sizes, alignments and which operands exist -- never through a pointer
    GemmParams p = gp(any, K, any, K, any, act == 2 ? N / 2 : N, M, N, K);
    p.act = act; p.out_f32 = out_f32;
    if (has_residual) { p.residual = any; p.ldr = N; p.res_f32 = has_residual == 2; }   // 2: the fp32 residual stream (with out_f32)
    if (has_ln) { p.ln_stats = (const float*)any; p.ln_s = (const float*)any; p.ln_c = (const float*)any; }
    if (ws_bytes > 0) { p.ws = (float*)any; p.ws_bytes = ws_bytes; }
    if (with_norm) { p.norm_w = any; p.norm_out = any; p.ld_norm = N; p.norm_eps = 1e-5f; }
    if (with_norm && !gemm_fuses_norm(p)) { p.norm_w = nullptr; p.norm_out = nullptr; }   // (what the prefill does: a separate norm launch)
    const int r = gemm_plan_describe(p, text_out, text_len);
    if (r < 0) return fail(EMMAX_ERR_INVALID, "emmax_gemm_plan: unsupported shape (K%%64, N%%128)");
    return 0;
}
int emmax_gemm_launches(int M, int N, int K, int act, int out_f32, int has_ln, int has_residual, int with_norm, int64_t ws_bytes, int has_bias, int has_scale,
                        int lda, int ldw, int ldc, int ldr, int n_store, int a_hl, int c_align, int res_align, int ksplit, char* text_out, int text_len) {
    if (!text_out || text_len < 16) return fail(EMMAX_ERR_INVALID, "emmax_gemm_launches: text buffer of at least 16 bytes");
    if (c_align < 0 || c_align > 15 || res_align < 0 || res_align > 15 || lda < 1 || ldw < 1)
        return fail(EMMAX_ERR_INVALID, "emmax_gemm_launches: alignments are addresses modulo 16 (0..15), pitches positive");
    // the launchers look at sizes, pitches, alignments and which operands exist -- never through a pointer; A and W get bases of their own
    // because the parts of a plan are told apart by their offsets from them
    void* const any = (void*)(uintptr_t)256;
    GemmParams p = gp((void*)((uintptr_t)1 << 40), lda, (void*)((uintptr_t)1 << 41), ldw, (void*)(((uintptr_t)1 << 42) + c_align), ldc, M, N, K);
    p.act = act; p.out_f32 = out_f32; p.N_store = n_store; p.a_hl = a_hl;
    if (has_bias) p.bias = any;
    if (has_scale) p.scale = any;
    if (has_residual) { p.residual = (void*)(((uintptr_t)1 << 43) + res_align); p.ldr = ldr; p.res_f32 = has_residual == 2; }
    if (has_ln) { p.ln_stats = (const float*)any; p.ln_s = (const float*)any; p.ln_c = (const float*)any; }
    if (ws_bytes > 0) { p.ws = (float*)any; p.ws_bytes = ws_bytes; }
    if (with_norm) { p.norm_w = any; p.norm_out = any; p.ld_norm = N; p.norm_eps = 1e-5f; }
    if (with_norm && ksplit == 0 && !gemm_fuses_norm(p)) { p.norm_w = nullptr; p.norm_out = nullptr; }   // (as emmax_gemm_plan: the caller then runs the norm itself)
    const int n = gemm_list_launches(p, ksplit, text_out, text_len);
    if (n < 0) return fail(EMMAX_ERR_INVALID, "emmax_gemm_launches: the launchers refuse this problem (or the text buffer is too small)");
    return n;
}
int emmax_op_gemm_ln(const void* X, int ldx, void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* gamma, const void* beta,
                     const void* bias, float eps, int act, float* stats_ws, float* ln_s_ws, float* ln_c_ws, emmax_stream stream) {
    if (!X || !W || !C || !gamma || !stats_ws || !ln_s_ws || !ln_c_ws) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_ln: null argument");
    if (((uintptr_t)stats_ws & 7) || (((uintptr_t)ln_s_ws | (uintptr_t)ln_c_ws) & 3))   // (mean, rstd) pairs are read as 8 bytes
        return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_ln: workspaces must be 8-byte (stats) / 4-byte (ln_s, ln_c) aligned");
    hipStream_t st = (hipStream_t)stream;
    KCHK(launch_ln_fold(W, ldw, N, K, gamma, beta, bias, ln_s_ws, ln_c_ws, st));
    KCHK(launch_row_stats(X, stats_ws, M, K, ldx, eps, st));
    GemmParams p = gp(X, ldx, W, ldw, C, ldc, M, N, K);
    p.act = act; p.ln_stats = stats_ws; p.ln_s = ln_s_ws; p.ln_c = ln_c_ws;
    int r = launch_gemm(p, st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_gemm_ln: unsupported shape (K%%64, N%%128, ld%%8, act in {0,1})");
    return 0;
}
int emmax_op_layernorm(const void* x, void* y, const void* w, const void* b, int rows, int D, float eps, emmax_stream st) {
    int r = launch_layernorm(x, y, w, b, rows, D, D, D, eps, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_layernorm: unsupported shape");
    return 0;
}
int emmax_op_rmsnorm(const void* x, void* y, const void* w, int rows, int D, float eps, emmax_stream st) {
    int r = launch_rmsnorm(x, y, w, rows, D, D, D, eps, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_rmsnorm: unsupported shape");
    return 0;
}
int emmax_op_attention(const void* qkv, int ld_qkv, int q_off, int k_off, int v_off, void* out, int ld_out, const int32_t* cu, int B,
                       int max_seqlen, int Hq, int Hkv, int head_dim, float scale, int causal, emmax_stream st) {
    AttnParams a;
    a.qkv = qkv; a.out = out; a.cu_seqlens = cu; a.ld_qkv = ld_qkv; a.q_off = q_off; a.k_off = k_off; a.v_off = v_off;
    a.ld_out = ld_out; a.B = B; a.max_seqlen = max_seqlen; a.Hq = Hq; a.Hkv = Hkv; a.scale = scale; a.causal = causal;
    int r = launch_attention(a, head_dim, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_attention: unsupported head_dim/strides");
    return 0;
}
int emmax_op_decode_attention(const void* q, const void* kcache, const void* vcache, const int32_t* page_table, const int32_t* ctx_len,
                              const int32_t* done, float* part_out, int B, int Hq, int Hkv, int page, int max_pages, int nsplit, float scale,
                              int* nsplit_out, emmax_stream st) {
    if (!q || !kcache || !vcache || !page_table || !ctx_len || !part_out) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention: null argument");
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || Hkv < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention: bad B / heads");
    DecodeAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = Hq * 128; a.kcache = kcache; a.vcache = vcache; a.page_table = page_table; a.ctx_len = ctx_len; a.done = done;
    a.part = part_out; a.Hkv = Hkv; a.page = page; a.max_pages = max_pages; a.scale = scale;
    const int ns = nsplit > 0 ? nsplit : decode_attn_nsplit(B, Hkv);
    if (nsplit_out) *nsplit_out = ns;
    if (ns > 16) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention: nsplit %d > 16", ns);
    int r = launch_decode_attn(a, B, Hq, 128, ns, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_decode_attention: unsupported (GQA group in {1,2,4,8}, page = 2^k, max_pages <= 512, nsplit = 2^k)");
    return 0;
}
int emmax_op_decode_attention_direct(const void* q, const void* kcache, const void* vcache, const int32_t* page_table, const int32_t* ctx_len,
                                     const int32_t* done, void* o_out, int B, int Hq, int Hkv, int page, int max_pages, float scale,
                                     emmax_stream st) {
    if (!q || !kcache || !vcache || !page_table || !ctx_len || !o_out) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention_direct: null argument");
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || Hkv < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention_direct: bad B / heads");
    DecodeAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = Hq * 128; a.kcache = kcache; a.vcache = vcache; a.page_table = page_table; a.ctx_len = ctx_len; a.done = done;
    a.part = nullptr; a.Hkv = Hkv; a.page = page; a.max_pages = max_pages; a.scale = scale; a.o_out = o_out;
    int r = launch_decode_attn(a, B, Hq, 128, 1, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_decode_attention_direct: unsupported (GQA group in {1,2,4,8}, page = 2^k, max_pages <= 512)");
    return 0;
}
int emmax_op_decode_attention_kv8(const void* q, void* kcache8, void* vcache8, float* kscale, float* vscale, const void* kv_stage,
                                  const int32_t* page_table, const int32_t* ctx_len, const int32_t* done, float* part_out, void* o_out, int B, int Hq,
                                  int Hkv, int page, int max_pages, int nsplit, float scale, emmax_stream st) {
    if (!q || !kcache8 || !vcache8 || !kscale || !vscale || !kv_stage || !page_table || !ctx_len || (!part_out && !o_out))
        return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention_kv8: null argument");
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || Hkv < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention_kv8: bad B / heads");
    DecodeAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = Hq * 128; a.kcache = kcache8; a.vcache = vcache8; a.kscale = kscale; a.vscale = vscale; a.kv_stage = kv_stage;
    a.page_table = page_table; a.ctx_len = ctx_len; a.done = done; a.part = part_out; a.o_out = o_out;
    a.Hkv = Hkv; a.page = page; a.max_pages = max_pages; a.scale = scale;
    const int ns = o_out ? 1 : (nsplit > 0 ? nsplit : decode_attn_nsplit(B, Hkv));
    if (ns > 16) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention_kv8: nsplit %d > 16", ns);
    int r = launch_decode_attn(a, B, Hq, 128, ns, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_decode_attention_kv8: unsupported (GQA group in {1,2,4,8}, page = 2^k, max_pages <= 512, nsplit = 2^k)");
    return 0;
}
// ---- the form of the prefill / ViT attention, host only (attention.hip: attention_form -- what launch_attention dispatches on) ----
int emmax_attention_plan(int B, int max_seqlen, int Hq, int Hkv, int head_dim, int causal, int* resident_out, int* query_waves_out, int* producer_waves_out,
                         int* key_groups_out, int* lazy_out, int* rows_out) {
    AttnForm f;
    if (!attention_form(B, max_seqlen, Hq, Hkv, head_dim, causal ? 1 : 0, &f))
        return fail(EMMAX_ERR_INVALID, "emmax_attention_plan: unsupported (B >= 1, max_seqlen >= 1, Hq a multiple of Hkv, head_dim in {64, 72, 128})");
    if (resident_out) *resident_out = f.resident;
    if (query_waves_out) *query_waves_out = f.qwaves;
    if (producer_waves_out) *producer_waves_out = f.pwaves;
    if (key_groups_out) *key_groups_out = f.kgroups;
    if (lazy_out) *lazy_out = f.lazy;
    if (rows_out) *rows_out = f.rows;
    return 0;
}
// ---- the forms of the decode attention, host only (decode_attn.hip: decode_attn_form / group_attn_form -- what the launchers dispatch on) ----
static void attn_plan_operands(DecodeAttnParams& a, int Hq, int Hkv, int direct, int kv8) {
    void* const any = (void*)(uintptr_t)256;   // the form looks at which operands exist -- never through a pointer
    memset(&a, 0, sizeof(a));
    a.q = any; a.ldq = Hq * 128; a.kcache = any; a.vcache = any; a.page_table = (const int32_t*)any; a.ctx_len = (const int32_t*)any;
    a.part = (float*)any; a.Hkv = Hkv; a.page = 64; a.max_pages = 1;
    if (direct) a.o_out = any;
    if (kv8) { a.kv_stage = any; a.kscale = (float*)any; a.vscale = (float*)any; }
}
int emmax_decode_attn_plan(int B, int Hq, int Hkv, int nsplit, int direct, int kv8, int* G_out, int* nw_out, int* direct_out, int* deep_out,
                           int* nsplit_out) {
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || Hkv < 1 || Hq < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_decode_attn_plan: bad B / heads");
    const bool step = nsplit == 0 && direct == -1;   // what a B-row step launches: decode_attn_nsplit + the one-split rule (step.hip: run_decode_stage)
    if (!step && (nsplit < 1 || nsplit > 16 || (direct != 0 && direct != 1)))
        return fail(EMMAX_ERR_INVALID, "emmax_decode_attn_plan: nsplit 1..16 with direct 0 / 1, or nsplit 0 with direct -1 (a step's own choice)");
    if (step) { nsplit = decode_attn_nsplit(B, Hkv); direct = attn_direct_rule(B, Hkv, false) ? 1 : 0; }
    DecodeAttnParams a;
    attn_plan_operands(a, Hq, Hkv, direct, kv8);
    DecodeAttnForm f;
    if (!decode_attn_form(a, B, Hq, nsplit, &f))
        return fail(EMMAX_ERR_INVALID, "emmax_decode_attn_plan: unsupported (GQA group in {1,2,4,8}, nsplit = 2^k, one split for the direct form)");
    if (G_out) *G_out = f.G;
    if (nw_out) *nw_out = f.nw;
    if (direct_out) *direct_out = f.direct;
    if (deep_out) *deep_out = f.deep;
    if (nsplit_out) *nsplit_out = f.nsplit;
    return 0;
}
int emmax_group_attn_plan(int B, int N, int Hq, int Hkv, int kv8, int* span_width_out, int* span_nsplit_out, int* span_chunks_out, int* tail_G_out) {
    if (Hkv < 1 || Hq < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_group_attn_plan: bad heads");
    DecodeAttnParams a;
    attn_plan_operands(a, Hq, Hkv, 1, kv8);
    GroupAttnForm f;
    if (!group_attn_form(a, B, N, Hq, &f))
        return fail(EMMAX_ERR_INVALID, "emmax_group_attn_plan: unsupported (whole groups of N >= 2 rows, B <= %d, GQA group in {1,2,4,8})", EMMAX_MAX_DECODE_BATCH);
    if (span_width_out) *span_width_out = f.width;
    if (span_nsplit_out) *span_nsplit_out = f.nsplit;
    if (span_chunks_out) *span_chunks_out = f.chunks;
    if (tail_G_out) *tail_G_out = f.G;
    return 0;
}
// ---- extend_attn.hip as pure ops: n new rows per sequence over the paged cache.  cu and base are read back and checked on the host BEFORE
// anything is launched (the call synchronises the stream and cannot be captured) ----
int emmax_extend_attn_plan(int B, int max_n, int max_L, int Hq, int Hkv, int nsplit, int kv8, int* G_out, int* tokens_per_block_out, int* query_tiles_out,
                           int* nsplit_out, int* split_form_out) {
    ExtendAttnPlan f;
    if (B > EMMAX_MAX_DECODE_BATCH || !extend_attn_plan(B, max_n, max_L, Hq, Hkv, nsplit, kv8, &f))
        return fail(EMMAX_ERR_INVALID, "emmax_extend_attn_plan: unsupported (B 1..%d, 1 <= max_n <= max_L, GQA group in {1,2,4,8}, nsplit 0..16)", EMMAX_MAX_DECODE_BATCH);
    if (G_out) *G_out = f.G;
    if (tokens_per_block_out) *tokens_per_block_out = f.qt;
    if (query_tiles_out) *query_tiles_out = f.nqt;
    if (nsplit_out) *nsplit_out = f.nsplit;
    if (split_form_out) *split_form_out = f.split;
    return 0;
}
// ---- score.hip as a pure op: the scoring launch and its merge ----
int emmax_score_plan(int rows, int V, int K, int64_t ws_bytes, int* row_tiles_out, int* col_tiles_out, int* slices_out, int* tiles_per_slice_out) {
    ScoreForm f;
    if (!score_form(rows, V, K, ws_bytes, 0, &f))
        return fail(EMMAX_ERR_INVALID, "emmax_score_plan: unsupported (rows >= 1, V >= 1, K a multiple of 64, a scratch of at least 12 x rows bytes)");
    if (row_tiles_out) *row_tiles_out = f.row_tiles;
    if (col_tiles_out) *col_tiles_out = f.col_tiles;
    if (slices_out) *slices_out = f.slices;
    if (tiles_per_slice_out) *tiles_per_slice_out = f.tps;
    return 0;
}
int emmax_op_score_rows(const void* x_dev, int ldx, const void* W_dev, int ldw, int rows, int V, int Np, int K, const int32_t* targets_dev, int slices, float* ws_dev,
                        int64_t ws_bytes, float* lse_out_dev, float* target_logit_out_dev, int32_t* argmax_out_dev, emmax_stream st) {
    const char* who = "emmax_op_score_rows";
    if (!x_dev || !W_dev || !targets_dev || !ws_dev || !lse_out_dev || !target_logit_out_dev || !argmax_out_dev) return fail(EMMAX_ERR_INVALID, "%s: null argument", who);
    if (rows < 1 || V < 1) return fail(EMMAX_ERR_INVALID, "%s: rows %d and V %d must be at least 1", who, rows, V);
    if (K < 64 || K % 64) return fail(EMMAX_ERR_INVALID, "%s: K %d is not a multiple of 64 (one K step of the tile)", who, K);
    if (Np < V || Np % 128) return fail(EMMAX_ERR_INVALID, "%s: Np %d must be V = %d padded to a multiple of 128 (the kernel reads whole 128-row tiles of W)", who, Np, V);
    if (ldx < K || ldw < K || ldx % 8 || ldw % 8 || (((uintptr_t)x_dev | (uintptr_t)W_dev) & 15) || ((uintptr_t)ws_dev & 3))
        return fail(EMMAX_ERR_INVALID, "%s: ldx %d / ldw %d at least K in multiples of 8, x and W 16-byte aligned (16-byte requests)", who, ldx, ldw);
    const int col_tiles = (V + 127) / 128;
    if (slices < 0 || slices > col_tiles) return fail(EMMAX_ERR_INVALID, "%s: %d slices outside 0..%d (the 128-column tiles below V = %d)", who, slices, col_tiles, V);
    ScoreForm f;
    if (!score_form(rows, V, K, ws_bytes, slices, &f))
        return fail(EMMAX_ERR_INVALID, "%s: a scratch of %lld bytes is too small for %d slice(s) of %d rows (12 bytes per row and slice)", who, (long long)ws_bytes,
                    slices ? slices : 1, rows);
    ScoreParams p;
    memset(&p, 0, sizeof(p));
    p.X = x_dev; p.W = W_dev; p.targets = targets_dev; p.ws = ws_dev; p.lse = lse_out_dev; p.target_logit = target_logit_out_dev; p.argmax = argmax_out_dev;
    p.ldx = ldx; p.ldw = ldw; p.rows = rows; p.V = V; p.K = K;
    const int r = launch_score_rows(p, f, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s: launch failure", who);
    return 0;
}
// cu / base of an extension op on the host: 0 = cu[0] < cu[1] < .. = total_rows, 0 <= base[b], base[b] + n[b] <= limit
static int extend_op_lengths(const char* who, const int32_t* cu, const int32_t* base, int B, int total_rows, long limit, int* max_n, int* max_L, hipStream_t st) {
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || total_rows < B) return fail(EMMAX_ERR_INVALID, "%s: B %d (1..%d), total_rows %d (>= B)", who, B, EMMAX_MAX_DECODE_BATCH, total_rows);
    int32_t h_cu[EMMAX_MAX_DECODE_BATCH + 1], h_base[EMMAX_MAX_DECODE_BATCH];
    HIPCHK(hipMemcpyAsync(h_cu, cu, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_base, base, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_cu[0] != 0 || h_cu[B] != total_rows) return fail(EMMAX_ERR_INVALID, "%s: cu_seqlens runs %d..%d, not 0..total_rows = %d", who, h_cu[0], h_cu[B], total_rows);
    *max_n = 0; *max_L = 0;
    for (int b = 0; b < B; ++b) {
        const int n = h_cu[b + 1] - h_cu[b];
        if (n < 1) return fail(EMMAX_ERR_INVALID, "%s: sequence %d has %d new rows (>= 1)", who, b, n);
        if (h_base[b] < 0 || (long)h_base[b] + n > limit)
            return fail(EMMAX_ERR_INVALID, "%s: sequence %d: base %d + %d new rows outside 0..%ld (the page table / the RoPE tables)", who, b, h_base[b], n, limit);
        *max_n = std::max(*max_n, n);
        *max_L = std::max(*max_L, h_base[b] + n);
    }
    return 0;
}
static int op_extend_attention(const char* who, ExtendAttnParams& a, int total_rows, int page, int nsplit, int kv8, long long ws_floats, int* nsplit_out,
                               hipStream_t st) {
    if (!a.q || !a.out || !a.kcache || !a.vcache || !a.page_table || !a.cu || !a.base) return fail(EMMAX_ERR_INVALID, "%s: null argument", who);
    if (page != 64) return fail(EMMAX_ERR_INVALID, "%s: page %d (one K / V tile is one page of 64 keys)", who, page);
    if (a.Hkv < 1 || a.Hq < 1 || a.Hq % a.Hkv || a.max_pages < 1) return fail(EMMAX_ERR_INVALID, "%s: heads %d / %d, max_pages %d", who, a.Hq, a.Hkv, a.max_pages);
    if (a.ldq % 8 || a.q_off % 8 || a.ld_out % 8 || a.q_off < 0 || a.q_off + a.Hq * 128 > a.ldq || a.ld_out < a.Hq * 128)
        return fail(EMMAX_ERR_INVALID, "%s: ldq %d, q_off %d, ld_out %d in multiples of 8, the %d heads of 128 inside a row", who, a.ldq, a.q_off, a.ld_out, a.Hq);
    if ((((uintptr_t)a.q | (uintptr_t)a.out | (uintptr_t)a.part) & 15) || (((uintptr_t)a.kcache | (uintptr_t)a.vcache) & (kv8 ? 7 : 15)) ||
        (((uintptr_t)a.kscale | (uintptr_t)a.vscale | (uintptr_t)a.cu | (uintptr_t)a.base | (uintptr_t)a.page_table) & 3))
        return fail(EMMAX_ERR_INVALID, "%s: q, out, the workspace and bf16 pages 16-byte aligned, e4m3 pages 8-byte, scales and tables 4-byte", who);
    int max_n = 0, max_L = 0;
    if (int r = extend_op_lengths(who, a.cu, a.base, a.B, total_rows, (long)a.max_pages * page, &max_n, &max_L, st)) return r;
    ExtendAttnPlan f;
    if (!extend_attn_plan(a.B, max_n, max_L, a.Hq, a.Hkv, nsplit, kv8, &f)) return fail(EMMAX_ERR_INVALID, "%s: unsupported (GQA group in {1,2,4,8}, nsplit 0..16)", who);
    if (nsplit_out) *nsplit_out = f.nsplit;
    if (f.split && (!a.part || ws_floats < (long long)total_rows * a.Hq * f.nsplit * EMMAX_PSTRIDE))
        return fail(EMMAX_ERR_INVALID, "%s: %d splits need a workspace of total_rows x Hq x nsplit x %d = %lld floats (given %lld)", who, f.nsplit, EMMAX_PSTRIDE,
                    (long long)total_rows * a.Hq * f.nsplit * EMMAX_PSTRIDE, ws_floats);
    const int r = launch_extend_attn(a, f, total_rows, st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s: launch failure", who);
    return 0;
}
int emmax_op_extend_attention(const void* q, int ldq, int q_off, const void* kcache, const void* vcache, const int32_t* page_table, const int32_t* cu,
                              const int32_t* base, int B, int total_rows, int Hq, int Hkv, int page, int max_pages, int nsplit, float scale, void* out, int ld_out,
                              float* ws, long long ws_floats, int* nsplit_out, emmax_stream st) {
    ExtendAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = ldq; a.q_off = q_off; a.out = out; a.ld_out = ld_out; a.kcache = kcache; a.vcache = vcache; a.page_table = page_table; a.cu = cu; a.base = base;
    a.part = ws; a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.max_pages = max_pages; a.scale = scale;
    return op_extend_attention("emmax_op_extend_attention", a, total_rows, page, nsplit, 0, ws_floats, nsplit_out, (hipStream_t)st);
}
int emmax_op_extend_attention_kv8(const void* q, int ldq, int q_off, const void* kcache8, const void* vcache8, const float* kscale, const float* vscale,
                                  const int32_t* page_table, const int32_t* cu, const int32_t* base, int B, int total_rows, int Hq, int Hkv, int page, int max_pages,
                                  int nsplit, float scale, void* out, int ld_out, float* ws, long long ws_floats, int* nsplit_out, emmax_stream st) {
    if (!kscale || !vscale) return fail(EMMAX_ERR_INVALID, "emmax_op_extend_attention_kv8: null argument");
    ExtendAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = ldq; a.q_off = q_off; a.out = out; a.ld_out = ld_out; a.kcache = kcache8; a.vcache = vcache8; a.kscale = kscale; a.vscale = vscale;
    a.page_table = page_table; a.cu = cu; a.base = base; a.part = ws; a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.max_pages = max_pages; a.scale = scale;
    return op_extend_attention("emmax_op_extend_attention_kv8", a, total_rows, page, nsplit, 1, ws_floats, nsplit_out, (hipStream_t)st);
}
// ---- taps.hip as pure ops.  The lengths are read back and checked first, as above: ld_keys holds every key a row can see ----
static int op_attn_probs(const char* who, AttnProbsParams& a, int total_rows, int page, int kv8, hipStream_t st) {
    if (!a.q || !a.probs || !a.kcache || !a.page_table || !a.cu || !a.base) return fail(EMMAX_ERR_INVALID, "%s: null argument", who);
    if (page != 64) return fail(EMMAX_ERR_INVALID, "%s: page %d (one K tile is one page of 64 keys)", who, page);
    if (a.Hkv < 1 || a.Hq < 1 || a.Hq % a.Hkv || a.max_pages < 1) return fail(EMMAX_ERR_INVALID, "%s: heads %d / %d, max_pages %d", who, a.Hq, a.Hkv, a.max_pages);
    const int G = a.Hq / a.Hkv;
    if (G != 1 && G != 2 && G != 4 && G != 8) return fail(EMMAX_ERR_INVALID, "%s: unsupported GQA group %d (1, 2, 4 or 8)", who, G);
    if (a.ldq % 8 || a.q_off % 8 || a.q_off < 0 || a.q_off + a.Hq * 128 > a.ldq)
        return fail(EMMAX_ERR_INVALID, "%s: ldq %d, q_off %d in multiples of 8, the %d heads of 128 inside a row", who, a.ldq, a.q_off, a.Hq);
    if (a.ld_keys < 4 || a.ld_keys % 4) return fail(EMMAX_ERR_INVALID, "%s: ld_keys %d is not a positive multiple of 4 (16-byte stores)", who, a.ld_keys);
    if ((((uintptr_t)a.q | (uintptr_t)a.probs) & 15) || ((uintptr_t)a.kcache & (kv8 ? 7 : 15)) ||
        (((uintptr_t)a.kscale | (uintptr_t)a.cu | (uintptr_t)a.base | (uintptr_t)a.page_table) & 3))
        return fail(EMMAX_ERR_INVALID, "%s: q, probs and bf16 pages 16-byte aligned, e4m3 pages 8-byte, scales and tables 4-byte", who);
    int max_n = 0, max_L = 0;
    if (int r = extend_op_lengths(who, a.cu, a.base, a.B, total_rows, (long)a.max_pages * page, &max_n, &max_L, st)) return r;
    if (max_L > a.ld_keys) return fail(EMMAX_ERR_INVALID, "%s: ld_keys %d is smaller than the %d keys a row sees", who, a.ld_keys, max_L);
    const int r = launch_attn_probs(a, max_n, kv8, st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s: launch failure", who);
    return 0;
}
int emmax_op_attn_probs(const void* q, int ldq, int q_off, const void* kcache, const int32_t* page_table, const int32_t* cu, const int32_t* base, int B,
                        int total_rows, int Hq, int Hkv, int page, int max_pages, float scale, float* probs, int ld_keys, emmax_stream st) {
    AttnProbsParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = ldq; a.q_off = q_off; a.kcache = kcache; a.page_table = page_table; a.cu = cu; a.base = base; a.probs = probs; a.ld_keys = ld_keys;
    a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.max_pages = max_pages; a.scale = scale;
    return op_attn_probs("emmax_op_attn_probs", a, total_rows, page, 0, (hipStream_t)st);
}
int emmax_op_attn_probs_kv8(const void* q, int ldq, int q_off, const void* kcache8, const float* kscale, const int32_t* page_table, const int32_t* cu,
                            const int32_t* base, int B, int total_rows, int Hq, int Hkv, int page, int max_pages, float scale, float* probs, int ld_keys,
                            emmax_stream st) {
    if (!kscale) return fail(EMMAX_ERR_INVALID, "emmax_op_attn_probs_kv8: null argument");
    AttnProbsParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = ldq; a.q_off = q_off; a.kcache = kcache8; a.kscale = kscale; a.page_table = page_table; a.cu = cu; a.base = base; a.probs = probs;
    a.ld_keys = ld_keys; a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.max_pages = max_pages; a.scale = scale;
    return op_attn_probs("emmax_op_attn_probs_kv8", a, total_rows, page, 1, (hipStream_t)st);
}
int emmax_op_tap_rows(const void* src, int src_f32, int ld_src, float* dst, int rows, int H, const void* norm_w, float eps, emmax_stream st) {
    if (!src || !dst) return fail(EMMAX_ERR_INVALID, "emmax_op_tap_rows: null argument");
    if (rows < 1 || H < 8 || H % 8 || ld_src < H || ld_src % (src_f32 ? 4 : 8) || (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)norm_w) & 15))
        return fail(EMMAX_ERR_INVALID, "emmax_op_tap_rows: rows %d (>= 1), H %d (a multiple of 8), ld_src %d (>= H, 16-byte rows), 16-byte aligned pointers", rows, H,
                    ld_src);
    TapRowsParams p;
    memset(&p, 0, sizeof(p));
    p.src = src; p.src_f32 = src_f32 ? 1 : 0; p.ld_src = ld_src; p.dst = dst; p.rows = rows; p.H = H; p.norm_w = norm_w; p.eps = eps;
    const int r = launch_tap_rows(p, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_tap_rows: launch failure");
    return 0;
}
int emmax_op_rope_kv_write_at(void* qkv, int ld, int q_off, int k_off, int v_off, const int32_t* cu, const int32_t* base, int B, int total_rows, const float* cos_t,
                              const float* sin_t, int max_pos, void* kcache, void* vcache, const int32_t* page_table, int max_pages, int Hq, int Hkv, int head_dim,
                              int page, emmax_stream stream) {
    const char* who = "emmax_op_rope_kv_write_at";
    if (!qkv || !cu || !base || !cos_t || !sin_t || !page_table) return fail(EMMAX_ERR_INVALID, "%s: null argument", who);
    if ((kcache == nullptr) != (vcache == nullptr)) return fail(EMMAX_ERR_INVALID, "%s: kcache and vcache go together (both null: rotate only)", who);
    if (Hq < 1 || Hkv < 1 || page < 1 || max_pages < 1 || max_pos < 1) return fail(EMMAX_ERR_INVALID, "%s: heads %d / %d, page %d, max_pages %d, max_pos %d", who, Hq, Hkv, page, max_pages, max_pos);
    if (head_dim < 16 || head_dim % 16 || (ld | q_off | k_off | v_off) % 8 || q_off < 0 || k_off < 0 || v_off < 0 || q_off + Hq * head_dim > ld || k_off + Hkv * head_dim > ld ||
        v_off + Hkv * head_dim > ld)
        return fail(EMMAX_ERR_INVALID, "%s: head_dim %d in multiples of 16, ld %d and the offsets %d / %d / %d in multiples of 8, the heads inside a row", who, head_dim, ld, q_off, k_off, v_off);
    if ((((uintptr_t)qkv | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)cos_t | (uintptr_t)sin_t) & 15) || (((uintptr_t)cu | (uintptr_t)base | (uintptr_t)page_table) & 3))
        return fail(EMMAX_ERR_INVALID, "%s: qkv, the caches and the RoPE tables must be 16-byte aligned, the index arrays 4-byte aligned", who);
    int max_n = 0, max_L = 0;
    if (int r = extend_op_lengths(who, cu, base, B, total_rows, std::min((long)max_pages * page, (long)max_pos), &max_n, &max_L, (hipStream_t)stream)) return r;
    const int r = launch_rope_kv_write_at(qkv, ld, q_off, k_off, v_off, cu, base, B, total_rows, cos_t, sin_t, kcache, vcache, page_table, max_pages, Hq, Hkv, head_dim, page,
                                          max_pos, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s: launch failure", who);
    return 0;
}
// the grouped form (decode_attn.hip: launch_group_attn) as a pure op: the shapes and the groups' shared page counts are checked on the host
// BEFORE anything is launched (the counts are read back: the call synchronises the stream and cannot be captured)
static int op_group_attention(const char* who, DecodeAttnParams& a, int B, int Hq, int N, const int32_t* shared_pages, hipStream_t st) {
    if (!a.q || !a.kcache || !a.vcache || !a.page_table || !a.ctx_len || !a.o_out || !a.part || !shared_pages) return fail(EMMAX_ERR_INVALID, "%s: null argument", who);
    if (N < 2 || B < 1 || B % N) return fail(EMMAX_ERR_INVALID, "%s: %d rows are not whole groups of N = %d >= 2 rows", who, B, N);
    if (!group_attn_takes(B, N, Hq, a.Hkv) || a.max_pages < 1 || a.max_pages > 512 || a.page < 1 || (a.page & (a.page - 1)))
        return fail(EMMAX_ERR_INVALID, "%s: unsupported (B <= %d, GQA group in {1,2,4,8}, page = 2^k, max_pages <= 512)", who, EMMAX_MAX_DECODE_BATCH);
    int32_t sh[EMMAX_MAX_DECODE_BATCH], ctx[EMMAX_MAX_DECODE_BATCH];
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(sh, shared_pages, (size_t)(B / N) * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ctx, a.ctx_len, (size_t)B * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
        const int g = b / N;
        if (sh[g] < 0 || sh[g] > a.max_pages) return fail(EMMAX_ERR_INVALID, "%s: group %d shares %d pages of a table of %d", who, g, sh[g], a.max_pages);
        // (a span past a row's context would leave the row's tail empty: it would write zeros and drop the partials)
        if ((long long)sh[g] * a.page > ctx[b]) return fail(EMMAX_ERR_INVALID, "%s: group %d shares %d pages, row %d holds %d keys", who, g, sh[g], b, ctx[b]);
    }
    a.grp_shared = shared_pages;
    const int r = launch_group_attn(a, B, N, Hq, 128, st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "%s: launch failed (%d)", who, r);
    return 0;
}
int emmax_op_decode_attention_group(const void* q, const void* kcache, const void* vcache, const int32_t* page_table, const int32_t* ctx_len,
                                    const int32_t* done, void* o_out, int B, int Hq, int Hkv, int page, int max_pages, float scale, int N,
                                    const int32_t* shared_pages, float* part_ws, emmax_stream st) {
    if (Hkv < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention_group: bad heads");
    DecodeAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = Hq * 128; a.kcache = kcache; a.vcache = vcache; a.page_table = page_table; a.ctx_len = ctx_len; a.done = done;
    a.part = part_ws; a.Hkv = Hkv; a.page = page; a.max_pages = max_pages; a.scale = scale; a.o_out = o_out;
    return op_group_attention("emmax_op_decode_attention_group", a, B, Hq, N, shared_pages, (hipStream_t)st);
}
int emmax_op_decode_attention_group_kv8(const void* q, void* kcache8, void* vcache8, float* kscale, float* vscale, const void* kv_stage,
                                        const int32_t* page_table, const int32_t* ctx_len, const int32_t* done, float* part_ws, void* o_out, int B,
                                        int Hq, int Hkv, int page, int max_pages, int N, const int32_t* shared_pages, float scale, emmax_stream st) {
    if (Hkv < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention_group_kv8: bad heads");
    if (!kscale || !vscale || !kv_stage) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_attention_group_kv8: null argument");
    DecodeAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = Hq * 128; a.kcache = kcache8; a.vcache = vcache8; a.kscale = kscale; a.vscale = vscale; a.kv_stage = kv_stage;
    a.page_table = page_table; a.ctx_len = ctx_len; a.done = done; a.part = part_ws; a.o_out = o_out;
    a.Hkv = Hkv; a.page = page; a.max_pages = max_pages; a.scale = scale;
    return op_group_attention("emmax_op_decode_attention_group_kv8", a, B, Hq, N, shared_pages, (hipStream_t)st);
}
// ---- exact numerics: single-kernel entry points (fp32 in, fp32 out; hl_ws: caller scratch for the two-term image of the operand) ----
int emmax_op_x_gemm(const float* A32, int lda, const void* W, int ldw, float* C32, int ldc, int M, int N, int K, const void* bias, int act,
                    const float* residual32, int ldr, void* hl_ws, void* ws, int64_t ws_bytes, emmax_stream stream) {
    if (!A32 || !W || !C32 || !hl_ws) return fail(EMMAX_ERR_INVALID, "emmax_op_x_gemm: null argument");
    if (K % 64 || N % 128) return fail(EMMAX_ERR_INVALID, "emmax_op_x_gemm: K %% 64, N %% 128 required");
    hipStream_t st = (hipStream_t)stream;
    KCHK(launch_x_split_rows(A32, hl_ws, M, K, K, lda, 2 * K, st));
    GemmParams p = gp(hl_ws, 2 * K, W, ldw, C32, ldc, M, N, 2 * K);
    p.a_hl = 1; p.out_f32 = 1; p.bias = bias; p.act = act;
    if (act == 2) p.N_store = N;
    if (residual32) { p.residual = residual32; p.res_f32 = 1; p.ldr = ldr; }
    if (ws) { p.ws = (float*)ws; p.ws_bytes = ws_bytes; }
    int r = launch_gemm(p, st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_x_gemm: unsupported shape or launch failure");
    return 0;
}
int emmax_op_x_rownorm(int mode, const float* x, float* y32, const void* w, const void* b, int rows, int D, float eps, void* hl_ws, emmax_stream stream) {
    if (!x || !y32 || !hl_ws || (mode != 0 && !w) || (mode == 2 && !b)) return fail(EMMAX_ERR_INVALID, "emmax_op_x_rownorm: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int Dp = pad_to(D, 64);
    int r = mode == 0 ? launch_x_split_rows(x, hl_ws, rows, D, Dp, D, 2 * Dp, st)
          : mode == 1 ? (D % 64 ? -1 : launch_x_rmsnorm(x, hl_ws, w, rows, D, D, 2 * Dp, eps, st))
                      : launch_x_layernorm(x, hl_ws, w, b, rows, D, Dp, D, 2 * Dp, eps, st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_x_rownorm: unsupported shape (D %% 8; RMSNorm: D %% 64)");
    KCHK(launch_x_join_rows(hl_ws, y32, rows, D, 2 * Dp, D, st));
    return 0;
}
int emmax_op_x_attention(const float* qkv32, int ld_qkv, int q_off, int k_off, int v_off, const int32_t* cu, int B,
                         int max_seqlen, int Hq, int Hkv, int head_dim, float scale, int causal, void* hl_ws, emmax_stream stream) {
    if (!qkv32 || !cu || !hl_ws) return fail(EMMAX_ERR_INVALID, "emmax_op_x_attention: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int Dq = Hq * head_dim, Dp = pad_to(Dq, 64);
    AttnParams a;
    a.qkv = qkv32; a.out = hl_ws; a.cu_seqlens = cu; a.ld_qkv = ld_qkv; a.q_off = q_off; a.k_off = k_off; a.v_off = v_off;
    a.ld_out = 2 * Dp; a.B = B; a.max_seqlen = max_seqlen; a.Hq = Hq; a.Hkv = Hkv; a.scale = scale; a.causal = causal;
    int r = launch_x_attention(a, head_dim, st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_x_attention: unsupported head_dim (64, 72, 128) / strides");
    return 0;   // the result stays in hl_ws as HL rows of pitch 2 * pad64(Hq * head_dim): emmax_op_x_join widens them
}
int emmax_op_x_join(const void* hl, float* out32, int rows, int D, emmax_stream stream) {
    if (!hl || !out32) return fail(EMMAX_ERR_INVALID, "emmax_op_x_join: null argument");
    const int Dp = pad_to(D, 64);
    KCHK(launch_x_join_rows(hl, out32, rows, D, 2 * Dp, D, (hipStream_t)stream));
    return 0;
}
int emmax_op_x_decode_attention(const float* q32, const void* kcache32, const void* vcache32, int64_t kv24_elems, const int32_t* page_table,
                                const int32_t* ctx_len, const int32_t* done, float* part_out, int B, int Hq, int Hkv, int page, int max_pages, int nsplit,
                                float scale, emmax_stream st) {
    if (!q32 || !kcache32 || !vcache32 || !page_table || !ctx_len || !part_out) return fail(EMMAX_ERR_INVALID, "emmax_op_x_decode_attention: null argument");
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || Hkv < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_op_x_decode_attention: bad B / heads");
    DecodeAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q32; a.ldq = Hq * 128; a.kcache = kcache32; a.vcache = vcache32; a.page_table = page_table; a.ctx_len = ctx_len; a.done = done;
    a.part = part_out; a.Hkv = Hkv; a.page = page; a.max_pages = max_pages; a.scale = scale; a.kv24 = kv24_elems;
    int r = launch_x_decode_attn(a, B, Hq, 128, nsplit, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_x_decode_attention: unsupported (GQA group in {1,2,4,8}, page = 2^k, max_pages <= 512, nsplit = 2^k)");
    return 0;
}
int emmax_op_x_decode_attention_direct(float* q32, const void* kcache32, const void* vcache32, int64_t kv24_elems, const int32_t* page_table,
                                       const int32_t* ctx_len, const int32_t* done, int B, int Hq, int Hkv, int page, int max_pages, float scale,
                                       emmax_stream st) {
    if (!q32 || !kcache32 || !vcache32 || !page_table || !ctx_len) return fail(EMMAX_ERR_INVALID, "emmax_op_x_decode_attention_direct: null argument");
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || Hkv < 1 || Hq % Hkv) return fail(EMMAX_ERR_INVALID, "emmax_op_x_decode_attention_direct: bad B / heads");
    DecodeAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q32; a.ldq = Hq * 128; a.kcache = kcache32; a.vcache = vcache32; a.page_table = page_table; a.ctx_len = ctx_len; a.done = done;
    a.o_out = q32; a.Hkv = Hkv; a.page = page; a.max_pages = max_pages; a.scale = scale; a.kv24 = kv24_elems;   // in place, as run_decode_stage launches it
    int r = launch_x_decode_attn(a, B, Hq, 128, 1, (hipStream_t)st);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_x_decode_attention_direct: unsupported (GQA group in {1,2,4,8}, page = 2^k, max_pages <= 512)");
    return 0;
}
// ---- one decode stage through the product's own dispatch (tests/test_decode_stages_gpu.py) ----------------------------
// e4m3 (OCP: bias 7, no infinities, 0x7f / 0xff = NaN) as the fp8 KV cache holds it
static float e4m3_to_float(uint8_t v) {
    const int e = (v >> 3) & 15, mant = v & 7;
    float f;
    if (e == 15 && mant == 7) f = NAN;
    else if (e == 0) f = ldexpf((float)mant, -9);
    else f = ldexpf((float)(8 + mant), e - 10);
    return (v & 0x80) ? -f : f;
}
static float bits_to_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// the session's own per-row state swapped for the op's scratch rows while a stage runs (host pointers only: nothing on the device moves)
namespace {
struct OpRows {
    emmax_session* s;
    RowState saved;
    explicit OpRows(emmax_session* s_) : s(s_), saved(s_->rows) {
        int32_t* c = s->op_state;   // seven columns of op_rows rows -- ctx_len first, then cur_tok -- and the output rows
        const int R = s->op_rows;
        s->rows = RowState{/* cur_tok */ c + R, /* ctx_len */ c, c + 2 * R, c + 3 * R, c + 4 * R, c + 5 * R, c + 6 * R, s->op_out};
    }
    OpRows(const OpRows&) = delete;
    ~OpRows() { s->rows = saved; }
};
}  // namespace

static int decode_stage_run(emmax_session* s, int layer, int stage, int B, const void* h_in, const float* h32_in, const int32_t* ctx_host,
                            const int32_t* pt_host, const void* x_in, void* h_out, float* h32_out, void* y_out, int32_t* tok_out, int* via_out,
                            hipStream_t st) {
    emmax_model* m = s->m;
    const int R = s->op_rows, H = m->H;
    const size_t x4 = s->exact ? 4 : 2;   // bytes of an activation element the stages hand on
    if (h_in) HIPCHK(hipMemcpyAsync(s->dh, h_in, (size_t)R * H * 2, hipMemcpyDeviceToDevice, st));
    if (h32_in) HIPCHK(hipMemcpyAsync(s->dh32, h32_in, (size_t)R * H * 4, hipMemcpyDeviceToDevice, st));
    OpRows swap(s);
    HIPCHK(hipMemsetAsync(s->op_state, 0, (size_t)R * 8 * 4, st));
    KCHK(launch_set_ints(s->rows.max_new, R, 1 << 30, st));
    KCHK(launch_set_ints(s->rows.stop_after, R, -1, st));
    int r = 0;
    s->last_via = EMMAX_VIA_NONE;
    if (stage == STAGE_QKV) {
        HIPCHK(hipMemcpyAsync(s->rows.ctx_len, ctx_host, (size_t)B * 4, hipMemcpyHostToDevice, st));
        if (pt_host) HIPCHK(hipMemcpyAsync(s->page_table, pt_host, (size_t)B * s->max_pages * 4, hipMemcpyHostToDevice, st));
        r = run_decode_stage(s, B, layer, stage, st);
        if (pt_host) {   // the identity table again, whatever the launch did
            std::vector<int32_t> id((size_t)B * s->max_pages);
            for (size_t i = 0; i < id.size(); ++i) id[i] = (int32_t)i;
            HIPCHK(hipMemcpyAsync(s->page_table, id.data(), id.size() * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));   // (`id` is pageable host memory)
        }
        if (r == 0 && y_out) HIPCHK(hipMemcpyAsync(y_out, s->exact ? (void*)s->dq32 : (void*)s->dq, (size_t)B * m->q_dim * x4, hipMemcpyDeviceToDevice, st));
    } else if (stage == STAGE_OPROJ) {
        int ns = 1;
        const int form = decode_oproj_form(s->m, s->exact, B, &ns);
        if (form == 1) HIPCHK(hipMemcpyAsync(s->part, x_in, (size_t)B * m->cfg.n_heads * ns * EMMAX_PSTRIDE * 4, hipMemcpyDeviceToDevice, st));
        else if (form == 2) HIPCHK(hipMemcpyAsync(s->dq32, x_in, (size_t)B * m->q_dim * 4, hipMemcpyDeviceToDevice, st));
        else HIPCHK(hipMemcpyAsync(s->datt, x_in, (size_t)B * m->q_dim * 2, hipMemcpyDeviceToDevice, st));
        r = run_decode_stage(s, B, layer, stage, st);
    } else if (stage == STAGE_GATEUP) {
        r = run_decode_stage(s, B, layer, stage, st);
        if (r == 0 && y_out) HIPCHK(hipMemcpyAsync(y_out, s->exact ? (void*)s->dact32 : (void*)s->dact, (size_t)B * m->inter_p * x4, hipMemcpyDeviceToDevice, st));
    } else if (stage == STAGE_DOWN) {
        HIPCHK(hipMemcpyAsync(s->exact ? (void*)s->dact32 : (void*)s->dact, x_in, (size_t)B * m->inter_p * x4, hipMemcpyDeviceToDevice, st));
        r = run_decode_stage(s, B, layer, stage, st);
    } else {   // STAGE_LMHEAD: the logit rows and the greedy finish over the session's partial buffers, against the op's own per-row state
        r = run_lm_head_step(s, B, false, (float*)y_out, true, st, 0);
        if (r == 0 && tok_out) HIPCHK(hipMemcpyAsync(tok_out, s->rows.cur_tok, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
    }
    if (via_out) *via_out = s->last_via;
    if (r) return r;
    if (h_out) HIPCHK(hipMemcpyAsync(h_out, s->dh, (size_t)R * H * 2, hipMemcpyDeviceToDevice, st));
    if (h32_out) HIPCHK(hipMemcpyAsync(h32_out, s->dh32, (size_t)R * H * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int emmax_op_decode_stage(emmax_session* s, int layer, int stage, int B, const void* h_in, const float* h32_in, const int32_t* ctx_len_host,
                          const int32_t* page_table_host, const void* x_in, void* h_out, float* h32_out, void* y_out, int32_t* tok_out, int* via_out,
                          int* oproj_form_out, int* nsplit_out, emmax_stream stream) {
    if (!s) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: null session");
    emmax_model* m = s->m;
    if (stage != STAGE_QKV && stage != STAGE_OPROJ && stage != STAGE_GATEUP && stage != STAGE_DOWN && stage != STAGE_LMHEAD)
        return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: stage %d is not a projection stage (0 qkv, 2 o-proj, 3 gate/up, 4 down, 5 lm-head)", stage);
    if (B < 1 || B > s->op_rows) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: B %d outside 1..%d", B, s->op_rows);
    if (stage != STAGE_LMHEAD && (layer < 0 || layer >= m->cfg.n_layers))
        return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: layer %d outside 0..%d", layer, m->cfg.n_layers - 1);
    int ns = 1;
    const int form = decode_oproj_form(s->m, s->exact, B, &ns);
    if (oproj_form_out) *oproj_form_out = form;
    if (nsplit_out) *nsplit_out = ns;
    if (via_out) *via_out = EMMAX_VIA_NONE;
    if (stage == STAGE_OPROJ && !x_in && !h_in && !h32_in) return 0;   // the query form: which input the o-proj of B rows reads, nothing launched
    if (s->samp.on || s->proc.on || s->warp.on || s->rules.on || s->scores.on || s->beam.K || s->slots_open)
        return fail(EMMAX_ERR_STATE, "emmax_op_decode_stage: the session must be greedy (no sampling, processing, scores, beams or open slots)");
    if (!decode_batch_served(m, B, s->exact))   // (a prefill is held to it by the limit; this op is the one way past that)
        return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: steps of %d rows are served with one-split attention and an intermediate size above 4096 only (emmax_model_max_decode_batch)", B);
    if (B >= EMMAX_MFMA_MIN_BATCH && !m->aux_built)
        return fail(EMMAX_ERR_STATE, "%d rows decode on the fragment-major weight copies: call emmax_model_build_aux first", B);
    if (!h_in || (!h32_in && (s->exact || emmax_tune().resid32))) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: the hidden rows (bf16 and the fp32 stream) are required");
    if ((stage == STAGE_OPROJ || stage == STAGE_DOWN) && !x_in) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: the stage's input rows are required");
    if (stage == STAGE_LMHEAD && !y_out) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: the logit rows are required");
    if (stage == STAGE_QKV) {
        if (!ctx_len_host) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: ctx_len is required");
        for (int b = 0; b < B; ++b)
            if (ctx_len_host[b] < 0 || ctx_len_host[b] > s->max_ctx - 2)
                return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: ctx_len[%d] = %d outside 0..%d", b, ctx_len_host[b], s->max_ctx - 2);
        if (page_table_host) {   // together a permutation of the pages rows 0 .. B own
            const int n = B * s->max_pages;
            std::vector<char> seen((size_t)n, 0);
            for (int i = 0; i < n; ++i) {
                const int pg = page_table_host[i];
                if (pg < 0 || pg >= n || seen[pg]) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_stage: page_table is not a permutation of pages 0..%d (entry %d = %d)", n - 1, i, pg);
                seen[pg] = 1;
            }
        }
    }
    return decode_stage_run(s, layer, stage, B, h_in, h32_in, ctx_len_host, page_table_host, x_in, h_out, h32_out, y_out, tok_out, via_out, (hipStream_t)stream);
}

int emmax_op_decode_route(const emmax_model* m, int stage, int B, int exact, int* via_out) {
    if (!m) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_route: null model");
    if (stage != STAGE_QKV && stage != STAGE_OPROJ && stage != STAGE_GATEUP && stage != STAGE_DOWN && stage != STAGE_LMHEAD)
        return fail(EMMAX_ERR_INVALID, "emmax_op_decode_route: stage %d is not a projection stage (0 qkv, 2 o-proj, 3 gate/up, 4 down, 5 lm-head)", stage);
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_route: B %d outside 1..%d", B, EMMAX_MAX_DECODE_BATCH);
    const int via = decode_stage_route(m, stage, B, exact != 0);
    if (via_out) *via_out = via > 0 ? via : EMMAX_VIA_NONE;
    if (via > 0) return 0;
    return fail(EMMAX_ERR_INVALID, "emmax_op_decode_route: no launcher family takes the %s projection of this model at batch %d%s%s", decode_stage_name(stage), B,
                exact ? " in exact numerics" : "", via < 0 ? " (decode_km.hip refuses it and decode_mfma.hip's copy is only built with the tuning switch km = 0)" : "");
}

int emmax_op_decode_kv_read(emmax_session* s, int layer, int row, int p0, int n, const int32_t* page_row_host, int from_stage, float* k_out_host,
                            float* v_out_host, emmax_stream stream) {
    if (!s || !k_out_host || !v_out_host) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_kv_read: null argument");
    emmax_model* m = s->m;
    const int Hkv = m->cfg.n_kv_heads, hd = m->cfg.head_dim;
    if (layer < 0 || layer >= m->cfg.n_layers || row < 0 || row >= s->rows_total) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_kv_read: layer / row out of range");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (from_stage) {   // fp8 KV cache: the step's new rows as the qkv launch left them, bf16 [rows][Hkv][2][hd]
        if (!s->kv8) return fail(EMMAX_ERR_STATE, "emmax_op_decode_kv_read: the session has no kv_stage rows (tuning switch kv_fp8 at emmax_session_create)");
        std::vector<bf16> raw((size_t)Hkv * 2 * hd);
        HIPCHK(hipMemcpy(raw.data(), s->kv_stage + (size_t)row * Hkv * 2 * hd, raw.size() * 2, hipMemcpyDeviceToHost));
        for (int hk = 0; hk < Hkv; ++hk)
            for (int d = 0; d < hd; ++d) {
                k_out_host[hk * hd + d] = bits_to_float((uint32_t)raw[((size_t)hk * 2) * hd + d] << 16);
                v_out_host[hk * hd + d] = bits_to_float((uint32_t)raw[((size_t)hk * 2 + 1) * hd + d] << 16);
            }
        return 0;
    }
    if (n < 1 || p0 < 0 || p0 + n > s->max_ctx) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_kv_read: positions %d..%d outside 0..%d", p0, p0 + n - 1, s->max_ctx - 1);
    std::vector<int32_t> pt((size_t)s->max_pages);
    if (page_row_host) memcpy(pt.data(), page_row_host, pt.size() * 4);
    else HIPCHK(hipMemcpy(pt.data(), s->page_table + (size_t)row * s->max_pages, pt.size() * 4, hipMemcpyDeviceToHost));
    const int64_t n_pages = (int64_t)s->rows_total * s->max_pages;
    const int eb = kv_elem_bytes(s->kv_fmt);
    std::vector<uint8_t> raw((size_t)hd * 4), ext((size_t)hd);
    for (int i = 0; i < n; ++i) {
        const int pos = p0 + i, pg = pt[pos / PAGE];
        if (pg < 0 || pg >= n_pages) return fail(EMMAX_ERR_INVALID, "emmax_op_decode_kv_read: page id %d outside 0..%lld", pg, (long long)n_pages - 1);
        for (int hk = 0; hk < Hkv; ++hk) {
            const size_t rowi = ((size_t)pg * Hkv + hk) * PAGE + pos % PAGE;
            for (int is_v = 0; is_v < 2; ++is_v) {
                float* out = (is_v ? v_out_host : k_out_host) + ((size_t)i * Hkv + hk) * hd;
                const char* base = (const char*)(is_v ? vcache_of(s, layer) : kcache_of(s, layer));
                if (s->kv_fmt == KV_X24) {
                    HIPCHK(hipMemcpy(raw.data(), base + rowi * hd * 2, (size_t)hd * 2, hipMemcpyDeviceToHost));
                    HIPCHK(hipMemcpy(ext.data(), base + (size_t)s->kv24 * 2 + rowi * hd, (size_t)hd, hipMemcpyDeviceToHost));
                    for (int d = 0; d < hd; ++d) out[d] = bits_to_float(((uint32_t)((const uint16_t*)raw.data())[d] << 16) | ((uint32_t)ext[d] << 8));
                    continue;
                }
                HIPCHK(hipMemcpy(raw.data(), base + rowi * hd * eb, (size_t)hd * eb, hipMemcpyDeviceToHost));
                if (s->kv_fmt == KV_F32) {
                    memcpy(out, raw.data(), (size_t)hd * 4);
                } else if (s->kv_fmt == KV_FP8) {
                    float sc = 0.f;
                    HIPCHK(hipMemcpy(&sc, (is_v ? vscale_of(s, layer) : kscale_of(s, layer)) + rowi, 4, hipMemcpyDeviceToHost));
                    for (int d = 0; d < hd; ++d) out[d] = e4m3_to_float(raw[d]) * sc;
                } else {
                    for (int d = 0; d < hd; ++d) out[d] = bits_to_float((uint32_t)((const uint16_t*)raw.data())[d] << 16);
                }
            }
        }
    }
    return 0;
}

int emmax_op_gemv(const void* x, const void* W, void* y, int B, int N, int K, emmax_stream st) {
    GemvParams p = plain_gemv(x, W, y, N, K);
    if (decode_gemv_init() != 0) return fail(EMMAX_ERR_HIP, "could not raise the dynamic LDS limit of the GEMV kernels");
    int r = launch_decode_gemv(GEMV_PLAIN, p, B, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_gemv: unsupported shape (B<=8, K%%8)");
    return 0;
}

int emmax_op_resize_bicubic_u8(const uint8_t* src, int B, int H, int W, uint8_t* dst, int OH, int OW, uint8_t* tmp,
                               const int32_t* bounds_h, const int32_t* kk_h, int ksize_h, const int32_t* bounds_v, const int32_t* kk_v,
                               int ksize_v, emmax_stream st) {
    if (!src || !dst || B < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return fail(EMMAX_ERR_INVALID, "emmax_op_resize_bicubic_u8: bad argument");
    if ((W != OW && (!bounds_h || !kk_h)) || (H != OH && (!bounds_v || !kk_v)) || (W != OW && H != OH && !tmp))
        return fail(EMMAX_ERR_INVALID, "emmax_op_resize_bicubic_u8: missing tables / scratch");
    int r = launch_resize_bicubic_u8(src, B, H, W, dst, OH, OW, tmp, bounds_h, kk_h, ksize_h, bounds_v, kk_v, ksize_v, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_HIP, "emmax_op_resize_bicubic_u8: launch failed");
    return 0;
}
int emmax_op_quant_fm8(const void* W, int ld, void* W8, float* scales, int N, int K, emmax_stream st) {
    int r = launch_quant_fm8(W, ld, W8, scales, N, K, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_quant_fm8: N %% 16, K %% 64, ld %% 8 required");
    return 0;
}
int emmax_op_quant_rm8(const void* W, int ld, void* W8, float* scales, int N, int K, emmax_stream st) {
    int r = launch_quant_rm8(W, ld, W8, scales, N, K, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_quant_rm8: K %% 16, ld %% 8 required");
    return 0;
}
int emmax_op_quant_mxfp4(const void* W, int ld, void* tiles, void* scales, int N, int K, int perm, int perm_hd, emmax_stream st) {
    return op_quant_mx(PW_MX4, "emmax_op_quant_mxfp4", W, ld, tiles, scales, N, K, perm, perm_hd, st);
}
int emmax_op_dequant_mxfp4(const void* tiles, const void* scales, void* W, int ld, int N, int K, int perm, int perm_hd, emmax_stream st) {
    return op_dequant_mx(PW_MX4, "emmax_op_dequant_mxfp4", tiles, scales, W, ld, N, K, perm, perm_hd, st);
}
int emmax_op_gemm_small_mxfp4(const void* x, const void* tiles, const void* scales, void* y, int B, int N, int K, emmax_stream st) {
    return op_gemm_small_mx(PW_MX4, "emmax_op_gemm_small_mxfp4", x, tiles, scales, y, B, N, K, st);
}
int emmax_op_quant_mxfp6(const void* W, int ld, void* tiles, void* scales, int N, int K, int perm, int perm_hd, emmax_stream st) {
    return op_quant_mx(PW_MX6, "emmax_op_quant_mxfp6", W, ld, tiles, scales, N, K, perm, perm_hd, st);
}
int emmax_op_dequant_mxfp6(const void* tiles, const void* scales, void* W, int ld, int N, int K, int perm, int perm_hd, emmax_stream st) {
    return op_dequant_mx(PW_MX6, "emmax_op_dequant_mxfp6", tiles, scales, W, ld, N, K, perm, perm_hd, st);
}
int emmax_op_gemm_small_mxfp6(const void* x, const void* tiles, const void* scales, void* y, int B, int N, int K, emmax_stream st) {
    return op_gemm_small_mx(PW_MX6, "emmax_op_gemm_small_mxfp6", x, tiles, scales, y, B, N, K, st);
}
int emmax_op_gemm_wide_mxfp4(const void* x, const void* tiles, const void* scales, void* y, int B, int N, int K, emmax_stream st) {
    if (!x || !tiles || !scales || !y) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_wide_mxfp4: null argument");
    if (B < 17 || B > EMMAX_KMP_ROWS) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_wide_mxfp4: batch %d outside 17..%d", B, EMMAX_KMP_ROWS);
    GemvParams p = plain_gemv(x, tiles, y, N, K, PW_MX4, scales);
    // decode_kmp.hip's MX4 form as a pure op: the shape is wide by definition here (no model, no switch); its own check decides the rest
    ProjShape s = proj_shape(GEMV_PLAIN, p);
    s.mx4_wide = true;
    ProjGeom g;
    const bool ok = N >= 16 && N <= 32768 && K >= 128 && decode_kmp_takes(s, B, &g);
    const int r = ok ? launch_decode_kmp(GEMV_PLAIN, p, B, (hipStream_t)st, nullptr, &g) : -2;
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_gemm_wide_mxfp4: unsupported shape (N %% 16 and N <= 32768; K %% 128 and K >= 1024; K <= 4096, or K <= 11264 with N <= 4096)");
    return 0;
}
int emmax_op_gemv_fp8(const void* x, const void* W8, const float* scales, void* y, int B, int N, int K, emmax_stream st) {
    if (B < 1 || B > 2) return fail(EMMAX_ERR_INVALID, "emmax_op_gemv_fp8: batch must be 1..2");
    if (!scales) return fail(EMMAX_ERR_INVALID, "emmax_op_gemv_fp8: scales required");
    if (decode_gemv_init()) return fail(EMMAX_ERR_HIP, "emmax_op_gemv_fp8: init failed");
    GemvParams p = plain_gemv(x, W8, y, N, K, scales ? PW_FP8 : PW_BF16, scales);
    int r = launch_decode_gemv(GEMV_PLAIN, p, B, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_gemv_fp8: unsupported shape (K %% 16, B * K * 2 bytes of LDS)");
    return 0;
}
int emmax_op_gemm_small_fp8(const void* x, const void* W8, const float* scales, void* y, int B, int N, int K, emmax_stream st) {
    GemvParams p = plain_gemv(x, W8, y, N, K, scales ? PW_FP8 : PW_BF16, scales);
    if (!scales) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_small_fp8: scales required");
    int r;
    if (B <= 8) {   // decode_mfma.hip stages eight rows
        if (decode_mfma_init() != 0) return fail(EMMAX_ERR_HIP, "could not raise the dynamic LDS limit of the MFMA decode kernels");
        r = launch_decode_mfma(GEMV_PLAIN, p, B, (hipStream_t)st);
    } else if (K > 4096) {   // 9-32 rows: the K-split kernels (natural row order: the same e4m3 tiles); the phased down form is y = h + W x: h = 0
        HIPCHK(hipMemsetAsync(y, 0, (size_t)B * N * 2, (hipStream_t)st));
        r = launch_decode_km(GEMV_RESID, p, B, (hipStream_t)st);
    } else {
        r = launch_decode_km(GEMV_PLAIN, p, B, (hipStream_t)st);
    }
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_gemm_small_fp8: unsupported shape (N %% 16, K %% 64; 1 <= B <= 8; 9 <= B <= 32: the shapes of emmax_op_gemm_small_km)");
    return 0;
}
int emmax_op_repack_fm(const void* W, int ld, void* W_fm, int N, int K, emmax_stream st) {
    int r = launch_repack_fm(W, ld, W_fm, N, K, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_repack_fm: N %% 16, K %% 32, ld %% 8 required");
    return 0;
}
int emmax_op_repack_km(const void* W, int ld, void* W_km, int N, int K, int perm, int head_dim, emmax_stream st) {
    int r = launch_repack_km(W, ld, W_km, N, K, perm, head_dim, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_repack_km: N %% 16, K %% 32, ld %% 8 (perm 1: N %% head_dim, head_dim %% 16; perm 2: N %% 32) required");
    return 0;
}
int emmax_op_gemm_small_km(const void* x, const void* W_km, void* y, int B, int N, int K, emmax_stream st) {
    GemvParams p = plain_gemv(x, W_km, y, N, K);
    int r;
    if (K > 4096) {   // the phased kernel of the down projection (y = h + W x): h = 0
        HIPCHK(hipMemsetAsync(y, 0, (size_t)B * N * 2, (hipStream_t)st));
        r = launch_decode_km(GEMV_RESID, p, B, (hipStream_t)st);
    } else {
        r = launch_decode_km(GEMV_PLAIN, p, B, (hipStream_t)st);
    }
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_gemm_small_km: unsupported shape (1 <= B <= 32, N %% 16; K %% 256 and K <= 4096 and N <= 32768, or the phased form: K %% 32, K <= 11264 at B <= 8, 12288 at B <= 16; B > 16: K %% 32, K <= 11264, N <= 4096 there)");
    return 0;
}
int emmax_op_gemm_small(const void* x, const void* W_fm, void* y, int B, int N, int K, emmax_stream st) {
    GemvParams p = plain_gemv(x, W_fm, y, N, K);
    if (decode_mfma_init() != 0) return fail(EMMAX_ERR_HIP, "could not raise the dynamic LDS limit of the MFMA decode kernels");
    int r = launch_decode_mfma(GEMV_PLAIN, p, B, (hipStream_t)st);
    if (r) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_small: unsupported shape (1 <= B <= 8, N %% 16, K %% 32)");
    return 0;
}

// ---- the prefill's stage kernels one by one (ABI 12; tests/test_prefill_stages_gpu.py): pure ops, no session, no device allocation ----------
int emmax_op_gemm_stream(const void* A, int lda, const void* W, int ldw, float* C32, int ldc, const float* residual32, int ldr, int M, int N, int K,
                         const void* bias, int act, const void* scale, int n_store, int ksplit, void* ws, int64_t ws_bytes, const void* norm_w,
                         void* norm_out, int ld_norm, float eps, emmax_stream stream) {
    if (!A || !W || !C32) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: null argument");
    if (M < 1 || N < 1 || K < 1 || K % 64 || N % 128 || lda % 8 || ldw % 8 || lda < K || ldw < K)
        return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: M %d, N %d (%% 128), K %d (%% 64), lda %d / ldw %d (%% 8, >= K)", M, N, K, lda, ldw);
    if (act != 0 && act != 1) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: act %d (0 none, 1 GELU; SwiGLU has no fp32 stream form)", act);
    if (n_store < 1 || n_store > N || ldc < n_store) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: n_store %d outside 1..N or ldc %d < n_store", n_store, ldc);
    if (residual32 && ldr < n_store) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: ldr %d < n_store %d", ldr, n_store);
    if (((uintptr_t)C32 | (uintptr_t)residual32 | (uintptr_t)A | (uintptr_t)W) & 15)   // (the epilogues read and write 16 bytes wherever ld %% 4 == 0)
        return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: A, W and the fp32 rows must be 16-byte aligned");
    if (ksplit != 0 && (ksplit < 2 || ksplit > K / 64)) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: ksplit %d (0 = the launch plan, else 2..K / 64 = %d)", ksplit, K / 64);
    if (ws && (ws_bytes < 0 || ((uintptr_t)ws & 15))) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: the workspace must be 16-byte aligned");
    if (ksplit >= 2 && (!ws || (long long)ksplit * M * N * 4 > ws_bytes))
        return fail(EMMAX_ERR_NOMEM, "emmax_op_gemm_stream: %d slices need a workspace of %lld bytes (%lld given)", ksplit, (long long)ksplit * M * N * 4, (long long)(ws ? ws_bytes : 0));
    if ((norm_w == nullptr) != (norm_out == nullptr)) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: norm_w and norm_out go together");
    GemmParams p = gp(A, lda, W, ldw, C32, ldc, M, N, K);
    p.bias = bias; p.act = act; p.scale = scale; p.out_f32 = 1; p.res_f32 = 1; p.N_store = n_store;
    p.residual = residual32 ? residual32 : C32;   // (null: the stream is its own residual -- the prefill's aliased form)
    p.ldr = residual32 ? ldr : ldc;
    if (ws) { p.ws = (float*)ws; p.ws_bytes = ws_bytes; }
    if (norm_out) {
        p.norm_w = norm_w; p.norm_out = norm_out; p.ld_norm = ld_norm; p.norm_eps = eps;
        // the norm is never skipped: a path that cannot apply it in its reduce pass refuses the call
        if (ld_norm < N) return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: ld_norm %d < N %d", ld_norm, N);
        if (ksplit == 0 ? !gemm_fuses_norm(p) : !gemm_splitk_fuses_norm(p))
            return fail(EMMAX_ERR_INVALID, "emmax_op_gemm_stream: this path does not fuse the RMSNorm (act 0, N = 4096 whole rows, 16-byte aligned rows of ld %% 8, %s)",
                        ksplit == 0 ? "and a launch plan that splits K with the given workspace" : "explicit slices");
    }
    const int r = ksplit == 0 ? launch_gemm(p, (hipStream_t)stream) : launch_gemm_splitk(p, ksplit, (hipStream_t)stream, emmax_tune().gemm_sk_big > 0 ? 1 : 0);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_gemm_stream: unsupported shape or launch failure");
    return 0;
}
int emmax_op_rmsnorm_f32(const float* x, int ldx, void* y, int ldy, const void* w, int rows, int D, float eps, emmax_stream stream) {
    if (!x || !y || !w) return fail(EMMAX_ERR_INVALID, "emmax_op_rmsnorm_f32: null argument");
    if (rows < 1 || D < 8 || ldx < D || ldy < D || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w) & 15))
        return fail(EMMAX_ERR_INVALID, "emmax_op_rmsnorm_f32: rows %d, D %d, ldx %d / ldy %d (>= D), 16-byte aligned pointers", rows, D, ldx, ldy);
    const int r = launch_rmsnorm_f32(x, y, w, rows, D, ldx, ldy, eps, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_rmsnorm_f32: unsupported shape (D %% 8, D <= 8192, ldx %% 4, ldy %% 8)");
    return 0;
}
int emmax_op_rope_kv_write(void* qkv, int ld, int q_off, int k_off, int v_off, const int32_t* cu, int B, int total_rows, const float* cos_t, const float* sin_t,
                           void* kcache, void* vcache, const int32_t* page_table, int max_pages, int Hq, int Hkv, int head_dim, int page, emmax_stream stream) {
    if (!qkv || !cu || !cos_t || !sin_t || !page_table) return fail(EMMAX_ERR_INVALID, "emmax_op_rope_kv_write: null argument");
    if ((kcache == nullptr) != (vcache == nullptr)) return fail(EMMAX_ERR_INVALID, "emmax_op_rope_kv_write: kcache and vcache go together (both null: rotate only)");
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || total_rows < 1 || Hq < 1 || Hkv < 1 || page < 1 || max_pages < 1)
        return fail(EMMAX_ERR_INVALID, "emmax_op_rope_kv_write: B %d (1..%d), total_rows %d, heads %d / %d, page %d, max_pages %d", B, EMMAX_MAX_DECODE_BATCH, total_rows, Hq, Hkv, page, max_pages);
    // V moves in 16-byte pieces in both kernels: rows, offsets and heads in multiples of 8 elements
    if (head_dim < 8 || head_dim % 8 || (ld | q_off | k_off | v_off) % 8 || q_off < 0 || k_off < 0 || v_off < 0 || q_off + Hq * head_dim > ld || k_off + Hkv * head_dim > ld ||
        v_off + Hkv * head_dim > ld)
        return fail(EMMAX_ERR_INVALID, "emmax_op_rope_kv_write: head_dim %d, ld %d and the offsets %d / %d / %d in multiples of 8, the heads inside a row", head_dim, ld, q_off, k_off, v_off);
    if ((((uintptr_t)qkv | (uintptr_t)kcache | (uintptr_t)vcache) & 15) || (((uintptr_t)cos_t | (uintptr_t)sin_t | (uintptr_t)cu | (uintptr_t)page_table) & 3))
        return fail(EMMAX_ERR_INVALID, "emmax_op_rope_kv_write: qkv and the caches must be 16-byte aligned, the tables 4-byte aligned");
    const int r = launch_rope_kv_write(qkv, ld, q_off, k_off, v_off, cu, B, total_rows, cos_t, sin_t, kcache, vcache, page_table, max_pages, Hq, Hkv, head_dim, page,
                                       (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_rope_kv_write: launch failure");
    return 0;
}
int emmax_op_kv_quant_rows(void* qkv, int ld, int k_off, int v_off, const int32_t* cu, int B, int total_rows, void* k8, void* v8, float* kscale, float* vscale,
                           const int32_t* page_table, int max_pages, int Hkv, int head_dim, int page, emmax_stream stream) {
    if (!qkv || !cu || !k8 || !v8 || !kscale || !vscale || !page_table) return fail(EMMAX_ERR_INVALID, "emmax_op_kv_quant_rows: null argument");
    if (head_dim != 128) return fail(EMMAX_ERR_INVALID, "emmax_op_kv_quant_rows: head_dim %d (the fp8 KV cache holds rows of 128)", head_dim);
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || total_rows < 1 || Hkv < 1 || page < 1 || max_pages < 1)
        return fail(EMMAX_ERR_INVALID, "emmax_op_kv_quant_rows: B %d (1..%d), total_rows %d, Hkv %d, page %d, max_pages %d", B, EMMAX_MAX_DECODE_BATCH, total_rows, Hkv, page, max_pages);
    if ((ld | k_off | v_off) % 8 || k_off < 0 || v_off < 0 || k_off + Hkv * 128 > ld || v_off + Hkv * 128 > ld)
        return fail(EMMAX_ERR_INVALID, "emmax_op_kv_quant_rows: ld %d and the offsets %d / %d in multiples of 8, the heads inside a row", ld, k_off, v_off);
    if (((uintptr_t)qkv & 15) || (((uintptr_t)k8 | (uintptr_t)v8) & 7) || (((uintptr_t)kscale | (uintptr_t)vscale | (uintptr_t)cu | (uintptr_t)page_table) & 3))
        return fail(EMMAX_ERR_INVALID, "emmax_op_kv_quant_rows: qkv must be 16-byte aligned, the e4m3 pages 8-byte, scales and tables 4-byte");
    const int r = launch_kv_quant_rows(qkv, ld, k_off, v_off, cu, B, total_rows, k8, v8, kscale, vscale, page_table, max_pages, Hkv, head_dim, page, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_kv_quant_rows: launch failure");
    return 0;
}
int emmax_op_embed_splice(const int32_t* ids, int P_max, const int32_t* cu, const void* E, const void* patches, void* h, float* h32, int B, int max_seqlen,
                          int n_patches, int hidden, int vocab, emmax_stream stream) {
    if (!ids || !cu || !E || !h) return fail(EMMAX_ERR_INVALID, "emmax_op_embed_splice: null argument");
    if (n_patches < 0 || (n_patches > 0 && !patches)) return fail(EMMAX_ERR_INVALID, "emmax_op_embed_splice: n_patches %d needs the patch rows (0: text only)", n_patches);
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || P_max < 1 || max_seqlen < 1 || max_seqlen > n_patches + P_max || vocab < 1 || hidden < 8 || hidden % 8)
        return fail(EMMAX_ERR_INVALID, "emmax_op_embed_splice: B %d (1..%d), P_max %d, max_seqlen %d (1..n_patches + P_max), vocab %d, hidden %d (%% 8)", B, EMMAX_MAX_DECODE_BATCH, P_max,
                    max_seqlen, vocab, hidden);
    if ((((uintptr_t)E | (uintptr_t)patches | (uintptr_t)h | (uintptr_t)h32) & 15) || (((uintptr_t)ids | (uintptr_t)cu) & 3))
        return fail(EMMAX_ERR_INVALID, "emmax_op_embed_splice: rows must be 16-byte aligned, ids and cu 4-byte aligned");
    const int r = launch_embed_splice(ids, P_max, cu, E, patches, h, B, max_seqlen, n_patches, hidden, vocab, (hipStream_t)stream, h32);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_embed_splice: launch failure");
    return 0;
}
int emmax_op_gather_last_rows(const void* in, const float* in32, void* out, float* out32, const int32_t* cu, int B, int D, emmax_stream stream) {
    if ((!in && !in32) || !out || !cu) return fail(EMMAX_ERR_INVALID, "emmax_op_gather_last_rows: null argument (source rows as bf16 or as fp32, bf16 out, cu)");
    if (in && in32) return fail(EMMAX_ERR_INVALID, "emmax_op_gather_last_rows: one source, bf16 or fp32");
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || D < 8 || D % 8) return fail(EMMAX_ERR_INVALID, "emmax_op_gather_last_rows: B %d (1..%d), D %d (%% 8)", B, EMMAX_MAX_DECODE_BATCH, D);
    if ((((uintptr_t)in | (uintptr_t)in32 | (uintptr_t)out | (uintptr_t)out32) & 15) || ((uintptr_t)cu & 3))
        return fail(EMMAX_ERR_INVALID, "emmax_op_gather_last_rows: rows must be 16-byte aligned, cu 4-byte aligned");
    const int r = launch_gather_last_rows(in, out, cu, B, D, (hipStream_t)stream, out32, in32);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_gather_last_rows: launch failure");
    return 0;
}

// ---- the vision encode's glue kernels one by one (tests/test_vision_stages_gpu.py): pure ops, no session, no device allocation ----------------
// The launchers check almost nothing: each op refuses here what its kernel cannot do, and then nothing is launched.
int emmax_op_patch_gather(const void* src, void* out, int B, int img, int patch, int kpad, int chan0, const float* mean_host, const float* std_host,
                          int from_u8, int hl, emmax_stream stream) {
    if (!src || !out || !mean_host || !std_host) return fail(EMMAX_ERR_INVALID, "emmax_op_patch_gather: null argument");
    if (B < 1 || img < 1 || patch < 1 || img % patch) return fail(EMMAX_ERR_INVALID, "emmax_op_patch_gather: B %d, img %d, patch %d (img %% patch == 0)", B, img, patch);
    if (kpad < 3 * patch * patch) return fail(EMMAX_ERR_INVALID, "emmax_op_patch_gather: kpad %d below 3 patch^2 = %d", kpad, 3 * patch * patch);
    if (hl && kpad % 64) return fail(EMMAX_ERR_INVALID, "emmax_op_patch_gather: the HL form holds 64 hi and 64 lo per 64 elements: kpad %d %% 64", kpad);
    if (!from_u8 && chan0 != 0 && chan0 != 3) return fail(EMMAX_ERR_INVALID, "emmax_op_patch_gather: chan0 %d (a tower's three of six pixel channels: 0 or 3)", chan0);
    if (((uintptr_t)out & 1) || (!from_u8 && ((uintptr_t)src & 1))) return fail(EMMAX_ERR_INVALID, "emmax_op_patch_gather: bf16 rows must be 2-byte aligned");
    const int r = hl ? launch_x_patch_gather(from_u8 != 0, src, out, B, img, patch, kpad, chan0, mean_host, std_host, (hipStream_t)stream)
                     : launch_patch_gather(from_u8 != 0, src, out, B, img, patch, kpad, chan0, mean_host, std_host, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_patch_gather: launch failure");
    return 0;
}
int emmax_op_assemble_tokens(const void* pe, const void* pos, const void* cls, const void* reg, void* tokens, int B, int n_patches, int has_cls, int n_reg,
                             int D, int ld, int f32, emmax_stream stream) {
    if (!pe || !pos || !tokens) return fail(EMMAX_ERR_INVALID, "emmax_op_assemble_tokens: null argument");
    if (has_cls != 0 && has_cls != 1) return fail(EMMAX_ERR_INVALID, "emmax_op_assemble_tokens: has_cls %d (0 or 1)", has_cls);
    if ((has_cls && !cls) || (n_reg > 0 && !reg)) return fail(EMMAX_ERR_INVALID, "emmax_op_assemble_tokens: the cls row / the %d register rows are required", n_reg);
    if (B < 1 || n_patches < 1 || n_reg < 0 || D < 1 || ld < D) return fail(EMMAX_ERR_INVALID, "emmax_op_assemble_tokens: B %d, n_patches %d, n_reg %d, D %d, ld %d (>= D)", B, n_patches, n_reg, D, ld);
    if (((uintptr_t)pe | (uintptr_t)tokens) & (f32 ? 3 : 1)) return fail(EMMAX_ERR_INVALID, "emmax_op_assemble_tokens: misaligned rows");
    const int r = f32 ? launch_x_assemble_tokens((const float*)pe, pos, cls, reg, (float*)tokens, B, n_patches, has_cls + n_reg, has_cls, D, ld, (hipStream_t)stream)
                      : launch_assemble_tokens(pe, pos, cls, reg, tokens, B, n_patches, has_cls + n_reg, has_cls, D, ld, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_assemble_tokens: launch failure");
    return 0;
}
int emmax_op_copy_rows(const void* in, int ld_in, void* out, int B, int rows_in, int r_off, int rows_out, int D, int ld_out, int col_off, emmax_stream stream) {
    if (!in || !out) return fail(EMMAX_ERR_INVALID, "emmax_op_copy_rows: null argument");
    if (B < 1 || rows_in < 1 || rows_out < 1 || r_off < 0 || r_off + rows_out > rows_in)
        return fail(EMMAX_ERR_INVALID, "emmax_op_copy_rows: B %d, rows %d..%d of %d", B, r_off, r_off + rows_out - 1, rows_in);
    if (D < 8 || (D | ld_in | ld_out | col_off) % 8 || col_off < 0 || ld_in < D || col_off + D > ld_out)
        return fail(EMMAX_ERR_INVALID, "emmax_op_copy_rows: D %d, ld_in %d, ld_out %d, col_off %d in multiples of 8 (16-byte moves), D <= ld_in, col_off + D <= ld_out", D, ld_in,
                    ld_out, col_off);
    if (((uintptr_t)in | (uintptr_t)out) & 15) return fail(EMMAX_ERR_INVALID, "emmax_op_copy_rows: rows must be 16-byte aligned");
    const int r = launch_copy_rows(in, ld_in, out, B, rows_in, r_off, rows_out, D, ld_out, col_off, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_copy_rows: launch failure");
    return 0;
}
int emmax_op_row_stats(const void* x, int ldx, float* stats, int rows, int D, float eps, emmax_stream stream) {
    if (!x || !stats) return fail(EMMAX_ERR_INVALID, "emmax_op_row_stats: null argument");
    if (rows < 1 || D < 8 || D % 8 || D > 8192 || ldx % 8 || ldx < D)
        return fail(EMMAX_ERR_INVALID, "emmax_op_row_stats: rows %d, D %d (%% 8, <= 8192), ldx %d (%% 8, >= D)", rows, D, ldx);
    if (((uintptr_t)x & 15) || ((uintptr_t)stats & 7)) return fail(EMMAX_ERR_INVALID, "emmax_op_row_stats: x must be 16-byte aligned, the (mean, rstd) pairs 8-byte");
    const int r = launch_row_stats(x, stats, rows, D, ldx, eps, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_row_stats: launch failure");
    return 0;
}
int emmax_op_ln_fold(void* W, int ldw, int N, int K, const void* gamma, const void* beta, const void* bias, float* ln_s, float* ln_c, emmax_stream stream) {
    if (!W || !gamma || !ln_s || !ln_c) return fail(EMMAX_ERR_INVALID, "emmax_op_ln_fold: null argument (beta and bias may be null)");
    if (N < 1 || K < 1 || ldw < K) return fail(EMMAX_ERR_INVALID, "emmax_op_ln_fold: N %d, K %d, ldw %d (>= K)", N, K, ldw);
    if (((uintptr_t)W | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)bias) & 1 || (((uintptr_t)ln_s | (uintptr_t)ln_c) & 3))
        return fail(EMMAX_ERR_INVALID, "emmax_op_ln_fold: misaligned argument");
    const int r = launch_ln_fold(W, ldw, N, K, gamma, beta, bias, ln_s, ln_c, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_ln_fold: launch failure");
    return 0;
}
int emmax_op_x_to_bf16(const float* x, int ldx, void* y, int ldy, int rows, int D, emmax_stream stream) {
    if (!x || !y) return fail(EMMAX_ERR_INVALID, "emmax_op_x_to_bf16: null argument");
    if (rows < 1 || D < 8 || (D | ldx | ldy) % 8 || ldx < D || ldy < D)
        return fail(EMMAX_ERR_INVALID, "emmax_op_x_to_bf16: rows %d, D %d, ldx %d, ldy %d in multiples of 8, pitches >= D", rows, D, ldx, ldy);
    if (((uintptr_t)x | (uintptr_t)y) & 15) return fail(EMMAX_ERR_INVALID, "emmax_op_x_to_bf16: rows must be 16-byte aligned");
    const int r = launch_x_to_bf16(x, ldx, y, ldy, rows, D, (hipStream_t)stream);
    if (r) return fail(r == -4 ? EMMAX_ERR_HIP : EMMAX_ERR_INVALID, "emmax_op_x_to_bf16: launch failure");
    return 0;
}


}  // extern "C"
