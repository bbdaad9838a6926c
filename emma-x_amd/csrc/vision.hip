// vision.hip -- the vision encode: the two ViT towers (on two streams at small batches) and the projector, in bf16 and in exact numerics;
// the GEMM parameter helpers every GEMM stage uses (session.h); emmax_vision_*.
#include "session.h"

GemmParams gp(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.N_store = N;
    return p;
}

// GEMM parameters of a session stage: as gp(), plus the session's split-K scratch
GemmParams gps(emmax_session* s, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K) {
    GemmParams p = gp(A, lda, W, ldw, C, ldc, M, N, K);
    p.ws = s->splitk_ws;
    p.ws_bytes = s->splitk_bytes;
    return p;
}

// one tower's scratch (run_vision): set 0 = the session's shared buffers (either tower, any batch), set 1 = tower 1's own (two-stream form)
struct VisScratch {
    bf16 *vA, *vpe, *vtok, *vln, *vqkv, *vatt, *vmlp;
    float *vstats, *ws;
    int64_t ws_bytes;
};

// One stage of the bf16 encode of tower t over scratch v.  run_tower strings them together, and emmax_op_vision_stage runs one on its own
// (tests/test_vision_stages_gpu.py): the same code either way.  VS_EMBED / VS_FEATURES ignore `i`; the block stages read T.blk[i].
enum { VS_EMBED = EMMAX_VSTAGE_EMBED, VS_QKV = EMMAX_VSTAGE_QKV, VS_ATTN = EMMAX_VSTAGE_ATTN, VS_PROJ = EMMAX_VSTAGE_PROJ, VS_FC1 = EMMAX_VSTAGE_FC1,
       VS_FC2 = EMMAX_VSTAGE_FC2, VS_FEATURES = EMMAX_VSTAGE_FEATURES, VS_PJ1 = EMMAX_VSTAGE_PJ1, VS_PJ2 = EMMAX_VSTAGE_PJ2, VS_PJ3 = EMMAX_VSTAGE_PJ3,
       VS_EMBED_PIXELS = EMMAX_VSTAGE_EMBED_PIXELS };

static int tower_stage(emmax_session* s, int t, const VisScratch& v, int i, int stage, bool from_u8, const void* src, int B, int col_off, hipStream_t st) {
    emmax_model* m = s->m;
    const TowerW& T = m->tw[t];
    const emmax_tower_config& tc = m->cfg.tower[t];
    const int np = m->tw[0].n_patches, rows = B * T.N;
    auto gpv = [&](const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K) {
        GemmParams p = gp(A, lda, W, ldw, C, ldc, M, N, K);
        p.ws = v.ws;
        p.ws_bytes = v.ws_bytes;
        return p;
    };
    GemmParams g;
    if (stage == VS_EMBED) {
        KCHK(launch_patch_gather(from_u8, src, v.vA, B, tc.image_size, tc.patch, T.Kpe, 3 * t, tc.mean, tc.std, st));
        g = gpv(v.vA, T.Kpe, T.patch_w, T.Kpe, v.vpe, T.Dp, B * np, T.Dp, T.Kpe);
        g.bias = T.patch_b;
        KCHK(launch_gemm(g, st));
        KCHK(launch_assemble_tokens(v.vpe, T.pos, T.cls, T.reg, v.vtok, B, np, T.n_prefix, tc.has_cls, T.D, T.Dp, st));
        return 0;
    }
    if (stage == VS_FEATURES) {
        // drop prefix tokens, no final norm, concat along the feature axis (modeling_prismatic.py:120-123)
        KCHK(launch_copy_rows(v.vtok, T.Dp, s->feats, B, T.N, T.n_prefix, np, T.D, m->Vp, col_off, st));
        return 0;
    }
    const BlockW& k = T.blk[i];
    if (stage == VS_QKV) {
        // LayerNorm folded into the projection: only the row statistics are computed here, the GEMM reads the raw rows and
        // its epilogue finishes the algebra (kernels.h) -- no normalised copy of the tokens is ever written or re-read
        if (m->ln_folded) {
            KCHK(launch_row_stats(v.vtok, v.vstats, rows, T.D, T.Dp, tc.ln_eps, st));
            g = gpv(v.vtok, T.Dp, k.qkv_w, T.Dp, v.vqkv, T.D3p, rows, T.D3p, T.Dp);
            g.ln_stats = v.vstats; g.ln_s = k.ln1_s; g.ln_c = k.ln1_c;
        } else {
            KCHK(launch_layernorm(v.vtok, v.vln, k.n1w, k.n1b, rows, T.D, T.Dp, T.Dp, tc.ln_eps, st));
            g = gpv(v.vln, T.Dp, k.qkv_w, T.Dp, v.vqkv, T.D3p, rows, T.D3p, T.Dp);
            g.bias = k.qkv_b;
        }
        KCHK(launch_gemm(g, st));
    } else if (stage == VS_ATTN) {
        AttnParams a;
        a.qkv = v.vqkv; a.out = v.vatt; a.cu_seqlens = s->cu_vit[t];
        a.ld_qkv = T.D3p; a.q_off = 0; a.k_off = T.D; a.v_off = 2 * T.D; a.ld_out = T.Dp;
        a.B = B; a.max_seqlen = T.N; a.Hq = tc.num_heads; a.Hkv = tc.num_heads;
        a.scale = 1.0f / sqrtf((float)T.hd); a.causal = 0;
        KCHK(launch_attention(a, T.hd, st));
    } else if (stage == VS_PROJ) {
        g = gpv(v.vatt, T.Dp, k.proj_w, T.Dp, v.vtok, T.Dp, rows, T.Dp, T.Dp);
        g.bias = k.proj_b; g.scale = tc.layerscale ? k.ls1 : nullptr; g.residual = v.vtok; g.ldr = T.Dp;
        KCHK(launch_gemm(g, st));
    } else if (stage == VS_FC1) {
        if (m->ln_folded) {
            KCHK(launch_row_stats(v.vtok, v.vstats, rows, T.D, T.Dp, tc.ln_eps, st));
            g = gpv(v.vtok, T.Dp, k.fc1_w, T.Dp, v.vmlp, T.Mp, rows, T.Mp, T.Dp);
            g.ln_stats = v.vstats; g.ln_s = k.ln2_s; g.ln_c = k.ln2_c;
        } else {
            KCHK(launch_layernorm(v.vtok, v.vln, k.n2w, k.n2b, rows, T.D, T.Dp, T.Dp, tc.ln_eps, st));
            g = gpv(v.vln, T.Dp, k.fc1_w, T.Dp, v.vmlp, T.Mp, rows, T.Mp, T.Dp);
            g.bias = k.fc1_b;
        }
        g.act = 1;
        KCHK(launch_gemm(g, st));
    } else {   // VS_FC2
        g = gpv(v.vmlp, T.Mp, k.fc2_w, T.Mp, v.vtok, T.Dp, rows, T.Dp, T.Mp);
        g.bias = k.fc2_b; g.scale = tc.layerscale ? k.ls2 : nullptr; g.residual = v.vtok; g.ldr = T.Dp;
        KCHK(launch_gemm(g, st));
    }
    return 0;
}

// the projector behind the concatenated features: pj1 and pj2 with GELU, pj3 plain
static int projector_stage(emmax_session* s, int stage, int B, hipStream_t st) {
    emmax_model* m = s->m;
    const int R = B * m->tw[0].n_patches;
    GemmParams g;
    if (stage == VS_PJ1) {
        g = gps(s, s->feats, m->Vp, m->pj1_w, m->Vp, s->pj1, m->P1p, R, m->P1p, m->Vp);
        g.bias = m->pj1_b; g.act = 1;
    } else if (stage == VS_PJ2) {
        g = gps(s, s->pj1, m->P1p, m->pj2_w, m->P1p, s->pj2, m->H, R, m->H, m->P1p);
        g.bias = m->pj2_b; g.act = 1;
    } else {
        g = gps(s, s->pj2, m->H, m->pj3_w, m->H, s->patch_embeds, m->H, R, m->H, m->H);
        g.bias = m->pj3_b;
    }
    KCHK(launch_gemm(g, st));
    return 0;
}

// blocks [i0, i1) of tower t; i0 == 0: the patch embedding in front of them, i1 == n_blocks: the feature copy behind them
static int run_tower(emmax_session* s, int t, const VisScratch& v, bool from_u8, const void* src, int B, int col_off, hipStream_t st, int i0 = 0,
                     int i1 = 1 << 30) {
    const int nb = s->m->tw[t].n_blocks;
    i1 = std::min(i1, nb);
    if (i0 == 0)
        if (int r = tower_stage(s, t, v, 0, VS_EMBED, from_u8, src, B, col_off, st)) return r;
    for (int i = i0; i < i1; ++i)
        for (int stage = VS_QKV; stage <= VS_FC2; ++stage)
            if (int r = tower_stage(s, t, v, i, stage, from_u8, src, B, col_off, st)) return r;
    if (i1 == nb)
        if (int r = tower_stage(s, t, v, 0, VS_FEATURES, from_u8, src, B, col_off, st)) return r;
    return 0;
}

// ---- exact numerics (tuning switch exact; exact.hip): the same stages on fp32 activations --------------------------------------------
// C[M, N] f32 = A (HL rows, K real columns padded to Kp) . W^T: both bf16 terms of A through the bf16 MFMAs (GemmParams::a_hl)
GemmParams gpx(emmax_session* s, const void* A_hl, int Kp, const void* W, int ldw, float* C, int ldc, int M, int N) {
    GemmParams p = gps(s, A_hl, 2 * Kp, W, ldw, C, ldc, M, N, 2 * Kp);
    p.a_hl = 1;
    p.out_f32 = 1;
    return p;
}

static int run_tower_x(emmax_session* s, int t, bool from_u8, const void* src, int B, int col_off, hipStream_t st) {
    emmax_model* m = s->m;
    const TowerW& T = m->tw[t];
    const emmax_tower_config& tc = m->cfg.tower[t];
    const int np = m->tw[0].n_patches, rows = B * T.N;
    KCHK(launch_x_patch_gather(from_u8, src, s->xhla, B, tc.image_size, tc.patch, T.Kpe, 3 * t, tc.mean, tc.std, st));
    GemmParams g = gpx(s, s->xhla, T.Kpe, T.patch_w, T.Kpe, s->x32a, T.Dp, B * np, T.Dp);
    g.bias = T.patch_b;
    KCHK(launch_gemm(g, st));
    KCHK(launch_x_assemble_tokens(s->x32a, T.pos, T.cls, T.reg, s->xtok32, B, np, T.n_prefix, tc.has_cls, T.D, T.Dp, st));
    if (T.Dp != T.D) HIPCHK(hipMemsetAsync(s->xhlb, 0, (size_t)rows * 2 * T.Dp * 2, st));   // the attention writes the real columns only
    auto into_tokens = [&](GemmParams& q, const void* bias, const void* ls) {   // tokens += LayerScale . (A W^T + bias), fp32 rows
        q.C = s->xtok32; q.ldc = T.Dp; q.bias = bias; q.scale = tc.layerscale ? ls : nullptr;
        q.residual = s->xtok32; q.res_f32 = 1; q.ldr = T.Dp;
    };
    for (int i = 0; i < T.n_blocks; ++i) {
        const BlockW& k = T.blk[i];
        KCHK(launch_x_layernorm(s->xtok32, s->xhla, k.n1w, k.n1b, rows, T.D, T.Dp, T.Dp, 2 * T.Dp, tc.ln_eps, st));
        g = gpx(s, s->xhla, T.Dp, k.qkv_w, T.Dp, s->x32a, T.D3p, rows, T.D3p);
        g.bias = k.qkv_b;
        KCHK(launch_gemm(g, st));
        AttnParams a;
        a.qkv = s->x32a; a.out = s->xhlb; a.cu_seqlens = s->cu_vit[t];
        a.ld_qkv = T.D3p; a.q_off = 0; a.k_off = T.D; a.v_off = 2 * T.D; a.ld_out = 2 * T.Dp;
        a.B = B; a.max_seqlen = T.N; a.Hq = tc.num_heads; a.Hkv = tc.num_heads;
        a.scale = 1.0f / sqrtf((float)T.hd); a.causal = 0;
        KCHK(launch_x_attention(a, T.hd, st));
        g = gpx(s, s->xhlb, T.Dp, k.proj_w, T.Dp, nullptr, 0, rows, T.Dp);
        into_tokens(g, k.proj_b, k.ls1);
        KCHK(launch_gemm(g, st));
        KCHK(launch_x_layernorm(s->xtok32, s->xhla, k.n2w, k.n2b, rows, T.D, T.Dp, T.Dp, 2 * T.Dp, tc.ln_eps, st));
        g = gpx(s, s->xhla, T.Dp, k.fc1_w, T.Dp, s->x32a, T.Mp, rows, T.Mp);
        g.bias = k.fc1_b; g.act = 1;
        KCHK(launch_gemm(g, st));
        KCHK(launch_x_split_rows(s->x32a, s->xhlb, rows, T.Mp, T.Mp, T.Mp, 2 * T.Mp, st));
        g = gpx(s, s->xhlb, T.Mp, k.fc2_w, T.Mp, nullptr, 0, rows, T.Dp);
        into_tokens(g, k.fc2_b, k.ls2);
        KCHK(launch_gemm(g, st));
    }
    // drop prefix tokens, no final norm, concat along the feature axis (modeling_prismatic.py:120-123): fp32 rows
    for (int b = 0; b < B; ++b)
        HIPCHK(hipMemcpy2DAsync(s->xfeats32 + (size_t)b * np * m->Vp + col_off, (size_t)m->Vp * 4, s->xtok32 + ((size_t)b * T.N + T.n_prefix) * T.Dp,
                                (size_t)T.Dp * 4, (size_t)T.D * 4, np, hipMemcpyDeviceToDevice, st));
    return 0;
}

static int run_vision_x(emmax_session* s, bool from_u8, const void* src, int B, void* out, hipStream_t st) {
    emmax_model* m = s->m;
    const int np = m->tw[0].n_patches, R = B * np;
    if (m->ln_folded) return fail(EMMAX_ERR_STATE, "exact numerics: the model was finalized with folded LayerNorms (set exact = 1 before emmax_model_finalize)");
    int col_off = 0;
    for (int t = 0; t < 2; ++t) {
        if (int r = run_tower_x(s, t, from_u8, src, B, col_off, st)) return r;
        col_off += m->tw[t].D;
    }
    KCHK(launch_x_split_rows(s->xfeats32, s->xhla, R, m->Vp, m->Vp, m->Vp, 2 * m->Vp, st));
    GemmParams g = gpx(s, s->xhla, m->Vp, m->pj1_w, m->Vp, s->x32a, m->P1p, R, m->P1p);
    g.bias = m->pj1_b; g.act = 1;
    KCHK(launch_gemm(g, st));
    KCHK(launch_x_split_rows(s->x32a, s->xhlb, R, m->P1p, m->P1p, m->P1p, 2 * m->P1p, st));
    g = gpx(s, s->xhlb, m->P1p, m->pj2_w, m->P1p, s->x32a, m->H, R, m->H);
    g.bias = m->pj2_b; g.act = 1;
    KCHK(launch_gemm(g, st));
    KCHK(launch_x_split_rows(s->x32a, s->xhla, R, m->H, m->H, m->H, 2 * m->H, st));
    g = gpx(s, s->xhla, m->H, m->pj3_w, m->H, s->xpe32, m->H, R, m->H);
    g.bias = m->pj3_b;
    KCHK(launch_gemm(g, st));
    // an exact session exchanges patch embeddings as FP32 rows [B, n_patches, hidden] (include/emmax.h): the caller's copy, if it wants one
    if (out && out != (void*)s->xpe32) HIPCHK(hipMemcpyAsync(out, s->xpe32, (size_t)R * m->H * 4, hipMemcpyDeviceToDevice, st));
    s->vision_B = B;
    return 0;
}

static int run_vision(emmax_session* s, bool from_u8, const void* src, int B, void* out, hipStream_t st) {
    emmax_model* m = s->m;
    if (!m->finalized) return fail(EMMAX_ERR_STATE, "model not finalized");
    if (B <= 0 || B > s->max_batch) return fail(EMMAX_ERR_INVALID, "vision batch %d outside 1..%d", B, s->max_batch);
    if (s->exact) return run_vision_x(s, from_u8, src, B, out, st);
    const int np = m->tw[0].n_patches;
    const VisScratch v0 = {s->vA, s->vpe, s->vtok, s->vln, s->vqkv, s->vatt, s->vmlp, s->vstats, s->splitk_ws, s->splitk_bytes};
    // Two streams (round 5; tuning switch vis_streams: 1 = on, the default; 0 = one stream): the towers share nothing but the frames and write
    // disjoint columns of `feats`; at one frame each is a chain of ~180 under-filled, launch-latency-bound kernels, and side by side they take
    // the time of the longer chain -- 5.01 -> 3.14 ms at one frame, 7.03 -> 5.36 at 8, 16.6 -> 13.9 at 32, 54.4 -> 52.5 at 128, 106.0 -> 104.8
    // at 256 (one tower's tile tails and launch ramps under the other's kernels; profiles/r05_vision_two_streams.txt).  Identical results:
    // same kernels, same plans (tower 1 has a split-K scratch of the session's size).
    const int vsw = emmax_tune().vis_streams;
    const bool two = s->vis_stream && B <= s->vis2_B && vsw != 0;
    if (two) {
        const VisScratch v1 = {s->v2A, s->v2pe, s->v2tok, s->v2ln, s->v2qkv, s->v2att, s->v2mlp, s->v2stats, s->v2splitk_ws, s->v2splitk_bytes};
        HIPCHK(hipEventRecord(s->ev_vfork, st));
        HIPCHK(hipStreamWaitEvent(s->vis_stream, s->ev_vfork, 0));
        // the launches of the two chains ENQUEUED alternately, block by block: one host thread feeds both streams, and with tower 1's ~180
        // launches enqueued first tower 0 started ~0.6 ms late at one frame
        int r = 0;
        const int nb = std::max(m->tw[0].n_blocks, m->tw[1].n_blocks);
        for (int i = 0; i < nb && r == 0; ++i) {
            if (i < m->tw[1].n_blocks) r = run_tower(s, 1, v1, from_u8, src, B, m->tw[0].D, s->vis_stream, i, i + 1);
            if (r == 0 && i < m->tw[0].n_blocks) r = run_tower(s, 0, v0, from_u8, src, B, 0, st, i, i + 1);
        }
        // (joined even on an error: the caller's stream must not run ahead of work queued on ours)
        HIPCHK(hipEventRecord(s->ev_vjoin, s->vis_stream));
        HIPCHK(hipStreamWaitEvent(st, s->ev_vjoin, 0));
        if (r) return r;
    } else {
        int col_off = 0;
        for (int t = 0; t < 2; ++t) {
            if (int r = run_tower(s, t, v0, from_u8, src, B, col_off, st)) return r;
            col_off += m->tw[t].D;
        }
    }
    for (int stage = VS_PJ1; stage <= VS_PJ3; ++stage)
        if (int r = projector_stage(s, stage, B, st)) return r;
    if (out && out != s->patch_embeds)
        HIPCHK(hipMemcpyAsync(out, s->patch_embeds, (size_t)B * np * m->H * 2, hipMemcpyDeviceToDevice, st));
    s->vision_B = B;
    return 0;
}

extern "C" {

int emmax_vision_encode(emmax_session* s, const uint8_t* frames, int B, void* out, emmax_stream st) {
    if (!s || !frames) return fail(EMMAX_ERR_INVALID, "null argument");
    return run_vision(s, true, frames, B, out, (hipStream_t)st);
}
int emmax_vision_encode_pixels(emmax_session* s, const void* px, int B, void* out, emmax_stream st) {
    if (!s || !px) return fail(EMMAX_ERR_INVALID, "null argument");
    return run_vision(s, false, px, B, out, (hipStream_t)st);
}
int emmax_vision_features(emmax_session* s, int B, void* out, emmax_stream st) {
    if (!s || !out) return fail(EMMAX_ERR_INVALID, "null argument");
    if (B != s->vision_B) return fail(EMMAX_ERR_STATE, "no vision result for batch %d", B);
    emmax_model* m = s->m;
    if (s->exact) {   // the fp32 features, rounded for the caller
        KCHK(launch_x_to_bf16(s->xfeats32, m->Vp, out, m->V, B * m->tw[0].n_patches, m->V, (hipStream_t)st));
        return 0;
    }
    HIPCHK(hipMemcpy2DAsync(out, (size_t)m->V * 2, s->feats, (size_t)m->Vp * 2, (size_t)m->V * 2, (size_t)B * m->tw[0].n_patches,
                            hipMemcpyDeviceToDevice, (hipStream_t)st));
    return 0;
}

// ---- one stage of the bf16 encode through tower_stage / projector_stage (tests/test_vision_stages_gpu.py) -----------------------------------
// packed rows [rows, w] <-> the session's rows of pitch ld; the padding columns w .. ld keep whatever the session holds there
static int rows_in(bf16* dst, int ld, const void* src, int rows, int w, hipStream_t st) {
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)ld * 2, src, (size_t)w * 2, (size_t)w * 2, rows, hipMemcpyDeviceToDevice, st));
    return 0;
}
static int rows_out(void* dst, const bf16* src, int ld, int rows, int w, hipStream_t st) {
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)w * 2, src, (size_t)ld * 2, (size_t)w * 2, rows, hipMemcpyDeviceToDevice, st));
    return 0;
}

int emmax_op_vision_stage(emmax_session* s, int tower, int block, int stage, int B, const void* in, const void* tok_in, void* out, emmax_stream stream) {
    if (!s || !in || !out) return fail(EMMAX_ERR_INVALID, "emmax_op_vision_stage: null argument");
    emmax_model* m = s->m;
    if (!m->finalized) return fail(EMMAX_ERR_STATE, "model not finalized");
    if (s->exact) return fail(EMMAX_ERR_STATE, "emmax_op_vision_stage: an exact-numerics session runs other kernels (tests/test_exact_gpu.py holds them)");
    if (stage < VS_EMBED || stage > VS_EMBED_PIXELS) return fail(EMMAX_ERR_INVALID, "emmax_op_vision_stage: stage %d outside 0..%d", stage, VS_EMBED_PIXELS);
    if (B < 1 || B > s->max_batch) return fail(EMMAX_ERR_INVALID, "emmax_op_vision_stage: B %d outside 1..%d", B, s->max_batch);
    hipStream_t st = (hipStream_t)stream;
    const int np = m->tw[0].n_patches, R = B * np;
    s->vision_B = 0;   // the scratch of the last encode is overwritten: emmax_vision_features has nothing to hand out
    if (stage >= VS_PJ1 && stage <= VS_PJ3) {
        if (stage == VS_PJ1) { if (int r = rows_in(s->feats, m->Vp, in, R, m->V, st)) return r; }
        else if (stage == VS_PJ2) { if (int r = rows_in(s->pj1, m->P1p, in, R, m->P1, st)) return r; }
        else if (int r = rows_in(s->pj2, m->H, in, R, m->H, st)) return r;
        if (int r = projector_stage(s, stage, B, st)) return r;
        if (stage == VS_PJ1) return rows_out(out, s->pj1, m->P1p, R, m->P1, st);
        return rows_out(out, stage == VS_PJ2 ? s->pj2 : s->patch_embeds, m->H, R, m->H, st);
    }
    if (tower < 0 || tower > 1) return fail(EMMAX_ERR_INVALID, "emmax_op_vision_stage: tower %d outside 0..1", tower);
    const TowerW& T = m->tw[tower];
    const bool per_block = stage >= VS_QKV && stage <= VS_FC2;
    if (per_block && (block < 0 || block >= T.n_blocks)) return fail(EMMAX_ERR_INVALID, "emmax_op_vision_stage: block %d outside 0..%d", block, T.n_blocks - 1);
    if ((stage == VS_PROJ || stage == VS_FC2) && !tok_in) return fail(EMMAX_ERR_INVALID, "emmax_op_vision_stage: the token rows the branch is added to are required");
    const VisScratch v = {s->vA, s->vpe, s->vtok, s->vln, s->vqkv, s->vatt, s->vmlp, s->vstats, s->splitk_ws, s->splitk_bytes};
    const int rows = B * T.N, D = T.D;
    const void* src = nullptr;
    int r = 0;
    switch (stage) {
    case VS_EMBED: case VS_EMBED_PIXELS: src = in; break;                         // frames uint8 [B, img, img, 3] / pixels bf16 [B, 6, img, img]
    case VS_QKV: case VS_FC1: case VS_FEATURES: r = rows_in(v.vtok, T.Dp, in, rows, D, st); break;
    case VS_ATTN: r = rows_in(v.vqkv, T.D3p, in, rows, 3 * D, st); break;
    case VS_PROJ: r = rows_in(v.vatt, T.Dp, in, rows, D, st); break;
    default: r = rows_in(v.vmlp, T.Mp, in, rows, T.M, st); break;                 // VS_FC2
    }
    if (r) return r;
    if (stage == VS_PROJ || stage == VS_FC2) { if ((r = rows_in(v.vtok, T.Dp, tok_in, rows, D, st))) return r; }
    if (stage == VS_FEATURES && tok_in) { if ((r = rows_in(s->feats, m->Vp, tok_in, R, m->V, st))) return r; }   // the feature rows the copy lands in
    const int run = stage == VS_EMBED_PIXELS ? VS_EMBED : stage;
    if ((r = tower_stage(s, tower, v, block, run, stage == VS_EMBED, src, B, tower == 0 ? 0 : m->tw[0].D, st))) return r;
    switch (stage) {
    case VS_QKV: return rows_out(out, v.vqkv, T.D3p, rows, 3 * D, st);
    case VS_ATTN: return rows_out(out, v.vatt, T.Dp, rows, D, st);
    case VS_FC1: return rows_out(out, v.vmlp, T.Mp, rows, T.M, st);
    case VS_FEATURES: return rows_out(out, s->feats, m->Vp, R, m->V, st);
    default: return rows_out(out, v.vtok, T.Dp, rows, D, st);                      // embed, proj, fc2: the token rows
    }
}

}  // extern "C"
