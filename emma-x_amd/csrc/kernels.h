// kernels.h -- parameter blocks and host launchers of the gfx950 kernels (internal to libemmax_hip.so).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "common.h"

// ---- gemm.hip ----
struct GemmParams {
    const void* A;         // bf16 [M, lda]
    const void* W;         // bf16 [N, ldw]  (K contiguous)
    void* C;               // bf16 / f32 [M, ldc]
    const void* bias;      // bf16 [N] or null
    const void* scale;     // bf16 [N] or null (LayerScale)
    const void* residual;  // bf16 [M, ldr] or null
    int M, N, K;
    int lda, ldw, ldc, ldr;
    int res_f32;           // 1: `residual` is f32 [M, ldr] -- the fp32 residual stream of the prefill (round 5); needs out_f32 (C may alias it: every
                           //    element is read and written by the same thread).  Honoured by the direct epilogue and the split-K reduce passes
    int N_store;           // columns >= N_store are not written
    int act;               // 0 none, 1 gelu(erf), 2 swiglu over 16-col interleaved (gate,up)
    int out_f32;
    // split-K (under-filled problems with a long K, e.g. M = 768 prefill o / down, batch-1 ViT fc2): `ksplit` K slices per
    // tile write fp32 partial tiles to `ws` ([ksplit][M][N] floats), a second kernel sums them and applies the epilogue.
    // ws == null: never split.  ksplit is set by launch_gemm.
    float* ws;
    long long ws_bytes;
    int ksplit;
    // LayerNorm folded into this GEMM (the ViT qkv / fc1 projections): A holds the RAW rows x, W holds
    // W' = bf16(W .* gamma) (launch_ln_fold at finalize), and the epilogue finishes the algebra per output element
    //     y[m, n] = rstd[m] * (acc[m, n] - mean[m] * ln_s[n]) + ln_c[n],   ln_s[n] = sum_k W'[n, k],  ln_c[n] = sum_k W[n, k] beta[k] + bias[n]
    // = LN(x) W^T + bias without ever writing LN(x).  ln_stats: f32 [M][2] = (mean, rstd) per row (launch_row_stats);
    // ln_s / ln_c: f32 [N].  All three null: plain GEMM.  bias must be null when they are set (it lives in ln_c).
    const float* ln_stats;
    const float* ln_s;
    const float* ln_c;
    // RMSNorm of the RESULT rows fused into the split-K reduce pass (one-frame prefill: o-proj -> post-attention norm, down -> the next
    // layer's input norm): norm_out bf16 [M, ld_norm] = RMSNorm(C; norm_w, norm_eps), written next to C.  Only honoured on the whole-problem
    // split-K path -- ask gemm_fuses_norm(p) first, and run launch_rmsnorm yourself when it says no.
    const void* norm_w;
    void* norm_out;
    int ld_norm;
    float norm_eps;
    // exact numerics (round 6, tuning switch `exact`): A holds every activation as TWO bf16 terms x = hi + lo (16 mantissa bits), laid out
    // per 64 elements as [64 x hi][64 x lo] ("HL rows": K steps 2 j / 2 j + 1 of A are the two terms of W's K step j).  The caller passes
    // K = 2 x the real K and lda = the HL row pitch; W keeps its real K columns.  Both terms go through the SAME bf16 MFMAs into the same
    // fp32 accumulators: weights are exact bf16, products are exact in fp32, so the result carries the fp32 reference's arithmetic to
    // ~2^-17 relative per operand instead of the 2^-9 of one bf16 term.
    int a_hl;
    int dbg;               // tools only: 1 = skip the operand DMA after K step 1 (LDS + MFMA time alone), 2 = skip the stores
    long long* trace;      // tools only (tools/gemm_trace.hip): block 0 writes wall_clock64() stamps per tile phase; null in the product
};
// bf16 results leave through the staged epilogue (whole rows through a wave's LDS window, 16-byte stores) when this holds, else through the
// direct one.  ONE predicate: both GEMM kernels evaluate it on the device, gemm_form on the host (act: the kernel's ACT)
__host__ __device__ inline bool gemm_staged_ok(const GemmParams& p, int act) {
    const int n_ok = p.N < p.N_store ? p.N : p.N_store;
    return (p.ldc & 7) == 0 && (((size_t)p.C) & 15) == 0 && !(p.dbg & 8) &&
           (act == 2 ? (p.N & 15) == 0 : (n_ok & 7) == 0) &&                                         // 16-byte row-layout stores possible
           (!p.residual || ((p.ldr & 3) == 0 && (((size_t)p.residual) & 7) == 0));                  // ... and 8-byte residual requests
}
// the instantiation launch_gemm_geom takes (it dispatches on this struct; emmax_gemm_launches prints it) and the epilogue the kernel will then
// take at run time.  Host only, from the parameter block and the tuning switches gemm_deep / gemm_dbg.
//   geom  0 = 128 x 128 x 64, 1 = 256 x 256 x 64, 2 = 128 x 256 x 32        act, out_f32, ln, deep: the kernel's template arguments
//   epi   GEMM_EPI_STAGED, or the direct epilogue with 8- / 16-byte stores (ldc % 4 == 0) or element by element
enum { GEMM_EPI_STAGED = 0, GEMM_EPI_DIRECT_VEC = 1, GEMM_EPI_DIRECT_ELT = 2 };
struct GemmForm { int geom, act, out_f32, ln, deep, epi; };
bool gemm_form(const GemmParams& p, int big, GemmForm* f);                   // false = a shape launch_gemm_geom refuses
// every kernel launch launch_gemm(p) (ksplit = 0) or launch_gemm_splitk(p, ksplit) would make, one line each, WITHOUT launching: the launchers
// themselves run with their launches diverted into the text.  Returns the number of launches, -1 = refused (host only)
int gemm_list_launches(const GemmParams& p, int ksplit, char* buf, int len);
int launch_gemm(const GemmParams& p, hipStream_t stream);                     // picks the 256x256 or the 128x128 tile geometry
int launch_gemm_geom(const GemmParams& p, int big, hipStream_t stream);       // explicit geometry (tools, tests)
int gemm_big_tiles(const GemmParams& p);
int gemm_plan_describe(const GemmParams& p, char* buf, int len);              // the plan launch_gemm would run, as text (host only); returns its kind or -1
bool gemm_fuses_norm(const GemmParams& p);                                    // launch_gemm(p) will apply p.norm_* (see GemmParams)
int launch_gemm_splitk(const GemmParams& p, int ksplit, hipStream_t stream, int big = 0);  // ksplit K slices per tile (128x128; big: 256x256) + reduce / epilogue pass (needs p.ws)
bool gemm_splitk_fuses_norm(const GemmParams& p);                             // launch_gemm_splitk(p, ...) can apply p.norm_* (explicit slices: tools, tests)

// ---- norm.hip ----
int launch_layernorm(const void* x, void* y, const void* w, const void* b, int rows, int D, int ldx, int ldy, float eps,
                     hipStream_t stream);
int launch_rmsnorm(const void* x, void* y, const void* w, int rows, int D, int ldx, int ldy, float eps, hipStream_t stream);
int launch_rmsnorm_f32(const float* x, void* y, const void* w, int rows, int D, int ldx, int ldy, float eps, hipStream_t stream);   // fp32 rows in, bf16 out
// LayerNorm statistics alone: stats f32 [rows][2] = (mean, rstd) of every bf16 row (two-pass variance from registers, as launch_layernorm)
int launch_row_stats(const void* x, float* stats, int rows, int D, int ldx, float eps, hipStream_t stream);
// fold a LayerNorm into the [N, ldw] bf16 weight of the projection that consumes it (in place): W[n, k] <- bf16(W[n, k] * gamma[k]),
// ln_s[n] = sum_k W'[n, k] (of the rounded values), ln_c[n] = sum_k W[n, k] * beta[k] + bias[n] (fp32; bias may be null)
int launch_ln_fold(void* W, int ldw, int N, int K, const void* gamma, const void* beta, const void* bias, float* ln_s, float* ln_c,
                   hipStream_t stream);

// ---- attention.hip ----
struct AttnParams {
    const void* qkv;
    void* out;
    const int32_t* cu_seqlens;
    int ld_qkv, q_off, k_off, v_off, ld_out;
    int B, max_seqlen, Hq, Hkv;
    float scale;
    int causal;
};
// the instantiation launch_attention takes (it dispatches on this struct; emmax_attention_plan prints it): the resident or the ring kernel, query
// waves, producer waves (resident), key groups over the same query waves (AttnCfg::KSPL), the lazy reference maximum, query rows per block (ring) /
// resident rows per item.  Host only, from the shape and the tuning switches attn_resident / attn_ksplit / attn_lazy.  false = a shape refused
struct AttnForm { int resident, head_dim, qwaves, pwaves, kgroups, lazy, rows; };
bool attention_form(int B, int max_seqlen, int Hq, int Hkv, int head_dim, int causal, AttnForm* f);
int launch_attention(const AttnParams& p, int head_dim, hipStream_t stream);
int launch_x_attention(const AttnParams& p, int head_dim, hipStream_t stream);   // exact.hip: fp32 q / k / v rows in, HL rows out, fp32 MFMA

// ---- exact.hip: the exact-numerics mode (tuning switch `exact`; GemmParams::a_hl) ----
// "HL rows": bf16 rows holding every element as two terms, per 64 elements [64 x hi][64 x lo]; pitch >= 2 x the padded width
int launch_x_split_rows(const float* x, void* y_hl, int rows, int D, int Dp, int ldx, int ldy, hipStream_t stream);
int launch_x_rmsnorm(const float* x, void* y_hl, const void* w, int rows, int D, int ldx, int ldy, float eps, hipStream_t stream);
int launch_x_layernorm(const float* x, void* y_hl, const void* w, const void* b, int rows, int D, int Dp, int ldx, int ldy, float eps, hipStream_t stream);
int launch_x_join_rows(const void* x_hl, float* y, int rows, int D, int ldx, int ldy, hipStream_t stream);   // y = hi + lo (tests)
int launch_x_to_bf16(const float* x, int ldx, void* y, int ldy, int rows, int D, hipStream_t stream);
int launch_x_patch_gather(bool from_u8, const void* src, void* out_hl, int B, int img, int patch, int kpad, int chan0, const float* mean, const float* std,
                          hipStream_t stream);
int launch_x_assemble_tokens(const float* pe, const void* pos, const void* cls, const void* reg, float* tokens, int B, int n_patches, int n_prefix, int has_cls,
                             int D, int ld, hipStream_t stream);
int launch_x_embed_splice(const int32_t* ids, int P_max, const int32_t* cu, const void* E, const float* patches32, const void* patches_bf, float* h32, int B,
                          int max_seqlen, int n_patches, int hidden, int vocab, hipStream_t stream);
int launch_x_rope_kv_write(float* qkv, int ld, int q_off, int k_off, int v_off, const int32_t* cu, int B, int total_rows, const float* cos_t, const float* sin_t,
                           void* kcache, void* vcache, long long kv24, const int32_t* page_table, int max_pages, int Hq, int Hkv, int hd, int page, hipStream_t stream);

// ---- misc.hip ----
int launch_patch_gather(bool from_u8, const void* src, void* out, int B, int img, int patch, int kpad, int chan0,
                        const float* mean, const float* std, hipStream_t stream);
int launch_assemble_tokens(const void* pe, const void* pos, const void* cls, const void* reg, void* tokens, int B,
                           int n_patches, int n_prefix, int has_cls, int D, int ld, hipStream_t stream);
int launch_copy_rows(const void* in, int ld_in, void* out, int B, int rows_in, int r_off, int rows_out, int D, int ld_out,
                     int col_off, hipStream_t stream);
#define EMMAX_MAX_DECODE_BATCH 64   // rows of a decode step: 17-32 = two 16-wide MFMA batch tiles, 33-64 = two halves of two (decode_kmp.hip; decode_km.hip: 16 rows); rounds 1-4: 8, round 5: 32
#define EMMAX_KMP_ROWS 32           // rows one decode_kmp.hip half stages: the down projection and the lm-head of 33-64 rows run as two launches of <= 32
#define EMMAX_MAX_STOP_IDS 16
struct PrefillState {
    int B;
    int S[EMMAX_MAX_DECODE_BATCH];
};
// ROW STATE: the generation state every row of a session has (session.h: emmax_session::rows), one int32 per row and the output row
struct RowState {
    int32_t *cur_tok, *ctx_len, *done, *n_out, *max_new, *stop_m, *stop_after, *out_ids /* [rows][max_out] */;
    RowState from(int r0, int max_out) const {   // host: the view from row r0 on
        return {cur_tok + r0, ctx_len + r0, done + r0, n_out + r0, max_new + r0, stop_m + r0, stop_after + r0, out_ids + (size_t)r0 * max_out};
    }
};
// ROW COLUMNS: a session's per-row device arrays as one list (session.hip: session_row_cols) -- row r of a column is the move_bytes bytes at
// base + r * stride_bytes, both multiples of 4.  A staged commit moves every column of a row, a slot fork the `inherit` ones: an array that
// is in the list cannot be forgotten by either
enum { ROWS_CORE = 0, ROWS_SAMPLING, ROWS_PROCESSING, ROWS_WARPERS, ROWS_RULES, ROWS_AUTOMATON, ROWS_TOPLP };
struct RowCol {
    char* base;
    uint32_t stride_bytes, move_bytes;
    uint8_t owner, inherit;   // ROWS_*; a forked follower takes its source's
};
struct RowCols {
    int n;
    RowCol col[32];
};
// per-row decode state of B fresh sequences (rows: already the view from the first row / slot on)
int launch_prefill_state(const PrefillState& st, int32_t* cu, const RowState& rows, hipStream_t stream);
// emmax_slots_commit: staging rows src[i] become slots slot[i]: every column of the row copied, page-table rows swapped (the slot's old
// pages become the staging row's), the staging row left done with an empty context
struct CommitParams {
    int n, max_pages;
    int slot[EMMAX_MAX_DECODE_BATCH], src[EMMAX_MAX_DECODE_BATCH];
    int32_t* page_table;
    RowCols cols;
    int32_t *done, *ctx_len;
};
static_assert(sizeof(CommitParams) <= 2048, "CommitParams travels as a kernel argument (4 KiB in all)");
int launch_slots_commit(const CommitParams& c, hipStream_t stream);
// emmax_slots_fork: the freshly prefilled slot `src` forked into the n idle slots dst[] (one block per follower).  Follower f hides its own
// first nfull pages (hidden[f][i] = table[f][i]) and references the source's (table[f][i] = table[src][i]: the slot table is a permutation,
// nothing here assumes the identity); from the prompt's partial page on it keeps its own pages, and entry j of the copy list names that
// page's copy (launch_beam_copy consumes it: src = -1 where the prompt ends on a page boundary).  Fresh decode state as
// emmax_group_fork_kernel leaves it, the source's inherited columns (cols), the uploaded sampling parameters in_*[j], and with an
// automaton set (aut_start, else both null) the source's start state as the follower's state
struct SlotForkParams {
    int n, rows, src, S, max_pages;
    int dst[EMMAX_MAX_DECODE_BATCH];
    int32_t *page_table, *hidden, *copy_src, *copy_dst, *copy_ntok;
    RowState st;
    RowCols cols;
    const float *in_t, *in_p;
    const int32_t* in_k;
    const uint64_t* in_seed;
    const uint32_t* in_sub;
    float *temperature, *top_p;
    int32_t* top_k;
    uint64_t* seed;
    uint32_t* subseq;
    int32_t *aut_start, *aut_state;
};
static_assert(sizeof(SlotForkParams) <= 2048, "SlotForkParams travels as a kernel argument (4 KiB in all)");
int launch_slots_fork(const SlotForkParams& p, hipStream_t stream);
// table[i] = hidden[i], hidden[i] = -1 wherever hidden[i] >= 0, i < n: a released follower takes its own pages back (its two rows), an
// owner's slot takes its heir's (the owner's table row, the heir's hidden row), and every row at once when slot serving ends
int launch_slots_unhide(int32_t* table, int32_t* hidden, int n, hipStream_t stream);
int launch_set_int(int32_t* p, int32_t v, hipStream_t stream);
int launch_set_ints(int32_t* p, int n, int32_t v, hipStream_t stream);
int launch_slots_idle(int n, const RowState& rows, int32_t pad_id, hipStream_t stream);
int launch_embed_splice(const int32_t* ids, int P_max, const int32_t* cu, const void* E, const void* patches, void* h, int B,
                        int max_seqlen, int n_patches, int hidden, int vocab, hipStream_t stream, float* h32 = nullptr);   // h32: the rows also as fp32
int launch_rope_kv_write(void* qkv, int ld, int q_off, int k_off, int v_off, const int32_t* cu, int B, int total_rows,
                         const float* cos_t, const float* sin_t, void* kcache, void* vcache, const int32_t* page_table,
                         int max_pages, int Hq, int Hkv, int hd, int page, hipStream_t stream);
// fp8 KV cache: quantise the prefill's K / V rows (K rotated in place by launch_rope_kv_write with null cache pointers) into e4m3 pages + row scales
int launch_kv_quant_rows(void* qkv /* rows written back as bf16(e4m3 x scale): the prefill attention sees what the cache holds */, int ld, int k_off, int v_off, const int32_t* cu, int B, int total_rows, void* k8, void* v8, float* kscale,
                         float* vscale, const int32_t* page_table, int max_pages, int Hkv, int hd, int page, hipStream_t stream);
int launch_resize_bicubic_u8(const uint8_t* src, int B, int H, int W, uint8_t* dst, int OH, int OW, uint8_t* tmp, const int32_t* bounds_h,
                             const int32_t* kk_h, int ksize_h, const int32_t* bounds_v, const int32_t* kk_v, int ksize_v, hipStream_t stream);
// out32: the rows also as fp32; in32 != null: the source rows are fp32 (`in` unused)
int launch_gather_last_rows(const void* in, void* out, const int32_t* cu, int B, int D, hipStream_t stream, float* out32 = nullptr, const float* in32 = nullptr);

// ---- tuning switches (model.hip) ----
// ONE table of named integers, read from the environment (EMMAX_<NAME>) ONCE, when the library first needs a value; after that only
// emmax_tuning_set() (include/emmax.h) changes them.  No launcher calls getenv.  Defaults are the product path; the other values
// are the A/B partners DESIGN.md's measurements quote.
struct EmmaxTune {
    int graph;           // 0: eager launch-ahead decode steps (default); 1: replay a captured hipGraph of the step
    int ks;              // 1: batch 1-2 bf16 projections on decode_ks.hip; 0: decode.hip's LDS-staged GEMV
    int ks_oproj;        // 1: ... including the o-proj with the split merge (one block per CU); 0: decode.hip's kernel
    int ks_oproj_grid;   // grid cap of that o-proj launch (256)
    int km;              // 1: batch >= 3 (and fp8) projections on decode_km.hip; 0: decode_mfma.hip
    int km_down;         // 1: ... including the two-phase down projection
    int km_roll;         // 1: decode_km.hip refills a weight register as soon as its MFMA has issued (rolling ring); 0: a tile's sixteen refills together
    int attn_deep;       // bf16 decode attention: four chunks of keys in flight per wave instead of two (the fp8-cache form always has four): -1 = from 1024 blocks (batch 32), 0 never, 1 always
    int attn_ksplit;     // causal prefill attention (head_dim 128): two key groups per block (8 waves) -- -1 = when the launch leaves <= 1 block per CU (one frame), 0 never, 1 always
    int attn_lazy;       // causal prefill attention (head_dim 128): 1 = lazy reference maximum (round 5), 0 = the running maximum of rounds 1-4 (bit-regression probes)
    int vis_streams;     // vision encode: 1 = the two towers side by side on two streams (default; batches up to 256 frames), 0 = one after the other on the caller's stream
    int attn_nw;         // waves per decode-attention block: 0 = by shape (4; 8 for the one-split form when that leaves <= 256 blocks), 4 / 8 forced
    int streamk;         // 1: stream-K work split in decode_mfma.hip; 0: whole tasks per block
    int fp8_gemv;        // -1: default routing of the batch 1-2 fp8 projections; >= 0: bit mask (1 qkv, 2 o-proj, 4 gate/up, 8 down, 16 lm-head) on the row GEMV
    int attn_group;      // decode attention of a grouped step (sample groups, beams): the shared prompt pages read once per group and the rows' own tails by a second
                         //   launch -- -1 = at the shapes where that was measured faster (sample groups of 4-16 rows at 32 / 48 / 64 rows; step.hip: attn_group_rows), 1 = wherever the kernels
                         //   take the step, 0 = never: one launch, every row streams its whole context
    int attn_nsplit;     // 0: KV splits of the decode attention chosen from (B, kv heads); > 0: forced (rounded down to 2^k, <= 16)
    int attn_direct;     // 1: with one KV split the attention launch writes the normalised bf16 row itself
    int fold_embed;      // 1: layer 0's qkv launch gathers the embedding row itself (batch 1-2, bf16)
    int mfma_xbar;       // 1: decode_mfma.hip orders the activation requests ahead of the weight head with a block barrier
    int gemm_big;        // -1: planned tile geometry; 0 / 1: all small / all big tiles, no split-K
    int gemm_splitk;     // 1: split-K for under-filled long-K GEMMs
    int gemm_sk_big;     // split-K tile geometry: -1 = planned (128 x 128, or 256 x 256 when the cost model prefers it), 0 / 1 = small / big forced (tools)
    int gemm_hybrid;     // 1: a column remainder behind whole rounds of big tiles goes through K-split small tiles when K is long (one-frame prefill gate/up)
    int gemm_normfuse;   // 1: the split-K reduce pass of the one-frame prefill o-proj / down also applies the RMSNorm that follows
    int gemm_deep;       // GEMM main loop: -1 = by geometry (256x256: staggered wave groups, 128x128: deep A ring), 0 = two stages + one barrier per step, 1 = third LDS stage for A, 3 = staggered wave groups (256x256 only)
    int gemm_dbg;        // lab: OR-ed into GemmParams::dbg (16 = the second half of the waves requests its slabs mid-step)
    int gemm_lnfuse;     // 1: LayerNorm / RMSNorm applied by the GEMM that consumes the normalised rows (no separate norm pass)
    int attn_resident;   // -1: resident ViT attention kernel where measured faster; 0: never; 2: whenever it fits (tests)
    int kv_fp8;          // 1: sessions created from now on keep the paged KV cache as e4m3 rows + one fp32 scale per (token, head) row (opt-in: half the attention bytes of a decode step, its own error line in the tests); 0: bf16
    int resid32;         // 1: prefill and decode step keep the residual stream in fp32 (GemmParams::res_f32, GemvParams::h32); 2: the decode step only; 0: bf16 rows (rounds 1-4)
    int mx4_wide;        // 1: MXFP4 models CREATED from now on serve 17-64 rows on decode_kmp.hip's MX4 form (read at emmax_model_create and frozen in the model: emmax_model_mxfp4_wide); 0: 1-16 rows (default)
    int exact;           // 1: EXACT NUMERICS (round 6) -- models finalized and sessions created from now on carry fp32 activations end to end, every bf16
                         //    MFMA / dot2 activation operand as two bf16 terms (hi + lo), fp32 attention (fp32 MFMA) over an fp32 KV cache: the
                         //    reference's fp32 CPU arithmetic to ~1e-5 of max|logit| instead of 2.4e-2.  Batch 1-2 sessions on bf16 weights; the model
                         //    keeps the ViT LayerNorms unfolded.  0: the bf16-operand product path (default)
    int epoch;           // bumped by every emmax_tuning_set: sessions drop captured graphs when it moves
};
const EmmaxTune& emmax_tune();

// ---- the weight format of a decode projection: ONE value from emmax_config.decode_fp8 to the kernels' template argument ----
// fp8: the row copy for the staged GEMV, the e4m3 tiles for the MFMA families; MX4 / MX6: decode_km.hip's block-scaled tiles (MX4 also decode_kmp.hip's)
enum { PW_BF16 = 0, PW_FP8 = 1, PW_MX4 = 2, PW_MX6 = 3, PW_COUNT = 4 };
struct WFmt {
    const char* name;   // as the error texts spell it
    int code;           // emmax_config.decode_fp8 (3 is no format)
    int ks;             // elements of a row per load step: one 16-byte load per lane feeds ks / 32 MFMAs
    int tile_bytes;     // bytes of a 16-row tile of one load step
    bool mx;            // block-scaled: an e8m0 code stream beside the tiles, WFMT_SCALE_BYTES per tile (one dword of four codes per row)
};
constexpr WFmt WFMT[PW_COUNT] = {{"bf16", 0, 32, 1024, false}, {"fp8", 1, 64, 1024, false}, {"MXFP4", 2, 128, 1024, true}, {"MXFP6", 4, 128, 1536, true}};
constexpr int WFMT_SCALE_BYTES = 64;
constexpr bool wfmt_is_mx(int f) { return WFMT[f].mx; }
constexpr int wfmt_fps(int f) { return WFMT[f].ks / 32; }                           // MFMA fragments (32 elements) per load step
constexpr int wfmt_bytes_per_k(int f) { return WFMT[f].tile_bytes / WFMT[f].ks; }   // bytes of 16 rows x one k: 32 / 16 / 8 / 12
constexpr size_t wfmt_bytes(int f, size_t N, size_t K) { return N / 16 * K * wfmt_bytes_per_k(f); }                                 // a matrix's tiles
constexpr size_t wfmt_scale_bytes(int f, size_t N, size_t K) { return WFMT[f].mx ? N / 16 * (K / WFMT[f].ks) * WFMT_SCALE_BYTES : 0; }   // ... its code stream
inline int wfmt_of_code(int code) {   // -1: no format
    for (int f = 0; f < PW_COUNT; ++f)
        if (WFMT[f].code == code) return f;
    return -1;
}

// ---- decode.hip: the LDS-staged GEMV, the embedding gather ----
enum { GEMV_QKV = 0, GEMV_RESID = 1, GEMV_GATEUP = 2, GEMV_LMHEAD = 3, GEMV_PLAIN = 4 };
struct GemvParams {
    const void* x;          // bf16 [B, ldx] activations
    const void* W;          // bf16 [rows, ldw]
    void* y;                // output (mode dependent): q buffer / h (in place) / act / plain
    const void* norm_w;     // bf16 [K] RMSNorm weight (NORM modes)
    int K, ldw, ldx, ldy;
    int n_rows;             // weight rows (QKV: (Hq+2Hkv)*hd; GATEUP: 2*inter_p interleaved; LMHEAD: vocab; else output rows)
    int n_groups;           // 2-row groups (set by the launcher)
    int max_parts;          // LMHEAD: capacity of part_val / part_idx in blocks
    int kc;                 // K phase length (set by the launcher)
    int batch;              // MFMA path: runtime batch (set by the launcher)
    float eps;
    // QKV epilogue
    int head_dim, Hq, Hkv, page, max_pages;
    const int32_t* ctx_len;
    const int32_t* page_table;
    const float* cos_t;
    const float* sin_t;
    void* kcache;
    void* vcache;
    // LMHEAD epilogue
    float* part_val;
    int32_t* part_idx;
    float* logits_out;      // optional f32 [B, n_rows]
    // RESID with x = merged attention output: split partials f32 [B][Hq][nsplit][132] (null: x is a bf16 vector)
    const float* attn_part;
    int nsplit;
    void* kv_stage;         // QKV, fp8 KV cache (round 5, opt-in): the new K / V rows go to bf16 [B][Hkv][2][head_dim] instead of the paged cache;
                            //   the attention launch of the step quantises them (one scale per row) and appends them
    const float* wscale;    // per-row fp32 scales when W is an fp8 copy (MFMA path: fragment-major tiles; GEMV: rows in span order); null: bf16
    int n_pairs;            // GEMV, set by the launcher: row pairs (fp8 groups hold two)
    unsigned long long* sk_ws;   // MFMA path: stream-K granules [256 blocks][2 tiles][256] of {f32, tag} (null: whole tasks per block)
    int sk_kt8, sk_q, sk_r;      // MFMA path, set by the launcher: super-steps per task (0: whole tasks), per-block share and remainder
    unsigned int sk_magic;       // ... and ceil(2^32 / sk_kt8)
    int qk_shift;                // MFMA QKV, set by the launcher: log2(head_dim / 32)
    int x_bar;                   // MFMA path, set by the launcher: block barrier between the activation requests and the weight head
    int max_grid;           // 0: default persistent grid; > 0: cap (the K-split o-proj with the split merge runs one block per CU)
    int ks_shift;           // K-split kernel, QKV, set by its launcher: log2(head_dim / 2)
    const int32_t* x_tok;   // K-split kernel, non-null: x row b = x[x_tok[b]] (p.x = embedding table, ids clamped to x_vocab): the embed launch
    void* x_copy;           //   folded into layer 0's qkv; block 0 also copies the rows to x_copy [B, ldx] (the residual stream)
    int x_vocab;
    // fp32 residual stream (round 5, tuning switch resid32): h32 f32 [B, ldh] is the MASTER copy of the hidden rows of a decode step, the
    // bf16 rows (p.x of the NORM modes = p.y of the RESID modes) its mirror.  RESID modes (o-proj, down) add into h32 in place and store
    // bf16(sum) in the mirror; NORM modes (qkv, gate/up, lm-head) read either -- the batch 1-2 kernels the fp32 rows (free there: statistics
    // and x g in fp32, one rounding), the batch >= 3 / fp8 MFMA kernels the mirror (the fp32 rows cost them 1.5 % of a step).  Either way
    // the stream is no longer rounded after each of the 64 additions of a token: the mirror is re-derived from fp32 every time.
    float* h32;
    int ldh;
    // exact numerics (round 6, tuning switch `exact`; decode_ks.hip, batch 1-2): every activation operand enters the dot products as TWO bf16
    // terms (hi + lo of the fp32 value; the fp32 stream h32 must be set), and what the projections hand on stays fp32 -- QKV: p.y = f32 q rows
    // [B, ldy], the K / V rows go to an fp32 paged cache (kcache / vcache as float); GATEUP: p.y = f32 [B, ldy]; RESID over the SwiGLU
    // product: p.x = f32 [B, ldx]; RESID over the attention partials: the merge stays fp32 until it is split.
    int exact;
    long long kv24;         // exact numerics: > 0 = the K / V caches are 24-bit (common.h: x24) -- kcache / vcache point at the bf16 plane of kv24 elements,
                            //   the 8-bit extension plane follows it; 0 = fp32 rows
    const void* w_codes;    // block-scaled tiles (WFmt::mx; launch_quant_mx): their e8m0 scale stream; null otherwise
    int wfmt;               // PW_*: what W holds -- the ONE statement of the format (proj_shape and the launchers' dispatch read it; wscale / w_codes are
                            //   the operands that go with it).  Written by gemv_set_weights alone; a zero-initialised block is bf16
};
static_assert(sizeof(GemvParams) == 312 && offsetof(GemvParams, w_codes) == 296 && offsetof(GemvParams, wfmt) == 304,
              "GemvParams travels by value: the kernels read it at the offsets they were compiled for");
// the only writer of (W, wscale, w_codes, wfmt): scales = the per-row fp32 scales of an fp8 copy, or the code stream of block-scaled tiles
static inline void gemv_set_weights(GemvParams& p, int wfmt, const void* W, const void* scales = nullptr) {
    p.W = W;
    p.wfmt = wfmt;
    p.wscale = wfmt == PW_FP8 ? (const float*)scales : nullptr;
    p.w_codes = wfmt_is_mx(wfmt) ? scales : nullptr;
}
// (where the QKV epilogues put the new K / V rows: gemv_kv_row / gemv_kv_store_x, decode_epilogue.h -- device code, this is also a host header)

// ---- who decides what a launcher takes ----
// ProjShape: what the five decode projection families read of a launch to decide whether they take it -- no pointers, so the planner
// (step.hip: proj_route, model_max_decode_batch) asks before any arena or session exists.  Every family has ONE pure check,
// <family>_takes(shape, B, geometry out): no HIP call, no stream; it reads emmax_tune() where the launcher did (km_down, km_roll, ks_oproj).
// The launcher derives the shape, asks its own check and launches from the geometry it returned (or from the one its caller already
// got from the same check: the `geom` argument of the launchers): a launcher has no shape-based refusal its check does not report.
struct ProjShape {
    int mode, K, n_rows, head_dim, Hq;
    int wfmt;                            // PW_*
    bool exact, h32, attn_part, x_tok;   // exact numerics; the fp32 stream is present; split partials in (nsplit of them); the folded embedding gather
    int nsplit, max_parts, max_grid;
    bool ld_ok;                          // ldw and ldx are multiples of 8
    bool mx4_wide;                       // MXFP4 tiles at 17-64 rows: decode_kmp.hip's MX4 form may take them (the model froze the tuning switch mx4_wide; proj_shape leaves it false)
};
static inline ProjShape proj_shape(int mode, const GemvParams& p) {
    return {mode, p.K, p.n_rows, p.head_dim, p.Hq, p.wfmt, p.exact != 0, p.h32 != nullptr,
            p.attn_part != nullptr, p.x_tok != nullptr, p.nsplit, p.max_parts, p.max_grid, p.ldw % 8 == 0 && p.ldx % 8 == 0};
}
// the launch geometry a check hands its launcher (fields a family does not use stay 0)
struct ProjGeom {
    int grid, n_groups;     // blocks; row groups / tiles of the matrix (GemvParams::n_groups)
    int kc;                 // GemvParams::kc as the kernel reads it: LDS rows (ks), K phase length (gemv, mfma), tiles per block (km)
    size_t smem;            // dynamic LDS bytes
    int shift;              // ks: ks_shift, mfma: qk_shift
    int cpl, f8;            // ks: 16-byte chunks per lane; staged GEMV: block shape of the fp8 rows (0: bf16)
    int nb, phased, roll;   // km: staged rows (8 / 16), the phased down form, the rolling refill (exact numerics: GemvParams::exact)
    int tmax, nph, nh;      // kmp: tiles per block, phases, halves
};
bool decode_ks_takes(const ProjShape& s, int B, ProjGeom* g = nullptr);     // decode_ks.hip
bool decode_gemv_takes(const ProjShape& s, int B, ProjGeom* g = nullptr);   // decode.hip's own staged kernel (fp8: the row GEMV)
bool decode_km_takes(const ProjShape& s, int B, ProjGeom* g = nullptr);     // decode_km.hip; 17-64 rows: decode_kmp.hip's answer
bool decode_kmp_takes(const ProjShape& s, int B, ProjGeom* g = nullptr);    // decode_kmp.hip
bool decode_mfma_takes(const ProjShape& s, int B, ProjGeom* g = nullptr);   // decode_mfma.hip
// staged_out (optional): 1 when decode.hip's own LDS-staged kernel served the call, 0 when decode_ks.hip took it.
// The staged kernel exists for the fused modes at B = 1, 2 (bf16 and fp8 rows) and for GEMV_PLAIN at B <= 8 (fp8 rows: B <= 2); any other
// (mode, B) returns -1 -- launch_proj (step.hip) sends every batch >= EMMAX_MFMA_MIN_BATCH to the MFMA kernels.
int launch_decode_gemv(int mode, const GemvParams& p, int B, hipStream_t stream, int* grid_out = nullptr, int* staged_out = nullptr);
// ... its own staged kernel alone, from a geometry decode_gemv_takes returned (launch_proj: the route has asked already)
int launch_decode_gemv_staged(int mode, const GemvParams& p, int B, const ProjGeom& g, hipStream_t stream, int* grid_out = nullptr);
// decode_ks.hip: the batch 1-2 bf16 projections with K split across the waves of a block (activation slice in registers, no
// block-wide stage); returns -2 for a shape it does not take.  launch_decode_gemv tries it first (tuning switch `ks` = 0: never).
int launch_decode_ks(int mode, const GemvParams& p, int B, hipStream_t stream, int* grid_out = nullptr, const ProjGeom* geom = nullptr);
bool decode_ks_enabled();
int decode_gemv_init();   // raise the dynamic-LDS limit of every GEMV instantiation (call once, outside graph capture)
int launch_decode_embed(const int32_t* cur_tok, const void* E, void* h, int B, int hidden, int vocab, hipStream_t stream, float* h32 = nullptr);

// ---- decode_attn.hip ----
struct DecodeAttnParams {
    const void* q;          // bf16 [B, ldq] rotated queries
    const void* kcache;     // bf16 [pages][Hkv][page][hd]
    const void* vcache;
    const int32_t* page_table;
    const int32_t* ctx_len;
    const int32_t* done;    // int32 [B] or null: finished / idle rows read no K/V (their partials are written empty)
    float* part;            // f32 [B][Hq][nsplit][132] = { o[128] un-normalised, m, l, pad }
    void* o_out;            // non-null (one split only): the block normalises its result and writes the bf16 row [B, ldq] itself
    // fp8 KV cache (kv_stage non-null): kcache / vcache are e4m3 bytes [pages][Hkv][page][hd], kscale / vscale fp32 [pages][Hkv][page]; the
    // step's new rows come from kv_stage bf16 [B][Hkv][2][hd] (written by the qkv launch): every block that needs key L - 1 quantises it
    // itself, split 0 appends it to the cache
    const void* kv_stage;
    float* kscale;
    float* vscale;
    int ldq, Hkv, page, max_pages;
    int page_shift;         // log2(page), set by the launcher
    float scale;
    long long kv24;         // exact numerics (launch_x_decode_attn): > 0 = 24-bit caches (GemvParams::kv24), 0 = fp32 rows
    // grouped form (launch_group_attn): rows g N .. g N + N - 1 hold the same page ids in their first grp_shared[g] table entries.  A DEVICE
    // array: a captured step is replayed for later prompts of other lengths
    const int32_t* grp_shared;
    int grp_N, grp_nsplit, grp_Hq;   // rows per group; splits of the shared span; q heads (set by the launcher)
};
int decode_attn_nsplit(int B, int Hkv);
// the instantiation launch_decode_attn takes (it dispatches on this struct; emmax_decode_attn_plan prints it): template arguments G, NW, DIRECT,
// KV8, DEEP and the grid's split count.  false = a shape the launcher refuses.  Host only: looks at which operands exist, never through them
struct DecodeAttnForm { int G, nw, direct, kv8, deep, nsplit; };
bool decode_attn_form(const DecodeAttnParams& p, int B, int Hq, int nsplit, DecodeAttnForm* f);
bool attn_direct_rule(int B, int Hkv, bool exact);   // step.hip: the one-split direct form in a B-row step (attn_direct_on without a model)
int launch_decode_attn(const DecodeAttnParams& p, int B, int Hq, int head_dim, int nsplit, hipStream_t stream);
// The attention of a step whose B rows are B / N groups on shared prompt pages, in two launches: the span [0, grp_shared[g] * page) once per
// group into split partials (p.part: group_attn_nsplit() per (row, head)), then one block per (row, kv head) over the row's own tail, which
// folds the partials in and writes the bf16 row (p.o_out).  bf16 and fp8 cache; -1 for a shape it does not take (group_attn_takes)
enum { EMMAX_GROUP_ATTN_MAX_SPLITS = 8 };
bool group_attn_takes(int B, int N, int Hq, int Hkv);
int group_attn_nsplit(int B, int N, int Hq, int Hkv);
// the two launches of launch_group_attn (it dispatches on this struct): queries per span block, span splits, query chunks per (group, kv head), tail G
struct GroupAttnForm { int width, nsplit, chunks, G, kv8; };
bool group_attn_form(const DecodeAttnParams& p, int B, int N, int Hq, GroupAttnForm* f);
int launch_group_attn(const DecodeAttnParams& p, int B, int N, int Hq, int head_dim, hipStream_t stream);
int launch_x_decode_attn(const DecodeAttnParams& p, int B, int Hq, int head_dim, int nsplit, hipStream_t stream);   // exact.hip: fp32 q, fp32 cache

// ---- extend_attn.hip: n new tokens per sequence on top of a cached context ----
// packed row i of sequence b (rows cu[b] .. cu[b + 1]) sits at position base[b] + i; cu and base are device arrays
struct ExtendAttnParams {
    const void* q;          // bf16 packed rows [total, ldq], head h of a row at q_off + h * 128 (already rotated)
    void* out;              // bf16 [total, ld_out]
    const void* kcache;     // bf16 [pages][Hkv][64][128], or e4m3 bytes with kscale / vscale fp32 [pages][Hkv][64]
    const void* vcache;
    const float* kscale;
    const float* vscale;
    const int32_t* page_table;   // [B][max_pages]
    const int32_t* cu;           // [B + 1]
    const int32_t* base;         // [B]: the sequences' cached lengths BEFORE the append
    float* part;                 // split form: f32 [total][Hq][nsplit][132] = { o[128] un-normalised, m, l, pad }
    int ldq, q_off, ld_out, B, Hq, Hkv, max_pages;
    float scale;
};
// what launch_extend_attn dispatches on (emmax_extend_attn_plan prints it): GQA group, tokens per block (128 / G), query tiles per sequence, key
// splits, the split form (partials + merge pass) or the direct one, the e4m3 cache
struct ExtendAttnPlan { int G, qt, nqt, nsplit, split, kv8; };
// max_n / max_L: upper bounds of the new rows / of base + n of any sequence; nsplit 0 = the planner's choice.  false: a shape the launcher refuses
bool extend_attn_plan(int B, int max_n, int max_L, int Hq, int Hkv, int nsplit, int kv8, ExtendAttnPlan* f);
int launch_extend_attn(const ExtendAttnParams& p, const ExtendAttnPlan& f, int total_rows, hipStream_t stream);   // page = 64, head_dim = 128
// launch_rope_kv_write / launch_kv_quant_rows at position base[b] + i (the quantising pass leaves the qkv rows as they are); max_pos: rows of cos / sin
int launch_rope_kv_write_at(void* qkv, int ld, int q_off, int k_off, int v_off, const int32_t* cu, const int32_t* base, int B, int total_rows,
                            const float* cos_t, const float* sin_t, void* kcache, void* vcache, const int32_t* page_table, int max_pages, int Hq,
                            int Hkv, int hd, int page, int max_pos, hipStream_t stream);
// the rows' state when they grow by st.S[b] tokens: base[b] = ctx_len[b], cu = the packed offsets of the new rows, ctx_len += S; the rest as launch_prefill_state.
// aut_state / aut_start (both or neither): a row outside the automaton (state -1) enters at its start state, the others keep their state
int launch_extend_state(const PrefillState& st, int32_t* cu, int32_t* base, const RowState& rows, int32_t* aut_state, const int32_t* aut_start,
                        hipStream_t stream);
int launch_kv_quant_rows_at(const void* qkv, int ld, int k_off, int v_off, const int32_t* cu, const int32_t* base, int B, int total_rows, void* k8,
                            void* v8, float* kscale, float* vscale, const int32_t* page_table, int max_pages, int Hkv, int hd, int page,
                            hipStream_t stream);

// ---- score.hip: log-sum-exp, one target logit and the argmax of rows x lm-head, no logit stored ----
struct ScoreParams {
    const void* X;               // bf16 [rows, ldx]: the finally-normed rows
    const void* W;               // bf16 [Np, ldw]: the lm-head, Np = V padded to 128
    const int32_t* targets;      // [rows]: the id whose logit is wanted; outside [0, V) (-100): 0.0f
    float* ws;                   // three planes [slices][rows]: m, l (fp32), idx (int32)
    float *lse, *target_logit;   // [rows]
    int32_t* argmax;             // [rows]
    int ldx, ldw, rows, V, K;
    // filled by launch_score_rows from the form
    float *part_m, *part_l;
    int32_t* part_i;
    int row_tiles, col_tiles, slices, tps;
};
// what launch_score_rows dispatches on (emmax_score_plan prints it): 128-row tiles, 128-column tiles below V, vocabulary slices, tiles per slice
struct ScoreForm { int row_tiles, col_tiles, slices, tps; };
// slices_forced 0: about two blocks per CU, capped by the column tiles and by ws_bytes / (12 rows).  false: a shape, a slice count or a scratch the launcher refuses
bool score_form(int rows, int V, int K, long long ws_bytes, int slices_forced, ScoreForm* f);
int launch_score_rows(const ScoreParams& p, const ScoreForm& f, hipStream_t stream);

// ---- taps.hip: what a session hands out of a pass it runs anyway ----
// rows x H of the residual stream (fp32 rows, or bf16 rows: src_f32 = 0) into fp32 [rows][H]; norm_w != nullptr: the RMSNorm of each row, fp32 throughout.
// gather (may be null): the source row of row r is gather[r], clamped to gather_rows (a step's embedding rows, read by token id).
// gen_idx (may be null; a decode step): row r lands gen_idx[r] x gen_stride floats further on -- nothing where done[r] != 0 or the index is outside 0 .. max_new - 1
struct TapRowsParams {
    const void* src;
    float* dst;
    const void* norm_w;
    const int32_t *gather, *gen_idx, *done;
    long long gen_stride;
    int src_f32, ld_src, rows, H, gather_rows, max_new;
    float eps;
};
int launch_tap_rows(const TapRowsParams& p, hipStream_t stream);
// fp32 softmax(scale q . K^T) of the new query rows over the paged cache: ExtendAttnParams' q / K / tables (base == nullptr: every sequence at 0)
struct AttnProbsParams {
    const void* q;               // bf16 packed rows [total, ldq], head h of a row at q_off + h * 128 (already rotated)
    const void* kcache;          // bf16 [pages][Hkv][64][128], or e4m3 bytes with kscale fp32 [pages][Hkv][64]
    const float* kscale;
    const int32_t* page_table;   // [B][max_pages]
    const int32_t* cu;           // [B + 1], or nullptr: one new row per sequence, packed row b (a decode step)
    const int32_t* base;         // [B] or nullptr
    float* probs;                // f32 [total][Hq][ld_keys]: keys 0 .. base + i of row i, zeros behind them
    const int32_t *gen_idx, *done;   // a decode step (both or neither): sequence b's rows land gen_idx[b] x gen_stride floats further on; nothing where
    long long gen_stride;            // done[b] != 0 or the index is outside 0 .. max_new - 1
    int ldq, q_off, B, Hq, Hkv, max_pages, ld_keys, max_new;
    float scale;
};
// max_n: an upper bound of the new rows of any sequence (the grid); page = 64, head_dim = 128, GQA group in {1, 2, 4, 8}, ld_keys % 4 == 0
int launch_attn_probs(const AttnProbsParams& p, int max_n, int kv8, hipStream_t stream);

// ---- decode.hip: the greedy finish of a step ----
struct FinishParams {
    const float* part_val;
    const int32_t* part_idx;
    int n_part, B;
    int32_t* cur_tok;
    int32_t* ctx_len;
    int32_t* done;
    int32_t* n_out;
    int32_t* out_ids;
    const int32_t* max_new_p;   // device int[B]: per-row token budget
    // early exit (emmax_session_set_stop): stop_cfg = {n_trigger, n_after}; a row is done n_after tokens after it emitted
    // the trigger id sequence.  stop_m[b] = trigger ids matched so far, stop_after[b] = tokens since the match (-1: none yet)
    const int32_t* stop_ids;
    const int32_t* stop_cfg;
    int32_t* stop_m;
    int32_t* stop_after;
    int max_out, max_ctx;
    int eos_id, pad_id;
    int is_prefill;
};
int launch_decode_finish(const FinishParams& p, hipStream_t stream);
// The bookkeeping of row b once its token is known (one thread; the greedy finish of decode.hip and the sampled finish of sample.hip both
// end here): token budget, `ctx_len`, output row (cleared at a prefill), EOS / budget / stop rule / cache end, next current token.
// lp_row (sampled finish only, else null): the row's log-probabilities beside out_ids, written at the token's place; stop_row: the row is
// done after this token whatever it is (an all-NaN logit row in a sampled step).
__device__ __forceinline__ void emmax_finish_row(const FinishParams& p, int b, int tok, float* lp_row, float lp, bool stop_row) {
    int was_done = p.done[b];
    int n = p.n_out[b];
    const int budget_n = p.max_new_p[b];
    if (!p.is_prefill && !was_done && n >= budget_n) {   // token budget already spent before this step
        was_done = 1;
        p.done[b] = 1;
    }
    if (!p.is_prefill && !was_done) p.ctx_len[b] += 1;   // the token consumed by this step now sits in the cache
    if (p.is_prefill)   // fresh sequence: clear the output row
        for (int i = 0; i < p.max_out; ++i) {
            p.out_ids[(size_t)b * p.max_out + i] = p.pad_id;
            if (lp_row) lp_row[i] = 0.f;
        }
    if (was_done) {
        tok = p.pad_id;
    } else {
        if (n < p.max_out) {
            p.out_ids[(size_t)b * p.max_out + n] = tok;
            if (lp_row) lp_row[n] = lp;
        }
        n += 1;
        p.n_out[b] = n;
        // stop on EOS, on the token budget, or when the next append would overflow the cache
        const bool budget = !p.is_prefill && n >= budget_n;
        // early exit: n_after tokens after the trigger id sequence (e.g. "POLICIES:" + the 8 action-line tokens)
        bool stop = false;
        const int n_trig = p.stop_cfg[0];
        if (n_trig > 0) {
            int aft = p.stop_after[b];
            if (aft >= 0) {
                aft += 1;
            } else {
                int mp = p.stop_m[b];
                mp = (tok == p.stop_ids[mp]) ? mp + 1 : ((tok == p.stop_ids[0]) ? 1 : 0);   // single-restart matcher
                if (mp == n_trig) {
                    aft = 0;
                    mp = 0;
                }
                p.stop_m[b] = mp;
            }
            p.stop_after[b] = aft;
            stop = aft >= 0 && aft >= p.stop_cfg[1];
        }
        if (tok == p.eos_id || budget || stop || p.ctx_len[b] + 1 >= p.max_ctx || stop_row) p.done[b] = 1;
    }
    p.cur_tok[b] = tok;
}
// ---- verify.hip: a window of guessed tokens per row through the extension pass, and the accept walk behind it ----
// cu / base of the pass and the rows' token budget; ctx_len / done / n_out / stop match / output row stay (pointers already offset to the first row)
int launch_verify_state(const PrefillState& st, int32_t* cu, int32_t* base, const int32_t* ctx_len, int32_t* max_new, int budget, hipStream_t stream);
// one block per sequence of f.B: window row i of sequence b is ids[b][i], argmax[cu[b] + i] the model's token behind it.  The walk emits
// argmax[cu[b] + i] through emmax_finish_row (f.is_prefill = 0; part_* unused) for i = 0, 1, .. while the row is not done, i + 1 < the window and
// the token equals ids[b][i + 1].  emitted[b]: tokens emitted; new_ids (may be null) [cu[b] ..]: those tokens
struct VerifyAcceptParams {
    FinishParams f;
    const int32_t *argmax, *ids, *cu;
    int P_max;
    int32_t *emitted, *new_ids;
};
int launch_verify_accept(const VerifyAcceptParams& p, hipStream_t stream);
// ---- sample.hip: seeded temperature / top-k / top-p sampling over fp32 logit rows (emmax_op_sample, include/emmax.h) ----
#define EMMAX_SAMPLE_MAX_V 32768    // entries of one row: 1024 lanes x 32 registers
struct SampleParams {
    const float* logits;        // f32 [B, ld]
    int ld, V;
    const float* temperature;   // per row: 0 = greedy (argmax, lowest id on ties)
    const int32_t* top_k;       // 0 = off
    const float* top_p;         // 1 = off
    const uint64_t* seed;
    const uint32_t* subseq;
    const int32_t* step;        // per-row Philox step
    int32_t* tok_out;           // [B]
    float* logprob_out;         // [B]: l_tok - logsumexp(l)
};
int launch_sample(const SampleParams& p, int B, hipStream_t stream);
// the finish of a SAMPLED step (sampling on, include/emmax.h: emmax_session_set_sampling): one 1024-thread block per row draws the row's
// token from its fp32 logits exactly as emmax_sample_kernel does (step = the row's n_out: its generation index) and ends in
// emmax_finish_row; done / idle rows draw nothing.  Replaces launch_decode_finish in a sampled step (same launch count).
struct SampleFinishParams {
    FinishParams f;             // rows f.B; part_val / part_idx / n_part unused
    const float* logits;        // f32 [B, ld]: complete rows of the lm-head launch this finish follows
    int ld, V;
    const float* temperature;   // [B] (as SampleParams)
    const int32_t* top_k;
    const float* top_p;
    const uint64_t* seed;
    const uint32_t* subseq;
    float* logprob;             // [B][f.max_out], beside f.out_ids
};
int launch_sample_finish(const SampleFinishParams& p, hipStream_t stream);
// the finish of a step with LOGITS PROCESSING or SCORES on (include/emmax.h: emmax_session_set_processing / emmax_session_set_scores): the
// same kernel body again, which first applies the row's repetition penalty, n-gram ban and min-new-tokens EOS ban to its fp32 logits (history
// = the row's prompt ids, then out_ids[0 .. n_out)), then draws (sampling on) or takes the argmax (sampling off: temperature null) and
// stores the row's processed scores / raw logits at its generation index when scores are bound.  Replaces the greedy or sampled finish.
#define EMMAX_MAX_NGRAM 32
struct ProcFinishParams : SampleFinishParams {
    int row0;                   // the session row of block 0 (the scores' batch index of block b is row0 + b)
    const float* penalty;       // [B] repetition penalty (1 = off); penalty / ngram / min_new null: processing off (scores only)
    const int32_t* ngram;       // [B] no_repeat_ngram_size, 0 = off, <= EMMAX_MAX_NGRAM
    const int32_t* min_new;     // [B] EOS is -inf while n_out < min_new
    const int32_t* hist;        // [B][max_prompt] the rows' prompt ids (text ids as the prefill got them)
    const int32_t* hist_len;    // [B]
    int max_prompt;
    const uint64_t* score_words;   // null: no scores.  Else device words {scores f32*, logits f32*, max_new, rows}: buffers [max_new][rows][V]
};
int launch_proc_finish(const ProcFinishParams& p, hipStream_t stream);
// the EXT form of that finish (include/emmax.h: emmax_session_set_warpers / emmax_session_set_token_rules; emmax_op_sample_ext): the token
// rules join the processors (biases before the repetition penalty, bans with the n-gram ban) and min_p / typical_p / epsilon_cutoff /
// eta_cutoff follow top-k and top-p.  Its own instantiation of the kernel body: a session that uses none of them never launches it
#define EMMAX_MAX_RULES 512         // rules of a table
#define EMMAX_MAX_RULE_IDS 16       // ids of one rule
#define EMMAX_MAX_RULE_TOTAL 8192   // ids of all rules
struct RuleTable {
    const int32_t* n;           // device word: the rule count (a session's table changes without a re-capture); null: n_host
    int n_host;
    const int32_t* off;         // [n + 1] offsets into ids; null: no rules
    const int32_t* ids;
    const int32_t* flags;       // [n] bits 0-1 kind (0 sequence_bias, 1 bad_words, 2 suppress, 3 begin_suppress), bit 2 begin-only
    const float* bias;          // [n] (bias rules)
};
struct ExtFinishParams : ProcFinishParams {
    const float *min_p, *typical_p, *eps_cut, *eta_cut;   // [B] each, 0 = off; all null: no warpers
    RuleTable rt;
    const uint32_t* rule_en;    // [B] bit k: the rules of kind k apply to the row
    // the op form (emmax_op_sample_ext): tok_out non-null -- no row state is read or written (f.is_prefill = 1, f.max_out = 0: the history is
    // hist alone, f.n_out the rows' generation index), the results go here
    int32_t* tok_out;           // [B]
    float* logprob_out;         // [B]
    float* scores_out;          // [B][V] or null
};
int launch_ext_finish(const ExtFinishParams& p, hipStream_t stream);
// the CONSTRAINED form of the EXT finish (include/emmax.h: emmax_session_set_automaton; emmax_op_sample_constrained): a token automaton over
// token classes joins the bans.  A row in state s >= 0 keeps the ids whose class bit is set in allow[s] (every other id becomes -inf with the
// n-gram ban), and the one thread that ends the row moves it to next[s][cls[tok]] (-1: the row is done after this token).  A state outside
// 0 .. n_states allows nothing.  Its own instantiation again: a session without an automaton never launches it
#define EMMAX_MAX_AUT_STATES 1024
#define EMMAX_MAX_AUT_CLASSES 256
struct ConFinishParams : ExtFinishParams {
    const uint8_t* cls;         // [V] class of every id (read as dwords where four ids of a lane's group lie below V)
    const uint32_t* allow;      // [n_states][8] bit c: class c is allowed
    const int16_t* next;        // [n_states][next_ld]
    int n_states, next_ld;
    int32_t* state;             // [B] in / out; -1: the row is unconstrained
    int32_t* state_out;         // (the op form) [B] the state after the token, state is read only; null: state is updated in place
};
int launch_con_finish(const ConFinishParams& p, hipStream_t stream);
// top-N and watched-token log-probabilities of rows of fp32 logits (include/emmax.h: emmax_op_top_logprobs / emmax_session_set_top_logprobs):
// one 1024-thread block per row, over the RAW row -- lse as emmax_sample_kernel computes it, the first n_top non-NaN entries by (value
// descending, id ascending) as (id, l - lse), and l[watch_ids[w]] - lse.
//   the op form (words null):   row b's results at top_ids / top_lp [b][n_top] and watch_lp [b][n_watch];
//   the step form (words set):  device words {top_ids, top_lp, watch_lp, n_top, n_watch, max_new}; block b is session row row0 + b and writes
//                               entry [row0 + b][t], t = n_out[b], of buffers [rows][max_new][n] -- unless the row emits nothing (not a prefill
//                               and done or out of budget) or t >= max_new.  It runs BEFORE the finish that advances n_out / done.
#ifndef EMMAX_MAX_TOP_LOGPROBS
#define EMMAX_MAX_TOP_LOGPROBS 20
#define EMMAX_MAX_WATCH_IDS 256
#endif
enum { TOPLP_W_IDS = 0, TOPLP_W_LP = 1, TOPLP_W_WATCH = 2, TOPLP_W_NTOP = 3, TOPLP_W_NWATCH = 4, TOPLP_W_MAXNEW = 5, TOPLP_WORDS = 6 };
struct TopLogprobParams {
    const float* logits;        // f32 [B, ld]
    int ld, V;
    int n_top, n_watch;         // (op form) 0 = that part is off
    int32_t* top_ids;
    float *top_lp, *watch_lp;
    const int32_t* watch_ids;   // device [n_watch], each in [0, V)
    const uint64_t* words;      // the step form, else null
    int row0, is_prefill;
    const int32_t *n_out, *done, *max_new_p;   // (step form) the rows' state, already offset to row0
};
int launch_top_logprobs(const TopLogprobParams& p, int B, hipStream_t stream);
// ---- beam.hip: beam search in the decode step (include/emmax.h, ABI 9) ----
#ifndef EMMAX_MAX_BEAMS
#define EMMAX_MAX_BEAMS 8
#endif
// per-row candidates: block b reads logits row b, writes its lse and its best 2K (acc, token) pairs, best first, at slot b (prefill form:
// block g reads the prefill's row g with score 0 and writes slot g * K)
struct BeamRowParams {
    const float* logits;        // f32 [blocks][ld]
    int ld, V, K, is_prefill;
    const float* run_score;     // [rows] running scores (not read at a prefill)
    const int32_t* done;        // [rows]: a done group's rows are skipped
    const int32_t* n_out;       // [rows]: the step's index
    float* cand_acc;            // [rows][2 EMMAX_MAX_BEAMS]
    int32_t* cand_tok;          // ... token, -1 = no candidate
    float* row_lse;             // [rows]
    const uint64_t* score_words;   // null, or the device words of emmax_session_set_scores: the raw row goes to logits[step][slot]
};
int launch_beam_rows(const BeamRowParams& p, int blocks, hipStream_t stream);
// per-group merge + HF's beam state + trace + per-row decode state + page-table gather (one wave per group)
struct BeamMergeParams {
    int K, V, is_prefill, eos_id, pad_id, max_pages, max_out, tr_ld;
    int es_mode;                // early_stopping: 0 False, 1 True, 2 "never"
    int lp_pos;                 // length_penalty > 0
    const float* pw;            // [max_out + 1]: fp32(n ** length_penalty)
    const float* cand_acc;
    const int32_t* cand_tok;
    const float* row_lse;
    float *run_score, *fin_score;
    int32_t *fin_flag, *fin_t, *fin_par, *fin_tok;   // the kept hypotheses: finished flag, the step, parent beam and token they ended with
    int32_t* grp_state;         // [groups][4]: {early-stop heuristic unsatisfied, done, next free page, -}
    int32_t *cur_tok, *ctx_len, *done, *n_out;
    const int32_t* max_new_p;
    int32_t *page_table, *spare, *copy_src, *copy_dst, *copy_ntok;
    int32_t* grp_shared;        // [groups], prefill form: the complete prompt pages every beam of the group references (DecodeAttnParams::grp_shared)
    int32_t *tr_tok, *tr_par;   // [max_out][tr_ld]
    float *tr_score, *tr_lse;
    int32_t* tc_idx;            // [max_out][2 tr_ld]
    float* tc_acc;
    int S[EMMAX_MAX_DECODE_BATCH];   // prefill form: the groups' prompt contexts
};
int launch_beam_merge(const BeamMergeParams& p, int groups, hipStream_t stream);
// the partial-page copies the merge listed, over every plane of every layer of the paged cache
struct BeamCopyParams {
    char* kv;
    long long layer_stride;     // bytes
    int n_planes, Hkv, n_pages;
    long long plane_off[4];     // bytes from the layer's base
    int plane_rb[4];            // bytes per (token, kv head) row
    const int32_t *copy_src, *copy_dst, *copy_ntok;
};
int launch_beam_copy(const BeamCopyParams& p, int rows, int n_layers, hipStream_t stream);
int launch_beam_reset(int rows, int K, float* run_score, float* fin_score, int32_t* fin_flag, int32_t* fin_t, int32_t* fin_par, int32_t* fin_tok,
                      int32_t* grp_state, int32_t* copy_src, hipStream_t stream);
int launch_beam_pages(int32_t* pt, int rows, int max_pages, int step, hipStream_t stream);
struct BeamResolveParams {
    int rows, K, max_out, max_new, tr_ld, pad_id;
    const int32_t *fin_t, *fin_par, *fin_tok, *tr_tok, *tr_par;
    const float* fin_score;
    int32_t *seq, *bidx, *len;  // [rows][max_out], [rows][max_out], [rows]
    float* score;
};
int launch_beam_resolve(const BeamResolveParams& p, hipStream_t stream);
// ---- beam.hip: sample groups (include/emmax.h: emmax_session_set_sample_groups) ----
// the fork of G prefilled groups into G x N rows (one wave per group): the page-table rows g N + j (the prompt's complete pages by reference
// to row g N's, every later page the row's own), the rows' fresh decode state, and the copy list of the prompt's partial page
// (launch_beam_copy consumes it: src = -1 where nothing is copied)
struct GroupForkParams {
    int N, max_pages;
    int32_t *page_table, *copy_src, *copy_dst, *copy_ntok;
    RowState st;
    int32_t* grp_shared;             // [groups]: the complete prompt pages the group's rows share (DecodeAttnParams::grp_shared)
    int S[EMMAX_MAX_DECODE_BATCH];   // the groups' prompt contexts
};
int launch_group_fork(const GroupForkParams& p, int groups, hipStream_t stream);
// rows[g N + j] = rows[g] for every group g and sample j, in place (rows of row_bytes bytes, a multiple of 4): destination rows overlap
// source rows for g >= 1, so every thread owns a column and walks the groups from the highest down
int launch_group_bcast(void* rows, long long row_bytes, int groups, int N, hipStream_t stream);
// the prompt ids of rows 0 .. B of a prefill (ids [B][P_max]) into dst [B][max_prompt], their lengths into dst_len
struct HistParams {
    const int32_t* ids;
    int P_max, B, max_prompt;
    int32_t *dst, *dst_len;
    int len[EMMAX_MAX_DECODE_BATCH];
};
int launch_hist_fill(const HistParams& h, hipStream_t stream);
int launch_set_tokens(const RowState& rows, const int32_t* toks, int B, int budget, hipStream_t stream);


// ---- decode_km.hip: batch 3-16 projections with K <= 4096 on MFMA, K split across the waves, activations as register fragments ----
// p.W = the km copy (launch_repack_km: fragment-major tiles; perm 1 / 2 = the row orders that put the qkv RoPE pairs / the
// (gate, up) pairs inside one 16-row tile).  -2: shape outside the kernel, the caller falls back to launch_decode_mfma.
int launch_repack_km(const void* src, int ld, void* dst, int N, int K, int perm, int head_dim, hipStream_t stream);
int launch_decode_km(int mode, const GemvParams& p, int B, hipStream_t stream, int* grid_out = nullptr, const ProjGeom* geom = nullptr);
// The block-scaled copies (WFmt::mx) of a row-major bf16 matrix in the km row order (perm / head_dim as launch_repack_km): blocks of 32 consecutive k of
// one row share the exponent e = floor(log2(amax)) - 2 clamped to [-127, 127] (code e + 127; an all-zero block: code 127); the scale stream is one dword
// of four codes per (tile, row), in the tiles' order.  N % 16 == 0, K % 128 == 0, ld % 8 == 0.  launch_dequant_mx writes the values the copy holds back
// as bf16 rows (exact), each at the source row the permutation took it from.
//   PW_MX4 (OCP MX v1.0 MXFP4): elements w / 2^e rounded to nearest even onto +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating.  A tile = 16 rows x 128 k in
//     1 KiB, lane-major (emmax_decode_km_kernel).
//   PW_MX6 (OCP MXFP6 e2m3; include/emmax.h pins the format): onto +-{0, 0.125 .. 0.875, 1 .. 1.875, 2 .. 3.75, 4 .. 7.5}, saturating.  A tile = 1536 B:
//     lane (row r, block g) = 16 g + r owns the 32 elements of ONE scale block as six dwords (element i in bits [6 i, 6 i + 6)): dwords 0-3 at byte
//     16 lane of the tile's first KiB, dwords 4-5 at byte 8 lane of the 512 B behind it (both loads of a wave are contiguous).
// -1: a shape outside the rules, or a format that is not block-scaled
int launch_quant_mx(int wfmt, const void* src, int ld, void* tiles, void* codes, int N, int K, int perm, int head_dim, hipStream_t stream);
int launch_dequant_mx(int wfmt, const void* tiles, const void* codes, void* dst, int ld, int N, int K, int perm, int head_dim, hipStream_t stream);
bool decode_km_enabled();
int decode_km_init();   // raise the dynamic-LDS limit of every instantiation (call once, outside graph capture)
// decode_kmp.hip: batch 17-32 (two batch tiles per weight tile, the K slice in phases), bf16 weights, same copies; launch_decode_km routes there
int launch_decode_kmp(int mode, const GemvParams& p, int B, hipStream_t stream, int* grid_out = nullptr, const ProjGeom* geom = nullptr);
int decode_kmp_init();

// ---- decode_mfma.hip: small-batch (B >= 3) projections on MFMA over the fragment-major weight copy ----
int launch_repack_fm(const void* src, int ld, void* dst, int N, int K, hipStream_t stream);
int launch_quant_fm8(const void* src, int ld, void* dst, float* scales, int N, int K, hipStream_t stream, int perm = 0, int head_dim = 0);   // fp8 e4m3 + per-row scale
int launch_quant_rm8(const void* src, int ld, void* dst, float* scales, int N, int K, hipStream_t stream);   // same values, rows in the GEMV's span order
int launch_decode_mfma(int mode, const GemvParams& p, int B, hipStream_t stream, int* grid_out = nullptr, const ProjGeom* geom = nullptr);   // p.W = fragment-major copy
int decode_mfma_init();
#define EMMAX_MFMA_MIN_BATCH 3
