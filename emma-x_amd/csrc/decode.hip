// decode.hip -- the LDS-staged dot-product GEMV of the autoregressive decode step (HBM-bound, one token per sequence) and the step's small
// kernels.  Replaces the projections of HF `LlamaDecoderLayer` at q_len == 1 + one greedy step of `GenerationMixin.generate`
// (cached branch of prismatic/extern/hf/modeling_prismatic.py:325-341; loop invoked at :519 and
// prismatic/models/vlms/prismatic.py:659-663).
//
// The staged GEMV: weights bf16 [N,K] row-major (or the e4m3 row copy of emmax_quant_rm8_kernel) are read exactly once with 16-byte
// non-temporal loads, many loads in flight per lane, straight to VGPRs (no LDS round trip for data that is not shared); the B
// activation vectors are staged once per block in LDS (bf16) and read back with broadcast-free ds_read_b128; products go through
// v_dot2c_f32_bf16 with fp32 accumulation; rows are reduced across the wave.
// Fusions (no activation round trip through HBM beyond one bf16 vector per stage):
//   qkv    : RMSNorm prologue  -> GEMV -> RoPE (rotate-half) -> q buffer / paged K,V cache append
//   oproj  : merge of the attention split partials -> GEMV -> + residual (in place)
//   gateup : RMSNorm prologue  -> GEMV over 16-row interleaved (gate,up) -> SiLU(gate)*up
//   down   : GEMV -> + residual (in place)
//   lmhead : final RMSNorm prologue -> GEMV -> per-block greedy argmax (logits never reach HBM)
// It serves the fused modes at batch 1-2 (bf16 shapes decode_ks.hip does not take, the tuning switch ks = 0, the fp8 rows) and plain rows
// up to batch 8 (emmax_op_gemv).  The other projection families: decode_ks.hip (batch 1-2, K-split), decode_km.hip / decode_kmp.hip and
// decode_mfma.hip (MFMA, batch >= 3 and fp8); their shared epilogues: decode_epilogue.h; the decode attention: decode_attn.hip.
// Also here: the e4m3 row quantiser, the embedding gather, the greedy finish of a step and emmax_set_tokens_kernel.
// All step-varying state (positions, current tokens, done flags) is read from device memory -> hipGraph-capturable.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "decode_epilogue.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// GEMV.  Persistent blocks of 512 threads = 8 waves; block b owns a contiguous range of row GROUPS, its waves interleave
// inside the range.  A group is 2 weight rows: (row d, row d+hd/2) of one head for QKV, (gate_i, up_i) for GATEUP, two
// consecutive rows otherwise.  The activation prologue (RMSNorm / attention-split merge + staging into LDS) runs once
// per block; a wave keeps one block of 2 rows x 8 x 16 B of weights in flight: the block is consumed, its successor (the
// next 8 steps of the group, or the head of the next group) is requested, and only then is a finished group reduced;
// the very first block is requested before the prologue (qkv / o-proj: right behind the prologue's own loads).
// (tools/gemv_sweep.hip: this structure streams 180 MB at ~6.1 TB/s, 97 % of a read-only kernel with the same pattern.)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GW = 8;   // waves per GEMV block

// row-major bf16 [N, ld] -> fp8 e4m3 (OCP) rows of K bytes in the GEMV's span order + one fp32 scale per row (amax / 448, the
// values of emmax_quant_fm8_kernel).  A row is cut into spans of 128 chunks of 8 elements (the last one shorter: nc chunks, nc
// even); the 16-byte granule l of a span holds chunk l (bytes 0-7) and chunk nc/2 + l (bytes 8-15).  One block per row; K % 16 == 0.
__global__ __launch_bounds__(256) void emmax_quant_rm8_kernel(const bf16_t* __restrict__ src, int ld, uint8_t* __restrict__ dst,
                                                             float* __restrict__ scales, int N, int K) {
    const int n = blockIdx.x, tid = threadIdx.x;
    __shared__ float red[4];
    const bf16_t* row = src + (size_t)n * ld;
    float amax = 0.f;
    for (int c = tid; c < K / 8; c += 256) {
        const u32x4_t v = *(const u32x4_t*)(row + c * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fmaxf(fabsf(bf_lo(v[j])), fabsf(bf_hi(v[j]))));
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
    if (tid == 0) scales[n] = scale;
    for (int c = tid; c < K / 8; c += 256) {
        const u32x4_t v = *(const u32x4_t*)(row + c * 8);
        const int sp = c >> 7, ci = c & 127, nc2 = min(128, K / 8 - sp * 128) >> 1;
        const int l = ci < nc2 ? ci : ci - nc2, half = ci < nc2 ? 0 : 1;
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf_lo(v[0]) / scale, bf_hi(v[0]) / scale, lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf_lo(v[1]) / scale, bf_hi(v[1]) / scale, lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf_lo(v[2]) / scale, bf_hi(v[2]) / scale, hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf_lo(v[3]) / scale, bf_hi(v[3]) / scale, hi, true);
        u32x2_t w = {(uint32_t)lo, (uint32_t)hi};
        *(u32x2_t*)(dst + (size_t)n * K + sp * 1024 + l * 16 + half * 8) = w;
    }
}

// B <= 2: two resident blocks per CU (<= 128 VGPRs); larger batches keep more accumulators and run one block per CU
#ifdef DECODE_LAB_TRACE
__device__ unsigned long long g_gemv_trace[1024 * 8];   // [block][stamp]: s_memrealtime (100 MHz) of wave 0
#define GEMV_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_gemv_trace[blockIdx.x * 8 + (k)] = wall_clock64(); } while (0)
#else
#define GEMV_STAMP(k) do { } while (0)
#endif
// F8 > 0 (B <= 2): the weights are the row-major e4m3 copy of emmax_quant_rm8_kernel above + one fp32 scale per row.  A 16-byte
// load is then 16 weights: a step covers a SPAN of up to 128 activation chunks (1024 elements), and lane l of the span holds the
// weights of chunks (l, nc/2 + l) of it (nc = chunks in the span), so that the two LDS reads of a step are each consecutive
// over the lanes, like the bf16 path's one.  Rows are half as long in bytes, so the block shape follows the matrix (the launcher
// picks): F8 = 3 -- groups of FOUR rows (two pairs) x 4 steps, the bf16 path's 16 KiB per wave in flight, for matrices with
// enough rows to give every wave a group (qkv, gate/up, lm-head); F8 = 1 / 2 -- two rows x 4 / 12 steps for the 4096-row
// matrices, whose 2048 pairs are one per wave of a one-block-per-CU grid: the WHOLE pair is requested up front (o-proj: K = 4096
// is four spans; down: K = 11008 is eleven -- 96 weight registers, which one block per CU affords).  De-quantisation is exact (e4m3 fits bf16:
// v_cvt_scalef32_pk_bf16_fp8 with scale 1, two values per instruction, ~4.5 clocks), the products accumulate in fp32 and the row
// scale multiplies the reduced sum.
template <int B, int MODE, bool NORM, bool XATTN = false, int F8 = 0>
__global__ __launch_bounds__(GW * 64, (B <= 2 && F8 != 1 && F8 != 2 ? 4 : 2)) void emmax_decode_gemv_kernel(GemvParams p) {
    GEMV_STAMP(0);
    constexpr bool FP8 = F8 > 0;
    static_assert(!FP8 || B <= 2, "the fp8 GEMV serves batch 1-2");
    constexpr int NR = F8 == 3 ? 4 : 2;            // weight rows per group
    constexpr int NP = NR / 2;                     // row PAIRS per group (the epilogues work on pairs)
    constexpr int U = F8 == 2 ? 12 : F8 ? 4 : 8;   // 16-byte loads per row per block (bf16: 8 * 64 lanes * 8 elements = 4096 elements)
    constexpr int NT = GW * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4_t* xs = (u32x4_t*)smem;   // [B][KC/8 + 1] 16-byte chunks; chunk nch of a row is zero (lanes past the end of K read it)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bf16_t* __restrict__ W = (const bf16_t*)p.W;
    const int K = p.K;
    const int KC = p.kc;   // elements per K phase (multiple of 8)
    const bool multi_phase = KC < K;
    const int XS = (KC >> 3) + 1;   // chunks per staged row

    // contiguous share of the groups for this block
    const int G = gridDim.x, bid = blockIdx.x;
    const int gq = p.n_groups / G, gr = p.n_groups % G;
    const int g_lo = bid * gq + min(bid, gr), g_hi = g_lo + gq + (bid < gr ? 1 : 0);
    const int rounds = (g_hi - g_lo + GW - 1) / GW;

    auto pair_rows = [&](int g, int& r0, int& r1) {   // g: pair index (= group index on the bf16 path)
        if (MODE == GEMV_QKV) {
            const int half = p.head_dim >> 1;
            const int hb = g / half, d = g - hb * half;
            r0 = hb * p.head_dim + d;
            r1 = r0 + half;
        } else if (MODE == GEMV_GATEUP) {
            r0 = (g >> 4) * 32 + (g & 15);
            r1 = r0 + 16;
        } else {
            r0 = 2 * g;
            r1 = min(2 * g + 1, p.n_rows - 1);
        }
    };

    // The wave's work is a linear sequence of 8-step blocks: for every round (group) x K phase x 512-chunk block.
    // A step = one 16-byte load per lane per row.  The producer cursor runs exactly one block ahead of the consumer:
    // once the current block is consumed, the next one is requested into the same registers (sixteen loads back to back),
    // across group and phase boundaries.
    const int n_phase = (K + KC - 1) / KC;
    struct Cursor { int rd, ph, blk; };
    auto phase_nch = [&](int ph) { return min(KC, K - ph * KC) >> 3; };           // 16-byte chunks in a phase
    auto phase_nblk = [&](int ph) { return FP8 ? ((phase_nch(ph) + 127) / 128 + U - 1) / U : (phase_nch(ph) + 64 * U - 1) / (64 * U); };
    auto advance = [&](Cursor& c) {
        if (++c.blk >= phase_nblk(c.ph)) {
            c.blk = 0;
            if (++c.ph >= n_phase) { c.ph = 0; ++c.rd; }
        }
    };
    u32x4_t wr[NR][U];
    const u32x4_t* w0p = nullptr;   // row pointers of the producer's current (group, phase)
    const u32x4_t* w1p = nullptr;
    const u32x4_t* w8p[NR];         // fp8 rows
#pragma unroll
    for (int r = 0; r < NR; ++r) w8p[r] = nullptr;
    auto producer_rows = [&](const Cursor& c) {
        const int g = g_lo + c.rd * GW + wave;
        int r0, r1;
        if (FP8) {   // (single phase; ldw = bytes per row)
            const uint8_t* W8 = (const uint8_t*)p.W;
            const int gg = min(g, g_hi - 1);
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                pair_rows(min(gg * NP + i, p.n_pairs - 1), r0, r1);
                w8p[2 * i] = (const u32x4_t*)(W8 + (size_t)r0 * p.ldw);
                w8p[2 * i + 1] = (const u32x4_t*)(W8 + (size_t)r1 * p.ldw);
            }
            return;
        }
        pair_rows(min(g, g_hi - 1), r0, r1);
        w0p = (const u32x4_t*)(W + (size_t)r0 * p.ldw + c.ph * KC);
        w1p = (const u32x4_t*)(W + (size_t)r1 * p.ldw + c.ph * KC);
    };
    // FP8: chunks of span s = step u of block blk, and whether this lane holds weights of it
    auto span_nc = [&](int s) { return min(128, (K >> 3) - s * 128); };
    auto issue_step = [&](const Cursor& c, int u, bool active) {
        if constexpr (FP8) {
            const int sp = c.blk * U + u;
            const bool ok = active && lane < (span_nc(sp) >> 1);
            const int at = sp * 64 + lane;
#pragma unroll
            for (int r = 0; r < NR; ++r) wr[r][u] = ok ? ld_nt(w8p[r] + at) : (u32x4_t){0u, 0u, 0u, 0u};
        } else {
            const int ch = c.blk * 64 * U + u * 64 + lane;
            const bool ok = active && ch < phase_nch(c.ph);
            wr[0][u] = ok ? ld_nt(w0p + ch) : (u32x4_t){0u, 0u, 0u, 0u};
            wr[1][u] = ok ? ld_nt(w1p + ch) : (u32x4_t){0u, 0u, 0u, 0u};
        }
    };

    // ---- head of the weight stream: it does not depend on x.  UNCONDITIONAL loads (clamped addresses; lanes and waves past
    // the end fetch a valid row again and meet the zero chunk of x), so that hipcc can count them: the prologue's own loads
    // are requested FIRST where they are a fixed handful, and waited for with vmcnt(16) while the 64 MB first burst of the
    // chip is still landing -- loads return in order, so x queued BEHIND the burst arrived ~10 us into the launch ----
    Cursor P = {0, 0, 0}, Cc = {0, 0, 0};
    const int my_rounds = (g_lo + wave < g_hi) ? (g_hi - g_lo - wave + GW - 1) / GW : 0;   // groups this wave really owns
    auto issue_head = [&](bool counted) {
        producer_rows(P);
        const int nch0 = phase_nch(0);
        if (counted && FP8) {   // (lanes past a span's end re-read the row's last granule and meet the zero chunk of x)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int at = min(u * 64 + lane, (nch0 >> 1) - 1);
#pragma unroll
                for (int r = 0; r < NR; ++r) wr[r][u] = ld_nt(w8p[r] + at);
            }
        } else if (counted) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ch = min(u * 64 + lane, nch0 - 1);
                wr[0][u] = ld_nt(w0p + ch);
                wr[1][u] = ld_nt(w1p + ch);
            }
        } else {   // nothing is waited for by count behind these: the predicated form (it keeps hipcc's loop shape at B = 2)
#pragma unroll
            for (int u = 0; u < U; ++u) issue_step(P, u, my_rounds > 0);
        }
        advance(P);
    };
    const bool one_pass = NORM && !XATTN && !multi_phase && (K >> 3) <= NT;
    // x first pays for the qkv projection only (-0.9 us); gate/up and lm-head lose 1.5 us with it, the plain rows of the down
    // projection gain nothing.
    // The o-proj prologue (XATTN: merge of the attention split partials) also goes first: with every load of a chunk's merge
    // requested up front (branch-free, split count as a template argument -- only affordable while the weight block is not
    // occupying 64 registers) it is one round trip of ~1 us; as a loop BEHIND the weight stream it was sixteen dependent
    // round trips, ~5 of the 11 us of the launch.
    // (Tried and removed: plain rows staged first as one four-chunk burst per thread -- next to the 64-register weight head it
    // spilled 44-84 registers at the 128-VGPR cap of two blocks per CU.)
    // fp8: every one-pass prologue goes first -- the first burst is most of the matrix, the refills cannot go out before x is
    // staged, and x requested behind the burst arrived 7 us into a 19 us gate/up launch (tools/gemv_lab.hip)
    const bool head_first = !((one_pass && (MODE == GEMV_QKV || FP8)) || XATTN);
    if (head_first) issue_head(false);

    // chunk c (8 elements) of activation row b of a NORM mode: from the fp32 residual stream when the step keeps one (GemvParams::h32;
    // rounded to bf16 here, once per read -- decode_ks.hip, the product path at these batches, keeps statistics and x g in fp32)
    auto ld_x8 = [&](int b, int c) -> u32x4_t {
        if (p.h32) return f32x8_to_bf16(ld_f32x8(p.h32 + (size_t)b * p.ldh + (size_t)c * 8));
        return *((const u32x4_t*)((const bf16_t*)p.x + (size_t)b * p.ldx) + c);
    };
    // ---- RMSNorm statistics ----
    float rstd[B];
    // single-pass prologue: when the whole row fits one 16-byte chunk per thread, x and the norm weight are read ONCE
    // (both loads issued together), the statistics come from registers and the normalised row goes straight to LDS --
    // one L2 round trip instead of two on the critical path of every qkv / gate-up / lm-head launch
    if (one_pass) {
        __shared__ float red1p[GW][B];
        const bool mine = tid < (K >> 3);
        const int ct = min(tid, (K >> 3) - 1);
        u32x4_t xv[B];
        const u32x4_t wv = *((const u32x4_t*)p.norm_w + ct);
#pragma unroll
        for (int b = 0; b < B; ++b) xv[b] = ld_x8(b, ct);
        if (!head_first) issue_head(true);
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[b][j] = mine ? xv[b][j] : 0u;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = bf_lo(xv[b][j]), bb = bf_hi(xv[b][j]);
                ss += a * a + bb * bb;
            }
            ss = wave_sum(ss);
            if (lane == 0) red1p[wave][b] = ss;
        }
        GEMV_STAMP(5);
        __syncthreads();
        GEMV_STAMP(6);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < GW; ++w) t += red1p[w][b];
            rstd[b] = rsqrtf(t / (float)K + p.eps);
            if (mine) {
                u32x4_t v = xv[b];
#pragma unroll
                for (int j = 0; j < 4; ++j) {   // one v_cvt_pk_bf16_f32 per rounding of a pair
                    const uint32_t r = pack_bf16x2(bf_lo(v[j]) * rstd[b], bf_hi(v[j]) * rstd[b]);
                    v[j] = pack_bf16x2(bf_lo(r) * bf_lo(wv[j]), bf_hi(r) * bf_hi(wv[j]));
                }
                xs[b * XS + tid] = v;
            }
            if (tid == NT - 1) xs[b * XS + (K >> 3)] = (u32x4_t){0u, 0u, 0u, 0u};
        }
    } else if (NORM) {
        __shared__ float red[GW][B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            float ss = 0.f;
            for (int c = tid; c < (K >> 3); c += NT) {
                const u32x4_t v = ld_x8(b, c);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a = bf_lo(v[j]), bb = bf_hi(v[j]);
                    ss += a * a + bb * bb;
                }
            }
            ss = wave_sum(ss);
            if (lane == 0) red[wave][b] = ss;
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < B; ++b) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < GW; ++w) t += red[w][b];
            rstd[b] = rsqrtf(t / (float)K + p.eps);
        }
    }

    // stage x[:, kc0 : kc0 + 8*nch] into LDS (normalised if NORM, merged from the attention partials if XATTN)
    auto stage_x = [&](int kc0, int nch, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;   // the call in front of the main loop (no weight block live yet)
        if (!XATTN && !NORM) {
            // plain rows (down projection: 22 KB per row): four loads in flight per thread, then the LDS writes
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const u32x4_t* xr = (const u32x4_t*)((const bf16_t*)p.x + (size_t)b * p.ldx + kc0);
                for (int c0 = tid; c0 < nch; c0 += 4 * NT) {
                    u32x4_t v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (c0 + j * NT < nch) ? *(xr + c0 + j * NT) : (u32x4_t){0u, 0u, 0u, 0u};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j * NT < nch) xs[b * XS + c0 + j * NT] = v[j];
                }
                if (tid == NT - 1) xs[b * XS + nch] = (u32x4_t){0u, 0u, 0u, 0u};
            }
            return;
        }
        if (XATTN) {
            // chunk cg = head (cg>>4), elements (cg&15)*8..+8 of the split partials.  A thread's FIRST chunk is merged with
            // every load in flight at once (needs ~60 registers: before the weight block exists); the weight stream is
            // requested right behind it; any further chunk (K > 4096) takes the low-register loop.
            auto merge_at = [&](int c, int b, bool fast) {
                const int cg = (kc0 >> 3) + c;
                const float* pp = p.attn_part + (size_t)(b * p.Hq + (cg >> 4)) * p.nsplit * EMMAX_PSTRIDE;
                const int d0 = (cg & 15) * 8;
                // 8 splits is what decode_attn_nsplit gives at batch 1-2 for every head count up to 32
                return (fast && p.nsplit == 8) ? attn_merge_chunk<8, 4>(pp, d0) : attn_merge_chunk_loop(pp, d0, p.nsplit);
            };
            if (tid < nch) {
#pragma unroll
                for (int b = 0; b < B; ++b) xs[b * XS + tid] = merge_at(tid, b, FIRST);
            }
            if (FIRST) {
                __builtin_amdgcn_sched_barrier(0);
                issue_head(true);
                __builtin_amdgcn_sched_barrier(0);
            }
            for (int c = tid + NT; c < nch; c += NT)
#pragma unroll
                for (int b = 0; b < B; ++b) xs[b * XS + c] = merge_at(c, b, false);
            if (tid == NT - 1)
#pragma unroll
                for (int b = 0; b < B; ++b) xs[b * XS + nch] = (u32x4_t){0u, 0u, 0u, 0u};
            return;
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const u32x4_t* xr = (const u32x4_t*)((const bf16_t*)p.x + (size_t)b * p.ldx + kc0);
            for (int c = tid; c < nch; c += NT) {
                u32x4_t v = NORM ? ld_x8(b, (kc0 >> 3) + c) : xr[c];
                if (NORM) {
                    const u32x4_t wv = *((const u32x4_t*)((const bf16_t*)p.norm_w + kc0) + c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // HF LlamaRMSNorm: fp32 normalise -> downcast -> * weight (-> downcast)
                        const float a = bf2f(f2bf(bf_lo(v[j]) * rstd[b])) * bf_lo(wv[j]);
                        const float bb = bf2f(f2bf(bf_hi(v[j]) * rstd[b])) * bf_hi(wv[j]);
                        v[j] = pack_bf16x2(a, bb);
                    }
                }
                xs[b * XS + c] = v;
            }
            if (tid == NT - 1) xs[b * XS + nch] = (u32x4_t){0u, 0u, 0u, 0u};
        }
    };
    if (!one_pass) stage_x(0, phase_nch(0), std::true_type{});
    GEMV_STAMP(1);
    __syncthreads();
    GEMV_STAMP(2);

    // LMHEAD: running best over this wave's rows
    float best[B];
    int besti[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        best[b] = -INFINITY;
        besti[b] = 0x7fffffff;
    }
    float acc[NR][B];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int b = 0; b < B; ++b) acc[r][b] = 0.f;

    float red[NR][B];
    // Epilogue operands are fetched when a group STARTS, not when its dot products are done: the old residual values (RESID)
    // and the row's position / page id / cos-sin pair (QKV) are dependent global loads (~0.7-1.5 us from L2) that would
    // otherwise sit at the tail of every group with the wave's weight ring idle behind them.  Lane b serves batch row b.
    const int eb = lane < B ? lane : 0;
    int pre_pos = 0, pre_pg = 0;
    float pre_a[NP], pre_b[NP];                          // RESID: h[r0], h[r1];  QKV: cos, sin
    float wsc[NR];                                       // FP8: the group's row scales
#pragma unroll
    for (int i = 0; i < NP; ++i) pre_a[i] = pre_b[i] = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) wsc[r] = 1.f;
    if (MODE == GEMV_QKV) qkv_row_pos(p, eb, pre_pos, pre_pg);
    auto prefetch_epilogue = [&](int rd) {
        const int g = g_lo + rd * GW + wave;
        if (g >= g_hi) return;
        if constexpr (FP8) {   // every lane: the lm-head compares on all of them
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                int r0, r1;
                pair_rows(min(g * NP + i, p.n_pairs - 1), r0, r1);
                wsc[2 * i] = p.wscale[r0];
                wsc[2 * i + 1] = p.wscale[r1];
            }
        }
        if (lane >= B) return;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int pg = FP8 ? min(g * NP + i, p.n_pairs - 1) : g;
            if (MODE == GEMV_RESID) {
                int r0, r1;
                pair_rows(pg, r0, r1);
                pre_a[i] = resid_fetch(p, eb, r0, p.h32 != nullptr);
                pre_b[i] = resid_fetch(p, eb, r1, p.h32 != nullptr);
            } else if (MODE == GEMV_QKV) {
                const int half = p.head_dim >> 1, hb = pg / half;
                qkv_rope_fetch(p, pre_pos, hb, pg - hb * half, pre_a[i], pre_b[i]);
            }
        }
    };
    // every wave of the block walks the same number of rounds (block-uniform barriers in the multi-phase case)
    while (Cc.rd < rounds) {
        const bool valid = Cc.rd < my_rounds;
        if (Cc.blk == 0 && Cc.ph == 0) prefetch_epilogue(Cc.rd);
        if (multi_phase && Cc.blk == 0 && (Cc.rd != 0 || Cc.ph != 0)) {   // new phase: restage x (loads keep flying)
            __syncthreads();
            stage_x(Cc.ph * KC, phase_nch(Cc.ph), std::false_type{});
            __syncthreads();
        }
        const bool p_active = P.rd < my_rounds;
        if (P.blk == 0) producer_rows(P);
        const int nch = phase_nch(Cc.ph);
        if constexpr (FP8) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int sp = Cc.blk * U + u, base = sp * 128;
                if (valid && base < nch) {   // wave-uniform
                    const int nc2 = span_nc(sp) >> 1;
                    const bool l_ok = lane < nc2;
                    const int cc0 = l_ok ? base + lane : nch, cc1 = l_ok ? base + nc2 + lane : nch;   // past the end: the zero chunk
                    u32x4_t xa[B], xb[B];
#pragma unroll
                    for (int b = 0; b < B; ++b) {
                        xa[b] = xs[b * XS + cc0];
                        xb[b] = xs[b * XS + cc1];
                    }
#pragma unroll
                    for (int r = 0; r < NR; ++r) {
                        // dwords 0-1 of the granule: the 8 weights of chunk cc0, dwords 2-3: of chunk cc1 (emmax_quant_rm8_kernel)
                        uint32_t w[8];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            w[2 * j] = fp8x2_to_bf16x2<false>(wr[r][u][j]);
                            w[2 * j + 1] = fp8x2_to_bf16x2<true>(wr[r][u][j]);
                        }
#pragma unroll
                        for (int b = 0; b < B; ++b) {
                            float a = acc[r][b];
                            a = dot2_bf16(w[0], xa[b][0], a);
                            a = dot2_bf16(w[1], xa[b][1], a);
                            a = dot2_bf16(w[2], xa[b][2], a);
                            a = dot2_bf16(w[3], xa[b][3], a);
                            a = dot2_bf16(w[4], xb[b][0], a);
                            a = dot2_bf16(w[5], xb[b][1], a);
                            a = dot2_bf16(w[6], xb[b][2], a);
                            a = dot2_bf16(w[7], xb[b][3], a);
                            acc[r][b] = a;
                        }
                    }
                }
            }
        } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = Cc.blk * 64 * U + u * 64 + lane;
            if (valid && Cc.blk * 64 * U + u * 64 < nch) {   // wave-uniform
                const int cc = min(c, nch);   // past the end: the zero chunk
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    const u32x4_t xv = xs[b * XS + cc];
#pragma unroll
                    for (int r = 0; r < NR; ++r) {
                        float a = acc[r][b];
                        a = dot2_bf16(wr[r][u][0], xv[0], a);
                        a = dot2_bf16(wr[r][u][1], xv[1], a);
                        a = dot2_bf16(wr[r][u][2], xv[2], a);
                        a = dot2_bf16(wr[r][u][3], xv[3], a);
                        acc[r][b] = a;
                    }
                }
            }
        }
        }
        // refill the whole block AFTER it is consumed: sixteen requests back to back (two rows x 8 KiB, consecutive addresses).
        // This is the order hipcc picked by itself at B = 1 and it is the fast one -- the per-step interleaving it chose at
        // B = 2 (refill of step u between the dot products of steps u and u+1, counted waits) is 2 us slower per gate/up launch
#pragma unroll
        for (int u = 0; u < U; ++u) issue_step(P, u, p_active);
#ifdef DECODE_LAB_TRACE
        if (Cc.rd == 0 && Cc.ph == 0 && Cc.blk == 0) GEMV_STAMP(3);
#endif
        const bool group_done = (Cc.ph == n_phase - 1) && (Cc.blk == phase_nblk(Cc.ph) - 1);
        const int g = g_lo + Cc.rd * GW + wave;
        advance(Cc);
        advance(P);
        if (!group_done || !valid) continue;

#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const float t = wave_sum(acc[r][b]);
                acc[r][b] = 0.f;
                red[r][b] = FP8 ? t * wsc[r] : t;
            }

#pragma unroll
        for (int i = 0; i < NP; ++i) {
        const int pg = FP8 ? g * NP + i : g;   // the pair's index
        if (FP8 && pg >= p.n_pairs) continue;
        float red0[B], red1[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            red0[b] = red[2 * i][b];
            red1[b] = red[2 * i + 1][b];
        }
        int r0, r1;
        pair_rows(pg, r0, r1);
        if (MODE == GEMV_PLAIN) {
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (lane == b) {   // (here and below: a store's address is formed before its value -- the order decides hipcc's schedule)
                    bf16_t* y0 = (bf16_t*)p.y + (size_t)b * p.ldy + r0;
                    *y0 = f2bf(red0[b]);
                    if (2 * pg + 1 < p.n_rows) {
                        bf16_t* y1 = (bf16_t*)p.y + (size_t)b * p.ldy + r1;
                        *y1 = f2bf(red1[b]);
                    }
                }
        } else if (MODE == GEMV_RESID) {
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (lane == b) {
                    if (p.h32) {   // fp32 master copy of the residual stream; the bf16 rows below mirror it
                        float* hq = p.h32 + (size_t)b * p.ldh;
                        hq[r0] = pre_a[i] + red0[b];
                        if (2 * pg + 1 < p.n_rows) hq[r1] = pre_b[i] + red1[b];
                    }
                    bf16_t* hp = (bf16_t*)p.y + (size_t)b * p.ldy;
                    bf16_t* h0 = hp + r0;
                    *h0 = f2bf(pre_a[i] + red0[b]);
                    if (2 * pg + 1 < p.n_rows) {
                        bf16_t* h1 = hp + r1;
                        *h1 = f2bf(pre_b[i] + red1[b]);
                    }
                }
        } else if (MODE == GEMV_GATEUP) {
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (lane == b) swiglu_finish<false>(p, b, pg, red0[b], red1[b]);
        } else if (MODE == GEMV_QKV) {
            const int hd = p.head_dim, half = hd >> 1;
            const int hb = pg / half, d = pg - hb * half;
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (lane == b) {
                    const int pos = pre_pos;
                    // linear outputs are bf16 activations in the reference; RoPE acts on those
                    const float x0 = bf2f(f2bf(red0[b])), x1 = bf2f(f2bf(red1[b]));
                    if (hb < p.Hq + p.Hkv) {
                        const float cs = pre_a[i], sn = pre_b[i];
                        const bf16_t y0 = f2bf(x0 * cs - x1 * sn), y1 = f2bf(x1 * cs + x0 * sn);
                        if (hb < p.Hq) {
                            bf16_t* q = (bf16_t*)p.y + (size_t)b * p.ldy + hb * hd;
                            q[d] = y0;
                            *(q + d + half) = y1;
                        } else {
                            const int pgid = pre_pg;
                            bf16_t* kc = gemv_kv_row(p, false, b, pgid, pos, hb - p.Hq);
                            kc[d] = y0;
                            *(kc + d + half) = y1;
                        }
                    } else {
                        const int pgid = pre_pg;
                        bf16_t* vc = gemv_kv_row(p, true, b, pgid, pos, hb - p.Hq - p.Hkv);
                        bf16_t* v0 = vc + d;
                        *v0 = f2bf(x0);
                        bf16_t* v1 = vc + d + half;
                        *v1 = f2bf(x1);
                    }
                }
        } else if (MODE == GEMV_LMHEAD) {
#pragma unroll
            for (int b = 0; b < B; ++b) {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int row = r == 0 ? r0 : r1;
                    if (r == 1 && 2 * pg + 1 >= p.n_rows) continue;
                    const float v = r == 0 ? red0[b] : red1[b];
                    lmhead_take(v, row, best[b], besti[b]);
                    if (p.logits_out && lane == 0) p.logits_out[(size_t)b * p.n_rows + row] = v;
                }
            }
        }
        }
    }

    GEMV_STAMP(4);
    if (MODE == GEMV_LMHEAD) {
        // block best; first index wins ties (torch.argmax semantics); one partial per block
        __shared__ float bv[GW][B];
        __shared__ int bi[GW][B];
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < B; ++b) {
                bv[wave][b] = best[b];
                bi[wave][b] = besti[b];
            }
        }
        __syncthreads();
        // thread b: the eight waves' candidates of batch row b, starting from wave 0's
        if (tid < B) {
            const auto slot = [&](int k) { return (k + 1) * B + tid; };
            lmhead_col_finish(p, B, tid, &bv[0][0], &bi[0][0], GW - 1, slot, bv[0][tid], bi[0][tid]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// h[b] = E[cur_tok[b]]
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emmax_decode_embed_kernel(const int32_t* __restrict__ cur_tok, const bf16_t* __restrict__ E,
                                                                bf16_t* __restrict__ h, int hidden, int vocab, float* __restrict__ h32) {
    const int b = blockIdx.x;
    int id = cur_tok[b];
    id = min(max(id, 0), vocab - 1);
    const u32x4_t* s = (const u32x4_t*)(E + (size_t)id * hidden);
    u32x4_t* o = (u32x4_t*)(h + (size_t)b * hidden);
    if (h32) {   // fp32 residual stream: the embedding row widened (exact), beside the bf16 row
        for (int c = threadIdx.x; c < hidden / 8; c += blockDim.x) {
            const f32x8_t f = bf16x8_to_f32(s[c]);
            float* hp = h32 + (size_t)b * hidden + (size_t)c * 8;
            *(f32x4_t*)hp = f.lo;
            *(f32x4_t*)(hp + 4) = f.hi;
        }
    }
    for (int c = threadIdx.x; c < hidden / 8; c += blockDim.x) o[c] = s[c];
}

// ---------------------------------------------------------------------------------------------------------------------
// Finish a step: argmax over the lm-head partials, EOS / length bookkeeping, next current token.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emmax_decode_finish_kernel(FinishParams p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ float sv[256];
    __shared__ int si[256];
    float best = -INFINITY;
    int besti = 0x7fffffff;
    for (int i = tid; i < p.n_part; i += 256) {
        const float v = *(p.part_val + (size_t)i * p.B + b);
        const int ii = *(p.part_idx + (size_t)i * p.B + b);
        if (v > best || (v == best && ii < besti)) {
            best = v;
            besti = ii;
        }
    }
    sv[tid] = best;
    si[tid] = besti;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float v = sv[tid + s];
            const int ii = si[tid + s];
            if (v > sv[tid] || (v == sv[tid] && ii < si[tid])) {
                sv[tid] = v;
                si[tid] = ii;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        int tok = si[0];
        if (tok == 0x7fffffff) tok = p.pad_id;
        emmax_finish_row(p, b, tok, nullptr, 0.f, false);
    }
}

// caller-supplied continuation (teacher forcing / the HF cached forward step): the row decodes again whatever the engine's own
// greedy prediction was -- clear the done flag and the stop-rule state, lift the token budget
__global__ void emmax_set_tokens_kernel(RowState r, const int32_t* toks, int B, int budget) {
    const int i = threadIdx.x;
    if (i < B) {
        r.cur_tok[i] = toks[i];
        r.done[i] = 0;
        r.stop_m[i] = 0;
        r.stop_after[i] = -1;
        r.max_new[i] = budget;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------
// persistent grid: 2 blocks of 8 waves per CU when the staged activations allow it, never more blocks than work
static int gemv_grid(int B, size_t smem, int n_groups, int max_grid = 0) {
    int grid = (B > 2 || smem > 72 * 1024) ? 256 : 512;
    if (max_grid > 0) grid = min(grid, max_grid);
    // a partial second layer of blocks is worse than none: the CUs that hold two blocks finish ~4 us after the others (the fp8
    // qkv rows are 384 blocks' worth of four-row groups: 16.6 us with 384 blocks, 15.0 with 256; tools/gemv_lab.hip)
    if (grid == 512 && cdiv(n_groups, GW) < 512) grid = 256;
    return min(grid, cdiv(n_groups, GW));
}
// block shape of the fp8 GEMV (template argument F8): four-row groups when that still gives every wave of the 512-block grid one,
// else two rows x 12 steps when the row has more than eight spans, else two rows x 4 steps
static int gemv_fp8_shape(int n_rows, int K) {
    if (n_rows >= 4 * 512 * GW * 3 / 4) return 3;
    return K > 8 * 1024 ? 2 : 1;
}

template <int B, int MODE, bool NORM, bool XATTN = false, int F8 = 0>
static int launch_gemv_t(const GemvParams& p, const ProjGeom& g, hipStream_t stream) {
    auto kern = emmax_decode_gemv_kernel<B, MODE, NORM, XATTN, F8>;
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(GW * 64), g.smem, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

template <int MODE, bool NORM, bool XATTN = false>
static int launch_gemv_mode(const GemvParams& p, int B, const ProjGeom& g, hipStream_t stream) {
    if (g.f8) {   // fp8 rows (batch 1-2, one K phase)
#define CASEF(BB, FF) if (B == BB && g.f8 == FF) return launch_gemv_t<BB, MODE, NORM, XATTN, FF>(p, g, stream)
        CASEF(1, 1); CASEF(1, 2); CASEF(1, 3); CASEF(2, 1); CASEF(2, 2); CASEF(2, 3);
#undef CASEF
        return -1;
    }
#define CASEB(BB) case BB: return launch_gemv_t<BB, MODE, NORM, XATTN>(p, g, stream)
    switch (B) {
        CASEB(1); CASEB(2);
    }
    if constexpr (MODE == GEMV_PLAIN) {   // 3-8 rows: plain rows only (emmax_op_gemv); a fused step of that size runs on the MFMA kernels
        switch (B) {
            CASEB(3); CASEB(4); CASEB(5); CASEB(6); CASEB(7); CASEB(8);
        }
    }
#undef CASEB
    return -1;
}

// What the staged kernel takes: the fused modes at 1-2 rows (bf16 rows, or the fp8 row copy of launch_quant_rm8), GEMV_PLAIN up to 8 rows
// (fp8 rows: 2); K in K phases that keep B * kc * 2 bytes of activations under ~128 KiB of LDS -- ONE phase for the modes with a norm
// prologue and for fp8 rows.
bool decode_gemv_takes(const ProjShape& s, int B, ProjGeom* out) {
    if (s.K % 8 || !s.ld_ok || s.K <= 0) return false;
    if (s.mode < GEMV_QKV || s.mode > GEMV_PLAIN) return false;
    const bool fp8 = s.wfmt == PW_FP8, norm = s.mode == GEMV_QKV || s.mode == GEMV_GATEUP || s.mode == GEMV_LMHEAD;
    if (B < 1 || B > ((s.mode == GEMV_PLAIN && !fp8) ? 8 : 2) || wfmt_is_mx(s.wfmt)) return false;
    ProjGeom g = {};
    const int cap = (128 * 1024 / 2 / B) & ~511;
    g.kc = s.K <= cap ? s.K : (cdiv(cdiv(s.K, cdiv(s.K, cap)), 512) * 512);
    if ((norm || fp8) && g.kc != s.K) return false;
    if (fp8 && s.K % 16) return false;
    const int n_pairs = (s.mode == GEMV_QKV || s.mode == GEMV_GATEUP) ? s.n_rows / 2 : (s.n_rows + 1) / 2;
    g.n_groups = n_pairs;
    if (fp8) {
        g.f8 = gemv_fp8_shape(s.n_rows, s.K);
        if (g.f8 == 3) g.n_groups = (n_pairs + 1) / 2;   // groups of two pairs
    }
    g.smem = (size_t)B * (g.kc * 2 + 16);
    g.grid = gemv_grid(B, g.smem, g.n_groups, (g.f8 == 1 || g.f8 == 2) ? 256 : s.max_grid);
    if (s.mode == GEMV_LMHEAD) g.grid = min(g.grid, s.max_parts);
    if (out) *out = g;
    return true;
}

template <int MODE, bool NORM, bool XATTN = false>
static int gemv_init_mode() {
    const int lim = 160 * 1024 - 4096;
    hipError_t e = hipSuccess;
#define SETB(BB) if (e == hipSuccess) e = hipFuncSetAttribute((const void*)emmax_decode_gemv_kernel<BB, MODE, NORM, XATTN>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)
    SETB(1); SETB(2);
    if constexpr (MODE == GEMV_PLAIN) { SETB(3); SETB(4); SETB(5); SETB(6); SETB(7); SETB(8); }   // (launch_gemv_mode)
#undef SETB
#define SETF(BB, FF) if (e == hipSuccess) e = hipFuncSetAttribute((const void*)emmax_decode_gemv_kernel<BB, MODE, NORM, XATTN, FF>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)
    SETF(1, 1); SETF(1, 2); SETF(1, 3); SETF(2, 1); SETF(2, 2); SETF(2, 3);
#undef SETF
    return e == hipSuccess ? 0 : -4;
}
int decode_gemv_init() {
    static int done = -1;
    if (done == 0) return 0;
    int r = gemv_init_mode<GEMV_QKV, true>();
    if (!r) r = gemv_init_mode<GEMV_RESID, false>();
    if (!r) r = gemv_init_mode<GEMV_RESID, false, true>();
    if (!r) r = gemv_init_mode<GEMV_GATEUP, true>();
    if (!r) r = gemv_init_mode<GEMV_LMHEAD, true>();
    if (!r) r = gemv_init_mode<GEMV_PLAIN, false>();
    done = r;
    return r;
}

int launch_quant_rm8(const void* src, int ld, void* dst, float* scales, int N, int K, hipStream_t stream) {
    if (N <= 0 || K <= 0 || K % 16 || ld % 8) return -1;
    hipLaunchKernelGGL(emmax_quant_rm8_kernel, dim3(N), dim3(256), 0, stream, (const bf16_t*)src, ld, (uint8_t*)dst, scales, N, K);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_decode_gemv_staged(int mode, const GemvParams& p_in, int B, const ProjGeom& g, hipStream_t stream, int* grid_out) {
    GemvParams p = p_in;
    p.kc = g.kc; p.n_groups = g.n_groups;
    p.n_pairs = (mode == GEMV_QKV || mode == GEMV_GATEUP) ? p.n_rows / 2 : (p.n_rows + 1) / 2;
    if (grid_out) *grid_out = g.grid;
    switch (mode) {
        case GEMV_QKV: return launch_gemv_mode<GEMV_QKV, true>(p, B, g, stream);
        case GEMV_RESID:
            return p.attn_part ? launch_gemv_mode<GEMV_RESID, false, true>(p, B, g, stream) : launch_gemv_mode<GEMV_RESID, false>(p, B, g, stream);
        case GEMV_GATEUP: return launch_gemv_mode<GEMV_GATEUP, true>(p, B, g, stream);
        case GEMV_LMHEAD: return launch_gemv_mode<GEMV_LMHEAD, true>(p, B, g, stream);
        default: return launch_gemv_mode<GEMV_PLAIN, false>(p, B, g, stream);
    }
}

// p.wscale set: p.W is the fp8 row copy of launch_quant_rm8 (ldw = bytes per row), batch 1-2.  -1: neither decode_ks.hip nor the staged kernel takes it
int launch_decode_gemv(int mode, const GemvParams& p, int B, hipStream_t stream, int* grid_out, int* staged_out) {
    const ProjShape s = proj_shape(mode, p);
    ProjGeom g;
    if (staged_out) *staged_out = 0;
    if (decode_ks_enabled() && decode_ks_takes(s, B, &g)) return launch_decode_ks(mode, p, B, stream, grid_out, &g);   // batch 1-2, bf16, K % 64 == 0
    if (!decode_gemv_takes(s, B, &g)) return -1;
    if (staged_out) *staged_out = 1;
    return launch_decode_gemv_staged(mode, p, B, g, stream, grid_out);
}

int launch_decode_embed(const int32_t* cur_tok, const void* E, void* h, int B, int hidden, int vocab, hipStream_t stream, float* h32) {
    hipLaunchKernelGGL(emmax_decode_embed_kernel, dim3(B), dim3(256), 0, stream, cur_tok, (const bf16_t*)E, (bf16_t*)h, hidden, vocab, h32);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_decode_finish(const FinishParams& p_in, hipStream_t stream) {
    FinishParams p = p_in;
    hipLaunchKernelGGL(emmax_decode_finish_kernel, dim3(p.B), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_set_tokens(const RowState& rows, const int32_t* toks, int B, int budget, hipStream_t stream) {
    hipLaunchKernelGGL(emmax_set_tokens_kernel, dim3(1), dim3(64), 0, stream, rows, toks, B, budget);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

#ifdef DECODE_LAB_TRACE
// lab builds only (tools/decode_stage_trace.py): the phase stamps of the most recent GEMV launch, [block][8]
extern "C" int emmax_debug_gemv_trace(unsigned long long* host_out, int n_words) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_gemv_trace), (size_t)n_words * 8) == hipSuccess ? 0 : -1;
}
#endif

