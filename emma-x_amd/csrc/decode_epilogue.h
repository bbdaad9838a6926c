// decode_epilogue.h -- what the five decode projection kernel families (decode.hip, decode_ks.hip, decode_km.hip, decode_kmp.hip,
// decode_mfma.hip) do once a result element is known: RoPE + K / V append (qkv), + residual (o-proj, down), SwiGLU (gate/up), the greedy
// candidate and the block's best per batch column (lm-head).  The families differ in how they stream weights and reduce over K.  Shared
// here: where a K / V row goes, the position / page and cos / sin fetch, the residual fetch, SwiGLU, the lm-head candidate rule and column
// scan, and the 4-row tile prefetch and finish of decode_km.hip / decode_kmp.hip for every mode but qkv.  NOT shared, each kernel keeps its
// own text: the RoPE rotation with its q / K / V stores (five bf16 copies, two exact ones) and the element-level residual add + stores of
// decode.hip, decode_ks.hip and decode_mfma.hip -- the notes below say why.  Device code only; every helper is force-inlined and takes
// scalars and references, so that a kernel keeps live exactly what it kept when the text stood in its own file (the kernels sit at the
// edge of the register file), and none of them decides WHEN an operand is requested: the fetch helpers are called where each kernel had
// its loads.
#pragma once

#include "common.h"
#include "kernels.h"

// where the QKV epilogues put element block (head hk, K or V) of batch row b: the paged bf16 cache, or the staging rows of the fp8 KV cache
__device__ __forceinline__ bf16_t* gemv_kv_row(const GemvParams& p, bool is_v, int b, int pg, int pos, int hk) {
    if (p.kv_stage) return (bf16_t*)p.kv_stage + (((size_t)b * p.Hkv + hk) * 2 + (is_v ? 1 : 0)) * p.head_dim;
    return (bf16_t*)(is_v ? p.vcache : p.kcache) + (((size_t)pg * p.Hkv + hk) * p.page + pos % p.page) * p.head_dim;
}
// exact numerics: element d of the (page, kv head, position) row of the fp32 / 24-bit paged cache
__device__ __forceinline__ void gemv_kv_store_x(const GemvParams& p, bool is_v, int pg, int pos, int hk, int d, float v) {
    const size_t idx = (((size_t)pg * p.Hkv + hk) * p.page + pos % p.page) * p.head_dim + d;
    void* base = is_v ? p.vcache : p.kcache;
    if (p.kv24 > 0) {
        const uint32_t u = x24_bits(v);
        ((bf16_t*)base)[idx] = (bf16_t)(u >> 16);
        ((uint8_t*)base + (size_t)p.kv24 * 2)[idx] = (uint8_t)(u >> 8);
    } else {
        ((float*)base)[idx] = v;
    }
}

// ---- QKV: one RoPE pair (d, d + head_dim / 2) of head block hb (q heads, then K heads, then V heads) of batch row b ----
// the row's position and the page that holds it
__device__ __forceinline__ void qkv_row_pos(const GemvParams& p, int b, int& pos, int& pg) {
    pos = p.ctx_len[b];
    pg = p.page_table[(size_t)b * p.max_pages + pos / p.page];
}
// cos / sin of (pos, d); V heads are not rotated: cs / sn keep what the caller put there
__device__ __forceinline__ void qkv_rope_fetch(const GemvParams& p, int pos, int hb, int d, float& cs, float& sn) {
    const int half = p.head_dim >> 1;
    if (hb < p.Hq + p.Hkv) {
        cs = p.cos_t[(size_t)pos * half + d];
        sn = p.sin_t[(size_t)pos * half + d];
    }
}
// The pair's rotation and stores stay in each kernel's own text.  `x0 * cs - x1 * sn` is contracted by hipcc into an fma around ONE of the two
// products, the source does not say which, and the bf16 result depends on it; with the text in place every kernel keeps the arithmetic it
// had.  Through a shared helper the choice is hipcc's again per call site, and decode_kmp.hip's six-tile qkv forms (256 VGPRs, spilling)
// also needed more scratch.  Writing the fma out (__fmaf_rn around the product each kernel fuses today) would pin the arithmetic but needs
// one variant per kernel: not done.

// ---- residual (o-proj, down): h += W x in place.  r32: the fp32 stream p.h32 is the master copy (GemvParams::h32), the bf16 rows p.y its
// mirror (what the NORM modes of the batch >= 3 / fp8 kernels read) ----
__device__ __forceinline__ float resid_fetch(const GemvParams& p, int b, int row, bool r32) {
    return r32 ? p.h32[(size_t)b * p.ldh + row] : bf2f(*((const bf16_t*)p.y + (size_t)b * p.ldy + row));
}
// The element-level add + stores stay in each kernel: decode.hip and decode_mfma.hip multiply by the fp8 row scale right before the add,
// and whether hipcc contracts that multiply into the add is decided per call site (one rounding or two: the fp32 stream would show it);
// decode_ks.hip rounds the pair's two mirrors with one v_cvt_pk_bf16_f32.  The 4-row tile form below is shared.

// ---- SwiGLU (gate/up): element col of the activation row.  EX (exact numerics): the IEEE quotient, the product stays fp32 ----
template <bool EX>
__device__ __forceinline__ void swiglu_finish(const GemvParams& p, int b, int col, float g, float u) {
    if constexpr (EX) ((float*)p.y)[(size_t)b * p.ldy + col] = silu_precise(g) * u;
    else {   // (the address before the value: the order of the instructions decides hipcc's schedule in the callers)
        bf16_t* y = (bf16_t*)p.y + (size_t)b * p.ldy + col;
        *y = f2bf(silu(g) * u);
    }
}

// ---- lm-head: greedy argmax with torch.argmax's tie rule -- take if greater; on equality the lower index ----
__device__ __forceinline__ void lmhead_take(float x, int i, float& best, int& besti) {
    if (x > best || (x == best && i < besti)) {
        best = x;
        besti = i;
    }
}
// logit x of vocabulary row `row` of batch row b (rows past the vocabulary: padding of the last tile).  decode_km.hip / decode_kmp.hip had
// `x > best` alone here: the same for every logit above -inf (a thread's rows ascend), but a thread whose logits are all -inf now names its
// first row, not INT_MAX; a block whose whole column is -inf then reports its lowest row as the partial's index instead of INT_MAX
__device__ __forceinline__ void lmhead_row(const GemvParams& p, int b, int row, float x, float& best, int& besti) {
    if (row < p.n_rows) {
        lmhead_take(x, row, best, besti);
        if (p.logits_out) p.logits_out[(size_t)b * p.n_rows + row] = x;
    }
}
// the block's best of batch column col: thread col folds the n LDS slots slot(0) .. slot(n - 1) of its column into (v0, i0) -- the caller
// sets the start: (-inf, INT_MAX), or its first slot -- and writes the block's partial
template <class Slot>
__device__ __forceinline__ void lmhead_col_finish(const GemvParams& p, int B, int col, const float* bv, const int* bi, int n, Slot slot, float v0, int i0) {
    for (int k = 0; k < n; ++k) {
        const int e = slot(k);
        lmhead_take(bv[e], bi[e], v0, i0);
    }
    *(p.part_val + (size_t)blockIdx.x * B + col) = v0;
    *(p.part_idx + (size_t)blockIdx.x * B + col) = i0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The 4-row tile form of decode_km.hip / decode_kmp.hip: a thread finalises rows 4 rq + j (j < 4) of a 16-row tile -- and, where rows r and
// r + 8 of a tile belong together (qkv, gate/up: the row-permuted copies, km_src_row), their partners -- for ONE batch column c.
// Two functions: the operands are requested before the weight stream starts, the finish runs behind the block's barrier.
// ---------------------------------------------------------------------------------------------------------------------
template <bool R32>
__device__ __forceinline__ void tile4_resid_prefetch(const GemvParams& p, int c, int row0, float (&pre)[4]) {
    if constexpr (R32) {
        const f32x4_t hv = *(const f32x4_t*)(p.h32 + (size_t)c * p.ldh + row0);
#pragma unroll
        for (int j = 0; j < 4; ++j) pre[j] = hv[j];
    } else {
        const bf16_t* hp = (const bf16_t*)p.y + (size_t)c * p.ldy + row0;
#pragma unroll
        for (int j = 0; j < 4; ++j) pre[j] = bf2f(hp[j]);
    }
}
template <bool R32>
__device__ __forceinline__ void tile4_resid_finish(const GemvParams& p, int c, int row0, const float (&pre)[4], const float (&v)[4]) {
    if constexpr (R32) *(f32x4_t*)(p.h32 + (size_t)c * p.ldh + row0) = (f32x4_t){pre[0] + v[0], pre[1] + v[1], pre[2] + v[2], pre[3] + v[3]};
    bf16_t* hp = (bf16_t*)p.y + (size_t)c * p.ldy + row0;
#pragma unroll
    for (int j = 0; j < 4; ++j) hp[j] = f2bf(pre[j] + v[j]);
}
// RESID: pre_a = the old residual values; QKV: position, page, pre_a / pre_b = cos / sin of the four pairs (tile = head block hb, block
// of 8 pairs inside the head: d = 8 (tile % (hd / 16)) + 4 rq + j).  The arrays arrive zeroed.
template <int MODE, bool R32>
__device__ __forceinline__ void tile4_prefetch(const GemvParams& p, int c, int tile, int rq, float (&pre_a)[4], float (&pre_b)[4], int& pos, int& pg) {
    if (MODE == GEMV_RESID) {
        tile4_resid_prefetch<R32>(p, c, tile * 16 + 4 * rq, pre_a);
    } else if (MODE == GEMV_QKV) {
        qkv_row_pos(p, c, pos, pg);
        const int tph = p.head_dim / 16;
        const int hb = tile / tph, d0 = 8 * (tile - hb * tph) + 4 * rq;
#pragma unroll
        for (int j = 0; j < 4; ++j) qkv_rope_fetch(p, pos, hb, d0 + j, pre_a[j], pre_b[j]);
    }
}
// v: the rows' results, u: their partners'.  best / besti: the thread's running lm-head candidate (rows ascend inside a thread).  Every mode
// but qkv (see above).
template <int MODE, bool R32, bool EX>
__device__ __forceinline__ void tile4_finish(const GemvParams& p, int c, int tile, int rq, const float (&v)[4], const float (&u)[4], const float (&pre_a)[4],
                                             float& best, int& besti) {
    const int row0 = tile * 16 + 4 * rq;   // natural-order matrices
    if (MODE == GEMV_PLAIN) {
        bf16_t* yp = (bf16_t*)p.y + (size_t)c * p.ldy + row0;
#pragma unroll
        for (int j = 0; j < 4; ++j) yp[j] = f2bf(v[j]);
    } else if (MODE == GEMV_RESID) {
        tile4_resid_finish<R32>(p, c, row0, pre_a, v);
    } else if (MODE == GEMV_GATEUP) {
#pragma unroll
        for (int j = 0; j < 4; ++j) swiglu_finish<EX>(p, c, 8 * tile + 4 * rq + j, v[j], u[j]);
    } else if (MODE == GEMV_LMHEAD) {
#pragma unroll
        for (int j = 0; j < 4; ++j) lmhead_row(p, c, row0 + j, v[j], best, besti);
    }
}
