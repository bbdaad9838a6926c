// decode_attn.hip -- split-KV decode attention over the paged bf16 / fp8 KV cache: one query token per sequence (the attention of HF
// `LlamaDecoderLayer` at q_len == 1).  16 lanes per key row, 4 keys per wave load, fp32 online softmax inside a split; the splits' partials
// are merged by the o-proj that follows (the staging prologues of decode.hip, decode_ks.hip, decode_km.hip, decode_mfma.hip; common.h:
// attn_merge_chunk), or, with one split per (row, head), the launch writes the bf16 attention row itself.  exact.hip holds the fp32 form.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PSTRIDE = EMMAX_PSTRIDE;   // floats per attention split partial: 128 o + m + l + 2 pad (16-byte aligned rows)

// ---------------------------------------------------------------------------------------------------------------------
// Split-KV decode attention over the paged cache.  grid (NSPLIT, Hkv, B), 256 threads.
// A 16-lane group owns one key at a time (lane = 16-byte chunk of the 128-wide row; 4 keys per wave load instruction,
// fully coalesced) and keeps its own online-softmax state (m, l, o[8 per lane]); K and V of a whole chunk of keys are
// requested before the first score is computed, so 2*KU 16-byte loads per lane are in flight.  The 16 group states of
// the block are merged through shuffles + LDS, and the block writes one partial per (row, head, split):
//   part[((b*Hq + h)*nsplit + s) * PSTRIDE] = { o[0..HD) un-normalised, m, l, pad }
// The cross-split merge is fused into the staging prologue of the o-proj GEMV (XATTN).
// ---------------------------------------------------------------------------------------------------------------------
// DIRECT (one KV split per (row, head): batch >= 5 at 32 heads): nothing to merge -- the block holds the head's whole result,
// normalises it and writes the bf16 row the o-proj reads (the arithmetic of a one-split merge), no partials, no o-proj prologue.
// (A cross-split merge inside this launch was measured in round 3 and removed in round 4: 12.6 against 5.7 us at B = 1)
// KV8 (round 5, opt-in fp8 KV cache): K / V pages hold e4m3 rows with one fp32 scale per (token, head) row -- 8 bytes per lane and key
// instead of 16, de-quantised in registers (v_cvt_scalef32_pk_bf16_fp8 with the row's scale) right before the dot products.  The key the
// qkv launch of THIS step produced (position L - 1) waits as bf16 in p.kv_stage: every block quantises it itself (so that this step sees
// the values every later step will read back) and split 0 appends bytes + scale to the cache.
// DEEP: four chunks of keys in flight per wave instead of two (always with KV8; bf16: tuning switch attn_deep)
// GRP (grouped steps: N rows per prompt on the prompt's pages, launch_group_attn): the rows of group g = b / N hold the same page ids in their
// first p.grp_shared[g] table entries, sh = grp_shared[g] * page keys that N blocks per kv head would each stream for themselves.  Two launches,
// the kernel boundary between them the only hand-off (no counters, no last-arriver block, no fences):
//   GRP_SPAN  grid (splits, Hkv, groups x query chunks): a block reads each K / V row of its slice of [0, sh) ONCE and scores it against up to G
//             (row, q head) pairs of the group -- query j of the group is row g N + j / gqa, head hk gqa + j % gqa: the G-queries-per-key loop
//             of GQA with the rows of a group in the role of the heads of a kv group.  Queries past N gqa and those of finished rows are
//             computed and never stored.  One partial per (row, head, split) in p.part, the empty partial for an empty slice.  Every key is an
//             old one: the fp8-cache form de-quantises with the row scale, no staging row.
//   GRP_TAIL  the DIRECT form over the row's own keys [sh, L): before it normalises, the block folds in the row's p.grp_nsplit shared partials
//             (attn_merge_chunk's arithmetic).  The range holds at least the key this step appended.
enum { GRP_OFF = 0, GRP_TAIL = 1, GRP_SPAN = 2 };
template <int HD, int G, bool DIRECT = false, int NW = 4, bool KV8 = false, bool DEEP = KV8, int GRP = GRP_OFF>
__global__ __launch_bounds__(NW * 64) void emmax_decode_attn_kernel(DecodeAttnParams p) {
    static_assert(GRP != GRP_TAIL || DIRECT, "the tail form finishes the row");
    static_assert(GRP != GRP_SPAN || !DIRECT, "the shared span hands partials on");
    // waves per block: 4 (8-wave blocks were measured no faster at batch 1-2, where 512 four-wave blocks already put 8 waves on a CU,
    // DESIGN.md section 6); the one-split form of batch 5-8 is 256 blocks = ONE per CU: NW = 8 there (tuning switch attn_nw, round 5)
    constexpr int NT = NW * 64;
    static_assert(HD == 128, "decode attention maps 16 lanes x 8 elements onto one 128-wide K/V row");
    constexpr int KU = G <= 2 ? 4 : 2;    // keys per lane group per chunk (block chunk = 16 * KU keys), two chunks in flight
    constexpr int SP = 512;  // page ids kept in LDS = the longest page table the launcher accepts (32 K tokens at 64 per page)
    __shared__ int s_pages[SP];
    __shared__ float red_o[NW][G][HD];
    __shared__ float red_ml[NW][G][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kg = lane >> 4, ch = lane & 15;       // key group within the wave, 16-byte chunk within the row
    const int split = blockIdx.x, hk = blockIdx.y;
    int b = blockIdx.z;
    const int nsplit = gridDim.x;
    // SPAN: blockIdx.z = group x query chunk; b becomes the group's first row (its table row holds the shared pages), j0 the chunk's first query
    int gqa = 1, nq = 0, j0 = 0;
    if constexpr (GRP == GRP_SPAN) {
        gqa = p.grp_Hq / p.Hkv;
        nq = p.grp_N * gqa;
        const int nchunk = (nq + G - 1) / G, g = b / nchunk;
        j0 = (b - g * nchunk) * G;
        b = g * p.grp_N;
    }
    int sh_pages = 0;   // (clamped: whatever the array holds, no key index leaves the page table)
    if constexpr (GRP != GRP_OFF) sh_pages = min(max(p.grp_shared[b / p.grp_N], 0), p.max_pages);
    // ONE memory round trip for everything in front of the K/V loads: the context length and the done flag (scalar loads,
    // requested first), the row's whole page table (<= SP entries, two per thread, kept in registers until all requests are
    // out, then written to LDS) and q.  (A loop that waited for each table load, then a dependent scalar load for the length,
    // then another for the flag cost three extra round trips -- half of this 7 us kernel.)
    const int ctx_now = p.ctx_len[b];
    const int done_word = *(p.done ? p.done + b : p.ctx_len + b);   // always a load, never a branch with its own wait in front of
    const int row_done = p.done ? done_word : 0;                  // the q / page-table requests
    const int32_t* ptab = p.page_table + (size_t)b * p.max_pages;
    // q (already rotated, bf16) for the G heads of this kv head: lane holds elements ch*8 .. +8
    u32x4_t q[G];
    int qhead[G];      // SPAN: (row, head) index row * Hq + head of query gq, and whether its partial is stored
    bool qlive[G];
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
        if constexpr (GRP == GRP_SPAN) {
            const int j = min(j0 + gq, nq - 1), row = b + j / gqa, head = hk * gqa + j % gqa;
            qhead[gq] = row * p.grp_Hq + head;
            qlive[gq] = j0 + gq < nq && !(p.done && p.done[row] != 0);
            q[gq] = *(const u32x4_t*)((const bf16_t*)p.q + (size_t)row * p.ldq + head * HD + ch * 8);
            continue;
        }
        q[gq] = *(const u32x4_t*)((const bf16_t*)p.q + (size_t)b * p.ldq + (hk * G + gq) * HD + ch * 8);
    }
    const int pt0 = ptab[min(tid, p.max_pages - 1)], pt1 = ptab[min(tid + NT, p.max_pages - 1)];
    __builtin_amdgcn_sched_barrier(0);   // every request above is out before the first wait (hipcc sinks the q load below the LDS write otherwise)
    s_pages[tid] = pt0;
    if (NT < SP) s_pages[tid + NT] = pt1;
    const int sh = sh_pages << p.page_shift;
    const int L = GRP == GRP_SPAN ? sh : ctx_now + 1;   // keys including the one appended by the qkv kernel of this step (SPAN: the shared ones)
    int kps = (L + nsplit - 1) >> __builtin_ctz(nsplit);   // the split count is a power of two (launcher)
    kps = (kps + 15) & ~15;
    const int k0 = (GRP == GRP_TAIL ? sh : 0) + split * kps;   // (TAIL: one split, [sh, L))
    const int k1 = min(L, k0 + kps);
    const int Hq = p.Hkv * G;
    float* part = p.part + ((size_t)(b * Hq + hk * G) * nsplit + split) * PSTRIDE;

    if constexpr (GRP == GRP_SPAN) {
        bool any = false;
#pragma unroll
        for (int gq = 0; gq < G; ++gq) any = any || qlive[gq];
        if (!any) return;   // every row of the chunk has finished: the tail launch writes their zeros and reads no partial
        if (k0 >= L) {      // empty slice (or no shared page at all): the empty partial
#pragma unroll
            for (int gq = 0; gq < G; ++gq)
                if (qlive[gq])
                    for (int j = tid; j < PSTRIDE; j += NT) p.part[((size_t)qhead[gq] * nsplit + split) * PSTRIDE + j] = (j == HD) ? -INFINITY : 0.f;
            return;
        }
    } else if (k0 >= L || row_done) {   // empty split, or a row that no longer decodes: no K/V traffic
        if constexpr (DIRECT) {   // a row that no longer decodes: zeros (what the merge of an empty partial gives)
            for (int i = tid; i < G * (HD / 8); i += NT)
                *((u32x4_t*)((bf16_t*)p.o_out + (size_t)b * p.ldq + hk * G * HD) + i) = (u32x4_t){0u, 0u, 0u, 0u};
            return;
        }
        for (int i = tid; i < G * PSTRIDE; i += NT) {
            const int gq = i / PSTRIDE, j = i - gq * PSTRIDE;
            float* dst = part + (size_t)gq * nsplit * PSTRIDE + j;
            *dst = (j == HD) ? -INFINITY : 0.f;
        }
        return;
    }

    const bf16_t* kc = (const bf16_t*)p.kcache;
    const bf16_t* vc = (const bf16_t*)p.vcache;
    const uint8_t* kc8 = (const uint8_t*)p.kcache;
    const uint8_t* vc8 = (const uint8_t*)p.vcache;
    // KV8: the step's new K / V row of this kv head, requested now (one round trip with the page table), quantised below
    u32x4_t new_k = {0u, 0u, 0u, 0u}, new_v = {0u, 0u, 0u, 0u};
    if constexpr (KV8 && GRP != GRP_SPAN) {
        const bf16_t* st = (const bf16_t*)p.kv_stage + ((size_t)b * p.Hkv + hk) * 2 * HD + ch * 8;
        new_k = *(const u32x4_t*)st;
        new_v = *(const u32x4_t*)(st + HD);
    }

    __syncthreads();
    if constexpr (KV8 && GRP != GRP_SPAN) {
        // one scale per row (e4m3_row_scale of the amax) over the 16 lanes of a key group (every group of every wave holds the same row)
        auto requant = [&](u32x4_t& v, uint8_t* cache, float* scales) {
            float am = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) am = fmaxf(am, fmaxf(fabsf(bf_lo(v[j])), fabsf(bf_hi(v[j]))));
            am = row16_max(am);
            const float sc = e4m3_row_scale(am);
            const u32x2_t q8 = quant8_e4m3(v, 1.0f / sc);
            v = dequant8_e4m3(q8, sc);
            if (split == 0 && tid < 16) {   // append: bytes + scale at position L - 1
                const int pos = L - 1, pg = s_pages[pos >> p.page_shift];
                const size_t rowi = (((size_t)pg * p.Hkv + hk) << p.page_shift) + (pos & (p.page - 1));
                *(u32x2_t*)(cache + rowi * HD + ch * 8) = q8;
                if (tid == 0) scales[rowi] = sc;
            }
        };
        requant(new_k, (uint8_t*)p.kcache, p.kscale);
        requant(new_v, (uint8_t*)p.vcache, p.vscale);
    }

    float m[G], l[G], o[G][8];
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
        m[gq] = -INFINITY;
        l[gq] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[gq][j] = 0.f;
    }

    // software pipeline: two register chunk buffers; the loads of chunk i+1 are issued before the scores of chunk i are
    // computed, so every wave has K/V requests in flight at all times (a 1/8 split of a 1K context is two chunks: both
    // are requested up front)
    // KV8: kv / vv carry the raw bytes in [0..1] and the row's scale in [2] until consume_chunk de-quantises them
    auto load_chunk = [&](int kb, u32x4_t (&kv)[KU], u32x4_t (&vv)[KU], bool (&ok)[KU]) {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const int key = kb + u * (4 * NW) + wave * 4 + kg;
            ok[u] = key < k1;
            const int kk = ok[u] ? key : k0;
            if constexpr (KV8) {
                const int pg8 = s_pages[kk >> p.page_shift];
                const size_t rowi = (((size_t)pg8 * p.Hkv + hk) << p.page_shift) + (kk & (p.page - 1));
                const u32x2_t k8 = __builtin_nontemporal_load((const u32x2_t*)(kc8 + rowi * HD + ch * 8)),   // (non-temporal: see the bf16 path below)
                              v8 = __builtin_nontemporal_load((const u32x2_t*)(vc8 + rowi * HD + ch * 8));
                // (the position the lane READ, in every form -- a masked lane re-reads key k0, and a split or tail that is the new key alone
                // starts on the row the cache does not hold yet: bytes and scale there are anything, and 0 x NaN is not 0.  With the position
                // read, is_new below hands such a lane the staging row.  The plain form carried `key` until tests/test_decode_attn_forms_gpu.py
                // poisoned the cache past the context: ctx a multiple of the split's key count, ctx = 0 with one split)
                kv[u] = (u32x4_t){k8[0], k8[1], __float_as_uint(p.kscale[rowi]), (uint32_t)kk};
                vv[u] = (u32x4_t){v8[0], v8[1], __float_as_uint(p.vscale[rowi]), 0u};
                continue;
            }
            // the page id ALWAYS comes from LDS (the launcher rejects tables longer than SP): a select between the LDS copy and
            // the global table became a FLAT load, whose wait (vmcnt(0) lgkmcnt(0)) also drained the K/V loads in flight --
            // every key's lookup waited for the previous key's rows
            const int pg = s_pages[kk >> p.page_shift];
            const size_t off = ((((size_t)pg * p.Hkv + hk) << p.page_shift) + (kk & (p.page - 1))) * HD + ch * 8;
            // NON-TEMPORAL loads (round 5): a K / V row is read by ONE block, once per step -- as plain loads the rows were allocated in the
            // XCD's L2 and in the MALL on their way through, displacing the lines every block of the NEXT launches re-reads (activation rows,
            // norm weights, RoPE tables).  Measured, builds alternating on one box (profiles/r05_attn_kv_nt_ab.txt): this launch 5.63 ->
            // 5.42 us at batch 1, 19.9 -> 18.3 at 8 rows, 69.0 -> 61.7 at 32; the whole step 2.593 -> 2.568 ms/token, 3.26 -> 3.19, 5.37 -> 5.11 ms
            kv[u] = __builtin_nontemporal_load((const u32x4_t*)(kc + off));
            vv[u] = __builtin_nontemporal_load((const u32x4_t*)(vc + off));
        }
    };
    auto consume_chunk = [&](u32x4_t (&kv)[KU], u32x4_t (&vv)[KU], const bool (&ok)[KU]) {
        if constexpr (KV8) {   // bytes -> bf16 x scale; the key of this step comes from the staging row (its cache bytes may not have landed)
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                const bool is_new = GRP != GRP_SPAN && (int)kv[u][3] == L - 1;
                const u32x4_t kd = dequant8_e4m3((u32x2_t){kv[u][0], kv[u][1]}, __uint_as_float(kv[u][2]));
                const u32x4_t vd = dequant8_e4m3((u32x2_t){vv[u][0], vv[u][1]}, __uint_as_float(vv[u][2]));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    kv[u][j] = is_new ? new_k[j] : kd[j];
                    vv[u][j] = is_new ? new_v[j] : vd[j];
                }
            }
        }
#pragma unroll
        for (int gq = 0; gq < G; ++gq) {
            float sc[KU];
            float mc = -INFINITY;
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                float s = 0.f;
                s = dot2_bf16(kv[u][0], q[gq][0], s);
                s = dot2_bf16(kv[u][1], q[gq][1], s);
                s = dot2_bf16(kv[u][2], q[gq][2], s);
                s = dot2_bf16(kv[u][3], q[gq][3], s);
                s = row16_sum(s);   // the 16 lanes of a key group are one DPP row
                s = ok[u] ? s * p.scale : -INFINITY;
                sc[u] = s;
                mc = fmaxf(mc, s);
            }
            const float mn = fmaxf(m[gq], mc);
            const float msafe = (mn == -INFINITY) ? 0.f : mn;
            const float alpha = __expf(m[gq] - msafe);
            float ls = l[gq] * alpha;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[gq][j] *= alpha;
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                const float pw = __expf(sc[u] - msafe);
                ls += pw;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o[gq][2 * j] += pw * bf_lo(vv[u][j]);
                    o[gq][2 * j + 1] += pw * bf_hi(vv[u][j]);
                }
            }
            l[gq] = ls;
            m[gq] = mn;
        }
    };
    if constexpr (DEEP) {
        // FOUR chunks in flight: at 8 bytes per lane and key two chunks are 8 KiB per wave -- the launch was a latency chain (one chunk
        // per ~1.1 us round trip: 18.9 us for 53 MB at batch 8); the raw bytes of four chunks take the registers two bf16 chunks did
        constexpr int CHK = (4 * NW) * KU;
        u32x4_t kvA[KU], vvA[KU], kvB[KU], vvB[KU], kvC[KU], vvC[KU], kvD[KU], vvD[KU];
        bool okA[KU], okB[KU], okC[KU], okD[KU];
        load_chunk(k0, kvA, vvA, okA);
        if (k0 + CHK < k1) load_chunk(k0 + CHK, kvB, vvB, okB);
        if (k0 + 2 * CHK < k1) load_chunk(k0 + 2 * CHK, kvC, vvC, okC);
        for (int kb = k0; kb < k1; kb += 4 * CHK) {               // every condition is block-uniform
            if (kb + 3 * CHK < k1) load_chunk(kb + 3 * CHK, kvD, vvD, okD);
            consume_chunk(kvA, vvA, okA);
            if (kb + 4 * CHK < k1) load_chunk(kb + 4 * CHK, kvA, vvA, okA);
            if (kb + CHK < k1) consume_chunk(kvB, vvB, okB);
            if (kb + 5 * CHK < k1) load_chunk(kb + 5 * CHK, kvB, vvB, okB);
            if (kb + 2 * CHK < k1) consume_chunk(kvC, vvC, okC);
            if (kb + 6 * CHK < k1) load_chunk(kb + 6 * CHK, kvC, vvC, okC);
            if (kb + 3 * CHK < k1) consume_chunk(kvD, vvD, okD);
        }
    } else {
        u32x4_t kvA[KU], vvA[KU], kvB[KU], vvB[KU];
        bool okA[KU], okB[KU];
        load_chunk(k0, kvA, vvA, okA);
        for (int kb = k0; kb < k1; kb += 2 * (4 * NW) * KU) {
            const bool hasB = kb + (4 * NW) * KU < k1;          // block-uniform
            if (hasB) load_chunk(kb + (4 * NW) * KU, kvB, vvB, okB);
            consume_chunk(kvA, vvA, okA);
            if (kb + 2 * (4 * NW) * KU < k1) load_chunk(kb + 2 * (4 * NW) * KU, kvA, vvA, okA);
            if (hasB) consume_chunk(kvB, vvB, okB);
        }
    }

    // ---- merge the 4 key groups of the wave (lanes with equal ch), then the 4 waves through LDS ----
#pragma unroll
    for (int gq = 0; gq < G; ++gq) {
        const float mw = rows_max(m[gq]);
        const float msafe = (mw == -INFINITY) ? 0.f : mw;
        const float f = __expf(m[gq] - msafe);
        // every lane of a 16-lane key group carries the same l: after the two exchanges each lane holds the wave sum
        const float lv = rows_sum(l[gq] * f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = rows_sum(o[gq][j] * f);
            if (kg == 0) red_o[wave][gq][ch * 8 + j] = v;
        }
        if (lane == 0) {
            red_ml[wave][gq][0] = mw;
            red_ml[wave][gq][1] = lv;
        }
    }
    __syncthreads();
    auto part_value = [&](int gq, int j) {
        float M = red_ml[0][gq][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) M = fmaxf(M, red_ml[w][gq][0]);
        const float msafe = (M == -INFINITY) ? 0.f : M;
        float v = 0.f;
        if (j < HD) {
#pragma unroll
            for (int w = 0; w < NW; ++w) v += red_o[w][gq][j] * __expf(red_ml[w][gq][0] - msafe);
        } else if (j == HD) {
            v = M;
        } else if (j == HD + 1) {
#pragma unroll
            for (int w = 0; w < NW; ++w) v += red_ml[w][gq][1] * __expf(red_ml[w][gq][0] - msafe);
        }
        return v;
    };
    if constexpr (DIRECT) {   // this block holds the head's whole result -- normalise and write the bf16 row directly
        for (int i = tid; i < G * (HD / 8); i += NT) {
            const int gq = i / (HD / 8), c = i - gq * (HD / 8);
            if constexpr (GRP == GRP_TAIL) {   // the row's shared partials and this block's own: attn_merge_chunk_loop's arithmetic
                const float* sp = p.part + (size_t)(b * Hq + hk * G + gq) * p.grp_nsplit * PSTRIDE;
                const float mt = part_value(gq, HD);
                float M = mt;
                for (int s = 0; s < p.grp_nsplit; ++s) M = fmaxf(M, sp[s * PSTRIDE + HD]);
                const float wt = (mt == -INFINITY) ? 0.f : __expf(mt - M);
                float den = part_value(gq, HD + 1) * wt, a8[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) a8[j] = part_value(gq, c * 8 + j) * wt;
                for (int s = 0; s < p.grp_nsplit; ++s) {
                    const float ms = sp[s * PSTRIDE + HD];
                    const float wgt = (ms == -INFINITY) ? 0.f : __expf(ms - M);
                    den = __builtin_fmaf(sp[s * PSTRIDE + HD + 1], wgt, den);
                    const f32x4_t o0 = *(const f32x4_t*)(sp + s * PSTRIDE + c * 8);
                    const f32x4_t o1 = *(const f32x4_t*)(sp + s * PSTRIDE + c * 8 + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        a8[j] = __builtin_fmaf(o0[j], wgt, a8[j]);
                        a8[4 + j] = __builtin_fmaf(o1[j], wgt, a8[4 + j]);
                    }
                }
                const float inv = den > 0.f ? 1.0f / den : 0.f;
                u32x4_t v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = pack_bf16x2(a8[2 * j] * inv, a8[2 * j + 1] * inv);
                *((u32x4_t*)((bf16_t*)p.o_out + (size_t)b * p.ldq + (hk * G + gq) * HD) + c) = v;
                continue;
            }
            const float den = part_value(gq, HD + 1);
            const float inv = den > 0.f ? 1.0f / den : 0.f;   // the arithmetic of attn_merge_chunk<1> (weight exp(m - M) = 1)
            u32x4_t v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = pack_bf16x2(part_value(gq, c * 8 + 2 * j) * inv, part_value(gq, c * 8 + 2 * j + 1) * inv);
            *((u32x4_t*)((bf16_t*)p.o_out + (size_t)b * p.ldq + (hk * G + gq) * HD) + c) = v;
        }
        return;
    }
    if constexpr (GRP == GRP_SPAN) {
#pragma unroll
        for (int gq = 0; gq < G; ++gq)
            if (qlive[gq])
                for (int j = tid; j < PSTRIDE; j += NT) p.part[((size_t)qhead[gq] * nsplit + split) * PSTRIDE + j] = part_value(gq, j);
        return;
    }
    for (int i = tid; i < G * PSTRIDE; i += NT) {
        const int gq = i / PSTRIDE, j = i - gq * PSTRIDE;
        float* dst = part + (size_t)gq * nsplit * PSTRIDE + j;
        *dst = part_value(gq, j);
    }
}

}  // namespace

// splits of the KV range per (row, kv head): ~512 blocks in flight, at most 8 partials to merge
int decode_attn_nsplit(int B, int Hkv) {
    const int forced = emmax_tune().attn_nsplit;
    if (forced > 0) {   // rounded down to a power of two (the kernel divides by shifting)
        int f = forced > 16 ? 16 : forced;
        while (f & (f - 1)) f &= f - 1;
        return f;
    }
    // batch 1-2: ~512 blocks of 4 waves (8 splits at 32 heads).  Batch >= 3: one block per CU is enough and every split less
    // halves the partials the o-proj has to merge for 8 rows -- at B = 8 (32 heads) ONE split: attention 20.5 -> 20.0 us, o-proj
    // 12.6 -> 11.0 us, step 3.373 -> 3.297 ms (4 splits: 22.3 / 15.5 us)
    int ns = (B >= 3 ? 256 : 512) / (B * Hkv);
    if (ns < 1) ns = 1;
    if (ns > 8) ns = 8;
    while (ns & (ns - 1)) ns &= ns - 1;   // power of two: the o-proj prologue merges with a branch-free unrolled loop
    return ns;
}

// THE instantiation choice of launch_decode_attn, on the host and from the shapes, the operands that exist and the tuning switches alone
bool decode_attn_form(const DecodeAttnParams& p, int B, int Hq, int nsplit, DecodeAttnForm* f) {
    if (B < 1 || p.Hkv < 1 || Hq < 1 || Hq % p.Hkv) return false;
    if (p.max_pages < 1 || p.max_pages > 512 || p.page < 1 || (p.page & (p.page - 1))) return false;   // table fits the kernel's LDS copy; page = 2^k
    if (nsplit < 1 || (nsplit & (nsplit - 1))) return false;   // the kernel divides the keys among the splits by shifting
    if (p.o_out && nsplit != 1) return false;   // the direct form exists for one split only (nothing to merge)
    if (p.kv_stage && (!p.kscale || !p.vscale)) return false;   // fp8 KV cache: bytes + one scale per row
    const int G = Hq / p.Hkv;
    if (G != 1 && G != 2 && G != 4 && G != 8) return false;
    const int nw = emmax_tune().attn_nw;
    const bool nw8 = nw == 8 || (nw == 0 && p.o_out && (long)p.Hkv * B <= 256);
    // four chunks of keys in flight (bf16 cache): measured on one box (profiles/r05_attn_deep_k32_spread_ab.txt) -- B = 32 (1024 blocks, four
    // per CU) 73.0 -> 68.5 us per launch, B = 8 / 16 (256 / 512 blocks) 20.0 -> 20.6 / 36.9 -> 37.3: on from 1024 blocks (-1 = that rule)
    const int deep_sw = emmax_tune().attn_deep;
    const bool deep = G <= 2 && (deep_sw > 0 || (deep_sw < 0 && (long)nsplit * p.Hkv * B >= 1024));   // (G >= 4: no registers for it)
    f->G = G; f->nsplit = nsplit; f->direct = p.o_out ? 1 : 0; f->kv8 = p.kv_stage ? 1 : 0;
    f->deep = (f->kv8 || deep) ? 1 : 0;                        // (the fp8-cache form always has four chunks in flight, at every G)
    f->nw = (!f->kv8 && !deep && f->direct && nw8) ? 8 : 4;    // (eight waves: the bf16 direct form alone, and never with four chunks)
    return true;
}

int launch_decode_attn(const DecodeAttnParams& p_in, int B, int Hq, int head_dim, int nsplit, hipStream_t stream) {
    if (head_dim != 128) return -1;
    DecodeAttnParams p = p_in;
    DecodeAttnForm f;
    if (!decode_attn_form(p, B, Hq, nsplit, &f)) return -1;
    p.page_shift = 0;
    while ((1 << p.page_shift) < p.page) ++p.page_shift;
    dim3 grid(f.nsplit, p.Hkv, B), block(f.nw * 64);
    switch (f.G) {
#define ATTN_CASE(GG)                                                                                                   \
    case GG:                                                                                                           \
        if (f.kv8 && f.direct) hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG, true, 4, true>), grid, block, 0, stream, p); \
        else if (f.kv8) hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG, false, 4, true>), grid, block, 0, stream, p); \
        else if (f.direct && f.deep) hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG, true, 4, false, true>), grid, block, 0, stream, p); \
        else if (f.deep) hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG, false, 4, false, true>), grid, block, 0, stream, p); \
        else if (f.direct && f.nw == 8) hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG, true, 8>), grid, block, 0, stream, p); \
        else if (f.direct) hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG, true>), grid, block, 0, stream, p);     \
        else hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG>), grid, block, 0, stream, p);                         \
        break
        ATTN_CASE(1); ATTN_CASE(2); ATTN_CASE(4); ATTN_CASE(8);
#undef ATTN_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- grouped steps: the shared span once per group, then the rows' tails (the kernel's GRP forms) ----
// queries per span block: the narrowest instantiated width that holds the group's N x gqa (row, q head) pairs, else chunks of 8
static int group_attn_width(int nq) { return nq <= 2 ? 2 : nq <= 4 ? 4 : 8; }
bool group_attn_takes(int B, int N, int Hq, int Hkv) {
    if (N < 2 || B < N || B > EMMAX_MAX_DECODE_BATCH || B % N || Hkv < 1 || Hq % Hkv) return false;
    const int gqa = Hq / Hkv;
    return gqa == 1 || gqa == 2 || gqa == 4 || gqa == 8;
}
// splits of the shared span: about one block per CU, as decode_attn_nsplit argues for batch >= 3 (one group of 8 rows at 32 heads: 8 splits, eight
// groups: one); at most EMMAX_GROUP_ATTN_MAX_SPLITS partials for the tail to fold in
int group_attn_nsplit(int B, int N, int Hq, int Hkv) {
    const int nq = N * (Hq / Hkv), w = group_attn_width(nq), blocks = Hkv * (B / N) * ((nq + w - 1) / w);
    int ns = 1;   // the smallest power of two (the kernel divides the keys among the splits by shifting) that leaves no CU without a block:
    while (ns * blocks < 256 && ns < EMMAX_GROUP_ATTN_MAX_SPLITS) ns *= 2;   // rounding DOWN left 160 blocks at five groups of 8 -- 5.93 -> 6.11 ms per step
    return ns;
}

bool group_attn_form(const DecodeAttnParams& p, int B, int N, int Hq, GroupAttnForm* f) {
    if (!group_attn_takes(B, N, Hq, p.Hkv)) return false;
    if (p.max_pages < 1 || p.max_pages > 512 || p.page < 1 || (p.page & (p.page - 1))) return false;   // as launch_decode_attn
    if (p.kv_stage && (!p.kscale || !p.vscale)) return false;
    const int G = Hq / p.Hkv, nq = N * G, w = group_attn_width(nq);
    f->width = w; f->nsplit = group_attn_nsplit(B, N, Hq, p.Hkv); f->chunks = (nq + w - 1) / w; f->G = G; f->kv8 = p.kv_stage ? 1 : 0;
    return true;
}

int launch_group_attn(const DecodeAttnParams& p_in, int B, int N, int Hq, int head_dim, hipStream_t stream) {
    GroupAttnForm f;
    if (head_dim != 128 || !group_attn_form(p_in, B, N, Hq, &f)) return -1;
    DecodeAttnParams p = p_in;
    if (!p.o_out || !p.part || !p.grp_shared) return -1;
    p.page_shift = 0;
    while ((1 << p.page_shift) < p.page) ++p.page_shift;
    p.grp_N = N; p.grp_Hq = Hq; p.grp_nsplit = f.nsplit;
    const dim3 span(f.nsplit, p.Hkv, (B / N) * f.chunks), tail(1, p.Hkv, B), block(256);
    switch (f.width) {
#define SPAN_CASE(W)                                                                                                                   \
    case W:                                                                                                                            \
        if (f.kv8) hipLaunchKernelGGL((emmax_decode_attn_kernel<128, W, false, 4, true, true, GRP_SPAN>), span, block, 0, stream, p); \
        else hipLaunchKernelGGL((emmax_decode_attn_kernel<128, W, false, 4, false, false, GRP_SPAN>), span, block, 0, stream, p);      \
        break
        SPAN_CASE(2); SPAN_CASE(4); SPAN_CASE(8);
#undef SPAN_CASE
        default: return -1;
    }
    if (hipGetLastError() != hipSuccess) return -4;
    switch (f.G) {
#define TAIL_CASE(GG)                                                                                                                  \
    case GG:                                                                                                                           \
        if (f.kv8) hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG, true, 4, true, true, GRP_TAIL>), tail, block, 0, stream, p); \
        else hipLaunchKernelGGL((emmax_decode_attn_kernel<128, GG, true, 4, false, false, GRP_TAIL>), tail, block, 0, stream, p);      \
        break
        TAIL_CASE(1); TAIL_CASE(2); TAIL_CASE(4); TAIL_CASE(8);
#undef TAIL_CASE
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
