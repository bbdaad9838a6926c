// extend_attn.hip -- extending a cached context by n tokens per sequence: RoPE + K / V append at an offset, and causal attention of the n new
// query rows over the PAGED cache (bf16 or e4m3 + row scale), the n rows the append has just written included (HF `LlamaAttention` at
// q_len = n with a past of base tokens).  attention.hip reads K / V from the packed qkv buffer of its own launch, decode_attn.hip takes one
// query row per sequence: this file is the launch between them.
//
//   emmax_rope_kv_write_at_kernel   the pass of misc.hip (emmax_rope_kv_write_vec_kernel): packed row i of sequence b sits at position
//                                   base[b] + i -- cos / sin and the page slot are taken there.  The same fmaf forms: bit-identical rows
//   emmax_kv_quant_rows_at_kernel   fp8 KV cache: misc.hip's emmax_kv_quant_rows_kernel at that position (e4m3 bytes + e4m3_row_scale).  The qkv
//                                   rows are NOT written back: the attention below reads keys and values from the cache alone
//   emmax_extend_attn_kernel        grid (splits, Hkv x query tiles, B), 4 waves.  A block owns 128 query rows of ONE kv head: 128 / G tokens x the G
//                                   query heads of the kv head (row r = token r / G, head r % G), so the heads of a GQA group share every K / V tile.
//                                   A wave owns 32 of the rows with Q^T, running max / sum and O^T in registers, as in attention.hip:
//                                   S^T = K . Q^T and O^T = V^T . P^T on v_mfma_f32_32x32x16_bf16, P rounded to bf16 for the second product, the
//                                   row sum taken from the fp32 values.  One K / V tile = one page (64 keys: 16 KB contiguous per kv head, 8 KB +
//                                   64 scales as e4m3): ONE page-table lookup per tile, block-uniform (a scalar load), requested a tile ahead of
//                                   its use; the tile travels global -> registers -> LDS (two LDS images, one barrier per tile), e4m3 rows are
//                                   widened on that way (attention.hip's LDS-DMA ring is not done here: DESIGN.md section 4 says what it would
//                                   take).  Rows of a page past the sequence's last key are replaced by zeros on the way in (the cache may hold
//                                   anything there, and 0 x NaN is not 0 in the second product).  Row i sees keys 0 .. base + i:
//                                   mask code runs only on the tiles that touch a split's first key, the wave's diagonal or the block's last key.
//                                   Key-split form: split s takes keys [s kps, (s + 1) kps) with kps = ceil(L / nsplit) rounded up to 16 (L = base +
//                                   n, the decode attention's rule; empty splits allowed) and writes fp32 partials {o[128] un-normalised, m, l, pad}
//                                   per (packed row, head, split); emmax_extend_attn_merge_kernel folds them into the bf16 row.  One split: the
//                                   block normalises and writes the bf16 row itself.
// Lengths live on the device (cu, base); the host sizes the grid from upper bounds and blocks past a sequence's real extent exit.  Nothing
// indexes the page table past max_pages or a cos / sin row past max_pos, whatever base holds.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;

constexpr int PSTRIDE = EMMAX_PSTRIDE;

__global__ __launch_bounds__(256) void emmax_rope_kv_write_at_kernel(bf16_t* __restrict__ qkv, int ld, int q_off, int k_off, int v_off,
                                                                    const int32_t* __restrict__ cu, const int32_t* __restrict__ base, int B,
                                                                    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                    bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache,
                                                                    const int32_t* __restrict__ page_table, int max_pages, int Hq, int Hkv, int hd,
                                                                    int page, int max_pos) {
    const int row = blockIdx.x;
    if (row >= cu[B]) return;
    int b = 0;
    while (b + 1 < B && row >= cu[b + 1]) ++b;
    const int pos = base[b] + (row - cu[b]);
    if (pos < 0 || pos >= max_pos || pos / page >= max_pages) return;   // (the host checked its upper bound: never taken by a session)
    const int half = hd >> 1, hc = half >> 3;    // 8-pair chunks per head
    bf16_t* r = qkv + (size_t)row * ld;
    const float* cs = cos_t + (size_t)pos * half;
    const float* sn = sin_t + (size_t)pos * half;
    const int pg = page_table[(size_t)b * max_pages + pos / page], slot = pos % page;
    for (int i = threadIdx.x; i < (Hq + Hkv) * hc; i += blockDim.x) {
        const int hh = i / hc, d = (i - hh * hc) * 8;
        bf16_t* x = (hh < Hq) ? (r + q_off + hh * hd) : (r + k_off + (hh - Hq) * hd);
        const u32x4_t lo = *(const u32x4_t*)(x + d), hi = *(const u32x4_t*)(x + d + half);
        const f32x4_t c0 = *(const f32x4_t*)(cs + d), c1 = *(const f32x4_t*)(cs + d + 4);
        const f32x4_t s0 = *(const f32x4_t*)(sn + d), s1 = *(const f32x4_t*)(sn + d + 4);
        u32x4_t ylo, yhi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ca = j < 2 ? c0[2 * j] : c1[2 * j - 4], cb = j < 2 ? c0[2 * j + 1] : c1[2 * j - 3];
            const float sa = j < 2 ? s0[2 * j] : s1[2 * j - 4], sb = j < 2 ? s0[2 * j + 1] : s1[2 * j - 3];
            const float x0a = bf_lo(lo[j]), x0b = bf_hi(lo[j]), x1a = bf_lo(hi[j]), x1b = bf_hi(hi[j]);
            // (the fused forms of misc.hip's pass, term for term)
            ylo[j] = pack_bf16x2(fmaf(x0a, ca, -(x1a * sa)), fmaf(x0b, cb, -(x1b * sb)));
            yhi[j] = pack_bf16x2(fmaf(x0a, sa, x1a * ca), fmaf(x0b, sb, x1b * cb));
        }
        *(u32x4_t*)(x + d) = ylo;
        *(u32x4_t*)(x + d + half) = yhi;
        if (hh >= Hq && kcache) {   // (null: fp8 KV cache -- the quantising pass appends the rows)
            bf16_t* kc = kcache + (((size_t)pg * Hkv + (hh - Hq)) * page + slot) * hd;
            *(u32x4_t*)(kc + d) = ylo;   // (plain stores: the attention launch behind this pass reads the rows back)
            *(u32x4_t*)(kc + d + half) = yhi;
        }
    }
    for (int i = threadIdx.x; vcache && i < Hkv * hd / 8; i += blockDim.x) {
        const int hk = i / (hd / 8), ch = i - hk * (hd / 8);
        const u32x4_t v = *(const u32x4_t*)(r + v_off + hk * hd + ch * 8);
        *(u32x4_t*)(vcache + (((size_t)pg * Hkv + hk) * page + slot) * hd + ch * 8) = v;
    }
}

__global__ __launch_bounds__(256) void emmax_kv_quant_rows_at_kernel(const bf16_t* __restrict__ qkv, int ld, int k_off, int v_off,
                                                                    const int32_t* __restrict__ cu, const int32_t* __restrict__ base, int B,
                                                                    uint8_t* __restrict__ k8, uint8_t* __restrict__ v8, float* __restrict__ kscale,
                                                                    float* __restrict__ vscale, const int32_t* __restrict__ page_table,
                                                                    int max_pages, int Hkv, int page) {
    constexpr int HD = 128;
    const int row = blockIdx.x;
    if (row >= cu[B]) return;
    int b = 0;
    while (b + 1 < B && row >= cu[b + 1]) ++b;
    const int pos = base[b] + (row - cu[b]);
    if (pos < 0 || pos / page >= max_pages) return;
    const int pg = page_table[(size_t)b * max_pages + pos / page], slot = pos % page;
    const bf16_t* r = qkv + (size_t)row * ld;
    const int grp = threadIdx.x >> 4, ch = threadIdx.x & 15;
    for (int i = grp; i < 2 * Hkv; i += 16) {   // (a 16-lane group = one DPP row: the reduction never mixes an idle group in)
        const bool is_v = i >= Hkv;
        const int hk = is_v ? i - Hkv : i;
        const u32x4_t v = *(const u32x4_t*)(r + (is_v ? v_off : k_off) + hk * HD + ch * 8);
        float am = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) am = fmaxf(am, fmaxf(fabsf(bf_lo(v[j])), fabsf(bf_hi(v[j]))));
        am = row16_max(am);
        const float sc = e4m3_row_scale(am);
        const size_t rowi = ((size_t)pg * Hkv + hk) * page + slot;
        *(u32x2_t*)((is_v ? v8 : k8) + rowi * HD + ch * 8) = quant8_e4m3(v, 1.0f / sc);
        if (ch == 0) (is_v ? vscale : kscale)[rowi] = sc;
    }
}

// per-row state of B sequences that grow by st.S[b] tokens (misc.hip: emmax_prefill_state_kernel for a row that keeps its context): base = the
// cached length before, cu = the packed offsets of the new rows, ctx_len += the new rows; done / n_out / token budget / stop match as a prefill
// leaves them.  aut_state / aut_start (an automaton is set, else null): a row keeps its state; one outside the automaton (state -1) enters at its
// start state.  Pointers already offset to the first row
__global__ void emmax_extend_state_kernel(PrefillState st, int32_t* cu, int32_t* base, RowState r, int32_t* aut_state, const int32_t* aut_start) {
    if (threadIdx.x == 0) {
        int acc = 0;
        cu[0] = 0;
        for (int b = 0; b < st.B; ++b) {
            acc += st.S[b];
            cu[b + 1] = acc;
            base[b] = r.ctx_len[b];
            r.ctx_len[b] += st.S[b];
            r.done[b] = 0;
            r.n_out[b] = 0;
            r.max_new[b] = 0x7fffffff;   // no token budget until a generate / slot call sets one
            r.stop_m[b] = 0;
            r.stop_after[b] = -1;
            if (aut_state && aut_state[b] < 0) aut_state[b] = aut_start[b];
        }
    }
}

__device__ __forceinline__ float half_max(float v) {   // max over the two half-waves (lanes l and l ^ 32)
    float a, b;
    swap_halves(v, a, b);
    return fmaxf(a, b);
}
__device__ __forceinline__ float half_sum(float v) {
    float a, b;
    swap_halves(v, a, b);
    return a + b;
}

constexpr int HD = 128, TILE = 64, NW = 4, NT = NW * 64;
constexpr int KP = HD + 8;    // K row pitch in LDS, bf16 elements: 272 B = 16 B x odd (attention.hip: conflict-free ds_read_b128)
constexpr int VP = 160;       // V row pitch: 320 B = 64 B x odd (the four key rows of a transpose read land in different bank quarters)
constexpr int NKK = HD / 16, NDB = HD / 32;

template <int G, bool KV8, bool SPLIT>
__global__ __launch_bounds__(NT) void emmax_extend_attn_kernel(ExtendAttnParams p) {
    constexpr int QT = 128 / G;   // tokens per block
    __shared__ __attribute__((aligned(16))) bf16_t sK[2][TILE * KP];
    __shared__ __attribute__((aligned(16))) bf16_t sV[2][TILE * VP];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hi = lane >> 5;
    const int split = SPLIT ? (int)blockIdx.x : 0, nsplit = SPLIT ? (int)gridDim.x : 1;
    const int hk = (int)blockIdx.y % p.Hkv, qt = (int)blockIdx.y / p.Hkv, b = blockIdx.z;
    const int start = p.cu[b];
    const int n = p.cu[b + 1] - start;
    const int t_blk0 = qt * QT;
    if (n <= 0 || t_blk0 >= n) return;   // past the sequence's real extent
    const int base = max(p.base[b], 0);
    const int Lseq = min(base + n, p.max_pages * TILE);   // keys of the sequence once the append has run (never past the page table)
    int kps = (Lseq + nsplit - 1) / nsplit;
    kps = (kps + 15) & ~15;
    const int Lblk = min(Lseq, base + min(n, t_blk0 + QT));   // the last key any row of the block sees, + 1
    const int k0 = split * kps, k1 = min(Lblk, k0 + kps);

    // this lane's query row, and the wave's first / last token
    const int r = wave * 32 + ql;
    const int t = t_blk0 + r / G, head = hk * G + r % G;
    const bool row_ok = t < n;
    const int tc = min(t, n - 1);                   // (rows past the sequence compute on its last token's window and are never stored)
    const int lim_row = min(k1, base + tc + 1);     // the row sees keys [k0, lim_row)
    const int t_w0 = t_blk0 + (wave * 32) / G;
    const bool wave_live = t_w0 < n;
    const int t_w1 = min(n - 1, t_blk0 + (wave * 32 + 31) / G);
    const int lim_w_min = min(k1, base + min(t_w0, n - 1) + 1), lim_w_max = min(k1, base + t_w1 + 1);

    float* prow = nullptr;
    if constexpr (SPLIT) prow = p.part + (((size_t)(start + tc) * p.Hq + head) * nsplit + split) * PSTRIDE;
    if (k0 >= k1) {   // an empty split: the empty partial of every row of the block
        if constexpr (SPLIT) {
            if (row_ok)
                for (int j = hi * (PSTRIDE / 2); j < (hi + 1) * (PSTRIDE / 2); ++j) prow[j] = (j == HD) ? -INFINITY : 0.f;
        }
        return;
    }

    // Q^T fragments (B operand): lane (ql, hi) holds Q[row][16 kk + 8 hi .. +8]
    bf16x8_t qf[NKK];
    {
        const bf16_t* qrow = (const bf16_t*)p.q + (size_t)(start + tc) * p.ldq + p.q_off + head * HD + hi * 8;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (row_ok) v = *(const u32x4_t*)(qrow + kk * 16);
            qf[kk] = __builtin_bit_cast(bf16x8_t, v);
        }
    }
    f32x16_t o[NDB];
    float m_run = -INFINITY, l_run = 0.f;   // l_run: this lane's share of the row sum (its 16 keys of every 32-key group)
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) o[i][rr] = 0.f;
    const float c = p.scale * 1.44269504088896340736f;   // exp(x * scale) = exp2(x * c)

    // ---- tile staging: thread tid owns the 16-byte chunks tid + 256 i of the page's 64 x 16 (row = chunk / 16) ----
    const int32_t* __restrict__ ptab = p.page_table + (size_t)b * p.max_pages;
    u32x4_t kr[4], vr[4];           // bf16 cache: the chunks;  e4m3 cache: [0..1] the 8 bytes, [2] the row's scale
    auto load_tile = [&](int j) {   // j < max_pages: k1 <= Lseq <= max_pages * TILE
        const int pg = ptab[j];     // block-uniform: one scalar load per tile
        const size_t row0 = ((size_t)pg * p.Hkv + hk) * TILE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ck = tid + NT * i, row = ck >> 4, ch = ck & 15;
            if constexpr (KV8) {
                const u32x2_t k8 = *(const u32x2_t*)((const uint8_t*)p.kcache + (row0 + row) * HD + ch * 8);
                const u32x2_t v8 = *(const u32x2_t*)((const uint8_t*)p.vcache + (row0 + row) * HD + ch * 8);
                kr[i] = (u32x4_t){k8[0], k8[1], __float_as_uint(p.kscale[row0 + row]), 0u};
                vr[i] = (u32x4_t){v8[0], v8[1], __float_as_uint(p.vscale[row0 + row]), 0u};
            } else {
                kr[i] = *(const u32x4_t*)((const bf16_t*)p.kcache + (row0 + row) * HD + ch * 8);
                vr[i] = *(const u32x4_t*)((const bf16_t*)p.vcache + (row0 + row) * HD + ch * 8);
            }
        }
    };
    auto store_tile = [&](int j, int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ck = tid + NT * i, row = ck >> 4, ch = ck & 15;
            u32x4_t k = kr[i], v = vr[i];
            if constexpr (KV8) {   // the e4m3 form widens here
                k = dequant8_e4m3((u32x2_t){kr[i][0], kr[i][1]}, __uint_as_float(kr[i][2]));
                v = dequant8_e4m3((u32x2_t){vr[i][0], vr[i][1]}, __uint_as_float(vr[i][2]));
            }
            if (j * TILE + row >= Lseq) {   // past the sequence's last key: whatever the cache holds there stays out of the products
                k = (u32x4_t){0u, 0u, 0u, 0u};
                v = (u32x4_t){0u, 0u, 0u, 0u};
            }
            *(u32x4_t*)(&sK[buf][row * KP + ch * 8]) = k;
            *(u32x4_t*)(&sV[buf][row * VP + ch * 8]) = v;
        }
    };

    // lane-constant LDS offsets (attention.hip)
    const int k_off = ql * KP + hi * 8;                                        // K fragment: row ql of a 32-key group, + 16 kk
    const int i16 = lane & 15;
    const int v_off = (4 * hi + (i16 >> 2)) * VP + 16 * ((lane >> 4) & 1) + (i16 & 3) * 4;   // + key base * VP + 32 db

    // ---- one softmax step over the 64 keys of a tile.  EDGE steps mask; the others carry no mask code ----
    auto step = [&](auto edge_tag, int kv0, const bf16_t* __restrict__ Kg, const bf16_t* __restrict__ Vg) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        f32x16_t st[2];
#pragma unroll
        for (int gi = 0; gi < 2; ++gi)
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const bf16x8_t kf = *(const bf16x8_t*)(&Kg[gi * 32 * KP + k_off + kk * 16]);
                const f32x16_t zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                st[gi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], kk == 0 ? zero : st[gi], 0, 0, 0);
            }
        if (EDGE) {
            // key of register rr: kv0 + 32 gi + (rr & 3) + 8 (rr >> 2) + 4 hi; visible iff in [k0, lim_row)
            const int lo = k0 - kv0 - 4 * hi, lim = lim_row - kv0 - 4 * hi;
#pragma unroll
            for (int gi = 0; gi < 2; ++gi)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int idx = gi * 32 + (rr & 3) + 8 * (rr >> 2);
                    st[gi][rr] = (idx >= lo && idx < lim) ? st[gi][rr] : -INFINITY;
                }
        }
        float m_tile = st[0][0];
#pragma unroll
        for (int gi = 0; gi < 2; ++gi)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) m_tile = fmaxf(m_tile, st[gi][rr]);
        m_tile = half_max(m_tile);
        // (a row may see no key of a step, or none yet: a split that starts past its diagonal.  Its reference maximum is 0 until it sees one)
        const float m_new = fmaxf(m_run, m_tile);
        const float msafe = (m_new == -INFINITY) ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f((m_run - msafe) * c);
        const float mc = msafe * c;
        m_run = m_new;
        u32x4_t pf[2][2];
        float psum = 0.f;
#pragma unroll
        for (int gi = 0; gi < 2; ++gi)
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(st[gi][8 * mm + 2 * tt], c, -mc));
                    const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(st[gi][8 * mm + 2 * tt + 1], c, -mc));
                    psum += p0 + p1;
                    pf[gi][mm][tt] = pack_bf16x2(p0, p1);
                }
        l_run = __builtin_fmaf(l_run, alpha, psum);
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) o[i][rr] *= alpha;
        // O^T += V^T . P^T : k steps of 16 keys, V^T fragments by the LDS transpose read
#pragma unroll
        for (int gi = 0; gi < 2; ++gi)
#pragma unroll
            for (int mm = 0; mm < 2; ++mm) {
                const bf16_t* vb = Vg + (gi * 32 + mm * 16) * VP + v_off;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;
                    const s16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vb + db * 32));
                    const s16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vb + 8 * VP + db * 32));
                    const u32x2_t w0 = __builtin_bit_cast(u32x2_t, a0), w1 = __builtin_bit_cast(u32x2_t, a1);
                    const u32x4_t av = {w0[0], w0[1], w1[0], w1[1]};
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, av), __builtin_bit_cast(bf16x8_t, pf[gi][mm]), o[db], 0, 0, 0);
                }
            }
    };

    // ---- the tiles [k0 / 64, (k1 - 1) / 64]: tile j + 1 is requested before the math of tile j and written to the other LDS image behind it;
    // the barrier that ends tile j orders both (everybody is done reading image j & 1 before tile j + 2 is written into it) ----
    const int j0 = k0 / TILE, j1 = (k1 - 1) / TILE;
    load_tile(j0);
    store_tile(j0, 0);
    __syncthreads();
    for (int j = j0; j <= j1; ++j) {
        const int buf = (j - j0) & 1, kv0 = j * TILE;
        const bool more = j < j1;   // block-uniform
        if (more) load_tile(j + 1);
        if (wave_live && kv0 < lim_w_max) {   // wave-uniform: a wave skips the tiles past its own last row's diagonal
            if (kv0 < k0 || kv0 + TILE > lim_w_min) step(std::true_type{}, kv0, sK[buf], sV[buf]);
            else step(std::false_type{}, kv0, sK[buf], sV[buf]);
        }
        if (more) store_tile(j + 1, buf ^ 1);
        __syncthreads();
    }

    // ---- lane (ql, hi) holds d = 32 db + 8 a + 4 hi + (0..3) of its row in o[db][4 a .. 4 a + 3] ----
    const float l_tot = half_sum(l_run);
    if (!row_ok) return;
    if constexpr (SPLIT) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int a = 0; a < 4; ++a)
                *(f32x4_t*)(prow + db * 32 + a * 8 + hi * 4) = (f32x4_t){o[db][4 * a], o[db][4 * a + 1], o[db][4 * a + 2], o[db][4 * a + 3]};
        if (hi == 0) {
            prow[HD] = m_run * p.scale;   // in the units of the scaled scores (-inf: the row saw no key of this split)
            prow[HD + 1] = l_tot;
            prow[HD + 2] = 0.f;
            prow[HD + 3] = 0.f;
        }
    } else {
        const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
        bf16_t* orow = (bf16_t*)p.out + (size_t)(start + t) * p.ld_out + head * HD;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                u32x2_t w;
                w[0] = pack_bf16x2(o[db][4 * a] * inv, o[db][4 * a + 1] * inv);
                w[1] = pack_bf16x2(o[db][4 * a + 2] * inv, o[db][4 * a + 3] * inv);
                *(u32x2_t*)(orow + db * 32 + a * 8 + hi * 4) = w;
            }
    }
}

// the splits of a (packed row, head) folded into the bf16 row: weights exp(m_s - M), fp32 (common.h: attn_merge_chunk's arithmetic).  One block
// per packed row, a thread per (head, 8 columns)
__global__ __launch_bounds__(256) void emmax_extend_attn_merge_kernel(const float* __restrict__ part, bf16_t* __restrict__ out, int ld_out,
                                                                     const int32_t* __restrict__ cu, int B, int Hq, int nsplit) {
    const int row = blockIdx.x;
    if (row >= cu[B]) return;
    for (int i = threadIdx.x; i < Hq * (HD / 8); i += blockDim.x) {
        const int head = i / (HD / 8), ch = i - head * (HD / 8);
        const float* sp = part + ((size_t)row * Hq + head) * nsplit * PSTRIDE;
        float M = -INFINITY;
        for (int s = 0; s < nsplit; ++s) M = fmaxf(M, sp[s * PSTRIDE + HD]);
        float den = 0.f, a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < nsplit; ++s) {
            const float ms = sp[s * PSTRIDE + HD];
            const float wgt = (ms == -INFINITY) ? 0.f : __expf(ms - M);
            den = __builtin_fmaf(sp[s * PSTRIDE + HD + 1], wgt, den);
            const f32x4_t o0 = *(const f32x4_t*)(sp + s * PSTRIDE + ch * 8);
            const f32x4_t o1 = *(const f32x4_t*)(sp + s * PSTRIDE + ch * 8 + 4);
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
        *(u32x4_t*)(out + (size_t)row * ld_out + head * HD + ch * 8) = v;
    }
}

}  // namespace

// THE planner, on the host and from shapes alone.  Work items = (sequence, kv head, query tile); while they do not fill the chip's 256 CUs
// the key range is split -- never finer than one page per split, never more than 16 partials per row
bool extend_attn_plan(int B, int max_n, int max_L, int Hq, int Hkv, int nsplit, int kv8, ExtendAttnPlan* f) {
    if (B < 1 || max_n < 1 || max_L < max_n || Hkv < 1 || Hq < 1 || Hq % Hkv || nsplit < 0 || nsplit > 16) return false;
    const int G = Hq / Hkv;
    if (G != 1 && G != 2 && G != 4 && G != 8) return false;
    f->G = G;
    f->qt = 128 / G;
    f->nqt = (max_n + f->qt - 1) / f->qt;
    f->kv8 = kv8 ? 1 : 0;
    const long items = (long)B * Hkv * f->nqt;
    if (nsplit == 0) {
        nsplit = 1;
        if (items < 256) {
            const int pages = (max_L + 63) / 64;
            nsplit = (int)((256 + items - 1) / items);
            if (nsplit > pages) nsplit = pages;
            if (nsplit > 16) nsplit = 16;
        }
    }
    f->nsplit = nsplit;
    f->split = nsplit > 1 ? 1 : 0;
    return true;
}

int launch_rope_kv_write_at(void* qkv, int ld, int q_off, int k_off, int v_off, const int32_t* cu, const int32_t* base, int B, int total_rows,
                            const float* cos_t, const float* sin_t, void* kcache, void* vcache, const int32_t* page_table, int max_pages, int Hq,
                            int Hkv, int hd, int page, int max_pos, hipStream_t stream) {
    // the 16-byte form alone (head_dim % 16 == 0, aligned rows and tables): every model the prefill's own vector pass serves
    const bool vec = (hd & 15) == 0 && ((ld | q_off | k_off | v_off) & 7) == 0 && (((size_t)qkv | (size_t)kcache | (size_t)vcache) & 15) == 0 &&
                     (((size_t)cos_t | (size_t)sin_t) & 15) == 0;
    if (!vec || B < 1 || total_rows < 1 || page < 1 || max_pages < 1 || max_pos < 1) return -1;
    hipLaunchKernelGGL(emmax_rope_kv_write_at_kernel, dim3(total_rows), dim3(256), 0, stream, (bf16_t*)qkv, ld, q_off, k_off, v_off, cu, base, B, cos_t,
                       sin_t, (bf16_t*)kcache, (bf16_t*)vcache, page_table, max_pages, Hq, Hkv, hd, page, max_pos);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_kv_quant_rows_at(const void* qkv, int ld, int k_off, int v_off, const int32_t* cu, const int32_t* base, int B, int total_rows, void* k8,
                            void* v8, float* kscale, float* vscale, const int32_t* page_table, int max_pages, int Hkv, int hd, int page,
                            hipStream_t stream) {
    if (hd != 128 || (ld | k_off | v_off) % 8 || B < 1 || total_rows < 1 || page < 1 || max_pages < 1) return -1;
    hipLaunchKernelGGL(emmax_kv_quant_rows_at_kernel, dim3(total_rows), dim3(256), 0, stream, (const bf16_t*)qkv, ld, k_off, v_off, cu, base, B,
                       (uint8_t*)k8, (uint8_t*)v8, kscale, vscale, page_table, max_pages, Hkv, page);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_extend_state(const PrefillState& st, int32_t* cu, int32_t* base, const RowState& rows, int32_t* aut_state, const int32_t* aut_start,
                        hipStream_t stream) {
    if (st.B < 1 || st.B > EMMAX_MAX_DECODE_BATCH || (aut_state && !aut_start)) return -1;
    hipLaunchKernelGGL(emmax_extend_state_kernel, dim3(1), dim3(64), 0, stream, st, cu, base, rows, aut_state, aut_start);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_extend_attn(const ExtendAttnParams& p, const ExtendAttnPlan& f, int total_rows, hipStream_t stream) {
    if (p.B < 1 || total_rows < 1 || p.max_pages < 1 || p.Hq != p.Hkv * f.G || f.nsplit < 1 || f.nsplit > 16 || f.nqt < 1) return -1;
    if ((p.ldq | p.q_off | p.ld_out) & 7) return -1;
    if (f.kv8 && (!p.kscale || !p.vscale)) return -1;
    if (f.split && !p.part) return -1;
    const dim3 grid(f.nsplit, p.Hkv * f.nqt, p.B), block(NT);
    switch (f.G) {
#define EXT_CASE(GG)                                                                                                              \
    case GG:                                                                                                                      \
        if (f.kv8 && f.split) hipLaunchKernelGGL((emmax_extend_attn_kernel<GG, true, true>), grid, block, 0, stream, p);          \
        else if (f.kv8) hipLaunchKernelGGL((emmax_extend_attn_kernel<GG, true, false>), grid, block, 0, stream, p);               \
        else if (f.split) hipLaunchKernelGGL((emmax_extend_attn_kernel<GG, false, true>), grid, block, 0, stream, p);             \
        else hipLaunchKernelGGL((emmax_extend_attn_kernel<GG, false, false>), grid, block, 0, stream, p);                         \
        break
        EXT_CASE(1); EXT_CASE(2); EXT_CASE(4); EXT_CASE(8);
#undef EXT_CASE
        default: return -1;
    }
    if (hipGetLastError() != hipSuccess) return -4;
    if (f.split) {
        hipLaunchKernelGGL(emmax_extend_attn_merge_kernel, dim3(total_rows), dim3(256), 0, stream, (const float*)p.part, (bf16_t*)p.out, p.ld_out,
                           p.cu, p.B, p.Hq, f.nsplit);
        if (hipGetLastError() != hipSuccess) return -4;
    }
    return 0;
}
