// taps.hip -- what a session hands OUT of a pass it runs anyway (the residual stream, the attention maps): caller-owned fp32 buffers that no
// kernel of the model reads back.  Nothing here touches an existing kernel: the taps read what the passes leave behind.
//
//   emmax_tap_rows_kernel       rows x H of the residual stream (fp32, or bf16 when the stream is bf16) into fp32 rows, a wave per row, 16-byte
//                               accesses, no LDS.  With a weight: the RMSNorm of the row in fp32 with an fp32 result, y = fl(fl(x rstd) w),
//                               rstd = rsqrt(sum x^2 / H + eps) -- HF's last hidden state is norm(h_L), not h_L
//   emmax_attn_probs_kernel     grid (Hkv x query tiles, B), 4 waves: for sequence b, head h and new query row i at position p = base[b] + i the
//                               fp32 row softmax(scale q . K^T) over keys 0 .. p, keys read from the PAGED cache alone (extend_attn.hip's contract:
//                               a prefill's or an extension's append pass, or a decode step's attention launch, has written the row's own key).
//                               base == nullptr: 0 (a prefill).  The block / wave / lane layout, the K tile (one page, 272-byte pitch, widened
//                               from e4m3 and cleared past the sequence's end on its way global -> registers -> LDS, one block-uniform
//                               page-table lookup per tile requested a tile ahead), S^T = K Q^T on v_mfma_f32_32x32x16_bf16 and c = fl(scale log2 e)
//                               are extend_attn.hip's.  There is no V.  TWO passes over the block's keys:
//                                 1: the running maximum m and the fp32 row sum l = sum 2^(fl(s c - m c)), rescaled as the maximum moves
//                                 2: the scores again, and fl(2^(fl(s c - m c)) x fl(1 / l)) stored
//                               Output fp32 [packed row][Hq][ld_keys]: every entry of a live row is written -- probabilities at keys 0 .. p, exact
//                               zeros from p + 1 to ld_keys - 1 (the caller never clears the buffer); rows of other sequences and blocks past a
//                               sequence's real extent write nothing.  The kernel is bound by its stores (a wave's 32 rows x 64 keys of a tile are
//                               8 KB), and the MFMA leaves a lane 4 consecutive keys of ONE row: the tile goes through a per-wave LDS image
//                               (pitch 68 floats) and leaves as 16 lanes x 16 bytes = 256 contiguous bytes of a row per quarter-wave, 4 rows per store
//                               instruction.  ld_keys % 4 == 0 keeps every 16-byte store aligned and wholly inside or outside a row.  The stores are
//                               NON-TEMPORAL: measured against plain ones 0.79 x the time at eight sequences of 768 rows, 0.94 x
//                               at one, no difference where the launch is not store-bound.
// A decode step's form of both kernels (gen_idx != nullptr; the map: cu == nullptr, one row per sequence at base = ctx_len): sequence b's rows land
// gen_idx[b] x gen_stride floats further on -- its slot of a [max_new][...] buffer, the generation index the step's finish is about to fill -- and a
// sequence that is done, or whose index is outside 0 .. max_new - 1, writes nothing; max_new == 1: every live sequence lands in slot 0.
// Lengths live on the device (cu, base); the host sizes the grid from upper bounds.  Nothing indexes the page table past max_pages, and no
// store lands at a key >= ld_keys, whatever base holds.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

template <bool SRC32>
__global__ __launch_bounds__(256) void emmax_tap_rows_kernel(TapRowsParams p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const int H = p.H, ld_src = p.ld_src;
    const float eps = p.eps;
    const bf16_t* __restrict__ w = (const bf16_t*)p.norm_w;
    float* __restrict__ dst = p.dst;
    if (p.gen_idx) {   // a decode step: the row's slot is its generation index; a row that no longer decodes writes nothing
        const int t = p.max_new == 1 ? 0 : p.gen_idx[row];   // (one slot: the single-step form, every live row lands in it)
        if (p.done[row] != 0 || t < 0 || t >= p.max_new) return;
        dst += (size_t)t * p.gen_stride;
    }
    const int srow = p.gather ? min(max(p.gather[row], 0), p.gather_rows - 1) : row;   // (the embedding row of the step's token)
    const void* __restrict__ src = SRC32 ? (const void*)((const float*)p.src + (size_t)srow * ld_src) : (const void*)((const bf16_t*)p.src + (size_t)srow * ld_src);
    constexpr int CE = SRC32 ? 4 : 8;   // elements of a 16-byte chunk of the source
    const int nchunk = H / CE;
    auto chunk = [&](int c, float* v) {
        if constexpr (SRC32) {
            const f32x4_t x = *(const f32x4_t*)((const float*)src + c * 4);
            v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
        } else {
            const u32x4_t x = *(const u32x4_t*)((const bf16_t*)src + c * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[2 * j] = bf_lo(x[j]); v[2 * j + 1] = bf_hi(x[j]); }
        }
    };
    float rstd = 1.f;
    if (w) {
        float ss = 0.f;
        for (int c = lane; c < nchunk; c += 64) {
            float v[CE];
            chunk(c, v);
#pragma unroll
            for (int e = 0; e < CE; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
        }
        rstd = rsqrtf(wave_sum(ss) / (float)H + eps);
    }
    float* d = dst + (size_t)row * H;
    for (int c = lane; c < nchunk; c += 64) {   // (the second read of a row comes from the cache: a row is 16 KB at most)
        float v[CE];
        chunk(c, v);
        if (w) {
            typedef __attribute__((ext_vector_type(CE / 2))) uint32_t wv_t;   // CE bf16 weights: 8 or 16 bytes
            const wv_t wv = *(const wv_t*)(w + c * CE);
#pragma unroll
            for (int e = 0; e < CE; ++e) v[e] = (v[e] * rstd) * ((e & 1) ? bf_hi(wv[e >> 1]) : bf_lo(wv[e >> 1]));
        }
#pragma unroll
        for (int q = 0; q < CE / 4; ++q) *(f32x4_t*)(d + c * CE + 4 * q) = (f32x4_t){v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
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
constexpr int KP = HD + 8;    // K row pitch in LDS, bf16 elements: 272 B = 16 B x odd (extend_attn.hip)
constexpr int PP = TILE + 4;  // pitch of a wave's probability image, floats: 272 B again
constexpr int NKK = HD / 16;

template <int G, bool KV8>
__global__ __launch_bounds__(NT) void emmax_attn_probs_kernel(AttnProbsParams p) {
    constexpr int QT = 128 / G;   // tokens per block
    __shared__ __attribute__((aligned(16))) bf16_t sK[2][TILE * KP];
    __shared__ __attribute__((aligned(16))) float sP[NW][32 * PP];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, hi = lane >> 5;
    const int hk = (int)blockIdx.x % p.Hkv, qt = (int)blockIdx.x / p.Hkv, b = blockIdx.y;
    const int start = p.cu ? p.cu[b] : b;                 // cu == nullptr: one new row per sequence (a decode step)
    const int n = p.cu ? p.cu[b + 1] - start : 1;
    const int t_blk0 = qt * QT;
    if (n <= 0 || t_blk0 >= n) return;   // past the sequence's real extent
    float* __restrict__ probs = p.probs;
    if (p.gen_idx) {   // a decode step: the row's slot is its generation index; a row that no longer decodes writes nothing
        const int gi = p.max_new == 1 ? 0 : p.gen_idx[b];   // (one slot: the single-step form, every live row lands in it)
        if (p.done[b] != 0 || gi < 0 || gi >= p.max_new) return;
        probs += (size_t)gi * p.gen_stride;
    }
    const int base = p.base ? max(p.base[b], 0) : 0;
    const int Lseq = min(base + n, p.max_pages * TILE);         // keys of the sequence (never past the page table)
    const int Lblk = min(Lseq, base + min(n, t_blk0 + QT));     // the last key any row of the block sees, + 1

    // this lane's query row, and the wave's first / last token
    const int r = wave * 32 + ql;
    const int t = t_blk0 + r / G, head = hk * G + r % G;
    const bool row_ok = t < n;
    const int tc = min(t, n - 1);                   // (rows past the sequence compute on its last token's window and are never stored)
    const int lim_row = min(Lblk, base + tc + 1);   // the row sees keys [0, lim_row)
    const int t_w0 = t_blk0 + (wave * 32) / G;
    const bool wave_live = t_w0 < n;
    const int t_w1 = min(n - 1, t_blk0 + (wave * 32 + 31) / G);
    const int lim_w_min = min(Lblk, base + min(t_w0, n - 1) + 1), lim_w_max = min(Lblk, base + t_w1 + 1);

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
    const float c = p.scale * 1.44269504088896340736f;   // exp(x * scale) = exp2(x * c)

    // ---- tile staging: thread tid owns the 16-byte chunks tid + 256 i of the page's 64 x 16 (row = chunk / 16) ----
    const int32_t* __restrict__ ptab = p.page_table + (size_t)b * p.max_pages;
    u32x4_t kr[4];                  // bf16 cache: the chunks;  e4m3 cache: [0..1] the 8 bytes, [2] the row's scale
    auto load_tile = [&](int j) {   // j < max_pages: Lblk <= Lseq <= max_pages * TILE
        const int pg = ptab[j];     // block-uniform: one scalar load per tile
        const size_t row0 = ((size_t)pg * p.Hkv + hk) * TILE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ck = tid + NT * i, row = ck >> 4, ch = ck & 15;
            if constexpr (KV8) {
                const u32x2_t k8 = *(const u32x2_t*)((const uint8_t*)p.kcache + (row0 + row) * HD + ch * 8);
                kr[i] = (u32x4_t){k8[0], k8[1], __float_as_uint(p.kscale[row0 + row]), 0u};
            } else {
                kr[i] = *(const u32x4_t*)((const bf16_t*)p.kcache + (row0 + row) * HD + ch * 8);
            }
        }
    };
    auto store_tile = [&](int j, int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ck = tid + NT * i, row = ck >> 4, ch = ck & 15;
            u32x4_t k = kr[i];
            if constexpr (KV8) k = dequant8_e4m3((u32x2_t){kr[i][0], kr[i][1]}, __uint_as_float(kr[i][2]));   // the e4m3 form widens here
            if (j * TILE + row >= Lseq) k = (u32x4_t){0u, 0u, 0u, 0u};   // past the sequence's last key: whatever the cache holds there stays out
            *(u32x4_t*)(&sK[buf][row * KP + ch * 8]) = k;
        }
    };

    const int k_off = ql * KP + hi * 8;   // K fragment: row ql of a 32-key group, + 16 kk
    // raw scores of the tile's 64 keys: register rr of st[gi] is key 32 gi + (rr & 3) + 8 (rr >> 2) + 4 hi of this lane's row
    auto scores = [&](const bf16_t* __restrict__ Kg, f32x16_t (&st)[2]) {
#pragma unroll
        for (int gi = 0; gi < 2; ++gi)
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const bf16x8_t kf = *(const bf16x8_t*)(&Kg[gi * 32 * KP + k_off + kk * 16]);
                const f32x16_t zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                st[gi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], kk == 0 ? zero : st[gi], 0, 0, 0);
            }
    };

    // ---- pass 1: one online step over a tile.  EDGE steps mask; the others carry no mask code ----
    float m_run = -INFINITY, l_run = 0.f;   // l_run: this lane's share of the row sum (its 16 keys of every 32-key group)
    auto step1 = [&](auto edge_tag, int kv0, const bf16_t* __restrict__ Kg) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        f32x16_t st[2];
        scores(Kg, st);
        if (EDGE) {
            const int lim = lim_row - kv0 - 4 * hi;
#pragma unroll
            for (int gi = 0; gi < 2; ++gi)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) st[gi][rr] = (gi * 32 + (rr & 3) + 8 * (rr >> 2) < lim) ? st[gi][rr] : -INFINITY;
        }
        float m_tile = st[0][0];
#pragma unroll
        for (int gi = 0; gi < 2; ++gi)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) m_tile = fmaxf(m_tile, st[gi][rr]);
        m_tile = half_max(m_tile);
        const float m_new = fmaxf(m_run, m_tile);
        const float msafe = (m_new == -INFINITY) ? 0.f : m_new;   // (a row past its diagonal in this tile and without a key so far: never a live row)
        const float alpha = __builtin_amdgcn_exp2f((m_run - msafe) * c);
        const float mc = msafe * c;
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int gi = 0; gi < 2; ++gi)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) psum += __builtin_amdgcn_exp2f(__builtin_fmaf(st[gi][rr], c, -mc));
        l_run = __builtin_fmaf(l_run, alpha, psum);
    };

    // ---- pass 2: the tile's probabilities into the wave's LDS image, then out along the key axis ----
    float mc_fin = 0.f, inv_fin = 0.f;
    float* __restrict__ sPw = sP[wave];
    auto emit = [&](int kv0, const bf16_t* __restrict__ Kg) {
        f32x16_t st[2];
        scores(Kg, st);
        const int lim = lim_row - kv0 - 4 * hi;
#pragma unroll
        for (int gi = 0; gi < 2; ++gi)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                f32x4_t v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = __builtin_amdgcn_exp2f(__builtin_fmaf(st[gi][4 * a + e], c, -mc_fin)) * inv_fin;
                    v[e] = (gi * 32 + 8 * a + e < lim) ? x : 0.f;   // above the diagonal: an exact zero
                }
                *(f32x4_t*)(sPw + ql * PP + gi * 32 + 8 * a + 4 * hi) = v;
            }
    };
    // the wave's 32 rows x 64 keys of tile kv0: quarter-wave q writes 256 contiguous bytes of row 4 i + q.  from_lds false: zeros
    const size_t out_row0 = (size_t)(start + t_blk0) * p.Hq + hk * G;
    auto flush = [&](int kv0, bool from_lds) {
        const int col = 4 * (lane & 15);
        if (kv0 + col >= p.ld_keys) return;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rw = 4 * i + (lane >> 4), rr = wave * 32 + rw;
            if (t_blk0 + rr / G >= n) continue;   // a row past the sequence
            f32x4_t v = {0.f, 0.f, 0.f, 0.f};
            if (from_lds) v = *(const f32x4_t*)(sPw + rw * PP + col);
            f32x4_t* dst = (f32x4_t*)(probs + (out_row0 + (size_t)(rr / G) * p.Hq + rr % G) * p.ld_keys + kv0 + col);
#ifdef EMMAX_PROBS_PLAIN_STORES   // the A/B partner of the measurement: `make plain-stores`, tools/taps_bench.py --lib-b
            *dst = v;
#else
            __builtin_nontemporal_store(v, dst);   // (nothing on the device reads it back)
#endif
        }
    };

    // ---- the tiles [0, (Lblk - 1) / 64], twice: tile u + 1 is requested before the math of tile u and written to the other LDS image behind it;
    // the barrier that ends a tile orders both (extend_attn.hip).  Pass 2 starts while pass 1's last tile is still being computed ----
    const int nt = (Lblk - 1) / TILE + 1;
    load_tile(0);
    store_tile(0, 0);
    __syncthreads();
    for (int u = 0; u < 2 * nt; ++u) {
        const int j = u < nt ? u : u - nt, buf = u & 1, kv0 = j * TILE;
        const bool more = u + 1 < 2 * nt;   // block-uniform
        const int jn = u + 1 < nt ? u + 1 : u + 1 - nt;
        if (more) load_tile(jn);
        if (u < nt) {
            if (wave_live && kv0 < lim_w_max) {   // wave-uniform: a wave skips the tiles past its own last row's diagonal
                if (kv0 + TILE > lim_w_min) step1(std::true_type{}, kv0, sK[buf]);
                else step1(std::false_type{}, kv0, sK[buf]);
            }
        } else {
            if (u == nt) {
                const float l_tot = half_sum(l_run);
                inv_fin = l_tot > 0.f ? 1.0f / l_tot : 0.f;
                mc_fin = (m_run == -INFINITY ? 0.f : m_run) * c;
            }
            if (wave_live) {
                if (kv0 < lim_w_max) {
                    emit(kv0, sK[buf]);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the image is read across lanes: LDS runs in order inside a wave
                    __builtin_amdgcn_wave_barrier();
                    flush(kv0, true);
                    __builtin_amdgcn_wave_barrier();
                } else {
                    flush(kv0, false);
                }
            }
        }
        if (more) store_tile(jn, buf ^ 1);
        __syncthreads();
    }
    // ---- the keys no row of the block sees, up to ld_keys: zeros ----
    if (wave_live)
        for (int kv0 = nt * TILE; kv0 < p.ld_keys; kv0 += TILE) flush(kv0, false);
}

}  // namespace

int launch_tap_rows(const TapRowsParams& p, hipStream_t stream) {
    if (p.rows <= 0) return 0;
    if (!p.src || !p.dst || p.H < 8 || p.H % 8 || p.ld_src < p.H || p.ld_src % (p.src_f32 ? 4 : 8) || (((size_t)p.src | (size_t)p.dst | (size_t)p.norm_w) & 15)) return -1;
    if (p.gen_idx && (!p.done || p.max_new < 1 || (p.gen_stride & 3))) return -1;
    if (p.gather && p.gather_rows < 1) return -1;
    const dim3 grid((p.rows + 3) / 4), block(256);
    if (p.src_f32) hipLaunchKernelGGL((emmax_tap_rows_kernel<true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((emmax_tap_rows_kernel<false>), grid, block, 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_attn_probs(const AttnProbsParams& p, int max_n, int kv8, hipStream_t stream) {
    if (p.B < 1 || p.B > 65535 || max_n < 1 || p.max_pages < 1 || p.Hkv < 1 || p.Hq < 1 || p.Hq % p.Hkv) return -1;
    if (!p.q || !p.kcache || !p.page_table || !p.probs || (kv8 && !p.kscale)) return -1;
    if (p.gen_idx && (!p.done || p.max_new < 1 || (p.gen_stride & 3))) return -1;
    if ((p.ldq | p.q_off) & 7 || p.ld_keys < 4 || (p.ld_keys & 3) || ((size_t)p.probs & 15)) return -1;
    const int G = p.Hq / p.Hkv;
    if (G != 1 && G != 2 && G != 4 && G != 8) return -1;
    const int qt = 128 / G, nqt = (max_n + qt - 1) / qt;
    const dim3 grid(p.Hkv * nqt, p.B), block(NT);
    switch (G) {
#define PROBS_CASE(GG)                                                                                                  \
    case GG:                                                                                                            \
        if (kv8) hipLaunchKernelGGL((emmax_attn_probs_kernel<GG, true>), grid, block, 0, stream, p);                    \
        else hipLaunchKernelGGL((emmax_attn_probs_kernel<GG, false>), grid, block, 0, stream, p);                       \
        break
        PROBS_CASE(1); PROBS_CASE(2); PROBS_CASE(4); PROBS_CASE(8);
#undef PROBS_CASE
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
