// decode_km.hip -- batch 3-16 decode projections with K <= 4096 on MFMA, K split across the waves of a block ("km"; round 5: rows 9-16 --
// the batch is the 16-wide N side of the MFMA -- through the template argument NB; batches 17-32 are routed to decode_kmp.hip).
// Replaces the q_len == 1 linears of HF `LlamaDecoderLayer` at small batch (cached branch of
// prismatic/extern/hf/modeling_prismatic.py:325-341; the configs[2] per-GPU shard), like decode_mfma.hip, with the structure
// that made the batch-1 kernel of decode_ks.hip faster:
//
//   * one block of 8 waves per CU; wave w owns the k-steps [w KT/8, (w+1) KT/8) of EVERY 16-row tile of the block.  Its slice of
//     the activations lives in registers for the whole launch, already in MFMA B-operand form (16 fragments of 8 bf16 per lane:
//     batch row = lane & 15, rows past the batch are zero) -- no LDS stage, no barrier in front of the weight stream, no LDS
//     read per MFMA;
//   * weights stream from a fragment-major copy (one 1 KiB tile = the A operand of one v_mfma_f32_16x16x32_bf16) with
//     non-temporal buffer loads, the tile in an SGPR offset: TWO tiles (32 KiB) per wave in flight, i.e. 64 MB on the chip like
//     the batch-1 kernel (decode_mfma.hip keeps 16 MB in flight: at ~3 us of loaded latency that alone bounds it near 5.3 TB/s);
//     every load is unconditional (tiles / steps past the end carry an out-of-range offset and return zeros for free), so the
//     waits are counted;
//   * the eight K-slice partial tiles meet in LDS once, at the end of the block, where the fused epilogues run;
//   * the pairs the epilogues need live INSIDE a tile: the qkv and gate/up copies are row-permuted when they are built (rows
//     0-7 of a tile = elements d .. d+7 of a head / gate rows, rows 8-15 = d+64 .. d+71 / the matching up rows), so the work
//     unit is ONE tile for every matrix: 768 qkv tiles are 3 per block (as 384 two-tile tasks they were 1.5 and needed the
//     stream-K split of decode_mfma.hip);
//   * RMSNorm folded in as in decode_ks.hip: y = rstd * W (x .* g), the sum of squares per wave slice, 1/rms in the epilogue.
// The down projection (K = 11008: 43 k-steps per wave would need 172 activation registers) has its own two-phase kernel below
// (emmax_decode_kmd_kernel).
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "decode_epilogue.h"

namespace {

constexpr int KM_WAVES = 8;
constexpr int KM_NT = KM_WAVES * 64;
constexpr int KM_STEPS = 16;      // bf16 k-steps (32 elements) per tile and wave: K <= 8 * 16 * 32 = 4096
constexpr int KM_MAX_TILES = 8;   // tiles per block the LDS partial sums hold
constexpr int PSTRIDE = EMMAX_PSTRIDE;

// row-major [N, ld] -> fragment-major tiles in the km row order (N % 16 == 0, K % 32 == 0)
__global__ __launch_bounds__(256) void emmax_repack_km_kernel(const bf16_t* __restrict__ src, int ld, u32x4_t* __restrict__ dst, int N, int K,
                                                             int perm, int head_dim) {
    const size_t total = (size_t)N * K / 8;
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < total; c += (size_t)gridDim.x * 256) {
        const int lane = (int)(c & 63);
        const size_t tile = c >> 6;
        const int kt = (int)(tile % (K / 32)), nt = (int)(tile / (K / 32));
        const int n = km_src_row(perm, head_dim, nt, lane & 15), k = kt * 32 + (lane >> 4) * 8;
        dst[c] = *(const u32x4_t*)(src + (size_t)n * ld + k);
    }
}

// ---- MXFP4 copies (kernels.h: launch_quant_mx) -- integer arithmetic only, so that bf16 denormals and the clamped exponent come out as the
// format defines them whatever the float modes are.  One thread per (tile, row): 128 k = four blocks, 16 dwords of elements + one of codes.
// |w| = S 2^q with S the 8-bit significand; x = |w| / 2^e as the fixed-point number x 2^42, compared with the midpoints of the e2m1 grid
// (ties to the even code: <= below an even code's upper midpoint, < below an odd one's)
__device__ __forceinline__ uint32_t mx4_code(uint32_t mag /* bf16 bits without the sign */, int e) {
    const int E = (int)(mag >> 7);
    const uint64_t S = E ? (0x80u | (mag & 0x7fu)) : (mag & 0x7fu);
    const int sh = (E ? E : 1) - 127 - 7 - e + 42;   // x 2^42 = S << sh;  x < 8 (or saturates): sh <= 38
    const uint64_t x = sh < 0 ? 0 : sh > 40 ? ~0ull : (S << sh);
    const uint64_t q = 1ull << 40;   // 0.25
    return x <= q ? 0u : x < 3 * q ? 1u : x <= 5 * q ? 2u : x < 7 * q ? 3u : x <= 10 * q ? 4u : x < 14 * q ? 5u : x <= 20 * q ? 6u : 7u;
}
// bf16 bits of +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}[code & 7] 2^e, e in [-127, 127] (denormal results included)
__device__ __forceinline__ uint32_t mx4_value_bits(uint32_t code, int e) {
    const uint32_t c = code & 7u, sign = (code & 8u) << 12;
    if (!c) return 0u;   // (zeros are +0 whatever the sign nibble says)
    const int p = e + (c == 1 ? -1 : (int)(c >> 1) - 1);   // value = (1 + man / 2) 2^p
    const uint32_t man = c == 1 ? 0u : (c & 1u);
    if (p >= -126) return sign | ((uint32_t)(p + 127) << 7) | (man << 6);
    return sign | ((2u + man) << (p + 132));            // p = -127, -128: (2 + man) 2^(p - 1) in units of 2^-133
}
// what the block-scaled formats share.  The e8m0 code of a block from its largest magnitude (bf16 bits without the sign): floor(log2(amax)) - 2 clamped at
// -127 (bf16 cannot reach the upper clamp) -- the exponent field less 2, zero for denormals; an all-zero block: 127
__device__ __forceinline__ uint32_t mx_block_amax(const u32x4_t (&v)[4]) {
    uint32_t amax = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int d = 0; d < 4; ++d) amax = max(amax, max(v[g][d] & 0x7fffu, (v[g][d] >> 16) & 0x7fffu));
    return amax;
}
__device__ __forceinline__ int mx_block_code(uint32_t amax) {
    const int E = (int)(amax >> 7);
    return amax == 0 ? 127 : max(E - 2, 0);
}
// (the (tile, row) index prologue stays written out in the four kernels below: shared as a device function it changes their instruction streams)
__global__ __launch_bounds__(256) void emmax_quant_mx4_kernel(const bf16_t* __restrict__ src, int ld, uint32_t* __restrict__ tiles, uint32_t* __restrict__ scales,
                                                             int N, int K, int perm, int head_dim) {
    const int KT = K / 128;
    const size_t total = (size_t)N * KT;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i & 15);
        const size_t tile = i >> 4;
        const int kt = (int)(tile % KT), nt = (int)(tile / KT);
        const bf16_t* row = src + (size_t)km_src_row(perm, head_dim, nt, r) * ld + (size_t)kt * 128;
        uint32_t codes = 0;
        for (int j = 0; j < 4; ++j) {
            u32x4_t v[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) v[g] = *(const u32x4_t*)(row + j * 32 + g * 8);
            const int code = mx_block_code(mx_block_amax(v));
            const int e = code - 127;
            codes |= (uint32_t)code << (8 * j);
#pragma unroll
            for (int g = 0; g < 4; ++g) {   // lane (g, r) of the tile: dword j = its 8 elements of MFMA step j
                uint32_t q = 0;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const uint32_t lo = v[g][d] & 0xffffu, hi = v[g][d] >> 16;
                    q |= (mx4_code(lo & 0x7fffu, e) | ((lo >> 12) & 8u)) << (8 * d);
                    q |= (mx4_code(hi & 0x7fffu, e) | ((hi >> 12) & 8u)) << (8 * d + 4);
                }
                tiles[(tile * 64 + (size_t)(g * 16 + r)) * 4 + j] = q;
            }
        }
        scales[i] = codes;
    }
}
__global__ __launch_bounds__(256) void emmax_dequant_mx4_kernel(const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ scales, bf16_t* __restrict__ dst,
                                                               int ld, int N, int K, int perm, int head_dim) {
    const int KT = K / 128;
    const size_t total = (size_t)N * KT * 16;   // one thread per (tile, lane, dword): 8 elements
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int j = (int)(i & 3), lane = (int)((i >> 2) & 63), r = lane & 15, g = lane >> 4;
        const size_t tile = i >> 8;
        const int kt = (int)(tile % KT), nt = (int)(tile / KT);
        const uint32_t q = tiles[i];
        const int e = (int)((scales[tile * 16 + r] >> (8 * j)) & 0xffu) - 127;
        u32x4_t o;
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = mx4_value_bits(q >> (8 * d), e) | (mx4_value_bits(q >> (8 * d + 4), e) << 16);
        *(u32x4_t*)(dst + (size_t)km_src_row(perm, head_dim, nt, r) * ld + (size_t)kt * 128 + j * 32 + g * 8) = o;
    }
}

// ---- MXFP6 e2m3 copies (kernels.h: launch_quant_mx) -- the same integer arithmetic, blocks, scale rule and scale stream as the MXFP4 pair.
// x = |w| / 2^e as the fixed-point number x 2^42 (mx4_code above); the grid's step is 1/8 below 2 (subnormals and the first binade), 1/4 in
// [2, 4), 1/2 in [4, 8): round to nearest in the binade's step, ties to the even multiple -- a carry into the next binade lands on its first
// code, which is even -- and saturate at code 31 (7.5)
__device__ __forceinline__ uint32_t mx6_code(uint32_t mag /* bf16 bits without the sign */, int e) {
    const int E = (int)(mag >> 7);
    const uint64_t S = E ? (0x80u | (mag & 0x7fu)) : (mag & 0x7fu);
    const int sh = (E ? E : 1) - 127 - 7 - e + 42;
    const uint64_t x = sh < 0 ? 0 : (S << min(sh, 50));   // (2^50 and above saturate like anything from 7.75 on)
    const int b = x < (2ull << 42) ? 39 : x < (4ull << 42) ? 40 : 41;   // log2 of the step in units of 2^-42
    const uint64_t n = (x + ((1ull << (b - 1)) - 1) + ((x >> b) & 1ull)) >> b;
    const uint32_t code = (uint32_t)n + (b == 39 ? 0u : b == 40 ? 8u : 16u);   // [2, 4): n = 8 .. 16 -> codes 16 .. 24; [4, 8): -> 24 .. 32
    return min(code, 31u);
}
// bf16 bits of the e2m3 value of the 6-bit code times 2^e, e in [-127, 127]: I 2^t with I = 1 .. 15 (exact, denormal results included; past the
// largest bf16: infinity)
__device__ __forceinline__ uint32_t mx6_value_bits(uint32_t code, int e) {
    const uint32_t c = code & 31u, sign = (code & 32u) << 10;
    if (!c) return 0u;
    const uint32_t I = c < 8 ? c : (8u | (c & 7u));
    const int t = e - 3 + (c < 16 ? 0 : (int)(c >> 3) - 1);
    const int hb = 31 - __clz((int)I);
    const int P = t + hb;
    if (P > 127) return sign | 0x7f80u;
    if (P >= -126) return sign | ((uint32_t)(P + 127) << 7) | ((I << (7 - hb)) & 0x7fu);
    return sign | (I << (t + 133));   // t >= -130
}
// One thread per (tile, row): 128 k = four blocks; block g of row r is lane 16 g + r of the tile: dwords 0-3 of its six in the tile's first KiB, 4-5 behind it
__global__ __launch_bounds__(256) void emmax_quant_mx6_kernel(const bf16_t* __restrict__ src, int ld, uint32_t* __restrict__ tiles, uint32_t* __restrict__ scales,
                                                             int N, int K, int perm, int head_dim) {
    const int KT = K / 128;
    const size_t total = (size_t)N * KT;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i & 15);
        const size_t tile = i >> 4;
        const int kt = (int)(tile % KT), nt = (int)(tile / KT);
        const bf16_t* row = src + (size_t)km_src_row(perm, head_dim, nt, r) * ld + (size_t)kt * 128;
        uint32_t codes = 0;
        for (int g = 0; g < 4; ++g) {
            u32x4_t v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = *(const u32x4_t*)(row + g * 32 + c * 8);
            const int code = mx_block_code(mx_block_amax(v));
            const int e = code - 127;
            codes |= (uint32_t)code << (8 * g);
            uint32_t q[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    const uint32_t h = (v[c][d >> 1] >> (16 * (d & 1))) & 0xffffu;
                    const uint32_t el = mx6_code(h & 0x7fffu, e) | ((h >> 10) & 32u);
                    const int bit = 6 * (8 * c + d);   // element i of the block in bits [6 i, 6 i + 6) of the 192
                    q[bit >> 5] |= el << (bit & 31);
                    if ((bit & 31) > 26) q[(bit >> 5) + 1] |= el >> (32 - (bit & 31));
                }
            const size_t lane = (size_t)(g * 16 + r);
#pragma unroll
            for (int d = 0; d < 4; ++d) tiles[tile * 384 + lane * 4 + d] = q[d];
            tiles[tile * 384 + 256 + lane * 2] = q[4];
            tiles[tile * 384 + 256 + lane * 2 + 1] = q[5];
        }
        scales[i] = codes;
    }
}
__global__ __launch_bounds__(256) void emmax_dequant_mx6_kernel(const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ scales, bf16_t* __restrict__ dst,
                                                               int ld, int N, int K, int perm, int head_dim) {
    const int KT = K / 128;
    const size_t total = (size_t)N * KT * 16;   // one thread per (tile, lane, quarter): 8 elements
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i & 3), lane = (int)((i >> 2) & 63), r = lane & 15, g = lane >> 4;
        const size_t tile = i >> 8;
        const int kt = (int)(tile % KT), nt = (int)(tile / KT);
        uint32_t q[6];
#pragma unroll
        for (int d = 0; d < 4; ++d) q[d] = tiles[tile * 384 + (size_t)lane * 4 + d];
        q[4] = tiles[tile * 384 + 256 + (size_t)lane * 2];
        q[5] = tiles[tile * 384 + 256 + (size_t)lane * 2 + 1];
        const int e = (int)((scales[tile * 16 + r] >> (8 * g)) & 0xffu) - 127;
        uint32_t h[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int bit = 6 * (8 * c + d);
            uint32_t el = q[bit >> 5] >> (bit & 31);
            if ((bit & 31) > 26) el |= q[(bit >> 5) + 1] << (32 - (bit & 31));
            h[d] = mx6_value_bits(el & 63u, e);
        }
        const u32x4_t o = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
        *(u32x4_t*)(dst + (size_t)km_src_row(perm, head_dim, nt, r) * ld + (size_t)kt * 128 + g * 32 + c * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// grid: one block per CU; block b owns a contiguous range of tiles (launcher: at most KM_MAX_TILES).
// Dynamic LDS: float part[8 waves][tiles_cap][64][4] + float sumsq[8][16] + the activation staging (XATTN: the merged rows, bf16
// [B][K]; else one window of 8 row slices per wave).
// FP8: the tiles are e4m3 (16 rows x 64 k per KiB, decode_mfma.hip's emmax_quant_fm8_kernel layout) + one fp32 scale per row,
// de-quantised in registers (exact), two MFMAs per load.
// ---------------------------------------------------------------------------------------------------------------------
// (v_mfma_f32_16x16x32_fp8_fp8 on e4m3-quantised activations was measured in round 3: no faster -- the kernel is memory-bound by 14x --
// and 1.0e-1 of max|logit| from the oracle; removed from the product source)
// R32 (RESID modes): the residual stream's master copy is the fp32 buffer p.h32 (GemvParams) -- the epilogue adds into it and mirrors
// the sum into the bf16 rows p.y, which is what the NORM modes of this file read (fetching the fp32 rows instead cost the batch-8
// step 1.5 %: twice the prologue bytes in front of every qkv / gate-up / lm-head launch; the rounding that matters -- the one that
// used to accumulate over the 64 additions of a token -- is gone either way)
// NB: batch rows the prologue stages (8: batch <= 8; 16: batch 9-16 -- round 5: the batch is the 16-wide N side of the MFMA, columns 8-15
// were zeros until then).  LDS (not XATTN): ONE region per wave -- its activation window [NB][XPITCH] during the prologue, its partial
// tiles [tiles_cap][64][4] afterwards (the window is dead once the wave holds its fragments; nobody else touches the region before
// the block's only barrier) -- then sumsq[8][16]: 8 x 16.25 KiB at NB = 16, where window + partial tiles side by side would not fit.
// ROLL (tuning switch km_roll): a weight register is refilled with its step of the tile two ahead as soon as its MFMA has issued (32 KiB
// per wave in flight at all times) instead of all sixteen once the tile is done (16-32 KiB)
// EX (exact numerics, round 6, batch 3-8; NB = 16): the activations arrive as fp32 rows and enter the MFMA as two bf16 terms -- the hi terms of row b in
// batch column b, the lo terms in column b + 8: the eight columns a batch <= 8 leaves empty carry the second term, so the weight stream, the
// MFMA count and the register budget are those of the plain kernel; the epilogue adds columns b and b + 8 and hands fp32 results on (fp32 q rows,
// fp32 RoPE with torch's per-product rounding, the 24-bit / fp32 cache, the SwiGLU product in fp32) as decode_ks.hip's EX form does at batch 1-2.
// register state of the block-scaled forms (WF below): QD sets of a tile's QS load steps -- per step the lane's 16 bytes and the row's scale dword; MX6: also
// dwords 4-5 of the lane's six (an 8-byte load).  Nothing in the other forms: everything that touches it sits under `if constexpr (MX)`
template <int WF, int QD, int QS> struct MxTiles {};
template <int QD, int QS> struct MxTiles<PW_MX4, QD, QS> { u32x4_t w[QD][QS]; uint32_t s[QD][QS]; };
template <int QD, int QS> struct MxTiles<PW_MX6, QD, QS> { u32x4_t w[QD][QS]; u32x2_t h[QD][QS]; uint32_t s[QD][QS]; };
// WF (weight format of the tiles, kernels.h: WFMT): PW_BF16; PW_FP8 (above); PW_MX4: OCP MXFP4 -- e2m1 elements, one e8m0 scale per 32 k of a row.  One 1 KiB tile =
// 16 rows x 128 k: lane l holds row l & 15, dword j of its 16 bytes = the 8 k of group l >> 4 of the tile's j-th 32-wide MFMA step (element e in
// nibble e), so ONE load feeds four MFMAs; the scales are a second stream in the same tile order, one dword of four e8m0 codes per (tile, row)
// = 64 B per tile, fetched by the sixteen rows' lanes as one request.  v_cvt_scalef32_pk_bf16_fp4 widens two elements and applies the block
// scale (the code shifted into an fp32 exponent); a de-quantised value is exact in bf16, so MFMA, prologues and epilogues are the bf16 form's.
// Four tiles (16 KiB + scales) per wave in flight.
// PW_MX6: OCP MXFP6 e2m3, the same blocks and scale stream.  One tile = 16 rows x 128 k = 1536 B: lane l (row l & 15, g = l >> 4) owns the 32 elements of
// scale block g of its row -- six dwords, 16 bytes at 16 l of the tile's first KiB and 8 bytes at 8 l of the 512 B behind it, both requests contiguous
// across the wave -- because v_cvt_scalef32_pk32_bf16_fp6 takes ONE scale for its 32 elements.  One conversion gives the lane the A fragments of the
// step's four MFMAs: MFMA j takes elements 8 j .. 8 j + 7 = k0 + 32 g + 8 j + (0 .. 7), where the MX4 form has k0 + 32 j + 8 g -- so the activation
// fragments of these instantiations are fetched with the roles of j and g exchanged (x_chunk below; the blocks stay contiguous in k as OCP defines them).
// Three tiles (18 KiB + scales) per wave in flight: six dwords a step and the conversion's sixteen result registers leave room for no fourth set.
template <int MODE, bool NORM, bool XATTN, int WF, bool R32, int NB, bool ROLL, bool EX = false>
__global__ __launch_bounds__(KM_NT, 2) void emmax_decode_km_kernel(GemvParams p) {
    constexpr bool FP8 = WF == PW_FP8, MX4 = WF == PW_MX4, MX6 = WF == PW_MX6, MX = wfmt_is_mx(WF);
    static_assert(!EX || (NB == 16 && WF == PW_BF16 && !ROLL), "exact numerics: sixteen window rows = eight batch rows x two terms, bf16 weights");
    extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g4 = lane >> 4, c16 = lane & 15;
    const int B = p.batch, K = p.K;
    constexpr int KS = WFMT[WF].ks;               // elements per load step
    constexpr int NSTEP = KM_STEPS * 32 / KS;     // load steps per tile and wave
    const int KT = K / KS;                        // load steps of a whole row
    const int KTW = KT / KM_WAVES;                // ... of this wave's slice (launcher: K % (8 * KS) == 0, KTW <= NSTEP)
    const int tiles_cap = p.kc;                   // launcher
    constexpr int XPITCH = KM_STEPS * 64 + 16;    // bytes per staged row slice (+16: the four k-groups of a fragment read hit different banks)
    // bytes of a wave's region: XATTN: its partial tiles only (the merged rows [B][K] bf16 follow the regions and sumsq)
    const int wreg = XATTN ? tiles_cap * 1024 : max(NB * XPITCH, tiles_cap * 1024);
    auto part_of = [&](int w) { return (float*)(km_smem + (size_t)w * wreg); };   // [tiles_cap][64][4]
    float* sumsq = (float*)(km_smem + (size_t)KM_WAVES * wreg);      // [KM_WAVES][16]
    unsigned char* xlds = (unsigned char*)(sumsq + KM_WAVES * 16);   // XATTN: the merged rows [B][K] bf16 (EX: [16][K], rows b / b + 8 = the two terms)
    auto col_live = [&](int c) { return EX ? (c & 7) < B : c < B; };   // batch column c of the MFMA carries a row

    const int G = gridDim.x, bid = blockIdx.x;
    const int n_tiles = p.n_groups;
    const int tq = n_tiles / G, tr = n_tiles % G;
    const int t_lo = bid * tq + min(bid, tr), ntb = tq + (bid < tr ? 1 : 0);

    // ---- epilogue operands of this thread's (tile, lane) slot, requested before anything else ----
    // thread (tl = tid >> 6, l = tid & 63) finalises tile tl of the block: rows 4 (l >> 4) + j, batch column l & 15
    const int e_tl = tid >> 6, e_l = lane, e_c = e_l & 15, e_rq = e_l >> 4;
    const bool e_pairs = MODE == GEMV_QKV || MODE == GEMV_GATEUP;          // rows r, r + 8 of a tile belong together
    const bool e_on = e_tl < ntb && e_c < B && (!EX || e_c < 8) && (!e_pairs || e_rq < 2);
    const int e_tile = t_lo + min(e_tl, max(ntb - 1, 0));
    float pre_a[4] = {0.f, 0.f, 0.f, 0.f}, pre_b[4] = {0.f, 0.f, 0.f, 0.f};
    int pre_pos = 0, pre_pg = 0;
    if (e_on) tile4_prefetch<MODE, R32>(p, e_c, e_tile, e_rq, pre_a, pre_b, pre_pos, pre_pg);

    // ---- weight stream: buffer loads, the (tile, step) offset in an SGPR, the lane's 16 bytes in the VGPR offset ----
    // (16 rows x K x 1 or 2 bytes keeps the parent's spelling: as one factor wfmt_bytes_per_k, or behind a helper, every bf16 kernel's scalar multiplies change operand order)
    const unsigned w_bytes = wfmt_is_mx(WF) ? (unsigned)((size_t)p.n_groups * wfmt_bytes_per_k(WF) * (size_t)K) : (unsigned)((size_t)p.n_groups * 16 * (size_t)K * (FP8 ? 1 : 2));
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (int)w_bytes, 0x00020000);
    const unsigned voff = (unsigned)lane * 16u;
    u32x4_t wa[NSTEP], wb[NSTEP];   // two tiles in flight
    auto issue_one = [&](u32x4_t (&w)[NSTEP], int tl, int s) {   // step s of tile tl of the block (uniform); past the end: out of range = zeros, no traffic
        const int ok = (tl < ntb && s < KTW) ? -1 : 0;
        const unsigned so = ((unsigned)(((t_lo + tl) * KT + wave * KTW + s) * WFMT[WF].tile_bytes) & (unsigned)ok) | (w_bytes & (unsigned)~ok);
        w[s] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, voff, so, 2));   // aux 2 = nt
    };
    auto issue = [&](u32x4_t (&w)[NSTEP], int tl) {
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) issue_one(w, tl, s);
    };
    // block-scaled tiles: QD register sets of a tile's four load steps (MX4: four; MX6: three -- six dwords a step and the conversion's sixteen result registers
    // leave room for no fourth), and each step's scale dword (the rows' lanes: 4 bytes at 4 (lane & 15) of the tile's 64)
    constexpr int QD = MX6 ? 3 : 4, QS = NSTEP;
    MxTiles<WF, QD, QS> q;
    auto issue_mx_one = [&](int d, int tl, int s) {   // step s of tile tl of the block into set d (uniform); past the block's tiles or the wave's slice every offset
        if constexpr (MX) {                            // is masked past its descriptor: zeros, no traffic, scale code 0
            const unsigned s_bytes = w_bytes / (unsigned)(WFMT[WF].tile_bytes / WFMT_SCALE_BYTES);
            const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.w_codes, 0, (int)s_bytes, 0x00020000);
            const int ok = (tl < ntb && s < KTW) ? -1 : 0;
            const unsigned ti = (unsigned)((t_lo + tl) * KT + wave * KTW + s);
            const unsigned so = ((ti * (unsigned)WFMT[WF].tile_bytes) & (unsigned)ok) | (w_bytes & (unsigned)~ok);
            q.w[d][s] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, voff, so, 2));
            if constexpr (MX6) q.h[d][s] = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(wrsrc, 1024u + (unsigned)lane * 8u, so, 2));
            q.s[d][s] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(srsrc, (unsigned)c16 * 4u, ((ti * (unsigned)WFMT_SCALE_BYTES) & (unsigned)ok) | (s_bytes & (unsigned)~ok), 2);
        }
    };
    auto issue_mx = [&](int d, int tl) {
#pragma unroll
        for (int s = 0; s < QS; ++s) issue_mx_one(d, tl, s);
    };
    auto issue_first = [&]() { if constexpr (MX) issue_mx(0, 0); else issue(wa, 0); };
    // 16-byte chunk (8 elements) of the wave's slice that fragment s holds for k-group g: 4 s + g; MX6 (fragment 4 S + j of load step S): 16 S + 4 g + j
    auto x_chunk = [&](int s, int g) { return MX6 ? (s >> 2) * 16 + g * 4 + (s & 3) : s * 4 + g; };

    // ---- activations: this wave's K slice as MFMA B fragments (batch row = lane & 15, k = 8 (lane >> 4) .. + 8 of a 32-step) ----
    // Fetched ROW-shaped -- one contiguous 1 KiB request per batch row, lane l the 8 elements [8 l, 8 l + 8) of the slice -- and
    // turned into fragments through a wave-private LDS window (no barrier: only this wave writes and reads it).  Fetched
    // fragment-shaped (every instruction 16 bytes from each of B rows x 4 k-groups) the 32 requests of a wave touched 4x the cache
    // lines and held the CU's address path for ~3 us: qkv 28.8 us against 22.4 for decode_mfma.hip at B = 8.
    bf16x8_t xf[KM_STEPS];
    const int ksl = K / KM_WAVES / 32;   // 32-element fragments in the wave's slice
    if constexpr (XATTN) {
        // o-proj: the block merges the attention split partials once (every thread one 8-element chunk per row), through LDS
        issue_first();
        const int nch = K >> 3;
        for (int c = tid; c < nch; c += KM_NT) {
            unsigned char* dst = xlds + (size_t)c * 16;
            if constexpr (EX) {   // the merged chunk in fp32, split into its two terms: rows b and b + 8
                for (int b = 0; b < B; ++b) {
                    float m8[8];
                    (void)attn_merge_chunk_loop(p.attn_part + (size_t)(b * p.Hq + (c >> 4)) * p.nsplit * PSTRIDE, (c & 15) * 8, p.nsplit, m8);
                    u32x4_t hi, lo;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const hl2_t t = split_hl2(m8[2 * e], m8[2 * e + 1]);
                        hi[e] = t.hi;
                        lo[e] = t.lo;
                    }
                    *(u32x4_t*)(dst + (size_t)b * K * 2) = hi;
                    *(u32x4_t*)(dst + (size_t)(b + 8) * K * 2) = lo;
                }
                continue;
            }
            switch (p.nsplit) {
                case 1: stage_attn_rows<1>(p.attn_part, dst, K * 2, B, p.Hq, c); break;
                case 2: stage_attn_rows<2>(p.attn_part, dst, K * 2, B, p.Hq, c); break;
                case 4: stage_attn_rows<4>(p.attn_part, dst, K * 2, B, p.Hq, c); break;
                case 8: stage_attn_rows<8>(p.attn_part, dst, K * 2, B, p.Hq, c); break;
                default:
                    for (int b = 0; b < B; ++b)
                        *(u32x4_t*)(dst + (size_t)b * K * 2) =
                            attn_merge_chunk_loop(p.attn_part + (size_t)(b * p.Hq + (c >> 4)) * p.nsplit * PSTRIDE, (c & 15) * 8, p.nsplit);
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KM_STEPS; ++s) {
            // (two spellings of one address: written through x_chunk for every format, the fp8 / MX4 forms compile to three scalar instructions in
            // another order than before -- they keep theirs)
            const int k0 = MX6 ? wave * ksl * 32 + x_chunk(s, g4) * 8 : (wave * ksl + s) * 32 + g4 * 8;
            const u32x4_t v = (s < ksl && col_live(c16)) ? *(const u32x4_t*)(xlds + ((size_t)c16 * K + k0) * 2) : (u32x4_t){0u, 0u, 0u, 0u};
            xf[s] = __builtin_bit_cast(bf16x8_t, v);
        }
    } else {
        unsigned char* xw = km_smem + (size_t)wave * wreg;                           // this wave's window: [NB rows][XPITCH]
        const bool mine = lane < ksl * 4;                                            // 16-byte chunks of the slice
        const int ch = min(lane, ksl * 4 - 1);
        if constexpr (EX) {
            // fp32 rows (NORM: the residual stream h32; else the fp32 operand p.x): lane l holds elements [8 l, 8 l + 8) of the wave's slice of every
            // batch row; statistics and x g in fp32, then the two terms into window rows b (hi) and b + 8 (lo)
            const float* src = NORM ? (const float*)p.h32 : (const float*)p.x;
            const size_t ld = NORM ? (size_t)p.ldh : (size_t)p.ldx;
            f32x4_t xq[8][2];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const float* rp = src + (size_t)min(b, B - 1) * ld + (size_t)wave * ksl * 32 + (size_t)ch * 8;
                xq[b][0] = *(const f32x4_t*)rp;
                xq[b][1] = *(const f32x4_t*)(rp + 4);
            }
            u32x4_t nwv = {0u, 0u, 0u, 0u};
            if constexpr (NORM) nwv = *((const u32x4_t*)((const bf16_t*)p.norm_w + wave * ksl * 32) + ch);
            issue_first();
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                float ss = 0.f;
                u32x4_t hi, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float a = (mine && b < B) ? xq[b][e >> 1][2 * (e & 1)] : 0.f, c = (mine && b < B) ? xq[b][e >> 1][2 * (e & 1) + 1] : 0.f;
                    if constexpr (NORM) {
                        ss += a * a + c * c;
                        a *= bf_lo(nwv[e]);
                        c *= bf_hi(nwv[e]);
                    }
                    const hl2_t t = split_hl2(a, c);
                    hi[e] = t.hi;
                    lo[e] = t.lo;
                }
                if constexpr (NORM) {
                    const float t = wave_sum(ss);
                    if (lane == 0) sumsq[wave * 16 + b] = t;
                }
                *(u32x4_t*)(xw + (size_t)b * XPITCH + (size_t)lane * 16) = hi;
                *(u32x4_t*)(xw + (size_t)(b + 8) * XPITCH + (size_t)lane * 16) = lo;
            }
        } else {
        u32x4_t xr[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) xr[b] = *((const u32x4_t*)((const bf16_t*)p.x + (size_t)min(b, B - 1) * p.ldx + wave * ksl * 32) + ch);
        u32x4_t nwv = {0u, 0u, 0u, 0u};
        if constexpr (NORM) nwv = *((const u32x4_t*)((const bf16_t*)p.norm_w + wave * ksl * 32) + ch);
        issue_first();   // behind the activation requests: those are waited for by count while the first tile is in flight
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float ss = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t v = (mine && b < B) ? xr[b][e] : 0u;
                if constexpr (NORM) {
                    const float a = bf_lo(v), c = bf_hi(v);
                    ss += a * a + c * c;
                    v = pack_bf16x2(a * bf_lo(nwv[e]), c * bf_hi(nwv[e]));
                }
                xr[b][e] = v;
            }
            if constexpr (NORM) {
                const float t = wave_sum(ss);
                if (lane == 0) sumsq[wave * 16 + b] = t;
            }
            *(u32x4_t*)(xw + (size_t)b * XPITCH + (size_t)lane * 16) = xr[b];   // lanes past the slice write zeros (never read)
        }
        }
        // wave-private: the reads below only need this wave's own LDS writes to have landed (hipcc's lgkmcnt), no barrier
#pragma unroll
        for (int s = 0; s < KM_STEPS; ++s) {
            const u32x4_t v = (s < ksl && col_live(c16)) ? *(const u32x4_t*)(xw + (size_t)c16 * XPITCH + (size_t)x_chunk(s, g4) * 16) : (u32x4_t){0u, 0u, 0u, 0u};
            xf[s] = __builtin_bit_cast(bf16x8_t, v);
        }
    }
    if constexpr (MX) {
#pragma unroll
        for (int d = 1; d < QD; ++d) issue_mx(d, d);
    } else
    issue(wb, 1);   // the second tile once the prologue's temporaries are dead (all of them next to two tiles would not fit 256 VGPRs)

    // ---- main loop: two tiles per trip (register sets a / b); a set is consumed MFMA by MFMA and refilled with the tile two ahead ----
    auto run_tile = [&](u32x4_t (&w)[NSTEP], int tl) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            if constexpr (FP8) {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16x8(w[s][0], w[s][1]), xf[2 * s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16x8(w[s][2], w[s][3]), xf[2 * s + 1], acc, 0, 0, 0);
            } else {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w[s]), xf[s], acc, 0, 0, 0);
            }
            if constexpr (ROLL) issue_one(w, tl + 2, s);
        }
        if constexpr (!ROLL) {
            __builtin_amdgcn_sched_barrier(0);
            issue(w, tl + 2);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (tl < ntb) *(f32x4_t*)(part_of(wave) + ((size_t)tl * 64 + lane) * 4) = acc;
    };
    // block-scaled tiles: set d holds tile tl; per load step four MFMAs, and the set's step is refilled with the tile QD ahead as soon as they have issued.  Only
    // the widening differs -- MX4: one conversion per MFMA, byte j of the step's scale dword shifted into the exponent of its scale operand; MX6: ONE conversion
    // (the lane's block, byte g of the row's scale dword) for the four
    auto run_tile_mx = [&](int d, int tl) {
        if constexpr (MX) {
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                bf16x8_t a[4];
                if constexpr (MX6) mx6x32_to_bf16x8(q.w[d][s], q.h[d][s], e8m0_scale(q.s[d][s], g4), a);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (MX4) a[j] = mx4x8_to_bf16x8(q.w[d][s][j], e8m0_scale(q.s[d][s], j));
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], xf[4 * s + j], acc, 0, 0, 0);
                }
                issue_mx_one(d, tl + QD, s);
            }
            if (tl < ntb) *(f32x4_t*)(part_of(wave) + ((size_t)tl * 64 + lane) * 4) = acc;
        }
    };
    if constexpr (MX) {
        for (int tl = 0; tl < ntb; tl += QD) {
#pragma unroll
            for (int d = 0; d < QD; ++d) run_tile_mx(d, tl + d);
        }
    } else {
        for (int tl = 0; tl < ntb; tl += 2) {
            run_tile(wa, tl);
            run_tile(wb, tl + 1);
        }
    }
    __syncthreads();

    // ---- epilogue: thread (tl, l): rows 4 (l >> 4) + j of tile tl, batch column l & 15 ----
    float v[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f};   // u: the partner rows r + 8 (qkv, gate/up)
    if (e_on) {
#pragma unroll
        for (int w = 0; w < KM_WAVES; ++w) {
            const f32x4_t a = *(const f32x4_t*)(part_of(w) + ((size_t)e_tl * 64 + e_l) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += a[j];
            if (e_pairs) {
                const f32x4_t b2 = *(const f32x4_t*)(part_of(w) + ((size_t)e_tl * 64 + e_l + 32) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) u[j] += b2[j];
            }
        }
        if constexpr (EX) {   // the lo terms' products: batch column e_c + 8 of the same rows
            float vl[4] = {0.f, 0.f, 0.f, 0.f}, ul[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < KM_WAVES; ++w) {
                const f32x4_t a = *(const f32x4_t*)(part_of(w) + ((size_t)e_tl * 64 + e_l + 8) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) vl[j] += a[j];
                if (e_pairs) {
                    const f32x4_t b2 = *(const f32x4_t*)(part_of(w) + ((size_t)e_tl * 64 + e_l + 40) * 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) ul[j] += b2[j];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] += vl[j]; u[j] += ul[j]; }
        }
        float sc = 1.f;
        if constexpr (NORM) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < KM_WAVES; ++w) t += sumsq[w * 16 + e_c];
            sc = rsqrtf(t / (float)K + p.eps);
        }
        // (rstd and the row's weight scale are multiplied TOGETHER first here; decode_kmp.hip applies them one after the other -- two
        // roundings in another order, so the scaling is not part of the shared tile finish)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float sv = sc, su = sc;
            if constexpr (FP8) {
                sv *= p.wscale[e_tile * 16 + 4 * e_rq + j];
                if (e_pairs) su *= p.wscale[e_tile * 16 + 8 + 4 * e_rq + j];
            }
            v[j] *= sv;
            u[j] *= su;
        }
    }
    float best = -INFINITY;
    int besti = 0x7fffffff;
    if (e_on && MODE == GEMV_QKV) {
        if constexpr (EX) {
            // nothing is rounded to bf16: fp32 RoPE (every product rounded on its own, as torch does), fp32 q rows, 24-bit / fp32 cache rows
            const int hd = p.head_dim, half = hd >> 1, tph = hd / 16;
            const int hb = e_tile / tph, d0 = 8 * (e_tile - hb * tph) + 4 * e_rq;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = d0 + j;
                if (hb < p.Hq + p.Hkv) {
                    const float y0 = __fadd_rn(__fmul_rn(v[j], pre_a[j]), -__fmul_rn(u[j], pre_b[j]));
                    const float y1 = __fadd_rn(__fmul_rn(u[j], pre_a[j]), __fmul_rn(v[j], pre_b[j]));
                    if (hb < p.Hq) {
                        float* q = (float*)p.y + (size_t)e_c * p.ldy + hb * hd;
                        q[d] = y0;
                        q[d + half] = y1;
                    } else {
                        gemv_kv_store_x(p, false, pre_pg, pre_pos, hb - p.Hq, d, y0);
                        gemv_kv_store_x(p, false, pre_pg, pre_pos, hb - p.Hq, d + half, y1);
                    }
                } else {
                    gemv_kv_store_x(p, true, pre_pg, pre_pos, hb - p.Hq - p.Hkv, d, v[j]);
                    gemv_kv_store_x(p, true, pre_pg, pre_pos, hb - p.Hq - p.Hkv, d + half, u[j]);
                }
            }
        } else {
            const int hd = p.head_dim, half = hd >> 1, tph = hd / 16;
            const int hb = e_tile / tph, d0 = 8 * (e_tile - hb * tph) + 4 * e_rq;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = d0 + j;
                // linear outputs are bf16 activations in the reference; RoPE acts on those
                const float x0 = bf2f(f2bf(v[j])), x1 = bf2f(f2bf(u[j]));
                if (hb < p.Hq + p.Hkv) {
                    const bf16_t y0 = f2bf(x0 * pre_a[j] - x1 * pre_b[j]), y1 = f2bf(x1 * pre_a[j] + x0 * pre_b[j]);
                    if (hb < p.Hq) {
                        bf16_t* q = (bf16_t*)p.y + (size_t)e_c * p.ldy + hb * hd;
                        q[d] = y0;
                        q[d + half] = y1;
                    } else {
                        bf16_t* kc = gemv_kv_row(p, false, e_c, pre_pg, pre_pos, hb - p.Hq);
                        kc[d] = y0;
                        kc[d + half] = y1;
                    }
                } else {
                    bf16_t* vc = gemv_kv_row(p, true, e_c, pre_pg, pre_pos, hb - p.Hq - p.Hkv);
                    vc[d] = f2bf(x0);
                    vc[d + half] = f2bf(x1);
                }
            }
        }
    } else if (e_on) {
        tile4_finish<MODE, R32, EX>(p, e_c, e_tile, e_rq, v, u, pre_a, best, besti);
    }
    if (MODE == GEMV_LMHEAD) {
        // block best per batch column: the 32 slots (tile, row quarter) of a column through LDS; first index wins ties
        __syncthreads();                      // every thread has read its partial sums
        float* bv = part_of(0);               // [512] + [512]: 4 KiB of wave 0's region (>= its 8.1 KiB window)
        int* bi = (int*)(bv + KM_NT);         // [512]
        bv[tid] = best;
        bi[tid] = besti;
        __syncthreads();
        if (tid < B) {
            const auto slot = [&](int k) { return (k >> 2) * 64 + (k & 3) * 16 + tid; };
            lmhead_col_finish(p, B, tid, bv, bi, KM_WAVES * 4, slot, -INFINITY, 0x7fffffff);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The down projection at batch 3-16 (K = 11008: 43 k-steps per wave -- 172 registers of activation fragments, or 176 KB of LDS for
// eight rows, neither exists).  One 16-row tile per block; the wave's K slice runs in PHASES of FR fragments (NB = 8 rows: two phases
// of 22; NB = 16 rows, round 5: four of 12): the row slices of a phase go through the wave-private LDS window (row-shaped requests,
// no barrier), the fragments are read just in time, one ds_read_b128 per MFMA; the row slices of the next two phases wait in two
// register sets and replace the window's contents when the phase's MFMAs are done.  Weights: the first phase's steps in flight from
// the start (22 / 12 KiB per wave), every register refilled with the next phase's step as soon as its MFMA has issued.
// y = h + W x in place (+ the per-row scale with fp8 weights).
// ---------------------------------------------------------------------------------------------------------------------
// (block-scaled tiles: a load step is four fragments, so eight rows run two phases of 24 -- 97 KiB of windows against 89)
template <int NB, int WF = 0> struct KdShape {
    static constexpr int FR = NB == 8 ? (22 + wfmt_fps(WF) - 1) / wfmt_fps(WF) * wfmt_fps(WF) : 12;   // fragments (32 elements) per phase and wave: whole load steps
    static constexpr int NPH = NB == 8 ? 2 : 4;       // phases: K <= 8 waves x NPH x FR x 32 = 11264 / 12288
    static constexpr int XP = FR * 64 + 16;           // bytes per staged row slice
    static constexpr int CH = (FR * 4 + 63) / 64;     // 16-byte chunks per lane and row of a phase
};
// EX (exact numerics, batch 3-8; NB = 16): p.x holds the fp32 SwiGLU product; window rows b / b + 8 = the two bf16 terms of batch row b (see
// emmax_decode_km_kernel); the row registers hold the fp32 chunk as two quads (r[2 b], r[2 b + 1]).
template <int WF, bool R32, int NB, bool EX = false>
__global__ __launch_bounds__(KM_NT, 2) void emmax_decode_kmd_kernel(GemvParams p) {
    constexpr bool FP8 = WF == PW_FP8, MX4 = WF == PW_MX4, MX6 = WF == PW_MX6, MX = wfmt_is_mx(WF);
    static_assert(!EX || (NB == 16 && WF == PW_BF16 && R32), "exact numerics: eight batch rows x two terms, bf16 weights, fp32 residual stream");
    extern __shared__ __attribute__((aligned(16))) unsigned char km_smem[];
    using S = KdShape<NB, WF>;
    constexpr int FR = S::FR, NPH = S::NPH, XP = S::XP, CH = S::CH;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g4 = lane >> 4, c16 = lane & 15;
    const int B = p.batch, K = p.K;
    constexpr int FPS = wfmt_fps(WF), KS = WFMT[WF].ks;      // fragments / elements per load step
    constexpr int NST = FR / FPS;                            // load steps per phase
    const int KT = K / KS;
    const int kq = KT / KM_WAVES, kr = KT % KM_WAVES;
    const int k_lo = wave * kq + min(wave, kr), k_n = kq + (wave < kr ? 1 : 0);   // this wave's load steps (launcher: k_n <= NPH NST)
    float* part = (float*)km_smem;                                                 // [KM_WAVES][64][4]
    unsigned char* xw = km_smem + KM_WAVES * 1024 + (size_t)wave * NB * XP;        // this wave's window
    const int tile = blockIdx.x;

    // epilogue operands of thread (lane l of wave 0): rows 4 (l >> 4) + j, batch column l & 15
    const bool e_on = tid < 64 && c16 < B && (!EX || c16 < 8);
    float pre[4] = {0.f, 0.f, 0.f, 0.f};
    if (e_on) tile4_resid_prefetch<R32>(p, c16, tile * 16 + 4 * g4, pre);

    // ---- activation row slices of a phase: lane l holds chunks l (and l + 64) of the phase's slice, for every batch row ----
    auto phase_steps = [&](int ph) { return max(0, min(NST, k_n - ph * NST)); };
    auto load_rows = [&](int ph_in, u32x4_t (&r)[NB][CH]) {
        const int nch = phase_steps(ph_in) * (KS / 8);          // 16-byte chunks in the slice
        // a phase past the wave's slice (a short K: 4160 = 17 steps per wave leaves NB = 16's phases 2 and 3 empty) loads phase 0's first chunk
        // again: its address would lie past the row -- past the buffer for the last row -- and store_rows writes zeros for it anyway
        const int ph = nch > 0 ? ph_in : 0;
        if constexpr (EX) {
            static_assert(!EX || CH == 1, "one chunk per lane and row");
            const float* b32 = (const float*)p.x + (size_t)(k_lo + ph * NST) * KS + (size_t)min(lane, max(nch - 1, 0)) * 8;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const float* rp = b32 + (size_t)min(b, B - 1) * p.ldx;
                r[2 * b][0] = *(const u32x4_t*)rp;
                r[2 * b + 1][0] = *(const u32x4_t*)(rp + 4);
            }
            return;
        }
        const bf16_t* base = (const bf16_t*)p.x + (size_t)(k_lo + ph * NST) * KS;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int h = 0; h < CH; ++h) {
                const int c = min(lane + 64 * h, max(nch - 1, 0));
                r[b][h] = *((const u32x4_t*)(base + (size_t)min(b, B - 1) * p.ldx) + c);
            }
    };
    auto store_rows = [&](int ph, const u32x4_t (&r)[NB][CH]) {
        const int nch = phase_steps(ph) * (KS / 8);
        if constexpr (EX) {
            if (lane < FR * 4) {
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const bool live = lane < nch && b < B;
                    u32x4_t hi, lo;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const u32x4_t& q = r[2 * b + (e >> 1)][0];
                        const hl2_t t = split_hl2(live ? __uint_as_float(q[2 * (e & 1)]) : 0.f, live ? __uint_as_float(q[2 * (e & 1) + 1]) : 0.f);
                        hi[e] = t.hi;
                        lo[e] = t.lo;
                    }
                    *(u32x4_t*)(xw + (size_t)b * XP + (size_t)lane * 16) = hi;
                    *(u32x4_t*)(xw + (size_t)(b + 8) * XP + (size_t)lane * 16) = lo;
                }
            }
            return;
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int h = 0; h < CH; ++h) {
                const int c = lane + 64 * h;
                if (c < FR * 4) {   // chunks past the slice / rows past the batch: zeros
                    const bool live = c < nch && b < B;
                    *(u32x4_t*)(xw + (size_t)b * XP + (size_t)c * 16) = live ? r[b][h] : (u32x4_t){0u, 0u, 0u, 0u};
                }
            }
    };
    u32x4_t xa[NB][CH], xb[NB][CH];   // even / odd phases
    load_rows(0, xa);
    load_rows(1, xb);

    // ---- weights: phase 0 in flight now, later phases refilled register by register ----
    // (16 rows x K x 1 or 2 bytes keeps the parent's spelling: as one factor wfmt_bytes_per_k, or behind a helper, every bf16 kernel's scalar multiplies change operand order)
    const unsigned w_bytes = wfmt_is_mx(WF) ? (unsigned)((size_t)p.n_groups * wfmt_bytes_per_k(WF) * (size_t)K) : (unsigned)((size_t)p.n_groups * 16 * (size_t)K * (FP8 ? 1 : 2));
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (int)w_bytes, 0x00020000);
    const unsigned voff = (unsigned)lane * 16u;
    u32x4_t w[NST];
    // block-scaled tiles: the scale dword of each load step (emmax_decode_km_kernel: 64 B per tile in the tiles' order, 4 bytes per row) and, MX6, dwords 4-5 of
    // the lane's six; w[s] holds the lane's 16 bytes in every form (the struct's own w stays unused here)
    MxTiles<WF, 1, NST> q;
    auto issue_w = [&](int ph, int s) {   // load step s of phase ph (past the wave's slice: out of range = zeros, no traffic)
        const int ok = (ph * NST + s < k_n) ? -1 : 0;
        const unsigned so = ((unsigned)((tile * KT + k_lo + ph * NST + s) * WFMT[WF].tile_bytes) & (unsigned)ok) | (w_bytes & (unsigned)~ok);
        w[s] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, voff, so, 2));
        if constexpr (MX) {
            const unsigned s_bytes = w_bytes / (unsigned)(WFMT[WF].tile_bytes / WFMT_SCALE_BYTES);
            const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.w_codes, 0, (int)s_bytes, 0x00020000);
            if constexpr (MX6) q.h[0][s] = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(wrsrc, 1024u + (unsigned)lane * 8u, so, 2));
            q.s[0][s] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(srsrc, (unsigned)c16 * 4u, ((unsigned)((tile * KT + k_lo + ph * NST + s) * WFMT_SCALE_BYTES) & (unsigned)ok) | (s_bytes & (unsigned)~ok), 2);
        }
    };
#pragma unroll
    for (int s = 0; s < NST; ++s) issue_w(0, s);
    store_rows(0, xa);   // waits for the phase-0 rows only (counted: the phase-1 rows and the weights stay in flight)

    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    // batch column = lane & 15; columns past the batch are zero (their window rows hold zeros; NB = 8: columns 8-15 have no row at all)
    // (MX6: fragment 4 s + j of load step s is the lane's chunk 16 s + 4 g + j of the window row -- the roles of j and g exchanged, emmax_decode_km_kernel)
    const unsigned char* xcol = xw + (size_t)min(c16, NB - 1) * XP + (size_t)g4 * (MX6 ? 64 : 16);
    auto frag = [&](int f) {
        const u32x4_t v = *(const u32x4_t*)(xcol + (size_t)(MX6 ? (f >> 2) * 256 + (f & 3) * 16 : f * 64));
        return __builtin_bit_cast(bf16x8_t, (EX ? (c16 & 7) < B : c16 < B) ? v : (u32x4_t){0u, 0u, 0u, 0u});
    };
    auto mfma_step = [&](int s) {
        if constexpr (MX) {   // (the widening as in emmax_decode_km_kernel's run_tile_mx)
            bf16x8_t a[4];
            if constexpr (MX6) mx6x32_to_bf16x8(w[s], q.h[0][s], e8m0_scale(q.s[0][s], g4), a);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (MX4) a[j] = mx4x8_to_bf16x8(w[s][j], e8m0_scale(q.s[0][s], j));
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], frag(4 * s + j), acc, 0, 0, 0);
            }
        } else if constexpr (FP8) {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16x8(w[s][0], w[s][1]), frag(2 * s), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16x8(w[s][2], w[s][3]), frag(2 * s + 1), acc, 0, 0, 0);
        } else {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w[s]), frag(s), acc, 0, 0, 0);
        }
    };
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
        // the register set this phase's rows came from is free since they went into the window: request the rows two phases ahead
        if (ph + 2 < NPH) { if (ph & 1) load_rows(ph + 2, xb); else load_rows(ph + 2, xa); }
#pragma unroll
        for (int s = 0; s < NST; ++s) {
            mfma_step(s);
            if (ph + 1 < NPH) issue_w(ph + 1, s);   // the register's step of the next phase
        }
        // same wave, in order behind the fragment reads above: the next phase's rows replace this phase's
        if (ph + 1 < NPH) { if ((ph + 1) & 1) store_rows(ph + 1, xb); else store_rows(ph + 1, xa); }
    }

    *(f32x4_t*)(part + ((size_t)wave * 64 + lane) * 4) = acc;
    __syncthreads();
    if (e_on) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int wv = 0; wv < KM_WAVES; ++wv) {
            const f32x4_t a = *(const f32x4_t*)(part + ((size_t)wv * 64 + lane) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += a[j];
        }
        if constexpr (EX) {   // the lo terms' products: batch column c16 + 8
            float vl[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int wv = 0; wv < KM_WAVES; ++wv) {
                const f32x4_t a = *(const f32x4_t*)(part + ((size_t)wv * 64 + lane + 8) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) vl[j] += a[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += vl[j];
        }
        if constexpr (FP8) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= p.wscale[tile * 16 + 4 * g4 + j];
        }
        tile4_resid_finish<R32>(p, c16, tile * 16 + 4 * g4, pre, v);
    }
}

// (the launch functions below run behind decode_km_takes: every shape they meet has been accepted, the geometry is its answer)
template <int WF, int NB, bool EX = false>
int kmd_launch(const GemvParams& p, const ProjGeom& g, hipStream_t stream) {
    if constexpr (EX) {
        hipLaunchKernelGGL((emmax_decode_kmd_kernel<PW_BF16, true, 16, true>), dim3(g.grid), dim3(KM_NT), g.smem, stream, p);
    } else {
        if (p.h32) hipLaunchKernelGGL((emmax_decode_kmd_kernel<WF, true, NB>), dim3(g.grid), dim3(KM_NT), g.smem, stream, p);
        else hipLaunchKernelGGL((emmax_decode_kmd_kernel<WF, false, NB>), dim3(g.grid), dim3(KM_NT), g.smem, stream, p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

template <int MODE, bool NORM, bool XATTN, int WF, int NB, bool ROLL, bool EX = false>
int km_launch_nb(const GemvParams& p, const ProjGeom& g, hipStream_t stream) {
    if constexpr (EX) {   // exact numerics: fp32 rows in (h32 / p.x / the split partials), two terms per batch row, batch <= 8
        hipLaunchKernelGGL((emmax_decode_km_kernel<MODE, NORM, XATTN, PW_BF16, MODE == GEMV_RESID, 16, false, true>), dim3(g.grid), dim3(KM_NT), g.smem, stream, p);
        return hipGetLastError() == hipSuccess ? 0 : -4;
    }
    if constexpr (MODE == GEMV_RESID) {   // (NORM modes read the bf16 mirror: h32 is ignored there)
        if (p.h32) {
            hipLaunchKernelGGL((emmax_decode_km_kernel<MODE, NORM, XATTN, WF, true, NB, ROLL>), dim3(g.grid), dim3(KM_NT), g.smem, stream, p);
            return hipGetLastError() == hipSuccess ? 0 : -4;
        }
    }
    hipLaunchKernelGGL((emmax_decode_km_kernel<MODE, NORM, XATTN, WF, false, NB, ROLL>), dim3(g.grid), dim3(KM_NT), g.smem, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
template <int MODE, bool NORM, bool XATTN, int WF>
int km_launch_t(const GemvParams& p, const ProjGeom& g, hipStream_t stream) {
    if constexpr (wfmt_is_mx(WF) && XATTN) {   // split partials of 9-16 rows x K do not fit the LDS stage: those batches exist in the one-split form only
        return km_launch_nb<MODE, NORM, XATTN, WF, 8, false>(p, g, stream);
    } else {
        if constexpr (!wfmt_is_mx(WF)) {   // (the MX4 / MX6 forms always refill step by step: one instantiation per batch width)
            if (g.roll)
                return g.nb == 8 ? km_launch_nb<MODE, NORM, XATTN, WF, 8, true>(p, g, stream) : km_launch_nb<MODE, NORM, XATTN, WF, 16, true>(p, g, stream);
        }
        return g.nb == 8 ? km_launch_nb<MODE, NORM, XATTN, WF, 8, false>(p, g, stream) : km_launch_nb<MODE, NORM, XATTN, WF, 16, false>(p, g, stream);
    }
}

// exact numerics (GemvParams::exact), batch 3-8: the EX forms
int km_launch_mode_x(int mode, const GemvParams& p, const ProjGeom& g, hipStream_t stream) {
    switch (mode) {
        case GEMV_QKV: return km_launch_nb<GEMV_QKV, true, false, PW_BF16, 16, false, true>(p, g, stream);
        case GEMV_RESID:
            return p.attn_part ? km_launch_nb<GEMV_RESID, false, true, PW_BF16, 16, false, true>(p, g, stream)
                               : km_launch_nb<GEMV_RESID, false, false, PW_BF16, 16, false, true>(p, g, stream);
        case GEMV_GATEUP: return km_launch_nb<GEMV_GATEUP, true, false, PW_BF16, 16, false, true>(p, g, stream);
        case GEMV_LMHEAD: return km_launch_nb<GEMV_LMHEAD, true, false, PW_BF16, 16, false, true>(p, g, stream);
        default: return -2;
    }
}

template <int WF>
int km_launch_mode(int mode, const GemvParams& p, const ProjGeom& g, hipStream_t stream) {
    switch (mode) {
        case GEMV_QKV: return km_launch_t<GEMV_QKV, true, false, WF>(p, g, stream);
        case GEMV_RESID:
            if constexpr (WF == PW_BF16) {   // (the bf16 o-proj with the split merge stays on decode_mfma.hip: decode_km_takes)
                return km_launch_t<GEMV_RESID, false, false, WF>(p, g, stream);
            } else {
                return p.attn_part ? km_launch_t<GEMV_RESID, false, true, WF>(p, g, stream) : km_launch_t<GEMV_RESID, false, false, WF>(p, g, stream);
            }
        case GEMV_GATEUP: return km_launch_t<GEMV_GATEUP, true, false, WF>(p, g, stream);
        case GEMV_LMHEAD: return km_launch_t<GEMV_LMHEAD, true, false, WF>(p, g, stream);
        case GEMV_PLAIN: return km_launch_t<GEMV_PLAIN, false, false, WF>(p, g, stream);
        default: return -2;
    }
}

// the phased down kernel's shape constants by (staged rows, weight format)
struct KdDims { int fr, nph, xp; };
template <int NB, int WF> constexpr KdDims kd_dims() { return {KdShape<NB, WF>::FR, KdShape<NB, WF>::NPH, KdShape<NB, WF>::XP}; }
// the one step from a runtime weight format to the kernels' template argument: f(std::integral_constant<int, PW_*>)
template <class F> int with_wfmt(int wfmt, F&& f) {
    switch (wfmt) {
        case PW_BF16: return f(std::integral_constant<int, PW_BF16>{});
        case PW_FP8: return f(std::integral_constant<int, PW_FP8>{});
        case PW_MX4: return f(std::integral_constant<int, PW_MX4>{});
        case PW_MX6: return f(std::integral_constant<int, PW_MX6>{});
        default: return -2;
    }
}
KdDims kd_dims_of(int nb, int wfmt) {
    KdDims d = {};
    with_wfmt(wfmt, [&](auto wf) { d = nb == 8 ? kd_dims<8, decltype(wf)::value>() : kd_dims<16, decltype(wf)::value>(); return 0; });
    return d;
}

// the phased down form (y = h + W x, one 16-row tile per block): K in whole load steps, at least one per wave, a wave's share within
// NPH phases of FR fragments
bool kmd_takes(const ProjShape& s, int B, int nb, ProjGeom* g) {
    const int fps = wfmt_fps(s.wfmt), ks = WFMT[s.wfmt].ks;
    const KdDims d = kd_dims_of(nb, s.wfmt);
    if (s.K % ks || s.n_rows % 16 || s.attn_part) return false;
    if (cdiv(s.K / ks, KM_WAVES) > d.nph * (d.fr / fps) || s.K / ks < KM_WAVES) return false;
    if (s.exact && (!s.h32 || B > 8)) return false;
    g->phased = 1; g->nb = nb;
    g->n_groups = g->grid = s.n_rows / 16;
    g->smem = (size_t)KM_WAVES * 1024 + (size_t)KM_WAVES * nb * d.xp;
    return true;
}

// the K-split form: K in whole load steps for each of the eight waves and at most sixteen fragments per wave (K <= 4096), one block
// per CU with at most KM_MAX_TILES tiles each, one LDS region per wave (the window [NB][XPITCH] overlaid by the partial tiles) + sumsq
// (+ with split partials in: the merged rows)
bool kms_takes(const ProjShape& s, int B, int nb, ProjGeom* g) {
    const int ks = WFMT[s.wfmt].ks;
    if (s.K % (KM_WAVES * ks) || s.K > KM_WAVES * KM_STEPS * 32 || s.n_rows % 16) return false;
    if (s.mode == GEMV_QKV && (s.head_dim % 16 || s.head_dim < 16)) return false;
    g->nb = nb;
    g->n_groups = s.n_rows / 16;   // tiles
    g->grid = min(256, g->n_groups);
    if (s.mode == GEMV_LMHEAD) g->grid = min(g->grid, s.max_parts);
    if (g->grid < 1) return false;
    g->kc = cdiv(g->n_groups, g->grid);
    if (g->kc > KM_MAX_TILES) return false;
    if (g->kc & 1) g->kc += 1;   // the loop runs tiles in pairs
    const size_t wreg = s.attn_part ? (size_t)g->kc * 1024 : std::max((size_t)nb * (KM_STEPS * 64 + 16), (size_t)g->kc * 1024);
    g->smem = (size_t)KM_WAVES * wreg + KM_WAVES * 16 * 4 + (s.attn_part ? (size_t)(s.exact ? 16 : B) * s.K * 2 : 0);
    if (g->smem > 150 * 1024) return false;
    if (s.exact && (B > 8 || !s.h32)) return false;
    return true;
}

}  // namespace

// What this file takes (the km copy of the matrix: launch_repack_km; fp8: decode_mfma.hip's e4m3 tiles of the permuted rows; MXFP4 / MXFP6 tiles).
// 17-64 rows: decode_kmp.hip's answer (bf16 / fp8; MXFP4 under ProjShape::mx4_wide; MXFP6: none).  Exact numerics: 1-8 rows (two terms per batch row in the sixteen MFMA columns), bf16.
bool decode_km_takes(const ProjShape& s, int B, ProjGeom* out) {
    ProjGeom g = {};
    bool ok = false;
    const bool kfits = s.K % (KM_WAVES * 32) == 0 && s.K <= KM_WAVES * KM_STEPS * 32;
    if (B < 1 || B > EMMAX_MAX_DECODE_BATCH || s.mode < GEMV_QKV || s.mode > GEMV_PLAIN) return false;
    if (B > 16 && s.wfmt == PW_MX6) return false;   // MXFP6 tiles: 1-16 rows, this file's kernels only (decode_kmp.hip has no MX6 form)
    if (B > 16) return decode_kmp_takes(s, B, out);   // two batch tiles: decode_kmp.hip (MXFP4 tiles: only when the shape says wide, else this file's kernels only)
    if (s.attn_part && (s.mode != GEMV_RESID || s.K != s.Hq * 128)) return false;
    if (s.exact) {
        if (B > 8 || s.wfmt != PW_BF16 || s.mode == GEMV_PLAIN) return false;
        // RESID launches without split partials (fp32 rows in p.x): the o-proj behind a one-split attention launch on the K-split kernel when its K fits,
        // the down projection (and any other K) on the phased kernel
        ok = (s.mode == GEMV_RESID && !s.attn_part && !kfits) ? kmd_takes(s, B, 16, &g) : kms_takes(s, B, 16, &g);
    } else if (s.mode == GEMV_RESID && !s.attn_part && s.K > KM_WAVES * KM_STEPS * 32) {   // the down projection: the phased form (natural row order copy)
        // tuning switch km_down = 0: decode_mfma.hip, the A/B partner (no other kernel reads MXFP4 tiles: no switch there)
        ok = (wfmt_is_mx(s.wfmt) || emmax_tune().km_down) && kmd_takes(s, B, B <= 8 ? 8 : 16, &g);
    } else {
        // the bf16 o-proj with the split merge stays on decode_mfma.hip (12.5 against 15.4 us at B = 8: the merge of 8 rows
        // queues behind this kernel's 16 KiB weight heads); with fp8 weights this kernel is the faster one (10.3 against 10.8).
        // MXFP4 / MXFP6: split partials of 9-16 rows x K do not fit the LDS stage, those batches exist in the one-split form only
        if (s.attn_part && (s.wfmt == PW_BF16 || (wfmt_is_mx(s.wfmt) && B > 8))) return false;
        g.roll = !wfmt_is_mx(s.wfmt) && emmax_tune().km_roll;   // (the MX4 / MX6 forms always refill step by step)
        ok = kms_takes(s, B, B <= 8 ? 8 : 16, &g);
    }
    if (ok && out) *out = g;
    return ok;
}

// raise the dynamic-LDS limit of every instantiation (call once, outside graph capture)
int decode_km_init() {
    static int done = -1;
    if (done == 0) return 0;
    const int lim = 150 * 1024;
    hipError_t e = hipSuccess;
#define KM_SET4(M, N_, X, F, R, NB_, RL) \
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)emmax_decode_km_kernel<M, N_, X, F, R, NB_, RL>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)
#define KM_SET3(M, N_, X, F, R, NB_) KM_SET4(M, N_, X, F, R, NB_, false); KM_SET4(M, N_, X, F, R, NB_, true)
#define KM_SET2(M, N_, X, F, R) KM_SET3(M, N_, X, F, R, 8); KM_SET3(M, N_, X, F, R, 16)
#define KM_SET1(M, N_, X, F) KM_SET2(M, N_, X, F, false); if (M == GEMV_RESID) KM_SET2(M, N_, X, F, true)
#define KM_SET(M, N_, X) KM_SET1(M, N_, X, PW_BF16); KM_SET1(M, N_, X, PW_FP8)
    KM_SET(GEMV_QKV, true, false); KM_SET1(GEMV_RESID, false, true, PW_FP8); KM_SET(GEMV_RESID, false, false); KM_SET(GEMV_GATEUP, true, false);
    KM_SET(GEMV_LMHEAD, true, false); KM_SET(GEMV_PLAIN, false, false);
    // the forms of a block-scaled format (no rolling variant; the split merge: 1-8 rows)
#define KM_SETQ(F, M, N_, X, R) KM_SET4(M, N_, X, F, R, 8, false); KM_SET4(M, N_, X, F, R, 16, false)
#define KM_SETMX(F) \
    KM_SETQ(F, GEMV_QKV, true, false, false); KM_SETQ(F, GEMV_GATEUP, true, false, false); KM_SETQ(F, GEMV_LMHEAD, true, false, false); KM_SETQ(F, GEMV_PLAIN, false, false, false); \
    KM_SETQ(F, GEMV_RESID, false, false, false); KM_SETQ(F, GEMV_RESID, false, false, true);                                                                                     \
    KM_SET4(GEMV_RESID, false, true, F, false, 8, false); KM_SET4(GEMV_RESID, false, true, F, true, 8, false)
    KM_SETMX(PW_MX4); KM_SETMX(PW_MX6);
#undef KM_SETMX
#undef KM_SETQ
#undef KM_SET
#undef KM_SET1
#undef KM_SET2
#undef KM_SET3
#undef KM_SET4
#define KD_SET(F, R, NB_) \
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)emmax_decode_kmd_kernel<F, R, NB_>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)
    // (bf16 and fp8 stay interleaved: the kernels are emitted in the order of these lines and the assembly's block labels carry their number)
    KD_SET(PW_BF16, false, 8); KD_SET(PW_FP8, false, 8); KD_SET(PW_BF16, true, 8); KD_SET(PW_FP8, true, 8);
    KD_SET(PW_BF16, false, 16); KD_SET(PW_FP8, false, 16); KD_SET(PW_BF16, true, 16); KD_SET(PW_FP8, true, 16);
#define KD_SETF(F) KD_SET(F, false, 8); KD_SET(F, true, 8); KD_SET(F, false, 16); KD_SET(F, true, 16)
    KD_SETF(PW_MX4); KD_SETF(PW_MX6);
#undef KD_SETF
#undef KD_SET
#define KX_SET(M, N_, X) \
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)emmax_decode_km_kernel<M, N_, X, PW_BF16, M == GEMV_RESID, 16, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim)
    KX_SET(GEMV_QKV, true, false); KX_SET(GEMV_RESID, false, true); KX_SET(GEMV_RESID, false, false); KX_SET(GEMV_GATEUP, true, false); KX_SET(GEMV_LMHEAD, true, false);
#undef KX_SET
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)emmax_decode_kmd_kernel<PW_BF16, true, 16, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim);
    done = (e == hipSuccess) ? 0 : -4;
    return done;
}

// tuning switch `km` = 0 keeps every batch >= 3 projection on decode_mfma.hip (the A/B partner)
bool decode_km_enabled() { return emmax_tune().km != 0; }

// perm: 0 natural row order, 1 qkv (head_dim given), 2 gate/up (source in decode.hip's 16-row interleaved order)
int launch_repack_km(const void* src, int ld, void* dst, int N, int K, int perm, int head_dim, hipStream_t stream) {
    if (N % 16 || K % 32 || ld % 8) return -1;
    if (perm == 1 && (head_dim % 16 || N % head_dim)) return -1;
    if (perm == 2 && N % 32) return -1;
    hipLaunchKernelGGL(emmax_repack_km_kernel, dim3(2048), dim3(256), 0, stream, (const bf16_t*)src, ld, (u32x4_t*)dst, N, K, perm, head_dim);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// (every block-scaled tile covers 16 rows x 128 k: one set of shape rules)
static bool mx_shape_ok(int wfmt, int ld, int N, int K, int perm, int head_dim) {
    if (wfmt < 0 || wfmt >= PW_COUNT || !wfmt_is_mx(wfmt)) return false;
    if (N < 16 || N % 16 || K < WFMT[wfmt].ks || K % WFMT[wfmt].ks || ld % 8 || ld < K) return false;
    if (perm == 1 && (head_dim < 16 || head_dim % 16 || N % head_dim)) return false;
    if (perm == 2 && N % 32) return false;
    return perm >= 0 && perm <= 2;
}
int launch_quant_mx(int wfmt, const void* src, int ld, void* tiles, void* codes, int N, int K, int perm, int head_dim, hipStream_t stream) {
    if (!mx_shape_ok(wfmt, ld, N, K, perm, head_dim)) return -1;
    hipLaunchKernelGGL(wfmt == PW_MX6 ? emmax_quant_mx6_kernel : emmax_quant_mx4_kernel, dim3(2048), dim3(256), 0, stream, (const bf16_t*)src, ld, (uint32_t*)tiles,
                       (uint32_t*)codes, N, K, perm, head_dim);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_dequant_mx(int wfmt, const void* tiles, const void* codes, void* dst, int ld, int N, int K, int perm, int head_dim, hipStream_t stream) {
    if (!mx_shape_ok(wfmt, ld, N, K, perm, head_dim)) return -1;
    hipLaunchKernelGGL(wfmt == PW_MX6 ? emmax_dequant_mx6_kernel : emmax_dequant_mx4_kernel, dim3(2048), dim3(256), 0, stream, (const uint32_t*)tiles,
                       (const uint32_t*)codes, (bf16_t*)dst, ld, N, K, perm, head_dim);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// p.W: the km copy of the matrix (launch_repack_km; fp8: decode_mfma.hip's e4m3 tiles of the permuted rows + p.wscale in the same
// row order).  -2: decode_km_takes says no (K % 256, K > 4096, more than 8 tiles per block ...) -- the caller uses decode_mfma.hip.
int launch_decode_km(int mode, const GemvParams& p_in, int B, hipStream_t stream, int* grid_out, const ProjGeom* geom) {
    ProjGeom g;
    if (geom) g = *geom;
    else if (!decode_km_takes(proj_shape(mode, p_in), B, &g)) return -2;
    if (B > 16) return launch_decode_kmp(mode, p_in, B, stream, grid_out, &g);   // two batch tiles: decode_kmp.hip
    if (decode_km_init() != 0) return -4;
    GemvParams p = p_in;
    p.batch = B; p.n_groups = g.n_groups; p.kc = g.kc;
    if (grid_out) *grid_out = g.grid;
    if (p.exact) return g.phased ? kmd_launch<PW_BF16, 16, true>(p, g, stream) : km_launch_mode_x(mode, p, g, stream);
    return with_wfmt(p.wfmt, [&](auto wf) {
        constexpr int WF = decltype(wf)::value;
        if (g.phased) return g.nb == 8 ? kmd_launch<WF, 8>(p, g, stream) : kmd_launch<WF, 16>(p, g, stream);
        return km_launch_mode<WF>(mode, p, g, stream);
    });
}
