// score.hip -- teacher-forced scoring of packed rows against the lm-head without ever storing a logit.
// Replaces `logits = lm_head(norm(h))` followed by log_softmax / gather / argmax in torch (HF LlamaForCausalLM.forward with labels,
// prismatic/training/strategies/base_strategy.py:392-416): per row only the log-sum-exp, the logit of one target id and the argmax leave the chip.
//
//   logits[r, c] = sum_k X[r, k] . W[c, k]     X bf16 [rows, ldx] (the finally-normed rows), W bf16 [Np, ldw] (the lm-head), fp32 accumulate,
//   columns c >= V never influence an output (they are masked by SELECTION, so NaN / inf there are harmless).
//
// Launch 1, emmax_score_kernel: grid = row tiles x vocabulary slices.  A block (4 waves as 2 x 2, wave tile 64 x 64, the 128 x 128 x 64 two-stage
// structure of gemm.hip's small geometry: both operands HBM/L2 -> LDS by 16-byte global_load_lds, the bank swizzle on the SOURCE address) owns 128 rows
// and a contiguous run of 128-column tiles.  After a tile's K loop every lane folds its 16 accumulator values per row tile into its OWN running
// (max m, l = sum exp(x - m), index of the max): no cross-lane traffic per tile.  When the slice ends the 8 lane groups that share a row (4 lanes of a
// wave x the 2 waves side by side) meet once through LDS, and one (m, l, idx) per row and slice goes to the scratch planes [slices][rows].
// The target logit is written by the one lane that holds the target column, with the value that entered the statistics; columns are only COMPARED
// with the target, nothing is indexed by it.
// Launch 2, emmax_score_merge_kernel: per row M = max m_s, L = sum l_s exp(m_s - M), lse = M + log L, idx of the lowest slice attaining M.
// The launch boundary IS the reduce: no counters, flags or waits between blocks, nothing here can spin.
// Argmax: the lowest id wins a tie (torch semantics, decode.hip's rule) -- inside a lane (strict > in ascending column order), across tiles
// (strict >, later tiles hold higher ids), across lanes / waves (equal maxima: the lower id) and across slices (strict > in ascending slice order).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SBK = 64, SBM = 128, SBN = 128, S_MT = 4, S_NT = 4;
constexpr int S_OP = SBM * SBK * 2;        // operand tile bytes (16 KiB)
constexpr int S_SMEM = 4 * S_OP;           // [X0 | W0 | X1 | W1]: one array, 64 KiB, two blocks per CU
constexpr int S_DMA_BIAS = 4096;           // keeps the per-lane offset non-negative behind the slab immediates (gemm.hip)

// four 1 KiB slabs (8 rows of 128 bytes) per request group; M0 written and read inside ONE asm statement (gemm.hip: glds16_group4)
__device__ __forceinline__ void score_glds16x4(unsigned int lds_base, unsigned int v0, unsigned int v1, unsigned int v2, unsigned int v3, unsigned long long sbase) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %5 offset:0\n\t"
                 "global_load_lds_dwordx4 %2, %5 offset:1024\n\t"
                 "global_load_lds_dwordx4 %3, %5 offset:2048\n\t"
                 "global_load_lds_dwordx4 %4, %5 offset:3072"
                 ::"s"(__builtin_amdgcn_readfirstlane(lds_base)), "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(sbase)
                 : "m0", "memory");
}

__global__ __launch_bounds__(256, 2) void emmax_score_kernel(ScoreParams p) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int g = lane >> 4, li = lane & 15;

    // block b lives on XCD b & 7: the row tiles of one slice are neighbours INSIDE an XCD, so the slice's W tiles are fetched into one L2
    const int nblk = p.row_tiles * p.slices, per_xcd = gridDim.x >> 3;
    const int unit = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (unit >= nblk) return;
    const int slice = unit / p.row_tiles, rt = unit - slice * p.row_tiles;
    const int m0 = rt * SBM;
    const int t0 = slice * p.tps, t1 = min(t0 + p.tps, p.col_tiles);
    const int nk = p.K / SBK;

    // ---- DMA sources: wave w fills slabs 4 w .. 4 w + 3 (8 rows each) of both operand tiles; rows past the edge re-read the last row ----
    unsigned int offA_l[4], offB_l[4];
    const unsigned int lds0 = __builtin_amdgcn_readfirstlane((unsigned int)(uintptr_t)(__attribute__((address_space(3))) void*)smem);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (wave * 4 + j) * 8 + (lane >> 3);
        const int gm = min(m0 + row, p.rows - 1) - m0;
        const unsigned int chunk = ((lane & 7) ^ ((row >> 1) & 7)) * 16 + (S_DMA_BIAS - j * 1024);
        offA_l[j] = (unsigned int)gm * (unsigned int)(p.ldx * 2) + chunk;
        offB_l[j] = (unsigned int)row * (unsigned int)(p.ldw * 2) + chunk;   // (W has Np >= 128 col_tiles rows: never past the edge)
    }
    const unsigned long long baseA = (unsigned long long)(uintptr_t)((const bf16_t*)p.X + (size_t)m0 * p.ldx) - S_DMA_BIAS;
    unsigned long long baseB = 0;
    auto issue = [&](int kt, int st) {   // K step kt of the current tile into stage st
        const unsigned long long ko = (unsigned long long)kt * (SBK * 2);
        score_glds16x4(lds0 + st * (2 * S_OP) + wave * 4096, offA_l[0], offA_l[1], offA_l[2], offA_l[3], baseA + ko);
        score_glds16x4(lds0 + st * (2 * S_OP) + S_OP + wave * 4096, offB_l[0], offB_l[1], offB_l[2], offB_l[3], baseB + ko);
    };
    auto set_tile = [&](int t) { baseB = (unsigned long long)(uintptr_t)((const bf16_t*)p.W + (size_t)t * SBN * p.ldw) - S_DMA_BIAS; };

    // ---- fragment reads: row base + swizzled chunk ((row >> 1) & 7 == (li >> 1) & 7 for every 16-row tile) ----
    const int swz = (li >> 1) & 7;
    const int c0 = (g ^ swz) << 4;
    const int offA = (wm * 64 + li) * 128, offB = S_OP + (wn * 64 + li) * 128;
    auto ldA = [&](const unsigned char* st, int s_) { return *(const bf16x8_t*)(st + offA + (s_ % S_MT) * 2048 + ((s_ / S_MT) ? (c0 ^ 64) : c0)); };
    auto ldB = [&](const unsigned char* st, int kk, int j) { return *(const bf16x8_t*)(st + offB + j * 2048 + (kk ? (c0 ^ 64) : c0)); };

    // ---- a lane's rows (row tile i: row m0 + wm 64 + 16 i + li) and their targets; -1 = nothing to write from this launch ----
    int tgt[S_MT];
    float rm[S_MT], rl[S_MT];
    int ri[S_MT];
#pragma unroll
    for (int i = 0; i < S_MT; ++i) {
        const int row = m0 + wm * 64 + i * 16 + li;
        const int t = row < p.rows ? p.targets[row] : -1;
        tgt[i] = (t >= 0 && t < p.V) ? t : -1;
        rm[i] = -INFINITY; rl[i] = 0.f; ri[i] = 0x7fffffff;
    }

    set_tile(t0);
    issue(0, 0);
    for (int t = t0; t < t1; ++t) {
        f32x4_t acc[S_MT][S_NT];
#pragma unroll
        for (int i = 0; i < S_MT; ++i)
#pragma unroll
            for (int j = 0; j < S_NT; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): K step 0 has landed (the builtin form: gemm.hip)
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            int offs = (kt & 1) * (2 * S_OP);
            asm volatile("" : "+s"(offs));
            const unsigned char* st = smem + offs;
            if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
            bf16x8_t fb[2][S_NT], fa[4];
#pragma unroll
            for (int j = 0; j < S_NT; ++j) fb[0][j] = ldB(st, 0, j);
            fa[0] = ldA(st, 0);
            fa[1] = ldA(st, 1);
            __builtin_amdgcn_sched_group_barrier(0x100, S_NT + 2, 0);
#pragma unroll
            for (int s_ = 0; s_ < 2 * S_MT; ++s_) {
                const int kk = s_ / S_MT, i = s_ % S_MT;
                if (s_ + 2 < 2 * S_MT) fa[(s_ + 2) & 3] = ldA(st, s_ + 2);
                if (s_ < S_NT) fb[1][s_] = ldB(st, 1, s_);
#pragma unroll
                for (int j = 0; j < S_NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kk][j], fa[s_ & 3], acc[i][j], 0, 0, 0);
                if (s_ < S_NT && s_ + 2 < 2 * S_MT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                else if (s_ < S_NT || s_ + 2 < 2 * S_MT) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, S_NT, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next stage has landed ...
            __syncthreads();                                    // ... and everybody is done reading this one
        }
        // the next tile's first K step goes out ahead of the fold (every stage is free behind the barrier above)
        if (t + 1 < t1) {
            set_tile(t + 1);
            issue(0, 0);
        }
        // ---- fold.  Swapped-operand layout: lane (g, li) holds row li of row tile i and columns 16 j + 4 g + r of the wave's 64 ----
        const int cb = t * SBN + wn * 64 + g * 4;
#pragma unroll
        for (int i = 0; i < S_MT; ++i) {
            float bm = -INFINITY;
            int bi = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < S_NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = cb + j * 16 + r;
                    const float v = acc[i][j][r];
                    const bool ok = col < p.V;
                    if (ok && col == tgt[i]) p.target_logit[m0 + wm * 64 + i * 16 + li] = v;   // (tgt >= 0 only for rows < p.rows)
                    if (ok && v > bm) { bm = v; bi = col; }                                     // ascending columns, strict >: the lowest id stays
                }
            const float nm = fmaxf(rm[i], bm);
            if (nm != -INFINITY) {   // (only masked columns so far: the statistics stay as they are, no (-inf) - (-inf))
                float l = rl[i] * expf(rm[i] - nm);   // first update: 0 x exp(-inf) = 0; unchanged maximum: x 1
#pragma unroll
                for (int j = 0; j < S_NT; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) l += (cb + j * 16 + r < p.V) ? expf(acc[i][j][r] - nm) : 0.f;
                if (bm > rm[i]) ri[i] = bi;           // strict >: an earlier tile's (lower) id keeps a tie
                rl[i] = l; rm[i] = nm;
            }
        }
    }

    // ---- the slice has ended (the last step's barrier: nobody reads a stage any more, no request is in flight).  The 8 lane groups of a
    // row -- (wn, g) -- meet once: [plane][row 0..127][wn 4 + g] ----
    float* sm_m = (float*)smem;
    float* sm_l = sm_m + SBM * 8;
    int* sm_i = (int*)(sm_l + SBM * 8);
#pragma unroll
    for (int i = 0; i < S_MT; ++i) {
        const int e = (wm * 64 + i * 16 + li) * 8 + wn * 4 + g;
        sm_m[e] = rm[i]; sm_l[e] = rl[i]; sm_i[e] = ri[i];
    }
    __syncthreads();
    if (tid < SBM && m0 + tid < p.rows) {
        float M = -INFINITY;
        int idx = 0x7fffffff;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float me = sm_m[tid * 8 + e];
            const int ie = sm_i[tid * 8 + e];
            if (me > M || (me == M && ie < idx)) { M = me; idx = ie; }   // equal maxima: the lower id
        }
        float L = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float me = sm_m[tid * 8 + e];
            if (me != -INFINITY) L += sm_l[tid * 8 + e] * expf(me - M);   // (a lane group that saw masked columns only: skipped, no (-inf) - (-inf))
        }
        const size_t o = (size_t)slice * p.rows + m0 + tid;
        p.part_m[o] = M; p.part_l[o] = L; p.part_i[o] = idx;
    }
}

__global__ __launch_bounds__(256) void emmax_score_merge_kernel(ScoreParams p) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= p.rows) return;
    float M = -INFINITY;
    int idx = 0;
    for (int s = 0; s < p.slices; ++s) {
        const float ms = p.part_m[(size_t)s * p.rows + row];
        if (ms > M) { M = ms; idx = p.part_i[(size_t)s * p.rows + row]; }   // ascending slices, strict >: the lowest slice attaining M
    }
    float L = 0.f;
    for (int s = 0; s < p.slices; ++s) {
        const float ms = p.part_m[(size_t)s * p.rows + row];
        if (ms != -INFINITY) L += p.part_l[(size_t)s * p.rows + row] * expf(ms - M);
    }
    p.lse[row] = M + logf(L);
    p.argmax[row] = idx;
    const int t = p.targets[row];
    if (t < 0 || t >= p.V) p.target_logit[row] = 0.f;   // -100 and anything else outside the vocabulary: nothing was looked up
}

}  // namespace

// row tiles x slices ~ twice the CU count, capped by the column tiles and by the scratch (three fp32-sized planes [slices][rows]); every slice
// holds at least one tile.  slices_forced 0: the planner's choice.
bool score_form(int rows, int V, int K, long long ws_bytes, int slices_forced, ScoreForm* f) {
    if (rows < 1 || V < 1 || K < SBK || K % SBK) return false;
    const int row_tiles = (rows + SBM - 1) / SBM, col_tiles = (V + SBN - 1) / SBN;
    const long long cap = ws_bytes / (12LL * rows);
    int want = slices_forced;
    if (want == 0) {
        want = 2 * 256 / row_tiles;
        if (want < 1) want = 1;
        if (want > col_tiles) want = col_tiles;
        if ((long long)want > cap) want = (int)cap;
    }
    if (want < 1 || want > col_tiles || (long long)want > cap) return false;
    f->row_tiles = row_tiles; f->col_tiles = col_tiles;
    f->tps = (col_tiles + want - 1) / want;
    f->slices = (col_tiles + f->tps - 1) / f->tps;
    return true;
}

int launch_score_rows(const ScoreParams& p0, const ScoreForm& f, hipStream_t stream) {
    ScoreParams p = p0;
    p.row_tiles = f.row_tiles; p.col_tiles = f.col_tiles; p.slices = f.slices; p.tps = f.tps;
    p.part_m = p0.ws; p.part_l = p0.ws + (size_t)f.slices * p.rows; p.part_i = (int32_t*)(p0.ws + 2 * (size_t)f.slices * p.rows);
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)emmax_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, S_SMEM) != hipSuccess) return -4;
        attr_done = true;
    }
    const int nblk = f.row_tiles * f.slices;
    hipLaunchKernelGGL(emmax_score_kernel, dim3((nblk + 7) / 8 * 8), dim3(256), S_SMEM, stream, p);
    hipLaunchKernelGGL(emmax_score_merge_kernel, dim3((p.rows + 255) / 256), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
