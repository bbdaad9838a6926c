// beam.hip -- beam search inside the decode step (include/emmax.h, ABI 9): the beam finish, the KV reorder on the page table, the fork
// after a prefill and the resolution of the finished hypotheses.
//
// A step with beams on ends in THREE launches behind the lm-head (a greedy / sampled / processing step ends in one):
//   1. emmax_beam_rows_kernel      one 1024-thread block per running row (the row in registers, as emmax_sample_kernel holds it): lse of the
//                                  raw row, acc = (l - lse) + score, the row's best 2K candidates in (acc descending, token ascending) order;
//   2. emmax_beam_merge_kernel     one wave per group: the K-way merge of the rows' lists into the group's top 2K, HF's state updates
//                                  (running beams, finished set, early-stop heuristic, done flag), the trace, the per-row decode state, and
//                                  the page-table gather new[j] = old[parent(j)] with the list of partial pages to copy;
//   3. emmax_beam_copy_kernel      the copies of that list: (blocks, layers x planes, rows), wide non-temporal loads / stores.
// The merge needs every row's list (a grid-wide dependency) and the copy needs the chip, not one wave, so neither pair can share a launch.
// Every reduction has a fixed order, there are no float atomics and no atomics at all outside LDS-free code paths: two launches on the
// same inputs agree bit for bit, eager or replayed.
//
// SAMPLE GROUPS (N sampled rows per prompt) fork the same way once, after the prefill, and never reorder: emmax_group_fork_kernel writes the
// page-table rows, the rows' decode state and the copy list that emmax_beam_copy_kernel consumes; emmax_group_bcast_kernel gives the group's
// one logit row (and prompt-history row) to its N rows.  Their steps are ordinary sampled steps: nothing here runs in them.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <stdint.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int BT = 1024;            // threads per row
constexpr int BWV = BT / EMMAX_WAVE;
constexpr int BG = EMMAX_SAMPLE_MAX_V / (4 * BT);   // groups of four entries per lane
constexpr int C2 = 2 * EMMAX_MAX_BEAMS;             // candidate slots per row / group

struct BeamShared {
    float rf[BWV];
    int ri[BWV];
    float best_v;
    int best_i;
};

__device__ __forceinline__ bool bbetter(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ float bblock_max(float v, BeamShared& sh, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if (lane == 0) sh.rf[wave] = v;
    __syncthreads();
    float r = sh.rf[0];
#pragma unroll
    for (int w = 1; w < BWV; ++w) r = fmaxf(r, sh.rf[w]);
    __syncthreads();
    return r;
}
__device__ float bblock_sum(float v, BeamShared& sh, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) sh.rf[wave] = v;
    __syncthreads();
    float r = sh.rf[0];
#pragma unroll
    for (int w = 1; w < BWV; ++w) r += sh.rf[w];
    __syncthreads();
    return r;
}

// Block b = one running row.  Prefill form (rows_per_group == 1): block g reads the prefill's logit row g and writes slot g * K with score 0
// (the initial running scores [0, -1e9, ...] leave only beam 0's continuations among the top 2K).
__global__ __launch_bounds__(BT) void emmax_beam_rows_kernel(BeamRowParams p) {
    __shared__ BeamShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (EMMAX_WAVE - 1), wave = tid / EMMAX_WAVE;
    const int V = p.V, K = p.K;
    const int slot = p.is_prefill ? b * K : b;
    if (!p.is_prefill && p.done[slot] != 0) return;   // the group is done (block-uniform: one word per row)
    const float* row = p.logits + (size_t)b * p.ld;
    const bool vec = ((uintptr_t)row & 15) == 0;
    float z[BG * 4];
#pragma unroll
    for (int g = 0; g < BG; ++g) {
        const int i0 = (g * BT + tid) * 4;
        if (vec && i0 + 3 < V) {
            const f32x4_t v = *(const f32x4_t*)(row + i0);
#pragma unroll
            for (int c = 0; c < 4; ++c) z[g * 4 + c] = v[c];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) z[g * 4 + c] = (i0 + c < V) ? row[i0 + c] : -INFINITY;
        }
    }
    // the raw row, at the step's index, into the caller's logits buffer (emmax_session_set_scores)
    const int step = p.is_prefill ? 0 : p.n_out[slot];
    if (p.score_words) {
        float* lg = (float*)p.score_words[1];
        const int t_max = (int)p.score_words[2], rows = (int)p.score_words[3];
        if (lg && step < t_max && slot < rows) {
            const size_t off = ((size_t)step * rows + slot) * V;
            for (int i = tid; i < V; i += BT) lg[off + i] = row[i];
        }
    }
    // logsumexp of the raw logits: the order of emmax_sample_kernel (per-lane, wave butterfly, the 16 waves in order)
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < BG * 4; ++j) mx = fmaxf(mx, z[j]);
    mx = bblock_max(mx, sh, lane, wave);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < BG * 4; ++j) se += expf(z[j] - mx);
    se = bblock_sum(se, sh, lane, wave);
    const float lse = mx + logf(se);
    const float score = p.is_prefill ? 0.f : p.run_score[slot];
    // acc = fp32(fp32(l - lse) + score): two correctly rounded operations (no product anywhere: nothing to contract)
#pragma unroll
    for (int j = 0; j < BG * 4; ++j) z[j] = (z[j] - lse) + score;
    if (tid == 0) p.row_lse[slot] = lse;
    // the best 2K entries in (acc descending, token ascending) order: round r takes the best entry strictly behind round r - 1's.
    // NaN never compares: a row with a NaN has lse = NaN and contributes nothing
    float lv = INFINITY;
    int li = -1;
    for (int r = 0; r < 2 * K; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int g = 0; g < BG; ++g)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = (g * BT + tid) * 4 + c;
                const float v = z[g * 4 + c];
                const bool behind = v < lv || (v == lv && i > li);
                if (i < V && behind && bbetter(v, i, bv, bi)) { bv = v; bi = i; }
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (bbetter(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { sh.rf[wave] = bv; sh.ri[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            float v = sh.rf[0];
            int i = sh.ri[0];
            for (int w = 1; w < BWV; ++w)
                if (bbetter(sh.rf[w], sh.ri[w], v, i)) { v = sh.rf[w]; i = sh.ri[w]; }
            sh.best_v = v; sh.best_i = i;
        }
        __syncthreads();
        lv = sh.best_v; li = sh.best_i;
        const bool none = li == 0x7fffffff;
        if (tid == 0) {
            p.cand_acc[(size_t)slot * C2 + r] = none ? 0.f : lv;
            p.cand_tok[(size_t)slot * C2 + r] = none ? -1 : li;
        }
        if (none) {   // nothing is left: the remaining slots are empty (block-uniform)
            if (tid == 0)
                for (int q = r + 1; q < 2 * K; ++q) { p.cand_acc[(size_t)slot * C2 + q] = 0.f; p.cand_tok[(size_t)slot * C2 + q] = -1; }
            break;
        }
        __syncthreads();
    }
}

constexpr float NEG1E9 = -1.0e9f;

// the first not yet taken entry, replaced by any later one that compares greater: (value descending, index ascending), a NaN only where it
// comes first.  tests/beam_ref.py restates exactly this
__device__ int take_best(const float* v, int n, uint32_t& taken) {
    int best = -1;
    for (int i = 0; i < n; ++i) {
        if ((taken >> i) & 1u) continue;
        if (best < 0 || v[i] > v[best]) best = i;
    }
    if (best >= 0) taken |= 1u << best;
    return best;
}

// One wave per group.  Thread 0 runs the merge and HF's updates (K <= 8: a few hundred scalar operations); all lanes gather the page table.
__global__ __launch_bounds__(EMMAX_WAVE) void emmax_beam_merge_kernel(BeamMergeParams p) {
    const int g = blockIdx.x, tid = threadIdx.x, K = p.K, r0 = g * K;
    __shared__ int s_par[EMMAX_MAX_BEAMS];
    __shared__ int s_go, s_L;
    int32_t* gst = p.grp_state + 4 * g;   // {heuristic unsatisfied, done, next free page, -}
    if (!p.is_prefill && gst[1] != 0) {
        if (tid < K) p.copy_src[r0 + tid] = -1;
        return;
    }
    if (tid == 0) {
        const int t = p.is_prefill ? 0 : p.n_out[r0];
        const int n = t + 1, mx = p.max_new_p[r0];
        const int nrows = p.is_prefill ? 1 : K;
        // K-way merge of the rows' sorted lists: ties go to the lower flat index beam * V + token
        float c_acc[C2];
        int c_par[C2], c_tok[C2], head[EMMAX_MAX_BEAMS];
        for (int r = 0; r < nrows; ++r) head[r] = 0;
        int nc = 0;
        for (int c = 0; c < 2 * K; ++c) {
            int br = -1;
            float ba = 0.f;
            for (int r = 0; r < nrows; ++r) {
                if (head[r] >= 2 * K) continue;
                const size_t o = (size_t)(r0 + r) * C2 + head[r];
                if (p.cand_tok[o] < 0) continue;
                const float a = p.cand_acc[o];
                if (br < 0 || a > ba) { br = r; ba = a; }
            }
            if (br < 0) break;
            c_acc[nc] = ba; c_par[nc] = br; c_tok[nc] = p.cand_tok[(size_t)(r0 + br) * C2 + head[br]];
            head[br] += 1;
            nc += 1;
        }
        int go = 0;
        if (nc == 0) {   // no candidate left (NaN logits): the group is done with what it has
            gst[1] = 1;
            for (int j = 0; j < K; ++j) { p.done[r0 + j] = 1; p.cur_tok[r0 + j] = p.pad_id; p.copy_src[r0 + j] = -1; }
        } else {
            bool hits[C2], all_hit = true;
            float rl[C2], fs[EMMAX_MAX_BEAMS + C2];
            for (int c = 0; c < nc; ++c) {
                hits[c] = c_tok[c] == p.eos_id || n >= mx;
                all_hit = all_hit && hits[c];
                rl[c] = hits[c] ? c_acc[c] + NEG1E9 : c_acc[c];
            }
            // running beams: the best K that did not stop
            int sel[EMMAX_MAX_BEAMS];
            uint32_t taken = 0;
            for (int j = 0; j < K; ++j) sel[j] = take_best(rl, nc, taken);
            // finished set: the kept K merged with the candidates, masked as HF masks them
            bool full = p.es_mode == 1;
            float o_score[EMMAX_MAX_BEAMS];
            int o_flag[EMMAX_MAX_BEAMS], o_t[EMMAX_MAX_BEAMS], o_par[EMMAX_MAX_BEAMS], o_tok[EMMAX_MAX_BEAMS];
            for (int k = 0; k < K; ++k) {
                o_score[k] = p.fin_score[r0 + k]; o_flag[k] = p.fin_flag[r0 + k]; o_t[k] = p.fin_t[r0 + k];
                o_par[k] = p.fin_par[r0 + k]; o_tok[k] = p.fin_tok[r0 + k];
                full = full && o_flag[k] != 0;
                fs[k] = o_score[k];
            }
            const bool unsat = gst[0] != 0;
            const float pwn = p.pw[n];
            for (int c = 0; c < nc; ++c) {
                float sc = c_acc[c] / pwn;
                if (full) sc = sc + NEG1E9;
                if (!unsat) sc = sc + NEG1E9;
                if (!(hits[c] && c < K)) sc = sc + NEG1E9;
                fs[K + c] = sc;
            }
            taken = 0;
            bool all_fin = true;
            float fmin = 0.f;
            for (int k = 0; k < K; ++k) {
                const int i = take_best(fs, K + nc, taken);
                float sc;
                int fl, ft, fp, fk;
                if (i < K) { sc = o_score[i]; fl = o_flag[i]; ft = o_t[i]; fp = o_par[i]; fk = o_tok[i]; }
                else { const int c = i - K; sc = fs[i]; fl = (hits[c] && c < K) ? 1 : 0; ft = t; fp = c_par[c]; fk = c_tok[c]; }
                p.fin_score[r0 + k] = sc; p.fin_flag[r0 + k] = fl; p.fin_t[r0 + k] = ft; p.fin_par[r0 + k] = fp; p.fin_tok[r0 + k] = fk;
                all_fin = all_fin && fl != 0;
                fmin = (k == 0 || sc < fmin) ? sc : fmin;
            }
            // early-stop heuristic and the group's done flag
            const int Lh = (p.es_mode == 2 && p.lp_pos) ? mx : n;
            const float best = rl[sel[0]] / p.pw[Lh];
            bool any = false;
            for (int k = 0; k < K; ++k) any = any || best > (p.fin_flag[r0 + k] ? fmin : NEG1E9);
            const bool unsat2 = unsat && any;
            gst[0] = unsat2 ? 1 : 0;
            const bool done = !(unsat2 && !(all_fin && p.es_mode == 1) && !all_hit);
            gst[1] = done ? 1 : 0;
            // trace, running state, per-row decode state
            const int L = p.is_prefill ? p.S[g] : p.ctx_len[r0] + 1;
            if (t < p.max_out) {
                for (int j = 0; j < K; ++j) {
                    const size_t o = (size_t)t * p.tr_ld + r0 + j;
                    p.tr_tok[o] = c_tok[sel[j]]; p.tr_par[o] = c_par[sel[j]]; p.tr_score[o] = rl[sel[j]];
                    p.tr_lse[o] = (p.is_prefill && j > 0) ? 0.f : p.row_lse[r0 + j];
                }
                for (int c = 0; c < 2 * K; ++c) {
                    const size_t o = (size_t)t * 2 * p.tr_ld + 2 * r0 + c;
                    p.tc_idx[o] = c < nc ? c_par[c] * p.V + c_tok[c] : -1;
                    p.tc_acc[o] = c < nc ? c_acc[c] : 0.f;
                }
            }
            for (int j = 0; j < K; ++j) {
                p.run_score[r0 + j] = rl[sel[j]];
                p.cur_tok[r0 + j] = done ? p.pad_id : c_tok[sel[j]];
                p.n_out[r0 + j] = n;
                p.ctx_len[r0 + j] = L;
                p.done[r0 + j] = done ? 1 : 0;
                s_par[j] = c_par[sel[j]];
                if (done) p.copy_src[r0 + j] = -1;
            }
            s_L = L;
            go = done ? 0 : 1;
        }
        s_go = go;
    }
    __syncthreads();
    if (!s_go) return;
    // ---- the cache follows the beams: page-table gather, the partial page copied into the spare and swapped ----
    const int L = s_L, mp = p.max_pages;
    int32_t* pt = p.page_table + (size_t)r0 * mp;
    if (p.is_prefill) {
        // fork: the prefill wrote the group's first row over the first pages of the group's pool; every beam references the complete ones
        const int P0 = r0 * mp, nfull = L / 64, rem = L % 64;
        for (int i = tid; i < nfull && i < mp; i += EMMAX_WAVE)
            for (int j = 0; j < K; ++j) pt[(size_t)j * mp + i] = P0 + i;
        if (tid == 0) p.grp_shared[g] = min(nfull, mp);   // the reorders below gather whole table rows: these entries stay equal in the group
        if (tid == 0 && nfull < mp) {
            int next = P0 + (L + 63) / 64;
            for (int j = 0; j < K; ++j) {
                const int cur = (rem > 0 && j == 0) ? P0 + nfull : next++;
                pt[(size_t)j * mp + nfull] = cur;
                const bool cp = rem > 0 && j > 0;
                p.copy_src[r0 + j] = cp ? P0 + nfull : -1;
                p.copy_dst[r0 + j] = cur;
                p.copy_ntok[r0 + j] = rem;
            }
            for (int j = 0; j < K; ++j) p.spare[r0 + j] = next++;
            gst[2] = next;
        }
        return;
    }
    const int pi = (L - 1) / 64;   // the page this step appended to
    for (int i = tid; i < pi && i < mp; i += EMMAX_WAVE) {
        int old[EMMAX_MAX_BEAMS];
        for (int j = 0; j < K; ++j) old[j] = pt[(size_t)j * mp + i];
        for (int j = 0; j < K; ++j) pt[(size_t)j * mp + i] = old[s_par[j]];
    }
    if (tid == 0 && pi < mp) {
        int oldcur[EMMAX_MAX_BEAMS];
        for (int j = 0; j < K; ++j) oldcur[j] = pt[(size_t)j * mp + pi];
        int next = gst[2];
        const bool complete = L % 64 == 0;   // the page is full now: immutable, shared by reference like the ones before it
        for (int j = 0; j < K; ++j) {
            const int pj = s_par[j];
            int src = -1, now = oldcur[j];
            if (pj != j) {
                if (complete) {
                    now = oldcur[pj];
                } else {
                    src = oldcur[pj];
                    now = p.spare[r0 + j];
                    p.spare[r0 + j] = oldcur[j];
                }
            }
            pt[(size_t)j * mp + pi] = now;
            p.copy_src[r0 + j] = src;
            p.copy_dst[r0 + j] = now;
            p.copy_ntok[r0 + j] = L - pi * 64;
            if (complete && pi + 1 < mp) pt[(size_t)j * mp + pi + 1] = next++;
        }
        gst[2] = next;
    }
}

// Copies of the partial pages the merge listed: block (x, layer * planes + plane, row) moves tokens [0, ntok) of every kv head of one plane
// of one layer from page src to page dst.  A row with nothing to copy costs its blocks one load.
__global__ __launch_bounds__(256) void emmax_beam_copy_kernel(BeamCopyParams p) {
    const int j = blockIdx.z;
    const int src = p.copy_src[j];
    if (src < 0) return;
    const int dst = p.copy_dst[j], ntok = p.copy_ntok[j];
    if (src >= p.n_pages || dst < 0 || dst >= p.n_pages || ntok < 1 || ntok > 64 || src == dst) return;
    const int layer = blockIdx.y / p.n_planes, pl = blockIdx.y - layer * p.n_planes;
    char* base = p.kv + (size_t)layer * p.layer_stride + p.plane_off[pl];
    const int rb = p.plane_rb[pl];
    const size_t page_bytes = (size_t)p.Hkv * 64 * rb;
    const char* s = base + (size_t)src * page_bytes;
    char* d = base + (size_t)dst * page_bytes;
    const int seg = ntok * rb;   // bytes per kv head
    if ((seg & 15) == 0) {
        const int nv = seg >> 4, total = p.Hkv * nv;
        for (int v = blockIdx.x * 256 + threadIdx.x; v < total; v += gridDim.x * 256) {
            const int h = v / nv, o = v - h * nv;
            const size_t off = (size_t)h * 64 * rb + (size_t)o * 16;
            const u32x4_t x = __builtin_nontemporal_load((const u32x4_t*)(s + off));
            __builtin_nontemporal_store(x, (u32x4_t*)(d + off));
        }
    } else {
        const int nv = seg >> 2, total = p.Hkv * nv;
        for (int v = blockIdx.x * 256 + threadIdx.x; v < total; v += gridDim.x * 256) {
            const int h = v / nv, o = v - h * nv;
            const size_t off = (size_t)h * 64 * rb + (size_t)o * 4;
            *(uint32_t*)(d + off) = *(const uint32_t*)(s + off);
        }
    }
}

// fresh beam state of G groups (before the fork): running / finished scores, flags, group words
__global__ void emmax_beam_reset_kernel(int rows, int K, float* run_score, float* fin_score, int32_t* fin_flag, int32_t* fin_t, int32_t* fin_par,
                                        int32_t* fin_tok, int32_t* grp_state, int32_t* copy_src) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    run_score[r] = (r % K) == 0 ? 0.f : NEG1E9;
    fin_score[r] = NEG1E9;
    fin_flag[r] = 0; fin_t[r] = -1; fin_par[r] = 0; fin_tok[r] = -1;
    copy_src[r] = -1;
    if ((r % K) == 0) {
        int32_t* gst = grp_state + 4 * (r / K);
        gst[0] = 1; gst[1] = 0; gst[2] = 0; gst[3] = 0;
    }
}

// page_table[r][i] = base(r) + i: the identity (step 1) or, before a beam prefill, row g over the pool of group g (step K)
__global__ void emmax_beam_pages_kernel(int32_t* pt, int rows, int max_pages, int step) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * max_pages) return;
    const int r = i / max_pages, c = i - r * max_pages;
    pt[i] = r * step * max_pages + c;
}

// ---- sample groups: N sampled rows per prompt on the prompt's pages (include/emmax.h: emmax_session_set_sample_groups) ----
// One wave per group.  Nothing is reordered after this fork, so there are no spares: row g N + j references the complete prompt pages of
// row g N (where the prefill wrote them) and owns every page from the partial one on, out of its own static share r * max_pages + i.
__global__ __launch_bounds__(EMMAX_WAVE) void emmax_group_fork_kernel(GroupForkParams p) {
    const int g = blockIdx.x, tid = threadIdx.x, N = p.N, mp = p.max_pages, r0 = g * N;
    const int L = p.S[g], nfull = L / 64, rem = L % 64;
    for (int e = tid; e < N * mp; e += EMMAX_WAVE) {
        const int j = e / mp, i = e - j * mp;
        p.page_table[(size_t)(r0 + j) * mp + i] = (i < nfull ? r0 : r0 + j) * mp + i;
    }
    if (tid == 0) p.grp_shared[g] = min(nfull, mp);
    for (int j = tid; j < N; j += EMMAX_WAVE) {
        const int r = r0 + j;
        p.st.ctx_len[r] = L; p.st.done[r] = 0; p.st.n_out[r] = 0;
        p.st.max_new[r] = 0x7fffffff;   // (as emmax_prefill_state_kernel: no token budget until a generate call sets one)
        p.st.stop_m[r] = 0; p.st.stop_after[r] = -1;
        const bool cp = rem > 0 && j > 0 && nfull < mp;
        p.copy_src[r] = cp ? r0 * mp + nfull : -1;
        p.copy_dst[r] = r * mp + nfull;
        p.copy_ntok[r] = rem;
    }
}

// W = 16 (rows are multiples of 16 bytes at a 16-byte aligned base) or 4 bytes per column
template <class T>
__global__ __launch_bounds__(256) void emmax_group_bcast_kernel(char* rows, long long row_bytes, int G, int N) {
    const long long ncol = row_bytes / (long long)sizeof(T);
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < ncol; c += (long long)gridDim.x * 256)
        for (int g = G - 1; g >= 0; --g) {   // rows written so far lie behind (g + 1) N > g: every source is read before it is overwritten
            const T x = *(const T*)(rows + (size_t)g * row_bytes + (size_t)c * sizeof(T));
            for (int j = N - 1; j >= (g == 0 ? 1 : 0); --j) *(T*)(rows + ((size_t)g * N + j) * row_bytes + (size_t)c * sizeof(T)) = x;
        }
}

// the kept hypotheses, best first: thread (g, k) walks hypothesis k of group g back through the parent table
__global__ void emmax_beam_resolve_kernel(BeamResolveParams p) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.rows) return;
    const int g = r / p.K, r0 = g * p.K;
    int32_t* seq = p.seq + (size_t)r * p.max_out;
    int32_t* bix = p.bidx + (size_t)r * p.max_out;
    const int ft = p.fin_t[r];
    const int len = (ft >= 0 && ft < p.max_out) ? ft + 1 : 0;
    for (int i = len; i < p.max_new && i < p.max_out; ++i) { seq[i] = p.pad_id; bix[i] = -1; }
    p.len[r] = len;
    p.score[r] = p.fin_score[r];
    if (len == 0) return;
    int b = p.fin_par[r];
    seq[ft] = p.fin_tok[r];
    bix[ft] = r0 + b;
    for (int t = ft - 1; t >= 0; --t) {
        if (b < 0 || b >= p.K) break;
        const size_t o = (size_t)t * p.tr_ld + r0 + b;
        seq[t] = p.tr_tok[o];
        b = p.tr_par[o];
        bix[t] = r0 + b;
    }
}

}  // namespace

int launch_beam_rows(const BeamRowParams& p, int blocks, hipStream_t stream) {
    if (blocks < 1 || p.V < 2 * p.K || p.V > EMMAX_SAMPLE_MAX_V || p.ld < p.V || p.K < 2 || p.K > EMMAX_MAX_BEAMS) return -1;
    hipLaunchKernelGGL(emmax_beam_rows_kernel, dim3(blocks), dim3(BT), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_beam_merge(const BeamMergeParams& p, int groups, hipStream_t stream) {
    if (groups < 1 || p.K < 2 || p.K > EMMAX_MAX_BEAMS || p.max_pages < 1) return -1;
    hipLaunchKernelGGL(emmax_beam_merge_kernel, dim3(groups), dim3(EMMAX_WAVE), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_beam_copy(const BeamCopyParams& p, int rows, int n_layers, hipStream_t stream) {
    if (rows < 1 || n_layers < 1 || p.n_planes < 1 || p.n_planes > 4 || p.Hkv < 1) return -1;
    for (int i = 0; i < p.n_planes; ++i)
        if (p.plane_rb[i] < 4 || (p.plane_rb[i] & 3) || ((p.plane_rb[i] * 64) & 15)) return -1;
    // enough blocks to fill the chip when every row copies: a 7B page (32 heads x 64 tokens x 256 bytes) is 32768 vectors = 8 x 256 x 16
    hipLaunchKernelGGL(emmax_beam_copy_kernel, dim3(8, n_layers * p.n_planes, rows), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_beam_reset(int rows, int K, float* run_score, float* fin_score, int32_t* fin_flag, int32_t* fin_t, int32_t* fin_par, int32_t* fin_tok,
                      int32_t* grp_state, int32_t* copy_src, hipStream_t stream) {
    hipLaunchKernelGGL(emmax_beam_reset_kernel, dim3((rows + 63) / 64), dim3(64), 0, stream, rows, K, run_score, fin_score, fin_flag, fin_t, fin_par,
                       fin_tok, grp_state, copy_src);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_beam_pages(int32_t* pt, int rows, int max_pages, int step, hipStream_t stream) {
    const int n = rows * max_pages;
    hipLaunchKernelGGL(emmax_beam_pages_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, pt, rows, max_pages, step);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_group_fork(const GroupForkParams& p, int groups, hipStream_t stream) {
    if (groups < 1 || p.N < 2 || (long long)groups * p.N > EMMAX_MAX_DECODE_BATCH || p.max_pages < 1) return -1;
    for (int g = 0; g < groups; ++g)
        if (p.S[g] < 1 || p.S[g] >= p.max_pages * 64) return -1;
    hipLaunchKernelGGL(emmax_group_fork_kernel, dim3(groups), dim3(EMMAX_WAVE), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_group_bcast(void* rows, long long row_bytes, int groups, int N, hipStream_t stream) {
    if (!rows || groups < 1 || N < 2 || (long long)groups * N > EMMAX_MAX_DECODE_BATCH || row_bytes < 4 || (row_bytes & 3)) return -1;
    const bool wide = (row_bytes & 15) == 0 && ((uintptr_t)rows & 15) == 0;
    const long long ncol = row_bytes / (wide ? 16 : 4);
    const int blocks = (int)std::min<long long>((ncol + 255) / 256, 1024);
    if (wide) hipLaunchKernelGGL(emmax_group_bcast_kernel<u32x4_t>, dim3(blocks), dim3(256), 0, stream, (char*)rows, row_bytes, groups, N);
    else hipLaunchKernelGGL(emmax_group_bcast_kernel<uint32_t>, dim3(blocks), dim3(256), 0, stream, (char*)rows, row_bytes, groups, N);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
int launch_beam_resolve(const BeamResolveParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(emmax_beam_resolve_kernel, dim3((p.rows + 63) / 64), dim3(64), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
