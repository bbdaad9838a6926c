// sample.hip -- seeded temperature / top-k / top-p sampling over rows of fp32 logits (emmax_op_sample, include/emmax.h).
//
// One 1024-thread workgroup per row; the row (V <= 32768) sits in registers, 32 entries per lane as 8 groups of 4 consecutive ids
// (entry i = 4 (g * 1024 + tid) + c), so one Philox4x32-10 call gives the noise of a lane's four entries.  Per row:
//   1. row maximum and logsumexp of the raw logits (wave butterflies, then the 16 wave results in a fixed order): the log-probability
//      l_tok - logsumexp(l) of the emitted token;
//   2. temperature 0: the token is the argmax, lowest id on ties;
//   3. z = l / T; top-k threshold = the k-th largest z, top-p threshold over the kept entries with integer masses
//      W_i = floor(exp(z_i - max z) 2^32): both by one radix walk over the order-preserving uint32 key of z (8-bit digits, per-wave LDS
//      histograms of 64-bit integer masses, integer atomics only -- the kept set does not depend on the order work arrives in);
//   4. Gumbel-max over the kept entries: token = argmax z_i + g_i, g_i = -log(-log u_i), u_i from Philox4x32-10 with key = seed and
//      counter (i / 4, step, subseq, 0) -- noise that depends on (seed, subseq, step, i) only, not on the row's place in the batch.
// No float atomics anywhere: every reduction has a fixed order, and two launches on the same inputs agree bit for bit.
// The kernel body and its helpers are sample_kernel.h (sample_con.hip instantiates the constrained form from it); here: the top-N kernel and the
// launchers of the five forms this object holds.
#include "sample_kernel.h"

namespace {

// ---- top-N and watched-token log-probabilities (include/emmax.h: emmax_op_top_logprobs; kernels.h: TopLogprobParams) -----------------
// A kernel of its own beside the finish, not one more form of emmax_sample_kernel (whose processing finish already spills).  Per row:
//   1. the row into registers and its lse, exactly as emmax_sample_kernel does both (block_max / block_sum: the same bits);
//   2. NaN entries take the one key below every number (0) and -0 becomes +0, so that key order is the order of the fp32 values; the key of
//      the n-th largest entry by radix_threshold over the keys >= 1;
//   3. the entries above that key, and of those equal to it the lowest ids (their rank by id: one integer block scan of the lanes' counts per
//      register group -- ids rise with the group, then the lane), into LDS: at most n of them, in the order the atomics hand out;
//   4. wave 0 ranks them by (key descending, id ascending) -- a total order, so the result does not depend on step 3's -- and writes the pairs;
//   5. the watched entries straight from the row.
struct TopShared {
    uint32_t key[EMMAX_MAX_TOP_LOGPROBS];
    int id[EMMAX_MAX_TOP_LOGPROBS];
    int n;
    unsigned long long wsum[2][SWV];
};

__global__ __launch_bounds__(ST) void emmax_top_logprobs_kernel(TopLogprobParams p) {
    __shared__ SampleShared sh;
    __shared__ TopShared ts;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (EMMAX_WAVE - 1), wave = tid / EMMAX_WAVE;
    const int V = p.V;
    int nt = p.n_top, nw = p.n_watch;
    int32_t* ti = p.top_ids;
    float *tl = p.top_lp, *wl = p.watch_lp;
    if (p.words) {   // the step form: entry [row][t] of the bound buffers, for a row that emits a token now (block-uniform)
        const int t = p.n_out[b];
        if (!p.is_prefill && (p.done[b] != 0 || t >= p.max_new_p[b])) return;
        const int T = (int)p.words[TOPLP_W_MAXNEW];
        if (t < 0 || t >= T) return;
        nt = (int)p.words[TOPLP_W_NTOP]; nw = (int)p.words[TOPLP_W_NWATCH];
        const size_t e = (size_t)(p.row0 + b) * T + t;
        ti = (int32_t*)p.words[TOPLP_W_IDS] + e * nt; tl = (float*)p.words[TOPLP_W_LP] + e * nt; wl = (float*)p.words[TOPLP_W_WATCH] + e * nw;
    } else {
        ti += (size_t)b * nt; tl += (size_t)b * nt; wl += (size_t)b * nw;
    }
    nt = min(max(nt, 0), min(EMMAX_MAX_TOP_LOGPROBS, V));   // (the host checked both: the LDS lists hold this many)
    nw = min(max(nw, 0), EMMAX_MAX_WATCH_IDS);
    const float* row = p.logits + (size_t)b * p.ld;
    const bool vec = ((uintptr_t)row & 15) == 0;
    float z[SG * 4];
#pragma unroll
    for (int g = 0; g < SG; ++g) {
        const int i0 = (g * ST + tid) * 4;
        if (vec && i0 + 3 < V) {
            const f32x4_t v = *(const f32x4_t*)(row + i0);
#pragma unroll
            for (int c = 0; c < 4; ++c) z[g * 4 + c] = v[c];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) z[g * 4 + c] = (i0 + c < V) ? row[i0 + c] : -INFINITY;
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SG * 4; ++j) mx = fmaxf(mx, z[j]);
    mx = block_max(mx, sh, lane, wave);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < SG * 4; ++j) se += expf(z[j] - mx);
    se = block_sum(se, sh, lane, wave);
    const float lse = mx + logf(se);

    if (nt > 0) {
#pragma unroll
        for (int j = 0; j < SG * 4; ++j) z[j] = (z[j] != z[j]) ? __uint_as_float(0xffffffffu) : z[j] + 0.f;
        const uint32_t thr = radix_threshold<false>(z, 0.f, tid, V, 1u, (double)nt, sh, lane, wave);
        uint32_t gt = 0, eq = 0;   // bit j: entry z[j] is above / at the threshold key
#pragma unroll
        for (int j = 0; j < SG * 4; ++j) {
            const uint32_t key = fkey(z[j]);
            if (entry_id(j, tid) < V && key >= 1u) {
                if (key > thr) gt |= 1u << j;
                else if (key == thr) eq |= 1u << j;
            }
        }
        const int n_gt = (int)block_sum_u64((unsigned long long)__popc(gt), sh, lane, wave);   // < nt: what the threshold means
        // the lanes' counts of threshold entries per register group, 16 bits each (a group holds at most 4096), scanned over the block
        unsigned long long mine[2] = {0ull, 0ull}, incl[2];
#pragma unroll
        for (int g = 0; g < SG; ++g) mine[g >> 2] |= (unsigned long long)__popc((eq >> (g * 4)) & 15u) << ((g & 3) * 16);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            incl[h] = mine[h];
#pragma unroll
            for (int o = 1; o < EMMAX_WAVE; o <<= 1) {
                const unsigned long long t = __shfl_up(incl[h], o);
                if (lane >= o) incl[h] += t;
            }
            if (lane == EMMAX_WAVE - 1) ts.wsum[h][wave] = incl[h];
        }
        if (tid == 0) ts.n = 0;
        __syncthreads();
        int before = 0;   // threshold entries of the groups below the one at hand
        const int need = nt - n_gt;
#pragma unroll
        for (int g = 0; g < SG; ++g) {
            const int h = g >> 2, sft = (g & 3) * 16;
            unsigned long long below = 0, all = 0;
#pragma unroll
            for (int w = 0; w < SWV; ++w) {
                const unsigned long long s = ts.wsum[h][w];
                if (w < wave) below += s;
                all += s;
            }
            int rank = before + (int)(((below + incl[h] - mine[h]) >> sft) & 0xffffu);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = g * 4 + c;
                const bool is_eq = (eq >> j) & 1u;
                if (((gt >> j) & 1u) || (is_eq && rank < need)) {
                    const int slot = atomicAdd(&ts.n, 1);
                    if (slot < EMMAX_MAX_TOP_LOGPROBS) { ts.key[slot] = fkey(z[j]); ts.id[slot] = entry_id(j, tid); }
                }
                if (is_eq) rank += 1;
            }
            before += (int)((all >> sft) & 0xffffu);
        }
        __syncthreads();
        if (wave == 0 && lane < nt) {
            const int n = min(ts.n, nt);
            if (lane < n) {
                const uint32_t key = ts.key[lane];
                const int id = ts.id[lane];
                int r = 0;
                for (int k = 0; k < n; ++k) r += (ts.key[k] > key || (ts.key[k] == key && ts.id[k] < id)) ? 1 : 0;
                ti[r] = id;
                tl[r] = row[id] - lse;
            } else {   // fewer than n_top entries that are not NaN
                ti[lane] = -1;
                tl[lane] = -INFINITY;
            }
        }
    }
    for (int w = tid; w < nw; w += ST) {
        const int id = p.watch_ids[w];
        wl[w] = (id >= 0 && id < V) ? row[id] - lse : __int_as_float(0x7fc00000);
    }
}


}  // namespace

int launch_top_logprobs(const TopLogprobParams& p, int B, hipStream_t stream) {
    if (B < 1 || p.V < 1 || p.V > EMMAX_SAMPLE_MAX_V || p.ld < p.V || !p.logits) return -1;
    if (p.words) {
        if (!p.n_out || !p.done || !p.max_new_p || !p.watch_ids || p.row0 < 0) return -1;
    } else {
        if (p.n_top < 0 || p.n_top > EMMAX_MAX_TOP_LOGPROBS || p.n_top > p.V || p.n_watch < 0 || p.n_watch > EMMAX_MAX_WATCH_IDS) return -1;
        if (p.n_top > 0 && (!p.top_ids || !p.top_lp)) return -1;
        if (p.n_watch > 0 && (!p.watch_ids || !p.watch_lp)) return -1;
        if (p.n_top == 0 && p.n_watch == 0) return 0;   // both parts off: nothing to compute
    }
    hipLaunchKernelGGL(emmax_top_logprobs_kernel, dim3(B), dim3(ST), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_sample(const SampleParams& p, int B, hipStream_t stream) {
    if (B < 1 || p.V < 1 || p.V > EMMAX_SAMPLE_MAX_V || p.ld < p.V) return -1;
    hipLaunchKernelGGL(emmax_sample_kernel<SampleParams>, dim3(B), dim3(ST), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_proc_finish(const ProcFinishParams& p, hipStream_t stream) {
    if (p.f.B < 1 || p.V < 1 || p.V > EMMAX_SAMPLE_MAX_V || p.ld < p.V) return -1;
    if (p.penalty && (!p.ngram || !p.min_new || !p.hist || !p.hist_len || p.max_prompt < 1)) return -1;
    hipLaunchKernelGGL(emmax_sample_kernel<ProcFinishParams>, dim3(p.f.B), dim3(ST), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_sample_finish(const SampleFinishParams& p, hipStream_t stream) {
    if (p.f.B < 1 || p.V < 1 || p.V > EMMAX_SAMPLE_MAX_V || p.ld < p.V) return -1;
    hipLaunchKernelGGL(emmax_sample_kernel<SampleFinishParams>, dim3(p.f.B), dim3(ST), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_ext_finish(const ExtFinishParams& p, hipStream_t stream) {
    if (p.f.B < 1 || p.V < 1 || p.V > EMMAX_SAMPLE_MAX_V || p.ld < p.V) return -1;
    if (p.penalty && (!p.ngram || !p.min_new || !p.hist || !p.hist_len || p.max_prompt < 1)) return -1;
    if (p.rt.off && (!p.penalty || !p.rt.ids || !p.rt.flags || !p.rt.bias || !p.rule_en || (!p.rt.n && (p.rt.n_host < 0 || p.rt.n_host > EMMAX_MAX_RULES)))) return -1;
    if (p.min_p && (!p.typical_p || !p.eps_cut || !p.eta_cut)) return -1;
    if (p.tok_out && (!p.logprob_out || !p.f.is_prefill || p.f.max_out != 0)) return -1;
    hipLaunchKernelGGL(emmax_sample_kernel<ExtFinishParams>, dim3(p.f.B), dim3(ST), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
