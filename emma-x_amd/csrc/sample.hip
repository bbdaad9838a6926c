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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int ST = 1024;            // threads per row
constexpr int SWV = ST / EMMAX_WAVE;
constexpr int SG = EMMAX_SAMPLE_MAX_V / (4 * ST);   // groups of four entries per lane

// order-preserving key: a < b  <=>  fkey(a) < fkey(b) (finite values and infinities)
__device__ __forceinline__ uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), counter c, key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    }
}

// g = -log(-log u), u = ((x >> 8) + 0.5) 2^-24.  -log u is evaluated on exactly representable floats: -logf(u) below 1/2,
// -log1pf(-(1 - u)) above (u itself would round to 1 at the top of the range and give an infinite g)
__device__ __forceinline__ float gumbel_of(uint32_t x) {
    const uint32_t k = x >> 8;
    const float e = (k < (1u << 23)) ? -logf((float)(2u * k + 1u) * 0x1p-25f) : -log1pf(-(float)((1u << 25) - 2u * k - 1u) * 0x1p-25f);
    return -logf(e);
}

// top-p mass of an entry: floor(exp(z - max z) 2^32) (exact scaling by 2^32, truncating conversion)
__device__ __forceinline__ unsigned long long mass_of(float z, float zmax) { return (unsigned long long)(expf(z - zmax) * 4294967296.0f); }

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

struct SampleShared {
    unsigned long long hist[SWV][256];
    unsigned long long tot[256];
    float rf[SWV];
    int ri[SWV];
    unsigned long long ru[SWV];
    unsigned long long sel_a;
    int sel_d;
};

// block reductions: wave butterfly (every lane of a wave ends with the same value), then the 16 wave values in wave order
__device__ float block_max(float v, SampleShared& sh, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if (lane == 0) sh.rf[wave] = v;
    __syncthreads();
    float r = sh.rf[0];
#pragma unroll
    for (int w = 1; w < SWV; ++w) r = fmaxf(r, sh.rf[w]);
    __syncthreads();
    return r;
}
__device__ float block_sum(float v, SampleShared& sh, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) sh.rf[wave] = v;
    __syncthreads();
    float r = sh.rf[0];
#pragma unroll
    for (int w = 1; w < SWV; ++w) r += sh.rf[w];
    __syncthreads();
    return r;
}
__device__ unsigned long long block_sum_u64(unsigned long long v, SampleShared& sh, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) sh.ru[wave] = v;
    __syncthreads();
    unsigned long long r = 0;
#pragma unroll
    for (int w = 0; w < SWV; ++w) r += sh.ru[w];
    __syncthreads();
    return r;
}
// (value, index) argmax, ties to the lowest index
__device__ int block_argmax(float v, int i, SampleShared& sh, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if (lane == 0) { sh.rf[wave] = v; sh.ri[wave] = i; }
    __syncthreads();
    float bv = sh.rf[0];
    int bi = sh.ri[0];
#pragma unroll
    for (int w = 1; w < SWV; ++w)
        if (better(sh.rf[w], sh.ri[w], bv, bi)) { bv = sh.rf[w]; bi = sh.ri[w]; }
    __syncthreads();
    return bi;
}

// Radix walk over the keys of the entries with key >= lo (entry mass: 1, or floor(w 2^32) when MASS).  Returns the threshold key t:
// the entries with key >= t are exactly those whose mass strictly above them, sum_{key_j > key_i} mass_j, is below `target`
// (or zero: the maximum is always kept).  With unit masses and target k that is "key >= the k-th largest key" (ties kept).
template <bool MASS>
__device__ uint32_t radix_threshold(const float (&z)[SG * 4], float zmax, int tid, int V, uint32_t lo, double target,
                                    SampleShared& sh, int lane, int wave) {
    uint32_t prefix = 0, mask = 0;
    unsigned long long above = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int j = lane; j < 256; j += EMMAX_WAVE) sh.hist[wave][j] = 0;
        __syncthreads();
#pragma unroll
        for (int g = 0; g < SG; ++g)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = (g * ST + tid) * 4 + c;
                const uint32_t key = fkey(z[g * 4 + c]);
                if (i < V && key >= lo && (key & mask) == prefix) {
                    const unsigned long long m = MASS ? mass_of(z[g * 4 + c], zmax) : 1ull;
                    atomicAdd(&sh.hist[wave][(key >> shift) & 255u], m);
                }
            }
        __syncthreads();
        if (tid < 256) {
            unsigned long long s = 0;
#pragma unroll
            for (int v = 0; v < SWV; ++v) s += sh.hist[v][tid];
            sh.tot[tid] = s;
        }
        __syncthreads();
        if (wave == 0) {   // lane l holds bins 4l .. 4l + 3; S(d) = mass in the bins above d
            const unsigned long long c0 = sh.tot[4 * lane], c1 = sh.tot[4 * lane + 1], c2 = sh.tot[4 * lane + 2], c3 = sh.tot[4 * lane + 3];
            const unsigned long long mine = c0 + c1 + c2 + c3;
            unsigned long long incl = mine;   // inclusive suffix sum over lanes lane .. 63
#pragma unroll
            for (int o = 1; o < EMMAX_WAVE; o <<= 1) {
                const unsigned long long t = __shfl_down(incl, o);
                if (lane + o < EMMAX_WAVE) incl += t;
            }
            const unsigned long long up = above + (incl - mine);
            const unsigned long long s3 = up, s2 = up + c3, s1 = s2 + c2, s0 = s1 + c1;
            auto ok = [&](unsigned long long s) { return s == 0 || (double)s < target; };
            // the satisfying bins are a top range (S falls as d rises): the lowest one of the lowest lane that has one
            const int dl = ok(s0) ? 0 : ok(s1) ? 1 : ok(s2) ? 2 : ok(s3) ? 3 : -1;
            const unsigned long long sd = dl == 0 ? s0 : dl == 1 ? s1 : dl == 2 ? s2 : s3;
            const unsigned long long bal = __ballot(dl >= 0);
            const int L = __ffsll((long long)bal) - 1;   // bin 255 always qualifies (S = the mass above the prefix, which qualified)
            if (lane == L) {
                sh.sel_d = 4 * lane + dl;
                sh.sel_a = sd;
            }
        }
        __syncthreads();
        prefix |= (uint32_t)sh.sel_d << shift;
        mask |= 255u << shift;
        above = sh.sel_a;
        __syncthreads();
    }
    return prefix;
}

// the Philox step of row b: the caller's (emmax_op_sample), or the row's generation index n_out (the finish of a sampled decode step: 0 for
// the token a prefill emits)
__device__ __forceinline__ int row_step(const SampleParams& p, int b) { return p.step[b]; }
__device__ __forceinline__ int row_step(const SampleFinishParams& p, int b) { return p.f.n_out[b]; }
// the row's temperature: a processing / scores finish with sampling off has none (every row greedy, whatever samp_t still holds)
__device__ __forceinline__ float row_temperature(const SampleParams& p, int b) { return p.temperature[b]; }
__device__ __forceinline__ float row_temperature(const SampleFinishParams& p, int b) { return p.temperature[b]; }
__device__ __forceinline__ float row_temperature(const ProcFinishParams& p, int b) { return p.temperature ? p.temperature[b] : 0.f; }

// id j of row b's history: the prompt ids, then the ids the row has emitted
__device__ __forceinline__ int hist_id(const int32_t* prompt, int plen, const int32_t* out, int j) { return j < plen ? prompt[j] : out[j - plen]; }

// ---- the EXT forms (include/emmax.h: emmax_op_sample_ext; kernels.h: ExtFinishParams) -----------------------------------------------
// entry j of a lane (register z[j]) is id 4 ((j / 4) ST + tid) + j % 4
__device__ __forceinline__ int entry_id(int j, int tid) { return ((j >> 2) * ST + tid) * 4 + (j & 3); }

// The radix walk of radix_threshold over any per-entry (active, key, mass): returns the threshold key t such that the active entries with
// key >= t are exactly those whose mass strictly above them is below `target` (or zero).  A copy of that walk rather than its generalisation:
// the existing instantiations are to keep their code object byte for byte
template <class F>
__device__ uint32_t radix_walk(F entry, double target, SampleShared& sh, int tid, int lane, int wave) {
    uint32_t prefix = 0, mask = 0;
    unsigned long long above = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int j = lane; j < 256; j += EMMAX_WAVE) sh.hist[wave][j] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SG * 4; ++j) {
            uint32_t key;
            unsigned long long m;
            if (entry(j, key, m) && (key & mask) == prefix) atomicAdd(&sh.hist[wave][(key >> shift) & 255u], m);
        }
        __syncthreads();
        if (tid < 256) {
            unsigned long long s = 0;
#pragma unroll
            for (int v = 0; v < SWV; ++v) s += sh.hist[v][tid];
            sh.tot[tid] = s;
        }
        __syncthreads();
        if (wave == 0) {   // lane l holds bins 4l .. 4l + 3; S(d) = mass in the bins above d
            const unsigned long long c0 = sh.tot[4 * lane], c1 = sh.tot[4 * lane + 1], c2 = sh.tot[4 * lane + 2], c3 = sh.tot[4 * lane + 3];
            const unsigned long long mine = c0 + c1 + c2 + c3;
            unsigned long long incl = mine;
#pragma unroll
            for (int o = 1; o < EMMAX_WAVE; o <<= 1) {
                const unsigned long long t = __shfl_down(incl, o);
                if (lane + o < EMMAX_WAVE) incl += t;
            }
            const unsigned long long up = above + (incl - mine);
            const unsigned long long s3 = up, s2 = up + c3, s1 = s2 + c2, s0 = s1 + c1;
            auto ok = [&](unsigned long long s) { return s == 0 || (double)s < target; };
            const int dl = ok(s0) ? 0 : ok(s1) ? 1 : ok(s2) ? 2 : ok(s3) ? 3 : -1;
            const unsigned long long sd = dl == 0 ? s0 : dl == 1 ? s1 : dl == 2 ? s2 : s3;
            const unsigned long long bal = __ballot(dl >= 0);
            const int L = __ffsll((long long)bal) - 1;
            if (lane == L) {
                sh.sel_d = 4 * lane + dl;
                sh.sel_a = sd;
            }
        }
        __syncthreads();
        prefix |= (uint32_t)sh.sel_d << shift;
        mask |= 255u << shift;
        above = sh.sel_a;
        __syncthreads();
    }
    return prefix;
}

// The warpers behind top-k / top-p (include/emmax.h), in HF's order, on the kept set `km` (bit j: entry j of this lane is kept) of the row
// z = l / T: min_p, typical_p, epsilon_cutoff, eta_cutoff.  Integer masses W = mass_of(z, zmax); every sum has a fixed order.
__device__ void warp_row(const ExtFinishParams& p, int b, int tid, const float (&z)[SG * 4], float zmax, uint32_t& km, SampleShared& sh,
                         int lane, int wave) {
    const float mp = p.min_p[b], ty = p.typical_p[b], ep = p.eps_cut[b], et = p.eta_cut[b];
    auto kept_mass = [&]() {
        unsigned long long t = 0;
#pragma unroll
        for (int j = 0; j < SG * 4; ++j)
            if ((km >> j) & 1u) t += mass_of(z[j], zmax);
        return block_sum_u64(t, sh, lane, wave);
    };
    // H = -sum p_i lp_i over the kept set: p_i = fp32(W_i) / fp32(S), lp_i = (z_i - zmax) - lnZ; lane entries in register order, then block_sum
    auto entropy = [&](float invS, float lnZ) {
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < SG * 4; ++j)
            if ((km >> j) & 1u) {
                const float pj = __fmul_rn((float)mass_of(z[j], zmax), invS);
                e = __fadd_rn(e, __fmul_rn(pj, (z[j] - zmax) - lnZ));
            }
        return -block_sum(e, sh, lane, wave);
    };
    if (mp > 0.f) {   // W_i >= floor(min_p 2^32): the maximum's mass is 2^32
        const unsigned long long M = (unsigned long long)(mp * 4294967296.0f);
#pragma unroll
        for (int j = 0; j < SG * 4; ++j)
            if (((km >> j) & 1u) && mass_of(z[j], zmax) < M) km &= ~(1u << j);
    }
    if (ty > 0.f && ty < 1.f) {
        const unsigned long long S = kept_mass();
        if (S > 0) {
            const float lnZ = logf((float)S * 0x1p-32f), invS = 1.f / (float)S;
            const float H = entropy(invS, lnZ);
            // ascending distance |(-lp_i) - H|: the walk runs on the complemented key
            auto entry = [&](int j, uint32_t& key, unsigned long long& m) {
                key = ~fkey(fabsf(-((z[j] - zmax) - lnZ) - H));
                m = mass_of(z[j], zmax);
                return ((km >> j) & 1u) != 0;
            };
            const uint32_t t = radix_walk(entry, (double)ty * (double)S, sh, tid, lane, wave);
#pragma unroll
            for (int j = 0; j < SG * 4; ++j)
                if (((km >> j) & 1u) && ~fkey(fabsf(-((z[j] - zmax) - lnZ) - H)) < t) km &= ~(1u << j);
        }
    }
    const bool eps_on = ep > 0.f && ep < 1.f, eta_on = et > 0.f && et < 1.f;
    if (eps_on || eta_on) {
        float cm = -INFINITY;   // the largest kept z (typical_p may have dropped the row's maximum): it always stays
#pragma unroll
        for (int j = 0; j < SG * 4; ++j)
            if ((km >> j) & 1u) cm = fmaxf(cm, z[j]);
        cm = block_max(cm, sh, lane, wave);
        for (int pass = 0; pass < 2; ++pass) {
            if (!(pass == 0 ? eps_on : eta_on)) continue;
            const unsigned long long S = kept_mass();
            if (S == 0) break;
            float cut = ep;
            if (pass == 1) {
                const float H = entropy(1.f / (float)S, logf((float)S * 0x1p-32f));
                cut = fminf(et, __fmul_rn(sqrtf(et), expf(-H)));
            }
            const double line = (double)cut * (double)S;   // keep W_i >= fp64(cut) fp64(S), one rounding
#pragma unroll
            for (int j = 0; j < SG * 4; ++j)
                if (((km >> j) & 1u) && (double)mass_of(z[j], zmax) < line && z[j] < cm) km &= ~(1u << j);
        }
    }
}

// The token rules of an EXT processing finish against the tail of the row's history (include/emmax.h): rule r = ids off[r] .. off[r + 1],
// flags (bits 0-1 kind: 0 sequence_bias, 1 bad_words, 2 suppress, 3 begin_suppress; bit 2: fires at n_out == 0 only), enabled by bit `kind`
// of the row's enable word.  A rule of n ids fires when n == 1, or n <= L and the history ends with its first n - 1 ids.  Bans go into the
// ban bitmap; a bias rule leaves its last id in lid[r] (-1: did not fire)
__device__ void match_rules(const ExtFinishParams& p, int b, int tid, int V, int n_out, const int32_t* prompt, int plen, const int32_t* out, int L,
                            int R, uint32_t* ban, int* lid) {
    const uint32_t en = p.rule_en[b];
    for (int r = tid; r < EMMAX_MAX_RULES; r += ST) {
        int hit = -1;
        if (r < R) {
            const int o = p.rt.off[r], n = p.rt.off[r + 1] - o, fl = p.rt.flags[r];
            if (o >= 0 && n >= 1 && n <= EMMAX_MAX_RULE_IDS && o + n <= EMMAX_MAX_RULE_TOTAL && ((en >> (fl & 3)) & 1u) && (!(fl & 4) || n_out == 0) &&
                (n == 1 || n <= L)) {
                bool same = true;
                for (int k = 0; k < n - 1 && same; ++k) same = hist_id(prompt, plen, out, L - (n - 1) + k) == p.rt.ids[o + k];
                const int id = p.rt.ids[o + n - 1];
                if (same && id >= 0 && id < V) {
                    if (fl & 3) atomicOr(&ban[id >> 5], 1u << (id & 31));
                    else hit = id;
                }
            }
        }
        lid[r] = hit;
    }
}

// The biases of the fired sequence_bias rules, added to the row held in z: per id the biases are summed in rule order from 0 (fp32), by the
// first fired rule of that id, and the sum is added once (HF: scores + bias) by the lane that holds the id
__device__ void apply_bias(const ExtFinishParams& p, int tid, int R, float (&z)[SG * 4], const int* lid, int* own, float* bsum) {
    for (int r = tid; r < EMMAX_MAX_RULES; r += ST) {
        const int id = r < R ? lid[r] : -1;
        bool first = id >= 0;
        for (int j = 0; j < r && first; ++j) first = lid[j] != id;
        float acc = 0.f;
        if (first)
            for (int j = r; j < R; ++j)
                if (lid[j] == id) acc += p.rt.bias[j];
        own[r] = first ? id : -1;
        bsum[r] = acc;
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        const int id = own[r];
        if (id >= 0 && ((id >> 2) & (ST - 1)) == tid) {
            const int jj = ((id >> 2) / ST) * 4 + (id & 3);
            const float a = bsum[r];
#pragma unroll
            for (int j = 0; j < SG * 4; ++j)
                if (j == jj) z[j] += a;
        }
    }
}

// The logits processors of a processing finish (include/emmax.h), in HF's order, on the row held in z (entry i = 4 (g * ST + tid) + c):
// repetition penalty over the distinct ids of the history, n-gram ban, EOS ban while n_out < min_new.  The presence and ban bitmaps are
// LDS words set with integer atomicOr only, so the processed row does not depend on the order work arrives in.
template <class P>
__device__ void process_row(const P& p, int b, int tid, int V, int n_out, float (&z)[SG * 4], uint32_t* pres, uint32_t* ban) {
    constexpr bool EXT = std::is_same<P, ExtFinishParams>::value;
    const float pen = p.penalty[b];
    const int ng = p.ngram[b], mn = p.min_new[b];
    const int plen = min(max(p.hist_len[b], 0), p.max_prompt);
    const int32_t* prompt = p.hist + (size_t)b * p.max_prompt;
    const int32_t* out = p.f.out_ids + (size_t)b * p.f.max_out;
    const int L = plen + min(n_out, p.f.max_out);
    const int W = (V + 31) / 32;
    for (int w = tid; w < W; w += ST) { pres[w] = 0u; ban[w] = 0u; }
    __syncthreads();
    [[maybe_unused]] int R = 0;
    if constexpr (EXT) {
        if (p.rt.off) {
            __shared__ int lid[EMMAX_MAX_RULES], own[EMMAX_MAX_RULES];
            __shared__ float bsum[EMMAX_MAX_RULES];
            R = min(max(p.rt.n ? *p.rt.n : p.rt.n_host, 0), EMMAX_MAX_RULES);
            match_rules(p, b, tid, V, n_out, prompt, plen, out, L, R, ban, lid);
            __syncthreads();
            apply_bias(p, tid, R, z, lid, own, bsum);
        }
    }
    if (pen != 1.f)
        for (int j = tid; j < L; j += ST) {
            const int id = hist_id(prompt, plen, out, j);
            if (id >= 0 && id < V) atomicOr(&pres[id >> 5], 1u << (id & 31));
        }
    if (ng > 0 && L >= ng)   // start j: H[j .. j + ng - 2] == H[L - ng + 1 .. L - 1] bans H[j + ng - 1]
        for (int j = tid; j + ng <= L; j += ST) {
            bool same = true;
            for (int k = 0; k < ng - 1 && same; ++k) same = hist_id(prompt, plen, out, j + k) == hist_id(prompt, plen, out, L - ng + 1 + k);
            if (same) {
                const int id = hist_id(prompt, plen, out, j + ng - 1);
                if (id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
            }
        }
    __syncthreads();
    const int eos = n_out < mn ? p.f.eos_id : -1;
#pragma unroll
    for (int g = 0; g < SG; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = (g * ST + tid) * 4 + c;
            if (i >= V) continue;
            float x = z[g * 4 + c];
            if ((pres[i >> 5] >> (i & 31)) & 1u) x = x < 0.f ? x * pen : x / pen;
            if (((ban[i >> 5] >> (i & 31)) & 1u) || i == eos) x = -INFINITY;
            z[g * 4 + c] = x;
        }
}

// a row of z (entry i = 4 (g * ST + tid) + c; the first V entries) to dst
__device__ __forceinline__ void store_row(float* dst, const float (&z)[SG * 4], int tid, int V) {
    const bool vec = ((uintptr_t)dst & 15) == 0;
#pragma unroll
    for (int g = 0; g < SG; ++g) {
        const int i0 = (g * ST + tid) * 4;
        if (vec && i0 + 3 < V) {
            *(f32x4_t*)(dst + i0) = f32x4_t{z[g * 4], z[g * 4 + 1], z[g * 4 + 2], z[g * 4 + 3]};
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i0 + c < V) dst[i0 + c] = z[g * 4 + c];
        }
    }
}

// One kernel body for all three uses, so the draw exists once: P = SampleParams is emmax_op_sample (token and log-probability out); P =
// SampleFinishParams is the finish of a sampled step (kernels.h), whose row then ends in the bookkeeping every finish shares; P =
// ProcFinishParams is that finish with the logits processors before the draw and the scores store after it.  (A template kernel rather
// than a shared device function: inlining the draw into two kernels raised the spills of this one from 75 to 88 VGPRs.)
template <class P>
__global__ __launch_bounds__(ST) void emmax_sample_kernel(P p) {
    constexpr bool EXT = std::is_same<P, ExtFinishParams>::value;   // the processing finish with the token rules and the further warpers
    constexpr bool PROC = std::is_same<P, ProcFinishParams>::value || EXT;
    constexpr bool FIN = std::is_same<P, SampleFinishParams>::value || PROC;
    __shared__ SampleShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (EMMAX_WAVE - 1), wave = tid / EMMAX_WAVE;
    const int V = p.V, step = row_step(p, b);
    const float* row = p.logits + (size_t)b * p.ld;
    if constexpr (FIN) {   // a row that is done, idle or out of budget reads no logits and draws nothing (block-uniform: one word per row)
        const FinishParams& f = p.f;
        if (!f.is_prefill && (f.done[b] != 0 || step >= f.max_new_p[b])) {
            if (tid == 0) emmax_finish_row(f, b, f.pad_id, p.logprob + (size_t)b * f.max_out, 0.f, false);
            return;
        }
    }
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
    // logsumexp of the raw logits, fixed order
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SG * 4; ++j) mx = fmaxf(mx, z[j]);
    mx = block_max(mx, sh, lane, wave);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < SG * 4; ++j) se += expf(z[j] - mx);
    se = block_sum(se, sh, lane, wave);
    const float lse = mx + logf(se);

    const float T = row_temperature(p, b);
    bool dead = false;   // (processing finish) no finite entry is left: the row emits pad and is done
    if constexpr (PROC) {
        if (p.penalty) {
            __shared__ uint32_t pres[EMMAX_SAMPLE_MAX_V / 32], ban[EMMAX_SAMPLE_MAX_V / 32];
            process_row(p, b, tid, V, step, z, pres, ban);
            mx = -INFINITY;   // the maximum of the processed row (z / T's is mx / T: division by T > 0 keeps the order)
#pragma unroll
            for (int j = 0; j < SG * 4; ++j) mx = fmaxf(mx, z[j]);
            mx = block_max(mx, sh, lane, wave);
            dead = !(mx > -INFINITY);
        }
    }
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    uint32_t kept = 0;   // (processing finish, T > 0) the kept set: key(z) >= kept
    [[maybe_unused]] uint32_t km = 0;   // (EXT, T > 0) the kept set: bit j = entry z[j]
    if (dead) {
    } else if (!(T > 0.f)) {   // greedy: argmax, lowest id on ties
#pragma unroll
        for (int g = 0; g < SG; ++g)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = (g * ST + tid) * 4 + c;
                if (i < V && better(z[g * 4 + c], i, bv, bi)) { bv = z[g * 4 + c]; bi = i; }
            }
    } else {
#pragma unroll
        for (int j = 0; j < SG * 4; ++j) z[j] = z[j] / T;
        const float zmax = mx / T;
        const int k = p.top_k[b];
        const float tp = p.top_p[b];
        uint32_t thr = 0;   // kept: key(z) >= thr
        if (k > 0 && k < V) thr = radix_threshold<false>(z, zmax, tid, V, 0u, (double)k, sh, lane, wave);
        if (tp < 1.f) {
            unsigned long long tot = 0;
#pragma unroll
            for (int g = 0; g < SG; ++g)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int i = (g * ST + tid) * 4 + c;
                    if (i < V && fkey(z[g * 4 + c]) >= thr) tot += mass_of(z[g * 4 + c], zmax);
                }
            tot = block_sum_u64(tot, sh, lane, wave);
            thr = radix_threshold<true>(z, zmax, tid, V, thr, (double)tp * (double)tot, sh, lane, wave);
        }
        kept = thr;
        // Gumbel-max over the kept entries; Philox only for groups with a kept entry
        const uint32_t k0 = (uint32_t)p.seed[b], k1 = (uint32_t)(p.seed[b] >> 32), sub = p.subseq[b];
        if constexpr (EXT) {   // the same draw over the kept bits the warpers leave (-inf and NaN entries are never kept)
#pragma unroll
            for (int j = 0; j < SG * 4; ++j)
                if (entry_id(j, tid) < V && fkey(z[j]) >= thr && z[j] > -INFINITY) km |= 1u << j;
            if (p.min_p) warp_row(p, b, tid, z, zmax, km, sh, lane, wave);
#pragma unroll
            for (int g = 0; g < SG; ++g) {
                if (!((km >> (g * 4)) & 15u)) continue;
                const int q = g * ST + tid;
                uint32_t x[4] = {(uint32_t)q, (uint32_t)step, sub, 0u};
                philox4x32_10(x, k0, k1);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if ((km >> (g * 4 + c)) & 1u) {
                        const float s = z[g * 4 + c] + gumbel_of(x[c]);
                        if (better(s, 4 * q + c, bv, bi)) { bv = s; bi = 4 * q + c; }
                    }
            }
        } else
#pragma unroll
        for (int g = 0; g < SG; ++g) {
            const int q = g * ST + tid;
            bool any = false;
#pragma unroll
            for (int c = 0; c < 4; ++c) any |= (4 * q + c < V) && fkey(z[g * 4 + c]) >= thr;
            if (!any) continue;
            uint32_t x[4] = {(uint32_t)q, (uint32_t)step, sub, 0u};
            philox4x32_10(x, k0, k1);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = 4 * q + c;
                if (i < V && fkey(z[g * 4 + c]) >= thr) {
                    const float s = z[g * 4 + c] + gumbel_of(x[c]);
                    if (better(s, i, bv, bi)) { bv = s; bi = i; }
                }
            }
        }
    }
    const int tok = block_argmax(bv, bi, sh, lane, wave);
    if constexpr (PROC) {   // HF scores (the processed row; z / T on the kept set and -inf off it when sampling) and logits at index step
        if (p.score_words) {
            float* sc = (float*)p.score_words[0];
            float* lg = (float*)p.score_words[1];
            const int t_max = (int)p.score_words[2], rows = (int)p.score_words[3], r = p.row0 + b;
            if (step < t_max && r < rows) {
                const size_t off = ((size_t)step * rows + r) * V;
                if (sc) {
                    if (T > 0.f && !dead)
#pragma unroll
                        for (int j = 0; j < SG * 4; ++j) z[j] = (EXT ? ((km >> j) & 1u) != 0 : fkey(z[j]) >= kept) ? z[j] : -INFINITY;
                    store_row(sc + off, z, tid, V);
                }
                if (lg)
                    for (int i = tid; i < V; i += ST) lg[off + i] = row[i];
            }
        }
    }
    if constexpr (EXT) {
        if (p.scores_out) {   // (the op form) the row's scores, as the scores store above
            if (T > 0.f && !dead)
#pragma unroll
                for (int j = 0; j < SG * 4; ++j) z[j] = ((km >> j) & 1u) ? z[j] : -INFINITY;
            store_row(p.scores_out + (size_t)b * V, z, tid, V);
        }
    }
    if (tid == 0) {
        // (an all-NaN row keeps no entry: the token is -1, its log-probability NaN.  In a step -1 never reaches cur_tok, whose row the next
        // step's embedding gather reads: the row emits pad and is done)
        const bool ok = tok >= 0 && tok < V;
        const float lp = ok ? row[tok] - lse : __int_as_float(0x7fc00000);
        if constexpr (EXT) {
            if (p.tok_out) {   // the op form: no row state
                p.tok_out[b] = ok ? tok : dead ? p.f.pad_id : -1;
                p.logprob_out[b] = lp;
            } else {
                emmax_finish_row(p.f, b, ok ? tok : p.f.pad_id, p.logprob + (size_t)b * p.f.max_out, lp, !ok);
            }
        } else if constexpr (FIN) {
            emmax_finish_row(p.f, b, ok ? tok : p.f.pad_id, p.logprob + (size_t)b * p.f.max_out, lp, !ok);
        } else {
            p.tok_out[b] = ok ? tok : -1;
            p.logprob_out[b] = lp;
        }
    }
}

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
