// sample_kernel.h -- the one kernel body of the sampling finishes (emmax_sample_kernel<P>) and the device helpers it shares with the top-N kernel:
// included by sample.hip (emmax_op_sample, the sampled, processing and EXT finishes, emmax_top_logprobs_kernel) and by sample_con.hip (the
// constrained finish, a translation unit of its own: see there).  Everything here sits in an unnamed namespace: each translation unit
// instantiates the forms it launches and no other.
#pragma once
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
    constexpr bool CON = std::is_same<P, ConFinishParams>::value;
    constexpr bool EXT = std::is_same<P, ExtFinishParams>::value || CON;
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
    if constexpr (!CON) {
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
    } else {
        // the automaton's mask joins the bans (a loop of its own: the other instantiations keep their code): the eight allow words of the
        // row's state are block-uniform, the four class bytes of a lane's group are one dword (byte loads where the group crosses V or the
        // array is not dword-aligned)
        const int st = p.state[b];
        const bool con = st >= 0, known = st >= 0 && st < p.n_states;   // a state the table does not have allows nothing
        uint32_t aw[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) aw[k] = known ? p.allow[(size_t)st * 8 + k] : 0u;
#pragma unroll
        for (int g = 0; g < SG; ++g) {
            const int i0 = (g * ST + tid) * 4;
            uint32_t cw = 0;
            if (con && i0 < V) {
                if (i0 + 3 < V && ((uintptr_t)p.cls & 3) == 0) {
                    cw = *(const uint32_t*)(p.cls + i0);
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (i0 + c < V) cw |= (uint32_t)p.cls[i0 + c] << (8 * c);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = i0 + c;
                if (i >= V) continue;
                float x = z[g * 4 + c];
                if ((pres[i >> 5] >> (i & 31)) & 1u) x = x < 0.f ? x * pen : x / pen;
                if (((ban[i >> 5] >> (i & 31)) & 1u) || i == eos) x = -INFINITY;
                const uint32_t k = (cw >> (8 * c)) & 255u;
                uint32_t w = aw[0];   // (a select chain: aw stays in registers)
#pragma unroll
                for (int q = 1; q < 8; ++q) w = (k >> 5) == (uint32_t)q ? aw[q] : w;
                if (con && !((w >> (k & 31u)) & 1u)) x = -INFINITY;
                z[g * 4 + c] = x;
            }
        }
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
    constexpr bool CON = std::is_same<P, ConFinishParams>::value;   // the EXT finish with the token automaton
    constexpr bool EXT = std::is_same<P, ExtFinishParams>::value || CON;   // the processing finish with the token rules and the further warpers
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
        [[maybe_unused]] bool accept = false;
        if constexpr (CON) {   // the row emits a token (a row that is done, idle or out of budget left above): its state moves on that token
            const int st = p.state[b];
            int ns = st;
            if (ok && st >= 0 && st < p.n_states) {
                const int k = p.cls[tok];
                ns = k < p.next_ld ? (int)p.next[(size_t)st * p.next_ld + k] : -1;
                accept = ns < 0;
                if (accept) ns = -1;
            }
            (p.state_out ? p.state_out : p.state)[b] = ns;
        }
        if constexpr (EXT) {
            if (p.tok_out) {   // the op form: no row state
                p.tok_out[b] = ok ? tok : dead ? p.f.pad_id : -1;
                p.logprob_out[b] = lp;
            } else {
                emmax_finish_row(p.f, b, ok ? tok : p.f.pad_id, p.logprob + (size_t)b * p.f.max_out, lp, !ok || accept);
            }
        } else if constexpr (FIN) {
            emmax_finish_row(p.f, b, ok ? tok : p.f.pad_id, p.logprob + (size_t)b * p.f.max_out, lp, !ok);
        } else {
            p.tok_out[b] = ok ? tok : -1;
            p.logprob_out[b] = lp;
        }
    }
}

}  // namespace
