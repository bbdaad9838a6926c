"""Host reference of the seeded sampler (include/emmax.h, emma-x_amd/csrc/sample.hip): numpy Philox4x32-10 and the kept-set / draw /
log-probability rules.  z = l / T is formed in float32 (the device's correctly rounded division, so the top-k set is the device's);
everything after it -- the top-p integer masses, the Gumbel noise, the scores, the log-softmax -- in float64."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32-valued array [..., 4]; key: (k0, k1) ints or arrays broadcastable to ctr[..., 0].  Returns uint32 [..., 4]."""
    c = [np.asarray(ctr[..., j], dtype=np.uint64) for j in range(4)]
    k0 = np.asarray(key[0], dtype=np.uint64) & MASK32
    k1 = np.asarray(key[1], dtype=np.uint64) & MASK32
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & MASK32
            k1 = (k1 + np.uint64(W1)) & MASK32
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack([x.astype(np.uint32) for x in c], axis=-1)


def noise_words(V, seed, step, subseq):
    """x_i for i < V: word i % 4 of Philox4x32-10(counter (i / 4, step, subseq, 0), key (seed lo, seed hi))."""
    q = np.arange((V + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q, np.full_like(q, step), np.full_like(q, subseq), np.zeros_like(q)], axis=-1)
    out = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    return out.reshape(-1)[:V]


def gumbel(x):
    u = ((x.astype(np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def kept_set(l, T, k, p):
    """Boolean mask of rules 2-4 over one fp32 logit row (T > 0); also returns z (float32) and the top-p slack (relative distance of
    the boundary entry's mass-above to top_p * total, inf when top-p is off)."""
    l = np.asarray(l, dtype=np.float32)
    V = l.shape[0]
    z = (l / np.float32(T)).astype(np.float32)
    keep = np.ones(V, dtype=bool)
    if 0 < k < V:
        kth = np.sort(z)[::-1][k - 1]
        keep = z >= kth
    slack = np.inf
    if np.float32(p) < 1:
        zmax = np.float64(z.max())
        W = np.where(keep, np.floor(np.exp(z.astype(np.float64) - zmax) * 2.0 ** 32), 0).astype(np.uint64)
        P = float(np.float32(p)) * float(int(W.sum()))
        order = np.argsort(-z.astype(np.float64), kind="stable")
        zs = z[order]
        Ws = W[order]
        cum = np.cumsum(Ws)                       # inclusive, descending z
        # mass strictly above each entry: the cumulative sum before the first entry of its value
        first = np.searchsorted(-zs, -zs, side="left")
        above = np.where(first > 0, cum[np.maximum(first - 1, 0)], 0).astype(np.float64)
        keep_s = (above == 0) | (above < P)
        kp = np.zeros(V, dtype=bool)
        kp[order] = keep_s
        keep = keep & kp
        tot = float(int(W.sum()))
        slack = float(np.min(np.abs(above - P)) / tot) if tot > 0 else np.inf
    return keep, z, slack


def sample_row(l, T, k, p, seed, subseq, step):
    """(token, log-probability, margin) of one row: margin = top-2 gap of the perturbed scores over the kept set (inf when greedy or
    one entry is kept)."""
    l = np.asarray(l, dtype=np.float32)
    V = l.shape[0]
    l64 = l.astype(np.float64)
    m = l64.max()
    lse = m + np.log(np.exp(l64 - m).sum())
    if not T > 0:
        tok = int(np.argmax(l))
        return tok, float(l64[tok] - lse), np.inf
    keep, z, _ = kept_set(l, T, k, p)
    g = gumbel(noise_words(V, seed, step, subseq))
    s = np.where(keep, z.astype(np.float64) + g, -np.inf)
    tok = int(np.argmax(s))
    top2 = np.sort(s[keep])[-2:] if keep.sum() > 1 else None
    margin = float(top2[1] - top2[0]) if top2 is not None else np.inf
    return tok, float(l64[tok] - lse), margin
