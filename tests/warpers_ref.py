"""Host reference of the EXT finish (include/emmax.h: emmax_session_set_warpers / emmax_session_set_token_rules / emmax_op_sample_ext; the
kernel: emma-x_amd/csrc/sample.hip): a numpy replay of the documented arithmetic of min_p / typical_p / epsilon_cutoff / eta_cutoff behind
sampling_ref.kept_set, and of the token rules around processing_ref.process_row.

The warpers' decisions are threshold comparisons, so a row is only a fair test where its nearest entry clears the threshold by more than
the arithmetic's own error.  kept_set_ext therefore returns, per decision, the SLACK of the row (the distance of the nearest entry to the
threshold) and the decision QUANTITIES themselves; it runs either as an fp32 emulation of the pinned device arithmetic (emulate=True: fp32
exp / log, the device's reduction order for the entropy) or in float64 with HF's formulas (emulate=False).  LINE_* are twice the worst
difference between the two, per decision quantity, measured on the committed rows (tests/test_warpers.py re-measures them); every committed
row clears every line, so no row is skipped anywhere."""
import numpy as np

import processing_ref
import sampling_ref

ST, WAVE, LANE_ENTRIES = 1024, 64, 32   # sample.hip: threads per row, lanes per wave, entries per lane (V <= 32768)

# twice the worst |fp32 emulation - float64| per decision quantity over ROWS x CASES below (measure_lines; test_warpers re-measures)
# (measured worst: 2.2e-7, 6.9e-7, 4.7e-6, 2.2e-7, 3.9e-6)
LINE_MIN_P = 5e-7      # relative, W_i / (min_p 2^32) within a factor 2 of the threshold
LINE_EPSILON = 1.5e-6  # relative, p_i / epsilon likewise
LINE_ETA = 1e-5        # relative, p_i / eta' likewise (eta' carries the entropy's error)
LINE_TYP_CUM = 5e-7    # absolute, cumulative probability in ascending distance
LINE_TYP_DIST = 8e-6   # absolute, the distance |(-log p_i) - H|
MARGIN = 1e-4          # the Gumbel top-2 gap a row's draw must clear (tests/test_sampling_gpu.py's)

# the committed rows: logits N(0, 2.5^2), one seed per row; CASES = (T, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff)
V_BIG, V_SMALL = 32064, 37
ROW_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
CASES = (
    (1.0, 0, 1.0, 0.05, 0.0, 0.0, 0.0),      # each warper alone
    (1.0, 0, 1.0, 0.2, 0.0, 0.0, 0.0),
    (1.0, 0, 1.0, 0.0, 0.2, 0.0, 0.0),
    (1.0, 0, 1.0, 0.0, 0.9, 0.0, 0.0),
    (1.0, 0, 1.0, 0.0, 0.0, 3e-4, 0.0),
    (1.0, 0, 1.0, 0.0, 0.0, 1e-3, 0.0),
    (1.0, 0, 1.0, 0.0, 0.0, 0.0, 3e-4),
    (1.0, 0, 1.0, 0.0, 0.0, 0.0, 1e-3),
    (0.8, 50, 0.9, 0.05, 0.9, 3e-4, 1e-3),   # all of them chained behind top-k 50 / top-p 0.9
    (1.3, 50, 0.9, 0.2, 0.2, 1e-3, 3e-4),
)


def logits_row(seed, V):
    return (np.random.default_rng(seed).standard_normal(V) * 2.5).astype(np.float32)


def _lane_sum32(vals, mask):
    """The device's fp32 block sum of vals over mask (arrays over ids): a lane's entries in register order (id 4 ((j / 4) 1024 + tid) + j % 4),
    the xor butterfly 32..1 inside each wave, then the 16 wave results in order."""
    V = vals.shape[0]
    full = np.zeros(ST * LANE_ENTRIES, dtype=np.float32)
    full[:V] = np.where(mask, vals, np.float32(0)).astype(np.float32)
    lanes = full.reshape(LANE_ENTRIES // 4, ST, 4).transpose(1, 0, 2).reshape(ST, LANE_ENTRIES)   # [tid][j]
    acc = np.zeros(ST, dtype=np.float32)
    for j in range(LANE_ENTRIES):
        acc = (acc + lanes[:, j]).astype(np.float32)   # (an entry off the mask adds 0: the sum's bits do not move)
    idx = np.arange(ST)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[idx ^ o]).astype(np.float32)
    r = np.float32(acc[0])
    for w in range(1, ST // WAVE):
        r = np.float32(r + acc[w * WAVE])
    return r


class _Arith:
    """The two arithmetics of the warpers: the device's (fp32 exp / log, integer masses, fixed-order fp32 entropy) and float64 with HF's formulas."""

    def __init__(self, z, zmax, emulate):
        self.z, self.emulate = z, emulate
        if emulate:
            e = np.exp((z - np.float32(zmax)).astype(np.float32)).astype(np.float32)
            self.W = np.floor(e.astype(np.float64) * 2.0 ** 32)                      # integer masses (exact in float64: < 2^53)
        else:
            self.W = np.exp(z.astype(np.float64) - np.float64(zmax)) * 2.0 ** 32     # unrounded
        self.d = z.astype(np.float64) - np.float64(zmax) if not emulate else (z - np.float32(zmax)).astype(np.float32)

    def total(self, keep):
        return float(self.W[keep].sum())   # (the emulation's is an exact integer sum)

    def logp_entropy(self, keep):
        """(lp_i, H) over the kept set."""
        S = self.total(keep)
        if self.emulate:
            S32 = np.float32(S)
            lnZ = np.float32(np.log(np.float32(S32 * np.float32(2.0 ** -32))))
            inv = np.float32(np.float32(1) / S32)
            lp = (self.d - lnZ).astype(np.float32)
            p = (self.W.astype(np.float32) * inv).astype(np.float32)
            with np.errstate(invalid="ignore"):
                term = (p * lp).astype(np.float32)
            return lp, np.float32(-_lane_sum32(term, keep))
        lp = self.d - np.log(S * 2.0 ** -32)
        p = self.W / S
        return lp, float(-(p[keep] * lp[keep]).sum())


def kept_set_ext(l, T, k, p, min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, emulate=True):
    """Kept mask of one fp32 logit row (T > 0) after top-k / top-p (sampling_ref.kept_set) and the four warpers in HF's order (0 = off).
    Returns (keep, z, info): info[name] = {"slack": ..., "q": {...}} per active decision -- min_p / epsilon / eta: slack = the smallest
    |q_i - 1| with q_i = mass over threshold (relative); typical: "slack" = the smallest distance of a cumulative-mass boundary to typical_p
    (absolute, in probability) and "gap" = the distance gap between the last kept and the first dropped entry."""
    keep, z, tp_slack = sampling_ref.kept_set(l, T, k, p)
    keep = keep & (z > -np.inf)   # (NaN and -inf entries are never kept)
    info = {"top_p": {"slack": tp_slack}}
    if not keep.any():
        return keep, z, info
    zmax = z[keep].max()
    A = _Arith(z, zmax, emulate)
    ids = np.arange(z.shape[0])
    if min_p > 0:
        thr = np.floor(float(np.float32(min_p)) * 2.0 ** 32) if emulate else float(min_p) * 2.0 ** 32
        q = A.W / thr
        info["min_p"] = {"slack": float(np.abs(q[keep] - 1).min()), "q": np.where(keep, q, np.nan)}
        keep = keep & (A.W >= thr)
    if 0 < typical_p < 1:
        S = A.total(keep)
        lp, H = A.logp_entropy(keep)
        dist = np.abs((-lp) - H)
        if emulate:
            dist = dist.astype(np.float32)
        target = float(np.float32(typical_p)) * S if emulate else float(typical_p) * S
        kid = ids[keep]
        order = kid[np.argsort(dist[kid].astype(np.float64), kind="stable")]
        ds, Ws = dist[order].astype(np.float64), A.W[order]
        cum = np.cumsum(Ws)
        first = np.searchsorted(ds, ds, side="left")                 # the first entry of each tie group
        before = np.where(first > 0, cum[np.maximum(first - 1, 0)], 0.0)
        ok = (before == 0) | (before < target)
        kp = np.zeros_like(keep)
        kp[order] = ok
        nk = int(ok.sum())
        gap = float(ds[nk] - ds[nk - 1]) if nk < len(ds) else np.inf
        bounds = np.concatenate([before, cum]) / S
        info["typical"] = {"slack": float(np.abs(bounds - (target / S)).min()), "gap": gap,
                           "q": {"dist": np.where(keep, dist.astype(np.float64), np.nan), "p": np.where(keep, A.W / S, np.nan), "H": float(H)}}
        keep = keep & kp
    for name, cut in (("epsilon", epsilon_cutoff), ("eta", eta_cutoff)):
        if not 0 < cut < 1:
            continue
        S = A.total(keep)
        if S == 0:
            break
        cmax = z[keep].max()
        c = np.float32(cut) if emulate else float(cut)
        if name == "eta":
            _, H = A.logp_entropy(keep)
            if emulate:
                c = np.float32(min(np.float32(cut), np.float32(np.sqrt(np.float32(cut)) * np.float32(np.exp(np.float32(-H))))))
            else:
                c = min(float(cut), float(np.sqrt(cut) * np.exp(-H)))
        line = float(c) * S
        q = A.W / line
        others = keep & (z < cmax)   # (the largest kept z stays whatever its mass)
        info[name] = {"slack": float(np.abs(q[others] - 1).min()) if others.any() else np.inf, "q": np.where(keep, q, np.nan), "cut": float(c)}
        keep = keep & ((A.W >= line) | (z >= cmax))
    return keep, z, info


def clears(info):
    """Every decision of a row clears its line."""
    ok = info.get("top_p", {}).get("slack", np.inf) > 1e-6   # (tests/test_sampling_gpu.py's line for the top-p walk)
    ok &= info.get("min_p", {}).get("slack", np.inf) > LINE_MIN_P
    ok &= info.get("epsilon", {}).get("slack", np.inf) > LINE_EPSILON
    ok &= info.get("eta", {}).get("slack", np.inf) > LINE_ETA
    ok &= info.get("typical", {}).get("slack", np.inf) > LINE_TYP_CUM and info.get("typical", {}).get("gap", np.inf) > LINE_TYP_DIST
    return bool(ok)


def _near(qe, q64):
    """Worst relative difference of the ratios q over the entries within a factor 2 of the threshold (far entries decide nothing; the masses
    of the far tail are a few integer units, whose relative rounding says nothing about the comparison)."""
    with np.errstate(invalid="ignore"):
        near = (q64 > 0.5) & (q64 < 2.0) & np.isfinite(qe)
    return float(np.abs(qe[near] / q64[near] - 1.0).max()) if near.any() else 0.0


def measure_lines(rows):
    """Worst |fp32 emulation - float64| per decision quantity over rows = [(logits, case)]: {"min_p", "epsilon", "eta", "typ_cum", "typ_dist"}."""
    worst = {"min_p": 0.0, "epsilon": 0.0, "eta": 0.0, "typ_cum": 0.0, "typ_dist": 0.0}
    for l, (T, k, p, mp, ty, ep, et) in rows:
        _, _, ie = kept_set_ext(l, T, k, p, mp, ty, ep, et, emulate=True)
        _, _, i64 = kept_set_ext(l, T, k, p, mp, ty, ep, et, emulate=False)
        for name in ("min_p", "epsilon", "eta"):
            if name in ie and name in i64:
                worst[name] = max(worst[name], _near(ie[name]["q"], i64[name]["q"]))
        if "typical" in ie and "typical" in i64:
            de, d64 = ie["typical"]["q"]["dist"], i64["typical"]["q"]["dist"]
            both = np.isfinite(de) & np.isfinite(d64)
            worst["typ_dist"] = max(worst["typ_dist"], float(np.abs(de[both] - d64[both]).max()))
            # cumulative probability in the float64 order, with either arithmetic's masses: the order is the distance's business
            order = np.flatnonzero(both)[np.argsort(d64[both], kind="stable")]
            ce, c64 = np.cumsum(ie["typical"]["q"]["p"][order]), np.cumsum(i64["typical"]["q"]["p"][order])
            worst["typ_cum"] = max(worst["typ_cum"], float(np.abs(ce - c64).max()))
    return worst


def committed_rows():
    """[(row seed, V, logits, case)] of the committed grid: every ROW_SEEDS row of both sizes with every CASE whose index has its parity, so a
    batch of 8 rows carries 8 different parameter sets (ragged parameters per row)."""
    out = []
    for V in (V_BIG, V_SMALL):
        for r, seed in enumerate(ROW_SEEDS):
            l = logits_row(seed, V)
            for c in range(r % 2, len(CASES), 2):
                out.append((seed, V, l, CASES[c]))
    return out


def sample_row_ext(l, case, seed, subseq, step):
    """(token, log-probability, margin, keep, scores) of one row: sampling_ref.sample_row's draw over kept_set_ext's kept set."""
    T, k, p, mp, ty, ep, et = case
    l = np.asarray(l, dtype=np.float32)
    V = l.shape[0]
    l64 = l.astype(np.float64)
    m = l64.max()
    lse = m + np.log(np.exp(l64 - m).sum())
    if not T > 0:
        tok = int(np.argmax(l))
        return tok, float(l64[tok] - lse), np.inf, None, l.copy()
    keep, z, _ = kept_set_ext(l, T, k, p, mp, ty, ep, et)
    g = sampling_ref.gumbel(sampling_ref.noise_words(V, seed, step, subseq))
    s = np.where(keep, z.astype(np.float64) + g, -np.inf)
    tok = int(np.argmax(s))
    top2 = np.sort(s[keep])[-2:] if keep.sum() > 1 else None
    margin = float(top2[1] - top2[0]) if top2 is not None else np.inf
    return tok, float(l64[tok] - lse), margin, keep, np.where(keep, z, np.float32(-np.inf)).astype(np.float32)


# ---- token rules --------------------------------------------------------------------------------------------------------------------
def fired(rule_ids, hist):
    """A rule of n ids fires when n == 1, or n <= len(hist) and the history ends with its first n - 1 ids."""
    n = len(rule_ids)
    return n == 1 or (n <= len(hist) and [int(x) for x in hist[len(hist) - (n - 1):]] == [int(x) for x in rule_ids[:-1]])


def process_row_ext(logits, hist, n_out, penalty=1.0, ngram=0, min_new=0, eos_id=2, rules=(), enable=15):
    """One fp32 logit row through the token rules and processing_ref.process_row, in HF's order.  rules = [(kind, ids, bias)] in table
    order (emmax.sampling.LogitsProcessing.rules): kind 0 biases are summed per target id in fp32 from 0 in rule order and added once, before
    the repetition penalty; kinds 1-3 are -inf after it (kind 3 only at n_out == 0).  Targets past V are ignored."""
    x = np.array(logits, dtype=np.float32, copy=True)
    V = x.shape[0]
    acc, banned = {}, set()
    for kind, ids, bias in rules:
        if not (enable >> kind) & 1 or (kind == 3 and n_out != 0) or not fired(ids, hist) or not 0 <= ids[-1] < V:
            continue
        if kind == 0:
            acc[ids[-1]] = np.float32(acc.get(ids[-1], np.float32(0)) + np.float32(bias))
        else:
            banned.add(ids[-1])
    for i, b in acc.items():
        x[i] = np.float32(x[i] + b)
    x = processing_ref.process_row(x, hist, n_out, penalty, ngram, min_new, eos_id)
    for i in banned:
        x[i] = -np.inf
    return x
