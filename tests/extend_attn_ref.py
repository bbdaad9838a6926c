"""References, inputs and tolerances of tests/test_extend_attn_gpu.py.  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

The extension attention (emma-x_amd/csrc/extend_attn.hip) computes, for every sequence b of a launch, the causal attention of n[b] NEW query rows
over a paged cache that already holds base[b] + n[b] keys: row i sees keys 0 .. base[b] + i.  This module holds

  * the CASE BUILDER: packed q rows, the sequences' keys and values, and a paged cache (bf16, or e4m3 + a power-of-two scale per row) with a random
    non-identity table in which every page no sequence references and every position past base + n holds NaN (bf16 NaN; e4m3 0x7F with a NaN
    scale).  Unused table entries are valid ids of NaN pages: a wrong lookup shows as a wrong VALUE, never as a fault;
  * ref64: float64 softmax(q k^T / sqrt(128)) v over each new row's own keys (fp8: over the de-quantised values), and the row's log-sum-exp;
  * emu32: the kernel's documented roundings in torch fp32, in an order of its own: fp32 scores; an online softmax over chunks of 32 keys counted
    from the split's first key (the kernel walks pages of 64); p = 2^(fl(s c - m c)) with c = fl(scale log2 e); the row sum from the fp32 p, the
    value product from p ROUNDED TO bf16 (the second MFMA's operand) accumulated in fp32; an fp32 merge of the splits by the decode attention's rule
    (kps = ceil(L / nsplit) rounded up to 16, L = base + n; empty splits allowed); ONE bf16 rounding of the finished row;
  * the CASES (each launch tagged with the plan it must reach: tests/test_extend_attn_ref.py proves the tags cover every plan emmax_extend_attn_plan
    can return) and the tolerance table SPREAD, measured here as |emu32 - ref64| and pinned by tests/test_extend_attn_ref.py.
    `python tests/extend_attn_ref.py` prints the measurement.

Error measures (o, spread, po per packed row -- all heads of one token, which attends over its own keys and has its own scale -- worst row of a
launch; rel per sequence):
  o      the bf16 rows: max |got - ref| / rms(ref)          rel    max |got - ref| / max |ref|  (the project's relerr)
  spread the smallest atol fraction at which assert_elementwise (rtol 1e-2) passes on the row
  po     the split form's fp32 partials merged in float64, as o          plse   their log-sum-exp, |got - ref| / max(1, |ref|)
Bound = 2 x SPREAD (the device's v_exp_f32, its MFMA summation order and its reference maxima are not reproduced).  The bf16 rows have the project's
floor on top: rtol 1e-2, atol 4e-3 rms(ref) (test_ops_gpu.assert_elementwise) and relerr < 8e-3.  The fp32 partials have none.
"""

import math

import torch

from decode_attn_ref import BF16_ATOL, BF16_REL, FACTOR, HD, HEADS, NAN, PAGE, PSTRIDE, SCALE, bf, err_o, err_rel, quant_rows_e4m3, spread_bf16

LOG2E = 1.4426950408889634
C32 = torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)   # the kernel's c = fl(scale x log2 e)
KINDS = ("bf16", "fp8")
NSPLITS = (1, 2, 3, 0)   # forced, and 0 = the planner's own choice
# (base, n) at the loop edges -- tiles are pages of 64 keys, a wave owns 32 query rows, a block 128 / G tokens:
#   base 0 = a plain causal prefill; (0, 1) / (0, 2): one or two keys, every split but the first left EMPTY; n < 32: waves without rows
#   first page partial: base 1, 63, 65, 127, 200;  last page partial / complete: base + n = 64, 128, 129, 329
#   diagonal inside a page: (1, 31), (65, 33), (200, 31);  on a page edge: (63, 1), (63, 2), (64, 1), (127, 2), (128, 1)
#   n = 32 / 33 / 63 / 64 / 65 / 129: a wave's and a block's last row, one row past it;  (1025, 3): a long prefix, 17 pages
EDGE = ((0, 1), (0, 2), (0, 65), (0, 129), (1, 31), (1, 63), (63, 1), (63, 2), (63, 65), (64, 1), (64, 64), (65, 33), (65, 63), (127, 2), (127, 33), (128, 1),
        (128, 32), (200, 31), (200, 129), (1025, 3))
RAGGED = ((63, 33), (200, 2), (0, 65))   # B = 3, three different (base, n)
MAX_PAGES = 19   # ceil(1028 / 64) = 17 used


class Case:
    """Host tensors of one launch: packed q, per-sequence K / V (what the REFERENCE attends over: kd / vd, de-quantised), cache planes, table"""


def build(kind, G, pairs, seed, max_pages=MAX_PAGES):
    Hq, Hkv = HEADS[G]
    c = Case()
    c.kind, c.G, c.Hq, c.Hkv, c.pairs, c.max_pages = kind, G, Hq, Hkv, tuple(pairs), max_pages
    B = c.B = len(pairs)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: bf(torch.randn(*s, generator=g))
    vary = (lambda n: 0.5 + 2.0 * torch.rand(n, Hkv, 1, generator=g)) if kind == "fp8" else (lambda n: 1.0)   # fp8: the row scales vary
    c.base = [p[0] for p in pairs]
    c.n = [p[1] for p in pairs]
    c.cu = [0]
    for n in c.n:
        c.cu.append(c.cu[-1] + n)
    c.total = c.cu[-1]
    c.q = rnd(c.total, Hq, HD)
    K = [bf(rnd(b + n, Hkv, HD) * vary(b + n)) for b, n in pairs]
    V = [bf(rnd(b + n, Hkv, HD) * vary(b + n)) for b, n in pairs]
    assert all(b + n <= max_pages * PAGE for b, n in pairs)
    n_pages = c.n_pages = B * max_pages
    c.table = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed + 7919)).view(B, max_pages).to(torch.int32)
    shape = (n_pages, Hkv, PAGE, HD)
    if kind == "fp8":
        K8, KS, KD = zip(*[quant_rows_e4m3(k) for k in K])
        V8, VS, VD = zip(*[quant_rows_e4m3(v) for v in V])
        c.kd, c.vd = list(KD), list(VD)
        c.kc, c.vc = torch.full(shape, 0x7F, dtype=torch.uint8), torch.full(shape, 0x7F, dtype=torch.uint8)   # e4m3 NaN
        c.ks, c.vs = torch.full(shape[:3], NAN), torch.full(shape[:3], NAN)
        src = [(c.kc, K8), (c.vc, V8), (c.ks, KS), (c.vs, VS)]
    else:
        c.kd, c.vd = K, V
        c.kc, c.vc = torch.full(shape, NAN).to(torch.bfloat16), torch.full(shape, NAN).to(torch.bfloat16)
        src = [(c.kc, [k.to(torch.bfloat16) for k in K]), (c.vc, [v.to(torch.bfloat16) for v in V])]
    for b in range(B):
        L = c.base[b] + c.n[b]
        for t0 in range(0, L, PAGE):
            pg, n = int(c.table[b, t0 // PAGE]), min(PAGE, L - t0)
            for dst, rows in src:
                dst[pg, :, :n] = rows[b][t0:t0 + n].transpose(0, 1)
    return c


def edge_case(kind, G):
    return build(kind, G, EDGE + RAGGED, 9000 + 100 * KINDS.index(kind) + G)


def ragged_case(kind, G):
    return build(kind, G, RAGGED, 9500 + 100 * KINDS.index(kind) + G, max_pages=5)


# ---- float64 reference -----------------------------------------------------------------------------------------------------------------------
def split_range(L, nsplit, s):
    kps = (-(-L // nsplit) + 15) & ~15
    return s * kps, min(L, (s + 1) * kps)


def _scores(c, b, dtype):
    """scaled-free scores [n, Hq, L] and values [L, Hq, 128] of sequence b, and the causal mask [n, L]"""
    rep = c.Hq // c.Hkv
    kk, vv = c.kd[b].to(dtype).repeat_interleave(rep, dim=1), c.vd[b].to(dtype).repeat_interleave(rep, dim=1)
    q = c.q[c.cu[b]:c.cu[b + 1]].to(dtype)
    s = torch.einsum("nhd,lhd->nhl", q, kk)
    L = c.base[b] + c.n[b]
    vis = torch.arange(L)[None, :] <= (c.base[b] + torch.arange(c.n[b]))[:, None]
    return s, vv, vis


def ref64(c):
    """(o [total, Hq, 128], lse [total, Hq]) in float64"""
    o = torch.zeros(c.total, c.Hq, HD, dtype=torch.float64)
    lse = torch.zeros(c.total, c.Hq, dtype=torch.float64)
    for b in range(c.B):
        s, vv, vis = _scores(c, b, torch.float64)
        s = (s * SCALE).masked_fill(~vis[:, None, :], -math.inf)
        o[c.cu[b]:c.cu[b + 1]] = torch.einsum("nhl,lhd->nhd", torch.softmax(s, dim=-1), vv)
        lse[c.cu[b]:c.cu[b + 1]] = torch.logsumexp(s, dim=-1)
    return o, lse


# ---- fp32 emulation --------------------------------------------------------------------------------------------------------------------------
def _split32(s, vv, vis, k0, k1, chunk=32):
    """online softmax of one split in fp32: s [n, H, L] raw scores, vis [n, L].  Returns (o [n, H, 128] un-normalised, m [n, H] in raw-score
    units (-inf: the row saw no key), l [n, H])"""
    n, H, _ = s.shape
    m = torch.full((n, H), -math.inf)
    l = torch.zeros(n, H)
    o = torch.zeros(n, H, HD)
    for a in range(k0, k1, chunk):
        e = min(k1, a + chunk)
        sc = s[:, :, a:e].masked_fill(~vis[:, None, a:e], -math.inf)
        mn = torch.maximum(m, sc.max(dim=-1).values)
        ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
        alpha = torch.exp2(((m - ms) * C32).float())
        p = torch.exp2((sc * C32 - (ms * C32)[..., None]).float())
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + torch.einsum("nhl,lhd->nhd", bf(p), vv[a:e])
        m = mn
    return o, m, l


def emu32(c, nsplit):
    """dict(o = bf16 rows as fp32 [total, Hq, 128], po / plse = the merged fp32 partials before the bf16 rounding and their log-sum-exp)"""
    out = dict(o=torch.zeros(c.total, c.Hq, HD), po=torch.zeros(c.total, c.Hq, HD), plse=torch.zeros(c.total, c.Hq))
    for b in range(c.B):
        s, vv, vis = _scores(c, b, torch.float32)
        L = c.base[b] + c.n[b]
        parts = []
        for sp in range(nsplit):
            k0, k1 = split_range(L, nsplit, sp)
            if k0 < k1:
                parts.append(_split32(s, vv, vis, k0, k1))
        m = torch.stack([p[1] for p in parts]) * SCALE                       # [ns, n, H] in the units of the scaled scores
        M = m.max(dim=0).values
        w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp((m - M).float()))
        oo, ll = torch.zeros_like(parts[0][0]), torch.zeros_like(parts[0][2])
        for i, p in enumerate(parts):
            oo = oo + p[0] * w[i][..., None]
            ll = ll + p[2] * w[i]
        row = oo * (1.0 / ll)[..., None]
        r = slice(c.cu[b], c.cu[b + 1])
        out["po"][r], out["plse"][r], out["o"][r] = row, M + torch.log(ll), bf(row)
    return out


def merge_partials(part):
    """f32 [total, Hq, nsplit, 132] -> (merged o [total, Hq, 128], lse [total, Hq]) in float64"""
    p = part.double()
    o, m, l = p[..., :HD], p[..., HD], p[..., HD + 1]
    M = m.max(dim=-1, keepdim=True).values
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - M))
    den = (l * w).sum(-1)
    return (o * w[..., None]).sum(-2) / den[..., None], M.squeeze(-1) + torch.log(den)


# ---- error measures --------------------------------------------------------------------------------------------------------------------------
def errors(c, got, ref, split):
    """got: dict(o [total, Hq, 128]) (+ po, plse with split).  Every measure per sequence (its rows: one block of numbers), worst sequence"""
    ro, rl = ref
    rms = ro.pow(2).mean(dim=(1, 2)).sqrt()                                          # per packed row (a row attends over its own keys: its own scale)
    d = (got["o"].double() - ro).abs()
    e = dict(o=(d.amax(dim=(1, 2)) / rms).max().item(),
             spread=max(0.0, ((d - 1e-2 * ro.abs()).amax(dim=(1, 2)) / rms).max().item()),
             rel=max(err_rel(got["o"][c.cu[b]:c.cu[b + 1]], ro[c.cu[b]:c.cu[b + 1]]) for b in range(c.B)))   # the project's relerr, per sequence
    if split:
        e["po"] = ((got["po"].double() - ro).abs().amax(dim=(1, 2)) / rms).max().item()
        e["plse"] = ((got["plse"].double() - rl).abs() / rl.abs().clamp_min(1.0)).max().item()
    return e


# ---- plans -----------------------------------------------------------------------------------------------------------------------------------
def plan_tag(G, kv8, split):
    """the instantiation a launch takes: (GQA group, e4m3 cache, split form) -- tokens per block and the grid follow from G and the lengths"""
    return ("extend", G, 1 if kv8 else 0, 1 if split else 0)


def expected_nsplit(B, max_n, max_L, Hq, Hkv, nsplit):
    """the planner's rule (extend_attn.hip: extend_attn_plan), restated: items = B x Hkv x query tiles; one split once they fill 256 CUs"""
    if nsplit:
        return nsplit
    qt = 128 // (Hq // Hkv)
    items = B * Hkv * -(-max_n // qt)
    if items >= 256:
        return 1
    return max(1, min(-(-256 // items), -(-max_L // 64), 16))


def case_plans():
    """every plan tag some GPU case asserts before it launches"""
    tags = set()
    pairs = EDGE + RAGGED
    for kind in KINDS:
        for G in HEADS:
            for ns in NSPLITS:
                n = expected_nsplit(len(pairs), max(p[1] for p in pairs), max(p[0] + p[1] for p in pairs), *HEADS[G], ns)
                tags.add(plan_tag(G, kind == "fp8", n > 1))
    return tags


# ---- the tolerance table ---------------------------------------------------------------------------------------------------------------------
# SPREAD[kind][form] = {measure: worst |emu32 - ref64|} over the edge launch of every G and split count ("split": 2 and 3 splits and the planner's;
# "direct": one split).  Measured on the CPU by measure() -- no GPU output involved.
SPREAD = {
    "bf16": {"split": {"o": 0.0198, "plse": 2.46e-07, "po": 0.00913, "rel": 0.00378, "spread": 0.00766}, "direct": {"o": 0.0181, "rel": 0.00387, "spread": 0.00766}},
    "fp8": {"split": {"o": 0.0274, "plse": 1.69e-07, "po": 0.0132, "rel": 0.0033, "spread": 0.00544}, "direct": {"o": 0.0274, "rel": 0.0033, "spread": 0.00574}},
}


def tolerances(kind, split):
    b = {k: FACTOR * v for k, v in SPREAD[kind]["split" if split else "direct"].items()}
    b["spread"] = max(BF16_ATOL, b["spread"])   # a bf16 row: never below the project's line
    b["rel"] = max(BF16_REL, b["rel"])
    return b


def measure(kind):
    out = {"split": {}, "direct": {}}
    for G in HEADS:
        c = edge_case(kind, G)
        ref = ref64(c)
        seen = set()
        for ns in NSPLITS:
            n = expected_nsplit(c.B, max(c.n), max(b + x for b, x in c.pairs), c.Hq, c.Hkv, ns)
            if n in seen:
                continue
            seen.add(n)
            e = errors(c, emu32(c, n), ref, n > 1)
            into = out["split" if n > 1 else "direct"]
            for k, v in e.items():
                into[k] = max(into.get(k, 0.0), v)
    return out


def _fmt(d):
    return "{" + ", ".join(f'"{k}": {v:.3g}' for k, v in sorted(d.items())) + "}"


if __name__ == "__main__":
    print("SPREAD = {")
    for kind in KINDS:
        r = measure(kind)
        print(f'    "{kind}": {{"split": {_fmt(r["split"])}, "direct": {_fmt(r["direct"])}}},')
    print("}")
