"""References, inputs and tolerances of tests/test_decode_attn_forms_gpu.py.  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

The decode attention (emma-x_amd/csrc/decode_attn.hip, exact.hip) is launched in many forms: split partials or the finished row, four or eight
waves, two or four chunks of keys in flight, bf16 / fp8 / fp32 / 24-bit caches, the grouped span + tail pair.  This module holds, for all of them,

  * the CASE BUILDER: q, the rows' keys and values, and a paged cache with a random non-identity table in which every page no row references and
    every position past a row's context holds NaN (bf16 NaN; e4m3 0x7F with a NaN scale -- including position ctx, which the launch appends; fp32
    NaN).  Unused table entries are valid ids of NaN pages: a wrong lookup shows as a wrong VALUE, never as a fault;
  * ref64 / ref_partials64: float64 softmax(q k^T / sqrt(128)) v over each row's own keys 0 .. ctx (fp8 / 24-bit: over the de-quantised values),
    whole and per split [k0, k1) by the kernel's documented rule (kps = ceil(L / nsplit) rounded up to 16, k0 = split * kps);
  * emu32: the documented roundings in torch fp32, in a summation order of its own (16 interleaved online-softmax states per split, merged
    pairwise): fp32 scores, fp32 softmax through the device's fast exponential 2^(fl(x log2 e)), an fp32 merge of splits / span + tail, ONE bf16
    rounding of a finished row of the default-numerics forms; the fp8 forms see the step's key re-quantised (e4m3 x power-of-two row scale);
  * the INPUT FAMILIES, CASES (each tagged with the launch plan it must reach: tests/test_decode_attn_plan.py proves the tags cover every plan a
    step or a group route can reach) and the tolerance table SPREAD, measured here as |emu32 - ref64| and pinned by
    tests/test_decode_attn_ref.py.  `python tests/decode_attn_ref.py` prints the measurement.

Error measures (one number per output, worst over the rows of a case):
  o    the finished / merged row:  max |got - ref| / rms(ref) over a row's live heads         lse   |lse - ref| / max(1, |ref|),  lse = m + log l
  on   a split's normalised partial o / l, as o, over the non-empty splits                    rel   max |got - ref| / max |ref|  (the project's relerr)
Bound = 2 x SPREAD (the factor of decode_stage_ref.tolerances: the device's v_exp_f32 and its reduction tree are not reproduced).  The bf16-row
outputs (direct, grouped) have the project's floor on top: rtol 1e-2, atol 4e-3 rms(ref) (assert_elementwise) and relerr < 8e-3.  The fp32 outputs
(partials, merged partials, exact rows) have none.
"""

import math

import torch

HD, PAGE, PSTRIDE = 128, 64, 132
SCALE = HD ** -0.5
LOG2E = 1.4426950408889634
NAN = float("nan")
HEADS = {1: (2, 2), 2: (4, 2), 4: (8, 2), 8: (8, 1)}   # GQA group -> (q heads, kv heads): the smallest that reach each instantiation
FAMILIES = ("random", "sink", "last", "one_split", "flat", "low", "offset", "ragged")
KINDS = ("bf16", "fp8", "x32", "x24")
# L = ctx + 1 at every edge of the chunk loops: CHK = 4 NW KU keys per block chunk is 32 (G >= 4), 64 (G <= 2, or eight waves at G >= 4) or 128
# (eight waves at G <= 2); the loop stride is 2 CHK, 4 CHK with four chunks in flight.  {1, 2, 16, 17, CHK - 1, CHK, CHK + 1, 2 CHK +- 1, 4 CHK,
# 4 CHK + 1, 8 CHK + 1} for the three CHK.  With splits: L = 1 leaves every split but the first empty, L = 16 the second of two, L = 17 puts one
# key into it; ctx = 16 / 32 with two splits and ctx = 0 with one are the fp8 corners (a split that holds the new key alone)
EDGE_L = (1, 2, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 1025)
EDGE_CTX = tuple(L - 1 for L in EDGE_L)
RAGGED_CTX = (0, 1, 15, 16, 17, 1024)
MAX_PAGES = 21   # ceil(1025 / 64) = 17 used


def bf(x):
    return x.to(torch.bfloat16).float()


def quant_rows_e4m3(x):
    """[..., 128] -> (e4m3 bytes, fp32 scale per row: the smallest power of two with amax / scale <= 448 (common.h: e4m3_row_scale), bf16(e4m3 x scale))"""
    r = x.abs().amax(dim=-1, keepdim=True).float() / 448.0
    sc = torch.where(r > 0, torch.exp2(torch.ceil(torch.log2(r.clamp_min(1e-38)))), torch.ones_like(r)).float()
    q8 = (x.float() / sc).to(torch.float8_e4m3fn)
    return q8.view(torch.uint8), sc.squeeze(-1), bf(q8.float() * sc)


def x24_planes(t):
    """fp32 -> (bf16 plane = top 16 bits, 8-bit extension plane, the fp32 value they hold) of the value rounded to 24 bits (exact.hip: x24_unpack8)"""
    u = (t.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff) + 0x80
    hi, ext = ((u >> 16) & 0xffff).to(torch.int32), ((u >> 8) & 0xff).to(torch.uint8)
    back = ((hi.to(torch.int64) << 16) | (ext.to(torch.int64) << 8)) & 0xffffffff
    back = torch.where(back >= 2 ** 31, back - 2 ** 32, back).to(torch.int32).view(torch.float32)
    return hi.to(torch.int16), ext, back


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def _plant(q, K, pos, rows, hk, rep, margin):
    """Make key `pos` of kv head hk the dominant one for every (row in rows, q head of hk): K[pos] = 2^e x bf16(mean of those q), the smallest e
    at which it scores >= margin above every other key (a power of two: the operand stays an exact bf16)."""
    qs = torch.stack([q[b, hk * rep + g] for b in rows for g in range(rep)]).double()   # [n, 128]
    u = bf(qs.mean(0).float())
    others = []
    for b in rows:
        k = K[b][:, hk].double()
        s = (torch.stack([q[b, hk * rep + g] for g in range(rep)]).double() @ k.T) * SCALE   # [rep, L]
        s[:, pos] = -1e30
        others.append(s.max(dim=1).values)
    other = torch.cat(others)
    own = (qs @ u.double()) * SCALE
    assert (own > 0).all(), "the queries of a planted key must share a direction"
    for e in range(-6, 24):
        if ((own * 2.0 ** e) - other).min() >= margin:
            break
    else:
        raise AssertionError("no power of two plants the key")
    for b in rows:
        K[b][pos, hk] = u * 2.0 ** e


def make_inputs(kind, family, Hq, Hkv, ctxs, seed, groups=None):
    """q [B, Hq, 128] and per row K, V [ctx + 1, Hkv, 128] (fp32 tensors holding exact bf16 values, unless kind is x32 / x24).
    groups: [(N, shared_pages)] in row order -- the rows of a group hold the same keys in [0, shared_pages * PAGE)."""
    g = torch.Generator().manual_seed(seed)
    B, rep = len(ctxs), Hq // Hkv
    rnd = (lambda *s: torch.randn(*s, generator=g)) if kind in ("x32", "x24") else (lambda *s: bf(torch.randn(*s, generator=g)))
    vary = (lambda n: 0.5 + 2.0 * torch.rand(n, Hkv, 1, generator=g)) if kind == "fp8" else (lambda n: 1.0)   # fp8: the row scales vary
    groups = groups or [(1, 0)] * B
    planted = family in ("sink", "last", "one_split")
    q = rnd(B, Hq, HD)
    if planted:   # the queries that see one planted key share a direction (a group's rows, a kv head's q heads)
        r0 = 0
        for N, _ in groups:
            u = torch.randn(1, Hkv, 1, HD, generator=g)
            n = torch.randn(N, Hkv, rep, HD, generator=g)
            q[r0:r0 + N] = (u + 0.5 * n).view(N, Hq, HD) if kind in ("x32", "x24") else bf((u + 0.5 * n).view(N, Hq, HD))
            r0 += N
    if family == "flat":
        q = torch.zeros(B, Hq, HD)
    K, V, r0 = [], [], 0
    for N, sh in groups:
        n_sh = sh * PAGE
        ks, vs = rnd(n_sh, Hkv, HD) * vary(n_sh), rnd(n_sh, Hkv, HD) * vary(n_sh)
        for j in range(N):
            n = ctxs[r0 + j] + 1 - n_sh
            assert n >= 1, "a group's shared pages are complete in every row"
            K.append(torch.cat([ks, rnd(n, Hkv, HD) * vary(n)]))
            V.append(torch.cat([vs, rnd(n, Hkv, HD) * vary(n)]))
        r0 += N
    if kind == "fp8":
        K, V = [bf(k) for k in K], [bf(v) for v in V]
    if family == "low":   # one coordinate carries -60: 32 x -21.25 / sqrt(128) = -60.1 (both exact in bf16); the other 127 spread the scores by ~1
        q[..., 0] = 32.0
        for k in K:
            k[..., 0] = -21.25
    if family == "offset":   # (bf16 near 1000 has steps of 4)
        V = [v * 8.0 + 1000.0 if kind in ("x32", "x24") else bf(v * 8.0 + 1000.0) for v in V]
    if planted:
        r0 = 0
        for N, sh in groups:
            rows = list(range(r0, r0 + N))
            for hk in range(Hkv):
                if family == "sink":      # key 0 (grouped: inside the shared span, one key for the whole group)
                    if sh:
                        _plant(q, K, 0, rows, hk, rep, 30.0)
                    else:
                        for b in rows:
                            _plant(q, K, 0, [b], hk, rep, 30.0)
                else:
                    for b in rows:   # last: the step's own key; one_split: a key in the middle, 110 above -- exp(-110) is 0 in fp32
                        _plant(q, K, ctxs[b] if family == "last" else ctxs[b] // 2, [b], hk, rep, 30.0 if family == "last" else 110.0)
            r0 += N
        if kind == "fp8":
            K = [bf(k) for k in K]
    return q, K, V


class Case:
    """Host tensors of one launch: q, the per-row K / V (what the REFERENCE attends over: kd / vd, de-quantised), cache planes, table, ctx."""


def build(kind, family, Hq, Hkv, ctxs, seed, groups=None, page=PAGE, max_pages=MAX_PAGES, done=()):
    c = Case()
    c.kind, c.family, c.Hq, c.Hkv, c.ctxs, c.page, c.max_pages, c.done, c.groups = kind, family, Hq, Hkv, list(ctxs), page, max_pages, tuple(done), groups
    B = c.B = len(ctxs)
    assert all(0 <= x < max_pages * page for x in ctxs)
    c.q, K, V = make_inputs(kind, family, Hq, Hkv, ctxs, seed, groups)
    g = torch.Generator().manual_seed(seed + 7919)
    n_pages = c.n_pages = B * max_pages
    table = torch.randperm(n_pages, generator=g).view(B, max_pages).to(torch.int32)   # random physical placement; unused entries: valid ids of NaN pages
    r0 = 0
    for N, sh in (groups or []):
        for j in range(N):
            table[r0 + j, :sh] = table[r0, :sh]   # the same physical ids (those row j held there are referenced by nobody now)
        r0 += N
    c.table = table
    shape = (n_pages, Hkv, page, HD)
    if kind == "fp8":
        K8, KS, KD = zip(*[quant_rows_e4m3(k) for k in K])
        V8, VS, VD = zip(*[quant_rows_e4m3(v) for v in V])
        c.kd, c.vd = list(KD), list(VD)
        c.k8, c.v8, c.ksc, c.vsc = list(K8), list(V8), list(KS), list(VS)
        c.kc, c.vc = torch.full(shape, 0x7F, dtype=torch.uint8), torch.full(shape, 0x7F, dtype=torch.uint8)   # e4m3 NaN
        c.ks, c.vs = torch.full(shape[:3], NAN), torch.full(shape[:3], NAN)
        c.stage = torch.stack([torch.stack([K[b][ctxs[b]], V[b][ctxs[b]]], dim=1) for b in range(B)]).to(torch.bfloat16).contiguous()   # [B][Hkv][2][128]
        n_cached = list(ctxs)   # keys 0 .. ctx - 1: position ctx is NaN until the launch appends it
        src = [(c.kc, K8), (c.vc, V8), (c.ks, KS), (c.vs, VS)]
    elif kind == "bf16":
        c.kd, c.vd = K, V
        c.kc, c.vc = torch.full(shape, NAN).to(torch.bfloat16), torch.full(shape, NAN).to(torch.bfloat16)
        n_cached = [x + 1 for x in ctxs]
        src = [(c.kc, [k.to(torch.bfloat16) for k in K]), (c.vc, [v.to(torch.bfloat16) for v in V])]
    else:
        if kind == "x24":
            K, V = [x24_planes(k)[2] for k in K], [x24_planes(v)[2] for v in V]   # the values the planes hold
        c.kd, c.vd = K, V
        c.kc, c.vc = torch.full(shape, NAN), torch.full(shape, NAN)
        n_cached = [x + 1 for x in ctxs]
        src = [(c.kc, K), (c.vc, V)]
    for b in range(B):
        for t0 in range(0, n_cached[b], page):
            pg, n = int(table[b, t0 // page]), min(page, n_cached[b] - t0)
            for dst, rows in src:
                dst[pg, :, :n] = rows[b][t0:t0 + n].transpose(0, 1)
    return c


# ---- float64 reference -----------------------------------------------------------------------------------------------------------------------
def split_range(L, nsplit, s, k_first=0):
    kps = (-(-L // nsplit) + 15) & ~15
    k0 = k_first + s * kps
    return k0, min(L, k0 + kps)


def _scores64(c, b):
    rep = c.Hq // c.Hkv
    kk, vv = c.kd[b].double().repeat_interleave(rep, dim=1), c.vd[b].double().repeat_interleave(rep, dim=1)   # [L, Hq, 128]
    return torch.einsum("hd,lhd->hl", c.q[b].double(), kk) * SCALE, vv


def ref64(c):
    ref = torch.zeros(c.B, c.Hq, HD, dtype=torch.float64)
    for b in range(c.B):
        if b in c.done:
            continue   # a row flagged done: zeros
        att, vv = _scores64(c, b)
        ref[b] = torch.einsum("hl,lhd->hd", torch.softmax(att, dim=-1), vv)
    return ref


def ref_partials64(c, nsplit):
    """(lse [B, Hq, nsplit], o / l [B, Hq, nsplit, 128]); an empty split (and every split of a done row): lse = -inf, o / l = 0"""
    lse = torch.full((c.B, c.Hq, nsplit), -math.inf, dtype=torch.float64)
    on = torch.zeros(c.B, c.Hq, nsplit, HD, dtype=torch.float64)
    for b in range(c.B):
        if b in c.done:
            continue
        att, vv = _scores64(c, b)
        for s in range(nsplit):
            k0, k1 = split_range(c.ctxs[b] + 1, nsplit, s)
            if k0 >= k1:
                continue
            lse[b, :, s] = torch.logsumexp(att[:, k0:k1], dim=-1)
            on[b, :, s] = torch.einsum("hl,lhd->hd", torch.softmax(att[:, k0:k1], dim=-1), vv[k0:k1])
    return lse, on


# ---- fp32 emulation --------------------------------------------------------------------------------------------------------------------------
def fast_exp(x):
    """the device's __expf: 2^(fl(x log2 e)), the product rounded to fp32 (exp(-inf) = 0)"""
    return torch.exp2((x * LOG2E).float())


def _merge32(o, m, l):
    """fp32 merge of states along dim 0: (o [n, H, 128], m [n, H], l [n, H]) -> one state; empty states (m = -inf) weigh 0"""
    M = m.max(dim=0).values
    Ms = torch.where(torch.isinf(M), torch.zeros_like(M), M)
    w = torch.where(torch.isinf(m), torch.zeros_like(m), fast_exp(m - Ms))
    oo, ll = torch.zeros_like(o[0]), torch.zeros_like(l[0])
    for i in range(o.shape[0]):   # sequential: an order of its own
        oo = oo + o[i] * w[i][:, None]
        ll = ll + l[i] * w[i]
    return oo, M, ll


def _partial32(att, vv, NS=16):
    """Online softmax over the keys of one range in fp32: NS interleaved states (key i belongs to state i % NS), one key per state and step,
    then their merge.  att [H, n] fp32, vv [n, H, 128] fp32 -> (o [H, 128] un-normalised, m [H], l [H])"""
    H, n = att.shape
    steps = -(-n // NS)
    pad = steps * NS - n
    a = torch.cat([att, torch.full((H, pad), -math.inf)], dim=1).view(H, steps, NS)
    v = torch.cat([vv, torch.zeros(pad, H, HD)], dim=0).view(steps, NS, H, HD)
    m = torch.full((NS, H), -math.inf)
    l = torch.zeros(NS, H)
    o = torch.zeros(NS, H, HD)
    for t in range(steps):
        s = a[:, t].T                                  # [NS, H]
        mn = torch.maximum(m, s)
        ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
        alpha, pw = fast_exp(m - ms), fast_exp(s - ms)
        l = l * alpha + pw
        o = o * alpha[..., None] + pw[..., None] * v[t]
        m = mn
    return _merge32(o, m, l)


def emu32(c, form):
    """form: dict(direct=0/1, nsplit=n) or dict(group=(N, span nsplit)).  Returns dict(o=[B, Hq, 128] fp32 (the finished or merged row),
    and for the split forms lse / on per split like ref_partials64)."""
    rep = c.Hq // c.Hkv
    bf16_row = c.kind in ("bf16", "fp8") and (form.get("direct") or "group" in form)
    out = dict(o=torch.zeros(c.B, c.Hq, HD))
    ns = form.get("nsplit", 1)
    if not form.get("direct") and "group" not in form:
        out["lse"] = torch.full((c.B, c.Hq, ns), -math.inf)
        out["on"] = torch.zeros(c.B, c.Hq, ns, HD)
    r0_of = {}
    if "group" in form:
        r0 = 0
        for N, sh in c.groups:
            for j in range(N):
                r0_of[r0 + j] = sh
            r0 += N
    for b in range(c.B):
        if b in c.done:
            continue
        kk, vv = c.kd[b].float().repeat_interleave(rep, dim=1), c.vd[b].float().repeat_interleave(rep, dim=1)
        att = (torch.einsum("hd,lhd->hl", c.q[b].float(), kk) * SCALE).float()
        L = c.ctxs[b] + 1
        if "group" in form:   # the span's splits over [0, sh), then the tail [sh, L)
            sh, gns = r0_of[b] * c.page, form["group"][1]
            ranges = [split_range(sh, gns, s) for s in range(gns)] + [(sh, L)]
        else:
            ranges = [split_range(L, ns, s) for s in range(ns)]
        parts = []
        for k0, k1 in ranges:
            if k0 >= k1:
                parts.append((torch.zeros(c.Hq, HD), torch.full((c.Hq,), -math.inf), torch.zeros(c.Hq)))
            else:
                parts.append(_partial32(att[:, k0:k1], vv[k0:k1]))
        if "lse" in out:
            for s, (o, m, l) in enumerate(parts):
                if not torch.isinf(m).all():
                    out["lse"][b, :, s] = m + torch.log(l)
                    out["on"][b, :, s] = o / l[:, None]
        o, m, l = _merge32(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), torch.stack([p[2] for p in parts]))
        row = o * (1.0 / l)[:, None]
        out["o"][b] = bf(row) if bf16_row else row
    return out


def merge_partials(part, nsplit):
    """f32 [B, Hq, nsplit, 132] -> (merged o [B, Hq, 128] (the o-proj prologue's merge, in float64), lse, o / l per split)"""
    p = part.double()
    o, m, l = p[..., :HD], p[..., HD], p[..., HD + 1]
    M = m.max(dim=-1, keepdim=True).values
    Ms = torch.where(torch.isinf(M), torch.zeros_like(M), M)
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - Ms))
    den = (l * w).sum(-1)
    merged = (o * w[..., None]).sum(-2) / torch.where(den > 0, den, torch.ones_like(den))[..., None]
    lse = torch.where(l > 0, m + torch.log(torch.where(l > 0, l, torch.ones_like(l))), torch.full_like(m, -math.inf))
    on = o / torch.where(l > 0, l, torch.ones_like(l))[..., None]
    return merged, lse, on


# ---- error measures --------------------------------------------------------------------------------------------------------------------------
def err_o(got, ref):
    """max |got - ref| / rms(ref) per row, worst row (rows whose reference is all zero -- done rows -- must be exactly zero)"""
    worst = 0.0
    g, r = got.double(), ref.double()
    for b in range(r.shape[0]):
        rms = r[b].pow(2).mean().sqrt().item()
        if rms == 0.0:
            assert (g[b] == 0).all(), f"row {b}: a done row / an empty split holds something"
            continue
        worst = max(worst, ((g[b] - r[b]).abs().max() / rms).item())
    return worst


def err_lse(got, ref):
    live = ~torch.isinf(ref)
    assert torch.equal(torch.isinf(got) & (got < 0), ~live), "the empty splits are not the reference's"
    if not live.any():
        return 0.0
    g, r = got.double()[live], ref.double()[live]
    return ((g - r).abs() / r.abs().clamp_min(1.0)).max().item()


def err_rel(got, ref):
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-6)).item()


def spread_bf16(got, ref, rtol=1e-2):
    """the smallest atol_frac at which assert_elementwise (tests/test_ops_gpu.py) passes: max (|err| - rtol |ref|) / rms(ref)"""
    g, r = got.double(), ref.double()
    return max(0.0, (((g - r).abs() - rtol * r.abs()).max() / r.pow(2).mean().sqrt()).item())


def errors(c, form, got, ref=None, refp=None):
    """every measure of a form's outputs: got = dict(o=...) (+ lse, on for the split forms)"""
    ref = ref64(c) if ref is None else ref
    e = dict(o=err_o(got["o"], ref), rel=err_rel(got["o"], ref))
    if "lse" in got:
        lse, on = ref_partials64(c, form["nsplit"]) if refp is None else refp
        e["lse"] = err_lse(got["lse"], lse)
        e["on"] = err_o(got["on"].reshape(c.B, -1, HD), on.reshape(c.B, -1, HD))
    elif c.kind in ("bf16", "fp8"):
        e["spread"] = spread_bf16(got["o"], ref)
    return e


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
# A launch plan is what emmax_decode_attn_plan / emmax_group_attn_plan answer: ("attn", G, nw, direct, deep, nsplit, kv8) or
# ("group", span width, span splits, query chunks, tail G, kv8).  Every variant below is run on every (G, family) batch of its cache kind.
def variants(kind, G):
    """[(name, tuning switches, direct, nsplit asked (0 = auto by shape), plan)] of one cache kind and GQA group -- the EDGE batches (19 rows)"""
    v = []
    if kind == "bf16":
        for ns in (1, 2, 4, 8, 16):
            v.append((f"split{ns}", {}, 0, ns, ("attn", G, 4, 0, 0, ns, 0)))
            if G <= 2:
                v.append((f"split{ns}-deep", {"attn_deep": 1}, 0, ns, ("attn", G, 4, 0, 1, ns, 0)))
        v.append(("direct-nw4", {"attn_deep": 0}, 1, 1, ("attn", G, 4, 1, 0, 1, 0)))
        v.append(("direct-nw8", {"attn_nw": 8, "attn_deep": 0}, 1, 1, ("attn", G, 8, 1, 0, 1, 0)))
        v.append(("direct-nw0", {"attn_nw": 0, "attn_deep": 0}, 1, 1, ("attn", G, 8, 1, 0, 1, 0)))   # by shape: Hkv x B <= 256
        if G <= 2:
            v.append(("direct-deep", {"attn_deep": 1}, 1, 1, ("attn", G, 4, 1, 1, 1, 0)))
    elif kind == "fp8":
        for ns in (1, 2, 4, 8, 16):
            v.append((f"split{ns}", {}, 0, ns, ("attn", G, 4, 0, 1, ns, 1)))
        v.append(("direct", {}, 1, 1, ("attn", G, 4, 1, 1, 1, 1)))
    else:
        for ns in (1, 2, 8):
            v.append((f"split{ns}", {}, 0, ns, ("x", G, 0, ns)))
        v.append(("direct", {}, 1, 1, ("x", G, 1, 1)))
    return v


def edge_case(kind, G, family, done=()):
    Hq, Hkv = HEADS[G]
    ctxs = list(EDGE_CTX)
    if family == "ragged":
        ctxs = list(RAGGED_CTX) * 2 + [300, 63]   # the issue's mix, twice, in one multi-row launch
    seed = 1000 * KINDS.index(kind) + 100 * G + FAMILIES.index(family)
    c = build(kind, "random" if family == "ragged" else family, Hq, Hkv, ctxs, seed, done=done)
    c.family = family
    return c


# bf16 forms a step reaches BY SHAPE (no switch set): (name, B, Hq, Hkv, asked nsplit, direct, plan); contexts <= 130 keep the caches small
BY_SHAPE = [
    ("nw4-B16-kv32", 16, 32, 32, 1, 1, ("attn", 1, 4, 1, 0, 1, 0)),        # every step of 9 - 31 rows at 32 kv heads
    ("deep-B32-kv32", 32, 32, 32, 1, 1, ("attn", 1, 4, 1, 1, 1, 0)),       # 1024 blocks: the default rule turns four chunks on
    ("deep-B64-kv16", 64, 32, 16, 1, 1, ("attn", 2, 4, 1, 1, 1, 0)),
    ("auto-B1-kv32", 1, 32, 32, 0, 0, ("attn", 1, 4, 0, 0, 8, 0)),         # nsplit 0 = what the session picks
    ("auto-B3-kv8", 3, 32, 8, 0, 0, ("attn", 4, 4, 0, 0, 8, 0)),
    ("split-deep-B64-kv16", 64, 32, 16, 2, 0, ("attn", 2, 4, 0, 1, 2, 0)),  # 2048 blocks: the split form with four chunks by the default rule
]
# grouped: (name, groups [(N, shared pages, ctxs)], Hq, Hkv, plan).  Tail G 1 / 2 / 4 / 8, span widths 2 / 4 / 8, two query chunks
GROUPED = [
    ("g1-w2", [(2, 1, [64, 100])], 2, 2, ("group", 2, 8, 1, 1)),
    ("g1-w4", [(4, 2, [128, 130, 191, 200])], 2, 2, ("group", 4, 8, 1, 1)),
    ("g2-w4", [(2, 1, [70, 64])], 4, 2, ("group", 4, 8, 1, 2)),
    ("g2-w8-2chunks", [(8, 3, [255, 192, 200, 193, 250, 192, 230, 194])], 4, 2, ("group", 8, 8, 2, 2)),
    ("g4-w8", [(2, 2, [130, 128])], 8, 2, ("group", 8, 8, 1, 4)),
    ("g4-w8-2chunks", [(3, 1, [64, 65, 100]), (3, 0, [5, 40, 63])], 8, 2, ("group", 8, 8, 2, 4)),
    ("g8-w8-2chunks", [(2, 2, [128, 140])], 8, 1, ("group", 8, 8, 2, 8)),
    ("g8-w8-9chunks", [(9, 1, [100] * 9)], 8, 1, ("group", 8, 8, 9, 8)),
    ("g1-w8", [(8, 1, [64, 70, 127, 128, 129, 64, 100, 90])], 2, 2, ("group", 8, 8, 1, 1)),   # one group of 8 rows at G = 1 (8 rows at 32 heads)
]
GROUP_FAMILIES = ("random", "sink", "last")


def _wide(Hq, Hkv, N, B):
    """B / N groups of N rows on one shared page, contexts 64 .. 123: enough span blocks (kv heads x groups x query chunks) for fewer span splits"""
    nq = N * (Hq // Hkv)
    w = 2 if nq <= 2 else 4 if nq <= 4 else 8
    chunks = -(-nq // w)
    blocks, ns = Hkv * (B // N) * chunks, 1
    while ns * blocks < 256 and ns < 8:
        ns *= 2
    return (f"wide-{Hq}-{Hkv}-N{N}-B{B}", [(N, 1, [64 + (7 * (r0 + j)) % 60 for j in range(N)]) for r0 in range(0, B, N)], Hq, Hkv,
            ("group", w, ns, chunks, Hq // Hkv))


# the span's split count falls with the number of span blocks (group_attn_nsplit): 4 / 2 / 1 splits at every width and tail G a step of 32 / 8 / 4 kv
# heads reaches.  Random inputs only
GROUPED_WIDE = [_wide(32, 32, 2, 4), _wide(32, 32, 2, 8), _wide(32, 32, 2, 16), _wide(32, 32, 4, 8), _wide(32, 32, 4, 16), _wide(32, 32, 4, 32),
                _wide(32, 32, 8, 16), _wide(32, 32, 8, 32), _wide(32, 32, 8, 64), _wide(32, 8, 16, 16), _wide(32, 8, 16, 32), _wide(32, 8, 16, 64),
                _wide(32, 4, 16, 32), _wide(32, 4, 16, 64)]
# the page table: (max_pages, page, ctx); B = 1, Hkv = 1.  512 x 64: the context reaches the LAST entry (the second half of the LDS copy); 257 / 256:
# the min(tid + NT, max_pages - 1) clamp on both sides of the half; 1: a table of one entry; page 16 through the ops
TABLES = [(512, 64, 32767), (512, 64, 32704), (257, 64, 16447), (256, 64, 16383), (1, 64, 63), (1, 64, 0), (21, 16, 335)]


def by_shape_case(x):
    name, B, Hq, Hkv = x[:4]
    return build("bf16", "random", Hq, Hkv, [(37 * b + 5) % 130 for b in range(B)], seed=B + Hkv, max_pages=3)


def table_case(kind, max_pages, page, ctx):
    return build(kind, "random", 1, 1, [ctx], 4242 + max_pages + ctx, page=page, max_pages=max_pages)


def grouped_case(name, kind, family):
    allg = GROUPED + GROUPED_WIDE
    g = next(x for x in allg if x[0] == name)
    groups = [(N, sh) for N, sh, _ in g[1]]
    ctxs = [x for _, _, cs in g[1] for x in cs]
    return build(kind, family, g[2], g[3], ctxs, 500 + allg.index(g) * 10 + GROUP_FAMILIES.index(family) + (5 if kind == "fp8" else 0), groups=groups,
                 max_pages=2 if g in GROUPED_WIDE else 8)


def group_tag(plan, kv8):
    """("group", span width, span splits, tail G, kv8): the form (the query chunks are a grid dimension)"""
    return ("group", plan[1], plan[2], plan[4], kv8)


def case_plans():
    """every plan tag some GPU case asserts before it launches (tests/test_decode_attn_plan.py: the closure)"""
    tags = set()
    for kind in ("bf16", "fp8"):
        for G in HEADS:
            tags |= {v[4] for v in variants(kind, G)}
    tags |= {x[6] for x in BY_SHAPE}
    for g in GROUPED + GROUPED_WIDE:
        tags |= {group_tag(g[4], 0), group_tag(g[4], 1)}
    return tags


# ---- the tolerance table ---------------------------------------------------------------------------------------------------------------------
# SPREAD[kind][form][family] = {measure: worst |emu32 - ref64|} over the edge batch of every G (form: "split" = every split count, "direct");
# GROUP_SPREAD[kind][family], TABLE_SPREAD[kind][form].  Measured on the CPU by measure() -- no GPU output involved.
SPREAD = {
    "bf16": {
        "split": {
            "random": {"lse": 1.64e-07, "o": 1.35e-06, "on": 4.79e-06, "rel": 1.4e-07},
            "sink": {"lse": 2.09e-07, "o": 3.61e-12, "on": 1.5e-06, "rel": 9.2e-13},
            "last": {"lse": 2.97e-07, "o": 4.98e-12, "on": 3.5e-06, "rel": 1.31e-12},
            "one_split": {"lse": 2.74e-07, "o": 0, "on": 1.56e-06, "rel": 0},
            "flat": {"lse": 4.43e-08, "o": 3.19e-07, "on": 3.91e-07, "rel": 1.43e-08},
            "low": {"lse": 5.24e-07, "o": 5.53e-05, "on": 0.000221, "rel": 1.23e-05},
            "offset": {"lse": 1.48e-07, "o": 4.49e-07, "on": 1.11e-06, "rel": 4.38e-07},
            "ragged": {"lse": 1.73e-07, "o": 1.52e-06, "on": 4.13e-06, "rel": 1.29e-07},
        },
        "direct": {
            "random": {"o": 0.0122, "rel": 0.00259, "spread": 0},
            "sink": {"o": 3.61e-12, "rel": 9.2e-13, "spread": 0},
            "last": {"o": 4.98e-12, "rel": 1.31e-12, "spread": 0},
            "one_split": {"o": 0, "rel": 0, "spread": 0},
            "flat": {"o": 0.0107, "rel": 0.00311, "spread": 0},
            "low": {"o": 0.0121, "rel": 0.00223, "spread": 7.29e-06},
            "offset": {"o": 0.002, "rel": 0.00196, "spread": 0},
            "ragged": {"o": 0.0115, "rel": 0.00236, "spread": 5.04e-09},
        },
    },
    "fp8": {
        "split": {
            "random": {"lse": 1.61e-07, "o": 2.91e-06, "on": 6.2e-06, "rel": 2.83e-07},
            "sink": {"lse": 1.7e-07, "o": 2.94e-13, "on": 3.11e-06, "rel": 4.85e-14},
            "last": {"lse": 1.52e-07, "o": 1.02e-12, "on": 2.85e-06, "rel": 1.39e-13},
            "one_split": {"lse": 1.72e-07, "o": 0, "on": 2.9e-06, "rel": 0},
            "flat": {"lse": 4.43e-08, "o": 3.11e-07, "on": 3.82e-07, "rel": 1.37e-08},
            "low": {"lse": 2.04e-07, "o": 3.44e-05, "on": 6.62e-05, "rel": 3.94e-06},
            "offset": {"lse": 1.77e-07, "o": 5.21e-07, "on": 8.06e-07, "rel": 5.17e-07},
            "ragged": {"lse": 1.5e-07, "o": 3.68e-06, "on": 5.34e-06, "rel": 2.82e-07},
        },
        "direct": {
            "random": {"o": 0.0169, "rel": 0.00251, "spread": 0},
            "sink": {"o": 2.94e-13, "rel": 4.85e-14, "spread": 0},
            "last": {"o": 1.02e-12, "rel": 1.39e-13, "spread": 0},
            "one_split": {"o": 0, "rel": 0, "spread": 0},
            "flat": {"o": 0.011, "rel": 0.00195, "spread": 0},
            "low": {"o": 0.0218, "rel": 0.00282, "spread": 1.66e-06},
            "offset": {"o": 0.00198, "rel": 0.00195, "spread": 0},
            "ragged": {"o": 0.0191, "rel": 0.00249, "spread": 0},
        },
    },
    "x32": {
        "split": {
            "random": {"lse": 5.42e-07, "o": 1.81e-06, "on": 3.77e-06, "rel": 1.49e-07},
            "sink": {"lse": 3.28e-07, "o": 1.39e-12, "on": 1.5e-06, "rel": 4.06e-13},
            "last": {"lse": 2.46e-07, "o": 2.95e-12, "on": 1.62e-06, "rel": 7.22e-13},
            "one_split": {"lse": 2.72e-07, "o": 0, "on": 1.75e-06, "rel": 0},
            "flat": {"lse": 4.43e-08, "o": 6.9e-07, "on": 9.07e-07, "rel": 4.9e-08},
            "low": {"lse": 4.7e-07, "o": 3.38e-05, "on": 8.9e-05, "rel": 9.71e-06},
            "offset": {"lse": 4.28e-07, "o": 4.4e-07, "on": 9.59e-07, "rel": 4.3e-07},
            "ragged": {"lse": 6.12e-07, "o": 1.28e-06, "on": 3.52e-06, "rel": 1.73e-07},
        },
        "direct": {
            "random": {"o": 1.49e-06, "rel": 1.49e-07},
            "sink": {"o": 1.39e-12, "rel": 4.06e-13},
            "last": {"o": 2.95e-12, "rel": 7.22e-13},
            "one_split": {"o": 0, "rel": 0},
            "flat": {"o": 6.9e-07, "rel": 4.9e-08},
            "low": {"o": 3.31e-05, "rel": 9.71e-06},
            "offset": {"o": 4.4e-07, "rel": 4.3e-07},
            "ragged": {"o": 1.24e-06, "rel": 1.73e-07},
        },
    },
    "x24": {
        "split": {
            "random": {"lse": 2.14e-07, "o": 1.6e-06, "on": 2.45e-06, "rel": 1.24e-07},
            "sink": {"lse": 4.01e-07, "o": 2.81e-12, "on": 1.7e-06, "rel": 8.36e-13},
            "last": {"lse": 2.63e-07, "o": 1.36e-12, "on": 1.5e-06, "rel": 3.85e-13},
            "one_split": {"lse": 3.04e-07, "o": 0, "on": 1.51e-06, "rel": 0},
            "flat": {"lse": 4.43e-08, "o": 5.91e-07, "on": 8.01e-07, "rel": 2.55e-08},
            "low": {"lse": 7.45e-07, "o": 6.37e-05, "on": 0.00018, "rel": 1.99e-05},
            "offset": {"lse": 6.27e-07, "o": 4.21e-07, "on": 8.68e-07, "rel": 4.08e-07},
            "ragged": {"lse": 4.89e-07, "o": 1.48e-06, "on": 2.7e-06, "rel": 1.74e-07},
        },
        "direct": {
            "random": {"o": 1.6e-06, "rel": 1.24e-07},
            "sink": {"o": 2.81e-12, "rel": 8.36e-13},
            "last": {"o": 1.36e-12, "rel": 3.85e-13},
            "one_split": {"o": 0, "rel": 0},
            "flat": {"o": 5.91e-07, "rel": 2.55e-08},
            "low": {"o": 6.37e-05, "rel": 1.99e-05},
            "offset": {"o": 4.21e-07, "rel": 4.08e-07},
            "ragged": {"o": 1.26e-06, "rel": 1.74e-07},
        },
    },
}
GROUP_SPREAD = {
    "bf16": {"random": {"o": 0.0211, "rel": 0.00293, "spread": 2.92e-07}, "sink": {"o": 1.3e-12, "rel": 4.69e-13, "spread": 0}, "last": {"o": 5.8e-13, "rel": 1.92e-13, "spread": 0}},
    "fp8": {"random": {"o": 0.0307, "rel": 0.00284, "spread": 1.31e-07}, "sink": {"o": 4.02e-13, "rel": 6.93e-14, "spread": 0}, "last": {"o": 4.53e-13, "rel": 9.54e-14, "spread": 0}},
}
TABLE_SPREAD = {
    "bf16": {"split": {"lse": 8.79e-08, "o": 2.55e-06, "on": 2.66e-06, "rel": 1.07e-06}, "direct": {"o": 0.00729, "rel": 0.00289, "spread": 0}},
    "fp8": {"split": {"lse": 6.63e-08, "o": 2.69e-06, "on": 2.72e-06, "rel": 9.85e-07}, "direct": {"o": 0.00923, "rel": 0.00288, "spread": 0}},
    "x32": {"split": {"lse": 8.92e-08, "o": 2.83e-06, "on": 2.94e-06, "rel": 1.18e-06}, "direct": {"o": 2.83e-06, "rel": 1.18e-06}},
    "x24": {"split": {"lse": 7.72e-08, "o": 2.49e-06, "on": 2.49e-06, "rel": 9.91e-07}, "direct": {"o": 2.49e-06, "rel": 9.91e-07}},
}
SHAPE_SPREAD = {"split": {"lse": 1.97e-07, "o": 1.61e-06, "on": 2.54e-06, "rel": 1.23e-07}, "direct": {"o": 0.0201, "rel": 0.00256, "spread": 4.29e-08}}
FACTOR = 2.0
BF16_RTOL, BF16_ATOL, BF16_REL = 1e-2, 4e-3, 8e-3   # the project's line for a bf16 row (tests/test_ops_gpu.py)


def tolerances(kind, form, family, table=None, shape=None):
    """{measure: bound} of one (cache kind, form, family).  form: "split" / "direct" / "group"; table / shape = "split" / "direct" for the page-table
    cases / the bf16 by-shape cases"""
    t = SHAPE_SPREAD[shape] if shape else TABLE_SPREAD[kind][table] if table else GROUP_SPREAD[kind][family] if form == "group" else SPREAD[kind][form][family]
    b = {k: FACTOR * v for k, v in t.items()}
    if "spread" in b:   # a bf16 row: never below the project's line
        b["spread"] = max(BF16_ATOL, b["spread"])
        b["rel"] = max(BF16_REL, b["rel"])
    return b


def _worst(into, e):
    for k, v in e.items():
        into[k] = max(into.get(k, 0.0), v)


def measure_edge(kind, family):
    """{form: {measure: worst}} over the four G of one (kind, family)"""
    out = {"split": {}, "direct": {}}
    for G in HEADS:
        c = edge_case(kind, G, family)
        ref = ref64(c)
        for ns in sorted({v[3] for v in variants(kind, G) if not v[2]}):
            _worst(out["split"], errors(c, dict(nsplit=ns), emu32(c, dict(nsplit=ns)), ref))
        _worst(out["direct"], errors(c, dict(direct=1), emu32(c, dict(direct=1, nsplit=1)), ref))
    return out


def measure_group(kind, family):
    out = {}
    for g in GROUPED + (GROUPED_WIDE if family == "random" else []):
        c = grouped_case(g[0], kind, family)
        _worst(out, errors(c, dict(group=1), emu32(c, dict(group=(g[1][0][0], g[4][2])))))
    return out


def measure_shape():
    out = {"split": {}, "direct": {}}
    for x in BY_SHAPE:
        c, ns, direct = by_shape_case(x), x[6][5], x[5]
        _worst(out["direct" if direct else "split"], errors(c, dict(nsplit=ns), emu32(c, dict(direct=direct, nsplit=ns))))
    return out


def measure_table(kind):
    out = {"split": {}, "direct": {}}
    for mp, page, ctx in TABLES:
        c = table_case(kind, mp, page, ctx)
        ref = ref64(c)
        for ns in (1, 8):
            _worst(out["split"], errors(c, dict(nsplit=ns), emu32(c, dict(nsplit=ns)), ref))
        _worst(out["direct"], errors(c, dict(direct=1), emu32(c, dict(direct=1, nsplit=1)), ref))
    return out


def _fmt(d):
    return "{" + ", ".join(f'"{k}": {v:.3g}' for k, v in sorted(d.items())) + "}"


if __name__ == "__main__":
    print("SPREAD = {")
    for kind in KINDS:
        print(f'    "{kind}": {{')
        res = {fam: measure_edge(kind, fam) for fam in FAMILIES}
        for form in ("split", "direct"):
            print(f'        "{form}": {{')
            for fam in FAMILIES:
                print(f'            "{fam}": {_fmt(res[fam][form])},')
            print("        },")
        print("    },")
    print("}\nGROUP_SPREAD = {")
    for kind in ("bf16", "fp8"):
        print(f'    "{kind}": {{' + ", ".join(f'"{fam}": {_fmt(measure_group(kind, fam))}' for fam in GROUP_FAMILIES) + "},")
    print("}\nTABLE_SPREAD = {")
    for kind in KINDS:
        r = measure_table(kind)
        print(f'    "{kind}": {{"split": {_fmt(r["split"])}, "direct": {_fmt(r["direct"])}}},')
    print("}")
    r = measure_shape()
    print(f'SHAPE_SPREAD = {{"split": {_fmt(r["split"])}, "direct": {_fmt(r["direct"])}}}')
