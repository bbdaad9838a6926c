"""References, cases and tolerances of the scoring pass (emma-x_amd/csrc/score.hip).  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

The kernel forms logits[r, c] = sum_k X[r, k] W[c, k] in fp32, tile by tile, and keeps three numbers per row: lse = log sum_{c < V} exp(logit),
the logit of one target id (0.0 for a target outside [0, V)) and the argmax (the lowest id wins a tie).  This module holds

  * the CASES: shapes, families and forced slice counts, with NaN-poisoned X rows behind `rows` and NaN / 3e38 W rows in [V, Np) -- a read that
    should have been masked shows as a wrong VALUE, never as a fault;
  * ref64: float64 throughout on the bf16-valued operands;
  * emu32: the kernel's documented structure in torch fp32, in an order of its own: fp32 products summed one by one in k order; per vocabulary slice
    and 64-column half of a tile (a wave's share) a running (m, l = sum exp(x - m), idx) over the slice's 128-column tiles in order; the two halves
    combined when the slice ends; the slices merged per row (M = max m_s, L = sum l_s exp(m_s - M), lse = M + log L, idx of the lowest slice attaining
    M); the target logit taken from the slice that holds its column;
  * the tolerance table SPREAD[K][family], measured here as |emu32 - ref64| and pinned by tests/test_score_ref.py.  `python tests/score_ref.py`
    prints the measurement.

Measures, per row, in units of that row's max |logit| (an all-zero row has no such unit: there it is log V, the row's lse):
  lse     |got - ref64|              logit   |got - ref64| of the target logit (targets outside [0, V): must be exactly 0.0)
Bound = FACTOR x SPREAD (decode_attn_ref.FACTOR: the device's MFMA summation order, its per-lane running statistics and its exp / log are not
reproduced).  No floor: the outputs are fp32.  argmax must equal ref64's wherever ref64's top-2 margin exceeds twice the logit bound, and the planted
answer in the tie rows and the all-zero rows.
"""

import math
from collections import namedtuple

import torch

from decode_attn_ref import FACTOR

NAN = float("nan")
BIG = 3e38
IGNORE = -100
FAMILIES = ("random", "large", "sink", "flat", "ties")
ROWS = (1, 15, 16, 17, 127, 128, 129, 300)
KS = (64, 128, 192, 256)
VOCABS = ((100, 128), (128, 128), (129, 256), (1000, 1024))

# slices: 0 = the planner's choice, else forced.  pad: what W rows [V, Np) hold.
Case = namedtuple("Case", "name family rows K V Np slices pad seed")


def _cases():
    out = []
    i = 0
    for K in KS:   # every K x every vocabulary; every row count twice
        for V, Np in VOCABS:
            rows = ROWS[(i * 3) % len(ROWS)]
            out.append(Case(f"random-r{rows}-k{K}-v{V}", "random", rows, K, V, Np, 0, ("nan", "big")[i & 1], 100 + i))
            i += 1
    for j, s in enumerate((1, 2, 3, 8, 0)):   # 8 column tiles: one slice, 4 + 4, 3 + 3 + 2, one tile each, the planner's
        out.append(Case(f"random-r129-k128-v1000-s{s}", "random", 129, 128, 1000, 1024, s, ("nan", "big")[j & 1], 200 + j))
    out.append(Case("random-r128-k4096-v384", "random", 128, 4096, 384, 384, 0, "nan", 300))
    # (at least 127 rows each: the spread is a maximum over the rows, and a handful of rows measures it badly)
    shapes = {"large": ((129, 129, 256, 0), (300, 1000, 1024, 3), (300, 100, 128, 0), (127, 128, 128, 0)),
              "sink": ((127, 1000, 1024, 0), (129, 129, 256, 2), (128, 100, 128, 0), (300, 1000, 1024, 8)),
              "flat": ((127, 100, 128, 0), (129, 1000, 1024, 3), (300, 129, 256, 0), (128, 128, 128, 0)),
              "ties": ((129, 1000, 1024, 3), (127, 1000, 1024, 3), (128, 1000, 1024, 3), (300, 1000, 1024, 3))}
    for f, fam in enumerate(("large", "sink", "flat", "ties")):
        for k, K in enumerate(KS):
            rows, V, Np, s = shapes[fam][k]
            out.append(Case(f"{fam}-r{rows}-k{K}-v{V}" + (f"-s{s}" if s else ""), fam, rows, K, V, Np, s, ("nan", "big")[(f + k) & 1], 400 + 10 * f + k))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def bf(x):
    return x.to(torch.bfloat16).float()


def plan(rows, V, ws_bytes, slices=0, cus=256):
    """the planner's rule (score.hip: score_form), restated: (row tiles, column tiles, slices, tiles per slice), or None where it refuses"""
    rt, ct = -(-rows // 128), -(-V // 128)
    cap = ws_bytes // (12 * rows)
    want = slices if slices else min(max(1, 2 * cus // rt), ct, cap)
    if want < 1 or want > ct or want > cap:
        return None
    tps = -(-ct // want)
    return rt, ct, -(-ct // tps), tps


WS_BYTES = 1 << 20   # the scratch the cases are launched with (no case needs a tenth of it)


def case_plan(c):
    return plan(c.rows, c.V, WS_BYTES, c.slices)


# the tie pairs of a `ties` case on 8 column tiles split 3 + 3 + 2: (lower id, higher id), placed inside one 16-column MFMA tile, in two tiles of
# one slice, in two slices, and with the higher twin in the padding [V, Np) (it must not win, and it cannot be a target)
def tie_pairs(c):
    return ((5, 9), (20, 128 + 20), (300, 900), (c.V - 3, c.V + 5))


Operands = namedtuple("Operands", "X W targets tie_rows flat_rows")


def operands(c):
    """X bf16-valued fp32 [row tiles x 128, K] (rows >= c.rows NaN), W [Np, K] (rows >= V poisoned), targets int32 [rows],
    tie_rows {row: planted argmax}, flat_rows [rows whose X is all zero]"""
    g = torch.Generator().manual_seed(c.seed)
    rt, ct, slices, tps = case_plan(c)
    X = bf(torch.randn(rt * 128, c.K, generator=g))
    W = bf(torch.randn(c.Np, c.K, generator=g))
    tie_rows, flat_rows = {}, []
    if c.family == "large":   # logits of order +-80 and beyond exp's fp32 range: sum exp(x) overflows without the maximum subtracted
        W = bf(W * (40.0 / math.sqrt(c.K)))
    elif c.family == "sink":   # one column far above the rest: l stays ~ 1, the lse is that column's logit
        # (magnitudes over four binades: with equal ones the K products share one bit grid and their fp32 sum is exact in any order)
        u = bf(torch.where(torch.rand(c.K, generator=g) < 0.5, -1.0, 1.0) * torch.exp2(4.0 * torch.rand(c.K, generator=g) - 3.0))
        X = bf(X + u)
        W[(c.seed * 37) % c.V] = bf(3.0 * u)
    elif c.family == "flat":
        flat_rows = sorted({0, c.rows // 2, c.rows - 1})
        X[flat_rows] = 0.0
    X[c.rows:] = NAN
    W[c.V:] = NAN if c.pad == "nan" else BIG
    # targets: columns 0, 127, 128, V - 1, the first and the last column of every slice, -100, then random ones
    want = [0, 127, 128, c.V - 1, IGNORE]
    for s in range(slices):
        want += [s * tps * 128, min((s + 1) * tps * 128, c.V) - 1]
    want = [t for t in want if t < c.V]
    tg = torch.randint(0, c.V, (c.rows,), generator=g, dtype=torch.int32)
    if c.family == "ties":
        for r, (a, b) in enumerate(tie_pairs(c)):   # row r's own direction in both twins: x . x ~ K against ~ sqrt(K) elsewhere
            W[a] = X[r]
            W[b] = X[r]
            tie_rows[r] = a
            tg[r] = b if b < c.V else a
        for j, t in enumerate(want):
            if len(tie_rows) + j < c.rows:
                tg[len(tie_rows) + j] = t
    else:
        if c.family == "sink":
            tg[::3] = (c.seed * 37) % c.V   # the sink itself: the logit the unit comes from
        for j, t in enumerate(want):
            tg[(j * 7 + c.rows // 3) % c.rows] = t
        if c.rows > 4:
            tg[1] = IGNORE
    return Operands(X, W, tg, tie_rows, flat_rows)


Ref = namedtuple("Ref", "lse logit argmax unit margin")


def ref64(c, o):
    """float64: lse, target logit (0 outside [0, V)), argmax (lowest id of the maximum), the row's unit max |logit| (all-zero row: log V), the top-2 margin"""
    Z = o.X[:c.rows].double() @ o.W[:c.V].double().T
    lse = torch.logsumexp(Z, dim=-1)
    t = o.targets.long()
    ok = (t >= 0) & (t < c.V)
    logit = torch.where(ok, Z.gather(1, t.clamp(0, c.V - 1)[:, None])[:, 0], torch.zeros(c.rows, dtype=torch.float64))
    top = Z.max(dim=-1).values
    ids = torch.arange(c.V)
    am = torch.where(Z == top[:, None], ids[None, :], c.V).min(dim=-1).values.int()
    unit = Z.abs().max(dim=-1).values
    unit = torch.where(unit == 0, torch.full_like(unit, math.log(c.V)), unit)
    if c.V > 1:
        t2 = Z.topk(2, dim=-1).values
        margin = t2[:, 0] - t2[:, 1]
    else:
        margin = torch.full((c.rows,), math.inf, dtype=torch.float64)
    return Ref(lse, logit, am, unit, margin)


def acc32(X, W):
    """fp32 [rows, N]: the products one by one in k order (a product of two bf16 values is exact: one rounding per step)"""
    acc = torch.zeros(X.shape[0], W.shape[0], dtype=torch.float32)
    for k in range(X.shape[1]):
        acc.addcmul_(X[:, k][:, None], W[:, k][None, :])
    return acc


PLANTS = ("no_max", "no_rescale", "highest_id", "unmasked", "wrong_slice", "no_guard")
Got = namedtuple("Got", "lse logit argmax")
_HI = 2 ** 31 - 1


def emu32(c, o, plant=""):
    rt, ct, slices, tps = case_plan(c)
    rows = c.rows
    Z = acc32(o.X[:rows], o.W)   # every column of W, the poisoned ones too: masked below by SELECTION, as the kernel does
    ids = torch.arange(ct * 128)
    Z = Z[:, : ct * 128]
    live = ids < (c.Np if plant == "unmasked" else c.V)
    Zm = torch.where(live[None, :], Z, torch.full_like(Z, -math.inf))
    hi = plant == "highest_id"
    ninf = torch.full((rows,), -math.inf)

    def pick(vals, cols):   # (maximum, its lowest id)
        bm = vals.max(dim=-1).values
        at = vals == bm[:, None]
        bi = torch.where(at, cols[None, :], -1).max(dim=-1).values if hi else torch.where(at, cols[None, :], _HI).min(dim=-1).values
        return bm, bi

    def scale(m, M):   # exp(m - M) with (-inf) - (-inf) guarded
        return torch.where(m == -math.inf, torch.zeros_like(m), torch.exp(m - torch.where(M == -math.inf, torch.zeros_like(M), M)))

    sm, sl, si = [], [], []
    for s in range(slices):
        hm, hl, hidx = [], [], []
        for h in range(2):
            m, l, idx = ninf.clone(), torch.zeros(rows), torch.full((rows,), _HI)
            for t in range(s * tps, min((s + 1) * tps, ct)):
                cols = ids[t * 128 + h * 64: t * 128 + h * 64 + 64]
                vals = Zm[:, cols]
                bm, bi = pick(vals, cols)
                mn = torch.maximum(m, bm)
                if plant == "no_guard":
                    ms = mn
                else:
                    ms = torch.where(mn == -math.inf, torch.zeros_like(mn), mn)   # only masked columns so far: nothing to subtract
                if plant == "no_max":
                    l = l + torch.exp(vals).sum(-1)
                else:
                    l = l * torch.exp(m - ms) + torch.exp(vals - ms[:, None]).sum(-1)
                idx = torch.where((bm >= m) & (bm > -math.inf) if hi else bm > m, bi, idx)
                m = mn
            if plant == "no_max":
                m = torch.where(m == -math.inf, m, torch.zeros_like(m))   # l is a plain sum of exp(x)
            hm.append(m); hl.append(l); hidx.append(idx)
        M = torch.maximum(hm[0], hm[1])
        if hi:
            idx = torch.where(hm[1] >= hm[0], hidx[1], hidx[0])
        else:
            idx = torch.where((hm[1] > hm[0]) | ((hm[1] == hm[0]) & (hidx[1] < hidx[0])), hidx[1], hidx[0])
        sm.append(M); sl.append(hl[0] * scale(hm[0], M) + hl[1] * scale(hm[1], M)); si.append(idx)
    M, idx = sm[0].clone(), si[0].clone()
    for s in range(1, slices):
        take = sm[s] >= M if hi else sm[s] > M
        M, idx = torch.where(take, sm[s], M), torch.where(take, si[s], idx)
    L = torch.zeros(rows)
    for s in range(slices):
        L = L + (sl[s] if plant == "no_rescale" else sl[s] * scale(sm[s], M))
    lse = M + torch.log(L)
    t = o.targets.long()
    ok = (t >= 0) & (t < c.V)
    col = t.clamp(0, c.V - 1)
    if plant == "wrong_slice":   # the column at the same place of the NEXT slice
        col = (col + tps * 128) % (ct * 128)
    logit = torch.where(ok, Z.gather(1, col[:, None])[:, 0], torch.zeros(rows))
    return Got(lse, logit, idx.int())


def errors(c, o, got, ref):
    """got: lse / logit fp32 [rows], argmax int32 [rows].  -> dict(lse, logit: worst row in the row's unit; zero: target logits that must be exactly 0.0
    and are not; argmax: rows past the margin whose id differs; planted: tie / all-zero rows whose id is not the planted one; clear: rows past the
    margin).  Non-finite outputs count as infinitely wrong."""
    def dist(a, b):
        d = (a.double() - b).abs() / ref.unit
        return torch.where(torch.isfinite(a.double()), d, torch.full_like(d, math.inf)).max().item()

    t = o.targets.long()
    out_of = (t < 0) | (t >= c.V)
    bound = tolerances(c)["logit"] if c.K in SPREAD and c.family in SPREAD[c.K] else 0.0
    planted = dict(o.tie_rows)
    planted.update({r: 0 for r in o.flat_rows})
    pr = torch.zeros(c.rows, dtype=torch.bool)
    pr[list(planted)] = True
    clear = (ref.margin / ref.unit > 2.0 * bound) & ~pr
    return dict(lse=dist(got.lse, ref.lse), logit=dist(got.logit, ref.logit),
                zero=int((got.logit[out_of] != 0).sum()),
                argmax=int((got.argmax[clear] != ref.argmax[clear]).sum()),
                planted=sum(int(got.argmax[r]) != a for r, a in planted.items()),
                clear=int(clear.sum()))


def within(c, e):
    """the errors of one launch against the case's bounds"""
    tol = tolerances(c)
    return e["lse"] <= tol["lse"] and e["logit"] <= tol["logit"] and e["zero"] == 0 and e["argmax"] == 0 and e["planted"] == 0


# SPREAD[K][family] = worst |emu32 - ref64| over the cases of that K and family, per row in the row's unit.  Measured on the CPU by measure() -- no GPU
# output involved.
SPREAD = {
    64: {"random": {"lse": 1.48e-07, "logit": 1.5e-07}, "large": {"lse": 1.5e-07, "logit": 1.19e-07}, "sink": {"lse": 9.03e-08, "logit": 7.59e-08}, "flat": {"lse": 1.87e-07, "logit": 1.02e-07}, "ties": {"lse": 1.62e-07, "logit": 9.38e-08}},
    128: {"random": {"lse": 2.94e-07, "logit": 1.49e-07}, "large": {"lse": 2.39e-07, "logit": 9.2e-08}, "sink": {"lse": 2.35e-07, "logit": 2.34e-07}, "flat": {"lse": 2.3e-07, "logit": 7.81e-08}, "ties": {"lse": 2.96e-07, "logit": 2.85e-07}},
    192: {"random": {"lse": 2.63e-07, "logit": 1.48e-07}, "large": {"lse": 2.35e-07, "logit": 1.62e-07}, "sink": {"lse": 2.19e-07, "logit": 2.19e-07}, "flat": {"lse": 3.53e-07, "logit": 2.41e-07}, "ties": {"lse": 4.13e-07, "logit": 2.86e-07}},
    256: {"random": {"lse": 4.68e-07, "logit": 3.52e-07}, "large": {"lse": 2.11e-07, "logit": 1.36e-07}, "sink": {"lse": 3.07e-07, "logit": 2.49e-07}, "flat": {"lse": 2.14e-07, "logit": 3.32e-07}, "ties": {"lse": 3.11e-07, "logit": 3.11e-07}},
    4096: {"random": {"lse": 1.76e-06, "logit": 9.09e-07}},
}


def tolerances(c):
    return {k: FACTOR * v for k, v in SPREAD[c.K][c.family].items()}


def measure():
    out = {}
    for c in CASES:
        o = operands(c)
        e = errors(c, o, emu32(c, o), ref64(c, o))
        assert e["zero"] == 0 and e["planted"] == 0, (c.name, e)
        d = out.setdefault(c.K, {}).setdefault(c.family, {"lse": 0.0, "logit": 0.0})
        d["lse"], d["logit"] = max(d["lse"], e["lse"]), max(d["logit"], e["logit"])
    return out


if __name__ == "__main__":
    print("SPREAD = {")
    for K, fams in sorted(measure().items()):
        print(f"    {K}: {{" + ", ".join(f'"{f}": {{"lse": {v["lse"]:.3g}, "logit": {v["logit"]:.3g}}}' for f, v in fams.items()) + "},")
    print("}")
