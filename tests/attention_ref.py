"""References, inputs and tolerances of tests/test_attention_forms_gpu.py.  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

The prefill / ViT attention (emma-x_amd/csrc/attention.hip) is two kernels in ten instantiations: the ring kernel at head_dim 64 and 72 with three
or four query waves, at head_dim 128 with the lazy reference maximum, without it (attn_lazy = 0) and as two key groups per block (KSPL = 2), and
the resident kernel at head_dim 64 (256 / 288 rows) and 72.  This module holds, for all of them,

  * the CASE BUILDER: a packed qkv buffer in one of three layouts (ViT 0 / D / 2D, LLaMA 0 / q_dim / q_dim + kv_dim, and one with q_off != 0 and
    gaps between the three), ld_qkv above the used columns; every unused column and one guard row before and after the buffer hold bf16 NaN; the
    output is NaN with padding columns and guard rows that must come back bit-untouched.  Ragged batches with empty sequences, GQA groups 1 / 2 / 4
    and Hkv = 1, B x Hq not a multiple of 8;
  * ref64: float64 softmax(q k^T scale [causal]) v per sequence and head;
  * emu32: the documented roundings in torch fp32, in a summation order of its own: bf16 operands, fp32 scores, 2^(s c - m c) with c = fl(scale
    log2 e) folded in, P rounded to bf16 for the PV product while the row sum adds the unrounded p, one online-softmax step per 64 or 32 keys (the
    form's step), the lazy rule of the forms that have it (the reference maximum moves only above +8 in the exp2 domain: P in (0, 2^8]), the
    two-group merge of KSPL = 2, ONE bf16 rounding of the finished row.  It also counts the LATE MOVES (a row whose reference moves after its first
    step) and the MIXED waves (a 32-query wave in which some rows move and others stay) of a case, and takes the MUTANTS of
    tests/test_attention_ref.py;
  * the INPUT FAMILIES, the CASES (each tagged with the plan it must reach: tests/test_attention_plan.py proves the tags cover all ten
    instantiations) and the tolerance table SPREAD, measured here as |emu32 - ref64| and pinned by tests/test_attention_ref.py.
    `python tests/attention_ref.py` prints the measurement.

Error measures (worst over the live rows of a case):
  o       max |got - ref| / rms(ref) per (row, head)           rel   max |got - ref| / max |ref|  (the project's relerr)
  spread  the smallest atol_frac at which assert_elementwise (tests/test_ops_gpu.py) passes at rtol 1e-2 on EVERY SEQUENCE of the launch by itself
          (the rms of a ragged batch is that of its long sequences: against it the bf16 rounding of a 5-key row's P looks like an error)
  flat    the `flat` family only: max |got - ref| / (2^-8 |ref|) -- 1 = half a bf16 ulp at the bottom of a binade; a zero of the reference is exact
Bound = 2 x SPREAD (the factor of decode_stage_ref.tolerances: the device's v_exp_f32 and its MFMA summation order are not reproduced), with the
project's bf16 line as a floor under `rel` and `spread` (8e-3; rtol 1e-2 with atol 4e-3 rms) and TODAY'S test_attention line as a cap over them
(relerr < 1e-2; atol 2e-2 rms): no family is looser than the tests this file joins.  `flat` is held at FLAT_BOUND whatever was measured.
"""

import functools
import math

import torch

LOG2E = 1.44269504088896340736
NAN = float("nan")
NAN_BITS = 0x7FC0   # the bf16 quiet NaN every poisoned element holds
FACTOR = 2.0
BF16_RTOL, BF16_ATOL, BF16_REL = 1e-2, 4e-3, 8e-3   # the project's line for a bf16 row (tests/test_ops_gpu.py: assert_elementwise)
TODAY_REL, TODAY_ATOL = 1e-2, 2e-2                  # tests/test_ops_gpu.py: test_attention (TOL, ATTN_ATOL)
FLAT_BOUND = 1.002                                  # half a bf16 ulp + the fp32 roundings of 1 / n and of the product


def bf(x):
    return x.to(torch.bfloat16).float()


# ---- the ten instantiations ------------------------------------------------------------------------------------------------------------------
# tag = what emmax_attention_plan answers: (kind, head_dim, query waves, producer waves, key groups, lazy, rows per block); step = keys per
# online-softmax step of a wave (ring 64 / 128: the 64-key tile, a tail of <= 32 keys as half a step -- the same numbers; 72, KSPL, resident: 32)
FORMS = {
    "ring64w3": dict(tag=("ring", 64, 3, 0, 1, 0, 96), step=64),
    "ring64w4": dict(tag=("ring", 64, 4, 0, 1, 0, 128), step=64),
    "ring72w3": dict(tag=("ring", 72, 3, 0, 1, 0, 96), step=32),
    "ring72w4": dict(tag=("ring", 72, 4, 0, 1, 0, 128), step=32),
    "ring128": dict(tag=("ring", 128, 4, 0, 1, 1, 128), step=64),
    "ring128nolazy": dict(tag=("ring", 128, 4, 0, 1, 0, 128), step=64),
    "ring128k2": dict(tag=("ring", 128, 4, 0, 2, 1, 128), step=32),
    "res64w8": dict(tag=("res", 64, 8, 2, 1, 1, 256), step=32),
    "res64w9": dict(tag=("res", 64, 9, 2, 1, 1, 288), step=32),
    "res72w8": dict(tag=("res", 72, 8, 2, 1, 1, 256), step=32),
}
for _f in FORMS.values():
    _f.update(hd=_f["tag"][1], kg=_f["tag"][4], lazy=_f["tag"][5], res=_f["tag"][0] == "res")
LAZY_FORMS = tuple(n for n, f in FORMS.items() if f["lazy"])
# the switches that steer a launch into the form whatever its item / block count (the BY_SHAPE cases set none)
FORM_TUNE = {
    "ring64w3": dict(attn_resident=0), "ring64w4": dict(attn_resident=0), "ring72w3": dict(attn_resident=0), "ring72w4": dict(attn_resident=0),
    "ring128": dict(attn_ksplit=0), "ring128nolazy": dict(attn_ksplit=0, attn_lazy=0), "ring128k2": dict(attn_ksplit=1),
    "res64w8": dict(attn_resident=2), "res64w9": dict(attn_resident=2), "res72w8": dict(attn_resident=2),
}
HEADS = {"g1": (2, 2), "g2": (4, 2), "g4": (8, 2), "kv1": (3, 1)}   # GQA group 1 / 2 / 4 and one kv head: the smallest that reach each path
FAMILY_HEADS = {"random": "g2", "boosted": "g1", "flat": "g4", "sink": "g2", "late_under8": "kv1", "late_over8": "g1", "late_60": "g4", "mixed": "kv1",
                "group0": "g2", "group1": "g4"}   # the edge batch of a family (random runs at all four)
FAMILIES = ("random", "boosted", "flat", "sink", "late_under8", "late_over8", "late_60", "mixed")
K2_FAMILIES = ("group0", "group1")   # ring128k2 only: the dominant key in either 32-key half of a tile
# the exp2-domain margin of a planted key over the reference maximum of the rows' first step (sink, group*: over every other key), (lo, hi)
WINDOWS = {"sink": (43.0, 60.0), "late_under8": (6.0, 7.9), "late_over8": (8.1, 10.0), "late_60": (55.0, 66.0), "mixed": (9.0, 14.0),
           "group0": (43.0, 60.0), "group1": (43.0, 60.0)}
EPS = 0.02   # the queries of a planted case: +-(u + EPS noise) -- one direction per kv head, so one key can be placed for all of them
# every edge of the loops: the 32-query wave, the 32 / 64-key step, the 64-key tile, the half-step tail, the 96 / 128-row block, the 256 / 288 rows
# of the resident forms and either side of both; 261 = DINOv2.  A causal batch of these lengths puts a wave's diagonal on a tile boundary (wave at
# 64 k), on a step boundary and inside a half step (wave at 64 k + 32) and at a sequence end inside a wave
EDGE = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 261, 288, 289)
LAYOUTS = ("vit", "llama", "shift")


def three_waves(n):
    return -(-n // 96) * 96 < -(-n // 128) * 128


def layout(name, Hq, Hkv, hd):
    """(q_off, k_off, v_off, ld_qkv, ld_out): offsets multiples of 8, ld_qkv a multiple of 8 above the used columns, ld_out a multiple of 4"""
    qd, kvd = Hq * hd, Hkv * hd
    if name == "vit":      # the ViT session: 0, D, 2D
        return 0, qd, 2 * qd, 2 * qd + kvd + 16, qd + 4
    if name == "llama":    # the LLaMA session: 0, q_dim, q_dim + kv_dim
        return 0, qd, qd + kvd, qd + 2 * kvd + 24, qd + 12
    return 8, qd + 16, qd + kvd + 32, qd + 2 * kvd + 40, qd + 8   # q_off != 0, a gap between q / k / v


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def first_step_keys(form, pos):
    """the keys of the first softmax step of the wave that meets key `pos` (KSPL: of the key group that holds it)"""
    f = FORMS[form]
    if f["kg"] == 2:
        g = (pos % 64) // 32
        return 32 * g, 32 * g + 32
    return 0, f["step"]


def plant_pos(n, i, family):
    """where sequence i of a batch gets its dominant key: None = nowhere (no later step).  Cycles over the places a key can be lost at: the
    sequence end, the last key of a tile, the first key of a tile, the first key of a half tile"""
    if family == "sink":
        return 0
    if family in K2_FAMILIES:
        half = 0 if family == "group0" else 32
        if n - 1 < 64 + half:
            return None
        t = ((n - 1 - half) // 64) * 64 + half   # the last tile's half that exists, past the first tile
        return min(n - 1, t + (5, 31, 0)[i % 3])
    if n <= 64:
        return None
    last_tile_end = ((n - 64) // 64) * 64 + 63          # the largest key = 63 (mod 64) below n
    last_tile0 = ((n - 1) // 64) * 64                    # the largest key = 0 (mod 64)
    last_half0 = ((n - 1 - 32) // 64) * 64 + 32          # the largest key = 32 (mod 64)
    return (n - 1, last_tile_end, last_tile0, last_half0)[i % 4]


def _plant(q, k, pos, hk, rep, rows, form, family, causal, scale):
    """K[pos, hk] = bf16(a u), u = the mean of the planted rows' queries, a the smallest factor on a 2^(1/64) grid at which EVERY planted row's
    margin (exp2 domain) over its reference lies in WINDOWS[family].  The reference: the maximum of the row's first step in this form (what the
    lazy rule compares with); sink / group*: the maximum over every other key the row sees."""
    lo, hi = WINDOWS[family]
    n = k.shape[0]
    qs = q[rows][:, hk * rep:(hk + 1) * rep].reshape(-1, q.shape[-1]).double()   # [m, hd]
    row_of = torch.tensor(rows).repeat_interleave(rep)
    sc = scale * LOG2E
    s = (qs @ k[:, hk].double().T) * sc                                          # [m, n]
    j = torch.arange(n)
    seen = (j[None, :] <= row_of[:, None]) if causal else torch.ones(len(row_of), n, dtype=torch.bool)
    if family in ("sink",) + K2_FAMILIES:
        ref_keys = seen & (j != pos)[None, :]
    else:
        k0, k1 = first_step_keys(form, pos)
        ref_keys = seen & ((j >= k0) & (j < k1) & (j != pos))[None, :]
    has = ref_keys.any(dim=1)
    if not has.any():
        return   # a sequence of one key
    ref = torch.where(ref_keys, s, torch.full_like(s, -math.inf)).max(dim=1).values
    u = qs.mean(0)
    for t in range(-8 * 64, 24 * 64):
        key = bf((u * 2.0 ** (t / 64.0)).float())
        marg = ((qs @ key.double()) * sc - ref)[has]
        if marg.min() >= lo:
            assert marg.max() <= hi, (family, form, n, pos, marg.min().item(), marg.max().item())
            k[pos, hk] = key
            return
    raise AssertionError("no factor plants the key")


def make_seq(form, family, n, Hq, Hkv, causal, g, i, boost=1.0):
    """q [n, Hq, hd], k, v [n, Hkv, hd]: fp32 tensors holding exact bf16 values; sequence i of its batch"""
    hd, rep = FORMS[form]["hd"], Hq // Hkv
    rnd = lambda *s: bf(torch.randn(*s, generator=g))
    q, k, v = rnd(n, Hq, hd), rnd(n, Hkv, hd), rnd(n, Hkv, hd)
    if family == "boosted":
        q = q * 8.0 * boost
    if family == "flat":   # every visible key weighs exactly 1 / n; V[j] = 2^(j // hd) e_(j mod hd): a column shows WHICH keys were summed
        q = torch.zeros(n, Hq, hd)
        v = torch.zeros(n, Hkv, hd)
        j = torch.arange(n)
        v[j, :, j % hd] = (2.0 ** (j // hd).float())[:, None]
    if family in WINDOWS and n:
        u = torch.randn(1, Hkv, 1, hd, generator=g)
        q = bf((u + EPS * torch.randn(n, Hkv, rep, hd, generator=g)).view(n, Hq, hd))
        sign = torch.ones(n)
        if family == "mixed":
            sign[torch.arange(n) % 2 == 1] = -1.0   # odd rows look away from the planted key: they stay while their neighbours move
        q = q * sign[:, None, None]
        pos = plant_pos(n, i, family)
        if pos is not None:
            rows = [r for r in range(n) if sign[r] > 0 and (not causal or r >= pos)]
            if rows:
                for hk in range(Hkv):
                    _plant(q, k, pos, hk, rep, rows, form, family, causal, hd ** -0.5)
    return q, k, v


class Case:
    """One launch: name, form, family, heads, lens, causal, layout, tune, by_shape; q / k / v per sequence (lists) once built"""

    def __init__(self, form, family, heads, lens, causal, lay, name=None, by_shape=False, seed=0, tune=None):
        self.form, self.family, self.heads, self.lens, self.causal, self.lay = form, family, heads, list(lens), int(causal), lay
        self.Hq, self.Hkv = HEADS[heads] if isinstance(heads, str) else heads
        self.hd = FORMS[form]["hd"]
        self.scale = self.hd ** -0.5
        self.by_shape = by_shape
        self.tune = {} if by_shape else dict(FORM_TUNE[form] if tune is None else tune)
        self.tag = FORMS[form]["tag"]
        self.name = name or f"{form}-{'causal' if causal else 'full'}-{family}-{heads}-{lay}-top{max(lens)}x{len(lens)}"
        self.seed = seed
        self.B, self.max_seqlen, self.total = len(lens), max(lens), sum(lens)
        self.built = False

    def build(self):
        if self.built:
            return self
        g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(self.name)) % (2 ** 31) + self.seed)
        self.q, self.k, self.v = [], [], []
        for i, n in enumerate(self.lens):
            q, k, v = make_seq(self.form, self.family, n, self.Hq, self.Hkv, self.causal, g, i)
            self.q.append(q), self.k.append(k), self.v.append(v)
        self.built = True
        return self

    def buffers(self):
        """(qkv bf16 [total + 2, ld] with NaN in every unused column and in the guard rows 0 and total + 1, cu int32 [B + 1] relative to row 1,
        out bf16 [total + 2, ld_out] all NaN, (q_off, k_off, v_off, ld, ld_out))"""
        self.build()
        q_off, k_off, v_off, ld, ld_out = layout(self.lay, self.Hq, self.Hkv, self.hd)
        qd, kvd = self.Hq * self.hd, self.Hkv * self.hd
        qkv = torch.full((self.total + 2, ld), NAN_BITS, dtype=torch.int16).view(torch.bfloat16)
        if self.total:
            qkv[1:-1, q_off:q_off + qd] = torch.cat(self.q).reshape(self.total, qd).to(torch.bfloat16)
            qkv[1:-1, k_off:k_off + kvd] = torch.cat(self.k).reshape(self.total, kvd).to(torch.bfloat16)
            qkv[1:-1, v_off:v_off + kvd] = torch.cat(self.v).reshape(self.total, kvd).to(torch.bfloat16)
        cu = torch.tensor([0] + list(torch.tensor(self.lens).cumsum(0)), dtype=torch.int32)
        out = torch.full((self.total + 2, ld_out), NAN_BITS, dtype=torch.int16).view(torch.bfloat16)
        return qkv, cu, out, (q_off, k_off, v_off, ld, ld_out)


# ---- float64 reference -----------------------------------------------------------------------------------------------------------------------
def ref64(c):
    """[total, Hq, hd] float64"""
    c.build()
    rep, outs = c.Hq // c.Hkv, []
    for b, n in enumerate(c.lens):
        if n == 0:
            continue
        q, k, v = c.q[b].double(), c.k[b].double().repeat_interleave(rep, dim=1), c.v[b].double().repeat_interleave(rep, dim=1)
        s = torch.einsum("nhd,mhd->hnm", q, k) * c.scale
        if c.causal:
            s = s.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), 1), -math.inf)
        outs.append(torch.einsum("hnm,mhd->nhd", torch.softmax(s, dim=-1), v))
    return torch.cat(outs) if outs else torch.zeros(0, c.Hq, c.hd, dtype=torch.float64)


# ---- fp32 emulation --------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_tile_last", "double_tile_first", "diag_shift", "skip_lazy_rescale", "wrong_row_alpha", "gqa_neighbour", "swap_merge", "stop_short")


def _exp2_fma(s, c, mc):
    """2^(fma(s, c, -mc)): the product exact (float64 holds 24 x 24 bits), ONE rounding to fp32, as v_fma_f32 does"""
    return torch.exp2((s.double() * float(c) - mc.double()[..., None]).float())


def emu32(c, mut=None, stats=None):
    """[total, Hq, hd] fp32 holding the bf16 rows the form's documented arithmetic gives.  mut: one of MUTANTS (tests/test_attention_ref.py).
    stats: a dict that receives late_moves (rows x heads x steps whose reference moved after the first step) and mixed_waves (wave-steps in
    which some live rows moved late and others stayed)"""
    c.build()
    f = FORMS[c.form]
    step, lazy, kg, hd, rep = f["step"], f["lazy"], f["kg"], f["hd"], c.Hq // c.Hkv
    cc = (torch.tensor(c.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))   # c = fl(scale x log2 e)
    late_moves = mixed = 0
    outs = []
    for b, n in enumerate(c.lens):
        if n == 0:
            continue
        hk = torch.arange(c.Hq) // rep
        if mut == "gqa_neighbour":
            hk = (hk + 1) % c.Hkv
        q, k, v = c.q[b], c.k[b][:, hk], c.v[b][:, hk]                      # [n, Hq, hd]
        S = torch.einsum("nhd,mhd->hnm", q, k).float()                      # fp32 scores [Hq, n, n]
        i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
        vis = (j <= i + (1 if mut == "diag_shift" else 0)) if c.causal else torch.ones(n, n, dtype=torch.bool)
        if mut == "stop_short" and n > 1:
            vis = vis & (j < n - 1)
        if mut == "drop_tile_last":
            vis = vis & (j % 64 != 63)
        wgt = torch.ones(n)
        if mut == "double_tile_first":
            wgt[torch.arange(n) % 64 == 0] = 2.0
        partner = torch.arange(n) ^ 1
        partner = torch.where(partner < n, partner, torch.arange(n))
        states = []
        for g in range(kg):
            m = torch.full((c.Hq, n), -math.inf)
            l = torch.zeros(c.Hq, n)
            O = torch.zeros(c.Hq, n, hd)
            blocks = [(t + 32 * g, min(n, t + 32 * g + 32)) for t in range(0, n, 64)] if kg == 2 else [(t, min(n, t + step)) for t in range(0, n, step)]
            for k0, k1 in blocks:
                if k0 >= n:
                    continue
                vb = vis[:, k0:k1]
                seen = vb.any(dim=1)                                        # rows that meet a key in this step
                sb = torch.where(vb[None], S[:, :, k0:k1], torch.tensor(-math.inf))
                mt = sb.max(dim=-1).values
                first = torch.isinf(m)
                if lazy:
                    move = seen[None] & (mt * cc > m * cc + 8.0)
                    m_new = torch.where(move, mt, m)
                    alpha = torch.where(move & ~first, torch.exp2((m - m_new) * cc), torch.ones_like(m))
                    late = move & ~first
                    late_moves += int(late.sum())
                    for w0 in range(0, n, 32):
                        lw, sw = late[:, w0:w0 + 32], seen[w0:w0 + 32]
                        mixed += int((lw.any(dim=1) & (~lw[:, sw]).any(dim=1)).sum())
                    alpha_o = alpha
                    if mut == "skip_lazy_rescale":
                        alpha_o = torch.ones_like(alpha)
                    if mut == "wrong_row_alpha":
                        alpha_o = alpha[:, partner]
                else:
                    m_new = torch.where(seen[None], torch.maximum(m, mt), m)
                    alpha = alpha_o = torch.where(first, torch.ones_like(m), torch.exp2((m - m_new) * cc))
                live = seen[None] & ~torch.isinf(m_new)
                p = torch.where(vb[None] & live[..., None], _exp2_fma(S[:, :, k0:k1], cc, torch.where(live, m_new * cc, torch.zeros_like(m))),
                                torch.zeros(1)) * wgt[k0:k1]
                l = l * alpha + p.sum(dim=-1)
                O = O * alpha_o[..., None] + torch.einsum("hnk,khd->hnd", bf(p), v[k0:k1])
                m = m_new
            states.append((m, l, O))
        m, l, O = states[0]
        if kg == 2:   # group 1 hands (m, l, O) over; a group that met no key: m = -inf, weight 2^-inf = 0
            m1, l1, O1 = states[1]
            M = torch.maximum(m, m1)
            a0 = torch.exp2((m - M) * cc)
            a1 = torch.where(torch.isinf(m1), torch.zeros_like(m1), torch.exp2((m1 - M) * cc))
            if mut == "swap_merge":
                a0, a1 = a1, a0
            l, O = l * a0 + l1 * a1, O * a0[..., None] + O1 * a1[..., None]
        inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        outs.append(bf(O * inv[..., None]).permute(1, 0, 2))
    if stats is not None:
        stats.update(late_moves=late_moves, mixed_waves=mixed)
    return torch.cat(outs) if outs else torch.zeros(0, c.Hq, hd)


# ---- error measures --------------------------------------------------------------------------------------------------------------------------
def errors(c, got, ref):
    """got, ref [total, Hq, hd].  flat: {"flat"}; every other family {"o", "rel", "spread"}"""
    g, r = got.double(), ref.double()
    if c.family == "flat":
        zero = r == 0
        if not (g[zero] == 0).all():
            return {"flat": math.inf}   # a key was summed into a column no visible key feeds
        return {"flat": ((g - r).abs()[~zero] / (2.0 ** -8 * r.abs()[~zero])).max().item()}
    rms = r.pow(2).mean(dim=-1, keepdim=True).sqrt()
    assert (rms > 0).all()
    spread, o = 0.0, 0
    for n in c.lens:   # per sequence: a row of 5 keys is not measured against the rms of a neighbour's rows of 256
        if n:
            gs, rs = g[o:o + n], r[o:o + n]
            spread, o = max(spread, (((gs - rs).abs() - BF16_RTOL * rs.abs()).max() / rs.pow(2).mean().sqrt()).item()), o + n
    return {"o": ((g - r).abs() / rms).max().item(), "rel": ((g - r).abs().max() / r.abs().max().clamp_min(1e-6)).item(), "spread": spread}


def violations(c, got, ref, tol=None):
    """the measures of `got` that exceed the bound of the case's (form, family) -- what fails the GPU test"""
    tol = tolerances(c.form, c.family) if tol is None else tol
    if not torch.isfinite(got).all():
        return [f"{c.name}: {int((~torch.isfinite(got)).sum())} values of live rows are not finite"]
    e = errors(c, got, ref)
    return [f"{c.name}: {k} {e[k]:.3g} > {tol[k]:.3g}" for k in tol if e[k] > tol[k]]


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
def _edge_lens(form):
    """every EDGE length the form takes as max_seqlen allows, an empty sequence in the middle and one at the end; B x Hq is no multiple of 8"""
    f = FORMS[form]
    top = {"ring64w3": 288, "ring72w3": 288, "res64w8": 256, "res72w8": 256, "res64w9": 288}.get(form, 289)
    lens = [n for n in EDGE if n <= top]
    lens = lens[:7] + [0] + lens[7:] + [0]
    return lens if len(lens) % 2 else lens + [top - 7]   # an odd B: B x Hq of 2, 3 or 4 heads leaves idle items in the XCD map


def _long_lens(form):
    """many ring wraps: 1025 keys (three waves by the rule; head_dim 128 always has four), 1024 and a tail where the rule gives four"""
    return [1025] if form in ("ring64w3", "ring72w3") or FORMS[form]["hd"] == 128 else [1000, 1024]


def form_cases(form):
    f = FORMS[form]
    hd128 = f["hd"] == 128
    main = 1 if hd128 else 0              # the causal LLaMA prefill / the bidirectional ViT
    fams = FAMILIES + (K2_FAMILIES if f["kg"] == 2 else ())
    cs = []
    for x, fam in enumerate(fams):
        cs.append(Case(form, fam, FAMILY_HEADS[fam], _edge_lens(form), main, LAYOUTS[x % 3]))
    for x, heads in enumerate(("g1", "g4", "kv1")):   # random (above: g2) at every GQA shape
        cs.append(Case(form, "random", heads, _edge_lens(form), main, LAYOUTS[(x + 1) % 3]))
    if not f["res"]:
        if f["kg"] == 1:      # the other mask: causal 64 / 72, bidirectional 128 (KSPL is causal only)
            cs.append(Case(form, "random", "g2", _edge_lens(form), 1 - main, "llama" if not hd128 else "vit"))
            cs.append(Case(form, "flat", "g1", _edge_lens(form), 1 - main, "shift"))
        for fam in ("random", "boosted") + (("late_over8",) if f["lazy"] else ()):
            cs.append(Case(form, fam, "g1", _long_lens(form), main, "llama" if hd128 else "vit"))
    else:
        # the persistent pipeline under attn_resident = 2: 257 - 512 items = two per block (the double buffer, the producer prefetch, one barrier per
        # item), > 512 = three (both buffers reused), at the towers' real lengths among shorter and empty sequences whose rows keep stale LDS
        top = f["tag"][6] if form != "res64w9" else 261
        for B in (17, 33):
            lens = [(top, top, 200, top, 5, 0, top - 1, 33)[i % 8] for i in range(B)]
            for fam in ("random", "boosted"):
                cs.append(Case(form, fam, (16, 16), lens, 0, "vit", name=f"{form}-items{B * 16}-{fam}"))
    return cs


# launches that reach their form with NO switch set: one frame's LLaMA prefill shape in small (blocks <= 256: two key groups), a causal launch of
# more than 256 blocks (the lazy ring), the ViT towers at the session's shapes, and 528 items of 261 / 256 tokens (the resident head_dim-64 forms)
BY_SHAPE = [
    Case("ring128k2", "random", "g2", [300], 1, "llama", name="shape-one-frame-prefill", by_shape=True),
    Case("ring128", "random", "g4", [129] * 17, 1, "llama", name="shape-many-blocks-prefill", by_shape=True),
    Case("ring128", "random", "g1", [200, 77], 0, "llama", name="shape-bidirectional-128", by_shape=True),
    Case("ring64w3", "random", (16, 16), [261], 0, "vit", name="shape-dinov2-one-frame", by_shape=True),
    Case("ring72w4", "random", (16, 16), [256], 0, "vit", name="shape-siglip-one-frame", by_shape=True),
    Case("res64w9", "random", (16, 16), [261] * 33, 0, "vit", name="shape-dinov2-33-frames", by_shape=True),
    Case("res64w8", "random", (16, 16), [256] * 32, 0, "vit", name="shape-64-32-frames-of-256", by_shape=True),
]
# one token past what the resident forms hold, under attn_resident = 2: the launch must fall back to the ring kernel
OVER_LIMIT = [
    Case("ring64w4", "random", "g1", [289, 0, 288, 289, 17], 0, "vit", name="over-limit-64-at-289", tune=dict(attn_resident=2)),
    Case("ring72w3", "random", "g1", [257, 256, 0, 257, 9], 0, "vit", name="over-limit-72-at-257", tune=dict(attn_resident=2)),
]


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = [c for form in FORMS for c in form_cases(form)] + BY_SHAPE + OVER_LIMIT
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


def cases_of(form, family):
    return [c for c in all_cases() if c.form == form and c.family == family]


def case_tags():
    """(tag, causal) of every GPU case (tests/test_attention_plan.py: the closure)"""
    return {(c.tag, c.causal) for c in all_cases()}


# ---- the tolerance table ---------------------------------------------------------------------------------------------------------------------
# SPREAD[form][family] = worst |emu32 - ref64| over the (form, family)'s cases.  Measured on the CPU by measure() -- no GPU output involved.
SPREAD = {
    "ring64w3": {
        "random": {"o": 0.0167, "rel": 0.0022, "spread": 0.00904},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0147, "rel": 0.00326, "spread": 0.00238},   # late moves 0, mixed waves 0
        "flat": {"flat": 0.929},   # late moves 0, mixed waves 0
        "sink": {"o": 1.32e-11, "rel": 3.94e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0117, "rel": 0.00289, "spread": 0.00443},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0115, "rel": 0.00246, "spread": 0.00443},   # late moves 0, mixed waves 0
        "late_60": {"o": 0.0131, "rel": 0.000858, "spread": 0.0051},   # late moves 0, mixed waves 0
        "mixed": {"o": 0.0137, "rel": 0.00272, "spread": 0.00503},   # late moves 0, mixed waves 0
    },
    "ring64w4": {
        "random": {"o": 0.0163, "rel": 0.00293, "spread": 0.0107},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0162, "rel": 0.0037, "spread": 0.00398},   # late moves 0, mixed waves 0
        "flat": {"flat": 0.929},   # late moves 0, mixed waves 0
        "sink": {"o": 1.28e-11, "rel": 3.51e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0117, "rel": 0.00318, "spread": 0.00519},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0137, "rel": 0.0024, "spread": 0.00493},   # late moves 0, mixed waves 0
        "late_60": {"o": 0.0128, "rel": 0.00142, "spread": 0.00741},   # late moves 0, mixed waves 0
        "mixed": {"o": 0.0133, "rel": 0.00228, "spread": 0.00402},   # late moves 0, mixed waves 0
    },
    "ring72w3": {
        "random": {"o": 0.0161, "rel": 0.00429, "spread": 0.0124},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0159, "rel": 0.00353, "spread": 0.00326},   # late moves 0, mixed waves 0
        "flat": {"flat": 0.929},   # late moves 0, mixed waves 0
        "sink": {"o": 1.59e-11, "rel": 4.11e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0123, "rel": 0.0014, "spread": 0.00588},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0122, "rel": 0.00214, "spread": 0.00396},   # late moves 0, mixed waves 0
        "late_60": {"o": 0.0151, "rel": 0.000852, "spread": 0.00475},   # late moves 0, mixed waves 0
        "mixed": {"o": 0.0138, "rel": 0.0022, "spread": 0.00617},   # late moves 0, mixed waves 0
    },
    "ring72w4": {
        "random": {"o": 0.0171, "rel": 0.00285, "spread": 0.00921},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0148, "rel": 0.00345, "spread": 0.00316},   # late moves 0, mixed waves 0
        "flat": {"flat": 0.929},   # late moves 0, mixed waves 0
        "sink": {"o": 1.14e-11, "rel": 3.11e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0111, "rel": 0.0022, "spread": 0.00472},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0126, "rel": 0.00252, "spread": 0.00594},   # late moves 0, mixed waves 0
        "late_60": {"o": 0.0133, "rel": 0.00136, "spread": 0.00539},   # late moves 0, mixed waves 0
        "mixed": {"o": 0.0163, "rel": 0.00387, "spread": 0.00464},   # late moves 0, mixed waves 0
    },
    "ring128": {
        "random": {"o": 0.018, "rel": 0.003, "spread": 0.0153},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0193, "rel": 0.00437, "spread": 0.00609},   # late moves 1621, mixed waves 580
        "flat": {"flat": 0.992},   # late moves 0, mixed waves 0
        "sink": {"o": 1.37e-11, "rel": 2.91e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0204, "rel": 0.00477, "spread": 0.00824},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0173, "rel": 0.0026, "spread": 0.0157},   # late moves 790, mixed waves 14
        "late_60": {"o": 0.0178, "rel": 0.00214, "spread": 0.00756},   # late moves 3152, mixed waves 56
        "mixed": {"o": 0.0166, "rel": 0.0026, "spread": 0.00941},   # late moves 600, mixed waves 42
    },
    "ring128nolazy": {
        "random": {"o": 0.0181, "rel": 0.00285, "spread": 0.0146},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0174, "rel": 0.00319, "spread": 0.00351},   # late moves 0, mixed waves 0
        "flat": {"flat": 0.992},   # late moves 0, mixed waves 0
        "sink": {"o": 1.05e-11, "rel": 2.77e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0163, "rel": 0.00273, "spread": 0.00727},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0164, "rel": 0.00243, "spread": 0.0112},   # late moves 0, mixed waves 0
        "late_60": {"o": 0.0195, "rel": 0.00227, "spread": 0.00866},   # late moves 0, mixed waves 0
        "mixed": {"o": 0.0154, "rel": 0.00239, "spread": 0.00766},   # late moves 0, mixed waves 0
    },
    "ring128k2": {
        "random": {"o": 0.018, "rel": 0.00241, "spread": 0.0176},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0201, "rel": 0.00352, "spread": 0.00481},   # late moves 3558, mixed waves 1146
        "flat": {"flat": 0.992},   # late moves 0, mixed waves 0
        "sink": {"o": 1.31e-11, "rel": 3.18e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0218, "rel": 0.00443, "spread": 0.0111},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0167, "rel": 0.00242, "spread": 0.0117},   # late moves 790, mixed waves 14
        "late_60": {"o": 0.0189, "rel": 0.00201, "spread": 0.0126},   # late moves 3152, mixed waves 56
        "mixed": {"o": 0.0168, "rel": 0.0037, "spread": 0.0112},   # late moves 600, mixed waves 42
        "group0": {"o": 0.0158, "rel": 0.00212, "spread": 0.00798},   # late moves 1940, mixed waves 32
        "group1": {"o": 0.0189, "rel": 0.00217, "spread": 0.0104},   # late moves 2648, mixed waves 64
    },
    "res64w8": {
        "random": {"o": 0.0184, "rel": 0.00377, "spread": 0.0104},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0235, "rel": 0.0055, "spread": 0.00634},   # late moves 69613, mixed waves 24001
        "flat": {"flat": 0.759},   # late moves 0, mixed waves 0
        "sink": {"o": 1.09e-11, "rel": 2.9e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0204, "rel": 0.00492, "spread": 0.00442},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.013, "rel": 0.00254, "spread": 0.00388},   # late moves 4146, mixed waves 0
        "late_60": {"o": 0.0167, "rel": 0.00149, "spread": 0.00503},   # late moves 16584, mixed waves 0
        "mixed": {"o": 0.0156, "rel": 0.0028, "spread": 0.00511},   # late moves 3123, mixed waves 195
    },
    "res64w9": {
        "random": {"o": 0.0212, "rel": 0.0038, "spread": 0.0133},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0238, "rel": 0.00431, "spread": 0.00746},   # late moves 71481, mixed waves 25672
        "flat": {"flat": 0.759},   # late moves 0, mixed waves 0
        "sink": {"o": 1.11e-11, "rel": 2.81e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0203, "rel": 0.0064, "spread": 0.0044},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0163, "rel": 0.00258, "spread": 0.00662},   # late moves 5260, mixed waves 0
        "late_60": {"o": 0.016, "rel": 0.000748, "spread": 0.0057},   # late moves 21040, mixed waves 0
        "mixed": {"o": 0.0164, "rel": 0.0025, "spread": 0.00545},   # late moves 3960, mixed waves 249
    },
    "res72w8": {
        "random": {"o": 0.0214, "rel": 0.00357, "spread": 0.0117},   # late moves 0, mixed waves 0
        "boosted": {"o": 0.0233, "rel": 0.0041, "spread": 0.00837},   # late moves 69757, mixed waves 23982
        "flat": {"flat": 0.759},   # late moves 0, mixed waves 0
        "sink": {"o": 1.19e-11, "rel": 3.72e-12, "spread": 0},   # late moves 0, mixed waves 0
        "late_under8": {"o": 0.0188, "rel": 0.00657, "spread": 0.0044},   # late moves 0, mixed waves 0
        "late_over8": {"o": 0.0117, "rel": 0.00239, "spread": 0.00499},   # late moves 4146, mixed waves 0
        "late_60": {"o": 0.0157, "rel": 0.00078, "spread": 0.00619},   # late moves 16584, mixed waves 0
        "mixed": {"o": 0.0133, "rel": 0.00248, "spread": 0.00631},   # late moves 3123, mixed waves 195
    },
}


def tolerances(form, family):
    if family == "flat":
        return {"flat": FLAT_BOUND}
    t = SPREAD[form][family]
    return {"o": FACTOR * t["o"], "rel": min(TODAY_REL, max(BF16_REL, FACTOR * t["rel"])), "spread": min(TODAY_ATOL, max(BF16_ATOL, FACTOR * t["spread"]))}


def capped():
    """the (form, family, measure) whose 2 x SPREAD exceeds today's test_attention line: the bound stays at that line"""
    return sorted((fo, fa, k) for fo, t in SPREAD.items() for fa, e in t.items() for k, line in (("rel", TODAY_REL), ("spread", TODAY_ATOL))
                  if k in e and FACTOR * e[k] > line)


def measure(form, family, stats=None):
    out, late, mixed = {}, 0, 0
    for c in cases_of(form, family):
        st = {}
        for k, v in errors(c, emu32(c, stats=st), ref64(c)).items():
            out[k] = max(out.get(k, 0.0), v)
        late, mixed = late + st["late_moves"], mixed + st["mixed_waves"]
    if stats is not None:
        stats.update(late_moves=late, mixed_waves=mixed)
    return out


def _fmt(d):
    return "{" + ", ".join(f'"{k}": {v:.3g}' for k, v in sorted(d.items())) + "}"


if __name__ == "__main__":
    print("SPREAD = {")
    for form in FORMS:
        print(f'    "{form}": {{')
        for fam in FAMILIES + (K2_FAMILIES if FORMS[form]["kg"] == 2 else ()):
            st = {}
            print(f'        "{fam}": {_fmt(measure(form, fam, st))},   # late moves {st["late_moves"]}, mixed waves {st["mixed_waves"]}')
        print("    },")
    print("}")
