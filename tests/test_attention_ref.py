"""CPU: the tolerance table of tests/test_attention_forms_gpu.py is what the fp32 emulation of the documented roundings measures against the float64
reference (attention_ref.py) -- not a number taken from a kernel's output, and not a stale or padded one -- and the bounds it gives are SENSITIVE:
mutants of the emulation (the ways a ring / resident attention kernel goes subtly wrong) exceed them on named cases.  Plus the properties of the
case builder the GPU tests lean on: the margins of the planted keys, the late moves of the lazy forms, the NaN poison."""

import math

import pytest
import torch

import attention_ref as R


def _families(form):
    return R.FAMILIES + (R.K2_FAMILIES if R.FORMS[form]["kg"] == 2 else ())


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(R.FORMS))
def test_tolerance_table_matches_the_emulation_and_lazy_forms_move_late(form):
    assert set(R.SPREAD[form]) == set(_families(form))
    for family in _families(form):
        st = {}
        measured, table = R.measure(form, family, st), R.SPREAD[form][family]
        assert set(measured) == set(table), (form, family)
        for k, v in measured.items():
            # 5 % for another BLAS's summation order; the table may not be padded: a measurement sits at 2/3 of its entry at least
            assert v <= 1.05 * table[k] + 1e-9, (form, family, k, v, table[k])
            if table[k] > 1e-6:
                assert v >= 0.66 * table[k], (form, family, k, v, table[k])
        tol = R.tolerances(form, family)
        assert all(measured[k] <= tol[k] for k in tol), (form, family, measured, tol)   # the emulation itself passes the GPU's bound
        # the lazy reference maximum: plain and sink inputs never move it after a wave's first step, a key just under +8 does not either (P up to
        # 2^8 instead), the boosted and the planted families do -- and `mixed` inside waves whose other rows stay
        if R.FORMS[form]["lazy"]:
            if family in ("boosted", "late_over8", "late_60", "mixed") + R.K2_FAMILIES:
                assert st["late_moves"] > 0, (form, family, st)
            if family in ("random", "sink", "late_under8", "flat"):
                assert st["late_moves"] == 0, (form, family, st)
            if family in ("mixed", "boosted"):
                assert st["mixed_waves"] > 0, (form, family, st)
        else:
            assert st == dict(late_moves=0, mixed_waves=0)


def test_every_lazy_case_of_the_moving_families_moves_late():
    for form in R.LAZY_FORMS:
        for family in ("boosted", "late_over8", "late_60", "mixed"):
            for c in R.cases_of(form, family):
                if "items" in c.name:
                    continue   # (the same family at 272 / 528 items: counted with its (form, family) above)
                st = {}
                R.emu32(c, stats=st)
                assert st["late_moves"] > 0, (c.name, st)


def test_bounds_are_twice_the_spread_between_the_bf16_line_and_todays_line():
    assert R.FACTOR == 2.0 and (R.BF16_RTOL, R.BF16_ATOL, R.BF16_REL) == (1e-2, 4e-3, 8e-3) and (R.TODAY_REL, R.TODAY_ATOL) == (1e-2, 2e-2)
    for form in R.FORMS:
        for fam in _families(form):
            t, s = R.tolerances(form, fam), R.SPREAD[form][fam]
            if fam == "flat":
                assert t == {"flat": R.FLAT_BOUND} and s["flat"] <= 1.0   # the emulation: within half a bf16 ulp of the exact count ratio
                continue
            assert t["o"] == 2.0 * s["o"] and t["o"] < 0.06
            assert t["rel"] == min(1e-2, max(8e-3, 2 * s["rel"])) and t["spread"] == min(2e-2, max(4e-3, 2 * s["spread"]))
            assert t["rel"] <= R.TODAY_REL and t["spread"] <= R.TODAY_ATOL   # no family is looser than test_ops_gpu.py::test_attention
    # where twice the spread would pass today's line the bound stays AT that line.  `spread` of the causal and the long cases: P is rounded to bf16
    # for the PV product, and an output that cancels to ~0 carries 2^-9 of its terms -- up to 1.6e-2 rms(sequence) in the emulation already;
    # `rel` of late_under8 on the resident forms: P reaches 2^7.9 on the planted key, one bf16 ulp of it is 2^-8 of the whole row
    capped = R.capped()
    assert {k for _, _, k in capped} <= {"rel", "spread"}
    for form, fam, k in capped:
        assert R.SPREAD[form][fam][k] < (R.TODAY_REL if k == "rel" else R.TODAY_ATOL), (form, fam, k)   # the emulation itself is inside the line


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------------
# mutant -> the cases that must kill it: (form, causal, family, heads) = the edge batch of that (form, family) under that mask
KILLS = {
    "drop_tile_last": [("ring64w3", 0, "flat", "g4"), ("ring128", 1, "late_60", "g4"), ("res72w8", 0, "late_under8", "kv1"), ("ring72w4", 0, "random", "g2"),
                       ("ring128nolazy", 1, "late_over8", "g1")],
    "double_tile_first": [("ring64w4", 0, "flat", "g4"), ("ring128k2", 1, "flat", "g4"), ("res64w8", 0, "flat", "g4"), ("ring72w3", 0, "boosted", "g1")],
    "diag_shift": [("ring64w3", 1, "flat", "g1"), ("ring72w4", 1, "random", "g2"), ("ring128", 1, "random", "g2"), ("ring128k2", 1, "flat", "g4"),
                   ("ring128nolazy", 1, "mixed", "kv1")],
    "skip_lazy_rescale": [("ring128", 1, "late_over8", "g1"), ("ring128", 1, "boosted", "g1"), ("ring128k2", 1, "late_60", "g4"), ("res64w8", 0, "late_over8", "g1"),
                          ("res64w9", 0, "boosted", "g1"), ("res72w8", 0, "late_60", "g4")],
    "wrong_row_alpha": [("ring128", 1, "mixed", "kv1"), ("ring128k2", 1, "mixed", "kv1"), ("res64w8", 0, "mixed", "kv1"), ("res64w9", 0, "mixed", "kv1"),
                        ("res72w8", 0, "mixed", "kv1")],
    "gqa_neighbour": [("ring128", 1, "sink", "g2"), ("ring64w3", 0, "random", "g2"), ("res72w8", 0, "random", "g4"), ("ring128k2", 1, "group1", "g4"),
                      ("ring72w4", 0, "sink", "g2")],
    "swap_merge": [("ring128k2", 1, "group0", "g2"), ("ring128k2", 1, "group1", "g4"), ("ring128k2", 1, "sink", "g2"), ("ring128k2", 1, "random", "kv1")],
    "stop_short": [("ring128nolazy", 1, "late_60", "g4"), ("ring72w3", 0, "flat", "g4"), ("res64w9", 0, "late_under8", "kv1"), ("ring64w4", 0, "random", "g1")],
}


def _case(form, causal, family, heads):
    return next(c for c in R.cases_of(form, family) if c.causal == causal and c.heads == heads)


def test_every_mutant_has_killers_and_every_family_kills():
    assert set(KILLS) == set(R.MUTANTS)
    killers = {fam for ks in KILLS.values() for _, _, fam, _ in ks}
    assert killers == set(R.FAMILIES + R.K2_FAMILIES), sorted(set(R.FAMILIES + R.K2_FAMILIES) - killers)   # a family that kills nothing has no place
    for mut in ("skip_lazy_rescale", "wrong_row_alpha"):
        assert {f for f, _, _, _ in KILLS[mut]} == set(R.LAZY_FORMS)   # on every form that has the lazy rule


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_mutants_exceed_the_bounds(mut):
    """The CPU proof that the GPU test fails on a subtly wrong kernel: the mutant's output, judged exactly as the GPU's is."""
    for key in KILLS[mut]:
        c = _case(*key)
        ref = R.ref64(c)
        assert not R.violations(c, R.emu32(c), ref), c.name
        v = R.violations(c, R.emu32(c, mut), ref)
        assert v, f"{mut} survives {c.name}"
        print(f"{mut} killed by {v[0]}")


# ---- the case builder --------------------------------------------------------------------------------------------------------------------------
def test_buffers_are_nan_wherever_the_kernel_must_not_read_or_write():
    for c in (_case("ring128", 1, "random", "g2"), _case("ring64w3", 0, "late_60", "g4"), _case("res72w8", 0, "mixed", "kv1")):
        qkv, cu, out, (q_off, k_off, v_off, ld, ld_out) = c.buffers()
        qd, kvd = c.Hq * c.hd, c.Hkv * c.hd
        used = torch.zeros(ld, dtype=torch.bool)
        for off, w in ((q_off, qd), (k_off, kvd), (v_off, kvd)):
            assert off % 8 == 0 and not used[off:off + w].any()
            used[off:off + w] = True
        assert ld % 8 == 0 and ld > max(q_off + qd, k_off + kvd, v_off + kvd) and ld_out % 4 == 0 and ld_out > qd
        assert qkv.shape == (c.total + 2, ld) and torch.isnan(qkv[0].float()).all() and torch.isnan(qkv[-1].float()).all()
        assert torch.isnan(qkv[1:-1, ~used].float()).all() and torch.isfinite(qkv[1:-1, used].float()).all()
        assert (out.view(torch.int16) == R.NAN_BITS).all() and out.shape == (c.total + 2, ld_out)
        assert cu.tolist() == [0] + torch.tensor(c.lens).cumsum(0).tolist() and 0 in c.lens and max(c.lens) == c.max_seqlen
    lays = {c.lay for c in R.all_cases()}
    assert lays == set(R.LAYOUTS) and R.layout("shift", 4, 2, 128)[0] != 0
    assert R.layout("vit", 16, 16, 64)[:3] == (0, 1024, 2048) and R.layout("llama", 32, 8, 128)[:3] == (0, 4096, 5120)


def test_edge_batches_hold_every_length_of_the_issue():
    want = {1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 261, 288, 289}
    assert set(R.EDGE) == want
    for form, f in R.FORMS.items():
        lens = {n for c in R.form_cases(form) for n in c.lens}
        top = f["tag"][6] if f["res"] else 289
        assert {n for n in want if n <= top} - lens <= ({289} if form in ("ring64w3", "ring72w3") else set()), (form, sorted(lens))   # 289 takes four waves
        assert 0 in lens
        if not f["res"]:
            assert max(lens) in (1024, 1025) and max(lens) < 1100
    assert {c.heads for c in R.all_cases() if isinstance(c.heads, str)} == {"g1", "g2", "g4", "kv1"}
    assert [h[0] // h[1] for h in R.HEADS.values()] == [1, 2, 4, 3] and R.HEADS["kv1"][1] == 1


@pytest.mark.parametrize("family", sorted(R.WINDOWS))
def test_planted_keys_sit_at_their_margins_and_stay_exact_bf16(family):
    """the exp2-domain margin of every planted key over its row's reference (the maximum of the row's first step in the form; sink / group*: every
    other key) lies in the family's window, for every row that sees it"""
    lo, hi = R.WINDOWS[family]
    forms = ("ring128k2",) if family in R.K2_FAMILIES else ("ring128", "ring128k2", "res64w9", "ring72w3")
    planted = 0
    for form in forms:
        c = R.cases_of(form, family)[0].build()
        rep, sc = c.Hq // c.Hkv, c.scale * R.LOG2E
        for b, n in enumerate(c.lens):
            pos = R.plant_pos(n, b, family)
            if n == 0:
                continue
            assert torch.equal(c.k[b], R.bf(c.k[b])) and torch.equal(c.q[b], R.bf(c.q[b]))
            if pos is None or n == 1:
                continue
            s = torch.einsum("nhd,mhd->hnm", c.q[b].double(), c.k[b].double().repeat_interleave(rep, dim=1)) * sc
            k0, k1 = (0, n) if family in ("sink",) + R.K2_FAMILIES else R.first_step_keys(form, pos)
            for r in range(n):
                if (c.causal and r < pos) or (family == "mixed" and r % 2):
                    continue
                top = min(k1, r + 1) if c.causal else k1
                keys = [j for j in range(k0, top) if j != pos]
                if keys:
                    marg = s[:, r, pos] - s[:, r, keys].max(dim=-1).values
                    assert marg.min() >= lo and marg.max() <= hi, (form, family, n, pos, r, marg)
                    planted += 1
            if family == "mixed":   # the odd rows look away
                odd = list(range(1, n, 2))
                assert (s[:, odd, pos] < s[:, odd, :min(32, n)].max(dim=-1).values).all()
    assert planted > 100
    assert R.WINDOWS["late_under8"][1] < 8.0 < R.WINDOWS["late_over8"][0] and R.WINDOWS["mixed"][0] > 8.0


def test_flat_shows_which_keys_were_summed():
    c = _case("ring64w3", 0, "flat", "g4").build()
    ref, o = R.ref64(c), 0
    for b, n in enumerate(c.lens):
        if n == 0:
            continue
        want = torch.zeros(64, dtype=torch.float64)
        for j in range(n):
            want[j % 64] += 2.0 ** (j // 64)
        assert torch.allclose(ref[o:o + n], (want / n).expand(n, c.Hq, 64), rtol=1e-13, atol=0)
        o += n
    c = _case("ring128", 1, "flat", "g4").build()
    ref = R.ref64(c)
    o = sum(c.lens[:c.lens.index(129)])
    assert math.isclose(ref[o + 5, 0, 5], 1 / 6, rel_tol=1e-13) and ref[o + 5, 0, 6] == 0
    assert math.isclose(ref[o + 128, 0, 0], 3 / 129, rel_tol=1e-13) and math.isclose(ref[o + 128, 0, 1], 1 / 129, rel_tol=1e-13)


def test_the_emulation_is_one_arithmetic_in_different_steps():
    """the same inputs through the 64-key step, the 32-key step, the lazy rule and the two key groups: all within a few bf16 ulps of the reference,
    none bit-equal to another by construction"""
    base = _case("ring128", 1, "boosted", "g1").build()
    ref = R.ref64(base)
    outs = {}
    for form in ("ring128", "ring128nolazy", "ring128k2"):
        c = R.Case(form, "boosted", "g1", base.lens, 1, base.lay, name=base.name)   # the same name: the same inputs
        c.build()
        assert all(torch.equal(a, b) for a, b in zip(c.q, base.q))
        outs[form] = R.emu32(c)
        assert R.errors(c, outs[form], ref)["o"] < 0.03
    assert not torch.equal(outs["ring128"], outs["ring128nolazy"]) and not torch.equal(outs["ring128"], outs["ring128k2"])
    assert math.isclose(float(2.0 ** -8), 0.00390625)
