"""CPU: the bounds of tests/score_ref.py are what its fp32 emulation measures against float64 on the cases' own inputs, the case generators keep
their promises on float64 alone, and the obvious errors, planted into that emulation, miss the bounds.  No GPU, no kernel output."""

import math

import pytest
import torch

import score_ref as S
from decode_attn_ref import FACTOR


@pytest.fixture(scope="module")
def table():
    return S.measure()


def test_the_table_is_the_measured_one(table):
    """every entry re-measured: at most 1.05 x the stored value, at least 2 / 3 of it (the rule of tests/test_gemm_ref.py)"""
    assert {(K, f) for K in S.SPREAD for f in S.SPREAD[K]} == {(K, f) for K in table for f in table[K]} == {(c.K, c.family) for c in S.CASES}
    for K, fams in table.items():
        for f, d in fams.items():
            for k, v in d.items():
                t = S.SPREAD[K][f][k]
                assert 2.0 / 3.0 * t <= v <= 1.05 * t, (K, f, k, v, t)


def test_bounds_are_twice_the_spread():
    assert FACTOR == 2.0
    for c in S.CASES:
        assert S.tolerances(c) == {k: 2.0 * v for k, v in S.SPREAD[c.K][c.family].items()}
        assert all(v > 0 for v in S.tolerances(c).values()), c.name


def test_the_cases_cover_the_shapes():
    assert {c.rows for c in S.CASES} >= set(S.ROWS)
    assert {(c.K, c.V, c.Np) for c in S.CASES if c.family == "random"} >= {(K, V, Np) for K in S.KS for V, Np in S.VOCABS}
    assert any(c.K == 4096 and c.rows == 128 and c.V == 384 for c in S.CASES)
    forced = {c.slices: S.case_plan(c) for c in S.CASES if c.name.startswith("random-r129-k128-v1000-s")}
    assert set(forced) == {0, 1, 2, 3, 8}
    assert forced[3] == (2, 8, 3, 3) and forced[2] == (2, 8, 2, 4) and forced[8] == (2, 8, 8, 1) and forced[1] == (2, 8, 1, 8)
    assert {c.family for c in S.CASES} == set(S.FAMILIES)
    assert {c.pad for c in S.CASES} == {"nan", "big"}
    for f in S.FAMILIES:
        assert {c.K for c in S.CASES if c.family == f} >= set(S.KS), f


@pytest.mark.parametrize("c", S.CASES, ids=[c.name for c in S.CASES])
def test_generator_conditions_on_ref64(c):
    o = S.operands(c)
    ref = S.ref64(c, o)
    rt, ct, slices, tps = S.case_plan(c)
    # poison: X rows behind `rows` up to the row tile, W rows in [V, Np)
    assert o.X.shape[0] == rt * 128 and torch.isfinite(o.X[:c.rows]).all() and (c.rows == rt * 128 or torch.isnan(o.X[c.rows:]).all())
    pad = o.W[c.V:]
    if c.family == "ties":   # one twin lives in the padding
        b = S.tie_pairs(c)[-1][1]
        assert c.V <= b < c.Np and torch.equal(o.W[b], o.W[S.tie_pairs(c)[-1][0]])
        pad = torch.cat([o.W[c.V:b], o.W[b + 1:]])
    assert torch.isnan(pad).all() if c.pad == "nan" else (pad == S.BIG).all()
    assert torch.isfinite(ref.lse).all()
    # targets: columns 0, 127, 128 (where the vocabulary has them), V - 1, both ends of every slice, and -100
    tg = set(o.targets.tolist())
    want = {0, c.V - 1} | {t for t in (127, 128) if t < c.V}
    for s in range(slices):
        want |= {s * tps * 128, min((s + 1) * tps * 128, c.V) - 1}
    if c.rows >= 2 * len(want) + 8:
        assert want <= tg and S.IGNORE in tg, (c.name, sorted(want - tg))
    assert all(t == S.IGNORE or 0 <= t < c.V for t in tg)
    # at least half of the rows clear the argmax margin (tie and all-zero rows are judged by their planted answer instead)
    e = S.errors(c, o, S.Got(ref.lse.float(), ref.logit.float(), ref.argmax), ref)
    assert e["argmax"] == 0 and e["planted"] == 0 and e["zero"] == 0
    assert 2 * e["clear"] >= c.rows, (c.name, e["clear"])
    if c.family == "large":   # a plain sum of exp(x) overflows fp32 in most rows
        assert (o.X[:c.rows].double() @ o.W[:c.V].double().T).max(dim=-1).values.gt(89.0).float().mean() > 0.5
    if c.family == "sink":
        sink = (c.seed * 37) % c.V
        assert (ref.argmax == sink).all() and (ref.margin > 20.0).all()
    if c.family == "flat":
        for r in o.flat_rows:
            assert ref.argmax[r] == 0 and abs(ref.lse[r].item() - math.log(c.V)) < 1e-12 and ref.margin[r] == 0
    if c.family == "ties":
        assert slices == 3 and tps == 3
        (a0, b0), (a1, b1), (a2, b2), (a3, b3) = S.tie_pairs(c)
        assert a0 // 16 == b0 // 16                                         # inside one MFMA tile
        assert a1 // 128 != b1 // 128 and a1 // 384 == b1 // 384            # two tiles of one slice
        assert a2 // 384 != b2 // 384                                       # two slices
        for r, (a, b) in enumerate(S.tie_pairs(c)):
            assert torch.equal(o.W[a], o.W[b]) and ref.argmax[r] == a and o.tie_rows[r] == a
            assert o.targets[r] == (b if b < c.V else a)
            if b < c.V:
                assert ref.margin[r] == 0


def test_the_emulation_passes_its_own_bounds():
    for c in S.CASES:
        o = S.operands(c)
        e = S.errors(c, o, S.emu32(c, o), S.ref64(c, o))
        assert S.within(c, e), (c.name, e)


@pytest.mark.parametrize("plant", S.PLANTS)
def test_planted_error_breaks_a_bound(plant):
    broken = []
    for c in S.CASES:
        if c.K > 256:
            continue
        o = S.operands(c)
        if not S.within(c, S.errors(c, o, S.emu32(c, o, plant), S.ref64(c, o))):
            broken.append(c.name)
    assert broken, f"planted `{plant}` passes every case"


def test_the_planner_restated():
    assert S.plan(768, 32000, 64 << 20) == (6, 250, 84, 3)
    assert S.plan(300, 1000, 1 << 20) == (3, 8, 8, 1)
    assert S.plan(129, 1000, 12 * 129 * 2) == (2, 8, 2, 4)      # the scratch caps the slices
    assert S.plan(129, 1000, 12 * 129 - 1) is None
    assert S.plan(129, 1000, 1 << 20, slices=9) is None
    assert S.plan(129, 1000, 1 << 20, slices=5) == (2, 8, 4, 2)  # 5 asked: 2 tiles per slice make 4
