"""CPU: the bounds of tests/gemm_ref.py are what its fp32 emulation measures against float64 on every case's own inputs, and the obvious errors,
planted into that emulation, miss them.  No GPU, no kernel output: only the parts of a plan (for the planted offset errors) come from the
library's host-only launch list."""

import pytest
import torch

import gemm_ref as G
import prefill_stage_ref as P

MEASURED = [(c, f) for c, f in G.ITEMS if f != "ties" and not c.same_as]


@pytest.fixture(scope="module")
def L():
    from emmax import _lib

    _lib.load()
    return _lib


def test_the_table_has_an_entry_for_every_bounded_case_and_no_other():
    assert set(G.SPREAD) == {(c.name, f) for c, f in MEASURED}
    assert len(G.FORMS) == 52


@pytest.mark.parametrize("c,family", MEASURED, ids=[f"{c.name}-{f}" for c, f in MEASURED])
def test_bound_is_the_measured_one(c, family):
    """the re-measured spread stays within the table (at most 1.05 x its entry, at least 2 / 3 of it); the emulation itself passes the bound; the
    bound nowhere exceeds the line tests/test_ops_gpu.py draws today (rtol 1e-2 / atol_frac 4e-3 for bf16, 1e-4 for fp32)"""
    s, worst, line = G.measure(c, family)
    t = G.SPREAD[(c.name, family)]
    assert 2.0 / 3.0 * t <= s <= 1.05 * t, (c.name, family, s, t)
    assert worst <= 1.0, (c.name, family, worst)
    assert line <= 1.0, f"{c.name} {family}: the bound is {line:.3g} x today's line: an emulation that needs more is wrong"
    if family == "random" and c.f32:   # the fp32 bounds are in units of a product term of rms ~ 1
        o = G.operands(c, family, G.sample_rows(c))
        unit = G.reference(c, o)[1].pow(2).mean().sqrt().item()
        assert 0.3 < unit < 4.0, (c.name, unit)


def ties_bits(c, plant=""):
    o = G.operands(c, "ties")
    ref, _ = G.reference(c, o)
    exact = ref.float()
    assert torch.equal(exact.double(), ref), c.name   # exactly representable
    stored, _ = G.emulate(c, o, plant)
    want = exact.view(torch.int32) if c.f32 else P.bf16_bits_rne(exact)
    got = stored.view(torch.int32) if c.f32 else P.bf16_bits_rne(stored)
    on_tie = int(((exact.view(torch.int32) & 0xFFFF) == 0x8000).sum())
    beside = int(((exact.view(torch.int32) & 0xFFFF) % 0x8000 != 0).sum())
    return int((got != want).sum()), on_tie, beside


def test_ties_family_is_exact_and_sits_on_and_beside_bf16_ties():
    n_tie = 0
    for c, f in G.ITEMS:
        if f != "ties" or c.M * c.N > 2 ** 18:
            continue
        wrong, on_tie, beside = ties_bits(c)
        assert wrong == 0, c.name            # the emulation, in its own summation order, lands on the exact value: every fp32 step is exact
        if not c.f32 and c.K >= 192:
            assert on_tie > 0 and beside > 0, (c.name, on_tie, beside)
            n_tie += on_tie
    assert n_tie > 1000


def misses(L, c, family, plant):
    if family == "ties":
        return ties_bits(c, plant)[0] > 0
    r0 = n1 = 0
    if c.kind in ("ROWS", "COLS", "HYBRID"):
        with L.tuning(**dict(c.tune)):
            r0, n1 = G.parts(G.launches(L, c))
    return G.measure(c, family, plant, r0, n1)[1] > 1.0


@pytest.mark.parametrize("plant", sorted(G.PLANTS))
def test_planted_error_misses_the_bound_in_every_family_it_concerns(L, plant):
    concerned = [c for c in G.CASES if G.PLANTS[plant](c) and not c.same_as]
    assert concerned, plant
    fams = sorted({f for c in concerned for f in c.families})
    for fam in fams:
        cases = sorted((c for c in concerned if fam in c.families), key=lambda c: c.M * c.N * c.K)
        assert any(misses(L, c, fam, plant) for c in cases), f"planted `{plant}` passes every {fam} case"


def test_planted_errors_change_most_cases_they_concern(L):
    """not one lucky case: the cheap plants miss the bound on every small `random` case they concern"""
    for plant in ("trunc", "drop_chunk", "swap_gate_up", "drop_mean", "bias_after_gelu", "scale_on_res", "round_before_res"):
        for c in G.CASES:
            if G.PLANTS[plant](c) and not c.same_as and not c.kind and c.M * c.N <= 2 ** 17 and c.M > 1:
                assert misses(L, c, "random", plant), (plant, c.name)
