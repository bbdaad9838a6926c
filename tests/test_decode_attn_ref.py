"""CPU: the tolerance table of tests/test_decode_attn_forms_gpu.py is what the fp32 emulation of the documented roundings measures against the
float64 reference (decode_attn_ref.py) -- not a number taken from a kernel's output, and not a stale or padded one.  Plus the properties of the
reference and of the case builder the GPU tests lean on."""

import math

import pytest
import torch

import decode_attn_ref as R


def _pinned(measured, table, what):
    assert set(measured) == set(table), (what, sorted(measured), sorted(table))
    for k, v in measured.items():
        # 5 % for another BLAS's summation order; the table may not be padded: a measurement sits at 2/3 of its entry at least
        assert v <= 1.05 * table[k] + 1e-9, (what, k, v, table[k])
        if table[k] > 1e-6:
            assert v >= 0.66 * table[k], (what, k, v, table[k])


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_tolerance_table_matches_the_emulation(kind, family):
    m = R.measure_edge(kind, family)
    for form in ("split", "direct"):
        _pinned(m[form], R.SPREAD[kind][form][family], (kind, form, family))


@pytest.mark.parametrize("family", R.GROUP_FAMILIES)
@pytest.mark.parametrize("kind", ("bf16", "fp8"))
def test_grouped_tolerances_match_the_emulation(kind, family):
    _pinned(R.measure_group(kind, family), R.GROUP_SPREAD[kind][family], (kind, family))


@pytest.mark.parametrize("kind", R.KINDS)
def test_page_table_tolerances_match_the_emulation(kind):
    m = R.measure_table(kind)
    for form in ("split", "direct"):
        _pinned(m[form], R.TABLE_SPREAD[kind][form], (kind, form))


def test_by_shape_tolerances_match_the_emulation():
    m = R.measure_shape()
    for form in ("split", "direct"):
        _pinned(m[form], R.SHAPE_SPREAD[form], ("by shape", form))


def test_bounds_are_twice_the_spread_and_only_bf16_rows_have_a_floor():
    assert R.FACTOR == 2.0
    for kind in R.KINDS:
        for fam in R.FAMILIES:
            t = R.tolerances(kind, "split", fam)   # fp32 partials, whatever the cache: no floor
            assert t == {k: 2.0 * v for k, v in R.SPREAD[kind]["split"][fam].items()} and "spread" not in t
            assert max(t["lse"], t["on"]) < 1e-3 and t["o"] < 2e-4
            d = R.tolerances(kind, "direct", fam)
            if kind in ("bf16", "fp8"):
                assert d["spread"] == max(4e-3, 2 * R.SPREAD[kind]["direct"][fam]["spread"]) and d["rel"] == max(8e-3, 2 * R.SPREAD[kind]["direct"][fam]["rel"])
            else:
                assert d == {k: 2.0 * v for k, v in R.SPREAD[kind]["direct"][fam].items()} and d["o"] < 2e-4
    for kind in ("bf16", "fp8"):
        for fam in R.GROUP_FAMILIES:
            assert R.tolerances(kind, "group", fam)["spread"] >= 4e-3


def test_split_ranges_follow_the_kernels_rule():
    assert R.split_range(1, 16, 0) == (0, 1) and all(R.split_range(1, 16, s)[0] >= 1 for s in range(1, 16))    # L = 1: fifteen empty splits
    assert R.split_range(16, 2, 0) == (0, 16) and R.split_range(16, 2, 1) == (16, 16)                            # L = 16 at two: the second is empty
    assert R.split_range(17, 2, 1) == (16, 17)                                                                   # L = 17: exactly the new key
    assert R.split_range(33, 2, 1) == (32, 33)                                                                   # ctx = 32 at two splits: again the new key alone
    assert R.split_range(1025, 8, 7) == (1008, 1025) and R.split_range(1000, 4, 3) == (768, 1000)


@pytest.mark.parametrize("kind", R.KINDS)
def test_cache_is_nan_wherever_no_row_reads(kind):
    c = R.build(kind, "random", 4, 2, [0, 63, 64, 130], seed=3)
    used = torch.zeros(c.n_pages, c.page, dtype=torch.bool)
    for b, ctx in enumerate(c.ctxs):
        n = ctx if kind == "fp8" else ctx + 1   # fp8: position ctx waits in the staging row
        for t in range(n):
            used[int(c.table[b, t // c.page]), t % c.page] = True
    assert 0 <= int(c.table.min()) and int(c.table.max()) < c.n_pages and len(set(c.table.flatten().tolist())) == c.table.numel()
    if kind == "fp8":
        assert (c.kc[~used[:, None].expand(-1, c.Hkv, -1)] == 0x7F).all() and torch.isnan(c.ks[~used[:, None].expand(-1, c.Hkv, -1)]).all()
        assert torch.isfinite(c.ks[used[:, None].expand(-1, c.Hkv, -1)]).all()
    else:
        nan = torch.isnan(c.kc.float()).all(dim=-1)   # [pages, Hkv, page]
        assert torch.equal(nan, ~used[:, None].expand(-1, c.Hkv, -1)) and torch.equal(torch.isnan(c.vc.float()).all(dim=-1), nan)


@pytest.mark.parametrize("family,margin", [("sink", 30.0), ("last", 30.0), ("one_split", 110.0)])
def test_planted_keys_dominate_by_the_margin_and_stay_exact_bf16(family, margin):
    for G, (Hq, Hkv) in R.HEADS.items():
        ctxs = [100, 17, 1024]
        q, K, V = R.make_inputs("bf16", family, Hq, Hkv, ctxs, seed=G)
        for b, ctx in enumerate(ctxs):
            pos = {"sink": 0, "last": ctx, "one_split": ctx // 2}[family]
            assert torch.equal(K[b], R.bf(K[b])) and torch.equal(q[b], R.bf(q[b]))
            s = torch.einsum("hd,lhd->hl", q[b].double(), K[b].double().repeat_interleave(G, dim=1)) * R.SCALE
            rest = torch.cat([s[:, :pos], s[:, pos + 1:]], dim=1).max(dim=1).values
            gap = s[:, pos] - rest
            assert gap.min() >= margin and gap.min() < 2 * margin + 40, (family, G, b, gap.min().item(), gap.max().item())
    if family == "one_split":
        assert math.exp(-110.0) < 2.0 ** -149   # every other split's merge weight is 0 in fp32


def test_flat_low_and_offset_are_what_they_say():
    c = R.build("bf16", "flat", 4, 2, [40, 200], seed=1)
    ref = R.ref64(c)
    for b in range(2):
        assert torch.allclose(ref[b], c.vd[b].double().mean(0).repeat_interleave(2, dim=0), rtol=0, atol=1e-12)   # the plain mean of V
    lse, _ = R.ref_partials64(c, 4)
    for s in range(4):
        k0, k1 = R.split_range(201, 4, s)
        assert torch.allclose(lse[1, :, s], torch.full((4,), math.log(k1 - k0), dtype=torch.float64))   # l = the split's key count, m = 0
    c = R.build("bf16", "low", 4, 2, [300], seed=2)
    lse, _ = R.ref_partials64(c, 1)
    assert (lse < -50).all() and (lse > -60).all()   # m near -60, log l up to log 301
    c = R.build("bf16", "offset", 4, 2, [300], seed=2)
    assert (R.ref64(c) > 950).all() and (R.ref64(c) < 1050).all()


def test_the_emulation_reproduces_done_rows_and_empty_splits():
    c = R.build("bf16", "random", 4, 2, [0, 15, 16, 300], seed=9, done=(1,))
    e = R.emu32(c, dict(nsplit=16))
    lse, on = R.ref_partials64(c, 16)
    assert torch.equal(torch.isinf(e["lse"]), torch.isinf(lse)) and torch.isinf(lse[1]).all() and torch.isinf(lse[0, :, 1:]).all()
    assert (e["o"][1] == 0).all() and (R.ref64(c)[1] == 0).all()
    assert R.errors(c, dict(nsplit=16), e)["o"] < 1e-5
