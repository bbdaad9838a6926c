"""CPU: the tolerance table of tests/test_extend_attn_gpu.py is what the fp32 emulation of the kernel's documented roundings measures against the
float64 reference (extend_attn_ref.py) -- not a number taken from a kernel's output, and not a stale or padded one; the properties of the
reference and the case builder the GPU tests lean on; the planner (emmax_extend_attn_plan, host only) and the closure of the cases' plan tags;
the new entry points in the header and the binding, at ABI 12."""

import ctypes as C
import math
import os
import re

import pytest
import torch

import extend_attn_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"emmax_extend": 8, "emmax_slot_extend": 6, "emmax_session_context": 5, "emmax_op_extend_attention": 22, "emmax_op_extend_attention_kv8": 24,
               "emmax_op_rope_kv_write_at": 21, "emmax_extend_attn_plan": 12}


@pytest.fixture(scope="module")
def lib():
    from emmax import _lib

    return _lib, _lib.load()


def plan(so, B, max_n, max_L, Hq, Hkv, nsplit=0, kv8=0):
    """(G, tokens per block, query tiles, splits, split form) or None where the call refuses"""
    o = [C.c_int(-7) for _ in range(5)]
    if so.emmax_extend_attn_plan(B, max_n, max_L, Hq, Hkv, nsplit, kv8, *[C.byref(x) for x in o]) != 0:
        return None
    return tuple(x.value for x in o)


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", X.KINDS)
def test_tolerance_table_matches_the_emulation(kind):
    m = X.measure(kind)
    for form in ("split", "direct"):
        table = X.SPREAD[kind][form]
        assert set(m[form]) == set(table), (kind, form)
        for k, v in m[form].items():
            # 5 % for another BLAS's summation order; the table may not be padded: a measurement sits at 2/3 of its entry at least
            assert v <= 1.05 * table[k] + 1e-9, (kind, form, k, v, table[k])
            if table[k] > 1e-6:
                assert v >= 0.66 * table[k], (kind, form, k, v, table[k])


def test_bounds_are_twice_the_spread_and_only_bf16_rows_have_a_floor():
    assert X.FACTOR == 2.0
    for kind in X.KINDS:
        t = X.tolerances(kind, True)
        s = X.SPREAD[kind]["split"]
        assert t["po"] == 2 * s["po"] and t["plse"] == 2 * s["plse"] and t["o"] == 2 * s["o"]   # the fp32 partials: no floor
        assert t["plse"] < 1e-6 and t["po"] < 5e-2
        for split in (True, False):
            t = X.tolerances(kind, split)
            s = X.SPREAD[kind]["split" if split else "direct"]
            assert t["spread"] == max(4e-3, 2 * s["spread"]) and t["rel"] == max(8e-3, 2 * s["rel"])


# ---- the reference and the cases ----------------------------------------------------------------------------------------------------------------
def test_split_ranges_follow_the_kernels_rule():
    assert X.split_range(1, 2, 0) == (0, 1) and X.split_range(1, 2, 1)[0] >= 1          # one key: the second split is empty
    assert X.split_range(329, 3, 0) == (0, 112) and X.split_range(329, 3, 2) == (224, 329)
    for L in (1, 2, 65, 129, 1028):
        for ns in (1, 2, 3, 16):
            ends = [X.split_range(L, ns, s) for s in range(ns)]
            assert ends[0][0] == 0 and max(e[1] for e in ends) == L and all(e[0] % 16 == 0 for e in ends)
            assert all(a[1] == b[0] for a, b in zip(ends, ends[1:]) if b[0] < L)


@pytest.mark.parametrize("kind", X.KINDS)
def test_cache_is_nan_wherever_no_row_reads(kind):
    c = X.edge_case(kind, 2)
    used = set()
    for b in range(c.B):
        L = c.base[b] + c.n[b]
        for t0 in range(0, L, X.PAGE):
            pg, n = int(c.table[b, t0 // X.PAGE]), min(X.PAGE, L - t0)
            used.add(pg)
            live = c.kc[pg, :, :n]
            assert not (torch.isnan(live.float()).any() if kind == "bf16" else torch.isnan(c.ks[pg, :, :n]).any())
            if kind == "bf16":
                assert torch.isnan(c.kc[pg, :, n:].float()).all() and torch.isnan(c.vc[pg, :, n:].float()).all()
            else:
                assert (c.kc[pg, :, n:] == 0x7F).all() and torch.isnan(c.ks[pg, :, n:]).all() and torch.isnan(c.vs[pg, :, n:]).all()
    for pg in range(c.n_pages):
        if pg not in used:
            assert torch.isnan(c.kc[pg].float()).all() if kind == "bf16" else ((c.vc[pg] == 0x7F).all() and torch.isnan(c.vs[pg]).all())
    assert not torch.equal(c.table, torch.arange(c.n_pages, dtype=torch.int32).view(c.B, c.max_pages))   # not the identity
    assert int(c.table.min()) >= 0 and int(c.table.max()) < c.n_pages and c.table.unique().numel() == c.n_pages   # unused entries: valid ids


def test_the_cases_hold_what_the_issue_lists():
    pairs = set(X.EDGE)
    assert {b for b, _ in pairs} >= {0, 1, 63, 64, 65, 127, 128, 200} and {n for _, n in pairs} >= {1, 2, 31, 32, 33, 63, 64, 65, 129}
    assert (1025, 3) in pairs and any(b == 0 and n > 64 for b, n in pairs)
    assert len(set(X.RAGGED)) == 3 and set(X.NSPLITS) == {0, 1, 2, 3}
    assert X.split_range(1, 2, 1)[0] >= 1 and (0, 1) in pairs   # a split left empty
    assert set(X.HEADS) >= {1, 2, 4}


def test_ref64_is_a_causal_softmax_over_the_rows_own_keys():
    c = X.build("bf16", 2, ((3, 2), (0, 3)), 11, max_pages=1)
    o, lse = X.ref64(c)
    # row 0 of sequence 1 (base 0): one key -- the value itself; sequence 0, row 1: keys 0 .. 4
    assert torch.allclose(o[2], c.vd[1][0].double().repeat_interleave(2, dim=0))
    q, k, v = c.q[1, 0].double(), c.kd[0][:, 0].double(), c.vd[0][:, 0].double()
    w = torch.softmax((k @ q) * X.SCALE, dim=0)
    assert torch.allclose(o[1, 0], w @ v) and math.isclose(lse[1, 0].item(), torch.logsumexp((k @ q) * X.SCALE, 0).item(), rel_tol=1e-12)
    # one split and three splits of the emulation agree with it far inside the table
    for ns in (1, 3):
        e = X.errors(c, X.emu32(c, ns), (o, lse), ns > 1)
        assert e["rel"] < 8e-3 and e["o"] < 0.05


# ---- the planner --------------------------------------------------------------------------------------------------------------------------------
PLAN_HEADS = [(32, 32), (32, 8), (32, 4), (4, 2), (8, 1), (2, 2), (8, 2)]


def test_planner_follows_its_rule_and_every_plan_has_a_case(lib):
    _, so = lib
    tags = X.case_plans()
    seen = set()
    for Hq, Hkv in PLAN_HEADS:
        G = Hq // Hkv
        for B in (1, 2, 3, 8, 23, 64):
            for max_n in (1, 8, 31, 32, 33, 64, 128, 129, 700):
                for base in (0, 1, 63, 768, 1300):
                    for kv8 in (0, 1):
                        for ns in (0, 1, 2, 3, 16):
                            p = plan(so, B, max_n, base + max_n, Hq, Hkv, ns, kv8)
                            want = X.expected_nsplit(B, max_n, base + max_n, Hq, Hkv, ns)
                            assert p == (G, 128 // G, -(-max_n // (128 // G)), want, 1 if want > 1 else 0), (Hq, Hkv, B, max_n, base, kv8, ns, p)
                            seen.add(X.plan_tag(G, kv8, want > 1))
    assert seen <= tags, sorted(seen - tags)   # CLOSURE: every plan the planner can return is the tag of a GPU case
    assert tags == {X.plan_tag(G, kv8, sp) for G in (1, 2, 4, 8) for kv8 in (0, 1) for sp in (0, 1)}
    # the common case: a short extension over a long prefix is split; once the items fill the chip, one split
    assert plan(so, 1, 32, 800, 32, 32)[3] == 8 and plan(so, 8, 128, 896, 32, 32)[3] == 1 and plan(so, 1, 8, 776, 32, 8)[3] == 13
    assert plan(so, 1, 1, 1, 32, 32)[3] == 1   # never finer than a page
    # refusals
    assert plan(so, 0, 1, 1, 2, 2) is None and plan(so, 65, 1, 1, 2, 2) is None and plan(so, 1, 0, 5, 2, 2) is None and plan(so, 1, 5, 4, 2, 2) is None
    assert plan(so, 1, 1, 1, 3, 1) is None and plan(so, 1, 1, 1, 4, 3) is None and plan(so, 1, 1, 1, 2, 2, 17) is None


# ---- bindings -----------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported_at_abi_12(lib):
    _lib, so = lib
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "emmax.h")).read())
    assert "#define EMMAX_ABI_VERSION 12" in flat and _lib.ABI_VERSION == 12 and so.emmax_abi_version() == 12
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, flat)
        assert m and name in _lib.SIGNATURES and hasattr(so, name), name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]) and _lib.SIGNATURES[name][0] is C.c_int, name
