"""CPU: which form of the decode attention a launch takes (emmax_decode_attn_plan / emmax_group_attn_plan: host only -- the launchers dispatch on
the structs these calls fill, so plan and launch cannot disagree).
  1. PINNED: the plan of every step of 1 .. 64 rows at five head shapes, under default tuning and six switch settings.
  2. every GPU case of tests/decode_attn_ref.py reaches the plan it is tagged with, under its own switches and at its own shape.
  3. CLOSURE: every plan a step can reach in those tables (bf16 and fp8 cache), and every group plan the grouped route can reach with N of 2, 3, 4,
     8 and 16, is the tag of at least one GPU case -- "every launched form" has a test.
"""

import ctypes as C

import pytest

import decode_attn_ref as R

HEADS = [(32, 32), (32, 8), (32, 4), (4, 2), (8, 1)]
TUNINGS = [{}, {"attn_nw": 0}, {"attn_nw": 8}, {"attn_deep": 0}, {"attn_deep": 1}, {"attn_direct": 0}, {"attn_nsplit": 4}]


@pytest.fixture(scope="module")
def lib():
    from emmax import _lib

    return _lib, _lib.load()


def attn_plan(so, B, Hq, Hkv, nsplit=0, direct=-1, kv8=0):
    """(G, nw, direct, deep, nsplit) or None where the call refuses"""
    o = [C.c_int(-7) for _ in range(5)]
    if so.emmax_decode_attn_plan(B, Hq, Hkv, nsplit, direct, kv8, *[C.byref(x) for x in o]) != 0:
        return None
    G, nw, d, deep, ns = [x.value for x in o]
    return (G, nw, d, deep, ns)


def group_plan(so, B, N, Hq, Hkv, kv8=0):
    """(span width, span splits, query chunks, tail G) or None"""
    o = [C.c_int(-7) for _ in range(4)]
    if so.emmax_group_attn_plan(B, N, Hq, Hkv, kv8, *[C.byref(x) for x in o]) != 0:
        return None
    return tuple(x.value for x in o)


def _key(t):
    return ",".join(f"{k}={v}" for k, v in t.items()) or "default"


# (first B, last B, (G, waves, direct, four chunks in flight, splits)): bf16 cache.  32 kv heads: 8 splits at 1 - 2 rows, 2 at 3 - 4, the one-split
# direct form from 5, four chunks in flight from 32 rows (1024 blocks); 8 / 4 kv heads reach one split at 17 / 33 rows; G >= 4 never has four chunks
PINNED = {
    ("default", (32, 32)): [(1, 2, (1, 4, 0, 0, 8)), (3, 4, (1, 4, 0, 0, 2)), (5, 31, (1, 4, 1, 0, 1)), (32, 64, (1, 4, 1, 1, 1))],
    ("default", (32, 8)): [(1, 4, (4, 4, 0, 0, 8)), (5, 8, (4, 4, 0, 0, 4)), (9, 16, (4, 4, 0, 0, 2)), (17, 64, (4, 4, 1, 0, 1))],
    ("default", (32, 4)): [(1, 8, (8, 4, 0, 0, 8)), (9, 16, (8, 4, 0, 0, 4)), (17, 32, (8, 4, 0, 0, 2)), (33, 64, (8, 4, 1, 0, 1))],
    ("default", (4, 2)): [(1, 16, (2, 4, 0, 0, 8)), (17, 32, (2, 4, 0, 0, 4)), (33, 64, (2, 4, 0, 0, 2))],
    ("default", (8, 1)): [(1, 32, (8, 4, 0, 0, 8)), (33, 64, (8, 4, 0, 0, 4))],
    ("attn_nw=0", (32, 32)): [(1, 2, (1, 4, 0, 0, 8)), (3, 4, (1, 4, 0, 0, 2)), (5, 8, (1, 8, 1, 0, 1)), (9, 31, (1, 4, 1, 0, 1)), (32, 64, (1, 4, 1, 1, 1))],
    ("attn_nw=0", (32, 8)): [(1, 4, (4, 4, 0, 0, 8)), (5, 8, (4, 4, 0, 0, 4)), (9, 16, (4, 4, 0, 0, 2)), (17, 32, (4, 8, 1, 0, 1)), (33, 64, (4, 4, 1, 0, 1))],
    ("attn_nw=0", (32, 4)): [(1, 8, (8, 4, 0, 0, 8)), (9, 16, (8, 4, 0, 0, 4)), (17, 32, (8, 4, 0, 0, 2)), (33, 64, (8, 8, 1, 0, 1))],
    ("attn_nw=0", (4, 2)): [(1, 16, (2, 4, 0, 0, 8)), (17, 32, (2, 4, 0, 0, 4)), (33, 64, (2, 4, 0, 0, 2))],
    ("attn_nw=0", (8, 1)): [(1, 32, (8, 4, 0, 0, 8)), (33, 64, (8, 4, 0, 0, 4))],
    ("attn_nw=8", (32, 32)): [(1, 2, (1, 4, 0, 0, 8)), (3, 4, (1, 4, 0, 0, 2)), (5, 31, (1, 8, 1, 0, 1)), (32, 64, (1, 4, 1, 1, 1))],
    ("attn_nw=8", (32, 8)): [(1, 4, (4, 4, 0, 0, 8)), (5, 8, (4, 4, 0, 0, 4)), (9, 16, (4, 4, 0, 0, 2)), (17, 64, (4, 8, 1, 0, 1))],
    ("attn_nw=8", (32, 4)): [(1, 8, (8, 4, 0, 0, 8)), (9, 16, (8, 4, 0, 0, 4)), (17, 32, (8, 4, 0, 0, 2)), (33, 64, (8, 8, 1, 0, 1))],
    ("attn_nw=8", (4, 2)): [(1, 16, (2, 4, 0, 0, 8)), (17, 32, (2, 4, 0, 0, 4)), (33, 64, (2, 4, 0, 0, 2))],
    ("attn_nw=8", (8, 1)): [(1, 32, (8, 4, 0, 0, 8)), (33, 64, (8, 4, 0, 0, 4))],
    ("attn_deep=0", (32, 32)): [(1, 2, (1, 4, 0, 0, 8)), (3, 4, (1, 4, 0, 0, 2)), (5, 64, (1, 4, 1, 0, 1))],
    ("attn_deep=0", (32, 8)): [(1, 4, (4, 4, 0, 0, 8)), (5, 8, (4, 4, 0, 0, 4)), (9, 16, (4, 4, 0, 0, 2)), (17, 64, (4, 4, 1, 0, 1))],
    ("attn_deep=0", (32, 4)): [(1, 8, (8, 4, 0, 0, 8)), (9, 16, (8, 4, 0, 0, 4)), (17, 32, (8, 4, 0, 0, 2)), (33, 64, (8, 4, 1, 0, 1))],
    ("attn_deep=0", (4, 2)): [(1, 16, (2, 4, 0, 0, 8)), (17, 32, (2, 4, 0, 0, 4)), (33, 64, (2, 4, 0, 0, 2))],
    ("attn_deep=0", (8, 1)): [(1, 32, (8, 4, 0, 0, 8)), (33, 64, (8, 4, 0, 0, 4))],
    ("attn_deep=1", (32, 32)): [(1, 2, (1, 4, 0, 1, 8)), (3, 4, (1, 4, 0, 1, 2)), (5, 64, (1, 4, 1, 1, 1))],
    ("attn_deep=1", (32, 8)): [(1, 4, (4, 4, 0, 0, 8)), (5, 8, (4, 4, 0, 0, 4)), (9, 16, (4, 4, 0, 0, 2)), (17, 64, (4, 4, 1, 0, 1))],
    ("attn_deep=1", (32, 4)): [(1, 8, (8, 4, 0, 0, 8)), (9, 16, (8, 4, 0, 0, 4)), (17, 32, (8, 4, 0, 0, 2)), (33, 64, (8, 4, 1, 0, 1))],
    ("attn_deep=1", (4, 2)): [(1, 16, (2, 4, 0, 1, 8)), (17, 32, (2, 4, 0, 1, 4)), (33, 64, (2, 4, 0, 1, 2))],
    ("attn_deep=1", (8, 1)): [(1, 32, (8, 4, 0, 0, 8)), (33, 64, (8, 4, 0, 0, 4))],
    ("attn_direct=0", (32, 32)): [(1, 2, (1, 4, 0, 0, 8)), (3, 4, (1, 4, 0, 0, 2)), (5, 31, (1, 4, 0, 0, 1)), (32, 64, (1, 4, 0, 1, 1))],
    ("attn_direct=0", (32, 8)): [(1, 4, (4, 4, 0, 0, 8)), (5, 8, (4, 4, 0, 0, 4)), (9, 16, (4, 4, 0, 0, 2)), (17, 64, (4, 4, 0, 0, 1))],
    ("attn_direct=0", (32, 4)): [(1, 8, (8, 4, 0, 0, 8)), (9, 16, (8, 4, 0, 0, 4)), (17, 32, (8, 4, 0, 0, 2)), (33, 64, (8, 4, 0, 0, 1))],
    ("attn_direct=0", (4, 2)): [(1, 16, (2, 4, 0, 0, 8)), (17, 32, (2, 4, 0, 0, 4)), (33, 64, (2, 4, 0, 0, 2))],
    ("attn_direct=0", (8, 1)): [(1, 32, (8, 4, 0, 0, 8)), (33, 64, (8, 4, 0, 0, 4))],
    ("attn_nsplit=4", (32, 32)): [(1, 7, (1, 4, 0, 0, 4)), (8, 64, (1, 4, 0, 1, 4))],
    ("attn_nsplit=4", (32, 8)): [(1, 64, (4, 4, 0, 0, 4))],
    ("attn_nsplit=4", (32, 4)): [(1, 64, (8, 4, 0, 0, 4))],
    ("attn_nsplit=4", (4, 2)): [(1, 64, (2, 4, 0, 0, 4))],
    ("attn_nsplit=4", (8, 1)): [(1, 64, (8, 4, 0, 0, 4))],
}


def _expand(segs):
    out = {}
    for b0, b1, p in segs:
        for B in range(b0, b1 + 1):
            assert B not in out
            out[B] = p
    assert sorted(out) == list(range(1, 65))
    return out


@pytest.mark.parametrize("tune", TUNINGS, ids=_key)
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: f"{h[0]}-{h[1]}")
def test_step_plans_are_pinned(lib, heads, tune):
    L, so = lib
    want = _expand(PINNED[(_key(tune), heads)])
    with L.tuning(**tune):
        for B in range(1, 65):
            assert attn_plan(so, B, *heads) == want[B], (B, heads, tune)
            # the fp8 cache: the same splits and the same direct rule; always four waves and four chunks in flight
            G, _, d, _, ns = want[B]
            assert attn_plan(so, B, *heads, kv8=1) == (G, 4, d, 1, ns), (B, heads, tune)


def test_default_tuning_is_what_the_tables_assume(lib):
    L, _ = lib
    assert [L.tuning_get(n) for n in ("attn_nw", "attn_deep", "attn_direct", "attn_nsplit")] == [4, -1, 1, 0]


@pytest.mark.parametrize("kind", ("bf16", "fp8"))
@pytest.mark.parametrize("G", sorted(R.HEADS))
def test_every_edge_variant_reaches_its_plan(lib, kind, G):
    L, so = lib
    Hq, Hkv = R.HEADS[G]
    B = len(R.EDGE_CTX)
    for name, tune, direct, ns, tag in R.variants(kind, G):
        with L.tuning(**tune):
            p = attn_plan(so, B, Hq, Hkv, ns, direct, int(kind == "fp8"))
        assert p is not None and ("attn", p[0], p[1], p[2], p[3], p[4], int(kind == "fp8")) == tag, (name, p, tag)


def test_every_by_shape_case_reaches_its_plan_with_no_switch_set(lib):
    _, so = lib
    for name, B, Hq, Hkv, ns, direct, tag in R.BY_SHAPE:
        p = attn_plan(so, B, Hq, Hkv, ns, direct) if ns else attn_plan(so, B, Hq, Hkv)
        assert ("attn",) + p + (0,) == tag, (name, p, tag)
    # ... and they are what a step launches: 9 - 31 rows at 32 kv heads, 32 rows, 64 rows at 16 kv heads
    assert attn_plan(so, 16, 32, 32) == (1, 4, 1, 0, 1) and attn_plan(so, 32, 32, 32) == (1, 4, 1, 1, 1) and attn_plan(so, 64, 32, 16) == (2, 4, 1, 1, 1)


def test_every_grouped_case_reaches_its_plan(lib):
    _, so = lib
    for name, groups, Hq, Hkv, plan in R.GROUPED + R.GROUPED_WIDE:
        B, N = sum(n for n, _, _ in groups), groups[0][0]
        for kv8 in (0, 1):
            assert ("group",) + group_plan(so, B, N, Hq, Hkv, kv8) == plan, (name, kv8)
    tails = {g[4][4] for g in R.GROUPED}
    widths = {g[4][1] for g in R.GROUPED}
    assert tails == {1, 2, 4, 8} and widths == {2, 4, 8} and any(g[4][3] == 2 for g in R.GROUPED)   # every tail G, every span width, two query chunks


def _step_plans(L, so, kv8):
    reached = set()
    for tune in TUNINGS:
        with L.tuning(**tune):
            for heads in HEADS:
                for B in range(1, 65):
                    G, nw, d, deep, ns = attn_plan(so, B, *heads, kv8=kv8)
                    reached.add(("attn", G, nw, d, deep, ns, kv8))
    return reached


def _group_plans(L, so, kv8):
    """the grouped route (step.hip: attn_group_rows, switch attn_group = 1): default numerics, a step whose attention is the one-split direct
    form, B whole groups of a width the launcher takes"""
    reached = set()
    for tune in TUNINGS:
        with L.tuning(**tune):
            for heads in HEADS:
                for B in range(1, 65):
                    if attn_plan(so, B, *heads, kv8=kv8)[2] != 1:
                        continue
                    for N in (2, 3, 4, 8, 16):
                        p = group_plan(so, B, N, *heads, kv8) if B % N == 0 else None
                        if p:
                            reached.add(R.group_tag(("group",) + p, kv8))
    return reached


def test_closure_every_reachable_plan_has_a_gpu_case(lib):
    L, so = lib
    tags = R.case_plans()
    for kv8 in (0, 1):
        steps, groups = _step_plans(L, so, kv8), _group_plans(L, so, kv8)
        assert len(steps) >= (8 if kv8 else 20) and len(groups) >= 10   # (the enumeration itself is not empty)
        assert steps <= tags, sorted(steps - tags)
        assert groups <= tags, sorted(groups - tags)
    # the instantiations named in the issue, by their tags: NW = 4 direct without four chunks, direct with four chunks, NW = 8, G = 4 on the bf16 cache
    for tag in (("attn", 1, 4, 1, 0, 1, 0), ("attn", 1, 4, 1, 1, 1, 0), ("attn", 2, 4, 1, 1, 1, 0), ("attn", 1, 8, 1, 0, 1, 0), ("attn", 4, 4, 0, 0, 8, 0),
                ("attn", 4, 8, 1, 0, 1, 0), ("attn", 8, 8, 1, 0, 1, 0)):
        assert tag in tags, tag


def test_plans_refuse_what_the_launchers_refuse(lib):
    _, so = lib
    assert attn_plan(so, 1, 32, 32, 2, 1) is None and b"emmax_decode_attn_plan" in so.emmax_last_error()    # the direct form has one split
    assert attn_plan(so, 1, 32, 32, 3, 0) is None and attn_plan(so, 1, 32, 32, 32, 0) is None                # 2^k, <= 16
    assert attn_plan(so, 1, 6, 2) is None and attn_plan(so, 1, 32, 5) is None and attn_plan(so, 1, 16, 1) is None   # GQA group 3 / not whole / 16
    assert attn_plan(so, 0, 32, 32) is None and attn_plan(so, 65, 32, 32) is None
    assert attn_plan(so, 1, 32, 32, 0, 0) is None and attn_plan(so, 1, 32, 32, 1, -1) is None                # half of "a step's own choice"
    assert so.emmax_decode_attn_plan(8, 32, 32, 0, -1, 0, None, None, None, None, None) == 0                 # every output is optional
    assert group_plan(so, 3, 2, 2, 2) is None and b"emmax_group_attn_plan" in so.emmax_last_error()          # B % N
    assert group_plan(so, 4, 1, 2, 2) is None and group_plan(so, 128, 2, 2, 2) is None and group_plan(so, 4, 2, 6, 2) is None
    assert group_plan(so, 64, 8, 32, 32) == (8, 1, 1, 1) and group_plan(so, 8, 8, 32, 32) == (8, 8, 1, 1)     # eight groups of 8 rows: one split; one: eight
