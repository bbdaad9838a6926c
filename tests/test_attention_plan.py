"""CPU: which instantiation of the prefill / ViT attention a launch takes (emmax_attention_plan: host only -- launch_attention dispatches on the
struct this call fills and launches the instantiation whose compile-time constants equal it, so plan and launch cannot disagree).
  1. PINNED: the plan of the three session shapes, of frame counts on either side of every threshold of the launcher, under every switch setting.
  2. every GPU case of tests/attention_ref.py reaches the plan it is tagged with, under its own switches and at its own shape.
  3. CLOSURE: every (instantiation, mask) a launch can reach over a grid of shapes and switch settings is the tag of at least one GPU case, and
     the instantiations reached are exactly the ten that attention.hip holds.
"""

import ctypes as C

import pytest

import attention_ref as R

TUNINGS = [{}, {"attn_resident": 0}, {"attn_resident": 2}, {"attn_ksplit": 0}, {"attn_ksplit": 1}, {"attn_lazy": 0}, {"attn_ksplit": 0, "attn_lazy": 0},
           {"attn_ksplit": 1, "attn_lazy": 0}]


@pytest.fixture(scope="module")
def lib():
    from emmax import _lib

    return _lib, _lib.load()


def attn_plan(so, B, max_seqlen, Hq, Hkv, hd, causal):
    """the tag of tests/attention_ref.py -- (kind, head_dim, query waves, producer waves, key groups, lazy, rows) -- or None where the call refuses"""
    o = [C.c_int(-7) for _ in range(6)]
    if so.emmax_attention_plan(B, max_seqlen, Hq, Hkv, hd, causal, *[C.byref(x) for x in o]) != 0:
        return None
    res, qw, pw, kgr, lazy, rows = [x.value for x in o]
    return ("res" if res else "ring", hd, qw, pw, kgr, lazy, rows)


def _tag(form):
    return R.FORMS[form]["tag"]


def _key(t):
    return ",".join(f"{k}={v}" for k, v in t.items()) or "default"


# (B, max_seqlen, Hq, Hkv, head_dim, causal) -> form, under default tuning
PINNED_DEFAULT = [
    # the three session shapes, one frame: DINOv2 261 x 16 x 64 (3 x 96 wastes 27 rows, 3 x 128 wastes 123), SigLIP 256 x 16 x 72, the LLaMA prefill
    ((1, 261, 16, 16, 64, 0), "ring64w3"), ((1, 256, 16, 16, 72, 0), "ring72w4"), ((1, 768, 32, 32, 128, 1), "ring128k2"),
    # head_dim 64: resident from 512 (sequence, head) items, 256 rows up to 256 tokens, 288 rows up to 288
    ((31, 261, 16, 16, 64, 0), "ring64w3"), ((32, 261, 16, 16, 64, 0), "res64w9"), ((511, 261, 1, 1, 64, 0), "ring64w3"), ((512, 261, 1, 1, 64, 0), "res64w9"),
    ((32, 256, 16, 16, 64, 0), "res64w8"), ((32, 257, 16, 16, 64, 0), "res64w9"), ((32, 288, 16, 16, 64, 0), "res64w9"), ((32, 289, 16, 16, 64, 0), "ring64w4"),
    ((256, 261, 16, 16, 64, 0), "res64w9"), ((32, 256, 16, 16, 64, 1), "ring64w4"),
    # head_dim 72: resident from 2048 items, up to 256 tokens
    ((127, 256, 16, 16, 72, 0), "ring72w4"), ((128, 256, 16, 16, 72, 0), "res72w8"), ((2047, 256, 1, 1, 72, 0), "ring72w4"), ((2048, 256, 1, 1, 72, 0), "res72w8"),
    ((128, 257, 16, 16, 72, 0), "ring72w3"), ((256, 256, 16, 16, 72, 0), "res72w8"), ((128, 256, 16, 16, 72, 1), "ring72w4"),
    # three waves where 96-row blocks waste fewer rows than 128-row blocks
    ((1, 96, 2, 2, 64, 0), "ring64w3"), ((1, 97, 2, 2, 64, 0), "ring64w4"), ((1, 128, 2, 2, 72, 0), "ring72w4"), ((1, 129, 2, 2, 72, 0), "ring72w3"),
    ((1, 192, 2, 2, 64, 1), "ring64w3"), ((1, 193, 2, 2, 64, 1), "ring64w4"), ((1, 288, 2, 2, 72, 0), "ring72w3"), ((1, 289, 2, 2, 72, 0), "ring72w4"),
    ((1, 1024, 2, 2, 64, 0), "ring64w4"), ((1, 1025, 2, 2, 64, 0), "ring64w3"),
    # head_dim 128: always four query waves; two key groups on a causal launch of at most 256 blocks = 8 ceil(items / 8) ceil(max_seqlen / 128)
    ((8, 128, 32, 32, 128, 1), "ring128k2"), ((257, 128, 1, 1, 128, 1), "ring128"), ((1, 1024, 32, 8, 128, 1), "ring128k2"), ((1, 1025, 32, 8, 128, 1), "ring128"),
    ((2, 768, 32, 32, 128, 1), "ring128"), ((1, 768, 32, 32, 128, 0), "ring128"), ((1, 1025, 2, 2, 128, 1), "ring128k2"),
]
# the same shapes under each switch: (tuning, shape) -> form
PINNED_SWITCHED = [
    ({"attn_resident": 0}, (256, 261, 16, 16, 64, 0), "ring64w3"), ({"attn_resident": 0}, (256, 256, 16, 16, 72, 0), "ring72w4"),
    ({"attn_resident": 2}, (1, 261, 16, 16, 64, 0), "res64w9"), ({"attn_resident": 2}, (1, 256, 16, 16, 72, 0), "res72w8"),
    ({"attn_resident": 2}, (1, 256, 8, 8, 64, 0), "res64w8"), ({"attn_resident": 2}, (1, 256, 7, 7, 64, 0), "ring64w4"),      # from 8 items
    ({"attn_resident": 2}, (1, 289, 16, 16, 64, 0), "ring64w4"), ({"attn_resident": 2}, (1, 257, 16, 16, 72, 0), "ring72w3"),  # it has to fit
    ({"attn_resident": 2}, (4, 200, 4, 2, 64, 1), "ring64w4"), ({"attn_resident": 2}, (8, 128, 2, 2, 128, 0), "ring128"),      # never causal, never 128
    ({"attn_ksplit": 0}, (1, 768, 32, 32, 128, 1), "ring128"), ({"attn_ksplit": 1}, (2, 768, 32, 32, 128, 1), "ring128k2"),
    ({"attn_ksplit": 1}, (1, 768, 32, 32, 128, 0), "ring128"),                                                                  # causal only
    ({"attn_lazy": 0}, (2, 768, 32, 32, 128, 1), "ring128nolazy"), ({"attn_lazy": 0}, (1, 768, 32, 32, 128, 0), "ring128nolazy"),
    ({"attn_lazy": 0}, (1, 768, 32, 32, 128, 1), "ring128k2"),                                                                  # the key-group form is lazy
    ({"attn_ksplit": 0, "attn_lazy": 0}, (1, 768, 32, 32, 128, 1), "ring128nolazy"),
    ({"attn_lazy": 0}, (32, 261, 16, 16, 64, 0), "res64w9"), ({"attn_lazy": 0}, (1, 261, 16, 16, 64, 0), "ring64w3"),            # head_dim 128 only
]


def test_default_tuning_is_what_the_tables_assume(lib):
    L, _ = lib
    assert [L.tuning_get(n) for n in ("attn_resident", "attn_ksplit", "attn_lazy")] == [-1, -1, 1]


def test_plans_are_pinned(lib):
    L, so = lib
    for shape, form in PINNED_DEFAULT:
        assert attn_plan(so, *shape) == _tag(form), (shape, form, attn_plan(so, *shape))
    for tune, shape, form in PINNED_SWITCHED:
        with L.tuning(**tune):
            assert attn_plan(so, *shape) == _tag(form), (tune, shape, form, attn_plan(so, *shape))
    for n in range(1, 1200):   # the 3 / 4 wave rule at every length
        want = "w3" if R.three_waves(n) else "w4"
        assert attn_plan(so, 1, n, 2, 2, 64, 0) == _tag("ring64" + want) and attn_plan(so, 1, n, 2, 2, 72, 1) == _tag("ring72" + want), n
        assert attn_plan(so, 1, n, 2, 2, 128, 0) == _tag("ring128")


def test_every_case_reaches_its_plan(lib):
    L, so = lib
    for c in R.all_cases():
        assert c.max_seqlen < 1100 and (c.Hq <= 8 or FORMS_BIG(c)), c.name
        with L.tuning(**c.tune):
            assert attn_plan(so, c.B, c.max_seqlen, c.Hq, c.Hkv, c.hd, c.causal) == c.tag, (c.name, attn_plan(so, c.B, c.max_seqlen, c.Hq, c.Hkv, c.hd, c.causal))
        if c.by_shape:
            assert c.tune == {}


def FORMS_BIG(c):
    """16 heads: the resident item-count cases and the session shapes only"""
    return "items" in c.name or c.by_shape


def test_resident_item_counts_cover_one_two_and_three_items_per_block():
    """persistent blocks: 8 x min(ceil(items / 8), 32); a block's items = ceil(items / 8) / 32 rounded up"""
    for form in ("res64w8", "res64w9", "res72w8"):
        per_block = set()
        for c in R.all_cases():
            if c.form == form:
                per_xcd = -(-c.B * c.Hq // 8)
                per_block.add(-(-per_xcd // 32))
                if c.Hq < 8 and "items" not in c.name and not c.by_shape:
                    assert (c.B * c.Hq) % 8, c.name   # the edge batches of 2, 3 and 4 heads leave idle items in the XCD map
        assert per_block == {1, 2, 3}, (form, per_block)


def _reachable(L, so):
    got = set()
    for tune in TUNINGS:
        with L.tuning(**tune):
            for hd in (64, 72, 128):
                for causal in (0, 1):
                    for B, Hq in ((1, 2), (1, 16), (1, 32), (8, 32), (32, 16), (33, 16), (128, 16), (257, 1)):
                        for n in (1, 96, 97, 128, 129, 256, 257, 261, 288, 289, 768, 1024, 1025):
                            got.add((attn_plan(so, B, n, Hq, Hq, hd, causal), causal))
    return got


def test_closure_every_reachable_instantiation_has_a_gpu_case(lib):
    L, so = lib
    reached, tags = _reachable(L, so), R.case_tags()
    assert {t for t, _ in reached} == {f["tag"] for f in R.FORMS.values()} and len(R.FORMS) == 10   # all ten, and nothing else
    assert reached <= tags, sorted(reached - tags)
    # as the issue lists them: ring 64 / 72 x 3 / 4 waves, ring 128 lazy / attn_lazy = 0 / two key groups, three resident configurations; each ring
    # form under both masks where the launcher permits it (the key groups are causal only, the resident forms never)
    for form, f in R.FORMS.items():
        masks = {causal for t, causal in tags if t == f["tag"]}
        assert masks == ({0} if f["res"] else {1} if f["kg"] == 2 else {0, 1}), (form, masks)
        assert {causal for t, causal in reached if t == f["tag"]} == masks, form


def test_plan_refuses_what_the_launcher_refuses(lib):
    _, so = lib
    assert attn_plan(so, 1, 100, 6, 4, 64, 0) is None and b"emmax_attention_plan" in so.emmax_last_error()   # Hq not a multiple of Hkv
    assert attn_plan(so, 1, 100, 4, 0, 64, 0) is None and attn_plan(so, 1, 100, 0, 1, 64, 0) is None
    assert attn_plan(so, 1, 100, 2, 2, 80, 0) is None and attn_plan(so, 1, 100, 2, 2, 256, 1) is None          # head_dim in {64, 72, 128}
    assert attn_plan(so, 0, 100, 2, 2, 64, 0) is None and attn_plan(so, 1, 0, 2, 2, 64, 0) is None             # nothing to launch
    assert so.emmax_attention_plan(1, 261, 16, 16, 64, 0, None, None, None, None, None, None) == 0             # every output is optional
    assert attn_plan(so, 1, 100, 6, 2, 64, 0) == _tag("ring64w4") and attn_plan(so, 1, 100, 3, 1, 128, 1) == _tag("ring128k2")   # any GQA group
