"""CPU: the cases of tests/test_gemm_forms_gpu.py reach every kernel instantiation of gemm.hip that a launch can reach, proved through the
host-only emmax_gemm_launches (the launchers themselves, their launches diverted into text) on the cross-compiled library.

  1. every GPU case makes exactly the launches it is tagged with, under its own tuning switches;
  2. closure: over a grid of shapes, operand sets, alignments and switch settings, through the argument sets the five op entry points can build,
     the instantiations reached are exactly gemm_ref.FORMS minus what no op entry point reaches (gemm_ref.NO_GPU_CASE), every one of them is
     launched by a GPU case, and every (instantiation, run-time sub-form) reached is the tag of a GPU case.  The main loop (gemm_deep) is taken
     out of the second statement: the epilogue a kernel takes does not depend on the loop in front of it, and the GPU file holds every
     non-default loop to bit equality with the default one.  Plan kinds: every (kind, operand the part arithmetic offsets) is a GPU case;
  3. refusals: launch_gemm_geom's shape checks answer through gemm_form without a launch.
"""

import itertools
import re

import pytest

import gemm_ref as G


@pytest.fixture(scope="module")
def L():
    from emmax import _lib

    _lib.load()
    return _lib


def pairs(tag):
    """a launch's tag -> its (instantiation without the main loop, sub-form) pairs: the epilogue path, the split-K slab, HL rows, run-time LN
    operands, the residual's type; a reduce kernel: its store branch and its residual branch"""
    inst, sub = tag.split("|")
    inst = re.sub(r"^(gemm:\w+:\d:\w+:\d):\d", r"\1", inst)
    return {(inst, f) for f in sub.split("+") if f != "res-none"}


def test_every_gpu_case_makes_the_launches_it_is_tagged_with(L):
    for c in G.CASES:
        with L.tuning(**dict(c.tune)):
            lines = G.launches(L, c)
        assert lines is not None, c.name
        assert tuple(G.tag_of(ln) for ln in lines) == c.want, (c.name, lines)


def test_the_plan_kind_cases_are_the_smallest_shapes_of_their_kind(L):
    """ROWS (big rows + small rows), COLS and HYBRID at the shapes gemm_ref pins; no smaller output reaches the kind on the searched grid, and every
    case stays at or below 2^25 output elements"""
    kinds = {"ROWS": "big rows 0..256 + small rows 256..257", "COLS": "cols 0..512: big | cols 512..640: small",
             "HYBRID": "hybrid cols 0..7168: big | cols 7168..7296: splitk ks=4"}
    for c in G.CASES:
        if c.kind in kinds:
            assert c.M * c.n_out <= 2 ** 25
            assert L.gemm_plan(c.M, c.N, c.K, act=c.act, ln=c.entry == "ln", residual=int(c.res != "none"), ws_bytes=c.ws) == kinds[c.kind], c.name
    rows = next(c for c in G.CASES if c.kind == "ROWS")
    cols = next(c for c in G.CASES if c.kind == "COLS")
    hyb = next(c for c in G.CASES if c.kind == "HYBRID")
    for K in (64, 128):
        for N in range(128, 2 ** 25 // 257, 128):
            for M in (257, 258, 300, 385, 513):
                if M * N < rows.M * rows.N:
                    assert not L.gemm_plan(M, N, K, ws_bytes=0).startswith("big rows"), (M, N, K)
    for K in (64, 128, 192):
        for N in (384, 640, 896, 1152):
            for M in range(256, cols.M * cols.N // N, 256):
                assert not L.gemm_plan(M, N, K, ws_bytes=0).startswith("cols"), (M, N, K)
    for N in range(384, 140 * 128, 128):   # (hybrid wants >= 32 K steps and more than one round of big tiles)
        for M in range(128, min(4097, hyb.M * hyb.N // N), 128):
            assert not L.gemm_plan(M, N, 2048, ws_bytes=256 << 20).startswith("hybrid"), (M, N)


def grid_calls():
    """argument sets the op entry points can build, as gemm_ref cases (name unused)"""
    shapes = [(1, 128, 64), (145, 384, 320), (273, 1280, 192), (512, 384, 2048), (257, 43776, 64), (28416, 640, 64), (2304, 7296, 2048), (5, 4096, 128), (64, 128, 1024)]
    aligns = [dict(), dict(ldc_pad=4, c_off=4), dict(ldc_pad=2), dict(ldr_pad=2)]
    for M, N, K in shapes:
        base = dict(name="grid", M=M, N=N, K=K)
        for al in aligns:
            for act, f32, bias, scale, res in itertools.product((0, 1, 2), (False, True), (False, True), (False, True), ("none", "sep", "alias")):
                if act == 2 and (bias or scale or res != "none"):
                    continue   # (SwiGLU ignores them)
                if res == "alias" and al.get("ldr_pad"):
                    continue
                kw = dict(base, act=act, out_f32=f32, bias=bias, scale=scale, res=res, **al)
                yield G.Case(entry="gemm", **kw)
                for ks, ws in ((0, 64 << 20), (2, 2 * M * N * 4), (3, 3 * M * N * 4)):
                    if ks <= K // 64:
                        yield G.Case(entry="splitk", ksplit=ks, ws=ws, **kw)
            for act, bias in itertools.product((0, 1), (False, True)):
                yield G.Case(entry="ln", act=act, bias=bias, **base, **al)
        for act, scale, res, ks, norm in itertools.product((0, 1), (False, True), ("alias", "sep"), (0, 2), (False, True)):
            for pad in (0, 1):
                yield G.Case(entry="stream", act=act, bias=scale, scale=scale, res=res, ksplit=ks, ws=(2 * M * N * 4 if ks else 64 << 20), norm=norm,
                             ldc_pad=pad, ldr_pad=pad, **base)
        for act, res, ws in itertools.product((0, 1, 2), ("none", "sep"), (0, 64 << 20)):
            if act == 2 and res != "none":
                continue
            yield G.Case(entry="x", act=act, bias=act != 2, res=res, ws=ws, **base)


SWITCHES = [dict(gemm_big=b, gemm_deep=d) for b in (-1, 0, 1, 2) for d in (-1, 0, 1, 3)] + \
           [dict(gemm_splitk=0), dict(gemm_sk_big=0), dict(gemm_sk_big=1), dict(gemm_hybrid=0), dict(gemm_normfuse=0), dict(gemm_sk_big=1, gemm_deep=0)]


def test_closure_the_gpu_cases_reach_what_the_launchers_reach(L):
    have_inst, have_tag = set(), set()
    for c in G.CASES:
        for t in c.want:
            have_inst.add(t.split("|")[0])
            have_tag |= pairs(t)
    assert have_inst == G.FORMS - G.NO_GPU_CASE, (sorted(G.FORMS - G.NO_GPU_CASE - have_inst), sorted(have_inst - G.FORMS))
    reached_inst, missing = set(), {}
    calls = list(grid_calls())
    for sw in SWITCHES:
        with L.tuning(**sw):
            for c in calls:
                if c.norm and not (c.N == 4096 and c.act == 0):
                    continue   # (emmax_op_gemm_stream refuses a norm it cannot fuse before it launches)
                lines = G.launches(L, c)
                for ln in lines or ():
                    t = G.tag_of(ln)
                    reached_inst.add(t.split("|")[0])
                    for pr in pairs(t) - have_tag:
                        missing.setdefault(pr, (sw, c))
    assert not missing, f"{len(missing)} reachable (instantiation, sub-form) without a GPU case, e.g. {sorted(missing)[:12]}; first: {next(iter(missing.items()))}"
    # the instantiations reached through the op entry points are the set of the module docstring and no others
    assert reached_inst == G.FORMS - G.NO_GPU_CASE, (sorted(G.FORMS - G.NO_GPU_CASE - reached_inst), sorted(reached_inst - G.FORMS))
    # ... and the one left is reached by the launcher when a session passes bf16 rows with norm_out
    line = L.gemm_launches(768, 4096, 4096, residual=1, norm=True, ws_bytes=64 << 20)
    assert [G.parse_line(x)[0] for x in line] == ["gemm:small:0:f32:0:1", "reduce_norm_bf16"]


def test_every_plan_kind_runs_every_operand_its_part_arithmetic_offsets():
    have = {(c.kind, op) for c in G.CASES for op in (("bias",) if c.bias and c.entry != "ln" else ()) + (("scale",) if c.scale else ()) +
            (("residual",) if c.res != "none" else ()) + (("ln",) if c.entry == "ln" else ()) + (("swiglu",) if c.act == 2 else ())}
    for kind in ("ROWS", "COLS"):       # launch_rows offsets A, C, residual, ln_stats; launch_gemm offsets W, C, bias, scale, residual, ln_s, ln_c
        for op in ("bias", "scale", "residual", "ln") + (("swiglu",) if kind == "ROWS" else ()):   # (no column split of (gate, up) groups)
            assert (kind, op) in have, (kind, op)
    for op in ("bias", "scale", "residual", "swiglu"):   # (no folded LayerNorm through split-K)
        assert ("HYBRID", op) in have, op


def test_refusals_answer_through_the_form_query_without_a_launch(L):
    ok = dict(M=145, N=384, K=320)
    assert L.gemm_launches(**ok, ln=True) is not None
    assert L.gemm_launches(**ok, ln=True, bias=True) is None                                   # LN with bias (it lives in ln_c)
    assert L.gemm_launches(**ok, ln=True, scale=True) is None
    assert L.gemm_launches(**ok, ln=True, residual=1) is None
    assert L.gemm_launches(**ok, ln=True, ksplit=2, ws_bytes=64 << 20) is None               # LN with split-K
    assert L.gemm_launches(**ok, residual=2, out_f32=True) is not None
    assert L.gemm_launches(**ok, residual=2, out_f32=False) is None                            # an fp32 residual stream yields an fp32 result
    assert L.gemm_launches(145, 384, 256, a_hl=1, out_f32=True) is not None
    assert L.gemm_launches(145, 384, 192, a_hl=1, out_f32=True, lda=192) is None              # HL rows: (hi, lo) pairs of K steps, K % 128
    assert L.gemm_launches(145, 384, 256, a_hl=1, out_f32=True, ln=True) is None
    with L.tuning(gemm_big=2):
        assert L.gemm_launches(**ok) is not None
        assert L.gemm_launches(145, 384, 256, a_hl=1, out_f32=True) is None                   # HL rows on the 32-deep tile
        assert L.gemm_launches(**ok, act=2, out_f32=True) is None                              # fp32 SwiGLU on the 32-deep tile
        assert L.gemm_launches(**ok, act=2) is not None
    assert L.gemm_launches(145, 384, 96) is None and L.gemm_launches(145, 200, 64) is None     # K % 64, N % 128
    assert L.gemm_launches(145, 384, 64, lda=68) is None                                       # lda % 8
    # split-K: every slice needs a K step of its own (5 steps in 4 slices of 2: the fourth would start past K)
    assert L.gemm_launches(**ok, ksplit=3, ws_bytes=64 << 20) is not None and L.gemm_launches(**ok, ksplit=5, ws_bytes=64 << 20) is not None
    assert L.gemm_launches(**ok, ksplit=4, ws_bytes=64 << 20) is None
    assert L.gemm_launches(**ok, ksplit=6, ws_bytes=64 << 20) is None
    assert L.gemm_launches(**ok, ksplit=2, ws_bytes=1024) is None                              # scratch too small
    assert L.gemm_launches(**ok, act=2, out_f32=True, ksplit=2, ws_bytes=64 << 20) is None   # SwiGLU through split-K: bf16 only


def test_the_launch_text_names_parts_and_k_slices(L):
    """the one-frame gate/up of the hot path: a round of big tiles, the remaining columns in 8 K slices of 8 steps, the SwiGLU reduce pass"""
    lines = L.gemm_launches(768, 22016, 4096, act=2, ws_bytes=64 << 20)
    d = [G.parse_line(x)[1] for x in lines]
    assert [x["kernel"] for x in d] == ["gemm", "gemm", "reduce2"]
    assert (d[0]["geom"], d[0]["rows"], d[0]["cols"], d[0]["epi"], d[0]["ks"], d[0]["ksteps"]) == ("big", "0..768", "0..21760", "staged", "1", "0..64")
    assert (d[1]["geom"], d[1]["cols"], d[1]["out"], d[1]["ks"]) == ("small", "21760..22016", "f32", "8")
    assert d[1]["ksteps"] == ",".join(f"{8 * i}..{8 * i + 8}" for i in range(8))
    assert (d[2]["cols"], d[2]["store"]) == ("21760..22016", "vec")
    uneven = G.parse_line(L.gemm_launches(145, 384, 320, ksplit=3, ws_bytes=64 << 20)[0])[1]
    assert uneven["ksteps"] == "0..2,2..4,4..5"
