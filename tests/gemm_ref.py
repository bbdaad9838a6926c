"""Cases, references, emulation and bounds of tests/test_gemm_forms_gpu.py.  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

gemm.hip holds 52 kernel instantiations (FORMS below): emmax_gemm_bf16_kernel in 8 (act, output, LN) x 5 (geometry, main loop) = 40,
emmax_gemm_k32_kernel in 7, three split-K reduce kernels and two reduce + RMSNorm kernels.  launch_gemm_geom dispatches on a GemmForm
(kernels.h), and emmax_gemm_launches prints every launch of a call with the form it takes and the epilogue the kernel then runs, so every CASE
below names the launches it must produce (`want`), tests/test_gemm_plan.py proves on the CPU that the cases reach what the launchers can reach,
and tests/test_gemm_forms_gpu.py runs them.

For every case this module holds
  * the operands of three input FAMILIES: `random` (prefill_stage_ref.gemm_operands: a product term of rms ~ 1), `cancel` (the residual, or the
    bias for row 0, is minus the rounded product: the outputs cancel to ~0 and only the fp32 arithmetic is left), `ties` (A, W, bias, residual
    small integers and a LayerScale of 1 / 1.5 / 2: every fp32 intermediate is exact in any summation order, the results are integers and
    halves of 128 .. 1500, i.e. exactly ON bf16 rounding ties (odd integers of 256 .. 511, 4 n + 2 of 512 .. 1023) and just beside them, so the
    stored bits have ONE right answer: round-to-nearest-even of the exact result -- truncation and double rounding miss it);
  * a float64 REFERENCE of the documented algebra (GemmParams, kernels.h; the LayerNorm fold: DESIGN.md section 4, with the rounded W' the
    GEMM multiplies by);
  * a float32 EMULATION of the kernel's arithmetic: products one by one in k order per K slice (K roundings: the most-rounded order), the
    slices summed in order, the epilogue in the kernel's order, the erf polynomial and x * rcp(1 + exp2(..)) ported to fp32;
  * the BOUND   |got - ref| <= a32 [+ half an ulp of bf16 at |ref| + a32],   a32 = 2^-24 |ref| + ACT_RTOL[act] |term| + 2 x SPREAD[case] x rms(term)
    with term = ref - residual.  SPREAD is what the emulation leaves above the first two terms, in units of rms(term), measured on the case's
    own inputs (`python tests/gemm_ref.py` prints the table; tests/test_gemm_ref.py pins it); 2 = prefill_stage_ref.GEMM_ORDER: the MFMA
    accumulates in an order the emulation does not reproduce.  ACT_RTOL: v_exp_f32 and v_rcp_f32 are accurate to 1 ulp (CDNA ISA guide) where
    the emulation's exp2 and quotient are correctly rounded -- GELU's one transcendental moves the result by at most 2^-23 of itself
    (x >= 0: x h <= x - x h; x < 0: the result IS -|x| h), SwiGLU's two by 2^-22.  The bf16 half ulp is taken from the exponent of
    |ref| + a32, not a flat 2^-9: rounding x = ref + d (|d| <= a32) to nearest moves it by at most half an ulp of x's own binade.
    No figure here comes from a kernel's output.

What the five op entry points cannot reach (and so no case has): the k32 geometry at K = 32, 96, 160 (launch_gemm_geom wants K % 64 for every
geometry: its cases run K = 64, 192, 320 = 2, 6, 10 steps of 32); LayerNorm with an fp32 result (emmax_op_gemm_ln stores bf16: the run-time LN
operands of the direct epilogue are reached through an unaligned C instead); emmax_splitk_reduce_norm_kernel<8, false> (only a session
with a bf16 residual stream passes norm_out with bf16 rows: tests/test_e2e_gpu.py runs it); split-K on the k32 geometry (no caller).
"""

import math
from dataclasses import dataclass, replace

import torch

import prefill_stage_ref as P
import vision_stage_ref as V

bf, bfr, gen = P.bf, P.bfr, P.gen
RT = 2.0 ** -24
ORDER = P.GEMM_ORDER
ACT_RTOL = {0: 0.0, 1: 2.0 ** -23, 2: 2.0 ** -22}
LN_EPS = 1e-6
GEOMS = ("small", "big", "k32")
TILE_M = {"small": 128, "big": 256, "k32": 128}
DEEP_DEFAULT = {"small": 1, "big": 3, "k32": 0}
DEEP_OTHER = {"small": (0,), "big": (0, 1), "k32": ()}

# ---- the instantiations -----------------------------------------------------------------------------------------------------------------------
EPI8 = ((0, "bf16", 0), (0, "f32", 0), (1, "bf16", 0), (1, "f32", 0), (2, "bf16", 0), (2, "f32", 0), (0, "bf16", 1), (1, "bf16", 1))
FORMS = {f"gemm:{g}:{a}:{o}:{ln}:{d}" for g, ds in (("small", (0, 1)), ("big", (0, 1, 3))) for d in ds for a, o, ln in EPI8}
FORMS |= {f"gemm:k32:{a}:{o}:{ln}:0" for a, o, ln in EPI8 if (a, o) != (2, "f32")}
FORMS |= {"reduce0", "reduce1", "reduce2", "reduce_norm_bf16", "reduce_norm_f32"}
assert len(FORMS) == 52
NO_GPU_CASE = {"reduce_norm_bf16"}   # (module docstring)


def parse_line(line):
    """a line of emmax_gemm_launches -> (instantiation, dict of its fields)"""
    head, *kv = line.split()
    d = dict(x.split("=", 1) for x in kv)
    d["kernel"] = head
    if head == "gemm":
        return f"gemm:{d['geom']}:{d['act']}:{d['out']}:{d['ln']}:{d['deep']}", d
    return head, d


def tag_of(line):
    """instantiation + the run-time sub-form: what a GPU case is tagged with"""
    inst, d = parse_line(line)
    if d["kernel"] == "gemm":
        sub = [d["epi"]]
        if int(d["ks"]) > 1:
            sub.append("slab")
        if d["hl"] == "1":
            sub.append("hl")
        if d["lnrt"] == "1" and d["epi"] != "staged":
            sub.append("ln-direct")
        if d["res"] != "none":
            sub.append("res-" + d["res"])
        return inst + "|" + "+".join(sub)
    return inst + "|" + d["out"] + "-" + d["store"] + "+res-" + d["res"]


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    entry: str                 # gemm | splitk | ln | stream | x: emmax_op_gemm, _splitk, _ln, _stream, emmax_op_x_gemm
    M: int
    N: int
    K: int
    act: int = 0
    out_f32: bool = False
    bias: bool = False
    scale: bool = False
    res: str = "none"          # none | sep (a residual of its own, pitch N + ldr_pad) | alias (C doubles as the residual); bf16 or fp32 as the entry has it
    ldc_pad: int = 0
    c_off: int = 0             # C starts this many ELEMENTS into its (16-byte aligned) rows
    ldr_pad: int = 0
    lda_pad: int = 0
    ldw_pad: int = 0
    n_store: int = 0           # stream: columns stored (0: N)
    ksplit: int = 0
    ws: int = 0                # bytes of split-K scratch (0: none)
    norm: bool = False         # stream: the reduce pass also applies the RMSNorm
    tune: tuple = ()           # tuning switches of the case, ((name, value), ..)
    families: tuple = ("random",)
    want: tuple = ()           # tag_of() of every launch, in order
    kind: str = ""             # plan kind the case is there for (ROWS / COLS / HYBRID / SPLITK)
    same_as: str = ""          # a non-default main loop: bit-identical to this case (and not bounded again)

    @property
    def n_out(self):
        return self.N // 2 if self.act == 2 else (self.n_store or self.N)

    @property
    def ldc(self):
        return self.n_out + self.ldc_pad

    @property
    def ldr(self):
        return self.n_out + self.ldr_pad

    @property
    def f32(self):
        return self.out_f32 or self.entry in ("stream", "x")

    @property
    def res_f32(self):
        return self.entry in ("stream", "x")

    @property
    def hl(self):
        return self.entry == "x"


def _gemm_tag(geom, act, f32, ln, deep, epi, slab=False, hl=False, ln_direct=False, res=None):
    sub = [epi] + (["slab"] if slab else []) + (["hl"] if hl else []) + (["ln-direct"] if ln_direct else []) + (["res-" + res] if res else [])
    return f"gemm:{geom}:{act}:{'f32' if f32 else 'bf16'}:{ln}:{deep}|" + "+".join(sub)


def _single(c, geom, deep=None):
    """the one launch of a case forced onto a geometry, from what the case asks for -- not from the library"""
    staged = (not c.f32 and c.ldc % 8 == 0 and c.c_off % 8 == 0 and (c.N % 16 == 0 if c.act == 2 else c.n_out % 8 == 0)
              and (c.res == "none" or (c.ldr if c.res == "sep" else c.ldc) % 4 == 0))
    epi = "staged" if staged else "direct-vec" if c.ldc % 4 == 0 else "direct-elt"
    ln = c.entry == "ln"
    res = None if c.res == "none" and c.entry != "stream" else ("f32" if c.res_f32 else "bf16")
    return _gemm_tag(geom, c.act, c.f32, int(ln and not c.f32), DEEP_DEFAULT[geom] if deep is None else deep, epi, hl=c.hl, ln_direct=ln and not staged, res=res)


def _forced(c, geom, deep=None):
    tune = (("gemm_big", GEOMS.index(geom)),) + ((("gemm_deep", deep),) if deep is not None else ())
    return replace(c, tune=c.tune + tune, want=(_single(c, geom, deep),))


def _cases():
    out = []
    Ns = {"small": (128, 384, 640), "big": (128, 384, 1280), "k32": (128, 384, 1280)}   # 640 / 1280: five tile columns, one more than a band of 4
    Ks = (64, 192, 320)   # one step (the prologue meets the epilogue); the three-stage A ring wraps exactly once; five steps, an odd count
    # (k32: 2, 6 and 10 steps of 32 -- K % 64 is required of every geometry)
    epis = (
        ("plain", dict(entry="gemm", bias=True, scale=True, res="sep", families=("random", "cancel", "ties"))),
        ("stream", dict(entry="stream", bias=True, scale=True, res="alias", families=("random", "cancel", "ties"))),
        ("gelu", dict(entry="gemm", act=1, bias=True, scale=True)),
        ("gelu32", dict(entry="stream", act=1, bias=True, scale=True, res="sep")),
        ("swiglu", dict(entry="gemm", act=2)),
        ("swiglu32", dict(entry="x", act=2)),
        ("ln", dict(entry="ln", bias=True)),
        ("ln_gelu", dict(entry="ln", act=1, bias=True)),
    )
    for geom in GEOMS:
        Ms = (1, TILE_M[geom] + 17 if geom == "small" else 273, 2 * TILE_M[geom])
        for ci, (ename, kw) in enumerate(epis):
            if geom == "k32" and kw["entry"] == "x":
                continue   # (HL rows and fp32 SwiGLU: refused on the 32-deep tile, tests/test_gemm_plan.py)
            for i in range(3):   # a Latin square over (M, N, K): every value of each with every epilogue, every pair of values somewhere
                M, N, K = Ms[i], Ns[geom][(i + ci) % 3], Ks[(i + 2 * ci) % 3]
                pads = dict(lda_pad=8, ldw_pad=16) if i == 1 and kw["entry"] != "x" else {}
                c = Case(name=f"{geom}-{ename}-{M}x{N}x{K}", M=M, N=N, K=K, **kw, **pads)
                out.append(_forced(c, geom))
                if i == 1:   # the other main loops of this (geometry, act, output, LN): bit-identical to the default one
                    for d in DEEP_OTHER[geom]:
                        out.append(replace(_forced(replace(c, name=c.name + f"-deep{d}", families=("random",)), geom, d), same_as=c.name))
        # ---- alignment: what sends a bf16 result through the direct epilogue, and its vector / element-wise branches
        M, N, K = Ms[1], 384, 192
        base = dict(entry="gemm", M=M, N=N, K=K, bias=True, scale=True, res="sep", lda_pad=8, ldw_pad=16, families=("random", "ties"))
        for nm, kw in (("ldc4-off8B", dict(ldc_pad=4, c_off=4)), ("ldc2", dict(ldc_pad=2)), ("ldr2", dict(ldr_pad=2)), ("ldr2-ldc2", dict(ldr_pad=2, ldc_pad=2)),
                       ("alias", dict(res="alias")), ("alias-ldc4", dict(res="alias", ldc_pad=4)), ("f32-bf16res", dict(out_f32=True)),
                       ("f32-bf16res-ldc1", dict(out_f32=True, ldc_pad=1, ldr_pad=1))):
            out.append(_forced(Case(name=f"{geom}-direct-{nm}", **{**base, **kw}), geom))
        for nm, kw in (("gelu-ldc4", dict(act=1, res="none", ldc_pad=4)), ("swiglu-ldc4", dict(act=2, bias=False, scale=False, res="none", ldc_pad=4)),
                       ("swiglu-ldc2", dict(act=2, bias=False, scale=False, res="none", ldc_pad=2)),
                       ("ln-ldc4", dict(entry="ln", scale=False, res="none", ldc_pad=4)), ("ln-gelu-ldc2", dict(entry="ln", act=1, scale=False, res="none", ldc_pad=2)),
                       ("ln-ldc2", dict(entry="ln", scale=False, res="none", ldc_pad=2)), ("ln-gelu-ldc4", dict(entry="ln", act=1, scale=False, res="none", ldc_pad=4)),
                       ("gelu-ldc2", dict(act=1, res="none", ldc_pad=2)), ("gelu-res", dict(act=1)), ("gelu-res-ldr2", dict(act=1, ldr_pad=2)),
                       ("gelu32-ldc1", dict(entry="stream", act=1, ldc_pad=1, ldr_pad=1)), ("stream-ldc1", dict(entry="stream", ldc_pad=1, ldr_pad=1)),
                       ("f32-gelu-bf16res", dict(act=1, out_f32=True))) + \
                      ((("swiglu32-ldc1", dict(entry="x", act=2, bias=False, scale=False, res="none", ldc_pad=1, lda_pad=0, ldw_pad=0)),
                        ("f32-swiglu", dict(act=2, bias=False, scale=False, res="none", out_f32=True))) if geom != "k32" else ()):
            out.append(_forced(Case(name=f"{geom}-direct-{nm}", **{**base, **kw, "families": ("random",)}), geom))
        if geom != "k32":   # two-term HL rows through the direct fp32 epilogue (K % 128 of the doubled K holds for every K % 64)
            out.append(_forced(Case(name=f"{geom}-hl-{M}x{N}x{K}", entry="x", M=M, N=N, K=K, bias=True, res="sep", families=("random", "cancel", "ties")), geom))
            out.append(_forced(Case(name=f"{geom}-hl-gelu-{M}x128x64", entry="x", M=M, N=128, K=64, act=1, bias=True), geom))
    # ---- the persistent walk: more tiles than resident blocks (512 small / k32, 256 big), so a block walks a second tile through the banding
    walk = dict(entry="gemm", K=64, bias=True, scale=True, res="sep")
    out.append(_forced(Case(name="small-walk-513", M=19 * 128 - 111, N=27 * 128, **walk), "small"))
    out.append(_forced(Case(name="big-walk-259", M=7 * 256 - 239, N=37 * 256, **walk), "big"))
    out.append(_forced(Case(name="k32-walk-513", M=19 * 128 - 111, N=27 * 256, **walk), "k32"))
    # ---- split-K with explicit slices: tile kernel (fp32 slab) + reduce pass
    def sk(name, geom="small", **kw):
        c = Case(name=name, **kw)
        ws = c.ksplit * c.M * c.N * 4
        slab = _gemm_tag(geom, 0, True, 0, DEEP_DEFAULT[geom], "direct-vec", slab=True)
        vec_c = (c.ldc % 4 == 0) if c.f32 else (c.ldc % 8 == 0 and c.c_off % 8 == 0)
        ldr = c.ldr if c.res == "sep" else c.ldc
        has_res = c.res != "none" or c.entry == "stream"
        vec_r = has_res and ((ldr % 4 == 0) if c.res_f32 else (ldr % 8 == 0)) and (c.res == "sep" or c.c_off % 8 == 0)
        rname = ("reduce_norm_f32" if c.norm else f"reduce{c.act}")
        rtag = f"{rname}|{'f32' if c.f32 else 'bf16'}-{'vec' if vec_c or c.norm else 'elt'}+res-" + \
               ("none" if not has_res else ("f32" if c.res_f32 else "bf16") + ("" if c.act == 2 else "-vec" if vec_r or c.norm else "-elt"))
        tune = (("gemm_sk_big", 1),) if geom == "big" else ()
        return replace(c, ws=ws, tune=tune, want=(slab, rtag), kind="SPLITK")
    e = dict(entry="splitk", M=145, N=384, K=320, bias=True, scale=True)
    for geom in ("small", "big"):
        g = dict(e, M=273) if geom == "big" else e
        out.append(sk(f"sk-{geom}-ks2-alias", geom, **g, ksplit=2, res="alias", families=("random", "cancel", "ties")))   # 5 K steps: slices of 3 + 2
        out.append(sk(f"sk-{geom}-ks3-sep", geom, **g, ksplit=3, res="sep", families=("random", "ties")))                  # 2 + 2 + 1
        out.append(sk(f"sk-{geom}-ks5", geom, **g, ksplit=5, res="sep"))                                                      # ks = K / 64: one step each
    out.append(sk("sk-elt-ldc2", **e, ksplit=3, res="sep", ldc_pad=2, ldr_pad=2, families=("random", "ties")))
    out.append(sk("sk-f32-bf16res", **e, ksplit=2, res="sep", out_f32=True, families=("random", "ties")))
    out.append(sk("sk-gelu", **dict(e, act=1), ksplit=3))
    out.append(sk("sk-gelu-elt", **dict(e, act=1), ksplit=2, ldc_pad=2))
    out.append(sk("sk-gelu-res", **dict(e, act=1), ksplit=2, res="sep"))
    out.append(sk("sk-gelu-res-elt", **dict(e, act=1), ksplit=3, res="sep", ldc_pad=2, ldr_pad=2))
    out.append(sk("sk-gelu-f32", **dict(e, act=1), ksplit=3, res="sep", out_f32=True))
    out.append(sk("sk-gelu-f32-elt", **dict(e, act=1), ksplit=2, out_f32=True, ldc_pad=1))
    out.append(sk("sk-stream-gelu", **dict(e, entry="stream", act=1), ksplit=2, res="sep"))
    out.append(sk("sk-stream-gelu-ldr1", **dict(e, entry="stream", act=1), ksplit=3, res="alias", ldc_pad=1))
    out.append(sk("sk-swiglu", entry="splitk", M=145, N=384, K=320, act=2, ksplit=3))
    out.append(sk("sk-swiglu-elt", entry="splitk", M=145, N=384, K=320, act=2, ksplit=2, ldc_pad=2))
    s = dict(entry="stream", M=145, N=384, K=320, bias=True, scale=True)
    out.append(sk("sk-stream-alias", **s, ksplit=3, res="alias", families=("random", "cancel", "ties")))
    out.append(sk("sk-stream-sep-ldr1", **s, ksplit=2, res="sep", ldr_pad=1, ldc_pad=1, families=("random", "ties")))
    for res in ("alias", "sep"):   # four rows per block plus one
        out.append(sk(f"sk-norm-{res}", entry="stream", M=5, N=4096, K=128, bias=True, scale=True, ksplit=2, res=res, norm=True))
    # HL rows with an even split: emmax_op_x_gemm takes its slices from the plan -- (64, 128, 1024): 32 steps of the doubled K, ks = 4
    c = Case(name="sk-hl-ks4", entry="x", M=64, N=128, K=1024, bias=True, res="sep", ws=4 * 64 * 128 * 4, kind="SPLITK")
    out.append(replace(c, want=(_gemm_tag("small", 0, True, 0, 1, "direct-vec", slab=True, hl=True), "reduce0|f32-vec+res-f32-vec")))
    # ---- plan kinds: the smallest shapes that reach them (tests/test_gemm_plan.py repeats the search), every operand the part arithmetic offsets
    st = lambda g, a, ln, res=None, **k: _gemm_tag(g, a, False, ln, DEEP_DEFAULT[g], "staged", res=res, **k)   # noqa: E731
    rows, cols, hyb = (257, 43776, 64), (28416, 640, 64), (2304, 7296, 2048)
    for nm, kw, a, ln, res in (("plain", dict(entry="gemm", bias=True, scale=True, res="sep"), 0, 0, "bf16"), ("ln", dict(entry="ln", bias=True), 0, 1, None),
                               ("swiglu", dict(entry="gemm", act=2), 2, 0, None)):
        out.append(Case(name=f"rows-{nm}", M=rows[0], N=rows[1], K=rows[2], **kw, kind="ROWS", want=(st("big", a, ln, res), st("small", a, ln, res))))
        if a != 2:   # (SwiGLU has no column split: the (gate, up) groups would part)
            out.append(Case(name=f"cols-{nm}", M=cols[0], N=cols[1], K=cols[2], **kw, kind="COLS", want=(st("big", a, ln, res), st("small", a, ln, res))))
    slab = _gemm_tag("small", 0, True, 0, 1, "direct-vec", slab=True)
    ws = 4 * hyb[0] * 128 * 4
    out.append(Case(name="hybrid-plain", entry="splitk", M=hyb[0], N=hyb[1], K=hyb[2], bias=True, scale=True, res="sep", ws=ws, kind="HYBRID",
                    want=(st("big", 0, 0, "bf16"), slab, "reduce0|bf16-vec+res-bf16-vec")))
    out.append(Case(name="hybrid-swiglu", entry="splitk", M=hyb[0], N=hyb[1], K=hyb[2], act=2, ws=ws, kind="HYBRID",
                    want=(st("big", 2, 0), slab, "reduce2|bf16-vec+res-none")))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
ITEMS = [(c, f) for c in CASES for f in c.families]


def launches(L, c, c_align=None, res_align=None):
    """emmax_gemm_launches for the case as its entry point builds the call (under the tuning switches in force): the lines, or None = refused"""
    esz = 4 if c.f32 else 2
    has_res = c.res != "none" or c.entry == "stream"
    c_align = (c.c_off * esz) % 16 if c_align is None else c_align
    if res_align is None:
        res_align = c_align if c.res != "sep" else 0
    K = 2 * c.K if c.hl else c.K
    return L.gemm_launches(c.M, c.N, K, act=c.act, out_f32=c.f32, ln=c.entry == "ln", residual=(2 if c.res_f32 else 1) if has_res else 0, norm=c.norm, ws_bytes=c.ws,
                           bias=c.bias and c.entry != "ln", scale=c.scale, lda=K if c.hl else c.K + c.lda_pad, ldw=c.K + c.ldw_pad, ldc=c.ldc,
                           ldr=(c.ldr if c.res == "sep" else c.ldc), n_store=c.N if c.act == 2 else c.n_out, a_hl=int(c.hl), c_align=c_align, res_align=res_align,
                           ksplit=c.ksplit)


def parts(lines):
    """(r0, n1) of a plan's parts from its launch lines: the first row of the second row part, the first column of the second column part (0: none)"""
    r0 = n1 = 0
    for ln in lines:
        _, d = parse_line(ln)
        r0, n1 = max(r0, int(d["rows"].split("..")[0])), max(n1, int(d["cols"].split("..")[0]))
    return r0, n1


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------
def sample_rows(c):
    """the rows the CPU measures on: all of a small case; of a large one the first and last rows, the rows around every tile-row boundary a plan
    may split at, and a spread of others.  (The emulation is element by element: a subset of the rows is a subset of the elements.)"""
    if c.M * c.N * c.K <= 2 ** 29:
        return None
    pick = {0, 1, c.M - 1, c.M - 2, c.M // 2, c.M // 3}
    pick |= {r for b in range(256, c.M, max(256, c.M // 8 // 256 * 256)) for r in (b - 1, b)}
    return torch.tensor(sorted(r for r in pick if 0 <= r < c.M)[:24])


def operands(c, family, rows=None):
    """CPU tensors of the case: A (bf16; x: fp32) [M, K], W bf16 [N, K], bias / scale bf16 [N], res (bf16 / fp32 [M, n_out]), gamma / beta (ln),
    norm_w.  rows: only these rows of A and res (the random streams are drawn for the whole case first, so a subset sees the same values)."""
    M, N, K = c.M, c.N, c.K
    tag = len(c.same_as or c.name)   # (a non-default main loop runs the operands of the case it must equal)
    g = gen(97, M, N, K, c.act, tag)
    o = {}
    if family == "ties":
        assert c.act == 0 and c.entry != "ln"
        A = torch.randint(0, 4, (M, K), generator=g).float()
        W = torch.randint(0, 4, (N, K), generator=g).float() * (torch.randint(0, 2, (N, 1), generator=g).float() * 2 - 1)
        o["A"] = A if c.hl else bf(A)
        o["W"] = bf(W)
        o["bias"] = bf(torch.randint(-8, 9, (N,), generator=g).float())
        o["scale"] = bf(torch.tensor([1.0, 1.5, 2.0])[torch.randint(0, 3, (N,), generator=g)])
        r = torch.randint(-64, 65, (M, c.n_out), generator=g).float()
        o["res"] = r + 0.25 if c.res_f32 else bf(r)
    else:
        A, W, bias, scale = P.gemm_operands(M, N, K, (M, N, K, c.act, tag))
        if c.entry == "ln":   # raw rows with a mean and a spread of their own per row: mean x ln_s is a large part of the accumulator
            A = bf(A.float() * (0.5 + torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g))
            o["gamma"] = bf(1.0 + 0.2 * torch.randn(K, generator=g))
            o["beta"] = bf(0.3 * torch.randn(K, generator=g))
        if c.hl:
            A = torch.randn(M, K, generator=g)   # fp32 rows: 24 significant bits, two bf16 terms keep 16
        if c.act == 2:
            W = bf(W.float() * 1.5)
        o.update(A=A, W=W, bias=bias, scale=scale)
        r = torch.randn(M, c.n_out, generator=g) * 2.0
        o["res"] = r if c.res_f32 else bf(r)
    if c.norm:
        o["norm_w"] = bf(1.0 + 0.1 * torch.randn(N, generator=g))
    if not c.bias:
        o["bias"] = None
    if not c.scale:
        o["scale"] = None
    if c.res == "none" and c.entry != "stream":
        o["res"] = None
    if family == "cancel":
        assert c.act == 0 and c.entry != "ln"
        term = reference(c, dict(o, res=None))[0]
        if o["res"] is not None:
            o["res"] = (-term).float() if c.res_f32 else bf(-term)
        else:   # row 0 cancels against the bias
            o["bias"] = bf(o["bias"].double() - term[0])
    if rows is not None:
        o["A"] = o["A"][rows]
        if o["res"] is not None:
            o["res"] = o["res"][rows]
    return o


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def swiglu_pairs(p):
    """[M, N] in the interleaved weight order -> (gate, up) [M, N / 2]: 16-column groups alternate"""
    M, N = p.shape
    v = p.view(M, N // 32, 2, 16)
    return v[:, :, 0].reshape(M, N // 2), v[:, :, 1].reshape(M, N // 2)


def reference(c, o):
    """float64 (result [M, n_out], term = result - residual) on the device of the operands"""
    A, W = o["A"].double(), o["W"].double()
    if c.entry == "ln":
        Wf = V.fold_bits(o["W"].cpu(), o["gamma"].cpu()).view(torch.bfloat16).to(A.device).double()   # the rounded W' the GEMM multiplies by
        mean = A.mean(-1, keepdim=True)
        rstd = torch.rsqrt((A - mean).pow(2).mean(-1, keepdim=True) + LN_EPS)
        ln_c = (W * o["beta"].double()).sum(-1) + (o["bias"].double() if o["bias"] is not None else 0.0)
        v = rstd * (A @ Wf.t() - mean * Wf.sum(-1)) + ln_c
    else:
        v = A @ W.t()
        if o["bias"] is not None:
            v = v + o["bias"].double()
    if c.act == 1:
        v = gelu64(v)
    if c.act == 2:
        gate, up = swiglu_pairs(v)
        v = gate * torch.sigmoid(gate) * up
    if o["scale"] is not None:
        v = v * o["scale"].double()
    v = v[:, : c.n_out]
    return (v + o["res"].double() if o["res"] is not None else v), v


def ref_norm(c, o, stream64):
    return P.ref_rmsnorm(stream64, o["norm_w"].double().to(stream64.device), P.NORM_EPS)


# ---- the fp32 emulation ---------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c_):
    """fp32 fused multiply-add: exact in float64 up to a double rounding 2^-29 below the fp32 ulp"""
    return (a.double() * b.double() + c_).float()


def emu_gelu(x):
    """common.h gelu_erf: max(x, 0) - |x| exp2(Q(min(|x|, 6))), Q a degree-6 polynomial by Horner with fused steps"""
    a = x.abs().clamp(max=6.0)
    q = fma32(torch.full_like(a, 3.3092673036e-05), a, torch.tensor(-7.6921858316e-04, dtype=torch.float32).double())
    for cf in (8.0807131948e-03, -5.3412099418e-02, -4.5877097672e-01, -1.1512017009e+00, -9.9999306113e-01):
        q = fma32(q, a, torch.tensor(cf, dtype=torch.float32).double())
    return fma32(-x.abs(), torch.exp2(q), x.clamp(min=0.0).double())


def emu_silu(x, precise=False):
    if precise:   # silu_precise: x / (1 + exp(-x))
        return x / (1.0 + torch.exp(-x))
    return x * (1.0 / (1.0 + torch.exp2(torch.tensor(-1.4426950408889634, dtype=torch.float32) * x)))


def trunc_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emu_acc(A, W, ks=1, hl=False, drop_last=False, drop_chunk=False):
    """fp32 accumulators: per K slice the products one by one in k order (a product of two bf16 values is exact: one rounding per step), the
    slices summed in order.  A fp32 [M, Kp] of bf16 values (HL: per 64 columns [64 hi][64 lo]), W fp32 [N, K]."""
    Kp = A.shape[1]
    nk = Kp // 64
    per = -(-nk // ks)
    total = None
    for s in range(ks):
        acc = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float32)
        t1 = min((s + 1) * per, nk)
        if drop_last and s == ks - 1 and nk % ks:
            t1 -= 1            # planted: the last K step of the short slice
        for t in range(s * per, t1):
            for k in range(64):
                if drop_chunk and t == 0 and 8 <= k < 16:
                    continue   # planted: one 8-element chunk
                acc.addcmul_(A[:, t * 64 + k][:, None], W[:, ((t >> 1) if hl else t) * 64 + k][None, :])
        total = acc if total is None else total + acc
    return total


def hl_rows(A32):
    """fp32 [M, K] -> [M, 2 K] of bf16 values, per 64 columns [64 x hi][64 x lo], hi = bf16(x), lo = bf16(x - hi) (exact.hip)"""
    hi = bfr(A32)
    lo = bfr(A32 - hi)
    M, K = A32.shape
    return torch.stack([hi.view(M, K // 64, 64), lo.view(M, K // 64, 64)], 2).reshape(M, 2 * K)


def emulate(c, o, plant="", r0=0, n1=0, row_ids=None):
    """fp32: what the kernels compute, and what they store (bf16 results: rounded to nearest even).  Returns (stored values as fp32, fp32 value in
    front of the last rounding).  plant: one of PLANTS -- the same arithmetic with one error built in.  r0 / n1: the parts of the plan (for the
    planted offset errors); row_ids: the rows of the case the operands hold (None: all)."""
    ks = max(c.ksplit, 1)
    if c.kind in ("SPLITK", "HYBRID") and c.ksplit == 0:
        ks = 4   # (planned slices: sk-hl-ks4 and the hybrid cases, pinned by their `want` and tests/test_gemm_plan.py)
    A = hl_rows(o["A"].float()) if c.hl else o["A"].float()
    Wf = V.fold_bits(o["W"], o["gamma"]).view(torch.bfloat16).float() if c.entry == "ln" else o["W"].float()
    kw = dict(drop_last=plant == "drop_last_kstep", drop_chunk=plant == "drop_chunk")
    if c.kind == "HYBRID":   # columns [0, n1) whole, columns [n1, N) in slices
        n1_ = n1 or (c.N - 128)
        acc = torch.cat([emu_acc(A, Wf[:n1_], **kw), emu_acc(A, Wf[n1_:], ks=ks, **kw)], 1)
    else:
        acc = emu_acc(A, Wf, ks=ks, hl=c.hl, **kw)
    N = c.N
    col = torch.arange(N)
    shift = torch.where(col >= n1, col - n1, col) if n1 else col
    if c.entry == "ln":
        mean, rstd = V.emu_row_stats(o["A"], LN_EPS)
        if plant == "stats_no_offset" and r0:   # rows of the second part read the statistics of rows 0 .. (where the sample holds that row)
            ids = (torch.arange(c.M) if row_ids is None else row_ids).tolist()
            pos = {r: i for i, r in enumerate(ids)}
            src = torch.tensor([pos.get(r - r0, i) if r >= r0 else i for i, r in enumerate(ids)])
            mean, rstd = mean[src], rstd[src]
        ln_s, ln_c = V.emu_fold_sums(o["W"], o["gamma"], o["beta"], o["bias"])
        if plant == "lnc_no_offset":
            ln_c = ln_c[shift]
        if plant == "drop_mean":
            v = acc * rstd[:, None] + ln_c[None, :]
        else:
            v = (acc - mean[:, None] * ln_s[None, :]) * rstd[:, None] + ln_c[None, :]
    else:
        b = o["bias"].float() if o["bias"] is not None else None
        if b is not None and plant == "bias_no_offset":
            b = b[shift]
        v = acc + b if b is not None and plant != "bias_after_gelu" else acc
    if c.act == 1:
        v = emu_gelu(v)
        if plant == "bias_after_gelu" and o["bias"] is not None:
            v = v + o["bias"].float()
    if c.act == 2:
        gate, up = swiglu_pairs(v)
        if plant == "swap_gate_up":
            gate, up = up, gate
        v = emu_silu(gate, precise=c.f32) * up
    res = o["res"].float()[:, : c.n_out] if o["res"] is not None else None
    sc = o["scale"].float() if o["scale"] is not None else None
    if plant == "scale_on_res" and sc is not None and res is not None:
        v = (v[:, : c.n_out] + res) * sc[: c.n_out]
        res = sc = None
    if sc is not None:
        v = v * sc
    v = v[:, : c.n_out]
    if res is not None:
        if plant == "round_before_res":
            v = bfr(v)
        v = v + res
    if c.f32:
        return v, v
    return (trunc_bf16(v) if plant == "trunc" else bfr(v)), v


PLANTS = {   # planted error -> which cases it concerns (the emulation with it must miss the bound on at least one case of every family it touches)
    "trunc": lambda c: not c.f32,
    "round_before_res": lambda c: not c.f32 and c.res != "none",
    "bias_after_gelu": lambda c: c.act == 1 and c.bias and c.entry != "ln",
    "scale_on_res": lambda c: c.scale and (c.res != "none" or c.entry == "stream"),
    "swap_gate_up": lambda c: c.act == 2,
    "drop_mean": lambda c: c.entry == "ln",
    "drop_last_kstep": lambda c: c.ksplit > 1 and (c.K // 64) % c.ksplit != 0,
    "drop_chunk": lambda c: True,
    "bias_no_offset": lambda c: c.kind in ("COLS", "HYBRID") and c.bias and c.entry != "ln",
    "lnc_no_offset": lambda c: c.kind == "COLS" and c.entry == "ln",
    "stats_no_offset": lambda c: c.kind == "ROWS" and c.entry == "ln",
}


# ---- the bound ----------------------------------------------------------------------------------------------------------------------------------
def half_ulp_bf16(x):
    """half the spacing of bf16 at |x| (float64), from the exponent: |x| = f 2^q, f in [0.5, 1) -> spacing 2^(q - 8); never below the spacing of
    the smallest normal binade"""
    _, q = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.exp2((q - 9).double())


def a32(c, ref, term, spread, unit):
    return RT * ref.abs() + ACT_RTOL[c.act] * term.abs() + ORDER * spread * unit


def allowed(c, ref, term, spread, unit=None):
    """the bound of the module docstring, element by element (float64).  unit: rms(term) of the WHOLE case"""
    unit = term.pow(2).mean().sqrt().item() if unit is None else unit
    a = a32(c, ref, term, spread, unit)
    return a if c.f32 else a + half_ulp_bf16(ref.abs() + a)


def spread_of(c, v32, ref, term, unit=None):
    """what the fp32 value in front of the last rounding leaves above 2^-24 |ref| + ACT_RTOL |term|, in units of rms(term)"""
    unit = term.pow(2).mean().sqrt().item() if unit is None else unit
    return ((v32.double() - ref).abs() - RT * ref.abs() - ACT_RTOL[c.act] * term.abs()).clamp_min(0).max().item() / unit


def worst_ratio(got, ref, allow):
    return ((got.double() - ref).abs() / allow).max().item()


def todays_line(c, ref, term):
    """the line tests/test_ops_gpu.py holds these kernels to: no bound here may exceed it.  (Its absolute part is a fraction of the largest
    output of a product that does not cancel: for the `cancel` family that is the largest term.)"""
    m = torch.maximum(ref.abs().max(), term.abs().max())
    return (1e-4 * ref.abs() + 1e-4 * m) if c.f32 else (1e-2 * ref.abs() + 4e-3 * m)


def measure(c, family, plant="", r0=0, n1=0):
    """(spread of the emulation, worst |stored - ref| / allowed under the TABLE's spread, fraction of `allowed` of today's line at its tightest)
    on the case's own inputs, on the CPU"""
    rows = sample_rows(c)
    o = operands(c, family, rows)
    ref, term = reference(c, o)
    stored, v32 = emulate(c, o, plant, r0, n1, rows)
    s = spread_of(c, v32, ref, term)
    allow = allowed(c, ref, term, SPREAD.get((c.name, family), s))
    return s, worst_ratio(stored, ref, allow), (allow / todays_line(c, ref, term)).max().item()


# (case, family) -> the spread the emulation measures (units of rms(term)); `python tests/gemm_ref.py` prints this table, tests/test_gemm_ref.py
# holds every re-measurement to at most 1.05 x its entry and at least 2 / 3 of it.  `ties` has no entry: its results are exact.
SPREAD = {
    ('small-plain-1x128x64', 'random'): 1.13e-07,   # stored / allowed 0.99, allowed / today's line 0.235
    ('small-plain-1x128x64', 'cancel'): 1.44e-07,   # stored / allowed 0.96, allowed / today's line 0.00105
    ('small-plain-145x384x192', 'random'): 1.11e-06,   # stored / allowed 1.00, allowed / today's line 0.247
    ('small-plain-145x384x192', 'cancel'): 1.28e-06,   # stored / allowed 0.90, allowed / today's line 0.00127
    ('small-plain-256x640x320', 'random'): 1.35e-06,   # stored / allowed 1.00, allowed / today's line 0.249
    ('small-plain-256x640x320', 'cancel'): 1.39e-06,   # stored / allowed 0.92, allowed / today's line 0.00196
    ('small-stream-1x384x320', 'random'): 1.17e-06,   # stored / allowed 0.54, allowed / today's line 0.00334
    ('small-stream-1x384x320', 'cancel'): 1.23e-06,   # stored / allowed 0.50, allowed / today's line 0.00632
    ('small-stream-145x640x64', 'random'): 5.84e-07,   # stored / allowed 0.58, allowed / today's line 0.00117
    ('small-stream-145x640x64', 'cancel'): 7.41e-07,   # stored / allowed 0.50, allowed / today's line 0.00227
    ('small-stream-256x128x192', 'random'): 7.61e-07,   # stored / allowed 0.56, allowed / today's line 0.00177
    ('small-stream-256x128x192', 'cancel'): 8.84e-07,   # stored / allowed 0.50, allowed / today's line 0.00307
    ('small-gelu-1x640x192', 'random'): 3.02e-07,   # stored / allowed 1.00, allowed / today's line 0.256
    ('small-gelu-145x128x320', 'random'): 1.23e-06,   # stored / allowed 1.00, allowed / today's line 0.243
    ('small-gelu-256x384x64', 'random'): 5.13e-07,   # stored / allowed 1.00, allowed / today's line 0.241
    ('small-gelu32-1x128x64', 'random'): 5.88e-08,   # stored / allowed 0.78, allowed / today's line 0.000961
    ('small-gelu32-145x384x192', 'random'): 8.76e-07,   # stored / allowed 0.57, allowed / today's line 0.00173
    ('small-gelu32-256x640x320', 'random'): 1.9e-06,   # stored / allowed 0.57, allowed / today's line 0.00317
    ('small-swiglu-1x384x320', 'random'): 5.82e-07,   # stored / allowed 1.00, allowed / today's line 0.245
    ('small-swiglu-145x640x64', 'random'): 4.03e-07,   # stored / allowed 1.00, allowed / today's line 0.243
    ('small-swiglu-256x128x192', 'random'): 8.38e-07,   # stored / allowed 1.00, allowed / today's line 0.259
    ('small-swiglu32-1x640x192', 'random'): 2.09e-05,   # stored / allowed 0.51, allowed / today's line 0.0489
    ('small-swiglu32-145x128x320', 'random'): 2.93e-05,   # stored / allowed 0.54, allowed / today's line 0.0333
    ('small-swiglu32-256x384x64', 'random'): 4.6e-05,   # stored / allowed 0.51, allowed / today's line 0.0465
    ('small-ln-1x128x64', 'random'): 2.68e-07,   # stored / allowed 0.98, allowed / today's line 0.237
    ('small-ln-145x384x192', 'random'): 1.53e-06,   # stored / allowed 1.00, allowed / today's line 0.266
    ('small-ln-256x640x320', 'random'): 3.2e-06,   # stored / allowed 1.00, allowed / today's line 0.254
    ('small-ln_gelu-1x384x320', 'random'): 1.66e-06,   # stored / allowed 1.00, allowed / today's line 0.227
    ('small-ln_gelu-145x640x64', 'random'): 7.77e-07,   # stored / allowed 1.00, allowed / today's line 0.261
    ('small-ln_gelu-256x128x192', 'random'): 1.5e-06,   # stored / allowed 1.00, allowed / today's line 0.258
    ('small-direct-ldc4-off8B', 'random'): 1.11e-06,   # stored / allowed 1.00, allowed / today's line 0.247
    ('small-direct-ldc2', 'random'): 8.63e-07,   # stored / allowed 1.00, allowed / today's line 0.253
    ('small-direct-ldr2', 'random'): 8.63e-07,   # stored / allowed 1.00, allowed / today's line 0.253
    ('small-direct-ldr2-ldc2', 'random'): 9.48e-07,   # stored / allowed 1.00, allowed / today's line 0.255
    ('small-direct-alias', 'random'): 8.39e-07,   # stored / allowed 1.00, allowed / today's line 0.243
    ('small-direct-alias-ldc4', 'random'): 1.11e-06,   # stored / allowed 1.00, allowed / today's line 0.247
    ('small-direct-f32-bf16res', 'random'): 1.3e-06,   # stored / allowed 0.51, allowed / today's line 0.00283
    ('small-direct-f32-bf16res-ldc1', 'random'): 1.07e-06,   # stored / allowed 0.53, allowed / today's line 0.00253
    ('small-direct-gelu-ldc4', 'random'): 1.03e-06,   # stored / allowed 1.00, allowed / today's line 0.237
    ('small-direct-swiglu-ldc4', 'random'): 9.27e-07,   # stored / allowed 1.00, allowed / today's line 0.232
    ('small-direct-swiglu-ldc2', 'random'): 9.27e-07,   # stored / allowed 1.00, allowed / today's line 0.232
    ('small-direct-ln-ldc4', 'random'): 1.53e-06,   # stored / allowed 1.00, allowed / today's line 0.266
    ('small-direct-ln-gelu-ldc2', 'random'): 1.69e-06,   # stored / allowed 1.00, allowed / today's line 0.265
    ('small-direct-ln-ldc2', 'random'): 1.53e-06,   # stored / allowed 1.00, allowed / today's line 0.266
    ('small-direct-ln-gelu-ldc4', 'random'): 1.69e-06,   # stored / allowed 1.00, allowed / today's line 0.265
    ('small-direct-gelu-ldc2', 'random'): 1.03e-06,   # stored / allowed 1.00, allowed / today's line 0.237
    ('small-direct-gelu-res', 'random'): 1.18e-06,   # stored / allowed 1.00, allowed / today's line 0.254
    ('small-direct-gelu-res-ldr2', 'random'): 1.32e-06,   # stored / allowed 1.00, allowed / today's line 0.265
    ('small-direct-gelu32-ldc1', 'random'): 8.76e-07,   # stored / allowed 0.57, allowed / today's line 0.00173
    ('small-direct-stream-ldc1', 'random'): 1.3e-06,   # stored / allowed 0.51, allowed / today's line 0.00283
    ('small-direct-f32-gelu-bf16res', 'random'): 1.24e-06,   # stored / allowed 0.56, allowed / today's line 0.00235
    ('small-direct-swiglu32-ldc1', 'random'): 3.58e-05,   # stored / allowed 0.52, allowed / today's line 0.0372
    ('small-direct-f32-swiglu', 'random'): 8.78e-07,   # stored / allowed 0.64, allowed / today's line 0.00214
    ('small-hl-145x384x192', 'random'): 1.08e-05,   # stored / allowed 0.50, allowed / today's line 0.0238
    ('small-hl-145x384x192', 'cancel'): 1.09e-05,   # stored / allowed 0.50, allowed / today's line 0.0517
    ('small-hl-gelu-145x128x64', 'random'): 1.87e-05,   # stored / allowed 0.50, allowed / today's line 0.0596
    ('big-plain-1x128x64', 'random'): 1.42e-07,   # stored / allowed 0.99, allowed / today's line 0.242
    ('big-plain-1x128x64', 'cancel'): 2.4e-07,   # stored / allowed 0.93, allowed / today's line 0.0012
    ('big-plain-273x384x192', 'random'): 1.34e-06,   # stored / allowed 1.00, allowed / today's line 0.255
    ('big-plain-273x384x192', 'cancel'): 1.46e-06,   # stored / allowed 0.90, allowed / today's line 0.00142
    ('big-plain-512x1280x320', 'random'): 1.68e-06,   # stored / allowed 1.00, allowed / today's line 0.248
    ('big-plain-512x1280x320', 'cancel'): 1.73e-06,   # stored / allowed 0.89, allowed / today's line 0.00198
    ('big-stream-1x384x320', 'random'): 4.6e-07,   # stored / allowed 0.56, allowed / today's line 0.00138
    ('big-stream-1x384x320', 'cancel'): 6.67e-07,   # stored / allowed 0.50, allowed / today's line 0.00402
    ('big-stream-273x1280x64', 'random'): 7.31e-07,   # stored / allowed 0.61, allowed / today's line 0.00142
    ('big-stream-273x1280x64', 'cancel'): 9.44e-07,   # stored / allowed 0.50, allowed / today's line 0.00258
    ('big-stream-512x128x192', 'random'): 1.04e-06,   # stored / allowed 0.54, allowed / today's line 0.00227
    ('big-stream-512x128x192', 'cancel'): 1.21e-06,   # stored / allowed 0.50, allowed / today's line 0.0038
    ('big-gelu-1x1280x192', 'random'): 6.06e-07,   # stored / allowed 1.00, allowed / today's line 0.228
    ('big-gelu-273x128x320', 'random'): 1.53e-06,   # stored / allowed 1.00, allowed / today's line 0.224
    ('big-gelu-512x384x64', 'random'): 5.1e-07,   # stored / allowed 1.00, allowed / today's line 0.229
    ('big-gelu32-1x128x64', 'random'): 5.5e-08,   # stored / allowed 0.81, allowed / today's line 0.000782
    ('big-gelu32-273x384x192', 'random'): 1e-06,   # stored / allowed 0.62, allowed / today's line 0.00199
    ('big-gelu32-512x1280x320', 'random'): 2.38e-06,   # stored / allowed 0.54, allowed / today's line 0.00352
    ('big-swiglu-1x384x320', 'random'): 4.39e-07,   # stored / allowed 1.00, allowed / today's line 0.258
    ('big-swiglu-273x1280x64', 'random'): 4.12e-07,   # stored / allowed 1.00, allowed / today's line 0.222
    ('big-swiglu-512x128x192', 'random'): 1.48e-06,   # stored / allowed 1.00, allowed / today's line 0.236
    ('big-swiglu32-1x1280x192', 'random'): 2.21e-05,   # stored / allowed 0.51, allowed / today's line 0.0511
    ('big-swiglu32-273x128x320', 'random'): 5.29e-05,   # stored / allowed 0.51, allowed / today's line 0.0796
    ('big-swiglu32-512x384x64', 'random'): 7.19e-05,   # stored / allowed 0.51, allowed / today's line 0.081
    ('big-ln-1x128x64', 'random'): 3.07e-07,   # stored / allowed 1.00, allowed / today's line 0.233
    ('big-ln-273x384x192', 'random'): 3.14e-06,   # stored / allowed 1.00, allowed / today's line 0.251
    ('big-ln-512x1280x320', 'random'): 2.51e-06,   # stored / allowed 1.00, allowed / today's line 0.252
    ('big-ln_gelu-1x384x320', 'random'): 8.97e-07,   # stored / allowed 0.99, allowed / today's line 0.241
    ('big-ln_gelu-273x1280x64', 'random'): 1.92e-06,   # stored / allowed 1.00, allowed / today's line 0.25
    ('big-ln_gelu-512x128x192', 'random'): 4.33e-06,   # stored / allowed 1.00, allowed / today's line 0.26
    ('big-direct-ldc4-off8B', 'random'): 1.34e-06,   # stored / allowed 1.00, allowed / today's line 0.255
    ('big-direct-ldc2', 'random'): 8.59e-07,   # stored / allowed 1.00, allowed / today's line 0.239
    ('big-direct-ldr2', 'random'): 8.59e-07,   # stored / allowed 1.00, allowed / today's line 0.239
    ('big-direct-ldr2-ldc2', 'random'): 1.11e-06,   # stored / allowed 1.00, allowed / today's line 0.245
    ('big-direct-alias', 'random'): 1.01e-06,   # stored / allowed 1.00, allowed / today's line 0.252
    ('big-direct-alias-ldc4', 'random'): 1.34e-06,   # stored / allowed 1.00, allowed / today's line 0.255
    ('big-direct-f32-bf16res', 'random'): 9.28e-07,   # stored / allowed 0.56, allowed / today's line 0.00203
    ('big-direct-f32-bf16res-ldc1', 'random'): 9.19e-07,   # stored / allowed 0.56, allowed / today's line 0.00204
    ('big-direct-gelu-ldc4', 'random'): 1.02e-06,   # stored / allowed 1.00, allowed / today's line 0.242
    ('big-direct-swiglu-ldc4', 'random'): 9.32e-07,   # stored / allowed 1.00, allowed / today's line 0.25
    ('big-direct-swiglu-ldc2', 'random'): 9.32e-07,   # stored / allowed 1.00, allowed / today's line 0.25
    ('big-direct-ln-ldc4', 'random'): 3.14e-06,   # stored / allowed 1.00, allowed / today's line 0.251
    ('big-direct-ln-gelu-ldc2', 'random'): 1.76e-06,   # stored / allowed 1.00, allowed / today's line 0.256
    ('big-direct-ln-ldc2', 'random'): 3.14e-06,   # stored / allowed 1.00, allowed / today's line 0.251
    ('big-direct-ln-gelu-ldc4', 'random'): 1.76e-06,   # stored / allowed 1.00, allowed / today's line 0.256
    ('big-direct-gelu-ldc2', 'random'): 1.02e-06,   # stored / allowed 1.00, allowed / today's line 0.242
    ('big-direct-gelu-res', 'random'): 1.3e-06,   # stored / allowed 1.00, allowed / today's line 0.237
    ('big-direct-gelu-res-ldr2', 'random'): 1.17e-06,   # stored / allowed 1.00, allowed / today's line 0.241
    ('big-direct-gelu32-ldc1', 'random'): 1e-06,   # stored / allowed 0.62, allowed / today's line 0.00199
    ('big-direct-stream-ldc1', 'random'): 9.28e-07,   # stored / allowed 0.56, allowed / today's line 0.00203
    ('big-direct-f32-gelu-bf16res', 'random'): 9.47e-07,   # stored / allowed 0.62, allowed / today's line 0.00176
    ('big-direct-swiglu32-ldc1', 'random'): 4.95e-05,   # stored / allowed 0.51, allowed / today's line 0.0673
    ('big-direct-f32-swiglu', 'random'): 1.06e-06,   # stored / allowed 0.74, allowed / today's line 0.00211
    ('big-hl-273x384x192', 'random'): 1.04e-05,   # stored / allowed 0.50, allowed / today's line 0.0247
    ('big-hl-273x384x192', 'cancel'): 1.05e-05,   # stored / allowed 0.50, allowed / today's line 0.0435
    ('big-hl-gelu-273x128x64', 'random'): 1.99e-05,   # stored / allowed 0.50, allowed / today's line 0.0613
    ('k32-plain-1x128x64', 'random'): 1.42e-07,   # stored / allowed 0.99, allowed / today's line 0.242
    ('k32-plain-1x128x64', 'cancel'): 2.4e-07,   # stored / allowed 0.93, allowed / today's line 0.0012
    ('k32-plain-273x384x192', 'random'): 1.34e-06,   # stored / allowed 1.00, allowed / today's line 0.255
    ('k32-plain-273x384x192', 'cancel'): 1.46e-06,   # stored / allowed 0.90, allowed / today's line 0.00142
    ('k32-plain-256x1280x320', 'random'): 1.5e-06,   # stored / allowed 1.00, allowed / today's line 0.256
    ('k32-plain-256x1280x320', 'cancel'): 1.57e-06,   # stored / allowed 0.89, allowed / today's line 0.00122
    ('k32-stream-1x384x320', 'random'): 4.6e-07,   # stored / allowed 0.56, allowed / today's line 0.00138
    ('k32-stream-1x384x320', 'cancel'): 6.67e-07,   # stored / allowed 0.50, allowed / today's line 0.00402
    ('k32-stream-273x1280x64', 'random'): 7.31e-07,   # stored / allowed 0.61, allowed / today's line 0.00142
    ('k32-stream-273x1280x64', 'cancel'): 9.44e-07,   # stored / allowed 0.50, allowed / today's line 0.00258
    ('k32-stream-256x128x192', 'random'): 8.66e-07,   # stored / allowed 0.56, allowed / today's line 0.00214
    ('k32-stream-256x128x192', 'cancel'): 1.18e-06,   # stored / allowed 0.50, allowed / today's line 0.00511
    ('k32-gelu-1x1280x192', 'random'): 6.06e-07,   # stored / allowed 1.00, allowed / today's line 0.228
    ('k32-gelu-273x128x320', 'random'): 1.53e-06,   # stored / allowed 1.00, allowed / today's line 0.224
    ('k32-gelu-256x384x64', 'random'): 4.88e-07,   # stored / allowed 1.00, allowed / today's line 0.238
    ('k32-gelu32-1x128x64', 'random'): 5.5e-08,   # stored / allowed 0.81, allowed / today's line 0.000782
    ('k32-gelu32-273x384x192', 'random'): 1e-06,   # stored / allowed 0.62, allowed / today's line 0.00199
    ('k32-gelu32-256x1280x320', 'random'): 1.93e-06,   # stored / allowed 0.56, allowed / today's line 0.00323
    ('k32-swiglu-1x384x320', 'random'): 4.39e-07,   # stored / allowed 1.00, allowed / today's line 0.258
    ('k32-swiglu-273x1280x64', 'random'): 4.12e-07,   # stored / allowed 1.00, allowed / today's line 0.222
    ('k32-swiglu-256x128x192', 'random'): 9.86e-07,   # stored / allowed 1.00, allowed / today's line 0.238
    ('k32-ln-1x128x64', 'random'): 3.07e-07,   # stored / allowed 1.00, allowed / today's line 0.233
    ('k32-ln-273x384x192', 'random'): 3.14e-06,   # stored / allowed 1.00, allowed / today's line 0.251
    ('k32-ln-256x1280x320', 'random'): 2.56e-06,   # stored / allowed 1.00, allowed / today's line 0.249
    ('k32-ln_gelu-1x384x320', 'random'): 8.97e-07,   # stored / allowed 0.99, allowed / today's line 0.241
    ('k32-ln_gelu-273x1280x64', 'random'): 1.92e-06,   # stored / allowed 1.00, allowed / today's line 0.25
    ('k32-ln_gelu-256x128x192', 'random'): 2.48e-06,   # stored / allowed 1.00, allowed / today's line 0.251
    ('k32-direct-ldc4-off8B', 'random'): 1.34e-06,   # stored / allowed 1.00, allowed / today's line 0.255
    ('k32-direct-ldc2', 'random'): 8.59e-07,   # stored / allowed 1.00, allowed / today's line 0.239
    ('k32-direct-ldr2', 'random'): 8.59e-07,   # stored / allowed 1.00, allowed / today's line 0.239
    ('k32-direct-ldr2-ldc2', 'random'): 1.11e-06,   # stored / allowed 1.00, allowed / today's line 0.245
    ('k32-direct-alias', 'random'): 1.01e-06,   # stored / allowed 1.00, allowed / today's line 0.252
    ('k32-direct-alias-ldc4', 'random'): 1.34e-06,   # stored / allowed 1.00, allowed / today's line 0.255
    ('k32-direct-f32-bf16res', 'random'): 9.28e-07,   # stored / allowed 0.56, allowed / today's line 0.00203
    ('k32-direct-f32-bf16res-ldc1', 'random'): 9.19e-07,   # stored / allowed 0.56, allowed / today's line 0.00204
    ('k32-direct-gelu-ldc4', 'random'): 1.02e-06,   # stored / allowed 1.00, allowed / today's line 0.242
    ('k32-direct-swiglu-ldc4', 'random'): 9.32e-07,   # stored / allowed 1.00, allowed / today's line 0.25
    ('k32-direct-swiglu-ldc2', 'random'): 9.32e-07,   # stored / allowed 1.00, allowed / today's line 0.25
    ('k32-direct-ln-ldc4', 'random'): 3.14e-06,   # stored / allowed 1.00, allowed / today's line 0.251
    ('k32-direct-ln-gelu-ldc2', 'random'): 1.76e-06,   # stored / allowed 1.00, allowed / today's line 0.256
    ('k32-direct-ln-ldc2', 'random'): 3.14e-06,   # stored / allowed 1.00, allowed / today's line 0.251
    ('k32-direct-ln-gelu-ldc4', 'random'): 1.76e-06,   # stored / allowed 1.00, allowed / today's line 0.256
    ('k32-direct-gelu-ldc2', 'random'): 1.02e-06,   # stored / allowed 1.00, allowed / today's line 0.242
    ('k32-direct-gelu-res', 'random'): 1.3e-06,   # stored / allowed 1.00, allowed / today's line 0.237
    ('k32-direct-gelu-res-ldr2', 'random'): 1.17e-06,   # stored / allowed 1.00, allowed / today's line 0.241
    ('k32-direct-gelu32-ldc1', 'random'): 1e-06,   # stored / allowed 0.62, allowed / today's line 0.00199
    ('k32-direct-stream-ldc1', 'random'): 9.28e-07,   # stored / allowed 0.56, allowed / today's line 0.00203
    ('k32-direct-f32-gelu-bf16res', 'random'): 9.47e-07,   # stored / allowed 0.62, allowed / today's line 0.00176
    ('small-walk-513', 'random'): 8.33e-07,   # stored / allowed 1.00, allowed / today's line 0.226
    ('big-walk-259', 'random'): 6.7e-07,   # stored / allowed 1.00, allowed / today's line 0.246
    ('k32-walk-513', 'random'): 7.72e-07,   # stored / allowed 1.00, allowed / today's line 0.251
    ('sk-small-ks2-alias', 'random'): 8.97e-07,   # stored / allowed 1.00, allowed / today's line 0.258
    ('sk-small-ks2-alias', 'cancel'): 1.03e-06,   # stored / allowed 0.92, allowed / today's line 0.0013
    ('sk-small-ks3-sep', 'random'): 5.03e-07,   # stored / allowed 1.00, allowed / today's line 0.256
    ('sk-small-ks5', 'random'): 6.55e-07,   # stored / allowed 1.00, allowed / today's line 0.262
    ('sk-big-ks2-alias', 'random'): 8.27e-07,   # stored / allowed 1.00, allowed / today's line 0.257
    ('sk-big-ks2-alias', 'cancel'): 9.67e-07,   # stored / allowed 0.94, allowed / today's line 0.00129
    ('sk-big-ks3-sep', 'random'): 7.09e-07,   # stored / allowed 1.00, allowed / today's line 0.255
    ('sk-big-ks5', 'random'): 4.95e-07,   # stored / allowed 1.00, allowed / today's line 0.249
    ('sk-elt-ldc2', 'random'): 6.35e-07,   # stored / allowed 1.00, allowed / today's line 0.246
    ('sk-f32-bf16res', 'random'): 8.74e-07,   # stored / allowed 0.54, allowed / today's line 0.00188
    ('sk-gelu', 'random'): 6.69e-07,   # stored / allowed 1.00, allowed / today's line 0.25
    ('sk-gelu-elt', 'random'): 1.01e-06,   # stored / allowed 1.00, allowed / today's line 0.25
    ('sk-gelu-res', 'random'): 1.06e-06,   # stored / allowed 1.00, allowed / today's line 0.258
    ('sk-gelu-res-elt', 'random'): 5.55e-07,   # stored / allowed 1.00, allowed / today's line 0.265
    ('sk-gelu-f32', 'random'): 5.39e-07,   # stored / allowed 0.63, allowed / today's line 0.00131
    ('sk-gelu-f32-elt', 'random'): 1.29e-06,   # stored / allowed 0.53, allowed / today's line 0.00303
    ('sk-stream-gelu', 'random'): 7.59e-07,   # stored / allowed 0.65, allowed / today's line 0.00162
    ('sk-stream-gelu-ldr1', 'random'): 9.03e-07,   # stored / allowed 0.59, allowed / today's line 0.00139
    ('sk-swiglu', 'random'): 7.14e-07,   # stored / allowed 1.00, allowed / today's line 0.255
    ('sk-swiglu-elt', 'random'): 8.13e-07,   # stored / allowed 1.00, allowed / today's line 0.267
    ('sk-stream-alias', 'random'): 6.76e-07,   # stored / allowed 0.53, allowed / today's line 0.00154
    ('sk-stream-alias', 'cancel'): 7.08e-07,   # stored / allowed 0.50, allowed / today's line 0.00253
    ('sk-stream-sep-ldr1', 'random'): 8.37e-07,   # stored / allowed 0.51, allowed / today's line 0.00187
    ('sk-norm-alias', 'random'): 4.3e-07,   # stored / allowed 0.56, allowed / today's line 0.00115
    ('sk-norm-sep', 'random'): 3.83e-07,   # stored / allowed 0.51, allowed / today's line 0.000903
    ('sk-hl-ks4', 'random'): 8.34e-06,   # stored / allowed 0.50, allowed / today's line 0.0227
    ('rows-plain', 'random'): 5.28e-07,   # stored / allowed 1.00, allowed / today's line 0.251
    ('cols-plain', 'random'): 4.33e-07,   # stored / allowed 1.00, allowed / today's line 0.25
    ('rows-ln', 'random'): 7.75e-07,   # stored / allowed 1.00, allowed / today's line 0.25
    ('cols-ln', 'random'): 7.45e-07,   # stored / allowed 1.00, allowed / today's line 0.251
    ('rows-swiglu', 'random'): 3.88e-07,   # stored / allowed 1.00, allowed / today's line 0.22
    ('hybrid-plain', 'random'): 4.94e-06,   # stored / allowed 1.00, allowed / today's line 0.258
    ('hybrid-swiglu', 'random'): 1.13e-05,   # stored / allowed 1.00, allowed / today's line 0.244
}


if __name__ == "__main__":
    torch.set_num_threads(8)
    print("SPREAD = {")
    for c_, f_ in ITEMS:
        if f_ == "ties" or c_.same_as:
            continue
        s_, w_, line_ = measure(c_, f_)
        print(f"    ({c_.name!r}, {f_!r}): {s_:.3g},   # stored / allowed {w_:.2f}, allowed / today's line {line_:.3g}")
    print("}")
