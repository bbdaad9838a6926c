"""gemm.hip on a real MI355X in every form a launch can take, each case through an op entry point (emmax_op_gemm, _splitk, _ln, _stream,
emmax_op_x_gemm) against the float64 reference and the bounds of tests/gemm_ref.py.

Every (case, family) first asserts its launch list (emmax_gemm_launches with the call's real pitches and pointer alignments: the instantiation
and the epilogue branch each kernel takes), then launches twice on fresh buffers and requires bit-equal results (split-K has no atomics; a
ring or barrier race is not deterministic), then checks, in this order: the live elements are finite; everything a kernel must not write
still holds its sentinel bits (the elements in front of C, the rows behind it, the padding columns n_out .. ldc, norm_out's padding, the
scratch behind ks x M x N floats, a separate residual); the bounds; on `ties`, bit equality with round-to-nearest-even of the exact result.
A and W carry NaN guard rows in front and behind and NaN padding columns K .. ld inside their allocations: an edge-tile clamp that reads a
wrong row, or a K offset that leaves the row, turns the result NaN.  The non-default main loops (gemm_deep) of a (geometry, act, output, LN)
must be bit-identical to the default one.  The module prints worst error / bound per (case, family) at its end.

What the obvious breaks do to this file -- each was built into a scratch copy of the library as an in-bounds VALUE error (no wait, barrier or
address touched) and this file run once against it (272 items):
  truncation instead of pack_bf16x2 in the staged epilogue only
      -> 82 fail: 61 `random` and 9 `cancel` items miss the bound by 1.76 .. 2.0 x (one ulp where half is allowed), all 12 staged `ties` items
         fail the bit comparison (14 of 128 .. 19434 of 55680 results); every staged bf16 form of all three geometries, the walk and the
         ROWS / COLS / HYBRID cases included; no direct-epilogue, fp32 or split-K item fails
  LayerScale applied after the residual in the staged epilogue
      -> 42 fail: every staged item with a LayerScale and a residual (21 `random`, 9 `cancel`, worst 6e3 .. 1e6 x the bound; 12 `ties`: 92 of
         128 .. 33320 of 55680 results); rows-plain, cols-plain and hybrid-plain among them
  cs (mean x ln_s) zeroed in the direct epilogue
      -> 12 fail: the four LN cases per geometry that reach the direct epilogue through an unaligned C (ln / ln-gelu at ldc + 2 and + 4), 6e5 .. 1.5e6 x
  u and v swapped in emmax_splitk_reduce_kernel<2>
      -> 3 fail: sk-swiglu, sk-swiglu-elt, hybrid-swiglu (1e5 .. 3e5 x)
  b.bias not offset by n1 in launch_gemm
      -> 2 fail: cols-plain and hybrid-plain (2e5 .. 2e6 x)
  q.ln_stats not offset by r0 in launch_rows
      -> 1 fails: rows-ln (5e5 x: row 256 normalised with the statistics of row 0)
  `n_ok - 4` -> `n_ok` in the staged bias clamp: not built.  The clamp only acts on column groups at or past n_ok, which are never stored, so the
      change cannot alter a stored value; all it does is read 8 bytes past the end of the bias array -- an address error, not a value error.
"""

import pytest
import torch

import gemm_ref as G
import prefill_stage_ref as P

pytestmark = pytest.mark.gpu

S16, S32 = 0x5A5B, 0x5A5B5C5D   # sentinel bit patterns (finite values in both formats)
FRONT = 64                      # sentinel elements in front of C (a multiple of 16 bytes: C's alignment is the case's c_off alone)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\n== GEMM forms: worst |got - ref| / bound ==")
    for (name, family), (w, what) in sorted(WORST.items()):
        print(f"{name:34s} {family:7s} {w:6.3f}  {what}")


def _lib():
    from emmax import _lib

    return _lib, _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sent(n, f32, device):
    return (torch.full((n,), S32, dtype=torch.int32, device=device).view(torch.float32) if f32
            else torch.full((n,), S16, dtype=torch.int16, device=device).view(torch.bfloat16))


def untouched(t):
    if t.numel() == 0:
        return True
    if t.element_size() == 2:
        return bool((t.contiguous().view(torch.int16) == S16).all())
    return bool((t.contiguous().view(torch.int32) == S32).all())


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def guarded(x, ld, device):
    """rows of x inside an allocation of NaN: a guard row in front and behind, padding columns up to ld.  Returns (buffer, pointer of row 0 of x)"""
    rows, cols = x.shape
    buf = torch.full((rows + 2, ld), float("nan"), dtype=x.dtype, device=device)
    buf[1: rows + 1, :cols] = x
    return buf, buf.data_ptr() + ld * x.element_size()


def launch(c, o, device):
    """one call of the case's entry point on fresh buffers.  Returns what the checks need."""
    L, lib = _lib()
    M, N, K = c.M, c.N, c.K
    f32 = c.f32
    esz = 4 if f32 else 2
    Abuf, Ap = guarded(o["A"], K if c.hl else K + c.lda_pad, device)
    Wbuf, Wp = guarded(o["W"], K + c.ldw_pad, device)
    ldc = c.ldc
    Cbuf = sent(FRONT + c.c_off + (M + 2) * ldc, f32, device)
    c0 = FRONT + c.c_off
    Cv = Cbuf[c0: c0 + M * ldc].view(M, ldc)
    Cp = Cbuf.data_ptr() + c0 * esz
    res = o["res"]
    Rbuf = Rv = None
    Rp, ldr = None, 0
    if res is not None and c.res == "sep":
        ldr = c.ldr
        Rbuf = sent(M * ldr + 8, c.res_f32, device)
        Rv = Rbuf[: M * ldr].view(M, ldr)
        Rv[:, : c.n_out] = res
        Rp = Rbuf.data_ptr()
    elif res is not None:
        Cv[:, : c.n_out] = res
        Rp, ldr = Cp, ldc
    R0 = Rbuf.clone() if Rbuf is not None else None
    ws = sent(c.ws // 4 + 1024, True, device) if c.ws else None
    norm_out = sent((M + 1) * (N + 8), False, device).view(M + 1, N + 8) if c.norm else None
    keep = [Abuf, Wbuf]
    if c.entry == "gemm":
        rc = lib.emmax_op_gemm(Ap, K + c.lda_pad, Wp, K + c.ldw_pad, Cp, ldc, M, N, K, L.ptr(o["bias"]), c.act, L.ptr(o["scale"]), Rp, ldr, int(c.out_f32), stream())
    elif c.entry == "splitk":
        rc = lib.emmax_op_gemm_splitk(Ap, K + c.lda_pad, Wp, K + c.ldw_pad, Cp, ldc, M, N, K, L.ptr(o["bias"]), c.act, L.ptr(o["scale"]), Rp, ldr, int(c.out_f32),
                                      c.ksplit, L.ptr(ws), c.ws, stream())
    elif c.entry == "ln":
        keep += [torch.empty(2 * M, dtype=torch.float32, device=device), torch.empty(N, dtype=torch.float32, device=device),
                 torch.empty(N, dtype=torch.float32, device=device)]
        rc = lib.emmax_op_gemm_ln(Ap, K + c.lda_pad, Wp, K + c.ldw_pad, Cp, ldc, M, N, K, o["gamma"].data_ptr(), o["beta"].data_ptr(), L.ptr(o["bias"]), G.LN_EPS, c.act,
                                  keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), stream())
    elif c.entry == "stream":
        rc = lib.emmax_op_gemm_stream(Ap, K + c.lda_pad, Wp, K + c.ldw_pad, Cp, ldc, Rp if c.res == "sep" else None, ldr if c.res == "sep" else 0, M, N, K,
                                      L.ptr(o["bias"]), c.act, L.ptr(o["scale"]), c.n_out, c.ksplit, L.ptr(ws), c.ws, L.ptr(o.get("norm_w")), L.ptr(norm_out),
                                      N + 8 if c.norm else 0, P.NORM_EPS, stream())
    else:
        keep.append(torch.empty(M * 2 * K, dtype=torch.bfloat16, device=device))
        rc = lib.emmax_op_x_gemm(Ap, K, Wp, K + c.ldw_pad, Cp, ldc, M, N, K, L.ptr(o["bias"]), c.act, Rp, ldr, keep[2].data_ptr(), L.ptr(ws), c.ws, stream())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a GPU fault: nothing more may run on this device in this session
        pytest.exit(f"{c.name}: the device faulted ({e}); stopping the session", returncode=3)
    assert rc == 0, (c.name, rc, lib.emmax_last_error())
    return dict(Cbuf=Cbuf, Cv=Cv, c0=c0, Rbuf=Rbuf, R0=R0, ws=ws, norm_out=norm_out, c_align=Cp % 16, res_align=(Rp or 0) % 16)


def check_sentinels(c, r):
    M, ldc = c.M, c.ldc
    assert untouched(r["Cbuf"][: r["c0"]]), "the elements in front of C were written"
    assert untouched(r["Cbuf"][r["c0"] + M * ldc:]), "rows past M were written"
    assert untouched(r["Cv"][:, c.n_out:]), "padding columns n_out .. ldc were written"
    if r["Rbuf"] is not None:
        assert torch.equal(bits(r["Rbuf"]), bits(r["R0"])), "the separate residual (or its padding) was written"
    if r["ws"] is not None:
        assert untouched(r["ws"][c.ws // 4:]), "the scratch behind ks x M x N floats was written"
    if r["norm_out"] is not None:
        assert untouched(r["norm_out"][M:]) and untouched(r["norm_out"][:M, c.N:]), "norm_out: rows past M / padding columns were written"


def run_case(c, family, device):
    """assert the launch list, launch twice, require equal bits and the sentinels; returns (operands on the device, the first result)"""
    L, _ = _lib()
    o = {k: (v.to(device) if v is not None else None) for k, v in G.operands(c, family).items()}
    lines = G.launches(L, c)   # (C and the residual at the alignments the case states: checked against the real pointers below)
    assert lines is not None and tuple(G.tag_of(ln) for ln in lines) == c.want, (c.name, lines, c.want)
    a = launch(c, o, device)
    assert G.launches(L, c, a["c_align"], a["res_align"]) == lines, f"{c.name}: the buffers are not aligned as the case states"
    b = launch(c, o, device)
    assert torch.equal(bits(a["Cbuf"]), bits(b["Cbuf"])), f"{c.name}: two launches on equal inputs differ"
    if c.norm:
        assert torch.equal(bits(a["norm_out"]), bits(b["norm_out"])), f"{c.name}: norm_out of two launches differs"
    got = a["Cv"][:, : c.n_out]
    assert torch.isfinite(got.float()).all(), f"{c.name}: a live element is not finite"
    check_sentinels(c, a)
    return o, a


@pytest.mark.parametrize("c,family", G.ITEMS, ids=[f"{c.name}-{f}" for c, f in G.ITEMS])
def test_gemm_form(device, tune, c, family):
    L, _ = _lib()
    tune(**dict(c.tune))
    o, a = run_case(c, family, device)
    got = a["Cv"][:, : c.n_out]
    if c.same_as:
        base = G.BY_NAME[c.same_as]
        with L.tuning(**{**dict(base.tune), "gemm_deep": -1}):
            _, b = run_case(base, family, device)
        assert torch.equal(bits(got), bits(b["Cv"][:, : c.n_out])), f"{c.name}: not bit-identical to the default main loop ({base.name})"
        WORST[(c.name, family)] = (0.0, f"bit-identical to {base.name}")
        return
    ref, term = G.reference(c, o)
    if family == "ties":
        exact = ref.float()
        assert torch.equal(exact.double(), ref), "the ties family must be exact in fp32"
        want = exact.view(torch.int32) if c.f32 else P.bf16_bits_rne(exact)
        wrong = bits(got) != want
        assert not wrong.any(), f"{c.name}: {int(wrong.sum())} of {wrong.numel()} results are not round-to-nearest-even of the exact value"
        on_tie = int(((exact.view(torch.int32) & 0xFFFF) == 0x8000).sum())
        WORST[(c.name, family)] = (0.0, f"bits equal; {on_tie} results exactly on a bf16 tie")
        return
    unit = term.pow(2).mean().sqrt().item()
    if family == "random" and c.f32:
        assert 0.3 < unit < 4.0, (c.name, unit)   # the inputs are what the table was measured on: a product term of rms ~ 1
    allow = G.allowed(c, ref, term, G.SPREAD[(c.name, family)], unit)
    err = (got.double() - ref).abs()
    w = (err / allow).max().item()
    WORST[(c.name, family)] = (w, f"max|err| {err.max().item():.3g}, rms(term) {unit:.3g}, spread bound {G.ORDER * G.SPREAD[(c.name, family)]:.3g}")
    print(f"{c.name} {family}: worst |err| / bound {w:.3f}; {WORST[(c.name, family)][1]}")
    assert w <= 1.0, f"{c.name} {family}: {int((err > allow).sum())} of {err.numel()} elements miss the bound; worst {w:.3g} x"
    if c.norm:   # norm_out against the float64 RMSNorm of the float64 stream: the norm's own bound + what the stream's fp32 error moves it by
        y = a["norm_out"][: c.M, : c.N].double()
        yr = G.ref_norm(c, o, ref)
        rstd = torch.rsqrt(ref.pow(2).mean(-1, keepdim=True) + P.NORM_EPS)
        a32 = G.a32(c, ref, term, G.SPREAD[(c.name, family)], unit)
        allow_n = P.norm_bound() * (yr.abs() + 2.0 ** -12 * yr.pow(2).mean().sqrt()) + a32 * rstd * o["norm_w"].double().abs() + yr.abs() * a32.max() * rstd
        wn = ((y - yr).abs() / allow_n).max().item()
        print(f"{c.name} {family}: norm_out worst |err| / bound {wn:.3f}")
        assert wn <= 1.0, f"{c.name}: norm_out misses its bound: worst {wn:.3g} x"
