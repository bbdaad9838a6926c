"""The LLM prefill's stage kernels one by one on a real MI355X, each through its op entry point (include/emmax.h, ABI 12) against the float64
or exact reference of tests/prefill_stage_ref.py: the GEMM onto the fp32 residual stream on every code path that honours GemmParams::res_f32,
the RMSNorm of fp32 rows, RoPE + the paged K / V append, the fp8 KV append, embed / splice, the last-row gather.

Every output and cache is pre-filled with a sentinel bit pattern, and every location an op must not write -- padding columns, rows past a
sequence's end, cache slots past each length, pages in no row's table -- is compared bitwise afterwards.  The bounds are the CPU
emulation's (prefill_stage_ref.py, pinned by tests/test_prefill_stage_ref.py); the exact ops are compared bit for bit.

What the obvious breaks do to this file -- each was built into a scratch copy of the library (all in bounds) and this file run against it:
  the fp32 residual rounded to bf16 where the direct epilogue and the reduce pass read it (gemm.hip)
      -> every direct, split and K-slice case misses the stream bound: spread 0.43 .. 0.5 of the product rms against bounds of 1.4e-6 .. 1.7e-5;
         the fused-norm cases fail on "the stream differs between the fused and the unfused reduce pass"
  the same in the reduce pass with the RMSNorm (emmax_splitk_reduce_norm_kernel<8, true>)
      -> every accepted fused-norm case, the one through the launch plan included, misses the stream bound
  slot = (pos + 1) % page in the RoPE kernels and the fp8 append (misc.hip)
      -> all 8 RoPE cases fail the bitwise K-cache comparison, all 5 fp8 cases the comparison of the K bytes
  only the first pass of every strided loop of misc.hip
      -> RoPE fails at (32, 32) heads for both head sizes and, through the element-wise kernel (its loop is per pair, not per 8 pairs),
         wherever heads x head_dim / 2 exceeds 256 threads: every case but (4, 2) heads of 72; the fp8 append fails at Hkv = 9 and 32 (rows 16 and up written back wrong) and passes at 1, 2, 8; splice and
         gather fail at 4096 columns and pass at 64
"""

import math

import pytest
import torch

import prefill_stage_ref as R

pytestmark = pytest.mark.gpu

S16, S32, S8 = 0x5A5B, 0x5A5B5C5D, 0x5A   # sentinel bit patterns (finite values in every format)


def _lib():
    from emmax import _lib

    return _lib, _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sent_bf16(shape, device):
    return torch.full(shape, S16, dtype=torch.int16, device=device).view(torch.bfloat16)


def sent_f32(shape, device):
    return torch.full(shape, S32, dtype=torch.int32, device=device).view(torch.float32)


def same_bits(a, b):
    """bitwise equality of two tensors of one dtype and shape"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def untouched(t):
    """every element of `t` still holds its sentinel"""
    if t.numel() == 0:
        return True
    if t.element_size() == 2:
        return bool((t.contiguous().view(torch.int16) == S16).all())
    if t.element_size() == 4:
        return bool((t.contiguous().view(torch.int32) == S32).all())
    return bool((t.contiguous().view(torch.uint8) == S8).all())


# =============================================================================================================================================
# the GEMM onto the fp32 residual stream
# =============================================================================================================================================
def _stream_gemm(device, M, N, K, *, n_store=None, ldc=None, ksplit=0, ws_bytes=0, separate=False, ldr=None, epi=False, norm=None, seed=0):
    """One call of emmax_op_gemm_stream on fresh operands.  Returns a dict with the stream afterwards, the float64 reference (on the device) and
    what the bound needs; asserts the sentinel checks itself.  norm: (norm_w, ld_norm) -> norm_out comes back too."""
    L, lib = _lib()
    n_store = N if n_store is None else n_store
    ldc = n_store if ldc is None else ldc
    A, W, bias, scale = (t.to(device) for t in R.gemm_operands(M, N, K, (M, N, K, seed)))
    if not epi:
        bias = scale = None
    res = R.stream_rows(M, n_store, (M, N, K, seed)).to(device)
    # C: M rows of ldc floats and two more rows that nothing may touch; padding columns n_store .. ldc likewise
    Cbuf = sent_f32(((M + 2) * ldc,), device)
    Cv = Cbuf[: M * ldc].view(M, ldc)
    if separate:
        ldr = n_store if ldr is None else ldr
        Rbuf = sent_f32((M * ldr,), device)
        Rbuf.view(M, ldr)[:, :n_store] = res
        res_ptr = Rbuf.data_ptr()
    else:
        Cv[:, :n_store] = res     # the stream is its own residual
        res_ptr, ldr = None, 0
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=device) if ws_bytes else None
    norm_out = None
    if norm is not None:
        norm_w, ld_norm = norm
        norm_out = sent_bf16((M + 1, ld_norm), device)
    rc = lib.emmax_op_gemm_stream(A.data_ptr(), K, W.data_ptr(), K, Cbuf.data_ptr(), ldc, res_ptr, ldr, M, N, K, L.ptr(bias), 0, L.ptr(scale), n_store, ksplit,
                                  L.ptr(ws), ws_bytes, norm[0].data_ptr() if norm else None, L.ptr(norm_out), norm[1] if norm else 0, R.NORM_EPS, stream())
    torch.cuda.synchronize()
    out = {"rc": rc, "C": Cv[:, :n_store].clone(), "res": res, "K": K, "norm_out": norm_out, "Cbuf": Cbuf}
    if rc != 0:
        return out
    assert untouched(Cbuf[M * ldc:]), "rows past M were written"
    assert untouched(Cv[:, n_store:]), "padding columns n_store .. ldc were written"
    if separate:
        Rv = Rbuf.view(M, ldr)
        assert same_bits(Rv[:, :n_store], res) and untouched(Rv[:, n_store:]), "the separate residual was written"
    if norm_out is not None:
        assert untouched(norm_out[M:]) and untouched(norm_out[:M, N:]), "norm_out: rows past M / padding columns were written"
    out["ref"] = R.ref_gemm_stream(A, W, res, bias, scale)[:, :n_store]
    return out


def _assert_stream(out, what):
    """|got - ref| <= 2^-24 |ref| + GEMM_ORDER x GEMM_SPREAD[K] x rms(product term), element by element, in float64 on the device"""
    assert out["rc"] == 0, (what, out["rc"], _lib()[1].emmax_last_error())
    got, ref, res = out["C"].double(), out["ref"], out["res"].double()
    assert torch.isfinite(got).all(), what
    unit = (ref - res).pow(2).mean().sqrt().item()
    spread = R.gemm_spread(got, ref, res)
    print(f"{what}: spread {spread:.3g} of the product rms (bound {R.gemm_atol(out['K']):.3g}); max|err| {(got - ref).abs().max().item():.3g}, product rms {unit:.3g}")
    assert 0.5 < unit < 3.0, (what, unit)   # the inputs are what the table was measured on: a product term of rms ~ 1
    assert spread <= R.gemm_atol(out["K"]), f"{what}: the stream misses the fp32 bound: spread {spread:.3g} > {R.gemm_atol(out['K']):.3g}"


@pytest.mark.parametrize("epi", [False, True], ids=["plain", "bias_scale"])
@pytest.mark.parametrize("separate", [False, True], ids=["aliased", "separate"])
def test_gemm_stream_small_tiles(device, epi, separate):
    """(130, 256, 128): the direct epilogue of the 128 x 128 geometry (plan: "small"), ragged rows; C aliased to the residual as the prefill
    runs it, and a separate residual with a pitch of its own"""
    _assert_stream(_stream_gemm(device, 130, 256, 128, epi=epi, separate=separate, ldr=260 if separate else None, ldc=264), f"small tiles epi={epi} separate={separate}")


@pytest.mark.parametrize("geom", [1, 2], ids=["big", "k32"])
def test_gemm_stream_big_and_k32_tiles(device, tune, geom):
    """(300, 384, 192) through gemm_big = 1 / 2: the direct epilogue of the 256 x 256 x 64 and the 128 x 256 x 32 geometries on ragged edge tiles"""
    tune(gemm_big=geom)
    _assert_stream(_stream_gemm(device, 300, 384, 192, epi=True), f"gemm_big={geom}")


@pytest.mark.parametrize("ksplit", [0, 2], ids=["direct", "splitk"])
def test_gemm_stream_n_store_below_n_with_an_odd_pitch(device, ksplit):
    """N = 256, n_store = 250 = ldc: not a multiple of 4, so every residual read and every store is scalar, and columns 250 .. 255 of the tile
    have nowhere to go -- the row behind would take them"""
    out = _stream_gemm(device, 130, 256, 128, n_store=250, epi=True, ksplit=ksplit, ws_bytes=2 * 130 * 256 * 4 if ksplit else 0)
    _assert_stream(out, f"n_store=250 ksplit={ksplit}")


def test_gemm_stream_column_split(device):
    """(32768, 1152, 128), the shape of test_gemm_column_split_plan: columns 0 .. 1023 on the big geometry, the half-empty last tile column as a
    launch of its own -- the residual, C, bias and scale pointers of that part are offset by n1 (plan pinned in test_prefill_stage_ref.py).
    Reference in float64 on the device."""
    _assert_stream(_stream_gemm(device, 32768, 1152, 128, epi=True), "column split")


def test_gemm_stream_row_split(device):
    """The smallest problem whose plan splits the rows with 0 < m1 < all tile rows (found by scanning emmax_gemm_plan; pinned on the CPU):
    (257, 43776, 64) = one row of 256 x 256 tiles + one row in small tiles, whose residual and C pointers are offset by r0 x ld"""
    from test_prefill_stage_ref import ROW_SPLIT_SHAPE

    M, N, K = ROW_SPLIT_SHAPE
    _assert_stream(_stream_gemm(device, M, N, K), "row split")


@pytest.mark.parametrize("M,N,K,ks,sk_big,ldr", [(261, 1024, 4352, 8, 0, None), (300, 384, 640, 3, 0, None), (300, 384, 640, 3, 1, None), (300, 384, 640, 3, 0, 385),
                                                 (261, 1024, 4352, 8, 0, 1028)],
                         ids=["ks8", "ks3", "ks3-big", "ks3-scalar-residual", "ks8-separate-vector-residual"])
def test_gemm_stream_explicit_splitk(device, tune, M, N, K, ks, sk_big, ldr):
    """K slices + the reduce pass: the vector residual read (aliased, ld % 4 == 0), the scalar one (a separate residual of odd pitch), a slice
    count that does not divide the K steps, and the slices taken from 256 x 256 tiles"""
    tune(gemm_sk_big=sk_big)
    out = _stream_gemm(device, M, N, K, ksplit=ks, ws_bytes=ks * M * N * 4, separate=ldr is not None, ldr=ldr, epi=True)
    assert out["rc"] == 0
    _assert_stream(out, f"splitk ({M}, {N}, {K}) ks={ks} big={sk_big} ldr={ldr}")


def _assert_norm_out(y, stream_ref, norm_w, stream_atol, what):
    """norm_out against the float64 RMSNorm of the float64 stream: the norm's bound, plus what the stream's own fp32 error (stream_atol, absolute)
    moves the normalised value by -- rstd |w| per unit of x"""
    x = stream_ref.double()
    ref = R.ref_rmsnorm(x, norm_w.double())
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + R.NORM_EPS)
    allow = R.norm_bound() * (ref.abs() + 2.0 ** -12 * ref.pow(2).mean().sqrt()) + stream_atol * rstd * norm_w.double().abs()
    err = (y.double() - ref).abs()
    print(f"{what}: norm_out scaled error {R.scaled_err(y, ref):.4g} (bound {R.norm_bound():.4g})")
    assert torch.isfinite(y.float()).all() and (err <= allow).all(), f"{what}: norm_out misses the bound at {int((err > allow).sum())} elements; worst {(err / allow).max().item():.3g} x"


@pytest.mark.parametrize("ks", [2, 3])
@pytest.mark.parametrize("K", [128, 512])
@pytest.mark.parametrize("M", [1, 5, 7])
def test_gemm_stream_fused_norm(device, M, K, ks):
    """The reduce pass with the RMSNorm (four rows per block: M = 1, 5, 7 leave waves without a row): the stream against float64, norm_out against
    the float64 norm of the float64 stream, and both bit-identical to the unfused pair emmax_op_gemm_stream + emmax_op_rmsnorm_f32.
    K = 128 has two K steps: three slices are refused, and nothing is written."""
    L, lib = _lib()
    N = 4096
    norm_w = R.bf(1.0 + 0.1 * torch.randn(N, generator=R.gen(79, M, K))).to(device)
    fused = _stream_gemm(device, M, N, K, ksplit=ks, ws_bytes=ks * M * N * 4, epi=True, norm=(norm_w, N + 8))
    if ks > K // 64:
        assert fused["rc"] == -1 and b"ksplit" in lib.emmax_last_error()
        assert untouched(fused["norm_out"]) and same_bits(fused["C"], fused["res"])
        return
    assert fused["rc"] == 0, lib.emmax_last_error()
    _assert_stream(fused, f"fused norm M={M} K={K} ks={ks}")
    y = fused["norm_out"][:M, :N]
    unit = (fused["ref"] - fused["res"].double()).pow(2).mean().sqrt().item()
    _assert_norm_out(y, fused["ref"], norm_w, R.gemm_atol(K) * unit + R.GEMM_RTOL * 256.0, f"fused norm M={M} K={K} ks={ks}")
    # the unfused pair, bit for bit
    plain = _stream_gemm(device, M, N, K, ksplit=ks, ws_bytes=ks * M * N * 4, epi=True)
    assert plain["rc"] == 0 and same_bits(plain["C"], fused["C"]), "the stream differs between the fused and the unfused reduce pass"
    y2 = sent_bf16((M, N), device)
    Cc = plain["C"].contiguous()
    L.check(lib.emmax_op_rmsnorm_f32(Cc.data_ptr(), N, y2.data_ptr(), N, norm_w.data_ptr(), M, N, R.NORM_EPS, stream()), "rmsnorm_f32")
    torch.cuda.synchronize()
    assert same_bits(y2, y.contiguous()), "norm_out differs from emmax_op_rmsnorm_f32 of the same stream"


def test_gemm_stream_fused_norm_through_the_launch_plan(device):
    """ksplit = 0: the plan of (7, 4096, 2048) with scratch is "splitk ks=4 +norm" (pinned on the CPU) -- gemm_fuses_norm's own route"""
    N, K, M = 4096, 2048, 7
    norm_w = R.bf(1.0 + 0.1 * torch.randn(N, generator=R.gen(83))).to(device)
    out = _stream_gemm(device, M, N, K, ksplit=0, ws_bytes=8 << 20, norm=(norm_w, N))
    assert out["rc"] == 0
    _assert_stream(out, "fused norm, planned")
    unit = (out["ref"] - out["res"].double()).pow(2).mean().sqrt().item()
    _assert_norm_out(out["norm_out"][:M, :N], out["ref"], norm_w, R.gemm_atol(K) * unit + R.GEMM_RTOL * 256.0, "fused norm, planned")


def test_gemm_stream_refuses_what_it_cannot_do(device):
    """A norm the chosen path cannot fuse fails the call -- it is never skipped -- and so does a workspace that is too small; nothing is written"""
    L, lib = _lib()
    M, K = 5, 512
    for N, n_store, act, ks, ws_bytes, rc_want, word in ((256, 256, 0, 2, None, -1, b"does not fuse"), (4096, 4096, 1, 2, None, -1, b"does not fuse"),
                                                         (4096, 4000, 0, 2, None, -1, b"does not fuse"),    # the norm needs whole rows
                                                         (4096, 4096, 0, 0, None, -1, b"does not fuse"),    # K = 512: the plan is one launch of small tiles
                                                         (4096, 4096, 0, 0, 1024, -1, b"does not fuse"),    # ... and with too small a scratch for any split
                                                         (4096, 4096, 0, 4, 4 * M * 4096 * 4 - 4, -3, b"workspace"), (4096, 4096, 0, 2, 1024, -3, b"workspace")):
        A, W, _, _ = (t.to(device) for t in R.gemm_operands(M, N, K, 1))
        Cd, y = sent_f32((M, N), device), sent_bf16((M, N), device)
        w = torch.ones(N, dtype=torch.bfloat16, device=device)
        nbytes = 4 * M * N * 4 if ws_bytes is None else ws_bytes
        ws = torch.empty(4 * M * N, dtype=torch.float32, device=device)
        rc = lib.emmax_op_gemm_stream(A.data_ptr(), K, W.data_ptr(), K, Cd.data_ptr(), N, None, 0, M, N, K, None, act, None, n_store, ks, ws.data_ptr(), nbytes, w.data_ptr(),
                                      y.data_ptr(), N, R.NORM_EPS, stream())
        torch.cuda.synchronize()
        assert rc == rc_want and word in lib.emmax_last_error(), (N, n_store, act, ks, ws_bytes, rc, lib.emmax_last_error())
        assert untouched(Cd) and untouched(y)


# =============================================================================================================================================
# RMSNorm
# =============================================================================================================================================
@pytest.mark.parametrize("D", R.NORM_DIMS)
@pytest.mark.parametrize("rows", R.NORM_ROWS)
def test_rmsnorm_f32(device, rows, D):
    """fp32 rows with the stream's magnitudes and massive channels in, bf16 out, pitches above D on both sides; one D per MAXV instantiation"""
    L, lib = _lib()
    x, w = R.norm_inputs(rows, D)
    ldx, ldy = D + 4, D + 8
    xd = sent_f32((rows, ldx), device)
    xd[:, :D] = x.to(device)
    x0 = xd.clone()
    y = sent_bf16((rows + 1, ldy), device)
    wd = w.to(device)
    L.check(lib.emmax_op_rmsnorm_f32(xd.data_ptr(), ldx, y.data_ptr(), ldy, wd.data_ptr(), rows, D, R.NORM_EPS, stream()), "rmsnorm_f32")
    torch.cuda.synchronize()
    assert untouched(y[rows:]) and untouched(y[:rows, D:]) and same_bits(xd, x0)
    got, ref = y[:rows, :D].cpu(), R.ref_rmsnorm(x, w)
    e = R.scaled_err(got, ref)
    print(f"rmsnorm_f32 rows={rows} D={D}: scaled error {e:.4g} (bound {R.norm_bound():.4g})")
    assert torch.isfinite(got.float()).all() and e <= R.norm_bound()


# =============================================================================================================================================
# RoPE and the paged K / V append
# =============================================================================================================================================
def _rope_run(device, x, Hq, Hkv, hd, table, n_pages, cos, sin, *, misalign, caches):
    """one launch on a fresh copy of the rows; returns (qkv afterwards incl. padding and tail rows, kcache, vcache)"""
    L, lib = _lib()
    lens = R.SEQ_LENS
    total, B = sum(lens), len(lens)
    q_dim, kv_dim = Hq * hd, Hkv * hd
    ld = q_dim + 2 * kv_dim + 8
    qkv = sent_bf16((total + 2, ld), device)
    qkv[:total, : q_dim + 2 * kv_dim] = x.view(total, -1).to(device)
    cu, _, _ = R.packing(lens)
    cu_d, table_d = cu.to(device), table.to(device)

    def place(t):   # the table at a 16-byte aligned address, or one float into a larger tensor: 4-byte aligned only
        buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=device)
        v = buf[1:1 + t.numel()] if misalign else buf[:t.numel()]
        v.copy_(t.reshape(-1).to(device))
        assert (v.data_ptr() % 16 != 0) == misalign and v.data_ptr() % 4 == 0
        return v

    cd, sd = place(cos), place(sin)
    kc = sent_bf16((n_pages, Hkv, R.PAGE, hd), device) if caches else None
    vc = sent_bf16((n_pages, Hkv, R.PAGE, hd), device) if caches else None
    L.check(lib.emmax_op_rope_kv_write(qkv.data_ptr(), ld, 0, q_dim, q_dim + kv_dim, cu_d.data_ptr(), B, total, cd.data_ptr(), sd.data_ptr(), L.ptr(kc), L.ptr(vc),
                                       table_d.data_ptr(), table.shape[1], Hq, Hkv, hd, R.PAGE, stream()), "rope_kv_write")
    torch.cuda.synchronize()
    return qkv, kc, vc


@pytest.mark.parametrize("hd", R.ROPE_HEAD_DIMS)
@pytest.mark.parametrize("Hq,Hkv", R.ROPE_HEADS)
def test_rope_kv_write(device, Hq, Hkv, hd):
    """Page 64, lengths [63, 64, 65, 1, 130], a shuffled page table with pages in no row's table.  head_dim 128: the 16-byte kernel, and the
    element-wise one selected by 4-byte aligned tables -- bit-identical; head_dim 72: the element-wise kernel with every access aligned."""
    lens = R.SEQ_LENS
    total, B, max_pages = sum(lens), len(lens), 3
    n_pages = B * max_pages + 3
    q_dim, kv_dim = Hq * hd, Hkv * hd
    x = R.qkv_rows(total, Hq, Hkv, hd, 0)
    table = R.shuffled_table(B, max_pages, n_pages, (Hq, Hkv, hd))
    cos, sin = R.rope_tables32(max(lens), hd)       # as the session builds them: [pos][hd / 2] fp32
    _, _, pos = R.packing(lens)
    ref = R.ref_rope(x[:, : Hq + Hkv], cos[pos], sin[pos])
    runs = []
    for misalign in ((False, True) if hd % 16 == 0 else (False,)):
        qkv, kc, vc = _rope_run(device, x, Hq, Hkv, hd, table, n_pages, cos, sin, misalign=misalign, caches=True)
        rows = qkv[:total].cpu()
        assert untouched(qkv[total:]) and untouched(qkv[:total, q_dim + 2 * kv_dim:]), "rows past the last sequence / padding columns were written"
        got = rows[:, : q_dim + kv_dim].reshape(total, Hq + Hkv, hd)
        e = R.scaled_err(got, ref)
        print(f"rope Hq={Hq} Hkv={Hkv} hd={hd} misalign={misalign}: scaled error {e:.4g} (bound {R.rope_bound():.4g})")
        assert torch.isfinite(got.float()).all() and e <= R.rope_bound()
        v_in = x[:, Hq + Hkv:]
        assert same_bits(rows[:, q_dim + kv_dim: q_dim + 2 * kv_dim].reshape(total, Hkv, hd), v_in), "the V columns of qkv were touched"
        # the caches: the rotated K rows as they stand in qkv and the V rows as they came in, at (page, head, slot); everything else the sentinel
        want_k = R.paged_scatter(sent_bf16((n_pages, Hkv, R.PAGE, hd), "cpu"), got[:, Hq:], table, lens)
        want_v = R.paged_scatter(sent_bf16((n_pages, Hkv, R.PAGE, hd), "cpu"), v_in, table, lens)
        assert same_bits(kc.cpu(), want_k), "K cache: rows differ from the in-place rotated rows, or a slot past a length / a foreign page was written"
        assert same_bits(vc.cpu(), want_v), "V cache: rows differ from the input, or a slot past a length / a foreign page was written"
        runs.append((rows, kc.cpu(), vc.cpu()))
    if len(runs) == 2:
        assert all(same_bits(a, b) for a, b in zip(*runs)), "the 16-byte and the element-wise kernel differ"
    # the null-cache mode (fp8 KV cache): rotates in place, writes nothing else
    qkv0, _, _ = _rope_run(device, x, Hq, Hkv, hd, table, n_pages, cos, sin, misalign=False, caches=False)
    assert same_bits(qkv0.cpu()[:total], runs[0][0]) and untouched(qkv0[total:])


# =============================================================================================================================================
# the fp8 KV append
# =============================================================================================================================================
@pytest.mark.parametrize("Hkv", R.KVQ_HEADS)
def test_kv_quant_rows(device, Hkv):
    """bytes and scales at (page, head, slot) bit for bit, the rows written back into qkv = bf16(e4m3 x scale) exactly, the q columns untouched;
    rows of varied scales, an all-zero row, amax exactly 448 x 2^k and the next bf16 above"""
    L, lib = _lib()
    lens = R.SEQ_LENS
    total, B, max_pages = sum(lens), len(lens), 3
    n_pages = B * max_pages + 3
    q_dim, kv_dim = 128, Hkv * 128
    ld = q_dim + 2 * kv_dim + 8
    x, edge = R.kv_rows(total, Hkv, 0)
    q8, sc, deq = R.ref_kv_quant(x)
    table = R.shuffled_table(B, max_pages, n_pages, Hkv)
    qkv = sent_bf16((total + 2, ld), device)
    qkv[:total, q_dim: q_dim + 2 * kv_dim] = x.view(total, -1).to(device)
    cu, _, _ = R.packing(lens)
    cu_d, table_d = cu.to(device), table.to(device)
    k8 = torch.full((n_pages, Hkv, R.PAGE, 128), S8, dtype=torch.uint8, device=device)
    v8 = torch.full((n_pages, Hkv, R.PAGE, 128), S8, dtype=torch.uint8, device=device)
    ks, vs = sent_f32((n_pages, Hkv, R.PAGE), device), sent_f32((n_pages, Hkv, R.PAGE), device)
    L.check(lib.emmax_op_kv_quant_rows(qkv.data_ptr(), ld, q_dim, q_dim + kv_dim, cu_d.data_ptr(), B, total, k8.data_ptr(), v8.data_ptr(), ks.data_ptr(), vs.data_ptr(),
                                       table_d.data_ptr(), max_pages, Hkv, 128, R.PAGE, stream()), "kv_quant_rows")
    torch.cuda.synchronize()
    assert untouched(qkv[total:]) and untouched(qkv[:total, :q_dim]) and untouched(qkv[:total, q_dim + 2 * kv_dim:]), "q columns / padding / rows past the end were written"
    back = qkv[:total, q_dim: q_dim + 2 * kv_dim].cpu().view(total, 2 * Hkv, 128)
    bad = (R.bits16(back) != R.bits16(deq)).any(-1).view(-1).nonzero().flatten().tolist()
    assert not bad, f"rows written back differ from bf16(e4m3 x scale) at flat rows {bad[:8]} (edge rows: {edge})"
    for name, got8, gots, sl in (("K", k8, ks, slice(0, Hkv)), ("V", v8, vs, slice(Hkv, 2 * Hkv))):
        want8 = R.paged_scatter(torch.full((n_pages, Hkv, R.PAGE, 128), S8, dtype=torch.uint8), q8[:, sl], table, lens)
        wants = R.paged_scatter(sent_f32((n_pages, Hkv, R.PAGE, 1), "cpu"), sc[:, sl, None], table, lens).squeeze(-1)
        assert same_bits(got8.cpu(), want8), f"{name} bytes differ, or a slot past a length / a foreign page was written"
        assert same_bits(gots.cpu(), wants), f"{name} scales differ, or a slot past a length / a foreign page was written"
    # head_dim != 128 is refused before anything is launched
    assert lib.emmax_op_kv_quant_rows(qkv.data_ptr(), ld, q_dim, q_dim + kv_dim, cu_d.data_ptr(), B, total, k8.data_ptr(), v8.data_ptr(), ks.data_ptr(), vs.data_ptr(),
                                      table_d.data_ptr(), max_pages, Hkv, 64, R.PAGE, stream()) == -1 and b"head_dim" in lib.emmax_last_error()


# =============================================================================================================================================
# embed / splice and the last-row gather
# =============================================================================================================================================
@pytest.mark.parametrize("with32", [False, True], ids=["bf16", "bf16+fp32"])
@pytest.mark.parametrize("n_patches", [0, 5])
@pytest.mark.parametrize("hidden", [64, 4096])
def test_embed_splice(device, hidden, n_patches, with32):
    """ragged lengths with P_max above the longest, ids of -3 and vocab + 7 (clamped), text only and with patches; the fp32 copy is the exact
    widening of the bf16 row.  hidden 4096 = 512 chunks: the chunk loop runs twice."""
    L, lib = _lib()
    g = R.gen(89, hidden, n_patches)
    V, lens, P_max = 50, [3, 1, 7, 4], 9
    B = len(lens)
    E = R.bf(torch.randn(V, hidden, generator=g))
    patches = R.bf(torch.randn(B, max(n_patches, 1), hidden, generator=g))
    ids = torch.randint(0, V, (B, P_max), generator=g, dtype=torch.int32)
    ids[0, 1], ids[2, 0], ids[2, 5], ids[3, 3] = -3, V + 7, -3, V + 7
    for b, n in enumerate(lens):
        ids[b, n:] = 12345678     # past a row's length: never read
    S = [n_patches + n for n in lens]
    cu = torch.tensor([0] + torch.tensor(S).cumsum(0).tolist(), dtype=torch.int32)
    total = int(cu[-1])
    want = R.ref_embed_splice(ids, lens, E, patches, n_patches)
    h = sent_bf16((total + 2, hidden), device)
    h32 = sent_f32((total + 2, hidden), device) if with32 else None
    Ed, pd, idd, cud = E.to(device), patches.to(device), ids.to(device), cu.to(device)
    L.check(lib.emmax_op_embed_splice(idd.data_ptr(), P_max, cud.data_ptr(), Ed.data_ptr(), pd.data_ptr() if n_patches else None, h.data_ptr(), L.ptr(h32), B, max(S) + 1,
                                      n_patches, hidden, V, stream()), "embed_splice")
    torch.cuda.synchronize()
    assert same_bits(h[:total].cpu(), want) and untouched(h[total:])
    if with32:
        assert same_bits(h32[:total].cpu(), want.float()) and untouched(h32[total:])


@pytest.mark.parametrize("form", ["bf16", "bf16+fp32", "from_fp32", "from_fp32+fp32"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D", [64, 4096])
def test_gather_last_rows(device, D, B, form):
    """the three forms of the kernel (bf16 copy, bf16 copy + widening, fp32 source rounded to nearest even with and without the fp32 copy);
    the fp32 source holds values exactly on bf16 ties and in the denormal range.  D = 4096 = 512 chunks: the chunk loop runs twice."""
    L, lib = _lib()
    lens = R.SEQ_LENS[:B]
    cu, _, _ = R.packing(lens)
    total = sum(lens)
    last = (cu[1:] - 1).long()
    from32, out32 = form.startswith("from_fp32"), form.endswith("+fp32")
    src32 = R.gather_source32(total, D, B)
    src = R.bf(torch.randn(total, D, generator=R.gen(97, D, B)))
    sd = (src32 if from32 else src).to(device)
    out = sent_bf16((B + 1, D), device)
    o32 = sent_f32((B + 1, D), device) if out32 else None
    cud = cu.to(device)
    L.check(lib.emmax_op_gather_last_rows(None if from32 else sd.data_ptr(), sd.data_ptr() if from32 else None, out.data_ptr(), L.ptr(o32), cud.data_ptr(), B, D, stream()),
            "gather_last_rows")
    torch.cuda.synchronize()
    assert untouched(out[B:]) and (o32 is None or untouched(o32[B:]))
    if from32:
        assert torch.equal(R.bits16(out[:B].cpu()), R.bf16_bits_rne(src32[last])), "fp32 -> bf16 is not round to nearest even"
        if out32:
            assert same_bits(o32[:B].cpu(), src32[last])
    else:
        assert same_bits(out[:B].cpu(), src[last])
        if out32:
            assert same_bits(o32[:B].cpu(), src[last].float())
