"""CPU: the bounds of tests/test_prefill_stages_gpu.py are what the fp32 emulation of the documented roundings measures against the float64
reference (prefill_stage_ref.py) -- not numbers taken from a kernel's output, and not stale or padded ones; the references are the oracle's
operations; the launch plans the GPU cases rely on are the ones the library makes; the fp8 scale rule has one answer at its boundary."""

import ctypes as C
import os

import pytest
import torch

import prefill_stage_ref as R


def _pinned(measured, entry, what):
    # a measurement sits under its entry (5 % for another BLAS's or libm's last bit) and the table is not padded: at least 2 / 3 of the entry
    assert measured <= 1.05 * entry, (what, measured, entry)
    assert measured >= 0.66 * entry, (what, measured, entry)


@pytest.mark.parametrize("K", sorted(R.GEMM_SPREAD))
def test_gemm_stream_bound_is_the_emulations_and_a_bf16_residual_fails_it(K):
    spread, spread_bf16_residual = R.measure_gemm(K)
    _pinned(spread, R.GEMM_SPREAD[K], f"gemm K={K}")
    # the property the bound exists for: one trip of the residual through bf16 misses it by orders of magnitude
    assert spread_bf16_residual > 1e4 * R.gemm_atol(K), (K, spread_bf16_residual, R.gemm_atol(K))
    assert R.GEMM_RTOL == 2.0 ** -24 and R.GEMM_ORDER == 2.0
    assert ROW_SPLIT_SHAPE == R.GEMM_CASE[64][:2] + (64,)   # the K = 64 entry is measured on the row-split case's own inputs


def test_rmsnorm_f32_bound_is_the_emulations():
    m = R.measure_norm()
    _pinned(m, R.NORM_REL, "rmsnorm_f32")
    assert m <= R.NORM_SUP and R.norm_bound() <= R.NORM_SUP   # two roundings of half a bf16 ulp each


def test_rope_bound_is_the_emulations():
    m = R.measure_rope()
    _pinned(m, R.ROPE_REL, "rope")
    assert m <= R.ROPE_SUP and R.rope_bound() <= R.ROPE_SUP   # one rounding


# ---- the references are the oracle's operations (compared in float64, within fp32 epsilon) ----------------------------------------------------
EPS32 = 2.0 ** -23


def test_rope_reference_is_the_oracles_rotation():
    from oracle import emmax_oracle as orc

    _, _, pos = R.packing(R.SEQ_LENS)
    for hd in R.ROPE_HEAD_DIMS:
        x = R.qkv_rows(len(pos), 4, 2, hd, 1)[:, :6].double()
        cos, sin = orc.rope_cos_sin(pos, hd, R.THETA, torch.float32)   # [rows][hd], the two halves equal
        want = x * cos.double()[:, None, :] + orc._rotate_half(x) * sin.double()[:, None, :]
        # the reference on the oracle's table values
        got = R.ref_rope(x, cos[:, : hd // 2], sin[:, : hd // 2])
        assert (got - want).abs().max().item() <= EPS32 * want.abs().max().item()
        # the tables the tests hand to the kernel are the oracle's (the session's construction: fp32 inv_freq, fp32 angle)
        c32, s32 = R.rope_tables32(max(R.SEQ_LENS), hd)
        assert (c32[pos].double() - cos[:, : hd // 2].double()).abs().max().item() <= 4 * EPS32 * max(R.SEQ_LENS)   # (|d cos| <= |d angle|: positions up to 129)
        assert (s32[pos].double() - sin[:, : hd // 2].double()).abs().max().item() <= 4 * EPS32 * max(R.SEQ_LENS)


def test_rmsnorm_reference_is_the_oracles_on_fp32_input():
    from oracle import emmax_oracle as orc

    for rows, D in ((5, 64), (5, 520), (3, 4096)):
        x, w = R.norm_inputs(rows, D)
        want = orc.rms_norm(x, w.float(), R.NORM_EPS).double()   # fp32 in: no downcast anywhere
        got = R.ref_rmsnorm(x, w)
        assert ((got - want).abs() <= 8 * EPS32 * want.abs() + 1e-30).all()


def test_splice_reference_is_the_oracles():
    from oracle import emmax_oracle as orc

    g = R.gen(71)
    V, H, B, P, n_patches = 50, 64, 3, 6, 5
    E = R.bf(torch.randn(V, H, generator=g))
    patches = R.bf(torch.randn(B, n_patches, H, generator=g))
    ids = torch.randint(0, V, (B, P), generator=g, dtype=torch.int32)
    want = orc.splice(ids, patches.float(), {"language_model.model.embed_tokens.weight": E.float()})   # [B][1 + n_patches + P - 1][H]
    got = R.ref_embed_splice(ids, [P] * B, E, patches, n_patches).float().view(B, n_patches + P, H)
    assert torch.equal(got, want)
    # ragged rows are prefixes of the same thing; out-of-range ids clamp to the table
    lens = [2, 6, 1]
    rag = R.ref_embed_splice(ids, lens, E, patches, n_patches).float()
    o = 0
    for b, n in enumerate(lens):
        assert torch.equal(rag[o:o + n_patches + n], want[b, : n_patches + n])
        o += n_patches + n
    bad = ids.clone()
    bad[0, 1], bad[1, 0] = -3, V + 7
    fix = ids.clone()
    fix[0, 1], fix[1, 0] = 0, V - 1
    assert torch.equal(R.ref_embed_splice(bad, [P] * B, E, patches, 0), R.ref_embed_splice(fix, [P] * B, E, patches, 0))


# ---- exact references ---------------------------------------------------------------------------------------------------------------------------
def test_bf16_rounding_on_the_bits_is_round_to_nearest_even():
    x = R.gather_source32(7, 4096, 0)
    assert torch.isfinite(x).all()
    u = x.view(torch.int32)
    assert ((u & 0xFFFF) == 0x8000).sum() > 1000 and (((u >> 23) & 0xFF) == 0).sum() > 1000   # ties and denormals are really in there
    assert torch.equal(R.bf16_bits_rne(x), R.bits16(x.to(torch.bfloat16)))
    # ties go to the even neighbour, both ways
    t = torch.tensor([0x3F808000, 0x3F818000, 0x00008000, 0x00018000], dtype=torch.int32).view(torch.float32)
    assert R.bf16_bits_rne(t).tolist() == [0x3F80, 0x3F82, 0x0000, 0x0002]


def test_fp8_scale_rule_is_exact_at_its_boundary():
    """fl32(448 x 2^k) x fl32(1 / 448) is exactly 2^k for k in -20 .. 19: the kernel's arithmetic (common.h: e4m3_row_scale multiplies by the
    rounded reciprocal and bumps the exponent when any mantissa bit is left) gives scale 2^k at amax = 448 x 2^k, as the rule says -- and the
    next power of two for the next bf16 above."""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(448.0, dtype=torch.float32)
    for k in range(-20, 20):
        top = torch.tensor(448.0 * 2.0 ** k, dtype=torch.float32)
        assert (top * inv).item() == 2.0 ** k, k
        nxt = torch.tensor(450.0 * 2.0 ** k, dtype=torch.float32)   # 448 = 1.75 x 2^8: one unit of the 7-bit mantissa field is 2
        assert nxt.to(torch.bfloat16).float().item() == nxt.item()           # representable: the next bf16 up
        r = (nxt * inv).item()
        assert 2.0 ** k < r < 2.0 ** (k + 1)
        assert R.e4m3_scale(top).item() == 2.0 ** k and R.e4m3_scale(nxt).item() == 2.0 ** (k + 1)
    assert R.e4m3_scale(torch.tensor(0.0)).item() == 1.0
    # the rule, against its definition in exact arithmetic on arbitrary bf16 maxima
    a = R.bf(torch.rand(4096, generator=R.gen(73)) * 1000.0 + 1e-3).double()
    s = R.e4m3_scale(a).double()
    assert (a / s <= 448.0).all() and (a / (s / 2) > 448.0).all()


def test_fp8_reference_rows_and_edges():
    x, edge = R.kv_rows(40, 9, 0)
    q8, sc, deq = R.ref_kv_quant(x)
    flat_sc, flat_q = sc.view(-1), q8.view(-1, 128)
    assert flat_sc[edge["zero"]].item() == 1.0 and int(flat_q[edge["zero"]].max()) == 0
    for k in (-3, 0, 4):
        assert flat_sc[edge[("top", k)]].item() == 2.0 ** k and flat_sc[edge[("next", k)]].item() == 2.0 ** (k + 1)
        assert int((flat_q[edge[("top", k)]] & 0x7F).max()) == 0x7E            # 448, the largest finite e4m3
    assert len(set(flat_sc.tolist())) >= 8                                       # varied scales
    assert torch.equal(deq.float(), (q8.view(torch.float8_e4m3fn).float() * sc[..., None]))   # e4m3 x power of two is exact in bf16


# ---- the launch plans the GPU cases rely on (host only) ------------------------------------------------------------------------------------------
ROW_SPLIT_SHAPE = (257, 43776, 64)


@pytest.fixture(scope="module")
def lib():
    from emmax import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib, _lib.load()


def test_stream_gemm_plans_of_the_gpu_cases(lib):
    L, so = lib
    plan = lambda M, N, K, **kw: L.gemm_plan(M, N, K, out_f32=True, residual=2, **kw)
    assert plan(130, 256, 128) == "small"
    assert plan(32768, 1152, 128) == "cols 0..1024: big | cols 1024..1152: small"
    # the row split with 0 < m1 < all tile rows: one big tile row and one row of small tiles
    M, N, K = ROW_SPLIT_SHAPE
    assert plan(M, N, K, ws_bytes=0) == plan(M, N, K) == "big rows 0..256 + small rows 256..257"
    # ... and no smaller problem (by M x N) has one -- the scan that picked the shape: every M from 1 up to where even N = 128 is no
    # smaller, every N (a multiple of 128) below M x N of the shape.  (Up to 256 rows there is one tile row: nothing to split.)
    def split(m, n):
        t = plan(m, n, K)
        return t.startswith("big rows 0..") and "+ small rows" in t
    assert [(m, n) for m in range(1, M * N // 128 + 1) for n in range(128, (M * N - 1) // m + 1, 128) if split(m, n)] == []
    # the fused norm through the launch plan, and where the plan cannot fuse it
    assert plan(7, 4096, 2048, norm=True) == "splitk ks=4 +norm"
    assert plan(7, 4096, 512, norm=True) == "small"
    with L.tuning(gemm_big=1):
        assert plan(300, 384, 192) == "forced big"
    with L.tuning(gemm_big=2):
        assert plan(300, 384, 192) == "forced k32"


def test_argument_checks_need_no_device(lib):
    """Only the refusals that the entry points' own argument checks make (ops.hip), each a return in front of the planner and of every launcher:
    nothing here can reach a launch, so made-up aligned addresses do.  What a planner or a launcher refuses -- a norm the path cannot fuse,
    a plan without scratch -- is tested on real buffers in test_prefill_stages_gpu.py."""
    L, so = lib
    p = 1 << 20
    call = lambda **kw: so.emmax_op_gemm_stream(p, kw.get("K", 128), p, kw.get("K", 128), p, kw.get("N", 4096), None, 0, 4, kw.get("N", 4096), kw.get("K", 128), None,
                                                kw.get("act", 0), None, kw.get("n_store", kw.get("N", 4096)), kw.get("ksplit", 2), kw.get("ws", p), kw.get("ws_bytes", 1 << 30),
                                                kw.get("norm_w", p), kw.get("norm_out", p), kw.get("N", 4096), 1e-5, None)
    assert call(ws_bytes=2 * 4 * 4096 * 4 - 1) == -3 and b"workspace" in so.emmax_last_error()
    assert call(ksplit=3) == -1 and b"ksplit" in so.emmax_last_error()                                # K = 128: two K steps
    assert call(norm_w=None) == -1 and b"go together" in so.emmax_last_error()
    assert call(act=2) == -1 and b"act" in so.emmax_last_error()
    assert call(N=100) == -1 and call(K=100) == -1
    assert call(n_store=4097) == -1 and b"n_store" in so.emmax_last_error()
    assert so.emmax_op_kv_quant_rows(p, 512, 128, 256, p, 1, 1, p, p, p, p, p, 1, 1, 72, 64, None) == -1 and b"head_dim" in so.emmax_last_error()
    assert so.emmax_op_rope_kv_write(p, 512, 0, 128, 256, p, 1, 1, p, p, p, None, p, 1, 1, 1, 128, 64, None) == -1 and b"go together" in so.emmax_last_error()
    assert so.emmax_op_rmsnorm_f32(p, 60, p, 64, p, 1, 64, 1e-5, None) == -1 and b"ldx" in so.emmax_last_error()
    assert so.emmax_op_embed_splice(p, 4, p, p, None, p, None, 1, 4, 5, 64, 10, None) == -1 and b"n_patches" in so.emmax_last_error()
    assert so.emmax_op_gather_last_rows(None, None, p, None, p, 1, 64, None) == -1 and b"null argument" in so.emmax_last_error()
