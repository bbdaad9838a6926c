"""MXFP4 decode weights (decode_weight_dtype = "mxfp4", emmax_config.decode_fp8 = 2) on the GPU.

  * the quantiser: emmax_op_quant_mxfp4 then emmax_op_dequant_mxfp4, bit-equal to the torch reference of tests/mxfp4_ref.py on random and
    hand-written blocks, in the natural row order and both of decode_km.hip's permutations;
  * every fused decode stage of an MXFP4 model through the step's own dispatch (emmax_op_decode_stage), against the float64 reference on the
    DE-QUANTISED weights with the checks of tests/test_decode_stages_gpu.py, the launcher family asserted (decode_km.hip at every batch 1-16);
  * the refusals (shapes, 17 rows, exact numerics), none of which launches anything;
  * end to end on the G4 shape with the tiny towers: planted ids, teacher-forced random-weight logits and ids (eager and hipGraph replay,
    bit-equal), and the prefill's logits -- prefill and decode evaluate the same quantised model, so "the oracle on the de-quantised weights" is the
    reference for every token.  Without the write-back of the de-quantised values into the prefill's rows the prefill checks miss by 3.3e-1 - 3.8e-1
    (profiles/mxfp4_quant_error.txt).
"""

import contextlib
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import decode_stage_ref as R
import mxfp4_ref as M
from conftest import ID_BUDGET_SHALLOW, above_id_line
from test_ops_gpu import assert_elementwise, relerr

pytestmark = pytest.mark.gpu

QKV, OPROJ, GATEUP, DOWN, LMHEAD = 0, 2, 3, 4, 5
KM = 4                                   # EMMAX_VIA_KM
VIA_NAME = {0: "none", 1: "ks", 2: "gemv", 3: "gemv_fp8", 4: "km", 5: "kmp", 6: "mfma"}
E2E_TOL = 3e-2                           # the 2-layer line of tests/test_operating_point_gpu.py / test_e2e_gpu.py


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def check(got, ref, out, what):
    rtol, atol, tol = M.tolerances4(out)
    err = relerr(got, ref)
    print(f"{what}: relerr {err:.3e} (bound {tol:.3e}), atol_frac {atol:.3e}")
    assert err < tol, f"{what}: relerr {err:.3e} >= {tol:.3e}"
    assert_elementwise(got, ref, rtol=rtol, atol_frac=atol, what=what)


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------------
def _quant_roundtrip(device, W, perm, hd):
    from emmax import _lib

    lib = _lib.load()
    N, K = W.shape
    src = W.to(device).contiguous()
    tiles = torch.empty(N * K // 2, dtype=torch.uint8, device=device)
    scales = torch.empty(N * K // 32, dtype=torch.uint8, device=device)
    dst = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device=device)
    st = _lib.current_stream()
    _lib.check(lib.emmax_op_quant_mxfp4(src.data_ptr(), K, tiles.data_ptr(), scales.data_ptr(), N, K, perm, hd, st), "emmax_op_quant_mxfp4")
    _lib.check(lib.emmax_op_dequant_mxfp4(tiles.data_ptr(), scales.data_ptr(), dst.data_ptr(), K, N, K, perm, hd, st), "emmax_op_dequant_mxfp4")
    torch.cuda.synchronize()
    return dst.cpu(), tiles.cpu(), scales.cpu()


@pytest.mark.parametrize("perm,hd", [(0, 0), (1, 32), (2, 0)], ids=["natural", "qkv-perm", "gateup-perm"])
def test_quant_dequant_is_bit_equal_to_the_torch_reference(device, perm, hd):
    """32 x 1024: random rows of very different scale with every hand-written block planted (ties, power-of-two amax, saturation at 7 2^k, the
    all-zero block, the clamped exponent with bf16 denormals, negatives).  The permutations only move rows between tiles: the values come back at
    the rows they were taken from."""
    W, want = M.adversarial_matrix()
    got, tiles, scales = _quant_roundtrip(device, W, perm, hd)
    want_bf = want.to(torch.bfloat16)
    assert torch.equal(want_bf.double(), want)
    bad = (bits(got) != bits(want_bf)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()}, want {want_bf[tuple(bad[0])].item()}"
    # a second pass over the de-quantised values changes nothing: what finalize writes back is a fixed point of the quantiser
    again, tiles2, scales2 = _quant_roundtrip(device, got, perm, hd)
    assert torch.equal(bits(again), bits(got))
    # the scale codes of the planted blocks, read back through the documented layout: natural order, tile (nt, kt) at nt * K / 128 + kt
    if perm == 0:
        _, e = M.quantize(W)
        codes = scales.view(32 // 16, 1024 // 128, 16, 4)            # [row tile][k tile][row][block of the tile]
        for r in range(32):
            for blk in range(1024 // 32):
                amax = W[r, blk * 32:(blk + 1) * 32].float().abs().max().item()
                want_code = 127 if amax == 0 else int(e[r, blk]) + 127
                assert int(codes[r // 16, blk // 4, r % 16, blk % 4]) == want_code, (r, blk)


def test_quantiser_refuses_shapes_outside_the_tiles(device):
    from emmax import _lib

    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    for N, K, ld, perm, hd in ((24, 128, 128, 0, 0), (32, 192, 192, 0, 0), (32, 128, 64, 0, 0), (32, 128, 128, 1, 24), (48, 128, 128, 2, 0), (32, 128, 128, 3, 0)):
        assert lib.emmax_op_quant_mxfp4(buf.data_ptr(), ld, buf.data_ptr(), buf.data_ptr(), N, K, perm, hd, _lib.current_stream()) == -1
        assert lib.emmax_op_dequant_mxfp4(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ld, N, K, perm, hd, _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert int(buf.max()) == 0


@pytest.mark.parametrize("rows", [8, 16], ids=["NB8", "NB16"])
def test_hardware_widening_on_every_scale_code_and_the_hand_written_blocks(device, rows):
    """What v_cvt_scalef32_pk_bf16_fp4 makes of the tiles, element by element, through the decode kernel itself (emmax_op_gemm_small_mxfp4: the
    K-split kernel's plain form, 8 and 16 staged rows).  Row r of a 32 x 1024 matrix holds ONE non-zero block -- the hand-written blocks, a block
    at scale code 0 (2^-127: the scale operand's exponent field is zero) and one at code 252 (the largest a bf16 weight reaches) -- and batch row b
    is one-hot at element b of every block, scaled by a power of two per block so that products and outputs are normal numbers: y[b, r] is then
    exactly x times ONE de-quantised element (zeros add nothing), and the expectation is the torch reference's value, a priori.
    Elements whose de-quantised value is a bf16 DENORMAL (below 2^-126: only in the code-0 and clamped blocks) reach the MFMA as denormal
    operands, which the matrix pipe is allowed to flush: for those, and only those, 0 is accepted beside the exact value (the prefill GEMM reads
    the same denormals through the same pipe)."""
    from emmax import _lib

    lib = _lib.load()
    N, K = 32, 1024
    t = 2.0 ** -127
    blocks = [(n, b.double(), 1.0) for n, b, _ in M.adversarial_blocks()]
    code0 = torch.zeros(32, dtype=torch.float64)
    code0[:8] = torch.tensor([6 * t, -4 * t, 3 * t, 2 * t, 1.5 * t, -1 * t, 0.5 * t, 5 * t])      # amax 1.5 2^-125: e = -127 without clamping
    top = torch.zeros(32, dtype=torch.float64)
    top[:6] = torch.tensor([1.5 * 2.0 ** 127, -(2.0 ** 127), 2.0 ** 126, 3 * 2.0 ** 125, -(2.0 ** 124), 2.0 ** 120])   # e = 125, code 252
    blocks += [("code-0", code0, 1.0), ("code-252", top, 1.0)]
    W = torch.zeros(N, K, dtype=torch.float64)
    sx = torch.ones(K // 32, dtype=torch.float64)
    for r, (name, blk, _) in enumerate(blocks):
        amax = blk.abs().max().item()
        W[r, r * 32:(r + 1) * 32] = blk
        sx[r] = 2.0 ** 64 if 0 < amax < 2.0 ** -100 else 2.0 ** -64 if amax > 2.0 ** 100 else 1.0
    Wb = W.to(torch.bfloat16)
    assert torch.equal(Wb.double(), W)
    _, e = M.quantize(Wb)
    assert int(e[len(blocks) - 2, len(blocks) - 2]) == -127 and int(e[len(blocks) - 1, len(blocks) - 1]) == 125
    want_w = M.quant_dequant(Wb)
    src = Wb.to(device)
    tiles = torch.empty(N * K // 2, dtype=torch.uint8, device=device)
    scales = torch.empty(N * K // 32, dtype=torch.uint8, device=device)
    st = _lib.current_stream()
    _lib.check(lib.emmax_op_quant_mxfp4(src.data_ptr(), K, tiles.data_ptr(), scales.data_ptr(), N, K, 0, 0, st), "emmax_op_quant_mxfp4")
    flushed = 0
    for off in range(0, 32, rows):
        x = torch.zeros(rows, K, dtype=torch.float64)
        for b in range(rows):
            x[b, off + b::32] = sx
        xb = x.to(torch.bfloat16)
        assert torch.equal(xb.double(), x)
        y = torch.full((rows, N), float("nan"), dtype=torch.bfloat16, device=device)
        xd = xb.to(device)
        _lib.check(lib.emmax_op_gemm_small_mxfp4(xd.data_ptr(), tiles.data_ptr(), scales.data_ptr(), y.data_ptr(), rows, N, K, st), "emmax_op_gemm_small_mxfp4")
        torch.cuda.synchronize()
        got = y.cpu()
        for r, (name, _, _) in enumerate(blocks):
            for b in range(rows):
                w = want_w[r, r * 32 + off + b].item()
                want = torch.tensor(w * sx[r].item(), dtype=torch.float64).to(torch.bfloat16)
                assert float(want) == w * sx[r].item()                                   # the expectation is exact in bf16
                g = got[b, r]
                ok = bits(g.reshape(1)).item() == bits(want.reshape(1)).item() or (float(g) == 0.0 and float(want) == 0.0)
                if not ok and 0 < abs(w) < 2.0 ** -126 and float(g) == 0.0:
                    flushed += 1
                    ok = True
                assert ok, f"block {name}, element {off + b}: got {float(g)!r}, de-quantised weight {w!r} x {sx[r].item()!r} = {float(want)!r}"
        assert (got[:, len(blocks):] == 0).all(), "rows without a block gave non-zero outputs"
    print(f"bf16-denormal weight elements that reached the output as 0: {flushed}")


# ---- engines ----------------------------------------------------------------------------------------------------------------------------
class Eng4:
    """one MXFP4 model + session and the float64 de-quantised weights its references read"""

    def __init__(self, device, model, max_batch, kv_fp8=False, sd=None):
        from emmax import _lib
        from emmax.engine import EmmaxEngine

        self.L, self.lib = _lib, _lib.load()
        self.model, self.kv_fp8 = model, kv_fp8
        self.cfg = M.make_cfg4(model)
        self.sd = sd if sd is not None else M.make_state_dict4(model)
        self.W = M.Weights4(self.sd, self.cfg)
        with (_lib.tuning(kv_fp8=1) if kv_fp8 else contextlib.nullcontext()):
            self.eng = EmmaxEngine(self.cfg, dict(self.sd), device=device, max_batch=max_batch, max_prompt=R.MAX_PROMPT, max_ctx=R.MAX_CTX)
        self.eng.ensure_decode_batch(max_batch)
        assert int(self.lib.emmax_model_aux_bytes(self.eng._model)) == 0
        self.device, self.rows = device, max_batch
        self.Hq, self.Hkv = M.MODELS4[model]
        self.hidden, self.q_dim = M.HIDDEN4, self.Hq * R.HEAD_DIM
        self.max_pages = (R.MAX_CTX + R.PAGE - 1) // R.PAGE
        self.eng.kv.random_(0, 256)
        torch.cuda.synchronize()

    def hidden_rows(self, seed, scale=1.0):
        return M.hidden_rows4(self.rows, seed, scale)

    def oproj_form(self, B):
        form, ns, via = C.c_int(-1), C.c_int(0), C.c_int(0)
        self.L.check(self.lib.emmax_op_decode_stage(self.eng._session, 0, OPROJ, B, None, None, None, None, None, None, None, None, None, C.byref(via),
                                                    C.byref(form), C.byref(ns), self.L.current_stream()), "oproj form")
        return form.value, ns.value

    def run(self, stage, B, layer=0, h32=None, h=None, ctx=None, pages=None, x=None):
        dev = self.device
        h32_d = h32.to(dev).contiguous()
        h_d = (h if h is not None else R.bf(h32)).to(dev).contiguous()
        assert h_d.shape == (self.rows, self.hidden) and h32_d.shape == (self.rows, self.hidden)
        h_out, h32_out = torch.empty_like(h_d), torch.empty_like(h32_d)
        y = tok = None
        if stage == QKV:
            y = torch.full((B, self.q_dim), float("nan"), dtype=torch.bfloat16, device=dev)
        elif stage == GATEUP:
            y = torch.full((B, M.INTER4), float("nan"), dtype=torch.bfloat16, device=dev)
        elif stage == LMHEAD:
            y = torch.full((B, R.VOCAB), float("nan"), dtype=torch.float32, device=dev)
            tok = torch.full((B,), -7, dtype=torch.int32, device=dev)
        x_d = x.to(dev).contiguous() if x is not None else None
        ctx_c = (C.c_int32 * B)(*ctx) if ctx is not None else None
        pt_c = None
        if pages is not None:
            flat = pages.reshape(-1).tolist()
            pt_c = (C.c_int32 * len(flat))(*flat)
        via = C.c_int(0)
        rc = self.lib.emmax_op_decode_stage(self.eng._session, layer, stage, B, h_d.data_ptr(), h32_d.data_ptr(), ctx_c, pt_c, self.L.ptr(x_d),
                                            h_out.data_ptr(), h32_out.data_ptr(), self.L.ptr(y), self.L.ptr(tok), C.byref(via), None, None,
                                            self.L.current_stream())
        self.L.check(rc, f"emmax_op_decode_stage(stage {stage}, B {B})")
        torch.cuda.synchronize()
        assert via.value == KM, f"stage {stage} at B {B} ran on {VIA_NAME.get(via.value, via.value)}, expected km"
        return {"h": h_out.cpu(), "h32": h32_out.cpu(), "y": None if y is None else y.cpu(), "tok": None if tok is None else tok.cpu()}

    def kv_read(self, layer, row, p0, n, page_row=None, from_stage=False):
        nn = 1 if from_stage else n
        k = np.empty((nn, self.Hkv, R.HEAD_DIM), dtype=np.float32)
        v = np.empty_like(k)
        pr = (C.c_int32 * self.max_pages)(*page_row.tolist()) if page_row is not None else None
        self.L.check(self.lib.emmax_op_decode_kv_read(self.eng._session, layer, row, p0, n, pr, int(from_stage), k.ctypes.data_as(C.POINTER(C.c_float)),
                                                      v.ctypes.data_as(C.POINTER(C.c_float)), self.L.current_stream()), "emmax_op_decode_kv_read")
        return k, v

    def kv_token_rows(self, raw):
        """[layers][K / V][pages][kv heads][64 tokens][bytes of a token row] of the raw bf16 paged region"""
        n_pages = self.rows * self.max_pages
        return raw.view(R.LAYERS, 2, n_pages, self.Hkv, R.PAGE, R.HEAD_DIM * 2)


@pytest.fixture(scope="module")
def engines(device):
    made = {}
    spec = {"G4": dict(model="G4", max_batch=8), "W4": dict(model="W4", max_batch=16), "G4kv8": dict(model="G4", max_batch=8, kv_fp8=True)}

    def get(name):
        if name not in made:
            made[name] = Eng4(device, **spec[name])
        return made[name]

    yield get
    for e in made.values():
        e.eng.close()


CASES = [pytest.param(m, B, id=f"{m}-B{B}") for m in ("G4", "W4") for B in M.BATCHES4[m]]


# ---- QKV --------------------------------------------------------------------------------------------------------------------------------
def _qkv_once(e, B, li, pages, kv8=False):
    h32, h = e.hidden_rows((B, li))
    x = h32[:B]
    ctx = R.ctx_rows(B, li)
    pt = pages if pages is not None else torch.arange(B * e.max_pages, dtype=torch.int32).view(B, e.max_pages)
    e.eng.kv.random_(0, 256)
    win = []
    for b in range(B):
        p0 = max(ctx[b] - 1, 0)
        win.append((p0, e.kv_read(li, b, p0, ctx[b] + 2 - p0, pt[b])))
    before = e.eng.kv.clone()
    out = e.run(QKV, B, li, h32=h32, h=h, ctx=ctx, pages=pages)
    q_ref, k_ref, v_ref = R.ref_qkv(e.W, li, x, ctx)
    check(out["y"], q_ref, "q", f"q rows (layer {li})")
    assert torch.equal(bits(out["h"]), bits(h)) and torch.equal(bits(out["h32"]), bits(h32)), "qkv changed the hidden rows"
    k_new, v_new = [], []
    for b in range(B):
        if kv8:
            k, v = e.kv_read(li, b, 0, 1, from_stage=True)
            k_new.append(k[0]); v_new.append(v[0])
            continue
        p0, (k0, v0) = win[b]
        k1, v1 = e.kv_read(li, b, p0, ctx[b] + 2 - p0, pt[b])
        at = ctx[b] - p0
        k_new.append(k1[at]); v_new.append(v1[at])
        for j in range(k1.shape[0]):
            if j != at:
                assert np.array_equal(k0[j].view(np.int32), k1[j].view(np.int32)) and np.array_equal(v0[j].view(np.int32), v1[j].view(np.int32)), \
                    f"row {b}: position {p0 + j} changed by the append at {ctx[b]}"
    check(torch.from_numpy(np.stack(k_new)), k_ref, "k", f"K rows (layer {li})")
    check(torch.from_numpy(np.stack(v_new)), v_ref, "v", f"V rows (layer {li})")
    after = e.eng.kv
    if kv8:
        assert torch.equal(before, after), "fp8 KV cache: the qkv launch wrote into the cache"
        return
    changed = (e.kv_token_rows(before) != e.kv_token_rows(after)).any(-1).cpu()
    want = torch.zeros_like(changed)
    for b in range(B):
        want[li, :, int(pt[b][ctx[b] // R.PAGE]), :, ctx[b] % R.PAGE] = True
    assert torch.equal(changed, want), f"K / V token rows changed: {changed.nonzero().tolist()[:8]} ..., expected {want.nonzero().tolist()[:8]} ..."


@pytest.mark.parametrize("model,B", CASES)
def test_qkv_rope_and_kv_append(engines, model, B):
    """q rows, the rotated K row and the V row at ctx_len[b] (contexts 0 .. max_ctx - 2 mixed in one batch) on the identity and on a shuffled
    page table; every other cache row, the other layer and the hidden rows bit-unchanged"""
    e = engines(model)
    for li in range(R.LAYERS):
        _qkv_once(e, B, li, None)
        _qkv_once(e, B, li, R.shuffled_pages(B, e.max_pages, (B, li)))


def test_qkv_with_fp8_kv_cache_writes_the_staging_rows(engines):
    e = engines("G4kv8")
    _qkv_once(e, 3, 1, R.shuffled_pages(3, e.max_pages, (3, 1, 1)), kv8=True)


# ---- O-PROJ / DOWN ------------------------------------------------------------------------------------------------------------------------
def _resid_once(e, stage, B, li):
    if stage == OPROJ:
        form_in, ns = e.oproj_form(B)
        if form_in == 1:   # split partials: unequal maxima, one empty split -- the reference is the float64 merge
            x = R.attn_partials(B, e.Hq, ns, (B, li))
            assert ns > 1
            wx, out_name = R.ref_oproj(e.W, li, R.ref_merge(x)), "oproj_split"
        else:
            assert form_in == 0
            x = R.attn_rows(B, e.q_dim, (B, li))
            wx, out_name = R.ref_oproj(e.W, li, x), "oproj"
    else:
        x = M.act_rows4(B, (B, li))
        wx, out_name = M.ref_down4(e.W, li, x), "down"
    rms = wx.pow(2).mean().sqrt().item()
    # the fp32 stream: not bf16-representable and ~30 x the size of W x -- a kernel adding into the bf16 mirror instead loses W x in its rounding
    h32, h = e.hidden_rows((B, li, stage), scale=30.0 * rms)
    assert not torch.equal(h32, h.float())
    res = e.run(stage, B, li, h32=h32, h=h, x=x)
    what = f"{'o-proj' if stage == OPROJ else 'down'} (layer {li}, B {B}, {out_name})"
    check(res["h32"][:B].double() - h32[:B].double(), wx, out_name, what + ": h32_out - h32_in against W x")
    assert torch.equal(bits(res["h"][:B]), bits(R.bf(res["h32"][:B]))), what + ": the bf16 mirror is not bf16(h32_out)"
    assert torch.equal(bits(res["h"][B:]), bits(h[B:])) and torch.equal(bits(res["h32"][B:]), bits(h32[B:])), what + f": rows {B}.. changed"
    return out_name


@pytest.mark.parametrize("model,B", CASES)
def test_oproj_residual_and_split_merge(engines, model, B):
    e = engines(model)
    names = {_resid_once(e, OPROJ, B, li) for li in range(R.LAYERS)}
    # both input forms are covered by the cases: 2 kv heads split at every batch, 32 kv heads run one split from 5 rows on
    assert names == ({"oproj_split"} if model == "G4" else {"oproj"})


@pytest.mark.parametrize("model,B", CASES)
def test_down_residual_phased_kernel(engines, model, B):
    """K = 4224 = 33 load steps of 128 over eight waves: wave 0 owns five, the others four (two phases at 1-8 rows, four at 9-16)"""
    e = engines(model)
    for li in range(R.LAYERS):
        _resid_once(e, DOWN, B, li)


# ---- GATE/UP ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,B", CASES)
def test_gateup_swiglu(engines, model, B):
    e = engines(model)
    for li in range(R.LAYERS):
        h32, h = e.hidden_rows((B, li, 3))
        res = e.run(GATEUP, B, li, h32=h32, h=h)
        check(res["y"], R.ref_gateup(e.W, li, h32[:B]), "gateup", f"gate/up (layer {li}, B {B})")
        assert torch.equal(bits(res["h"]), bits(h)) and torch.equal(bits(res["h32"]), bits(h32)), "gate/up changed the hidden rows"


# ---- LM-HEAD ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,B", CASES)
def test_lmhead_logits_and_greedy_token(engines, model, B):
    e = engines(model)
    h32, h = e.hidden_rows((B, 99))
    res = e.run(LMHEAD, B, h32=h32, h=h)
    ref = R.ref_lmhead(e.W, h32[:B])
    check(res["y"], ref, "lmhead", f"lm-head logits (B {B})")
    rtol, atol, _ = M.tolerances4("lmhead")
    tok = res["tok"].tolist()
    for b in range(B):
        assert 0 <= tok[b] < R.VOCAB
        top = torch.topk(ref[b], 2)
        tol = atol * ref[b].pow(2).mean().sqrt().item() + rtol * top.values[0].abs().item()
        if (top.values[0] - top.values[1]).item() > 2.0 * tol:   # a priori: twice the logit tolerance
            assert tok[b] == int(top.indices[0]), f"row {b}: token {tok[b]}, reference argmax {int(top.indices[0])}"
        assert tok[b] == int(res["y"][b].argmax()), f"row {b}: the finish picked {tok[b]}, the logit row's own argmax is {int(res['y'][b].argmax())}"
    assert torch.equal(bits(res["h"]), bits(h)) and torch.equal(bits(res["h32"]), bits(h32)), "lm-head changed the hidden rows"


NEG_BEST = 31999
TIE_I, TIE_J = 1029, 30003   # tiles 64 / 1875: different tiles and blocks, i < j


def _crafted_sd(kind):
    """model W4 with a modified lm_head and final norm (as tests/test_decode_stages_gpu.py crafts them).  `negative`: every lm_head entry < 0 and
    the norm weight positive, so that positive hidden rows give strictly negative logits -- also after quantisation: an element that rounds to
    zero comes back as +0, never positive, and no row rounds to zero as a whole; row NEG_BEST is the least negative by a wide margin.
    `tie`: rows TIE_I < TIE_J identical (0.25: on the grid) and the global maximum."""
    sd = dict(M.make_state_dict4("W4"))
    head = sd["language_model.lm_head.weight"].float()
    sd["language_model.model.norm.weight"] = R.bf(sd["language_model.model.norm.weight"].float().abs() + 0.05)
    if kind == "negative":
        head = -head.abs() - 1e-3
        head[NEG_BEST] = -1e-4
    else:
        head[TIE_I] = 0.25
        head[TIE_J] = head[TIE_I]
    sd["language_model.lm_head.weight"] = R.bf(head)
    return sd


@pytest.mark.parametrize("kind", ["negative", "tie"])
def test_lmhead_argmax_edge_cases(device, kind):
    """every logit negative (the zero rows that pad the vocabulary to the tile would win an unguarded argmax), and two identical rows in different
    tiles holding the maximum (the lower id wins): 1, 5 and 16 rows (both staged widths)"""
    e = Eng4(device, "W4", 16, sd=_crafted_sd(kind))
    try:
        for B in (1, 5, 16):
            h32 = (torch.rand(e.rows, e.hidden, generator=R.gen(41, B)) + 0.1).float()
            res = e.run(LMHEAD, B, h32=h32)
            ref = R.ref_lmhead(e.W, h32[:B])
            tok = res["tok"].tolist()
            if kind == "negative":
                assert (ref < 0).all() and (res["y"] < 0).all()
                assert [int(i) for i in ref.argmax(-1)] == [NEG_BEST] * B
                assert tok == [NEG_BEST] * B, tok
            else:
                assert all(int(i) in (TIE_I, TIE_J) for i in ref.argmax(-1)) and torch.allclose(ref[:, TIE_I], ref[:, TIE_J], rtol=1e-12, atol=0)
                assert torch.equal(bits(res["y"][:, TIE_I]), bits(res["y"][:, TIE_J])), "the two rows' logits differ: the tie is not one"
                assert tok == [TIE_I] * B, tok
    finally:
        e.eng.close()


# ---- refusals: decided on the host, before any launch -----------------------------------------------------------------------------------------
def test_refusals_name_the_format_and_launch_nothing(device):
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.engine import _config_c

    so = _lib.load()
    torch.cuda.synchronize()
    bad = EmmaXConfig.tiny()                      # hidden 256: no MXFP4 kernel takes K = 256
    bad.decode_weight_dtype = "mxfp4"
    h, cc = C.c_void_p(), _config_c(bad)
    assert so.emmax_model_create(C.byref(cc), C.byref(h)) == -1 and b"MXFP4" in so.emmax_last_error()
    h, cc = C.c_void_p(), _config_c(M.make_cfg4("W4"))
    assert so.emmax_model_create(C.byref(cc), C.byref(h)) == 0
    assert so.emmax_model_max_decode_batch(h) == 16
    ws, kv = C.c_int64(), C.c_int64()
    assert so.emmax_session_bytes(h, 16, 8, 320, C.byref(ws), C.byref(kv)) == 0
    assert so.emmax_session_bytes(h, 17, 8, 320, C.byref(ws), C.byref(kv)) == -1 and b"MXFP4" in so.emmax_last_error()
    with _lib.tuning(exact=1):
        assert so.emmax_session_bytes(h, 1, 8, 320, C.byref(ws), C.byref(kv)) == -1 and b"MXFP4" in so.emmax_last_error()
    so.emmax_model_destroy(h)
    with pytest.raises(_lib.EmmaxError, match="MXFP4"):   # the same refusals through the engine: the model is built, the session is not
        Eng4(device, "W4", 17)
    with pytest.raises(_lib.EmmaxError, match="MXFP4"):
        from emmax.engine import EmmaxEngine

        EmmaxEngine(M.make_cfg4("G4"), dict(M.make_state_dict4("G4")), device=device, max_batch=1, max_prompt=R.MAX_PROMPT, max_ctx=R.MAX_CTX, exact=True)


def test_arena_of_an_mxfp4_7b_model():
    """sizing only, no GPU memory: bf16 arena + 6.61 B parameters x 4.25 / 8 bytes within 2 %"""
    from test_mxfp4_ref import test_arena_of_an_mxfp4_7b_model as sizing

    sizing()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _model(device, sd_bf, max_batch, max_prompt=40):
    from emmax.modeling import EmmaXForActionPrediction

    return EmmaXForActionPrediction(M.e2e_cfg(), dict(sd_bf)).to(device, max_batch=max_batch, max_prompt=max_prompt)


def test_planted_generation_equals_the_oracle_on_dequantised_weights(device):
    """generate at B = 1 and a ragged B = 3: ids equal to the oracle's on the de-quantised planted weights and to the a-priori chain
    (tests/test_mxfp4_ref.py: every one of these steps clears the id line on the CPU)"""
    from emmax.weights import planted_chain

    cfg = M.e2e_cfg()
    sd_bf = M.e2e_state_dict(True, M.E2E_PLANTED_SEED)
    sd_q = M.dequant_state_dict(sd_bf)
    model = _model(device, sd_bf, 3)
    assert model.config.decode_weight_dtype == "mxfp4"
    for frames, rows in M.planted_rows(cfg):
        _, new_ids, lens = model.generate_actions_batch(torch.from_numpy(frames).to(device), rows, max_new_tokens=M.PLANTED_MAX_NEW)
        for b, row in enumerate(rows):
            got = new_ids[b, : int(lens[b])].cpu().tolist()
            chain = planted_chain(cfg, row[-1], M.PLANTED_MAX_NEW)
            ref, _ = M.oracle_trace(cfg, sd_q, frames[b:b + 1], row, len(chain))
            assert got == ref == chain, (b, got, ref, chain)
            assert got[-1] == cfg.eos_token_id and (new_ids[b, int(lens[b]):] == cfg.pad_token_id).all()
    model.engine.close()


@pytest.fixture(scope="module")
def random_e2e(device):
    cfg = M.e2e_cfg()
    sd_bf = M.e2e_state_dict(False, M.E2E_RANDOM_SEED)
    sd_q = M.dequant_state_dict(sd_bf)
    frames, rows = M.e2e_inputs(8, M.E2E_LENS8, seed=2024)
    gens, traces = [], []
    for b in range(8):
        g, t = M.oracle_trace(cfg, sd_q, frames[b:b + 1], rows[b], M.E2E_STEPS)
        gens.append(g)
        traces.append(t)
    model = _model(device, sd_bf, 8)
    yield cfg, model, sd_q, frames, rows, gens, traces
    model.engine.close()


def _teacher_forced(model, frames, rows, gens, traces, sel, T, device):
    eng = model.engine
    model._prefill([rows[i] for i in sel], None, torch.from_numpy(frames[sel]).to(device), max_new=T + 1)
    worst, checked, agree, logits = 0.0, 0, 0, []
    for t in range(T):
        got = eng.last_logits().float().cpu()
        logits.append(got.clone())
        for j, i in enumerate(sel):
            ref = traces[i][t]
            worst = max(worst, (got[j] - ref).abs().max().item() / ref.abs().max().item())
            if above_id_line(ref, ID_BUDGET_SHALLOW):
                checked += 1
                agree += int(int(got[j].argmax()) == gens[i][t])
        eng.set_current_tokens([gens[i][t] for i in sel])
        eng.decode_step()
    return worst, checked, agree, logits


# (row, step) pairs of the 16 teacher-forced steps whose oracle margin clears the id line, counted with the CPU oracle for seed E2E_RANDOM_SEED:
# row 0 alone 11 of 16, the eight rows 70 of 128
ABOVE_LINE = {1: 11, 8: 70}


@pytest.mark.parametrize("sel", [[0], list(range(8))], ids=["B1", "B8"])
def test_random_weights_teacher_forced_eager_and_graph(device, random_e2e, tune, sel):
    """16 teacher-forced steps: per-step logits against the oracle on the de-quantised weights at the 2-layer tolerance (step 0 comes out of the
    prefill: its GEMMs read the written-back rows), the argmax wherever the oracle's margin clears the a-priori id line, and the hipGraph replay
    of the step bit-equal to the eager launches"""
    cfg, model, _, frames, rows, gens, traces = random_e2e
    tune(graph=0)
    worst, checked, agree, eager = _teacher_forced(model, frames, rows, gens, traces, sel, M.E2E_STEPS, device)
    assert not model.engine.graph_active()
    print(f"B {len(sel)}: worst |err| / max|ref| {worst:.3e}, argmax checked {checked}, agreed {agree}")
    assert worst < E2E_TOL, worst
    assert checked == ABOVE_LINE[len(sel)] and checked * 4 >= len(sel) * M.E2E_STEPS, checked
    assert agree == checked, (agree, checked)
    tune(graph=1)
    worst_g, checked_g, agree_g, replay = _teacher_forced(model, frames, rows, gens, traces, sel, M.E2E_STEPS, device)
    assert model.engine.graph_active()
    assert (checked_g, agree_g) == (checked, agree)
    for t, (a, b) in enumerate(zip(eager, replay)):
        assert torch.equal(bits(a), bits(b)), f"step {t}: the replayed graph's logits differ from the eager launches'"


def test_prefill_logits_follow_the_quantised_model(device, random_e2e):
    """the prefill's own lm-head GEMM over the last position of every row (forward), against the same oracle: what fails if the de-quantised
    values are not written back into the row-major copies -- and the unquantised oracle is NOT what the prefill computes"""
    from oracle import emmax_oracle as orc

    cfg, model, sd_q, frames, rows, gens, traces = random_e2e
    sel = [0, 1, 2]
    out = model.forward(input_ids=[rows[i] for i in sel], frames_u8=torch.from_numpy(frames[sel]).to(device), use_cache=True)
    sd_plain = {k: v.float() for k, v in M.e2e_state_dict(False, M.E2E_RANDOM_SEED).items()}
    for j, i in enumerate(sel):
        got = out.logits[j].float().cpu()
        ref = traces[i][0]
        err = (got[-1] - ref).abs().max().item() / ref.abs().max().item()
        assert err < E2E_TOL, (i, err)
        with torch.inference_mode():
            plain, _, _ = orc.vla_prefill_logits(torch.tensor([rows[i]]), orc.preprocess_frames(frames[i:i + 1], cfg), sd_plain, cfg)
        off = (got[-1] - plain[0, -1]).abs().max().item() / plain[0, -1].abs().max().item()
        assert off > 3 * E2E_TOL, (i, off)   # (random weights: 3.3e-1 - 3.8e-1 on the CPU, profiles/mxfp4_quant_error.txt) -- the quantised model is a different model, and the prefill runs it
