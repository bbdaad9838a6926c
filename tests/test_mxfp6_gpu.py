"""MXFP6 e2m3 decode weights (decode_weight_dtype = "mxfp6", emmax_config.decode_fp8 = 4) on the GPU.

  * the quantiser: emmax_op_quant_mxfp6 then emmax_op_dequant_mxfp6, bit-equal to the torch reference of tests/mxfp6_ref.py on random and
    hand-written blocks, in the natural row order and both of decode_km.hip's permutations; the tiles byte for byte the documented layout;
  * what v_cvt_scalef32_pk32_bf16_fp6 makes of hand-packed tiles, element by element, through emmax_op_gemm_small_mxfp6: every one of the 64 element
    codes at every one of a lane's 32 positions (the bit order of the six dwords), every scale code 0 .. 254, on every load step of every wave;
  * every fused decode stage of an MXFP6 model through the step's own dispatch (emmax_op_decode_stage), against the float64 reference on the
    DE-QUANTISED weights with the checks of tests/test_decode_stages_gpu.py, the launcher family asserted (decode_km.hip at every batch 1-16);
  * end to end on the G4 shape with the tiny towers: planted ids, teacher-forced random-weight logits and ids (eager and hipGraph replay,
    bit-equal), the prefill's logits -- prefill and decode evaluate the same quantised model;
  * what the format is for: draft-verified decoding and emmax_extend on an MXFP6 model (an fp8 model still refuses the draft);
  * the refusals (17 rows, exact numerics), none of which launches anything.
"""

import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import decode_stage_ref as R
import mxfp6_ref as M
from conftest import ID_BUDGET_SHALLOW, above_id_line
from test_mxfp4_gpu import Eng4, bits
from test_ops_gpu import assert_elementwise, relerr

pytestmark = pytest.mark.gpu

QKV, OPROJ, GATEUP, DOWN, LMHEAD = 0, 2, 3, 4, 5
E2E_TOL = 3e-2                           # the 2-layer line of tests/test_operating_point_gpu.py / test_e2e_gpu.py


def check(got, ref, out, what):
    rtol, atol, tol = M.tolerances6(out)
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
    tiles = torch.empty(N * K * 6 // 8, dtype=torch.uint8, device=device)
    scales = torch.empty(N * K // 32, dtype=torch.uint8, device=device)
    dst = torch.full((N, K), float("nan"), dtype=torch.bfloat16, device=device)
    st = _lib.current_stream()
    _lib.check(lib.emmax_op_quant_mxfp6(src.data_ptr(), K, tiles.data_ptr(), scales.data_ptr(), N, K, perm, hd, st), "emmax_op_quant_mxfp6")
    _lib.check(lib.emmax_op_dequant_mxfp6(tiles.data_ptr(), scales.data_ptr(), dst.data_ptr(), K, N, K, perm, hd, st), "emmax_op_dequant_mxfp6")
    torch.cuda.synchronize()
    return dst.cpu(), tiles.cpu(), scales.cpu()


@pytest.mark.parametrize("perm,hd", [(0, 0), (1, 32), (2, 0)], ids=["natural", "qkv-perm", "gateup-perm"])
def test_quant_dequant_is_bit_equal_to_the_torch_reference(device, perm, hd):
    """32 x 1024: random rows of very different scale with every hand-written block planted (every magnitude with both signs, the ties of every
    binade, saturation, the all-zero block, the clamped exponent with bf16 denormals, the largest bf16).  The permutations only move rows between
    tiles: the values come back at the rows they were taken from.  Natural order: the tile and scale streams are byte for byte what the
    documented layout (mxfp6_ref.pack_tiles) makes of the reference's codes."""
    W, want = M.adversarial_matrix()
    got, tiles, scales = _quant_roundtrip(device, W, perm, hd)
    want_bf = want.to(torch.bfloat16)
    assert torch.equal(want_bf.double(), want)
    bad = (bits(got) != bits(want_bf)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()}, want {want_bf[tuple(bad[0])].item()}"
    # a second pass over the de-quantised values changes nothing: what finalize writes back is a fixed point of the quantiser
    again, _, _ = _quant_roundtrip(device, got, perm, hd)
    assert torch.equal(bits(again), bits(got))
    if perm == 0:
        q, e = M.quantize(W)
        amax0 = W.float().view(32, 32, 32).abs().amax(-1) == 0
        code = torch.where(amax0, torch.full_like(e, 127), e + 127).to(torch.uint8)
        neg = torch.signbit(W.float())               # the sign bit is the weight's own, also where the magnitude rounds to zero (and for -0)
        want_tiles, want_scales = M.pack_tiles(M.codes_of(q, negative=neg), code)
        assert torch.equal(scales, want_scales), "scale stream differs from the documented layout"
        bad = (tiles != want_tiles).nonzero()
        assert bad.numel() == 0, f"{bad.shape[0]} tile bytes differ from the documented layout, first at byte {int(bad[0])}"


def test_quantiser_refuses_shapes_outside_the_tiles(device):
    from emmax import _lib

    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    for N, K, ld, perm, hd in ((24, 128, 128, 0, 0), (32, 192, 192, 0, 0), (32, 128, 64, 0, 0), (32, 128, 128, 1, 24), (48, 128, 128, 2, 0), (32, 128, 128, 3, 0)):
        assert lib.emmax_op_quant_mxfp6(buf.data_ptr(), ld, buf.data_ptr(), buf.data_ptr(), N, K, perm, hd, _lib.current_stream()) == -1
        assert lib.emmax_op_dequant_mxfp6(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ld, N, K, perm, hd, _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert int(buf.max()) == 0


WN, WK = 256, 2048


def _widening_matrix():
    """256 x 2048, hand-packed.  Row r holds ONE non-zero block, block r % 64 of its 64 -- K = 2048 is two load steps per wave, so the planted blocks
    sit on every wave's first and last load step, the last ones directly in front of the next wave's slice (the first step past a wave's own) --
    with scale code r (0 .. 254; row 255 stays empty: code 255 is e8m0's NaN) and element code (r + p) % 64 at position p: every one of the 64 codes at
    every one of the 32 positions within rows 0 .. 63, every scale code once.  Rows with codes 253 / 254 keep magnitudes below 2 (element codes
    (r + p) % 16, alternating signs) so that the value is finite in bf16.  Returns (codes, scale codes, value float64 [N, K], block of row)."""
    r = torch.arange(WN)[:, None]
    p = torch.arange(32)[None, :]
    el = (r + p) % 64
    el = torch.where(r >= 253, (r + p) % 16 + 32 * (p % 2), el)
    codes = torch.zeros(WN, WK, dtype=torch.uint8)
    sc = torch.full((WN, WK // 32), 127, dtype=torch.uint8)
    val = torch.zeros(WN, WK, dtype=torch.float64)
    grid = torch.tensor(M.E2M3, dtype=torch.float64)
    for row in range(WN - 1):
        b = row % 64
        codes[row, b * 32:(b + 1) * 32] = el[row].to(torch.uint8)
        sc[row, b] = row
        v = grid[el[row] % 32] * torch.where(el[row] >= 32, -1.0, 1.0).double()
        val[row, b * 32:(b + 1) * 32] = v * 2.0 ** (row - 127)
    return codes, sc, val


@pytest.mark.parametrize("rows", [8, 16], ids=["NB8", "NB16"])
def test_hardware_widening_every_code_at_every_position_and_every_scale_code(device, rows):
    """What v_cvt_scalef32_pk32_bf16_fp6 makes of the tiles, element by element, through the decode kernel itself (emmax_op_gemm_small_mxfp6: the
    K-split kernel's plain form, 8 and 16 staged rows).  Batch row b is one-hot at element off + b of every block, scaled by a power of two per
    block (2^(31 - block): the four rows that share a block index have scale codes 64 apart, the products land on 2^-96 .. 2^96 times the element)
    so that products and outputs are normal numbers: y[b, r] is exactly x times ONE de-quantised element, and the expectation is the e2m3 value of
    the planted code times 2^(scale code - 127), a priori.  A wrong order of the 32 elements inside the six dwords, or of the six dwords over the two
    loads, shows as another element's value; a wrong activation fragment order as another position's.
    Elements whose de-quantised value is a bf16 DENORMAL (below 2^-126: scale codes 0 .. 3) reach the MFMA as denormal operands, which the matrix
    pipe is allowed to flush: for those, and only those, 0 is accepted beside the exact value -- for all of
    them or for none."""
    from emmax import _lib

    lib = _lib.load()
    codes, sc, val = _widening_matrix()
    assert torch.equal(val.to(torch.bfloat16).double(), val)              # every planted value is exact in bf16
    for p in range(32):                                                    # the coverage the test is about
        assert set(codes[:64, :].view(64, 64, 32)[torch.arange(64), torch.arange(64), p].tolist()) == set(range(64))
    assert sorted(sc[torch.arange(WN - 1), torch.arange(WN - 1) % 64].tolist()) == list(range(255))
    tiles_h, scales_h = M.pack_tiles(codes, sc)
    tiles, scales = tiles_h.to(device), scales_h.to(device)
    sx = torch.pow(torch.tensor(2.0, dtype=torch.float64), 31.0 - torch.arange(WK // 32).double())
    st = _lib.current_stream()
    flushed = denormal = 0
    for off in range(0, 32, rows):
        x = torch.zeros(rows, WK, dtype=torch.float64)
        for b in range(rows):
            x[b, off + b::32] = sx
        xb = x.to(torch.bfloat16)
        assert torch.equal(xb.double(), x)
        y = torch.full((rows, WN), float("nan"), dtype=torch.bfloat16, device=device)
        xd = xb.to(device)
        _lib.check(lib.emmax_op_gemm_small_mxfp6(xd.data_ptr(), tiles.data_ptr(), scales.data_ptr(), y.data_ptr(), rows, WN, WK, st), "emmax_op_gemm_small_mxfp6")
        torch.cuda.synchronize()
        got = y.cpu()
        for r in range(WN - 1):
            blk = r % 64
            for b in range(rows):
                w = val[r, blk * 32 + off + b].item()
                want = torch.tensor(w * sx[blk].item(), dtype=torch.float64).to(torch.bfloat16)
                assert float(want) == w * sx[blk].item()                               # the expectation is exact in bf16
                g = got[b, r]
                denormal += int(0 < abs(w) < 2.0 ** -126)
                ok = bits(g.reshape(1)).item() == bits(want.reshape(1)).item() or (float(g) == 0.0 and float(want) == 0.0)
                if not ok and 0 < abs(w) < 2.0 ** -126 and float(g) == 0.0:
                    flushed += 1
                    ok = True
                assert ok, (f"row {r} (scale code {r}), position {off + b} (element code {int(codes[r, blk * 32 + off + b])}): got {float(g)!r}, "
                            f"de-quantised weight {w!r} x {sx[blk].item()!r} = {float(want)!r}")
        assert (got[:, WN - 1] == 0).all(), "the empty row gave non-zero outputs"
    print(f"bf16-denormal weight elements that reached the output as 0: {flushed} of {denormal}")
    # flushing denormal operands is a mode of the matrix pipe, not a property of an element: all of them or none -- a block zeroed for another
    # reason (a wrong mask on scale codes 0 .. 3) is neither
    assert denormal > 0 and flushed in (0, denormal), (flushed, denormal)


def test_dequantiser_on_every_code_and_scale_code(device):
    """emmax_op_dequant_mxfp6 over the hand-packed tiles of the widening test: every element code at every position, every scale code 0 .. 254,
    bit-equal to the e2m3 value times 2^(code - 127) (bf16 denormals included: integer arithmetic, nothing is flushed)"""
    from emmax import _lib

    lib = _lib.load()
    codes, sc, val = _widening_matrix()
    tiles_h, scales_h = M.pack_tiles(codes, sc)
    tiles, scales = tiles_h.to(device), scales_h.to(device)
    dst = torch.full((WN, WK), float("nan"), dtype=torch.bfloat16, device=device)
    _lib.check(lib.emmax_op_dequant_mxfp6(tiles.data_ptr(), scales.data_ptr(), dst.data_ptr(), WK, WN, WK, 0, 0, _lib.current_stream()), "emmax_op_dequant_mxfp6")
    torch.cuda.synchronize()
    got, want = dst.cpu(), val.to(torch.bfloat16)
    same = (bits(got) == bits(want)) | ((got.float() == 0) & (want.float() == 0))
    bad = (~same).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()!r}, want {want[tuple(bad[0])].item()!r}"


# ---- engines ----------------------------------------------------------------------------------------------------------------------------
class Eng6(Eng4):
    """one MXFP6 model + session and the float64 de-quantised weights its references read (test_mxfp4_gpu.Eng4's stage runner on this format)"""

    def __init__(self, device, model, max_batch, kv_fp8=False, sd=None):
        from emmax import _lib
        from emmax.engine import EmmaxEngine

        self.L, self.lib = _lib, _lib.load()
        self.model, self.kv_fp8 = model, kv_fp8
        self.cfg = M.make_cfg6(model)
        self.sd = sd if sd is not None else M.make_state_dict6(model)
        self.W = M.Weights6(self.sd, self.cfg)
        with (_lib.tuning(kv_fp8=1) if kv_fp8 else contextlib.nullcontext()):
            self.eng = EmmaxEngine(self.cfg, dict(self.sd), device=device, max_batch=max_batch, max_prompt=R.MAX_PROMPT, max_ctx=R.MAX_CTX)
        self.eng.ensure_decode_batch(max_batch)
        assert int(self.lib.emmax_model_aux_bytes(self.eng._model)) == 0
        self.device, self.rows = device, max_batch
        self.Hq, self.Hkv = M.MODELS6[model]
        self.hidden, self.q_dim = M.HIDDEN6, self.Hq * R.HEAD_DIM
        self.max_pages = (R.MAX_CTX + R.PAGE - 1) // R.PAGE
        self.eng.kv.random_(0, 256)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def engines(device):
    made = {}
    spec = {"G4": dict(model="G4", max_batch=8), "W4": dict(model="W4", max_batch=16), "G4kv8": dict(model="G4", max_batch=8, kv_fp8=True)}

    def get(name):
        if name not in made:
            made[name] = Eng6(device, **spec[name])
        return made[name]

    yield get
    for e in made.values():
        e.eng.close()


CASES = [pytest.param(m, B, id=f"{m}-B{B}") for m in ("G4", "W4") for B in M.BATCHES6[m]]


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
        x = M.act_rows6(B, (B, li))
        wx, out_name = M.ref_down6(e.W, li, x), "down"
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
    rtol, atol, _ = M.tolerances6("lmhead")
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
    """model W4 with a modified lm_head and final norm (as tests/test_mxfp4_gpu.py crafts them).  `negative`: every lm_head entry < 0 and the norm
    weight positive, so that positive hidden rows give strictly negative logits -- also after quantisation: an element that rounds to zero comes
    back as +0, never positive, and no row rounds to zero as a whole; row NEG_BEST is the least negative by a wide margin.
    `tie`: rows TIE_I < TIE_J identical (0.25: on the grid) and the global maximum."""
    sd = dict(M.make_state_dict6("W4"))
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
    e = Eng6(device, "W4", 16, sd=_crafted_sd(kind))
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
def test_refusals_name_the_format_and_leave_the_session_usable(device, engines):
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.engine import EmmaxEngine, _config_c

    so = _lib.load()
    e = engines("W4")
    torch.cuda.synchronize()
    bad = EmmaXConfig.tiny()                      # hidden 256: no MXFP6 kernel takes K = 256
    bad.decode_weight_dtype = "mxfp6"
    h, cc = C.c_void_p(), _config_c(bad)
    assert so.emmax_model_create(C.byref(cc), C.byref(h)) == -1 and b"MXFP6" in so.emmax_last_error()
    ws, kv = C.c_int64(), C.c_int64()
    assert so.emmax_model_max_decode_batch(e.eng._model) == 16
    assert so.emmax_session_bytes(e.eng._model, 16, 8, 320, C.byref(ws), C.byref(kv)) == 0
    assert so.emmax_session_bytes(e.eng._model, 17, 8, 320, C.byref(ws), C.byref(kv)) == -1 and b"MXFP6" in so.emmax_last_error()
    with _lib.tuning(exact=1):
        assert so.emmax_session_bytes(e.eng._model, 1, 8, 320, C.byref(ws), C.byref(kv)) == -1 and b"MXFP6" in so.emmax_last_error()
    with pytest.raises(_lib.EmmaxError, match="MXFP6"):   # the same refusals through the engine: the model is built, the session is not
        Eng6(device, "W4", 17)
    with pytest.raises(_lib.EmmaxError, match="MXFP6"):
        EmmaxEngine(M.make_cfg6("G4"), dict(M.make_state_dict6("G4")), device=device, max_batch=1, max_prompt=R.MAX_PROMPT, max_ctx=R.MAX_CTX, exact=True)
    # the session that was there before is usable: a stage of it still runs and is right
    h32, h = e.hidden_rows((16, 99))
    res = e.run(LMHEAD, 16, h32=h32, h=h)
    check(res["y"], R.ref_lmhead(e.W, h32[:16]), "lmhead", "lm-head logits after the refusals (B 16)")


def test_arena_of_an_mxfp6_7b_model():
    """sizing only, no GPU memory: bf16 arena + 6.61 B parameters x 6.25 / 8 bytes"""
    from test_mxfp6_ref import test_arena_of_an_mxfp6_7b_model as sizing

    sizing()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _model(device, sd_bf, max_batch, max_prompt=40, **kw):
    from emmax.modeling import EmmaXForActionPrediction

    return EmmaXForActionPrediction(M.e2e_cfg(), dict(sd_bf)).to(device, max_batch=max_batch, max_prompt=max_prompt, **kw)


@pytest.fixture(scope="module")
def planted_model(device):
    cfg = M.e2e_cfg()
    sd_bf = M.e2e_state_dict(True, M.E2E_PLANTED_SEED)
    model = _model(device, sd_bf, 3, max_prompt=64)
    assert model.config.decode_weight_dtype == "mxfp6"
    yield cfg, model, sd_bf
    model.engine.close()


def test_planted_generation_equals_the_oracle_on_dequantised_weights(device, planted_model):
    """generate at B = 1 and a ragged B = 3: ids equal to the oracle's on the de-quantised planted weights and to the a-priori chain
    (tests/test_mxfp6_ref.py: every one of these steps clears the id line on the CPU)"""
    from emmax.weights import planted_chain

    cfg, model, sd_bf = planted_model
    sd_q = M.dequant_state_dict(sd_bf)
    for frames, rows in M.planted_rows(cfg):
        _, new_ids, lens = model.generate_actions_batch(torch.from_numpy(frames).to(device), rows, max_new_tokens=M.PLANTED_MAX_NEW)
        for b, row in enumerate(rows):
            got = new_ids[b, : int(lens[b])].cpu().tolist()
            chain = planted_chain(cfg, row[-1], M.PLANTED_MAX_NEW)
            ref, _ = M.oracle_trace(cfg, sd_q, frames[b:b + 1], row, len(chain))
            assert got == ref == chain, (b, got, ref, chain)
            assert got[-1] == cfg.eos_token_id and (new_ids[b, int(lens[b]):] == cfg.pad_token_id).all()


# ---- what the format is for: one model for every pass -------------------------------------------------------------------------------------------
def test_drafted_generation_equals_the_plain_call_and_accepts_the_answer(device, planted_model):
    """generate_ids(rows, draft=[...]) on an MXFP6 model: the verify pass multiplies by the de-quantised rows the decode step streams as tiles, so a
    draft changes the number of weight passes and nothing else -- the ids of the plain call whatever the draft says (the answer itself, a
    corrupted answer, an unrelated guess, no draft for a row), and the answer as its own draft is accepted.  An fp8 model still refuses."""
    from emmax.config import EmmaXConfig
    from emmax.drafting import DraftParams
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import planted_chain, synthetic_state_dict

    cfg, model, _ = planted_model
    params = DraftParams(window=8)
    for frames, rows in M.planted_rows(cfg):
        fr = torch.from_numpy(frames).to(device)
        ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=M.PLANTED_MAX_NEW)
        plain = [ids[b, : int(lens[b])].cpu().tolist() for b in range(len(rows))]
        assert plain == [planted_chain(cfg, r[-1], M.PLANTED_MAX_NEW) for r in rows]
        wrong = [[3 + (t + 17) % 30000 if i % 5 == 2 else t for i, t in enumerate(p)] for p in plain]
        unrelated = [[7 + 3 * i for i in range(len(p))] for p in plain]
        for name, draft in (("answer", [list(p) for p in plain]), ("corrupted", wrong), ("unrelated", unrelated),
                            ("mixed", [list(plain[0])] + [None] * (len(rows) - 1))):
            model.last_draft_stats = None
            ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=M.PLANTED_MAX_NEW, draft=draft, draft_params=params)
            got = [ids[b, : int(lens[b])].cpu().tolist() for b in range(len(rows))]
            stats = model.last_draft_stats
            print(f"B {len(rows)} draft {name}: {stats.passes} passes, {stats.plain_steps} plain steps, accepted {stats.accepted} of {stats.drafted}")
            assert got == plain, (name, got, plain)
            if name == "answer":
                assert all(a >= 1 for a in stats.accepted), stats
            if name == "unrelated":
                assert sum(stats.accepted) == 0, stats
    cfg8 = EmmaXConfig.tiny()
    cfg8.decode_weight_dtype = "fp8"
    m8 = EmmaXForActionPrediction(cfg8, {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg8, seed=5, planted=True).items()})
    with pytest.raises(NotImplementedError, match="fp8"):
        m8.generate_ids([[1, 5, 9]], frames_u8=torch.zeros(1, 224, 224, 3, dtype=torch.uint8), max_new_tokens=8, draft=[[5, 6]])


def test_extend_then_teacher_forced_steps_follow_the_quantised_model(device, planted_model):
    """prefill a prompt, emmax_extend it by 21 tokens, then 6 teacher-forced decode steps: the extension's logit rows and every step's logits
    against the fp32 oracle's whole-sequence forward on the de-quantised weights -- the extension GEMMs read the written-back rows, the steps the
    tiles: one model"""
    from oracle import emmax_oracle as orc

    cfg, model, sd_bf = planted_model
    sd_q = M.dequant_state_dict(sd_bf)
    eng = model.engine
    P_LEN, X_LEN, T = [12, 7], [21, 5], 6
    frames, rows = M.e2e_inputs(2, [p + x + T for p, x in zip(P_LEN, X_LEN)], seed=303)
    P = [r[:p] for r, p in zip(rows, P_LEN)]
    X = [r[p:p + x] for r, p, x in zip(rows, P_LEN, X_LEN)]
    Tf = [r[p + x:] for r, p, x in zip(rows, P_LEN, X_LEN)]
    ref = []
    with torch.inference_mode():
        for b in range(2):
            logits, _, _ = orc.vla_prefill_logits(torch.tensor([rows[b]]), orc.preprocess_frames(frames[b:b + 1], cfg), sd_q, cfg)
            ref.append(logits[0].float())
    S = [cfg.n_patches + p for p in P_LEN]
    model._prefill(P, None, torch.from_numpy(frames).to(device), max_new=max(X_LEN) + T + 2)
    assert eng.context_lengths(0, 2) == S
    assert eng.extend(X, max_new_tokens=T + 1) == [s + x for s, x in zip(S, X_LEN)]
    got = eng.prefill_logits()
    worst = 0.0
    for b in range(2):
        want = ref[b][S[b]:S[b] + X_LEN[b]]
        g = got[b].float().cpu()
        assert g.shape == want.shape
        worst = max(worst, ((g - want).abs().max() / want.abs().max()).item())
    tol = M.tolerances6("lmhead")[2]         # the stage tolerance of the logits
    print(f"extension rows: worst |err| / max|ref| {worst:.3e} (bound {tol:.3e})")
    assert worst < tol, worst
    for t in range(T):
        eng.set_current_tokens([Tf[b][t] for b in range(2)])
        eng.decode_step()
        lg = eng.last_logits().float().cpu()
        for b in range(2):
            want = ref[b][S[b] + X_LEN[b] + t]
            worst = max(worst, ((lg[b] - want).abs().max() / want.abs().max()).item())
    print(f"+ {T} teacher-forced steps: worst |err| / max|ref| {worst:.3e} (bound {tol:.3e})")
    assert worst < tol, worst


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


# (row, step) pairs of the 16 teacher-forced steps whose oracle margin clears the id line, counted with the CPU oracle on the de-quantised MXFP6
# weights of seed E2E_RANDOM_SEED: row 0 alone 15 of 16, the eight rows 107 of 128
ABOVE_LINE = {1: 15, 8: 107}


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
    """the prefill's own lm-head GEMM over the last position of every row (forward), against the oracle on the de-quantised weights: what fails
    if the de-quantised values are not written back into the row-major copies is the bit-level agreement below -- the format's own error on
    random weights is of the size of the tolerance, so the sharper statement is that the prefill is CLOSER to the quantised model than to the
    unquantised one on every row"""
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
        fmt = (ref - plain[0, -1]).abs().max().item() / plain[0, -1].abs().max().item()
        print(f"row {i}: from the quantised oracle {err:.3e}, from the unquantised {off:.3e} (the two oracles apart: {fmt:.3e})")
        assert err < off, (i, err, off)
