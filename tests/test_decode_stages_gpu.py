"""Every fused decode-step projection against a float64 reference, ONE stage at a time through the step's own dispatch
(emmax_op_decode_stage, include/emmax.h: launch_proj / stage_params / run_decode_stage / run_lm_head_step of step.hip, the weight copies of
emmax_model_finalize / emmax_model_build_aux, the two-launch splits).  The whole-model tests see these kernels only through final logits at
1.5e-2 .. 4.5e-2 of max|logit|; here each stage's own outputs are compared: the RMSNorm prologue, RoPE and the paged K / V append (bf16 cache,
the fp8 cache's staging rows, the 24-bit cache of exact numerics), SwiGLU over the interleaved (gate, up) rows, the residual add into the fp32
stream and its bf16 mirror, the split merge in the o-proj, the lm-head's argmax partials and logit rows, and the row-permuted weight copies.

Models (tests/decode_stage_ref.py): hidden 256, head_dim 128, 2 layers, vocab 32064 (a 64-row tail past the last 128), intermediate size 4160
(just past 4096: the phased down kernels of decode_km.hip / decode_kmp.hip run, with phases shorter than full).  G = 4 / 2 heads (GQA, split
attention partials at every batch), W = 32 / 32 heads (one split from 5 rows on: decode batches up to 64), H = W at hidden 512 (fp8 only).  References are plain torch in
float64 from the HF-named weights (fp8: the de-quantised values); tolerances come from a CPU emulation of the documented roundings, never from
a kernel's output (decode_stage_ref.py).  Every test asserts the launcher family the op reports, so a silent fall-back cannot pass for coverage.

Cells (stage x launcher family x weights) that launch_proj cannot reach, or cannot reach at these dimensions:
  * bf16 weights on the fp8 row GEMV, fp8 weights on decode_ks.hip / the staged GEMV: the families are defined by the weight type.
  * exact numerics on the staged GEMV, the fp8 row GEMV, decode_kmp.hip, decode_mfma.hip: launch_proj serves exact sessions from the two-term
    forms of decode_ks.hip (1-2 rows) and decode_km.hip (3-8 rows, larger batches in chunks of 8) or fails.
  * bf16 o-proj with split partials on decode_km.hip (it hands that form to decode_mfma.hip) and on decode_kmp.hip (9+ rows need one split).
  * bf16 weights on decode_mfma.hip above 8 rows, and the staged GEMV / decode_ks.hip above 2 rows -- except the ONE-row remainder of a 33-row
    down projection / lm-head (32 + 1 rows: the second launch is a batch-1 launch), which is asserted as such below.
  * fp8 qkv / gate-up / lm-head on decode_km.hip and on decode_kmp.hip up to 32 rows AT HIDDEN 256: the fp8 tiles need K in whole 64-element
    steps per wave (K % 512; decode_kmp.hip: K >= 512), so batches 1-8 fall back to decode_mfma.hip and 9-32 rows are REFUSED (asserted with
    the error text); the 33-64 row form (four-way K split) takes them.  The fp8 o-proj (K = q_dim) and down (phased) run on both.  Model H
    (hidden 512) covers those cells.
"""

import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import decode_stage_ref as R
from test_ops_gpu import assert_elementwise, relerr

pytestmark = pytest.mark.gpu

from decode_stage_ref import CASES, DOWN, GATEUP, GEMV, GEMV_FP8, KM, KMP, KS, LMHEAD, MFMA, OPROJ, QKV, REFUSED, VIA_NAME

# ---- engines ---------------------------------------------------------------------------------------------------------------------------
class Eng:
    """one model + session and the float64 weights its references read"""

    def __init__(self, device, model, fp8=False, exact=False, kv_fp8=False, max_batch=8, sd=None, km0_aux=False):
        from emmax import _lib
        from emmax.engine import EmmaxEngine

        self.L, self.lib = _lib, _lib.load()
        self.model, self.fp8, self.exact, self.kv_fp8 = model, fp8, exact, kv_fp8
        self.cfg = R.make_cfg(model, fp8)
        self.sd = sd if sd is not None else R.make_state_dict(model)
        self.W = R.Weights(self.sd, self.cfg, fp8)
        with (_lib.tuning(kv_fp8=1) if kv_fp8 else contextlib.nullcontext()):
            self.eng = EmmaxEngine(self.cfg, dict(self.sd), device=device, max_batch=max_batch, max_prompt=R.MAX_PROMPT, max_ctx=R.MAX_CTX, exact=exact)
        with (_lib.tuning(km=0) if km0_aux else contextlib.nullcontext()):   # km = 0 at build time: decode_mfma.hip's qkv / gate-up copies as well
            self.eng.ensure_decode_batch(max_batch)
        self.device = device
        self.rows = min(max_batch, 64)
        self.Hq, self.Hkv, self.hidden = R.MODELS[model]
        self.q_dim = self.Hq * R.HEAD_DIM
        self.max_pages = (R.MAX_CTX + R.PAGE - 1) // R.PAGE
        self.eng.kv.random_(0, 256)   # neighbours of an appended row hold something a stray store would change
        torch.cuda.synchronize()

    def hidden_rows(self, seed, scale=1.0):
        return R.hidden_rows(self.rows, seed, scale, self.hidden)

    @property
    def act_dtype(self):
        return torch.float32 if self.exact else torch.bfloat16

    def oproj_form(self, B):
        form, ns, via = C.c_int(-1), C.c_int(0), C.c_int(0)
        self.L.check(self.lib.emmax_op_decode_stage(self.eng._session, 0, OPROJ, B, None, None, None, None, None, None, None, None, None, C.byref(via),
                                                    C.byref(form), C.byref(ns), self.L.current_stream()), "oproj form")
        return form.value, ns.value

    def run(self, stage, B, layer=0, h32=None, h=None, ctx=None, pages=None, x=None):
        """-> dict(h, h32 [rows], y, tok, via); raises EmmaxError with the library's message on a refusal (via is kept in self.last_via)"""
        dev = self.device
        h32_d = h32.to(dev).contiguous() if h32 is not None else torch.zeros(self.rows, self.hidden, device=dev)
        h_d = (h if h is not None else R.bf(h32)).to(dev).contiguous()
        assert h_d.shape == (self.rows, self.hidden) and h32_d.shape == (self.rows, self.hidden)
        h_out, h32_out = torch.empty_like(h_d), torch.empty_like(h32_d)
        y = tok = None
        if stage == QKV:
            y = torch.full((B, self.q_dim), float("nan"), dtype=self.act_dtype, device=dev)
        elif stage == GATEUP:
            y = torch.full((B, R.INTER_P), float("nan"), dtype=self.act_dtype, device=dev)
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
        want = self.route(stage, B)   # the host-only route query: the same family, or the same refusal, as what really launches below
        rc = self.lib.emmax_op_decode_stage(self.eng._session, layer, stage, B, h_d.data_ptr(), h32_d.data_ptr(), ctx_c, pt_c, self.L.ptr(x_d),
                                            h_out.data_ptr(), h32_out.data_ptr(), self.L.ptr(y), self.L.ptr(tok), C.byref(via), None, None,
                                            self.L.current_stream())
        self.last_via = via.value
        self.last_route = want
        assert rc != 0 or via.value == want, f"stage {stage}, B {B}: ran on {VIA_NAME[via.value]}, the route says {VIA_NAME[want]}"
        self.L.check(rc, f"emmax_op_decode_stage(stage {stage}, B {B})")
        torch.cuda.synchronize()
        return {"h": h_out.cpu(), "h32": h32_out.cpu(), "y": None if y is None else y.cpu(), "tok": None if tok is None else tok.cpu(), "via": via.value}

    def route(self, stage, B):
        via = C.c_int(0)
        rc = self.lib.emmax_op_decode_route(self.eng._model, stage, B, int(self.exact), C.byref(via))
        return via.value if rc == 0 else REFUSED

    def kv_read(self, layer, row, p0, n, page_row=None, from_stage=False):
        nn = 1 if from_stage else n
        k = np.empty((nn, self.Hkv, R.HEAD_DIM), dtype=np.float32)
        v = np.empty_like(k)
        pr = (C.c_int32 * self.max_pages)(*page_row.tolist()) if page_row is not None else None
        self.L.check(self.lib.emmax_op_decode_kv_read(self.eng._session, layer, row, p0, n, pr, int(from_stage), k.ctypes.data_as(C.POINTER(C.c_float)),
                                                      v.ctypes.data_as(C.POINTER(C.c_float)), self.L.current_stream()), "emmax_op_decode_kv_read")
        return k, v

    def kv_token_rows(self, raw):
        """bool-comparable view [layers][K / V][pages][kv heads][64 tokens][bytes of a token row] of the raw paged region (bf16 and 24-bit
        formats: include/emmax.h gives the layouts)"""
        n_pages = self.rows * self.max_pages
        n = n_pages * self.Hkv * R.PAGE
        eb = 3 if self.exact else 2
        per = raw.view(R.LAYERS, 2, n * R.HEAD_DIM * eb)
        main = per[..., : n * R.HEAD_DIM * 2].reshape(R.LAYERS, 2, n_pages, self.Hkv, R.PAGE, R.HEAD_DIM * 2)
        if not self.exact:
            return main
        ext = per[..., n * R.HEAD_DIM * 2:].reshape(R.LAYERS, 2, n_pages, self.Hkv, R.PAGE, R.HEAD_DIM)
        return torch.cat([main, ext], dim=-1)


@pytest.fixture(scope="module")
def engines(device):
    """engines by name, built on first use and kept for the module"""
    made = {}
    spec = {
        "G": dict(model="G", max_batch=8, km0_aux=True),
        "W": dict(model="W", max_batch=64),
        "G8": dict(model="G", fp8=True, max_batch=8),
        "W8": dict(model="W", fp8=True, max_batch=64),
        "GX": dict(model="G", exact=True, max_batch=8),
        "Gkv8": dict(model="G", kv_fp8=True, max_batch=8),
        "H8": dict(model="H", fp8=True, max_batch=32),
    }

    def get(name):
        if name not in made:
            made[name] = Eng(device, **spec[name])
        return made[name]

    yield get
    for e in made.values():
        e.eng.close()


def operand_form(e, via, resid32):
    """which documented rounding form the launcher's norm prologue has (decode_stage_ref.py)"""
    if e.exact:
        return "exact"
    if via == KS:
        return "f32" if resid32 else "mirror"
    return "mirror" if via in (KM, KMP) else "hf"


def check(got, ref, form, out, what):
    rtol, atol, tol = R.tolerances(form, out)
    err = relerr(got, ref)
    print(f"{what}: relerr {err:.3e} (bound {tol:.3e}), atol_frac {atol:.3e}")
    assert err < tol, f"{what}: relerr {err:.3e} >= {tol:.3e}"
    assert_elementwise(got, ref, rtol=rtol, atol_frac=atol, what=what)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def setup_case(engines, tune, eng, B, sw):
    e = engines(eng)
    if sw:
        tune(**sw)
    return e, e.L.tuning_get("resid32") != 0 or e.exact


def expect_refusal(e, fn):
    with pytest.raises(e.L.EmmaxError) as ei:
        fn()
    msg = str(ei.value)
    assert "launch_proj" in msg and "failed (-1)" in msg, msg   # decode_mfma.hip stages at most 8 rows: nothing is left to serve the shape
    assert e.last_route == REFUSED, f"the launch was refused, the route says {VIA_NAME[e.last_route]}"


# ---- QKV: norm prologue, RoPE, the K / V append ---------------------------------------------------------------------------------------------
def _qkv_once(e, B, li, want_via, resid32, pages, kv8=False):
    h32, h = e.hidden_rows((B, li))
    x = (h32 if resid32 else h.float())[:B]
    ctx = R.ctx_rows(B, li)
    pt = pages if pages is not None else torch.arange(B * e.max_pages, dtype=torch.int32).view(B, e.max_pages)
    e.eng.kv.random_(0, 256)   # fresh bytes: an earlier case may have appended the very same rows at the very same place (then nothing would change)
    win = []
    for b in range(B):   # the window ctx - 1 .. ctx + 1 of every row, before the launch
        p0 = max(ctx[b] - 1, 0)
        win.append((p0, e.kv_read(li, b, p0, ctx[b] + 2 - p0, pt[b])))
    before = e.eng.kv.clone()
    out = e.run(QKV, B, li, h32=h32, h=h, ctx=ctx, pages=pages)
    assert out["via"] == want_via, f"qkv ran on {VIA_NAME[out['via']]}, expected {VIA_NAME[want_via]}"
    form = operand_form(e, out["via"], resid32)
    q_ref, k_ref, v_ref = R.ref_qkv(e.W, li, x, ctx)
    check(out["y"], q_ref, form, "q", f"q rows (layer {li})")
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
        for j in range(k1.shape[0]):   # the neighbours (across a page boundary at 63 / 64 / 127 / 128): bit-unchanged
            if j != at:
                assert np.array_equal(k0[j].view(np.int32), k1[j].view(np.int32)) and np.array_equal(v0[j].view(np.int32), v1[j].view(np.int32)), \
                    f"row {b}: position {p0 + j} changed by the append at {ctx[b]}"
    check(torch.from_numpy(np.stack(k_new)), k_ref, form, "k", f"K rows (layer {li})")
    check(torch.from_numpy(np.stack(v_new)), v_ref, form, "v", f"V rows (layer {li})")
    after = e.eng.kv
    if kv8:   # the rows wait in kv_stage for the attention launch: the cache itself is untouched
        assert torch.equal(before, after), "fp8 KV cache: the qkv launch wrote into the cache"
        return
    # nothing but (layer, K and V, the row's page of position ctx, every kv head, token ctx % 64) changed -- no other row, no other layer
    changed = (e.kv_token_rows(before) != e.kv_token_rows(after)).any(-1).cpu()
    want = torch.zeros_like(changed)
    for b in range(B):
        want[li, :, int(pt[b][ctx[b] // R.PAGE]), :, ctx[b] % R.PAGE] = True
    assert torch.equal(changed, want), f"K / V token rows changed: {changed.nonzero().tolist()[:8]} ..., expected {want.nonzero().tolist()[:8]} ..."


@pytest.mark.parametrize("eng,B,sw,via", CASES)
def test_qkv_rope_and_kv_append(engines, tune, eng, B, sw, via):
    """q rows, the rotated K row and the V row at position ctx_len[b] of row b's pages (contexts 0, 1, 63, 64, 65, 127, 128, max_ctx - 2 mixed
    in one batch), once on the identity page table and once on a shuffled one; the positions before and after, every other row and the other
    layer bit-unchanged.  Layer 1 as well as layer 0: the per-layer cache offset."""
    e, resid32 = setup_case(engines, tune, eng, B, sw)
    if via[QKV] == REFUSED:
        h32, h = e.hidden_rows((B, 0))
        expect_refusal(e, lambda: e.run(QKV, B, 0, h32=h32, h=h, ctx=R.ctx_rows(B)))
        return
    for li in range(R.LAYERS):
        _qkv_once(e, B, li, via[QKV], resid32, None)
        _qkv_once(e, B, li, via[QKV], resid32, R.shuffled_pages(B, e.max_pages, (B, li)))


@pytest.mark.parametrize("B", [1, 3, 8])
def test_qkv_with_fp8_kv_cache_writes_the_staging_rows(engines, B):
    """kv_fp8 session: the new K / V rows land in kv_stage (bf16, for the attention launch to quantise), the cache stays untouched"""
    e = engines("Gkv8")
    for li in range(R.LAYERS):
        _qkv_once(e, B, li, KS if B < 3 else KM, True, R.shuffled_pages(B, e.max_pages, (B, li, 1)), kv8=True)


def test_qkv_refuses_positions_and_page_tables_outside_the_rows(engines):
    """the op validates on the host, before anything is launched: no test can hand a kernel an out-of-range position or page"""
    e = engines("G")
    h32, h = e.hidden_rows(1)
    before = e.eng.kv.clone()
    for bad in ([R.MAX_CTX - 1, 0], [0, -1], [1 << 20, 0]):
        with pytest.raises(e.L.EmmaxError, match="ctx_len"):
            e.run(QKV, 2, 0, h32=h32, h=h, ctx=bad)
    pt = torch.arange(2 * e.max_pages, dtype=torch.int32).view(2, e.max_pages)
    for edit in ((0, 0, 2 * e.max_pages), (1, 1, 0), (0, 2, -1)):   # a page of another row, a page twice, a negative page
        p = pt.clone()
        p[edit[0], edit[1]] = edit[2]
        with pytest.raises(e.L.EmmaxError, match="permutation"):
            e.run(QKV, 2, 0, h32=h32, h=h, ctx=[0, 1], pages=p)
    assert torch.equal(before, e.eng.kv)
    # ... and a shuffled launch leaves the identity table behind: the same launch without a table writes row b's own pages again
    e.run(QKV, 2, 0, h32=h32, h=h, ctx=[5, 70], pages=R.shuffled_pages(2, e.max_pages, 7))
    mid = e.eng.kv.clone()
    h32b, hb = e.hidden_rows(2)   # other values: a launch through a table left shuffled would show in the shuffled pages
    e.run(QKV, 2, 0, h32=h32b, h=hb, ctx=[5, 70])
    changed = (e.kv_token_rows(mid) != e.kv_token_rows(e.eng.kv)).any(-1).cpu().nonzero()
    assert set(int(p) for p in changed[:, 2]) == {0, e.max_pages + 1}, changed.tolist()[:8]


# ---- O-PROJ / DOWN: the residual add into the fp32 stream and its bf16 mirror -----------------------------------------------------------------
def _resid_once(e, stage, B, li, want_via, resid32):
    out_name = "down"
    if stage == OPROJ:
        form_in, ns = e.oproj_form(B)
        if form_in == 1:   # split partials: unequal maxima, one empty split -- the reference is the float64 merge
            x = R.attn_partials(B, e.Hq, ns, (B, li))
            assert ns > 1 and torch.isinf(x[:, :, 1, 128]).all()
            wx = R.ref_oproj(e.W, li, R.ref_merge(x))
            out_name = "oproj_split"
        else:
            x = R.attn_rows32(B, e.q_dim, (B, li)) if form_in == 2 else R.attn_rows(B, e.q_dim, (B, li))
            assert (form_in == 2) == e.exact
            wx = R.ref_oproj(e.W, li, x)
            out_name = "oproj"
    else:
        x = R.act_rows32(B, R.INTER_P, (B, li)) if e.exact else R.act_rows(B, R.INTER_P, (B, li))
        wx = R.ref_down(e.W, li, x)
    rms = wx.pow(2).mean().sqrt().item()
    # the fp32 stream: not bf16-representable and ~30 x the size of W x -- a kernel adding into the bf16 mirror instead loses W x in its rounding
    h32, h = e.hidden_rows((B, li, stage), scale=(30.0 if resid32 else 1.0) * rms)
    assert not torch.equal(h32, h.float())
    res = e.run(stage, B, li, h32=h32, h=h, x=x)
    assert res["via"] == want_via, f"stage {stage} ran on {VIA_NAME[res['via']]}, expected {VIA_NAME[want_via]}"
    form = operand_form(e, res["via"], resid32)
    what = f"{'o-proj' if stage == OPROJ else 'down'} (layer {li}, B {B})"
    if resid32:
        check(res["h32"][:B].double() - h32[:B].double(), wx, form, out_name, what + ": h32_out - h32_in against W x")
        assert torch.equal(bits(res["h"][:B]), bits(R.bf(res["h32"][:B]))), what + ": the bf16 mirror is not bf16(h32_out)"
    else:   # bf16 rows only: the mirror IS the stream, one more output rounding (inside rtol)
        check(res["h"][:B].double(), h[:B].double() + wx, form, out_name, what + ": dh_out against bf16(dh_in + W x)")
        assert torch.equal(bits(res["h32"]), bits(h32)), what + ": resid32 = 0 wrote the fp32 stream"
    assert torch.equal(bits(res["h"][B:]), bits(h[B:])) and torch.equal(bits(res["h32"][B:]), bits(h32[B:])), what + f": rows {B}.. changed"
    if B > 32:
        assert torch.isfinite(res["h32"][32:B]).all() and not torch.equal(res["h32"][32:B], h32[32:B]), what + ": rows 32.. not written"


@pytest.mark.parametrize("eng,B,sw,via", CASES)
def test_oproj_residual_and_split_merge(engines, tune, eng, B, sw, via):
    e, resid32 = setup_case(engines, tune, eng, B, sw)
    for li in range(R.LAYERS):
        _resid_once(e, OPROJ, B, li, via[OPROJ], resid32)


@pytest.mark.parametrize("eng,B,sw,via", CASES)
def test_down_residual_phased_kernels(engines, tune, eng, B, sw, via):
    e, resid32 = setup_case(engines, tune, eng, B, sw)
    for li in range(R.LAYERS):
        _resid_once(e, DOWN, B, li, via[DOWN], resid32)


# ---- GATE/UP: SwiGLU over the interleaved rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eng,B,sw,via", CASES)
def test_gateup_swiglu(engines, tune, eng, B, sw, via):
    """silu(g) * u for every one of the 4160 columns (inter_p = inter here: no padding columns), from gate_proj / up_proj by their HF names"""
    e, resid32 = setup_case(engines, tune, eng, B, sw)
    assert R.INTER_P == R.INTER
    for li in range(R.LAYERS):
        h32, h = e.hidden_rows((B, li, 3))
        if via[GATEUP] == REFUSED:
            expect_refusal(e, lambda: e.run(GATEUP, B, li, h32=h32, h=h))
            continue
        res = e.run(GATEUP, B, li, h32=h32, h=h)
        assert res["via"] == via[GATEUP], f"gate/up ran on {VIA_NAME[res['via']]}, expected {VIA_NAME[via[GATEUP]]}"
        ref = R.ref_gateup(e.W, li, (h32 if resid32 else h.float())[:B])
        check(res["y"], ref, operand_form(e, res["via"], resid32), "gateup", f"gate/up (layer {li}, B {B})")
        assert torch.equal(bits(res["h"]), bits(h)) and torch.equal(bits(res["h32"]), bits(h32)), "gate/up changed the hidden rows"


# ---- LM-HEAD: logit rows, argmax partials, the greedy finish ------------------------------------------------------------------------------------
def _lmhead_tokens_ok(e, res, ref, form, B):
    rtol, atol, _ = R.tolerances(form, "lmhead")
    tok = res["tok"].tolist()
    checked = 0
    for b in range(B):
        assert 0 <= tok[b] < R.VOCAB, f"row {b}: token {tok[b]} outside the vocabulary"
        top = torch.topk(ref[b], 2)
        tol = atol * ref[b].pow(2).mean().sqrt().item() + rtol * top.values[0].abs().item()
        if (top.values[0] - top.values[1]).item() > 2.0 * tol:   # a priori: twice the logit tolerance
            assert tok[b] == int(top.indices[0]), f"row {b}: token {tok[b]}, reference argmax {int(top.indices[0])}"
            checked += 1
        assert tok[b] == int(res["y"][b].argmax()), f"row {b}: the finish picked {tok[b]}, the logit row's own argmax is {int(res['y'][b].argmax())}"
    return checked


@pytest.mark.parametrize("eng,B,sw,via", CASES)
def test_lmhead_logits_and_greedy_token(engines, tune, eng, B, sw, via):
    """all 32064 logits of every row, and the token the greedy finish picks from the launch's argmax partials"""
    e, resid32 = setup_case(engines, tune, eng, B, sw)
    h32, h = e.hidden_rows((B, 99))
    if via[LMHEAD] == REFUSED:
        expect_refusal(e, lambda: e.run(LMHEAD, B, h32=h32, h=h))
        return
    res = e.run(LMHEAD, B, h32=h32, h=h)
    assert res["via"] == via[LMHEAD], f"lm-head ran on {VIA_NAME[res['via']]}, expected {VIA_NAME[via[LMHEAD]]}"
    form = operand_form(e, res["via"], resid32)
    if B == 33:
        form = "mirror"   # rows 0 .. 31 ran on decode_kmp.hip (the wider form), row 32 on decode_ks.hip
    ref = R.ref_lmhead(e.W, (h32 if resid32 else h.float())[:B])
    check(res["y"], ref, form, "lmhead", f"lm-head logits (B {B})")
    _lmhead_tokens_ok(e, res, ref, form, B)
    assert torch.equal(bits(res["h"]), bits(h)) and torch.equal(bits(res["h32"]), bits(h32)), "lm-head changed the hidden rows"


def _crafted_sd(kind):
    """model W with a modified lm_head and final norm.  `negative`: every lm_head entry <= 0 and the norm weight positive, so that positive
    hidden rows give strictly negative logits everywhere (a zero-padded row past the vocabulary would win an unguarded argmax); row NEG_BEST
    is the least negative by a wide margin.  `tie`: rows TIE_I < TIE_J identical and the global maximum."""
    sd = dict(R.make_state_dict("W"))
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


NEG_BEST = 31999
TIE_I, TIE_J = 1029, 30003   # tiles 64 / 1875: different tiles, different blocks of every launcher's grid, i < j


@pytest.fixture(scope="module")
def crafted(device):
    made = {}

    def get(kind, fp8):
        if (kind, fp8) not in made:
            made[(kind, fp8)] = Eng(device, "W", fp8=fp8, max_batch=64, sd=_crafted_sd(kind))
        return made[(kind, fp8)]

    yield get
    for e in made.values():
        e.eng.close()


CRAFT_CASES = [
    pytest.param(False, 1, {}, KS, id="ks-B1"), pytest.param(False, 2, {"ks": 0}, GEMV, id="gemv-B2"),
    pytest.param(False, 3, {}, KM, id="km-B3"), pytest.param(False, 16, {}, KM, id="km-B16"),
    pytest.param(False, 17, {}, KMP, id="kmp-B17"), pytest.param(False, 33, {}, KS, id="kmp32-ks1-B33"), pytest.param(False, 64, {}, KMP, id="kmp-B64"),
    pytest.param(True, 1, {}, GEMV_FP8, id="gemv_fp8-B1"), pytest.param(True, 2, {}, MFMA, id="fp8-mfma-B2"), pytest.param(True, 8, {}, MFMA, id="fp8-mfma-B8"),
]


@pytest.mark.parametrize("fp8,B,sw,via", CRAFT_CASES)
@pytest.mark.parametrize("kind", ["negative", "tie"])
def test_lmhead_argmax_edge_cases(crafted, tune, kind, fp8, B, sw, via):
    """1. every logit strictly negative: the token must be inside the vocabulary and the reference's (the zero rows that pad the vocabulary to
    the tile would win otherwise).  2. two identical lm_head rows i < j hold the global maximum: the lower id wins, across tiles, blocks and
    (above 32 rows) the two launches."""
    e = crafted(kind, fp8)
    if sw:
        tune(**sw)
    h32 = torch.rand(e.rows, e.hidden, generator=R.gen(41, B)) + 0.1   # all positive: with the positive norm weight, so is the normalised row
    res = e.run(LMHEAD, B, h32=h32.float())
    assert res["via"] == via, f"lm-head ran on {VIA_NAME[res['via']]}, expected {VIA_NAME[via]}"
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


def test_model_w_decodes_sixty_four_rows(engines):
    e = engines("W")
    assert e.lib.emmax_model_max_decode_batch(e.eng._model) == 64
    assert e.oproj_form(9) == (0, 1) and e.oproj_form(64) == (0, 1)     # one split: the o-proj reads bf16 rows
    g = engines("G")
    assert g.oproj_form(1)[0] == 1 and g.oproj_form(8)[0] == 1           # GQA, 2 kv heads: split partials at every batch
