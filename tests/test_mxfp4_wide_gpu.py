"""MXFP4 decode weights at 17-64 rows on the GPU (tuning switch mx4_wide, frozen into the model at emmax_model_create; decode_kmp.hip's MX4 form).

  1. the widening, element by element, through the kmp kernel itself (emmax_op_gemm_wide_mxfp4): tests/test_mxfp4_gpu.py's one-hot construction at
     B = 32 and 17, on K = 1024 / 4096 (one and four phases per wave), 4224 and 11008 (the eleven-phase form, waves of unequal slices), the blocks
     planted on every wave's last load step and on the first one past a short wave's slice;
  2. every fused stage through the step's own dispatch (emmax_op_decode_stage) against the float64 reference on the de-quantised weights, with the
     checks of tests/test_mxfp4_gpu.py and the tolerance table of tests/mxfp4_wide_ref.py (reference against reference, measured on the CPU), the
     launcher family asserted per launch: model W4 at 17, 32, 33, 40 and 64 rows, model T4 (hidden 4096: the many-tile rings) at 32 and 64;
  3. end to end on the W4 shape with the tiny towers: planted ids of a ragged batch of 24, 16 teacher-forced random-weight steps at 40 rows (eager and
     hipGraph replay, bit-equal), 24 request slots serving 40 ragged requests, and a narrow engine in the same process that still refuses 17 rows.
Every test here fails without the feature: the model limit is 16, the session is refused, the op does not exist.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import decode_stage_ref as R
import mxfp4_ref as M
import mxfp4_wide_ref as W
from test_mxfp4_gpu import E2E_TOL, Eng4, VIA_NAME, _crafted_sd, _teacher_forced, bits, NEG_BEST, TIE_I, TIE_J
from test_ops_gpu import assert_elementwise, relerr

pytestmark = pytest.mark.gpu

QKV, OPROJ, GATEUP, DOWN, LMHEAD = 0, 2, 3, 4, 5
KM, KMP = 4, 5


def check(got, ref, out, what):
    rtol, atol, tol = W.tolerances(out)
    err = relerr(got, ref)
    print(f"{what}: relerr {err:.3e} (bound {tol:.3e}), atol_frac {atol:.3e}")
    assert err < tol, f"{what}: relerr {err:.3e} >= {tol:.3e}"
    assert_elementwise(got, ref, rtol=rtol, atol_frac=atol, what=what)


# ---- 1. the widening through the kmp kernel -------------------------------------------------------------------------------------------------
def _planted_steps(K):
    """load steps (128 k) that carry a block: every wave's LAST step, the first step past the slice of a wave that is one short, then the waves'
    first steps -- decode_kmp.hip's split of K / 128 steps over eight waves, restated"""
    KT = K // 128
    kq, kr = divmod(KT, 8)
    lo = [w * kq + min(w, kr) for w in range(8)]
    n = [kq + (1 if w < kr else 0) for w in range(8)]
    last = [lo[w] + n[w] - 1 for w in range(8)]
    past = [lo[w] + n[w] for w in range(8) if kr and n[w] == kq and lo[w] + n[w] < KT]
    steps = []
    for s in last + past + lo:
        if s not in steps:
            steps.append(s)
    return steps[:16], n


@pytest.mark.parametrize("K", [1024, 4096, 4224, 11008])
@pytest.mark.parametrize("B", [32, 17])
def test_hardware_widening_through_the_wide_kernel(device, B, K):
    """Row r of a 32 x K matrix holds ONE non-zero block (the hand-written blocks, scale code 0, scale code 252) and batch row b is one-hot at
    element off + b of every block, so y[b, r] is exactly one de-quantised element: bit equality with the torch reference, 0 accepted only where
    the weight is a bf16 denormal.  A phase, tile or scale index off by one moves a block's element or its scale: a wrong element, not a
    tolerance miss.  B = 17: rows 17-31 of the second batch tile are not there -- nothing of them may reach an output."""
    from emmax import _lib

    lib = _lib.load()
    N = 32
    t = 2.0 ** -127
    blocks = [(n, b.double()) for n, b, _ in M.adversarial_blocks()]
    code0 = torch.zeros(32, dtype=torch.float64)
    code0[:8] = torch.tensor([6 * t, -4 * t, 3 * t, 2 * t, 1.5 * t, -1 * t, 0.5 * t, 5 * t])
    top = torch.zeros(32, dtype=torch.float64)
    top[:6] = torch.tensor([1.5 * 2.0 ** 127, -(2.0 ** 127), 2.0 ** 126, 3 * 2.0 ** 125, -(2.0 ** 124), 2.0 ** 120])
    blocks += [("code-0", code0), ("code-252", top)]
    steps, per_wave = _planted_steps(K)
    assert len(steps) in (8, 16)
    if K == 4224:
        assert per_wave == [5, 4, 4, 4, 4, 4, 4, 4]
    if K == 11008:
        assert per_wave == [11] * 6 + [10] * 2
    W_ = torch.zeros(N, K, dtype=torch.float64)
    sx = torch.ones(K // 32, dtype=torch.float64)
    where = []
    for r in range(N):
        name, blk = blocks[r % len(blocks)]
        kb = steps[r % len(steps)] * 4 + (r + r // len(steps)) % 4       # the row's K block: all four scale bytes of a step are used
        assert kb not in [w[1] for w in where]
        where.append((name, kb))
        amax = blk.abs().max().item()
        W_[r, kb * 32:(kb + 1) * 32] = blk
        sx[kb] = 2.0 ** 64 if 0 < amax < 2.0 ** -100 else 2.0 ** -64 if amax > 2.0 ** 100 else 1.0
    Wb = W_.to(torch.bfloat16)
    assert torch.equal(Wb.double(), W_)
    want_w = M.quant_dequant(Wb)
    src = Wb.to(device)
    tiles = torch.empty(N * K // 2, dtype=torch.uint8, device=device)
    scales = torch.empty(N * K // 32, dtype=torch.uint8, device=device)
    st = _lib.current_stream()
    _lib.check(lib.emmax_op_quant_mxfp4(src.data_ptr(), K, tiles.data_ptr(), scales.data_ptr(), N, K, 0, 0, st), "emmax_op_quant_mxfp4")
    flushed = 0
    for off in ((0,) if B == 32 else (0, 15)):
        x = torch.zeros(B, K, dtype=torch.float64)
        for b in range(B):
            x[b, off + b::32] = sx
        xb = x.to(torch.bfloat16)
        assert torch.equal(xb.double(), x)
        y = torch.full((B, N), float("nan"), dtype=torch.bfloat16, device=device)
        xd = xb.to(device)
        _lib.check(lib.emmax_op_gemm_wide_mxfp4(xd.data_ptr(), tiles.data_ptr(), scales.data_ptr(), y.data_ptr(), B, N, K, st), "emmax_op_gemm_wide_mxfp4")
        torch.cuda.synchronize()
        got = y.cpu()
        for r, (name, kb) in enumerate(where):
            for b in range(B):
                w = want_w[r, kb * 32 + off + b].item()
                want = torch.tensor(w * sx[kb].item(), dtype=torch.float64).to(torch.bfloat16)
                assert float(want) == w * sx[kb].item()                                   # the expectation is exact in bf16
                g = got[b, r]
                ok = bits(g.reshape(1)).item() == bits(want.reshape(1)).item() or (float(g) == 0.0 and float(want) == 0.0)
                if not ok and 0 < abs(w) < 2.0 ** -126 and float(g) == 0.0:
                    flushed += 1
                    ok = True
                assert ok, f"row {r} block {name} at K block {kb} (step {kb // 4}), element {off + b}: got {float(g)!r}, de-quantised weight {w!r} x {sx[kb].item()!r} = {float(want)!r}"
    print(f"K {K} B {B}: steps {steps}, bf16-denormal weight elements that reached the output as 0: {flushed}")


def test_wide_op_refusals_launch_nothing(device):
    from emmax import _lib

    lib = _lib.load()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
    y = torch.full((64, 64), float("nan"), dtype=torch.bfloat16, device=device)
    before = bits(y).clone()
    for B, N, K in ((16, 32, 1024), (33, 32, 1024), (32, 32, 1000), (32, 32, 12288), (32, 24, 1024), (32, 32, 896), (32, 8192, 4224)):
        assert lib.emmax_op_gemm_wide_mxfp4(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), y.data_ptr(), B, N, K, _lib.current_stream()) == -1, (B, N, K)
        assert b"emmax_op_gemm_wide_mxfp4" in lib.emmax_last_error()
    assert lib.emmax_op_gemm_wide_mxfp4(None, buf.data_ptr(), buf.data_ptr(), y.data_ptr(), 32, 32, 1024, _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(bits(y), before) and int(buf.max()) == 0


# ---- 2. the fused stages ----------------------------------------------------------------------------------------------------------------------
class EngW(Eng4):
    """one WIDE MXFP4 model + session of ROWS rows, and the float64 de-quantised weights its references read"""

    def __init__(self, device, model, max_batch=W.ROWS, sd=None):
        from emmax import _lib
        from emmax.engine import EmmaxEngine

        self.L, self.lib = _lib, _lib.load()
        self.model, self.kv_fp8 = model, False
        self.dims = W.MODELS[model]
        self.cfg = W.make_cfg(model)
        self.sd = sd if sd is not None else W.make_state_dict(model)
        self.W = W.WeightsW(self.sd, self.cfg)
        assert _lib.tuning_get("mx4_wide") == 0
        self.eng = EmmaxEngine(self.cfg, dict(self.sd), device=device, max_batch=max_batch, max_prompt=R.MAX_PROMPT, max_ctx=R.MAX_CTX, mxfp4_wide=True)
        assert _lib.tuning_get("mx4_wide") == 0 and self.eng.mxfp4_wide and self.eng.max_decode_batch() == 64
        self.eng.ensure_decode_batch(max_batch)
        assert int(self.lib.emmax_model_aux_bytes(self.eng._model)) == 0
        self.device, self.rows = device, max_batch
        self.Hq, self.Hkv = self.dims["heads"]
        self.hidden, self.q_dim = self.dims["hidden"], self.Hq * R.HEAD_DIM
        self.max_pages = (R.MAX_CTX + R.PAGE - 1) // R.PAGE
        self.eng.kv.random_(0, 256)
        torch.cuda.synchronize()

    def hidden_rows(self, seed, scale=1.0):
        h32, h = R.hidden_rows(self.rows, seed, scale, self.hidden)
        return h32, h

    @staticmethod
    def want_via(stage, B):
        """the family of the stage's LAST launch: down and lm-head run in chunks of 32 rows, and a tail of 1-16 rows is a decode_km.hip launch"""
        tail = B if stage not in (DOWN, LMHEAD) or B <= 32 else B - 32
        return KMP if tail > 16 else KM

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
            y = torch.full((B, self.dims["inter"]), float("nan"), dtype=torch.bfloat16, device=dev)
        elif stage == LMHEAD:
            y = torch.full((B, self.dims["vocab"]), float("nan"), dtype=torch.float32, device=dev)
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
        want = self.want_via(stage, B)
        assert via.value == want, f"stage {stage} at B {B}: the last launch ran on {VIA_NAME.get(via.value, via.value)}, expected {VIA_NAME[want]}"
        return {"h": h_out.cpu(), "h32": h32_out.cpu(), "y": None if y is None else y.cpu(), "tok": None if tok is None else tok.cpu()}

    def kv_token_rows(self, raw):
        n_pages = self.rows * self.max_pages
        return raw.view(self.dims["layers"], 2, n_pages, self.Hkv, R.PAGE, R.HEAD_DIM * 2)


@pytest.fixture(scope="module")
def engines(device):
    made = {}

    def get(name):
        if name not in made:
            made[name] = EngW(device, name)
        return made[name]

    yield get
    for e in made.values():
        e.eng.close()


def _qkv_once(e, B, li, pages):
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
    check(out["y"], q_ref, "q", f"q rows (layer {li}, B {B})")
    assert torch.equal(bits(out["h"]), bits(h)) and torch.equal(bits(out["h32"]), bits(h32)), "qkv changed the hidden rows"
    k_new, v_new = [], []
    for b in range(B):
        p0, (k0, v0) = win[b]
        k1, v1 = e.kv_read(li, b, p0, ctx[b] + 2 - p0, pt[b])
        at = ctx[b] - p0
        k_new.append(k1[at]); v_new.append(v1[at])
        for j in range(k1.shape[0]):
            if j != at:
                assert np.array_equal(k0[j].view(np.int32), k1[j].view(np.int32)) and np.array_equal(v0[j].view(np.int32), v1[j].view(np.int32)), \
                    f"row {b}: position {p0 + j} changed by the append at {ctx[b]}"
    check(torch.from_numpy(np.stack(k_new)), k_ref, "k", f"K rows (layer {li}, B {B})")
    check(torch.from_numpy(np.stack(v_new)), v_ref, "v", f"V rows (layer {li}, B {B})")
    changed = (e.kv_token_rows(before) != e.kv_token_rows(e.eng.kv)).any(-1).cpu()
    want = torch.zeros_like(changed)
    for b in range(B):
        want[li, :, int(pt[b][ctx[b] // R.PAGE]), :, ctx[b] % R.PAGE] = True
    assert torch.equal(changed, want), f"K / V token rows changed: {changed.nonzero().tolist()[:8]} ..., expected {want.nonzero().tolist()[:8]} ..."


def _resid_once(e, stage, B, li):
    if stage == OPROJ:
        assert e.oproj_form(B) == (0, 1)                  # one split: the bf16 attention rows
        x = W.attn_rows(e.model, (B, li))[:B]
        wx, out_name = R.ref_oproj(e.W, li, x), "oproj"
    else:
        x = W.act_rows(e.model, (B, li))[:B]
        wx, out_name = M.ref_down4(e.W, li, x), "down"
    rms = wx.pow(2).mean().sqrt().item()
    # the fp32 stream: not bf16-representable and ~30 x the size of W x -- a kernel adding into the bf16 mirror instead loses W x in its rounding
    h32, h = e.hidden_rows((B, li, stage), scale=30.0 * rms)
    assert not torch.equal(h32, h.float())
    res = e.run(stage, B, li, h32=h32, h=h, x=x)
    what = f"{'o-proj' if stage == OPROJ else 'down'} (layer {li}, B {B})"
    check(res["h32"][:B].double() - h32[:B].double(), wx, out_name, what + ": h32_out - h32_in against W x")
    assert torch.equal(bits(res["h"][:B]), bits(R.bf(res["h32"][:B]))), what + ": the bf16 mirror is not bf16(h32_out)"
    assert torch.equal(bits(res["h"][B:]), bits(h[B:])) and torch.equal(bits(res["h32"][B:]), bits(h32[B:])), what + f": rows {B}.. changed"


def _gateup_once(e, B, li):
    h32, h = e.hidden_rows((B, li, 3))
    res = e.run(GATEUP, B, li, h32=h32, h=h)
    check(res["y"], R.ref_gateup(e.W, li, h32[:B]), "gateup", f"gate/up (layer {li}, B {B})")
    assert torch.equal(bits(res["h"]), bits(h)) and torch.equal(bits(res["h32"]), bits(h32)), "gate/up changed the hidden rows"


def _lmhead_once(e, B):
    vocab = e.dims["vocab"]
    h32, h = e.hidden_rows((B, 99))
    res = e.run(LMHEAD, B, h32=h32, h=h)
    ref = R.ref_lmhead(e.W, h32[:B])
    check(res["y"], ref, "lmhead", f"lm-head logits (B {B})")
    rtol, atol, _ = W.tolerances("lmhead")
    tok = res["tok"].tolist()
    for b in range(B):
        assert 0 <= tok[b] < vocab
        top = torch.topk(ref[b], 2)
        tol = atol * ref[b].pow(2).mean().sqrt().item() + rtol * top.values[0].abs().item()
        if (top.values[0] - top.values[1]).item() > 2.0 * tol:   # a priori: twice the logit tolerance
            assert tok[b] == int(top.indices[0]), f"row {b}: token {tok[b]}, reference argmax {int(top.indices[0])}"
        assert tok[b] == int(res["y"][b].argmax()), f"row {b}: the finish picked {tok[b]}, the logit row's own argmax is {int(res['y'][b].argmax())}"
    assert torch.equal(bits(res["h"]), bits(h)) and torch.equal(bits(res["h32"]), bits(h32)), "lm-head changed the hidden rows"


W4_CASES = [pytest.param(B, id=f"W4-B{B}") for B in W.BATCHES["W4"]]


@pytest.mark.parametrize("B", W4_CASES)
def test_qkv_rope_and_kv_append(engines, B):
    """q rows, the rotated K row and the V row at ctx_len[b] on the identity and on a shuffled page table; every other cache row bit-unchanged.
    Three tiles per block; one load step per wave (33-64 rows: one per wave of a half, two phases' worth of rows in the other half's window)"""
    e = engines("W4")
    for li in range(R.LAYERS):
        _qkv_once(e, B, li, None)
        _qkv_once(e, B, li, R.shuffled_pages(B, e.max_pages, (B, li)))


@pytest.mark.parametrize("B", W4_CASES)
def test_oproj_residual(engines, B):
    """K = 4096: four full phases per wave at 17-32 rows, eight at 33-64 (one tile per block: the whole slice requested up front)"""
    e = engines("W4")
    for li in range(R.LAYERS):
        _resid_once(e, OPROJ, B, li)


@pytest.mark.parametrize("B", W4_CASES)
def test_down_residual_eleven_phase_form(engines, B):
    """K = 4224 = 33 load steps: wave 0 owns five, the others four; above 32 rows two launches (40 = 32 + 8: the tail on decode_km.hip)"""
    e = engines("W4")
    for li in range(R.LAYERS):
        _resid_once(e, DOWN, B, li)


@pytest.mark.parametrize("B", W4_CASES)
def test_gateup_swiglu(engines, B):
    e = engines("W4")
    for li in range(R.LAYERS):
        _gateup_once(e, B, li)


@pytest.mark.parametrize("B", W4_CASES)
def test_lmhead_logits_and_greedy_token(engines, B):
    """2004 tiles: six per block; above 32 rows two launches with their own argmax partials"""
    _lmhead_once(engines("W4"), B)


@pytest.mark.parametrize("stage", ["qkv", "gateup", "lmhead"])
def test_many_tile_rings_at_hidden_4096(engines, stage):
    """model T4: K = 4096 is four phases per wave at 32 rows and eight at 64 -- the weight ring is refilled while it is consumed (qkv: three tiles x six
    phases of lookahead; gate/up and the lm-head: four tiles per block on the six-tile form, three phases), which hidden 1024 never does"""
    e = engines("T4")
    try:
        for B in W.BATCHES["T4"]:
            if stage not in W.T4_STAGES[B]:
                continue
            if stage == "qkv":
                _qkv_once(e, B, 0, R.shuffled_pages(B, e.max_pages, (B, 0)))
            elif stage == "gateup":
                _gateup_once(e, B, 0)
            else:
                _lmhead_once(e, B)
    finally:
        e.W.drop()


@pytest.mark.parametrize("kind", ["negative", "tie"])
def test_lmhead_argmax_edge_cases(device, kind):
    """every logit negative (the zero rows that pad the vocabulary to the tile would win an unguarded argmax), and two identical rows in different
    tiles holding the maximum (the lower id wins): 17 rows (one launch of two batch tiles) and 40 (32 + 8: two launches, two families)"""
    e = EngW(device, "W4", 40, sd=_crafted_sd(kind))
    try:
        for B in (17, 40):
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


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------------------
def _model(device, sd_bf, max_batch=W.E2E_MAX_BATCH, max_prompt=40):
    from emmax.modeling import EmmaXForActionPrediction

    model = EmmaXForActionPrediction(W.e2e_cfg(), dict(sd_bf)).to(device, max_batch=max_batch, max_prompt=max_prompt, mxfp4_wide=True)
    assert model.engine.mxfp4_wide and model.engine.max_decode_batch() == 64
    return model


@pytest.fixture(scope="module")
def planted_model(device):
    model = _model(device, W.e2e_state_dict(True, W.E2E_PLANTED_SEED))
    yield model
    model.engine.close()


def test_planted_generation_of_a_ragged_batch_of_24(device, planted_model):
    """ids equal to the oracle's on the de-quantised planted weights and to the a-priori chain, row by row"""
    from emmax.weights import planted_chain

    cfg = W.e2e_cfg()
    sd_q = M.dequant_state_dict(W.e2e_state_dict(True, W.E2E_PLANTED_SEED))
    frames, rows, steps = W.planted_batch(cfg)
    ref = W.planted_oracle(cfg, sd_q, frames, rows)
    _, new_ids, lens = planted_model.generate_actions_batch(torch.from_numpy(frames).to(device), rows, max_new_tokens=W.PLANTED_MAX_NEW)
    for b, row in enumerate(rows):
        got = new_ids[b, : int(lens[b])].cpu().tolist()
        chain = planted_chain(cfg, row[-1], W.PLANTED_MAX_NEW)
        assert got == ref[b][: len(chain)] == chain, (b, got, ref[b], chain)
        assert got[-1] == cfg.eos_token_id and (new_ids[b, int(lens[b]):] == cfg.pad_token_id).all()


def test_slot_serving_24_slots_40_requests(device, planted_model):
    """tests/test_serving_gpu.py's claim on MXFP4 weights above 16 rows: every request's ids equal its own bs = 1 generate"""
    from emmax.serving import Request, SlotScheduler

    cfg = W.e2e_cfg()
    eng = planted_model.engine
    frames, rows, budgets = W.serving_requests(cfg)
    fr = torch.from_numpy(frames).to(device)
    want = []
    for i in range(len(rows)):
        ids, lens = planted_model.generate_ids(rows[i:i + 1], frames_u8=fr[i:i + 1], max_new_tokens=budgets[i])
        want.append(ids[0, : int(lens[0])].cpu().tolist())

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    sch = SlotScheduler(eng, encode, n_slots=W.SLOTS, poll_every=4, encode_ahead=4)
    for i in range(len(rows)):
        sch.submit(Request(i, fr[i], rows[i], max_new_tokens=budgets[i]))
    res = sch.run()
    assert sorted(r.rid for r in res) == list(range(len(rows)))
    for r in res:
        assert r.ids == want[r.rid], f"request {r.rid} (slot {r.slot})"
    assert len({r.slot for r in res}) > 16, "the requests never occupied more than 16 slots"


@pytest.fixture(scope="module")
def random_e2e(device):
    cfg = W.e2e_cfg()
    sd_bf = W.e2e_state_dict(False, W.E2E_RANDOM_SEED)
    sd_q = M.dequant_state_dict(sd_bf)
    frames, rows = W.random_e2e_inputs()
    gens, traces = W.oracle_trace_batch(cfg, sd_q, frames, rows, W.E2E_STEPS)
    model = _model(device, sd_bf)
    yield cfg, model, frames, rows, gens, traces
    model.engine.close()


def test_random_weights_teacher_forced_at_40_rows_eager_and_graph(device, random_e2e, tune):
    """16 teacher-forced steps at B = 40: per-step logits against the oracle on the de-quantised weights at the 2-layer tolerance, the argmax on the
    pinned (row, step) pairs whose oracle margin clears the a-priori id line (counted on the CPU: tests/test_mxfp4_wide_ref.py), and the hipGraph
    replay of the step bit-equal to the eager launches"""
    cfg, model, frames, rows, gens, traces = random_e2e
    sel = list(range(W.E2E_B))
    tune(graph=0)
    worst, checked, agree, eager = _teacher_forced(model, frames, rows, gens, traces, sel, W.E2E_STEPS, device)
    assert not model.engine.graph_active()
    print(f"B {len(sel)}: worst |err| / max|ref| {worst:.3e}, argmax checked {checked}, agreed {agree}")
    assert worst < E2E_TOL, worst
    assert checked == W.E2E_ABOVE_LINE and checked * 4 >= len(sel) * W.E2E_STEPS, checked
    assert agree == checked, (agree, checked)
    tune(graph=1)
    worst_g, checked_g, agree_g, replay = _teacher_forced(model, frames, rows, gens, traces, sel, W.E2E_STEPS, device)
    assert model.engine.graph_active()
    assert (checked_g, agree_g) == (checked, agree)
    for t, (a, b) in enumerate(zip(eager, replay)):
        assert torch.equal(bits(a), bits(b)), f"step {t}: the replayed graph's logits differ from the eager launches'"


def test_a_narrow_engine_in_the_same_process_still_refuses_17_rows(device, planted_model):
    from emmax import _lib

    assert planted_model.engine.mxfp4_wide and _lib.tuning_get("mx4_wide") == 0
    with pytest.raises(_lib.EmmaxError, match="MXFP4 decode weights serve batches of 1-16 rows; max_batch 17"):
        Eng4(device, "W4", 17)
    e = Eng4(device, "W4", 16)
    try:
        assert not e.eng.mxfp4_wide and e.eng.max_decode_batch() == 16
    finally:
        e.eng.close()
    from emmax.engine import EmmaxEngine

    narrow = EmmaxEngine(M.make_cfg4("W4"), dict(M.make_state_dict4("W4")), device=device, max_batch=16, max_prompt=R.MAX_PROMPT, max_ctx=R.MAX_CTX, mxfp4_wide=False)
    try:
        assert not narrow.mxfp4_wide and narrow.max_decode_batch() == 16
    finally:
        narrow.close()
