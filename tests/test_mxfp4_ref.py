"""CPU: the MXFP4 format as the tests' torch reference states it (tests/mxfp4_ref.py) against hand-written cases, the public surface of the
decode weight format (validation, the C mapping, the loaders), the tolerance table of tests/test_mxfp4_gpu.py against the fp32 emulation, and
the planted end-to-end inputs: the oracle on the de-quantised planted weights still emits the a-priori chain, every step above the id line."""

import copy
import ctypes as C

import pytest
import torch

import decode_stage_ref as R
import mxfp4_ref as M
from conftest import ID_BUDGET_SHALLOW, above_id_line


def _qd(vals, fill=0.0):
    b = torch.full((1, M.BLOCK), float(fill), dtype=torch.float32)
    b[0, : len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return M.quant_dequant(b)[0, : len(vals)].tolist()


def test_every_tie_rounds_to_the_even_code():
    # amax 4 pins e = 0 (floor(log2 4) - 2): the elements are their own grid coordinates
    assert _qd([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5]) == [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0]
    assert _qd([5.0, 4.0]) == [4.0, 4.0]                      # amax 5: still e = 0; the tie between 4 and 6 goes to 4
    assert _qd([-4.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5]) == [-4.0, 0.0, -1.0, -1.0, -2.0, -2.0, -4.0]
    # just off the ties: nearest wins
    assert _qd([4.0, 0.251953125, 0.248046875, 1.2578125, 1.2421875, 3.515625, 3.484375]) == [4.0, 0.5, 0.0, 1.5, 1.0, 4.0, 3.0]


def test_amax_power_of_two_and_saturation():
    for k in (-20, -3, 0, 7, 30):
        s = 2.0 ** k
        q, e = M.quantize(torch.tensor([[8.0 * s, 3.0 * s] + [0.0] * 30]))
        assert int(e[0, 0]) == k + 1 and q[0, :2].tolist() == [4.0, 1.5]       # amax 2^(k+3): e = k + 1, amax sits on 4
        q, e = M.quantize(torch.tensor([[7.0 * s, -7.0 * s, 6.5 * s, 5.0 * s] + [0.0] * 28]))
        assert int(e[0, 0]) == k and q[0, :4].tolist() == [6.0, -6.0, 6.0, 4.0]  # amax 7 2^k: e = k, 7 saturates to 6
        assert _qd([7.0 * s, 1.0 * s]) == [6.0 * s, 1.0 * s]


def test_all_zero_block_and_exponent_clamp():
    q, e = M.quantize(torch.zeros(1, 64))
    assert (q == 0).all() and (M.dequantize(q, e) == 0).all() and not torch.signbit(M.dequantize(q, e)).any()
    t = 2.0 ** -127
    w = torch.tensor([[2 * t, 1.5 * t, 1.25 * t, 0.5 * t, 0.25 * t, -t, 2.0 ** -133] + [0.0] * 25], dtype=torch.float32)
    assert torch.equal(w.to(torch.bfloat16).float(), w)          # bf16 denormals
    q, e = M.quantize(w)
    assert int(e[0, 0]) == -127                                  # floor(log2(2^-126)) - 2 = -128 clamps
    assert M.dequantize(q, e)[0, :7].tolist() == [2 * t, 1.5 * t, t, 0.5 * t, 0.0, -t, 0.0]
    # the upper clamp is out of a bf16 weight's reach: the largest finite bf16 asks for e = 125
    assert int(M.quantize(torch.tensor([[3.3895e38] + [0.0] * 31]).to(torch.bfloat16))[1][0, 0]) == 125


@pytest.mark.parametrize("name,block,want", M.adversarial_blocks(), ids=[n for n, _, _ in M.adversarial_blocks()])
def test_hand_written_blocks(name, block, want):
    assert torch.equal(M.quant_dequant(block[None])[0], want)


def test_every_dequantised_value_is_exact_in_bf16_and_requantises_to_itself():
    W, want = M.adversarial_matrix()
    got = M.quant_dequant(W)
    assert torch.equal(got, want)
    assert torch.equal(got.to(torch.bfloat16).double(), got)                       # round trip through bf16 unchanged
    assert torch.equal(M.quant_dequant(got.to(torch.bfloat16)), got)               # idempotent: the write-back changes nothing on a second pass
    g = R.gen(47)
    W = (torch.randn(64, 256, generator=g) * 0.02).to(torch.bfloat16)
    d = M.quant_dequant(W)
    assert torch.equal(d.to(torch.bfloat16).double(), d)
    q, e = M.quantize(W)
    assert set(q.abs().unique().tolist()) <= set(M.E2M1)
    # nearest on the grid: no grid point of the block's scale is closer to w than the one chosen (saturation aside)
    grid = torch.tensor(M.E2M1, dtype=torch.float64)
    x = W.double().view(64, 8, 32).abs() / torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())[..., None]
    best = (x[..., None] - grid).abs().min(-1).values
    assert torch.allclose((x - q.view(64, 8, 32).abs()).abs(), best, rtol=0, atol=0)
    # per row: fusing q / k / v (or gate / up) rows into one matrix does not change a row's blocks
    assert torch.equal(M.quant_dequant(torch.cat([W, W.flip(0)]))[:64], d)


# ---- the public surface -----------------------------------------------------------------------------------------------------------------
def test_decode_weight_dtype_validation_and_c_mapping():
    from emmax.config import DECODE_WEIGHT_DTYPES, EmmaXConfig, check_decode_weight_dtype
    from emmax.engine import _config_c

    assert DECODE_WEIGHT_DTYPES == {"bf16": 0, "fp8": 1, "mxfp4": 2, "mxfp6": 4}
    for name, code in DECODE_WEIGHT_DTYPES.items():
        cfg = EmmaXConfig.tiny()
        cfg.decode_weight_dtype = check_decode_weight_dtype(name)
        assert _config_c(cfg).decode_fp8 == code
    assert _config_c(EmmaXConfig.tiny()).decode_fp8 == 0          # the default stays bf16
    for bad in ("nf4", "int4", "MXFP4", "", None, 4):
        with pytest.raises(ValueError, match="decode_weight_dtype"):
            check_decode_weight_dtype(bad)
        cfg = EmmaXConfig.tiny()
        cfg.decode_weight_dtype = bad
        with pytest.raises(ValueError, match="decode_weight_dtype"):
            _config_c(cfg)


def test_loaders_take_the_format_and_still_refuse_bitsandbytes(tmp_path):
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction

    for kw in (dict(load_in_4bit=True), dict(load_in_8bit=True), dict(load_in_4bit=True, decode_weight_dtype="mxfp4")):
        with pytest.raises(NotImplementedError, match="decode_weight_dtype"):
            EmmaXForActionPrediction.from_pretrained(str(tmp_path), **kw)
    with pytest.raises(ValueError, match="decode_weight_dtype"):   # validated before the checkpoint is touched
        EmmaXForActionPrediction.from_pretrained(str(tmp_path / "no-such-dir"), decode_weight_dtype="nf4")
    with pytest.raises(ValueError, match="decode_weight_dtype"):   # ... and before any weight is generated
        EmmaXForActionPrediction.from_synthetic(EmmaXConfig.tiny(), device="cuda:0", decode_weight_dtype="int4")


def test_the_library_takes_the_format_and_refuses_shapes_and_sessions_outside_it():
    """host only: emmax_model_create / emmax_session_bytes / emmax_model_arena_bytes allocate nothing on a device"""
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.engine import _config_c

    so = _lib.load()
    assert _lib.ABI_VERSION == 12   # (the format came with ABI 11; 12 added the prefill stage ops, new symbols only)

    def create(cfg):
        h, cc = C.c_void_p(), _config_c(cfg)
        return so.emmax_model_create(C.byref(cc), C.byref(h)), h

    bad = EmmaXConfig.tiny()                      # hidden 256
    bad.decode_weight_dtype = "mxfp4"
    rc, _ = create(bad)
    assert rc == -1 and b"MXFP4" in so.emmax_last_error() and b"1024" in so.emmax_last_error()
    short = M.make_cfg4("G4")
    short.llm.intermediate_size = 4096            # not above 4096: the phased down kernel is the only MXFP4 down kernel
    rc, _ = create(short)
    assert rc == -1 and b"intermediate" in so.emmax_last_error()
    cc = _config_c(M.make_cfg4("G4"))
    cc.decode_fp8 = 3
    h = C.c_void_p()
    assert so.emmax_model_create(C.byref(cc), C.byref(h)) == -1 and b"decode_fp8" in so.emmax_last_error()
    for name, rows in (("G4", 8), ("W4", 16)):    # 2 kv heads: split partials at 9 rows -> 8; 32 kv heads: one split -> 16
        rc, h = create(M.make_cfg4(name))
        assert rc == 0 and so.emmax_model_max_decode_batch(h) == rows and so.emmax_model_aux_bytes(h) == 0
        ws, kv = C.c_int64(), C.c_int64()
        assert so.emmax_session_bytes(h, rows, 8, 320, C.byref(ws), C.byref(kv)) == 0
        assert so.emmax_session_bytes(h, rows + 1, 8, 320, C.byref(ws), C.byref(kv)) == -1
        assert b"MXFP4" in so.emmax_last_error() and str(rows + 1).encode() in so.emmax_last_error()
        with _lib.tuning(exact=1):
            assert so.emmax_session_bytes(h, 1, 8, 320, C.byref(ws), C.byref(kv)) == -1 and b"MXFP4" in so.emmax_last_error()
        so.emmax_model_destroy(h)
    rc, h = create(M.make_cfg4("W4"))
    ws, kv = C.c_int64(), C.c_int64()
    assert so.emmax_session_bytes(h, 17, 8, 320, C.byref(ws), C.byref(kv)) == -1 and b"MXFP4" in so.emmax_last_error()
    so.emmax_model_destroy(h)


def test_arena_of_an_mxfp4_7b_model():
    """the bf16 arena + 6.61 B LLM projection parameters x 4.25 bits, nothing in a second arena; LLaMA-2-7B shapes (K 4096 / 11008 = 86 x 128) pass"""
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.engine import _config_c

    so = _lib.load()
    sizes = {}
    for name in ("bf16", "mxfp4"):
        cfg = copy.deepcopy(EmmaXConfig.emma_x_7b())
        cfg.decode_weight_dtype = name
        h, cc = C.c_void_p(), _config_c(cfg)
        assert so.emmax_model_create(C.byref(cc), C.byref(h)) == 0, so.emmax_last_error()
        sizes[name] = (so.emmax_model_arena_bytes(h), so.emmax_model_aux_bytes(h), so.emmax_model_max_decode_batch(h))
        so.emmax_model_destroy(h)
    assert sizes["mxfp4"][1] == 0 and sizes["mxfp4"][2] == 16
    L = EmmaXConfig.emma_x_7b().llm
    vocab_p = (L.vocab_size + 127) // 128 * 128
    params = L.num_layers * (4 * L.hidden_size * L.hidden_size + 3 * L.hidden_size * L.intermediate_size) + vocab_p * L.hidden_size
    assert abs(params - 6.61e9) < 0.01e9
    want = sizes["bf16"][0] + params * 4.25 / 8
    assert abs(sizes["mxfp4"][0] - want) < 0.02 * want, (sizes, want)
    assert abs(sizes["mxfp4"][0] - want) < 1e6                  # (in fact to the 256-byte alignment of its tensors)


# ---- the tolerance table ----------------------------------------------------------------------------------------------------------------
def test_tolerance_table_matches_the_emulation():
    spread, rel = M.measure4(quiet=True)
    for out in M.OUTPUTS:
        assert spread[out] <= 1.05 * M.SPREAD4[out] + 1e-9, (out, spread[out], M.SPREAD4[out])
        assert rel[out] <= 1.05 * M.REL4[out] + 1e-9, (out, rel[out], M.REL4[out])
        if M.SPREAD4[out] > 1e-6:    # not padded
            assert spread[out] >= 0.66 * M.SPREAD4[out], (out, spread[out], M.SPREAD4[out])
        rtol, atol, tol = M.tolerances4(out)
        assert rtol == 1e-2 and atol == max(4e-3, 2 * M.SPREAD4[out]) and tol == max(1e-2, 2 * M.REL4[out])


# ---- the planted end-to-end inputs ----------------------------------------------------------------------------------------------------------
def test_planted_chain_survives_quantisation_with_margin():
    """the fp32 oracle on the DE-QUANTISED planted weights emits the a-priori chain on every row the GPU test generates, and every step's top-2
    margin clears the id line (ID_BUDGET_SHALLOW): PLANTED_*_STEPS ordinary steps + 8 action tokens + EOS per row, none dropped"""
    from emmax.weights import planted_chain

    cfg = M.e2e_cfg()
    sd_q = M.dequant_state_dict(M.e2e_state_dict(True, M.E2E_PLANTED_SEED))
    (fr1, rows1), (fr3, rows3) = M.planted_rows(cfg)
    cases = [(fr1[:1], rows1[0], M.PLANTED_B1_STEPS)] + [(fr3[b:b + 1], rows3[b], M.PLANTED_B3_STEPS[b]) for b in range(3)]
    for frames, row, steps in cases:
        n = steps + 8 + 1
        assert n <= M.PLANTED_MAX_NEW
        gen, trace = M.oracle_trace(cfg, sd_q, frames, row, n)
        chain = planted_chain(cfg, row[-1], M.PLANTED_MAX_NEW)
        assert len(chain) == n and chain[-1] == cfg.eos_token_id
        assert gen == chain, (gen, chain)
        for t in range(n):
            assert above_id_line(trace[t], ID_BUDGET_SHALLOW), (steps, t)
