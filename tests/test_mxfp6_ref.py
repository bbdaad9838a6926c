"""CPU: the MXFP6 e2m3 format as the tests' torch reference states it (tests/mxfp6_ref.py) against hand-written cases, its error figure beside
MXFP4's, the public surface of the decode weight format (validation, the C mapping, the loaders), the host-only library checks, the tolerance table
of tests/test_mxfp6_gpu.py against the fp32 emulation, and the planted end-to-end inputs on the de-quantised weights."""

import copy
import ctypes as C

import pytest
import torch

import decode_stage_ref as R
import mxfp4_ref as M4
import mxfp6_ref as M
from conftest import ID_BUDGET_SHALLOW, above_id_line


def _qd(vals, fill=0.0):
    b = torch.full((1, M.BLOCK), float(fill), dtype=torch.float32)
    b[0, : len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return M.quant_dequant(b)[0, : len(vals)].tolist()


def test_the_grid_is_e2m3():
    assert len(set(M.E2M3)) == 32 and M.E2M3[0] == 0.0 and M.E2M3[1] == 0.125 and M.E2M3[7] == 0.875 and M.E2M3[8] == 1.0 and M.E2M3[31] == 7.5
    assert list(M.E2M3) == sorted(M.E2M3)
    for c, v in enumerate(M.E2M3):     # sign . two exponent bits . three mantissa bits, bias 1
        E, m = c >> 3, c & 7
        assert v == (m / 8.0 if E == 0 else (1 + m / 8.0) * 2.0 ** (E - 1))


def test_every_tie_rounds_to_the_even_code():
    # amax 4 pins e = 0 (floor(log2 4) - 2): the elements are their own grid coordinates
    assert _qd([4.0, 0.0625, 0.1875, 0.9375, 1.0625, 1.9375, 2.125, 2.375, 3.875]) == [4.0, 0.0, 0.25, 1.0, 1.0, 2.0, 2.0, 2.5, 4.0]
    assert _qd([7.25, 4.25, 4.75]) == [7.0, 4.0, 5.0]        # amax 7.25: still e = 0; the tie between 7 and 7.5 goes to 7
    assert _qd([-4.0, -0.0625, -0.1875, -1.0625, -2.375]) == [-4.0, 0.0, -0.25, -1.0, -2.5]
    # just off the ties: nearest wins
    assert _qd([4.0, 0.064453125, 0.060546875, 2.140625, 2.109375]) == [4.0, 0.125, 0.0, 2.25, 2.0]
    # every midpoint of two neighbouring magnitudes goes to the one with the even code
    for c in range(31):
        mid = (M.E2M3[c] + M.E2M3[c + 1]) / 2
        assert _qd([7.5, mid])[1] == M.E2M3[c + (c & 1)], (c, mid)


def test_amax_power_of_two_and_saturation():
    for k in (-20, -3, 0, 7, 30):
        s = 2.0 ** k
        q, e = M.quantize(torch.tensor([[8.0 * s, 3.0 * s] + [0.0] * 30]))
        assert int(e[0, 0]) == k + 1 and q[0, :2].tolist() == [4.0, 1.5]       # amax 2^(k+3): e = k + 1, amax sits on 4
        q, e = M.quantize(torch.tensor([[7.75 * s, -7.75 * s, 7.625 * s, 7.5 * s, 7.25 * s] + [0.0] * 27]))
        assert int(e[0, 0]) == k and q[0, :5].tolist() == [7.5, -7.5, 7.5, 7.5, 7.0]   # amax 7.75 2^k: e = k, everything above 7.5 saturates
        assert _qd([7.75 * s, 1.0 * s]) == [7.5 * s, 1.0 * s]


def test_all_zero_block_and_both_exponent_clamps():
    q, e = M.quantize(torch.zeros(1, 64))
    assert (e == 0).all() and (q == 0).all() and (M.dequantize(q, e) == 0).all() and not torch.signbit(M.dequantize(q, e)).any()
    t = 2.0 ** -127
    w = torch.tensor([[2 * t, 1.5 * t, 1.0625 * t, 0.125 * t, -t, 2.0 ** -131, 2.0 ** -133] + [0.0] * 25], dtype=torch.float32)
    assert torch.equal(w.to(torch.bfloat16).float(), w)          # bf16 denormals
    q, e = M.quantize(w)
    assert int(e[0, 0]) == -127                                  # floor(log2(2^-126)) - 2 = -128 clamps
    assert M.dequantize(q, e)[0, :7].tolist() == [2 * t, 1.5 * t, t, 0.125 * t, -t, 0.0, 0.0]
    # the upper clamp is out of a bf16 weight's reach (the largest finite bf16 asks for e = 125) ...
    assert int(M.quantize(torch.tensor([[3.3895e38] + [0.0] * 31]).to(torch.bfloat16))[1][0, 0]) == 125
    # ... the rule still clamps: amax 2^130 wants e = 128, gets 127, and lands on x = 8, which saturates
    q, e = M.quantize(torch.tensor([[2.0 ** 130, -(2.0 ** 129), 2.0 ** 127] + [0.0] * 29], dtype=torch.float64))
    assert int(e[0, 0]) == 127 and q[0, :3].tolist() == [7.5, -4.0, 1.0]


@pytest.mark.parametrize("name,block,want", M.adversarial_blocks(), ids=[n for n, _, _ in M.adversarial_blocks()])
def test_hand_written_blocks(name, block, want):
    assert torch.equal(M.quant_dequant(block[None])[0], want)


def test_the_hand_written_blocks_cover_the_grid():
    """every one of the 32 magnitudes with both signs, block by block; the clamped scale, the largest scale of a bf16 weight, the all-zero block"""
    seen, es = set(), set()
    for name, b, _ in M.adversarial_blocks():
        q, e = M.quantize(b[None])
        seen |= {(abs(v), v < 0) for v in q[0].tolist() if v != 0}
        es.add((int(e[0, 0]), bool((b == 0).all())))
    assert {m for m, _ in seen} == set(M.E2M3[1:]) and {m for m, n in seen if n} == set(M.E2M3[1:])
    assert (-127, False) in es and (125, False) in es and (0, True) in es


def test_every_dequantised_value_is_exact_in_bf16_and_requantises_to_itself():
    W, want = M.adversarial_matrix()
    got = M.quant_dequant(W)
    assert torch.equal(got, want)
    assert torch.equal(got.to(torch.bfloat16).double(), got)                       # round trip through bf16 unchanged
    assert torch.equal(M.quant_dequant(got.to(torch.bfloat16)), got)               # idempotent: the write-back changes nothing on a second pass
    g = R.gen(53)
    W = (torch.randn(64, 256, generator=g) * 0.02).to(torch.bfloat16)
    d = M.quant_dequant(W)
    assert torch.equal(d.to(torch.bfloat16).double(), d)
    q, e = M.quantize(W)
    assert set(q.abs().unique().tolist()) <= set(M.E2M3) and q.abs().max() <= 7.5
    # nearest on the grid: no grid point of the block's scale is closer to w than the one chosen (saturation aside)
    grid = torch.tensor(M.E2M3, dtype=torch.float64)
    x = W.double().view(64, 8, 32).abs() / torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())[..., None]
    best = (x[..., None] - grid).abs().min(-1).values
    assert torch.allclose((x - q.view(64, 8, 32).abs()).abs(), best, rtol=0, atol=0)
    # per row: fusing q / k / v (or gate / up) rows into one matrix does not change a row's blocks
    assert torch.equal(M.quant_dequant(torch.cat([W, W.flip(0)]))[:64], d)
    # the codes and the packing are each other's inverse on the documented layout: element i of a block in bits [6 i, 6 i + 6)
    codes = M.codes_of(q)
    tiles, scales = M.pack_tiles(codes, (e + 127).to(torch.uint8))
    assert tiles.numel() == 64 * 256 * 6 // 8 and scales.numel() == 64 * 256 // 32
    lane = 16 * 3 + 5                                  # tile (nt 1, kt 1), row 5, block 3 = row 21, k 128 + 96 ..
    base = (1 * 2 + 1) * 1536
    raw = bytes(tiles[base + 16 * lane: base + 16 * lane + 16].tolist()) + bytes(tiles[base + 1024 + 8 * lane: base + 1024 + 8 * lane + 8].tolist())
    word = int.from_bytes(raw, "little")
    assert [(word >> (6 * i)) & 63 for i in range(32)] == codes[21, 224:256].tolist()
    assert int(scales[((1 * 2 + 1) * 16 + 5) * 4 + 3]) == int(e[21, 7]) + 127


def test_error_figure_beside_mxfp4():
    """gaussian [256, 4096] weights, fixed seed: the relative RMS error of quantise-then-de-quantise is a property of the grid -- e2m3 0.0284 against
    MXFP4's 0.1150 (measured with numpy; 5 % headroom for the seed)"""
    W = torch.randn(256, 4096, generator=torch.Generator().manual_seed(0), dtype=torch.float64).float()
    rms = W.double().pow(2).mean().sqrt()
    e6 = ((M.quant_dequant(W) - W.double()).pow(2).mean().sqrt() / rms).item()
    e4 = ((M4.quant_dequant(W) - W.double()).pow(2).mean().sqrt() / rms).item()
    print(f"relative RMS error: mxfp6 {e6:.4f}, mxfp4 {e4:.4f}")
    assert e6 <= 0.030 and e6 < e4 / 3.5, (e6, e4)


# ---- the public surface -----------------------------------------------------------------------------------------------------------------
def test_decode_weight_dtype_validation_and_c_mapping():
    from emmax.config import DECODE_WEIGHT_DTYPES, EmmaXConfig, check_decode_weight_dtype
    from emmax.engine import _config_c

    assert DECODE_WEIGHT_DTYPES == {"bf16": 0, "fp8": 1, "mxfp4": 2, "mxfp6": 4}
    assert check_decode_weight_dtype("mxfp6") == "mxfp6"
    cfg = EmmaXConfig.tiny()
    cfg.decode_weight_dtype = "mxfp6"
    assert _config_c(cfg).decode_fp8 == 4
    for name, code in DECODE_WEIGHT_DTYPES.items():
        cfg.decode_weight_dtype = name
        assert _config_c(cfg).decode_fp8 == code
    for bad in ("nf4", "int4", "MXFP4", "MXFP6", "mxfp6_e3m2", "", None, 4):
        with pytest.raises(ValueError, match="decode_weight_dtype") as ei:
            check_decode_weight_dtype(bad)
        assert all(n in str(ei.value) for n in ("bf16", "fp8", "mxfp4", "mxfp6"))
        cfg.decode_weight_dtype = bad
        with pytest.raises(ValueError, match="decode_weight_dtype"):
            _config_c(cfg)


def test_loaders_take_the_format_and_still_refuse_bitsandbytes(tmp_path):
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction

    for kw in (dict(load_in_4bit=True), dict(load_in_4bit=True, decode_weight_dtype="mxfp6")):
        with pytest.raises(NotImplementedError, match="mxfp6"):
            EmmaXForActionPrediction.from_pretrained(str(tmp_path), **kw)
    # the name passes the validation: what fails next is the missing checkpoint, not the format
    with pytest.raises(Exception) as ei:
        EmmaXForActionPrediction.from_pretrained(str(tmp_path / "no-such-dir"), decode_weight_dtype="mxfp6")
    assert not (isinstance(ei.value, ValueError) and "decode_weight_dtype" in str(ei.value))
    with pytest.raises(ValueError, match="mxfp4_wide"):   # the wide form is MXFP4's alone: refused before any weight is generated
        EmmaXForActionPrediction.from_synthetic(EmmaXConfig.tiny(), device="cuda:0", decode_weight_dtype="mxfp6", mxfp4_wide=True)
    cfg = M.make_cfg6("G4")
    assert cfg.decode_weight_dtype == "mxfp6"
    with pytest.raises(ValueError, match="mxfp4_wide"):
        EmmaXForActionPrediction(cfg, {}).to("cuda:0", mxfp4_wide=True)


def test_the_library_takes_the_format_and_refuses_shapes_and_sessions_outside_it():
    """host only: emmax_model_create / emmax_session_bytes / emmax_model_arena_bytes allocate nothing on a device"""
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.engine import _config_c

    so = _lib.load()
    assert _lib.ABI_VERSION == 12   # new symbols only
    for sym in ("emmax_op_quant_mxfp6", "emmax_op_dequant_mxfp6", "emmax_op_gemm_small_mxfp6"):
        assert hasattr(so, sym)

    def create(cfg):
        h, cc = C.c_void_p(), _config_c(cfg)
        return so.emmax_model_create(C.byref(cc), C.byref(h)), h

    bad = EmmaXConfig.tiny()                      # hidden 256
    bad.decode_weight_dtype = "mxfp6"
    rc, _ = create(bad)
    assert rc == -1 and b"MXFP6" in so.emmax_last_error() and b"1024" in so.emmax_last_error()
    short = M.make_cfg6("G4")
    short.llm.intermediate_size = 4096            # not above 4096: the phased down kernel is the only MXFP6 down kernel
    rc, _ = create(short)
    assert rc == -1 and b"MXFP6" in so.emmax_last_error() and b"intermediate" in so.emmax_last_error()
    for name, rows in (("G4", 8), ("W4", 16)):    # 2 kv heads: split partials at 9 rows -> 8; 32 kv heads: one split -> 16
        rc, h = create(M.make_cfg6(name))
        assert rc == 0, so.emmax_last_error()
        assert so.emmax_model_max_decode_batch(h) == rows and so.emmax_model_aux_bytes(h) == 0 and so.emmax_model_mxfp4_wide(h) == 0
        ws, kv = C.c_int64(), C.c_int64()
        assert so.emmax_session_bytes(h, rows, 8, 320, C.byref(ws), C.byref(kv)) == 0
        assert so.emmax_session_bytes(h, rows + 1, 8, 320, C.byref(ws), C.byref(kv)) == -1
        assert b"MXFP6" in so.emmax_last_error() and str(rows + 1).encode() in so.emmax_last_error()
        with _lib.tuning(exact=1):
            assert so.emmax_session_bytes(h, 1, 8, 320, C.byref(ws), C.byref(kv)) == -1 and b"MXFP6" in so.emmax_last_error()
        so.emmax_model_destroy(h)
    with _lib.tuning(mx4_wide=1):                 # the switch is MXFP4's: an MXFP6 model created under it still serves 1-16 rows
        rc, h = create(M.make_cfg6("W4"))
        assert rc == 0 and so.emmax_model_mxfp4_wide(h) == 0 and so.emmax_model_max_decode_batch(h) == 16
    ws, kv = C.c_int64(), C.c_int64()
    assert so.emmax_session_bytes(h, 17, 8, 320, C.byref(ws), C.byref(kv)) == -1 and b"MXFP6" in so.emmax_last_error()
    so.emmax_model_destroy(h)


def test_arena_of_an_mxfp6_7b_model():
    """the bf16 arena + 6.61 B LLM projection parameters x 6.25 bits, nothing in a second arena; LLaMA-2-7B shapes (K 4096 / 11008 = 86 x 128) pass"""
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.engine import _config_c

    so = _lib.load()
    sizes = {}
    for name in ("bf16", "mxfp6"):
        cfg = copy.deepcopy(EmmaXConfig.emma_x_7b())
        cfg.decode_weight_dtype = name
        h, cc = C.c_void_p(), _config_c(cfg)
        assert so.emmax_model_create(C.byref(cc), C.byref(h)) == 0, so.emmax_last_error()
        sizes[name] = (so.emmax_model_arena_bytes(h), so.emmax_model_aux_bytes(h), so.emmax_model_max_decode_batch(h))
        so.emmax_model_destroy(h)
    assert sizes["mxfp6"][1] == 0 and sizes["mxfp6"][2] == 16
    L = EmmaXConfig.emma_x_7b().llm
    vocab_p = (L.vocab_size + 127) // 128 * 128
    params = L.num_layers * (4 * L.hidden_size * L.hidden_size + 3 * L.hidden_size * L.intermediate_size) + vocab_p * L.hidden_size
    assert abs(params - 6.61e9) < 0.01e9
    want = sizes["bf16"][0] + params * 6.25 / 8
    assert abs(sizes["mxfp6"][0] - want) < 1e6, (sizes, want)


# ---- the tolerance table ----------------------------------------------------------------------------------------------------------------
def test_tolerance_table_matches_the_emulation():
    spread, rel = M.measure6(quiet=True)
    for out in M.OUTPUTS:
        assert spread[out] <= 1.05 * M.SPREAD6[out] + 1e-9, (out, spread[out], M.SPREAD6[out])
        assert rel[out] <= 1.05 * M.REL6[out] + 1e-9, (out, rel[out], M.REL6[out])
        if M.SPREAD6[out] > 1e-6:    # not padded
            assert spread[out] >= 0.66 * M.SPREAD6[out], (out, spread[out], M.SPREAD6[out])
        rtol, atol, tol = M.tolerances6(out)
        assert rtol == 1e-2 and atol == max(4e-3, 2 * M.SPREAD6[out]) and tol == max(1e-2, 2 * M.REL6[out])


# ---- the planted end-to-end inputs ----------------------------------------------------------------------------------------------------------
def test_planted_chain_survives_quantisation_with_margin():
    """the fp32 oracle on the DE-QUANTISED planted weights emits the a-priori chain on every row the GPU tests generate, and every step's top-2
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
