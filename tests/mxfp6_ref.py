"""References, inputs and tolerances of tests/test_mxfp6_gpu.py and tests/test_mxfp6_ref.py.  TEST INFRASTRUCTURE ONLY (plain torch / numpy on the CPU).

  * the MXFP6 e2m3 quantiser / de-quantiser in torch, what include/emmax.h pins (OCP MX v1.0): blocks of 32 consecutive K elements of one weight row,
    shared exponent e = floor(log2(amax)) - 2 clamped to [-127, 127] (an all-zero block: e = 0), elements w / 2^e rounded to nearest, ties to even,
    onto +-{0, 0.125 .. 0.875, 1 .. 1.875, 2 .. 3.75, 4 .. 7.5}, magnitudes above 7.5 saturate;
  * the element codes and the tile layout as kernels.h / include/emmax.h document them (`codes_of`, `pack_tiles`): what the hardware-widening test plants;
  * `Weights6`: decode_stage_ref.Weights with that de-quantiser -- the float64 reference of every stage test is "the model on de-quantised weights";
  * the stage models are tests/mxfp4_ref.py's (hidden 1024, intermediate 4224 = 33 load steps, G4 / W4) with decode_weight_dtype = "mxfp6", and the
    tolerance table is measured the same way (`python tests/mxfp6_ref.py` prints it, tests/test_mxfp6_ref.py re-checks it);
  * the end-to-end configuration (the G4 shape with the tiny towers), planted and random inputs: mxfp4_ref.py's, on this format.

The rounding here is written per binade (round half to even on the grid step of the element's binade, torch.round); the library's quantiser rounds a
fixed-point integer: two independent statements of the same rule.
"""

import numpy as np
import torch

import decode_stage_ref as R
import mxfp4_ref as M4

BLOCK = 32
# the 32 magnitudes by code: 0 .. 7 subnormals (c / 8), then (1 + m / 8) 2^(E - 1) for E = 1, 2, 3
E2M3 = tuple(c / 8.0 if c < 8 else (1.0 + (c & 7) / 8.0) * 2.0 ** ((c >> 3) - 1) for c in range(32))


# ---- the format --------------------------------------------------------------------------------------------------------------------------
def quantize(W):
    """W [N, K] (K % 32 == 0) -> (q float64 [N, K]: signed grid values, e int64 [N, K / 32]: the blocks' shared exponents)"""
    N, K = W.shape
    assert K % BLOCK == 0
    w = W.double().view(N, K // BLOCK, BLOCK)
    amax = w.abs().amax(-1)
    _, ex = torch.frexp(amax)                      # amax = m 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = (ex.long() - 3).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    x = w.abs() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -e.double())[..., None]
    # round half to even on the step of the binade: 1/8 below 2 (subnormals and [1, 2)), 1/4 in [2, 4), 1/2 from 4 on; above 7.5 saturates
    q = torch.where(x < 2.0, torch.round(x * 8.0) / 8.0, torch.where(x < 4.0, torch.round(x * 4.0) / 4.0, torch.round(x * 2.0) / 2.0)).clamp_max(7.5)
    q = torch.where(w < 0, -q, q)
    return q.view(N, K), e


def dequantize(q, e):
    """the values the copy holds, float64 (every one exact in bf16 while it is finite there); zeros are +0"""
    N, K = q.shape
    v = q.view(N, K // BLOCK, BLOCK) * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())[..., None]
    return torch.where(v == 0, torch.zeros_like(v), v).view(N, K)


def quant_dequant(W):
    return dequantize(*quantize(W))


def codes_of(q, negative=None):
    """signed grid values -> the 6-bit element codes (sign, two exponent bits, three mantissa bits); `negative`: the sign bits (default: q < 0)"""
    table = torch.tensor(E2M3, dtype=torch.float64)
    mag = (q.abs()[..., None] == table).long().argmax(-1)
    assert torch.equal(table[mag], q.abs().double())
    neg = (q < 0) if negative is None else negative
    return (mag + 32 * neg.long()).to(torch.uint8)


def pack_tiles(codes, scale_codes):
    """the tile and scale streams of a matrix in the NATURAL row order, as launch_quant_mx writes them for MXFP6: codes uint8 [N, K], scale_codes uint8
    [N, K / 32] -> (tiles uint8 [N K 6 / 8], scales uint8 [N K / 32]).  Tile (nt, kt) = 16 rows x 128 k at 1536 (nt K / 128 + kt): lane 16 g + r owns
    block g of row r as 192 bits, element i in bits [6 i, 6 i + 6), little endian; bytes 0-15 at 16 lane of the tile's first KiB, bytes 16-23 at
    8 lane of the 512 B behind it.  Scales: one dword per (tile, row), byte g = block g's code."""
    N, K = codes.shape
    NT, KT = N // 16, K // 128
    c = codes.numpy().astype(np.uint32).reshape(NT, 16, KT, 4, 8, 4)          # [nt][r][kt][g][group of four elements][element]
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)  # four elements = 24 bits
    by = np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], -1).astype(np.uint8).reshape(NT, 16, KT, 4, 24)
    by = by.transpose(0, 2, 3, 1, 4)                                          # [nt][kt][g][r][24]: lane = 16 g + r
    tiles = np.concatenate([by[..., :16].reshape(NT, KT, 1024), by[..., 16:].reshape(NT, KT, 512)], -1)
    sc = scale_codes.numpy().reshape(NT, 16, KT, 4).transpose(0, 2, 1, 3)     # [nt][kt][r][g]
    return torch.from_numpy(np.ascontiguousarray(tiles).reshape(-1)), torch.from_numpy(np.ascontiguousarray(sc).reshape(-1))


is_decode_projection = M4.is_decode_projection


def dequant_state_dict(sd):
    """fp32 state dict of the model an MXFP6 engine evaluates: every LLM decode projection de-quantised, everything else as it is"""
    return {k: (quant_dequant(v).float() if is_decode_projection(k) else v.float()) for k, v in sd.items()}


class Weights6(R.Weights):
    """float64 views of a model's LLM weights by HF name, every decode projection de-quantised from MXFP6"""

    def __init__(self, sd, cfg):
        super().__init__(sd, cfg, fp8=False)

    def get(self, key):
        if key not in self.cache:
            w = self.sd["language_model." + key]
            self.cache[key] = quant_dequant(w) if is_decode_projection("language_model." + key) else w.double()
        return self.cache[key]


# ---- the stage models: mxfp4_ref.py's shapes on this format -----------------------------------------------------------------------------------
HIDDEN6, INTER6 = M4.HIDDEN4, M4.INTER4
MODELS6, BATCHES6 = M4.MODELS4, M4.BATCHES4
OUTPUTS = R.OUTPUTS
hidden_rows6, act_rows6, ref_down6, emu_down6 = M4.hidden_rows4, M4.act_rows4, M4.ref_down4, M4.emu_down4


def make_cfg6(model):
    cfg = M4.make_cfg4(model)
    cfg.decode_weight_dtype = "mxfp6"
    return cfg


make_state_dict6 = M4.make_state_dict4     # (the bf16 weights do not depend on the format)

# ---- tolerances: decode_stage_ref.py's rule on these models' inputs --------------------------------------------------------------------------
# atol_frac = max(4e-3, 2 x SPREAD), TOL = max(1e-2, 2 x REL): SPREAD / REL of the fp32 emulation of the documented roundings ("mirror" form)
# against the float64 reference, both on the de-quantised MXFP6 weights, worst over every (model, batch, layer) input of the GPU tests.  A
# de-quantised weight is exact in bf16, so nothing here is specific to the format; the figures differ from mxfp4_ref.py's only because the weights do.
SPREAD6 = {"q": 9.67e-3, "k": 1.22e-2, "v": 1.06e-2, "gateup": 3.10e-2, "oproj_split": 8.42e-3, "oproj": 1.0e-7, "down": 1.0e-7, "lmhead": 1.02e-2}
REL6 = {"q": 6.03e-3, "k": 5.36e-3, "v": 4.52e-3, "gateup": 4.52e-3, "oproj_split": 2.05e-3, "oproj": 1.53e-7, "down": 1.28e-7, "lmhead": 2.61e-3}


def tolerances6(out):
    """(rtol, atol_frac, TOL) of output `out`"""
    return R.RTOL, max(4e-3, 2.0 * SPREAD6[out]), max(1e-2, 2.0 * REL6[out])


def measure6(quiet=False, models=("G4", "W4")):
    worst = {k: 0.0 for k in OUTPUTS}
    rel = {k: 0.0 for k in OUTPUTS}

    def note(name, e, r):
        worst[name] = max(worst[name], R.spread(e, r, R.RTOL))
        rel[name] = max(rel[name], ((e.double() - r.double()).abs().max() / r.double().abs().max()).item())

    for model in models:
        W = Weights6(make_state_dict6(model), make_cfg6(model))
        Hq = MODELS6[model][0]
        for B in BATCHES6[model]:
            for li in range(R.LAYERS):
                h32, _ = hidden_rows6(B, (B, li))
                ctx = R.ctx_rows(B, li)
                for name, e, r in zip("qkv", R.emu_qkv(W, li, h32, ctx, "mirror"), R.ref_qkv(W, li, h32, ctx)):
                    note(name, e, r)
                note("gateup", R.emu_gateup(W, li, h32, "mirror"), R.ref_gateup(W, li, h32))
                part = R.attn_partials(B, Hq, 8, (B, li))
                note("oproj_split", R.emu_oproj(W, li, R.emu_merge(part)), R.ref_oproj(W, li, R.ref_merge(part)))
                x = R.attn_rows(B, Hq * R.HEAD_DIM, (B, li))
                note("oproj", R.emu_oproj(W, li, x), R.ref_oproj(W, li, x))
                a = act_rows6(B, (B, li))
                note("down", emu_down6(W, li, a), ref_down6(W, li, a))
            h32, _ = hidden_rows6(B, (B, 99))
            note("lmhead", R.emu_lmhead(W, h32, "mirror"), R.ref_lmhead(W, h32))
    if not quiet:
        print("mxfp6 spread " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        print("mxfp6 relerr " + "  ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    return worst, rel


# ---- hand-written blocks: every rule of the format once --------------------------------------------------------------------------------------
def adversarial_blocks():
    """list of (name, block [32] float32 (bf16-representable), expected de-quantised block [32] float64)"""
    out = []

    def blk(vals, fill=0.0):
        b = torch.full((BLOCK,), float(fill), dtype=torch.float64)
        b[: len(vals)] = torch.tensor(vals, dtype=torch.float64)
        return b

    grid = torch.tensor(E2M3, dtype=torch.float64)
    # every one of the 32 magnitudes is its own image (7.5 pins e = 0: floor(log2 7.5) - 2), both signs; zero comes back as +0
    out.append(("every-magnitude", grid.flip(0).clone(), grid.flip(0).clone()))
    out.append(("every-magnitude-negative", -grid.flip(0), torch.where(grid.flip(0) == 0, torch.zeros(BLOCK, dtype=torch.float64), -grid.flip(0))))
    # ties, amax 4 (e = 0): the midpoint of two neighbours goes to the even code -- subnormals (step 1/8: 0.0625 -> 0, 0.1875 -> 0.25, 0.9375 -> 1:
    # the carry into the first normal), the first binade (1.0625 -> 1, 1.1875 -> 1.25, 1.9375 -> 2: the carry into the next binade), [2, 4) (step
    # 1/4: 2.125 -> 2, 2.375 -> 2.5, 3.875 -> 4)
    ties_in = [4.0, 0.0625, 0.1875, 0.3125, 0.4375, 0.9375, 1.0625, 1.1875, 1.9375, 2.125, 2.375, 3.625, 3.875]
    ties_out = [4.0, 0.0, 0.25, 0.25, 0.5, 1.0, 1.0, 1.25, 2.0, 2.0, 2.5, 3.5, 4.0]
    out.append(("ties", blk(ties_in), blk(ties_out)))
    out.append(("ties-negative", -blk(ties_in), torch.where(blk(ties_out) == 0, torch.zeros(BLOCK, dtype=torch.float64), -blk(ties_out))))
    # ties of the top binade, amax 7.25 (e = 0, step 1/2): 4.25 -> 4, 4.75 -> 5, 6.75 -> 7, 7.25 -> 7 (odd / even by the mantissa's last bit)
    out.append(("ties-top-binade", blk([7.25, 4.25, 4.75, 5.25, 6.75, -7.25]), blk([7.0, 4.0, 5.0, 5.0, 7.0, -7.0])))
    # just off the ties: nearest wins
    out.append(("off-ties", blk([4.0, 0.0625 + 2 ** -9, 0.1875 - 2 ** -9, 1.0625 + 2 ** -7, 1.1875 - 2 ** -7, 2.125 + 2 ** -6, 2.375 - 2 ** -6]),
                blk([4.0, 0.125, 0.125, 1.125, 1.125, 2.25, 2.25])))
    # the same ties scaled by 2^-9 and 2^20: the exponent moves, the codes do not
    for k in (-9, 20):
        out.append((f"ties-2^{k}", blk(ties_in) * 2.0 ** k, blk(ties_out) * 2.0 ** k))
    # amax = 7.75 2^k (and 8 - 2^-5, the largest bf16 below 8): above 7.5, saturates; 7.625 too; 7.25 is the tie between 7 and 7.5 -> 7
    out.append(("saturates", blk([7.75 * 2 ** -3, -7.96875 * 2 ** -3, 7.625 * 2 ** -3, 7.5 * 2 ** -3, 2 ** -3, 7.25 * 2 ** -3]),
                blk([7.5 * 2 ** -3, -7.5 * 2 ** -3, 7.5 * 2 ** -3, 7.5 * 2 ** -3, 2 ** -3, 7.0 * 2 ** -3])))
    # amax an exact power of two: e = log2(amax) - 2, amax sits on 4
    out.append(("amax-pow2", blk([8.0, 7.0, 6.5, 3.0, 1.0, 0.90625, -8.0, 0.1875]), blk([8.0, 7.0, 6.5, 3.0, 1.0, 1.0, -8.0, 0.25])))
    out.append(("all-zero", blk([]), blk([])))
    # the lower clamp: amax = 2^-126 wants e = -128 and gets -127, so amax lands on x = 2 (not 4); bf16 denormals in and out: 2^-131 is x = 0.0625,
    # half of the smallest subnormal's step: the tie goes to 0; 3 2^-131 (0.1875) -> 0.25; the smallest bf16, 2^-133, rounds to 0
    t = 2.0 ** -127
    out.append(("exponent-clamps", blk([2 * t, 1.5 * t, 1.0625 * t, 0.5 * t, 0.125 * t, -1.0 * t, 2.0 ** -131, 3 * 2.0 ** -131, 2.0 ** -133]),
                blk([2 * t, 1.5 * t, 1.0 * t, 0.5 * t, 0.125 * t, -1.0 * t, 0.0, 0.25 * t, 0.0])))
    # the largest scale a bf16 weight reaches: amax 1.9921875 2^127 -> e = 125 (code 252)
    top = 2.0 ** 125
    out.append(("largest-bf16", blk([7.96875 * top, -7.0 * top, 0.125 * top, 0.0625 * top]), blk([7.5 * top, -7.0 * top, 0.125 * top, 0.0])))
    # negative values round by magnitude, sign kept; a negative that rounds to zero comes back as +0
    out.append(("negative", blk([-4.0, -3.0, -2.875, 2.375, -0.0625, -0.0703125, -1.5, 0.05859375], fill=-0.59765625),
                blk([-4.0, -3.0, -3.0, 2.5, 0.0, -0.125, -1.5, 0.0], fill=-0.625)))
    for name, b, want in out:
        assert torch.equal(b.float().to(torch.bfloat16).double(), b), name   # the inputs are bf16 weights
    return [(n, b.float(), w) for n, b, w in out]


def adversarial_matrix(N=32, K=1024, seed=5):
    """a random bf16 [N, K] matrix (rows of very different scale) with the hand-written blocks planted in it, and the expected de-quantised matrix"""
    g = R.gen(61, seed)
    W = torch.randn(N, K, generator=g) * torch.pow(torch.tensor(2.0), torch.randint(-12, 6, (N, 1), generator=g).float())
    W = W.to(torch.bfloat16).float()
    want = quant_dequant(W)
    for i, (_, b, w) in enumerate(adversarial_blocks()):
        r, c = (5 * i + 3) % N, ((7 * i + 2) % (K // BLOCK)) * BLOCK
        W[r, c:c + BLOCK] = b
        want[r, c:c + BLOCK] = w
    return W.to(torch.bfloat16), want


# ---- end to end: the G4 shape with the tiny towers (mxfp4_ref.py's inputs) ---------------------------------------------------------------------
E2E_PLANTED_SEED, E2E_RANDOM_SEED, E2E_STEPS, E2E_LENS8 = M4.E2E_PLANTED_SEED, M4.E2E_RANDOM_SEED, M4.E2E_STEPS, M4.E2E_LENS8
PLANTED_B1_STEPS, PLANTED_B3_STEPS, PLANTED_B3_LENS, PLANTED_MAX_NEW = M4.PLANTED_B1_STEPS, M4.PLANTED_B3_STEPS, M4.PLANTED_B3_LENS, M4.PLANTED_MAX_NEW
e2e_inputs, planted_rows, oracle_trace = M4.e2e_inputs, M4.planted_rows, M4.oracle_trace


def e2e_cfg():
    return make_cfg6("G4")


def e2e_state_dict(planted, seed):
    return M4.e2e_state_dict(planted, seed)


if __name__ == "__main__":
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "emma-x_amd")]
    torch.set_num_threads(8)
    measure6()
