"""References, inputs and tolerances of tests/test_mxfp4_gpu.py and tests/test_mxfp4_ref.py.  TEST INFRASTRUCTURE ONLY (plain torch on the CPU).

  * the MXFP4 quantiser / de-quantiser in torch, bit for bit what include/emmax.h pins (OCP MX v1.0): blocks of 32 consecutive K elements of one
    weight row, shared exponent e = floor(log2(amax)) - 2 clamped to [-127, 127] (an all-zero block: e = 0), elements w / 2^e rounded to nearest,
    ties to even, onto +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, magnitudes above 6 saturate;
  * `Weights4`: decode_stage_ref.Weights with that de-quantiser -- the float64 reference of every stage test is "the model on de-quantised weights";
  * the stage models (hidden 1024: the smallest K the MXFP4 kernels take; intermediate 4224 = 33 x 128, just past 4096: the phased down kernel with
    uneven wave slices), their inputs, and the tolerance table, measured with the fp32 emulation of decode_stage_ref.py ("mirror" form: decode_km.hip
    reads the bf16 mirror) against the float64 reference on these inputs (`python tests/mxfp4_ref.py` prints it, tests/test_mxfp4_ref.py re-checks it);
  * the end-to-end configuration (the G4 shape with the tiny towers), its planted and random inputs.

The rounding here is written per binade (round half to even on the grid step of the element's binade); the library's quantiser compares against
the grid's midpoints in integer arithmetic: two independent statements of the same rule.
"""

import torch

import decode_stage_ref as R

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32


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
    # round half to even on the step of the binade: 0.5 below 2, 1 in [2, 4), 2 from 4 on; above 6 saturates
    q = torch.where(x < 2.0, torch.round(x * 2.0) / 2.0, torch.where(x < 4.0, torch.round(x), torch.round(x / 2.0) * 2.0)).clamp_max(6.0)
    q = torch.where(w < 0, -q, q)
    return q.view(N, K), e


def dequantize(q, e):
    """the values the copy holds, float64 (every one exact in bf16); zeros are +0"""
    N, K = q.shape
    v = q.view(N, K // BLOCK, BLOCK) * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())[..., None]
    return torch.where(v == 0, torch.zeros_like(v), v).view(N, K)


def quant_dequant(W):
    return dequantize(*quantize(W))


PROJ_KEYS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def is_decode_projection(key):
    return key.startswith("language_model.") and (any(p in key for p in PROJ_KEYS) or key.endswith("lm_head.weight"))


def dequant_state_dict(sd):
    """fp32 state dict of the model an MXFP4 engine evaluates: every LLM decode projection de-quantised (q / k / v and gate / up per row each: a
    per-row block scale does not depend on the packing), everything else as it is"""
    return {k: (quant_dequant(v).float() if is_decode_projection(k) else v.float()) for k, v in sd.items()}


class Weights4(R.Weights):
    """float64 views of a model's LLM weights by HF name, every decode projection de-quantised from MXFP4"""

    def __init__(self, sd, cfg):
        super().__init__(sd, cfg, fp8=False)

    def get(self, key):
        if key not in self.cache:
            w = self.sd["language_model." + key]
            self.cache[key] = quant_dequant(w) if is_decode_projection("language_model." + key) else w.double()
        return self.cache[key]


# ---- the stage models --------------------------------------------------------------------------------------------------------------------
HIDDEN4, INTER4 = 1024, 4224       # INTER4 = 33 load steps of 128: wave 0 of the phased down kernel owns five, the others four
MODELS4 = {"G4": (8, 2), "W4": (32, 32)}                    # name -> (query heads, kv heads)
BATCHES4 = {"G4": [1, 2, 3, 8], "W4": [5, 9, 16]}
OUTPUTS = R.OUTPUTS


def make_cfg4(model):
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny()
    L = cfg.llm
    L.intermediate_size, L.num_layers, L.head_dim, L.vocab_size, L.hidden_size = INTER4, R.LAYERS, R.HEAD_DIM, R.VOCAB, HIDDEN4
    L.num_heads, L.num_kv_heads = MODELS4[model]
    cfg.decode_weight_dtype = "mxfp4"
    return cfg


def make_state_dict4(model, seed=3):
    from emmax.weights import synthetic_state_dict

    return {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(make_cfg4(model), seed=seed).items()}


def hidden_rows4(rows, seed, scale=1.0):
    return R.hidden_rows(rows, seed, scale, HIDDEN4)


def act_rows4(B, seed):
    return R.bf(torch.randn(B, INTER4, generator=R.gen(23, seed)))   # (INTER4 is its own padded width: no padding columns)


def ref_down4(W, li, x):
    return x.double() @ W.layer(li, "mlp.down_proj").t()


def emu_down4(W, li, x):
    return x.float() @ W.layer(li, "mlp.down_proj").float().t()


# ---- tolerances: decode_stage_ref.py's rule on these models' inputs --------------------------------------------------------------------------
# atol_frac = max(4e-3, 2 x SPREAD), TOL = max(1e-2, 2 x REL): SPREAD / REL of the fp32 emulation of the documented roundings ("mirror" form)
# against the float64 reference, both on the de-quantised weights, worst over every (model, batch, layer) input of the GPU tests.  A de-quantised
# MXFP4 weight is exact in bf16, so nothing here is specific to the format: the figures differ from decode_stage_ref.py's because K is 1024, not 256.
SPREAD4 = {"q": 9.51e-3, "k": 1.15e-2, "v": 9.54e-3, "gateup": 3.41e-2, "oproj_split": 7.37e-3, "oproj": 1.0e-7, "down": 1.0e-7, "lmhead": 1.02e-2}
REL4 = {"q": 5.56e-3, "k": 6.03e-3, "v": 3.81e-3, "gateup": 4.78e-3, "oproj_split": 2.01e-3, "oproj": 1.48e-7, "down": 1.42e-7, "lmhead": 2.56e-3}


def tolerances4(out):
    """(rtol, atol_frac, TOL) of output `out`"""
    return R.RTOL, max(4e-3, 2.0 * SPREAD4[out]), max(1e-2, 2.0 * REL4[out])


def measure4(quiet=False, models=("G4", "W4")):
    worst = {k: 0.0 for k in OUTPUTS}
    rel = {k: 0.0 for k in OUTPUTS}

    def note(name, e, r):
        worst[name] = max(worst[name], R.spread(e, r, R.RTOL))
        rel[name] = max(rel[name], ((e.double() - r.double()).abs().max() / r.double().abs().max()).item())

    for model in models:
        W = Weights4(make_state_dict4(model), make_cfg4(model))
        Hq = MODELS4[model][0]
        for B in BATCHES4[model]:
            for li in range(R.LAYERS):
                h32, _ = hidden_rows4(B, (B, li))
                ctx = R.ctx_rows(B, li)
                for name, e, r in zip("qkv", R.emu_qkv(W, li, h32, ctx, "mirror"), R.ref_qkv(W, li, h32, ctx)):
                    note(name, e, r)
                note("gateup", R.emu_gateup(W, li, h32, "mirror"), R.ref_gateup(W, li, h32))
                part = R.attn_partials(B, Hq, 8, (B, li))
                note("oproj_split", R.emu_oproj(W, li, R.emu_merge(part)), R.ref_oproj(W, li, R.ref_merge(part)))
                x = R.attn_rows(B, Hq * R.HEAD_DIM, (B, li))
                note("oproj", R.emu_oproj(W, li, x), R.ref_oproj(W, li, x))
                a = act_rows4(B, (B, li))
                note("down", emu_down4(W, li, a), ref_down4(W, li, a))
            h32, _ = hidden_rows4(B, (B, 99))
            note("lmhead", R.emu_lmhead(W, h32, "mirror"), R.ref_lmhead(W, h32))
    if not quiet:
        print("mxfp4 spread " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        print("mxfp4 relerr " + "  ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    return worst, rel


# ---- hand-written blocks: every rule of the format once --------------------------------------------------------------------------------------
def adversarial_blocks():
    """list of (name, block [32] float32 (bf16-representable), expected de-quantised block [32] float64)"""
    out = []

    def blk(vals, fill=0.0):
        b = torch.full((BLOCK,), float(fill), dtype=torch.float64)
        b[: len(vals)] = torch.tensor(vals, dtype=torch.float64)
        return b

    ties_in = [4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]          # amax 4: e = 0, the elements are their own x
    ties_out = [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    out.append(("ties", blk(ties_in), blk(ties_out)))
    out.append(("ties-negative", -blk(ties_in), torch.where(blk(ties_out) == 0, torch.zeros(BLOCK, dtype=torch.float64), -blk(ties_out))))
    # the same block scaled by 2^-9 and 2^20: the exponent moves, the codes do not
    for k in (-9, 20):
        out.append((f"ties-2^{k}", blk(ties_in) * 2.0 ** k, blk(ties_out) * 2.0 ** k))
    # amax an exact power of two: e = log2(amax) - 2, amax sits on 4 and neighbours keep three binades of grid below it
    out.append(("amax-pow2", blk([8.0, 7.0, 6.5, 3.0, 1.0, 0.90625, -8.0]), blk([8.0, 8.0, 6.0, 3.0, 1.0, 1.0, -8.0])))
    # amax = 7 2^k: x = 7 is above 6 and saturates (e = k: floor(log2(7 2^k)) = k + 2)
    out.append(("amax-7-saturates", blk([7.0 * 2 ** -3, -7.0 * 2 ** -3, 6.5 * 2 ** -3, 2 ** -3, 5 * 2 ** -3]),
                blk([6.0 * 2 ** -3, -6.0 * 2 ** -3, 6.0 * 2 ** -3, 2 ** -3, 4 * 2 ** -3])))
    out.append(("all-zero", blk([]), blk([])))
    # the exponent clamps: amax = 2^-126 wants e = -128 and gets -127, so amax lands on x = 2 (not 4); bf16 denormals in and out
    t = 2.0 ** -127
    out.append(("exponent-clamps", blk([2 * t, 1.5 * t, 1.25 * t, 0.5 * t, 0.25 * t, -1.0 * t, 2.0 ** -133]),
                blk([2 * t, 1.5 * t, 1.0 * t, 0.5 * t, 0.0, -1.0 * t, 0.0])))
    # negative values round by magnitude, sign kept (amax 4: e = 0); a negative that rounds to zero comes back as +0
    out.append(("negative", blk([-4.0, -3.0, -2.875, 2.375, -0.2578125, -0.2421875, -1.5, 0.099609375], fill=-0.59765625),
                blk([-4.0, -3.0, -3.0, 2.0, -0.5, 0.0, -1.5, 0.0], fill=-0.5)))
    for name, b, want in out:
        assert torch.equal(b.float().to(torch.bfloat16).double(), b), name   # the inputs are bf16 weights
    return [(n, b.float(), w) for n, b, w in out]


def adversarial_matrix(N=32, K=1024, seed=5):
    """a random bf16 [N, K] matrix (rows of very different scale) with the hand-written blocks planted in it, and the expected de-quantised matrix"""
    g = R.gen(43, seed)
    W = torch.randn(N, K, generator=g) * torch.pow(torch.tensor(2.0), torch.randint(-12, 6, (N, 1), generator=g).float())
    W = W.to(torch.bfloat16).float()
    want = quant_dequant(W)
    for i, (_, b, w) in enumerate(adversarial_blocks()):
        r, c = (5 * i + 3) % N, ((7 * i + 2) % (K // BLOCK)) * BLOCK
        W[r, c:c + BLOCK] = b
        want[r, c:c + BLOCK] = w
    return W.to(torch.bfloat16), want


# ---- end to end: the G4 shape with the tiny towers ------------------------------------------------------------------------------------------
E2E_PLANTED_SEED = 5
E2E_RANDOM_SEED = 21
E2E_STEPS = 16                      # teacher-forced steps of the random-weight test
E2E_LENS8 = [24, 9, 17, 30, 5, 12, 21, 28]
# planted weights: ordinary steps before the action prefix, per row; the chain is steps + 8 action tokens + EOS long
PLANTED_B1_STEPS = 6
PLANTED_B3_STEPS = [2, 9, 4]
PLANTED_B3_LENS = [10, 17, 5]
PLANTED_MAX_NEW = 24


def e2e_cfg():
    cfg = make_cfg4("G4")
    return cfg


def e2e_state_dict(planted, seed):
    from emmax.weights import synthetic_state_dict

    return {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(e2e_cfg(), seed=seed, planted=planted).items()}


def e2e_inputs(B, P, seed=1234, last=None):
    import numpy as np

    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(B, 224, 224, 3), dtype=np.uint8)
    rows = []
    for b in range(B):
        n = P if isinstance(P, int) else P[b]
        r = [1] + [int(x) for x in rng.integers(3, 31744, size=n - 1)]
        if last is not None:
            r[-1] = last if isinstance(last, int) else last[b]
        rows.append(r)
    return frames, rows


def planted_rows(cfg):
    """(frames, rows) of the B = 1 and the ragged B = 3 planted cases"""
    from emmax.weights import planted_start_token

    one = e2e_inputs(1, 14, last=planted_start_token(cfg, PLANTED_B1_STEPS))
    three = e2e_inputs(3, PLANTED_B3_LENS, seed=77, last=[planted_start_token(cfg, k) for k in PLANTED_B3_STEPS])
    return one, three


def oracle_trace(cfg, sd_ref, frames, row, T):
    """greedy ids and per-step last-position logits of one row over T steps (step 0 from the prefill), the fp32 oracle on `sd_ref`"""
    from oracle import emmax_oracle as orc

    with torch.inference_mode():
        ids, trace = orc.greedy_generate(torch.tensor([row]), orc.preprocess_frames(frames, cfg), sd_ref, cfg, T, eos_token_id=None, return_trace=True)
    return ids[0, len(row):].tolist(), [t.float() for t in trace]


if __name__ == "__main__":
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "emma-x_amd")]
    torch.set_num_threads(8)
    measure4()
