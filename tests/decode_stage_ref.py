"""References, inputs and tolerances of tests/test_decode_stages_gpu.py.  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

Three things live here so that the GPU tests and the CPU measurement of the tolerances use the same code and the same inputs:

  * the float64 REFERENCE of every fused decode stage, built from the HF-named weights of the state dict (q_proj / k_proj / v_proj,
    gate_proj / up_proj, ...), never from the packed arena: packing, interleave and row permutation are under test;
  * a float32 EMULATION of every stage that applies exactly the roundings the kernel sources document and nothing else;
  * the tolerance constants, derived from the spread of that emulation against the reference on the tests' own inputs
    (`python tests/decode_stage_ref.py` prints the measurement; tests/test_decode_stage_tolerances.py re-checks it without a GPU).

The roundings (emma-x_amd/csrc/decode*.hip), most-rounded form of each stage:
  RMSNorm prologue   decode_ks.hip reads the fp32 stream: x g in fp32, ONE rounding to bf16, rstd applied to the fp32 sum.  decode_km.hip /
                     decode_kmp.hip read the bf16 mirror: bf16(bf16(x) g).  decode.hip's staged GEMV and decode_mfma.hip follow HF's LlamaRMSNorm on
                     the mirror: bf16(bf16(bf16(x) rstd) g).  The emulation takes the last form (three roundings): the widest.
  QKV epilogue       the linear output is rounded to bf16, RoPE in fp32 on those values (fp32 cos / sin tables from fp32 pos * inv_freq, HF's
                     LlamaRotaryEmbedding order), the rotated q / K rounded to bf16; V is the rounded linear output.
  SwiGLU epilogue    bf16(silu(g) u) with g, u the fp32 sums (silu through the hardware exp2 / rcp: ~1 ulp of fp32 each).
  residual add       h32 + W x in fp32; the bf16 mirror is bf16 of that same fp32 value.
  split merge        fp32 merge of the partials, ONE rounding of the merged row to bf16 (the MFMA / dot2 operand).
  lm-head            fp32 logits of the normalised operand.
  exact numerics     every activation operand enters as two bf16 terms hi + lo (2^-17 relative), fp32 everywhere else; 24-bit K / V cache
                     (2^-16 relative per element); fp32 RoPE with every product rounded on its own.
"""

import math

import pytest
import torch

# ---- dimensions (ISSUE: the smallest at which every kernel family is reached) ------------------------------------------------------------
HIDDEN, HEAD_DIM, LAYERS, VOCAB, INTER = 256, 128, 2, 32064, 4160
MAX_PROMPT = 8
MAX_CTX = 320          # 5 pages of 64; contexts up to MAX_CTX - 2 = 318
PAGE = 64
PSTRIDE = 132
INTER_P = (INTER + 63) // 64 * 64   # the activation rows' pitch: the intermediate size padded to 64
MODELS = {"G": (4, 2, HIDDEN), "W": (32, 32, HIDDEN), "H": (32, 32, 512)}   # name -> (query heads, kv heads, hidden); H: fp8 tiles on the K-split kernels need K % 512

# ---- stages and launcher families (include/emmax.h: the stage numbers of emmax_op_decode_stage, EMMAX_VIA_*) ----------------------------------
QKV, OPROJ, GATEUP, DOWN, LMHEAD = 0, 2, 3, 4, 5
KS, GEMV, GEMV_FP8, KM, KMP, MFMA = 1, 2, 3, 4, 5, 6
REFUSED = -1
VIA_NAME = {0: "none", KS: "ks", GEMV: "gemv", GEMV_FP8: "gemv_fp8", KM: "km", KMP: "kmp", MFMA: "mfma", REFUSED: "refused"}



# ---- the routing table (ISSUE): (engine, rows, switches, expected launcher per stage) -------------------------------------------------------
def _all(v):
    return {QKV: v, OPROJ: v, GATEUP: v, DOWN: v, LMHEAD: v}


def _case(eng, B, sw, via):
    name = f"{eng}-B{B}" + "".join(f"-{k}{v}" for k, v in sw.items())
    return pytest.param(eng, B, sw, via, id=name)


KM_SPLIT = {QKV: KM, OPROJ: MFMA, GATEUP: KM, DOWN: KM, LMHEAD: KM}       # the bf16 o-proj with split partials stays on decode_mfma.hip
F8_SMALL_K = {QKV: MFMA, OPROJ: KM, GATEUP: MFMA, DOWN: KM, LMHEAD: MFMA}  # fp8 tiles at K = 256: decode_km.hip refuses (K % 512), decode_mfma.hip serves
CASES = [
    _case("G", 1, {}, _all(KS)), _case("G", 2, {}, _all(KS)), _case("G", 1, {"resid32": 0}, _all(KS)),
    _case("G", 1, {"ks": 0}, _all(GEMV)), _case("G", 2, {"ks": 0}, _all(GEMV)), _case("G", 1, {"ks": 0, "resid32": 0}, _all(GEMV)),
    _case("G", 3, {}, KM_SPLIT), _case("G", 8, {}, KM_SPLIT), _case("G", 3, {"km": 0}, _all(MFMA)), _case("G", 8, {"km": 0}, _all(MFMA)),
    _case("W", 5, {}, _all(KM)), _case("W", 9, {}, _all(KM)), _case("W", 16, {}, _all(KM)),
    _case("W", 17, {}, _all(KMP)), _case("W", 32, {}, _all(KMP)),
    # 33 rows: down / lm-head run as 32 + 1 rows, and the one-row launch is a batch-1 launch (decode_ks.hip); 64 rows: 32 + 32
    _case("W", 33, {}, {QKV: KMP, OPROJ: KMP, GATEUP: KMP, DOWN: KS, LMHEAD: KS}), _case("W", 64, {}, _all(KMP)),
    # fp8 weights, 1-2 rows: the default mask puts the o-proj (and at one row the lm-head) on the row GEMV
    _case("G8", 1, {}, {QKV: MFMA, OPROJ: GEMV_FP8, GATEUP: MFMA, DOWN: KM, LMHEAD: GEMV_FP8}),
    _case("G8", 2, {}, {QKV: MFMA, OPROJ: GEMV_FP8, GATEUP: MFMA, DOWN: KM, LMHEAD: MFMA}),
    _case("G8", 1, {"fp8_gemv": 0}, F8_SMALL_K), _case("G8", 2, {"fp8_gemv": 0}, F8_SMALL_K),
    _case("G8", 1, {"fp8_gemv": 31}, _all(GEMV_FP8)), _case("G8", 2, {"fp8_gemv": 31}, _all(GEMV_FP8)),
    _case("G8", 3, {}, F8_SMALL_K), _case("G8", 8, {}, F8_SMALL_K),
    _case("W8", 8, {}, F8_SMALL_K),
    _case("W8", 16, {}, {QKV: REFUSED, OPROJ: KM, GATEUP: REFUSED, DOWN: KM, LMHEAD: REFUSED}),
    _case("W8", 32, {}, {QKV: REFUSED, OPROJ: KMP, GATEUP: REFUSED, DOWN: KMP, LMHEAD: REFUSED}),
    _case("W8", 64, {}, {QKV: KMP, OPROJ: KMP, GATEUP: KMP, DOWN: KMP, LMHEAD: REFUSED}),
    # hidden 512: the fp8 qkv / gate-up / lm-head on the K-split kernels (8 and 16 staged rows of decode_km.hip, decode_kmp.hip)
    _case("H8", 3, {}, _all(KM)), _case("H8", 16, {}, _all(KM)), _case("H8", 32, {}, _all(KMP)),
    _case("GX", 1, {}, _all(KS)), _case("GX", 2, {}, _all(KS)), _case("GX", 3, {}, _all(KM)), _case("GX", 8, {}, _all(KM)),
    # a split count other than 8: the o-proj merges the partials in a loop (attn_merge_chunk_loop) -- the staged GEMV's, decode_ks.hip's fp32 one
    _case("G", 2, {"ks": 0, "attn_nsplit": 4}, _all(GEMV)), _case("GX", 2, {"attn_nsplit": 4}, _all(KS)),
]


# ---- tolerances ------------------------------------------------------------------------------------------------------------------------
# assert_elementwise(got, ref, rtol, atol_frac): |err| <= atol_frac * rms(ref) + rtol * |ref|; relerr: max|err| / max|ref|.  The project's
# bf16 line (tests/test_ops_gpu.py) is TOL = 1e-2, rtol = 1e-2, atol_frac = 4e-3.  The fused stages round more often than a plain projection,
# so per (operand form, output):   atol_frac = max(4e-3, 2 x SPREAD),   TOL = max(1e-2, 2 x REL)
# where SPREAD is the smallest atol_frac at which the fp32 EMULATION below passes against the float64 reference at rtol = 1e-2, and REL its
# relerr, worst over every (model, batch, layer, bf16 / de-quantised fp8 weights) input the tests use.  Measured on the CPU, no GPU output
# involved (`python tests/decode_stage_ref.py` prints them; tests/test_decode_stage_tolerances.py keeps the table honest):
SPREAD = {
    "f32":    {"q": 9.72e-3, "k": 1.01e-2, "v": 7.37e-3, "gateup": 2.62e-2, "lmhead": 8.16e-3},
    "mirror": {"q": 1.22e-2, "k": 1.32e-2, "v": 1.12e-2, "gateup": 2.98e-2, "lmhead": 1.18e-2},
    "hf":     {"q": 1.46e-2, "k": 1.42e-2, "v": 1.45e-2, "gateup": 4.30e-2, "lmhead": 1.43e-2},
    "exact":  {"q": 3.24e-5, "k": 1.07e-5, "v": 8.62e-6, "gateup": 2.24e-5, "lmhead": 1.05e-5, "oproj_split": 9.49e-6, "oproj": 6.73e-6, "down": 9.46e-6},
}
REL = {
    "f32":    {"q": 5.86e-3, "k": 6.03e-3, "v": 4.41e-3, "gateup": 5.34e-3, "lmhead": 1.92e-3},
    "mirror": {"q": 6.29e-3, "k": 6.60e-3, "v": 4.22e-3, "gateup": 7.24e-3, "lmhead": 2.80e-3},
    "hf":     {"q": 8.08e-3, "k": 6.72e-3, "v": 5.29e-3, "gateup": 7.28e-3, "lmhead": 3.45e-3},
    "exact":  {"q": 1.08e-5, "k": 1.17e-5, "v": 1.36e-5, "gateup": 4.40e-6, "lmhead": 2.74e-6, "oproj_split": 4.14e-6, "oproj": 3.07e-6, "down": 2.98e-6},
}
# the stages without a norm prologue do not depend on the operand form: the split merge rounds the merged row once, bf16 rows go in as they are
for _f in ("f32", "mirror", "hf"):
    SPREAD[_f].update({"oproj_split": 9.20e-3, "oproj": 4.5e-7, "down": 2.5e-7})
    REL[_f].update({"oproj_split": 2.36e-3, "oproj": 4.3e-7, "down": 4.3e-7})
RTOL = 1e-2
# exact numerics: rtol = 2^-15 -- a two-term operand is 2^-17 per operand, the 24-bit cache 2^-16 per element, the fp32 epilogue a few 2^-24
# each; atol_frac and TOL from the two-term emulation in the same way with that floor.  (The widest line, q / K, is the fp32 RoPE angle
# pos * inv_freq at positions up to 318: 318 x 2^-23 rad.)
X_RTOL = 2.0 ** -15


def tolerances(form, out):
    """(rtol, atol_frac, TOL) of output `out` computed through operand form `form`"""
    if form == "exact":
        return X_RTOL, max(X_RTOL, 2.0 * SPREAD[form][out]), max(X_RTOL, 2.0 * REL[form][out])
    return RTOL, max(4e-3, 2.0 * SPREAD[form][out]), max(1e-2, 2.0 * REL[form][out])


def bf(x):
    return x.to(torch.bfloat16)


def bfr(x):
    """round to bf16 and back: the value a bf16 store keeps"""
    return x.to(torch.bfloat16).to(x.dtype)


def make_cfg(model, fp8=False):
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny()
    L = cfg.llm
    L.intermediate_size, L.num_layers, L.head_dim, L.vocab_size = INTER, LAYERS, HEAD_DIM, VOCAB
    L.num_heads, L.num_kv_heads, L.hidden_size = MODELS[model]
    if fp8:
        cfg.decode_weight_dtype = "fp8"
    return cfg


def make_state_dict(model, seed=3):
    """bf16 state dict of model `model` (HF names)"""
    from emmax.weights import synthetic_state_dict

    return {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(make_cfg(model), seed=seed).items()}


def dequant_e4m3_rows(W):
    """the values an fp8 weight copy holds: per-row scale amax / 448, e4m3 (OCP) codes -- as tests/test_ops_gpu.py pins the quantiser"""
    W = W.float()
    scale = W.abs().amax(dim=1).clamp_min(1e-30) / 448.0
    return ((W / scale[:, None]).to(torch.float8_e4m3fn).float() * scale[:, None]).double()


class Weights:
    """float64 views of one model's LLM weights by HF name; fp8: the de-quantised values of every decode projection.  The fused qkv matrix is
    quantised per row of [q; k; v], gate and up per row each: a per-row scale does not depend on the packing."""

    def __init__(self, sd, cfg, fp8=False):
        self.cfg, self.fp8 = cfg, fp8
        self.sd = sd
        self.cache = {}

    def get(self, key):
        if key not in self.cache:
            w = self.sd["language_model." + key]
            is_proj = w.dim() == 2 and "embed_tokens" not in key
            self.cache[key] = dequant_e4m3_rows(w) if (self.fp8 and is_proj) else w.double()
        return self.cache[key]

    def layer(self, li, name):
        return self.get(f"model.layers.{li}.{name}.weight")


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def gen(*seed):
    """a generator seeded by the (nested) integers of `seed`"""
    flat = []
    for s in seed:
        flat += [int(v) for v in s] if isinstance(s, (tuple, list)) else [int(s)]
    n = 0
    for v in flat:
        n = (n * 1000003 + v + 1) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(n)
    return g


def hidden_rows(R, seed, scale=1.0, hidden=HIDDEN):
    """fp32 hidden rows that are NOT bf16-representable, and their bf16 mirror"""
    h32 = (torch.randn(R, hidden, generator=gen(11, seed)) * scale).float()
    return h32, bf(h32)


CTX_MIX = [0, 1, 63, 64, 65, 127, 128, MAX_CTX - 2]


def ctx_rows(B, shift=0):
    return [CTX_MIX[(b + shift) % len(CTX_MIX)] for b in range(B)]


def shuffled_pages(B, max_pages, seed):
    perm = torch.randperm(B * max_pages, generator=gen(13, seed))
    return perm.view(B, max_pages).to(torch.int32)


def attn_rows(B, q_dim, seed):
    return bf(torch.randn(B, q_dim, generator=gen(17, seed)))


def attn_partials(B, Hq, ns, seed):
    """split partials [B][Hq][ns][132] with unequal maxima across the splits and split 1 EMPTY (l = 0, m = -inf, o = 0: what the attention
    kernel writes for a split without keys); ns = 1: one live split"""
    g = gen(19, seed)
    part = torch.zeros(B, Hq, ns, PSTRIDE)
    part[..., :128] = torch.randn(B, Hq, ns, 128, generator=g) * 3.0
    part[..., 128] = torch.randn(B, Hq, ns, generator=g) * 4.0          # m: maxima several e-folds apart
    part[..., 129] = torch.rand(B, Hq, ns, generator=g) * 5.0 + 0.5     # l
    if ns > 1:
        part[:, :, 1, :128] = 0.0
        part[:, :, 1, 128] = float("-inf")
        part[:, :, 1, 129] = 0.0
    return part.float()


def attn_rows32(B, q_dim, seed):
    """exact numerics: the fp32 attention rows (not bf16-representable)"""
    return torch.randn(B, q_dim, generator=gen(29, seed)).float()


def act_rows32(B, inter_p, seed):
    x = torch.randn(B, inter_p, generator=gen(31, seed)).float()
    x[:, INTER:] = 0.0
    return x


def act_rows(B, inter_p, seed):
    x = torch.randn(B, inter_p, generator=gen(23, seed))
    x[:, INTER:] = 0.0   # padding columns of the activation rows are zero in the product
    return bf(x)


# ---- float64 references ----------------------------------------------------------------------------------------------------------------
def rmsnorm64(x, g, eps):
    x = x.double()
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g.double()


def rope_tables64(pos, theta):
    i = torch.arange(HEAD_DIM // 2, dtype=torch.float64)
    inv = theta ** (-2.0 * i / HEAD_DIM)
    f = torch.as_tensor(pos, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.cos(f), torch.sin(f)


def rope_tables32(pos, theta):
    """the session's fp32 tables (session.hip): inv_freq fp32, pos * inv_freq fp32, cos / sin of that fp32 angle"""
    half = HEAD_DIM // 2
    inv = torch.tensor([1.0 / math.pow(torch.tensor(theta, dtype=torch.float32).item(), (2 * i) / HEAD_DIM) for i in range(half)]).float()
    f = torch.as_tensor(pos, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cos(f.double()).float(), torch.sin(f.double()).float()


def rotate(x, cos, sin):
    """HF rotate-half pairing (d, d + 64); x [B][heads][128], cos / sin [B][64]"""
    half = HEAD_DIM // 2
    x0, x1 = x[..., :half], x[..., half:]
    c, s = cos[:, None, :], sin[:, None, :]
    return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1)


def ref_qkv(W, li, x, ctx):
    cfg = W.cfg.llm
    xn = rmsnorm64(x, W.layer(li, "input_layernorm"), cfg.rms_eps)
    B = x.shape[0]
    q = (xn @ W.layer(li, "self_attn.q_proj").t()).view(B, cfg.num_heads, HEAD_DIM)
    k = (xn @ W.layer(li, "self_attn.k_proj").t()).view(B, cfg.num_kv_heads, HEAD_DIM)
    v = (xn @ W.layer(li, "self_attn.v_proj").t()).view(B, cfg.num_kv_heads, HEAD_DIM)
    cos, sin = rope_tables64(ctx, cfg.rope_theta)
    return rotate(q, cos, sin).reshape(B, -1), rotate(k, cos, sin), v


def ref_merge(part):
    p = part.double()
    m, l, o = p[..., 128], p[..., 129], p[..., :128]
    M = m.max(dim=-1, keepdim=True).values
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - M))
    den = (l * w).sum(-1)
    out = (o * w[..., None]).sum(-2) / den[..., None]
    return out.reshape(part.shape[0], -1)


def ref_oproj(W, li, x):
    return x.double() @ W.layer(li, "self_attn.o_proj").t()


def ref_gateup(W, li, x):
    xn = rmsnorm64(x, W.layer(li, "post_attention_layernorm"), W.cfg.llm.rms_eps)
    g = xn @ W.layer(li, "mlp.gate_proj").t()
    u = xn @ W.layer(li, "mlp.up_proj").t()
    return torch.nn.functional.silu(g) * u


def ref_down(W, li, x):
    return x.double()[:, :INTER] @ W.layer(li, "mlp.down_proj").t()


def ref_lmhead(W, x):
    xn = rmsnorm64(x, W.get("model.norm.weight"), W.cfg.llm.rms_eps)
    return xn @ W.get("lm_head.weight").t()


# ---- fp32 emulations: the documented roundings, nothing else -------------------------------------------------------------------------------
def emu_norm_operand(x32, g, eps, form):
    """the activation operand of a NORM stage in one of the documented forms, and the factor its fp32 sum is scaled by"""
    g = g.float()
    x32 = x32.float()
    if form == "exact":   # x g in fp32, two terms; rstd on the sum
        xg = x32 * g
        hi = bfr(xg)
        return hi + bfr(xg - hi), torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + eps)
    if form == "f32":     # decode_ks.hip on the fp32 stream: ONE rounding
        return bfr(x32 * g), torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + eps)
    xm = bfr(x32)         # the bf16 mirror
    rstd = torch.rsqrt(xm.pow(2).mean(-1, keepdim=True) + eps)
    if form == "mirror":  # decode_km.hip / decode_kmp.hip (and decode_ks.hip without the fp32 stream)
        return bfr(xm * g), rstd
    assert form == "hf"   # decode.hip's staged GEMV, decode_mfma.hip: HF LlamaRMSNorm on the mirror
    return bfr(bfr(xm * rstd) * g), torch.ones_like(rstd)


def emu_split(x32):
    hi = bfr(x32.float())
    return hi + bfr(x32.float() - hi)


def emu_qkv(W, li, x32, ctx, form):
    cfg = W.cfg.llm
    exact = form == "exact"
    op, sc = emu_norm_operand(x32, W.layer(li, "input_layernorm"), cfg.rms_eps, form)
    B = x32.shape[0]
    lin = lambda name, heads: ((op @ W.layer(li, name).float().t()) * sc).view(B, heads, HEAD_DIM)
    q, k, v = lin("self_attn.q_proj", cfg.num_heads), lin("self_attn.k_proj", cfg.num_kv_heads), lin("self_attn.v_proj", cfg.num_kv_heads)
    cos, sin = rope_tables32(ctx, cfg.rope_theta)
    if exact:
        x24 = lambda t: ((t.float().view(torch.int32) + 0x80) & ~0xFF).view(torch.float32)   # the 24-bit cache: top 24 bits, rounded
        return rotate(q, cos, sin).reshape(B, -1), x24(rotate(k, cos, sin)), x24(v)
    q, k, v = bfr(q), bfr(k), bfr(v)
    return bfr(rotate(q, cos, sin)).reshape(B, -1), bfr(rotate(k, cos, sin)), v


def emu_merge(part, exact=False):
    p = part.float()
    m, l, o = p[..., 128], p[..., 129], p[..., :128]
    M = m.max(dim=-1, keepdim=True).values
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - M))
    den = (l * w).sum(-1)
    out = ((o * w[..., None]).sum(-2) * (1.0 / den)[..., None]).reshape(part.shape[0], -1)
    return emu_split(out) if exact else bfr(out)


def emu_oproj(W, li, x, exact=False):
    return (emu_split(x) if exact else x.float()) @ W.layer(li, "self_attn.o_proj").float().t()


def emu_gateup(W, li, x32, form):
    exact = form == "exact"
    op, sc = emu_norm_operand(x32, W.layer(li, "post_attention_layernorm"), W.cfg.llm.rms_eps, form)
    g = (op @ W.layer(li, "mlp.gate_proj").float().t()) * sc
    u = (op @ W.layer(li, "mlp.up_proj").float().t()) * sc
    y = torch.nn.functional.silu(g) * u
    return y if exact else bfr(y)


def emu_down(W, li, x, exact=False):
    return (emu_split(x) if exact else x.float())[:, :INTER] @ W.layer(li, "mlp.down_proj").float().t()


def emu_lmhead(W, x32, form):
    op, sc = emu_norm_operand(x32, W.get("model.norm.weight"), W.cfg.llm.rms_eps, form)
    return (op @ W.get("lm_head.weight").float().t()) * sc


def spread(got, ref, rtol):
    """the smallest atol_frac at which assert_elementwise(got, ref, rtol, atol_frac) passes"""
    g, r = got.double(), ref.double()
    return ((g - r).abs() - rtol * r.abs()).clamp_min(0).max().item() / r.pow(2).mean().sqrt().item()


# the (model, batch) inputs of the GPU tests: every batch of the routing table
BATCHES = {"G": [1, 2, 3, 8], "W": [5, 9, 16, 17, 32, 33, 64], "H": [3, 16, 32]}   # (H: fp8 weights only)


FORMS = ("f32", "mirror", "hf")
OUTPUTS = ("q", "k", "v", "gateup", "oproj_split", "oproj", "down", "lmhead")


def measure(form, fp8=False, models=("G", "W", "H"), quiet=False):
    """worst spread per output over every input the tests use, for one operand form ("exact": model G only)"""
    exact = form == "exact"
    rtol = X_RTOL if exact else RTOL
    worst = {k: 0.0 for k in OUTPUTS}
    rel = {k: 0.0 for k in OUTPUTS}

    def note(name, e, r):
        worst[name] = max(worst[name], spread(e, r, rtol))
        rel[name] = max(rel[name], ((e.double() - r.double()).abs().max() / r.double().abs().max()).item())

    for model in models:
        if (exact and model != "G") or (model == "H" and not fp8):
            continue
        cfg = make_cfg(model, fp8)
        hidden = MODELS[model][2]
        W = Weights(make_state_dict(model), cfg, fp8)
        Hq, Hkv = MODELS[model][:2]
        for B in BATCHES[model]:
            for li in range(LAYERS):
                h32, _ = hidden_rows(B, (B, li), hidden=hidden)
                ctx = ctx_rows(B, li)
                for name, e, r in zip("qkv", emu_qkv(W, li, h32, ctx, form), ref_qkv(W, li, h32, ctx)):
                    note(name, e, r)
                note("gateup", emu_gateup(W, li, h32, form), ref_gateup(W, li, h32))
                part = attn_partials(B, Hq, 8, (B, li))
                note("oproj_split", emu_oproj(W, li, emu_merge(part, exact), exact), ref_oproj(W, li, ref_merge(part)))
                x = attn_rows(B, Hq * HEAD_DIM, (B, li)) if not exact else attn_rows32(B, Hq * HEAD_DIM, (B, li))
                note("oproj", emu_oproj(W, li, x, exact), ref_oproj(W, li, x))
                a = act_rows(B, INTER_P, (B, li)) if not exact else act_rows32(B, INTER_P, (B, li))
                note("down", emu_down(W, li, a, exact), ref_down(W, li, a))
            h32, _ = hidden_rows(B, (B, 99), hidden=hidden)
            note("lmhead", emu_lmhead(W, h32, form), ref_lmhead(W, h32))
    if not quiet:
        print(f"form {form} fp8={fp8}: spread " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        print(f"form {form} fp8={fp8}: relerr " + "  ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    return worst, rel


if __name__ == "__main__":
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "emma-x_amd"))
    torch.set_num_threads(8)
    for f in FORMS:
        measure(f)
        measure(f, fp8=True)
    measure("exact")
