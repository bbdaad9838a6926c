"""References, inputs and bounds of tests/test_vision_stages_gpu.py.  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

As tests/prefill_stage_ref.py does for the LLM prefill, this module holds for every stage of the bf16 vision encode (csrc/vision.hip) and for
its glue kernels

  * a float64 REFERENCE of the documented operation -- the timm block and PatchEmbed, the processor's (u / 255 - mean) / std, the projector
    (tests/test_vision_stage_ref.py composes them over all blocks and compares with oracle.emmax_oracle, so they are the model's operations and
    not restatements of the kernels);
  * a float32 EMULATION that applies exactly the roundings the kernel sources document and nothing else;
  * the BOUNDS, each the figure that emulation measures against the reference on the GPU tests' own inputs (`python tests/vision_stage_ref.py`
    prints the measurement; tests/test_vision_stage_ref.py pins the table to it: every measurement at or below 1.05 x its entry and at least
    2 / 3 of it).  No figure here comes from a kernel's output.

The ops with one right answer are compared bit for bit: copy_rows, x_to_bf16 (round to nearest even, written out on the integer bits), both
planes of the HL gather, assemble_tokens (one fp32 add of two bf16 values, one rounding), the uint8 gather (bf16 of three fp32 operations),
the folded weight W' = bf16(W gamma).

The roundings (emma-x_amd/csrc):
  GEMM            gemm.hip: exact products of bf16 operands accumulated in fp32; v = (acc - mean ln_s) rstd + ln_c (plain: acc + bias), exact-erf
                  GELU (2.8e-7 absolute, the source says), x LayerScale, + the bf16 residual, ONE bf16 rounding.  The emulation accumulates
                  product by product in k order.
  LayerNorm       norm.hip: fp32 sum, mean, variance about the mean, rsqrt; bf16((x - mean) rstd w + b).
  row statistics  norm.hip: the same statistics alone, per lane over the row's 16-byte chunks, then a pairwise tree over the 64 lanes.
  ln_fold         norm.hip: W' = bf16(W gamma) (the product of two bf16 values is exact in fp32); ln_s = sum W', ln_c = sum W beta + bias in fp32,
                  per thread over k = tid + 256 i, a tree over each wave, then the four waves in order.
  gather          misc.hip / exact.hip: fl32(fl32(fl32((float)u / 255) - mean) / sd), bf16 of it; HL: hi = bf16(v), lo = bf16(v - hi).
  assemble        misc.hip: bf16(pe + pos) from bf16 pe (the patch GEMM's rounded output) and bf16 pos.

The bound of every GEMM-like stage:  |got - ref| <= e + RTOL (|ref| + e),  e = ORDER x PRE[case] x rms(ref) (+ GELU_ABS behind a GELU)
  PRE       the error of the emulation's fp32 value IN FRONT OF the final bf16 rounding, max over the elements in units of rms(ref).  It is the
            fp32 accumulation for a GEMM of exact bf16 inputs (~1e-7), and the bf16 rounding of a SECOND operand where a stage has one: the
            LayerNorm's output or the folded weight in qkv / fc1, the gathered pixels and the patch GEMM's output in embed (~1e-2).
  RTOL      2^-8: the one bf16 rounding of that value -- half an ulp of an 8-bit significand, of a value within e of the reference.
  ORDER     2: the kernel's summation order is not the emulation's (as in prefill_stage_ref.py).
  GELU_ABS  2.8e-7: gemm.hip's own figure for its erf.
Sums compared as fp32 (row statistics, ln_s, ln_c): ORDER x the emulation's error + 2^-24, the rounding of the result itself, which any order
of summation leaves (the emulation's order happens to be exact on some of the inputs).
"""

import math

import torch

from prefill_stage_ref import bf, bf16_bits_rne, bfr, bits16, gen  # noqa: F401  (re-exported for the tests)

RTOL = 2.0 ** -8
ORDER = 2.0
GELU_ABS = 2.8e-7
TOWER_PREFIXES = ("vision_backbone.featurizer.", "vision_backbone.fused_featurizer.")
B_MAX = 3                      # the GPU tests run B = 1 and 3: frames(B) are the first B of these
# a third tower's normalisation, used only by the pure gather op: every channel its own mean and std, far apart
ODD_MEAN, ODD_STD = (0.3, 0.5, 0.7), (0.2, 0.4, 0.8)


def cfg_tiny():
    from emmax.config import EmmaXConfig

    return EmmaXConfig.tiny()


def n_blocks(tw):
    return tw.take_index + 1


# ---- the discriminating state dict -----------------------------------------------------------------------------------------------------------
# synthetic_state_dict draws every LayerScale around 0.1, every bias around 0.01 and every prefix token around 0: its tensors can stand in
# for one another unnoticed.  Here every tensor of the vision path has a scale and a sign of its own (kind -> (offset, spread)), so that any
# mis-wiring moves a stage by orders of magnitude more than its bound (test_vision_stage_ref.py shows it on the CPU).
_VISION_KINDS = {
    "patch_embed.proj.bias": (0.8, 0.3), "norm1.weight": (1.5, 0.2), "norm1.bias": (0.5, 0.2), "norm2.weight": (0.6, 0.1), "norm2.bias": (-0.4, 0.2),
    "attn.qkv.bias": (0.7, 0.3), "attn.proj.bias": (-1.0, 0.3), "mlp.fc1.bias": (0.3, 0.3), "mlp.fc2.bias": (1.2, 0.3),
    "ls1.scale_factor": (0.1, 0.01), "ls2.scale_factor": (1.5, 0.15), "cls_token": (2.0, 0.3), "pos_embed": (0.0, 0.3),
    "fc1.bias": (0.4, 0.2), "fc2.bias": (-0.3, 0.2), "fc3.bias": (0.9, 0.2),
}


def state_dict(cfg=None, seed=7):
    """bf16-representable fp32 tensors under the real key names: the vision path's as described above, the LLM's from synthetic_state_dict"""
    from emmax.weights import param_shapes, synthetic_state_dict

    cfg = cfg or cfg_tiny()
    sd = synthetic_state_dict(cfg, seed=seed)
    for idx, (key, shape, kind) in enumerate(param_shapes(cfg)):
        if not (key.startswith("vision_backbone.") or key.startswith("projector.")):
            continue
        r = torch.randn(shape, generator=gen(97, seed, idx))
        tower1 = key.startswith(TOWER_PREFIXES[1])
        suffix = next((s for s in _VISION_KINDS if key.endswith(s)), None)
        if key.endswith("reg_token"):      # every register row its own constant: +0.7, -1.4, +2.1, -2.8
            off = torch.tensor([(j + 1) * 0.7 * (-1) ** j for j in range(shape[1])]).view(1, -1, 1)
            t = off + 0.3 * r
        elif suffix is not None:
            off, spread = _VISION_KINDS[suffix]
            t = (-off if tower1 and suffix.endswith("bias") else off) + spread * r    # tower 1's biases have the other sign
        else:                                # a matrix: unit-gain rows
            fan_in = math.prod(shape[1:])
            t = r * ((0.5 if key.endswith("qkv.weight") else 1.0) / math.sqrt(fan_in))
        sd[key] = t
    return {k: bfr(v.float()) for k, v in sd.items()}


def frames(B=B_MAX):
    """uint8 [B, 224, 224, 3]: smooth structure plus noise, every byte value present"""
    g = gen(101)
    yy, xx = torch.meshgrid(torch.arange(224.0), torch.arange(224.0), indexing="ij")
    out = []
    for b in range(B_MAX):
        chans = [127.5 + 90.0 * torch.sin(xx / (9.0 + 3 * c + b) + c) * torch.cos(yy / (11.0 + 2 * b - c)) + 25.0 * torch.randn(224, 224, generator=g) for c in range(3)]
        out.append(torch.stack(chans, -1))
    return torch.stack(out).round().clamp(0, 255).to(torch.uint8)[:B].contiguous()


def massive_rows(rows, D, seed):
    """token-like rows with a large common offset per row and massive channels, as test_gemm_with_layernorm_folded_in builds them; bf16 values"""
    g = gen(103, seed, rows, D)
    x = torch.randn(rows, D, generator=g) * 0.7 + 3.0 * torch.randn(rows, 1, generator=g)
    x[:, 5 % D] += 40.0
    x[::7, 100 % D] -= 25.0
    return bfr(x.float())


# ---- error measures ----------------------------------------------------------------------------------------------------------------------------
def rms(x):
    return x.double().pow(2).mean().sqrt().item()


def pre_err(v, ref):
    """max |v - ref| in units of rms(ref): the emulation's value in front of its last rounding against the reference"""
    g, r = v.double(), ref.double()
    return ((g - r).abs().max() / r.pow(2).mean().sqrt()).item()


def allowed(ref, entry, act=False):
    """the element-wise bound of a GEMM-like stage (module docstring)"""
    r = ref.double()
    e = ORDER * entry * r.pow(2).mean().sqrt() + (GELU_ABS if act else 0.0)
    return e + RTOL * (r.abs() + e)


F32_HALF_ULP = 2.0 ** -24


def sum_bound(entry):
    """the bound of a sum kept as fp32, in the units of its entry"""
    return ORDER * entry + F32_HALF_ULP


def worst(got, ref, entry, act=False):
    """max |err| / allowed: <= 1 passes"""
    return ((got.double() - ref.double()).abs() / allowed(ref, entry, act)).max().item()


# ---- the gather ----------------------------------------------------------------------------------------------------------------------------------
def patches_of(img_bchw, patch):
    """[B, C, H, W] -> [B (H / p) (W / p), C p p] in conv-weight order k = c p^2 + dy p + dx, patches row-major"""
    B, C, H, W = img_bchw.shape
    gp = H // patch
    x = img_bchw.reshape(B, C, gp, patch, gp, patch).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B * gp * gp, C * patch * patch)


def ref_normalize(u8_bhwc, mean, std):
    """float64 [B, 3, H, W] = (u / 255 - mean) / std, the processor's to_tensor + normalize"""
    x = u8_bhwc.permute(0, 3, 1, 2).double() / 255.0
    return (x - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)


def emu_normalize(u8_bhwc, mean, std):
    """fp32, the three operations one by one on fp32 constants (torch divides and subtracts with correct rounding)"""
    x = u8_bhwc.permute(0, 3, 1, 2).to(torch.float32) / torch.tensor(255.0, dtype=torch.float32)
    x = x - torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    return x / torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)


def pad_cols(x, kpad):
    out = torch.zeros(x.shape[0], kpad, dtype=x.dtype)
    out[:, : x.shape[1]] = x
    return out


def gather_u8_bits(u8_bhwc, patch, kpad, mean, std):
    """the bf16 gather of uint8 frames, exact: int16 bit patterns [B gp^2, kpad]"""
    return bf16_bits_rne(pad_cols(patches_of(emu_normalize(u8_bhwc, mean, std), patch), kpad))


def hl_split(v32):
    """fp32 -> (hi, lo) bf16 bit patterns: hi = bf16(v), lo = bf16(v - hi), the subtraction exact in fp32"""
    hi = bf16_bits_rne(v32)
    lo = bf16_bits_rne(v32 - hi.view(torch.bfloat16).float())
    return hi, lo


def hl_rows(v32):
    """[rows, kpad] fp32 -> the HL image [rows, 2 kpad] as bit patterns: per 64 elements, 64 hi then 64 lo"""
    hi, lo = hl_split(v32)
    rows, k = v32.shape
    return torch.stack([hi.view(rows, k // 64, 64), lo.view(rows, k // 64, 64)], 2).reshape(rows, 2 * k)


def ref_assemble_bits(pe, pos, cls, reg, B, has_cls, f32=False):
    """tokens [B, has_cls + n_reg + np, D]: bit patterns (bf16 form: one fp32 add of two bf16 values, one rounding) or fp32 values (exact form)"""
    n_p, D = pos.shape
    body = pe.float().view(B, n_p, D) + pos.float()
    pre = ([cls.float().view(1, 1, D).expand(B, 1, D)] if has_cls else []) + ([reg.float().view(1, -1, D).expand(B, -1, D)] if reg is not None else [])
    t = torch.cat(pre + [body], 1)
    return t if f32 else bf16_bits_rne(t)


# ---- row statistics and the LayerNorm fold ---------------------------------------------------------------------------------------------------------
def lane_tree(v):
    """the wave's reduction: a pairwise tree over the last axis (64 lanes, or the 4 x 16 of wave_sum: the same tree)"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def ref_row_stats(x, eps):
    """float64 (mean, rsqrt(var + eps)), variance about the mean"""
    x = x.double()
    mean = x.mean(-1)
    return mean, torch.rsqrt((x - mean[:, None]).pow(2).mean(-1) + eps)


def emu_row_stats(x, eps):
    """fp32 in the kernel's order: lane l holds chunks l, l + 64, ..; per chunk s += x[2 j] + x[2 j + 1]; a tree over the lanes"""
    rows, D = x.shape
    nch = D // 8
    nv = -(-nch // 64)
    xp = torch.zeros(rows, nv * 64 * 8, dtype=torch.float32)
    xp[:, :D] = x.float()
    xp = xp.view(rows, nv, 64, 4, 2)
    valid = (torch.arange(nv * 64 * 8) < D).view(1, nv, 64, 4, 2)
    s = torch.zeros(rows, 64)
    for i in range(nv):
        for j in range(4):
            s = s + (xp[:, i, :, j, 0] + xp[:, i, :, j, 1])
    mean = lane_tree(s) / torch.tensor(float(D))
    d = torch.where(valid, xp - mean.view(rows, 1, 1, 1, 1), torch.zeros(()))
    vs = torch.zeros(rows, 64)
    for i in range(nv):
        for j in range(4):
            vs = vs + (d[:, i, :, j, 0] * d[:, i, :, j, 0] + d[:, i, :, j, 1] * d[:, i, :, j, 1])
    return mean, torch.rsqrt(lane_tree(vs) / torch.tensor(float(D)) + torch.tensor(eps, dtype=torch.float32))


def stats_err(mean, rstd, x, eps):
    """(error of the mean in units of the row's rms, relative error of rstd): maxima over the rows"""
    m64, r64 = ref_row_stats(x, eps)
    row_rms = x.double().pow(2).mean(-1).sqrt().clamp_min(1e-30)
    return ((mean.double() - m64).abs() / row_rms).max().item(), ((rstd.double() - r64).abs() / r64).max().item()


def fold_bits(W, gamma):
    """W' = bf16(W gamma): the product is exact in fp32, one rounding"""
    return bf16_bits_rne(W.float() * gamma.float())


def ref_fold_sums(W, gamma, beta, bias):
    """float64 ln_s (over the ROUNDED W', which is what the GEMM multiplies by) and ln_c"""
    Wf = fold_bits(W, gamma).view(torch.bfloat16).double()
    c = (W.double() * beta.double()).sum(-1) if beta is not None else torch.zeros(W.shape[0], dtype=torch.float64)
    return Wf.sum(-1), c + (bias.double() if bias is not None else 0.0)


def emu_fold_sums(W, gamma, beta, bias):
    N, K = W.shape
    n = -(-K // 256)
    Wf = torch.zeros(N, n * 256)
    Wf[:, :K] = fold_bits(W, gamma).view(torch.bfloat16).float()
    Wb = torch.zeros(N, n * 256)
    if beta is not None:
        Wb[:, :K] = W.float() * beta.float()
    s, c = torch.zeros(N, 256), torch.zeros(N, 256)
    for i in range(n):
        s = s + Wf[:, i * 256:(i + 1) * 256]
        c = c + Wb[:, i * 256:(i + 1) * 256]
    out = []
    for v in (s, c):
        w4 = lane_tree(v.view(N, 4, 64))
        out.append(((w4[:, 0] + w4[:, 1]) + w4[:, 2]) + w4[:, 3])
    return out[0], out[1] + (bias.float() if bias is not None else 0.0)


def fold_err(got_s, got_c, W, gamma, beta, bias):
    """errors of ln_s and ln_c in units of the sum of the magnitudes of their terms: maxima over the rows"""
    rs, rc = ref_fold_sums(W, gamma, beta, bias)
    Wf = fold_bits(W, gamma).view(torch.bfloat16).double()
    l1s = Wf.abs().sum(-1).clamp_min(1e-30)
    l1c = ((W.double() * beta.double()).abs().sum(-1) if beta is not None else torch.zeros_like(rc)) + (bias.double().abs() if bias is not None else 0.0)
    return ((got_s.double() - rs).abs() / l1s).max().item(), ((got_c.double() - rc).abs() / l1c.clamp_min(1e-30)).max().item()


def fold_case(N, K, seed):
    g = gen(107, seed, N, K)
    W = bfr(torch.randn(N, K, generator=g) / math.sqrt(K))
    gamma = bfr(1.5 + 0.2 * torch.randn(K, generator=g))
    beta = bfr(0.5 + 0.2 * torch.randn(K, generator=g))
    bias = bfr(0.7 + 0.3 * torch.randn(N, generator=g))
    return W, gamma, beta, bias


# ---- the stages: float64 references ------------------------------------------------------------------------------------------------------------------
def _w(sd, key, dt):
    return sd[key].to(dt)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, w, b, eps):
    mean = x.mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt((x - mean).pow(2).mean(-1, keepdim=True) + eps) * w + b


def ref_embed(img, sd, t, tw, dt=torch.float64):
    """img [B, 3, H, W] normalised pixels -> tokens [B N, D]: PatchEmbed (a conv with stride = kernel = a GEMM over the patches), + pos_embed on the
    patch tokens only, cls then the registers in front (timm _pos_embed, no_embed_class)"""
    p = TOWER_PREFIXES[t]
    B, D = img.shape[0], tw.embed_dim
    A = patches_of(img.to(dt), tw.patch)
    pe = A @ _w(sd, p + "patch_embed.proj.weight", dt).reshape(D, -1).t() + _w(sd, p + "patch_embed.proj.bias", dt)
    tok = pe.view(B, tw.n_patches, D) + _w(sd, p + "pos_embed", dt)
    pre = ([_w(sd, p + "cls_token", dt).expand(B, -1, -1)] if tw.has_cls else []) + ([_w(sd, p + "reg_token", dt).expand(B, -1, -1)] if tw.n_reg else [])
    return torch.cat(pre + [tok], 1).reshape(B * tw.n_tokens, D)


def ref_qkv(tok, sd, t, i, tw, dt=torch.float64):
    p = f"{TOWER_PREFIXES[t]}blocks.{i}."
    h = layer_norm(tok.to(dt), _w(sd, p + "norm1.weight", dt), _w(sd, p + "norm1.bias", dt), tw.ln_eps)
    return h @ _w(sd, p + "attn.qkv.weight", dt).t() + _w(sd, p + "attn.qkv.bias", dt)


def ref_attn(qkv, tw, dt=torch.float64):
    """qkv [B N, 3 D] -> [B N, D]: softmax(q k^T / sqrt(hd)) v per frame and head"""
    N, D, H = tw.n_tokens, tw.embed_dim, tw.num_heads
    hd = D // H
    x = qkv.to(dt).view(-1, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    att = ((x[0] * hd ** -0.5) @ x[1].transpose(-2, -1)).softmax(-1)
    return (att @ x[2]).transpose(1, 2).reshape(-1, D)


def ref_proj(att, tok, sd, t, i, tw, dt=torch.float64):
    p = f"{TOWER_PREFIXES[t]}blocks.{i}."
    a = att.to(dt) @ _w(sd, p + "attn.proj.weight", dt).t() + _w(sd, p + "attn.proj.bias", dt)
    if tw.layerscale:
        a = a * _w(sd, p + "ls1.scale_factor", dt)
    return tok.to(dt) + a


def ref_fc1(tok, sd, t, i, tw, dt=torch.float64):
    p = f"{TOWER_PREFIXES[t]}blocks.{i}."
    h = layer_norm(tok.to(dt), _w(sd, p + "norm2.weight", dt), _w(sd, p + "norm2.bias", dt), tw.ln_eps)
    return gelu(h @ _w(sd, p + "mlp.fc1.weight", dt).t() + _w(sd, p + "mlp.fc1.bias", dt))


def ref_fc2(mlp, tok, sd, t, i, tw, dt=torch.float64):
    p = f"{TOWER_PREFIXES[t]}blocks.{i}."
    f = mlp.to(dt) @ _w(sd, p + "mlp.fc2.weight", dt).t() + _w(sd, p + "mlp.fc2.bias", dt)
    if tw.layerscale:
        f = f * _w(sd, p + "ls2.scale_factor", dt)
    return tok.to(dt) + f


def ref_features(tok, feats, t, cfg):
    """the tower's patch rows (prefix dropped, no final norm) into its column range of the feature rows [B np, V]"""
    tw = cfg.towers[t]
    col = sum(x.embed_dim for x in cfg.towers[:t])
    out = feats.clone()
    out.view(-1, tw.n_patches, out.shape[-1])[:, :, col:col + tw.embed_dim] = tok.view(-1, tw.n_tokens, tw.embed_dim)[:, tw.n_prefix:].to(out.dtype)
    return out


def ref_pj(k, x, sd, dt=torch.float64):
    """projector layer k = 1, 2, 3: fc3(gelu(fc2(gelu(fc1(x)))))"""
    y = x.to(dt) @ _w(sd, f"projector.fc{k}.weight", dt).t() + _w(sd, f"projector.fc{k}.bias", dt)
    return gelu(y) if k < 3 else y


def chain(sd, cfg, frames_u8):
    """the float64 reference chain over all blocks and the projector; every activation by name: (t, 'tok'), (t, i, 'qkv' | 'att' | 'tok1' | 'mlp' |
    'tok2'), 'feats', 'pj1', 'pj2', 'pj3'.  (t, i, 'tok0') is block i's input."""
    act = {}
    B = frames_u8.shape[0]
    feats = torch.zeros(B * cfg.n_patches, cfg.vision_dim, dtype=torch.float64)
    for t, tw in enumerate(cfg.towers):
        tok = ref_embed(ref_normalize(frames_u8, tw.mean, tw.std), sd, t, tw)
        act[(t, "tok")] = tok
        for i in range(n_blocks(tw)):
            act[(t, i, "tok0")] = tok
            act[(t, i, "qkv")] = ref_qkv(tok, sd, t, i, tw)
            act[(t, i, "att")] = ref_attn(act[(t, i, "qkv")], tw)
            act[(t, i, "tok1")] = ref_proj(act[(t, i, "att")], tok, sd, t, i, tw)
            act[(t, i, "mlp")] = ref_fc1(act[(t, i, "tok1")], sd, t, i, tw)
            tok = act[(t, i, "tok2")] = ref_fc2(act[(t, i, "mlp")], act[(t, i, "tok1")], sd, t, i, tw)
        act[(t, "out")] = tok
        feats = ref_features(tok, feats, t, cfg)
    act["feats"] = feats
    act["pj1"] = ref_pj(1, feats, sd)
    act["pj2"] = ref_pj(2, act["pj1"], sd)
    act["pj3"] = ref_pj(3, act["pj2"], sd)
    return act


# ---- the stages: fp32 emulations ------------------------------------------------------------------------------------------------------------------------
def emu_dot(A, W):
    """fp32 A W^T of bf16 values, the products one by one in k order (each step one rounding)"""
    a, w = A.float(), W.float()
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k in range(a.shape[1]):
        acc.addcmul_(a[:, k:k + 1], w[:, k][None, :])
    return acc


def emu_epilogue(acc, bias=None, act=False, scale=None, res=None, stats=None, ln_s=None, ln_c=None, rounded=True):
    """gemm.hip: v = (acc - mean ln_s) rstd + ln_c (plain: acc + bias); GELU; x scale; + residual; one bf16 rounding (rounded = False: v itself)"""
    if stats is not None:
        v = (acc - stats[0][:, None] * ln_s[None, :]) * stats[1][:, None] + ln_c[None, :]
    else:
        v = acc + (bias.float() if bias is not None else 0.0)
    if act:
        v = gelu(v)
    if scale is not None:
        v = v * scale.float()
    if res is not None:
        v = v + res.float()
    return bfr(v) if rounded else v


def emu_layernorm(x, w, b, eps):
    mean, rstd = emu_row_stats(x, eps)
    return bfr((x.float() - mean[:, None]) * rstd[:, None] * w.float() + b.float())


def emu_ln_gemm(x, W, gamma, beta, bias, eps, folded, act=False, rounded=True):
    if folded:
        s, c = emu_fold_sums(W, gamma, beta, bias)
        return emu_epilogue(emu_dot(x, fold_bits(W, gamma).view(torch.bfloat16)), act=act, stats=emu_row_stats(x, eps), ln_s=s, ln_c=c, rounded=rounded)
    return emu_epilogue(emu_dot(emu_layernorm(x, gamma, beta, eps), W), bias=bias, act=act, rounded=rounded)


def emu_embed(frames_u8, sd, t, tw, rounded=True):
    p = TOWER_PREFIXES[t]
    B, D = frames_u8.shape[0], tw.embed_dim
    A = gather_u8_bits(frames_u8, tw.patch, 3 * tw.patch ** 2, tw.mean, tw.std).view(torch.bfloat16)
    pe = emu_epilogue(emu_dot(A, sd[p + "patch_embed.proj.weight"].reshape(D, -1)), bias=sd[p + "patch_embed.proj.bias"])
    tok = ref_assemble_bits(pe, sd[p + "pos_embed"].view(-1, D), sd.get(p + "cls_token"), sd.get(p + "reg_token"), B, 1 if tw.has_cls else 0, f32=True)
    return (bfr(tok) if rounded else tok).reshape(B * tw.n_tokens, D)


def emu_stage(stage, sd, cfg, t, i, x, tok=None, folded=True, rounded=True):
    """the emulation of one stage on the (bf16) inputs the GPU test hands the op"""
    tw = cfg.towers[t] if t is not None else None
    if stage in ("pj1", "pj2", "pj3"):
        k = int(stage[2])
        return emu_epilogue(emu_dot(x, sd[f"projector.fc{k}.weight"]), bias=sd[f"projector.fc{k}.bias"], act=k < 3, rounded=rounded)
    p = f"{TOWER_PREFIXES[t]}blocks.{i}."
    if stage == "qkv":
        return emu_ln_gemm(x, sd[p + "attn.qkv.weight"], sd[p + "norm1.weight"], sd[p + "norm1.bias"], sd[p + "attn.qkv.bias"], tw.ln_eps, folded, rounded=rounded)
    if stage == "fc1":
        return emu_ln_gemm(x, sd[p + "mlp.fc1.weight"], sd[p + "norm2.weight"], sd[p + "norm2.bias"], sd[p + "mlp.fc1.bias"], tw.ln_eps, folded, act=True, rounded=rounded)
    if stage == "proj":
        return emu_epilogue(emu_dot(x, sd[p + "attn.proj.weight"]), bias=sd[p + "attn.proj.bias"], scale=sd.get(p + "ls1.scale_factor") if tw.layerscale else None, res=tok, rounded=rounded)
    if stage == "fc2":
        return emu_epilogue(emu_dot(x, sd[p + "mlp.fc2.weight"]), bias=sd[p + "mlp.fc2.bias"], scale=sd.get(p + "ls2.scale_factor") if tw.layerscale else None, res=tok, rounded=rounded)
    raise ValueError(stage)


def ref_stage(stage, sd, cfg, t, i, x, tok=None):
    tw = cfg.towers[t] if t is not None else None
    if stage in ("pj1", "pj2", "pj3"):
        return ref_pj(int(stage[2]), x, sd)
    return {"qkv": lambda: ref_qkv(x, sd, t, i, tw), "fc1": lambda: ref_fc1(x, sd, t, i, tw), "proj": lambda: ref_proj(x, tok, sd, t, i, tw),
            "fc2": lambda: ref_fc2(x, tok, sd, t, i, tw), "attn": lambda: ref_attn(x, tw)}[stage]()


# ---- the cases of the GPU tests and their inputs -------------------------------------------------------------------------------------------------------
def stage_inputs(act, stage, t, i, B, cfg):
    """(x, tok) of a stage: the bf16 roundings of the reference chain's own activations, the first B frames' rows"""
    if stage in ("pj1", "pj2", "pj3"):
        src = {"pj1": "feats", "pj2": "pj1", "pj3": "pj2"}[stage]
        return bfr(act[src][: B * cfg.n_patches].float()), None
    rows = B * cfg.towers[t].n_tokens
    x = {"qkv": "tok0", "attn": "qkv", "proj": "att", "fc1": "tok1", "fc2": "mlp"}[stage]
    tok = {"proj": "tok0", "fc2": "tok1"}.get(stage)
    return bfr(act[(t, i, x)][:rows].float()), (bfr(act[(t, i, tok)][:rows].float()) if tok else None)


def stage_cases(cfg):
    """every bounded (stage, tower, block, form) of the GPU tests; form: 'fold' / 'ln' for qkv and fc1 (how the model was finalized), else ''"""
    out = []
    for t, tw in enumerate(cfg.towers):
        out.append(("embed", t, 0, ""))
        for i in (0, n_blocks(tw) - 1):
            for stage in ("qkv", "fc1"):
                out += [(stage, t, i, "fold"), (stage, t, i, "ln")]
            out += [("proj", t, i, ""), ("fc2", t, i, "")]
        for stage in ("qkv", "fc1"):
            out += [(stage + "_massive", t, 0, "fold"), (stage + "_massive", t, 0, "ln")]
    return out + [("pj1", None, 0, ""), ("pj2", None, 0, ""), ("pj3", None, 0, "")]


MASSIVE_ROWS = 261   # one frame's worth of token rows for the massive-channel inputs of qkv and fc1


def case_io(case, sd, cfg, act, B=B_MAX):
    """(inputs x, tok, float64 reference) of a bounded case at B frames"""
    stage, t, i, form = case
    if stage == "embed":
        tw = cfg.towers[t]
        return frames(B), None, ref_embed(ref_normalize(frames(B), tw.mean, tw.std), sd, t, tw)
    if stage.endswith("_massive"):
        x = massive_rows(MASSIVE_ROWS if t == 0 else 256, cfg.towers[t].embed_dim, (t, stage == "fc1_massive"))
        return x, None, ref_stage(stage[:-8], sd, cfg, t, i, x)
    x, tok = stage_inputs(act, stage, t, i, B, cfg)
    return x, tok, ref_stage(stage, sd, cfg, t, i, x, tok)


def measure_case(case, sd, cfg, act):
    stage, t, i, form = case
    x, tok, ref = case_io(case, sd, cfg, act)
    if stage == "embed":
        return pre_err(emu_embed(x, sd, t, cfg.towers[t], rounded=False), ref)
    return pre_err(emu_stage(stage.replace("_massive", ""), sd, cfg, t, i, x, tok, folded=form == "fold", rounded=False), ref)


# PRE[case]: what the emulation measures on the case's inputs at B = 3 (`python tests/vision_stage_ref.py`)
PRE = {
    ('embed', 0, 0, ''): 0.015,
    ('qkv', 0, 0, 'fold'): 0.006,
    ('qkv', 0, 0, 'ln'): 0.006,
    ('fc1', 0, 0, 'fold'): 0.008,
    ('fc1', 0, 0, 'ln'): 0.0095,
    ('proj', 0, 0, ''): 2.1e-07,
    ('fc2', 0, 0, ''): 7.5e-07,
    ('qkv', 0, 2, 'fold'): 0.0052,
    ('qkv', 0, 2, 'ln'): 0.0062,
    ('fc1', 0, 2, 'fold'): 0.0066,
    ('fc1', 0, 2, 'ln'): 0.0093,
    ('proj', 0, 2, ''): 1.2e-07,
    ('fc2', 0, 2, ''): 2.4e-07,
    ('qkv_massive', 0, 0, 'fold'): 0.0053,
    ('qkv_massive', 0, 0, 'ln'): 0.0095,
    ('fc1_massive', 0, 0, 'fold'): 0.0096,
    ('fc1_massive', 0, 0, 'ln'): 0.011,
    ('embed', 1, 0, ''): 0.011,
    ('qkv', 1, 0, 'fold'): 0.0057,
    ('qkv', 1, 0, 'ln'): 0.0066,
    ('fc1', 1, 0, 'fold'): 0.013,
    ('fc1', 1, 0, 'ln'): 0.017,
    ('proj', 1, 0, ''): 6.5e-07,
    ('fc2', 1, 0, ''): 3.9e-07,
    ('qkv', 1, 2, 'fold'): 0.0049,
    ('qkv', 1, 2, 'ln'): 0.0064,
    ('fc1', 1, 2, 'fold'): 0.0096,
    ('fc1', 1, 2, 'ln'): 0.018,
    ('proj', 1, 2, ''): 4.3e-07,
    ('fc2', 1, 2, ''): 2.8e-07,
    ('qkv_massive', 1, 0, 'fold'): 0.0045,
    ('qkv_massive', 1, 0, 'ln'): 0.0062,
    ('fc1_massive', 1, 0, 'fold'): 0.0087,
    ('fc1_massive', 1, 0, 'ln'): 0.016,
    ('pj1', None, 0, ''): 3.6e-06,
    ('pj2', None, 0, ''): 6.6e-06,
    ('pj3', None, 0, ''): 1.7e-06,
}

# row statistics: D -> (error of the mean in units of the row's rms, relative error of rstd), the emulation on stats_rows(261, D) -- token-like
# rows with a common offset and massive channels; asserted with ORDER on the device
STATS_DS = (8, 144, 1024, 1152, 2048, 4096, 8192)
STATS = {
    8: (0.0, 1.3e-07),
    144: (4.9e-08, 2e-07),
    1024: (5.7e-08, 1.5e-07),
    1152: (7.6e-08, 1.7e-07),
    2048: (8.6e-08, 1.5e-07),
    4096: (8.1e-08, 1.7e-07),
    8192: (9.6e-08, 3.5e-07),
}
# ln_fold: (N, K) -> (ln_s, ln_c) errors in units of the sum of the magnitudes of the terms
FOLD_SHAPES = ((384, 128), (432, 144), (8, 1152))
FOLD = {
    (384, 128): (0.0, 2.3e-08),
    (432, 144): (8.6e-09, 3.1e-08),
    (8, 1152): (0.0, 4.6e-09),
}


def stats_rows(rows, D, seed=0):
    return massive_rows(rows, D, (5, seed))


def measure_stats(D, eps=1e-6):
    x = stats_rows(261, D)
    m, r = emu_row_stats(x, eps)
    return stats_err(m, r, x, eps)


def measure_fold(N, K):
    W, gamma, beta, bias = fold_case(N, K, 0)
    return fold_err(*emu_fold_sums(W, gamma, beta, bias), W, gamma, beta, bias)


def measure_all():
    cfg = cfg_tiny()
    sd = state_dict(cfg)
    act = chain(sd, cfg, frames())
    return ({c: measure_case(c, sd, cfg, act) for c in stage_cases(cfg)}, {D: measure_stats(D) for D in STATS_DS}, {s: measure_fold(*s) for s in FOLD_SHAPES})


if __name__ == "__main__":
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "emma-x_amd")]
    sp, st, fo = measure_all()
    print("PRE = {")
    for c, v in sp.items():
        print(f"    {c!r}: {v:.3g},")
    print("}\nSTATS = {")
    for D, (a, b) in st.items():
        print(f"    {D}: ({a:.3g}, {b:.3g}),")
    print("}\nFOLD = {")
    for s, (a, b) in fo.items():
        print(f"    {s!r}: ({a:.3g}, {b:.3g}),")
    print("}")
