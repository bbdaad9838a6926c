"""References, inputs and bounds of tests/test_prefill_stages_gpu.py.  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

As tests/decode_stage_ref.py does for the decode step, this module holds for every stage kernel of the LLM prefill

  * a float64 REFERENCE of the documented operation (tests/test_prefill_stage_ref.py ties RoPE, RMSNorm and the splice to the oracle, so
    the reference is the model's operation and not a restatement of the kernel);
  * a float32 EMULATION that applies exactly the roundings the kernel sources document and nothing else;
  * the BOUNDS, each the figure that emulation measures against the reference on the tests' own inputs, written next to the case that
    measures it (`python tests/prefill_stage_ref.py` prints the measurement; tests/test_prefill_stage_ref.py pins the table to it: every
    measurement at or below 1.05 x its entry and at least 2 / 3 of it).  No figure here comes from a kernel's output.

The ops with one right answer have exact references and are compared bit for bit: embed / splice, the last-row gather (round to nearest
even, written out on the integer bits), the fp8 KV append (e4m3 bytes, power-of-two scales, the rows written back), the paged K / V append.

The roundings (emma-x_amd/csrc):
  fp32-stream GEMM   gemm.hip: exact products of bf16 operands accumulated in fp32, (acc + bias) * scale in fp32, ONE fp32 add of the fp32 residual.
                     The emulation accumulates product by product in k order -- K roundings, the most-rounded order a kernel can take (MFMA
                     blocks and split-K slices round less often).
  RMSNorm, fp32 rows norm.hip: fp32 sum of squares and rsqrt, bf16(bf16(x rstd) w) -- HF LlamaRMSNorm on an fp32 hidden state: two bf16 roundings.
  RoPE               misc.hip: y0 = fma(x0, c, -fl32(x1 s)), y1 = fma(x0, s, fl32(x1 c)) on fp32 table values, ONE bf16 rounding.
"""

import math

import torch

PAGE = 64
SEQ_LENS = [63, 64, 65, 1, 130]      # one slot short of a page, a whole page, one slot into the second, a single token, two pages and two slots
THETA = 10000.0


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


def bf(x):
    return x.to(torch.bfloat16)


def bfr(x):
    """round to bf16 and back: the value a bf16 store keeps"""
    return x.to(torch.bfloat16).to(x.dtype)


def fl32(x):
    """round a float64 value to fp32 and back"""
    return x.to(torch.float32).to(torch.float64)


def bf16_bits_rne(x32):
    """fp32 -> the bf16 bit pattern (int16), round to nearest, ties to even, on the integer bits: no library conversion involved.
    Finite inputs only (a carry out of the mantissa moves the exponent up, as it must)."""
    u = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (r & 0xFFFF).to(torch.int32).to(torch.int16)   # (wraps to the signed pattern)


def bits16(t):
    """the 16-bit patterns of a bf16 tensor"""
    return t.contiguous().view(torch.int16)


def scaled_err(got, ref, floor=2.0 ** -12):
    """max over the elements of |err| / (|ref| + floor x rms(ref)): a RELATIVE error per element, with an absolute allowance only for
    elements below rms / 4096 (there the fp32 arithmetic in front of the bf16 rounding -- 2^-24 of the terms -- is no longer small against
    2^-8 of the result)"""
    g, r = got.double(), ref.double()
    return ((g - r).abs() / (r.abs() + floor * r.pow(2).mean().sqrt())).max().item()


# ---- the fp32 residual stream ---------------------------------------------------------------------------------------------------------------
def stream_rows(M, n, seed):
    """fp32 stream rows as a prefill holds them: N(0, 30^2) with three massive channels of +-200; not bf16-representable"""
    g = gen(41, seed)
    x = torch.randn(M, n, generator=g) * 30.0
    for c in sorted({1 % n, n // 3, n - 2}):
        x[:, c] = torch.sign(torch.randn(M, generator=g)) * 200.0 + torch.randn(M, generator=g)
    return x.float()


def gemm_operands(M, N, K, seed):
    """A [M, K], W [N, K] bf16 scaled so that A W^T has rms ~ 1; bias and LayerScale-like scale bf16 [N]"""
    g = gen(43, seed)
    A = bf(torch.randn(M, K, generator=g))
    W = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    bias = bf(torch.randn(N, generator=g) * 0.5)
    scale = bf(torch.rand(N, generator=g) + 0.5)
    return A, W, bias, scale


def ref_gemm_stream(A, W, res, bias=None, scale=None):
    """float64: res + scale .* (A W^T + bias).  Runs on whatever device the operands live on."""
    p = A.double() @ W.double().t()
    if bias is not None:
        p = p + bias.double()
    if scale is not None:
        p = p * scale.double()
    return res.double() + p[:, : res.shape[1]]   # (a stream narrower than N: the columns that are stored)


def emu_gemm_term(A, W, bias=None, scale=None):
    """fp32: the products one by one in k order (a product of two bf16 values is exact in fp32: each step is one rounding), the epilogue in the
    kernel's order -- the term the stream takes, before the residual is added"""
    a, w = A.float(), W.float()
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k in range(a.shape[1]):
        acc.addcmul_(a[:, k:k + 1], w[:, k][None, :])
    if bias is not None:
        acc = acc + bias.float()
    if scale is not None:
        acc = acc * scale.float()
    return acc


# |got - ref| <= GEMM_RTOL |ref| + atol, atol = GEMM_ORDER x GEMM_SPREAD[K] x rms(A W^T term).
#   GEMM_RTOL   2^-24: the one fp32 add of the residual, correctly rounded, is half an ulp of the result.
#   GEMM_SPREAD what the product-by-product emulation leaves above that, in units of the rms of the product term (measure_gemm) -- the
#               accumulation, ~ sqrt(K) 2^-24 of the partial sums.  It is a maximum over the elements, and only the elements whose residual is
#               near zero count (elsewhere 2^-24 |ref| covers the error), so it grows with the number of elements and with the largest
#               term among them: it is measured on GEMM_CASE[K], the very inputs (shape, seed, epilogue) of the largest GPU case at that K,
#               not on a sample of another size.  (A 64 x 256 sample with bias and scale measures 2.33e-7 at K = 64 where the emulation on
#               the row-split case's own 11 M elements measures 7.15e-7.)
#               One entry per K, from the largest case, also bounds the smaller cases at that K: a maximum over the few hundred countable
#               elements of an M <= 7 case is one draw of a wide distribution, and another summation order is another draw -- a factor of 2
#               on such a figure would bound sampling noise, not the arithmetic.  The largest case's maximum is the stable one.
#   GEMM_ORDER  2: the kernel's summation order is not the emulation's.
# A residual that took one trip through bf16 is off by up to 2^-8 of its magnitude (0.5 at the +-200 channels): the same measurement with a bf16-rounded residual (second column
# below; units of the product rms) is 10^4 .. 10^5 times the bound, which tests/test_prefill_stage_ref.py asserts.
GEMM_RTOL = 2.0 ** -24
GEMM_ORDER = 2.0
GEMM_CASE = {   # K: (M, N, bias and scale) of the largest case of tests/test_prefill_stages_gpu.py at that K, seed 0
    64: (257, 43776, False),     # the row split
    128: (32768, 1152, True),    # the column split
    192: (300, 384, True),       # big and k32 tiles
    512: (7, 4096, True),        # the fused norm
    640: (300, 384, True),       # three K slices
    2048: (7, 4096, False),      # the fused norm through the launch plan
    4352: (261, 1024, True),     # eight K slices
}
GEMM_SPREAD = {   # K: measured spread            (bf16-rounded residual)
    64: 7.15e-7,     #                               0.50
    128: 1.28e-6,    #                               0.43
    192: 1.13e-6,    #                               0.45
    512: 1.47e-6,    #                               0.41
    640: 2.04e-6,    #                               0.42
    2048: 3.48e-6,   #                               0.48
    4352: 8.31e-6,   #                               0.43
}


def gemm_spread(got, ref, res):
    """the smallest atol, in units of rms(ref - res), at which |got - ref| <= GEMM_RTOL |ref| + atol holds everywhere"""
    g, r = got.double(), ref.double()
    unit = (r - res.double()).pow(2).mean().sqrt()
    return (((g - r).abs() - GEMM_RTOL * r.abs()).clamp_min(0).max() / unit).item()


def gemm_atol(K):
    return GEMM_ORDER * GEMM_SPREAD[K]


def measure_gemm(K):
    """(spread of the emulation, spread of the emulation fed a bf16-rounded residual) on the inputs of GEMM_CASE[K]"""
    M, N, epi = GEMM_CASE[K]
    A, W, bias, scale = gemm_operands(M, N, K, (M, N, K, 0))
    if not epi:
        bias = scale = None
    res = stream_rows(M, N, (M, N, K, 0))
    ref = ref_gemm_stream(A, W, res, bias, scale)
    term = emu_gemm_term(A, W, bias, scale)
    return gemm_spread(term + res, ref, res), gemm_spread(term + bfr(res), ref, res)


# ---- RMSNorm of fp32 rows ---------------------------------------------------------------------------------------------------------------------
NORM_ROWS = (1, 5, 261)
NORM_DIMS = (64, 520, 1152, 2048, 4096, 8192)   # one per MAXV instantiation of the kernel (1, 2, 4, 4, 8, 16); 520: the last 64-chunk step is partly empty
NORM_EPS = 1e-5
# scaled_err(got, ref) <= 1.05 x NORM_REL.  Measured over every (rows, D) of the test (measure_norm): two bf16 roundings, each up to half an ulp = 2^-8 relative,
# so the figure sits just under NORM_SUP = 2^-7 (+ second order), which the CPU test also asserts.  The device differs from the emulation in the
# order of the fp32 row sum and in rsqrt (a few ulp of fp32): that moves a bf16 rounding only next to a tie, where the error is half an ulp
# either way -- 5 %, as in the pin, and never past NORM_SUP.
NORM_REL = 7.69e-3
NORM_SUP = 2.0 ** -7 + 2.0 ** -14


def norm_inputs(rows, D, seed=0):
    x = stream_rows(rows, D, (rows, D, seed))
    w = bf(1.0 + 0.1 * torch.randn(D, generator=gen(47, rows, D, seed)))
    return x, w


def ref_rmsnorm(x, w, eps=NORM_EPS):
    x = x.double()
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.double()


def emu_rmsnorm_f32(x32, w, eps=NORM_EPS):
    x = x32.float()
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return bfr(bfr(x * rstd) * w.float())


def measure_norm():
    worst = 0.0
    for rows in NORM_ROWS:
        for D in NORM_DIMS:
            x, w = norm_inputs(rows, D)
            worst = max(worst, scaled_err(emu_rmsnorm_f32(x, w), ref_rmsnorm(x, w)))
    return worst


def norm_bound():
    return min(1.05 * NORM_REL, NORM_SUP)


# ---- RoPE and the paged K / V append --------------------------------------------------------------------------------------------------------------
ROPE_HEADS = ((4, 4), (4, 2), (8, 1), (32, 32))   # (32, 32): 64 heads x 8 chunks = 512 > 256 threads, the 16-byte kernel's loop runs twice
ROPE_HEAD_DIMS = (128, 72)                        # 72: not a multiple of 16 -> the element-wise kernel, every access aligned
# scaled_err(rotated q / k, float64 rotation by the same fp32 table values) <= 1.05 x ROPE_REL: ONE bf16 rounding.  Measured over every (heads,
# head_dim) of the test (measure_rope); the fused multiply-adds in front of the rounding are emulated as the kernel spells them and add nothing
# that shows (2^-24).  Never past ROPE_SUP = 2^-8, half a bf16 ulp (+ the fp32 share).
ROPE_REL = 3.89e-3
ROPE_SUP = 2.0 ** -8 + 2.0 ** -16


def rope_tables32(n_pos, hd, theta=THETA):
    """the session's tables (session.hip): inv_freq fp32, pos * inv_freq in fp32, cos / sin of that fp32 angle -> fp32 [n_pos][hd / 2]"""
    th = torch.tensor(theta, dtype=torch.float32)
    inv = 1.0 / torch.pow(th, (2.0 * torch.arange(hd // 2, dtype=torch.float32)) / float(hd))
    f = torch.arange(n_pos, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cos(f.double()).float(), torch.sin(f.double()).float()


def ref_rope(x, cos, sin):
    """float64 rotate-half rotation; x [rows][heads][hd], cos / sin [rows][hd / 2] (table rows already gathered by position)"""
    x = x.double()
    half = x.shape[-1] // 2
    x0, x1 = x[..., :half], x[..., half:]
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1)


def emu_rope(x, cos, sin):
    """the kernel's arithmetic: y0 = fma(x0, c, -fl32(x1 s)), y1 = fma(x0, s, fl32(x1 c)), one bf16 rounding.  In float64 a product of a bf16
    and an fp32 value is exact, so fl32 of the float64 sum is the fused result (up to a double rounding 2^-29 below the fp32 ulp)."""
    x = x.double()
    half = x.shape[-1] // 2
    x0, x1 = x[..., :half], x[..., half:]
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    y0 = fl32(x0 * c - fl32(x1 * s))
    y1 = fl32(x0 * s + fl32(x1 * c))
    return bfr(torch.cat([y0, y1], dim=-1).float())


def packing(lens):
    """(cu [B + 1], sequence of every packed row, position of every packed row)"""
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    seq = torch.cat([torch.full((n,), b, dtype=torch.int64) for b, n in enumerate(lens)])
    pos = torch.cat([torch.arange(n, dtype=torch.int64) for n in lens])
    return torch.tensor(cu, dtype=torch.int32), seq, pos


def qkv_rows(total, Hq, Hkv, hd, seed):
    """bf16 q / k / v heads of `total` packed rows: [total][Hq + 2 Hkv][hd]"""
    return bf(torch.randn(total, Hq + 2 * Hkv, hd, generator=gen(53, Hq, Hkv, hd, seed)) * 2.0)


def shuffled_table(B, max_pages, n_pages, seed):
    """page table [B][max_pages] of distinct pages drawn from 0 .. n_pages - 1 (n_pages > B max_pages: some pages are in no row's table)"""
    perm = torch.randperm(n_pages, generator=gen(59, B, max_pages, n_pages, seed))
    return perm[: B * max_pages].view(B, max_pages).to(torch.int32)


def paged_scatter(cache, rows, table, lens, page=PAGE):
    """cache [n_pages][H][page][d] <- rows [total][H][d]: token t of sequence b at page table[b][t / page], slot t % page; everything else stays"""
    _, seq, pos = packing(lens)
    pg = table.long()[seq, pos // page]
    cache[pg, :, pos % page, :] = rows
    return cache


def measure_rope():
    worst = 0.0
    total = sum(SEQ_LENS)
    _, _, pos = packing(SEQ_LENS)
    for hd in ROPE_HEAD_DIMS:
        cos, sin = rope_tables32(max(SEQ_LENS), hd)
        for Hq, Hkv in ROPE_HEADS:
            x = qkv_rows(total, Hq, Hkv, hd, 0)[:, : Hq + Hkv]
            worst = max(worst, scaled_err(emu_rope(x, cos[pos], sin[pos]), ref_rope(x, cos[pos], sin[pos])))
    return worst


def rope_bound():
    return min(1.05 * ROPE_REL, ROPE_SUP)


# ---- the fp8 KV append ------------------------------------------------------------------------------------------------------------------------
KVQ_HEADS = (1, 2, 8, 9, 32)   # 2 Hkv rows per token on 16 row groups: 9 and 32 repeat the group loop, 9 leaves 14 groups idle in the last pass


def e4m3_scale(amax):
    """the smallest power of two s with amax / s <= 448, exactly (1 for an all-zero row): amax = f 2^q with f in [0.5, 1) and 448 = 0.875 x 2^9,
    so s = 2^(q - 9) when f <= 0.875 and 2^(q - 8) otherwise.  A bf16 amax that is not 448 x 2^k is at least 2^-11 away from it in relative
    terms, far beyond the fp32 rounding of the kernel's amax x fl32(1 / 448): the rule has one answer the kernel can be held to."""
    a = amax.double()
    f, q = torch.frexp(a)
    e = torch.where(f <= 0.875, q - 9, q - 8)
    return torch.where(a > 0, torch.exp2(e.double()), torch.ones_like(a)).float()


def ref_kv_quant(x):
    """[..., 128] bf16 -> (e4m3 bytes as uint8, fp32 scale per row, the rows the cache then holds as bf16 = e4m3 x scale, exact).  As
    tests/test_ops_gpu.py's _quant_rows_e4m3, with the scale rule in exact arithmetic."""
    xf = x.float()
    sc = e4m3_scale(xf.abs().amax(dim=-1, keepdim=True))
    q8 = (xf / sc).to(torch.float8_e4m3fn)
    return q8.view(torch.uint8), sc.squeeze(-1), (q8.float() * sc).to(torch.bfloat16)


def kv_rows(total, Hkv, seed):
    """bf16 K / V rows [total][2 Hkv][128] with a power-of-two factor per row from 2^-6 to 2^6, and the edge rows: all zero, amax exactly
    448 x 2^k (k = -3, 0, 4), amax the next bf16 above that.  Returns (rows, the indices of the edge rows)."""
    g = gen(61, total, Hkv, seed)
    x = torch.randn(total, 2 * Hkv, 128, generator=g) * torch.exp2(torch.randint(-6, 7, (total, 2 * Hkv, 1), generator=g).float())
    x = bf(x)
    flat = x.view(-1, 128)
    n = flat.shape[0]
    edge = {}
    picks = torch.randperm(n, generator=g)[:7].tolist()
    edge["zero"] = picks[0]
    flat[picks[0]] = 0
    for i, k in enumerate((-3, 0, 4)):
        top = 448.0 * 2.0 ** k
        for j, val in ((0, top), (1, top * 450.0 / 448.0)):   # 448 = 0x43E0 = 1.75 x 2^8; the next bf16 up, 0x43E1, is 450
            r = picks[1 + 2 * i + j]
            row = bf(torch.randn(128, generator=g) * top / 6.0).float().clamp(-top * 0.99, top * 0.99)
            row[(17 * i + 5 * j) % 128] = -val if j else val
            flat[r] = bf(row)
            edge[("top" if j == 0 else "next", k)] = r
    return x, edge


# ---- embed / splice and the last-row gather ---------------------------------------------------------------------------------------------------------
def ref_embed_splice(ids, lens, E, patches, n_patches):
    """row s of sequence b: s == 0 ? E[ids[b][0]] : s <= n_patches ? patches[b][s - 1] : E[ids[b][s - n_patches]], ids clamped to the table;
    lens[b] ids per sequence, so n_patches + lens[b] rows.  Packed rows, dtype of E."""
    V = E.shape[0]
    out = []
    for b, n in enumerate(lens):
        idb = ids[b, :n].long().clamp(0, V - 1)
        e = E[idb]
        out.append(torch.cat([e[:1], patches[b, :n_patches], e[1:]], dim=0) if n_patches else e)
    return torch.cat(out, dim=0)


def gather_source32(rows, D, seed):
    """fp32 rows for the gather: ordinary values, values exactly on bf16 ties (low half 0x8000, upper half even and odd), the neighbours of
    ties, fp32 denormals and the range in which the bf16 result is denormal"""
    g = gen(67, rows, D, seed)
    x = (torch.randn(rows, D, generator=g) * 3.0).float()
    u = x.view(torch.int32)
    kind = torch.randint(0, 8, (rows, D), generator=g)
    hi = u & ~0xFFFF
    u = torch.where(kind == 1, hi | 0x8000, u)             # a tie
    u = torch.where(kind == 2, hi | 0x8001, u)             # just above a tie
    u = torch.where(kind == 3, hi | 0x7FFF, u)             # just below a tie
    den = torch.randint(1, 1 << 23, (rows, D), generator=g, dtype=torch.int32)
    sign = (u >> 31) << 31
    u = torch.where(kind == 4, sign | den, u)               # exponent field 0: fp32 denormals, among them bf16-denormal results and ties there
    u = torch.where(kind == 5, sign | (den & 0x7F0000) | 0x8000, u)   # ties in the denormal range
    return u.view(torch.float32).clone()


if __name__ == "__main__":
    torch.set_num_threads(8)
    for K in GEMM_SPREAD:
        s, s_bf = measure_gemm(K)
        print(f"gemm K={K}: spread {s:.3g} (table {GEMM_SPREAD[K]:.3g})  bf16-rounded residual {s_bf:.3g}  ratio to the bound {s_bf / gemm_atol(K):.3g}")
    print(f"rmsnorm_f32: scaled error {measure_norm():.4g} (table {NORM_REL:.4g}, sup {NORM_SUP:.4g})")
    print(f"rope: scaled error {measure_rope():.4g} (table {ROPE_REL:.4g}, sup {ROPE_SUP:.4g})")
