"""References, cases and tolerances of the taps (emma-x_amd/csrc/taps.hip).  TEST INFRASTRUCTURE ONLY (plain torch on the CPU, no GPU needed).

The probability kernel computes, for every sequence b of a launch, head h and NEW query row i at position p = base[b] + i, the fp32 row
softmax(scale q . K^T) over keys 0 .. p of the paged cache, and writes exact zeros from p + 1 to ld_keys - 1.  This module holds

  * the CASES: extend_attn_ref's builder (NaN-poisoned unused pages and positions, a random non-identity table: a wrong lookup shows as a wrong
    VALUE, never as a fault), its EDGE pairs (base, n) and its ragged B = 3 launch;
  * ref64_probs: float64 softmax over each row's own keys (fp8: over the de-quantised keys), as [total, Hq, ld_keys] with zeros behind the diagonal;
  * emu32_probs: the kernel's documented roundings in torch fp32, in an order of its own: fp32 scores; pass 1 an online maximum and row sum over
    chunks of 32 keys (the kernel walks pages of 64) with p = 2^(fl(s c - m c)), c = fl(scale log2 e); pass 2 fl(2^(fl(s c - m c)) x fl(1 / l));
  * ref64_rows / emu32_rows: the row copy with and without the RMSNorm, y = fl(fl(x rstd) w);
  * the tolerance table SPREAD, measured here as |emu32 - ref64| over the edge launch of every GQA group and pinned by tests/test_taps_ref.py.
    `python tests/taps_ref.py` prints the measurement.

Measures, per probability row (worst row of a launch):
  p      max |got - ref|                 sum    |sum of the row - 1|            above   entries != 0 behind the diagonal (a count: must be 0)
Bound = FACTOR x SPREAD (decode_attn_ref.FACTOR: the device's v_exp_f32, its MFMA summation order and its tile walk are not reproduced).  No floor:
the rows are fp32.
"""

import math

import torch

import extend_attn_ref as X
from decode_attn_ref import FACTOR, HD, HEADS, NAN, PAGE, SCALE, quant_rows_e4m3

KINDS = X.KINDS
C32 = X.C32
EDGE, RAGGED = X.EDGE, X.RAGGED
edge_case, ragged_case, build = X.edge_case, X.ragged_case, X.build


def max_keys(c):
    """the keys the longest row of the launch sees"""
    return max(b + n for b, n in c.pairs)


def min_ld_keys(c):
    """the smallest ld_keys the op takes for the case: every key of the longest row, in multiples of 4"""
    return (max_keys(c) + 3) // 4 * 4


def _raw_scores(c, b, dtype):
    """unscaled scores [n, Hq, L] of sequence b's new rows over its keys, and the causal mask [n, L]"""
    rep = c.Hq // c.Hkv
    kk = c.kd[b].to(dtype).repeat_interleave(rep, dim=1)
    q = c.q[c.cu[b]:c.cu[b + 1]].to(dtype)
    L = c.base[b] + c.n[b]
    vis = torch.arange(L)[None, :] <= (c.base[b] + torch.arange(c.n[b]))[:, None]
    return torch.einsum("nhd,lhd->nhl", q, kk), vis


def ref64_probs(c, ld_keys):
    out = torch.zeros(c.total, c.Hq, ld_keys, dtype=torch.float64)
    for b in range(c.B):
        s, vis = _raw_scores(c, b, torch.float64)
        s = (s * SCALE).masked_fill(~vis[:, None, :], -math.inf)
        out[c.cu[b]:c.cu[b + 1], :, : s.shape[-1]] = torch.softmax(s, dim=-1)
    return out


def emu32_probs(c, ld_keys, chunk=32):
    out = torch.zeros(c.total, c.Hq, ld_keys, dtype=torch.float32)
    for b in range(c.B):
        s, vis = _raw_scores(c, b, torch.float32)
        n, H, L = s.shape
        s = s.masked_fill(~vis[:, None, :], -math.inf)
        m = torch.full((n, H), -math.inf)
        l = torch.zeros(n, H)
        for a in range(0, L, chunk):   # pass 1
            sc = s[:, :, a:a + chunk]
            mn = torch.maximum(m, sc.max(dim=-1).values)
            ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
            alpha = torch.exp2(((m - ms) * C32).float())
            l = l * alpha + torch.exp2((sc * C32 - (ms * C32)[..., None]).float()).sum(-1)
            m = mn
        inv = (1.0 / l).float()
        p = torch.exp2((s * C32 - (m * C32)[..., None]).float()) * inv[..., None]   # pass 2 (masked scores: 2^-inf = 0)
        out[c.cu[b]:c.cu[b + 1], :, :L] = p
    return out


def live_mask(c, ld_keys):
    """bool [total, ld_keys]: key k is visible to packed row r"""
    vis = torch.zeros(c.total, ld_keys, dtype=torch.bool)
    for b in range(c.B):
        pos = c.base[b] + torch.arange(c.n[b])
        vis[c.cu[b]:c.cu[b + 1]] = torch.arange(ld_keys)[None, :] <= pos[:, None]
    return vis


def errors(c, got, ref):
    """got fp32 / ref float64 [total, Hq, ld_keys]"""
    g = got.double()
    above = ~live_mask(c, got.shape[-1])[:, None, :].expand_as(g)
    return dict(p=(g - ref).abs().max().item(), sum=(g.sum(-1) - 1.0).abs().max().item(), above=int((g[above] != 0).sum().item()))


# ---- the row copy --------------------------------------------------------------------------------------------------------------------------------
def ref64_rows(x, w=None, eps=1e-6):
    x = x.double()
    if w is None:
        return x
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.double()


def emu32_rows(x, w=None, eps=1e-6):
    x = x.float()
    if w is None:
        return x
    rstd = torch.rsqrt(x.pow(2).sum(-1, keepdim=True) / x.shape[-1] + eps)
    return (x * rstd) * w.float()


def rows_case(rows, H, seed):
    """a stream with a few large channels (what a residual stream looks like), a bf16 weight"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, H, generator=g)
    x[:, :: max(1, H // 7)] *= 30.0
    w = X.bf(1.0 + 0.2 * torch.randn(H, generator=g))
    return x, w


def err_rows(got, ref):
    """max |got - ref| / rms(ref), worst row"""
    rms = ref.double().pow(2).mean(-1).sqrt().clamp_min(1e-30)
    return ((got.double() - ref.double()).abs().amax(-1) / rms).max().item()


# ---- the LLaMA stack, every layer's stream and map ---------------------------------------------------------------------------------------------
# ref64: float64 throughout, on the (bf16-valued) weights the engine holds.  emu: the same in float64 with the session's rounding points (DESIGN.md
# section 2): the normed rows (two bf16 roundings: x rstd, then x w), every GEMM's bf16 result (qkv rows, attention rows, SwiGLU product), the rotated
# q / k rows, bf16 or e4m3 K / V, P rounded to bf16 for the value product, an fp32 residual stream.  Its accumulations stay float64: what the device's
# fp32 MFMA sums and its tile walks add on top is what FACTOR is for.
def _w(sd, li, name):
    return sd[f"language_model.model.layers.{li}.{name}.weight"].double()


def _norm(x, w, eps, emu):
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    if emu:
        return X.bf(X.bf(y.float()) * w.float()).double()
    return y * w


def _rope(x, pos, theta):
    """x [n, heads, hd] float64 at absolute positions pos [n]"""
    hd = x.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    f = pos.double()[:, None] * inv[None, :]
    cos, sin = torch.cat([f, f], -1).cos()[:, None, :], torch.cat([f, f], -1).sin()[:, None, :]
    return x * cos + torch.cat([-x[..., hd // 2:], x[..., : hd // 2]], -1) * sin


def llama_stack(x0, sd, lc, cache=None, emu=False, kv="bf16"):
    """One sequence: x0 [n, H] (the rows behind the embed / patch splice) on top of `cache` (per layer (K, V) [L, Hkv, hd] float64, or None).
    -> (streams: n_layers + 1 tensors [n, H], the last NORMED; maps: n_layers tensors [Hq, n, L + n]; the new cache).
    kv = "fp8": the cache holds e4m3 rows + a power-of-two scale, and every reader -- the maps, the attention of a prefill (its quantising pass
    writes the de-quantised rows back into the qkv buffer), of an extension and of a step -- sees the DE-QUANTISED rows, ref64's included"""
    r = (lambda t: X.bf(t.float()).double()) if emu else (lambda t: t)
    h = x0.double()
    n = h.shape[0]
    Hq, Hkv, hd = lc.num_heads, lc.num_kv_heads, lc.head_dim
    base = 0 if cache is None else cache[0][0].shape[0]
    pos = torch.arange(base, base + n)
    streams, maps, new_cache = [h], [], []
    for li in range(lc.num_layers):
        xn = _norm(h, _w(sd, li, "input_layernorm"), lc.rms_eps, emu)
        q = r(xn @ _w(sd, li, "self_attn.q_proj").T).view(n, Hq, hd)
        k = r(xn @ _w(sd, li, "self_attn.k_proj").T).view(n, Hkv, hd)
        v = r(xn @ _w(sd, li, "self_attn.v_proj").T).view(n, Hkv, hd)
        q, k = r(_rope(q, pos, lc.rope_theta)), r(_rope(k, pos, lc.rope_theta))
        if kv == "fp8":   # the cache holds e4m3 rows + a power-of-two scale: the keys and values every row reads are the DE-QUANTISED ones (ref64 too)
            k, v = quant_rows_e4m3(k.float())[2].double(), quant_rows_e4m3(v.float())[2].double()
        if cache is not None:
            k, v = torch.cat([cache[li][0], k]), torch.cat([cache[li][1], v])
        new_cache.append((k, v))
        rep = Hq // Hkv
        vis = torch.arange(base + n)[None, :] <= pos[:, None]
        sc = torch.einsum("nhd,lhd->hnl", q, k.repeat_interleave(rep, dim=1)) * (hd ** -0.5)
        P = torch.softmax(sc.masked_fill(~vis[None], -math.inf), dim=-1)
        maps.append(P)
        a = r(torch.einsum("hnl,lhd->nhd", r(P), v.repeat_interleave(rep, dim=1)).reshape(n, Hq * hd))
        h = h + a @ _w(sd, li, "self_attn.o_proj").T
        if emu:
            h = h.float().double()
        xn = _norm(h, _w(sd, li, "post_attention_layernorm"), lc.rms_eps, emu)
        g, u = xn @ _w(sd, li, "mlp.gate_proj").T, xn @ _w(sd, li, "mlp.up_proj").T
        h = h + r(torch.nn.functional.silu(g) * u) @ _w(sd, li, "mlp.down_proj").T
        if emu:
            h = h.float().double()
        streams.append(h)
    hn = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + lc.rms_eps) * sd["language_model.model.norm.weight"].double()
    streams[-1] = hn   # HF: the last entry is norm(h_L)
    return streams, maps, new_cache


def err_layers(got_streams, got_maps, ref):
    """per entry: hidden max |got - ref| / rms(ref entry); maps max |got - ref|"""
    rs, rm, _ = ref
    eh = [((g.double() - a).abs().max() / a.pow(2).mean().sqrt().clamp_min(1e-30)).item() for g, a in zip(got_streams, rs)]
    em = [(g.double() - a).abs().max().item() for g, a in zip(got_maps, rm)]
    return eh, em


def layer_bounds(x0, sd, lc, cache_ref=None, cache_emu=None, kv="bf16"):
    """(ref64 result, emu result, per-entry hidden bounds, per-layer map bounds): FACTOR x the emulation's distance from ref64 on these inputs.
    Entry 0 is the input itself: bound 0 (bit for bit)"""
    ref = llama_stack(x0, sd, lc, cache_ref, emu=False, kv=kv)
    emu = llama_stack(x0, sd, lc, cache_emu, emu=True, kv=kv)
    eh, em = err_layers(emu[0], emu[1], ref)
    return ref, emu, [FACTOR * e for e in eh], [FACTOR * e for e in em]


def tiny_text_case(gqa=True, seed=13, lens=(9, 33, 20)):
    """the text-only case the layer table is pinned on: EmmaXConfig.tiny's LLaMA (3 layers, hidden 256), synthetic weights, ragged rows"""
    from emmax.config import EmmaXConfig
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny(gqa=gqa)
    sd = {k: v.to(torch.bfloat16).float() for k, v in synthetic_state_dict(cfg, seed=seed, planted=False).items() if k.startswith("language_model.")}
    g = torch.Generator().manual_seed(seed + 1)
    rows = [[1] + torch.randint(3, 31744, (n - 1,), generator=g).tolist() for n in lens]
    return cfg, sd, rows


def measure_layers(gqa=True):
    """worst over the case's rows of |emu - ref64| per entry: (hidden [n_layers + 1], maps [n_layers])"""
    cfg, sd, rows = tiny_text_case(gqa)
    E = sd["language_model.model.embed_tokens.weight"]
    eh = [0.0] * (cfg.llm.num_layers + 1)
    em = [0.0] * cfg.llm.num_layers
    for r in rows:
        _, _, bh, bm = layer_bounds(E[torch.tensor(r)], sd, cfg.llm)
        eh = [max(a, b / FACTOR) for a, b in zip(eh, bh)]
        em = [max(a, b / FACTOR) for a, b in zip(em, bm)]
    return eh, em


# LAYERS[variant] = (hidden per entry, maps per layer): measure_layers() on tiny_text_case -- pinned by tests/test_taps_ref.py
LAYERS = {
    "gqa": ([0, 0.0252, 0.0189, 0.0188], [0.00032, 0.00043, 0.000386]),
    "mha": ([0, 0.0195, 0.0202, 0.0219], [0.00032, 0.000379, 0.000373]),
}


# ---- the tolerance table -----------------------------------------------------------------------------------------------------------------------
# SPREAD[kind] = {measure: worst |emu32 - ref64|} over the edge launch of every GQA group; "rows": the normed row copy (H = 256 and 4096).
# Measured on the CPU by measure() -- no GPU output involved.
SPREAD = {
    "bf16": {"p": 2.31e-07, "sum": 3.18e-07},
    "fp8": {"p": 2.73e-07, "sum": 5.1e-07},
    "rows": {"normed": 2.1e-06},
}
ROWS_SHAPES = ((5, 256), (3, 4096))


def tolerances(kind):
    return {k: FACTOR * v for k, v in SPREAD[kind].items()}


def measure(kind):
    out = {}
    if kind == "rows":
        for i, (rows, H) in enumerate(ROWS_SHAPES):
            x, w = rows_case(rows, H, 77 + i)
            for xx in (x, X.bf(x)):   # an fp32 stream and a bf16 one
                out["normed"] = max(out.get("normed", 0.0), err_rows(emu32_rows(xx, w), ref64_rows(xx, w)))
        return out
    for G in HEADS:
        c = edge_case(kind, G)
        ld = min_ld_keys(c)
        e = errors(c, emu32_probs(c, ld), ref64_probs(c, ld))
        assert e.pop("above") == 0
        for k, v in e.items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def _fmt(d):
    return "{" + ", ".join(f'"{k}": {v:.3g}' for k, v in sorted(d.items())) + "}"


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "emma-x_amd"))   # (the suite's conftest does this for the tests)
    print("SPREAD = {")
    for kind in KINDS + ("rows",):
        print(f'    "{kind}": {_fmt(measure(kind))},')
    print("}")
    print("LAYERS = {")
    for name, gqa in (("gqa", True), ("mha", False)):
        eh, em = measure_layers(gqa)
        print(f'    "{name}": ([' + ", ".join(f"{v:.3g}" for v in eh) + "], [" + ", ".join(f"{v:.3g}" for v in em) + "]),")
    print("}")
