"""CPU: the tolerance tables of tests/test_attn_probs_gpu.py and tests/test_taps_session_gpu.py are what the emulations of tests/taps_ref.py measure
against float64 -- not numbers taken from a kernel's output, and not stale or padded ones; the float64 restatement of the LLaMA stack returns what
HF ITSELF returns for output_hidden_states / output_attentions (tests/golden/llama_taps.npz, written by tools/make_llama_taps.py from
LlamaForCausalLM with eager attention on the weights of llama_mha.npz / llama_gqa.npz); the properties of the references the GPU tests lean on."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import taps_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------------
def _pinned(measured, table, what):
    # 5 % for another BLAS's summation order; the table may not be padded: a measurement sits at 2/3 of its entry at least
    assert measured <= 1.05 * table + 1e-12, (what, measured, table)
    if table > 1e-9:
        assert measured >= 0.66 * table, (what, measured, table)


@pytest.mark.parametrize("kind", T.KINDS + ("rows",))
def test_probability_and_row_tables_match_the_emulation(kind):
    m = T.measure(kind)
    assert set(m) == set(T.SPREAD[kind])
    for k, v in m.items():
        _pinned(v, T.SPREAD[kind][k], (kind, k))


@pytest.mark.parametrize("name,gqa", [("gqa", True), ("mha", False)])
def test_layer_table_matches_the_emulation(name, gqa):
    eh, em = T.measure_layers(gqa)
    th, tm = T.LAYERS[name]
    assert len(eh) == len(th) and len(em) == len(tm) and th[0] == 0 and eh[0] == 0   # entry 0 is the input: bit for bit
    for i, (v, t) in enumerate(zip(eh, th)):
        _pinned(v, t, (name, "hidden", i))
    for i, (v, t) in enumerate(zip(em, tm)):
        _pinned(v, t, (name, "map", i))


def test_bounds_are_factor_times_the_spread_without_a_floor():
    assert T.FACTOR == 2.0
    for kind in T.KINDS:
        t = T.tolerances(kind)
        assert t == {k: 2 * v for k, v in T.SPREAD[kind].items()} and t["p"] < 1e-6 and t["sum"] < 2e-6   # fp32 rows: a few ulp of 1
    assert T.tolerances("rows")["normed"] < 1e-5


# ---- the cases and the references ------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_extension_attentions_and_cover_what_the_launch_dispatches_on():
    import extend_attn_ref as X

    assert T.EDGE is X.EDGE and T.RAGGED is X.RAGGED
    pairs = set(T.EDGE)
    assert {(0, 1), (0, 2), (63, 1), (64, 1), (128, 1), (1025, 3)} <= pairs   # one and two keys, n = 1 on a page edge, the 17-page prefix
    assert {n for _, n in pairs} >= {1, 2, 31, 32, 33, 63, 64, 65, 129} and {b for b, _ in pairs} >= {0, 1, 63, 64, 65, 127, 128}
    # the launch dispatches on the GQA group and the cache format alone (no plan function): the GPU cases run every pair of them
    assert set(T.HEADS) == {1, 2, 4, 8} and set(T.KINDS) == {"bf16", "fp8"}
    c = T.edge_case("bf16", 2)
    assert T.min_ld_keys(c) == T.max_keys(c) == 1028
    r = T.ragged_case("fp8", 4)
    assert T.max_keys(r) == 202 and T.min_ld_keys(r) == 204


@pytest.mark.parametrize("kind", T.KINDS)
def test_ref64_probs_is_a_causal_softmax_with_zeros_behind_the_diagonal(kind):
    c = T.build(kind, 2, ((3, 2), (0, 3)), 11, max_pages=1)
    ld = 8
    p = T.ref64_probs(c, ld)
    assert p.shape == (5, c.Hq, ld) and torch.allclose(p.sum(-1), torch.ones(5, c.Hq, dtype=torch.float64))
    assert p[2, :, 0].eq(1).all() and p[2, :, 1:].eq(0).all()                 # sequence 1, row 0: one key
    assert p[0, :, 4:].eq(0).all() and p[0, :, :4].gt(0).all()                 # sequence 0, row 0 at position 3: keys 0 .. 3
    q, k = c.q[1, 1].double(), c.kd[0][:, 0].double()
    assert torch.allclose(p[1, 1, :5], torch.softmax((k @ q) * T.SCALE, dim=0))
    e = T.errors(c, T.emu32_probs(c, ld), p)
    assert e["above"] == 0 and e["p"] < 1e-6 and e["sum"] < 1e-6
    bad = T.emu32_probs(c, ld)
    bad[0, 0, 5] = 1e-9
    assert T.errors(c, bad, p)["above"] == 1                                   # the count sees one entry


def test_rows_reference_is_hf_rmsnorm():
    x, w = T.rows_case(4, 256, 5)
    y = T.ref64_rows(x, w, 1e-5)
    want = x.double() / (x.double().pow(2).mean(-1, keepdim=True) + 1e-5).sqrt() * w.double()
    assert torch.allclose(y, want, rtol=1e-12) and torch.equal(T.ref64_rows(x), x.double()) and torch.equal(T.emu32_rows(x), x)


# ---- ref64 against HF itself ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_llama_stack_returns_what_hf_returns(name):
    from emmax.config import LlmConfig

    g = np.load(os.path.join(ROOT, "tests", "golden", f"llama_{name}.npz"))
    t = np.load(os.path.join(ROOT, "tests", "golden", "llama_taps.npz"))
    h, inter, nl, nh, nkv, hd, vocab = [int(x) for x in g["cfg"]]
    lc = LlmConfig(hidden_size=h, intermediate_size=inter, num_layers=nl, num_heads=nh, num_kv_heads=nkv, head_dim=hd, vocab_size=vocab, rms_eps=1e-5,
                   rope_theta=10000.0)
    sd = {k.replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith("language_model")}
    emb = torch.from_numpy(g["embeds"][0])
    streams, maps, cache = T.llama_stack(emb, sd, lc)
    hid, att = torch.from_numpy(t[f"{name}__hidden"]), torch.from_numpy(t[f"{name}__attn"])
    assert hid.shape == (nl + 1, 9, h) and att.shape == (nl, nh, 9, 9) and torch.equal(hid[0], emb) and float(att.triu(1).abs().max()) == 0.0
    # HF computes in fp32: its distance from float64 is a few fp32 ulp of the entries' size
    for i in range(nl + 1):
        assert torch.allclose(streams[i].float(), hid[i], atol=2e-5, rtol=1e-5), (name, i)
    for i in range(nl):
        assert torch.allclose(maps[i].float(), att[i], atol=1e-6), (name, i)
    # the last entry is the NORMED one: the lm-head on it gives the stored logits
    lg = streams[-1] @ sd["language_model.lm_head.weight"].double().T
    assert torch.allclose(lg.float(), torch.from_numpy(g["prefill_logits"]), atol=2e-5, rtol=1e-5)
    # cached one-token steps: [1, H] rows and [Hq, 1, ctx] maps on top of the cache
    E = sd["language_model.model.embed_tokens.weight"]
    sh, sa = torch.from_numpy(t[f"{name}__step_hidden"]), torch.from_numpy(t[f"{name}__step_attn"])
    for s in range(sh.shape[0]):
        streams, maps, cache = T.llama_stack(E[torch.tensor([int(g["ids"][s])])], sd, lc, cache)
        ctx = 9 + s + 1
        for i in range(nl + 1):
            assert streams[i].shape == (1, h) and torch.allclose(streams[i][0].float(), sh[s, i], atol=2e-5, rtol=1e-5), (name, s, i)
        for i in range(nl):
            assert maps[i].shape == (nh, 1, ctx) and torch.allclose(maps[i][:, 0].float(), sa[s, i, :, :ctx], atol=1e-6) and float(sa[s, i, :, ctx:].abs().sum()) == 0.0


def test_emulation_differs_from_ref64_only_by_its_rounding_points():
    cfg, sd, rows = T.tiny_text_case(gqa=True)
    x0 = sd["language_model.model.embed_tokens.weight"][torch.tensor(rows[0])]
    ref, emu, bh, bm = T.layer_bounds(x0, sd, cfg.llm)
    assert bh[0] == 0 and all(0 < b < 0.2 for b in bh[1:]) and all(0 < b < 1e-2 for b in bm)      # bf16 operands: 2^-9 per rounding, a few per layer
    # a continuation over the caches equals the whole sequence (ref64: to float64 rounding)
    whole = T.llama_stack(x0, sd, cfg.llm)
    head = T.llama_stack(x0[:5], sd, cfg.llm)
    tail = T.llama_stack(x0[5:], sd, cfg.llm, head[2])
    for i in range(cfg.llm.num_layers + 1):
        assert torch.allclose(tail[0][i], whole[0][i][5:], atol=1e-10)
    for i in range(cfg.llm.num_layers):
        assert torch.allclose(tail[1][i], whole[1][i][:, 5:], atol=1e-12)
    # an e4m3 cache moves the maps by more than bf16 keys do, and ref64 over it is its own reference
    _, _, _, bm8 = T.layer_bounds(x0, sd, cfg.llm, kv="fp8")
    d = (T.llama_stack(x0, sd, cfg.llm, kv="fp8")[1][0] - whole[1][0]).abs().max().item()
    assert d > 0 and all(b > 0 for b in bm8)
