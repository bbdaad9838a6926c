"""output_hidden_states / output_attentions through the session's taps (include/emmax.h: emmax_session_set_pass_taps / _set_step_taps), on
EmmaXConfig.tiny's GQA variant (3 layers, hidden 256), B = 1 and a ragged B = 3.

Reference: tests/taps_ref.py -- llama_stack in float64 (ref64) and with the session's rounding points (emu), run on the engine's own bf16-valued
weights and on hidden_states[0] as input, which is itself checked BIT FOR BIT against the embedding table and the patch embeddings.  Per entry the
bound is FACTOR x |emu - ref64| (hidden: relative to the rms of the reference entry; maps: absolute): the pinned table taps_ref.LAYERS for the
text-only rows it was measured on, the same measurement on the call's own inputs everywhere else.  Never a number taken from the session.

  * forward, all four branches (multimodal, text-only, continuation on a handle with n = 5 and n = 1 where base > 0 comes from the device, the cached
    one-token step): HF's shapes, zeros above the diagonal, rows that sum to 1, every entry within its bound; an fp8-cache session against the
    restatement over de-quantised keys;
  * generate of 6 tokens, greedy and sampled, eager and replayed: ids and logit rows BITWISE equal to the same call without taps (the guard of the
    existing path), HF's shapes per element, and in all four the steps within the bounds of the restatement teacher-forced on the emitted ids; the
    same through an fp8-cache session's steps and cached forward (the de-quantised restatement); a row that stops early
    leaves zeros; tap_layers selects; predict_action's states are the step taps of the last entry; re-binding under graph replay; the C refusals.
Every test fails on a library or package without the feature (a missing symbol, or forward's NotImplementedError)."""

import numpy as np
import pytest
import torch

import taps_ref as T
from test_e2e_gpu import _inputs, _mk

pytestmark = pytest.mark.gpu

F = T.FACTOR
NEW = 6
ERR_INVALID, ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def M(device):
    cfg, sd, rows = T.tiny_text_case(gqa=True)
    model, sd_ref = _mk(cfg, 13, False, device, max_batch=3, max_prompt=64, max_ctx=400)
    for k, v in sd.items():
        assert torch.equal(v, sd_ref[k]), k   # the restatement runs on the weights the engine holds
    yield cfg, model, sd, rows
    model.engine.close()


def per_row(x, b):
    """row b of a stacked-or-list entry"""
    return x[b]


def check_maps_are_maps(maps, keys0, what):
    """[Hq, n, L]: L = the row's keys, zeros above the diagonal, rows sum to 1 over their live entries"""
    for li, m in enumerate(maps):
        Hq, n, L = m.shape
        assert L == keys0 and torch.isfinite(m).all(), (what, li, tuple(m.shape))
        pos = (L - n) + torch.arange(n)
        above = torch.arange(L)[None, :] > pos[:, None]
        assert (m[:, above] == 0).all(), f"{what}: layer {li}: non-zeros above the diagonal"
        assert ((m.double().sum(-1) - 1).abs() < 1e-5).all(), f"{what}: layer {li}: a row does not sum to 1"


def check_against(got_h, got_m, ref, bh, bm, what, sel_h=None, sel_m=None):
    nl = len(ref[1])
    sel_h = list(range(nl + 1)) if sel_h is None else sel_h
    sel_m = list(range(nl)) if sel_m is None else sel_m
    eh, em = T.err_layers(got_h, got_m, ([ref[0][i] for i in sel_h], [ref[1][i] for i in sel_m], None))
    print(f"{what}: hidden " + " ".join(f"{e:.3g}/{bh[i]:.3g}" for e, i in zip(eh, sel_h)) + "  maps " + " ".join(f"{e:.3g}/{bm[i]:.3g}" for e, i in zip(em, sel_m)))
    bad = [f"hidden[{i}] {e:.3g} > {bh[i]:.3g}" for e, i in zip(eh, sel_h) if e > bh[i]] + [f"map {i} {e:.3g} > {bm[i]:.3g}" for e, i in zip(em, sel_m) if e > bm[i]]
    assert not bad, f"{what}: " + ", ".join(bad)


def embed(sd, ids):
    return sd["language_model.model.embed_tokens.weight"][torch.tensor(ids)]


def cpu_rows(out, B):
    """(hidden per row: list over entries, maps per row: list over layers), on the host"""
    hs = [[per_row(e, b).float().cpu() for e in out.hidden_states] for b in range(B)] if out.hidden_states is not None else None
    at = [[per_row(e, b).float().cpu() for e in out.attentions] for b in range(B)] if out.attentions is not None else None
    return hs, at


def check_generated_steps(out, prompts, sd, cfg, what, kv="bf16"):
    """HF's layout of a tapped generate of NEW tokens on 3 multimodal rows, and EVERY step's states and maps within the bounds of the restatement
    teacher-forced on the emitted ids (it depends on neither sampling nor replay): the caches start from the prompt pass's own hidden_states[0]"""
    lc = cfg.llm
    nl, n_p = lc.num_layers, cfg.n_patches
    assert len(out.hidden_states) == NEW and len(out.attentions) == NEW and len(out.hidden_states[0]) == nl + 1 and len(out.attentions[1]) == nl
    S = [n_p + len(p) for p in prompts]
    new = [out.sequences[b, len(prompts[b]):len(prompts[b]) + NEW].tolist() for b in range(3)]
    x0 = [out.hidden_states[0][0][b].float().cpu() for b in range(3)]
    refc = [T.llama_stack(x, sd, lc, kv=kv)[2] for x in x0]
    emuc = [T.llama_stack(x, sd, lc, emu=True, kv=kv)[2] for x in x0]
    for t in range(1, NEW):
        for i in range(nl + 1):
            assert tuple(out.hidden_states[t][i].shape) == (3, 1, lc.hidden_size)
        for b in range(3):
            maps = [out.attentions[t][li][b].float().cpu() for li in range(nl)]
            check_maps_are_maps(maps, S[b] + t, f"{what} step {t} row {b}")   # ctx_t live entries that sum to 1
            hid = [out.hidden_states[t][i][b].float().cpu() for i in range(nl + 1)]
            assert torch.equal(hid[0], embed(sd, [new[b][t - 1]])), f"{what} step {t}: hidden_states[0] is not the embedding of the token the step consumed"
            ref = T.llama_stack(hid[0], sd, lc, refc[b], kv=kv)
            emu = T.llama_stack(hid[0], sd, lc, emuc[b], emu=True, kv=kv)
            eh, em = T.err_layers(emu[0], emu[1], ref)
            check_against(hid, maps, ref, [F * e for e in eh], [F * e for e in em], f"{what} step {t} row {b}")
            refc[b], emuc[b] = ref[2], emu[2]


# ---- forward: fresh passes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", [[0], [0, 1, 2]], ids=["B1", "B3ragged"])
def test_forward_text_only_returns_every_layer_within_the_pinned_table(M, sel):
    cfg, model, sd, rows = M
    rows = [rows[i] for i in sel]
    out = model.forward(input_ids=rows, output_hidden_states=True, output_attentions=True)
    nl = cfg.llm.num_layers
    assert len(out.hidden_states) == nl + 1 and len(out.attentions) == nl
    if len(rows) == 1:
        assert tuple(out.hidden_states[0].shape) == (1, len(rows[0]), cfg.llm.hidden_size) and out.hidden_states[0].dtype == torch.float32
        assert tuple(out.attentions[0].shape) == (1, cfg.llm.num_heads, len(rows[0]), len(rows[0]))
    else:
        assert isinstance(out.hidden_states[0], list) and isinstance(out.attentions[0], list) and isinstance(out.logits, list)   # the rule `logits` follows
    hs, at = cpu_rows(out, len(rows))
    bh, bm = [F * v for v in T.LAYERS["gqa"][0]], [F * v for v in T.LAYERS["gqa"][1]]
    for b, r in enumerate(rows):
        assert torch.equal(hs[b][0], embed(sd, r)), "hidden_states[0] is not the embedding rows bit for bit"
        check_maps_are_maps(at[b], len(r), f"text row {b}")
        check_against(hs[b], at[b], T.llama_stack(hs[b][0], sd, cfg.llm), bh, bm, f"text-only row {b} ({len(r)} ids)")


@pytest.mark.parametrize("B", [1, 3])
def test_forward_multimodal_counts_the_patch_rows_and_is_within_its_bounds(M, device, B):
    cfg, model, sd, _ = M
    frames, rows = _inputs(cfg, B, [7, 12, 9][:B], seed=4)
    out = model.forward(input_ids=rows, frames_u8=torch.from_numpy(frames).to(device), output_hidden_states=True, output_attentions=True,
                        output_projector_features=True)
    hs, at = cpu_rows(out, B)
    n_p = cfg.n_patches
    for b, r in enumerate(rows):
        S = n_p + len(r)
        assert tuple(hs[b][0].shape) == (S, cfg.llm.hidden_size) and tuple(at[b][0].shape) == (cfg.llm.num_heads, S, S)
        x0 = torch.cat([embed(sd, r[:1]), out.projector_features[b].float().cpu(), embed(sd, r[1:])])
        assert torch.equal(hs[b][0], x0), "hidden_states[0] is not [BOS] ++ patch rows ++ text rows bit for bit"
        check_maps_are_maps(at[b], S, f"multimodal row {b}")
        ref, _, bh, bm = T.layer_bounds(x0, sd, cfg.llm)
        check_against(hs[b], at[b], ref, bh, bm, f"multimodal row {b} (S = {S})")


def test_fp8_cache_maps_follow_the_dequantised_keys(device):
    from emmax import _lib

    cfg, sd, rows = T.tiny_text_case(gqa=True)
    with _lib.tuning(kv_fp8=1):
        model, _ = _mk(cfg, 13, False, device, max_batch=3, max_prompt=64, max_ctx=400)
        out = model.forward(input_ids=rows, output_hidden_states=True, output_attentions=True)
    hs, at = cpu_rows(out, len(rows))
    for b, r in enumerate(rows):
        check_maps_are_maps(at[b], len(r), f"fp8 row {b}")
        # ref64 and emu both over K / V as the cache holds them: e4m3 rows + a power-of-two scale, de-quantised
        ref, _, bh, bm = T.layer_bounds(hs[b][0], sd, cfg.llm, kv="fp8")
        check_against(hs[b], at[b], ref, bh, bm, f"fp8-cache row {b}")
    model.engine.close()


# ---- continuation and the cached step -------------------------------------------------------------------------------------------------------------
def test_continuation_and_cached_step_extend_the_restatements_cache(M, device):
    cfg, model, sd, rows = M
    lc = cfg.llm
    g = torch.Generator().manual_seed(3)
    more = [torch.randint(3, 31744, (5,), generator=g).tolist() for _ in rows]
    one = [torch.randint(3, 31744, (1,), generator=g).tolist() for _ in rows]
    step = [torch.randint(3, 31744, (1,), generator=g).tolist() for _ in rows]
    first = model.forward(input_ids=rows, use_cache=True)
    h = first.past_key_values
    refc = [T.llama_stack(embed(sd, r), sd, lc)[2] for r in rows]
    emuc = [T.llama_stack(embed(sd, r), sd, lc, emu=True)[2] for r in rows]
    ctx = [len(r) for r in rows]
    for name, new, kw in (("n = 5", more, {}), ("n = 1", one, {}), ("cached step", step, {"tensor": True})):
        ids = torch.tensor(new) if kw else new   # [B, 1] tensor + handle: the one-token cached step; lists: the extension pass
        out = model.forward(input_ids=ids, past_key_values=h, output_hidden_states=True, output_attentions=True)
        hs, at = cpu_rows(out, len(rows))
        for b in range(len(rows)):
            n = len(new[b])
            assert tuple(hs[b][0].shape) == (n, lc.hidden_size) and tuple(at[b][0].shape) == (lc.num_heads, n, ctx[b] + n), (name, b, tuple(at[b][0].shape))
            assert torch.equal(hs[b][0], embed(sd, new[b])), f"{name}: hidden_states[0] is not the embedding rows"
            check_maps_are_maps(at[b], ctx[b] + n, f"{name} row {b}")
            ref = T.llama_stack(hs[b][0], sd, lc, refc[b])
            emu = T.llama_stack(hs[b][0], sd, lc, emuc[b], emu=True)
            eh, em = T.err_layers(emu[0], emu[1], ref)
            check_against(hs[b], at[b], ref, [F * e for e in eh], [F * e for e in em], f"{name} row {b} (base {ctx[b]})")
            refc[b], emuc[b] = ref[2], emu[2]
            ctx[b] += n
        assert h.lengths == ctx
    assert model.engine.taps_bound == 0


# ---- generate -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1], ids=["eager", "graph"])
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_generate_with_taps_emits_the_same_ids_and_logits_bit_for_bit(M, device, tune, sample, graph):
    cfg, model, sd, rows = M
    tune(graph=graph)
    frames, prompts = _inputs(cfg, 3, [7, 12, 9], seed=6)
    fr = torch.from_numpy(frames).to(device)
    kw = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True, min_new_tokens=NEW)
    if sample:
        kw.update(do_sample=True, temperature=0.9, top_k=40, seed=17)
    plain = model.generate(prompts, frames_u8=fr, **kw)
    out = model.generate(prompts, frames_u8=fr, output_hidden_states=True, output_attentions=True, **kw)
    again = model.generate(prompts, frames_u8=fr, **kw)   # unbound again: the plain call after a tapped one
    assert torch.equal(plain.sequences, out.sequences) and torch.equal(plain.sequences, again.sequences)
    for t in range(NEW):
        assert torch.equal(plain.logits[t], out.logits[t]) and torch.equal(plain.logits[t], again.logits[t]), f"logit rows of token {t} differ with taps bound"
    assert model.engine.taps_bound == 0 and (not graph or model.engine.graph_active())
    check_generated_steps(out, prompts, sd, cfg, f"{'sampled' if sample else 'greedy'} {'graph' if graph else 'eager'}")


@pytest.mark.parametrize("graph", [0, 1], ids=["eager", "graph"])
def test_fp8_cache_steps_and_cached_forward_follow_the_dequantised_keys(device, tune, graph):
    """The step's key reaches an fp8 cache only in the attention launch: the map launched behind it must see it (de-quantised), as the restatement
    over e4m3 rows does -- through generate's steps, eager and replayed, and through forward's cached one-token step"""
    from emmax import _lib

    cfg, sd, rows = T.tiny_text_case(gqa=True)
    lc = cfg.llm
    frames, prompts = _inputs(cfg, 3, [7, 12, 9], seed=6)
    fr = torch.from_numpy(frames).to(device)
    with _lib.tuning(kv_fp8=1):
        model, _ = _mk(cfg, 13, False, device, max_batch=3, max_prompt=64, max_ctx=400)
    tune(graph=graph)
    out = model.generate(prompts, frames_u8=fr, output_hidden_states=True, output_attentions=True, max_new_tokens=NEW, return_dict_in_generate=True,
                         min_new_tokens=NEW)
    assert not graph or model.engine.graph_active()
    check_generated_steps(out, prompts, sd, cfg, f"fp8 cache {'graph' if graph else 'eager'}", kv="fp8")
    # forward: a prefill with a handle, then the cached one-token step
    first = model.forward(input_ids=rows, use_cache=True, output_hidden_states=True)
    toks = [[5], [77], [901]]
    step = model.forward(input_ids=torch.tensor(toks), past_key_values=first.past_key_values, output_hidden_states=True, output_attentions=True)
    hs, at = cpu_rows(step, 3)
    for b, r in enumerate(rows):
        x0 = embed(sd, r)
        refc, emuc = T.llama_stack(x0, sd, lc, kv="fp8")[2], T.llama_stack(x0, sd, lc, emu=True, kv="fp8")[2]
        check_maps_are_maps(at[b], len(r) + 1, f"fp8 cached step row {b}")
        assert torch.equal(hs[b][0], embed(sd, toks[b]))
        ref = T.llama_stack(hs[b][0], sd, lc, refc, kv="fp8")
        emu = T.llama_stack(hs[b][0], sd, lc, emuc, emu=True, kv="fp8")
        eh, em = T.err_layers(emu[0], emu[1], ref)
        check_against(hs[b], at[b], ref, [F * e for e in eh], [F * e for e in em], f"fp8 cached step row {b}")
    model.engine.close()


def test_a_row_that_stops_early_leaves_zeros_and_tap_layers_selects(M, device):
    from emmax.sampling import LogitsProcessing

    cfg, model, sd, rows = M
    lc = cfg.llm
    frames, prompts = _inputs(cfg, 3, [7, 12, 9], seed=6)
    fr = torch.from_numpy(frames).to(device)
    eos = cfg.eos_token_id
    proc = [LogitsProcessing(sequence_bias={(eos,): 1e4}, min_new_tokens=2), LogitsProcessing(min_new_tokens=NEW), LogitsProcessing(min_new_tokens=NEW)]
    ids, lens, taps = model.generate_ids(prompts, frames_u8=fr, max_new_tokens=NEW, processing=proc, hidden=[0, 2], attentions=[2])
    lens = lens.tolist()
    assert lens == [3, NEW, NEW] and int(ids[0, 2]) == eos, lens
    assert len(taps.hidden_states) == NEW and len(taps.hidden_states[1]) == 2 and len(taps.attentions[1]) == 1   # exactly the selected entries
    for t in range(1, NEW):
        h0, h2, m2 = taps.hidden_states[t][0], taps.hidden_states[t][1], taps.attentions[t][0]
        for b in range(3):
            live = t < lens[b]
            assert bool((h0[b] != 0).any()) == live and bool((h2[b] != 0).any()) == live and bool((m2[b] != 0).any()) == live, (t, b)
    # tap_layers through generate: [-1] = the normed last entry / the last layer's map; the same values as entry -1 of a full call
    kw = dict(frames_u8=fr, max_new_tokens=3, return_dict_in_generate=True, output_hidden_states=True, output_attentions=True, min_new_tokens=3)
    full = model.generate(prompts, **kw)
    last = model.generate(prompts, tap_layers=[-1], **kw)
    some = model.generate(prompts, tap_layers=[0, 2, 0], **kw)
    assert len(last.hidden_states[0]) == 1 and len(last.attentions[0]) == 1 and len(some.hidden_states[1]) == 2 and len(some.attentions[1]) == 2
    for t in range(3):
        for b in range(3):
            assert torch.equal(last.hidden_states[t][0][b], full.hidden_states[t][-1][b]) and torch.equal(last.attentions[t][0][b], full.attentions[t][-1][b])
            assert torch.equal(some.hidden_states[t][1][b], full.hidden_states[t][2][b]) and torch.equal(some.attentions[t][0][b], full.attentions[t][0][b])


def test_predict_action_returns_the_states_that_emitted_the_action_tokens(M, device):
    cfg, model, sd, rows = M
    frames, prompts = _inputs(cfg, 1, [9], seed=8)
    fr = torch.from_numpy(frames).to(device)
    key = next(iter(model.norm_stats))
    a0 = model.predict_action(prompts, unnorm_key=key, frames_u8=fr)
    a1, states = model.predict_action(prompts, unnorm_key=key, frames_u8=fr, return_hidden_states=True)
    dim = model.get_action_dim(key)
    assert np.array_equal(a0, a1) and tuple(states.shape) == (dim, cfg.llm.hidden_size) and states.dtype == torch.float32
    row = model._rows(prompts)[0]
    row = row if row[-1] == 29871 else row + [29871]
    _, _, taps = model.generate_ids([row], frames_u8=fr, max_new_tokens=dim, hidden=[cfg.llm.num_layers])
    want = torch.stack([taps.hidden_states[t][0][0][-1] for t in range(len(taps.hidden_states))])
    assert torch.equal(states[: want.shape[0]], want) and bool((states[0] != 0).any())


def test_rebinding_under_graph_replay_recaptures_and_stays_correct(M, device, tune):
    cfg, model, sd, rows = M
    tune(graph=1)
    frames, prompts = _inputs(cfg, 1, [9], seed=9)
    fr = torch.from_numpy(frames).to(device)
    kw = dict(frames_u8=fr, max_new_tokens=NEW, return_dict_in_generate=True, min_new_tokens=NEW)
    a = model.generate(prompts, output_hidden_states=True, **kw)
    b = model.generate(prompts, **kw)                                # unbound: re-captured without the taps
    c = model.generate(prompts, output_hidden_states=True, **kw)     # bound again, other buffers
    assert model.engine.graph_active() and torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences, c.sequences)
    for t in range(NEW):
        for i in range(cfg.llm.num_layers + 1):
            assert torch.equal(a.hidden_states[t][i], c.hidden_states[t][i]) and bool((c.hidden_states[t][i] != 0).any()), (t, i)
    assert a.hidden_states[1][0].data_ptr() != c.hidden_states[1][0].data_ptr()


def test_c_level_refusals_change_nothing(M, device):
    from emmax import _lib
    from emmax.sampling import BeamParams

    cfg, model, sd, rows = M
    eng = model.engine
    model._set_sampling(eng, 3, None)      # (what the generate tests left in the session: beams are refused beside it)
    model._set_processing(eng, 3, None)
    if eng.top_logprobs_bound:
        eng.clear_top_logprobs()
    lib, s, st = eng.lib, eng._session, _lib.current_stream()
    nl = cfg.llm.num_layers
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=device)
    assert lib.emmax_session_taps(s) == 0 and lib.emmax_session_taps(None) == -1
    assert lib.emmax_session_set_pass_taps(s, buf.data_ptr(), 1 << (nl + 1), None, 0, 0, st) == ERR_INVALID     # a bit above n_layers
    assert lib.emmax_session_set_pass_taps(s, None, 0, buf.data_ptr(), 1 << nl, 64, st) == ERR_INVALID          # ... above n_layers - 1
    assert lib.emmax_session_set_pass_taps(s, None, 0, buf.data_ptr(), 1, 66, st) == ERR_INVALID and "multiple of 4" in lib.emmax_last_error().decode()
    assert lib.emmax_session_set_pass_taps(s, buf.data_ptr(), 0, None, 0, 0, st) == ERR_INVALID                 # a buffer without a mask
    assert lib.emmax_session_taps(s) == 0
    # ld_keys too small: known at the pass, which refuses before it launches anything and leaves the binding as it was
    assert lib.emmax_session_set_pass_taps(s, None, 0, buf.data_ptr(), 1, 4, st) == 0 and lib.emmax_session_taps(s) == 1
    with pytest.raises(_lib.EmmaxError, match="ld_keys"):
        eng.prefill([rows[0]], None)
    assert lib.emmax_session_clear_taps(s, st) == 0 and lib.emmax_session_taps(s) == 0
    eng.prefill([rows[0]], None)
    assert lib.emmax_session_set_step_taps(s, buf.data_ptr(), 1, None, 0, 0, 0, st) == ERR_INVALID               # max_new outside 1..max_ctx
    assert lib.emmax_session_set_step_taps(s, None, 0, buf.data_ptr(), 1, 8, 4, st) == ERR_INVALID and "ld_keys" in lib.emmax_last_error().decode()
    assert lib.emmax_session_set_step_taps(s, buf.data_ptr(), 1, None, 0, 0, 4, st) == 0 and lib.emmax_session_taps(s) == 2
    eng.prefill([rows[0]], None)                                                                                 # another pass: the step taps were its rows'
    assert lib.emmax_session_taps(s) == 0
    # beams on / slots open: refused; turning them on unbinds
    assert lib.emmax_session_set_pass_taps(s, buf.data_ptr(), 1, None, 0, 0, st) == 0
    eng.set_beams(BeamParams(2))
    assert lib.emmax_session_taps(s) == 0
    assert lib.emmax_session_set_pass_taps(s, buf.data_ptr(), 1, None, 0, 0, st) == ERR_STATE and "beams" in lib.emmax_last_error().decode()
    eng.clear_beams()
    eng.slots_open(2)
    assert lib.emmax_session_set_pass_taps(s, buf.data_ptr(), 1, None, 0, 0, st) == ERR_STATE and "slots" in lib.emmax_last_error().decode()
    eng.prefill([rows[0]], None)   # a plain prefill ends slot serving
    assert lib.emmax_session_set_pass_taps(s, buf.data_ptr(), 1, None, 0, 0, st) == 0 and lib.emmax_session_clear_taps(s, st) == 0


def test_exact_sessions_refuse_taps(device):
    from emmax import _lib

    cfg, sd, rows = T.tiny_text_case(gqa=True)
    model, _ = _mk(cfg, 13, False, device, max_batch=1, max_prompt=64, max_ctx=400, exact=True)
    eng = model.engine
    buf = torch.zeros(4096, dtype=torch.float32, device=device)
    assert eng.lib.emmax_session_set_pass_taps(eng._session, buf.data_ptr(), 1, None, 0, 0, _lib.current_stream()) == ERR_STATE
    assert "exact" in eng.lib.emmax_last_error().decode()
    with pytest.raises(NotImplementedError, match="exact"):
        model.forward(input_ids=[rows[0]], output_hidden_states=True)
    eng.close()
