"""Extending a cached context through the session (emmax_extend / emmax_slot_extend / emmax_session_context) and the Python layers on top.

  * random tiny weights: prefill P, extend X (|X| crossing a page edge; a ragged B = 3) -- the logits of ALL new rows against the fp32 oracle's
    whole-sequence rows [S, S + n), the cached K / V rows [S, S + n) against the oracle's, then 8 teacher-forced decode steps, eager and with
    the step replayed as a graph; bf16, GQA, fp8 and MXFP4 decode weights (the oracle on the weights the engine evaluates), all at
    FEAT_TOL = 3e-2 max|ref| (tests/test_e2e_gpu.py: the project's written bar).  kv_fp8 sessions against the whole-sequence prefill of the same
    session (tests/test_extend_attn_gpu.py is the tight check of the e4m3 form);
  * planted weights: ids exact -- prefill, generate 6, extend with [pending token] + X, generate 10 = planted_chain from X's last id, B = 1 and a
    ragged B = 3; multi-turn through generate(past_key_values=) and generate_ids(continue_from=) = one prefill of the concatenation; a seeded
    sampled continuation = the sampled run behind a whole-sequence prefill; a constrained continuation emits allowed ids only;
  * forward(input_ids[B, n], past_key_values) = n single-token cached forwards; slots: held contexts and follow-ups; every refusal leaves the
    session usable.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import mxfp4_ref as M4
from test_e2e_gpu import FEAT_TOL, _inputs, _mk, rel

pytestmark = pytest.mark.gpu

T_STEPS = 8
P_LENS, X_LENS = [20, 9, 33], [50, 3, 31]   # contexts 276 / 265 / 289 -> 326 / 268 / 320: row 0 and row 2 cross the page edge at 320 / end on it


def _oracle_rows(cfg, sd_ref, frames, full, sd_decode=None):
    """fp32 oracle over the whole sequences: per row (logits [S, V], [(k, v)] per layer as [S, Hkv, hd]).  sd_decode (fp8 decode weights: the
    de-quantised e4m3 projections and lm-head, which only the decode STEPS stream): the last T_STEPS positions are cached one-token forwards on
    those weights behind a forward of the rest on sd_ref, as the engine computes them"""
    from oracle import emmax_oracle as orc

    out = []
    with torch.inference_mode():
        for b, row in enumerate(full):
            pix = orc.preprocess_frames(frames[b:b + 1], cfg)
            head = row if sd_decode is None else row[:-T_STEPS]
            logits, cache, _ = orc.vla_prefill_logits(torch.tensor([head]), pix, sd_ref, cfg)
            rows = [logits[0].float()]
            if sd_decode is not None:
                for tok in row[-T_STEPS:]:
                    lg, cache = orc.llama_forward(orc.embed_tokens(torch.tensor([[tok]]), sd_decode), sd_decode, cfg.llm, cache)
                    rows.append(lg[0].float())
            out.append((torch.cat(rows), [(k[0].transpose(0, 1).float(), v[0].transpose(0, 1).float()) for k, v in cache]))
    return out


def _dequant_e4m3_rows(w):
    """a decode projection as the fp8 engine streams it: e4m3 x one fp32 scale per row (tests/test_operating_point_gpu.py)"""
    w = w.float()
    scale = (w.abs().amax(dim=1, keepdim=True) / 448.0).clamp_min(1e-30)
    return (w / scale).to(torch.float8_e4m3fn).float() * scale


def _sequences(cfg, seed=99):
    frames, rows = _inputs(cfg, 3, [p + x + T_STEPS for p, x in zip(P_LENS, X_LENS)], seed=seed)
    P = [r[:p] for r, p in zip(rows, P_LENS)]
    X = [r[p:p + x] for r, p, x in zip(rows, P_LENS, X_LENS)]
    Tf = [r[p + x:] for r, p, x in zip(rows, P_LENS, X_LENS)]
    return frames, rows, P, X, Tf


def _kv_rows(eng, layer, row, p0, n):
    from emmax import _lib

    cfg = eng.cfg.llm
    k = np.empty((n, cfg.num_kv_heads, cfg.head_dim), dtype=np.float32)
    v = np.empty_like(k)
    _lib.check(eng.lib.emmax_op_decode_kv_read(eng._session, layer, row, p0, n, None, 0, k.ctypes.data_as(C.POINTER(C.c_float)),
                                               v.ctypes.data_as(C.POINTER(C.c_float)), _lib.current_stream()), "emmax_op_decode_kv_read")
    return torch.from_numpy(k), torch.from_numpy(v)


def _assert_rows_of_the_prefill(k, v, whole, li, what):
    """The appended K / V rows against the rows the SAME session's whole-sequence emmax_prefill writes at the same positions -- the check that
    sees one wrong cos / sin row or page slot, which 3e-2 of max|ref| against the fp32 oracle does not.  Layer 0: bit for bit -- its q / k / v
    rows depend on the token's own embedding alone (RMSNorm and the qkv GEMM are row-wise, the fp32 accumulation over K runs in the same order
    whatever M is), the RoPE pass is bit-identical at equal positions (tests/test_extend_attn_gpu.py) and V is copied.  Deeper layers: the hidden
    rows behind an attention launch of another tiling differ at the bf16 level, so the two results are two bf16 roundings (each within
    prefill_stage_ref.rope_bound() = one rounding of its own exact value) of inputs that themselves differ by a rounding per stage in between:
    they are held to the project's line between two bf16 results, relerr < TOL = 1e-2 (tests/test_ops_gpu.py) -- a third of the logit bar, and a
    rotation by a neighbouring position's angles moves the fast pairs by O(1) of their size."""
    from test_ops_gpu import TOL

    for name, a, b in (("K", k, whole[0]), ("V", v, whole[1])):
        if li == 0:
            assert torch.equal(a, b), f"{what}: {name} rows differ from the whole-sequence prefill's ({int((a != b).sum())} elements, worst {(a - b).abs().max().item():.3g})"
        else:
            e = ((a - b).abs().max() / b.abs().max()).item()
            assert e < TOL, f"{what}: {name} rows {e:.3g} from the whole-sequence prefill's, bound {TOL:.3g}"


def _prefill_extend_steps(model, cfg, frames, P, X, Tf, sel, ref, device, what):
    """prefill P[sel], extend X[sel], T_STEPS teacher-forced steps: every logit row and the new K / V rows against the oracle rows `ref`"""
    eng = model.engine
    n_p = cfg.n_patches
    S = [n_p + len(P[i]) for i in sel]
    # the rows [S, S + n) as the session's own whole-sequence prefill writes them: the tight reference of the appended rows (below)
    model._prefill([P[i] + X[i] for i in sel], None, torch.from_numpy(frames[sel]).to(device), max_new=T_STEPS + 2)
    whole_kv = [[_kv_rows(eng, li, j, S[j], len(X[i])) for li in range(cfg.llm.num_layers)] for j, i in enumerate(sel)]
    model._prefill([P[i] for i in sel], None, torch.from_numpy(frames[sel]).to(device), max_new=max(X_LENS) + T_STEPS + 2)
    assert eng.context_lengths(0, len(sel)) == S
    new_len = eng.extend([X[i] for i in sel], max_new_tokens=T_STEPS + 1)
    assert new_len == [s + len(X[i]) for s, i in zip(S, sel)]
    got = eng.prefill_logits()
    worst = 0.0
    for j, i in enumerate(sel):
        want = ref[i][0][S[j]:S[j] + len(X[i])]
        assert got[j].shape == want.shape
        worst = max(worst, rel(got[j], want))
        for li in range(cfg.llm.num_layers):   # the K / V rows the extension appended
            k, v = _kv_rows(eng, li, j, S[j], len(X[i]))
            rk, rv = ref[i][1][li]
            worst = max(worst, rel(k, rk[S[j]:S[j] + len(X[i])]), rel(v, rv[S[j]:S[j] + len(X[i])]))
            _assert_rows_of_the_prefill(k, v, whole_kv[j][li], li, f"{what} row {i} layer {li}")
    print(f"{what}: extension rows and K / V: worst rel {worst:.4f}")
    assert worst < FEAT_TOL, (what, worst)
    for t in range(T_STEPS):
        eng.set_current_tokens([Tf[i][t] for i in sel])
        eng.decode_step()
        lg = eng.last_logits().float().cpu()
        for j, i in enumerate(sel):
            worst = max(worst, rel(lg[j], ref[i][0][S[j] + len(X[i]) + t]))
    print(f"{what}: + {T_STEPS} teacher-forced steps: worst rel {worst:.4f}")
    assert worst < FEAT_TOL, (what, worst)
    assert eng.context_lengths(0, len(sel)) == [s + len(X[i]) + T_STEPS for s, i in zip(S, sel)]


@pytest.fixture(scope="module", params=["tiny", "gqa"])
def random_model(request, device):
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny(gqa=request.param == "gqa")
    model, sd_ref = _mk(cfg, 13, False, device, max_batch=3, max_prompt=96, max_ctx=400)
    frames, rows, P, X, Tf = _sequences(cfg)
    yield cfg, model, frames, P, X, Tf, _oracle_rows(cfg, sd_ref, frames, rows)
    model.engine.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("sel", [[0], [0, 1, 2]])
def test_extension_rows_kv_and_later_steps_match_the_oracle(device, random_model, tune, sel, graph):
    cfg, model, frames, P, X, Tf, ref = random_model
    tune(graph=graph)
    _prefill_extend_steps(model, cfg, frames, P, X, Tf, sel, ref, device, f"B={len(sel)} graph={graph}")
    if graph:
        assert model.engine.graph_active()


@pytest.fixture(scope="module", params=["fp8", "mxfp4"])
def quantised_model(request, device):
    """fp8 / MXFP4 decode weights, and the oracle on the weights the engine evaluates.  MXFP4: every decode projection de-quantised, prefill and
    decode alike (the prefill's GEMMs read the de-quantised rows).  fp8: the prefill's GEMMs -- the extension's too -- and emmax_prefill_logits
    read the bf16 rows, the decode STEPS stream e4m3 x a scale per row (projections and lm-head): the oracle forwards P + X on the bf16 weights and
    the teacher-forced steps on the de-quantised ones"""
    from emmax.modeling import EmmaXForActionPrediction

    if request.param == "mxfp4":
        cfg = M4.e2e_cfg()
        sd_bf = M4.e2e_state_dict(False, M4.E2E_RANDOM_SEED)
        sd_ref, sd_dec = M4.dequant_state_dict(sd_bf), None
    else:
        from emmax.config import EmmaXConfig
        from emmax.weights import synthetic_state_dict

        cfg = EmmaXConfig.tiny()
        cfg.decode_weight_dtype = "fp8"
        sd_bf = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=13, planted=False).items()}
        sd_ref = {k: v.float() for k, v in sd_bf.items()}
        proj = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
        sd_dec = {k: (_dequant_e4m3_rows(v) if k.startswith("language_model.") and (any(p in k for p in proj) or k.endswith("lm_head.weight")) else v)
                  for k, v in sd_ref.items()}
    model = EmmaXForActionPrediction(cfg, dict(sd_bf)).to(device, max_batch=3, max_prompt=96, max_ctx=400)
    frames, rows, P, X, Tf = _sequences(cfg)
    yield request.param, cfg, model, frames, P, X, Tf, _oracle_rows(cfg, sd_ref, frames, rows, sd_dec)
    model.engine.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_extension_on_quantised_decode_weights(device, quantised_model, tune, graph):
    """the new rows' logits, the appended K / V rows and 8 later steps against the oracle on the de-quantised weights, eager and replayed"""
    dtype, cfg, model, frames, P, X, Tf, ref = quantised_model
    tune(graph=graph)
    _prefill_extend_steps(model, cfg, frames, P, X, Tf, [0, 1, 2], ref, device, f"{dtype} B=3 graph={graph}")
    if graph:
        assert model.engine.graph_active()


def _forced_steps(eng, Tf, sel):
    out = []
    for t in range(T_STEPS):
        eng.set_current_tokens([Tf[i][t] for i in sel])
        eng.decode_step()
        out.append(eng.last_logits().float().cpu())
    return out


def test_kv_fp8_extension_equals_the_whole_sequence_prefill(device):
    """fp8 KV cache: extension rows, the rows' de-quantised K / V and the later steps against the whole-sequence emmax_prefill of the same session"""
    from emmax import _lib
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny(gqa=True)
    with _lib.tuning(kv_fp8=1):
        model, _ = _mk(cfg, 13, False, device, max_batch=3, max_prompt=96, max_ctx=400)
    eng, sel = model.engine, [0, 1, 2]
    frames, rows, P, X, Tf = _sequences(cfg)
    fr = torch.from_numpy(frames).to(device)
    model._prefill([P[i] + X[i] for i in sel], None, fr, max_new=T_STEPS + 2)
    S = [cfg.n_patches + len(P[i]) for i in sel]
    whole = [g[S[j]:].float().cpu() for j, g in enumerate(eng.prefill_logits())]
    whole_kv = [[_kv_rows(eng, li, j, S[j], len(X[j])) for li in range(cfg.llm.num_layers)] for j in sel]
    whole_steps = _forced_steps(eng, Tf, sel)
    model._prefill([P[i] for i in sel], None, fr, max_new=max(X_LENS) + T_STEPS + 2)
    eng.extend([X[i] for i in sel], max_new_tokens=T_STEPS + 1)
    worst, worst_kv, flipped, total = 0.0, 0.0, 0, 0
    for j, g in enumerate(eng.prefill_logits()):
        worst = max(worst, rel(g, whole[j]))
        for li in range(cfg.llm.num_layers):
            # the e4m3 rows of two runs whose inputs differ at the bf16 level: equal, or ONE code apart -- 2^-3 relative (3 mantissa bits), 2^-9 of
            # the row's largest value below the normal range -- at the COARSER of the two runs' row scales: the scale is the power of two above
            # amax / 448, and a row whose amax sits at a threshold takes the next one in one of the runs (every step twice as wide): 2 steps
            for a, b in zip(_kv_rows(eng, li, j, S[j], len(X[j])), whole_kv[j][li]):
                if li == 0:   # the same bf16 rows in (see _assert_rows_of_the_prefill): the same e4m3 bytes and the same scale out
                    assert torch.equal(a, b), f"kv_fp8 layer 0 row {j}: {int((a != b).sum())} elements differ from the whole-sequence prefill's"
                step = 0.125 * torch.maximum(a.abs(), b.abs()) + 2.0 ** -9 * b.abs().amax(dim=-1, keepdim=True)
                worst_kv = max(worst_kv, ((a - b).abs() / step).max().item())
                flipped += int((a != b).sum())
                total += a.numel()
    for a, b in zip(_forced_steps(eng, Tf, sel), whole_steps):
        worst = max(worst, rel(a, b))
    print(f"kv_fp8: logits worst rel against the whole-sequence prefill {worst:.4f}; K / V: {flipped} of {total} elements differ, worst {worst_kv:.3f} code steps")
    assert worst < FEAT_TOL, worst
    assert worst_kv <= 2.0, (worst_kv, flipped, total)
    eng.close()


# ---- planted weights: ids exact ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(device):
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny()
    model, _ = _mk(cfg, 5, True, device, max_batch=3, max_prompt=96, max_ctx=400)
    yield cfg, model
    model.engine.close()


def _planted_rows(cfg, B, steps, seed=31):
    from emmax.weights import planted_start_token

    frames, rows = _inputs(cfg, B, [10, 17, 5][:B], seed=seed)
    for b in range(B):
        rows[b][-1] = planted_start_token(cfg, steps[b])
    return frames, rows


def _turn_two(cfg, B, seed=47):
    """X per row: random ordinary ids ending in a start token 3 / 5 / 2 ordinary steps before the action prefix"""
    from emmax.weights import planted_start_token

    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.integers(3, 31744, size=n)] + [planted_start_token(cfg, k)] for n, k in zip([59, 4, 12][:B], [3, 5, 2][:B])]


@pytest.mark.parametrize("B", [1, 3])
def test_planted_generate_extend_generate_is_exact(device, planted, B):
    from emmax.weights import planted_chain

    cfg, model = planted
    eng = model.engine
    frames, rows = _planted_rows(cfg, B, [20, 30, 25])   # (far from the action prefix: 6 tokens leave every row running)
    X = _turn_two(cfg, B)
    fr = torch.from_numpy(frames).to(device)

    def run(sel):
        ids, lens, h = model.generate_ids([rows[i] for i in sel], frames_u8=fr[sel].contiguous(), max_new_tokens=6, return_handle=True)
        first = [ids[j, : int(lens[j])].cpu().tolist() for j in range(len(sel))]
        assert all(len(f) == 6 for f in first) and h.lengths == [cfg.n_patches + len(rows[i]) + 5 for i in sel]   # the 6th token is pending, not cached
        ids2, lens2, h2 = model.generate_ids([[first[j][-1]] + X[i] for j, i in enumerate(sel)], continue_from=h, max_new_tokens=10, return_handle=True)
        assert h2.n_patches == cfg.n_patches and all(b > a for a, b in zip(h.lengths, h2.lengths))
        return first, [ids2[j, : int(lens2[j])].cpu().tolist() for j in range(len(sel))]

    first, second = run(list(range(B)))
    for b in range(B):
        assert first[b] == planted_chain(cfg, rows[b][-1], 6)
        assert second[b] == planted_chain(cfg, X[b][-1], 10), (b, second[b])
    if B > 1:   # every row of the ragged batch equals its bs = 1 run
        for b in range(B):
            f1, s1 = run([b])
            assert f1[0] == first[b] and s1[0] == second[b]


def test_multi_turn_equals_one_prefill_of_the_concatenation(device, planted):
    cfg, model = planted
    frames, rows = _planted_rows(cfg, 1, [20])
    X = _turn_two(cfg, 1)[0]
    fr = torch.from_numpy(frames).to(device)
    out1 = model.generate(torch.tensor(rows), frames_u8=fr, max_new_tokens=6, return_dict_in_generate=True)
    seq1 = out1.sequences[0].tolist()
    assert out1.past_key_values.lengths == [cfg.n_patches + len(seq1) - 1]
    full = seq1 + X
    out2 = model.generate(torch.tensor([full]), past_key_values=out1.past_key_values, max_new_tokens=10, return_dict_in_generate=True)
    one = model.generate(torch.tensor([full]), frames_u8=fr, max_new_tokens=10)
    assert out2.sequences[0].tolist() == one[0].tolist()
    assert out2.past_key_values.lengths == [cfg.n_patches + out2.sequences.shape[1] - 1]
    # generate_ids(continue_from=) says the same
    _, _, h = model.generate_ids(rows, frames_u8=fr, max_new_tokens=6, return_handle=True)
    ids, lens = model.generate_ids([full[len(rows[0]) + 5:]], continue_from=h, max_new_tokens=10)
    assert ids[0, : int(lens[0])].cpu().tolist() == one[0, len(full):].tolist()
    # refusals in the style of the others, before the engine is touched
    for kw in (dict(num_beams=2), dict(num_return_sequences=2, do_sample=True), dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2)):
        with pytest.raises(NotImplementedError):
            model.generate(torch.tensor([full]), past_key_values=out2.past_key_values, max_new_tokens=4, **kw)


def test_sampled_and_constrained_continuations(device, planted):
    from emmax.constraints import action_bins
    from emmax.sampling import SamplingParams

    cfg, model = planted
    frames, rows = _planted_rows(cfg, 1, [20])
    X = _turn_two(cfg, 1)[0]
    fr = torch.from_numpy(frames).to(device)
    sp = SamplingParams(temperature=0.8, top_k=40, top_p=0.95, seed=1234)
    _, _, h = model.generate_ids(rows, frames_u8=fr, max_new_tokens=1, return_handle=True)   # caches the prompt alone
    ids, lens, lp = model.generate_ids([X], continue_from=h, max_new_tokens=10, sampling=sp, return_logprobs=True)
    ids_w, lens_w, lp_w = model.generate_ids([rows[0] + X], frames_u8=fr, max_new_tokens=10, sampling=sp, return_logprobs=True)
    n = int(lens[0])
    assert n == int(lens_w[0]) and ids[0, :n].tolist() == ids_w[0, :n].tolist()          # planted margins: the same draws pick the same ids
    assert (lp[0, :n] - lp_w[0, :n]).abs().max().item() < FEAT_TOL * 16                  # log-probabilities: the logit tolerance at |logit| <= 16
    # a constrained continuation emits only what the automaton allows: 7 action bins, then EOS
    _, _, h = model.generate_ids(rows, frames_u8=fr, max_new_tokens=1, return_handle=True)
    aut = action_bins(cfg.llm.vocab_size, cfg.n_action_bins, 7, token_vocab=model.vocab_size)
    ids, lens = model.generate_ids([X], continue_from=h, max_new_tokens=12, constraint=aut)
    got = ids[0, : int(lens[0])].tolist()
    lo = model.vocab_size - cfg.n_action_bins
    assert len(got) >= 7 and all(lo <= t < model.vocab_size for t in got[:7]) and got[7:] in ([], [cfg.eos_token_id]), got


def test_forward_with_past_key_values_serves_many_tokens(device, planted):
    cfg, model = planted
    frames, rows = _inputs(cfg, 2, [12, 12], seed=3)
    new = _inputs(cfg, 2, [6, 6], seed=4)[1]
    fr = torch.from_numpy(frames).to(device)
    out = model.forward(input_ids=torch.tensor(rows), frames_u8=fr, use_cache=True)
    h = out.past_key_values
    base = list(h.lengths)
    many = model.forward(input_ids=torch.tensor(new), past_key_values=h)
    assert tuple(many.logits.shape) == (2, 6, cfg.llm.vocab_size) and h.lengths == [b + 6 for b in base]
    assert model.engine.context_lengths(0, 2) == h.lengths
    got = many.logits.float().cpu()
    out = model.forward(input_ids=torch.tensor(rows), frames_u8=fr, use_cache=True)
    h = out.past_key_values
    for t in range(6):
        one = model.forward(input_ids=torch.tensor([[r[t]] for r in new]), past_key_values=h).logits[:, 0].float().cpu()
        assert rel(got[:, t], one) < FEAT_TOL, t
    assert h.lengths == [b + 6 for b in base]
    ragged = model.forward(input_ids=[new[0][:2], new[1][:5]], past_key_values=h)     # ragged rows: a list of per-row logits
    assert [tuple(t.shape) for t in ragged.logits] == [(2, cfg.llm.vocab_size), (5, cfg.llm.vocab_size)] and h.lengths == [base[0] + 8, base[1] + 11]


# ---- slots -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
def test_held_slots_take_follow_ups_while_the_others_decode(device, planted, overlap):
    from emmax.serving import Request, SlotScheduler
    from emmax.weights import planted_chain

    cfg, model = planted
    eng = model.engine
    frames, rows = _inputs(cfg, 5, [10, 17, 5, 8, 12], seed=61)
    from emmax.weights import planted_start_token

    for b, k in enumerate([3, 6, 30, 2, 4]):
        rows[b][-1] = planted_start_token(cfg, k)
    X = _turn_two(cfg, 2, seed=71)
    fr = torch.from_numpy(frames).to(device)
    encode = lambda fs: [eng.vision_encode(f[None].contiguous())[0] for f in fs]
    sch = SlotScheduler(eng, encode, n_slots=3, poll_every=2, overlap=overlap)   # (overlap: ordinary requests are staged beside the steps;
    budget = {0: 6, 1: 8, 2: 24, 3: 40, 4: 40}                                   # follow-ups always go onto their slot between two steps)
    for i in (0, 1, 2, 3):   # two held requests and two ordinary ones on three slots
        sch.submit(Request(i, fr[i], rows[i], max_new_tokens=budget[i], hold=i in (0, 1)))
    first = {r.rid: r for r in sch.run()}
    for i in (0, 1, 2, 3):
        assert first[i].ids == planted_chain(cfg, rows[i][-1], 40)[:budget[i]], i
    assert set(sch.held) == {first[0].slot, first[1].slot}
    # a follow-up on each held context while an ordinary request decodes beside them; a queued one waits for a release
    sch.results.clear()
    sch.submit(Request(4, fr[4], rows[4], max_new_tokens=40))
    for j, i in enumerate((0, 1)):
        sch.submit(Request(("f", i), None, [first[i].ids[-1]] + X[j], max_new_tokens=12, follow_up=first[i].context))
    second = {r.rid: r for r in sch.run()}
    assert second[4].ids == planted_chain(cfg, rows[4][-1], 40)          # the other slot's ids are unchanged by the extensions beside it
    for j, i in enumerate((0, 1)):
        assert second[("f", i)].ids == planted_chain(cfg, X[j][-1], 12) and second[("f", i)].slot == first[i].slot
    assert not sch.held and all(d for d in eng.slots_state()[0][:3])


def test_held_context_multi_turn_equals_bs1_and_release_frees_the_slot(device, planted):
    from emmax.serving import Request, SlotScheduler

    cfg, model = planted
    eng = model.engine
    frames, rows = _planted_rows(cfg, 2, [20, 25], seed=83)
    X = _turn_two(cfg, 1, seed=89)[0]
    fr = torch.from_numpy(frames).to(device)
    ids1, lens1, h = model.generate_ids([rows[0]], frames_u8=fr[:1].contiguous(), max_new_tokens=6, return_handle=True)
    t1 = ids1[0, : int(lens1[0])].tolist()
    ids2, lens2 = model.generate_ids([[t1[-1]] + X], continue_from=h, max_new_tokens=10)
    t2 = ids2[0, : int(lens2[0])].tolist()
    encode = lambda fs: [eng.vision_encode(f[None].contiguous())[0] for f in fs]
    sch = SlotScheduler(eng, encode, n_slots=1, poll_every=1, overlap=False)
    sch.submit(Request(0, fr[0], rows[0], max_new_tokens=6, hold=True))
    (r0,) = sch.run()
    assert r0.ids == t1
    sch.results.clear()
    sch.submit(Request(1, None, [t1[-1]] + X, max_new_tokens=10, follow_up=r0.context, hold=True))
    (r1,) = sch.run()
    assert r1.ids == t2 and r1.slot == r0.slot
    sch.submit(Request(2, fr[1], rows[1], max_new_tokens=4))
    with pytest.raises(RuntimeError, match="held"):
        sch.run()
    sch.release(r1.context)
    sch.results.clear()
    (r2,) = sch.run()
    assert r2.rid == 2 and len(r2.ids) == 4


def test_a_held_slot_keeps_its_cache_while_its_neighbours_decode(device, random_model):
    """RANDOM weights (planted ids follow from the last token alone and would not see a damaged context): a finished request's slot is held while
    the other slots decode on, then extended.  Its cached K / V rows are bit for bit what they were when it finished -- a done row's step writes
    nothing below its context length -- and the new rows' logits equal the bs = 1 run's: the same launches on the same inputs, held to the
    project's line between two bf16 results (tests/test_ops_gpu.py TOL)."""
    from test_ops_gpu import TOL

    cfg, model, frames, P, X, Tf, ref = random_model
    eng = model.engine
    fr = torch.from_numpy(frames).to(device)
    S = cfg.n_patches + len(P[0])
    model._prefill([P[0]], None, fr[:1].contiguous(), max_new=80)   # bs = 1: the extension drops the pending first token, as the held slot does
    eng.extend([X[0]], max_new_tokens=4)
    want = eng.prefill_logits()[0].float().cpu()
    pe = eng.vision_encode(fr)
    eng.slots_open(3)
    eng.slot_prefill(0, P[0], pe[0], 1)    # its one token is the prefill's: done at the next step, context S
    eng.slot_prefill(1, P[1], pe[1], 60)
    eng.slot_prefill(2, P[2], pe[2], 60)
    eng.slots_step(2)
    done, n_out = eng.slots_state()
    assert done[0] and not done[1] and not done[2] and eng.context_lengths(0, 1) == [S]
    before = [_kv_rows(eng, li, 0, 0, S) for li in range(cfg.llm.num_layers)]
    eng.slots_step(20)                      # the neighbours decode 20 tokens beside the held slot
    done, n_out = eng.slots_state()
    assert done[0] and n_out[1] == n_out[2] == 23 and eng.context_lengths(0, 1) == [S]
    for li, (k0, v0) in enumerate(before):
        k1, v1 = _kv_rows(eng, li, 0, 0, S)
        assert torch.equal(k0, k1) and torch.equal(v0, v1), f"layer {li}: the held slot's cached rows changed while the others decoded"
    others = [eng.slot_output(1, 23), eng.slot_output(2, 23)]
    eng.slot_extend(0, X[0], 4)
    got = eng.prefill_logits()[0].float().cpu()
    assert got.shape == want.shape and rel(got, want) < TOL, rel(got, want)
    assert rel(got, ref[0][0][S:S + len(X[0])]) < FEAT_TOL     # ... and the oracle's rows
    done, _ = eng.slots_state()
    assert not done[0] and eng.context_lengths(0, 1) == [S + len(X[0])]
    eng.slots_step(2)
    assert [eng.slot_output(1, 23), eng.slot_output(2, 23)] == others and eng.slots_state()[1][1] == 25   # the neighbours: untouched, and decoding on


def test_a_slot_inside_a_fork_group_is_not_extended(device, random_model):
    from emmax import _lib
    from emmax.sampling import SamplingParams

    cfg, model, frames, P, X, Tf, ref = random_model
    eng = model.engine
    pe = eng.vision_encode(torch.from_numpy(frames).to(device))
    p = SamplingParams(temperature=1.0, top_k=0, top_p=1.0, seed=77)
    eng.slots_open(3)
    eng.set_sampling([p], [p.seed], [0], row0=0)
    eng.slot_prefill(0, P[0], pe[0], 1)
    eng.slots_fork(0, [1], [p], [p.seed], [1])
    eng.slots_step(2)                        # both members finish (budget 1)
    for slot in (0, 1):                      # the owner and the follower: their prompt pages are shared
        with pytest.raises(_lib.EmmaxError, match="sample group") as e:
            eng.slot_extend(slot, X[0], 4)
        assert "status -5" in str(e.value)
    eng.slot_release(1)
    eng.slot_release(0)
    eng.slot_prefill(0, P[0], pe[0], 1)      # the session serves on: a slot of its own is prefilled, finishes and is extended
    eng.slots_step(2)
    eng.slot_extend(0, X[0], 4)
    assert eng.context_lengths(0, 1) == [cfg.n_patches + len(P[0]) + len(X[0])]
    eng.slots_open(3)
    eng.clear_sampling()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_usable(device, planted):
    from emmax import _lib
    from emmax.sampling import BeamParams, LogitsProcessing, SamplingParams
    from emmax.weights import planted_chain

    cfg, model = planted
    eng = model.engine
    frames, rows = _planted_rows(cfg, 1, [20])
    fr = torch.from_numpy(frames).to(device)
    X = _turn_two(cfg, 1)[0]

    def fresh():
        model._prefill(rows, None, fr, max_new=80)

    def refused(code_word, msg):
        with pytest.raises(_lib.EmmaxError, match=msg) as e:
            eng.extend([X], max_new_tokens=10)
        assert f"status {code_word}" in str(e.value)

    fresh()
    eng.set_processing(LogitsProcessing(repetition_penalty=1.3), n=1)
    refused(-5, "max_prompt")                                   # history-reading processors: the message says why
    eng.clear_processing()
    eng.set_beams(BeamParams(num_beams=2))
    refused(-5, "beams")
    eng.clear_beams()
    eng.set_sampling(SamplingParams(temperature=1.0, top_k=0, top_p=1.0, seed=1), n=1)
    eng.set_sample_groups(2)
    refused(-5, "sample groups")
    eng.clear_sample_groups()
    eng.clear_sampling()
    fresh()
    room = eng.max_ctx - eng.context_lengths(0, 1)[0] - len(X)   # (max_ctx is the session's: an earlier forward(use_cache=True) may have raised it)
    with pytest.raises(_lib.EmmaxError, match="max_ctx") as e:   # capacity: context + new ids + tokens to generate one past max_ctx
        eng.extend([X], max_new_tokens=room + 1)
    assert "status -3" in str(e.value)
    with pytest.raises(_lib.EmmaxError, match="cache_reserve"):  # more new rows than the prefill holds: never a re-created session
        eng.extend([[5] * (eng.max_batch * (cfg.n_patches + eng.max_prompt) + 1)])
    epoch = eng.session_epoch
    eng.extend([X], max_new_tokens=10)                           # after all of them: the session extends and generates
    ids, lens = eng.generate(10)
    assert ids[0, : int(lens[0])].tolist() == planted_chain(cfg, X[-1], 10) and eng.session_epoch == epoch
    # exact numerics, and no prefill yet
    from emmax.config import EmmaXConfig

    xm, _ = _mk(EmmaXConfig.tiny(), 5, True, device, max_batch=1, max_prompt=32, max_ctx=330, exact=True)
    with pytest.raises(_lib.EmmaxError, match="exact"):
        xm.engine.extend([X[:4]])
    xm._prefill(rows, None, fr, max_new=8)
    with pytest.raises(_lib.EmmaxError, match="exact"):
        xm.engine.extend([X[:4]])
    ids, lens = xm.engine.generate(4)
    assert int(lens[0]) == 4
    xm.engine.close()
