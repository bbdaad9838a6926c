"""Draft-verified greedy decoding through the session (emmax_verify, emmax_session_set_budget, emmax_session_output) and the Python layers on top
(engine.verify, drafting.drafted_generate, generate_ids(draft=), generate(draft_ids= / prompt_lookup_num_tokens=), predict_action(draft_ids=),
OpenVLAInference(reuse_reasoning=True)).

  * planted weights (bf16, GQA, MXFP4 decode weights, fp8 KV cache; B = 1 and a ragged B = 3): whatever the draft says -- the true chain, the chain
    with substitutions at the first, an inner and the last position of a window, a deletion, an insertion, an unrelated draft, a draft shorter than
    the answer -- ids, lens and cached lengths are those of the plain run and of planted_chain; so are a stop rule and a budget that cut inside an
    accepted run, and a continue_from follow-up behind a drafted call.
  * random weights (planted ids follow from the last token alone: only these see a wrong rollback): prefill, 3 plain steps, one verify pass over the
    session's own greedy continuation corrupted at position j -- emitted == j + 1, the cached lengths, the window rows' logits and the kept K / V rows
    against the fp32 oracle, then 8 teacher-forced steps on the sequence actually cached (a stale key past the rollback point or a wrong ctx_len
    shows there), all at FEAT_TOL = 3e-2 max|ref| (tests/test_e2e_gpu.py); the fp8 KV cache against the same session's whole-sequence prefill.
  * free-running on random weights, drafted against plain, every token against the oracle's argmax above the project's a-priori id line.
  * every refusal of emmax_verify raises its message and leaves the session usable (the plain run's ids afterwards); fp8-weight and
    exact-numerics models refuse a draft; the model-level entry points.  (The Python refusals before the engine is touched: tests/test_draft_refusals.py.)
"""
import numpy as np
import pytest
import torch

import mxfp4_ref as M4
from conftest import ID_BUDGET_SHALLOW, above_id_line
from test_e2e_gpu import FEAT_TOL, _inputs, _mk, rel
from test_extend_session_gpu import _kv_rows, _oracle_rows

pytestmark = pytest.mark.gpu

WINDOW = 16          # the planted runs' window: several windows per answer, so that every position of a window is exercised
STEPS = [40, 23, 31]  # ordinary steps before the action prefix per row: answers of 49 / 32 / 40 ids (+ 7 action ids, + EOS)
MAX_NEW = 64


def _params(**kw):
    from emmax.drafting import DraftParams

    return DraftParams(**{"window": WINDOW, **kw})


# ---- planted weights: ids exact -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["bf16", "gqa", "mxfp4", "kv_fp8"])
def planted(request, device):
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction

    kind = request.param
    if kind == "mxfp4":
        cfg = M4.e2e_cfg()
        model = EmmaXForActionPrediction(cfg, dict(M4.e2e_state_dict(True, M4.E2E_PLANTED_SEED))).to(device, max_batch=3, max_prompt=96, max_ctx=480)
    else:
        cfg = EmmaXConfig.tiny(gqa=kind == "gqa")
        with _lib.tuning(**({"kv_fp8": 1} if kind == "kv_fp8" else {})):
            model, _ = _mk(cfg, 5, True, device, max_batch=3, max_prompt=96, max_ctx=480)
    yield kind, cfg, model
    model.engine.close()


def _planted_rows(cfg, B, seed=31):
    from emmax.weights import planted_start_token

    frames, rows = _inputs(cfg, B, [10, 17, 5][:B], seed=seed)
    for b in range(B):
        rows[b][-1] = planted_start_token(cfg, STEPS[b])
    return frames, rows


def _drafts(chain, rng):
    """the drafts of the issue for one answer: name -> ids"""
    def sub(at):
        d = list(chain)
        for k in at:
            d[k] = 3 + (d[k] + 17) % 30000
        return d
    w = WINDOW - 1   # draft ids per window: the first window covers chain[1 .. w]
    return {
        "true": list(chain),
        "sub-first-inner-last": sub([1, 1 + w // 2, w, w + 1]),   # the first, an inner and the last draft id of the first window, the first of the second
        "deletion": chain[:20] + chain[21:],
        "insertion": chain[:20] + [12345] + chain[20:],
        "unrelated": [int(x) for x in rng.integers(3, 30000, size=len(chain))],
        "short": chain[:len(chain) // 3],
    }


def _run(model, rows, fr, draft=None, max_new=MAX_NEW, **kw):
    if draft is not None:
        kw.update(draft=draft, draft_params=_params(), return_draft_stats=True)
    res = model.generate_ids(rows, frames_u8=fr, max_new_tokens=max_new, **kw)
    ids, lens = res[0], res[1]
    out = [ids[b, : int(lens[b])].cpu().tolist() for b in range(len(rows))]
    assert all(int(x) == model.config.pad_token_id for b in range(len(rows)) for x in ids[b, int(lens[b]):].cpu().tolist())
    return out, model.engine.context_lengths(0, len(rows)), res[2:]


@pytest.mark.parametrize("B", [1, 3])
def test_planted_drafted_runs_equal_the_plain_run(device, planted, B):
    from emmax.weights import planted_chain

    kind, cfg, model = planted
    frames, rows = _planted_rows(cfg, B)
    fr = torch.from_numpy(frames).to(device)
    plain, plain_ctx, _ = _run(model, rows, fr)
    chains = [planted_chain(cfg, rows[b][-1], MAX_NEW) for b in range(B)]
    assert plain == chains and all(len(c) >= 30 for c in chains)
    rng = np.random.default_rng(5)
    per_row = [_drafts(c, rng) for c in chains]
    for name in per_row[0]:
        # (ragged batch: every row another kind of draft, rotating -- and one row without a draft at all)
        names = [list(per_row[0])[(list(per_row[0]).index(name) + b) % len(per_row[0])] for b in range(B)]
        draft = [per_row[b][names[b]] for b in range(B)]
        if B == 3 and name == "short":
            draft[1] = None
        got, ctx, (stats,) = _run(model, rows, fr, draft=draft)
        assert got == plain, (kind, names, stats)
        assert ctx == plain_ctx, (kind, names)
        print(f"{kind} B={B} {names}: {stats.passes} passes, {stats.plain_steps} plain steps, accepted {stats.accepted} of {stats.drafted}")
        if B == 1 and name == "true":
            assert stats.plain_steps <= 1 and stats.passes <= -(-max(len(c) for c in chains) // WINDOW) + 1 and stats.accepted[0] >= len(chains[0]) - 2 - stats.passes
        if B == 1 and name == "unrelated":
            assert stats.passes == _params().give_up and stats.accepted == [0]


def test_stop_rule_and_budget_cut_inside_an_accepted_run(device, planted):
    kind, cfg, model = planted
    eng = model.engine
    frames, rows = _planted_rows(cfg, 3)
    fr = torch.from_numpy(frames).to(device)
    full, _, _ = _run(model, rows, fr)
    for max_new in (WINDOW + 5, 2 * WINDOW, 1, 2):   # the budget ends inside a window, at a window's last row, before any pass, at the first
        plain, ctx, _ = _run(model, rows, fr, max_new=max_new)
        got, ctx2, _ = _run(model, rows, fr, draft=[list(f) for f in full], max_new=max_new)
        assert got == plain and ctx2 == ctx and all(len(g) == min(max_new, len(f)) for g, f in zip(got, full)), (kind, max_new)
    # the stop rule: two ids of row 0's answer as the trigger (the second pass completes it: the first ends between them), 3 tokens after it
    k = WINDOW
    try:
        eng.set_stop(full[0][k:k + 2], 3)       # (the first pass emits ids 1 .. k: its last token is the trigger's first id)
        plain, ctx, _ = _run(model, rows, fr)
        assert len(plain[0]) == k + 2 + 3
        got, ctx2, _ = _run(model, rows, fr, draft=[list(f) for f in full])
        assert got == plain and ctx2 == ctx, kind
    finally:
        eng.set_stop((), 0)


def test_a_follow_up_continues_a_drafted_call(device, planted):
    kind, cfg, model = planted
    from emmax.weights import planted_chain, planted_start_token

    frames, rows = _planted_rows(cfg, 1)
    fr = torch.from_numpy(frames).to(device)
    X = [int(x) for x in np.random.default_rng(3).integers(3, 30000, size=9)] + [planted_start_token(cfg, 6)]

    def two_calls(draft):
        kw = {} if draft is None else dict(draft=[draft], draft_params=_params())
        ids, lens, h = model.generate_ids(rows, frames_u8=fr, max_new_tokens=30, return_handle=True, **kw)
        first = ids[0, : int(lens[0])].cpu().tolist()
        kw = {} if draft is None else dict(draft=[planted_chain(cfg, X[-1], 12)], draft_params=_params())
        ids2, lens2, h2 = model.generate_ids([[first[-1]] + X], continue_from=h, max_new_tokens=12, return_handle=True, **kw)
        return first, ids2[0, : int(lens2[0])].cpu().tolist(), h.lengths, h2.lengths

    want = two_calls(None)
    assert two_calls(planted_chain(cfg, rows[0][-1], 30)) == want
    assert want[1] == planted_chain(cfg, X[-1], 12)


# ---- random weights: the rollback ---------------------------------------------------------------------------------------------------------------
P_LENS = [20, 9, 33]   # contexts 276 / 265 / 289; + 3 plain steps: the window's first row sits at 279 / 268 / 292
N_WIN = [60, 12, 40]   # windows over positions 279..338 (the page edge 320 at row 41), 268..279, 292..331 (row 28)
T_FORCED = 8
# `emitted == j + 1` needs the pass (GEMM rows) and the plain steps (GEMV / MFMA decode rows) to pick the same ids along the continuation, which two
# correct implementations only do where the ids are not near-ties.  The weights / inputs seeds are therefore chosen, on the CPU and before any GPU run,
# so that the fp32 oracle's own greedy continuation of all three rows keeps its top-2 margin above the project's id line (2 x ID_BUDGET_SHALLOW = 3e-2 of
# max|logit|) at every one of its first 68 tokens: seeds (5, 100) -- margins >= 0.035, two ids alternating; the fp8-cache GQA model (1, 99) -- >= 0.077.
# (Most seed pairs of the tiny random model run into near-ties: (13, 99), the pair of tests/test_extend_session_gpu.py, has a margin of 7e-4 at token 28.)
RANDOM_SEED, RANDOM_INPUT_SEED = 5, 100
KV8_SEED, KV8_INPUT_SEED = 1, 99


def _greedy(model, eng, rows, fr, n):
    model._prefill(rows, None, fr, max_new=n)
    ids, lens = eng.generate(n)
    assert all(int(x) == n for x in lens.cpu().tolist()), "a random-weight row hit EOS: choose another seed"
    return [ids[b].cpu().tolist() for b in range(len(rows))]


def _corrupt(tok):
    return 3 + (tok + 1000) % 30000


def _rollback_case(model, cfg, sd_ref, frames, rows, sel, js, device, what, whole_session=False):
    """prefill rows[sel], 3 plain steps, one verify over the greedy continuation corrupted behind row js[.]: the assertions of the module docstring.
    whole_session: the references are the same session's whole-sequence prefills instead of the fp32 oracle (fp8 KV cache)."""
    eng = model.engine
    fr = torch.from_numpy(frames[sel]).to(device).contiguous()
    prompts = [rows[i] for i in sel]
    n = [N_WIN[i] for i in sel]
    g = _greedy(model, eng, prompts, fr, 4 + max(n) + 1)                     # t0 .. : the session's own plain greedy continuation
    tf = [[int(x) for x in np.random.default_rng(100 + i).integers(3, 30000, size=T_FORCED)] for i in sel]
    windows = []
    for b in range(len(sel)):
        w = g[b][3:3 + n[b]]                                                 # the pending token t3, then t4 ..
        if js[b] is not None:
            w[js[b] + 1] = _corrupt(w[js[b] + 1])
        windows.append(w)
    want_emitted = [n[b] if js[b] is None else js[b] + 1 for b in range(len(sel))]
    L = [cfg.n_patches + len(p) + 3 for p in prompts]
    seq_a = [prompts[b] + g[b][:3] + windows[b] for b in range(len(sel))]                            # what the pass sees
    seq_b = [prompts[b] + g[b][:3] + windows[b][:want_emitted[b]] + tf[b] for b in range(len(sel))]  # what is cached once the forced steps ran
    if whole_session:
        def whole(seqs):
            model._prefill(seqs, None, fr, max_new=2)
            return [x.float().cpu() for x in eng.prefill_logits()]
        ref_a, ref_b, ref_kv = whole(seq_a), whole(seq_b), None
    else:
        all_frames = np.concatenate([frames[sel], frames[sel]])
        oracle = _oracle_rows(cfg, sd_ref, all_frames, seq_a + seq_b)
        ref_a, ref_b = [o[0] for o in oracle[:len(sel)]], [o[0] for o in oracle[len(sel):]]
        ref_kv = [o[1] for o in oracle[:len(sel)]]
    model._prefill(prompts, None, fr, max_new=4 + max(n) + T_FORCED + 2)
    eng.set_budget(200)
    for _ in range(3):
        eng.decode_step()
    tail, n_out, done = eng.output_tail(0, 4)
    assert tail == [x[:4] for x in g] and n_out == [4] * len(sel) and done == [0] * len(sel)
    assert eng.context_lengths(0, len(sel)) == L
    emitted, new_ids, done = eng.verify(windows, max_new=200)
    print(f"{what}: emitted {emitted} (want {want_emitted})")
    assert emitted == want_emitted and done == [0] * len(sel)
    for b in range(len(sel)):   # the accepted guess ids, then the model's own token behind the last kept row
        assert new_ids[b][:-1] == windows[b][1:emitted[b]]
        assert new_ids[b][-1] == g[b][3 + emitted[b]]
    assert eng.context_lengths(0, len(sel)) == [l + e for l, e in zip(L, emitted)]
    assert eng.output_tail(4, 1)[1] == [4 + e for e in emitted]
    worst = 0.0
    got = eng.prefill_logits()
    for b in range(len(sel)):
        assert got[b].shape[0] == n[b]
        worst = max(worst, rel(got[b], ref_a[b][L[b]:L[b] + n[b]]))
        if ref_kv is not None:
            for li in range(cfg.llm.num_layers):
                k, v = _kv_rows(eng, li, b, L[b], emitted[b])
                rk, rv = ref_kv[b][li]
                worst = max(worst, rel(k, rk[L[b]:L[b] + emitted[b]]), rel(v, rv[L[b]:L[b] + emitted[b]]))
    print(f"{what}: window rows and kept K / V: worst rel {worst:.4f}")
    assert worst < FEAT_TOL, (what, worst)
    for t in range(T_FORCED):
        eng.set_current_tokens([tf[b][t] for b in range(len(sel))])
        eng.decode_step()
        lg = eng.last_logits().float().cpu()
        for b in range(len(sel)):
            worst = max(worst, rel(lg[b], ref_b[b][L[b] + emitted[b] + t]))
    print(f"{what}: + {T_FORCED} teacher-forced steps: worst rel {worst:.4f}")
    assert worst < FEAT_TOL, (what, worst)
    assert eng.context_lengths(0, len(sel)) == [l + e + T_FORCED for l, e in zip(L, emitted)]


@pytest.fixture(scope="module")
def random_model(device):
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny()
    model, sd_ref = _mk(cfg, RANDOM_SEED, False, device, max_batch=3, max_prompt=160, max_ctx=480)
    frames, rows = _inputs(cfg, 3, P_LENS, seed=RANDOM_INPUT_SEED)
    yield cfg, model, sd_ref, frames, rows
    model.engine.close()


@pytest.mark.parametrize("j", [0, 20, 40, 41, None])
def test_rollback_at_every_place_of_the_window(device, random_model, j):
    """row 0's window of 60 over positions 279 .. 338: the guess is wrong behind row j -- the first, a middle one, the rows whose kept context ends
    on the page edge 320 and one past it -- or nowhere"""
    cfg, model, sd_ref, frames, rows = random_model
    _rollback_case(model, cfg, sd_ref, frames, rows, [0], [j], device, f"B=1 j={j}")


def test_rollback_ragged_batch(device, random_model):
    cfg, model, sd_ref, frames, rows = random_model
    _rollback_case(model, cfg, sd_ref, frames, rows, [0, 1, 2], [41, None, 5], device, "B=3 j=41/none/5")


def test_rollback_on_the_fp8_kv_cache(device):
    from emmax import _lib
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny(gqa=True)
    with _lib.tuning(kv_fp8=1):
        model, _ = _mk(cfg, KV8_SEED, False, device, max_batch=3, max_prompt=160, max_ctx=480)
    frames, rows = _inputs(cfg, 3, P_LENS, seed=KV8_INPUT_SEED)
    _rollback_case(model, cfg, None, frames, rows, [0, 1, 2], [40, 3, None], device, "kv_fp8 B=3", whole_session=True)
    model.engine.close()


# ---- free-running on random weights ------------------------------------------------------------------------------------------------------------
# weights seed 3, prompt seed 9: the fp32 oracle's own free-running greedy ids clear the id line at 26 of 40 tokens (three distinct ids), computed on the
# CPU before this test was written (random tiny weights settle into short cycles: of twelve (weights, prompt) pairs tried, five clear half)
FREE_SEED, FREE_PROMPT_SEED, FREE_N = 3, 9, 40


def test_free_running_drafted_ids_against_the_oracle(device):
    """drafted against plain ids, and every emitted token against the oracle's argmax wherever the oracle's top-2 margin clears the a-priori line
    (tests/conftest.py: ID_BUDGET_SHALLOW = 1.5e-2 of max|logit| at <= 3 layers); at least half of the tokens must be checkable."""
    from emmax.config import EmmaXConfig
    from oracle import emmax_oracle as orc

    cfg = EmmaXConfig.tiny()
    model, sd_ref = _mk(cfg, FREE_SEED, False, device, max_batch=1, max_prompt=64, max_ctx=400)
    rng = np.random.default_rng(FREE_PROMPT_SEED)
    frames = rng.integers(0, 256, size=(1, 224, 224, 3), dtype=np.uint8)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=11)]]
    fr = torch.from_numpy(frames).to(device)
    plain, _, _ = _run(model, rows, fr, max_new=FREE_N)
    draft = list(plain[0])
    draft[9] = _corrupt(draft[9])
    got, _, (stats,) = _run(model, rows, fr, draft=[draft], max_new=FREE_N)
    print(f"free-running: {stats}")
    assert got == plain and stats.passes >= 1 and stats.accepted[0] >= 1
    with torch.inference_mode():   # the oracle teacher-forced along the emitted ids: row t predicts token t
        logits, _, _ = orc.vla_prefill_logits(torch.tensor([rows[0] + got[0][:-1]]), orc.preprocess_frames(frames, cfg), sd_ref, cfg)
    ref = logits[0, -len(got[0]):].float()
    checkable = 0
    for t, tok in enumerate(got[0]):
        if above_id_line(ref[t], ID_BUDGET_SHALLOW):
            checkable += 1
            assert tok == int(ref[t].argmax()), (t, tok, int(ref[t].argmax()))
    print(f"free-running: {checkable} of {len(got[0])} tokens above the id line")
    assert 2 * checkable >= len(got[0]), (checkable, len(got[0]))
    model.engine.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_every_session_refusal_names_its_cause_and_leaves_the_session_usable(device):
    """Every EMMAX_ERR_STATE refusal of emmax_verify with its own message (each mode set on its own, on a freshly prefilled session), the two argument
    refusals, and behind every one of them the session still generates the plain run's ids."""
    from emmax import _lib, taps
    from emmax.config import EmmaXConfig
    from emmax.constraints import action_bins
    from emmax.drafting import VerifyRefused
    from emmax.sampling import BeamParams, LogitsProcessing, SamplingParams

    cfg = EmmaXConfig.tiny()
    model, _ = _mk(cfg, 5, True, device, max_batch=2, max_prompt=96, max_ctx=480)
    eng = model.engine
    frames, rows = _planted_rows(cfg, 1)
    fr = torch.from_numpy(frames).to(device)
    before, _, _ = _run(model, rows, fr)
    sp = SamplingParams(temperature=1.0, top_k=0, top_p=1.0, seed=1)

    def fresh():
        model._prefill(rows, None, fr, max_new=80)   # (clears every mode of the call before, prefills, picks the first token)
        return eng.output_tail(0, 1)[0][0][0]

    def refused(msg, status=-5):
        with pytest.raises(_lib.EmmaxError, match=msg) as e:
            eng.verify([[tok, 5, 6]], max_new=10)
        assert f"status {status}" in str(e.value), str(e.value)

    def still_usable():
        after, _, _ = _run(model, rows, fr)
        assert after == before

    tok = fresh()
    eng.set_sampling(sp, n=1)
    refused("sampling is on")
    eng.clear_sampling()
    still_usable()

    tok = fresh()
    eng.set_processing(LogitsProcessing(repetition_penalty=1.3), n=1)
    refused("processors are on|processing is on")
    eng.clear_processing()
    still_usable()

    tok = fresh()
    eng.set_warpers(SamplingParams(temperature=1.0, top_k=0, top_p=1.0, seed=1, min_p=0.1), n=1)
    refused("warpers are on")
    eng.clear_warpers()
    still_usable()

    tok = fresh()
    eng.set_token_rules(LogitsProcessing(suppress_tokens=(7,)), n=1)
    refused("token rules are on")
    eng.clear_token_rules()
    if eng.processing:
        eng.clear_processing()
    still_usable()

    tok = fresh()
    eng.set_automaton(action_bins(cfg.llm.vocab_size, cfg.n_action_bins, 7, token_vocab=model.vocab_size))
    refused("token automaton is set")
    eng.clear_automaton()
    if eng.processing:
        eng.clear_processing()
    still_usable()

    tok = fresh()
    buf = torch.empty(10, 1, cfg.llm.vocab_size, dtype=torch.float32, device=device)
    eng.set_scores(None, buf, 10, rows=1)
    refused("scores are bound")
    eng.set_scores(None, None)
    still_usable()

    tok = fresh()
    eng.set_sampling(SamplingParams(temperature=0.0, top_k=0, top_p=1.0, seed=1), n=1)
    eng.set_top_logprobs(2, [], 8)
    refused("log-probabilities are bound")
    eng.clear_top_logprobs()
    eng.clear_sampling()
    still_usable()

    tok = fresh()
    eng.bind_step_taps(taps.TapSpec([cfg.llm.num_layers], []), 8, eng.context_lengths(0, 1)[0] + 8)
    refused("step taps are bound")
    eng.clear_taps()
    still_usable()

    tok = fresh()
    eng.set_beams(BeamParams(num_beams=2))
    refused("beams are on")
    eng.clear_beams()
    still_usable()

    tok = fresh()
    eng.set_sampling(sp, n=2)
    eng.set_sample_groups(2)
    refused("sample groups are on")
    eng.clear_sample_groups()
    eng.clear_sampling()
    still_usable()

    tok = fresh()
    eng.slots_open(1)
    refused("request slots are open")
    still_usable()                                                        # (a plain prefill ends slot serving)

    tok = fresh()
    with pytest.raises(_lib.EmmaxError, match="pending token") as e:      # the window must start with the row's pending token
        eng.verify([[tok + 1, 5, 6]], max_new=10)
    assert "status -1" in str(e.value)
    room = eng.max_ctx - eng.context_lengths(0, 1)[0]
    with pytest.raises(VerifyRefused, match="max_ctx"):                    # one row more than the cache holds: nothing changed
        eng.verify([[tok] + [5] * (room - 1)], max_new=10)
    assert eng.context_lengths(0, 1)[0] == eng.max_ctx - room and eng.output_tail(0, 1)[1] == [1]
    assert eng.verify([[tok] + [5] * (room - 2)], max_new=eng.max_ctx)[0][0] >= 1   # ... and the largest window it holds
    still_usable()
    model.engine.close()


def test_fp8_weight_and_exact_models_refuse_a_draft(device):
    from emmax import _lib
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny()
    frames, rows = _planted_rows(cfg, 1)
    fr = torch.from_numpy(frames).to(device)
    cfg8 = EmmaXConfig.tiny()
    cfg8.decode_weight_dtype = "fp8"
    m8, _ = _mk(cfg8, 5, True, device, max_batch=1, max_prompt=32, max_ctx=400)
    ids8, lens8 = m8.generate_ids(rows, frames_u8=fr, max_new_tokens=8)
    want8 = ids8[0, : int(lens8[0])].cpu().tolist()
    with pytest.raises(NotImplementedError, match="fp8"):
        m8.generate_ids(rows, frames_u8=fr, max_new_tokens=8, draft=[[5, 6]])
    m8._prefill(rows, None, fr, max_new=8)
    tok = m8.engine.output_tail(0, 1)[0][0][0]
    with pytest.raises(_lib.EmmaxError, match="fp8"):
        m8.engine.verify([[tok, 5]], max_new=8)
    ids8, lens8 = m8.generate_ids(rows, frames_u8=fr, max_new_tokens=8)
    assert ids8[0, : int(lens8[0])].cpu().tolist() == want8
    m8.engine.close()
    xm, _ = _mk(EmmaXConfig.tiny(), 5, True, device, max_batch=1, max_prompt=32, max_ctx=400, exact=True)
    idsx, lensx = xm.generate_ids(rows, frames_u8=fr, max_new_tokens=8)
    wantx = idsx[0, : int(lensx[0])].cpu().tolist()
    xm._prefill(rows, None, fr, max_new=8)
    with pytest.raises(NotImplementedError, match="exact"):
        xm.generate_ids(rows, frames_u8=fr, max_new_tokens=8, draft=[[5, 6]])
    with pytest.raises(_lib.EmmaxError, match="exact"):
        xm.engine.verify([[5, 6]], max_new=8)
    idsx, lensx = xm.generate_ids(rows, frames_u8=fr, max_new_tokens=8)
    assert idsx[0, : int(lensx[0])].cpu().tolist() == wantx
    xm.engine.close()


# ---- the model level ------------------------------------------------------------------------------------------------------------------------------
def test_generate_predict_action_and_the_simpler_env_wrapper(device):
    from emmax.config import EmmaXConfig
    from emmax.processing import EmmaXProcessor
    from emmax.simpler_env import OpenVLAInference
    from emmax.weights import planted_chain

    cfg = EmmaXConfig.tiny()
    model, _ = _mk(cfg, 5, True, device, max_batch=2, max_prompt=96, max_ctx=480)
    frames, rows = _planted_rows(cfg, 1)
    fr = torch.from_numpy(frames).to(device)
    chain = planted_chain(cfg, rows[0][-1], MAX_NEW)
    plain = model.generate(torch.tensor(rows), frames_u8=fr, max_new_tokens=MAX_NEW)
    assert plain[0, len(rows[0]):].tolist()[:len(chain)] == chain
    model.last_draft_stats = None
    out = model.generate(torch.tensor(rows), frames_u8=fr, max_new_tokens=MAX_NEW, draft_ids=[chain])
    assert torch.equal(out, plain) and model.last_draft_stats.accepted[0] >= len(chain) - 3 and model.last_draft_stats.passes <= 2
    out = model.generate(torch.tensor(rows), frames_u8=fr, max_new_tokens=MAX_NEW, draft_ids=[chain], return_dict_in_generate=True)
    assert torch.equal(out.sequences, plain) and out.past_key_values.lengths == [cfg.n_patches + plain.shape[1] - 1]
    # HF's prompt lookup: the prompt's own ids are the draft (here a prompt that holds the answer's beginning), window n + 1
    rows2 = [rows[0][:-1] + chain[:12][::-1] + [rows[0][-1]] + chain[:12] + [rows[0][-1]]]
    plain2 = model.generate(torch.tensor(rows2), frames_u8=fr, max_new_tokens=MAX_NEW)
    out2 = model.generate(torch.tensor(rows2), frames_u8=fr, max_new_tokens=MAX_NEW, prompt_lookup_num_tokens=8)
    assert torch.equal(out2, plain2) and model.last_draft_stats.accepted[0] >= 8 and max(model.last_draft_stats.drafted) > 0
    with pytest.raises(ValueError, match="one of"):
        model.generate(torch.tensor(rows), frames_u8=fr, max_new_tokens=8, draft_ids=[chain], prompt_lookup_num_tokens=4)
    # predict_action: the 7 action ids of an earlier call as the draft
    act = model.predict_action(torch.tensor(rows), frames_u8=fr, unnorm_key="bridge_orig")
    ids7 = list(model.last_generated_ids)
    assert len(ids7) == 7
    model.last_draft_stats = None
    act2 = model.predict_action(torch.tensor(rows), frames_u8=fr, unnorm_key="bridge_orig", draft_ids=ids7)
    # (one pass: the pending token + the 5 draft ids the budget of 7 leaves room for; the 7th id is the pass's own last token)
    assert np.array_equal(act, act2) and model.last_draft_stats.passes == 1 and model.last_draft_stats.accepted == [5] and model.last_generated_ids == ids7
    # the SimplerEnv wrapper: the second control step drafts with the first one's ids
    proc = EmmaXProcessor.from_pretrained(cfg=cfg)
    frame = np.random.default_rng(4).integers(0, 256, size=(480, 640, 3), dtype=np.uint8)
    task = "put the spoon on the towel"
    ref_pol = OpenVLAInference("unused", policy_setup="widowx_bridge", vla=model, processor=proc, device=device)
    want = [ref_pol.step(frame, task), ref_pol.step(frame, task)]
    pol = OpenVLAInference("unused", policy_setup="widowx_bridge", vla=model, processor=proc, device=device, reuse_reasoning=True)
    first = pol.step(frame, task)
    assert pol.last_draft_stats is None and pol._last_ids is not None
    second = pol.step(frame, task)
    assert pol.last_draft_stats is not None and pol.last_draft_stats.accepted[0] >= 1
    for (raw_w, act_w), (raw_g, act_g) in zip(want, [first, second]):
        for k in raw_w:
            assert np.array_equal(raw_w[k], raw_g[k]), k
        for k in act_w:
            assert np.array_equal(act_w[k], act_g[k]), k
    pol.reset(task)
    assert pol._last_ids is None
    model.engine.close()
