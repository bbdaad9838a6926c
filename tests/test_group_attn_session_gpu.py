"""The grouped decode attention inside the session (include/emmax.h: emmax_session_attn_grouped; step.hip: attn_group_rows): sample groups
and forked beams read each group's shared prompt pages once per step.

Two models, as tests/test_sample_groups_gpu.py builds them: the tiny configuration (2 q heads, 2 kv heads, at most 8 decode rows) with
attn_nsplit = 1 forced through the tuning table, so that its steps run the one-split attention form the route needs; and the 2-layer model at
7B layer dimensions (32 heads), where steps of 5 rows and more take that form by themselves.  Patches are 256 rows: a context is 256 + prompt
ids, so a prompt of 64 ids ends on a page boundary (5 shared pages), one of 60 ids crosses it while generating, one of 20 shares 4 pages.

Every test asserts on every step and every row it runs, and each first asks the session's own witness that the route was (or was not) taken."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
import sample_groups_ref as sg  # noqa: E402
from conftest import ID_BUDGET_SHALLOW, ID_BUDGET_TINY  # noqa: E402

pytestmark = pytest.mark.gpu

GRID = [(1.0, 50, 1.0), (0.8, 0, 0.9), (1.3, 20, 0.95), (0.0, 0, 1.0), (2.0, 0, 1.0), (0.6, 5, 0.7)]


def _tiny_model(device, max_batch, exact=False, kv8=False, max_prompt=64, max_ctx=256 + 64 + 40):
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=sg.WEIGHT_SEED).items()}
    with _lib.tuning(kv_fp8=int(kv8)):
        model = EmmaXForActionPrediction(cfg, dict(sd)).to(device, max_batch=max_batch, max_prompt=max_prompt, max_ctx=max_ctx, exact=exact)
    return model, cfg, sd


def _op_cfg():
    from emmax.config import EmmaXConfig, LlmConfig

    tiny = EmmaXConfig.tiny()
    llm = LlmConfig(hidden_size=4096, intermediate_size=11008, num_layers=2, num_heads=32, num_kv_heads=32, head_dim=128, vocab_size=32064,
                    max_position=2048)
    return EmmaXConfig(tiny.towers, llm, norm_stats=tiny.norm_stats)


@pytest.fixture(scope="module")
def op(device):
    """The 2-layer model at 7B layer dimensions (40 rows), its bf16 weights, and the same weights as fp32 on the device for the oracle."""
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = _op_cfg()
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=21).items()}
    model = EmmaXForActionPrediction(copy.deepcopy(cfg), dict(sd)).to(device, max_batch=40, max_prompt=64, max_ctx=256 + 64 + 24)
    return model, cfg, {k: v.float().to(device) for k, v in sd.items()}


def _inputs(lens, seed):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(len(lens), 224, 224, 3), dtype=np.uint8)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=n - 1)] for n in lens]
    return frames, rows


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def _oracle_rows(orc, sd32, cfg, frame, prompt, seqs, dev):
    """fp32 oracle logits in front of every emitted token of every row of one group: [len(seqs), T, vocab].  The restatement executes where
    sd32 lives (tests/test_operating_point_gpu.py pins the device-executed restatement against the host's; row 0 is compared again below)."""
    T = len(seqs[0])
    with torch.inference_mode():
        proj = orc.projector(orc.vision_backbone(orc.preprocess_frames(frame, cfg).to(dev), sd32, cfg), sd32)
        ids = torch.tensor([prompt + list(s) for s in seqs], dtype=torch.long, device=dev)
        logits, _ = orc.llama_forward(orc.splice(ids, proj.expand(len(seqs), -1, -1), sd32), sd32, cfg.llm, None)
        return logits[:, -T - 1:-1].float().cpu().numpy()


# ---- the route witness -------------------------------------------------------------------------------------------------------------------
def test_route_witness(device, op):
    from emmax import _lib
    from emmax.sampling import BeamParams, SamplingParams

    model, cfg, _ = op
    eng, lib = model.engine, model.engine.lib
    q = lambda B: lib.emmax_session_attn_grouped(eng._session, B)
    assert lib.emmax_session_attn_grouped(None, 8) == -1
    if eng.beams:
        eng.clear_beams()
    eng.clear_sample_groups()
    assert [q(B) for B in (4, 8, 16, 40)] == [0, 0, 0, 0]          # groups off
    eng.set_sampling(SamplingParams(1.0, 0, 1.0, seed=1), n=40)
    eng.set_sample_groups(8)
    # the default rule: the batches the two launches were measured faster at
    assert [q(B) for B in (8, 16, 24, 32, 40, 48, 56, 64)] == [0, 0, 0, 1, 0, 1, 0, 1]
    with _lib.tuning(attn_group=0):
        assert [q(B) for B in (8, 16, 32, 40, 64)] == [0, 0, 0, 0, 0]
    with _lib.tuning(attn_group=1):                                  # wherever the kernels take the step
        assert [q(B) for B in (8, 16, 40)] == [1, 1, 1] and eng.attn_grouped(16)
        assert q(12) == 0                                            # not whole groups
        eng.set_sample_groups(2)
        assert q(4) == 0 and q(8) == 1                               # 4 rows: the o-proj merges split partials there
    assert [q(B) for B in (32, 64)] == [0, 0]                        # N = 2 was not measured: not in the default rule
    eng.set_sample_groups(4)
    assert [q(B) for B in (32, 36, 64)] == [1, 0, 1]
    eng.clear_sample_groups()
    assert [q(B) for B in (8, 16, 40)] == [0, 0, 0] and not eng.attn_grouped(8)
    eng.clear_sampling()
    # beams: only behind their fork
    frames, rows = _inputs([20], seed=3)
    eng.set_beams(BeamParams(8))
    assert q(8) == 0
    eng.clear_beams()
    model.generate_ids(rows, frames_u8=torch.from_numpy(frames).to(device), max_new_tokens=3, stop_on_eos=False, beams=BeamParams(8, 1.0, False, 8))
    assert eng.beams == 8 and [q(B) for B in (8, 32, 40, 64)] == [0, 0, 0, 0]   # beams at 32 / 64 rows were not measured: forced only
    with _lib.tuning(attn_group=1):
        assert [q(B) for B in (8, 16, 40)] == [1, 1, 1]
        assert [q(B) for B in (32, 64)] == [1, 1]
    with _lib.tuning(attn_group=0):
        assert q(32) == 0
    eng.clear_beams()
    with _lib.tuning(attn_group=1):
        assert q(8) == 0
    # exact numerics never takes it; the tiny configuration does once its steps run the one-split form
    with _lib.tuning(attn_nsplit=1, attn_group=1):
        for exact, want in ((False, 1), (True, 0)):
            tiny, _, _ = _tiny_model(device, 8, exact=exact)
            tiny.engine.set_sampling(SamplingParams(1.0, 0, 1.0, seed=1), n=8)
            tiny.engine.set_sample_groups(2)
            assert lib.emmax_session_attn_grouped(tiny.engine._session, 8) == want, exact
    tiny.engine.clear_sample_groups()
    tiny, _, _ = _tiny_model(device, 8)
    tiny.engine.set_sampling(SamplingParams(1.0, 0, 1.0, seed=1), n=8)
    tiny.engine.set_sample_groups(2)
    with _lib.tuning(attn_group=1):
        assert lib.emmax_session_attn_grouped(tiny.engine._session, 8) == 0   # eight splits at 2 kv heads: today's launch


# ---- sample groups against the oracle ----------------------------------------------------------------------------------------------------
def _groups_against_oracle(device, model, cfg, sd32, lens, N, T, budget, route, host_row=False):
    from emmax import _lib
    from emmax.sampling import SamplingParams
    from oracle import emmax_oracle as orc

    G, V = len(lens), cfg.llm.vocab_size
    frames, rows = _inputs(lens, seed=77 + G)
    fr = torch.from_numpy(frames).to(device)
    params = [SamplingParams(*GRID[r % len(GRID)], seed=100 + 7 * r) for r in range(G * N)]
    lg = torch.full((T, G * N, V), float("nan"), dtype=torch.float32, device=device)
    with _lib.tuning(attn_group={"default": -1, True: 1, False: 0}[route]):   # "default": the switch as shipped -- the rule itself must take the step
        ids, lens_out = model.generate_ids(rows, frames_u8=fr, max_new_tokens=T, stop_on_eos=False, sampling=params, logits=lg, num_samples=N)
        assert model.engine.attn_grouped(G * N) == bool(route)
    ids, lg = ids.cpu().numpy(), lg.cpu().numpy()
    assert (lens_out.cpu().numpy() == T).all() and np.isfinite(lg).all()
    worst = 0.0
    for g in range(G):
        ref = _oracle_rows(orc, sd32, cfg, frames[g: g + 1], rows[g], [ids[g * N + j].tolist() for j in range(N)], sd32["language_model.lm_head.weight"].device)
        if host_row and g == 0:   # the device-executed restatement against the host's, one row
            host = _oracle_rows(orc, {k: v.cpu() for k, v in sd32.items()}, cfg, frames[:1], rows[0], [ids[0].tolist()], "cpu")
            assert np.abs(host[0] - ref[0]).max() <= 1e-4 * np.abs(host[0]).max()
        for j in range(N):
            got = lg[:, g * N + j]
            err = np.abs(got - ref[j]).max(axis=1) / np.abs(ref[j]).max(axis=1)
            worst = max(worst, float(err.max()))
            assert (err <= budget).all(), (g, j, int(np.argmax(err)), float(err.max()))
    print(f"{G} x {N} rows, prompts {lens}, route {'on' if route else 'off'}: worst |logit err| / max|logit| over {T} steps = {worst:.3e} (line {budget:.1e})")


@pytest.mark.parametrize("lens,route", [([60], True), ([64, 20], True), ([64, 20], False), ([64, 20, 60, 33, 7], True), ([64, 20, 60, 33], "default")],
                         ids=["8rows", "16rows", "16rows-route-off", "40rows", "32rows-default-switch"])
def test_sample_groups_against_the_oracle(device, op, lens, route):
    """8, 16 and 40 rows of N = 8 with the route forced (attn_group = 1), and 32 rows under the default switch, where the rule takes the
    step by itself: a prompt that ends on a page boundary, one that crosses it while generating (60 + 8 tokens), different lengths in one
    batch.  Every row's logits at every step against the fp32 oracle teacher-forced on the row's own ids."""
    model, cfg, sd32 = op
    _groups_against_oracle(device, model, cfg, sd32, lens, 8, 8, ID_BUDGET_SHALLOW, route, host_row=len(lens) == 1)


def test_sample_groups_fp8_cache_against_the_oracle(device):
    """One group of 8 rows over the e4m3 cache (tiny configuration), against the oracle that knows nothing of the cache format: 2.5 x the
    bf16 cache's budget, the factor tests/test_operating_point_gpu.py fixes for the e4m3 cache."""
    from emmax import _lib

    with _lib.tuning(attn_nsplit=1, attn_group=1):
        model, cfg, sd = _tiny_model(device, 8, kv8=True)
        _groups_against_oracle(device, model, cfg, {k: v.float() for k, v in sd.items()}, [60], 8, 8, 2.5 * ID_BUDGET_TINY, True)


# ---- the draw inside the step ------------------------------------------------------------------------------------------------------------
def _external_loop(model, rows, fr, params, N, n):
    """On the same group session: prefill (fork), then n times last_logits -> sample_logits(subseqs = row, steps = t) ->
    set_current_tokens -> decode_step."""
    from emmax.sampling import sample_logits

    eng, R = model.engine, len(rows) * N
    model._prefill(rows, frames_u8=fr, max_new=n + 2, sampling=params, num_samples=N)
    assert eng.sample_groups == N and eng.attn_grouped(R)
    ids = np.zeros((R, n), dtype=np.int64)
    lps = np.zeros((R, n), dtype=np.float32)
    for t in range(n):
        lg = eng.last_logits()
        tok, lp = sample_logits(lg.contiguous(), params, subseqs=list(range(R)), steps=t)
        ids[:, t] = tok.cpu().numpy()
        lps[:, t] = lp.cpu().numpy()
        eng.set_current_tokens(tok.tolist())
        eng.decode_step()
    return ids, lps


def test_the_draw_is_the_steps_own(device, op):
    """2 x 8 rows with the route on: ids and log-probability bits of generate equal an external loop over emmax_op_sample on the same session."""
    from emmax import _lib
    from emmax.sampling import SamplingParams

    model, cfg, _ = op
    N, n = 8, 6
    frames, rows = _inputs([60, 20], seed=12)
    fr = torch.from_numpy(frames).to(device)
    params = [SamplingParams(*GRID[r % len(GRID)], seed=300 + 3 * r) for r in range(2 * N)]
    with _lib.tuning(attn_group=1):
        ids, lens, lp = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, sampling=params, return_logprobs=True, num_samples=N)
        assert model.engine.attn_grouped(2 * N)
        ids, lp = ids.cpu().numpy(), lp.cpu().numpy()
        want_ids, want_lp = _external_loop(model, rows, fr, params, N, n)
    for r in range(2 * N):
        assert ids[r].tolist() == want_ids[r].tolist(), (r, ids[r].tolist(), want_ids[r].tolist())
        assert _bits(lp[r]).tolist() == _bits(want_lp[r]).tolist(), r
    assert len({tuple(r.tolist()) for r in ids}) >= 2


# ---- graph replay ------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_is_bit_equal_and_reads_the_shared_count_from_the_device(device):
    """Tiny configuration, 2 x 4 rows.  Eager and replayed steps agree bit for bit; then THE SAME captured step (one tuning epoch, the same
    batch) serves a prompt that shares 4 pages after one that shared 5: a count baked into the captured launch would make rows 1 .. 3 of a
    group read row 0's private fifth page as if it were shared."""
    from emmax import _lib
    from emmax.sampling import SamplingParams

    N, T = 4, 10
    params = [SamplingParams(*GRID[r % len(GRID)], seed=500 + r) for r in range(2 * N)]
    with _lib.tuning(attn_nsplit=1, attn_group=1):
        model, cfg, _ = _tiny_model(device, 8)
        eng = model.engine
        runs = {}
        for graph in (0, 1):
            with _lib.tuning(graph=graph):
                for name, lens in (("five pages", [64, 64]), ("four pages", [20, 33])):
                    frames, rows = _inputs(lens, seed=40 + lens[0])
                    eng.set_sampling(params)
                    eng.set_sample_groups(N)
                    eng.prefill(rows, eng.vision_encode(torch.from_numpy(frames).to(device)))
                    assert eng.attn_grouped(2 * N)
                    ids, lens_out, lp = eng.generate(T, False, return_logprobs=True)
                    assert eng.graph_active() == bool(graph)
                    runs[graph, name] = (ids.cpu().numpy(), _bits(lp.cpu().numpy()), _bits(eng.last_logits().cpu().numpy()))
        eng.clear_sample_groups()
    for name in ("five pages", "four pages"):
        for a, b in zip(runs[0, name], runs[1, name]):
            assert np.array_equal(a, b), name
        assert len({tuple(r.tolist()) for r in runs[0, name][0]}) >= 2


# ---- beams -------------------------------------------------------------------------------------------------------------------------------
def _after(orc, sd32, cfg, frame, prompt, seqs, dev):
    """the oracle's logit row behind prompt + seq, for every seq (all of one length): [len(seqs), vocab]"""
    return _oracle_rows(orc, sd32, cfg, frame, prompt, [list(s) + [0] for s in seqs], dev)[:, -1]   # (the appended id is not read)


def _oracle_beams(orc, sd32, cfg, frame, prompt, K, T, dev):
    """HF beam search (tests/beam_ref.py) over the fp32 oracle's rows: the K kept hypotheses [K, T], best first, and their scores."""
    grp = beam_ref.BeamGroup(K, cfg.llm.vocab_size, T, -1, 1.0, False)
    rows = _after(orc, sd32, cfg, frame, prompt, [[]], dev)
    for t in range(T):
        grp.step(rows)
        if t + 1 < T:
            rows = _after(orc, sd32, cfg, frame, prompt, [grp.lineage(t, k)[0] for k in range(K)], dev)
    seqs, _, scores, _ = grp.result(cfg.pad_token_id, row0=0)
    return np.asarray(seqs), np.asarray(scores, dtype=np.float64)


def _lineage(tr, g, t, k):
    toks, b = [], k
    for s in range(t, -1, -1):
        toks.append(int(tr["tok"][s, g, b]))
        b = int(tr["parent"][s, g, b])
    return toks[::-1]


@pytest.mark.parametrize("K", [4, 8])
def test_beams_on_planted_margins_route_on_and_off(device, K):
    """Two prompts (one ending on a page boundary) of K beams on margin-boosted (planted) weights at 7B layer dimensions, route on and off.
      1. the two routes emit the same K hypotheses per group, and their scores agree within 1e-2 x max(1, |score|) -- the form of the beam
         tests' own tolerance (tests/test_beam_search.py: 1e-5 x max(1, |score|) between two fp32 implementations); the factor is what the
         arithmetic allows here: the routes differ by an fp32 re-association of one softmax merge per layer, whose result is rounded to a
         bf16 attention row (2^-8 = 3.9e-3 relative per ulp) in each of the 2 layers;
      2. with the route on, every logit row of every step sits within ID_BUDGET_SHALLOW of the fp32 oracle teacher-forced on the lineage the
         beam had when it read the row -- which holds only if each beam reads its own tail behind the shared pages, after every reorder;
      3. the hypotheses are those of beam search over the oracle's rows.  K = 4: all four, in order.  K = 8: every hypothesis whose oracle
         score is separated from the other kept scores by more than twice the a-priori score budget (a log-probability carries the budget of
         its logit and of the lse: 2 x ID_BUDGET_SHALLOW x max|logit|; with length_penalty 1 a score is the mean of T of them).  On these
         weights that is the planted chain (score ~ 0 against ~ -max|logit| for the rest); the runner-ups are separated by 1e-4 .. 1e-1, far inside
         the budget, and every one that is exempted is printed with its gap and whether it equals the oracle's all the same.  Measured at
         K = 8: 12 of the 14 exempted hypotheses equal the oracle's; the two that do not are hypotheses 6 and 7 of group 0, whose oracle
         scores differ by 1.03e-4 -- and the device emits the same ids there with the route OFF as with it on."""
    from emmax import _lib
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.sampling import BeamParams
    from emmax.weights import planted_start_token, synthetic_state_dict
    from oracle import emmax_oracle as orc

    cfg, T = _op_cfg(), 6
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=5, planted=True).items()}
    model = EmmaXForActionPrediction(copy.deepcopy(cfg), dict(sd)).to(device, max_batch=16, max_prompt=64, max_ctx=256 + 64 + 24)
    sd32 = {k: v.float().to(device) for k, v in sd.items()}
    frames, rows = _inputs([64, 21], seed=9)
    rows = [r[:-1] + [planted_start_token(cfg, 9 + i)] for i, r in enumerate(rows)]
    fr = torch.from_numpy(frames).to(device)
    out = {}
    for route in (True, False):
        lg = torch.full((T, 2 * K, cfg.llm.vocab_size), float("nan"), dtype=torch.float32, device=device)
        with _lib.tuning(attn_group=1 if route else 0):
            model.generate_ids(rows, frames_u8=fr, max_new_tokens=T, stop_on_eos=False, logits=lg, beams=BeamParams(K, 1.0, False, K))
            assert model.engine.attn_grouped(2 * K) == route
        seq, ln, sc, _ = [x.cpu().numpy() for x in model.engine.beam_result()]
        out[route] = (seq, sc, lg.cpu().numpy(), {k: v.cpu().numpy() for k, v in model.engine.beam_trace().items()})
    model.engine.clear_beams()
    assert np.array_equal(out[True][0], out[False][0])
    diff = np.abs(out[True][1].astype(np.float64) - out[False][1])
    bound = 1e-2 * np.maximum(1.0, np.abs(out[False][1]))
    print(f"K = {K}: max |score on - score off| = {diff.max():.3e}, worst share of its bound {float((diff / bound).max()):.3f}; scores {out[False][1].min():.3f} .. {out[False][1].max():.3f}")
    assert (diff <= bound).all(), (diff, bound)
    seq, _, lg, tr = out[True]
    worst = 0.0
    for g in range(2):
        for t in range(T):
            seqs = [[]] if t == 0 else [_lineage(tr, g, t - 1, k) for k in range(K)]   # (step 0 reads the prefill's one row)
            ref = _after(orc, sd32, cfg, frames[g: g + 1], rows[g], seqs, device)
            got = lg[t, g * K: g * K + len(seqs)]
            err = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
            worst = max(worst, float(err.max()))
            assert (err <= ID_BUDGET_SHALLOW).all(), (g, t, err)
        want, wsc = _oracle_beams(orc, sd32, cfg, frames[g: g + 1], rows[g], K, T, device)
        budget = 2 * ID_BUDGET_SHALLOW * float(np.nanmax(np.abs(lg[:, g * K: (g + 1) * K])))
        gap = np.array([np.abs(np.delete(wsc, k) - wsc[k]).min() for k in range(K)])
        required = [k for k in range(K) if K == 4 or gap[k] > 2 * budget]
        assert 0 in required, (g, gap, budget)
        for k in range(K):
            same = want[k].tolist() == seq[g, k].tolist()
            if k in required:
                assert same, (g, k, want[k].tolist(), seq[g, k].tolist())
            else:
                print(f"K = {K} group {g} hypothesis {k}: exempt, oracle score gap {gap[k]:.3e} <= 2 x budget {2 * budget:.3e}; equal to the oracle's: {same}")
    print(f"K = {K}, route on: worst |logit err| / max|logit| over 2 x {K} rows x {T} steps = {worst:.3e} (line {ID_BUDGET_SHALLOW:.1e})")
