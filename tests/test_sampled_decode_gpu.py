"""Sampling inside the decode step on a real MI355X (include/emmax.h ABI 7: emmax_session_set_sampling; the sampled finish in
emma-x_amd/csrc/sample.hip): temperature 0 against greedy generate, the in-step draw against the external loop over emmax_op_sample,
graph replay against eager launches, the fp32 oracle, batch-position independence in exact numerics, slot serving and state hygiene.

The tiny configuration takes batches of up to 8 rows; 17-64 rows (the kmp kernels and the chunked lm-head) run on the 7B-layer-dims,
2-layer synthetic model of test_operating_point_gpu.py with short prompts."""
import copy

import numpy as np
import pytest
import torch

import sampling_ref as ref

pytestmark = pytest.mark.gpu


def _tiny_model(device, max_batch, exact=False, fp8=False, kv8=False, seed=6):
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    if fp8:
        cfg.decode_weight_dtype = "fp8"
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=seed).items()}
    with _lib.tuning(kv_fp8=int(kv8)):   # (the KV format is read when the session is created: the capacity below is never outgrown)
        model = EmmaXForActionPrediction(cfg, dict(sd)).to(device, max_batch=max_batch, max_prompt=24, exact=exact)
    return model, cfg, sd


def _inputs(B, seed=21, lo=6, hi=20):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(B, 224, 224, 3), dtype=np.uint8)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=int(n))] for n in rng.integers(lo, hi, size=B)]
    return frames, rows


def _op_cfg():
    from emmax.config import EmmaXConfig, LlmConfig

    tiny = EmmaXConfig.tiny()
    llm = LlmConfig(hidden_size=4096, intermediate_size=11008, num_layers=2, num_heads=32, num_kv_heads=32, head_dim=128,
                    vocab_size=32064, max_position=2048)
    return EmmaXConfig(tiny.towers, llm, norm_stats=tiny.norm_stats)


@pytest.fixture(scope="module")
def op_setup():
    from emmax.weights import synthetic_state_dict

    cfg = _op_cfg()
    sd_bf = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=21).items()}
    frames, rows = _inputs(64, seed=77, lo=8, hi=24)
    return cfg, sd_bf, frames, rows


def _op_model(op_setup, device, exact=False):
    from emmax.modeling import EmmaXForActionPrediction

    cfg, sd_bf, _, _ = op_setup
    return EmmaXForActionPrediction(copy.deepcopy(cfg), dict(sd_bf)).to(device, max_batch=64, max_prompt=32, max_ctx=256 + 32 + 40, exact=exact)


def _greedy_and_t0(model, rows, fr, n, graph):
    from emmax import _lib
    from emmax.sampling import SamplingParams

    with _lib.tuning(graph=int(graph)):
        ids_g, lens_g = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False)
        ids_g, lens_g = ids_g.cpu(), lens_g.cpu()
        assert not model.engine.sampling
        ids_s, lens_s, lp = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False,
                                               sampling=SamplingParams(0.0, 0, 1.0, seed=9), return_logprobs=True)
        assert model.engine.sampling and model.engine.graph_active() == bool(graph)
    return ids_g, lens_g, ids_s.cpu(), lens_s.cpu(), lp.cpu()


@pytest.mark.parametrize("mode", ["default", "exact", "fp8", "kv8"])
def test_temperature_zero_equals_greedy_tiny(device, mode):
    """every row at T = 0: the sampled finish takes the argmax of the fp32 logits the lm-head wrote -- the greedy ids, bit for bit"""
    model, _, _ = _tiny_model(device, 8, exact=mode == "exact", fp8=mode == "fp8", kv8=mode == "kv8")
    frames, rows = _inputs(8)
    fr = torch.from_numpy(frames).to(device)
    for B in (1, 2, 8):
        for graph in (0, 1):
            ids_g, lens_g, ids_s, lens_s, lp = _greedy_and_t0(model, rows[:B], fr[:B], 12, graph)
            assert torch.equal(lens_g, lens_s) and torch.equal(ids_g, ids_s), (mode, B, graph)
            assert bool(torch.isfinite(lp[:, 0]).all()) and bool((lp[:, 0] <= 0).all())


@pytest.mark.parametrize("exact,batches", [(False, (17, 64)), (True, (17,))])
def test_temperature_zero_equals_greedy_operating_point(device, op_setup, exact, batches):
    """17 and 64 rows (two-tile kmp kernels, the lm-head in launches of 32 rows; exact numerics: chunks of 8): T = 0 is greedy"""
    model = _op_model(op_setup, device, exact=exact)
    _, _, frames, rows = op_setup
    fr = torch.from_numpy(frames).to(device)
    for B in batches:
        for graph in (0, 1):
            ids_g, lens_g, ids_s, lens_s, _ = _greedy_and_t0(model, rows[:B], fr[:B], 6, graph)
            assert torch.equal(lens_g, lens_s) and torch.equal(ids_g, ids_s), (exact, B, graph)


def _mixed_params(B, seed0=100):
    from emmax.sampling import SamplingParams

    grid = [(1.0, 50, 1.0), (0.8, 0, 0.9), (1.3, 20, 0.95), (0.0, 0, 1.0), (2.0, 0, 1.0), (0.6, 5, 0.7)]
    return [SamplingParams(*grid[b % len(grid)], seed=seed0 + 7 * b) for b in range(B)]


def _external_loop(model, rows, fr, params, n):
    """prefill, then n times: last_logits -> sample_logits(steps=t, subseqs=b) -> set_current_tokens -> decode_step"""
    from emmax.sampling import sample_logits

    eng = model.engine
    B = len(rows)
    model._prefill(rows, frames_u8=fr, max_new=n + 2)
    ids = np.zeros((B, n), dtype=np.int64)
    lps = np.zeros((B, n), dtype=np.float32)
    for t in range(n):
        tok, lp = sample_logits(eng.last_logits()[:B].contiguous(), params, subseqs=list(range(B)), steps=t)
        ids[:, t] = tok.cpu().numpy()
        lps[:, t] = lp.cpu().numpy()
        eng.set_current_tokens(tok.tolist())
        eng.decode_step()
    return ids, lps


def _check_in_step_equals_loop(model, rows, fr, n):
    B = len(rows)
    params = _mixed_params(B)
    ids, lens, lp = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, sampling=params, return_logprobs=True)
    ids, lens, lp = ids.cpu().numpy(), lens.cpu().numpy(), lp.cpu().numpy()
    want_ids, want_lp = _external_loop(model, rows, fr, params, n)
    nonargmax = 0
    for b in range(B):
        L = int(lens[b])
        assert L >= 1
        assert ids[b, :L].tolist() == want_ids[b, :L].tolist(), b
        assert lp[b, :L].view(np.uint32).tolist() == want_lp[b, :L].view(np.uint32).tolist(), b
        nonargmax += int(params[b].temperature > 0)
    assert nonargmax > 0


@pytest.mark.parametrize("exact", [False, True])
def test_in_step_equals_external_loop_tiny(device, exact):
    """B = 3, mixed per-row T / top-k / top-p: the in-step ids and log-probability bits are the external loop's (emmax_op_sample)"""
    model, _, _ = _tiny_model(device, 3, exact=exact)
    frames, rows = _inputs(3, seed=5)
    _check_in_step_equals_loop(model, rows, torch.from_numpy(frames).to(device), 16)


def test_in_step_equals_external_loop_40_rows(device, op_setup):
    """B = 40: the lm-head in launches of 32 + 8 rows, each followed by its own sampled finish over complete logit rows"""
    model = _op_model(op_setup, device)
    _, _, frames, rows = op_setup
    _check_in_step_equals_loop(model, rows[:40], torch.from_numpy(frames[:40]).to(device), 5)


def test_graph_replay_equals_eager_and_seeds(device):
    """the sampled step replayed from the captured graph gives the eager ids and log-probabilities bit for bit; one seed repeats, two differ"""
    from emmax import _lib
    from emmax.sampling import SamplingParams

    model, _, _ = _tiny_model(device, 2)
    frames, rows = _inputs(2, seed=8)
    fr = torch.from_numpy(frames).to(device)

    def run(seed, graph):
        with _lib.tuning(graph=graph):
            ids, lens, lp = model.generate_ids(rows, frames_u8=fr, max_new_tokens=20, stop_on_eos=False,
                                               sampling=SamplingParams(1.5, 0, 1.0, seed=seed), return_logprobs=True)
            assert model.engine.graph_active() == bool(graph)
        return ids.cpu(), lens.cpu(), lp.cpu()

    a = run(11, 0)
    b = run(11, 1)
    c = run(11, 1)
    d = run(12, 0)
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1])
        assert torch.equal(a[2].view(torch.int32), x[2].view(torch.int32))
    assert not torch.equal(a[0], d[0])


def test_sampled_generate_matches_the_oracle(device):
    """model.generate(do_sample=True, top-k / top-p) teacher-forced through the fp32 oracle and the reference sampler: ids agree wherever the
    Gumbel margin (and the kept-set boundary) clears 2 ID_BUDGET max|logit| / T, log-probabilities within the budget, and at least a quarter
    of the steps leave the argmax"""
    from conftest import ID_BUDGET_TINY
    from oracle import emmax_oracle as orc

    model, cfg, sd = _tiny_model(device, 2)
    frames, rows = _inputs(2, seed=21, lo=9, hi=13)
    fr = torch.from_numpy(frames).to(device)
    sd_ref = {k: v.float() for k, v in sd.items()}
    n = 24
    # a temperature from the data (steps far from one-hot), as the external-loop test picks it
    logits0, _, _ = orc.vla_prefill_logits(torch.tensor([rows[0]]), orc.preprocess_frames(frames[:1], cfg), sd_ref, cfg)
    top = torch.topk(logits0[0, -1].float(), 20).values
    T = float((top[0] - top[19]) / 3.0)
    required = nonargmax = steps = 0
    for k, p, seed in ((20, 1.0, 31), (0, 0.9, 32)):
        P = max(len(r) for r in rows)
        out = model.generate(torch.tensor([r + [0] * (P - len(r)) for r in rows]), attention_mask=torch.tensor([[1] * len(r) + [0] * (P - len(r)) for r in rows]),
                             frames_u8=fr, max_new_tokens=n, do_sample=True, temperature=T, top_k=k, top_p=p, seed=seed)
        _, _, lps = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, sampling=model._sampling_args(True, T, k, p, seed), return_logprobs=True)
        lps = lps.cpu().numpy()
        for b in range(2):
            got = [t for t in out[b, len(rows[b]):].tolist()]
            got = got[: n]
            while got and got[-1] == cfg.pad_token_id:
                got.pop()
            logits, _, _ = orc.vla_prefill_logits(torch.tensor([rows[b] + got]), orc.preprocess_frames(frames[b:b + 1], cfg), sd_ref, cfg)
            L = logits[0, -len(got) - 1:-1].float().numpy()
            for t, tok in enumerate(got):
                rt, rlp, margin = ref.sample_row(L[t], T, k, p, seed, b, t)
                line = 2 * ID_BUDGET_TINY * np.abs(L[t]).max()
                steps += 1
                nonargmax += int(tok != int(np.argmax(L[t])))
                assert abs(float(lps[b, t]) - rlp) <= line, (k, p, b, t, lps[b, t], rlp)
                if margin > line / T and ref.kept_set(L[t], T, k, p)[2] > line / T:
                    required += 1
                    assert tok == rt, (k, p, b, t, tok, rt, margin)
    assert required >= steps // 4 and nonargmax >= steps // 4, (required, nonargmax, steps)


def test_exact_numerics_batch_position_does_not_matter(device):
    """exact numerics: row b of a B = 8 sampled batch is its bs = 1 sampled run with the same (seed, subseq), id for id, up to the row's
    first step whose Gumbel margin (fp32 oracle, teacher-forced) is below the exact-numerics line"""
    from conftest import ID_BUDGET_EXACT
    from emmax.sampling import SamplingParams
    from oracle import emmax_oracle as orc

    model, cfg, sd = _tiny_model(device, 8, exact=True)
    frames, rows = _inputs(8, seed=3)
    fr = torch.from_numpy(frames).to(device)
    sd_ref = {k: v.float() for k, v in sd.items()}
    params = [SamplingParams([1.0, 0.7, 1.4][b % 3], [0, 50][b % 2], [1.0, 0.9][b % 2], seed=500 + b) for b in range(8)]
    n = 12
    ids8, lens8 = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, sampling=params)
    ids8, lens8 = ids8.cpu(), lens8.cpu()
    compared = 0
    for b in range(8):
        # bs = 1 with the batch row's (seed, subseq b)
        eng = model.engine
        eng.set_sampling([params[b]], subseqs=[b])
        eng.prefill([rows[b]], eng.vision_encode(fr[b:b + 1]))
        ids1, lens1 = eng.generate(n, False)
        one = ids1[0, : int(lens1[0])].cpu().tolist()
        row8 = ids8[b, : int(lens8[b])].tolist()
        logits, _, _ = orc.vla_prefill_logits(torch.tensor([rows[b] + one]), orc.preprocess_frames(frames[b:b + 1], cfg), sd_ref, cfg)
        L = logits[0, -len(one) - 1:-1].float().numpy()
        p = params[b]
        for t in range(min(len(one), len(row8))):
            _, _, margin = ref.sample_row(L[t], p.temperature, p.top_k, p.top_p, p.seed, b, t)
            line = 2 * ID_BUDGET_EXACT * np.abs(L[t]).max() / p.temperature
            if margin <= line or ref.kept_set(L[t], p.temperature, p.top_k, p.top_p)[2] <= line:
                break
            assert row8[t] == one[t], (b, t)
            compared += 1
    assert compared >= 8 * n // 2, compared


@pytest.mark.parametrize("overlap", [False, True])
def test_slot_serving_mixed_greedy_and_sampled(device, overlap):
    """12 requests on 4 slots, every third one greedy, the stop rule on: greedy requests return their bs = 1 greedy ids, sampled ones their
    bs = 1 sampled generate (same seed, subseq 0), and each request's ids do not depend on overlap"""
    from emmax.sampling import SamplingParams
    from emmax.serving import Request, SlotScheduler

    model, _, _ = _tiny_model(device, 4, exact=True)
    eng = model.engine
    frames, rows = _inputs(12, seed=44)
    fr = torch.from_numpy(frames).to(device)
    samp = [None if i % 3 == 0 else SamplingParams([1.0, 0.8][i % 2], [50, 0][i % 2], [1.0, 0.9][i % 2], seed=900 + i) for i in range(12)]
    budgets = [10 + (i * 5) % 13 for i in range(12)]
    trig = [rows[0][3], rows[0][4]]   # (rarely emitted: the rule is armed, the ids stay comparable to a rule-free run)
    want, want_lp = [], []
    for i in range(12):
        ids, lens, *lp = model.generate_ids([rows[i]], frames_u8=fr[i:i + 1], max_new_tokens=budgets[i], stop_on_eos=True,
                                            sampling=None if samp[i] is None else [samp[i]], return_logprobs=samp[i] is not None)
        want.append(ids[0, : int(lens[0])].cpu().tolist())
        want_lp.append(lp[0][0, : int(lens[0])].cpu().tolist() if lp else None)

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    sch = SlotScheduler(eng, encode, n_slots=4, poll_every=3, stop_trigger=trig, stop_after=50, overlap=overlap)
    for i in range(12):
        sch.submit(Request(i, fr[i], rows[i], max_new_tokens=budgets[i], sampling=samp[i]))
    res = sch.run()
    assert sorted(r.rid for r in res) == list(range(12)) and not eng.sampling
    for r in res:
        assert r.ids == want[r.rid], (overlap, r.rid, samp[r.rid])
        assert (r.logprobs is None) == (samp[r.rid] is None)
        if r.logprobs is not None:
            # (4 slots and bs = 1 run different exact-numerics kernels: the same ids, log-probabilities to the last bits)
            assert np.abs(np.float32(r.logprobs) - np.float32(want_lp[r.rid])).max() <= 1e-4, r.rid


def test_greedy_after_sampled_is_unchanged(device):
    """after a sampled generate, a greedy generate returns what it returned before sampling ever ran, and the session is greedy again"""
    model, _, _ = _tiny_model(device, 2)
    frames, rows = _inputs(2, seed=12)
    fr = torch.from_numpy(frames).to(device)
    P = max(len(r) for r in rows)
    ids_t = torch.tensor([r + [0] * (P - len(r)) for r in rows])
    mask = torch.tensor([[1] * len(r) + [0] * (P - len(r)) for r in rows])
    before = model.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16)
    torch.manual_seed(3)
    s1 = model.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16, do_sample=True, temperature=1.5)
    assert model.engine.sampling
    after = model.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16, do_sample=False)
    assert not model.engine.sampling
    assert torch.equal(before, after)
    torch.manual_seed(3)
    s2 = model.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16, do_sample=True, temperature=1.5)
    assert torch.equal(s1, s2) and not torch.equal(s1, before)
