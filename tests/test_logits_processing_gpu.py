"""Logits processors and scores inside the decode step on a real MI355X (include/emmax.h ABI 8: emmax_session_set_processing /
emmax_session_set_scores; the processing finish in emma-x_amd/csrc/sample.hip): neutral processing against greedy, the stored scores
against processing_ref.py, the fp32 oracle teacher-forced, the n-gram and min-new-tokens properties, graph replay against eager, batch
independence in exact numerics, slot serving and state hygiene."""
import numpy as np
import pytest
import torch

import processing_ref as pref
import sampling_ref as ref
from test_sampled_decode_gpu import _inputs, _op_model, _tiny_model, op_setup  # noqa: F401  (op_setup: the module fixture)

pytestmark = pytest.mark.gpu


def _bufs(n, B, V, device):
    return (torch.full((n, B, V), float("nan"), dtype=torch.float32, device=device),
            torch.full((n, B, V), float("nan"), dtype=torch.float32, device=device))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _neutral_equals_greedy(model, rows, fr, n, graph):
    from emmax import _lib
    from emmax.sampling import LogitsProcessing

    V = model.config.llm.vocab_size
    with _lib.tuning(graph=int(graph)):
        ids_g, lens_g = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False)
        ids_g, lens_g = ids_g.cpu(), lens_g.cpu()
        assert not model.engine.processing and not model.engine.scores_bound
        sc, lg = _bufs(n, len(rows), V, fr.device)
        ids_p, lens_p = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, processing=LogitsProcessing(),
                                           scores=sc, logits=lg)
        # (generate_ids unbinds the buffers when it returns)
        assert model.engine.processing and not model.engine.scores_bound and model.engine.graph_active() == bool(graph)
    assert torch.equal(lens_g, lens_p.cpu()) and torch.equal(ids_g, ids_p.cpu())
    # neutral processors: the scores are the raw logits, bit for bit, and their argmax is the token
    assert torch.equal(sc[0].view(torch.int32), lg[0].view(torch.int32))
    assert torch.equal(sc[0].argmax(-1).cpu().to(torch.int32), ids_g[:, 0])


@pytest.mark.parametrize("mode", ["default", "exact", "fp8", "kv8"])
def test_neutral_processing_equals_greedy_tiny(device, mode):
    model, _, _ = _tiny_model(device, 8, exact=mode == "exact", fp8=mode == "fp8", kv8=mode == "kv8")
    frames, rows = _inputs(8)
    fr = torch.from_numpy(frames).to(device)
    for B in (1, 2, 8):
        for graph in (0, 1):
            _neutral_equals_greedy(model, rows[:B], fr[:B], 10, graph)


@pytest.mark.parametrize("exact,batches", [(False, (17, 64)), (True, (17,))])
def test_neutral_processing_equals_greedy_operating_point(device, op_setup, exact, batches):
    model = _op_model(op_setup, device, exact=exact)
    _, _, frames, rows = op_setup
    fr = torch.from_numpy(frames).to(device)
    for B in batches:
        for graph in (0, 1):
            _neutral_equals_greedy(model, rows[:B], fr[:B], 5, graph)


def test_scores_are_the_processed_rows(device):
    """penalty 1.3, n = 3, min_new_tokens 4 on a model whose EOS is the token row 0 would emit first: greedy scores[t][b] =
    processing_ref on logits[t][b] and the row's history, bit for bit (EOS -inf at t = 3, back at t = 4), and their argmax is the emitted
    token; sampled scores are z / T on the reference kept set and -inf off it.  Positions past a row's length stay NaN."""
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.sampling import LogitsProcessing, SamplingParams

    model, cfg, sd = _tiny_model(device, 2)
    frames, rows = _inputs(2, seed=31)
    fr = torch.from_numpy(frames).to(device)
    V, n = cfg.llm.vocab_size, 14
    ids, _ = model.generate_ids(rows, frames_u8=fr, max_new_tokens=2, stop_on_eos=False, processing=LogitsProcessing(1.3, 3, 0))
    eos = int(ids[0, 0])   # the processed argmax of row 0 at t = 0 without the EOS ban
    cfg2 = type(cfg)(cfg.towers, cfg.llm, norm_stats=cfg.norm_stats)
    cfg2.eos_token_id = eos
    model = EmmaXForActionPrediction(cfg2, dict(sd)).to(device, max_batch=2, max_prompt=24)
    proc = LogitsProcessing(1.3, 3, 4)
    for sampling in (None, SamplingParams(0.8, 20, 1.0, seed=77)):
        sc, lg = _bufs(n, 2, V, device)
        ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, processing=proc, sampling=sampling,
                                       scores=sc, logits=lg)
        assert not model.engine.scores_bound
        ids, lens, sc, lg = ids.cpu().numpy(), lens.cpu().numpy(), sc.cpu().numpy(), lg.cpu().numpy()
        back = 0
        for b in range(2):
            assert lens[b] >= 5 and eos not in ids[b, :4].tolist(), (b, lens[b], ids[b])
            for t in range(int(lens[b])):
                hist = rows[b] + ids[b, :t].tolist()
                want = pref.process_row(lg[t, b], hist, t, 1.3, 3, 4, eos)
                assert (want[eos] == -np.inf) == (t < 4 or eos in pref.banned_ngram_ids(hist, 3)), (b, t)
                back += int(t == 4 and np.isfinite(want[eos]))
                if sampling is None:
                    np.testing.assert_array_equal(_bits(sc[t, b]), _bits(want), err_msg=f"{b} {t}")
                    assert int(np.argmax(sc[t, b])) == ids[b, t]
                else:
                    np.testing.assert_array_equal(_bits(sc[t, b]), _bits(pref.scores_row(want, 0.8, 20, 1.0)), err_msg=f"{b} {t}")
                    assert np.isfinite(sc[t, b, ids[b, t]])
            assert np.isnan(sc[int(lens[b]):, b]).all() and np.isnan(lg[int(lens[b]):, b]).all()
        assert back >= 1   # EOS is back in the device's row at t = 4 (the boundary is pinned from both sides)
        if sampling is None:   # without the ban row 0 would have emitted EOS at once
            assert int(np.argmax(pref.process_row(lg[0, 0], rows[0], 0, 1.3, 3, 0, eos))) == eos


@pytest.mark.parametrize("exact", [False, True])
def test_processed_greedy_matches_the_oracle(device, exact):
    """greedy with penalty 1.5 and n = 3, teacher-forced through the fp32 oracle: the ids are the argmax of the numpy-processed oracle
    logits wherever the processed top-2 margin clears the line, and at least a quarter of the steps leave the raw argmax"""
    from conftest import ID_BUDGET_EXACT, ID_BUDGET_TINY
    from emmax.sampling import LogitsProcessing
    from oracle import emmax_oracle as orc

    budget = ID_BUDGET_EXACT if exact else ID_BUDGET_TINY
    model, cfg, sd = _tiny_model(device, 2, exact=exact)
    frames, rows = _inputs(2, seed=23, lo=9, hi=13)
    fr = torch.from_numpy(frames).to(device)
    sd_ref = {k: v.float() for k, v in sd.items()}
    n = 24
    ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, processing=LogitsProcessing(1.5, 3, 0))
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    required = moved = steps = 0
    for b in range(2):
        got = ids[b, : int(lens[b])].tolist()
        logits, _, _ = orc.vla_prefill_logits(torch.tensor([rows[b] + got]), orc.preprocess_frames(frames[b:b + 1], cfg), sd_ref, cfg)
        L = logits[0, -len(got) - 1:-1].float().numpy()
        for t, tok in enumerate(got):
            proc = pref.process_row(L[t], rows[b] + got[:t], t, 1.5, 3, 0, cfg.eos_token_id)
            line = 2 * 1.5 * budget * np.abs(L[t]).max()
            top2 = np.sort(proc[np.isfinite(proc)])[-2:]
            steps += 1
            moved += int(pref.greedy(proc) != int(np.argmax(L[t])))
            if top2[1] - top2[0] > line:
                required += 1
                assert tok == pref.greedy(proc), (exact, b, t, tok, pref.greedy(proc))
    assert required >= steps // 4 and moved >= steps // 4, (required, moved, steps)


def test_processed_sampling_matches_the_oracle(device):
    """sampling after the processors (penalty 1.2, n = 2, top-k 20), teacher-forced: the ids are ref.sample_row over the processed oracle
    rows wherever the Gumbel margin clears the line"""
    from conftest import ID_BUDGET_TINY
    from emmax.sampling import LogitsProcessing, SamplingParams
    from oracle import emmax_oracle as orc

    model, cfg, sd = _tiny_model(device, 2)
    frames, rows = _inputs(2, seed=27, lo=9, hi=13)
    fr = torch.from_numpy(frames).to(device)
    sd_ref = {k: v.float() for k, v in sd.items()}
    n, T, k, seed = 20, 1.0, 20, 41
    ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, processing=LogitsProcessing(1.2, 2, 0),
                                   sampling=SamplingParams(T, k, 1.0, seed=seed))
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    required = steps = 0
    for b in range(2):
        got = ids[b, : int(lens[b])].tolist()
        logits, _, _ = orc.vla_prefill_logits(torch.tensor([rows[b] + got]), orc.preprocess_frames(frames[b:b + 1], cfg), sd_ref, cfg)
        L = logits[0, -len(got) - 1:-1].float().numpy()
        for t, tok in enumerate(got):
            proc = pref.process_row(L[t], rows[b] + got[:t], t, 1.2, 2, 0, cfg.eos_token_id)
            rt, _, margin = ref.sample_row(proc, T, k, 1.0, seed, b, t)
            line = 2 * 1.2 * ID_BUDGET_TINY * np.abs(L[t]).max() / T
            steps += 1
            if margin > line:
                required += 1
                assert tok == rt, (b, t, tok, rt, margin)
    assert required >= steps // 4, (required, steps)


def test_no_ngram_repeats(device):
    """B = 8, n = 1..4 mixed, 64 tokens: no n-gram occurs twice in any row's prompt + output"""
    from emmax.sampling import LogitsProcessing

    model, _, _ = _tiny_model(device, 8)
    frames, rows = _inputs(8, seed=9)
    fr = torch.from_numpy(frames).to(device)
    ns = [1 + b % 4 for b in range(8)]
    ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=64, stop_on_eos=False,
                                   processing=[LogitsProcessing(1.0, n, 0) for n in ns])
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    for b in range(8):
        out = ids[b, : int(lens[b])].tolist()
        assert len(out) >= 16, (b, len(out))
        seq, n = rows[b] + out, ns[b]
        # the ban covers every n-gram that ends in an emitted token
        grams = [tuple(seq[j:j + n]) for j in range(len(seq) - n + 1)]
        prompt_grams = set(tuple(rows[b][j:j + n]) for j in range(len(rows[b]) - n + 1))
        new = grams[len(rows[b]) - n + 1:] if len(rows[b]) >= n else grams
        seen = set(prompt_grams)
        for g in new:
            assert g not in seen, (b, n, g)
            seen.add(g)


def test_min_new_tokens_holds_eos_back(device):
    """a model whose EOS is the token a row greedily emits first: the row stops at once without min_new_tokens, and emits no EOS before
    index 6 with min_new_tokens = 6 (also through min_length)"""
    from emmax.sampling import LogitsProcessing

    model, cfg, sd = _tiny_model(device, 1)
    frames, rows = _inputs(1, seed=4)
    fr = torch.from_numpy(frames).to(device)
    ids, _ = model.generate_ids(rows, frames_u8=fr, max_new_tokens=4, stop_on_eos=False)
    first = int(ids[0, 0])
    from emmax.modeling import EmmaXForActionPrediction

    cfg2 = type(cfg)(cfg.towers, cfg.llm, norm_stats=cfg.norm_stats)
    cfg2.eos_token_id = first
    m2 = EmmaXForActionPrediction(cfg2, dict(sd)).to(device, max_batch=1, max_prompt=24)
    ids, lens = m2.generate_ids(rows, frames_u8=fr, max_new_tokens=12)
    assert int(lens[0]) == 1 and int(ids[0, 0]) == first
    ids, lens = m2.generate_ids(rows, frames_u8=fr, max_new_tokens=12, processing=LogitsProcessing(1.0, 0, 6))
    out = ids[0, : int(lens[0])].cpu().tolist()
    assert len(out) >= 6 and first not in out[:6], out
    P = len(rows[0])
    seq = m2.generate(torch.tensor(rows), frames_u8=fr, max_new_tokens=12, min_length=P + 6)
    assert seq[0, P:P + len(out)].tolist() == out


def test_graph_replay_equals_eager_with_processing_and_sampling(device):
    from emmax import _lib
    from emmax.sampling import LogitsProcessing, SamplingParams

    model, cfg, _ = _tiny_model(device, 2)
    frames, rows = _inputs(2, seed=8)
    fr = torch.from_numpy(frames).to(device)
    V, n = cfg.llm.vocab_size, 20

    def run(graph):
        sc, lg = _bufs(n, 2, V, device)
        with _lib.tuning(graph=graph):
            ids, lens, lp = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, return_logprobs=True,
                                               sampling=SamplingParams(1.2, 0, 0.95, seed=5), processing=LogitsProcessing(1.4, 2, 3),
                                               scores=sc, logits=lg)
            assert model.engine.graph_active() == bool(graph)
        return ids.cpu(), lens.cpu(), lp.cpu().view(torch.int32), sc.cpu().view(torch.int32), lg.cpu().view(torch.int32)

    a = run(0)
    with _lib.tuning(graph=1):   # a graph captured with processing but without sampling must not be replayed for the sampled call
        model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, processing=LogitsProcessing(1.4, 2, 3))
    b, c = run(1), run(1)
    for x in (b, c):
        for u, v in zip(a, x):
            assert torch.equal(u, v)


def test_exact_numerics_rows_with_different_processors(device):
    """exact numerics, B = 8, every row its own processors: each row's ids equal its bs = 1 run"""
    from emmax.sampling import LogitsProcessing

    model, _, _ = _tiny_model(device, 8, exact=True)
    frames, rows = _inputs(8, seed=13)
    fr = torch.from_numpy(frames).to(device)
    procs = [LogitsProcessing([1.0, 1.2, 1.5, 0.8][b % 4], [0, 2, 3, 1][(b // 2) % 4], [0, 4][b % 2]) for b in range(8)]
    ids8, lens8 = model.generate_ids(rows, frames_u8=fr, max_new_tokens=16, stop_on_eos=False, processing=procs)
    ids8, lens8 = ids8.cpu(), lens8.cpu()
    for b in range(8):
        ids1, lens1 = model.generate_ids([rows[b]], frames_u8=fr[b:b + 1], max_new_tokens=16, stop_on_eos=False, processing=[procs[b]])
        assert ids8[b, : int(lens8[b])].tolist() == ids1[0, : int(lens1[0])].cpu().tolist(), b


@pytest.mark.parametrize("overlap", [False, True])
def test_slot_serving_mixed_processed_sampled_plain(device, overlap):
    """exact numerics, 12 requests on 4 slots: processed, sampled, processed + sampled and plain requests; each returns its own bs = 1
    generate_ids, and the session has neither processing nor sampling after the serve"""
    from emmax.sampling import LogitsProcessing, SamplingParams
    from emmax.serving import Request, SlotScheduler

    model, _, _ = _tiny_model(device, 4, exact=True)
    eng = model.engine
    frames, rows = _inputs(12, seed=45)
    fr = torch.from_numpy(frames).to(device)
    proc = [LogitsProcessing(1.3, 2, 3) if i % 4 in (1, 2) else None for i in range(12)]
    samp = [SamplingParams(0.9, 20, 1.0, seed=300 + i) if i % 4 in (2, 3) else None for i in range(12)]
    budgets = [8 + (i * 5) % 11 for i in range(12)]
    want = []
    for i in range(12):
        ids, lens = model.generate_ids([rows[i]], frames_u8=fr[i:i + 1], max_new_tokens=budgets[i], stop_on_eos=True,
                                       sampling=None if samp[i] is None else [samp[i]], processing=None if proc[i] is None else [proc[i]])
        want.append(ids[0, : int(lens[0])].cpu().tolist())

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    sch = SlotScheduler(eng, encode, n_slots=4, poll_every=3, overlap=overlap)
    for i in range(12):
        sch.submit(Request(i, fr[i], rows[i], max_new_tokens=budgets[i], sampling=samp[i], processing=proc[i]))
    res = sch.run()
    assert sorted(r.rid for r in res) == list(range(12)) and not eng.sampling and not eng.processing
    for r in res:
        assert r.ids == want[r.rid], (overlap, r.rid, proc[r.rid], samp[r.rid])


def test_state_hygiene(device):
    """a sampled call, then a processed greedy call, then a plain call: the plain call matches a fresh session; a retired slot's
    processors and history do not reach the next request; generate(return_dict_in_generate=True, output_scores=True).sequences is the
    plain generate tensor"""
    from emmax.sampling import LogitsProcessing, SamplingParams
    from emmax.serving import Request, SlotScheduler

    frames, rows = _inputs(2, seed=12)
    P = max(len(r) for r in rows)
    ids_t = torch.tensor([r + [0] * (P - len(r)) for r in rows])
    mask = torch.tensor([[1] * len(r) + [0] * (P - len(r)) for r in rows])
    fresh, _, _ = _tiny_model(device, 2)
    fr = torch.from_numpy(frames).to(device)
    want = fresh.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16)
    del fresh
    model, _, _ = _tiny_model(device, 2)
    model.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16, do_sample=True, seed=4)
    processed = model.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16, repetition_penalty=1.5, no_repeat_ngram_size=2)
    assert model.engine.processing and not model.engine.sampling
    plain = model.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16)
    assert not model.engine.processing and not model.engine.scores_bound
    assert torch.equal(plain, want) and not torch.equal(processed, want)
    out = model.generate(ids_t, attention_mask=mask, frames_u8=fr, max_new_tokens=16, return_dict_in_generate=True, output_scores=True,
                         output_logits=True)
    assert torch.equal(out.sequences, want) and len(out.scores) == want.shape[1] - P and len(out.logits) == len(out.scores)
    for t, s in enumerate(out.scores):   # neutral: the scores are the logits; the argmax is the emitted token
        assert torch.equal(s.view(torch.int32), out.logits[t].view(torch.int32))
    assert torch.equal(out.scores[0].argmax(-1).cpu(), want[:, P])

    # one slot: a processed request, then a plain one with the other request's prompt -- the plain one returns its own greedy ids
    eng = model.engine
    plain_ids, lens = model.generate_ids([rows[1]], frames_u8=fr[1:2], max_new_tokens=12)
    plain_ids = plain_ids[0, : int(lens[0])].cpu().tolist()

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    sch = SlotScheduler(eng, encode, n_slots=1, poll_every=2)
    sch.submit(Request(0, fr[0], rows[0], max_new_tokens=12, processing=LogitsProcessing(2.0, 1, 5)))
    sch.submit(Request(1, fr[1], rows[1], max_new_tokens=12))
    res = {r.rid: r for r in sch.run()}
    assert res[1].ids == plain_ids
