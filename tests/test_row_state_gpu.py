"""Every per-row array of a session in one serve (emma-x_amd/csrc/session.hip: session_row_cols).  The serving tests of the single features
each leave most of the optional arrays off; here sampling, logits processing, warpers, token rules, the token automaton and the top-N /
watched log-probabilities are all on at once, and every request differs from its neighbours in every column, so that a column the staged
commit or the slot fork skips, or moves with the wrong stride, shows as another request's parameters."""
import numpy as np
import pytest
import torch

import constraint_ref as cr
from test_warpers_gpu import _inputs, _model

pytestmark = pytest.mark.gpu

WATCH = [5, 31999, 17, 0, 1234]   # one list for the run
N_REQ = 7


def _requests(rows):
    """Per request: sampling (two greedy), processing over ONE rule table (the enable words 0, 1, 4 and 5 of it), automaton start, top-N,
    whether it watches, samples, budget"""
    from emmax.sampling import LogitsProcessing, SamplingParams

    ban, bias = {"suppress_tokens": list(range(3, 40))}, {"sequence_bias": {(41,): 6.0, (41, 42): 6.0}}
    samp = [SamplingParams(1.0, 50, 1.0, 700, min_p=0.02),
            None,
            SamplingParams(0.8, 0, 0.9, 701, typical_p=0.9),
            SamplingParams(0.9, 40, 0.95, 702, min_p=0.05),
            SamplingParams(1.1, 30, 1.0, 703, typical_p=0.8),
            None,
            SamplingParams(0.7, 20, 0.85, 704, min_p=0.1)]
    proc = [LogitsProcessing(1.2, 0, 1, **ban),
            LogitsProcessing(1.0, 2, 0, **bias),
            None,
            LogitsProcessing(1.3, 3, 2, **ban, **bias),
            LogitsProcessing(1.1, 0, 3),
            LogitsProcessing(1.4, 2, 1, **ban),
            LogitsProcessing(1.0, 4, 0, **bias)]
    starts = [3, None, 0, 5, None, 7, 2]
    n_top = [2, 5, 0, 5, 2, 0, 5]
    asks_watch = [True, False, True, True, False, True, False]
    nsamp = [1, 1, 1, 3, 1, 1, 1]
    budgets = [5, 8, 3, 6, 7, 4, 6]
    assert len({p.rule_enable if p is not None else 0 for p in proc}) == 4 and all(len(x) == N_REQ == len(rows) for x in (samp, proc, starts, n_top, asks_watch, nsamp, budgets))
    return samp, proc, starts, n_top, asks_watch, nsamp, budgets


@pytest.mark.parametrize("overlap", [False, True])
def test_every_owner_on_in_one_serve(device, overlap):
    """Exact numerics, 3 slots, 7 requests with ragged prompts and budgets of 3-8 tokens; request 3 is a group of 3 samples, so with overlap
    a fork follows a staged commit.  Each (request, sample) equals the same request run alone through generate_ids: ids exactly, the sampled
    requests' log-probabilities, the top-N ids exactly, the top-N and watched log-probabilities -- log-probabilities by the rule of the
    serving tests of tests/test_sampled_decode_gpu.py and tests/test_top_logprobs_gpu.py (3 slots and bs = 1 run different exact-numerics
    kernels: equal to 1e-4; the largest difference, printed, measures 3.8e-6 with and without overlap) -- and the session is plain again
    afterwards.  The scheduler refuses no pairing of these features: nothing is left out."""
    from emmax.serving import Request, SlotScheduler

    model, cfg = _model(device, 3, exact=True)
    eng = model.engine
    aut = cr.make_automaton(cfg.llm.vocab_size)
    frames, rows = _inputs(N_REQ, seed=58)
    fr = torch.from_numpy(frames).to(device)
    samp, proc, starts, n_top, asks_watch, nsamp, budgets = _requests(rows)
    want = {}
    for i in range(N_REQ):
        kw = {} if starts[i] is None else {"constraint": aut, "constraint_start": starts[i]}
        if nsamp[i] > 1:
            kw["num_samples"] = nsamp[i]
        out = model.generate_ids([rows[i]], frames_u8=fr[i:i + 1], max_new_tokens=budgets[i], stop_on_eos=True,
                                 sampling=None if samp[i] is None else [samp[i]] * nsamp[i], return_logprobs=samp[i] is not None,
                                 processing=None if proc[i] is None else [proc[i]] * nsamp[i], top_logprobs=n_top[i],
                                 watch_ids=WATCH if asks_watch[i] else None, **kw)
        ids, lens = out[:2]
        lp = out[2] if samp[i] is not None else None
        top = out[-1] if n_top[i] or asks_watch[i] else None
        for j in range(nsamp[i]):
            L = int(lens[j])
            want[(i, j)] = (ids[j, :L].cpu().tolist(), None if lp is None else lp[j, :L].cpu().numpy(),
                            None if top is None else (top.top_ids[j, :L].cpu().numpy(), top.top_logprobs[j, :L].cpu().numpy(), top.watch_logprobs[j, :L].cpu().numpy()))
    assert len({tuple(want[(3, j)][0]) for j in range(3)}) > 1   # the group's samples differ

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    sch = SlotScheduler(eng, encode, n_slots=3, poll_every=2, overlap=overlap, automaton=aut)
    for i in range(N_REQ):
        sch.submit(Request(i, fr[i], rows[i], max_new_tokens=budgets[i], sampling=samp[i], processing=proc[i], num_samples=nsamp[i],
                           top_logprobs=n_top[i], watch_ids=WATCH if asks_watch[i] else None, constraint_start=starts[i]))
    res = sch.run()
    assert sorted((r.rid, r.sample) for r in res) == sorted(want) and sch.overlap == overlap
    assert not overlap or sch.overlapped_admissions >= 1
    assert not eng.sampling and not eng.processing and not eng.warpers and not eng.token_rules and not eng.automaton and not eng.top_logprobs_bound
    worst = 0.0
    for r in res:
        i = r.rid
        w_ids, w_lp, w_top = want[(i, r.sample)]
        assert r.ids == w_ids, (overlap, i, r.sample, r.ids, w_ids)
        assert (r.top_logprobs is None) == (n_top[i] == 0) and (r.watch_logprobs is None) == (not asks_watch[i])
        diffs = []
        if samp[i] is not None:
            diffs.append(np.abs(np.float32(r.logprobs) - w_lp).max())
        if n_top[i]:
            assert [[p[0] for p in row] for row in r.top_logprobs] == w_top[0][:, :n_top[i]].tolist(), (overlap, i, r.sample)
            diffs.append(np.abs(np.float32([[p[1] for p in row] for row in r.top_logprobs]) - w_top[1][:, :n_top[i]]).max())
        if asks_watch[i]:
            diffs.append(np.abs(np.float32(r.watch_logprobs) - w_top[2]).max())
        worst = max([worst] + [float(d) for d in diffs])
        assert all(d <= 1e-4 for d in diffs), (overlap, i, r.sample, diffs)
    print("overlap", overlap, "largest log-probability difference to bs = 1:", worst)
