"""Top-N and watched-token log-probabilities, host side (no GPU): the numpy reference on hand-worked rows, the argument folding and refusals of
generate_ids / generate / predict_action / generate_batch over stub engines, the slot scheduler against a fake engine (per-request trimming,
one watch list per run, nothing new called when nobody asks, commit and fork bookkeeping), generate_batch's renormalisation, and the new C
symbols in header / ctypes table / INTEGRATION.md / library with the ABI still 12."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import top_logprobs_ref as ref  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_serving import FakeEngine, FakeStagedEngine, _encode_factory, _plans  # noqa: E402

NEW_SYMBOLS = ("emmax_op_top_logprobs", "emmax_session_set_top_logprobs", "emmax_session_clear_top_logprobs", "emmax_session_top_logprobs")
INF, NAN = float("inf"), float("nan")


# ---- the reference against hand-worked rows ---------------------------------------------------------------------------------------------
def test_reference_hand_worked_rows():
    # softmax of log [1, 2, 4, 1] / 8: probabilities 1/8, 1/4, 1/2, 1/8
    row = np.log(np.array([1, 2, 4, 1], dtype=np.float64)).astype(np.float32)
    ids, lp = ref.top_row(row, 3)
    assert ids.tolist() == [2, 1, 0]   # equal values (ids 0 and 3) by the lower id
    assert np.allclose(lp, np.log([0.5, 0.25, 0.125]), atol=1e-7)
    ids, lp = ref.top_row(row, 4)
    assert ids.tolist() == [2, 1, 0, 3]
    assert np.allclose(ref.watch_row(row, [3, 3, 2]), np.log([0.125, 0.125, 0.5]), atol=1e-7)
    # all equal: ids 0 .. N - 1, each log(1 / V)
    ids, lp = ref.top_row(np.full(7, 2.5, dtype=np.float32), 4)
    assert ids.tolist() == [0, 1, 2, 3] and np.allclose(lp, -math.log(7))
    # -inf entries are ordinary candidates behind every number, by id
    row = np.array([-INF, 0.0, -INF, 0.0], dtype=np.float32)
    ids, lp = ref.top_row(row, 4)
    assert ids.tolist() == [1, 3, 0, 2] and np.allclose(lp[:2], -math.log(2)) and (lp[2:] == -INF).all()
    # +0 and -0 are one value
    ids, _ = ref.top_row(np.array([-0.0, 0.0, -0.0], dtype=np.float32), 3)
    assert ids.tolist() == [0, 1, 2]
    # a NaN: the other entries in order, every log-probability NaN, the place past them (-1, -inf)
    row = np.array([1.0, NAN, 3.0], dtype=np.float32)
    ids, lp = ref.top_row(row, 3)
    assert ids.tolist() == [2, 0, -1] and np.isnan(lp[:2]).all() and lp[2] == -INF
    assert np.isnan(ref.watch_row(row, [0, 1])).all()
    ids, lp = ref.top_row(np.full(3, NAN, dtype=np.float32), 2)
    assert ids.tolist() == [-1, -1] and (lp == -INF).all()
    ti, tl, wl = ref.top_rows(np.stack([row, row]), 2, [0])
    assert ti.shape == (2, 2) and tl.shape == (2, 2) and wl.shape == (2, 1)
    # the comparison helpers
    assert ref.close(np.float32([NAN, -INF, 1.0]), [NAN, -INF, 1.0 + 5e-6], 1e-5) and not ref.close(np.float32([1.0]), [1.1], 1e-5)
    assert not ref.close(np.float32([1.0]), [NAN], 1e-5) and not ref.close(np.float32([INF]), [-INF], 1e-5)
    assert ref.same_bits(np.float32([NAN, 1.0]), np.float32([NAN, 1.0])) and not ref.same_bits(np.float32([0.0]), np.float32([-0.0]))


# ---- argument folding and refusals ------------------------------------------------------------------------------------------------------
def _model():
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    return EmmaXForActionPrediction(cfg, synthetic_state_dict(cfg, seed=1)), cfg


def _untouchable(m):
    def boom():
        raise AssertionError("engine was touched")

    m._need_engine = boom


def test_refusals_come_before_the_engine():
    from emmax.sampling import MAX_TOP_LOGPROBS, MAX_WATCH_IDS, BeamParams, check_top_logprobs

    assert (MAX_TOP_LOGPROBS, MAX_WATCH_IDS) == (20, 256) == (ref.MAX_TOP, ref.MAX_WATCH)
    assert check_top_logprobs(0, None) == (0, []) and check_top_logprobs(20, range(256), 32064) == (20, list(range(256)))
    assert check_top_logprobs(3, [7, 7], 8) == (3, [7, 7])   # duplicates allowed
    for n, w, v in [(21, None, None), (-1, None, None), (True, None, None), (2.0, None, None), (5, None, 4), (1, range(257), None), (1, [8], 8), (1, [-1], 8),
                    (1, [1.5], 8)]:
        with pytest.raises(ValueError):
            check_top_logprobs(n, w, v)
    m, cfg = _model()
    _untouchable(m)
    rows = [[1, 5, 6]]
    ids = torch.tensor(rows)
    for kw in (dict(top_logprobs=21), dict(watch_ids=[cfg.llm.vocab_size]), dict(watch_ids=list(range(257))), dict(top_logprobs=-2)):
        with pytest.raises(ValueError):
            m.generate_ids(rows, max_new_tokens=4, **kw)
        with pytest.raises(ValueError):
            m.generate(ids, max_new_tokens=4, return_dict_in_generate=True, **kw)
    with pytest.raises(NotImplementedError, match="outside the hot path"):
        m.generate_ids(rows, max_new_tokens=4, beams=BeamParams(2), top_logprobs=3)
    with pytest.raises(NotImplementedError, match="outside the hot path"):
        m.generate(ids, max_new_tokens=4, num_beams=2, return_dict_in_generate=True, watch_ids=[1])
    with pytest.raises(NotImplementedError, match="outside the hot path"):
        m.predict_action(ids, num_beams=2, return_bin_logprobs=True)
    for kw in (dict(top_logprobs=3), dict(watch_ids=[4])):   # the two arguments live in the generate output
        with pytest.raises(ValueError, match="return_dict_in_generate"):
            m.generate(ids, max_new_tokens=4, **kw)
    with pytest.raises(AssertionError, match="engine was touched"):   # valid arguments reach the engine
        m.generate_ids(rows, max_new_tokens=4, top_logprobs=3)


def test_generate_folds_the_arguments_and_fills_the_output():
    from emmax.modeling import TopLogprobsOutput

    m, cfg = _model()
    _untouchable(m)
    seen, lens = {}, [3, 2]

    def fake(rows, pixel_values=None, frames_u8=None, max_new_tokens=512, **kw):
        seen.clear()
        seen.update(kw)
        n = len(rows)
        ids = torch.full((n, max_new_tokens), cfg.pad_token_id, dtype=torch.int32)
        for r in range(n):
            ids[r, : lens[r]] = 100 + r
        out = (ids, torch.tensor(lens[:n], dtype=torch.int32))
        if "top_logprobs" in kw:
            N, W = kw["top_logprobs"], len(kw["watch_ids"] or [])
            out += (TopLogprobsOutput(torch.arange(n * max_new_tokens * N, dtype=torch.int32).reshape(n, max_new_tokens, N),
                                      torch.zeros(n, max_new_tokens, N), torch.ones(n, max_new_tokens, W), torch.zeros(n, max_new_tokens)),)
        return out

    m.generate_ids = fake
    rows = torch.tensor([[1, 7, 8], [1, 9, 10]])
    out = m.generate(rows, max_new_tokens=6, return_dict_in_generate=True, top_logprobs=4, watch_ids=(5, 5, 9))
    assert seen["top_logprobs"] == 4 and seen["watch_ids"] == [5, 5, 9]
    assert tuple(out.top_token_ids.shape) == (2, 3, 4) and tuple(out.top_logprobs.shape) == (2, 3, 4) and tuple(out.watch_logprobs.shape) == (2, 3, 3)   # T = 3
    assert out.top_token_ids[1, 0].tolist() == [24, 25, 26, 27] and out["watch_logprobs"] is out.watch_logprobs
    out = m.generate(rows, max_new_tokens=6, return_dict_in_generate=True, watch_ids=[5])
    assert seen["top_logprobs"] == 0 and out.top_token_ids is None and out.top_logprobs is None and tuple(out.watch_logprobs.shape) == (2, 3, 1)
    out = m.generate(rows, max_new_tokens=6, return_dict_in_generate=True, top_logprobs=2)
    assert seen["watch_ids"] is None and out.watch_logprobs is None and tuple(out.top_logprobs.shape) == (2, 3, 2)
    # nobody asks: generate_ids is called exactly as before, and the fields are None
    out = m.generate(rows, max_new_tokens=6, return_dict_in_generate=True)
    assert "top_logprobs" not in seen and "watch_ids" not in seen
    assert out.top_token_ids is None and out.top_logprobs is None and out.watch_logprobs is None
    m.generate(rows, max_new_tokens=6)
    assert "top_logprobs" not in seen and "watch_ids" not in seen


class _Eng:
    """the engine calls generate_ids makes, recorded"""

    def __init__(self, cfg, calls, rows_total=4):
        self.cfg, self.calls, self.R = cfg, calls, rows_total
        self.beams = self.sample_groups = 0
        self.processing = self.sampling = self.scores_bound = self.token_rules = self.warpers = False
        self.top_logprobs_bound = False
        self._top_bufs = None

    def max_decode_batch(self):
        return 8

    def ensure_capacity(self, *a):
        pass

    def set_sampling(self, p, n=None):
        ps = p if isinstance(p, (list, tuple)) else [p]
        self.calls.append(("sampling", n, ps[0].temperature))
        self.sampling = True

    def clear_sampling(self):
        self.calls.append(("clear_sampling",))
        self.sampling = False

    def set_sample_groups(self, n):
        self.calls.append(("groups", n))
        self.sample_groups = n

    def clear_sample_groups(self):
        self.sample_groups = 0

    def set_top_logprobs(self, n, watch, max_new):
        assert self.sampling, "bound behind sampling"
        self.calls.append(("top", n, list(watch), max_new))
        self.top_logprobs_bound = True
        W = len(watch)
        self._top_bufs = (torch.arange(self.R * max_new * n, dtype=torch.int32).reshape(self.R, max_new, n), torch.zeros(self.R, max_new, n),
                          torch.zeros(self.R, max_new, W))

    def clear_top_logprobs(self):
        self.calls.append(("clear_top",))
        self.top_logprobs_bound = False

    def prefill(self, rows, patches):
        assert self.top_logprobs_bound == any(c[0] == "top" for c in self.calls)
        self.calls.append(("prefill", len(rows)))
        self.B = len(rows) * (self.sample_groups or 1)

    def generate(self, max_new, stop_on_eos, return_logprobs=False):
        self.calls.append(("generate", max_new, return_logprobs))
        out = (torch.zeros(self.B, max_new, dtype=torch.int32), torch.full((self.B,), max_new, dtype=torch.int32))
        return out + (torch.zeros(self.B, max_new),) if return_logprobs else out


def test_generate_ids_binds_runs_and_restores():
    from emmax.modeling import TopLogprobsOutput
    from emmax.sampling import SamplingParams

    m, cfg = _model()
    calls = []
    eng = _Eng(cfg, calls)
    m._need_engine = lambda: eng
    m._encode_images = lambda *a: None
    fr = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    rows = [[1, 2], [1, 3]]
    # a greedy caller: temperature-0 sampling underneath, bound behind it, and greedy again afterwards
    ids, lens, top = m.generate_ids(rows, frames_u8=fr, max_new_tokens=5, top_logprobs=3, watch_ids=[9, 9])
    assert calls == [("sampling", 2, 0.0), ("top", 3, [9, 9], 5), ("prefill", 2), ("generate", 5, True), ("clear_top",), ("clear_sampling",)]
    assert isinstance(top, TopLogprobsOutput) and not eng.sampling and not eng.top_logprobs_bound
    assert tuple(top.top_ids.shape) == (2, 5, 3) and tuple(top.top_logprobs.shape) == (2, 5, 3) and tuple(top.watch_logprobs.shape) == (2, 5, 2)
    assert tuple(top.logprobs.shape) == (2, 5) and top.top_ids[1, 0].tolist() == [15, 16, 17]   # the first B of the session's rows
    # a sampling caller keeps sampling on; return_logprobs keeps its place in the tuple; G x N rows with num_samples
    calls.clear()
    p = SamplingParams(1.0, 0, 1.0, seed=3)
    ids, lens, lp, top = m.generate_ids(rows[:1], frames_u8=fr[:1], max_new_tokens=4, sampling=p, return_logprobs=True, watch_ids=[1], num_samples=3)
    assert calls == [("sampling", 3, 1.0), ("top", 0, [1], 4), ("groups", 3), ("prefill", 1), ("generate", 4, True), ("clear_top",)]
    assert eng.sampling and tuple(top.watch_logprobs.shape) == (3, 4, 1) and tuple(top.top_ids.shape) == (3, 4, 0) and lp is top.logprobs
    # nobody asks: no new engine method is called, and a binding an earlier call left is cleared
    calls.clear()
    eng.top_logprobs_bound = True
    out = m.generate_ids(rows, frames_u8=fr, max_new_tokens=4)
    assert len(out) == 2 and calls == [("clear_sampling",), ("clear_top",), ("prefill", 2), ("generate", 4, False)]


def test_predict_action_bin_columns_and_renormalisation():
    from emmax.actions import action_bin_token_ids, token_ids_to_actions
    from emmax.modeling import EmmaXForActionPrediction, TopLogprobsOutput

    m, cfg = _model()
    _untouchable(m)
    bins = action_bin_token_ids(m.vocab_size, cfg.n_action_bins)
    assert len(bins) == 256 and bins[0] == m.vocab_size - 1 and bins[255] == m.vocab_size - 256
    centers = m.bin_centers
    for k in (0, 17, 254):   # column k is the bin whose centre the id decodes to
        assert token_ids_to_actions(np.array([bins[k]]), m.vocab_size, centers)[0] == centers[k]
    dim = m.get_action_dim()
    rng = np.random.default_rng(2)
    wl = torch.from_numpy(rng.standard_normal((1, dim, 256)).astype(np.float32) - 9.0)
    seen = {}

    def fake(rows, pixel_values=None, frames_u8=None, max_new_tokens=512, **kw):
        seen.update(kw, max_new=max_new_tokens)
        ids = torch.tensor([[bins[3 + t] for t in range(max_new_tokens)]], dtype=torch.int32)
        return ids, torch.tensor([max_new_tokens], dtype=torch.int32), TopLogprobsOutput(None, None, wl, None)

    m.generate_ids = fake
    act, lp = m.predict_action(torch.tensor([[1, 5, 6]]), return_bin_logprobs=True)
    assert seen["watch_ids"] == bins and seen["top_logprobs"] == 0 and seen["max_new"] == dim
    assert act.shape == (dim,) and lp.shape == (dim, 256) and lp.dtype == np.float32
    x = wl[0].double().numpy()
    want = x - np.log(np.exp(x).sum(-1, keepdims=True))
    assert np.abs(lp - want).max() <= 1e-6 and np.abs(np.exp(lp.astype(np.float64)).sum(-1) - 1).max() <= 1e-6
    # -inf and NaN pass through the renormalisation as themselves
    r = EmmaXForActionPrediction.renormalize_logprobs(np.array([[-INF, math.log(0.25), math.log(0.25)], [NAN, 0.0, 0.0]]))
    assert r[0, 0] == -INF and np.allclose(r[0, 1:], math.log(0.5)) and np.isnan(r[1]).all()


def test_generate_batch_strings_and_renormalisation():
    from emmax.modeling import EmmaXGenerateOutput
    from emmax.tokenizer_stub import StubTokenizer

    m, cfg = _model()
    _untouchable(m)

    class Tok(StubTokenizer):
        table = {s: 400 + k for k, s in enumerate(m.TRIGGER_STRINGS)}

        def encode(self, text, add_special_tokens=True):
            if not add_special_tokens and text in self.table:
                return [self.table[text]]
            return super().encode(text, add_special_tokens)

    assert m.TRIGGER_STRINGS[:4] == ["True", "False", "Yes", "No"] and m.TRIGGER_STRINGS[4:] == [chr(65 + i) for i in range(26)]
    assert m.string2idx(Tok()) == {s: [400 + k] for k, s in enumerate(m.TRIGGER_STRINGS)}
    img = torch.zeros(6, 8, 8)
    with pytest.raises(ValueError, match="no tokenizer"):
        m.generate_batch(img, ["q"], return_string_probabilities=["Yes"])
    with pytest.raises(ValueError, match='String "No" is tokenized as more than one token'):   # the stand-in tokenizer spells it as several
        m.generate_batch(img, ["q"], return_string_probabilities=["No"], tokenizer=StubTokenizer())
    with pytest.raises(ValueError, match='"Maybe"'):
        m.generate_batch(img, ["q"], return_string_probabilities=["Maybe"], tokenizer=Tok())
    with pytest.raises(ValueError, match="pixel_values"):
        m.generate_batch([1, 2], ["q"], tokenizer=Tok())
    with pytest.raises(ValueError, match="one image"):
        m.generate_batch(torch.zeros(3, 6, 8, 8), ["q", "r"], tokenizer=Tok())
    V = cfg.llm.vocab_size
    rng = np.random.default_rng(4)
    first = (rng.standard_normal((2, V)) * 3).astype(np.float32)   # the first generated position's raw rows
    seen = {}

    def fake_generate(input_ids=None, pixel_values=None, **kw):
        seen.update(kw, rows=input_ids, pv=pixel_values)
        n = len(input_ids)
        P = max(len(r) for r in input_ids)
        seq = torch.full((n, P + 2), cfg.pad_token_id, dtype=torch.long)
        for b, r in enumerate(input_ids):
            seq[b, : len(r)] = torch.tensor(r)
            seq[b, len(r): len(r) + 2] = torch.tensor([3 + ord("o"), 3 + ord("k")])
        if "watch_ids" not in kw:
            return seq
        lp = torch.from_numpy(np.stack([ref.log_softmax64(first[b])[kw["watch_ids"]] for b in range(n)]).astype(np.float32))
        return EmmaXGenerateOutput(sequences=seq, watch_logprobs=lp[:, None, :].expand(n, 2, len(kw["watch_ids"])))

    m.generate = fake_generate
    texts = ["is the drawer open?", "which one"]
    names = ["Yes", "No", "B"]
    probs = m.generate_batch(img, texts, return_string_probabilities=names, tokenizer=Tok(), max_new_tokens=2)
    idx = [Tok.table[s] for s in names]
    assert seen["watch_ids"] == idx and seen["return_dict_in_generate"] is True and seen["max_new_tokens"] == 2 and tuple(seen["pv"].shape) == (2, 6, 8, 8)
    assert seen["rows"] == [Tok().encode(t) for t in texts]
    for b in range(2):   # softmax(row)[ids] / sum, restated
        e = np.exp(first[b].astype(np.float64) - first[b].max())
        sm = (e / e.sum())[idx]
        assert np.abs(np.asarray(probs[b]) - sm / sm.sum()).max() <= 1e-6 and isinstance(probs[b], list)
    seen.clear()
    out = m.generate_batch({"dino": torch.zeros(3, 8, 8), "siglip": torch.zeros(3, 8, 8)}, texts, tokenizer=Tok(), max_new_tokens=2)
    assert out == ["ok", "ok"] and "watch_ids" not in seen and set(seen["pv"]) == {"dino", "siglip"} and tuple(seen["pv"]["dino"].shape) == (2, 3, 8, 8)


# ---- the scheduler against a fake engine ------------------------------------------------------------------------------------------------
def _entry(rid, t, n, W):
    """what the fake device writes for request rid's token t: n (id, logprob) pairs and W watched values"""
    return [1000 * rid + 10 * t + k for k in range(n)], [-(rid + t + k) / 8.0 for k in range(n)], [-(rid + t) / 4.0 - w for w in range(W)]


class _TopMixin:
    """the sampling and top-logprob calls of the engine, recorded; a slot's state carries its request's entries (so a commit moves them)"""

    def _init_top(self):
        self.calls, self.bound, self.samp_on = [], None, False

    def set_sampling(self, params, seeds=None, subseqs=None, row0=0, n=None):
        self.calls.append(("set_sampling", row0, [p.temperature for p in params]))
        self.samp_on = True

    def set_sampling_staged(self, params, seeds=None, subseqs=None, n=None):
        self.calls.append(("set_sampling_staged", [p.temperature for p in params]))
        self.samp_on = True

    def clear_sampling(self):
        self.calls.append(("clear_sampling",))
        self.samp_on = False

    def slot_logprobs(self, slot, n):
        return [0.0] * n

    def set_top_logprobs(self, n, watch, max_new):
        assert self.samp_on and self.bound is None, "bound once, behind sampling"
        self.bound = (n, list(watch), max_new)
        self.calls.append(("set_top_logprobs", n, list(watch), max_new))

    def clear_top_logprobs(self):
        self.calls.append(("clear_top_logprobs",))
        self.bound = None

    def slot_top_logprobs(self, slot, n):
        st = self.slots[slot]
        N, watch, T = self.bound
        assert n <= min(len(st["out"]), T)
        rid, j = st["rid"], st.get("sample", 0)
        rows = [_entry(rid if t == 0 else rid + 100 * j, t, N, len(watch)) for t in range(n)]   # (entry 0 is the prompt's: a fork copies it)
        return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]

    def slots_fork(self, src, dsts, params, seeds, subseqs, staged=None):
        s0 = self.slots[src]
        assert len(s0["out"]) == 1, "fork before any decode step"
        self.calls.append(("slots_fork", src, list(dsts), list(subseqs), staged))
        for d, sub in zip(dsts, subseqs):
            assert self.slots[d] is None
            self.slots[d] = {"plan": s0["plan"], "budget": s0["budget"], "out": [s0["plan"][0]], "rid": s0["rid"], "sample": sub}


class TopEngine(_TopMixin, FakeEngine):
    def __init__(self, plans):
        FakeEngine.__init__(self, plans)
        self._init_top()


class TopStagedEngine(_TopMixin, FakeStagedEngine):
    def __init__(self, plans, lag=2):
        FakeStagedEngine.__init__(self, plans, lag)
        self._init_top()


@pytest.mark.parametrize("staged", [False, True])
def test_scheduler_trims_per_request_and_binds_once(staged):
    from emmax.sampling import SamplingParams
    from emmax.serving import Request, SlotScheduler

    lengths = [6, 3, 9, 4, 7, 5]
    plans = _plans(lengths)
    eng = TopStagedEngine(plans) if staged else TopEngine(plans)
    sch = SlotScheduler(eng, _encode_factory([]), n_slots=4, poll_every=2)
    assert sch.overlap == staged
    watch = [11, 11, 40]
    n_top = [0, 5, 20, 0, 2, 0]
    asks = [True, False, True, False, False, False]
    nsamp = [1, 1, 1, 1, 3, 1]
    samp = [None, None, SamplingParams(1.0, 0, 1.0, seed=5), None, SamplingParams(0.9, 0, 1.0, seed=6), None]
    for i in range(6):
        sch.submit(Request(i, i, [1, 2 + i], max_new_tokens=8 + i, sampling=samp[i], num_samples=nsamp[i], top_logprobs=n_top[i],
                           watch_ids=watch if asks[i] else None))
    res = sch.run()
    assert len(res) == 8
    # one binding for the run: the largest N, the one list, the largest budget -- behind sampling on every slot, cleared before sampling is
    binds = [c for c in eng.calls if c[0] == "set_top_logprobs"]
    assert binds == [("set_top_logprobs", 20, watch, 13)]
    assert eng.calls[0] == ("set_sampling", 0, [0.0] * 4) and eng.calls[1] == binds[0]
    assert eng.calls[-2:] == [("clear_top_logprobs",), ("clear_sampling",)] and eng.bound is None
    forks = [c for c in eng.calls if c[0] == "slots_fork"]
    assert len(forks) == 1 and forks[0][3] == [1, 2] and (forks[0][4] is not None) == staged
    for r in res:
        i, L = r.rid, len(r.ids)
        assert L == min(lengths[i], 8 + i)
        assert (r.top_logprobs is None) == (n_top[i] == 0) and (r.watch_logprobs is None) == (not asks[i])
        key = lambda t: i if t == 0 else i + 100 * r.sample   # entry 0 is the prompt's: the same for every sample of a group
        if n_top[i]:
            assert len(r.top_logprobs) == L and all(len(row) == n_top[i] for row in r.top_logprobs)
            for t, row in enumerate(r.top_logprobs):
                ids, lps, _ = _entry(key(t), t, 20, 3)
                assert row == list(zip(ids[: n_top[i]], lps[: n_top[i]])), (i, t)
        if asks[i]:
            assert r.watch_logprobs == [_entry(key(t), t, 20, 3)[2] for t in range(L)]
    assert sorted(r.sample for r in res if r.rid == 4) == [0, 1, 2]


def test_scheduler_one_watch_list_per_run_and_submit_checks():
    from emmax.serving import Request, SlotScheduler

    eng = TopEngine(_plans([3, 3]))
    sch = SlotScheduler(eng, _encode_factory([]), n_slots=2)
    for bad in (dict(top_logprobs=21), dict(top_logprobs=-1), dict(watch_ids=list(range(257))), dict(watch_ids=[-3])):
        with pytest.raises(ValueError):
            sch.submit(Request(9, 9, [1, 2], **bad))
    sch.submit(Request(0, 0, [1, 2], watch_ids=[4, 5]))
    sch.submit(Request(1, 1, [1, 2], watch_ids=[5, 4]))
    with pytest.raises(ValueError, match="one list"):
        sch.run()
    assert eng.calls == []   # refused at run, before the engine is touched


@pytest.mark.parametrize("staged", [False, True])
def test_scheduler_calls_nothing_new_when_nobody_asks(staged):
    """the fake engines of tests/test_serving.py have none of the new methods: a run without top_logprobs / watch_ids must not need them"""
    from emmax.serving import Request, SlotScheduler

    lengths = [5, 2, 7]
    eng = FakeStagedEngine(_plans(lengths)) if staged else FakeEngine(_plans(lengths))
    sch = SlotScheduler(eng, _encode_factory([]), n_slots=2, poll_every=2)
    for i in range(3):
        sch.submit(Request(i, i, [1, 2]))
    res = sch.run()
    assert sorted(len(r.ids) for r in res) == sorted(lengths)
    assert all(r.top_logprobs is None and r.watch_logprobs is None for r in res)


# ---- the C surface ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_documented_and_exported():
    """fails on the parent commit: the four symbols exist nowhere there"""
    from emmax import _lib

    header = open(os.path.join(ROOT, "include", "emmax.h")).read()
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    so = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(so, name), name
        assert re.search(r"^\|[^|]*`%s`" % name, table, re.M), f"{name} is missing from the INTEGRATION.md table"
    assert re.search(r"#define EMMAX_ABI_VERSION 12\b", header) and _lib.ABI_VERSION == 12
    assert re.search(r"#define EMMAX_MAX_TOP_LOGPROBS 20\b", header) and re.search(r"#define EMMAX_MAX_WATCH_IDS 256\b", header)
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW_SYMBOLS] == [11, 9, 2, 1]
    # host-side validation: null and out-of-range arguments are refused before anything launches
    assert so.emmax_session_top_logprobs(None) == -1
    assert so.emmax_session_set_top_logprobs(None, 5, None, None, 0, None, None, 8, None) == -1 and so.emmax_session_clear_top_logprobs(None, None) == -1
    assert so.emmax_op_top_logprobs(None, 40, 1, 40, 5, None, None, 0, None, None, None) == -1
    buf = (np.zeros(64, dtype=np.float32)).ctypes.data   # (a host address: the calls below are refused before any pointer is read)
    for ld, V, n, W in [(40, 40, 21, 0), (40, 40, 0, 257), (40, 10, 11, 0), (39, 40, 5, 0), (40, 40, -1, 0), (40, 0, 0, 1), (40000, 32769, 1, 0)]:
        assert so.emmax_op_top_logprobs(buf, ld, 1, V, n, buf, buf, W, buf, buf, None) == -1, (ld, V, n, W)
    assert so.emmax_op_top_logprobs(buf, 40, 1, 40, 5, None, buf, 0, None, None, None) == -1   # a null pointer of a part that is on
    assert so.emmax_op_top_logprobs(buf, 40, 1, 40, 0, None, None, 2, None, buf, None) == -1
