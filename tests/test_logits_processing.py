"""CPU: logits processing at the host layer (include/emmax.h ABI 8).  The numpy reference of processing_ref.py against transformers'
own processors and warpers; the argument checks of modeling.generate (before any engine call); neutral values leave processing off;
the return_dict_in_generate output against a patched generate_ids; the slot scheduler's call order against fake engines (a serve
without processing never calls the new methods)."""
import numpy as np
import pytest
import torch

import processing_ref as pref
from emmax.sampling import LogitsProcessing, SamplingParams
from emmax.serving import Request, SlotScheduler

from test_serving import FakeEngine, FakeStagedEngine

EOS = 2


def _row(rng, V):
    return (rng.standard_normal(V) * 3).astype(np.float32)   # about half the entries negative


def _hist(rng, V, L):
    pool = rng.integers(0, V, size=max(2, L // 3))   # a small pool: ids and n-grams repeat
    return [int(x) for x in rng.choice(pool, size=L)]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_reference_matches_transformers_processors(n):
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(100 + n)
    V = 97
    for trial in range(20):
        P = int(rng.integers(1, 12))
        n_out = int(rng.integers(0, 10))
        hist = _hist(rng, V, P + n_out)
        row = _row(rng, V)
        pen = float(rng.choice([0.7, 1.1, 1.3, 1.5, 2.0]))
        m = int(rng.integers(0, 12))
        ids = torch.tensor([hist], dtype=torch.long)
        want = torch.from_numpy(row.copy())[None]
        want = lp.RepetitionPenaltyLogitsProcessor(pen)(ids, want)
        want = lp.NoRepeatNGramLogitsProcessor(n)(ids, want)
        want = lp.MinNewTokensLengthLogitsProcessor(P, m, EOS)(ids, want)
        got = pref.process_row(row, hist, n_out, pen, n, m, EOS)
        np.testing.assert_array_equal(got, want[0].numpy())
        if n_out < m:
            assert got[EOS] == -np.inf
        # HF min_length L on this row (prompt P): the same ban while P + n_out < L
        L = P + m
        ml = lp.MinLengthLogitsProcessor(L, EOS)(ids, torch.from_numpy(row.copy())[None])[0].numpy()
        np.testing.assert_array_equal(ml, pref.process_row(row, hist, n_out, min_new=max(0, L - P), eos_id=EOS))


def test_min_new_tokens_boundary():
    row = np.zeros(8, dtype=np.float32)
    assert pref.process_row(row, [1, 3], 5, min_new=6)[EOS] == -np.inf
    assert pref.process_row(row, [1, 3], 6, min_new=6)[EOS] == 0.0
    assert pref.process_row(row, [1, 3], 0, min_new=0)[EOS] == 0.0


def test_scores_reference_matches_transformers_warpers():
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(5)
    V = 211
    for T, k in ((0.7, 0), (1.0, 20), (1.3, 5)):
        hist = _hist(rng, V, 30)
        proc = pref.process_row(_row(rng, V), hist, 10, 1.2, 3, 0)
        want = torch.from_numpy(proc.copy())[None]
        want = lp.TemperatureLogitsWarper(T)(None, want)
        if k:
            want = lp.TopKLogitsWarper(k)(None, want)
        np.testing.assert_array_equal(pref.scores_row(proc, T, k, 1.0), want[0].numpy())
    proc = pref.process_row(_row(rng, V), _hist(rng, V, 20), 4, 1.5, 2, 0)
    np.testing.assert_array_equal(pref.scores_row(proc), proc)


def test_reference_edges():
    assert pref.banned_ngram_ids([5, 6, 7, 5, 6], 3) == {7}
    assert pref.banned_ngram_ids([5, 6], 3) == set()          # HF: cur_len + 1 < n bans nothing; L = n - 1 has no n-gram yet
    assert pref.banned_ngram_ids([4, 4, 9], 1) == {4, 9}      # n = 1: every id seen
    row = np.array([2.0, -2.0, 1.0, 0.5], dtype=np.float32)
    got = pref.process_row(row, [0, 1, 1, 0], 0, penalty=2.0, eos_id=3)   # once per id, whatever the multiplicity
    np.testing.assert_array_equal(got, np.array([1.0, -4.0, 1.0, 0.5], dtype=np.float32))
    assert pref.greedy(np.full(4, -np.inf, dtype=np.float32)) == -1


def test_logits_processing_validates():
    assert LogitsProcessing().neutral
    for kw in ({"repetition_penalty": 0.0}, {"repetition_penalty": -1.0}, {"repetition_penalty": float("nan")}, {"repetition_penalty": float("inf")},
               {"no_repeat_ngram_size": -1}, {"no_repeat_ngram_size": 33}, {"no_repeat_ngram_size": 1.5}, {"min_new_tokens": -1},
               {"min_new_tokens": 2.5}):
        with pytest.raises(ValueError):
            LogitsProcessing(**kw)
    assert not LogitsProcessing(no_repeat_ngram_size=32).neutral


@pytest.fixture(scope="module")
def model():
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    m = EmmaXForActionPrediction(cfg, synthetic_state_dict(cfg, seed=1))

    def no_engine():
        raise AssertionError("the engine was touched before the arguments were checked")

    m._need_engine = no_engine
    return m


def test_generate_rejects_bad_processor_arguments_before_the_engine(model):
    ids = torch.tensor([[1, 5, 6]])
    for kw in ({"repetition_penalty": 0.0}, {"repetition_penalty": -2.0}, {"no_repeat_ngram_size": -1}, {"no_repeat_ngram_size": 40},
               {"min_new_tokens": -3}, {"min_length": -1}, {"min_length": 2.5}):
        with pytest.raises(ValueError):
            model.generate(ids, max_new_tokens=4, **kw)
    with pytest.raises(ValueError):
        model.predict_action(ids, unnorm_key=None, repetition_penalty=-1.0)
    with pytest.raises(NotImplementedError):   # still pinned
        model.generate(ids, num_beams=2, repetition_penalty=1.2, max_new_tokens=4)
    with pytest.raises(NotImplementedError):
        model.generate_actions(image=None, prompt_text="x", type="act", do_sample=True, repetition_penalty=1.2)


def test_neutral_values_leave_processing_off(model):
    rows = [[1, 5, 6, 7], [1, 9]]
    assert model._processing_args(rows) is None
    assert model._processing_args(rows, 1.0, 0, 0, 1) is None
    assert model._processing_args(rows, None, None, None, 4) is None          # min_length within the prompt
    assert model._processing_args(rows, 1.1, None, None, None) == LogitsProcessing(1.1, 0, 0)
    assert model._processing_args(rows, None, 3, None, None) == LogitsProcessing(1.0, 3, 0)
    assert model._processing_args(rows, None, None, 2, 9) == LogitsProcessing(1.0, 0, 5)   # m = max(2, 9 - P_max 4)
    assert model._processing_args(rows, None, None, 7, 9) == LogitsProcessing(1.0, 0, 7)


class _Patched:
    """generate_ids stand-in: fills the bound score / logit buffers like the step (index t < lens[b] only) and records the call."""

    def __init__(self, lens, V):
        self.lens, self.V, self.calls = lens, V, []

    def __call__(self, rows, pixel_values, frames_u8, max_new_tokens, sampling=None, processing=None, scores=None, logits=None):
        self.calls.append({"processing": processing, "scores": scores is not None, "logits": logits is not None, "max_new": max_new_tokens})
        B = len(rows)
        ids = torch.full((B, max_new_tokens), 0, dtype=torch.int32)
        for b, n in enumerate(self.lens):
            ids[b, :n] = torch.arange(10, 10 + n)
            for buf, base in ((scores, 1.0), (logits, 2.0)):
                if buf is not None:
                    for t in range(n):
                        buf[t, b] = base + t
        return ids, torch.tensor(self.lens, dtype=torch.int32)


def test_return_dict_in_generate_structure(monkeypatch):
    from types import SimpleNamespace

    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction, EmmaXGenerateOutput

    cfg = EmmaXConfig.tiny()
    m = EmmaXForActionPrediction(cfg, None)
    V = cfg.llm.vocab_size
    fake = _Patched([3, 1], V)
    monkeypatch.setattr(m, "generate_ids", fake)
    monkeypatch.setattr(m, "_need_engine", lambda: SimpleNamespace(device="cpu"))
    ids = torch.tensor([[1, 5, 6], [1, 7, 8]])
    plain = m.generate(ids, max_new_tokens=5)
    assert isinstance(plain, torch.Tensor) and fake.calls[-1] == {"processing": None, "scores": False, "logits": False, "max_new": 5}
    assert isinstance(m.generate(ids, max_new_tokens=5, output_scores=True), torch.Tensor)   # as HF: scores need return_dict_in_generate
    assert not fake.calls[-1]["scores"]
    out = m.generate(ids, max_new_tokens=5, return_dict_in_generate=True, output_scores=True, output_logits=True, repetition_penalty=1.3)
    assert isinstance(out, EmmaXGenerateOutput) and torch.equal(out.sequences, plain) and torch.equal(out["sequences"], plain)
    assert fake.calls[-1]["processing"] == LogitsProcessing(1.3, 0, 0)
    assert isinstance(out.scores, tuple) and len(out.scores) == 3 and len(out.logits) == 3
    for t in range(3):
        assert out.scores[t].shape == (2, V) and out.scores[t].dtype == torch.float32
        assert torch.all(out.scores[t][0] == 1.0 + t) and torch.all(out.logits[t][0] == 2.0 + t)
    assert torch.all(out.scores[0][1] == 1.0)
    for t in (1, 2):   # past row 1's length
        assert torch.isnan(out.scores[t][1]).all() and torch.isnan(out.logits[t][1]).all()
    only = m.generate(ids, max_new_tokens=5, return_dict_in_generate=True)
    assert only.scores is None and only.logits is None and torch.equal(only.sequences, plain)
    assert not fake.calls[-1]["scores"] and not fake.calls[-1]["logits"]
    m.generate(ids, max_new_tokens=5, min_length=9)   # min_length beyond the prompt: m = 9 - 3, max_new untouched
    assert fake.calls[-1]["processing"] == LogitsProcessing(1.0, 0, 6) and fake.calls[-1]["max_new"] == 5


class ProcFake(FakeEngine):
    def __init__(self, plans):
        super().__init__(plans)
        self.calls = []

    def set_processing(self, params, row0=0):
        self.calls.append(("proc", row0, [p.repetition_penalty for p in params]))

    def clear_processing(self):
        self.calls.append(("clear_proc",))

    def set_sampling(self, params, seeds=None, subseqs=None, row0=0):
        self.calls.append(("set", row0))

    def clear_sampling(self):
        self.calls.append(("clear",))

    def slot_prefill(self, slot, ids, pe, max_new):
        self.calls.append(("prefill", slot))
        super().slot_prefill(slot, ids, pe, max_new)

    def slot_logprobs(self, slot, n):
        return [-1.0] * n


class ProcStagedFake(FakeStagedEngine):
    def __init__(self, plans, lag=2):
        super().__init__(plans, lag)
        self.calls = []

    def set_processing_staged(self, params):
        assert self.in_admission, "staged parameters go on the admission stream"
        self.calls.append(("proc_staged", [p.repetition_penalty for p in params]))

    def clear_processing(self):
        self.calls.append(("clear_proc",))

    def slots_prefill_staged(self, prompts, embeds, max_new):
        self.calls.append(("staged", len(prompts)))
        return super().slots_prefill_staged(prompts, embeds, max_new)


def _encode(frames):
    return [{"rid": f, "encoded": True} for f in frames]


def _plans(n):
    return {i: [100 + i] * (3 + i % 4) for i in range(n)}


def test_scheduler_sets_processing_then_sampling_before_each_prefill():
    eng = ProcFake(_plans(6))
    sch = SlotScheduler(eng, _encode, n_slots=2, poll_every=1)
    for i in range(6):
        sch.submit(Request(i, i, [1, 2], max_new_tokens=8, processing=LogitsProcessing(1.5, 2, 0) if i % 3 == 0 else None,
                           sampling=SamplingParams(0.9, 10, 1.0, seed=i) if i == 1 else None))
    sch.run()
    prefills = [k for k, c in enumerate(eng.calls) if c[0] == "prefill"]
    assert len(prefills) == 6
    for k in prefills:   # processing, then sampling, then the prefill, all for the same slot
        assert eng.calls[k - 1] == ("set", eng.calls[k][1]) and eng.calls[k - 2][:2] == ("proc", eng.calls[k][1])
    pens = sorted(c[2][0] for c in eng.calls if c[0] == "proc")
    assert pens == [1.0] * 4 + [1.5] * 2   # requests without processing get neutral processors
    assert set(eng.calls[-2:]) == {("clear_proc",), ("clear",)}


def test_scheduler_sets_staged_processing_before_the_staged_prefill():
    eng = ProcStagedFake(_plans(7))
    sch = SlotScheduler(eng, _encode, n_slots=3, poll_every=1, overlap=True, stage_batch=2)
    for i in range(7):
        sch.submit(Request(i, i, [1, 2], max_new_tokens=8, processing=LogitsProcessing(1.2, 0, 3) if i == 4 else None))
    sch.run()
    staged = [k for k, c in enumerate(eng.calls) if c[0] == "staged"]
    assert staged
    for k in staged:
        assert eng.calls[k - 1][0] == "proc_staged" and len(eng.calls[k - 1][1]) == eng.calls[k][1]
    assert eng.calls[-1] == ("clear_proc",)


def test_serves_without_processing_never_call_the_processing_methods():
    # the plain fakes lack set_processing / clear_processing: any call would raise AttributeError
    for eng, kw in ((FakeEngine(_plans(5)), {}), (FakeStagedEngine(_plans(5)), {"overlap": True})):
        sch = SlotScheduler(eng, _encode, n_slots=2, poll_every=1, **kw)
        for i in range(5):
            sch.submit(Request(i, i, [1, 2], max_new_tokens=8))
        assert sorted(r.rid for r in sch.run()) == list(range(5))


class _StubEngine:
    """Records every call: a refused buffer must leave it untouched."""

    def __init__(self, V):
        from types import SimpleNamespace

        self.cfg = SimpleNamespace(llm=SimpleNamespace(vocab_size=V))
        self.device = "cpu"
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: self.calls.append(name)


def test_score_buffers_with_another_batch_dimension_are_refused_before_anything_is_bound(monkeypatch):
    from emmax.config import EmmaXConfig
    from emmax.engine import EmmaxEngine
    from emmax.modeling import EmmaXForActionPrediction

    cfg = EmmaXConfig.tiny()
    V = cfg.llm.vocab_size
    m = EmmaXForActionPrediction(cfg, None)
    stub = _StubEngine(V)
    monkeypatch.setattr(m, "_need_engine", lambda: stub)
    monkeypatch.setattr(m, "_prefill", lambda *a, **k: stub.calls.append("_prefill"))
    rows = [[1, 5, 6], [1, 7]]
    for bad in (torch.empty(4, 1, V), torch.empty(4, 3, V), torch.empty(5, 2, V), torch.empty(4, 2, V - 1), torch.empty(4, 2, V, dtype=torch.float16),
                torch.empty(2, 4, V).transpose(0, 1)):
        for kw in ({"scores": bad}, {"logits": bad}, {"scores": torch.empty(4, 2, V), "logits": bad}):
            with pytest.raises(ValueError):
                m.generate_ids(rows, max_new_tokens=4, **kw)
            with pytest.raises(ValueError):   # the host layer below generate_ids refuses them too
                EmmaXForActionPrediction._set_processing(stub, 2, None, kw.get("scores"), kw.get("logits"), 4)
    assert stub.calls == []
    # the engine itself: the batch dimension must be the rows it is told (before any C call)
    eng = _StubEngine(V)
    eng.device = "cpu"
    with pytest.raises(ValueError):
        EmmaxEngine.set_scores(eng, torch.empty(4, 1, V), None, 4, rows=2)
    with pytest.raises(ValueError):
        EmmaxEngine.set_scores(eng, torch.empty(4, 2, V), None, 4)   # rows not given
    assert eng.calls == []
    # the right shape passes the checks and reaches the prefill
    stub.generate = lambda n, stop, return_logprobs=False: (torch.zeros(2, n, dtype=torch.int32), torch.ones(2, dtype=torch.int32))
    m.generate_ids(rows, max_new_tokens=4, scores=torch.empty(4, 2, V))
    assert stub.calls[0] == "_prefill"


def test_generate_ids_unbinds_the_buffers_when_it_returns(monkeypatch):
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction

    cfg = EmmaXConfig.tiny()
    V = cfg.llm.vocab_size
    m = EmmaXForActionPrediction(cfg, None)
    calls = []

    class Eng:
        def generate(self, n, stop, return_logprobs=False):
            calls.append("generate")
            return torch.zeros(2, n, dtype=torch.int32), torch.ones(2, dtype=torch.int32)

        def set_scores(self, scores, logits, max_new=0, rows=0):
            calls.append(("set_scores", scores is None and logits is None))

    eng = Eng()
    monkeypatch.setattr(m, "_need_engine", lambda: eng)
    monkeypatch.setattr(m, "_prefill", lambda *a, **k: calls.append("_prefill"))
    m.generate_ids([[1, 5], [1, 6]], max_new_tokens=3, logits=torch.empty(3, 2, V))
    assert calls == ["_prefill", "generate", ("set_scores", True)]
    calls.clear()
    m.generate_ids([[1, 5], [1, 6]], max_new_tokens=3)
    assert calls == ["_prefill", "generate"]
