"""CPU: sampling in the decode step at the host layer -- the argument checks of modeling.generate(do_sample=True) (before any engine call),
and the slot scheduler's order of set_sampling vs. prefill / staged prefill against a fake engine.  Greedy-only serves never call the new
engine methods (the fakes of test_serving.py do not have them)."""
import pytest
import torch

from emmax.sampling import SamplingParams
from emmax.serving import Request, SlotScheduler

from test_serving import FakeEngine, FakeStagedEngine


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


def test_generate_rejects_bad_sampling_arguments_before_the_engine(model):
    ids = torch.tensor([[1, 5, 6]])
    for kw in ({"temperature": 0.0}, {"temperature": -1.0}, {"top_p": 0.0}, {"top_p": 1.5}, {"top_k": -1}, {"temperature": float("nan")}):
        with pytest.raises(ValueError):
            model.generate(ids, do_sample=True, max_new_tokens=4, **kw)
    with pytest.raises(NotImplementedError):
        model.generate(ids, do_sample=True, num_beams=2, max_new_tokens=4)
    with pytest.raises(NotImplementedError):   # generate_actions stays greedy, as the reference only ever calls it
        model.generate_actions(image=None, prompt_text="x", type="act", do_sample=True)


def test_sampling_arguments_take_the_hf_defaults_and_torch_seed(model):
    p = model._sampling_args(True, seed=7)
    assert (p.temperature, p.top_k, p.top_p, p.seed) == (1.0, 50, 1.0, 7)
    assert model._sampling_args(True, 0.7, 0, 0.9, 3) == SamplingParams(0.7, 0, 0.9, 3)
    torch.manual_seed(11)
    a = model._sampling_args(True)
    torch.manual_seed(11)
    b = model._sampling_args(True)
    assert a == b and a.seed is not None
    g = torch.Generator().manual_seed(5)
    assert model._sampling_args(True, generator=g).seed == model._sampling_args(True, generator=torch.Generator().manual_seed(5)).seed
    state = torch.get_rng_state()
    assert model._sampling_args(False, temperature=0.0) is None   # greedy: nothing drawn, temperature 0 allowed (openvla_utils.py calls it so)
    assert torch.equal(state, torch.get_rng_state())


class SamplingFake(FakeEngine):
    def __init__(self, plans):
        super().__init__(plans)
        self.calls = []

    def set_sampling(self, params, seeds=None, subseqs=None, row0=0):
        self.calls.append(("set", row0, [p.temperature for p in params], list(seeds), list(subseqs)))

    def clear_sampling(self):
        self.calls.append(("clear",))

    def slot_prefill(self, slot, ids, pe, max_new):
        self.calls.append(("prefill", slot))
        super().slot_prefill(slot, ids, pe, max_new)

    def slot_logprobs(self, slot, n):
        return [-1.0] * n


class SamplingStagedFake(FakeStagedEngine):
    def __init__(self, plans, lag=2):
        super().__init__(plans, lag)
        self.calls = []

    def set_sampling_staged(self, params, seeds=None, subseqs=None):
        assert self.in_admission, "staged parameters go on the admission stream"
        self.calls.append(("set_staged", [p.temperature for p in params], list(seeds), list(subseqs)))

    def clear_sampling(self):
        self.calls.append(("clear",))

    def slots_prefill_staged(self, prompts, embeds, max_new):
        self.calls.append(("staged", len(prompts)))
        return super().slots_prefill_staged(prompts, embeds, max_new)

    def slot_logprobs(self, slot, n):
        return [-1.0] * n


def _encode(frames):
    return [{"rid": f, "encoded": True} for f in frames]


def _plans(n):
    return {i: [100 + i] * (3 + i % 4) for i in range(n)}


def test_scheduler_sets_parameters_before_each_prefill():
    eng = SamplingFake(_plans(6))
    sch = SlotScheduler(eng, _encode, n_slots=2, poll_every=1)
    for i in range(6):
        sch.submit(Request(i, i, [1, 2], max_new_tokens=8, sampling=SamplingParams(0.9, 10, 1.0, seed=40 + i) if i % 2 else None))
    res = sch.run()
    assert sorted(r.rid for r in res) == list(range(6))
    prefills = [k for k, c in enumerate(eng.calls) if c[0] == "prefill"]
    assert len(prefills) == 6
    for k in prefills:   # every prefill right after the parameters of its own slot
        assert eng.calls[k - 1][0] == "set" and eng.calls[k - 1][1] == eng.calls[k][1]
    sets = [c for c in eng.calls if c[0] == "set"]
    assert sorted((c[2][0], c[3][0]) for c in sets) == sorted([(0.0, 0)] * 3 + [(0.9, 40 + i) for i in (1, 3, 5)])
    assert all(c[4] == [0] for c in sets)   # a request draws with its own seed and subseq 0
    assert eng.calls[-1] == ("clear",)
    for r in res:
        assert (r.logprobs is None) == (r.rid % 2 == 0)


def test_scheduler_sets_staged_parameters_before_the_staged_prefill():
    eng = SamplingStagedFake(_plans(7))
    sch = SlotScheduler(eng, _encode, n_slots=3, poll_every=1, overlap=True, stage_batch=2)
    for i in range(7):
        sch.submit(Request(i, i, [1, 2], max_new_tokens=8, sampling=SamplingParams(1.0, 0, 0.8, seed=i) if i == 4 else None))
    sch.run()
    staged = [k for k, c in enumerate(eng.calls) if c[0] == "staged"]
    assert staged
    for k in staged:
        assert eng.calls[k - 1][0] == "set_staged" and len(eng.calls[k - 1][1]) == eng.calls[k][1]
    assert any(c[0] == "set_staged" and 1.0 in c[1] for c in eng.calls)
    assert eng.calls[-1] == ("clear",)


def test_greedy_serve_never_calls_the_sampling_methods():
    # the plain fakes lack set_sampling / clear_sampling / slot_logprobs: any call would raise AttributeError
    for eng, kw in ((FakeEngine(_plans(5)), {}), (FakeStagedEngine(_plans(5)), {"overlap": True})):
        sch = SlotScheduler(eng, _encode, n_slots=2, poll_every=1, **kw)
        for i in range(5):
            sch.submit(Request(i, i, [1, 2], max_new_tokens=8))
        res = sch.run()
        assert sorted(r.rid for r in res) == list(range(5)) and all(r.logprobs is None for r in res)
