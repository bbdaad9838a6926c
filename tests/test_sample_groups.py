"""Sample groups, host side (no GPU): generate(do_sample=True, num_return_sequences=N) over a stub engine, the argument checks before the
engine is touched, the new C symbols in header / ctypes table / INTEGRATION.md / library, and the seeds and temperatures the GPU tests use,
fixed with the fp32 oracle and tests/sampling_ref.py so that "the rows of a group diverge" is a property of the inputs."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_groups_ref as sg  # noqa: E402
from conftest import ID_BUDGET_TINY, ROOT  # noqa: E402

NEW_SYMBOLS = ("emmax_session_set_sample_groups", "emmax_session_clear_sample_groups", "emmax_session_sample_groups")


def _model():
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    return EmmaXForActionPrediction(cfg, synthetic_state_dict(cfg, seed=1)), cfg


def _fake_generate_ids(m, cfg, lens, seen):
    def fake(rows, pixel_values=None, frames_u8=None, max_new_tokens=512, **kw):
        seen.clear()
        seen.update(kw)
        n = len(rows) * kw.get("num_samples", 1)
        ids = torch.full((n, max_new_tokens), cfg.pad_token_id, dtype=torch.int32)
        for r in range(n):
            ids[r, : lens[r]] = 100 + r
        return ids, torch.tensor(lens[:n], dtype=torch.int32)

    m.generate_ids = fake


def test_generate_returns_b_times_n_rows_in_hf_order():
    m, cfg = _model()
    m._need_engine = lambda: (_ for _ in ()).throw(AssertionError("no engine is needed for plain sequences"))
    lens, seen = [3, 6, 2, 5, 4, 1], {}
    _fake_generate_ids(m, cfg, lens, seen)
    rows = torch.tensor([[1, 7, 8], [1, 9, 10]])
    out = m.generate(rows, max_new_tokens=6, do_sample=True, num_return_sequences=3, seed=4)
    assert seen["num_samples"] == 3 and "beams" not in seen
    assert seen["sampling"].seed == 4
    assert out.shape == (2 * 3, 3 + 6) and out.dtype == torch.long       # [B N, P + T], T = the longest returned
    for r in range(6):   # row b N + j starts with prompt b: HF's expand_inputs_for_generation order
        want = rows[r // 3].tolist() + [100 + r] * lens[r]
        assert out[r].tolist() == want + [cfg.pad_token_id] * (9 - len(want)), r
    # N = 1 is a plain sampled call: generate_ids is called exactly as before
    lens[:] = [3, 2]
    out = m.generate(rows, max_new_tokens=6, do_sample=True, num_return_sequences=1, seed=4)
    assert "num_samples" not in seen and out.shape == (2, 3 + 3)
    m.generate(rows, max_new_tokens=6, do_sample=True, seed=4)
    assert "num_samples" not in seen
    m.generate(rows, max_new_tokens=6)
    assert "num_samples" not in seen and "beams" not in seen


def test_generate_scores_and_logits_have_b_times_n_rows():
    from emmax.modeling import EmmaXGenerateOutput

    m, cfg = _model()

    class Eng:
        device = "cpu"

    m._need_engine = lambda: Eng()
    lens, seen = [2, 4, 3, 1], {}
    _fake_generate_ids(m, cfg, lens, seen)
    rows = torch.tensor([[1, 7, 8], [1, 9, 10]])
    d = m.generate(rows, max_new_tokens=5, do_sample=True, num_return_sequences=2, seed=1, output_scores=True, output_logits=True,
                   return_dict_in_generate=True)
    V = cfg.llm.vocab_size
    assert isinstance(d, EmmaXGenerateOutput) and d.sequences.shape == (4, 3 + 4)
    assert seen["scores"].shape == seen["logits"].shape == (5, 4, V)
    assert len(d.scores) == len(d.logits) == 4 and d.scores[0].shape == d.logits[0].shape == (4, V)


def test_predict_action_and_batch_pass_the_group_on():
    m, cfg = _model()
    seen = {}

    def fake(rows, pixel_values=None, frames_u8=None, max_new_tokens=512, *a, **kw):
        seen.clear()
        seen.update(kw)
        n = len(rows) * kw.get("num_samples", 1)
        ids = torch.stack([m.vocab_size - 1 - 10 * r - torch.arange(7, dtype=torch.int32) for r in range(n)])   # distinct action bins per row
        return ids, torch.full((n,), 7, dtype=torch.int32)

    m.generate_ids = fake
    a = m.predict_action(torch.tensor([[1, 5, 6]]), unnorm_key=None, do_sample=True, num_return_sequences=4, seed=2)
    assert seen["num_samples"] == 4 and a.shape == (4, 7) and not np.array_equal(a[0], a[1])
    a1 = m.predict_action(torch.tensor([[1, 5, 6]]), unnorm_key=None, do_sample=True, seed=2)
    assert "num_samples" not in seen and a1.shape == (7,) and np.array_equal(a1, a[0])
    from emmax.sampling import SamplingParams

    acts, ids, lens = m.generate_actions_batch(None, [[1, 2], [1, 3]], max_new_tokens=7, sampling=SamplingParams(1.0, 0, 1.0, seed=3), num_samples=2)
    assert seen["num_samples"] == 2 and acts.shape == (4, 7) and ids.shape == (4, 7)
    m.generate_actions_batch(None, [[1, 2], [1, 3]], max_new_tokens=7)
    assert "num_samples" not in seen


def test_group_arguments_are_checked_before_the_engine():
    from emmax.sampling import BeamParams, SamplingParams

    m, cfg = _model()

    def no_engine():
        raise AssertionError("the engine was touched before the arguments were checked")

    m._need_engine = no_engine
    ids = torch.tensor([[1, 5, 6], [1, 7, 8]])
    for bad in (0, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="num_return_sequences"):
            m.generate(ids, max_new_tokens=4, do_sample=True, num_return_sequences=bad)
        with pytest.raises(ValueError, match="num_samples"):
            m.generate_ids([[1, 5, 6]], max_new_tokens=4, sampling=SamplingParams(1.0, 0, 1.0, seed=1), num_samples=bad)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.predict_action(ids[:1], unnorm_key=None, do_sample=True, num_return_sequences=0)
    with pytest.raises(ValueError, match="num_samples"):
        m.generate_actions_batch(None, [[1, 2]], sampling=SamplingParams(1.0, 0, 1.0, seed=1), num_samples=0)
    # B x N above the decode batch: both numbers are named
    with pytest.raises(ValueError, match=r"2 prompts x 33 samples"):
        m.generate(ids, max_new_tokens=4, do_sample=True, num_return_sequences=33)
    with pytest.raises(ValueError, match=r"2 prompts x 33 samples"):
        m.generate_ids([[1, 5, 6], [1, 7, 8]], max_new_tokens=4, sampling=SamplingParams(1.0, 0, 1.0, seed=1), num_samples=33)
    # N greedy rows of one prompt are identical: refused, as HF refuses them
    with pytest.raises(ValueError, match="greedy"):
        m.generate_ids([[1, 5, 6]], max_new_tokens=4, num_samples=2)
    with pytest.raises(ValueError, match="[Gg]reedy"):
        m.generate(ids, max_new_tokens=4, num_return_sequences=2)
    with pytest.raises(ValueError, match="beams"):
        m.generate_ids([[1, 5, 6]], max_new_tokens=4, beams=BeamParams(2), num_samples=2)
    # what stays as it is
    with pytest.raises(NotImplementedError, match="beam sampling"):
        m.generate(ids, max_new_tokens=4, do_sample=True, num_beams=2, num_return_sequences=2)
    with pytest.raises(NotImplementedError):
        m.generate_actions(image=None, prompt_text="x", type="act", do_sample=True, num_return_sequences=2)
    # valid arguments reach the engine
    with pytest.raises(AssertionError, match="engine was touched"):
        m.generate(ids, max_new_tokens=4, do_sample=True, num_return_sequences=3, seed=1)


def test_prefill_sets_and_clears_groups_on_the_engine():
    """_prefill turns groups on for N > 1 (after beams are cleared and sampling is set for all B N rows) and clears what an earlier call left."""
    from emmax.sampling import SamplingParams

    m, cfg = _model()
    calls = []

    class Eng:
        beams = 0
        sample_groups = 0
        processing = sampling = scores_bound = False

        def max_decode_batch(self):
            return 8

        def ensure_capacity(self, *a):
            calls.append(("capacity", a[0]))

        def set_sampling(self, p, n=None):
            calls.append(("sampling", n))

        def clear_sampling(self):
            calls.append(("clear_sampling",))

        def set_sample_groups(self, n):
            calls.append(("groups", n))
            self.sample_groups = n

        def clear_sample_groups(self):
            calls.append(("clear_groups",))
            self.sample_groups = 0

        def prefill(self, rows, patches):
            calls.append(("prefill", len(rows)))

    eng = Eng()
    m._need_engine = lambda: eng
    m._encode_images = lambda *a: None
    fr = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    m._prefill([[1, 2], [1, 3]], frames_u8=fr, max_new=4, sampling=SamplingParams(1.0, 0, 1.0, seed=1), num_samples=3)
    assert calls == [("capacity", 6), ("sampling", 6), ("groups", 3), ("prefill", 2)]
    calls.clear()
    m._prefill([[1, 2], [1, 3]], frames_u8=fr, max_new=4)
    assert calls == [("capacity", 2), ("clear_groups",), ("prefill", 2)] and eng.sample_groups == 0
    with pytest.raises(ValueError, match=r"2 prompts x 5 samples exceed the 8 rows"):
        m._prefill([[1, 2], [1, 3]], frames_u8=fr, max_new=4, sampling=SamplingParams(1.0, 0, 1.0, seed=1), num_samples=5)


def test_new_symbols_are_declared_bound_documented_and_exported():
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
    assert re.search(r"#define EMMAX_ABI_VERSION 12\b", header) and _lib.ABI_VERSION == 12   # (additions to ABI 11; 12: the prefill stage ops)
    assert so.emmax_session_sample_groups(None) == -1
    assert so.emmax_session_set_sample_groups(None, 2, None) != 0 and so.emmax_session_clear_sample_groups(None, None) != 0   # null session


@pytest.fixture(scope="module")
def oracle_weights():
    from emmax.config import EmmaXConfig
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    return cfg, {k: v.to(torch.bfloat16).float() for k, v in synthetic_state_dict(cfg, seed=sg.WEIGHT_SEED).items()}


@pytest.mark.parametrize("name", list(sg.CASES))
def test_pinned_seeds_make_the_rows_of_every_group_diverge(oracle_weights, name):
    """For the inputs, temperature and seed the GPU tests use: in every group the step-0 reference draws whose Gumbel margin (and kept-set
    slack) clears 2 ID_BUDGET_TINY max|logit| / T hold at least two distinct tokens.  A device whose logits are within the budget must draw
    those tokens, so its rows diverge at step 0 whatever the hardware does below the budget."""
    cfg, sd_ref = oracle_weights
    L = sg.first_rows(name, cfg, sd_ref)
    T0 = sg.temperature(L[0])
    print(name, "T0 of the oracle", T0, "pinned", sg.T0[name])
    assert T0 > 0 and abs(T0 - sg.T0[name]) <= 1e-5 * T0   # (the oracle's BLAS may order a sum differently: the draws below use the pinned value)
    draws = sg.step0_draws(name, L, ID_BUDGET_TINY)
    N = sg.CASES[name][2]
    assert len(draws) == len(sg.CASES[name][1]) and all(len(g) == N for g in draws)
    print(name, "draws", draws)
    assert sg.diverge(draws), (name, draws)
    if name == "mixed":   # one row of the mixed case is greedy: the row the GPU test compares with a plain greedy run
        assert sg.row_grid(name)[0][0] == 0.0 and sg.params(name)[0].temperature == 0.0
