"""Beam search, host side (no GPU): tests/beam_ref.py against transformers' own beam search, BeamParams, the argument checks of the
model's public calls before the engine is touched, output shapes over a stub engine, and the refusals of serving / dist."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402

from emmax.sampling import BeamParams  # noqa: E402

SEEDS = (11, 23)          # fixed: the cases below are the same on every run
VOCAB, T, PAD = 512, 24, 3   # (a pad id of 0 would make HF fill with the EOS id instead: `pad_token_id or eos_token_id`)
LM_SCALE = 60.0           # a randomly initialised model is nearly flat: candidates closer than fp32 can tell apart


def _tiny_llama(seed):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=VOCAB, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=4, max_position_embeddings=128, pad_token_id=PAD, bos_token_id=1, eos_token_id=2,
                      tie_word_embeddings=False)
    m = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(LM_SCALE)
    return m


def _step_fn(model, prompt):
    def fn(seqs):
        ids = torch.tensor([prompt + list(s) for s in seqs], dtype=torch.long)
        with torch.no_grad():
            return model(input_ids=ids).logits[:, -1, :].float().numpy()
    return fn


def _pick_eos(model, prompt, K):
    """An id that beams of this model really emit at different steps: the most frequent token among the running beams of an EOS-free run
    between steps 2 and T / 2."""
    r = beam_ref.beam_search(_step_fn(model, prompt), K, VOCAB, T, eos=-1, pad=PAD)
    toks = [t for rec in r["trace"][2: T // 2] for t in rec["tok"]]
    vals, counts = np.unique(np.array(toks), return_counts=True)
    return int(vals[np.argmax(counts)])


CASES = list(itertools.product((2, 4, 8), (0.0, 1.0, 2.0), (False, True, "never")))


def test_beam_ref_matches_transformers_beam_search():
    """K in {2, 4, 8} x length_penalty in {0, 1, 2} x early_stopping in {False, True, "never"} x num_return_sequences in {1, K}, two seeds:
    sequences and beam_indices equal, sequences_scores within 1e-5 relative.  A case whose smallest gap between adjacent candidates among
    the best 2K + 1 is below 1e-5 * max(1, |score|) is left out (HF's own fp32 log-softmax may order it either way); at most a quarter may be."""
    total = skipped = 0
    length_sets = []
    for seed in SEEDS:
        model = _tiny_llama(seed)
        prompt = [1] + [int(x) for x in np.random.default_rng(seed).integers(3, VOCAB, size=7)]
        eos_of = {K: _pick_eos(model, prompt, K) for K in (2, 4, 8)}
        for K, lp, es in CASES:
            eos = eos_of[K]
            ref = beam_ref.beam_search(_step_fn(model, prompt), K, VOCAB, T, eos=eos, pad=PAD, length_penalty=lp, early_stopping=es, gaps=True)
            for nrs in (1, K):
                total += 1
                if ref["min_gap"] < 1e-5:
                    skipped += 1
                    continue
                out = model.generate(torch.tensor([prompt]), attention_mask=torch.ones(1, len(prompt), dtype=torch.long), max_new_tokens=T,
                                     num_beams=K, num_return_sequences=nrs, length_penalty=lp, early_stopping=es, do_sample=False,
                                     eos_token_id=eos, pad_token_id=PAD, return_dict_in_generate=True, output_scores=True)
                P = len(prompt)
                hf_new = out.sequences[:, P:].numpy()
                Tl = hf_new.shape[1]
                lens = ref["lengths"][:nrs]
                assert Tl == int(lens.max()), (seed, K, lp, es, nrs, Tl, lens)
                assert np.array_equal(hf_new, ref["sequences"][:nrs, :Tl]), (seed, K, lp, es, nrs)
                assert np.array_equal(out.beam_indices.numpy(), ref["beam_indices"][:nrs, :Tl]), (seed, K, lp, es, nrs)
                hs, rs = out.sequences_scores.numpy().astype(np.float64), ref["scores"][:nrs].astype(np.float64)
                assert np.all(np.abs(hs - rs) <= 1e-5 * np.maximum(1.0, np.abs(rs))), (seed, K, lp, es, nrs, hs, rs)
                if nrs == K:
                    length_sets.append(len(set(int(x) for x in lens)))
    assert skipped * 4 <= total, f"{skipped} of {total} cases left out for near-equal candidates"
    assert max(length_sets) > 1, "no case finished hypotheses of different lengths: the EOS choice shows nothing"
    assert sum(1 for n in length_sets if n > 1) >= len(length_sets) // 4


def test_beam_ref_replays_its_own_trace_and_orders_ties_by_flat_index():
    rng = np.random.default_rng(5)
    V, K = 64, 4
    rows = rng.standard_normal((K, V)).astype(np.float32)
    rows[1:] = rows[0]                     # equal rows and equal scores: every candidate is tied across the four beams
    g = beam_ref.BeamGroup(K, V, 8)
    rec = g.step(rows, scores=np.zeros(K, np.float32))
    idx = rec["cand_idx"]
    acc = np.array(rec["cand_acc"], np.float32)
    assert all(acc[i] >= acc[i + 1] for i in range(len(acc) - 1))
    for i in range(len(acc) - 1):
        if acc[i] == acc[i + 1]:
            assert idx[i] < idx[i + 1]
    assert idx[0] // V == 0 and idx[:4] == [idx[0] + b * V for b in range(4)]   # a tie goes to the lower beam first
    rows[3] = rng.standard_normal(V).astype(np.float32)
    # a row with a NaN contributes nothing
    rows[2, 3] = np.nan
    g2 = beam_ref.BeamGroup(K, V, 8)
    rec2 = g2.step(rows, scores=np.zeros(K, np.float32))
    assert all(i // V != 2 for i in rec2["cand_idx"])
    g3 = beam_ref.BeamGroup(2, V, 8)
    rec3 = g3.step(np.full((2, V), np.nan, np.float32))
    assert rec3["done"] and rec3["cand_idx"] == [-1] * 4


def test_beam_params_validation():
    assert BeamParams(4).num_return_sequences == 1 and BeamParams(4).early_stopping is False and BeamParams(4).length_penalty == 1.0
    BeamParams(8, 0.0, "never", 8)
    for bad in (dict(num_beams=1), dict(num_beams=9), dict(num_beams=2.0), dict(num_beams=True), dict(num_beams=4, length_penalty=float("inf")),
                dict(num_beams=4, length_penalty=float("nan")), dict(num_beams=4, early_stopping="always"), dict(num_beams=4, early_stopping=1),
                dict(num_beams=4, num_return_sequences=5), dict(num_beams=4, num_return_sequences=0)):
        with pytest.raises(ValueError):
            BeamParams(**bad)


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


def test_beam_arguments_are_checked_before_the_engine(model):
    ids = torch.tensor([[1, 5, 6]])
    for kw in (dict(num_beams=0), dict(num_beams=9), dict(num_beams=2, num_return_sequences=3), dict(num_beams=2, early_stopping="sometimes"),
               dict(num_beams=2, length_penalty=float("nan")), dict(num_beams=1, num_return_sequences=2), dict(num_beams=2.5)):
        with pytest.raises(ValueError):
            model.generate(ids, max_new_tokens=4, **kw)
    with pytest.raises(ValueError):
        model.predict_action(ids, unnorm_key=None, num_beams=2, num_return_sequences=3)
    with pytest.raises(ValueError):
        model.generate_actions(image=None, prompt_text="x", type="act", num_beams=12)
    # not built: beam sampling, processors on beam log-probabilities, scores with beams
    for kw in (dict(do_sample=True), dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=3),
               dict(output_scores=True, return_dict_in_generate=True)):
        with pytest.raises(NotImplementedError):
            model.generate(ids, num_beams=2, max_new_tokens=4, **kw)
    assert model._beam_args(None) is None and model._beam_args(1) is None
    assert model._beam_args(4, 2, 0.5, "never") == BeamParams(4, 0.5, "never", 2)
    # neutral processor values pass (the reference's callers always send min_length=1), and then the call reaches the engine
    with pytest.raises(AssertionError, match="engine was touched"):
        model.generate(ids, num_beams=2, max_new_tokens=4, min_length=1, repetition_penalty=1.0)


class _StubEngine:
    """Stands in for the engine behind generate_ids: K hypotheses per prompt, best first, of known lengths."""

    def __init__(self, K, T, lens):
        self.K, self.T, self.lens = K, T, lens

    def beam_result(self):
        G = len(self.lens) // self.K
        sc = -torch.arange(G * self.K, dtype=torch.float32).reshape(G, self.K)
        bix = torch.full((G, self.K, self.T), -1, dtype=torch.int32)
        for r, n in enumerate(self.lens):
            bix[r // self.K, r % self.K, :n] = r
        return None, None, sc, bix


def test_generate_output_shapes_with_beams():
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction, EmmaXGenerateOutput
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    m = EmmaXForActionPrediction(cfg, synthetic_state_dict(cfg, seed=1))
    K, T = 4, 6
    lens = [3, 6, 2, 5, 4, 1, 6, 6]
    stub = _StubEngine(K, T, lens)
    m._need_engine = lambda: stub
    seen = {}

    def fake_generate_ids(rows, pixel_values=None, frames_u8=None, max_new_tokens=512, **kw):
        seen.update(kw)
        ids = torch.full((len(rows) * K, max_new_tokens), cfg.pad_token_id, dtype=torch.int32)
        for r, n in enumerate(lens):
            ids[r, :n] = 100 + r
        return ids, torch.tensor(lens, dtype=torch.int32)

    m.generate_ids = fake_generate_ids
    rows = torch.tensor([[1, 7, 8], [1, 9, 10]])
    out = m.generate(rows, max_new_tokens=T, num_beams=K, num_return_sequences=2, length_penalty=2.0, early_stopping=True)
    assert seen["beams"] == BeamParams(K, 2.0, True, 2)
    assert out.shape == (2 * 2, 3 + 6) and out.dtype == torch.long            # [B * num_return_sequences, P + T], T = the longest returned
    assert out[0].tolist() == [1, 7, 8, 100, 100, 100] + [cfg.pad_token_id] * 3
    assert out[1].tolist() == [1, 7, 8] + [101] * 6
    assert out[2].tolist() == [1, 9, 10, 104, 104, 104, 104] + [cfg.pad_token_id] * 2
    d = m.generate(rows, max_new_tokens=T, num_beams=K, num_return_sequences=K, return_dict_in_generate=True)
    assert isinstance(d, EmmaXGenerateOutput) and d.sequences.shape == (8, 9)
    assert d.sequences_scores.shape == (8,) and d.beam_indices.shape == (8, 6) and d.scores is None and d.logits is None
    assert d.beam_indices[2].tolist() == [2, 2, -1, -1, -1, -1]
    # K = 1 is not a beam run: generate_ids is called exactly as a greedy call spells it
    seen.clear()
    lens[:] = [3, 2]
    K1 = m.generate
    K = 1
    K1(rows, max_new_tokens=T, num_beams=1)
    assert "beams" not in seen


def test_serving_and_dist_refuse_beams():
    from emmax import dist as edist
    from emmax.serving import Request, SlotScheduler

    req = Request(rid=0, frame=None, prompt_ids=[1, 2], beams=BeamParams(2))
    with pytest.raises(NotImplementedError, match="beam"):
        SlotScheduler.submit(object.__new__(SlotScheduler), req)
    with pytest.raises(NotImplementedError, match="beam"):
        edist.generate_actions_dp(None, torch.zeros(1, 4, 4, 3, dtype=torch.uint8), [[1, 2]], beams=BeamParams(2))
