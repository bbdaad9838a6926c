"""CPU: what a draft is refused with at the model level (emmax/modeling.py: _check_draft, generate's mapping of its arguments onto it,
predict_action / generate_actions) -- each raises NotImplementedError in one line BEFORE the engine is touched, so a model that was never moved to a
device (it has no engine: touching one would raise another error) pins them.  The session-level refusals of emmax_verify and what the session
does afterwards are tests/test_verify_session_gpu.py's."""
import pytest
import torch

from emmax.config import EmmaXConfig
from emmax.constraints import action_bins
from emmax.modeling import EmmaXForActionPrediction
from emmax.sampling import BeamParams, LogitsProcessing, SamplingParams
from emmax.weights import synthetic_state_dict

ROWS = [[1, 5, 6, 7]]
DRAFT = [[8, 9, 10]]


@pytest.fixture(scope="module")
def model():
    cfg = EmmaXConfig.tiny()
    m = EmmaXForActionPrediction(cfg, synthetic_state_dict(cfg, seed=5, planted=True))
    assert m.engine is None
    return m


def _frames():
    return torch.zeros(1, 224, 224, 3, dtype=torch.uint8)


def _aut(m):
    return action_bins(m.config.llm.vocab_size, m.config.n_action_bins, 7, token_vocab=m.vocab_size)


GENERATE_IDS_CASES = {
    "sampling": (lambda m: dict(sampling=SamplingParams(temperature=1.0, top_k=0, top_p=1.0, seed=1)), "do_sample / sampling"),
    "return_logprobs": (lambda m: dict(return_logprobs=True), "do_sample / sampling"),
    "processing": (lambda m: dict(processing=LogitsProcessing(repetition_penalty=1.3)), "logits processors"),
    "constraint": (lambda m: dict(constraint=_aut(m)), "a constraint"),
    "beams": (lambda m: dict(beams=BeamParams(num_beams=2)), "num_beams > 1"),
    "num_samples": (lambda m: dict(num_samples=2), "num_return_sequences > 1"),
    "scores": (lambda m: dict(scores=torch.empty(8, 1, m.config.llm.vocab_size)), "output_scores"),
    "logits": (lambda m: dict(logits=torch.empty(8, 1, m.config.llm.vocab_size)), "output_scores"),
    "top_logprobs": (lambda m: dict(top_logprobs=2), "top_logprobs"),
    "watch_ids": (lambda m: dict(watch_ids=[5]), "top_logprobs"),
    "hidden": (lambda m: dict(hidden=[0]), "output_hidden_states"),
    "attentions": (lambda m: dict(attentions=[0]), "output_hidden_states"),
}


@pytest.mark.parametrize("name", sorted(GENERATE_IDS_CASES))
def test_generate_ids_refuses_a_draft_with(model, name):
    make, msg = GENERATE_IDS_CASES[name]
    with pytest.raises(NotImplementedError, match=msg) as e:
        model.generate_ids(ROWS, frames_u8=_frames(), max_new_tokens=8, draft=DRAFT, **make(model))
    assert "draft" in str(e.value) and "\n" not in str(e.value)


def test_generate_ids_refuses_a_draft_on_fp8_decode_weights():
    cfg = EmmaXConfig.tiny()
    cfg.decode_weight_dtype = "fp8"
    m = EmmaXForActionPrediction(cfg, synthetic_state_dict(cfg, seed=5, planted=True))
    with pytest.raises(NotImplementedError, match="fp8 decode weights"):
        m.generate_ids(ROWS, frames_u8=_frames(), max_new_tokens=8, draft=DRAFT)


def test_generate_ids_checks_the_drafts_shape(model):
    for bad in ([[1], [2]], "abc", 5):
        with pytest.raises(ValueError, match="one list of ids or None per row"):
            model.generate_ids(ROWS, frames_u8=_frames(), max_new_tokens=8, draft=bad)


GENERATE_CASES = {
    "do_sample": (dict(do_sample=True), "do_sample / sampling"),
    "num_beams": (dict(num_beams=2), "num_beams > 1"),
    "num_return_sequences": (dict(num_return_sequences=2, do_sample=True), "do_sample / sampling|num_return_sequences"),
    "repetition_penalty": (dict(repetition_penalty=1.2), "logits processors"),
    "no_repeat_ngram_size": (dict(no_repeat_ngram_size=2), "logits processors"),
    "min_new_tokens": (dict(min_new_tokens=3), "logits processors"),
    "bad_words_ids": (dict(bad_words_ids=[[5]]), "logits processors"),
    "suppress_tokens": (dict(suppress_tokens=[5]), "logits processors"),
    "output_scores": (dict(output_scores=True, return_dict_in_generate=True), "output_scores"),
    "output_logits": (dict(output_logits=True, return_dict_in_generate=True), "output_scores"),
    "top_logprobs": (dict(top_logprobs=2, return_dict_in_generate=True), "top_logprobs"),
    "watch_ids": (dict(watch_ids=[5], return_dict_in_generate=True), "top_logprobs"),
    "output_hidden_states": (dict(output_hidden_states=True, return_dict_in_generate=True), "output_hidden_states"),
    "output_attentions": (dict(output_attentions=True, return_dict_in_generate=True), "output_hidden_states"),
    "logits_processor": (dict(logits_processor=[object()]), "logits_processor"),
    "stopping_criteria": (dict(stopping_criteria=[object()]), "stopping_criteria"),
    "prefix_allowed_tokens_fn": (dict(prefix_allowed_tokens_fn=lambda b, ids: [1]), "prefix_allowed_tokens_fn"),
}


@pytest.mark.parametrize("how", ["draft_ids", "prompt_lookup_num_tokens"])
@pytest.mark.parametrize("name", sorted(GENERATE_CASES))
def test_generate_refuses_a_draft_with(model, name, how):
    kw, msg = GENERATE_CASES[name]
    draft = dict(draft_ids=DRAFT) if how == "draft_ids" else dict(prompt_lookup_num_tokens=4)
    with pytest.raises(NotImplementedError, match=msg) as e:
        model.generate(torch.tensor(ROWS), frames_u8=_frames(), max_new_tokens=8, **draft, **kw)
    assert "draft" in str(e.value)


def test_generate_refuses_a_constraint_with_a_draft(model):
    with pytest.raises(NotImplementedError, match="a constraint"):
        model.generate(torch.tensor(ROWS), frames_u8=_frames(), max_new_tokens=8, draft_ids=DRAFT, constraint=_aut(model))


def test_generate_takes_one_kind_of_draft(model):
    with pytest.raises(ValueError, match="one of"):
        model.generate(torch.tensor(ROWS), frames_u8=_frames(), max_new_tokens=8, draft_ids=DRAFT, prompt_lookup_num_tokens=4)


def test_predict_action_refuses_a_draft_with(model):
    common = dict(frames_u8=_frames(), unnorm_key="bridge_orig", draft_ids=[5, 6, 7])
    for kw, msg in ((dict(constrain_to_bins=True), "a constraint"), (dict(do_sample=True), "do_sample / sampling"), (dict(num_beams=2), "num_beams > 1"),
                    (dict(return_bin_logprobs=True), "top_logprobs"), (dict(return_hidden_states=True), "output_hidden_states"),
                    (dict(repetition_penalty=1.2), "logits processors")):
        with pytest.raises(NotImplementedError, match=msg) as e:
            model.predict_action(torch.tensor(ROWS), **common, **kw)
        assert "draft" in str(e.value), kw


def test_without_a_draft_the_model_asks_for_its_engine(model):
    """the same calls without a draft get past every draft check: the first thing they miss is the engine"""
    with pytest.raises(Exception) as e:
        model.generate_ids(ROWS, frames_u8=_frames(), max_new_tokens=8)
    assert not isinstance(e.value, NotImplementedError)
