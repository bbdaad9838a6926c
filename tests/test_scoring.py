"""CPU: the host side of scoring -- the label alignment (emmax/scoring.py: targets_for) against HF's own `loss` (tests/golden/llama_loss.npz,
written by tools/make_llama_loss.py), the multimodal splice, the extension alignment, the refusals, and the action metrics against a numpy
restatement of prismatic/training/strategies/base_strategy.py:392-416."""

import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from emmax.actions import ActionTokenizer, action_token_metrics
from emmax.config import EmmaXConfig
from emmax.scoring import IGNORE_INDEX, targets_for


def loss64(logit_rows, targets):
    """float64: mean of -(logit[target] - lse) over the targets that are not -100; NaN over nothing (HF's mean)"""
    tot, n = 0.0, 0
    for z, tg in zip(logit_rows, targets):
        z = torch.as_tensor(z).double()
        lse = torch.logsumexp(z, dim=-1)
        for r, t in enumerate(tg):
            if t != IGNORE_INDEX:
                tot -= (z[r, t] - lse[r]).item()
                n += 1
    return tot / n if n else math.nan


@pytest.mark.parametrize("name", ["mha", "gqa"])
def test_targets_reproduce_hf_loss(name):
    g = np.load(os.path.join(GOLDEN, f"llama_{name}.npz"))
    f = np.load(os.path.join(GOLDEN, "llama_loss.npz"))
    logits, vocab = g["prefill_logits"], int(g["cfg"][6])
    rows = [list(range(logits.shape[0]))]   # (only the lengths matter)
    labels, want = f[f"{name}__labels"], f[f"{name}__loss"]
    assert labels.shape == (4, 9) and (labels[0] != -100).all() and (labels[3] == -100).all()
    assert 0 < (labels[1] != -100).sum() < 9 and (labels[2] != -100).tolist() == [False] * 8 + [True]
    for p in range(4):
        tg = targets_for(labels[p][None], rows, vocab=vocab)
        got = loss64([logits], tg)
        if p == 3:
            assert math.isnan(got) and math.isnan(want[p])
        else:
            assert abs(got - want[p]) <= 1e-6 * abs(want[p]), (p, got, want[p])
    # the right-padded batch of two rows: the short row is the long one's prefix (causal: its logits are the long row's first rows)
    lab, mask = f[f"{name}__batch_labels"], f[f"{name}__batch_mask"]
    lens = mask.sum(-1).tolist()
    assert lens == [9, 6]
    tg = targets_for(torch.from_numpy(lab), [list(range(n)) for n in lens], attention_mask=torch.from_numpy(mask), vocab=vocab)
    assert [len(t) for t in tg] == lens
    got = loss64([logits, logits[: lens[1]]], tg)
    assert abs(got - float(f[f"{name}__batch_loss"])) <= 1e-6 * abs(float(f[f"{name}__batch_loss"])), (got, f[f"{name}__batch_loss"])


def test_shift_and_ignored_positions():
    assert targets_for([[5, 6, 7, 8]], [[1, 2, 3, 4]]) == [[6, 7, 8, -100]]
    assert targets_for([[5, -100, 7, -100]], [[1, 2, 3, 4]]) == [[-100, 7, -100, -100]]
    assert targets_for(None, [[1, 2, 3], [4, 5]]) == [[2, 3, -100], [5, -100]]                       # labels = the ids: perplexity
    assert targets_for([[9]], [[1]]) == [[-100]]
    # right padding: what lies behind a row's length is no row of the pass
    lab = torch.tensor([[5, 6, 7, 8], [9, 10, -100, -100]])
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]])
    assert targets_for(lab, [[1, 2, 3, 4], [1, 2]], attention_mask=mask) == [[6, 7, 8, -100], [10, -100]]
    with pytest.raises(ValueError, match="labels"):
        targets_for([[5, 6, 7]], [[1, 2, 3, 4]])
    with pytest.raises(ValueError, match="rows"):
        targets_for([[5, 6, 7, 8]], [[1, 2, 3, 4], [1, 2]])


def test_multimodal_splice_ignores_exactly_the_patch_rows_behind_row_0():
    np_ = 7
    lab = [11, 12, 13, 14]
    (tg,) = targets_for([lab], [[1, 2, 3, 4]], n_patches=np_)
    assert len(tg) == np_ + 4
    # the spliced labels are [11, -100 x 7, 12, 13, 14]; shifted by one: rows 0 .. 6 ignored, row 7 (the last patch row) predicts 12
    assert tg == [-100] * np_ + [12, 13, 14, -100]
    spliced = lab[:1] + [-100] * np_ + lab[1:]
    assert [i for i, x in enumerate(spliced) if x == -100] == list(range(1, np_ + 1))                # exactly n_patches rows behind row 0
    assert tg == spliced[1:] + [-100]


def test_extension_alignment():
    # the new ids alone: row i is scored against new label i + 1, the first new id is never a target, whatever n_patches says
    assert targets_for([[21, 22, 23]], [[1, 2, 3]], n_patches=7, new_rows_only=True) == [[22, 23, -100]]
    assert targets_for(None, [[1, 2, 3], [4, 5]], new_rows_only=True) == [[2, 3, -100], [5, -100]]


def test_label_outside_the_vocabulary_is_refused():
    with pytest.raises(ValueError, match="outside"):
        targets_for([[5, 100, 7]], [[1, 2, 3]], vocab=100)
    with pytest.raises(ValueError, match="outside"):
        targets_for([[5, -1, 7]], [[1, 2, 3]], vocab=100)
    assert targets_for([[5, 99, -100]], [[1, 2, 3]], vocab=100) == [[99, -100, -100]]


def test_forward_refuses_before_the_engine_is_touched():
    from emmax.modeling import EmmaXForActionPrediction, KVHandle

    cfg = EmmaXConfig.tiny()
    m = EmmaXForActionPrediction(cfg, None)   # no engine: reaching for it raises something else
    with pytest.raises(ValueError, match="outside"):
        m.forward(input_ids=torch.tensor([[1, 5, 6]]), labels=torch.tensor([[1, 5, cfg.llm.vocab_size]]))
    with pytest.raises(ValueError, match="outside"):
        m.score(input_ids=torch.tensor([[1, 5, 6]]), labels=torch.tensor([[1, 5, cfg.llm.vocab_size]]))
    with pytest.raises(AssertionError, match="labels"):
        m.forward(input_ids=torch.tensor([[5]]), labels=torch.tensor([[5]]), past_key_values=KVHandle(None, [4]))
    with pytest.raises(ValueError, match="n > 1"):
        m.score(input_ids=torch.tensor([[5]]), past_key_values=KVHandle(None, [4]))


class _Tok:
    vocab_size = 32000


def test_action_token_metrics_against_the_reference_formula():
    cfg = EmmaXConfig.tiny()
    at = ActionTokenizer(_Tok(), bins=cfg.n_action_bins)
    assert cfg.action_vocab_size == _Tok.vocab_size and at.action_token_begin_idx == cfg.action_vocab_size - (cfg.n_action_bins + 1)
    rng = np.random.default_rng(3)
    b = at.action_token_begin_idx
    gt = rng.integers(b - 3, cfg.action_vocab_size, size=(3, 40))          # ids around the first action id: both sides of the mask
    gt[:, ::5] = -100
    gt[0, :3] = [b - 1, b, b + 1]
    pred = np.where(rng.random(gt.shape) < 0.5, gt, rng.integers(b - 3, cfg.action_vocab_size, size=gt.shape))
    mask = gt > b
    acc = ((pred == gt) & mask).sum() / mask.sum()
    l1 = np.abs(at.decode_token_ids_to_actions(pred[mask]) - at.decode_token_ids_to_actions(gt[mask])).mean()
    m = action_token_metrics(pred, gt, cfg)
    assert m["n_action_tokens"] == int(mask.sum()) and 0 < m["action_accuracy"] < 1 and m["l1_loss"] > 0
    assert m["action_accuracy"] == pytest.approx(acc, rel=0, abs=1e-15) and m["l1_loss"] == pytest.approx(l1, rel=1e-14)
    # per-row lists and tensors give the same numbers
    m2 = action_token_metrics([torch.from_numpy(r) for r in pred], [r.tolist() for r in gt], cfg)
    assert m2 == m
    none = action_token_metrics(np.array([5, 6]), np.array([-100, 7]), cfg)
    assert none["n_action_tokens"] == 0 and math.isnan(none["action_accuracy"]) and math.isnan(none["l1_loss"])
    with pytest.raises(ValueError):
        action_token_metrics(np.array([5, 6]), np.array([7]), cfg)


def test_the_decode_is_the_goldens():
    a = np.load(os.path.join(GOLDEN, "action_decode.npz"))
    cfg = EmmaXConfig.tiny()
    ids = a["ids"].astype(np.int64)
    at = ActionTokenizer(_Tok(), bins=cfg.n_action_bins)
    assert np.array_equal(at.decode_token_ids_to_actions(ids), a["actions"])
    # predictions one bin off the golden ids: the L1 is the mean distance of neighbouring centres, the accuracy 0
    inside = ids[(ids > at.action_token_begin_idx + 1) & (ids < cfg.action_vocab_size - 1)]
    assert inside.size > 10
    m = action_token_metrics(inside - 1, inside, cfg)
    want = np.abs(at.decode_token_ids_to_actions(inside - 1) - at.decode_token_ids_to_actions(inside)).mean()
    assert m["action_accuracy"] == 0.0 and m["l1_loss"] == pytest.approx(want, rel=1e-14) and m["n_action_tokens"] == inside.size
