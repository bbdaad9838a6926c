"""
actions.py -- 7-DoF action <-> token-id mapping on the last 256 vocabulary ids, and un-normalisation.

Behavioural mirror of `ActionTokenizer` (prismatic/vla/action_tokenizer.py:13-72) and of the tail of
`OpenVLAForActionPrediction.predict_action` (prismatic/extern/hf/modeling_prismatic.py:522-535).  Host-side integer and
fp64 numpy math; bit-exact against the reference (tests/golden/action_decode.npz).
"""

from __future__ import annotations

from typing import Any, Dict, List, Sequence, Union

import numpy as np


class ActionTokenizer:
    """Uniform `bins`-level discretiser that re-uses the `bins` least-used (= last) token ids of the base tokenizer."""

    def __init__(self, tokenizer, bins: int = 256, min_action: int = -1, max_action: int = 1) -> None:
        self.tokenizer, self.n_bins = tokenizer, bins
        self.min_action, self.max_action = min_action, max_action
        edges = np.linspace(min_action, max_action, bins)
        self.bins = edges
        self.bin_centers = (edges[:-1] + edges[1:]) / 2.0
        self.action_token_begin_idx: int = int(tokenizer.vocab_size - (bins + 1))

    # continuous -> text (what the training data contains)
    def __call__(self, action: np.ndarray) -> Union[str, List[str]]:
        ids = self.encode_ids(action)
        if ids.ndim == 1:
            return self.tokenizer.decode(list(ids))
        return self.tokenizer.batch_decode(ids.tolist())

    def encode_ids(self, action: np.ndarray) -> np.ndarray:
        """continuous -> token ids (no text round trip)."""
        clipped = np.clip(action, a_min=float(self.min_action), a_max=float(self.max_action))
        return self.tokenizer.vocab_size - np.digitize(clipped, self.bins)

    # token ids -> bin centres
    def decode_token_ids_to_actions(self, action_token_ids: np.ndarray) -> np.ndarray:
        return token_ids_to_actions(action_token_ids, self.tokenizer.vocab_size, self.bin_centers)

    @property
    def vocab_size(self) -> int:
        return self.n_bins


def token_ids_to_actions(ids: np.ndarray, vocab_size: int, centers: np.ndarray) -> np.ndarray:
    """id -> bin index (vocab_size - id - 1, clamped to the valid centre range) -> centre value."""
    idx = np.clip(vocab_size - np.asarray(ids) - 1, a_min=0, a_max=centers.shape[0] - 1)
    return centers[idx]


def _flat_ids(x) -> np.ndarray:
    """a [B, S] tensor / array, or a list of per-row tensors / arrays / lists -> one flat int64 array"""
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy().reshape(-1).astype(np.int64)
    if isinstance(x, np.ndarray):
        return x.reshape(-1).astype(np.int64)
    parts = [_flat_ids(r) if hasattr(r, "__len__") or hasattr(r, "detach") else np.array([r], dtype=np.int64) for r in x]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def action_token_metrics(predicted_ids, targets, config) -> Dict[str, float]:
    """The action metrics of the reference's training / validation step (prismatic/training/strategies/base_strategy.py:392-416), from
    teacher-forced predictions: predicted_ids and targets are aligned row for row (what `score(...).predicted_ids` and `scoring.targets_for`
    return -- the shift and the patch splice are already in them; [B, S] or per-row lists).  mask = target > action_token_begin_idx (the ids
    of the action bins); action_accuracy = (prediction == target) over the mask; l1_loss = mean |centre(prediction) - centre(target)| over
    the mask, de-tokenised as ActionTokenizer.decode_token_ids_to_actions.  NaN where the mask is empty, as the reference's 0 / 0."""
    pred, gt = _flat_ids(predicted_ids), _flat_ids(targets)
    if pred.shape != gt.shape:
        raise ValueError(f"{pred.shape[0]} predictions for {gt.shape[0]} targets: the two are aligned row for row")
    vocab, bins = int(config.action_vocab_size), int(config.n_action_bins)
    edges = np.linspace(-1, 1, bins)
    centers = (edges[:-1] + edges[1:]) / 2.0
    mask = gt > vocab - (bins + 1)
    n = int(mask.sum())
    if n == 0:
        return dict(action_accuracy=float("nan"), l1_loss=float("nan"), n_action_tokens=0)
    acc = float(((pred == gt) & mask).sum()) / n
    l1 = float(np.abs(token_ids_to_actions(pred[mask], vocab, centers) - token_ids_to_actions(gt[mask], vocab, centers)).mean())
    return dict(action_accuracy=acc, l1_loss=l1, n_action_tokens=n)


def action_bin_token_ids(vocab_size: int, n_bins: int = 256) -> List[int]:
    """The token id of every action bin, in bin order: bin k is id vocab_size - 1 - k (the inverse of token_ids_to_actions' index)."""
    return [int(vocab_size) - 1 - k for k in range(int(n_bins))]


def unnormalize(normalized: np.ndarray, stats: Dict[str, Any], lo_key: str = "q01", hi_key: str = "q99") -> np.ndarray:
    """Map [-1,1] back to the dataset range on masked dimensions (gripper dimension passes through)."""
    lo, hi = np.array(stats[lo_key]), np.array(stats[hi_key])
    mask = stats.get("mask", np.ones_like(stats[lo_key], dtype=bool))
    return np.where(mask, 0.5 * (np.asarray(normalized) + 1) * (hi - lo) + lo, normalized)
