"""
scoring.py -- the host side of a teacher-forced scoring pass: which id every logit row is scored against.

`forward(labels=...)` of the reference hands `labels` to HF's LlamaForCausalLM, which shifts them (row t is scored against the label of position
t + 1) and takes the mean cross-entropy over the labels that are not -100; the multimodal branch first splices the labels the way it splices the
embeddings, `[labels[:1], -100 x n_patches, labels[1:]]` (prismatic/extern/hf/modeling_prismatic.py:393-401).  The engine scores packed rows
against one target id per row (include/emmax.h: emmax_prefill_score); this module is the one place that knows the alignment.  Host only: lists of
ints in, lists of ints out.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

IGNORE_INDEX = -100


def _label_rows(labels, lens: Sequence[int], attention_mask=None) -> List[List[int]]:
    """labels ([B, P] tensor / array / nested lists, padded like the ids, or ragged lists) -> per row the first lens[b] labels"""
    if hasattr(labels, "detach"):
        labels = labels.detach().to("cpu")
    if hasattr(labels, "tolist"):
        labels = labels.tolist()
    labels = list(labels)
    if labels and not isinstance(labels[0], (list, tuple)):
        labels = [labels]
    if len(labels) != len(lens):
        raise ValueError(f"labels hold {len(labels)} rows, input_ids {len(lens)}")
    out = []
    for b, (lab, n) in enumerate(zip(labels, lens)):
        lab = [int(x) for x in lab]
        if len(lab) < n or (attention_mask is None and len(lab) != n):
            raise ValueError(f"row {b}: {len(lab)} labels for {n} input ids (labels are aligned with input_ids)")
        out.append(lab[:n])   # right padding: the positions behind the row's length are not rows of the pass
    return out


def targets_for(labels, rows: Sequence[Sequence[int]], attention_mask=None, n_patches: int = 0, new_rows_only: bool = False,
                vocab: Optional[int] = None) -> List[List[int]]:
    """The target id of every logit row of a pass over `rows` (per-row id lists, padding already cut), -100 where nothing is scored.

    labels: aligned with the input ids ([B, P] with the ids' right padding, or ragged rows); -100 = ignored; None = the ids themselves (perplexity).
    n_patches > 0 (a multimodal pass): the labels are spliced first, [labels[:1], -100 x n_patches, labels[1:]], so row 0 (BOS) and the patch rows
    but the last get -100 and the last patch row is scored against labels[1].
    new_rows_only (an extension of a cached context): the rows are the NEW ids alone and the labels cover them alone; row i is scored against new
    label i + 1.  The first new id is never a target: the row that predicts it belongs to the earlier pass.
    HF's shift: row t is scored against the label of position t + 1; the last row gets -100.
    vocab: a label outside [0, vocab) other than -100 raises ValueError."""
    lens = [len(r) for r in rows]
    lab = [list(map(int, r)) for r in rows] if labels is None else _label_rows(labels, lens, attention_mask)
    if new_rows_only:
        n_patches = 0
    out = []
    for b, l in enumerate(lab):
        if vocab is not None:
            for x in l:
                if x != IGNORE_INDEX and not 0 <= x < vocab:
                    raise ValueError(f"row {b}: label {x} outside [0, vocab = {vocab}) (and not {IGNORE_INDEX})")
        if n_patches:
            l = l[:1] + [IGNORE_INDEX] * n_patches + l[1:]
        out.append(l[1:] + [IGNORE_INDEX])
    return out


@dataclass
class EmmaXScoreOutput:
    """score(...): loss fp32 0-dim device tensor (mean of -log p over the scored rows; NaN when nothing is scored); token_logprobs / predicted_ids /
    lse aligned with the logit rows -- [B, S] when the rows have equal length, else a list per row -- token_logprobs[b][t] = log p(target of row t),
    NaN where nothing was scored, predicted_ids[b][t] = what logits[b][t].argmax() would be; n_scored: the scored rows (host int)."""
    loss: Any = None
    token_logprobs: Any = None
    predicted_ids: Any = None
    lse: Any = None
    n_scored: int = 0
    past_key_values: Optional[Any] = None
