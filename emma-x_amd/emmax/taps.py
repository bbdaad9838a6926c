"""
taps.py -- the host side of output_hidden_states / output_attentions (include/emmax.h: emmax_session_set_pass_taps / _set_step_taps): which
layers a call selects, the buffers the session fills, and HF's structures cut out of them.  Plain Python and torch; nothing here launches.

`tap_layers`: HF indices into the tuples a full call returns -- hidden_states has n_layers + 1 entries (0 = the embeddings / patch rows, i = behind
layer i, n_layers = the last layer NORMED), attentions has n_layers -- negative allowed, duplicates count once, None = all (HF's meaning).  The
returned tuples hold the selected entries only, in ascending order.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch


def select_layers(tap_layers, n_entries: int, what: str) -> List[int]:
    """`tap_layers` against a tuple of n_entries entries -> ascending indices, each once"""
    if tap_layers is None:
        return list(range(n_entries))
    if isinstance(tap_layers, (int, bool)) or not isinstance(tap_layers, (list, tuple)) or len(tap_layers) == 0:
        raise ValueError(f"tap_layers must be a non-empty list of layer indices or None (all), got {tap_layers!r}")
    out = set()
    for i in tap_layers:
        if isinstance(i, bool) or not isinstance(i, int):
            raise ValueError(f"tap_layers holds integers, got {i!r}")
        if not -n_entries <= i < n_entries:
            raise ValueError(f"tap_layers index {i} is outside the {n_entries} entries of {what} (-{n_entries} .. {n_entries - 1})")
        out.add(i % n_entries)
    return sorted(out)


def layer_mask(indices: Sequence[int]) -> int:
    m = 0
    for i in indices:
        m |= 1 << int(i)
    return m


@dataclass
class TapSpec:
    """what a call selects: indices into hidden_states (0 .. n_layers) and attentions (0 .. n_layers - 1); an empty list = not asked for"""
    hidden: List[int]
    attn: List[int]

    @property
    def any(self) -> bool:
        return bool(self.hidden or self.attn)


def tap_spec(n_layers: int, output_hidden_states, output_attentions, tap_layers=None) -> Optional[TapSpec]:
    """None when neither output is asked for (tap_layers alone selects nothing and is checked all the same)"""
    hid = select_layers(tap_layers, n_layers + 1, "hidden_states") if output_hidden_states else []
    att = select_layers(tap_layers, n_layers, "attentions") if output_attentions else []
    if not output_hidden_states and not output_attentions:
        if tap_layers is not None:
            select_layers(tap_layers, n_layers + 1, "hidden_states")
        return None
    return TapSpec(hid, att)


def round_keys(n: int) -> int:
    """ld_keys for rows that see up to n keys: the kernel's stores are 16 bytes"""
    return max(4, (int(n) + 3) // 4 * 4)


def pass_shapes(spec: TapSpec, total_rows: int, H: int, Hq: int, ld_keys: int) -> Tuple[Optional[tuple], Optional[tuple]]:
    """shapes of the pass taps' buffers: hidden [n_sel, total_rows, H], attentions [n_sel, total_rows, Hq, ld_keys]"""
    return ((len(spec.hidden), total_rows, H) if spec.hidden else None, (len(spec.attn), total_rows, Hq, ld_keys) if spec.attn else None)


def step_shapes(spec: TapSpec, max_new: int, B: int, H: int, Hq: int, ld_keys: int) -> Tuple[Optional[tuple], Optional[tuple]]:
    """shapes of the step taps' buffers: hidden [max_new, n_sel, B, H], attentions [max_new, n_sel, B, Hq, ld_keys]"""
    return ((max_new, len(spec.hidden), B, H) if spec.hidden else None, (max_new, len(spec.attn), B, Hq, ld_keys) if spec.attn else None)


def stacked_or_list(per_row: List[torch.Tensor]):
    """the rule `logits` follows: one stacked tensor when the rows have one shape, else the list"""
    return torch.stack(per_row) if len({tuple(t.shape) for t in per_row}) == 1 else per_row


def cut_pass(hidden: Optional[torch.Tensor], attn: Optional[torch.Tensor], n_new: Sequence[int], keys: Sequence[int]):
    """The pass taps' buffers as HF's structures.  n_new[b]: packed rows of sequence b; keys[b]: the keys its last row sees (base + n).
    -> (hidden_states: tuple over the selected entries of [B, n, H] (or a list per row), attentions: tuple of [B, Hq, n, L] (or a list))"""
    cu = [0]
    for n in n_new:
        cu.append(cu[-1] + int(n))
    hs = at = None
    if hidden is not None:
        hs = tuple(stacked_or_list([hidden[i, cu[b]:cu[b + 1]] for b in range(len(n_new))]) for i in range(hidden.shape[0]))
    if attn is not None:
        at = tuple(stacked_or_list([attn[i, cu[b]:cu[b + 1], :, : int(keys[b])].permute(1, 0, 2) for b in range(len(n_new))]) for i in range(attn.shape[0]))
    return hs, at


def cut_step(hidden: Optional[torch.Tensor], attn: Optional[torch.Tensor], t: int, keys: Sequence[int]):
    """Slot t of the step taps' buffers: hidden_states tuple of [B, 1, H], attentions tuple of [B, Hq, 1, keys[b]] (a list per row when they differ)"""
    hs = at = None
    if hidden is not None:
        hs = tuple(hidden[t, i][:, None, :] for i in range(hidden.shape[1]))
    if attn is not None:
        at = tuple(stacked_or_list([attn[t, i, b, :, None, : int(keys[b])] for b in range(attn.shape[2])]) for i in range(attn.shape[1]))
    return hs, at

