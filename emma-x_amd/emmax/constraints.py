"""
constraints.py -- constrained decoding: token automata for the decode step (include/emmax.h: emmax_session_set_automaton).

A TokenAutomaton is what HF's `prefix_allowed_tokens_fn` would compute, compiled ahead of time so that it can run inside a captured step:

    cls   uint8  [V]      the class of every token id (ids that behave alike in every state share a class; at most 256 classes)
    allow uint32 [S, 8]   bit c of row s: class c is allowed in state s (at most 1024 states)
    next  int16  [S, C]   the state after a token of class c in state s; -1 (DONE): the row is done after this token

A row enters at a start state (`entry` names some) or is unconstrained (start -1).  `walk` is the host replay of what the step does.

Builders: from_transitions (a table of transitions; classes by partition refinement), build (segments in a row: Literal, AnyOf, FreeUntil,
OneOf), action_bins and policy_line (the two shapes this model needs).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Hashable, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .actions import action_bin_token_ids

MAX_STATES = 1024    # include/emmax.h: EMMAX_MAX_AUT_STATES
MAX_CLASSES = 256    # EMMAX_MAX_AUT_CLASSES
DONE = -1            # a transition's target: the row is done after the token
ANY = None           # a transition's ids: every id of the vocabulary (later entries of the state override it)


class TokenAutomaton:
    """The three tables, validated, with the named start states `entry`."""

    def __init__(self, vocab: int, cls, allow, next, entry: Optional[Dict[str, int]] = None):
        self.vocab = int(vocab)
        self.cls = np.ascontiguousarray(cls, dtype=np.uint8)
        self.allow = np.ascontiguousarray(allow, dtype=np.uint32)
        self.next = np.ascontiguousarray(next, dtype=np.int16)
        self.entry = dict(entry or {})
        self.validate()

    @property
    def n_states(self) -> int:
        return int(self.allow.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.next.shape[1])

    def validate(self) -> None:
        V, S = self.vocab, self.allow.shape[0] if self.allow.ndim == 2 else -1
        if V < 1 or self.cls.shape != (V,):
            raise ValueError(f"TokenAutomaton: cls must be uint8 [{V}], got {self.cls.shape}")
        if self.allow.ndim != 2 or self.allow.shape[1] != 8 or self.next.ndim != 2 or self.next.shape[0] != S:
            raise ValueError(f"TokenAutomaton: allow must be uint32 [S, 8] and next int16 [S, C], got {self.allow.shape} and {self.next.shape}")
        C = self.next.shape[1]
        if not 1 <= S <= MAX_STATES:
            raise ValueError(f"TokenAutomaton: {S} states outside 1..{MAX_STATES}")
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f"TokenAutomaton: {C} classes outside 1..{MAX_CLASSES}")
        if int(self.cls.max()) >= C:
            raise ValueError(f"TokenAutomaton: class {int(self.cls.max())} of token {int(self.cls.argmax())} outside 0..{C - 1}")
        if int(self.next.min()) < -1 or int(self.next.max()) >= S:
            raise ValueError(f"TokenAutomaton: next states must lie in -1..{S - 1}")
        for name, s in self.entry.items():
            if not 0 <= int(s) < S:
                raise ValueError(f"TokenAutomaton: entry {name!r} = {s} outside 0..{S - 1}")

    def tables(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(cls, allow, next) as the C ABI takes them: contiguous uint8 [V], uint32 [S, 8], int16 [S, C]."""
        return self.cls, self.allow, self.next

    def start_state(self, start: Union[None, int, str]) -> int:
        """None -> -1 (unconstrained); a name -> entry[name]; an int is checked against the states."""
        if start is None:
            return -1
        if isinstance(start, str):
            if start not in self.entry:
                raise ValueError(f"constraint_start {start!r} is not one of the automaton's entries {sorted(self.entry)}")
            return int(self.entry[start])
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not -1 <= int(start) < self.n_states:
            raise ValueError(f"constraint_start {start!r} outside -1..{self.n_states - 1}")
        return int(start)

    def starts(self, start, rows: int) -> List[int]:
        """`constraint_start` of a call -> one start state per row: None with entries = the entry "start" (else state 0) for every row, a
        name / int = that for every row, a list = one per row (None in a list: that row is unconstrained)."""
        if isinstance(start, (list, tuple)):
            if len(start) != rows:
                raise ValueError(f"constraint_start has {len(start)} entries for {rows} rows")
            return [self.start_state(s) for s in start]
        if start is None:
            start = self.entry.get("start", 0)
        return [self.start_state(start)] * rows

    def class_allowed(self, state: int) -> np.ndarray:
        """bool [C]: the classes allowed in `state`."""
        c = np.arange(self.n_classes)
        return ((self.allow[state, c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)

    def allowed(self, state: int) -> np.ndarray:
        """bool [V]: the ids allowed in `state` (-1: all of them; a state the table does not have: none)."""
        if state == -1:
            return np.ones(self.vocab, dtype=bool)
        if not 0 <= state < self.n_states:
            return np.zeros(self.vocab, dtype=bool)
        return self.class_allowed(state)[self.cls]

    def step(self, state: int, tok: int) -> int:
        """The state after `tok` in `state` (what the step's one thread computes); raises on a token the state forbids."""
        if state == -1:
            return -1
        if not 0 <= tok < self.vocab or not self.allowed(state)[tok]:
            raise ValueError(f"token {tok} is not allowed in state {state}")
        return int(self.next[state, self.cls[tok]])

    def walk(self, ids: Iterable[int], start: Union[None, int, str] = 0) -> List[int]:
        """Host replay: the state after each of `ids`, entering at `start`.  Raises ValueError on a token the automaton forbids, and on a
        token behind the one that ended the row."""
        s = self.start_state(start)
        unconstrained = s == -1
        out = []
        for n, t in enumerate(ids):
            if s == -1 and not unconstrained:
                raise ValueError(f"token {int(t)} at index {n} follows the token that ended the row")
            s = self.step(s, int(t))
            out.append(s)
        return out


# ---- from a transition table -----------------------------------------------------------------------------------------------
def from_transitions(vocab: int, transitions: Dict[Hashable, Sequence[Tuple[Optional[Iterable[int]], Hashable]]],
                     entry: Optional[Dict[str, Hashable]] = None) -> TokenAutomaton:
    """{state: [(ids, next_state), ...]}: in `state` the listed ids are allowed and lead to `next_state` (DONE / -1: the row is done after the
    token); ids = ANY / None names every id, and a later entry of a state overrides an earlier one.  States are numbered in the order of the
    dict.  Ids with identical columns (the same fate in every state) share a class: partition refinement, classes numbered by their lowest id."""
    V = int(vocab)
    if V < 1:
        raise ValueError(f"vocab {vocab} < 1")
    names = list(transitions)
    S = len(names)
    if not 1 <= S <= MAX_STATES:
        raise ValueError(f"{S} states outside 1..{MAX_STATES}")
    index = {n: i for i, n in enumerate(names)}

    def target(t):
        if t is None or (isinstance(t, (int, np.integer)) and not isinstance(t, bool) and int(t) == DONE and DONE not in index):
            return DONE
        if t not in index:
            raise ValueError(f"transition to {t!r}, which is not a state")
        return index[t]

    FORBID = -2
    # the classes so far, and the fate (next state, DONE or FORBID) of every class in the states seen so far: [states seen, classes] int16 -- a
    # state's row over the vocabulary lives only until it has refined the classes
    cls = np.zeros(V, dtype=np.int64)
    fate = np.zeros((0, 1), dtype=np.int16)
    row = np.empty(V, dtype=np.int16)
    for name in names:
        row[:] = FORBID
        for ids, nxt in transitions[name]:
            t = target(nxt)
            if ids is ANY:
                row[:] = t
                continue
            a = np.asarray(list(ids), dtype=np.int64)
            if a.size and (a.min() < 0 or a.max() >= V):
                raise ValueError(f"state {name!r}: token id outside 0..{V - 1}")
            row[a] = t
        # refine: ids of one class that differ in this state part ways
        _, new = np.unique(cls * (S + 2) + (row.astype(np.int64) + 2), return_inverse=True)
        n_cls = int(new.max()) + 1
        if n_cls > MAX_CLASSES:
            raise ValueError(f"{n_cls} token classes after state {name!r}: more than {MAX_CLASSES}")
        old_of_new = np.empty(n_cls, dtype=np.int64)
        old_of_new[new] = cls          # (every new class lies inside one old class)
        here = np.empty(n_cls, dtype=np.int16)
        here[new] = row                # (... and has one fate in this state)
        fate = np.vstack([fate[:, old_of_new], here[None]])
        cls = new
    # number the classes by their lowest id
    first = np.full(n_cls, V, dtype=np.int64)
    np.minimum.at(first, cls, np.arange(V))
    order = np.argsort(first, kind="stable")
    rank = np.empty(n_cls, dtype=np.int64)
    rank[order] = np.arange(n_cls)
    cls = rank[cls]
    fate = fate[:, order]
    allow = np.zeros((S, 8), dtype=np.uint32)
    ok = fate != FORBID
    for c in range(n_cls):
        allow[:, c >> 5] |= np.where(ok[:, c], np.uint32(1 << (c & 31)), np.uint32(0)).astype(np.uint32)
    nxt = np.where(ok, fate, DONE).astype(np.int16)
    ent = {}
    for k, v in (entry or {}).items():
        if v not in index:
            raise ValueError(f"entry {k!r}: {v!r} is not a state")
        ent[k] = index[v]
    return TokenAutomaton(V, cls.astype(np.uint8), allow, nxt, ent)


# ---- from segments ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Literal:
    """exactly these ids, in order"""
    ids: Sequence[int]


@dataclass(frozen=True)
class AnyOf:
    """exactly n tokens from a set"""
    ids: Sequence[int]
    n: int = 1


@dataclass(frozen=True)
class FreeUntil:
    """anything until the id sequence has been emitted (a KMP automaton over the trigger: overlapping prefixes are followed)"""
    trigger: Sequence[int]


@dataclass(frozen=True)
class OneOf:
    """one of several whole id sequences (a trie); no alternative may be a prefix of another"""
    alternatives: Sequence[Sequence[int]]


def _kmp_delta(trig: List[int]) -> List[Dict[int, int]]:
    """delta[k][t]: trigger ids matched after token t with k matched before (tokens not listed: 0)"""
    m = len(trig)
    fail = [0] * (m + 1)
    k = 0
    for i in range(1, m):
        while k and trig[i] != trig[k]:
            k = fail[k]
        if trig[i] == trig[k]:
            k += 1
        fail[i + 1] = k
    delta: List[Dict[int, int]] = []
    for k in range(m):
        d = {}
        for t in set(trig):
            j = k
            while j and trig[j] != t:
                j = fail[j]
            d[t] = j + 1 if trig[j] == t else 0
        delta.append(d)
    return delta


def build(vocab: int, segments: Sequence[Union[Literal, AnyOf, FreeUntil, OneOf]], end: Union[str, Iterable[int]] = "done") -> TokenAutomaton:
    """The segments one after another.  end: "done" -- the token that completes the last segment ends the row; "free" -- anything
    afterwards (the stop rule, EOS or the budget end the row); ids -- exactly one of these ids (an EOS, say), which ends the row.
    entry: "start" and "segment<k>" (the state segment k is entered at)."""
    if not segments:
        raise ValueError("build: at least one segment")
    trans: Dict[Hashable, list] = {}
    tail: Dict[Hashable, list] = {}
    if isinstance(end, str):
        if end not in ("done", "free"):
            raise ValueError(f'build: end must be "done", "free" or a list of ids, got {end!r}')
        cont: Hashable = DONE
        if end == "free":
            cont = ("end",)
            tail[cont] = [(ANY, cont)]
    else:
        cont = ("end",)
        tail[cont] = [(list(end), DONE)]
    # compile from the back: every segment hands its last token to the entry of what follows it
    compiled: List[Tuple[Hashable, Dict[Hashable, list]]] = []
    for k in range(len(segments) - 1, -1, -1):
        seg, st = segments[k], {}
        if isinstance(seg, Literal) or isinstance(seg, AnyOf):
            sets = [[int(t)] for t in seg.ids] if isinstance(seg, Literal) else [list(seg.ids)] * int(seg.n)
            if not sets or any(len(x) == 0 for x in sets):
                raise ValueError(f"build: segment {k} is empty")
            for j, ids in enumerate(sets):
                st[(k, j)] = [(ids, (k, j + 1) if j + 1 < len(sets) else cont)]
        elif isinstance(seg, FreeUntil):
            trig = [int(t) for t in seg.trigger]
            if not trig:
                raise ValueError(f"build: segment {k} has an empty trigger")
            for j, d in enumerate(_kmp_delta(trig)):
                st[(k, j)] = [(ANY, (k, 0))] + [([t], (k, n) if n < len(trig) else cont) for t, n in sorted(d.items())]
        elif isinstance(seg, OneOf):
            alts = [tuple(int(t) for t in a) for a in seg.alternatives]
            if not alts or any(len(a) == 0 for a in alts):
                raise ValueError(f"build: segment {k} has no alternative, or an empty one")
            alts = sorted(set(alts))
            for a in alts:
                for b in alts:
                    if a != b and b[: len(a)] == a:
                        raise ValueError(f"build: segment {k}: alternative {list(a)} is a prefix of {list(b)}")
            nodes = {(): 0}
            for a in alts:
                for i in range(1, len(a)):
                    nodes.setdefault(a[:i], len(nodes))
            for pre, j in sorted(nodes.items(), key=lambda kv: kv[1]):
                out = {}
                for a in alts:
                    if a[: len(pre)] == pre:
                        t = a[len(pre)]
                        out[t] = (k, nodes[a[: len(pre) + 1]]) if len(a) > len(pre) + 1 else cont
                st[(k, j)] = [([t], n) for t, n in sorted(out.items())]
        else:
            raise ValueError(f"build: segment {k} is {type(seg).__name__}, not Literal / AnyOf / FreeUntil / OneOf")
        compiled.append(((k, 0), st))
        cont = (k, 0)
    entry = {"start": (0, 0)}
    for (e, st) in reversed(compiled):
        trans.update(st)
        entry[f"segment{e[0]}"] = e
    trans.update(tail)
    if len(trans) > MAX_STATES:
        raise ValueError(f"build: {len(trans)} states: more than {MAX_STATES}")
    return from_transitions(vocab, trans, entry)


def action_bins(vocab: int, n_bins: int = 256, dim: int = 7, token_vocab: Optional[int] = None) -> TokenAutomaton:
    """`dim` tokens from the action bins, then done.  token_vocab: the vocabulary size the bin ids count down from (default: vocab)."""
    return build(vocab, [AnyOf(action_bin_token_ids(token_vocab if token_vocab is not None else vocab, n_bins), dim)], end="done")


def policy_line(trigger_ids: Sequence[int], vocab: int, n_bins: int = 256, dim: int = 7, then: Union[str, Iterable[int]] = "free",
                token_vocab: Optional[int] = None) -> TokenAutomaton:
    """Free text until `trigger_ids` (the ids of "POLICIES:"), then exactly `dim` bin tokens, then `then` ("free": anything again -- the stop rule
    still ends the row)."""
    bins = action_bin_token_ids(token_vocab if token_vocab is not None else vocab, n_bins)
    return build(vocab, [FreeUntil(list(trigger_ids)), AnyOf(bins, dim)], end=then)


def policy_line_from_tokenizer(tokenizer, vocab: int, marker: str = "POLICIES:", n_bins: int = 256, dim: int = 7,
                               then: Union[str, Iterable[int]] = "free", token_vocab: Optional[int] = None) -> TokenAutomaton:
    """policy_line with the trigger ids taken from `tokenizer` as serving.stop_rule_from_tokenizer takes them."""
    from .serving import stop_rule_from_tokenizer

    trigger, _ = stop_rule_from_tokenizer(tokenizer, marker, 0)
    return policy_line(list(trigger), vocab, n_bins, dim, then, token_vocab)
