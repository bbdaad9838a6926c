"""Draft-verified greedy decoding: the drafting policy and the host loop above engine.verify (include/emmax.h: emmax_verify).

A robot policy is called several times a second on almost the same scene, and the reasoning it writes at control step t + 1 is mostly,
token for token, the reasoning of step t.  That previous answer is the DRAFT: the loop feeds the next stretch of it teacher-forced through one
verify pass and keeps the longest prefix the model's own argmax agrees with, so the ids are exactly those of plain greedy decoding whatever the
draft says -- a wrong draft costs passes, never a token.  Pure Python over an engine with four calls (verify, decode_step, set_budget,
output_tail); no torch is needed to import this module.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

# the policy's constants, named once
DEFAULT_WINDOW = 128    # ids of one verify window, the pending token included (one pass over 128 rows costs about what three decode steps cost)
DEFAULT_NGRAM = 3       # emitted ids a lost cursor looks for in the draft; shorter n-grams down to MIN_NGRAM
MIN_NGRAM = 2
DEFAULT_BURST = 4       # plain decode steps while no live row has a window, before the next re-synchronisation attempt
DEFAULT_GIVE_UP = 2     # consecutive verify passes without one accepted draft id after which a row drafts no more in this call
PLAIN_CHUNK = 16        # plain steps between two looks at the done flags once no row drafts any more (emmax_generate's interval)


class VerifyRefused(RuntimeError):
    """engine.verify found no room for the windows (EMMAX_ERR_NOMEM): nothing changed, the loop falls back to plain decode steps."""


@dataclass
class DraftParams:
    window: int = DEFAULT_WINDOW
    ngram: int = DEFAULT_NGRAM
    burst: int = DEFAULT_BURST
    give_up: int = DEFAULT_GIVE_UP

    def __post_init__(self):
        if self.window < 2 or self.ngram < MIN_NGRAM or self.burst < 1 or self.give_up < 1:
            raise ValueError(f"DraftParams: window >= 2, ngram >= {MIN_NGRAM}, burst >= 1, give_up >= 1 (got {self})")


@dataclass
class DraftStats:
    passes: int = 0                 # verify passes of the call
    plain_steps: int = 0            # plain decode steps of the call
    refused: int = 0                # verify calls that found no room
    drafted: List[int] = field(default_factory=list)    # per row: draft ids put into windows
    accepted: List[int] = field(default_factory=list)   # per row: draft ids the model agreed with

    @property
    def tokens_per_pass(self) -> float:
        return (sum(self.accepted) + self.passes) / self.passes if self.passes else 0.0


class DraftCursor:
    """Where one row stands in its draft.  pos: the draft index of the id expected behind the row's pending token, None = lost."""

    def __init__(self, draft: Sequence[int], params: DraftParams):
        self.draft = [int(t) for t in draft]
        self.params = params
        self.pos: Optional[int] = 0
        self.last = 0               # the last synchronised position: where a re-synchronisation looks first
        self.miss = 0               # while lost: the draft index that was wrong, and the ids emitted since (the wrong one included)
        self.since = 0
        self.guessed = False        # the position is a guess that no accepted draft id has confirmed yet
        self.hist: List[int] = []   # the last ngram emitted ids
        self.fails = 0              # consecutive verify passes that accepted no draft id
        self.off = len(self.draft) == 0

    def window(self, room: int) -> List[int]:
        """The draft ids behind the pending token: at most window - 1 and at most `room`."""
        if self.off or self.pos is None:
            return []
        return self.draft[self.pos:self.pos + max(min(self.params.window - 1, room), 0)]

    def feed(self, tok: int) -> None:
        """One emitted id: it advances the cursor or loses it."""
        self.hist = (self.hist + [int(tok)])[-self.params.ngram:]
        if self.off:
            return
        if self.pos is None:
            self.since += 1
        elif self.pos < len(self.draft) and self.draft[self.pos] == tok:
            self.pos += 1
            self.last = self.pos
            self.guessed = False
        else:
            self.miss, self.since, self.pos = self.pos, 1, None

    def _find(self, key: List[int]) -> Optional[int]:
        d, n = self.draft, len(key)
        first = max(self.last - n, 0)
        for s in list(range(first, len(d) - n + 1)) + list(range(0, min(first, len(d) - n + 1))):
            if d[s:s + n] == key:
                return s + n
        return None

    def resync(self) -> None:
        """A lost cursor looks for the last emitted ids in the draft -- forward from the last synchronised position first, then from the start,
        n-grams from `ngram` down to 2.  If nothing is found directly after a mismatch it tries ONCE the substitution guess: just behind the
        draft id that was wrong.  A guess that the next pass does not confirm is not followed by another at once: the row decodes plainly, and
        only when `burst` more ids have brought no n-gram either does it guess again, at the place a run of substitutions would have reached
        (so a draft that has nothing to do with the answer fails `give_up` passes and is dropped, while an insertion or a deletion is found
        again by its n-gram as soon as the ids behind it are out)."""
        if self.off or self.pos is not None:
            return
        for n in range(min(self.params.ngram, len(self.hist)), MIN_NGRAM - 1, -1):
            at = self._find(self.hist[-n:])
            if at is not None:
                self.pos = self.last = at
                self.guessed = False
                return
        if (not self.guessed or self.since > self.params.burst) and self.miss + self.since <= len(self.draft):
            self.pos = self.miss + self.since
            self.guessed = True

    def passed(self, n_drafted: int, n_accepted: int) -> None:
        """The outcome of a verify pass in which the row's window held n_drafted draft ids."""
        if n_drafted == 0:
            return
        self.fails = 0 if n_accepted > 0 else self.fails + 1
        if self.fails >= self.params.give_up:
            self.off = True


def drafted_generate(engine, drafts: Sequence[Optional[Sequence[int]]], max_new: int,
                     params: Optional[DraftParams] = None) -> Tuple[List[List[int]], List[int], DraftStats]:
    """The greedy generation of the engine's live rows -- prefilled (or extended), first token picked -- with one draft (or None) per row.
    While any live row has a window, one engine.verify for the whole batch (rows without one ride along with their pending token alone);
    otherwise `burst` plain decode steps, then the new ids are read back and lost cursors try to re-synchronise.  Ends when every row is done.
    -> (ids per row, their counts, DraftStats); the ids are those of plain greedy decoding under the same budget and stop rule."""
    params = params or DraftParams()
    B = len(drafts)
    cur = [DraftCursor(d, params) if d is not None and len(d) else None for d in drafts]
    stats = DraftStats(drafted=[0] * B, accepted=[0] * B)
    engine.set_budget(max_new)
    first, n_out, done = engine.output_tail(0, 1)
    out: List[List[int]] = [list(first[b][:min(n_out[b], 1)]) for b in range(B)]
    done = [bool(x) or len(out[b]) >= max_new for b, x in enumerate(done)]   # (a prefill does not look at the budget: max_new = 1 ends here)

    def take(b: int, toks: Sequence[int]) -> None:
        for t in toks:
            out[b].append(int(t))
            if cur[b] is not None:
                cur[b].feed(int(t))

    for b in range(B):
        if cur[b] is not None:
            for t in out[b]:
                cur[b].feed(t)
            cur[b].resync()
    # a window is clipped to what the row may still emit (the budget) and to what its cache still holds: context + window + the pending token within
    # max_ctx (an engine that names neither is not asked).  The context is the prefill's plus the ids emitted since, the pending one not yet cached
    cap = getattr(engine, "max_ctx", None)
    ctx0 = engine.context_lengths(0, B) if cap is not None and hasattr(engine, "context_lengths") else None

    def room(b: int) -> int:
        r = max_new - len(out[b]) - 1
        return r if ctx0 is None else min(r, cap - (ctx0[b] + len(out[b]) - 1) - 2)

    while not all(done):
        wins = [[] if done[b] or cur[b] is None else cur[b].window(room(b)) for b in range(B)]
        if any(wins):
            pending = [out[b][-1] if out[b] else 0 for b in range(B)]
            try:
                emitted, new_ids, d2 = engine.verify([[pending[b]] + wins[b] for b in range(B)], max_new=max_new)
            except VerifyRefused:
                stats.refused += 1
                for c in cur:
                    if c is not None:
                        c.off = True
                continue
            stats.passes += 1
            for b in range(B):
                if done[b]:
                    continue
                take(b, new_ids[b][:emitted[b]])
                if cur[b] is not None:
                    acc = max(min(emitted[b] - 1, len(wins[b])), 0)
                    stats.drafted[b] += len(wins[b])
                    stats.accepted[b] += acc
                    cur[b].passed(len(wins[b]), acc)
                    cur[b].resync()
                done[b] = bool(d2[b])
            continue
        drafting = any(not done[b] and cur[b] is not None and not cur[b].off for b in range(B))
        left = max(max_new - len(out[b]) for b in range(B) if not done[b])
        steps = max(min(params.burst if drafting else PLAIN_CHUNK, left), 1)
        first_idx = min(len(out[b]) for b in range(B) if not done[b])
        last_idx = min(max(len(out[b]) for b in range(B) if not done[b]) + steps, max_new)
        for _ in range(steps):
            engine.decode_step()
        stats.plain_steps += steps
        tail, n_out, d2 = engine.output_tail(first_idx, last_idx - first_idx)
        for b in range(B):
            if done[b]:
                continue
            k = len(out[b]) - first_idx   # (rows of a ragged batch stand at different counts: the tail starts at the shortest)
            take(b, tail[b][k:max(n_out[b] - first_idx, k)])
            if cur[b] is not None:
                cur[b].resync()
            done[b] = bool(d2[b])
    return out, [len(o) for o in out], stats
