"""CPU: the drafting policy and the host loop of draft-verified decoding (emmax/drafting.py) against a fake engine whose "model" is a fixed
target sequence per row: whatever the draft says the output is the target, and the pass counts are what the policy promises."""
import importlib.util
import math
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (loaded by path: the module must import without torch, which the package's __init__ pulls in)
_spec = importlib.util.spec_from_file_location("emmax_drafting", os.path.join(ROOT, "emma-x_amd", "emmax", "drafting.py"))
drafting = importlib.util.module_from_spec(_spec)
import sys  # noqa: E402
sys.modules["emmax_drafting"] = drafting
_spec.loader.exec_module(drafting)
DraftParams, DraftCursor, drafted_generate, VerifyRefused = drafting.DraftParams, drafting.DraftCursor, drafting.drafted_generate, drafting.VerifyRefused

PAD = -7


class FakeEngine:
    """Rows in mid-generation whose greedy token at index n is targets[b][n]; a row is done when its target is exhausted (its EOS) or its budget
    is spent.  verify / decode_step / set_budget / output_tail follow include/emmax.h: emmax_verify and the calls around it."""

    def __init__(self, targets, refuse_verify=0):
        self.t = [list(t) for t in targets]
        self.n = [1] * len(targets)          # the prefill picked the first token
        self.budget = 1 << 30
        self.done = [len(t) <= 1 for t in self.t]
        self.refuse = refuse_verify
        self.verify_calls = self.step_calls = 0
        self.windows = []

    def set_budget(self, max_new):
        self.budget = max_new

    def _emit(self, b):
        if self.done[b]:
            return None
        if self.n[b] >= self.budget:
            self.done[b] = True
            return None
        tok = self.t[b][self.n[b]]
        self.n[b] += 1
        if self.n[b] >= len(self.t[b]) or self.n[b] >= self.budget:
            self.done[b] = True
        return tok

    def decode_step(self):
        self.step_calls += 1
        for b in range(len(self.t)):
            self._emit(b)

    def verify(self, windows, row0=0, max_new=None):
        assert row0 == 0 and len(windows) == len(self.t)
        if self.refuse:
            self.refuse -= 1
            raise VerifyRefused("no room")
        self.verify_calls += 1
        self.windows.append([len(w) for w in windows])
        self.budget = max_new
        emitted, new_ids = [], []
        for b, w in enumerate(windows):
            assert len(w) >= 1
            if not self.done[b]:
                assert w[0] == self.t[b][self.n[b] - 1], "the window must start with the row's pending token"
            got = []
            for i in range(len(w)):
                tok = self._emit(b)
                if tok is None:
                    break
                got.append(tok)
                if self.done[b] or i + 1 >= len(w) or tok != w[i + 1]:
                    break
            emitted.append(len(got))
            new_ids.append(got)
        return emitted, new_ids, [int(d) for d in self.done]

    def output_tail(self, first, n):
        assert n >= 1 and first >= 0
        return ([[(self.t[b][i] if i < self.n[b] else PAD) for i in range(first, first + n)] for b in range(len(self.t))],
                list(self.n), [int(d) for d in self.done])


def _run(targets, drafts, max_new=None, params=None, **kw):
    eng = FakeEngine(targets, **kw)
    max_new = max_new or max(len(t) for t in targets)
    ids, lens, stats = drafted_generate(eng, drafts, max_new, params)
    return eng, ids, lens, stats


def _mutate(rng, target, kind):
    d = list(target)
    if kind == "same":
        return d
    if kind == "empty":
        return []
    if kind == "unrelated":
        return [rng.randrange(1000, 2000) for _ in d]
    if kind == "short":
        return d[:max(len(d) // 2, 1)]
    for _ in range(rng.randrange(1, 5)):
        k = rng.randrange(len(d)) if d else 0
        if kind == "sub" and d:
            d[k] = rng.randrange(1000, 2000)
        elif kind == "ins":
            d.insert(k, rng.randrange(1000, 2000))
        elif kind == "del" and len(d) > 1:
            del d[k]
    return d


def test_output_equals_the_target_for_200_random_pairs():
    rng = random.Random(20240611)
    kinds = ["same", "sub", "ins", "del", "unrelated", "empty", "short"]
    for case in range(200):
        B = rng.randrange(1, 4)
        targets = [[rng.randrange(3, 40) for _ in range(rng.randrange(1, 90))] for _ in range(B)]   # a small alphabet: repeated n-grams
        drafts = [_mutate(rng, t, kinds[(case + b) % len(kinds)]) for b, t in enumerate(targets)]
        if case % 11 == 0:
            drafts[0] = None
        params = DraftParams(window=rng.choice([2, 3, 8, 33, 128]), ngram=rng.choice([2, 3, 4]), burst=rng.choice([1, 4]), give_up=rng.choice([1, 2, 3]))
        max_new = rng.choice([max(len(t) for t in targets), rng.randrange(1, 60)])
        eng, ids, lens, stats = _run(targets, drafts, max_new=max_new, params=params)
        want = [t[:max_new] for t in targets]
        assert ids == want, (case, params)
        assert lens == [len(w) for w in want]
        assert all(d or eng.n[b] >= max_new for b, d in enumerate(eng.done))   # (max_new = 1: the prefill's token was the budget)
        assert stats.passes == eng.verify_calls and stats.plain_steps == eng.step_calls
        assert all(0 <= a <= d for a, d in zip(stats.accepted, stats.drafted))


@pytest.mark.parametrize("n,w", [(64, 8), (65, 8), (100, 128), (129, 128), (257, 128), (40, 2)])
def test_identical_draft_takes_ceil_n_over_w_passes(n, w):
    target = list(range(10, 10 + n))
    eng, ids, _, stats = _run([target], [target], params=DraftParams(window=w))
    assert ids == [target] and stats.plain_steps <= 1  # (a last token for which the budget leaves no room for a draft id is a plain step)
    assert abs(stats.passes - math.ceil(n / w)) <= 1   # (the prefill's token and the bonus token of every pass)
    assert stats.accepted == stats.drafted or stats.accepted[0] >= stats.drafted[0] - 1


@pytest.mark.parametrize("k", [0, 1, 7, 8, 63, 127, 128, 199])
def test_one_substitution_costs_at_most_two_passes_and_a_burst(k):
    n, p = 200, DraftParams(window=64)
    target = list(range(10, 10 + n))
    draft = list(target)
    draft[k] = 5000
    base = _run([target], [target], params=p)[3]
    eng, ids, _, stats = _run([target], [draft], params=p)
    assert ids == [target]
    assert stats.passes <= base.passes + 2 and stats.plain_steps <= p.burst


def test_unrelated_draft_costs_exactly_give_up_passes_then_plain_steps():
    for give_up in (1, 2, 3):
        target = list(range(10, 110))
        p = DraftParams(give_up=give_up)
        eng, ids, _, stats = _run([target], [[5000 + i for i in range(100)]], params=p)
        assert ids == [target]
        assert stats.passes == give_up and stats.accepted == [0]
        rest = len(target) - 1 - give_up            # the prefill's token, one token per failed pass, the remainder as plain steps
        assert rest <= stats.plain_steps < rest + drafting.PLAIN_CHUNK


def test_no_draft_runs_plain_steps_only():
    target = list(range(10, 50))
    eng, ids, lens, stats = _run([target, target[:20]], [None, []])
    assert ids == [target, target[:20]] and lens == [40, 20] and stats.passes == 0 and eng.verify_calls == 0


def test_ragged_batch_where_one_row_finishes_early():
    targets = [list(range(10, 210)), list(range(300, 320)), list(range(400, 530))]
    drafts = [list(targets[0]), list(targets[1]), [7000] * 50]
    eng, ids, lens, stats = _run(targets, drafts, params=DraftParams(window=32))
    assert ids == targets and lens == [200, 20, 130]
    # the finished row rides along with one id; the row with the hopeless draft had a window in give_up passes and rode along alone in the others
    assert all(w[1] == 1 for w in eng.windows[1:]) and sum(w[2] > 1 for w in eng.windows) == DraftParams().give_up
    assert stats.accepted[2] == 0 and stats.accepted[0] >= 190


def test_insertion_and_deletion_resynchronise_by_ngram():
    target = list(range(10, 210))
    for draft in (target[:50] + [9000, 9001] + target[50:], target[:50] + target[53:]):
        eng, ids, _, stats = _run([target], [draft], params=DraftParams(window=64))
        assert ids == [target]
        assert stats.passes <= 8 and stats.plain_steps <= 2 * DraftParams().burst
        assert stats.accepted[0] >= 150


def test_budget_cuts_inside_an_accepted_run_and_clips_the_window():
    target = list(range(10, 210))
    eng, ids, lens, stats = _run([target], [target], max_new=70, params=DraftParams(window=64))
    assert ids == [target[:70]] and lens == [70]
    assert all(sum(w) <= 70 for w in eng.windows)   # no window reaches past the budget


def test_nomem_falls_back_to_plain_steps():
    target = list(range(10, 60))
    eng, ids, _, stats = _run([target], [target], refuse_verify=1)
    assert ids == [target] and stats.refused == 1 and stats.passes == 0 and stats.plain_steps >= len(target) - 1


def test_windows_are_clipped_to_the_rows_cache_room():
    class Capped(FakeEngine):
        max_ctx = 300

        def context_lengths(self, row0, n):
            return [270, 100][:n]      # after the prefill: row 0 has room for 28 more ids and its pending one, row 1 plenty

        def verify(self, windows, row0=0, max_new=None):
            for b, w in enumerate(windows):
                assert self.context_lengths(0, 2)[b] + (self.n[b] - 1) + len(w) + 1 <= self.max_ctx or self.done[b], (b, len(w))
            return super().verify(windows, row0, max_new)

    targets = [list(range(10, 38)), list(range(500, 640))]
    eng = Capped(targets)
    ids, lens, stats = drafted_generate(eng, [list(t) for t in targets], 140, DraftParams(window=64))
    assert ids == targets and stats.refused == 0 and stats.accepted[1] >= 130


def test_cursor_substitution_guess_and_give_up():
    c = DraftCursor([1, 2, 3, 4, 5, 6], DraftParams(window=4, give_up=2))
    c.feed(1)
    assert c.pos == 1 and c.window(10) == [2, 3, 4] and c.window(1) == [2]
    c.feed(2)
    c.feed(99)                       # the draft said 3
    assert c.pos is None
    c.resync()
    assert c.pos == 3                # just behind the draft id that was wrong
    c.feed(4)
    assert c.pos == 4
    c.passed(3, 0)
    c.passed(3, 0)
    assert c.off and c.window(10) == []


def test_params_are_validated():
    with pytest.raises(ValueError):
        DraftParams(window=1)
    with pytest.raises(ValueError):
        DraftParams(ngram=1)
