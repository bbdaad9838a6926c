"""CPU: the host side of constrained decoding (emmax/constraints.py; include/emmax.h: emmax_session_set_automaton).  The builders against
hand-written tables, the numpy replay (tests/constraint_ref.py) against transformers' PrefixConstrainedLogitsProcessor driven by a prefix
function derived from TokenAutomaton.walk, the margins of the rows the GPU test uses, the argument checks that raise before the engine is
touched, the scheduler's per-request plumbing against a fake engine, and the ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_ref as cr  # noqa: E402
import warpers_ref as wr  # noqa: E402
from conftest import ROOT  # noqa: E402
from emmax import constraints as ct  # noqa: E402
from emmax.actions import action_bin_token_ids  # noqa: E402
from emmax.sampling import SamplingParams  # noqa: E402
from emmax.serving import Request, SlotScheduler  # noqa: E402
from test_slot_groups import FakeStagedEngine, _encode  # noqa: E402

NEW_SYMBOLS = ("emmax_session_set_automaton", "emmax_session_set_automaton_starts", "emmax_slots_set_automaton_starts_staged",
               "emmax_session_clear_automaton", "emmax_session_automaton", "emmax_session_automaton_state", "emmax_op_sample_constrained")


def _allowed(aut, s):
    return sorted(np.flatnonzero(aut.allowed(s)).tolist())


# ---- builders against hand-written tables ---------------------------------------------------------------------------------------------
def test_from_transitions_refines_classes():
    """V = 10, two states.  Ids {0, 1} and {2, 3} differ in state "b" only, {4 .. 9} are allowed nowhere: three classes, numbered by
    their lowest id, and the tables are the hand-written ones."""
    aut = ct.from_transitions(10, {"a": [([0, 1, 2, 3], "b")], "b": [([0, 1], "a"), ([2, 3], ct.DONE)]}, entry={"start": "a", "second": "b"})
    assert aut.cls.tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 2, 2] and aut.n_classes == 3 and aut.n_states == 2
    assert aut.allow[:, 0].tolist() == [0b011, 0b011] and not aut.allow[:, 1:].any()
    assert aut.next[:, :2].tolist() == [[1, 1], [0, -1]]
    assert aut.entry == {"start": 0, "second": 1}
    # ANY, overridden by a later entry: everything loops, id 7 ends the row
    aut = ct.from_transitions(10, {0: [(ct.ANY, 0), ([7], ct.DONE)]})
    assert aut.n_classes == 2 and aut.cls.tolist() == [0] * 7 + [1] + [0] * 2 and aut.next.tolist() == [[0, -1]] and aut.allow[0, 0] == 0b11
    assert aut.walk([1, 2, 7]) == [0, 0, -1]
    with pytest.raises(ValueError, match="follows the token that ended the row"):
        aut.walk([7, 1])
    assert aut.walk([7, 1, 5], start=None) == [-1, -1, -1]   # an unconstrained row stays unconstrained


def test_walk_raises_on_a_forbidden_token():
    aut = ct.build(20, [ct.Literal([3, 4]), ct.AnyOf([5, 6], 2)], end="done")
    assert aut.walk([3, 4, 6, 5]) == [1, 2, 3, -1]
    assert _allowed(aut, 0) == [3] and _allowed(aut, 2) == [5, 6]
    with pytest.raises(ValueError, match="token 4 is not allowed in state 0"):
        aut.walk([4])
    with pytest.raises(ValueError, match="token 7 is not allowed"):
        aut.walk([3, 4, 7])
    assert aut.walk([6], start="segment1") == [3] and aut.entry == {"start": 0, "segment0": 0, "segment1": 2}


def test_free_until_follows_overlapping_prefixes():
    """A trigger with a repeated prefix, [a, a, b] fed a a a b: the third a keeps two ids matched (the stop rule's single-restart matcher
    would fall back to one and miss the trigger), so the b completes it and the next segment is entered."""
    a, b, x = 4, 9, 1
    aut = ct.build(16, [ct.FreeUntil([a, a, b]), ct.AnyOf([2, 3], 1)], end="done")
    seg1 = aut.entry["segment1"]
    assert aut.walk([a, a, a, b]) == [1, 2, 2, seg1]
    assert aut.walk([x, a, x, a, a, b]) == [0, 1, 0, 1, 2, seg1]
    assert all(len(_allowed(aut, s)) == 16 for s in range(3)) and _allowed(aut, seg1) == [2, 3]
    # the hand-written KMP table of a a b: rows = ids matched, columns = (other, a, b)
    col = {i: (1 if i == a else 2 if i == b else 0) for i in range(16)}
    want = [[0, 1, 0], [0, 2, 0], [0, 2, seg1]]
    for s in range(3):
        for i in range(16):
            assert aut.next[s, aut.cls[i]] == want[s][col[i]], (s, i)
    # a b a b c fed a b a b a b c
    aut = ct.build(16, [ct.FreeUntil([4, 9, 4, 9, 7])], end="done")
    assert aut.walk([4, 9, 4, 9, 4, 9, 7]) == [1, 2, 3, 4, 3, 4, -1]


def test_one_of_shares_prefixes():
    aut = ct.build(32, [ct.OneOf([[5, 6, 7], [5, 6, 8], [5, 9], [10]])], end=[2])
    assert _allowed(aut, 0) == [5, 10] and aut.walk([5, 6, 8, 2]) == [1, 2, 3, -1] and aut.walk([5, 9, 2])[-1] == -1 and aut.walk([10, 2]) == [3, -1]
    assert _allowed(aut, 1) == [6, 9] and _allowed(aut, 2) == [7, 8] and _allowed(aut, 3) == [2]
    assert aut.n_states == 4   # the trie's three inner nodes and the end state
    with pytest.raises(ValueError, match="is a prefix of"):
        ct.build(32, [ct.OneOf([[5, 6], [5, 6, 7]])])


def test_end_free_and_the_two_shapes_of_this_model():
    V = 320
    aut = ct.action_bins(V, 256, 7)
    bins = sorted(action_bin_token_ids(V, 256))
    assert aut.n_states == 7 and aut.n_classes == 2 and all(_allowed(aut, s) == bins for s in range(7))
    assert aut.walk([bins[0]] * 7) == [1, 2, 3, 4, 5, 6, -1]
    pol = ct.policy_line([70, 71], 400, 256, 3, token_vocab=320)
    seq = [1, 70, 70, 71, 100, 319, 64, 5, 6]
    st = pol.walk(seq)
    assert st[:4] == [0, 1, 1, 2] and st[4:7] == [3, 4, 5] and st[7:] == [5, 5] and len(_allowed(pol, 5)) == 400 and _allowed(pol, 3) == bins
    with pytest.raises(ValueError, match="not allowed"):
        pol.walk([70, 71, 63])   # 63 is below the bins

    class Tok:   # "\n" -> [13]; "\nPOLICIES:" -> [13, 70, 71]: the marker in context
        def __call__(self, text, add_special_tokens=False):
            return {"input_ids": [13] + ([70, 71] if text.endswith("POLICIES:") else [])}

    auto = ct.policy_line_from_tokenizer(Tok(), 400, n_bins=256, dim=3, token_vocab=320)
    assert (auto.cls == pol.cls).all() and (auto.allow == pol.allow).all() and (auto.next == pol.next).all()


def test_caps_and_validation_errors():
    with pytest.raises(ValueError, match="257 token classes"):   # every id its own fate: V classes
        ct.from_transitions(257, {0: [([i], 0 if i % 2 else ct.DONE) for i in range(257)], **{s: [([i for i in range(257) if (i >> (s - 1)) & 1], 0)] for s in range(1, 10)}})
    with pytest.raises(ValueError, match="1025 states"):
        ct.build(8, [ct.Literal([1] * 1025)])
    with pytest.raises(ValueError, match="1025 states"):
        ct.from_transitions(8, {s: [([1], 0)] for s in range(1025)})
    assert ct.build(8, [ct.Literal([1] * 1024)]).n_states == 1024
    with pytest.raises(ValueError, match="not a state"):
        ct.from_transitions(8, {0: [([1], 5)]})
    with pytest.raises(ValueError, match="outside 0..7"):
        ct.from_transitions(8, {0: [([8], 0)]})
    ok = ct.from_transitions(8, {0: [([1], 0)]})
    with pytest.raises(ValueError, match="class 3"):
        ct.TokenAutomaton(8, np.full(8, 3, np.uint8), ok.allow, ok.next)
    with pytest.raises(ValueError, match="next states"):
        ct.TokenAutomaton(8, ok.cls, ok.allow, np.full((1, 2), 1, np.int16))
    with pytest.raises(ValueError, match="cls must be"):
        ct.TokenAutomaton(9, ok.cls, ok.allow, ok.next)
    with pytest.raises(ValueError, match="entry"):
        ct.TokenAutomaton(8, ok.cls, ok.allow, ok.next, {"x": 1})
    with pytest.raises(ValueError, match="not one of the automaton's entries"):
        ok.start_state("nowhere")
    with pytest.raises(ValueError, match="outside -1..0"):
        ok.start_state(1)
    assert ok.starts(None, 3) == [0, 0, 0] and ok.starts([None, 0, -1], 3) == [-1, 0, -1]
    with pytest.raises(ValueError, match="2 entries for 3 rows"):
        ok.starts([0, 0], 3)


# ---- the replay against HF ------------------------------------------------------------------------------------------------------------
def _hf_masked(l, aut, prefix, start):
    """The row through HF's PrefixConstrainedLogitsProcessor, whose prefix function replays the emitted ids through .walk"""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor

    def allowed(batch_id, sent):
        st = aut.walk(sent.tolist(), start)
        return np.flatnonzero(aut.allowed(st[-1] if st else aut.start_state(start))).tolist()

    proc = PrefixConstrainedLogitsProcessor(allowed, num_beams=1)
    return proc(torch.tensor([prefix], dtype=torch.long), torch.from_numpy(np.asarray(l, dtype=np.float32))[None])[0].numpy()


@pytest.mark.parametrize("V", [wr.V_SMALL, 32000])
def test_replay_masks_what_hf_masks(V):
    """Along a walk through the eight states of the committed automaton, and through a policy line: the replay's masked row equals HF's."""
    aut = cr.make_automaton(V)
    l = wr.logits_row(3, V)
    prefix, s = [], 0
    for _ in range(10):
        got, hf = cr.mask_row(l, aut, s), _hf_masked(l, aut, prefix, 0)
        assert (np.isinf(got) == np.isinf(hf)).all() and (got[np.isfinite(got)] == hf[np.isfinite(hf)]).all() and np.isfinite(got).any()
        tok = int(np.argmax(np.where(np.arange(V) % 2 == 0, got, -np.inf)))   # an even id: the row moves to the next state
        prefix.append(tok)
        s = aut.step(s, tok)
    assert s == 10 % 8
    pol = ct.policy_line([5, 6], V, min(256, V // 2), 2)
    bins = action_bin_token_ids(V, min(256, V // 2))
    for prefix in ([], [5], [5, 6], [5, 6, bins[0]], [5, 6, bins[0], bins[1]], [5, 5, 6]):
        st = pol.walk(prefix)[-1] if prefix else 0
        got, hf = cr.mask_row(l, pol, st), _hf_masked(l, pol, prefix, 0)
        assert (np.isinf(got) == np.isinf(hf)).all() and (got[np.isfinite(got)] == hf[np.isfinite(hf)]).all()


# ---- the margins of the GPU test's rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", cr.SIZES)
def test_every_committed_row_clears_the_lines_under_the_mask(V):
    """No row is skipped on the GPU: each of the eight rows, masked by its state, clears warpers_ref's lines in both arithmetics (which then
    keep the same set) and its draw clears the Gumbel margin; the eight states keep eight different sets."""
    aut = cr.make_automaton(V)
    assert aut.n_states == 8 and aut.n_classes <= 64
    assert len({aut.allowed(s).tobytes() for s in range(8)}) == 8
    l0 = cr.committed_rows(V)[0][1]
    assert cr.CASES[0][0] == 0 and aut.allowed(0)[int(np.argmax(l0))]   # row 0 emits its unconstrained token: the GPU test compares its log-probability bits
    for b, l, state, case in cr.committed_rows(V):
        seed, sub, step = cr.row_params(b)
        assert cr.clears(l, aut, state, case, seed, sub, step), (V, b, case)
        row = cr.constrained_row(l, aut, state, n_out=step)
        if case[0] > 0:
            keep, _, _ = wr.kept_set_ext(row, *case)
            keep64, _, info64 = wr.kept_set_ext(row, *case, emulate=False)
            assert wr.clears(info64) and (keep == keep64).all() and keep.any() and not keep[~aut.allowed(state)].any()


# ---- the argument checks raise before the engine is touched -------------------------------------------------------------------------------
def test_constraint_arguments_raise_before_the_engine():
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction

    class NoEngine(EmmaXForActionPrediction):
        def __init__(self):
            self.config = EmmaXConfig.tiny()

        def _need_engine(self):
            raise AssertionError("the engine was touched")

    m = NoEngine()
    V = m.config.llm.vocab_size
    aut = ct.action_bins(V, 256, 7)
    ids = torch.tensor([[1, 5, 6]])
    with pytest.raises(NotImplementedError, match="constraint= with num_beams > 1"):
        m.generate(ids, constraint=aut, num_beams=2)
    with pytest.raises(NotImplementedError, match="constraint="):
        m.generate(ids, prefix_allowed_tokens_fn=lambda b, s: [1])
    with pytest.raises(ValueError, match="must be a constraints.TokenAutomaton"):
        m.generate_ids([[1, 5]], constraint=object())
    with pytest.raises(ValueError, match="constraint_start needs constraint="):
        m.generate_ids([[1, 5]], constraint_start=0)
    with pytest.raises(ValueError, match="the model's vocabulary has"):
        m.generate_ids([[1, 5]], constraint=ct.action_bins(V - 1, 256, 7))
    with pytest.raises(ValueError, match="not one of the automaton's entries"):
        m.generate_ids([[1, 5]], constraint=aut, constraint_start="policy")
    with pytest.raises(ValueError, match="1 entries for 2 rows"):
        m.generate_ids([[1, 5], [1, 6]], constraint=aut, constraint_start=[0])
    from emmax.sampling import BeamParams

    with pytest.raises(NotImplementedError, match="num_beams > 1"):
        m.generate_ids([[1, 5]], constraint=aut, beams=BeamParams(2))


def test_generate_actions_hands_the_constraint_on():
    """generate_actions has no argument of its own: constraint= / constraint_start= in its kwargs reach generate_ids (README form), and
    predict_action(constrain_to_bins=True) builds action_bins over the model's vocabulary, counting the bins down from the tokenizer's."""
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction

    calls = []

    class Recorder(EmmaXForActionPrediction):
        def __init__(self):
            self.config = EmmaXConfig.tiny()
            self.vocab_size = self.config.action_vocab_size
            self.tokenizer = None

        def generate_ids(self, rows, *a, **kw):
            calls.append(kw)
            n = kw["max_new_tokens"]
            return torch.zeros((1, n), dtype=torch.int32), torch.tensor([n], dtype=torch.int32)

        def _postprocess(self, ids, tokenizer, type="act"):
            return [np.zeros(7)], "text"

        def get_action_dim(self, key):
            return 7

        def get_action_stats(self, key):
            return {"q01": np.zeros(7), "q99": np.ones(7)}

        bin_centers = np.linspace(-1, 1, 256)

    m = Recorder()
    V = m.config.llm.vocab_size
    aut = ct.policy_line([5, 6], V, 256, token_vocab=m.vocab_size)
    m.generate_actions({"input_ids": torch.tensor([[1, 5, 6]]), "frames_u8": None}, object(), max_new_tokens=9, constraint=aut, constraint_start="start")
    assert calls[-1]["constraint"] is aut and calls[-1]["constraint_start"] == "start"
    m.generate_actions({"input_ids": torch.tensor([[1, 5, 6]]), "frames_u8": None}, object(), max_new_tokens=9)
    assert "constraint" not in calls[-1]
    m.predict_action(torch.tensor([[1, 5, 29871]]), "bridge_orig", constrain_to_bins=True)
    got = calls[-1]["constraint"]
    assert got.vocab == V and got.n_states == 7 and sorted(np.flatnonzero(got.allowed(0))) == sorted(action_bin_token_ids(m.vocab_size, 256))
    with pytest.raises(ValueError, match="one of constrain_to_bins= and constraint="):
        m.predict_action(torch.tensor([[1, 5, 29871]]), "bridge_orig", constrain_to_bins=True, constraint=aut)
    with pytest.raises(NotImplementedError, match="constrain_to_bins with num_beams > 1"):
        m.predict_action(torch.tensor([[1, 5, 29871]]), "bridge_orig", constrain_to_bins=True, num_beams=2)


# ---- the scheduler's plumbing ---------------------------------------------------------------------------------------------------------------
class FakeConstrainedEngine(FakeStagedEngine):
    def __init__(self, plans, lag=2):
        super().__init__(plans, lag)
        self.automaton_set, self.starts, self.staged_starts = None, {}, None

    def set_automaton(self, a):
        self.automaton_set = a
        self.log.append(("automaton",))

    def set_automaton_starts(self, starts, row0=0):
        assert self.automaton_set is not None
        for i, s in enumerate(starts):
            self.starts[row0 + i] = s

    def set_automaton_starts_staged(self, starts):
        assert self.automaton_set is not None and self.in_admission
        self.staged_starts = list(starts)

    def slots_commit(self, handle, slots, staged_idx=None):
        for slot, i in zip(slots, staged_idx):
            self.starts[slot] = self.staged_starts[i]
            self.staged_params.setdefault(i, None)   # (a greedy serve stages no sampling parameters)
        super().slots_commit(handle, slots, staged_idx)
        for slot in slots:
            self.log.append(("start", self.slots[slot]["rid"], self.starts[slot]))

    def slot_prefill(self, slot, ids, pe, max_new):
        super().slot_prefill(slot, ids, pe, max_new)
        self.log.append(("start", pe["rid"], self.starts[slot]))

    def clear_automaton(self):
        self.automaton_set = None
        self.log.append(("clear_automaton",))


@pytest.mark.parametrize("overlap", [False, True])
def test_scheduler_carries_per_request_starts(overlap):
    """Requests with a named start, a state, and none: every prefill is preceded by its rows' starts (-1 for the unconstrained), the
    automaton is set once for the run and cleared after it; a run without constrained requests calls nothing new."""
    aut = ct.build(64, [ct.FreeUntil([5]), ct.AnyOf([6, 7], 2)], end="free")
    plans = {(i, 0): [10 + i] * (3 + i) for i in range(5)}
    eng = FakeConstrainedEngine(plans)
    sch = SlotScheduler(eng, _encode, n_slots=2, poll_every=1, overlap=overlap, automaton=aut)
    starts = ["start", None, "segment1", 2, None]
    for i in range(5):
        sch.submit(Request(i, i, [1, 2], max_new_tokens=8, constraint_start=starts[i]))
    with pytest.raises(ValueError, match="not one of the automaton's entries"):
        sch.submit(Request(9, 9, [1], constraint_start="nowhere"))
    res = sch.run()
    assert sorted(r.rid for r in res) == list(range(5)) and all(r.ids == plans[(r.rid, 0)] for r in res)
    seen = {e[1]: e[2] for e in eng.log if e[0] == "start"}
    assert seen == {0: 0, 1: -1, 2: aut.entry["segment1"], 3: 2, 4: -1}
    assert [e for e in eng.log if e[0] in ("automaton", "clear_automaton")] == [("automaton",), ("clear_automaton",)] and eng.automaton_set is None
    # no constrained request: nothing new is called (the plain fake engine has none of the methods)
    plain = FakeStagedEngine(plans)
    sch = SlotScheduler(plain, _encode, n_slots=2, poll_every=1, overlap=overlap, automaton=aut)
    for i in range(3):
        sch.submit(Request(i, i, [1, 2], max_new_tokens=8, sampling=SamplingParams(1.0, 0, 1.0, seed=7)))   # (the fake stages sampled requests only)
    assert sorted(r.rid for r in sch.run()) == [0, 1, 2]
    with pytest.raises(ValueError, match="has no automaton"):
        SlotScheduler(FakeStagedEngine(plans), _encode, n_slots=2).submit(Request(0, 0, [1], constraint_start=0))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_stays_12_with_new_symbols_only():
    from emmax import _lib

    hdr = open(os.path.join(ROOT, "include", "emmax.h")).read()
    assert re.search(r"#define\s+EMMAX_ABI_VERSION\s+12\b", hdr) and _lib.ABI_VERSION == 12
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    n_args = len(re.search(r"int emmax_op_sample_constrained\((.*?)\);", hdr, re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES["emmax_op_sample_constrained"][1]) == len(_lib.SIGNATURES["emmax_op_sample_ext"][1]) + 7
    if os.path.isfile(_lib.LIB_PATH):
        import ctypes as C

        lib = C.CDLL(_lib.LIB_PATH)
        assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
