"""CPU: the host side of the EXT finish (include/emmax.h: emmax_session_set_warpers / emmax_session_set_token_rules / emmax_op_sample_ext).
The numpy replay of the documented arithmetic (tests/warpers_ref.py) is held to transformers' own classes; the lines a test row must clear
are re-measured; the argument folding, the dataclasses, the beam refusal, the scheduler's per-request plumbing and the ABI are checked
without a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warpers_ref as wr  # noqa: E402
from conftest import ROOT  # noqa: E402
from emmax.sampling import MAX_RULE_IDS, MAX_RULES, LogitsProcessing, SamplingParams, rule_table  # noqa: E402
from test_slot_groups import FakeStagedEngine, _encode  # noqa: E402

NEW_SYMBOLS = ("emmax_op_sample_ext", "emmax_session_set_warpers", "emmax_slots_set_warpers_staged", "emmax_session_clear_warpers", "emmax_session_warpers",
               "emmax_session_set_token_rules", "emmax_session_set_rule_enables", "emmax_slots_set_rule_enables_staged", "emmax_session_clear_token_rules",
               "emmax_session_token_rules")


@pytest.fixture(scope="module")
def rows():
    return wr.committed_rows()


# ---- the replay against HF's classes -------------------------------------------------------------------------------------------------
def hf_warped(l, case):
    """The row through HF's warpers in _get_logits_processor's order (fp32, as generate runs them)."""
    from transformers.generation import logits_process as lp

    T, k, p, mp, ty, ep, et = case
    s, ids = torch.from_numpy(np.asarray(l, dtype=np.float32))[None], torch.zeros((1, 1), dtype=torch.long)
    chain = [lp.TemperatureLogitsWarper(float(T))] if T != 1.0 else []
    chain += [lp.TopKLogitsWarper(k)] if k > 0 else []
    chain += [lp.TopPLogitsWarper(p)] if p < 1 else []
    chain += [lp.MinPLogitsWarper(mp)] if mp > 0 else []
    chain += [lp.TypicalLogitsWarper(ty)] if 0 < ty < 1 else []
    chain += [lp.EpsilonLogitsWarper(ep)] if ep > 0 else []
    chain += [lp.EtaLogitsWarper(et)] if et > 0 else []
    for w in chain:
        s = w(ids, s)
    return s[0].numpy()


def test_the_lines_are_twice_the_measured_arithmetic_error(rows):
    """LINE_* = 2 x the worst |fp32 emulation of the device arithmetic - float64| per decision quantity (rounded up, never more than 3 x)."""
    worst = wr.measure_lines([(l, c) for _, _, l, c in rows])
    for name, line in (("min_p", wr.LINE_MIN_P), ("epsilon", wr.LINE_EPSILON), ("eta", wr.LINE_ETA), ("typ_cum", wr.LINE_TYP_CUM),
                       ("typ_dist", wr.LINE_TYP_DIST)):
        print(name, "worst", worst[name], "line", line)
        assert worst[name] > 0 and 2 * worst[name] <= line <= 3 * worst[name], (name, worst[name], line)


def test_every_committed_row_clears_every_line(rows):
    """No row is skipped anywhere: each decision of each committed row is further from its threshold than the line, in both arithmetics
    (which then keep the same set), and its draw clears the Gumbel margin."""
    assert len(rows) == 2 * len(wr.ROW_SEEDS) * len(wr.CASES) // 2
    for seed, V, l, case in rows:
        keep, _, info = wr.kept_set_ext(l, *case)
        keep64, _, info64 = wr.kept_set_ext(l, *case, emulate=False)
        assert wr.clears(info) and wr.clears(info64), (seed, V, case, {k: (v.get("slack"), v.get("gap")) for k, v in info.items()})
        assert (keep == keep64).all() and keep.any()
        assert wr.sample_row_ext(l, case, 1000 + seed, seed % 3, seed)[2] > wr.MARGIN, (seed, V, case)


def test_replay_keeps_what_hf_keeps(rows):
    """V = 32064 and V = 37 (no multiple of 4), each warper alone and all chained behind top-k 50 / top-p 0.9: equal kept sets, equal scores."""
    for seed, V, l, case in rows:
        keep, z, _ = wr.kept_set_ext(l, *case)
        hf = hf_warped(l, case)
        assert ((hf > -np.inf) == keep).all(), (seed, V, case, int(keep.sum()), int((hf > -np.inf).sum()))
        assert (hf[keep] == z[keep]).all()   # z = l / T in fp32: HF's own division


def test_replay_corner_rows_against_hf():
    V = 37
    # min_p = 1: only the maxima stay (ties kept)
    l = wr.logits_row(11, V)
    l[[5, 20]] = l.max() + 1
    keep = wr.kept_set_ext(l, 1.0, 0, 1.0, 1.0)[0]
    assert sorted(np.flatnonzero(keep)) == [5, 20] and ((hf_warped(l, (1.0, 0, 1.0, 1.0, 0, 0, 0)) > -np.inf) == keep).all()
    # an exact tie at the min_p threshold is kept: logit differences of 0 and -ln 4 would need exp to be exact, so the tie is built from the
    # integer masses instead -- min_p = W_i / 2^32 for an entry's own (emulated) mass, which fp32 holds exactly when W_i < 2^24 2^k
    l = np.full(V, -30.0, dtype=np.float32)
    l[0], l[3], l[4], l[9] = 0.0, -2.0, -2.0, -2.5
    W = np.floor(np.float64(np.exp(np.float32(-2.0))) * 2.0 ** 32)
    mp = float(np.float32(W / 2.0 ** 32))
    assert np.floor(mp * 2.0 ** 32) == W
    keep, _, info = wr.kept_set_ext(l, 1.0, 0, 1.0, mp)
    assert sorted(np.flatnonzero(keep)) == [0, 3, 4] and info["min_p"]["slack"] == 0.0
    # a one-hot row (H = 0) through eta and typical keeps its entry; -inf entries from a ban stay out of every sum
    l = np.full(V, -np.inf, dtype=np.float32)
    l[7] = 1.5
    for case in ((1.0, 0, 1.0, 0, 0.5, 0, 0), (1.0, 0, 1.0, 0, 0, 0, 1e-3), (0.7, 0, 1.0, 0.1, 0.9, 1e-3, 1e-3)):
        keep = wr.kept_set_ext(l, *case)[0]
        assert np.flatnonzero(keep).tolist() == [7] and ((hf_warped(l, case) > -np.inf) == keep).all()
    l = wr.logits_row(12, V)
    l[[1, 2, 30]] = -np.inf
    for case in wr.CASES:
        keep, _, info = wr.kept_set_ext(l, *case)
        if wr.clears(info):
            assert ((hf_warped(l, case) > -np.inf) == keep).all() and not keep[[1, 2, 30]].any()


# ---- the token rules against HF's processors --------------------------------------------------------------------------------------------
def hf_processed(l, hist, n_out, proc, eos_id=2):
    from transformers.generation import logits_process as lp

    s, ids = torch.from_numpy(np.asarray(l, dtype=np.float32))[None], torch.tensor([hist], dtype=torch.long)
    chain = []
    if proc.sequence_bias:
        chain.append(lp.SequenceBiasLogitsProcessor({k: b for k, b in proc.sequence_bias}))
    if proc.repetition_penalty != 1.0:
        chain.append(lp.RepetitionPenaltyLogitsProcessor(proc.repetition_penalty))
    if proc.no_repeat_ngram_size:
        chain.append(lp.NoRepeatNGramLogitsProcessor(proc.no_repeat_ngram_size))
    if proc.bad_words_ids:
        chain.append(lp.NoBadWordsLogitsProcessor([list(w) for w in proc.bad_words_ids], eos_id))
    if proc.min_new_tokens:
        chain.append(lp.MinNewTokensLengthLogitsProcessor(len(hist) - n_out, proc.min_new_tokens, eos_id))
    if proc.suppress_tokens:
        chain.append(lp.SuppressTokensLogitsProcessor(list(proc.suppress_tokens)))
    if proc.begin_suppress_tokens:
        chain.append(lp.SuppressTokensAtBeginLogitsProcessor(list(proc.begin_suppress_tokens), len(hist) - n_out))
    for w in chain:
        s = w(ids, s)
    return s[0].numpy()


RULES = LogitsProcessing(1.3, 3, 2, sequence_bias={(6,): 2.5, (4, 6): -1.25, (9, 4, 6): 0.3, (2, 9, 4, 6): 7.0, (8, 8, 8, 8, 8, 8, 8, 5): 1.0, (4, 12): -3.0},
                         bad_words_ids=[[4, 13], [14], [9, 9, 15]], suppress_tokens=[16, 17], begin_suppress_tokens=[18, 6])
HISTS = ([1, 2, 9, 4], [2, 9, 4], [9, 4], [4], [1, 2, 9, 5], [4, 9], [3], [1, 7, 4, 7, 4, 7, 4], [9, 4, 2, 9, 4])


@pytest.mark.parametrize("V", [wr.V_BIG, wr.V_SMALL])
def test_token_rules_are_hf_bit_for_bit(V):
    """1-, 2-, 3- and 4-id rules that fire or miss by one position, a rule longer than the history, four rules summed on one id, bans with the
    repetition penalty and the n-gram ban, begin-only rules at n_out 0 and 1: processed rows equal HF's bit for bit (fp32)."""
    l = wr.logits_row(21, V)
    for hist in HISTS:
        for n_out in (0, 1, 3):
            if n_out > len(hist):
                continue
            mine = wr.process_row_ext(l, hist, n_out, RULES.repetition_penalty, RULES.no_repeat_ngram_size, RULES.min_new_tokens, 2, RULES.rules)
            hf = hf_processed(l, hist, n_out, RULES)
            assert mine.tobytes() == hf.tobytes(), (V, hist, n_out, np.flatnonzero(mine != hf))
    # the sum on id 6 after [.., 2, 9, 4]: ((0 + 2.5) - 1.25 + 0.3) + 7.0 in fp32, then added once
    x = wr.process_row_ext(l, [1, 2, 9, 4], 3, rules=RULES.rules)
    acc = np.float32(0)
    for b in (2.5, -1.25, 0.3, 7.0):
        acc = np.float32(acc + np.float32(b))
    assert x[6] == np.float32(l[6] + acc) and np.isinf(x[[13, 14, 16, 17]]).all() and x[12] == np.float32(l[12] - np.float32(3.0)) and x[18] == l[18]
    # ids past V are ignored; a row's enable word opts out per kind
    far = LogitsProcessing(sequence_bias={(V + 5,): 1.0}, suppress_tokens=[V, 3])
    x = wr.process_row_ext(l, [1], 0, rules=far.rules)
    assert np.isinf(x[3]) and (np.delete(x, 3) == np.delete(l, 3)).all()
    x = wr.process_row_ext(l, [1, 2, 9, 4], 0, rules=RULES.rules, enable=0b0101)
    assert np.isinf(x[[16, 17]]).all() and np.isfinite(x[[13, 14, 18]]).all() and x[6] == np.float32(l[6] + acc)
    # a row banned to nothing has no finite entry left
    ban_all = LogitsProcessing(suppress_tokens=list(range(37)))
    assert not np.isfinite(wr.process_row_ext(l[:37], [1], 0, rules=ban_all.rules)).any()


# ---- folding and validation ------------------------------------------------------------------------------------------------------------
def test_argument_folding_raises_what_hf_raises():
    from emmax.modeling import EmmaXForActionPrediction as M
    from transformers.generation import logits_process as lp

    rows = [[1, 5, 6]]
    for bad in ({(1, -2): 1.0}, {(): 1.0}, {(1, 2): 1}, {}, [[[1, 2], 3]], {"a": 1.0}):
        with pytest.raises(ValueError):
            lp.SequenceBiasLogitsProcessor(bad)
        with pytest.raises(ValueError):
            M._processing_args(rows, sequence_bias=bad)
    for bad in ([], [[1, -1]], [1, 2], "x"):
        with pytest.raises(ValueError):
            lp.NoBadWordsLogitsProcessor(bad)
        with pytest.raises(ValueError):
            M._processing_args(rows, bad_words_ids=bad)
    with pytest.raises(ValueError):   # (HF builds this processor and fails at its first call: refused here at once)
        M._processing_args(rows, bad_words_ids=[[]])
    for bad in ([-1], [], [1.5], 3):
        with pytest.raises(ValueError):
            M._processing_args(rows, suppress_tokens=bad)
        with pytest.raises(ValueError):
            M._processing_args(rows, begin_suppress_tokens=bad)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            lp.MinPLogitsWarper(bad)
        with pytest.raises(ValueError):
            M._sampling_args(True, min_p=bad)
    for kw in ({"typical_p": 0.0}, {"typical_p": 1.5}, {"epsilon_cutoff": 1.0}, {"epsilon_cutoff": -1e-3}, {"eta_cutoff": 1.0}):
        with pytest.raises(ValueError):
            M._sampling_args(True, **kw)
    # caps: 512 rules, 16 ids per rule, 8192 ids in all
    with pytest.raises(ValueError):
        LogitsProcessing(suppress_tokens=list(range(MAX_RULES + 1)))
    with pytest.raises(ValueError):
        LogitsProcessing(bad_words_ids=[list(range(MAX_RULE_IDS + 1))])
    LogitsProcessing(suppress_tokens=list(range(MAX_RULES)), )
    # what folds: both spellings of sequence_bias, the EOS filter of bad_words_ids, 1-id biases first in the table
    p = M._processing_args(rows, sequence_bias=[[[4, 6], -1.0], [[6], 2.0]], bad_words_ids=[[2], [7, 8]], eos_token_id=2)
    assert p.sequence_bias == (((4, 6), -1.0), ((6,), 2.0)) and p.bad_words_ids == ((7, 8),)
    assert p.rules == [(0, (6,), 2.0), (0, (4, 6), -1.0), (1, (7, 8), 0.0)] and p.rule_enable == 0b0011
    assert M._processing_args(rows, bad_words_ids=[[2]], eos_token_id=2) is None
    s = M._sampling_args(True, seed=3, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=1e-3)
    assert s.warpers == (0.05, 0.9, 3e-4, 1e-3) and s.seed == 3
    torch.manual_seed(0)
    assert M._sampling_args(True, min_p=0.1).min_p == 0.1           # (the drawn seed keeps the warpers)
    assert M._sampling_args(False, min_p=0.1) is None                # greedy ignores them, as it ignores top-k / top-p
    off, ids, flags, bias, en = rule_table([p, LogitsProcessing(), LogitsProcessing(bad_words_ids=[[7, 8]])])
    assert (off, ids, flags, bias, en) == ([0, 1, 3, 5], [6, 4, 6, 7, 8], [0, 0, 1], [2.0, -1.0, 0.0], [3, 0, 2])
    with pytest.raises(ValueError):
        rule_table([p, LogitsProcessing(bad_words_ids=[[9]])])      # one table per session
    assert rule_table([LogitsProcessing(1.2)]) is None


def test_dataclasses_stay_positional_and_neutral():
    s = SamplingParams(0.7, 40, 0.9, 5)
    assert (s.temperature, s.top_k, s.top_p, s.seed) == (0.7, 40, 0.9, 5) and not s.has_warpers and s.warpers == (0.0, 0.0, 0.0, 0.0)
    assert [f for f in SamplingParams.__dataclass_fields__][:4] == ["temperature", "top_k", "top_p", "seed"]
    assert SamplingParams(typical_p=1.0).warpers[1] == 0.0 and SamplingParams(min_p=1.0).has_warpers
    p = LogitsProcessing(1.2, 3, 4)
    assert (p.repetition_penalty, p.no_repeat_ngram_size, p.min_new_tokens) == (1.2, 3, 4) and not p.rules
    assert [f for f in LogitsProcessing.__dataclass_fields__][:3] == ["repetition_penalty", "no_repeat_ngram_size", "min_new_tokens"]
    assert LogitsProcessing().neutral
    for kw in ({"sequence_bias": {(3,): 1.0}}, {"bad_words_ids": [[3]]}, {"suppress_tokens": [3]}, {"begin_suppress_tokens": [3]}):
        assert not LogitsProcessing(**kw).neutral
    assert hash(LogitsProcessing(sequence_bias={(3,): 1.0})) == hash(LogitsProcessing(sequence_bias=[[[3], 1.0]]))


def test_beams_refuse_the_new_processors_before_the_engine():
    from emmax.modeling import EmmaXForActionPrediction as M

    for kw in ({"sequence_bias": {(3,): 1.0}}, {"bad_words_ids": [[3]]}, {"suppress_tokens": [3]}, {"begin_suppress_tokens": [3]}):
        proc = M._processing_args([[1, 2]], **kw)
        assert proc is not None
        with pytest.raises(NotImplementedError):
            M._beam_args(num_beams=4, processing=proc)


# ---- serving on a fake engine ----------------------------------------------------------------------------------------------------------
class FakeExtEngine(FakeStagedEngine):
    """... + the staged setters of the warpers and the rule enables: commit and fork carry a request's words."""

    def __init__(self, plans, lag=2):
        super().__init__(plans, lag)
        self.table, self.row_warp, self.row_en, self.stg_warp, self.stg_en, self.seen, self.cleared = None, {}, {}, {}, {}, {}, []

    def set_processing(self, params, row0=0, n=None):
        pass

    def set_processing_staged(self, params, n=None):
        assert self.in_admission

    def clear_processing(self):
        self.cleared.append("processing")

    def clear_sampling(self):
        super().clear_sampling()
        self.cleared.append("sampling")

    def set_token_rules(self, params, row0=0, n=None, enables=True):
        self.table = rule_table(params)[:4]
        assert not enables

    def set_rule_enables(self, words, row0=0):
        assert self.table is not None
        for i, w in enumerate(words):
            self.row_en[row0 + i] = w

    def set_rule_enables_staged(self, words):
        assert self.in_admission and self.table is not None
        self.stg_en = dict(enumerate(words))

    def set_warpers(self, params, row0=0, n=None):
        for i, p in enumerate(params):
            self.row_warp[row0 + i] = p.warpers

    def set_warpers_staged(self, params, n=None):
        assert self.in_admission
        self.stg_warp = {i: p.warpers for i, p in enumerate(params)}

    def slots_commit(self, handle, slots, staged_idx=None):
        super().slots_commit(handle, slots, staged_idx)
        for slot, i in zip(slots, staged_idx):
            self.row_warp[slot], self.row_en[slot] = self.stg_warp[i], self.stg_en[i]
            self.seen[(self.slots[slot]["rid"], 0)] = (self.row_warp[slot], self.row_en[slot])

    def slots_fork(self, src, dst, params, seeds, subseqs, staged=None):
        super().slots_fork(src, dst, params, seeds, subseqs, staged)
        for d, sb in zip(dst, subseqs):
            self.row_warp[d], self.row_en[d] = self.row_warp[src], self.row_en[src]
            self.seen[(self.slots[d]["rid"], sb)] = (self.row_warp[d], self.row_en[d])


def test_scheduler_carries_per_request_warpers_and_rule_enables():
    from emmax.serving import Request, SlotScheduler

    ban = {"suppress_tokens": [5, 6]}
    reqs = [(0, SamplingParams(1.0, 50, 1.0, 7, min_p=0.05), LogitsProcessing(**ban), 1),
            (1, SamplingParams(0.9, 0, 0.9, 8), None, 1),
            (2, SamplingParams(1.0, 50, 1.0, 9, min_p=0.2, eta_cutoff=1e-3), LogitsProcessing(1.2, sequence_bias={(3,): 1.0}), 3),
            (3, None, LogitsProcessing(sequence_bias={(3,): 1.0}, **ban), 1),
            (4, SamplingParams(1.0, 50, 1.0, 10, typical_p=0.9), LogitsProcessing(1.1), 1),
            (5, SamplingParams(1.0, 50, 1.0, 11, epsilon_cutoff=3e-4), LogitsProcessing(**ban), 1)]
    plans = {(rid, j): [10 * rid + j] * (4 + rid) for rid, _, _, n in reqs for j in range(n)}
    eng = FakeExtEngine(plans)
    sch = SlotScheduler(eng, _encode, n_slots=4, poll_every=1)
    assert sch.overlap
    for rid, s, p, n in reqs:
        sch.submit(Request(rid=rid, frame=rid, prompt_ids=[1, 4], sampling=s, processing=p, num_samples=n))
    res = sch.run()
    assert sorted((r.rid, r.sample) for r in res) == sorted(plans)
    assert eng.table == ([0, 1, 2, 3], [3, 5, 6], [0, 2, 2], [1.0, 0.0, 0.0])   # one table for the run: the bias, then the two bans
    want = {0: ((0.05, 0.0, 0.0, 0.0), 0b0100), 1: ((0.0,) * 4, 0), 2: ((0.2, 0.0, 0.0, 1e-3), 0b0001), 3: ((0.0,) * 4, 0b0101),
            4: ((0.0, 0.9, 0.0, 0.0), 0), 5: ((0.0, 0.0, 3e-4, 0.0), 0b0100)}
    for (rid, sample), got in eng.seen.items():
        assert got == want[rid], (rid, sample, got)
    assert set(eng.seen) == set(plans)                        # every sample of the group of request 2 carries its request's words
    assert eng.cleared == ["processing", "sampling"]          # (the C calls behind them reset the rules and the warpers)
    # a serve without the new fields calls none of the new setters
    eng2 = FakeStagedEngine({(0, 0): [1, 2, 3]})
    sch2 = SlotScheduler(eng2, _encode, n_slots=2, poll_every=1)
    sch2.submit(Request(rid=0, frame=0, prompt_ids=[1, 4], sampling=SamplingParams(1.0, 50, 1.0, 7)))
    assert [r.ids for r in sch2.run()] == [[1, 2, 3]]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_stays_12_with_new_symbols_only():
    from emmax import _lib

    header = open(os.path.join(ROOT, "include", "emmax.h")).read()
    assert "#define EMMAX_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    flat = re.sub(r"\s+", " ", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, flat) and name in _lib.SIGNATURES, name
    # the existing setters keep their prototypes and bindings
    old = {"emmax_op_sample": ("int emmax_op_sample(const float* logits_dev, int ld, int B, int V, const float* temperature_dev, const int32_t* top_k_dev, "
                               "const float* top_p_dev, const uint64_t* seed_dev, const uint32_t* subseq_dev, const int32_t* step_dev, int32_t* tok_out_dev, "
                               "float* logprob_out_dev, emmax_stream stream);", 13),
           "emmax_session_set_sampling": ("int emmax_session_set_sampling(emmax_session* s, int row0, int n, const float* temperature_host, const int32_t* top_k_host, "
                                          "const float* top_p_host, const uint64_t* seed_host, const uint32_t* subseq_host, emmax_stream stream);", 9),
           "emmax_slots_set_sampling_staged": ("int emmax_slots_set_sampling_staged(emmax_session* s, int n, const float* temperature_host, const int32_t* top_k_host, "
                                               "const float* top_p_host, const uint64_t* seed_host, const uint32_t* subseq_host, emmax_stream stream);", 8),
           "emmax_session_set_processing": ("int emmax_session_set_processing(emmax_session* s, int row0, int n, const float* penalty_host, const int32_t* ngram_host, "
                                            "const int32_t* min_new_host, emmax_stream stream);", 7),
           "emmax_slots_set_processing_staged": ("int emmax_slots_set_processing_staged(emmax_session* s, int n, const float* penalty_host, const int32_t* ngram_host, "
                                                 "const int32_t* min_new_host, emmax_stream stream);", 6),
           "emmax_slots_commit": ("int emmax_slots_commit(emmax_session* s, const int32_t* staged_idx_host, const int32_t* slots_host, int n, emmax_stream stream);", 5),
           "emmax_session_clear_sampling": ("int emmax_session_clear_sampling(emmax_session* s, emmax_stream stream);", 2),
           "emmax_session_clear_processing": ("int emmax_session_clear_processing(emmax_session* s, emmax_stream stream);", 2)}
    for name, (proto, nargs) in old.items():
        assert proto in flat, name
        assert len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is C.c_int, name
    if os.path.isfile(_lib.LIB_PATH):   # host-side validation: null and out-of-range arguments are refused before anything launches
        so = _lib.load()
        assert so.emmax_session_set_warpers(None, 0, 1, None, None, None, None, None) != 0
        assert so.emmax_session_set_token_rules(None, 1, None, None, None, None, None) != 0
        assert so.emmax_session_warpers(None) == -1 and so.emmax_session_token_rules(None) == -1
        assert so.emmax_op_sample_ext(None, 37, 1, 37, *([None] * 15), 0, 0, *([None] * 5), 2, 0, None, None, None, None) != 0
