"""Host reference of the constrained finish (include/emmax.h: emmax_session_set_automaton / emmax_op_sample_constrained; the kernel:
emma-x_amd/csrc/sample_kernel.h, ConFinishParams): a numpy replay.  The automaton's mask is one more ban, so the replay masks the processed row
and hands it to the existing replays -- warpers_ref.process_row_ext before the mask (biases, repetition penalty, the other bans: they commute
with it), warpers_ref.sample_row_ext after it (top-k / top-p, the warpers, the draw).  The log-probability is that of the RAW row.

The committed rows (committed_rows) are warpers_ref's logit rows at three vocabulary sizes under one shared automaton whose eight states
keep different sets; tests/test_constraint.py holds every one of them to warpers_ref's margin lines under the mask, so that no row is
skipped on the GPU."""
import numpy as np

import warpers_ref as wr
from emmax import constraints as ct

SIZES = (wr.V_SMALL, 32000, 32768)   # 37: no multiple of 4, one block of lanes; 32000: the model's; 32768: the kernel's cap (every register)

# (T, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff) of the eight rows of a batch: greedy, plain, top-k, top-p, warper sets
CASES = (
    (0.0, 0, 1.0, 0.0, 0.0, 0.0, 0.0),
    (1.0, 0, 1.0, 0.0, 0.0, 0.0, 0.0),
    (1.0, 50, 1.0, 0.0, 0.0, 0.0, 0.0),
    (0.9, 0, 0.9, 0.0, 0.0, 0.0, 0.0),
    (0.0, 0, 1.0, 0.0, 0.0, 0.0, 0.0),
    wr.CASES[8],
    (1.0, 0, 1.0, 0.05, 0.0, 0.0, 0.0),
    wr.CASES[9],
)
# the logit-row seed of row b, at every size: each such row clears warpers_ref's lines under state b's mask (tests/test_constraint.py checks it)
ROW_SEEDS = (0, 100, 200, 300, 400, 500, 600, 700)


def make_automaton(V):
    """Eight states with different kept sets, one shared table.  State k < 4 keeps the ids with (i + k) % 5 != 0; state k >= 4 keeps a range
    that shrinks from both ends.  An even id moves the row to the next state (mod 8), an odd one leaves it, and id V - 1 ends the row."""
    ids = np.arange(V)
    trans = {}
    for k in range(8):
        keep = (ids + k) % 5 != 0 if k < 4 else (ids >= (k - 3) * V // 16) & (ids < V - (k - 4) * V // 16)
        ok = ids[keep]
        trans[k] = [(ok[ok % 2 == 0], (k + 1) % 8), (ok[ok % 2 == 1], k)] + ([([V - 1], ct.DONE)] if keep[V - 1] else [])
    return ct.from_transitions(V, trans, entry={"start": 0})


def mask_row(x, aut, state):
    """The processed row under the automaton's mask: -inf at the ids `state` forbids (state -1: unconstrained)."""
    return np.where(aut.allowed(int(state)), x, np.float32(-np.inf)).astype(np.float32)


def constrained_row(logits, aut, state, hist=(1,), n_out=0, penalty=1.0, ngram=0, min_new=0, eos_id=2, rules=(), enable=15):
    """One raw fp32 logit row through the processors (warpers_ref.process_row_ext: HF's order) and the mask."""
    return mask_row(wr.process_row_ext(logits, list(hist), n_out, penalty, ngram, min_new, eos_id, rules, enable), aut, state)


def raw_logprob(logits, tok):
    l64 = np.asarray(logits, dtype=np.float64)
    m = l64.max()
    return float(l64[tok] - (m + np.log(np.exp(l64 - m).sum())))


def sample_constrained(logits, aut, state, case, seed, subseq, step, pad_id=0, **proc):
    """(token, raw log-probability, next state, margin, scores, dead) of one row.  A row with no finite entry left emits pad_id and keeps its
    state (dead); otherwise the state moves on the emitted token (-1: the row is done after it)."""
    row = constrained_row(logits, aut, state, n_out=step, **proc)
    if not (row > -np.inf).any():
        return pad_id, None, int(state), np.inf, row, True
    tok, _, margin, keep, sc = wr.sample_row_ext(row, case, seed, subseq, step)
    if not case[0] > 0:   # greedy: the margin is the gap between the two largest entries (ties go to the lowest id: no margin needed)
        margin = np.inf
    return tok, raw_logprob(logits, tok), aut.step(int(state), tok), margin, sc, False


def clears(logits, aut, state, case, seed, subseq, step, **proc):
    """The row's decisions under the mask clear warpers_ref's lines and its draw the Gumbel margin."""
    row = constrained_row(logits, aut, state, n_out=step, **proc)
    if not case[0] > 0:
        return bool((row > -np.inf).any())
    info = wr.kept_set_ext(row, *case)[2]
    return wr.clears(info) and wr.sample_row_ext(row, case, seed, subseq, step)[2] > wr.MARGIN


def row_params(b):
    """(seed, subseq, step) of row b of a committed batch"""
    return 2000 + b, b % 3, b


def committed_rows(V):
    """[(b, logits, state, case)]: the eight rows of the batch at vocabulary size V; row b is in state b."""
    return [(b, wr.logits_row(ROW_SEEDS[b], V), b, CASES[b]) for b in range(8)]
