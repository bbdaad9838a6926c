"""Seeded temperature / top-k / top-p sampling over rows of logits on the device (include/emmax.h: emmax_op_sample; the kernel:
emma-x_amd/csrc/sample.hip).

The defaults of SamplingParams are the HF GenerationConfig defaults (temperature 1.0, top-k 50, top-p 1.0).  A draw is reproducible
from its (seed, subseq, step): the noise of token id i is word i % 4 of Philox4x32-10 with key = seed and counter (i / 4, step, subseq, 0),
whatever the batch.  Temperature 0 is the argmax.  With the engine's cached step this makes a sampling loop::

    toks, lps = sample_logits(engine.last_logits(), params, seeds, steps=[t] * B)
    engine.set_current_tokens(toks.tolist()); engine.decode_step()
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

_U64 = (1 << 64) - 1
MAX_VOCAB = 32768   # EMMAX_SAMPLE_MAX_V (emma-x_amd/csrc/kernels.h): entries of one row


@dataclass(frozen=True)
class SamplingParams:
    temperature: float = 1.0   # finite, >= 0; 0 = greedy (top_k / top_p ignored)
    top_k: int = 50            # 0 = off
    top_p: float = 1.0         # (0, 1]; 1 = off
    seed: Optional[int] = None   # 64-bit; None = drawn from torch's default CPU generator (draw_seed)
    # the further warpers (include/emmax.h: emmax_session_set_warpers), in HF's order behind top_p; the defaults are off
    min_p: float = 0.0           # [0, 1]; 0 = off
    typical_p: float = 1.0       # (0, 1]; 1 = off
    epsilon_cutoff: float = 0.0  # [0, 1); 0 = off
    eta_cutoff: float = 0.0      # [0, 1); 0 = off

    def __post_init__(self):
        t = float(self.temperature)
        if not math.isfinite(t) or t < 0.0:
            raise ValueError(f"temperature must be finite and >= 0, got {self.temperature}")
        if int(self.top_k) != self.top_k or int(self.top_k) < 0:
            raise ValueError(f"top_k must be an integer >= 0, got {self.top_k}")
        p = float(self.top_p)
        if not (0.0 < p <= 1.0):
            raise ValueError(f"top_p must lie in (0, 1], got {self.top_p}")
        if self.seed is not None and not (0 <= int(self.seed) <= _U64):
            raise ValueError(f"seed must be a 64-bit unsigned integer, got {self.seed}")
        if not (0.0 <= float(self.min_p) <= 1.0):
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {self.min_p}")
        if not (0.0 < float(self.typical_p) <= 1.0):
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1 (1 = off), but is {self.typical_p}")
        if not (0.0 <= float(self.epsilon_cutoff) < 1.0):
            raise ValueError(f"`epsilon_cutoff` has to be a float > 0 and < 1 (0 = off), but is {self.epsilon_cutoff}")
        if not (0.0 <= float(self.eta_cutoff) < 1.0):
            raise ValueError(f"`eta_cutoff` has to be a float > 0 and < 1 (0 = off), but is {self.eta_cutoff}")

    @property
    def warpers(self) -> Tuple[float, float, float, float]:
        """(min_p, typical_p, epsilon_cutoff, eta_cutoff) as the device takes them: 0 = off."""
        t = float(self.typical_p)
        return float(self.min_p), 0.0 if t == 1.0 else t, float(self.epsilon_cutoff), float(self.eta_cutoff)

    @property
    def has_warpers(self) -> bool:
        return any(w != 0.0 for w in self.warpers)


MAX_NGRAM = 32   # EMMAX_MAX_NGRAM (emma-x_amd/csrc/kernels.h): the largest no_repeat_ngram_size
MAX_RULES, MAX_RULE_IDS, MAX_RULE_TOTAL = 512, 16, 8192   # EMMAX_MAX_RULES / _RULE_IDS / _RULE_TOTAL: the caps of a session's token-rule table
RULE_BIAS, RULE_BAD_WORDS, RULE_SUPPRESS, RULE_BEGIN_SUPPRESS = 0, 1, 2, 3   # rule kinds = bits of a row's enable word


def _is_id(t) -> bool:
    return isinstance(t, (int, np.integer)) and not isinstance(t, bool) and t >= 0


def fold_sequence_bias(sequence_bias) -> Optional[tuple]:
    """HF's `sequence_bias` ({tuple(ids): float} or [[ids, float], ...]) -> ((ids, bias), ...), with SequenceBiasLogitsProcessor's errors."""
    if sequence_bias is None:
        return None
    sb = sequence_bias
    if isinstance(sb, tuple) and all(isinstance(e, tuple) and len(e) == 2 and isinstance(e[0], tuple) for e in sb) and len(sb) > 0:
        sb = {e[0]: e[1] for e in sb}   # (already folded)
    if not isinstance(sb, (dict, list)) or len(sb) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sequence_bias}.")
    if isinstance(sb, list):
        if any(not isinstance(e, (list, tuple)) or len(e) != 2 or not isinstance(e[0], list) or len(e[0]) == 0 or not all(_is_id(t) for t in e[0])
               or not isinstance(e[1], float) for e in sb):
            raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is {sequence_bias}.")
        sb = {tuple(e[0]): e[1] for e in sb}
    if any(not isinstance(k, tuple) for k in sb):
        raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sequence_bias}.")
    if any(len(k) == 0 or not all(_is_id(t) for t in k) for k in sb):
        raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sequence_bias}.")
    if any(not isinstance(b, float) for b in sb.values()):
        raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sequence_bias}.")
    if any(math.isnan(b) for b in sb.values()):
        raise ValueError(f"`sequence_bias` values must not be NaN, but is {sequence_bias}.")
    return tuple((tuple(int(t) for t in k), float(b)) for k, b in sb.items())


def fold_bad_words(bad_words_ids, eos_token_id=None) -> Optional[tuple]:
    """HF's `bad_words_ids` -> (ids, ...), with NoBadWordsLogitsProcessor's errors; a lone EOS id is dropped as HF drops it."""
    if bad_words_ids is None:
        return None
    bw = [list(w) if isinstance(w, tuple) else w for w in bad_words_ids] if isinstance(bad_words_ids, tuple) else bad_words_ids
    if not isinstance(bw, list) or len(bw) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
    if any(not isinstance(w, list) for w in bw):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad_words_ids}.")
    if any(not all(_is_id(t) for t in w) for w in bw):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad_words_ids}.")
    if any(len(w) == 0 for w in bw):
        raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of positive integers, but is {bad_words_ids}.")
    eos = [] if eos_token_id is None else [int(e) for e in (eos_token_id if isinstance(eos_token_id, (list, tuple)) else [eos_token_id])]
    out, seen = [], set()
    for w in bw:
        t = tuple(int(x) for x in w)
        if (len(t) == 1 and t[0] in eos) or t in seen:
            continue
        seen.add(t)
        out.append(t)
    return tuple(out) if out else None


def fold_suppress(tokens, name: str) -> Optional[tuple]:
    """HF's `suppress_tokens` / `begin_suppress_tokens` -> (id, ...)."""
    if tokens is None:
        return None
    if not isinstance(tokens, (list, tuple)) or len(tokens) == 0 or not all(_is_id(t) for t in tokens):
        raise ValueError(f"`{name}` has to be a non-empty list of non-negative integers, but is {tokens}.")
    return tuple(dict.fromkeys(int(t) for t in tokens))


@dataclass(frozen=True)
class LogitsProcessing:
    """HF generate's repetition_penalty / no_repeat_ngram_size / min_new_tokens, applied in the decode step before the warpers
    (include/emmax.h: emmax_session_set_processing).  The defaults are HF's neutral values: processing off."""
    repetition_penalty: float = 1.0   # finite, > 0; 1 = off
    no_repeat_ngram_size: int = 0     # 0 = off, <= MAX_NGRAM
    min_new_tokens: int = 0           # EOS is banned while fewer tokens were emitted
    # the token rules (include/emmax.h: emmax_session_set_token_rules), folded to tuples (fold_*; HF's spellings are accepted and checked
    # as HF checks them); None = off.  A session holds one table: the rows that name a kind name the same rules
    sequence_bias: Optional[tuple] = None           # ((ids, bias), ...): bias added to ids[-1] when the history ends with ids[:-1]
    bad_words_ids: Optional[tuple] = None           # (ids, ...): the same match with -inf
    suppress_tokens: Optional[tuple] = None         # (id, ...): -inf at every step
    begin_suppress_tokens: Optional[tuple] = None   # (id, ...): -inf for the first generated token only

    def __post_init__(self):
        object.__setattr__(self, "sequence_bias", fold_sequence_bias(self.sequence_bias))
        object.__setattr__(self, "bad_words_ids", fold_bad_words(self.bad_words_ids))
        object.__setattr__(self, "suppress_tokens", fold_suppress(self.suppress_tokens, "suppress_tokens"))
        object.__setattr__(self, "begin_suppress_tokens", fold_suppress(self.begin_suppress_tokens, "begin_suppress_tokens"))
        rules = self.rules
        if len(rules) > MAX_RULES or any(len(ids) > MAX_RULE_IDS for _, ids, _ in rules) or sum(len(ids) for _, ids, _ in rules) > MAX_RULE_TOTAL:
            raise ValueError(f"token rules: at most {MAX_RULES} rules of at most {MAX_RULE_IDS} ids, {MAX_RULE_TOTAL} ids in all "
                             f"(got {len(rules)} rules, {sum(len(ids) for _, ids, _ in rules)} ids)")
        p = float(self.repetition_penalty)
        if not math.isfinite(p) or not p > 0.0:
            raise ValueError(f"repetition_penalty must be a finite float > 0, got {self.repetition_penalty}")
        n = self.no_repeat_ngram_size
        if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= MAX_NGRAM:
            raise ValueError(f"no_repeat_ngram_size must be an integer in 0..{MAX_NGRAM}, got {n}")
        m = self.min_new_tokens
        if isinstance(m, bool) or int(m) != m or int(m) < 0:
            raise ValueError(f"min_new_tokens must be an integer >= 0, got {m}")

    @property
    def neutral(self) -> bool:
        """No processor would change a row (HF adds none for these values)."""
        return float(self.repetition_penalty) == 1.0 and int(self.no_repeat_ngram_size) == 0 and int(self.min_new_tokens) == 0 and not self.rules

    @property
    def rules(self) -> list:
        """The rows of the device table, [(kind, ids, bias)]: sequence_bias with its 1-id rules first (HF adds those first), then
        bad_words_ids, suppress_tokens, begin_suppress_tokens."""
        sb = list(self.sequence_bias or ())
        out = [(RULE_BIAS, ids, b) for ids, b in sb if len(ids) == 1] + [(RULE_BIAS, ids, b) for ids, b in sb if len(ids) > 1]
        out += [(RULE_BAD_WORDS, ids, 0.0) for ids in self.bad_words_ids or ()]
        out += [(RULE_SUPPRESS, (t,), 0.0) for t in self.suppress_tokens or ()]
        out += [(RULE_BEGIN_SUPPRESS, (t,), 0.0) for t in self.begin_suppress_tokens or ()]
        return out

    @property
    def rule_enable(self) -> int:
        """The row's enable word: bit k set iff the row names rules of kind k."""
        return sum(1 << k for k, f in enumerate((self.sequence_bias, self.bad_words_ids, self.suppress_tokens, self.begin_suppress_tokens)) if f)


def rule_table(params: Sequence[LogitsProcessing]):
    """The one table of a session whose rows have `params`, and each row's enable word: (offsets, ids, flags, bias, enables), or None when
    no row names a rule.  The rows that name a kind must name the same rules (a session holds one table)."""
    fields = ("sequence_bias", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens")
    chosen = {}
    for p in params:
        for f in fields:
            v = getattr(p, f)
            if v and chosen.setdefault(f, v) != v:
                raise ValueError(f"rows of one session name different `{f}`: a session holds one rule table (rows opt in or out of it)")
    if not chosen:
        return None
    rules = LogitsProcessing(**chosen).rules
    off, ids, flags, bias = [0], [], [], []
    for kind, r, b in rules:
        ids += list(r)
        off.append(len(ids))
        flags.append(kind | (4 if kind == RULE_BEGIN_SUPPRESS else 0))
        bias.append(float(b))
    return off, ids, flags, bias, [p.rule_enable for p in params]


MAX_BEAMS = 8   # EMMAX_MAX_BEAMS (include/emmax.h)
MAX_DECODE_BATCH = 64   # EMMAX_MAX_DECODE_BATCH: rows of a decode step on any model (a model's own limit: engine.max_decode_batch())


@dataclass(frozen=True)
class BeamParams:
    """HF generate's beam search arguments (do_sample = False), run inside the decode step on shared KV pages (include/emmax.h:
    emmax_session_set_beams).  The checks are GenerationConfig.validate's."""
    num_beams: int = 2                  # 2 .. MAX_BEAMS (1 is not a beam run: it takes the greedy path)
    length_penalty: float = 1.0         # finite; hypotheses are ranked by score / length ** length_penalty
    early_stopping: Union[bool, str] = False   # False, True or "never"
    num_return_sequences: int = 1       # <= num_beams, best first

    def __post_init__(self):
        k = self.num_beams
        if isinstance(k, bool) or not isinstance(k, int) or not 2 <= k <= MAX_BEAMS:
            raise ValueError(f"num_beams must be an integer in 2..{MAX_BEAMS}, got {k}")
        lp = self.length_penalty
        if isinstance(lp, bool) or not isinstance(lp, (int, float)) or not math.isfinite(float(lp)):
            raise ValueError(f"length_penalty must be a finite float, got {lp}")
        es = self.early_stopping
        if not (es is True or es is False or es == "never"):
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {es}.")
        n = self.num_return_sequences
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"num_return_sequences must be an integer >= 1, got {n}")
        if n > k:
            raise ValueError(f"`num_return_sequences` ({n}) has to be smaller or equal to `num_beams` ({k}).")


def draw_seed(generator: Optional[torch.Generator] = None) -> int:
    """A 64-bit seed from `generator` (default: torch's global CPU generator, so torch.manual_seed(s) fixes it)."""
    hi = int(torch.randint(0, 1 << 32, (1,), generator=generator, dtype=torch.int64))
    lo = int(torch.randint(0, 1 << 32, (1,), generator=generator, dtype=torch.int64))
    return (hi << 32) | lo


def _per_row(v, B: int, what: str) -> list:
    vals = list(v) if isinstance(v, (list, tuple, range)) else [v] * B
    if len(vals) != B:
        raise ValueError(f"{what}: {len(vals)} values for {B} rows")
    return vals


def sample_logits(logits: torch.Tensor, params: Union[SamplingParams, Sequence[SamplingParams]], seeds=None, subseqs=0, steps=0,
                  generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Draw one token per row of `logits` (fp32 [B, V] on the device, V <= 32768, rows contiguous) on the current stream.
    params: one SamplingParams for all rows or one per row; seeds / subseqs / steps: one value for all rows or one per row (seeds default to
    each row's SamplingParams.seed, else a draw from `generator`).  Returns (tokens int32 [B], log-probabilities fp32 [B]) on the device:
    the log-probability is log_softmax(logits)[token] (T = 1, unfiltered)."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.device.type != "cuda":
        raise ValueError("sample_logits: logits must be a 2-D float32 tensor on a HIP device")
    B, V = logits.shape
    if B < 1 or not 1 <= V <= MAX_VOCAB:
        raise ValueError(f"sample_logits: {B} rows of {V} entries (1..{MAX_VOCAB})")
    if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < V):
        logits = logits.contiguous()
    ld = logits.stride(0) if B > 1 else V
    ps = _per_row(params, B, "params")
    if not all(isinstance(p, SamplingParams) for p in ps):
        raise ValueError("sample_logits: params must be SamplingParams")
    if seeds is None:
        seeds = [p.seed if p.seed is not None else draw_seed(generator) for p in ps]
    seeds = [int(s) & _U64 for s in _per_row(seeds, B, "seeds")]
    subseqs = [int(s) & 0xFFFFFFFF for s in _per_row(subseqs, B, "subseqs")]
    steps = [int(s) for s in _per_row(steps, B, "steps")]
    if any(not 0 <= s < 1 << 31 for s in steps):
        raise ValueError("sample_logits: steps must lie in 0 .. 2^31 - 1")
    dev = logits.device
    temp = torch.tensor([float(p.temperature) for p in ps], dtype=torch.float32).to(dev)
    top_k = torch.tensor([min(int(p.top_k), V) for p in ps], dtype=torch.int32).to(dev)
    top_p = torch.tensor([float(p.top_p) for p in ps], dtype=torch.float32).to(dev)
    seed_t = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64).to(dev)
    sub_t = torch.tensor([s - (1 << 32) if s >= 1 << 31 else s for s in subseqs], dtype=torch.int32).to(dev)
    step_t = torch.tensor(steps, dtype=torch.int32).to(dev)
    tok = torch.empty(B, dtype=torch.int32, device=dev)
    lp = torch.empty(B, dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.emmax_op_sample(logits.data_ptr(), ld, B, V, temp.data_ptr(), top_k.data_ptr(), top_p.data_ptr(), seed_t.data_ptr(),
                                   sub_t.data_ptr(), step_t.data_ptr(), tok.data_ptr(), lp.data_ptr(), _lib.current_stream()), "emmax_op_sample")
    return tok, lp


MAX_TOP_LOGPROBS = 20   # include/emmax.h: EMMAX_MAX_TOP_LOGPROBS
MAX_WATCH_IDS = 256     # include/emmax.h: EMMAX_MAX_WATCH_IDS (the model's n_action_bins)


def check_top_logprobs(n, watch_ids, vocab: Optional[int] = None, who: str = "top_logprobs") -> Tuple[int, list]:
    """(N, watch list) as the library takes them, checked on the host: 0 <= N <= MAX_TOP_LOGPROBS (and <= vocab), at most MAX_WATCH_IDS ids,
    each an integer in [0, vocab); None is no watch list.  Duplicates are allowed."""
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MAX_TOP_LOGPROBS:
        raise ValueError(f"{who}: top_logprobs must be an integer in 0..{MAX_TOP_LOGPROBS}, got {n!r}")
    if vocab is not None and n > vocab:
        raise ValueError(f"{who}: top_logprobs {n} exceeds the {vocab} entries of a row")
    ids = [] if watch_ids is None else list(watch_ids)
    if len(ids) > MAX_WATCH_IDS:
        raise ValueError(f"{who}: {len(ids)} watch ids (at most {MAX_WATCH_IDS})")
    for i in ids:
        if isinstance(i, bool) or not isinstance(i, int) or i < 0 or (vocab is not None and i >= vocab):
            raise ValueError(f"{who}: watch id {i!r} is not an integer in 0..{'' if vocab is None else vocab - 1}")
    return n, ids


def top_logprobs(logits: torch.Tensor, n: int, watch_ids: Optional[Sequence[int]] = None):
    """Top-n and watched-token log-probabilities of every row of `logits` (fp32 [B, V] on the device, V <= 32768) on the current stream
    (include/emmax.h: emmax_op_top_logprobs).  Returns (top_ids int32 [B, n], top_logprobs fp32 [B, n], watch_logprobs fp32 [B, W]) on the
    device: the n entries that are not NaN with the largest values, best first, equal values by the lower id, as (id, log_softmax(row)[id]);
    places past the entries that are not NaN hold (-1, -inf); and log_softmax(row)[watch_ids]."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.device.type != "cuda":
        raise ValueError("top_logprobs: logits must be a 2-D float32 tensor on a HIP device")
    B, V = logits.shape
    if B < 1 or not 1 <= V <= MAX_VOCAB:
        raise ValueError(f"top_logprobs: {B} rows of {V} entries (1..{MAX_VOCAB})")
    n, ids = check_top_logprobs(n, watch_ids, V)
    if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < V):
        logits = logits.contiguous()
    ld = logits.stride(0) if B > 1 else V
    dev = logits.device
    W = len(ids)
    top_ids = torch.empty(B, n, dtype=torch.int32, device=dev)
    top_lp = torch.empty(B, n, dtype=torch.float32, device=dev)
    watch_lp = torch.empty(B, W, dtype=torch.float32, device=dev)
    if n == 0 and W == 0:
        return top_ids, top_lp, watch_lp
    ids_t = torch.tensor(ids, dtype=torch.int32).to(dev) if W else None
    lib = _lib.load()
    _lib.check(lib.emmax_op_top_logprobs(logits.data_ptr(), ld, B, V, n, top_ids.data_ptr() if n else None, top_lp.data_ptr() if n else None, W,
                                         ids_t.data_ptr() if W else None, watch_lp.data_ptr() if W else None, _lib.current_stream()),
               "emmax_op_top_logprobs")
    return top_ids, top_lp, watch_lp
