"""Continuous batching for a fleet of cameras: a slot scheduler over the engine's slot-serving C ABI.

The reference answers one request at a time (`generate_actions`, prismatic.py:634-696: bs = 1, always decoded to EOS or
512 new tokens).  Here the decode batch is a set of independent request SLOTS: every slot owns its KV pages, context length,
token budget and stop state on the device; finished slots are refilled (vision encode + prefill, consecutive free slots in one packed pass) while the other
slots keep decoding, so a long reasoning chain never holds short ones back.  With a stop rule (`stop_trigger`,
`stop_after`) a request ends as soon as its action line is complete instead of at EOS -- the emitted ids are exactly the
prefix of the full greedy generation, so the parsed action is unchanged.

There is no shareable prompt prefix to cache across requests: the spliced sequence is [BOS] + 256 patch embeddings +
text[1:] (modeling_prismatic.py:379-384), so everything after BOS depends on the frame.  What CAN be kept is a request's own context: a
request submitted with hold=True keeps its slot when it finishes, and a follow-up request on that context appends its ids to the cached rows
(engine.slot_extend: no frame, no prefill) until the context is released.

The scheduler is host logic only (testable without a GPU against a fake engine); all state it polls lives on the device.
"""
from __future__ import annotations

import dataclasses
import time
from dataclasses import dataclass, field
from typing import Any, Callable, Deque, Dict, List, Optional, Sequence
from collections import deque


@dataclass
class Request:
    """One camera frame + prompt.  `frame` is whatever `encode` accepts (uint8 [H,W,3] tensor on the device)."""
    rid: Any
    frame: Any
    prompt_ids: Sequence[int]
    max_new_tokens: int = 512
    sampling: Any = None   # emmax.sampling.SamplingParams: drawn in the decode step with the request's seed (None: draw_seed()) and subseq 0; None = greedy
    processing: Any = None   # emmax.sampling.LogitsProcessing: HF's repetition penalty / n-gram ban / min-new-tokens in the decode step; None = off
    beams: Any = None        # beam groups are not served as slots: a request with emmax.sampling.BeamParams is refused at submit
    num_samples: int = 1     # > 1: a sample group -- one prefill, forked into num_samples slots that read the prompt's KV pages; sample j draws
                             # with (the request's seed, subseq j), so sample 0 is what the request returns with num_samples = 1.  Needs sampling
    top_logprobs: int = 0    # N in 1..20: every emitted token comes with the N most likely ids and their log-probabilities (RAW logits); 0 = off
    watch_ids: Optional[Sequence[int]] = None   # ... and with the log-probabilities of these ids (up to 256).  One list per run: the requests
                                                # that name a list name the same one
    hold: bool = False       # keep the slot (its KV context) when the request finishes: Result.context names it for a follow-up; it counts
                             # against n_slots until SlotScheduler.release(context)
    follow_up: Any = None    # a Result.context: the request's prompt_ids are appended to that held context (frame = None; the finished answer's
                             # last token is not cached -- pass it first to keep it) and decoding goes on in its slot.  Needs no free slot
    constraint_start: Any = None   # a state or entry name of the scheduler's automaton (SlotScheduler(automaton=...)): the request is decoded
                                   # under that constraint from there; None = unconstrained.  A sample group's samples all enter there
    output_hidden_states: bool = False   # hidden states / attention maps are not served as slots: a request that asks for them is refused at submit
    output_attentions: bool = False


@dataclass
class Result:
    rid: Any
    ids: List[int]
    slot: int
    t_submit: float
    t_admit: float
    t_done: float
    logprobs: Optional[List[float]] = None   # sampled requests: the log-probability of every emitted token
    sample: int = 0   # which sample of its request this is (Request.num_samples > 1: one Result per sample)
    top_logprobs: Optional[List[List[tuple]]] = None   # Request.top_logprobs = N: per emitted token its N (id, logprob) pairs, best first
    watch_logprobs: Optional[List[List[float]]] = None   # Request.watch_ids: per emitted token the log-probabilities of those ids
    context: Any = None   # Request.hold: the held context (opaque: slot + generation counter) for Request(follow_up=...) / SlotScheduler.release

    @property
    def latency_s(self) -> float:
        return self.t_done - self.t_submit


@dataclass(frozen=True)
class HeldContext:
    """What Result.context holds: the slot a finished request kept and the generation counter that tells this hold from later ones of the slot."""
    slot: int
    generation: int


@dataclass
class _Active:
    req: Request
    t_submit: float
    t_admit: float
    sample: int = 0


MAX_SLOTS = 64   # EMMAX_MAX_DECODE_BATCH (emma-x_amd/csrc/kernels.h): rows of a decode step


class SlotScheduler:
    """Greedy slot scheduler.

    engine   object with slots_open / slot_prefill / slots_step / slots_state / slot_output / slot_release / set_stop
             (emmax.engine.EmmaxEngine, or a fake in the CPU tests); slots_fork as well once a request asks for num_samples > 1
             and set_top_logprobs / slot_top_logprobs / clear_top_logprobs once one asks for top_logprobs or watch_ids, and set_automaton /
             set_automaton_starts(_staged) / clear_automaton once one names a constraint_start
    encode   frames (list) -> patch embeddings, one [n_patches, hidden] bf16 tensor per frame; called once per admission
             round with every frame admitted in that round, so the ViT runs batched
    n_slots  decode batch (<= 64; the engine's max_decode_batch())
    poll_every   decode steps between two device polls (a poll is one tiny D2H copy + sync; default 4 = ~13 ms at 7B shapes: a retired
                 slot is refilled within 4 steps -- 32 requests / 8 slots: 22.9 actions/s polling every 16 steps, 24.2 every 4)
    encode_ahead frames encoded per `encode` call: the frames being admitted plus the next ones in the queue, so the ViT
                 always runs at a useful batch (a lone frame costs ~6 ms, eight cost ~8 ms); their patch embeddings wait in
                 `self._embeds` (16 MB for eight 7B-shape frames) until their request is admitted
    automaton    a constraints.TokenAutomaton: the one automaton the run's requests may enter (Request.constraint_start says where; requests
                 without one are unconstrained).  It is set on the session for the runs in which some request names a start
    """

    def __init__(self, engine, encode: Callable[[List[Any]], List[Any]], n_slots: int = 8, poll_every: int = 4,
                 stop_trigger: Sequence[int] = (), stop_after: int = 0, clock: Callable[[], float] = time.perf_counter,
                 encode_ahead: int = 0, overlap: Optional[bool] = None, stage_batch: Optional[int] = None, automaton=None) -> None:
        if not 1 <= n_slots <= MAX_SLOTS:
            raise ValueError(f"n_slots {n_slots} outside 1..{MAX_SLOTS}")
        if poll_every < 1:
            raise ValueError("poll_every must be >= 1")
        self.engine = engine
        self.encode = encode
        self.n_slots = n_slots
        self.poll_every = poll_every
        self.clock = clock
        self.queue: Deque[tuple] = deque()
        self.active: Dict[int, _Active] = {}
        self.results: List[Result] = []
        self.steps = 0
        self.polls = 0
        self.encode_ahead = max(int(encode_ahead), 0)
        self._embeds: Dict[int, Any] = {}          # id(request) -> patch embeddings encoded ahead of admission
        # overlap: admissions (frame encode + prefill) run on the engine's admission stream into staging rows while the occupied
        # slots keep decoding, and join their slots between two decode steps (engine.admission / slots_prefill_staged /
        # slots_commit).  Default: on whenever the engine has the staged API.
        has = all(hasattr(engine, a) for a in ("admission", "slots_prefill_staged", "slots_commit"))
        if overlap and not has:
            raise ValueError("overlap=True needs an engine with admission / slots_prefill_staged / slots_commit")
        self.overlap = has if overlap is None else bool(overlap)
        # requests are staged AHEAD of need, `stage_batch` at a time (default: half the slots), whether or not a slot is free: a slot
        # that retires finds its successor prefilled and is refilled at the same poll
        self.stage_batch = max(1, min(int(stage_batch) if stage_batch else max(1, n_slots // 2), n_slots))
        self._pending = None                         # [staged handle, [(request, t_submit), ...], committed so far] of the staged batch
        self.overlapped_admissions = 0
        self._sampling = False                       # some request of the current run samples (run)
        self._processing = False                     # some request of the current run has logits processing (run)
        self._warpers = False                        # ... min_p / typical_p / epsilon_cutoff / eta_cutoff (run)
        self._rules = False                          # ... token rules (run)
        self._top = None                             # (N, watch list) bound for the current run, None when no request asks (run)
        self.held: Dict[int, int] = {}               # slot -> generation of the context a finished hold=True request keeps there
        self.followups: Deque[tuple] = deque()       # (request, t_submit) of follow-ups: admitted onto their context's slot, no free slot needed
        self._generation = 0
        self.automaton = automaton
        self._constrained = False                    # some request of the current run names a constraint_start (run)
        # a staged batch is at most max(stage_batch, free slots) <= n_slots requests: the session needs that many staging rows
        # (they cost KV pages, so a session only has them when a scheduler asks: engine.ensure_stage_rows re-creates it if needed)
        if self.overlap and hasattr(engine, "ensure_stage_rows"):
            engine.ensure_stage_rows(n_slots)
        engine.set_stop(list(stop_trigger), stop_after)
        if getattr(engine, "beams", 0):   # a beam generation ran on this session: slots are served with beams off
            engine.clear_beams()
        if getattr(engine, "sample_groups", 0):   # ... or a sample-group generation: slots are served with groups off
            engine.clear_sample_groups()
        engine.slots_open(n_slots)

    def submit(self, req: Request) -> None:
        if len(req.prompt_ids) < 1:
            raise ValueError("empty prompt")
        if getattr(req, "output_hidden_states", False) or getattr(req, "output_attentions", False):
            raise NotImplementedError("hidden states / attention maps are not served as request slots (the taps' buffers are a batch's, and slots come "
                                      "and go): use model.generate(..., return_dict_in_generate=True, output_hidden_states=True / output_attentions=True)")
        if getattr(req, "beams", None) is not None:
            raise NotImplementedError("beam search is not served as request slots: a beam group is num_beams rows that reorder together -- "
                                      "use model.generate(num_beams=...) / generate_ids(beams=...)")
        n = getattr(req, "num_samples", 1)
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"num_samples must be an integer >= 1, got {n!r}")
        if n > self.n_slots:
            raise ValueError(f"num_samples {n} exceeds the scheduler's {self.n_slots} slots: a group's samples are admitted together")
        if getattr(req, "hold", False) and n > 1:
            raise ValueError("hold=True keeps ONE context: a sample group (num_samples > 1) shares its prompt pages and is not held")
        if n > 1 and (req.sampling is None or float(req.sampling.temperature) == 0.0):
            raise ValueError(f"num_samples {n} needs sampling: {n} greedy samples of one prompt would be identical (set Request.sampling with a temperature > 0)")
        if getattr(req, "top_logprobs", 0) or getattr(req, "watch_ids", None) is not None:
            from .sampling import check_top_logprobs

            check_top_logprobs(req.top_logprobs, req.watch_ids, None, "Request")
        if getattr(req, "constraint_start", None) is not None:
            if self.automaton is None:
                raise ValueError(f"request {req.rid!r} names a constraint_start, but the scheduler has no automaton (SlotScheduler(automaton=...))")
            self.automaton.start_state(req.constraint_start)   # (validates: a ValueError names the entries)
        if getattr(req, "follow_up", None) is not None:
            self._check_context(req.follow_up, f"request {req.rid!r}: follow_up")
            if n > 1:
                raise ValueError("a follow-up continues ONE context: num_samples > 1 is not served on a held slot")
            if req.frame is not None:
                raise ValueError("a follow-up appends text to a cached context: frame must be None")
            if getattr(req, "processing", None) is not None and not req.processing.neutral:
                raise NotImplementedError("logits processing with a follow-up is outside the hot path: the processors' id history holds a prompt, not the held context")
            if any(r.follow_up == req.follow_up for r, _ in self.followups):
                raise ValueError(f"request {req.rid!r}: another follow-up of this context is already queued")
            self.followups.append((req, self.clock()))
            return
        self.queue.append((req, self.clock()))

    def _check_context(self, ctx, what: str) -> None:
        if not isinstance(ctx, HeldContext) or self.held.get(ctx.slot) != ctx.generation:
            raise ValueError(f"{what} names a released or unknown context (a Result.context of a hold=True request of this scheduler, not yet released)")

    def release(self, context) -> None:
        """Free the slot a hold=True request kept: its context is gone and the slot serves queued requests again."""
        self._check_context(context, "release")
        if any(r.follow_up == context for r, _ in self.followups):
            raise ValueError("a follow-up of this context is still queued")
        self.engine.slot_release(context.slot)
        del self.held[context.slot]

    def _free(self) -> List[int]:
        return [s for s in range(self.n_slots) if s not in self.active and s not in self.held]

    def _admit_followups(self) -> int:
        """Every queued follow-up goes onto its context's slot, between two decode steps: the new ids are appended to the cached rows and the
        slot decodes again.  The other slots are untouched."""
        n = 0
        while self.followups:
            req, t_sub = self.followups.popleft()
            slot = req.follow_up.slot
            self._set_constraint([req], row0=slot)
            self._set_sampling([req], row0=slot)
            try:
                self.engine.slot_extend(slot, list(req.prompt_ids), req.max_new_tokens)
            except Exception:
                # refused (the context has no room for the ids and the budget, say): the request is queued again, its context stays held, and the
                # error reaches the caller, who drops the request (followups.popleft) or releases the context
                self.followups.appendleft((req, t_sub))
                raise
            del self.held[slot]   # active again: its hold (if any) begins anew when it finishes
            self.active[slot] = _Active(req, t_sub, self.clock())
            n += 1
        return n

    def _sampling_rows(self, reqs):
        """(params, seeds, subseqs) of requests about to be prefilled: greedy ones at temperature 0, each request with its own seed and subseq 0."""
        from .sampling import SamplingParams, draw_seed

        params, seeds = [], []
        for r in reqs:
            p = r.sampling if r.sampling is not None else SamplingParams(temperature=0.0, top_k=0, top_p=1.0, seed=0)
            if p.seed is None:
                p = dataclasses.replace(p, seed=draw_seed())
                r.sampling = p   # the seed the request was served with
            params.append(p)
            seeds.append(p.seed)
        return params, seeds, [0] * len(reqs)

    def _set_processing(self, reqs, row0: int = 0, staged: bool = False) -> None:
        """A serve where some request has processing: every prefill is preceded by its rows' processors (neutral ones for the others).
        Other serves call nothing here.  Runs before _set_sampling, so sampling's call still comes right before the prefill."""
        if not self._processing:
            return
        from .sampling import LogitsProcessing

        params = [r.processing if r.processing is not None else LogitsProcessing() for r in reqs]
        if staged:
            self.engine.set_processing_staged(params)
        else:
            self.engine.set_processing(params, row0=row0)
        if self._rules:   # which kinds of the run's rule table each request takes
            words = [p.rule_enable for p in params]
            if staged:
                self.engine.set_rule_enables_staged(words)
            else:
                self.engine.set_rule_enables(words, row0=row0)

    def _set_constraint(self, reqs, row0: int = 0, staged: bool = False) -> None:
        """A serve where some request is constrained: every prefill is preceded by its rows' start states (-1 for the unconstrained ones).
        Other serves call nothing here."""
        if not self._constrained:
            return
        starts = [self.automaton.start_state(getattr(r, "constraint_start", None)) for r in reqs]
        if staged:
            self.engine.set_automaton_starts_staged(starts)
        else:
            self.engine.set_automaton_starts(starts, row0=row0)

    def _set_sampling(self, reqs, row0: int = 0, staged: bool = False) -> None:
        """A serve where some request samples: every prefill is preceded by its rows' parameters.  Greedy-only serves call nothing here."""
        if not self._sampling:
            return
        params, seeds, subs = self._sampling_rows(reqs)
        if staged:
            self.engine.set_sampling_staged(params, seeds, subs)
        else:
            self.engine.set_sampling(params, seeds, subs, row0=row0)
        if self._warpers:   # min_p / typical_p / epsilon_cutoff / eta_cutoff per request (off for the requests without them)
            if staged:
                self.engine.set_warpers_staged(params)
            else:
                self.engine.set_warpers(params, row0=row0)

    @staticmethod
    def _demand(req) -> int:
        return getattr(req, "num_samples", 1)

    def _fit(self, reqs, free: List[int]) -> List[List[int]]:
        """Strict FIFO: the slots of the requests of `reqs` that fit the `free` slots, in order -- request k takes the next num_samples
        free slots (a group needs all its slots at once; nothing overtakes a head that does not fit)."""
        mine, used = [], 0
        for r in reqs:
            if used + self._demand(r) > len(free):
                break
            mine.append(free[used:used + self._demand(r)])
            used += self._demand(r)
        return mine

    def _fork(self, req, slots, t_sub, t_adm, staged=None) -> None:
        """The samples 1.. of a group whose sample 0 was just prefilled into (or committed to) slots[0]: one fork into slots[1:]."""
        p = req.sampling   # (its seed is set: _set_sampling ran before the prefill)
        n = len(slots) - 1
        self.engine.slots_fork(slots[0], slots[1:], [p] * n, [p.seed] * n, list(range(1, n + 1)), staged=staged)
        for j, slot in enumerate(slots[1:], start=1):
            self.active[slot] = _Active(req, t_sub, t_adm, j)

    def _admit(self) -> int:
        free = self._free()
        mine = self._fit((r for r, _ in self.queue), free)   # sample 0 is prefilled into a request's first slot, the others are forked from it
        take = len(mine)
        if take == 0:
            return 0
        batch = [self.queue.popleft() for _ in range(take)]
        embeds = self._encode_for(batch)
        # runs of CONSECUTIVE free slots are prefilled in one packed pass (eight one-row prefills cost ~1.6x one eight-row pass);
        # engines without `slots_prefill` (test doubles) get the requests one by one
        slots = [m[0] for m in mine]
        i = 0
        while i < take:
            j = i + 1
            while j < take and slots[j] == slots[j - 1] + 1 and len(mine[i]) == 1 and len(mine[j]) == 1:
                j += 1
            if j - i > 1 and hasattr(self.engine, "slots_prefill"):
                self._set_processing([batch[k][0] for k in range(i, j)], row0=slots[i])
                self._set_constraint([batch[k][0] for k in range(i, j)], row0=slots[i])
                self._set_sampling([batch[k][0] for k in range(i, j)], row0=slots[i])
                self.engine.slots_prefill(slots[i], [list(batch[k][0].prompt_ids) for k in range(i, j)], embeds[i:j] if embeds[i] is not None else None,
                                          [batch[k][0].max_new_tokens for k in range(i, j)])
            else:
                for k in range(i, j):
                    self._set_processing([batch[k][0]], row0=slots[k])
                    self._set_constraint([batch[k][0]], row0=slots[k])
                    self._set_sampling([batch[k][0]], row0=slots[k])
                    self.engine.slot_prefill(slots[k], list(batch[k][0].prompt_ids), embeds[k], batch[k][0].max_new_tokens)
                    if len(mine[k]) > 1:   # before any decode step: the fork draws from the logit row this prefill left
                        self._fork(batch[k][0], mine[k], batch[k][1], self.clock())
            t_adm = self.clock()
            for k in range(i, j):
                self.active[slots[k]] = _Active(batch[k][0], batch[k][1], t_adm)
            i = j
        return take

    def _encode_for(self, batch) -> List[Any]:
        """Patch embeddings of the requests in `batch` (one ViT pass for those not encoded yet + the head of the queue)."""
        todo = [r for r, _ in batch if id(r) not in self._embeds]
        if todo:
            ahead = [r for r, _ in list(self.queue)[: max(self.encode_ahead - len(todo), 0)] if id(r) not in self._embeds]
            got = self.encode([r.frame for r in todo + ahead])
            if len(got) != len(todo) + len(ahead):
                raise RuntimeError(f"encode returned {len(got)} embeddings for {len(todo) + len(ahead)} frames")
            for r, pe in zip(todo + ahead, got):
                self._embeds[id(r)] = pe
        return [self._embeds.pop(id(r)) for r, _ in batch]

    def _start_admission(self) -> bool:
        """Overlap mode: issue frame encode + staged prefill of the next `stage_batch` queued requests on the admission stream --
        ahead of need, whether or not a slot is free; returns at once (nothing is awaited)."""
        if self._pending is not None or not self.queue:
            return False
        free = len(self._free())
        take = min(len(self.queue), max(self.stage_batch, free))
        batch = [self.queue.popleft() for _ in range(take)]
        try:
            with self.engine.admission():
                embeds = self._encode_for(batch)
                self._set_processing([r for r, _ in batch], staged=True)
                self._set_constraint([r for r, _ in batch], staged=True)
                self._set_sampling([r for r, _ in batch], staged=True)
                staged = self.engine.slots_prefill_staged([list(r.prompt_ids) for r, _ in batch], embeds if embeds[0] is not None else None,
                                                          [r.max_new_tokens for r, _ in batch])
        except Exception:
            # nothing was staged: the requests go back to the head of the queue in their order and the error reaches the caller
            # (they were popped and then neither requeued nor reported)
            for item in reversed(batch):
                self._embeds.pop(id(item[0]), None)
                self.queue.appendleft(item)
            raise
        self._pending = [staged, batch, 0]
        return True

    def _join_admission(self, wait: bool) -> int:
        """Move staged requests into the slots that are free right now, if the staged prefill has finished (wait=True: block for it
        -- the decode batch is idle, there is nothing else to do)."""
        if self._pending is None:
            return 0
        staged, batch, k0 = self._pending
        free = self._free()
        # the longest in-order prefix of what is still staged whose slots are free now (a group is one staged row and num_samples slots)
        mine = self._fit((r for r, _ in batch[k0:]), free)
        take = len(mine)
        if take == 0:
            return 0
        slots = [m[0] for m in mine]
        if not staged.ready():
            if not wait:
                return 0
            staged.wait()
        self.engine.slots_commit(staged, slots, list(range(k0, k0 + take)))
        t_adm = self.clock()
        for k, (m, (req, t_sub)) in enumerate(zip(mine, batch[k0:k0 + take])):
            self.active[m[0]] = _Active(req, t_sub, t_adm)
            if len(m) > 1:   # (the staging row keeps the prompt's logit row until the next staged prefill, which _start_admission issues later)
                self._fork(req, m, t_sub, t_adm, staged=k0 + k)
        self._pending[2] = k0 + take
        if self._pending[2] >= len(batch):
            self._pending = None
        self.overlapped_admissions += 1
        return sum(len(m) for m in mine)

    def _retire(self) -> int:
        done, n_out = self.engine.slots_state()
        self.polls += 1
        n = 0
        for slot in sorted(self.active):
            if done[slot]:
                a = self.active.pop(slot)
                ids = self.engine.slot_output(slot, int(n_out[slot]))
                lps = self.engine.slot_logprobs(slot, int(n_out[slot])) if a.req.sampling is not None else None
                top = watch = None
                n_top, ask_watch = getattr(a.req, "top_logprobs", 0), getattr(a.req, "watch_ids", None) is not None
                if self._top is not None and (n_top or ask_watch):   # the run's binding holds max N pairs per token: this request's first N
                    t_ids, t_lps, w_lps = self.engine.slot_top_logprobs(slot, int(n_out[slot]))
                    if n_top:
                        top = [[(int(i), float(v)) for i, v in zip(ri[:n_top], rv[:n_top])] for ri, rv in zip(t_ids, t_lps)]
                    if ask_watch:
                        watch = [[float(v) for v in row] for row in w_lps]
                ctx = None
                if getattr(a.req, "hold", False):   # the slot stays the request's: a follow-up continues its context
                    self._generation += 1
                    self.held[slot] = self._generation
                    ctx = HeldContext(slot, self._generation)
                else:
                    self.engine.slot_release(slot)
                self.results.append(Result(a.req.rid, ids, slot, a.t_submit, a.t_admit, self.clock(), lps, a.sample, top, watch, ctx))
                n += 1
        return n

    def run(self) -> List[Result]:
        """Serve until the queue is empty and every slot is idle.  Returns the results in completion order.  When some queued request
        samples, the session samples for the whole run (greedy requests at temperature 0: their greedy ids) and is greedy again after it.  Logits processing likewise (requests without it get neutral processors)."""
        everyone = list(self.queue) + list(self.followups)
        self._sampling = any(r.sampling is not None for r, _ in everyone)
        self._processing = any(getattr(r, "processing", None) is not None for r, _ in self.queue)
        if self._processing and self.followups:
            raise NotImplementedError("a run with follow-ups serves no logits processing: the session's processors read an id history that holds "
                                      "prompts only (serve the follow-ups in a run of their own)")
        self._warpers = any(r.sampling is not None and getattr(r.sampling, "has_warpers", False) for r, _ in everyone)
        with_rules = [r.processing for r, _ in self.queue if getattr(r, "processing", None) is not None and getattr(r.processing, "rule_enable", 0)]
        self._rules = bool(with_rules)
        self._constrained = any(getattr(r, "constraint_start", None) is not None for r, _ in everyone)
        self._top = self._top_of_run()
        if self._top is not None:
            self._sampling = True   # the binding reads the logit rows a sampling session writes: greedy requests at temperature 0
        try:
            if self._top is not None:   # bound once for the run, behind sampling on every slot (each admission sets its rows' own again)
                from .sampling import SamplingParams

                greedy = SamplingParams(temperature=0.0, top_k=0, top_p=1.0, seed=0)
                self.engine.set_sampling([greedy] * self.n_slots, [0] * self.n_slots, [0] * self.n_slots, row0=0)
                self.engine.set_top_logprobs(self._top[0], self._top[1], max(int(r.max_new_tokens) for r, _ in everyone))
            if self._rules:   # one rule table for the run (the requests that name a kind name the same rules); every row starts opted out
                self.engine.set_token_rules(with_rules, enables=False)
                self.engine.set_rule_enables([0] * self.n_slots)
            if self._constrained:   # one automaton for the run; every row starts unconstrained, each admission sets its rows' starts
                self.engine.set_automaton(self.automaton)
                self.engine.set_automaton_starts([-1] * self.n_slots)
            return self._run()
        finally:
            if self._constrained:
                self.engine.clear_automaton()
                self._constrained = False
            if self._top is not None:
                self.engine.clear_top_logprobs()
                self._top = None
            if self._processing:
                self.engine.clear_processing()
            if self._sampling:
                self.engine.clear_sampling()

    def _top_of_run(self):
        """(N, watch list) the run binds: N = the largest top_logprobs a queued request asks for (each Result is trimmed to its own), and the
        one watch list the requests name -- two different lists are a ValueError, as two rule tables are.  None: no request asks, and the
        run calls no engine method it did not call before."""
        n, watch = 0, None
        for r, _ in list(self.queue) + list(self.followups):
            n = max(n, int(getattr(r, "top_logprobs", 0) or 0))
            w = getattr(r, "watch_ids", None)
            if w is not None:
                w = [int(i) for i in w]
                if watch is not None and w != watch:
                    raise ValueError(f"request {r.rid!r} names a watch list that differs from another request's: a run serves one list")
                watch = w
        return None if n == 0 and not watch else (n, watch or [])

    def _run(self) -> List[Result]:
        if self.overlap:
            while self.queue or self.active or self._pending is not None or self.followups:
                self._admit_followups()
                self._start_admission()
                if self._join_admission(wait=not self.active):   # (idle decode batch: the admission is all there is to wait for)
                    self._start_admission()                       # staging rows free again: the next batch goes out at once
                if not self.active:
                    self._check_not_stuck()
                    continue
                self.engine.slots_step(self.poll_every)
                self.steps += self.poll_every
                self._retire()
            return self.results
        while self.queue or self.active or self.followups:
            self._admit_followups()
            self._admit()
            if not self.active:
                self._check_not_stuck()
                continue
            self.engine.slots_step(self.poll_every)
            self.steps += self.poll_every
            self._retire()
        return self.results


    def _check_not_stuck(self) -> None:
        """Nothing decodes: requests that wait while every slot they could take is HELD would wait for ever."""
        waiting = [r for r, _ in self.queue] + ([r for r, _ in self._pending[1][self._pending[2]:]] if self._pending is not None else [])
        if waiting and len(self._free()) < self._demand(waiting[0]):
            raise RuntimeError(f"{len(waiting)} requests wait but {len(self.held)} of the {self.n_slots} slots are held and none decodes: "
                               "release a held context (SlotScheduler.release) or serve with more slots")


def serve_static(engine_generate: Callable[[List[Request]], List[List[int]]], requests: Sequence[Request], batch: int) -> List[List[int]]:
    """The baseline the scheduler is measured against: fixed batches, each decoded until its slowest row is done."""
    out: List[List[int]] = []
    for i in range(0, len(requests), batch):
        out.extend(engine_generate(list(requests[i:i + batch])))
    return out


def stop_rule_from_tokenizer(tokenizer, marker: str = "POLICIES:", n_after: int = 8) -> tuple:
    """(trigger_ids, n_after) for `SlotScheduler(stop_trigger=..., stop_after=...)` / `engine.set_stop`.

    The Solver reads the action from the first line after `marker` (policy_parser.Solver.extract_action_policies, reference
    prismatic/vla/solver.py:107-137): a leading space token plus the 7 action-bin tokens, i.e. 8 ids.

    The marker is tokenised IN CONTEXT -- as it appears in generated text, right after a newline ("...MOVEMENT:\n..\nPOLICIES:\n"):
    a SentencePiece / LLaMA tokenizer given the bare string prepends its dummy prefix (`▁POL...`, or a lone 29871 `▁`), pieces
    that never occur after `\n` in running text, so a bare-string trigger would never fire and every request would run to EOS.
    Here "\n" + marker is encoded and everything up to and including the last id of the encoding of "\n" alone is dropped;
    the result is what the model actually emits for the marker.  At most 16 ids (the device-side matcher's capacity)."""
    def enc(text):
        ids = tokenizer(text, add_special_tokens=False)["input_ids"]
        return [int(t) for t in (ids[0] if ids and isinstance(ids[0], (list, tuple)) else ids)]

    head, full = enc("\n"), enc("\n" + marker)
    k = 0
    while k < len(head) and k < len(full) and head[k] == full[k]:
        k += 1
    ids = full[k:]
    if not 1 <= len(ids) <= 16:
        raise ValueError(f"marker {marker!r} tokenises to {len(ids)} ids in context; the stop rule takes 1..16")
    return ids, int(n_after)
