"""Sample groups as request slots, host side (no GPU): Request.num_samples through the slot scheduler against fake engines modelled on
tests/test_serving.py's, the new C symbols in header / ctypes table / library, and the inputs of tests/test_slot_groups_gpu.py fixed with the
fp32 oracle so that "the samples diverged" and "half of the steps are compared" are properties of the inputs.

The fake engine mimics the device-side contract of include/emmax.h: a slot emits one token per decode step until its planned length or its
budget; emmax_slots_fork needs a source whose prefill (or commit) no decode step has followed, idle destinations, and sampling on."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slot_groups_ref as sr  # noqa: E402
from conftest import ID_BUDGET_EXACT, ID_BUDGET_TINY, ROOT  # noqa: E402
from emmax.sampling import BeamParams, SamplingParams  # noqa: E402
from emmax.serving import Request, Result, SlotScheduler  # noqa: E402

NEW_SYMBOLS = ("emmax_slots_fork", "emmax_slots_page_state")


class FakeEngine:
    """plans: (rid, sample) -> the ids that sample would emit.  `log` records every call that matters for ordering."""

    def __init__(self, plans):
        self.plans, self.slots, self.log, self.steps = plans, {}, [], 0
        self.sampling_on, self.row_params, self.fresh = False, {}, set()

    def set_stop(self, trig, n_after):
        pass

    def slots_open(self, n):
        self.slots = {s: None for s in range(n)}

    def set_sampling(self, params, seeds=None, subseqs=None, row0=0, n=None, generator=None):
        self.sampling_on = True
        for i, (p, sd, sb) in enumerate(zip(params, seeds, subseqs)):
            self.row_params[row0 + i] = (p, sd, sb)

    def clear_sampling(self):
        self.sampling_on = False

    def _state(self, rid, sample, budget):
        plan = self.plans[(rid, sample)]
        return {"plan": plan, "budget": budget, "out": [plan[0]], "rid": rid, "sample": sample}

    def slot_prefill(self, slot, ids, pe, max_new):
        assert self.slots[slot] is None, "prefill into a busy slot"
        sub = self.row_params[slot][2] if self.sampling_on else 0
        assert sub == 0, "a request's own prefill draws with subseq 0"
        self.slots[slot] = self._state(pe["rid"], 0, max_new)
        self.fresh.add(slot)
        self.log.append(("prefill", slot, pe["rid"]))

    def slots_fork(self, src, dst, params, seeds, subseqs, staged=None):
        assert self.sampling_on, "a fork needs sampling"
        st = self.slots[src]
        assert st is not None and src in self.fresh, "the source's logit row is gone"
        assert len(dst) == len(params) == len(seeds) == len(subseqs) >= 1 and len(set(dst)) == len(dst) and src not in dst
        assert list(subseqs) == list(range(1, len(dst) + 1)) and all(sd == self.src_seed(src) for sd in seeds)
        for d, sb in zip(dst, subseqs):
            assert self.slots[d] is None, "fork into a busy slot"
            self.slots[d] = self._state(st["rid"], sb, st["budget"])
        self.log.append(("fork", src, tuple(dst), staged))

    def src_seed(self, src):
        return self.row_params[src][1]

    def _done(self, st):
        return len(st["out"]) >= min(len(st["plan"]), st["budget"])

    def slots_step(self, k):
        self.steps += k
        self.fresh.clear()
        self.log.append(("step", k))
        for _ in range(k):
            for st in self.slots.values():
                if st is not None and not self._done(st):
                    st["out"].append(st["plan"][len(st["out"])])

    def slots_state(self):
        return ([1 if (st is None or self._done(st)) else 0 for st in self.slots.values()],
                [0 if st is None else len(st["out"]) for st in self.slots.values()])

    def slot_output(self, slot, n):
        return list(self.slots[slot]["out"][:n])

    def slot_logprobs(self, slot, n):
        return [-1.0] * n

    def slot_release(self, slot):
        self.log.append(("release", slot))
        self.slots[slot] = None


class FakeStagedEngine(FakeEngine):
    """... + overlapped admission: a staged batch is ready `lag` decode steps after it was issued; a commit leaves the request's logit row in
    its staging row until the next staged prefill."""

    def __init__(self, plans, lag=2):
        super().__init__(plans)
        self.lag, self.in_admission, self.staged, self.staged_params, self.committed_from = lag, False, None, {}, {}

    def admission(self):
        eng = self

        class Ctx:
            def __enter__(self):
                eng.in_admission = True

            def __exit__(self, *a):
                eng.in_admission = False

        return Ctx()

    def set_sampling_staged(self, params, seeds=None, subseqs=None, n=None, generator=None):
        assert self.in_admission and all(sb == 0 for sb in subseqs)
        self.sampling_on = True
        self.staged_params = {i: (p, sd, sb) for i, (p, sd, sb) in enumerate(zip(params, seeds, subseqs))}

    def slots_prefill_staged(self, prompts, embeds, max_new):
        assert self.in_admission and self.staged is None
        eng, due = self, self.steps + self.lag

        class H:
            n = len(prompts)

            def ready(self):
                return eng.steps >= due

            def wait(self):
                eng.steps = max(eng.steps, due)

        self.committed_from = {}   # the staging rows' logit rows are the new batch's
        self.staged = (H(), [self._state(pe["rid"], 0, b) for pe, b in zip(embeds, max_new)])
        self.log.append(("staged", len(prompts)))
        return self.staged[0]

    def slots_commit(self, handle, slots, staged_idx=None):
        h, sts = self.staged
        assert h is handle and h.ready() and not self.in_admission and len(slots) == len(staged_idx) >= 1
        for slot, i in zip(slots, staged_idx):
            assert self.slots[slot] is None and sts[i] is not None
            self.slots[slot], sts[i] = sts[i], None
            self.row_params[slot] = self.staged_params[i]
            self.committed_from[slot] = i
            self.log.append(("commit", slot, self.slots[slot]["rid"]))
        if all(st is None for st in sts):
            self.staged = None

    def slots_fork(self, src, dst, params, seeds, subseqs, staged=None):
        if staged is not None:
            assert self.committed_from.get(src) == staged, "the staged request's logit row is gone"
            self.fresh.add(src)
        super().slots_fork(src, dst, params, seeds, subseqs, staged)


def _encode(frames):
    return [{"rid": f} for f in frames]


def _samp(seed=7, t=1.0):
    return SamplingParams(t, 0, 1.0, seed=seed)


def _plans(spec):
    """spec: rid -> (num_samples, length): sample j of request rid emits 1000 rid + 100 j + t"""
    return {(rid, j): [1000 * rid + 100 * j + t for t in range(n)] for rid, (k, n) in spec.items() for j in range(k)}


def test_num_samples_is_checked_at_submit():
    sch = SlotScheduler(FakeEngine({}), _encode, n_slots=4)
    for bad in (0, -1, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="num_samples"):
            sch.submit(Request(0, 0, [1, 2], sampling=_samp(), num_samples=bad))
    with pytest.raises(ValueError, match=r"num_samples 5 .* 4 slots"):
        sch.submit(Request(0, 0, [1, 2], sampling=_samp(), num_samples=5))
    with pytest.raises(ValueError, match="greedy"):
        sch.submit(Request(0, 0, [1, 2], num_samples=2))
    with pytest.raises(ValueError, match="greedy"):
        sch.submit(Request(0, 0, [1, 2], sampling=_samp(t=0.0), num_samples=2))
    with pytest.raises(NotImplementedError, match="beam"):   # the existing refusal comes first
        sch.submit(Request(0, 0, [1, 2], beams=BeamParams(2), num_samples=2))
    assert not sch.queue
    sch.submit(Request(0, 0, [1, 2], sampling=_samp(), num_samples=4))   # as many samples as slots is served
    sch.submit(Request(1, 1, [1, 2], num_samples=1))                     # a greedy single is what it was
    assert len(sch.queue) == 2
    assert Request(0, 0, [1]).num_samples == 1 and Result(0, [], 0, 0.0, 0.0, 0.0).sample == 0


def _run(engine_cls, spec, order, n_slots, **kw):
    plans = _plans(spec)
    eng = engine_cls(plans)
    sch = SlotScheduler(eng, _encode, n_slots=n_slots, poll_every=1, **kw)
    for rid in order:
        k = spec[rid][0]
        sch.submit(Request(rid, rid, [1, 5, rid + 3], sampling=_samp(seed=50 + rid) if k > 1 or rid % 2 else None, num_samples=k))
    return eng, sch, plans, sch.run()


@pytest.mark.parametrize("engine_cls", [FakeEngine, FakeStagedEngine])
def test_a_group_waits_for_all_its_slots_and_nothing_overtakes_it(engine_cls):
    """4 slots: singles 0 and 1 (long and short), a 3-sample request 2, a single 3 behind it.  Request 2 needs 3 free slots: it is admitted
    only once request 1 has retired (slots 1, 2, 3 free), although two slots were free all along, and request 3 does not overtake it."""
    spec = {0: (1, 30), 1: (1, 4), 2: (3, 6), 3: (1, 2), 4: (2, 5)}
    eng, sch, plans, res = _run(engine_cls, spec, [0, 1, 2, 3, 4], 4)
    assert sch.overlap == (engine_cls is FakeStagedEngine)
    got = {(r.rid, r.sample): r.ids for r in res}
    assert got == plans and len(res) == len(plans)                      # every sample completes, with its own Result.sample
    assert all(r.logprobs is not None for r in res if spec[r.rid][0] > 1)
    # the group's admission comes after request 1's release; request 3 is admitted after the group
    admit = {e[2]: i for i, e in enumerate(eng.log) if e[0] in ("prefill", "commit")}
    rel = [i for i, e in enumerate(eng.log) if e[0] == "release"]
    slot_of_1 = next(e[1] for e in eng.log if e[0] in ("prefill", "commit") and e[2] == 1)
    rel_1 = next(i for i in rel if eng.log[i][1] == slot_of_1)
    assert admit[0] < admit[1] < rel_1 < admit[2] < admit[3] < admit[4]
    forks = [e for e in eng.log if e[0] == "fork"]
    assert [len(f[2]) for f in forks] == [2, 1]                         # one fork per group, of num_samples - 1 slots
    three = forks[0]
    assert sorted((three[1],) + three[2]) == [1, 2, 3]                   # slot 0 still holds the long single
    assert {r.slot for r in res if r.rid == 2} == {1, 2, 3}


@pytest.mark.parametrize("engine_cls", [FakeEngine, FakeStagedEngine])
def test_one_fork_per_group_right_behind_its_prefill_and_samples_released_one_by_one(engine_cls):
    spec = {0: (3, 9), 1: (2, 3), 2: (1, 5), 3: (3, 4)}
    eng, sch, plans, res = _run(engine_cls, spec, [0, 1, 2, 3], 6)
    assert {(r.rid, r.sample): r.ids for r in res} == plans
    forks = [i for i, e in enumerate(eng.log) if e[0] == "fork"]
    assert len(forks) == 3
    for i in forks:
        src = eng.log[i][1]
        # between the source's prefill / commit and its fork: no decode step (other admissions may sit there)
        back = next(j for j in range(i - 1, -1, -1) if eng.log[j][0] in ("prefill", "commit") and eng.log[j][1] == src)
        assert all(e[0] != "step" for e in eng.log[back:i])
        assert (eng.log[i][3] is not None) == (engine_cls is FakeStagedEngine)
    # every sample's slot is released on its own, once
    rel = [e[1] for e in eng.log if e[0] == "release"]
    assert len(rel) == len(plans) == len(res)
    # the samples of request 0 have one length here, those of a group with ragged lengths retire at different polls
    plans2 = {(0, 0): [1, 2, 3, 4, 5, 6, 7], (0, 1): [8], (0, 2): [9, 10, 11]}
    eng2 = engine_cls(plans2)
    sch2 = SlotScheduler(eng2, _encode, n_slots=3, poll_every=1)
    sch2.submit(Request(0, 0, [1, 2], sampling=_samp(), num_samples=3))
    res2 = sch2.run()
    assert [r.sample for r in res2] == [1, 2, 0] and [r.ids for r in res2] == [[8], [9, 10, 11], [1, 2, 3, 4, 5, 6, 7]]
    steps_at_release = [sum(e[1] for e in eng2.log[:i] if e[0] == "step") for i, e in enumerate(eng2.log) if e[0] == "release"]
    assert steps_at_release == sorted(steps_at_release) and len(set(steps_at_release)) == 3


def test_an_engine_without_fork_serves_single_sample_traffic_unchanged():
    """The scheduler calls slots_fork only for num_samples > 1: test doubles and engines without it keep working."""

    class NoFork(FakeEngine):
        slots_fork = None

        def __getattribute__(self, name):
            if name == "slots_fork":
                raise AttributeError(name)
            return object.__getattribute__(self, name)

    spec = {i: (1, n) for i, n in enumerate([5, 12, 3, 8, 2, 9])}
    eng, sch, plans, res = _run(NoFork, spec, list(spec), 3)
    assert not hasattr(eng, "slots_fork")
    assert {(r.rid, r.sample): r.ids for r in res} == plans and all(r.sample == 0 for r in res)
    assert [e[0] for e in eng.log].count("fork") == 0


def test_new_symbols_are_declared_bound_and_exported():
    from emmax import _lib

    header = open(os.path.join(ROOT, "include", "emmax.h")).read()
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    so = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(so, name), name
    assert re.search(r"#define EMMAX_ABI_VERSION 12\b", header) and _lib.ABI_VERSION == 12 and so.emmax_abi_version() == 12
    assert so.emmax_slots_fork(None, 0, -1, None, 1, None, None, None, None, None, None) != 0   # null session: refused on the host
    assert so.emmax_slots_page_state(None, None, None, None) != 0


@pytest.fixture(scope="module")
def oracle_weights():
    from emmax.config import EmmaXConfig
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    return cfg, {k: v.to(torch.bfloat16).float() for k, v in synthetic_state_dict(cfg, seed=sr.WEIGHT_SEED).items()}


@pytest.mark.parametrize("name", list(sr.FORK))
def test_pinned_inputs_make_the_samples_of_the_group_diverge(oracle_weights, name):
    """For the prompt, temperature and seed of every engine-level GPU case: the step-0 reference draws of the N samples that clear the id
    line of the tiny configuration hold at least two distinct tokens, so a device within the budget draws diverging samples at step 0."""
    cfg, sd_ref = oracle_weights
    draws = sr.fork_step0(name, cfg, sd_ref, ID_BUDGET_TINY)
    print(name, draws)
    assert len(draws) == sr.N
    assert len({tok for tok, clear in draws if clear}) >= 2, draws
    frame, row, p = sr.fork_inputs(name)
    assert (256 + len(row)) % 64 == {"ctx64": 0, "ctx63": 63, "cross": 50}[name] and p.temperature > 0


def test_pinned_workload_leaves_half_of_the_steps_to_compare(oracle_weights):
    """The scheduler-level GPU test compares ids up to each sample's first step below the exact-numerics id line.  By the oracle alone (its
    own chains, the reference draw): at least half of all emitted steps lie before that step, every multi-sample request samples, and the
    samples of every group differ at step 0 or 1."""
    from oracle import emmax_oracle as orc

    cfg, sd_ref = oracle_weights
    total = clear = 0
    wl = sr.workload()
    assert {k for _, _, k, _, _ in wl} == {1, 2, 3} and sum(1 for _, _, k, p, _ in wl if p is None and k == 1) >= 2
    for i, (frame, row, k, p, budget) in enumerate(wl):
        patches = sr.oracle_patches(orc, cfg, sd_ref, frame)
        chains = [sr.oracle_chain(orc, cfg, sd_ref, patches, row, p, j, budget) for j in range(k)]
        for j, (ids, L) in enumerate(chains):
            total += len(ids)
            clear += sr.clear_steps(L, ids, p, j, ID_BUDGET_EXACT)
        if k > 1:
            assert len({tuple(ids[:2]) for ids, _ in chains}) == k, (i, [ids[:2] for ids, _ in chains])
    print("clear", clear, "of", total)
    assert 2 * clear >= total
