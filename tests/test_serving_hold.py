"""Held contexts in the slot scheduler (emmax/serving.py: Request(hold=True), Request(follow_up=...), SlotScheduler.release) against a fake
engine: no GPU, no HIP library.  The fake mimics the slot C ABI plus emmax_slot_extend: a follow-up lands on a slot whose request has
finished and was not released, and the slot then emits the follow-up's plan."""
import pytest

from emmax.serving import HeldContext, Request, SlotScheduler


class FakeEngine:
    def __init__(self, plans):
        self.plans = plans            # rid-keyed: the ids the "model" would emit to EOS
        self.slots = {}
        self.prefills, self.extends, self.released, self.log = [], [], [], []

    def set_stop(self, trig, n_after):
        pass

    def slots_open(self, n):
        self.slots = {s: None for s in range(n)}

    @staticmethod
    def _done(st):
        return len(st["out"]) >= min(len(st["plan"]), st["budget"])

    def slot_prefill(self, slot, ids, pe, max_new):
        assert self.slots[slot] is None, "prefill into a busy (or held) slot"
        rid = pe["rid"]
        self.slots[slot] = {"plan": self.plans[rid], "budget": max_new, "out": [self.plans[rid][0]], "rid": rid, "ctx": list(ids)}
        self.prefills.append((slot, rid))
        self.log.append(("prefill", slot, rid))

    def slot_extend(self, slot, ids, max_new):
        st = self.slots[slot]
        assert st is not None and self._done(st), "a follow-up extends a finished, unreleased request"
        rid = ("f", st["rid"], len(self.extends))
        plan = self.plans[("follow", tuple(ids))]
        self.slots[slot] = {"plan": plan, "budget": max_new, "out": [plan[0]], "rid": rid, "ctx": st["ctx"] + st["out"][:-1] + list(ids)}
        self.extends.append((slot, tuple(ids)))
        self.log.append(("extend", slot, tuple(ids)))

    def slots_step(self, k):
        for _ in range(k):
            for st in self.slots.values():
                if st is not None and not self._done(st):
                    st["out"].append(st["plan"][len(st["out"])])

    def slots_state(self):
        return ([1 if (st is None or self._done(st)) else 0 for st in self.slots.values()], [0 if st is None else len(st["out"]) for st in self.slots.values()])

    def slot_output(self, slot, n):
        return list(self.slots[slot]["out"][:n])

    def slot_release(self, slot):
        self.released.append(slot)
        self.log.append(("release", slot))
        self.slots[slot] = None


def encode(frames):
    return [{"rid": f} for f in frames]


def plans(lengths):
    return {i: [100 * i + t for t in range(n)] for i, n in enumerate(lengths)}


def test_a_held_slot_is_kept_and_not_refilled():
    p = plans([4, 9, 3, 6, 5])
    eng = FakeEngine(p)
    sch = SlotScheduler(eng, encode, n_slots=3, poll_every=1)
    for i in range(5):
        sch.submit(Request(i, i, [1, i + 3], max_new_tokens=64, hold=i in (0, 2)))
    res = {r.rid: r for r in sch.run()}
    assert {k: r.ids for k, r in res.items()} == p
    held = {res[0].context, res[2].context}
    assert all(isinstance(c, HeldContext) for c in held) and res[1].context is None and res[3].context is None
    assert {c.slot for c in held} == set(sch.held) and len(sch.held) == 2
    # the two held slots were prefilled exactly once; requests 3 and 4 went through the one slot left
    per_slot = {}
    for slot, rid in eng.prefills:
        per_slot.setdefault(slot, []).append(rid)
    assert per_slot[res[0].context.slot] == [0] and per_slot[res[2].context.slot] == [2]
    assert sorted(eng.released) == sorted(r.slot for r in res.values() if r.context is None)
    assert all(eng.slots[c.slot] is not None for c in held)   # still there


def test_follow_up_lands_on_its_slot_and_release_frees_it_for_the_queue():
    p = plans([5, 7, 30])
    p[("follow", (4, 8, 9))] = [900 + t for t in range(6)]
    p[("follow", (904, 11))] = [950 + t for t in range(3)]
    eng = FakeEngine(p)
    sch = SlotScheduler(eng, encode, n_slots=2, poll_every=2)
    sch.submit(Request(0, 0, [1, 5], max_new_tokens=64, hold=True))
    sch.submit(Request(1, 1, [1, 6], max_new_tokens=64))
    first = {r.rid: r for r in sch.run()}
    ctx = first[0].context
    # a follow-up while another request decodes: it needs no free slot, and the other slot's output is its own
    sch.results.clear()
    sch.submit(Request(2, 2, [1, 7], max_new_tokens=64))
    sch.submit(Request("why", None, [4, 8, 9], max_new_tokens=64, follow_up=ctx, hold=True))
    second = {r.rid: r for r in sch.run()}
    assert second["why"].ids == p[("follow", (4, 8, 9))] and second["why"].slot == ctx.slot and second[2].ids == p[2] and second[2].slot != ctx.slot
    assert eng.extends == [(ctx.slot, (4, 8, 9))]
    assert eng.log.index(("extend", ctx.slot, (4, 8, 9))) < eng.log.index(("prefill", second[2].slot, 2))   # the follow-up waits for no slot
    # the old context is gone (a new generation of the same slot): following it up again is refused, the new one works
    ctx2 = second["why"].context
    assert ctx2.slot == ctx.slot and ctx2 != ctx
    with pytest.raises(ValueError, match="released or unknown"):
        sch.submit(Request("stale", None, [3], follow_up=ctx))
    sch.results.clear()
    sch.submit(Request("again", None, [904, 11], max_new_tokens=64, follow_up=ctx2))   # not held any more afterwards
    third = sch.run()
    assert [r.ids for r in third] == [p[("follow", (904, 11))]] and third[0].context is None
    assert ctx.slot in eng.released and not sch.held


def test_release_frees_a_held_slot_for_a_queued_request():
    p = plans([3, 4, 6])
    eng = FakeEngine(p)
    sch = SlotScheduler(eng, encode, n_slots=1, poll_every=1)
    sch.submit(Request(0, 0, [1, 2], max_new_tokens=64, hold=True))
    (r0,) = sch.run()
    sch.submit(Request(1, 1, [1, 3], max_new_tokens=64))
    with pytest.raises(RuntimeError, match="held"):   # every slot is held and nothing decodes: the queued request would wait for ever
        sch.run()
    assert len(sch.queue) == 1 and eng.prefills == [(0, 0)]
    sch.release(r0.context)
    assert eng.released == [0] and not sch.held
    sch.results.clear()
    (r1,) = sch.run()
    assert r1.rid == 1 and r1.ids == p[1] and r1.slot == 0
    with pytest.raises(ValueError, match="released or unknown"):
        sch.release(r0.context)


def test_a_refused_follow_up_stays_queued_and_its_context_held():
    p = plans([3])
    p[("follow", (5, 6))] = [40, 41]
    eng = FakeEngine(p)
    sch = SlotScheduler(eng, encode, n_slots=1, poll_every=1)
    sch.submit(Request(0, 0, [1, 2], max_new_tokens=8, hold=True))
    (r0,) = sch.run()
    real, calls = eng.slot_extend, []

    def no_room(slot, ids, max_new):
        calls.append(slot)
        raise RuntimeError("context + new ids + tokens to generate exceed max_ctx")

    eng.slot_extend = no_room
    req = Request(1, None, [5, 6], max_new_tokens=8, follow_up=r0.context)
    sch.submit(req)
    with pytest.raises(RuntimeError, match="max_ctx"):
        sch.run()
    # nothing is lost: the request is at the head of the follow-up queue again, its context is still held, no slot became active
    assert calls == [r0.context.slot] and [r for r, _ in sch.followups] == [req] and sch.held == {r0.context.slot: r0.context.generation} and not sch.active
    eng.slot_extend = real
    sch.results.clear()
    (r1,) = sch.run()                                            # the caller fixed what was wrong: the same request is served
    assert r1.rid == 1 and r1.ids == [40, 41] and not sch.held


def test_refusals_at_submit():
    from emmax.sampling import LogitsProcessing, SamplingParams

    eng = FakeEngine(plans([3]))
    sch = SlotScheduler(eng, encode, n_slots=2, poll_every=1)
    with pytest.raises(ValueError, match="released or unknown"):
        sch.submit(Request(9, None, [3], follow_up=HeldContext(0, 1)))            # never handed out
    with pytest.raises(ValueError, match="released or unknown"):
        sch.submit(Request(9, None, [3], follow_up=(0, 1)))                       # not a context at all
    with pytest.raises(ValueError, match="hold"):
        sch.submit(Request(9, 0, [1, 2], hold=True, num_samples=2, sampling=SamplingParams(temperature=1.0, top_k=0, top_p=1.0, seed=1)))
    sch.submit(Request(0, 0, [1, 2], max_new_tokens=8, hold=True))
    (r,) = sch.run()
    with pytest.raises(ValueError, match="frame"):
        sch.submit(Request(1, 0, [3], follow_up=r.context))
    with pytest.raises(NotImplementedError, match="processing"):
        sch.submit(Request(1, None, [3], follow_up=r.context, processing=LogitsProcessing(repetition_penalty=1.3)))
    with pytest.raises(ValueError, match="empty"):
        sch.submit(Request(1, None, [], follow_up=r.context))
    eng.plans[("follow", (3,))] = [7, 8]
    sch.submit(Request(1, None, [3], follow_up=r.context))
    with pytest.raises(ValueError, match="already queued"):
        sch.submit(Request(2, None, [3], follow_up=r.context))
    with pytest.raises(ValueError, match="still queued"):
        sch.release(r.context)
    assert not eng.extends   # nothing reached the engine
