"""Sample groups as request slots on a real MI355X (include/emmax.h: emmax_slots_fork; the fork kernel in emma-x_amd/csrc/misc.hip,
run_slots_fork in step.hip, the release handover in generate.hip; Request.num_samples in emmax/serving.py).

Tiny configuration throughout (256 patch rows: context = 256 + prompt ids).  The inputs come from tests/slot_groups_ref.py;
tests/test_slot_groups.py shows on the CPU, with the fp32 oracle, that the samples of every group must diverge and that half of the
scheduler workload's steps lie above the id line -- both are properties of the inputs.
  1. FORKED IS BIT-EQUAL TO UNFORKED, on the device alone: a group of 3 served by one prefill + one fork against 3 single prefills of the
     same request into the same slots with subseq 0, 1, 2 -- same batch width, same slot positions, same kernels, only the page ids behind
     the prompt differ: ids, log-probability bits and last-logits bits at every step;
  2. through the scheduler against one-row generates with (seed, subseq j), blocking and overlapped admission;
  3. the handover: every release order of {owner, follower, follower} with the owner's slot overwritten by an unrelated request;
  4. the page-state invariant (table + hidden = a permutation) after the fork, every release, and the calls that end slot serving;
  5. the refusals, each decided on the host with the page state untouched."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_groups_ref as sg  # noqa: E402
import slot_groups_ref as sr  # noqa: E402
from conftest import ID_BUDGET_EXACT  # noqa: E402

pytestmark = pytest.mark.gpu

N_SLOTS, SRC, FOLLOW, OTHERS, SPARE = 6, 2, [4, 1], [0, 3], 5   # the followers are named out of order and are no neighbours of the source
MEMBERS = [SRC] + FOLLOW                                       # sample j sits in MEMBERS[j]
BUDGET = 40
MODES = ["default", "graph", "exact", "fp8w", "kv8"]
ERR_INVALID, ERR_STATE = -1, -5


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def models(device):
    """One tiny model per numerics mode, built on first use and shared by the tests of this file."""
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    made = {}

    def get(mode):
        if mode not in made:
            cfg = EmmaXConfig.tiny()
            if mode == "fp8w":
                cfg.decode_weight_dtype = "fp8"
            sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=sr.WEIGHT_SEED).items()}
            with _lib.tuning(kv_fp8=int(mode == "kv8")):   # (the KV format is read when the session is created: the capacity is never outgrown)
                made[mode] = EmmaXForActionPrediction(cfg, dict(sd)).to(device, max_batch=N_SLOTS, max_prompt=64, max_ctx=256 + 64 + BUDGET + 9,
                                                                        exact=mode == "exact")
        return made[mode]

    yield get
    made.clear()
    torch.cuda.empty_cache()


def _others(eng, device):
    """Two unrelated requests (one sampled, one greedy) and an unrelated LONG prompt for a slot a release freed."""
    from emmax.sampling import SamplingParams

    frames, rows = sg.inputs("indep")
    pe = eng.vision_encode(torch.from_numpy(frames).to(device))
    rng = np.random.default_rng(4242)
    long_row = [1] + [int(x) for x in rng.integers(3, 31744, size=61)]
    reqs = [(rows[0], pe[0], SamplingParams(sg.T0["indep"], 0, 1.0, seed=77)), (rows[1], pe[1], SamplingParams(0.0, 0, 1.0, seed=0))]
    return reqs, (long_row, pe[2], SamplingParams(0.0, 0, 1.0, seed=0))


def _last_logits(eng, slots):
    from emmax import _lib

    out = torch.empty(N_SLOTS, eng.cfg.llm.vocab_size, dtype=torch.float32, device=eng.device)
    _lib.check(eng.lib.emmax_last_logits(eng._session, out.data_ptr(), _lib.current_stream()), "emmax_last_logits")
    return _bits(out[slots].cpu().numpy())


def _read(eng, slot):
    done, n_out = eng.slots_state()
    n = int(n_out[slot])
    return eng.slot_output(slot, n), _bits(eng.slot_logprobs(slot, n)).tolist(), int(done[slot])


def _prefill(eng, slot, row, pe, p, subseq):
    eng.set_sampling([p], [p.seed], [subseq], row0=slot)
    eng.slot_prefill(slot, row, pe, BUDGET)


def _serve(model, device, case, forked, schedule, on_fork=None, on_release=None):
    """One serve of the group of `case` in slots MEMBERS beside the two unrelated requests.  forked: one prefill + one fork; else three
    single prefills with subseq 0, 1, 2.  schedule: ("step", k) | ("release", j) (sample j) | ("refill",) (the long prompt into the slot
    released last).  Returns (last-logit bits of every occupied slot after every step, {slot: (ids, log-probability bits, done)} read at
    each slot's release or at the end)."""
    eng = model.engine
    frame, row, p = sr.fork_inputs(case)
    pe = eng.vision_encode(torch.from_numpy(frame).to(device))[0]
    others, refill = _others(eng, device)
    eng.slots_open(N_SLOTS)
    for slot, (r, e, q) in zip(OTHERS, others):
        _prefill(eng, slot, r, e, q, 0)
    if forked:
        _prefill(eng, SRC, row, pe, p, 0)
        eng.slots_fork(SRC, FOLLOW, [p] * len(FOLLOW), [p.seed] * len(FOLLOW), list(range(1, sr.N)))
        if on_fork:
            on_fork(eng)
    else:
        for j, slot in enumerate(MEMBERS):
            _prefill(eng, slot, row, pe, p, j)
    holds = {slot: ("slot", slot) for slot in OTHERS}   # what every occupied slot holds: a sample of the group, or an unrelated request
    holds.update({slot: ("sample", j) for j, slot in enumerate(MEMBERS)})
    logits, final, last = [], {}, None
    for op in schedule:
        if op[0] == "step":
            for _ in range(op[1]):
                eng.slots_step(1)
                logits.append((tuple(sorted(holds)), _last_logits(eng, sorted(holds))))
        elif op[0] == "release":
            last = MEMBERS[op[1]]
            final[holds.pop(last)] = _read(eng, last)
            eng.slot_release(last)
            if on_release:
                on_release(eng, last)
        else:
            _prefill(eng, last, refill[0], refill[1], refill[2], 0)
            holds[last] = ("slot", last)
    for slot in sorted(holds):
        final[holds[slot]] = _read(eng, slot)
    for slot in sorted(holds):
        eng.slot_release(slot)
        if on_release and holds[slot][0] == "sample":
            on_release(eng, slot)
    eng.clear_sampling()
    return logits, final


def _assert_equal_serves(a, b):
    (la, fa), (lb, fb) = a, b
    assert len(la) == len(lb) and sorted(fa) == sorted(fb)
    for key in fa:
        assert fa[key][0] == fb[key][0], (key, fa[key][0], fb[key][0])          # ids
        assert fa[key][1] == fb[key][1], key                                      # log-probability bits
        assert fa[key][2] == fb[key][2], key
    for t, ((sa, xa), (sb, xb)) in enumerate(zip(la, lb)):
        assert sa == sb and np.array_equal(xa, xb), f"last logits differ at step {t + 1} (slots {sa})"


@pytest.mark.parametrize("case", list(sr.FORK))
@pytest.mark.parametrize("mode", MODES)
def test_forked_is_bit_equal_to_unforked(device, models, tune, mode, case):
    """Contexts 256 + 64 (no copy), 256 + 63 and 256 + 50 (the partial page is copied; 24 steps from remainder 50 take every sample across a
    page boundary onto its own pages), in default numerics eager and replayed, exact numerics, fp8 decode weights and the fp8 KV cache (four
    planes through the copy)."""
    model = models(mode)
    if mode == "graph":
        tune(graph=1)
    schedule = [("step", sr.FORK[case])]
    forked = _serve(model, device, case, True, schedule)
    if mode == "graph":
        assert model.engine.graph_active()
    plain = _serve(model, device, case, False, schedule)
    _assert_equal_serves(forked, plain)
    ids = [forked[1][("sample", j)][0] for j in range(sr.N)]
    print(mode, case, [i[:3] for i in ids])
    assert all(len(i) >= 2 for i in ids) and len({tuple(i[:2]) for i in ids}) >= 2, ids   # the samples diverged (tests/test_slot_groups.py: by the inputs)
    if case == "cross":
        assert max(len(i) for i in ids) >= 15                                             # past the page boundary at 14 new tokens


def _roles_checker(nfull):
    """on_fork / on_release callbacks that follow the group's membership on the host and check the page-state invariant on the device:
    a follower's first nfull entries are the owner's and its own pages are hidden; everything else is a row's own and hides nothing; the
    owned entries are a permutation of all page ids (so no slot outside the group references a shared page)."""
    state = {"owner": SRC, "followers": set(FOLLOW)}

    def check(eng):
        table, hidden = (x.numpy() for x in eng.slots_page_state())
        rows, mp = table.shape
        assert rows >= N_SLOTS and nfull < mp
        owned = []
        for r in range(rows):
            for i in range(mp):
                if r in state["followers"] and i < nfull:
                    assert table[r, i] == table[state["owner"], i] and hidden[r, i] >= 0, (r, i)
                    owned.append(int(hidden[r, i]))
                else:
                    assert hidden[r, i] == -1, (r, i, hidden[r, i])
                    owned.append(int(table[r, i]))
        assert sorted(owned) == list(range(rows * mp))
        return table, hidden

    def on_release(eng, slot):
        if slot == state["owner"]:
            state["owner"] = min(state["followers"]) if state["followers"] else None   # the heir: the lowest-numbered live follower
            state["followers"].discard(state["owner"])
        else:
            state["followers"].discard(slot)
        check(eng)

    return check, on_release, state


@pytest.mark.parametrize("order", list(itertools.permutations(range(sr.N))))
def test_handover_in_every_release_order(device, models, order):
    """5 steps, release sample order[0] and at once prefill an unrelated long prompt into its slot (which overwrites the pages that slot
    holds now), 20 steps, release order[1], 5 more steps.  Sample 0 is the owner of the shared pages.  Every sample's ids and
    log-probability bits, and every step's last logits, equal the unforked serve of the same schedule -- the survivors still read the prompt
    -- and the page state holds its invariant after the fork and after every release."""
    model = models("default")
    schedule = [("step", 5), ("release", order[0]), ("refill",), ("step", 20), ("release", order[1]), ("step", 5)]
    frame, row, p = sr.fork_inputs("cross")
    check, on_release, state = _roles_checker((256 + len(row)) // 64)
    forked = _serve(model, device, "cross", True, schedule, on_fork=check, on_release=on_release)
    assert state["owner"] is None and not state["followers"]
    plain = _serve(model, device, "cross", False, schedule)
    _assert_equal_serves(forked, plain)
    assert len(forked[1][("sample", order[2])][0]) >= 25 or forked[1][("sample", order[2])][2] == 1


def test_page_state_after_fork_releases_and_the_calls_that_end_slot_serving(device, models):
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    model = models("default")
    eng = model.engine
    frame, row, p = sr.fork_inputs("ctx63")
    nfull = (256 + len(row)) // 64
    fr = torch.from_numpy(frame).to(device)
    pe = eng.vision_encode(fr)[0]

    def fork():
        _prefill(eng, SRC, row, pe, p, 0)
        eng.slots_fork(SRC, FOLLOW, [p] * 2, [p.seed] * 2, [1, 2])

    def clean(table, hidden):
        assert (hidden.numpy() == -1).all() and sorted(table.numpy().ravel().tolist()) == list(range(table.numel()))

    eng.slots_open(N_SLOTS)
    clean(*eng.slots_page_state())
    fork()
    check, on_release, state = _roles_checker(nfull)
    table, hidden = check(eng)
    for f in FOLLOW:   # after the fork the followers' first nfull entries are the owner's, their partial page is their own
        assert (table[f, :nfull] == table[SRC, :nfull]).all() and table[f, nfull] != table[SRC, nfull]
    eng.slots_step(3)
    for slot in (SRC, 1, 4):   # owner first: slot 1 inherits, then is released itself while slot 4 still reads the pages
        eng.slot_release(slot)
        on_release(eng, slot)
    clean(*eng.slots_page_state())                      # the last member left nothing hidden
    fork()
    eng.slots_step(2)
    eng.slots_open(N_SLOTS)                             # a group still outstanding: re-opening gives every hidden page back
    clean(*eng.slots_page_state())
    fork()                                              # ... and so does the plain prefill that ends slot serving
    eng.clear_sampling()
    rows = [sg.inputs("indep")[1][0]]
    got, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=12, stop_on_eos=False)
    clean(*eng.slots_page_state())
    cfg = EmmaXConfig.tiny()
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=sr.WEIGHT_SEED).items()}
    fresh = EmmaXForActionPrediction(cfg, sd).to(device, max_batch=1, max_prompt=64)
    want, _ = fresh.generate_ids(rows, frames_u8=fr, max_new_tokens=12, stop_on_eos=False)
    assert got[0].cpu().tolist() == want[0].cpu().tolist()
    assert not eng.sampling and eng.sample_groups == 0 and eng.beams == 0


def test_refusals_are_decided_on_the_host(device, models):
    from emmax import _lib
    from emmax._lib import EmmaxError
    model = models("default")
    eng = model.engine
    eng.ensure_stage_rows(2)
    frame, row, p = sr.fork_inputs("ctx63")
    fr = torch.from_numpy(frame).to(device)
    pe = eng.vision_encode(fr)[0]

    def refused(code, cause, fn):
        torch.cuda.synchronize()
        before = eng.slots_page_state()
        with pytest.raises(EmmaxError) as e:
            fn()
        msg = str(e.value)
        assert f"status {code}:" in msg and re.search(cause, msg), msg
        torch.cuda.synchronize()
        after = eng.slots_page_state()
        assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])

    def fork(src=SRC, dst=FOLLOW, params=None, staged=None):
        n = len(dst)
        eng.slots_fork(src, dst, params or [p] * n, [p.seed] * n, list(range(1, n + 1)), staged=staged)

    # slots not open (a plain generate closed them)
    model.generate_ids([row], frames_u8=fr, max_new_tokens=2, stop_on_eos=False)
    refused(ERR_STATE, "emmax_slots_open", fork)
    eng.slots_open(N_SLOTS)
    # sampling off
    eng.slot_prefill(SRC, row, pe, BUDGET)
    refused(ERR_STATE, "greedy", fork)
    eng.slot_release(SRC)
    _prefill(eng, SRC, row, pe, p, 0)
    _prefill(eng, 0, row, pe, p, 0)
    # bad arguments
    refused(ERR_INVALID, "outside", lambda: fork(dst=[N_SLOTS]))
    refused(ERR_INVALID, "outside", lambda: fork(dst=[-1]))
    refused(ERR_INVALID, "source slot 9 outside", lambda: fork(src=9))
    refused(ERR_INVALID, "twice", lambda: fork(dst=[4, 4]))
    refused(ERR_INVALID, "is the source", lambda: fork(dst=[4, SRC]))
    refused(ERR_INVALID, "not idle", lambda: fork(dst=[4, 0]))
    refused(ERR_STATE, "holds no request", lambda: fork(src=SPARE, dst=[4]))

    def raw(dst, n, T=(C.c_float * 1)(1.0), k=0, top_p=1.0):   # (SamplingParams checks its values itself: bad ones go in below it)
        one = lambda t, v: (t * 1)(v)
        _lib.check(eng.lib.emmax_slots_fork(eng._session, SRC, -1, dst, n, T, one(C.c_int32, k), one(C.c_float, top_p), one(C.c_uint64, 1), one(C.c_uint32, 1),
                                            _lib.current_stream()), "emmax_slots_fork")

    four = (C.c_int32 * 1)(4)
    refused(ERR_INVALID, "temperature", lambda: raw(four, 1, T=(C.c_float * 1)(-1.0)))
    refused(ERR_INVALID, "temperature", lambda: raw(four, 1, T=(C.c_float * 1)(float("nan"))))
    refused(ERR_INVALID, "top_p", lambda: raw(four, 1, top_p=0.0))
    refused(ERR_INVALID, "top_k", lambda: raw(four, 1, k=-2))
    refused(ERR_INVALID, "null", lambda: raw(None, 1))
    refused(ERR_INVALID, "null", lambda: raw(four, 1, T=None))
    refused(ERR_INVALID, "< 1", lambda: raw(four, 0))
    # a decode step since the in-place prefill: the prompt's logit row is gone
    eng.slots_step(1)
    refused(ERR_STATE, "decode step", fork)
    eng.slot_release(SRC)
    # a live group: its slots take no prefill and no commit, and fork no second group
    _prefill(eng, SRC, row, pe, p, 0)
    fork()
    refused(ERR_STATE, "belongs to a sample group", lambda: eng.slot_prefill(4, row, pe, BUDGET))
    refused(ERR_STATE, "belongs to a sample group", lambda: eng.slots_prefill(1, [row, row], [pe, pe], [BUDGET, BUDGET]))
    refused(ERR_STATE, "already belongs", lambda: fork(src=4, dst=[SPARE]))
    with eng.admission():
        eng.set_sampling_staged([p], [p.seed], [0])
        st1 = eng.slots_prefill_staged([row], [pe], [BUDGET])
    st1.wait()
    refused(ERR_STATE, "belongs to a sample group", lambda: eng.slots_commit(st1, [4], [0]))
    eng.slots_commit(st1, [SPARE], [0])
    refused(ERR_STATE, "pass staged_idx", lambda: fork(src=SPARE, dst=[3]))                  # its logit row is the staging row's
    refused(ERR_STATE, "current staged batch", lambda: fork(src=SPARE, dst=[3], staged=1))   # ... of request 0, not 1
    with eng.admission():
        eng.set_sampling_staged([p], [p.seed], [0])
        st2 = eng.slots_prefill_staged([row], [pe], [BUDGET])
    st2.wait()
    refused(ERR_STATE, "current staged batch", lambda: fork(src=SPARE, dst=[3], staged=0))   # an older staged batch: that logit row was overwritten
    eng.slots_commit(st2, [3], [0])
    eng.slots_open(N_SLOTS)   # every hidden page back, no group left
    table, hidden = eng.slots_page_state()
    assert (hidden.numpy() == -1).all() and sorted(table.numpy().ravel().tolist()) == list(range(table.numel()))
    eng.clear_sampling()


_WANT, _SERVED = {}, {}


def _reference_runs(model, device, wl, fr):
    """Every sample's one-row generate with (seed_i, subseq j), and the step up to which its ids are REQUIRED to match: the oracle's rows
    teacher-forced on the one-row run, the rule of test_exact_numerics_batch_position_does_not_matter.  Computed once for both admissions."""
    from oracle import emmax_oracle as orc

    if _WANT:
        return _WANT
    from emmax.weights import synthetic_state_dict

    eng, cfg = model.engine, model.engine.cfg
    sd_ref = {k: v.to(torch.bfloat16).float() for k, v in synthetic_state_dict(cfg, seed=sr.WEIGHT_SEED).items()}
    for i, (frame, row, k, p, budget) in enumerate(wl):
        patches = sr.oracle_patches(orc, cfg, sd_ref, frame)
        for j in range(k):
            if p is None:
                ids, lens = model.generate_ids([row], frames_u8=fr[i], max_new_tokens=budget, stop_on_eos=True)
                one, lp = ids[0, : int(lens[0])].cpu().tolist(), None
            else:
                eng.set_sampling([p], [p.seed], [j])
                eng.prefill([row], eng.vision_encode(fr[i]))
                ids, lens, lps = eng.generate(budget, True, return_logprobs=True)
                eng.clear_sampling()
                one, lp = ids[0, : int(lens[0])].cpu().tolist(), lps[0, : int(lens[0])].cpu().numpy()
            logits, _ = orc.llama_forward(orc.splice(torch.tensor([row + one], dtype=torch.long), patches, sd_ref), sd_ref, cfg.llm, None)
            L = logits[0, -len(one) - 1:-1].float().numpy()
            _WANT[(i, j)] = (one, lp, sr.clear_steps(L, one, p, j, ID_BUDGET_EXACT))
    return _WANT


@pytest.mark.parametrize("overlap", [False, True])
def test_scheduler_samples_equal_their_one_row_runs(device, models, overlap):
    """Exact numerics, 6 slots, 10 requests mixing num_samples 1, 2 and 3 with greedy singles, different budgets, the stop rule armed:
    sample j of request i is the one-row generate with (seed_i, subseq j) -- ids up to the first step below the exact-numerics id line,
    log-probabilities within 1e-4 there -- on both admission paths, which agree with each other id for id."""
    from emmax.serving import Request, SlotScheduler

    model = models("exact")
    eng = model.engine
    wl = sr.workload()
    fr = [torch.from_numpy(f).to(device) for f, *_ in wl]
    want = _reference_runs(model, device, wl, fr)

    def encode(fs):
        pe = eng.vision_encode(torch.cat(fs))
        return [pe[i] for i in range(len(fs))]

    trig = [wl[0][1][3], wl[0][1][4]]   # (rarely emitted: the rule is armed, the ids stay comparable to a rule-free run)
    sch = SlotScheduler(eng, encode, n_slots=N_SLOTS, poll_every=3, stop_trigger=trig, stop_after=50, overlap=overlap)
    for i, (frame, row, k, p, budget) in enumerate(wl):
        sch.submit(Request(i, fr[i], row, max_new_tokens=budget, sampling=p, num_samples=k))
    res = sch.run()
    eng.set_stop([], 0)
    assert sch.overlap == overlap and not eng.sampling
    assert sorted((r.rid, r.sample) for r in res) == sorted(want)
    total = compared = 0
    for r in res:
        one, lp, n_clear = want[(r.rid, r.sample)]
        n = min(n_clear, len(r.ids), len(one))
        print(f"overlap={overlap} request {r.rid} sample {r.sample} slot {r.slot}: {len(r.ids)} ids, compared {n}")
        assert r.ids[:n] == one[:n], (r.rid, r.sample, r.ids, one)
        assert (r.logprobs is None) == (wl[r.rid][3] is None)
        if r.logprobs is not None and n:
            assert np.abs(np.float32(r.logprobs[:n]) - lp[:n]).max() <= 1e-4, (r.rid, r.sample)
        total += len(r.ids)
        compared += n
    assert 2 * compared >= total, (compared, total)
    mine = {(r.rid, r.sample): r.ids for r in res}
    other = _SERVED.setdefault("ids", mine)   # the two admission paths serve the same ids
    assert mine == other
