"""Top-N and watched-token log-probabilities on a real MI355X (include/emmax.h: emmax_op_top_logprobs / emmax_session_set_top_logprobs; the
kernel: emmax_top_logprobs_kernel in emma-x_amd/csrc/sample.hip).

Op level: crafted rows against the numpy reference (tests/top_logprobs_ref.py) -- ids exact, log-probabilities within 1e-5 of float64 (the
line tests/test_sampling_gpu.py holds emmax_op_sample's log-probability to), the emitted token's entry bit for bit emmax_op_sample's, a
second launch bit-identical.  In the step: the bound buffers against the op on the recorded raw rows, bit for bit."""
import numpy as np
import pytest
import torch

import top_logprobs_ref as ref

pytestmark = pytest.mark.gpu

LP_TOL = 1e-5
ERR_INVALID, ERR_STATE = -1, -5   # include/emmax.h
FILL = -777.0   # what the tests put into every output place before a launch


def _op(x, n, watch):
    """emmax_op_top_logprobs through its ctypes signature on x [B, V] (a view of rows ld apart), outputs pre-filled"""
    from emmax import _lib

    lib = _lib.load()
    B, V = x.shape
    dev = x.device
    W = len(watch)
    ti = torch.full((B, max(n, 1)), -5, dtype=torch.int32, device=dev)
    tl = torch.full((B, max(n, 1)), FILL, dtype=torch.float32, device=dev)
    wl = torch.full((B, max(W, 1)), FILL, dtype=torch.float32, device=dev)
    wi = torch.as_tensor(np.asarray(list(watch) or [0], dtype=np.int32), device=dev)
    _lib.check(lib.emmax_op_top_logprobs(x.data_ptr(), x.stride(0), B, V, n, ti.data_ptr() if n else None, tl.data_ptr() if n else None, W,
                                         wi.data_ptr() if W else None, wl.data_ptr() if W else None, _lib.current_stream()), "emmax_op_top_logprobs")
    torch.cuda.synchronize()
    return ti.cpu().numpy()[:, :n], tl.cpu().numpy()[:, :n], wl.cpu().numpy()[:, :W]


def _greedy_sample(x):
    """emmax_op_sample at temperature 0: (token, log-probability) of every row"""
    from emmax.sampling import SamplingParams, sample_logits

    tok, lp = sample_logits(x, SamplingParams(0.0, 0, 1.0, seed=1))
    torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy()


def _crafted(V, rng):
    """row sets of B = 3: random / all equal / equal maxima in different waves and a tie across the threshold; V - 3 entries at -inf / one
    NaN / all NaN; many ties (values on a coarse grid) / signed zeros / a wide random row"""
    rnd = lambda s: (rng.standard_normal(V) * s).astype(np.float32)
    equal = np.full(V, 0.375, dtype=np.float32)
    tie = rnd(1.0)
    # lane l of the kernel holds ids 4 l .. 4 l + 3 of every 4096: ids 256 apart sit in different waves
    top = sorted({3, V // 2, V - 1})
    thr = sorted({1, V // 3, (2 * V) // 3, V - 2} - set(top))
    tie[thr] = 6.0   # with 3 maxima above, N = 5 cuts through these: the lowest ids win
    tie[top] = 9.0
    ninf = np.full(V, -np.inf, dtype=np.float32)
    ninf[[0, V // 2, V - 1]] = np.array([0.5, 2.0, 0.5], dtype=np.float32)
    one_nan = rnd(2.0)
    one_nan[V // 3] = np.nan
    all_nan = np.full(V, np.nan, dtype=np.float32)
    grid = np.round(rnd(1.5) * 2.0) / 2.0
    zeros = np.where(rng.integers(0, 2, size=V) == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    zeros[V // 4] = -1.0
    return [np.stack([rnd(2.5), equal, tie]), np.stack([ninf, one_nan, all_nan]), np.stack([grid.astype(np.float32), zeros, rnd(6.0)])]


def _watch_lists(V, rng):
    w256 = [int(v) for v in rng.integers(0, V, size=256)]
    w256[7] = w256[3]   # duplicates are allowed
    w256[255] = V - 1
    w256[0] = 0
    return [[], [V // 2], w256]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("V", [20, 21, 1023, 32064, 32768])
def test_op_crafted_rows(device, V, pad):
    rng = np.random.default_rng(1000 * V + pad)
    ns = sorted({1, 5, 20, min(V, 20)})
    watches = _watch_lists(V, rng)
    for rows in _crafted(V, rng):
        buf = torch.full((3, V + pad), 1e30, dtype=torch.float32, device=device)   # (the pad columns hold what would win every order)
        buf[:, :V] = torch.from_numpy(rows).to(device)
        x = buf[:, :V]
        assert x.stride(0) == V + pad
        tok, lp = _greedy_sample(x)
        for k, n in enumerate(ns):
            watch = watches[k % len(watches)]
            ti, tl, wl = _op(x, n, watch)
            ri, rl, rw = ref.top_rows(rows, n, watch)
            assert (ti == ri).all(), (V, pad, n, ti.tolist(), ri.tolist())
            assert ref.close(tl, rl, LP_TOL), (V, pad, n, tl, rl)
            assert ref.close(wl, rw, LP_TOL), (V, pad, n)
            # the emitted (greedy) token is the first entry: the bits of emmax_op_sample's log-probability
            assert (ti[:, 0] == tok).all(), (ti[:, 0], tok)
            assert ref.same_bits(tl[:, 0], np.where(tok >= 0, lp, -np.inf).astype(np.float32)), (tl[:, 0], lp)
            ti2, tl2, wl2 = _op(x, n, watch)
            assert (ti2 == ti).all() and ref.same_bits(tl2, tl) and ref.same_bits(wl2, wl)
        # ... and watched: row b's greedy token at place b
        wt = [int(t) if t >= 0 else 0 for t in tok]
        _, _, wl = _op(x, 0, wt)
        for b in range(3):
            if tok[b] >= 0:
                assert ref.same_bits(wl[b, b : b + 1], lp[b : b + 1]), (b, wl[b], lp[b])


def test_op_all_equal_ids_and_independence_of_batch(device):
    """a row of equal values lists ids 0 .. N - 1; a row's result does not depend on its place in the batch or on B"""
    V = 32064
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((5, V)) * 3).astype(np.float32)
    rows[2] = -1.25
    x = torch.from_numpy(rows).to(device)
    watch = [int(v) for v in rng.integers(0, V, size=17)]
    ti, tl, wl = _op(x, 20, watch)
    assert ti[2].tolist() == list(range(20))
    for b in range(5):
        ti1, tl1, wl1 = _op(x[b : b + 1], 20, watch)
        assert (ti1[0] == ti[b]).all() and ref.same_bits(tl1[0], tl[b]) and ref.same_bits(wl1[0], wl[b])
    y = torch.from_numpy(rows[::-1].copy()).to(device)
    tir, tlr, wlr = _op(y, 20, watch)
    assert (tir[::-1] == ti).all() and ref.same_bits(tlr[::-1], tl) and ref.same_bits(wlr[::-1], wl)


def test_op_refusals_and_wrapper(device):
    from emmax import _lib
    from emmax.sampling import top_logprobs

    lib = _lib.load()
    x = torch.randn(2, 40, device=device)
    i32 = torch.zeros(2, 64, dtype=torch.int32, device=device)
    f32 = torch.zeros(2, 300, dtype=torch.float32, device=device)
    call = lambda ld, V, n, ti, tl, W, wi, wl: lib.emmax_op_top_logprobs(x.data_ptr(), ld, 2, V, n, ti, tl, W, wi, wl, _lib.current_stream())
    P, F = i32.data_ptr(), f32.data_ptr()
    assert call(40, 40, 5, P, F, 2, P, F) == 0
    assert call(40, 40, 0, None, None, 2, P, F) == 0 and call(40, 40, 5, P, F, 0, None, None) == 0   # either part may be off
    for bad in [(40, 40, 21, P, F, 0, None, None), (40, 40, 5, P, F, 257, P, F), (40, 10, 11, P, F, 0, None, None),
                (39, 40, 5, P, F, 0, None, None), (40, 40, 5, None, F, 0, None, None), (40, 40, 5, P, None, 0, None, None),
                (40, 40, 0, None, None, 2, None, F), (40, 40, 0, None, None, 2, P, None), (40, 40, -1, P, F, 0, None, None)]:
        assert call(*bad) == ERR_INVALID, bad
    torch.cuda.synchronize()
    ti, tl, wl = top_logprobs(x, 3, [1, 1, 39])
    ri, rl, rw = ref.top_rows(x.cpu().numpy(), 3, [1, 1, 39])
    assert (ti.cpu().numpy() == ri).all() and ref.close(tl.cpu().numpy(), rl, LP_TOL) and ref.close(wl.cpu().numpy(), rw, LP_TOL)
    for kw in [dict(n=21), dict(n=-1), dict(n=2, watch_ids=[40]), dict(n=2, watch_ids=[-1]), dict(n=2, watch_ids=list(range(40)) * 7)]:
        with pytest.raises(ValueError):
            top_logprobs(x, **kw)


# ---- in the step ------------------------------------------------------------------------------------------------------------------------
from test_sampled_decode_gpu import _inputs, _mixed_params, _op_cfg, _tiny_model   # noqa: E402  (the models and inputs of that file)

WATCH = [5, 31999, 5, 17, 0, 32063, 1234]   # duplicates allowed


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """bit-for-bit equality of two device / host tensors (every NaN one value)"""
    a, b = a.cpu(), b.cpu()
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    return ref.same_bits(a.numpy(), b.numpy())


def _op_t(x, n, watch):
    from emmax.sampling import top_logprobs

    return top_logprobs(x.contiguous(), n, watch)


def _check_against_op(ids, lens, top, raw, n, watch, bound=None):
    """every written entry [b, t] equals emmax_op_top_logprobs on the raw row the step recorded at [t, b]; the emitted token's entry, where it
    is among the top n or watched, carries the bits of the chosen log-probability"""
    B, T = ids.shape
    T = min(T, bound or T)
    ids_h, lp_h = ids.cpu().numpy(), top.logprobs.cpu().numpy()
    hits = 0
    for t in range(T):
        live = [b for b in range(B) if int(lens[b]) > t]
        if not live:
            continue
        ti, tl, wl = _op_t(raw[t][live], n, watch)
        if n:
            assert _same(top.top_ids[live, t], ti), t
            assert _same(top.top_logprobs[live, t], tl), t
        if watch:
            assert _same(top.watch_logprobs[live, t], wl), t
        for k, b in enumerate(live):
            tok = int(ids_h[b, t])
            row = ti[k].cpu().tolist() if n else []
            if tok in row:
                hits += 1
                assert ref.same_bits(tl[k, row.index(tok)].cpu().numpy().reshape(1), lp_h[b, t : t + 1]), (b, t)
            if tok in watch:
                assert ref.same_bits(wl[k, watch.index(tok)].cpu().numpy().reshape(1), lp_h[b, t : t + 1]), (b, t)
    return hits


def _gen(model, rows, fr, n, sampling=None, processing=None, n_top=20, watch=WATCH, record=True, num_samples=1, stop_on_eos=False):
    B = len(rows) * num_samples
    raw = torch.full((n, B, model.config.llm.vocab_size), float("nan"), dtype=torch.float32, device=fr.device) if record else None
    kw = {} if num_samples == 1 else {"num_samples": num_samples}
    ids, lens, top = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=stop_on_eos, sampling=sampling, processing=processing,
                                        logits=raw, top_logprobs=n_top, watch_ids=watch, **kw)
    return ids, lens.cpu(), top, raw


@pytest.fixture(scope="module")
def tiny8(device):
    model, _, _ = _tiny_model(device, 8)
    frames, rows = _inputs(8, seed=33)
    return model, torch.from_numpy(frames).to(device), rows


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_step_equals_op_on_recorded_rows(tiny8, B, graph):
    from emmax import _lib

    model, fr, rows = tiny8
    with _lib.tuning(graph=graph):
        for sampling in (None, _mixed_params(B)):
            ids, lens, top, raw = _gen(model, rows[:B], fr[:B], 12, sampling=sampling)
            assert model.engine.graph_active() == bool(graph)
            assert not model.engine.top_logprobs_bound and model.engine.sampling == (sampling is not None)
            hits = _check_against_op(ids, lens, top, raw, 20, WATCH)
            if sampling is None:   # greedy rows: every token is its row's first entry
                assert hits == int(lens.sum())
                for b in range(B):
                    assert _same(top.top_ids[b, : int(lens[b]), 0], ids[b, : int(lens[b])])


@pytest.mark.parametrize("graph", [0, 1])
def test_tokens_and_logprobs_unchanged(tiny8, graph):
    """greedy rows: the greedy ids; mixed sampled rows: ids and chosen log-probability bits with the feature on = off; and the values do not
    depend on whether the step also records its rows (the sampled finish / the processing finish)"""
    from emmax import _lib

    model, fr, rows = tiny8
    with _lib.tuning(graph=graph):
        g_ids, g_lens = model.generate_ids(rows[:3], frames_u8=fr[:3], max_new_tokens=12, stop_on_eos=False)
        ids, lens, top, _ = _gen(model, rows[:3], fr[:3], 12, record=False)
        assert _same(ids, g_ids) and _same(lens, g_lens) and not model.engine.sampling
        params = _mixed_params(3)
        s_ids, s_lens, s_lp = model.generate_ids(rows[:3], frames_u8=fr[:3], max_new_tokens=12, stop_on_eos=False, sampling=params, return_logprobs=True)
        ids, lens, top, _ = _gen(model, rows[:3], fr[:3], 12, sampling=params, record=False)
        assert _same(ids, s_ids) and _same(lens, s_lens) and _same(top.logprobs, s_lp)
        ids2, _, top2, _ = _gen(model, rows[:3], fr[:3], 12, sampling=params, record=True)
        assert _same(ids2, ids) and _same(top2.top_ids, top.top_ids) and _same(top2.top_logprobs, top.top_logprobs) and _same(top2.watch_logprobs, top.watch_logprobs)
        # the same draw again with every emitted token watched: its watched entry has the bits of the chosen log-probability
        ids_h, lp_h = ids.cpu().numpy(), top.logprobs.cpu().numpy()
        emitted = sorted({int(ids_h[b, t]) for b in range(3) for t in range(int(lens[b]))})
        ids3, _, top3, _ = _gen(model, rows[:3], fr[:3], 12, sampling=params, n_top=0, watch=emitted, record=False)
        assert _same(ids3, ids)
        w3 = top3.watch_logprobs.cpu().numpy()
        for b in range(3):
            for t in range(int(lens[b])):
                assert ref.same_bits(w3[b, t, emitted.index(int(ids_h[b, t]))].reshape(1), lp_h[b, t : t + 1]), (b, t)


def test_processing_on_reports_raw_values(tiny8):
    from emmax.sampling import LogitsProcessing

    model, fr, rows = tiny8
    proc = LogitsProcessing(repetition_penalty=1.1)
    p_ids, p_lens = model.generate_ids(rows[:3], frames_u8=fr[:3], max_new_tokens=12, stop_on_eos=False, processing=proc)
    ids, lens, top, raw = _gen(model, rows[:3], fr[:3], 12, processing=proc, n_top=5)
    assert _same(ids, p_ids) and _same(lens, p_lens)
    _check_against_op(ids, lens, top, raw, 5, WATCH)
    assert not model.engine.sampling and model.engine.processing


def _run_bound(model, rows, fr, n, params, n_top, watch, bound, alloc_T):
    """the engine's own calls with the test's pre-filled buffers: [R, alloc_T, k] allocations bound as [R][bound][k]"""
    import ctypes as C

    from emmax import _lib

    eng = model.engine
    B = len(rows)
    eng.ensure_capacity(B, max(len(r) for r in rows), n)
    patches = eng.vision_encode(fr)
    model._set_processing(eng, B, None)
    model._set_sampling(eng, B, params)
    R = eng.max_batch + eng.stage_rows
    ti = torch.full((R, alloc_T, n_top), -5, dtype=torch.int32, device=fr.device)
    tl = torch.full((R, alloc_T, n_top), FILL, dtype=torch.float32, device=fr.device)
    wl = torch.full((R, alloc_T, len(watch)), FILL, dtype=torch.float32, device=fr.device)
    wi = (C.c_int32 * len(watch))(*watch)
    _lib.check(eng.lib.emmax_session_set_top_logprobs(eng._session, n_top, ti.data_ptr(), tl.data_ptr(), len(watch), wi, wl.data_ptr(), bound,
                                                      _lib.current_stream()), "emmax_session_set_top_logprobs")
    assert eng.top_logprobs_bound
    eng.prefill(rows, patches)
    ids, lens, lp = eng.generate(n, True, return_logprobs=True)
    torch.cuda.synchronize()
    eng.clear_top_logprobs()
    return ids.cpu(), lens.cpu(), ti.cpu(), tl.cpu(), wl.cpu()


def test_unwritten_entries_keep_their_fill(tiny8):
    """a row that stops early leaves the entries past its length alone; a bound max_new below the generation leaves everything past it alone"""
    from emmax.sampling import SamplingParams

    model, fr, rows = tiny8
    eng = model.engine
    g_ids, _ = model.generate_ids(rows[:3], frames_u8=fr[:3], max_new_tokens=12, stop_on_eos=False)
    g = g_ids.cpu().tolist()
    trig, eos = g[1][2], model.config.eos_token_id   # a row is done one token after it emits `trig` (or at EOS)

    def length(row):
        stops = [t + 2 for t, v in enumerate(row) if v == trig] + [t + 1 for t, v in enumerate(row) if v == eos]
        return min(stops + [12])

    eng.set_stop([trig], 1)
    try:
        ids, lens, ti, tl, wl = _run_bound(model, rows[:3], fr[:3], 12, [SamplingParams(0.0, 0, 1.0, seed=1)] * 3, 5, WATCH, 12, 12)
    finally:
        eng.set_stop([], 0)
    lens = lens.tolist()
    assert lens == [length(r) for r in g] and lens[1] <= 4, lens
    for b in range(3):
        L = lens[b]
        assert (ti[b, :L] >= 0).all() and bool(torch.isfinite(tl[b, :L]).all()) and bool(torch.isfinite(wl[b, :L]).all())
        assert (ti[b, L:] == -5).all() and (tl[b, L:] == FILL).all() and (wl[b, L:] == FILL).all(), b
        assert ti[b, :L, 0].tolist() == ids[b, :L].tolist()
    assert (ti[3:] == -5).all() and (tl[3:] == FILL).all() and (wl[3:] == FILL).all()   # rows of no request
    # bound 5 of a 12-token generation: the buffers are [R][5][k] at the head of the allocation, entry t >= 5 is never written
    ids, lens, ti, tl, wl = _run_bound(model, rows[:3], fr[:3], 12, [SamplingParams(0.0, 0, 1.0, seed=1)] * 3, 5, WATCH, 5, 12)
    R = ti.shape[0]
    flat_i, flat_l, flat_w = ti.reshape(-1), tl.reshape(-1), wl.reshape(-1)
    assert (flat_i[R * 5 * 5 :] == -5).all() and (flat_l[R * 5 * 5 :] == FILL).all() and (flat_w[R * 5 * len(WATCH) :] == FILL).all()
    head = flat_i[: R * 5 * 5].reshape(R, 5, 5)
    assert head[:3, :, 0].tolist() == ids[:, :5].tolist() and (head[3:] == -5).all()


def test_exact_numerics_b2(device):
    model, _, _ = _tiny_model(device, 2, exact=True)
    frames, rows = _inputs(2, seed=9)
    fr = torch.from_numpy(frames).to(device)
    ids, lens, top, raw = _gen(model, rows, fr, 12, sampling=_mixed_params(2))
    _check_against_op(ids, lens, top, raw, 20, WATCH)


def test_sample_group_of_4(tiny8):
    from emmax.sampling import SamplingParams

    model, fr, rows = tiny8
    p = SamplingParams(1.2, 0, 1.0, seed=77)
    ids, lens, top, raw = _gen(model, rows[:1], fr[:1], 12, sampling=p, n_top=5, num_samples=4)
    assert ids.shape[0] == 4
    for j in range(1, 4):   # the samples drew token 0 from the prompt's one logit row
        assert _same(top.top_ids[j, 0], top.top_ids[0, 0]) and _same(top.top_logprobs[j, 0], top.top_logprobs[0, 0]) and _same(top.watch_logprobs[j, 0], top.watch_logprobs[0, 0])
    assert len({tuple(r) for r in ids.cpu().tolist()}) > 1
    ids1, lens1, top1, _ = _gen(model, rows[:1], fr[:1], 12, sampling=p, n_top=5, record=False)
    assert _same(top1.top_ids[0, 0], top.top_ids[0, 0]) and _same(top1.top_logprobs[0, 0], top.top_logprobs[0, 0]) and _same(top1.watch_logprobs[0, 0], top.watch_logprobs[0, 0])
    _check_against_op(ids, lens, top, raw, 5, WATCH)


@pytest.fixture(scope="module")
def op_model(device):
    import copy

    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = _op_cfg()
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=21).items()}
    model = EmmaXForActionPrediction(copy.deepcopy(cfg), sd).to(device, max_batch=17, max_prompt=32, max_ctx=256 + 32 + 40)
    frames, rows = _inputs(17, seed=77, lo=8, hi=24)
    return model, torch.from_numpy(frames).to(device), rows


@pytest.mark.parametrize("graph", [0, 1])
def test_step_equals_op_at_17_rows(op_model, graph):
    """the 7B-dims 2-layer model at 17 rows (the two-tile kernels), 6 new tokens"""
    from emmax import _lib

    model, fr, rows = op_model
    with _lib.tuning(graph=graph):
        ids, lens, top, raw = _gen(model, rows, fr, 6, sampling=_mixed_params(17), n_top=20)
        assert model.engine.graph_active() == bool(graph)
    _check_against_op(ids, lens, top, raw, 20, WATCH)


@pytest.mark.parametrize("overlap", [False, True])
def test_slot_serving(device, overlap):
    """4 slots, 8 requests of unequal budgets, one of them a group of 3: every Result's lists are the request's bs = 1 generate_ids output
    (ids exact, log-probabilities within 1e-4: the rule of test_sampled_decode_gpu.py for slots against bs = 1)"""
    from emmax.sampling import SamplingParams
    from emmax.serving import Request, SlotScheduler

    model, _, _ = _tiny_model(device, 4, exact=True)
    eng = model.engine
    frames, rows = _inputs(8, seed=52)
    fr = torch.from_numpy(frames).to(device)
    samp = [None if i % 3 == 0 else SamplingParams([1.0, 0.8][i % 2], [50, 0][i % 2], [1.0, 0.9][i % 2], seed=300 + i) for i in range(8)]
    budgets = [6 + (i * 5) % 9 for i in range(8)]
    n_top = [0, 5, 20, 3, 1, 0, 2, 20]
    asks_watch = [True, False, True, True, False, False, True, True]
    nsamp = [1, 1, 1, 1, 3, 1, 1, 1]
    want = {}
    for i in range(8):
        kw = {} if nsamp[i] == 1 else {"num_samples": 3}
        if not n_top[i] and not asks_watch[i]:
            continue
        ids, lens, top = model.generate_ids([rows[i]], frames_u8=fr[i:i + 1], max_new_tokens=budgets[i], stop_on_eos=True,
                                            sampling=None if samp[i] is None else samp[i], top_logprobs=n_top[i], watch_ids=WATCH if asks_watch[i] else None, **kw)
        for j in range(nsamp[i]):
            L = int(lens[j])
            want[(i, j)] = (ids[j, :L].cpu().tolist(), top.top_ids[j, :L].cpu().numpy(), top.top_logprobs[j, :L].cpu().numpy(), top.watch_logprobs[j, :L].cpu().numpy())

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    sch = SlotScheduler(eng, encode, n_slots=4, poll_every=3, overlap=overlap)
    for i in range(8):
        sch.submit(Request(i, fr[i], rows[i], max_new_tokens=budgets[i], sampling=samp[i], num_samples=nsamp[i], top_logprobs=n_top[i],
                           watch_ids=WATCH if asks_watch[i] else None))
    res = sch.run()
    assert len(res) == 10 and not eng.sampling and not eng.top_logprobs_bound
    for r in res:
        i = r.rid
        assert (r.top_logprobs is None) == (n_top[i] == 0) and (r.watch_logprobs is None) == (not asks_watch[i])
        if (i, r.sample) not in want:
            continue
        w_ids, w_ti, w_tl, w_wl = want[(i, r.sample)]
        assert r.ids == w_ids, (overlap, i, r.sample)
        if n_top[i]:
            assert [[p[0] for p in row] for row in r.top_logprobs] == w_ti.tolist(), (overlap, i, r.sample)
            assert np.abs(np.float32([[p[1] for p in row] for row in r.top_logprobs]) - w_tl).max() <= 1e-4
        if asks_watch[i]:
            assert np.abs(np.float32(r.watch_logprobs) - w_wl).max() <= 1e-4


def test_clear_and_refusals(tiny8):
    import ctypes as C

    from emmax import _lib
    from emmax.sampling import BeamParams, SamplingParams

    model, fr, rows = tiny8
    eng = model.engine
    lib = eng.lib
    g_ids, _ = model.generate_ids(rows[:2], frames_u8=fr[:2], max_new_tokens=8, stop_on_eos=False)
    ids, _, top, _ = _gen(model, rows[:2], fr[:2], 8, n_top=3, record=False)
    assert lib.emmax_session_top_logprobs(eng._session) == 0 and not eng.sampling
    after, _ = model.generate_ids(rows[:2], frames_u8=fr[:2], max_new_tokens=8, stop_on_eos=False)
    assert _same(after, g_ids) and _same(ids, g_ids)
    R, V = eng.max_batch + eng.stage_rows, model.config.llm.vocab_size
    ti = torch.zeros(R, 8, 20, dtype=torch.int32, device=fr.device)
    tl = torch.zeros(R, 8, 20, dtype=torch.float32, device=fr.device)
    wl = torch.zeros(R, 8, 256, dtype=torch.float32, device=fr.device)
    w = (C.c_int32 * 257)(*([3] * 257))
    bind = lambda n, W, wi=w, T=8: lib.emmax_session_set_top_logprobs(eng._session, n, ti.data_ptr(), tl.data_ptr(), W, wi, wl.data_ptr(), T, _lib.current_stream())
    assert bind(5, 2) == ERR_STATE   # the logit rows are off: neither sampling nor processing
    eng.set_beams(BeamParams(2))     # (works: nothing is bound)
    assert bind(5, 2) == ERR_STATE   # beams on
    eng.clear_beams()
    eng.set_sampling(SamplingParams(0.0, 0, 1.0, seed=1), n=2)
    assert bind(21, 0) == ERR_INVALID and bind(0, 257) == ERR_INVALID and bind(0, 0) == ERR_INVALID
    assert bind(5, 1, (C.c_int32 * 1)(V)) == ERR_INVALID and bind(5, 1, (C.c_int32 * 1)(-1)) == ERR_INVALID
    assert bind(5, 2, w, 0) == ERR_INVALID and bind(5, 2, w, eng.max_ctx + 1) == ERR_INVALID
    assert lib.emmax_session_top_logprobs(eng._session) == 0
    assert bind(20, 256) == 0 and lib.emmax_session_top_logprobs(eng._session) == 1
    assert lib.emmax_session_set_beams(eng._session, 2, 1.0, 0, _lib.current_stream()) == ERR_STATE   # refused while bound
    eng.clear_sampling()             # turns the logit rows off: unbinds
    assert lib.emmax_session_top_logprobs(eng._session) == 0 and lib.emmax_session_top_logprobs(None) == -1
    eng.set_beams(BeamParams(2))     # works again
    eng.clear_beams()
    after, _ = model.generate_ids(rows[:2], frames_u8=fr[:2], max_new_tokens=8, stop_on_eos=False)
    assert _same(after, g_ids)


def test_generate_predict_action_and_generate_batch(tiny8):
    """the public interface: generate's output fields, predict_action's bin log-probabilities, generate_batch's string probabilities"""
    from emmax.actions import action_bin_token_ids
    from emmax.tokenizer_stub import StubTokenizer

    model, fr, rows = tiny8
    P = len(rows[0])
    out = model.generate(torch.tensor([rows[0]]), frames_u8=fr[:1], max_new_tokens=6, return_dict_in_generate=True, output_logits=True, top_logprobs=4,
                         watch_ids=WATCH)
    T = out.sequences.shape[1] - P
    assert tuple(out.top_token_ids.shape) == (1, T, 4) and tuple(out.top_logprobs.shape) == (1, T, 4) and tuple(out.watch_logprobs.shape) == (1, T, len(WATCH))
    assert out.top_token_ids[0, :, 0].cpu().tolist() == out.sequences[0, P:].tolist()
    for t in range(T):
        ti, tl, wl = _op_t(out.logits[t], 4, WATCH)
        assert _same(out.top_token_ids[:, t], ti) and _same(out.top_logprobs[:, t], tl) and _same(out.watch_logprobs[:, t], wl)
    plain = model.generate(torch.tensor([rows[0]]), frames_u8=fr[:1], max_new_tokens=6, return_dict_in_generate=True)
    assert plain.top_token_ids is None and plain.top_logprobs is None and plain.watch_logprobs is None and torch.equal(plain.sequences, out.sequences)
    # predict_action
    a0 = model.predict_action(torch.tensor([rows[0]]), frames_u8=fr[:1])
    a1, lp = model.predict_action(torch.tensor([rows[0]]), frames_u8=fr[:1], return_bin_logprobs=True)
    dim = model.get_action_dim()
    assert np.array_equal(a0, a1) and lp.shape == (dim, model.config.n_action_bins) and lp.dtype == np.float32
    assert np.abs(np.log(np.exp(lp.astype(np.float64)).sum(-1))).max() <= 1e-5
    bins = action_bin_token_ids(model.vocab_size, model.config.n_action_bins)
    row = rows[0] if rows[0][-1] == 29871 else rows[0] + [29871]
    ids, lens, top = model.generate_ids([row], frames_u8=fr[:1], max_new_tokens=dim, watch_ids=bins)
    want = top.watch_logprobs[0].cpu().numpy().astype(np.float64)
    want = want - np.log(np.exp(want - want.max(-1, keepdims=True)).sum(-1, keepdims=True)) - want.max(-1, keepdims=True)
    assert np.abs(lp - want).max() <= 1e-5
    # generate_batch: a tokenizer whose trigger strings are one token each
    class Tok(StubTokenizer):
        table = {s: 400 + k for k, s in enumerate(model.TRIGGER_STRINGS)}

        def encode(self, text, add_special_tokens=True):
            if not add_special_tokens and text in self.table:
                return [self.table[text]]
            return super().encode(text, add_special_tokens)

    texts = ["is it open?", "pick one"]
    with pytest.raises(ValueError, match='"Yes"'):
        model.generate_batch(torch.zeros(6, 224, 224), texts, return_string_probabilities=["Yes", "No"], tokenizer=StubTokenizer(), max_new_tokens=2)   # several tokens
    with pytest.raises(ValueError, match='"Maybe"'):
        model.generate_batch(torch.zeros(6, 224, 224), texts, return_string_probabilities=["Maybe"], tokenizer=Tok(), max_new_tokens=2)
    img = torch.randn(6, 224, 224, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    probs = model.generate_batch(img, texts, return_string_probabilities=["Yes", "No", "A"], tokenizer=Tok(), max_new_tokens=2)
    tok = Tok()
    rows2 = [tok(t, truncation=True, return_tensors="pt").input_ids[0].tolist() for t in texts]
    o = model.generate(rows2, img[None].expand(2, -1, -1, -1), max_new_tokens=2, return_dict_in_generate=True, output_logits=True)
    sm = torch.softmax(o.logits[0].double(), dim=-1)[:, [Tok.table[s] for s in ("Yes", "No", "A")]]
    want = (sm / sm.sum(-1, keepdim=True)).cpu().numpy()
    assert np.abs(np.asarray(probs) - want).max() <= 1e-5 and np.abs(np.asarray(probs).sum(-1) - 1).max() <= 1e-12
    txt = model.generate_batch(img, texts, tokenizer=Tok(), max_new_tokens=3)
    assert isinstance(txt, list) and len(txt) == 2 and all(isinstance(t, str) for t in txt)
