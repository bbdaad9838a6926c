"""Sample groups on a real MI355X: generate(do_sample=True, num_return_sequences=N) as N sampled rows per prompt on the prompt's KV pages
(include/emmax.h: emmax_session_set_sample_groups; the fork in emma-x_amd/csrc/beam.hip, run_group_fork in step.hip).

Tiny configuration throughout (256 patch rows: context = 256 + prompt ids) except the operating-point and MXFP4 cases.  The inputs,
temperatures and seeds come from tests/sample_groups_ref.py; tests/test_sample_groups.py shows on the CPU, with the fp32 oracle, that the rows
of every group must diverge at step 0 for them -- so "the rows diverged" below is a property of the inputs.
  1. the DRAW is the step's own: ids and log-probability bits equal an external loop over emmax_op_sample on the same group session;
  2. the CACHE follows the fork: every row's raw logits at every step against the oracle, teacher-forced on the row's own ids;
  3. the same on the device alone, bit for bit (exact numerics, a private one-row session)."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_groups_ref as sg  # noqa: E402
from conftest import ID_BUDGET_EXACT, ID_BUDGET_TINY  # noqa: E402

pytestmark = pytest.mark.gpu


def _tiny_model(device, max_batch, exact=False, fp8=False, kv8=False, max_prompt=24, max_ctx=None):
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    if fp8:
        cfg.decode_weight_dtype = "fp8"
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=sg.WEIGHT_SEED).items()}
    with _lib.tuning(kv_fp8=int(kv8)):   # (the KV format is read when the session is created: the capacity below is never outgrown)
        model = EmmaXForActionPrediction(cfg, dict(sd)).to(device, max_batch=max_batch, max_prompt=max_prompt, max_ctx=max_ctx, exact=exact)
    return model, cfg, sd


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def _external_loop(model, rows, fr, params, N, n):
    """On the same group session: prefill (fork), then n times last_logits -> sample_logits(subseqs = row, steps = t) ->
    set_current_tokens -> decode_step."""
    from emmax.sampling import sample_logits

    eng, R = model.engine, len(rows) * N
    model._prefill(rows, frames_u8=fr, max_new=n + 2, sampling=params, num_samples=N)
    assert eng.sample_groups == N
    ids = np.zeros((R, n), dtype=np.int64)
    lps = np.zeros((R, n), dtype=np.float32)
    for t in range(n):
        lg = eng.last_logits()
        assert lg.shape[0] == R
        tok, lp = sample_logits(lg.contiguous(), params, subseqs=list(range(R)), steps=t)
        ids[:, t] = tok.cpu().numpy()
        lps[:, t] = lp.cpu().numpy()
        eng.set_current_tokens(tok.tolist())
        eng.decode_step()
    return ids, lps


def _check_in_step_equals_loop(model, rows, fr, params, N, n):
    """Test 1's comparison; returns the ids [G N, n]."""
    R = len(rows) * N
    ids, lens, lp = model.generate_ids(rows, frames_u8=fr, max_new_tokens=n, stop_on_eos=False, sampling=params, return_logprobs=True,
                                       num_samples=N)
    assert model.engine.sample_groups == N and tuple(ids.shape) == (R, n) and tuple(lp.shape) == (R, n)
    ids, lens, lp = ids.cpu().numpy(), lens.cpu().numpy(), lp.cpu().numpy()
    assert (lens == n).all()
    want_ids, want_lp = _external_loop(model, rows, fr, params, N, n)
    for r in range(R):
        assert ids[r].tolist() == want_ids[r].tolist(), (r, ids[r].tolist(), want_ids[r].tolist())
        assert _bits(lp[r]).tolist() == _bits(want_lp[r]).tolist(), r
    return ids


def _diverged(ids, G, N):
    return all(len({tuple(ids[g * N + j].tolist()) for j in range(N)}) >= 2 for g in range(G))


@pytest.mark.parametrize("exact", [False, True])
def test_the_draw_is_the_steps_own(device, exact):
    """G = 2, N = 3, mixed per-row temperature / top-k / top-p with row 0 greedy, 16 steps, default and exact numerics."""
    from oracle import emmax_oracle as orc

    model, cfg, sd = _tiny_model(device, 6, exact=exact)
    frames, rows = sg.inputs("mixed")
    fr = torch.from_numpy(frames).to(device)
    params, N, n = sg.params("mixed"), sg.CASES["mixed"][2], 16
    assert params[0].temperature == 0.0 and len({(p.temperature, p.top_k, p.top_p) for p in params}) >= 4
    ids = _check_in_step_equals_loop(model, rows, fr, params, N, n)
    assert _diverged(ids, 2, N), ids[:, :4]
    # row 0 (temperature 0) equals the greedy ids of a plain one-row run.  (Another batch size, so other kernels: the count printed below says
    # on how many of the steps the fp32 oracle's top-2 margin, teacher-forced on the greedy run, clears the a-priori id line of the numerics
    # mode -- conftest.py -- i.e. where equality follows from the error budget alone; on this nearly flat model that is none in default
    # numerics, and the ids are equal all the same.)
    one, _ = model.generate_ids(rows[:1], frames_u8=fr[:1], max_new_tokens=n, stop_on_eos=False)
    assert model.engine.sample_groups == 0 and not model.engine.sampling
    one = one[0].cpu().tolist()
    sd32 = {k: v.float() for k, v in sd.items()}
    logits, _, _ = orc.vla_prefill_logits(torch.tensor([rows[0] + one]), orc.preprocess_frames(frames[:1], cfg), sd32, cfg)
    L = logits[0, -n - 1:-1].float().numpy()
    budget = ID_BUDGET_EXACT if exact else ID_BUDGET_TINY
    clear = sum(int(np.sort(L[t])[-1] - np.sort(L[t])[-2] > 2 * budget * np.abs(L[t]).max()) for t in range(n))
    print(f"greedy row against the one-row run (exact={exact}): {clear} of {n} steps above the id line; group row {ids[0].tolist()} one-row run {one}")
    assert ids[0].tolist() == one


def _oracle_rows(orc, sd32, cfg, proj, prompt, got):
    """fp32 oracle logits in front of every emitted token: [len(got), vocab]"""
    ids = torch.tensor([prompt + list(got)], dtype=torch.long)
    logits, _ = orc.llama_forward(orc.splice(ids, proj, sd32), sd32, cfg.llm, None)
    return logits[0, -len(got) - 1:-1].float().numpy()


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("case", ["cross", "ctx64", "ctx63", "long"])
def test_cache_follows_the_fork_against_the_oracle(device, exact, case):
    """The four contexts of the beam test: prompt 50 + 24 new tokens (crosses a page boundary), prompt 64 (context % 64 == 0: no copy), prompt
    63, prompt 20 + 136 new tokens (G = 1, N = 2: two pages per row).  Every row's raw logits at every step within the budget of the
    oracle teacher-forced on that row's own ids -- which holds only if each row reads its own cache behind the shared prompt pages."""
    from oracle import emmax_oracle as orc

    T = {"cross": 24, "ctx64": 8, "ctx63": 8, "long": 136}[case]
    N, G = sg.CASES[case][2], len(sg.CASES[case][1])
    model, cfg, sd = _tiny_model(device, 8, exact=exact, max_prompt=64, max_ctx=256 + 64 + 140 + 1)
    frames, rows = sg.inputs(case)
    assert (256 + len(rows[0])) % 64 == {"cross": 50, "ctx64": 0, "ctx63": 63, "long": 20}[case]
    fr = torch.from_numpy(frames).to(device)
    V = cfg.llm.vocab_size
    lg = torch.full((T, G * N, V), float("nan"), dtype=torch.float32, device=device)
    ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=T, stop_on_eos=False, sampling=sg.params(case), logits=lg, num_samples=N)
    ids, lg = ids.cpu().numpy(), lg.cpu().numpy()
    assert (lens.cpu().numpy() == T).all() and np.isfinite(lg).all()
    assert _diverged(ids, G, N), ids[:, :4]
    sd32 = {k: v.float() for k, v in sd.items()}
    tol = 1e-4 if exact else ID_BUDGET_TINY
    worst = 0.0
    for g in range(G):
        proj = orc.projector(orc.vision_backbone(orc.preprocess_frames(frames[g: g + 1], cfg), sd32, cfg), sd32)
        for j in range(N):
            r = g * N + j
            ref = _oracle_rows(orc, sd32, cfg, proj, rows[g], ids[r].tolist())
            err = np.abs(lg[:, r] - ref).max(axis=1) / np.abs(ref).max(axis=1)
            worst = max(worst, float(err.max()))
            assert (err <= tol).all(), (case, r, int(np.argmax(err)), float(err.max()))
    print(f"{case} exact={exact}: worst |logit err| / max|logit| over {G * N} rows x {T} steps = {worst:.3e} (line {tol:.1e})")


def test_bit_identity_with_a_private_cache(device):
    """Exact numerics, G = 1, N = 2, 70 tokens from context 296 (crosses a page boundary): each row's recorded logits equal, bit for bit, a
    fresh one-row session teacher-forced through that row's ids (batches of 1 and 2 rows run the same exact-numerics kernels).  And two rows
    with the same (seed, subseq) stay bit-identical at every step."""
    T, N = 70, 2
    model, cfg, sd = _tiny_model(device, 2, exact=True, max_prompt=64, max_ctx=256 + 64 + 80)
    frames, rows = sg.inputs("private")
    assert 256 + len(rows[0]) == 296
    fr = torch.from_numpy(frames).to(device)
    V = cfg.llm.vocab_size
    params = sg.params("private")
    lg = torch.full((T, N, V), float("nan"), dtype=torch.float32, device=device)
    ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=T, stop_on_eos=False, sampling=params, logits=lg, num_samples=N)
    ids, lgh = ids.cpu().numpy(), lg.cpu().numpy()
    assert _diverged(ids, 1, N)
    single, _, _ = _tiny_model(device, 1, exact=True, max_prompt=64, max_ctx=256 + 64 + 80)
    for j in range(N):
        o = single(input_ids=torch.tensor([rows[0]]), frames_u8=fr[:1], use_cache=True)
        got = [single.engine.last_logits()[0].cpu().numpy()]   # (the decode lm-head over the prefill's last row, as the group run took it)
        for t in range(1, T):
            o = single(input_ids=torch.tensor([[int(ids[j, t - 1])]]), past_key_values=o.past_key_values)
            got.append(o.logits[0, -1].float().cpu().numpy())
        diff = [float(np.abs(lgh[t, j] - got[t]).max()) for t in range(T)]
        print(f"row {j}: teacher-forced one-row session, steps that differ {sum(d > 0 for d in diff)} of {T}, max |diff| {max(diff)}")
        for t in range(T):
            assert np.array_equal(_bits(lgh[t, j]), _bits(got[t])), (j, t, diff[t])
    # the same (seed, subseq) on both rows
    eng = model.engine
    lg.fill_(float("nan"))
    eng.set_sampling(params, subseqs=[0, 0])
    eng.set_scores(None, lg, T, rows=N)
    eng.prefill(rows, eng.vision_encode(fr))
    ids2, lens2, lp2 = eng.generate(T, False, return_logprobs=True)
    eng.set_scores(None, None)
    ids2, lp2, lg2 = ids2.cpu().numpy(), lp2.cpu().numpy(), lg.cpu().numpy()
    assert ids2[0].tolist() == ids2[1].tolist() == ids[0].tolist()   # (row 0 of the first run drew with subseq 0 too)
    assert np.array_equal(_bits(lp2[0]), _bits(lp2[1])) and np.array_equal(_bits(lg2[:, 0]), _bits(lg2[:, 1]))


@pytest.mark.parametrize("fmt", ["fp8", "kv8"])
def test_formats_fp8_weights_and_fp8_cache(device, fmt):
    """Test 1's comparison on fp8 decode weights and on the fp8 KV cache (four planes per layer go through the copy)."""
    model, cfg, _ = _tiny_model(device, 6, fp8=fmt == "fp8", kv8=fmt == "kv8")
    frames, rows = sg.inputs("mixed")
    ids = _check_in_step_equals_loop(model, rows, torch.from_numpy(frames).to(device), sg.params("mixed"), 3, 16)
    assert len({tuple(r.tolist()) for r in ids}) >= 2


def test_formats_mxfp4(device):
    """Test 1's comparison on an MXFP4 model: the G4 shape of tests/mxfp4_ref.py, G = 2 prompts x N = 4 samples = its 8 rows."""
    import mxfp4_ref as M
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.sampling import SamplingParams

    model = EmmaXForActionPrediction(M.e2e_cfg(), dict(M.e2e_state_dict(False, M.E2E_RANDOM_SEED))).to(device, max_batch=8, max_prompt=40)
    assert model.config.decode_weight_dtype == "mxfp4" and model.engine.max_decode_batch() >= 8
    frames, rows = M.e2e_inputs(2, [17, 9], seed=2024)
    params = [SamplingParams([0.0, 1.0, 0.7, 1.4][r % 4], [0, 0, 50, 0][r % 4], 1.0, seed=300) for r in range(8)]
    ids = _check_in_step_equals_loop(model, rows, torch.from_numpy(frames).to(device), params, 4, 16)
    assert len({tuple(r.tolist()) for r in ids}) >= 2


def _run_groups(model, rows, fr, params, N, T, subseqs=None, graph=False):
    """A group generation at the engine's level (row r draws with subseqs[r]); returns host ids, lens and log-probabilities."""
    from emmax import _lib

    eng = model.engine
    eng.ensure_capacity(len(rows) * N, max(len(r) for r in rows), T)
    patches = eng.vision_encode(fr)
    if eng.beams:
        eng.clear_beams()
    eng.set_sampling(params, subseqs=subseqs)
    eng.set_sample_groups(N)
    with _lib.tuning(graph=int(graph)):
        eng.prefill(rows, patches)
        ids, lens, lp = eng.generate(T, False, return_logprobs=True)
        assert eng.graph_active() == bool(graph)
    return ids.cpu().numpy(), lens.cpu().numpy(), lp.cpu().numpy()


def test_graph_replay_independent_groups_and_the_session_is_left_as_found(device):
    from emmax import _lib

    T, N, G = 20, 2, 3
    model, cfg, _ = _tiny_model(device, 6, exact=True)
    eng = model.engine
    frames, rows = sg.inputs("indep")
    fr = torch.from_numpy(frames).to(device)
    params = sg.params("indep")
    ws0, kv0 = C.c_int64(), C.c_int64()
    with _lib.tuning(exact=1):
        assert eng.lib.emmax_session_bytes(eng._model, 6, 24, 793, C.byref(ws0), C.byref(kv0)) == 0
    before, before_lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=T, stop_on_eos=False)
    before = before.cpu()
    eager = _run_groups(model, rows, fr, params, N, T)
    graph = _run_groups(model, rows, fr, params, N, T, graph=True)
    assert np.array_equal(eager[0], graph[0]) and np.array_equal(eager[1], graph[1]) and np.array_equal(_bits(eager[2]), _bits(graph[2]))
    assert _diverged(eager[0], G, N)
    # exact numerics: a group's ids do not depend on which other groups ran with it (its rows keep their seeds and subseqs)
    for g in range(G):
        one = _run_groups(model, rows[g: g + 1], fr[g: g + 1], params[g * N: (g + 1) * N], N, T, subseqs=[g * N + j for j in range(N)])
        assert np.array_equal(one[0], eager[0][g * N: (g + 1) * N]), g
        # (2 rows and 6 rows run different exact-numerics kernels: the same ids, log-probabilities to the last bits -- as test_sampled_decode_gpu.py
        # compares slot serving with bs = 1)
        assert np.abs(one[2] - eager[2][g * N: (g + 1) * N]).max() <= 1e-4, g
    # groups off again: the greedy generation of before, the identity page table, the same session bytes
    assert eng.sample_groups == N
    after, after_lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=T, stop_on_eos=False)
    assert eng.sample_groups == 0 and not eng.sampling
    assert torch.equal(before, after.cpu()) and torch.equal(before_lens.cpu(), after_lens.cpu())
    ws1, kv1 = C.c_int64(), C.c_int64()
    with _lib.tuning(exact=1):
        assert eng.lib.emmax_session_bytes(eng._model, 6, 24, 793, C.byref(ws1), C.byref(kv1)) == 0
    assert (ws0.value, kv0.value) == (ws1.value, kv1.value)
    assert kv1.value == 3 * 2 * 6 * 13 * 2 * 64 * 128 * 3   # 3 layers x K and V x 6 rows x 13 pages x 2 kv heads x 64 tokens x 128 x 24 bits: no spare pages


def test_refusals_name_their_cause(device):
    from emmax.sampling import BeamParams, SamplingParams

    model, cfg, _ = _tiny_model(device, 8)
    eng, lib = model.engine, model.engine.lib
    st = None
    err = lambda: lib.emmax_last_error().decode()
    assert lib.emmax_session_sample_groups(eng._session) == 0
    for n in (1, 0, -2, 9):   # outside 2 .. min(max_batch, the model's decode batch) = 8
        assert lib.emmax_session_set_sample_groups(eng._session, n, st) == -1 and "samples per group" in err(), n
    assert lib.emmax_session_clear_sample_groups(eng._session, st) == 0   # off already: nothing to do
    # beams on / groups on exclude each other
    eng.set_beams(BeamParams(2))
    assert lib.emmax_session_set_sample_groups(eng._session, 2, st) == -5 and "beams" in err()
    eng.clear_beams()
    eng.set_sample_groups(4)
    assert lib.emmax_session_sample_groups(eng._session) == 4 and eng.sample_groups == 4
    assert lib.emmax_session_set_beams(eng._session, 2, C.c_double(1.0), 0, st) == -5 and "sample groups" in err()
    assert lib.emmax_slots_open(eng._session, 2, st) == -5 and "sample groups" in err()
    # a prefill with groups on: sampling off is an error (N identical greedy rows), and G x N must fit
    frames = np.zeros((3, 224, 224, 3), dtype=np.uint8)
    patches = eng.vision_encode(torch.from_numpy(frames).to(device))
    rows = [[1, 5, 6, 7], [1, 8, 9], [1, 10, 11, 12]]
    if eng.sampling:
        eng.clear_sampling()
    with pytest.raises(Exception, match="-5.*sampling"):
        eng.prefill(rows[:1], patches[:1])
    eng.set_sampling(SamplingParams(1.0, 0, 1.0, seed=1), n=8)
    with pytest.raises(Exception, match=r"-1.*3 groups x 4 samples"):
        eng.prefill(rows, patches)
    eng.prefill(rows[:2], patches[:2])   # 2 x 4 = 8 rows fit
    ids, lens = eng.generate(4, False)
    assert tuple(ids.shape) == (8, 4)
    # slots open / groups: closed over
    eng.clear_sample_groups()
    assert lib.emmax_session_sample_groups(eng._session) == 0
    eng.slots_open(2)
    assert lib.emmax_session_set_sample_groups(eng._session, 2, st) == -5 and "slots" in err()
    assert lib.emmax_session_sample_groups(None) == -1


def _op_cfg():
    from emmax.config import EmmaXConfig, LlmConfig

    tiny = EmmaXConfig.tiny()
    llm = LlmConfig(hidden_size=4096, intermediate_size=11008, num_layers=2, num_heads=32, num_kv_heads=32, head_dim=128, vocab_size=32064,
                    max_position=2048)
    return EmmaXConfig(tiny.towers, llm, norm_stats=tiny.norm_stats)


def test_operating_point_16_and_40_rows(device):
    """7B layer dimensions (2 layers): G = 2, N = 8 (16 rows) and G = 5, N = 8 (40 rows: lm-head launches of 32 + 8, each followed by its own
    finish -- at the fork too).  Five steps, test 1's comparison."""
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.sampling import SamplingParams
    from emmax.weights import synthetic_state_dict

    cfg = _op_cfg()
    sd_bf = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=21).items()}
    model = EmmaXForActionPrediction(copy.deepcopy(cfg), sd_bf).to(device, max_batch=40, max_prompt=32, max_ctx=256 + 32 + 40)
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, size=(5, 224, 224, 3), dtype=np.uint8)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=int(n))] for n in rng.integers(8, 24, size=5)]
    fr = torch.from_numpy(frames).to(device)
    grid = [(1.0, 50, 1.0), (0.8, 0, 0.9), (1.3, 20, 0.95), (0.0, 0, 1.0), (2.0, 0, 1.0), (0.6, 5, 0.7)]
    for G in (2, 5):
        params = [SamplingParams(*grid[r % len(grid)], seed=100 + 7 * r) for r in range(G * 8)]
        ids = _check_in_step_equals_loop(model, rows[:G], fr[:G], params, 8, 5)
        assert len({tuple(r.tolist()) for r in ids}) >= 2
