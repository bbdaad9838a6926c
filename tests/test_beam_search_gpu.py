"""Beam search inside the decode step on a real MI355X (include/emmax.h ABI 9; emma-x_amd/csrc/beam.hip).

The tiny synthetic model is nearly flat (adjacent candidates differ by about one fp32 ulp of the score), so nothing here depends on which
of two near-equal candidates wins.  Instead:
  1. the SELECTION is replayed bit for bit by tests/beam_ref.py from the device's own raw logit rows, lse values and running scores;
  2. the CACHE is checked against the fp32 oracle: the sequence the trace gives every running beam, run through the oracle from scratch,
     must give the logit row the device recorded for that beam -- which it only does if the page table followed the parents;
  3. the same on the device alone (teacher-forced bs = 1 session, exact numerics, bit for bit).
The only tolerance on the selection is on lse itself: |lse - float64 log-sum-exp| <= 1e-5 max(1, |lse|) (an fp32 tree sum of 32064 terms
errs by about log2(V) 2^-24 ~ 1e-6 relative, expf / logf by a few ulp; the line leaves a factor of about 5)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
from conftest import ID_BUDGET_TINY  # noqa: E402

pytestmark = pytest.mark.gpu

# emmax_session_bytes(tiny configuration, max_batch 8, max_prompt 24, max_ctx 793): the KV bytes the PARENT commit's build returned on an
# MI355X (3 layers x K and V x 8 rows x 13 pages x 2 kv heads x 64 tokens x 128 x 2 bytes).  Beams must not grow them
PARENT_KV_BYTES_TINY_8 = 3 * 2 * 8 * 13 * 2 * 64 * 128 * 2


def _tiny_model(device, max_batch, exact=False, fp8=False, kv8=False, seed=6, max_prompt=24, max_ctx=None, eos=None):
    from emmax import _lib
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    if fp8:
        cfg.decode_weight_dtype = "fp8"
    if eos is not None:
        cfg.eos_token_id = eos
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=seed).items()}
    with _lib.tuning(kv_fp8=int(kv8)):   # (the KV format is read when the session is created: the capacity below is never outgrown)
        model = EmmaXForActionPrediction(cfg, dict(sd)).to(device, max_batch=max_batch, max_prompt=max_prompt, max_ctx=max_ctx, exact=exact)
    return model, cfg, sd


def _inputs(B, seed=21, lens=None, lo=6, hi=20):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(B, 224, 224, 3), dtype=np.uint8)
    lens = list(lens) if lens is not None else [int(n) for n in rng.integers(lo, hi, size=B)]
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=n - 1)] for n in lens]
    return frames, rows


def _run(model, rows, fr, T, beams, graph=False, stop_on_eos=False, want_logits=True):
    """One beam generation; returns host copies of the result, the trace and the recorded raw logit rows."""
    from emmax import _lib

    eng, K, G = model.engine, beams.num_beams, len(rows)
    V = model.config.llm.vocab_size
    lg = torch.full((T, G * K, V), float("nan"), dtype=torch.float32, device=fr.device) if want_logits else None
    with _lib.tuning(graph=int(graph)):
        ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=T, stop_on_eos=stop_on_eos, logits=lg, beams=beams)
        assert eng.beams == K
        if T > 2:
            assert eng.graph_active() == bool(graph)
    seq, ln, sc, bix = [x.cpu().numpy() for x in eng.beam_result()]
    tr = {k: v.cpu().numpy() for k, v in eng.beam_trace().items()}
    assert np.array_equal(ids.cpu().numpy().reshape(G, K, T), seq) and np.array_equal(lens.cpu().numpy().reshape(G, K), ln)
    return {"seq": seq, "len": ln, "score": sc, "bidx": bix, "tr": tr, "lg": lg.cpu().numpy() if want_logits else None}


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def _replay(out, G, K, V, T, eos, pad, lp, es):
    """Check 1: beam_ref over the device's raw rows, lse values and running scores reproduces every step and the result bit for bit."""
    tr, lg = out["tr"], out["lg"]
    groups = []
    for g in range(G):
        grp = beam_ref.BeamGroup(K, V, T, eos, lp, es)
        for t in range(T):
            if tr["tok"][t, g, 0] < 0 and tr["cand_idx"][t, g, 0] < 0:   # the group did not run this step
                assert grp.done, (g, t)
                assert (tr["tok"][t:, g] == -1).all() and (tr["parent"][t:, g] == -1).all()
                break
            assert not grp.done, (g, t)
            n = 1 if t == 0 else K
            rows = lg[t, g * K: g * K + n]
            lses = tr["lse"][t, g, :n]
            for r in range(n):
                want = float(beam_ref.lse_f64(rows[r]))
                print(f"lse g={g} t={t} r={r}: device {float(lses[r])!r} float64 {want!r}") if t < 2 and g == 0 else None
                assert abs(float(lses[r]) - want) <= 1e-5 * max(1.0, abs(want)), (g, t, r, float(lses[r]), want)
            rec = grp.step(rows, lses=lses, scores=None if t == 0 else tr["score"][t - 1, g])
            assert rec["cand_idx"] == tr["cand_idx"][t, g].tolist(), (g, t)
            assert np.array_equal(_bits(rec["cand_acc"]), _bits(tr["cand_acc"][t, g])), (g, t)
            assert rec["tok"] == tr["tok"][t, g].tolist() and rec["parent"] == tr["parent"][t, g].tolist(), (g, t)
            assert np.array_equal(_bits(rec["score"]), _bits(tr["score"][t, g])), (g, t)
        seqs, lens, scores, bidx = grp.result(pad, row0=g * K)
        assert np.array_equal(seqs, out["seq"][g]) and np.array_equal(lens, out["len"][g]), g
        assert np.array_equal(_bits(scores), _bits(out["score"][g])), (g, scores, out["score"][g])
        assert np.array_equal(bidx, out["bidx"][g]), g
        groups.append(grp)
    return groups


MODES = {"default": {}, "exact": {"exact": True}, "fp8": {"fp8": True}, "kv8": {"kv8": True}}


def _op_cfg():
    from emmax.config import EmmaXConfig, LlmConfig

    tiny = EmmaXConfig.tiny()
    llm = LlmConfig(hidden_size=4096, intermediate_size=11008, num_layers=2, num_heads=32, num_kv_heads=32, head_dim=128, vocab_size=32064,
                    max_position=2048)
    return EmmaXConfig(tiny.towers, llm, norm_stats=tiny.norm_stats)


@pytest.fixture(scope="module")
def op_sd():
    """The 7B-layer-dimension, 2-layer synthetic model of the operating-point tests: it takes decode batches of up to 64 rows."""
    from emmax.weights import synthetic_state_dict

    return {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(_op_cfg(), seed=21).items()}


def _op_model(op_sd, device, fp8=False, kv8=False, max_batch=64):
    from emmax import _lib
    from emmax.modeling import EmmaXForActionPrediction

    cfg = _op_cfg()
    if fp8:
        cfg.decode_weight_dtype = "fp8"
    with _lib.tuning(kv_fp8=int(kv8)):
        return EmmaXForActionPrediction(cfg, dict(op_sd)).to(device, max_batch=max_batch, max_prompt=32, max_ctx=256 + 32 + 40), cfg


@pytest.mark.parametrize("mode", list(MODES))
def test_selection_is_bit_exact(device, mode, op_sd):
    """Every numerics mode; eager and graph; G in {1, 3}; K in {2, 4, 8}; the three early_stopping values and length penalties 0, 1, 2 in
    rotation.  Outside exact numerics the tiny configuration decodes at most 8 rows: the combinations of more rows (3 groups of 4 or 8
    beams) run on the 7B-layer-dimension model, which takes 64."""
    from emmax.sampling import BeamParams

    model, cfg, _ = _tiny_model(device, 24 if mode == "exact" else 8, **MODES[mode])
    big = None
    V, T = cfg.llm.vocab_size, 10
    combos = [(K, G, graph) for K in (2, 4, 8) for G in (1, 3) for graph in (False, True)]
    for i, (K, G, graph) in enumerate(combos):
        m = model
        if G * K > model.engine.max_decode_batch():
            if big is None:
                big, _ = _op_model(op_sd, device, fp8=mode == "fp8", kv8=mode == "kv8", max_batch=24)
            m = big
        frames, rows = _inputs(G, seed=40 + G)
        fr = torch.from_numpy(frames).to(device)
        lp, es = (0.0, 1.0, 2.0)[i % 3], (False, True, "never")[(i // 3) % 3]
        out = _run(m, rows, fr, T, BeamParams(K, lp, es, K), graph=graph)
        _replay(out, G, K, V, T, -1, cfg.pad_token_id, lp, es)
        assert (out["len"] == T).all() and (np.diff(out["score"].astype(np.float64), axis=1) <= 0).all()


def _oracle_rows(orc, sd32, cfg, proj, prompt, seqs):
    ids = torch.tensor([prompt + list(s) for s in seqs], dtype=torch.long)
    emb = orc.splice(ids, proj.expand(len(seqs), -1, -1), sd32)
    logits, _ = orc.llama_forward(emb, sd32, cfg.llm, None)
    return logits[:, -1].float().numpy()


def _check_cache_against_oracle(out, groups, rows, frames, cfg, sd, K, T, tol, every=1):
    """Check 2.  Returns (steps where two beams share a parent, steps where a beam's parent is not itself)."""
    from oracle import emmax_oracle as orc

    sd32 = {k: v.float() for k, v in sd.items()}
    shared = moved = 0
    worst = 0.0
    for g, grp in enumerate(groups):
        proj = orc.projector(orc.vision_backbone(orc.preprocess_frames(frames[g: g + 1], cfg), sd32, cfg), sd32)
        ref0 = _oracle_rows(orc, sd32, cfg, proj, rows[g], [[]])[0]
        err = np.abs(out["lg"][0, g * K] - ref0).max() / np.abs(ref0).max()
        worst = max(worst, float(err))
        assert err <= tol, (g, 0, err)
        for t in range(1, len(grp.tok)):
            par = grp.par[t]
            shared += int(len(set(par)) < K)
            moved += int(any(p != k for k, p in enumerate(par)))
            if t % every and t != len(grp.tok) - 1:
                continue
            seqs = [grp.lineage(t - 1, k)[0] for k in range(K)]   # what running beam k had emitted when step t read its row
            ref = _oracle_rows(orc, sd32, cfg, proj, rows[g], seqs)
            got = out["lg"][t, g * K: (g + 1) * K]
            err = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
            worst = max(worst, float(err.max()))
            assert (err <= tol).all(), (g, t, err)
    print(f"cache vs oracle: worst |logit err| / max|logit| = {worst:.3e} (line {tol:.1e}); shared-parent steps {shared}, moved-parent steps {moved}")
    return shared, moved


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("case", ["cross", "ctx64", "ctx63", "long"])
def test_cache_follows_the_beams_against_the_oracle(device, exact, case):
    """Contexts: one that crosses a page boundary while generating, one that ends exactly on a page (context % 64 == 0), one a token before
    it (== 63), and one run of more than 128 new tokens (every beam fills two pages).  Patches are 256 rows: context = 256 + prompt ids."""
    from emmax.sampling import BeamParams

    plen, T, K = {"cross": (50, 24, 4), "ctx64": (64, 8, 4), "ctx63": (63, 8, 4), "long": (20, 136, 2)}[case]
    model, cfg, sd = _tiny_model(device, 8, exact=exact, max_prompt=64, max_ctx=256 + 64 + 140 + 1)
    G = 2 if case != "long" else 1
    frames, rows = _inputs(G, seed=50, lens=[plen] * G)
    fr = torch.from_numpy(frames).to(device)
    out = _run(model, rows, fr, T, BeamParams(K, 1.0, False, K))
    groups = _replay(out, G, K, cfg.llm.vocab_size, T, -1, cfg.pad_token_id, 1.0, False)
    tol = 1e-4 if exact else ID_BUDGET_TINY
    shared, moved = _check_cache_against_oracle(out, groups, rows, frames, cfg, sd, K, T, tol, every=1)
    assert shared >= 1 and moved >= 1, "the parents are the identity in this run: the test shows nothing"


def test_winning_lineage_equals_a_teacher_forced_single_row_session(device):
    """Check 3, exact numerics: the rows recorded along the best hypothesis' lineage equal, bit for bit, the raw logits of a fresh bs = 1
    session that is fed the same tokens.  One group of two beams: batches of 1 and 2 rows run the same exact-numerics kernels
    (decode_ks.hip), so the comparison is between the same arithmetic on a private cache and on the shared, reordered one; 70 tokens from a
    context of 296 cross a page boundary."""
    from emmax.sampling import BeamParams

    K, T = 2, 70
    model, cfg, sd = _tiny_model(device, 2, exact=True, max_prompt=64, max_ctx=256 + 64 + 80)
    frames, rows = _inputs(1, seed=61, lens=[40])
    fr = torch.from_numpy(frames).to(device)
    out = _run(model, rows, fr, T, BeamParams(K, 1.0, False, 1))
    assert (out["tr"]["parent"][1:, 0] != np.arange(K)[None, :]).any()
    single, _, _ = _tiny_model(device, 1, exact=True, max_prompt=64, max_ctx=256 + 64 + 80)
    best, bix = out["seq"][0, 0], out["bidx"][0, 0]
    o = single(input_ids=torch.tensor([rows[0]]), frames_u8=fr[:1], use_cache=True)
    got = [single.engine.last_logits()[0].cpu().numpy()]   # (the decode lm-head over the prefill's last row, as the beam run took it)
    for t in range(1, T):
        o = single(input_ids=torch.tensor([[int(best[t - 1])]]), past_key_values=o.past_key_values)
        got.append(o.logits[0, -1].float().cpu().numpy())
    diff = [float(np.abs(out["lg"][t, int(bix[t])] - got[t]).max()) for t in range(T)]
    print("teacher-forced bs = 1 against the winning lineage: steps that differ", sum(d > 0 for d in diff), "of", T, "max |diff|", max(diff))
    for t in range(T):
        assert np.array_equal(_bits(out["lg"][t, int(bix[t])]), _bits(got[t])), (t, diff[t])


def test_eos_and_stopping(device):
    """An EOS planted on a token some beams emit early: hypotheses of different lengths; early_stopping=True stops once K are finished,
    "never" runs on; the replay (check 1) holds throughout."""
    from emmax.sampling import BeamParams

    K, T = 4, 24
    model, cfg, _ = _tiny_model(device, 8)
    frames, rows = _inputs(2, seed=71)
    fr = torch.from_numpy(frames).to(device)
    free = _run(model, rows, fr, T, BeamParams(K, 1.0, False, K))
    toks = free["tr"]["tok"][2:8].reshape(-1)
    vals, counts = np.unique(toks[toks >= 0], return_counts=True)
    eos = int(vals[np.argmax(counts)])
    model, cfg, _ = _tiny_model(device, 8, eos=eos)
    runs = {}
    for es in (True, False, "never"):
        out = _run(model, rows, fr, T, BeamParams(K, 1.0, es, K), stop_on_eos=True)
        _replay(out, 2, K, cfg.llm.vocab_size, T, eos, cfg.pad_token_id, 1.0, es)
        runs[es] = out
        for g in range(2):
            for k in range(K):
                n = int(out["len"][g, k])
                row = out["seq"][g, k]
                assert eos not in row[: n - 1].tolist() and (row[n:] == cfg.pad_token_id).all() and (out["bidx"][g, k, n:] == -1).all()
                assert row[n - 1] == eos or n == T
    steps = {es: int((runs[es]["tr"]["tok"][:, :, 0] >= 0).sum(axis=0).max()) for es in runs}
    print("steps run per early_stopping value:", steps, "lengths:", {str(es): runs[es]["len"].tolist() for es in runs})
    assert any(len(set(runs[es]["len"][g].tolist())) > 1 for es in runs for g in range(2)), "no hypotheses of different lengths"
    assert steps[True] <= steps[False] <= steps["never"] and steps[True] < T
    # early_stopping=True: the group stopped at the step that finished its K-th hypothesis
    for g in range(2):
        n_run = int((runs[True]["tr"]["tok"][:, g, 0] >= 0).sum())
        assert int(runs[True]["len"][g].max()) == n_run


def test_graph_replay_equals_eager_and_groups_are_independent(device):
    from emmax.sampling import BeamParams

    K, T = 4, 20
    model, cfg, _ = _tiny_model(device, 12, exact=True)
    frames, rows = _inputs(3, seed=81)
    fr = torch.from_numpy(frames).to(device)
    bp = BeamParams(K, 1.0, False, K)
    eager = _run(model, rows, fr, T, bp, graph=False)
    graph = _run(model, rows, fr, T, bp, graph=True)
    for k in ("tok", "parent", "cand_idx"):
        assert np.array_equal(eager["tr"][k], graph["tr"][k]), k
    for k in ("score", "lse", "cand_acc"):
        assert np.array_equal(_bits(eager["tr"][k]), _bits(graph["tr"][k])), k
    assert np.array_equal(eager["seq"], graph["seq"]) and np.array_equal(_bits(eager["score"]), _bits(graph["score"]))
    assert np.array_equal(_bits(eager["lg"]), _bits(graph["lg"]))
    # exact numerics: group g of the 3-group batch equals its own single-group run bit for bit
    for g in range(3):
        one = _run(model, rows[g: g + 1], fr[g: g + 1], T, bp)
        assert np.array_equal(one["seq"][0], eager["seq"][g]) and np.array_equal(_bits(one["score"][0]), _bits(eager["score"][g])), g
        assert np.array_equal(one["tr"]["tok"][:, 0], eager["tr"]["tok"][:, g]) and np.array_equal(one["tr"]["parent"][:, 0], eager["tr"]["parent"][:, g])
        assert np.array_equal(_bits(one["tr"]["score"][:, 0]), _bits(eager["tr"]["score"][:, g])), g
        assert np.array_equal(one["bidx"][0], eager["bidx"][g] - g * K * (eager["bidx"][g] >= 0)), g


def test_one_beam_is_the_greedy_path(device):
    model, cfg, _ = _tiny_model(device, 4)
    frames, rows = _inputs(2, seed=91)
    fr = torch.from_numpy(frames).to(device)
    ids = torch.full((2, max(len(r) for r in rows)), cfg.pad_token_id, dtype=torch.long)
    mask = torch.zeros_like(ids)
    for b, r in enumerate(rows):
        ids[b, : len(r)] = torch.tensor(r)
        mask[b, : len(r)] = 1
    a = model.generate(ids, attention_mask=mask, frames_u8=fr, max_new_tokens=12)
    b = model.generate(ids, attention_mask=mask, frames_u8=fr, max_new_tokens=12, num_beams=1, num_return_sequences=1)
    assert torch.equal(a, b) and model.engine.beams == 0


def test_a_beam_run_leaves_the_session_as_it_found_it(device):
    """Greedy, sampled and slot-served generations after a beam run on the same session equal the ones before it; beams cleared: the step is
    what it was (graph replay active as before)."""
    from emmax import _lib
    from emmax.sampling import BeamParams, SamplingParams
    from emmax.serving import Request, SlotScheduler

    model, cfg, _ = _tiny_model(device, 8)
    frames, rows = _inputs(4, seed=95)
    fr = torch.from_numpy(frames).to(device)
    samp = SamplingParams(0.8, 20, 0.95, seed=5)

    def everything():
        eng = model.engine

        def encode(fs):
            pe = eng.vision_encode(torch.stack(fs))
            return [pe[i] for i in range(len(fs))]

        sched = SlotScheduler(eng, encode, n_slots=3, poll_every=3, overlap=False)   # (after a beam run: the scheduler turns beams off)
        for i in range(4):
            sched.submit(Request(i, fr[i], rows[i], max_new_tokens=10))
        served = {r.rid: r.ids for r in sched.run()}
        s_ids, s_lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=16, stop_on_eos=False, sampling=samp)
        with _lib.tuning(graph=1):   # (last: a plain prefill closes the request slots, which beams cannot be turned on over)
            g_ids, g_lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=16, stop_on_eos=False)
            g_graph = model.engine.graph_active()
        return g_ids.cpu(), g_lens.cpu(), g_graph, s_ids.cpu(), s_lens.cpu(), served

    before = everything()
    assert model.engine.beams == 0
    out = _run(model, rows[:2], fr[:2], 70, BeamParams(4, 1.0, False, 4))   # crosses a page boundary: shared pages, spares, fresh pages
    assert (out["tr"]["parent"][1:] != np.arange(4)[None, None, :]).any()
    after = everything()
    assert model.engine.beams == 0
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and before[2] == after[2] is True
    assert torch.equal(before[3], after[3]) and torch.equal(before[4], after[4])
    assert before[5] == after[5]


def test_session_bytes_do_not_grow(device):
    """emmax_session_bytes for 8 rows: the KV bytes equal what the parent commit's build returns for the same arguments (tiny configuration,
    max_batch 8, max_prompt 24, max_ctx 793; the constant was printed by the parent build).  The workspace grows by the beam state and
    trace (32 bytes per row and step of max_ctx)."""
    import ctypes as C

    model, cfg, _ = _tiny_model(device, 8)
    eng = model.engine
    ws, kv = C.c_int64(), C.c_int64()
    assert eng.lib.emmax_session_bytes(eng._model, 8, 24, 256 + 24 + 512 + 1, C.byref(ws), C.byref(kv)) == 0
    print("emmax_session_bytes(tiny, 8, 24, 793): ws", ws.value, "kv", kv.value)
    assert kv.value == PARENT_KV_BYTES_TINY_8 == 20447232


def test_nomem_is_reported_up_front(device):
    """A text-only prompt shorter than two pages with a long generation: K spares + K private pages per 64 tokens exceed the rows' share."""
    from emmax import _lib

    model, cfg, _ = _tiny_model(device, 8, max_prompt=24, max_ctx=256 + 24 + 100)
    from emmax.sampling import BeamParams

    eng = model.engine
    eng.set_beams(BeamParams(4))
    try:
        # 4 tokens of context: no complete prompt page to share.  The 4 rows own 4 x 6 = 24 pages; 330 new tokens need 1 prompt page + 3 copies
        # of it + 4 spares + 4 x 5 page boundaries = 28 (300 new tokens need 24 and fit)
        eng.prefill([[1, 5, 6, 7]], None)
        with pytest.raises(_lib.EmmaxError, match="-3.*do not fit"):
            eng.generate(330)
        ids, lens = eng.generate(300, stop_on_eos=False)
        assert (lens.cpu().numpy() == 300).all()
    finally:
        eng.clear_beams()


def test_surface_at_the_operating_point(device, op_sd):
    """generate / predict_action / generate_actions (both forms) with num_beams=4 at 7B layer dimensions (2 layers): shapes, best-first
    order, the action is the one decoded from the best sequence, and 16 groups x 4 beams = 64 rows run."""
    from emmax.config import EmmaXConfig, LlmConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.sampling import BeamParams
    from emmax.tokenizer_stub import StubTokenizer
    from emmax.weights import synthetic_state_dict

    model, cfg = _op_model(op_sd, device)
    frames, rows = _inputs(16, seed=77, lo=8, hi=24)
    fr = torch.from_numpy(frames).to(device)
    K, T = 4, 12
    ids = torch.tensor([rows[0]])
    d = model.generate(ids, frames_u8=fr[:1], max_new_tokens=T, num_beams=K, num_return_sequences=K, return_dict_in_generate=True, output_logits=True)
    assert d.sequences.shape == (K, len(rows[0]) + T) and d.sequences_scores.shape == (K,) and d.beam_indices.shape == (K, T)
    sc = d.sequences_scores.cpu().numpy().astype(np.float64)
    assert (np.diff(sc) <= 0).all() and len(d.logits) == T and d.logits[0].shape == (K, cfg.llm.vocab_size)
    best = d.sequences[0, len(rows[0]):].tolist()
    one = model.generate(ids, frames_u8=fr[:1], max_new_tokens=T, num_beams=K)
    assert one.shape == (1, len(rows[0]) + T) and one[0].tolist() == d.sequences[0].tolist()
    # predict_action decodes the best hypothesis of its 7 tokens
    dim = model.get_action_dim(None)
    act = model.predict_action(ids, unnorm_key=None, frames_u8=fr[:1], num_beams=K)
    seq7, _, _, _ = model.engine.beam_result()
    from emmax.actions import token_ids_to_actions, unnormalize
    want = unnormalize(token_ids_to_actions(np.array(seq7[0, 0, :dim].cpu().tolist()), model.vocab_size, model.bin_centers), model.get_action_stats(None))
    assert act.shape == (dim,) and np.array_equal(act, want)
    # generate_actions, both forms, decode the best sequence
    tok = StubTokenizer()
    feat = {"input_ids": ids, "frames_u8": fr[:1]}
    a1, text1 = model.generate_actions(feat, tok, max_new_tokens=T, num_beams=K)
    seq_b = model.engine.beam_result()[0][0, 0].cpu().tolist()
    n_b = int(model.engine.beam_result()[1][0, 0])
    w1, wt1 = model._postprocess(seq_b[:n_b], tok, "act")
    assert text1 == wt1 and np.array_equal(np.asarray(a1), np.asarray(w1[0]))
    # native form: generate_actions(image, prompt_text, type, ...) with the model's own tokenizer
    model.tokenizer = tok
    image = frames[0]
    got, text = model.generate_actions(image=image, prompt_text="put it down", type="act", max_new_tokens=T, min_length=1, do_sample=False, num_beams=K)
    seq_n, len_n = model.engine.beam_result()[:2]
    wn, wtn = model._postprocess(seq_n[0, 0, : int(len_n[0, 0])].cpu().tolist(), tok, "act")
    assert text == wtn and len(got) == len(wn) and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, wn))
    # 16 groups x 4 beams = 64 rows
    new_ids, lens = model.generate_ids(rows, frames_u8=fr, max_new_tokens=T, stop_on_eos=False, beams=BeamParams(K, 1.0, False, 1))
    assert new_ids.shape == (64, T) and (lens.cpu().numpy() == T).all()
    sc64 = model.engine.beam_result()[2].cpu().numpy().astype(np.float64)
    assert sc64.shape == (16, K) and (np.diff(sc64, axis=1) <= 0).all() and np.isfinite(sc64).all()
    acts, bi, bl = model.generate_actions_batch(fr[:4], rows[:4], max_new_tokens=T, stop_on_eos=False, beams=BeamParams(K))
    assert acts.shape == (4, 7) and bi.shape == (4, T)
