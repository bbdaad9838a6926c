"""The further warpers and the token rules on a real MI355X (include/emmax.h: emmax_op_sample_ext, emmax_session_set_warpers,
emmax_session_set_token_rules; the EXT finish in emma-x_amd/csrc/sample.hip).  Op level: the committed rows of tests/warpers_ref.py -- every
one of which clears its lines (tests/test_warpers.py) -- against the numpy replay and HF's classes, crafted rows, the token rules on crafted
histories.  Session level on the tiny config with 2 layers: generate() with the new arguments against the replay applied to each step's
returned logit row, graph replay against eager, sample groups and slot serving."""
import numpy as np
import pytest
import torch

import warpers_ref as wr
from test_sampling_gpu import _op_sample
from test_warpers import HISTS, RULES, hf_processed, hf_warped

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _dev(a, dtype, device):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=dtype)), device=device)


def _op_ext(logits, cases, seed, subseq, n_out, hists=None, proc=None, rules=None, enable=None, eos=2, pad=32000):
    """emmax_op_sample_ext on logits [B, V] (device): cases = per row (T, top_k, top_p, min_p, typical_p, epsilon, eta); hists = per-row
    histories with proc = per row (penalty, ngram, min_new); rules = [(kind, ids, bias)] with per-row enable words.
    Returns (tokens, log-probabilities, scores [B, V])."""
    from emmax import _lib

    lib = _lib.load()
    B, V = logits.shape
    dev = logits.device
    c = np.asarray(cases, dtype=np.float64).reshape(B, 7)
    t, kk, pp = _dev(c[:, 0], np.float32, dev), _dev(c[:, 1], np.int32, dev), _dev(c[:, 2], np.float32, dev)
    warp = [_dev(c[:, j], np.float32, dev) for j in range(3, 7)]
    sd = _dev(np.asarray(seed, dtype=np.uint64).view(np.int64), np.int64, dev)
    sq = _dev(np.asarray(subseq, dtype=np.uint32).view(np.int32), np.int32, dev)
    no = _dev(n_out, np.int32, dev)
    keep_alive, pa = [], [None] * 5
    max_hist = 0
    if hists is not None:
        max_hist = max(1, max(len(h) for h in hists))
        H = np.zeros((B, max_hist), dtype=np.int32)
        for b, h in enumerate(hists):
            H[b, : len(h)] = h
        pr = np.asarray(proc if proc is not None else [(1.0, 0, 0)] * B, dtype=np.float64).reshape(B, 3)
        keep_alive = [_dev(pr[:, 0], np.float32, dev), _dev(pr[:, 1], np.int32, dev), _dev(pr[:, 2], np.int32, dev), _dev(H, np.int32, dev),
                      _dev([len(h) for h in hists], np.int32, dev)]
        pa = [x.data_ptr() for x in keep_alive]
    ra, R = [None] * 5, 0
    if rules:
        off, ids = [0], []
        for _, r, _ in rules:
            ids += list(r)
            off.append(len(ids))
        R = len(rules)
        rt = [_dev(off, np.int32, dev), _dev(ids, np.int32, dev), _dev([k | (4 if k == 3 else 0) for k, _, _ in rules], np.int32, dev),
              _dev([b for _, _, b in rules], np.float32, dev), _dev(np.asarray(enable if enable is not None else [15] * B, dtype=np.uint32).view(np.int32), np.int32, dev)]
        keep_alive += rt
        ra = [x.data_ptr() for x in rt]
    tok = torch.full((B,), -7, dtype=torch.int32, device=dev)
    lp = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    sc = torch.full((B, V), float("nan"), dtype=torch.float32, device=dev)
    ld = logits.stride(0) if B > 1 else V
    _lib.check(lib.emmax_op_sample_ext(logits.data_ptr(), ld, B, V, t.data_ptr(), kk.data_ptr(), pp.data_ptr(), sd.data_ptr(), sq.data_ptr(), no.data_ptr(),
                                       *[w.data_ptr() for w in warp], *pa, max_hist, R, *ra, eos, pad, tok.data_ptr(), lp.data_ptr(), sc.data_ptr(),
                                       _lib.current_stream()), "emmax_op_sample_ext")
    torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy(), sc.cpu().numpy()


# ---- op level: the warpers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [wr.V_BIG, wr.V_SMALL])
def test_warpers_match_replay_and_hf(device, V):
    """The committed rows in batches of 8 with a different parameter set per row: the kept set (through the scores) equals the replay's and
    HF's, the scores are z on it bit for bit, the token is the replay's draw, the log-probability that of the raw row (emmax_op_sample's bits where it draws the same token); a second launch
    is bit-equal; a row moved to another place of a smaller batch gives the same bits."""
    rows = [r for r in wr.committed_rows() if r[1] == V]
    assert len(rows) == 40
    for b0 in range(0, len(rows), 8):
        batch = rows[b0:b0 + 8]
        B = len(batch)
        l = np.stack([r[2] for r in batch])
        x = torch.from_numpy(l).to(device)
        cases = [r[3] for r in batch]
        seeds, subs, steps = [1000 + r[0] for r in batch], [r[0] % 3 for r in batch], [r[0] for r in batch]
        tok, lp, sc = _op_ext(x, cases, seeds, subs, steps)
        tok2, lp2, sc2 = _op_ext(x, cases, seeds, subs, steps)
        assert (tok == tok2).all() and (_bits(lp) == _bits(lp2)).all() and (_bits(sc) == _bits(sc2)).all()
        tok0, lp0 = _op_sample(x, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], seeds, subs, steps)
        same = tok0 == tok   # (the same noise: a row whose draw survives the warpers draws the same token, with emmax_op_sample's bits)
        assert same.any() and (_bits(lp)[same] == _bits(lp0)[same]).all()
        for b, (seed, _, lb, case) in enumerate(batch):
            rt, rlp, margin, keep, rsc = wr.sample_row_ext(lb, case, seeds[b], subs[b], steps[b])
            assert margin > wr.MARGIN
            assert ((sc[b] > -np.inf) == keep).all(), (V, seed, case, int(keep.sum()), int((sc[b] > -np.inf).sum()))
            assert ((hf_warped(lb, case) > -np.inf) == keep).all()
            assert (_bits(sc[b]) == _bits(rsc)).all()
            assert int(tok[b]) == rt and abs(float(lp[b]) - rlp) <= 1e-5, (V, seed, case, int(tok[b]), rt)
        pick = [5, 0, 6][: min(3, B)]   # other places, another B
        tok3, lp3, sc3 = _op_ext(x[pick].contiguous(), [cases[i] for i in pick], [seeds[i] for i in pick], [subs[i] for i in pick], [steps[i] for i in pick])
        assert (tok3 == tok[pick]).all() and (_bits(lp3) == _bits(lp[pick])).all() and (_bits(sc3) == _bits(sc[pick])).all()


def test_warpers_crafted_rows(device):
    V = 1000
    far = np.full(V, -40.0, dtype=np.float32)
    # min_p = 1: only the maxima stay, an exact tie at the threshold (W = 2^32 = floor(min_p 2^32)) is kept -- all three are drawn
    tie = far.copy()
    tie[[3, 500, 999]] = 2.0
    seen = set()
    for s in range(8):
        t, _, sc = _op_ext(torch.from_numpy(np.tile(tie, (8, 1))).to(device), [(1.0, 0, 1.0, 1.0, 0, 0, 0)] * 8, [s] * 8, list(range(8)), [0] * 8)
        seen |= set(int(v) for v in t)
        assert (np.flatnonzero(sc[0] > -np.inf) == [3, 500, 999]).all()
    assert seen == {3, 500, 999}
    # min_p boundary on masses 0.5, 0.3, 0.2: 0.5 keeps {0, 1} (0.3 / 0.5 >= 0.5 > 0.2 / 0.5), 0.3 keeps all three
    row = np.full(V, -60.0, dtype=np.float32)
    row[:3] = np.log(np.array([0.5, 0.3, 0.2], dtype=np.float64)).astype(np.float32)
    x = torch.from_numpy(np.tile(row, (64, 1))).to(device)
    for mp, want in ((0.5, {0, 1}), (0.3, {0, 1, 2})):
        t, _, _ = _op_ext(x, [(1.0, 0, 1.0, mp, 0, 0, 0)] * 64, [7] * 64, list(range(64)), [1] * 64)
        assert set(int(v) for v in t) == want, (mp, sorted(set(t.tolist())))
    # ... typical_p on the same masses: H = 1.0297, distances 0.336 (0.5), 0.174 (0.3), 0.580 (0.2): 0.25 keeps {1}, 0.6 keeps {0, 1}
    for ty, want in ((0.25, {1}), (0.6, {0, 1}), (0.85, {0, 1, 2})):
        t, _, sc = _op_ext(x, [(1.0, 0, 1.0, 0, ty, 0, 0)] * 64, [9] * 64, list(range(64)), [2] * 64)
        assert set(int(v) for v in t) == want and set(np.flatnonzero(sc[0] > -np.inf)) == want, (ty, sorted(set(t.tolist())))
    # ... epsilon: 0.25 drops the 0.2 entry; eta 0.9: min(0.9, sqrt(0.9) exp(-H)) = 0.339 drops 0.3 and 0.2
    for case, want in (((1.0, 0, 1.0, 0, 0, 0.25, 0), {0, 1}), ((1.0, 0, 1.0, 0, 0, 0, 0.9), {0})):
        t, _, _ = _op_ext(x, [case] * 64, [11] * 64, list(range(64)), [3] * 64)
        assert set(int(v) for v in t) == want, (case, sorted(set(t.tolist())))
    # a one-hot row (H = 0) through typical and eta keeps its entry
    hot = np.full(V, -np.inf, dtype=np.float32)
    hot[77] = 1.5
    t, _, sc = _op_ext(torch.from_numpy(np.tile(hot, (3, 1))).to(device), [(1.0, 0, 1.0, 0, 0.5, 0, 0), (1.0, 0, 1.0, 0, 0, 0, 1e-3), (0.7, 0, 1.0, 0.1, 0.9, 1e-3, 1e-3)],
                      [1, 2, 3], [0] * 3, [0] * 3)
    assert t.tolist() == [77] * 3 and all((np.flatnonzero(sc[b] > -np.inf) == [77]).all() for b in range(3))
    # warpers on a temperature-0 row change nothing: the argmax, lowest id on ties, emmax_op_sample's log-probability bits
    rnd = np.random.default_rng(1).standard_normal(V).astype(np.float32)
    rnd[[10, 700]] = rnd.max() + 1.0
    x = torch.from_numpy(rnd[None]).to(device)
    t, lp, sc = _op_ext(x, [(0.0, 5, 0.5, 0.5, 0.5, 0.1, 0.1)], [0], [0], [0])
    t0, lp0 = _op_sample(x, [0.0], [0], [1.0], [0], [0], [0])
    assert int(t[0]) == int(t0[0]) == 10 and (_bits(lp) == _bits(lp0)).all() and (_bits(sc[0]) == _bits(rnd)).all()
    # an all-NaN row gives token -1
    t, lp, _ = _op_ext(torch.full((1, V), float("nan"), device=device), [(1.0, 0, 1.0, 0.1, 0.9, 1e-3, 1e-3)], [0], [0], [0])
    assert int(t[0]) == -1 and np.isnan(lp[0])


def test_banned_entries_feed_the_warpers(device):
    """-inf entries from a ban (the three largest logits suppressed) reach the warpers as entries that are never kept: the kept set and the
    draw equal the replay's on the processed row, for every committed case that clears its lines on it."""
    V = wr.V_BIG
    l = wr.logits_row(40, V)
    top3 = [int(i) for i in np.argsort(-l)[:3]]
    rules = [(2, (i,), 0.0) for i in top3]
    processed = wr.process_row_ext(l, [1, 5], 1, rules=rules)
    cases = [c for c in wr.CASES if wr.clears(wr.kept_set_ext(processed, *c)[2]) and wr.sample_row_ext(processed, c, 5, 0, 1)[2] > wr.MARGIN]
    assert len(cases) >= 8
    B = len(cases)
    x = torch.from_numpy(np.tile(l, (B, 1))).to(device)
    tok, _, sc = _op_ext(x, cases, [5] * B, [0] * B, [1] * B, hists=[[1, 5]] * B, rules=rules)
    for b, case in enumerate(cases):
        rt, _, _, keep, rsc = wr.sample_row_ext(processed, case, 5, 0, 1)
        assert not keep[top3].any() and ((sc[b] > -np.inf) == keep).all() and (_bits(sc[b]) == _bits(rsc)).all() and int(tok[b]) == rt, case


# ---- op level: the token rules ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [wr.V_BIG, wr.V_SMALL])
def test_token_rules_on_crafted_histories(device, V):
    """Greedy rows with penalty 1.3, n-gram 3, min_new 2 and the rule table of tests/test_warpers.py (1- to 4-id rules that fire or miss by one
    position, a rule longer than the history, four rules on one id, begin-only rules) on ragged histories: the scores are the replay's
    processed row bit for bit -- HF's, by the CPU test -- and the token its argmax."""
    l = wr.logits_row(21, V)
    combos = [(h, n) for h in HISTS for n in (0, 1, 3) if n <= len(h)]
    for b0 in range(0, len(combos), 8):
        part = combos[b0:b0 + 8]
        B = len(part)
        x = torch.from_numpy(np.tile(l, (B, 1))).to(device)
        tok, _, sc = _op_ext(x, [(0.0, 0, 1.0, 0, 0, 0, 0)] * B, [0] * B, [0] * B, [n for _, n in part], hists=[h for h, _ in part],
                             proc=[(1.3, 3, 2)] * B, rules=RULES.rules)
        for b, (h, n) in enumerate(part):
            want = wr.process_row_ext(l, h, n, 1.3, 3, 2, 2, RULES.rules)
            assert (_bits(sc[b]) == _bits(want)).all(), (V, h, n, np.flatnonzero(_bits(sc[b]) != _bits(want)))
            assert (_bits(want) == _bits(hf_processed(l, h, n, RULES))).all()
            assert int(tok[b]) == int(np.argmax(want))
    # enable words per row; ids past V are ignored; a row banned to nothing emits pad
    from emmax.sampling import LogitsProcessing

    far = LogitsProcessing(sequence_bias={(V + 5,): 1.0, (V - 1,): 0.5}, suppress_tokens=[V, 3])
    x = torch.from_numpy(np.tile(l, (4, 1))).to(device)
    tok, _, sc = _op_ext(x, [(0.0, 0, 1.0, 0, 0, 0, 0)] * 4, [0] * 4, [0] * 4, [0] * 4, hists=[[1]] * 4, rules=far.rules, enable=[15, 0, 1, 4])
    for b, en in enumerate([15, 0, 1, 4]):
        assert (_bits(sc[b]) == _bits(wr.process_row_ext(l, [1], 0, rules=far.rules, enable=en))).all(), en
    assert (_bits(sc[1]) == _bits(l)).all() and np.isinf(sc[0][3]) and sc[2][3] == l[3] and sc[2][V - 1] == np.float32(l[V - 1] + np.float32(0.5))
    if V == wr.V_SMALL:
        ban_all = [(2, (i,), 0.0) for i in range(V)]
        tok, lp, sc = _op_ext(x[:2], [(0.0, 0, 1.0, 0, 0, 0, 0), (1.0, 50, 0.9, 0.1, 0.9, 0, 0)], [0, 1], [0, 0], [0, 0], hists=[[1], [1]], rules=ban_all, pad=31)
        assert tok.tolist() == [31, 31] and np.isinf(sc).all()


def test_rules_penalty_and_warpers_in_hf_order(device):
    """A sampled row through everything at once: bias, repetition penalty on a biased id, -inf rules, then top-k / top-p and the four
    warpers -- the scores equal HF's chain on the processed row."""
    V = wr.V_BIG
    l = wr.logits_row(41, V)
    hist = [1, 2, 9, 4, 6, 13]
    want = wr.process_row_ext(l, hist, 2, 1.3, 3, 2, 2, RULES.rules)
    assert (_bits(want) == _bits(hf_processed(l, hist, 2, RULES))).all()
    cases = [c for c in wr.CASES[8:] + ((1.0, 0, 1.0, 0.05, 0.9, 0, 0),) if wr.clears(wr.kept_set_ext(want, *c)[2])]
    assert len(cases) >= 2
    B = len(cases)
    x = torch.from_numpy(np.tile(l, (B, 1))).to(device)
    tok, _, sc = _op_ext(x, cases, [3] * B, [0] * B, [2] * B, hists=[hist] * B, proc=[(1.3, 3, 2)] * B, rules=RULES.rules)
    for b, case in enumerate(cases):
        keep, z, _ = wr.kept_set_ext(want, *case)
        assert ((sc[b] > -np.inf) == keep).all() and (sc[b][keep] == z[keep]).all() and keep[int(tok[b])]
        assert ((hf_warped(want, case) > -np.inf) == keep).all()


# ---- session level --------------------------------------------------------------------------------------------------------------------------
def _model(device, max_batch, exact=False):
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    cfg.llm.num_layers = 2
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=6).items()}
    return EmmaXForActionPrediction(cfg, dict(sd)).to(device, max_batch=max_batch, max_prompt=24, exact=exact), cfg


def _inputs(B, seed=21, lo=6, hi=20):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(B, 224, 224, 3), dtype=np.uint8)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=int(n))] for n in rng.integers(lo, hi, size=B)]
    return frames, rows


def _rule_kwargs(rows):
    """Rules that fire on these prompts: the last prompt id of row 0 starts a 2-id bad word and a 2-id bias."""
    a = rows[0][-1]
    return {"suppress_tokens": [5, 6, 7], "bad_words_ids": [[a, 11], [12]], "sequence_bias": {(a, 13): 4.0, (14,): -2.0}, "begin_suppress_tokens": [15]}


GEN = {"do_sample": True, "temperature": 0.9, "top_k": 50, "top_p": 0.95, "seed": 123, "min_p": 0.02, "typical_p": 0.95, "repetition_penalty": 1.2}


CASE = (0.9, 50, 0.95, 0.02, 0.95, 0.0, 0.0)   # GEN's (T, top_k, top_p, min_p, typical_p, epsilon, eta)
INPUT_SEEDS = {1: 51, 3: 53}                   # prompts and frames on which every step of the call below clears its lines (asserted)
N_STEPS = 5


def _generate(model, cfg, rows, fr, graph, **kw):
    from emmax import _lib

    pad = torch.nn.utils.rnn.pad_sequence
    with _lib.tuning(graph=graph):
        out = model.generate(pad([torch.tensor(r) for r in rows], batch_first=True, padding_value=cfg.pad_token_id),
                             attention_mask=pad([torch.ones(len(r), dtype=torch.long) for r in rows], batch_first=True),
                             frames_u8=fr, max_new_tokens=N_STEPS, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
        assert model.engine.graph_active() == bool(graph) and model.engine.warpers and model.engine.token_rules
    return out.sequences.cpu().numpy(), torch.stack(out.scores).cpu().numpy(), torch.stack(out.logits).cpu().numpy()


def _replay_steps(cfg, rows, seq, sc, lg, proc):
    """Per (row, step) of a generate() call: (b, t, clears, scores equal, token equal), the replay applied to the step's returned raw
    logit row and the row's history."""
    out = []
    for b in range(len(rows)):
        hist = list(rows[b])
        for t in range(sc.shape[0]):
            if np.isnan(lg[t, b]).all():
                break
            want = wr.process_row_ext(lg[t, b], hist, t, proc.repetition_penalty, proc.no_repeat_ngram_size, proc.min_new_tokens, cfg.eos_token_id, proc.rules)
            tok_r, _, margin, keep, rsc = wr.sample_row_ext(want, CASE, GEN["seed"], b, t)
            tok = int(seq[b, len(rows[b]) + t])
            out.append((b, t, wr.clears(wr.kept_set_ext(want, *CASE)[2]) and margin > wr.MARGIN, bool((_bits(sc[t, b]) == _bits(rsc)).all()), tok == tok_r))
            hist.append(tok)
    return out


def _same(a, b):
    return a.shape == b.shape and bool((_bits(np.nan_to_num(a, neginf=-1.0)) == _bits(np.nan_to_num(b, neginf=-1.0))).all())


@pytest.mark.parametrize("B", [1, 3])
def test_generate_with_the_new_arguments(device, B):
    """generate(do_sample=True, min_p, typical_p, suppress_tokens, bad_words_ids, sequence_bias, begin_suppress_tokens, output_scores,
    output_logits): every step's scores are the replay applied to that step's returned raw logit row and the row's history, the token is the
    replay's draw; eager launches equal hipGraph replay bit for bit, and a replay with other parameters follows them (nothing is re-captured:
    the parameters are device words)."""
    from emmax.modeling import EmmaXForActionPrediction as M

    model, cfg = _model(device, 4)
    frames, rows = _inputs(B, seed=INPUT_SEEDS[B])
    fr = torch.from_numpy(frames).to(device)
    kw = dict(GEN, **_rule_kwargs(rows))
    proc = M._processing_args(rows, repetition_penalty=GEN["repetition_penalty"], eos_token_id=cfg.eos_token_id, **_rule_kwargs(rows))
    seq, sc, lg = _generate(model, cfg, rows, fr, 0, **kw)
    steps = _replay_steps(cfg, rows, seq, sc, lg, proc)
    print(steps)
    assert len(steps) >= 2 * B and all(s[2] for s in steps), [s for s in steps if not s[2]]   # no step is skipped: every one clears
    assert all(s[3] and s[4] for s in steps), [s for s in steps if not (s[3] and s[4])]
    assert np.isinf(sc[:, :, [5, 6, 7, 12]][~np.isnan(sc[:, :, 0])]).all() and np.isinf(sc[0, :, 15]).all()
    g1, g2 = _generate(model, cfg, rows, fr, 1, **kw), _generate(model, cfg, rows, fr, 1, **kw)
    for u, v, w in zip((seq, sc, lg), g1, g2):
        assert _same(u, v) and _same(v, w)
    # other parameters and another table on the captured graph: the replay equals the eager run with them
    over = dict(kw, min_p=0.3, typical_p=0.5, suppress_tokens=[8, 9], seed=124)
    e, g = _generate(model, cfg, rows, fr, 0, **over), _generate(model, cfg, rows, fr, 1, **over)
    assert all(_same(u, v) for u, v in zip(e, g)) and not _same(e[1], sc)


def test_calls_without_the_new_arguments_are_untouched(device):
    """The same sampled + processed call on a session that used the new arguments before, and on one that never had them set: bit-equal
    ids, scores and log-probabilities, and the session is back on the existing finish."""
    from emmax.sampling import LogitsProcessing, SamplingParams

    frames, rows = _inputs(2, seed=61)

    def run(model, first):
        fr = torch.from_numpy(frames).to(device)
        if first:
            model.generate_ids(rows, frames_u8=fr, max_new_tokens=4, stop_on_eos=False, sampling=SamplingParams(1.0, 50, 1.0, 3, min_p=0.1, eta_cutoff=1e-3),
                               processing=LogitsProcessing(1.1, suppress_tokens=[5]))
            assert model.engine.warpers and model.engine.token_rules
        V = model.config.llm.vocab_size
        sc = torch.full((8, 2, V), float("nan"), dtype=torch.float32, device=device)
        ids, lens, lp = model.generate_ids(rows, frames_u8=fr, max_new_tokens=8, stop_on_eos=False, sampling=SamplingParams(0.9, 40, 0.9, 5),
                                           processing=LogitsProcessing(1.3, 2, 1), scores=sc, return_logprobs=True)
        assert not model.engine.warpers and not model.engine.token_rules and model.engine.processing
        return ids.cpu(), lp.cpu().view(torch.int32), torch.nan_to_num(sc).cpu().view(torch.int32)

    a = run(_model(device, 2)[0], True)
    b = run(_model(device, 2)[0], False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_a_sample_group_shares_rules_and_warpers(device):
    """num_return_sequences = 4: the four samples of a prompt share the rule table and the warper values.  The three ids with the largest
    raw logits of the first step (always kept) are suppressed: they are -inf in every sample's scores at every step; min_p = 0.3 keeps
    fewer entries than the plain call in every sample; the four samples' first-step kept sets (one logit row, one parameter set) are the replay's."""
    model, cfg = _model(device, 4)
    frames, rows = _inputs(1, seed=70)
    fr = torch.from_numpy(frames).to(device)
    ids = torch.tensor(rows)
    base = {"do_sample": True, "temperature": 0.9, "top_k": 50, "seed": 9, "max_new_tokens": 5, "num_return_sequences": 4, "return_dict_in_generate": True,
            "output_scores": True, "output_logits": True}
    plain = model.generate(ids, frames_u8=fr, **base)
    assert not model.engine.warpers and not model.engine.token_rules
    psc, plg = torch.stack(plain.scores).cpu().numpy(), torch.stack(plain.logits).cpu().numpy()
    top3 = [int(i) for i in np.argsort(-plg[0, 0])[:3]]
    assert np.isfinite(psc[0][:, top3]).all()
    # min_p between the 25th and the 26th largest entry of the suppressed row (the tiny model's rows are flat: a fixed value would keep all 50)
    banned = wr.process_row_ext(plg[0, 0], rows[0], 0, rules=[(2, (i,), 0.0) for i in top3])
    z = np.sort((banned / np.float32(0.9)).astype(np.float32).astype(np.float64))[::-1]
    min_p = float(np.exp((z[24] + z[25]) / 2 - z[0]))
    keep, _, info = wr.kept_set_ext(banned, 0.9, 50, 1.0, min_p)
    assert wr.clears(info) and keep.sum() == 25, (min_p, int(keep.sum()), info["min_p"]["slack"])
    out = model.generate(ids, frames_u8=fr, min_p=min_p, suppress_tokens=top3, sequence_bias={(top3[0],): 5.0}, **base)
    assert model.engine.warpers and model.engine.token_rules
    seq, sc = out.sequences.cpu().numpy(), torch.stack(out.scores).cpu().numpy()
    assert seq.shape[0] == 4 and sc.shape[1] == 4
    live = ~np.isnan(sc[:, :, 0])
    assert live[0].all() and np.isinf(sc[:, :, top3][live]).all()
    assert all(((sc[0, j] > -np.inf) == keep).all() for j in range(4))   # one logit row, one parameter set: one kept set
    assert ((psc[0] > -np.inf).sum(-1) == 50).all() and ((sc[live] > -np.inf).sum(-1) < 50).all()


def test_slot_serving_with_per_request_warpers_and_rule_enables(device):
    """exact numerics, 4 slots, 6 requests with their own min_p and rule enables, overlapped admissions: each request returns its own
    bs = 1 generate_ids, and the session is plain again after the serve"""
    from emmax.sampling import LogitsProcessing, SamplingParams
    from emmax.serving import Request, SlotScheduler

    model, _ = _model(device, 4, exact=True)
    eng = model.engine
    frames, rows = _inputs(6, seed=45)
    fr = torch.from_numpy(frames).to(device)
    plain, _ = model.generate_ids([rows[0]], frames_u8=fr[:1], max_new_tokens=7, stop_on_eos=True, sampling=[SamplingParams(1.0, 50, 1.0, 300, min_p=0.02)])
    first = int(plain[0, 0])   # what request 0 emits first without rules: banned below, so its rules are seen to bite
    ban, bias = {"suppress_tokens": [first] + list(range(3, 40))}, {"sequence_bias": {(41,): 6.0, (41, 42): 6.0}}
    proc = [LogitsProcessing(**ban), None, LogitsProcessing(1.2, **bias), LogitsProcessing(**ban, **bias), LogitsProcessing(1.3, 2, 2), LogitsProcessing(**ban)]
    samp = [SamplingParams(1.0, 50, 1.0, 300 + i, min_p=[0.02, 0.0, 0.1, 0.3, 0.0, 0.05][i], epsilon_cutoff=[0, 0, 3e-4, 0, 0, 0][i]) if i != 3 else None
            for i in range(6)]
    budgets = [7, 9, 6, 10, 8, 5]
    want = []
    for i in range(6):
        ids, lens = model.generate_ids([rows[i]], frames_u8=fr[i:i + 1], max_new_tokens=budgets[i], stop_on_eos=True,
                                       sampling=None if samp[i] is None else [samp[i]], processing=None if proc[i] is None else [proc[i]])
        want.append(ids[0, : int(lens[0])].cpu().tolist())
    assert want[0][0] != first and first not in want[0]

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    sch = SlotScheduler(eng, encode, n_slots=4, poll_every=2, overlap=True)
    for i in range(6):
        sch.submit(Request(i, fr[i], rows[i], max_new_tokens=budgets[i], sampling=samp[i], processing=proc[i]))
    res = sch.run()
    assert sorted(r.rid for r in res) == list(range(6)) and sch.overlapped_admissions >= 1
    assert not eng.sampling and not eng.processing and not eng.warpers and not eng.token_rules
    for r in res:
        assert r.ids == want[r.rid], (r.rid, r.ids, want[r.rid])
