"""Constrained decoding on a real MI355X (include/emmax.h: emmax_op_sample_constrained, emmax_session_set_automaton; the CON finish of
emma-x_amd/csrc/sample_kernel.h).  Op level: the committed rows of tests/constraint_ref.py -- every one of which clears its lines under the mask
(tests/test_constraint.py) -- against the numpy replay, and crafted edges.  Session level on the tiny config with 2 layers: generate() with
constraint= against the replay applied to each step's returned raw logit row plus TokenAutomaton.walk, graph replay against eager, another
table on the captured graph, predict_action(constrain_to_bins=True), a policy line on a planted chain, slot serving, the refusals, clearing."""
import numpy as np
import pytest
import torch

import constraint_ref as cr
import warpers_ref as wr
from emmax import constraints as ct
from test_sampling_gpu import _op_sample
from test_warpers_gpu import _bits, _dev, _inputs, _model, _op_ext

pytestmark = pytest.mark.gpu


def _op_con(logits, cases, seed, subseq, n_out, aut, states, hists=None, proc=None, rules=None, enable=None, eos=2, pad=32000, tables=None):
    """emmax_op_sample_constrained on logits [B, V] (device): the arguments of test_warpers_gpu._op_ext, the automaton (or tables = (S, C,
    cls, allow, next) as arrays) and the rows' states.  Returns (tokens, log-probabilities, next states, scores [B, V])."""
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
    hists = hists if hists is not None else [[1]] * B
    max_hist = max(1, max(len(h) for h in hists))
    H = np.zeros((B, max_hist), dtype=np.int32)
    for b, h in enumerate(hists):
        H[b, : len(h)] = h
    pr = np.asarray(proc if proc is not None else [(1.0, 0, 0)] * B, dtype=np.float64).reshape(B, 3)
    pa = [_dev(pr[:, 0], np.float32, dev), _dev(pr[:, 1], np.int32, dev), _dev(pr[:, 2], np.int32, dev), _dev(H, np.int32, dev),
          _dev([len(h) for h in hists], np.int32, dev)]
    rt, ra, R = [], [None] * 5, 0
    if rules:
        off, ids = [0], []
        for _, r, _ in rules:
            ids += list(r)
            off.append(len(ids))
        R = len(rules)
        rt = [_dev(off, np.int32, dev), _dev(ids, np.int32, dev), _dev([k | (4 if k == 3 else 0) for k, _, _ in rules], np.int32, dev),
              _dev([b for _, _, b in rules], np.float32, dev), _dev(np.asarray(enable if enable is not None else [15] * B, dtype=np.uint32).view(np.int32), np.int32, dev)]
        ra = [x.data_ptr() for x in rt]
    S, C, cls, allow, nxt = tables if tables is not None else (aut.n_states, aut.n_classes, *aut.tables())
    assert cls.shape == (V,) and allow.shape == (S, 8) and nxt.shape == (S, C)
    at = [_dev(cls, np.uint8, dev), _dev(np.asarray(allow, dtype=np.uint32).view(np.int32), np.int32, dev), _dev(nxt, np.int16, dev), _dev(states, np.int32, dev)]
    tok = torch.full((B,), -7, dtype=torch.int32, device=dev)
    lp = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    ns = torch.full((B,), -7, dtype=torch.int32, device=dev)
    sc = torch.full((B, V), float("nan"), dtype=torch.float32, device=dev)
    ld = logits.stride(0) if B > 1 else V
    _lib.check(lib.emmax_op_sample_constrained(logits.data_ptr(), ld, B, V, t.data_ptr(), kk.data_ptr(), pp.data_ptr(), sd.data_ptr(), sq.data_ptr(), no.data_ptr(),
                                               *[w.data_ptr() for w in warp], *[x.data_ptr() for x in pa], max_hist, R, *ra, eos, pad, S, C,
                                               *[x.data_ptr() for x in at], tok.data_ptr(), lp.data_ptr(), ns.data_ptr(), sc.data_ptr(),
                                               _lib.current_stream()), "emmax_op_sample_constrained")
    torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy(), ns.cpu().numpy(), sc.cpu().numpy()


# ---- op level: the committed rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", cr.SIZES)
def test_constrained_rows_match_the_replay(device, V):
    """A batch of 8 rows, each in another state of one automaton, greedy and sampled (top-k, top-p, two warper sets): the kept set (through
    the scores) equals the replay's, the scores are equal bit for bit, the token is the replay's draw, the next state the replay's, the
    log-probability emmax_op_sample's bits on the raw row wherever that draws the same token; a second launch is bit-equal; a row moved to
    another place of a smaller batch gives the same bits."""
    aut = cr.make_automaton(V)
    rows = cr.committed_rows(V)
    x = torch.from_numpy(np.stack([r[1] for r in rows])).to(device)
    cases, states = [r[3] for r in rows], [r[2] for r in rows]
    seeds, subs, steps = zip(*[cr.row_params(b) for b in range(8)])
    tok, lp, ns, sc = _op_con(x, cases, seeds, subs, steps, aut, states)
    tok2, lp2, ns2, sc2 = _op_con(x, cases, seeds, subs, steps, aut, states)
    assert (tok == tok2).all() and (_bits(lp) == _bits(lp2)).all() and (ns == ns2).all() and (_bits(sc) == _bits(sc2)).all()
    tok0, lp0 = _op_sample(x, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], seeds, subs, steps)
    same = tok0 == tok   # (the same noise: a row whose unconstrained draw the mask allows draws it again, with emmax_op_sample's bits)
    print(V, "rows whose unconstrained token survives the mask:", int(same.sum()))
    assert same.any() and (_bits(lp)[same] == _bits(lp0)[same]).all()   # (row 0 is greedy and its maximum is allowed in state 0 at every size: tests/test_constraint.py)
    for b, l, state, case in rows:
        rt, rlp, rns, margin, rsc, dead = cr.sample_constrained(l, aut, state, case, seeds[b], subs[b], steps[b])
        assert not dead and margin > wr.MARGIN
        assert ((sc[b] > -np.inf) == (rsc > -np.inf)).all(), (V, b, int((rsc > -np.inf).sum()), int((sc[b] > -np.inf).sum()))
        assert not (sc[b] > -np.inf)[~aut.allowed(state)].any()
        assert (_bits(sc[b]) == _bits(rsc)).all()
        assert int(tok[b]) == rt and abs(float(lp[b]) - rlp) <= 1e-5 and int(ns[b]) == rns, (V, b, int(tok[b]), rt, int(ns[b]), rns)
    pick = [5, 0, 6]   # other places, another B
    tok3, lp3, ns3, sc3 = _op_con(x[pick].contiguous(), [cases[i] for i in pick], [seeds[i] for i in pick], [subs[i] for i in pick], [steps[i] for i in pick], aut,
                                  [states[i] for i in pick])
    assert (tok3 == tok[pick]).all() and (_bits(lp3) == _bits(lp[pick])).all() and (ns3 == ns[pick]).all() and (_bits(sc3) == _bits(sc[pick])).all()


def _tables(V, S, C, cls, allowed_classes, nxt=None):
    """(S, C, cls, allow, next): allowed_classes = {state: [classes]}; next defaults to 0 everywhere"""
    allow = np.zeros((S, 8), dtype=np.uint32)
    for s, cs in allowed_classes.items():
        for c in cs:
            allow[s, c >> 5] |= np.uint32(1 << (c & 31))
    return S, C, np.asarray(cls, dtype=np.uint8), allow, np.zeros((S, C), dtype=np.int16) if nxt is None else np.asarray(nxt, dtype=np.int16)


SAMPLED = (1.0, 50, 0.95, 0.0, 0.0, 0.0, 0.0)
GREEDY = (0.0, 0, 1.0, 0.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("V", cr.SIZES)
def test_constrained_crafted_edges(device, V):
    l = np.stack([wr.logits_row(50 + b, V) for b in range(4)])
    x = torch.from_numpy(l).to(device)
    cases, seeds, subs, steps = [GREEDY, SAMPLED, SAMPLED, GREEDY], [1, 2, 3, 4], [0, 1, 2, 0], [0, 1, 2, 3]
    # S = 1, C = 1, all allowed: the unconstrained op bit for bit
    tok, lp, ns, sc = _op_con(x, cases, seeds, subs, steps, None, [0] * 4, tables=_tables(V, 1, 1, np.zeros(V), {0: [0]}))
    tok0, lp0, sc0 = _op_ext(x, cases, seeds, subs, steps, hists=[[1]] * 4)
    assert (tok == tok0).all() and (_bits(lp) == _bits(lp0)).all() and (_bits(sc) == _bits(sc0)).all() and (ns == 0).all()
    # C = 256, the only allowed class is 255: word 7, bit 31
    cls = np.arange(V) % 256 if V >= 256 else np.where(np.arange(V) % 5 == 4, 255, np.arange(V) % 5)   # (37 ids cannot fill 256 classes)
    tok, _, ns, sc = _op_con(x, cases, seeds, subs, steps, None, [0] * 4, tables=_tables(V, 1, 256, cls, {0: [255]}))
    assert (cls[tok] == 255).all() and not (sc > -np.inf)[:, cls != 255].any() and (sc > -np.inf).any(1).all()
    for b in (0, 3):   # (the greedy rows: the scores are the whole masked row; the sampled rows keep a part of the class, the replay's)
        assert ((sc[b] > -np.inf) == (cls == 255)).all() and (_bits(sc[b][cls == 255]) == _bits(l[b][cls == 255])).all()
    for b in (1, 2):
        keep = wr.sample_row_ext(np.where(cls == 255, l[b], np.float32(-np.inf)).astype(np.float32), cases[b], seeds[b], subs[b], steps[b])[3]
        assert ((sc[b] > -np.inf) == keep).all()
    # S = 1024 with the row in state 1023, which allows class 1 = {id 5}; its next state is 1022
    cls = np.zeros(V, dtype=np.uint8)
    cls[5] = 1
    nxt = np.zeros((1024, 2), dtype=np.int16)
    nxt[1023, 1] = 1022
    tok, lp, ns, sc = _op_con(x, cases, seeds, subs, steps, None, [1023] * 4, tables=_tables(V, 1024, 2, cls, {1023: [1], 0: [0]}, nxt))
    assert (tok == 5).all() and (ns == 1022).all() and ((sc > -np.inf).sum(1) == 1).all()
    for b in range(4):
        assert abs(float(lp[b]) - cr.raw_logprob(l[b], 5)) <= 1e-5   # the log-probability of the RAW row, not of the masked one (that would be 0)
    # a state allowing exactly one id, at V - 1, and another at 0; a state allowing nothing gives pad_id and keeps its state; next = -1 is
    # reported; a row at -1 sits beside them
    cls = np.zeros(V, dtype=np.uint8)
    cls[V - 1], cls[0] = 1, 2
    nxt = np.array([[0, -1, 0], [0, 0, 3], [0, 0, 0], [0, 0, 0]], dtype=np.int16)
    tok, lp, ns, sc = _op_con(x, cases, seeds, subs, steps, None, [0, 1, 2, -1], tables=_tables(V, 4, 3, cls, {0: [1], 1: [2], 3: [0, 1, 2]}, nxt), pad=V - 3)
    assert tok.tolist()[:3] == [V - 1, 0, V - 3] and ns.tolist() == [-1, 3, 2, -1]
    assert np.flatnonzero(sc[0] > -np.inf).tolist() == [V - 1] and np.flatnonzero(sc[1] > -np.inf).tolist() == [0] and np.isinf(sc[2]).all()
    tok0, lp0, sc0 = _op_ext(x[3:], [GREEDY], [4], [0], [3], hists=[[1]])
    assert int(tok[3]) == int(tok0[0]) and (_bits(lp[3:]) == _bits(lp0)).all() and (_bits(sc[3]) == _bits(sc0[0])).all()
    # a state the table does not have (the op's n_states is 4) allows nothing
    tok, _, ns, sc = _op_con(x[:1], [GREEDY], [1], [0], [0], None, [4], tables=_tables(V, 4, 3, cls, {0: [1]}, nxt), pad=V - 3)
    assert int(tok[0]) == V - 3 and int(ns[0]) == 4 and np.isinf(sc).all()


@pytest.mark.parametrize("V", cr.SIZES)
def test_constraint_with_the_other_processors(device, V):
    """The mask beside a repetition penalty, an n-gram ban, a sequence bias on a forbidden id (it stays forbidden) and min_new on an allowed
    EOS: the scores are the replay's processed and masked row bit for bit, greedy and sampled."""
    aut = cr.make_automaton(V)
    l = wr.logits_row(77, V)
    state = 1                                   # keeps (i + 1) % 5 != 0: EOS (2) is allowed, 4 and 9 are not
    hist = [1, 6, 7, 11, 6, 7]                  # n-gram 3: (6, 7) -> 11 is banned; penalty on 1, 6, 7, 11
    l[[2, 4, 11, 6]] = l.max() + np.float32([4.0, 3.0, 2.0, 1.0])
    rules = [(0, (4,), 9.0), (0, (7, 8), 2.0)]   # a bias on the forbidden 4 (the largest entry by far afterwards), one on the allowed 8
    kw = dict(hist=hist, penalty=1.3, ngram=3, min_new=2, eos_id=2, rules=rules)
    want = cr.constrained_row(l, aut, state, n_out=1, **kw)
    assert np.isinf(want[[2, 4, 9, 11]]).all() and want[8] == np.float32(l[8] + np.float32(2.0)) and aut.allowed(state)[[2, 8, 6, 11]].all()
    assert cr.clears(l, aut, state, SAMPLED, 5, 0, 1, **{k: v for k, v in kw.items()})
    x = torch.from_numpy(np.tile(l, (2, 1))).to(device)
    tok, lp, ns, sc = _op_con(x, [GREEDY, SAMPLED], [5, 5], [0, 0], [1, 1], aut, [state] * 2, hists=[hist] * 2, proc=[(1.3, 3, 2)] * 2, rules=rules)
    assert (_bits(sc[0]) == _bits(want)).all() and int(tok[0]) == int(np.argmax(want))
    rt, rlp, rns, _, rsc, _ = cr.sample_constrained(l, aut, state, SAMPLED, 5, 0, 1, **kw)
    assert (_bits(sc[1]) == _bits(rsc)).all() and int(tok[1]) == rt and int(ns[1]) == rns and abs(float(lp[1]) - rlp) <= 1e-5
    # min_new spent: the allowed EOS is back
    tok, _, _, sc = _op_con(x[:1], [GREEDY], [5], [0], [2], aut, [state], hists=[hist + [6]], proc=[(1.0, 0, 2)])
    assert int(tok[0]) == 2 and np.isfinite(sc[0, 2])


# ---- session level ------------------------------------------------------------------------------------------------------------------------
HF = {"do_sample": True, "seed": 321}        # HF's defaults: temperature 1, top_k 50, top_p 1
HF_CASE = (1.0, 50, 1.0, 0.0, 0.0, 0.0, 0.0)
N_STEPS = 5


def _generate(model, cfg, rows, fr, graph, n=N_STEPS, **kw):
    from emmax import _lib

    pad = torch.nn.utils.rnn.pad_sequence
    with _lib.tuning(graph=graph):
        out = model.generate(pad([torch.tensor(r) for r in rows], batch_first=True, padding_value=cfg.pad_token_id),
                             attention_mask=pad([torch.ones(len(r), dtype=torch.long) for r in rows], batch_first=True),
                             frames_u8=fr, max_new_tokens=n, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
        assert model.engine.graph_active() == bool(graph and n > 2) and model.engine.automaton
    B = len(rows)
    return out.sequences.cpu().numpy(), torch.stack(out.scores).cpu().numpy(), torch.stack(out.logits).cpu().numpy(), model.engine.automaton_state(0, B)


def _replay(cfg, aut, starts, rows, seq, sc, lg, case, seed):
    """Per row: the states the replay walks through, every step's (clears, scores equal, token equal)"""
    states, steps = [], []
    for b in range(len(rows)):
        s = aut.start_state(starts[b])
        for t in range(sc.shape[0]):
            if np.isnan(lg[t, b]).all():
                break
            tok = int(seq[b, len(rows[b]) + t])
            rt, _, ns, margin, rsc, dead = cr.sample_constrained(lg[t, b], aut, s, case, seed, b, t, hist=rows[b] + seq[b, len(rows[b]): len(rows[b]) + t].tolist(),
                                                                 eos_id=cfg.eos_token_id)
            ok = not dead and (not case[0] > 0 or (wr.clears(wr.kept_set_ext(cr.constrained_row(lg[t, b], aut, s), *case)[2]) and margin > wr.MARGIN))
            steps.append((b, t, ok, bool((_bits(sc[t, b]) == _bits(rsc)).all()), tok == rt))
            s = ns
        states.append(s)
    return states, steps


@pytest.mark.parametrize("B,sampled", [(1, False), (1, True), (3, True)])
def test_generate_with_a_constraint(device, B, sampled):
    """generate(constraint=, constraint_start=) greedy, and sampled at B = 1 and at a ragged B = 3 whose rows enter at different states (one
    not at all): the replay plus .walk reproduce every emitted id, every step's scores and -- generation by generation, 1 to 5 tokens long --
    the states read back through emmax_session_automaton_state; hipGraph replay equals eager id for id."""
    model, cfg = _model(device, 4)
    V = cfg.llm.vocab_size
    aut = cr.make_automaton(V)
    frames, rows = _inputs(B, seed=80 + B)
    fr = torch.from_numpy(frames).to(device)
    starts = [3, None, 6][:B] if B > 1 else [0]
    kw = dict(HF if sampled else {}, constraint=aut, constraint_start=starts)
    case = HF_CASE if sampled else GREEDY
    for n in range(1, N_STEPS + 1):
        seq, sc, lg, got_states = _generate(model, cfg, rows, fr, 0, n=n, **kw)
        states, steps = _replay(cfg, aut, starts, rows, seq, sc, lg, case, HF.get("seed"))
        assert len(steps) == n * B and all(s[2] for s in steps), [s for s in steps if not s[2]]   # no step is skipped: every one clears
        assert all(s[3] and s[4] for s in steps), [s for s in steps if not (s[3] and s[4])]
        assert got_states == states, (n, got_states, states)
        for b in range(B):   # .walk agrees with the step-by-step replay, and raises on nothing
            new = seq[b, len(rows[b]): len(rows[b]) + n].tolist()
            assert (aut.walk(new, starts[b]) or [None])[-1] == states[b]
            if starts[b] is None:
                assert states[b] == -1
    g = _generate(model, cfg, rows, fr, 1, **kw)
    assert (g[0] == seq).all() and (_bits(np.nan_to_num(g[1], neginf=-1)) == _bits(np.nan_to_num(sc, neginf=-1))).all() and g[3] == got_states


def test_another_table_on_the_captured_graph(device):
    """Two generations under graph mode with two tables: the second needs no other graph (the tables are device words behind stable
    pointers) and follows its table -- it equals the eager run with that table, and differs from the first."""
    model, cfg = _model(device, 4)
    V = cfg.llm.vocab_size
    frames, rows = _inputs(2, seed=90)
    fr = torch.from_numpy(frames).to(device)
    a1 = cr.make_automaton(V)
    a2 = ct.build(V, [ct.AnyOf(list(range(1000, 1400)), 3), ct.AnyOf(list(range(500, 600)), 2)], end="done")
    g1 = _generate(model, cfg, rows, fr, 1, constraint=a1, **HF)
    g2 = _generate(model, cfg, rows, fr, 1, constraint=a2, **HF)
    for b, r in enumerate(rows):
        ids = g2[0][b, len(r): len(r) + N_STEPS].tolist()
        assert all(1000 <= t < 1400 for t in ids[:3]) and all(500 <= t < 600 for t in ids[3:5]), ids
        assert a2.walk(ids) == [1, 2, 3, 4, -1]
        assert g1[0][b, len(r): len(r) + N_STEPS].tolist() != ids
    assert g2[3] == [-1, -1]
    e2 = _generate(model, cfg, rows, fr, 0, constraint=a2, **HF)
    assert (e2[0] == g2[0]).all() and (_bits(np.nan_to_num(e2[1], neginf=-1)) == _bits(np.nan_to_num(g2[1], neginf=-1))).all()


def test_another_table_under_rows_that_keep_their_starts(device):
    """emmax_session_set_automaton while one is on: the rows' starts stay.  Row 0 starts at a state the second table does not have -- it
    allows nothing, the row emits pad_id and is done with its state kept; row 1 stays unconstrained; row 2's start exists in both tables and
    is followed in the second.  A start the second table lacks is refused from then on."""
    from emmax import _lib

    model, cfg = _model(device, 4)
    eng = model.engine
    V = cfg.llm.vocab_size
    a1 = cr.make_automaton(V)                                                                                     # 8 states
    a2 = ct.build(V, [ct.AnyOf(list(range(1000, 1400)), 3), ct.AnyOf(list(range(500, 600)), 2)], end="done")   # 5 states
    frames, rows = _inputs(3, seed=91)
    patches = eng.vision_encode(torch.from_numpy(frames).to(device))
    eng.set_automaton(a1)
    eng.set_automaton_starts([7, -1, 3])
    eng.set_automaton(a2)
    assert eng.automaton and eng.processing
    with pytest.raises(_lib.EmmaxError, match="outside -1..4"):
        eng.set_automaton_starts([7])
    eng.prefill(rows, patches)
    ids, lens = eng.generate(4, stop_on_eos=True)
    ids, lens = ids.cpu().tolist(), lens.cpu().tolist()
    states = eng.automaton_state(0, 3)
    assert ids[0][0] == cfg.pad_token_id and lens[0] == 1 and states[0] == 7
    assert lens[1] == 4 and states[1] == -1
    assert lens[2] == 2 and all(500 <= t < 600 for t in ids[2][:2]) and a2.walk(ids[2][:2], 3) == [4, -1] and states[2] == -1
    eng.clear_automaton()


def _planted(device, override, max_batch=4, exact=False):
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    cfg = EmmaXConfig.tiny()
    cfg.llm.num_layers = 2
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=5, planted=True, succ_override=override).items()}
    return EmmaXForActionPrediction(cfg, dict(sd)).to(device, max_batch=max_batch, max_prompt=24, exact=exact), cfg


def test_predict_action_constrained_to_bins(device):
    """A model planted to prefer a non-bin id at position 3 of the action tokens: the unconstrained call emits it (and maps it to a wrong
    bin unnoticed); with constrain_to_bins every id is a bin id -- greedy, and with num_return_sequences = 4 and the bin log-probabilities."""
    from emmax.actions import action_bin_token_ids
    from emmax.config import EmmaXConfig
    from emmax.weights import PLANTED_PREFIX_TOKEN, planted_chain

    cfg0 = EmmaXConfig.tiny()
    chain = planted_chain(cfg0, PLANTED_PREFIX_TOKEN, 3)   # positions 0, 1, 2
    stray = 777
    model, cfg = _planted(device, {chain[2]: stray})
    bins = set(action_bin_token_ids(cfg.action_vocab_size, cfg.n_action_bins))
    frames, _ = _inputs(1, seed=95)
    fr = torch.from_numpy(frames).to(device)
    prompt = torch.tensor([[1, 50, 60, 70, PLANTED_PREFIX_TOKEN]])
    seen = []
    inner = model.generate_ids

    def spy(*a, **k):
        res = inner(*a, **k)
        seen.append(res[0].cpu().numpy())
        return res

    model.generate_ids = spy
    uploads = []
    upload = model.engine.lib.emmax_session_set_automaton
    model.engine.lib.emmax_session_set_automaton = lambda *a: (uploads.append(1), upload(*a))[1]
    dim = model.get_action_dim("bridge_orig")
    a_free = model.predict_action(prompt, "bridge_orig", frames_u8=fr)
    a_con = model.predict_action(prompt, "bridge_orig", frames_u8=fr, constrain_to_bins=True)
    again = model.predict_action(prompt, "bridge_orig", frames_u8=fr, constrain_to_bins=True)   # the cached automaton is on the device already
    assert len(uploads) == 1 and (again == a_con).all() and (seen.pop() == seen[1]).all() and model.engine.automaton
    assert seen[0][0, :3].tolist() == chain and int(seen[0][0, 3]) == stray                      # the constraint has something to do
    assert seen[1].shape == (1, dim) and all(int(t) in bins for t in seen[1][0]) and seen[1][0, :3].tolist() == chain
    assert a_free.shape == a_con.shape == (dim,) and model.engine.automaton_state(0, 1) == [-1]   # done after the dim-th bin
    kw = dict(do_sample=True, seed=11, num_return_sequences=4)
    model.predict_action(prompt, "bridge_orig", frames_u8=fr, **kw)
    acts, lp = model.predict_action(prompt, "bridge_orig", frames_u8=fr, constrain_to_bins=True, return_bin_logprobs=True, **kw)
    assert any(int(row[3]) not in bins for row in seen[2]), seen[2]                               # the same seed, unconstrained: a stray id
    assert seen[3].shape == (4, dim) and all(int(t) in bins for row in seen[3] for t in row)
    model.engine.lib.emmax_session_set_automaton = upload
    assert acts.shape == (4, dim) and lp.shape == (4, dim, cfg.n_action_bins) and np.isfinite(lp).all()


def test_policy_line_on_a_planted_chain(device):
    """The planted chain emits the trigger in the middle of ordinary text: the `dim` tokens behind it are bins, the tokens before it are the
    unconstrained chain's, and behind the bins the model is free again -- it follows the planted successors of what it emitted."""
    from emmax.actions import action_bin_token_ids
    from emmax.weights import planted_chain

    model, cfg = _planted(device, None)
    bins = set(action_bin_token_ids(cfg.action_vocab_size, cfg.n_action_bins))
    frames, _ = _inputs(1, seed=96)
    fr = torch.from_numpy(frames).to(device)
    start, dim, n = 4000, 3, 7
    free = planted_chain(cfg, start, n)
    assert not bins & set(free)
    pol = ct.policy_line(free[1:3], cfg.llm.vocab_size, cfg.n_action_bins, dim, token_vocab=cfg.action_vocab_size)
    row = [1, 9, 8, start]
    ids0, lens0 = model.generate_ids([row], frames_u8=fr, max_new_tokens=n, stop_on_eos=False)
    assert ids0[0].cpu().tolist() == free
    ids, lens = model.generate_ids([row], frames_u8=fr, max_new_tokens=n, stop_on_eos=False, constraint=pol)
    got = ids[0].cpu().tolist()
    assert got[:3] == free[:3] and all(t in bins for t in got[3:3 + dim]) and got[3] != free[3]
    assert got[4:n] == planted_chain(cfg, got[3], n - 4)   # from the first bin on the model follows its own successors: bins, allowed or free
    states = pol.walk(got)
    assert states[2] == pol.entry["segment1"] and states[-1] == states[3 + dim - 1] == model.engine.automaton_state(0, 1)[0]


@pytest.mark.parametrize("overlap", [False, True])
def test_slot_serving_with_per_request_starts(device, overlap):
    """Exact numerics, 4 slots, 10 requests: starts mixed, some unconstrained, greedy and sampled, one with num_samples = 3.  Each result
    equals the same request run alone through generate_ids (commit and fork both move start and state), and the session is plain again."""
    from emmax.sampling import SamplingParams
    from emmax.serving import Request, SlotScheduler

    model, cfg = _model(device, 4, exact=True)
    eng = model.engine
    V = cfg.llm.vocab_size
    aut = cr.make_automaton(V)
    frames, rows = _inputs(10, seed=47)
    fr = torch.from_numpy(frames).to(device)
    starts = [0, None, 3, 5, None, "start", 7, 2, None, 4]
    samp = [SamplingParams(1.0, 50, 1.0, 400 + i) if i % 3 != 1 else None for i in range(10)]
    nsamp = [1, 1, 3, 1, 1, 1, 1, 1, 1, 1]
    budgets = [5, 7, 6, 4, 8, 5, 6, 3, 5, 7]
    want = {}
    for i in range(10):
        kw = {} if starts[i] is None else {"constraint": aut, "constraint_start": starts[i]}
        if nsamp[i] > 1:
            kw["num_samples"] = nsamp[i]
        ids, lens = model.generate_ids([rows[i]], frames_u8=fr[i:i + 1], max_new_tokens=budgets[i], stop_on_eos=True,
                                       sampling=None if samp[i] is None else [samp[i]] * nsamp[i], **kw)[:2]
        for j in range(nsamp[i]):
            want[(i, j)] = ids[j, : int(lens[j])].cpu().tolist()
            if starts[i] is not None:
                aut.walk(want[(i, j)], starts[i])   # (raises on a token the automaton forbids)
    assert len({tuple(want[(2, j)]) for j in range(3)}) > 1   # the group's samples differ

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    sch = SlotScheduler(eng, encode, n_slots=4, poll_every=2, overlap=overlap, automaton=aut)
    for i in range(10):
        sch.submit(Request(i, fr[i], rows[i], max_new_tokens=budgets[i], sampling=samp[i], num_samples=nsamp[i], constraint_start=starts[i]))
    res = sch.run()
    assert sorted((r.rid, r.sample) for r in res) == sorted(want) and sch.overlap == overlap
    assert not overlap or sch.overlapped_admissions >= 1
    assert not eng.sampling and not eng.processing and not eng.automaton
    for r in res:
        assert r.ids == want[(r.rid, r.sample)], (r.rid, r.sample, r.ids, want[(r.rid, r.sample)])


def test_refusals(device):
    """Beams and the automaton refuse each other in both orders; starts before a table, out-of-range starts, a bad table and
    emmax_set_current_tokens while a table is set are refused, and a refused call changes nothing."""
    from emmax import _lib
    from emmax.sampling import BeamParams

    model, cfg = _model(device, 4)
    eng = model.engine
    V = cfg.llm.vocab_size
    aut = cr.make_automaton(V)
    with pytest.raises(_lib.EmmaxError, match="no token automaton is set"):
        eng.set_automaton_starts([0])
    with pytest.raises(_lib.EmmaxError, match="no token automaton is set"):
        eng.automaton_state(0, 1)
    eng.set_beams(BeamParams(2))
    with pytest.raises(_lib.EmmaxError, match="not available while beams are on"):
        eng.set_automaton(aut)
    assert not eng.automaton and not eng.processing
    eng.clear_beams()
    eng.set_automaton(aut)
    assert eng.automaton and eng.processing and eng.automaton_state(0, 4) == [-1] * 4
    eng.clear_automaton()
    assert not eng.automaton and not eng.processing   # the neutral processing it had turned on is off again
    eng.set_automaton(aut)
    with pytest.raises(_lib.EmmaxError, match="beams cannot be turned on while a token automaton is set"):
        eng.set_beams(BeamParams(2))
    for bad in ([8], [-2], [0, 1, 2, 3, 4]):
        with pytest.raises(_lib.EmmaxError, match="outside"):
            eng.set_automaton_starts(bad)
    eng.set_automaton_starts([7, -1])
    broken = ct.TokenAutomaton(V, aut.cls, aut.allow, aut.next)
    broken.cls = broken.cls.copy()
    broken.cls[V - 1] = aut.n_classes   # (past validate(): the library checks again)
    with pytest.raises(_lib.EmmaxError, match="class"):
        eng.set_automaton(broken)
    frames, rows = _inputs(1, seed=97)
    ids, lens = model.generate_ids(rows, frames_u8=torch.from_numpy(frames).to(device), max_new_tokens=3, stop_on_eos=False, constraint=aut, constraint_start=[7])
    assert aut.walk(ids[0].cpu().tolist(), 7)[-1] == eng.automaton_state(0, 1)[0]
    with pytest.raises(_lib.EmmaxError, match="logits processing is on"):
        eng.set_current_tokens([5])
    eng.clear_automaton()
    assert not eng.automaton


def test_clearing_the_automaton_leaves_no_trace(device):
    """A session that decoded under a constraint, then without one: its generation equals that of a session that never had one, id for id
    and log-probability bit for bit, and it is back on the finish it used before."""
    from emmax.sampling import SamplingParams

    frames, rows = _inputs(2, seed=62)

    def run(model, first):
        fr = torch.from_numpy(frames).to(device)
        if first:
            aut = cr.make_automaton(model.config.llm.vocab_size)
            model.generate_ids(rows, frames_u8=fr, max_new_tokens=4, stop_on_eos=False, sampling=SamplingParams(1.0, 50, 1.0, 3), constraint=aut)
            assert model.engine.automaton and model.engine.processing
        ids, lens, lp = model.generate_ids(rows, frames_u8=fr, max_new_tokens=8, stop_on_eos=False, sampling=SamplingParams(0.9, 40, 0.9, 5), return_logprobs=True)
        assert not model.engine.automaton and not model.engine.processing
        greedy, _ = model.generate_ids(rows, frames_u8=fr, max_new_tokens=8, stop_on_eos=False)
        return ids.cpu(), lp.cpu().view(torch.int32), greedy.cpu()

    a = run(_model(device, 2)[0], True)
    b = run(_model(device, 2)[0], False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
