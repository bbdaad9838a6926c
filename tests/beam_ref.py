"""numpy restatement of the beam search of the decode step (include/emmax.h, ABI 9) in its pinned fp32 arithmetic.  TEST INFRASTRUCTURE ONLY.

Every score operation is one np.float32 operation, in the order the device performs them, so that a replay over the device's own logit
rows and lse values reproduces its candidate lists, parents, tokens, scores and finished set bit for bit:

    acc   = fp32(fp32(l - lse) + score)                 per running row; lse given (the device's) or float64 log-sum-exp rounded to fp32
    top   per group the best 2K of the K x V candidates, acc descending, equal acc by the lower flat index beam * V + token; NaN never enters
    run   best K of fp32(acc + -1e9 [stopped]), ties to the lower place in the list
    fin   best K of [kept K, fp32(acc / pw[n]) + -1e9 masks], ties to the lower place; pw[n] = fp32(n ** length_penalty) (double pow)
    stop  HF's heuristic and done flag (transformers 5.15 GenerationMixin._beam_search)

`BeamGroup.step` is one step of one group; `beam_search` drives it over a `step_fn(list of K generated-id lists) -> logits [K, V]`."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

F = np.float32
NEG = F(-1.0e9)


def lse_f64(row: np.ndarray) -> np.float32:
    r = np.asarray(row, dtype=np.float64)
    m = r.max()
    return F(m + np.log(np.exp(r - m).sum()))


def pw_table(n_max: int, length_penalty: float) -> np.ndarray:
    out = np.ones(n_max + 1, dtype=np.float32)
    for n in range(1, n_max + 1):
        out[n] = F(float(n) ** float(length_penalty))
    return out


def row_candidates(row: np.ndarray, lse, score, n: int):
    """The row's best n (acc, token) pairs, acc descending, token ascending on equal acc; NaN entries never enter."""
    acc = (np.asarray(row, dtype=np.float32) - F(lse)).astype(np.float32) + F(score)
    acc = acc.astype(np.float32)
    idx = np.nonzero(~np.isnan(acc))[0]
    if idx.size == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64)
    if idx.size > n:
        thr = np.partition(acc[idx], idx.size - n)[idx.size - n]
        idx = idx[acc[idx] >= thr]
    order = np.lexsort((idx, -acc[idx].astype(np.float64)))[:n]
    return acc[idx][order], idx[order]


def take_best(v: Sequence, taken: List[bool]) -> int:
    """The first entry not yet taken, replaced by any later one that compares greater (the device's rule; a NaN only where it comes first)."""
    best = -1
    for i in range(len(v)):
        if taken[i]:
            continue
        if best < 0 or v[i] > v[best]:
            best = i
    if best >= 0:
        taken[best] = True
    return best


class BeamGroup:
    def __init__(self, K: int, V: int, max_new: int, eos: int = -1, length_penalty: float = 1.0, early_stopping=False):
        self.K, self.V, self.max_new, self.eos = K, V, max_new, eos
        self.es = {False: 0, True: 1, "never": 2}[early_stopping]
        self.lp_pos = float(length_penalty) > 0.0
        self.pw = pw_table(max_new, length_penalty)
        self.run = np.full(K, NEG, np.float32)
        self.run[0] = F(0.0)
        # kept hypotheses: score, finished flag, and how they ended (step, parent beam, token); step -1 = never filled
        self.fin_score = np.full(K, NEG, np.float32)
        self.fin_flag = [False] * K
        self.fin_end = [(-1, 0, -1)] * K
        self.unsat, self.done, self.t = True, False, 0
        self.tok: List[List[int]] = []      # per step, per running beam
        self.par: List[List[int]] = []
        self.min_gap = np.inf               # smallest relative gap between adjacent candidates among the best 2K + 1 (see step)

    def step(self, rows: np.ndarray, lses: Optional[Sequence] = None, scores: Optional[Sequence] = None, gaps: bool = False):
        """One step over the logit rows of the running beams ([K, V]; step 0 may pass the single prefill row [1, V]).  lses: the rows' lse
        (default: float64, rounded); scores: the running scores to start from (default: the state's).  Returns the step's record."""
        K, V, t = self.K, self.V, self.t
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, V)
        nrows = rows.shape[0]
        if lses is None:
            lses = [lse_f64(r) for r in rows]
        run_in = self.run if scores is None else np.asarray(scores, dtype=np.float32)
        want = 2 * K + (1 if gaps else 0)
        accs, flats = [], []
        for r in range(nrows):
            a, tk = row_candidates(rows[r], lses[r], run_in[r], want)
            accs.append(a)
            flats.append(r * V + tk)
        acc = np.concatenate(accs).astype(np.float32)
        flat = np.concatenate(flats)
        order = np.lexsort((flat, -acc.astype(np.float64)))[:want]
        acc, flat = acc[order], flat[order]
        if gaps and acc.size > 1:
            g = (acc[:-1].astype(np.float64) - acc[1:].astype(np.float64)) / np.maximum(1.0, np.abs(acc[:-1].astype(np.float64)))
            self.min_gap = min(self.min_gap, float(g.min()))
        acc, flat = acc[: 2 * K], flat[: 2 * K]
        nc = acc.size
        rec = {"t": t, "cand_idx": [int(x) for x in flat] + [-1] * (2 * K - nc), "cand_acc": [F(x) for x in acc] + [F(0)] * (2 * K - nc),
               "lse": [F(x) for x in lses]}
        if nc == 0:
            self.done = True
            rec.update(tok=[-1] * K, parent=[-1] * K, score=[F(0)] * K, done=True)
            return rec
        n, mx = t + 1, self.max_new
        c_par = [int(x) // V for x in flat]
        c_tok = [int(x) % V for x in flat]
        hits = [c_tok[c] == self.eos or n >= mx for c in range(nc)]
        rl = [F(acc[c] + NEG) if hits[c] else F(acc[c]) for c in range(nc)]
        taken = [False] * nc
        sel = [take_best(rl, taken) for _ in range(K)]
        full = self.es == 1 and all(self.fin_flag)
        pwn = self.pw[n]
        fs = [F(x) for x in self.fin_score]
        for c in range(nc):
            sc = F(acc[c] / pwn)
            if full:
                sc = F(sc + NEG)
            if not self.unsat:
                sc = F(sc + NEG)
            if not (hits[c] and c < K):
                sc = F(sc + NEG)
            fs.append(sc)
        taken = [False] * (K + nc)
        n_score, n_flag, n_end = [], [], []
        for _ in range(K):
            i = take_best(fs, taken)
            if i < K:
                n_score.append(F(self.fin_score[i])); n_flag.append(self.fin_flag[i]); n_end.append(self.fin_end[i])
            else:
                c = i - K
                n_score.append(fs[i]); n_flag.append(bool(hits[c] and c < K)); n_end.append((t, c_par[c], c_tok[c]))
        self.fin_score, self.fin_flag, self.fin_end = np.array(n_score, np.float32), n_flag, n_end
        fmin = n_score[0]
        for s in n_score[1:]:
            fmin = s if s < fmin else fmin
        Lh = mx if (self.es == 2 and self.lp_pos) else n
        best = F(rl[sel[0]] / self.pw[Lh])
        any_ = any(best > (fmin if n_flag[k] else NEG) for k in range(K))
        self.unsat = self.unsat and any_
        self.done = not (self.unsat and not (all(n_flag) and self.es == 1) and not all(hits))
        self.run = np.array([rl[j] for j in sel], np.float32)
        self.tok.append([c_tok[j] for j in sel])
        self.par.append([c_par[j] for j in sel])
        self.t = n
        rec.update(tok=self.tok[-1], parent=self.par[-1], score=[F(x) for x in self.run], done=self.done)
        return rec

    def sequences_of_running(self) -> List[List[int]]:
        """The generated ids of the K running beams after the last step."""
        return [self.lineage(len(self.tok) - 1, k)[0] for k in range(self.K)]

    def lineage(self, t: int, k: int):
        """(tokens, parent beams) of running beam k after step t, steps 0 .. t."""
        toks, pars = [], []
        b = k
        for s in range(t, -1, -1):
            toks.append(self.tok[s][b])
            b = self.par[s][b]
            pars.append(b)
        return toks[::-1], pars[::-1]

    def result(self, pad: int, row0: int = 0):
        """Kept hypotheses, best first: (sequences [K][max_new] padded, lengths, scores fp32, beam_indices [K][max_new], -1 behind the end);
        beam_indices count rows from row0 (= group * K)."""
        seqs, lens, bidx = [], [], []
        for k in range(self.K):
            ft, fp, fk = self.fin_end[k]
            if ft < 0:
                toks, pars = [], []
            else:
                toks, pars = (self.lineage(ft - 1, fp) if ft > 0 else ([], []))
                toks, pars = toks + [fk], pars + [fp]
            lens.append(len(toks))
            seqs.append(toks + [pad] * (self.max_new - len(toks)))
            bidx.append([row0 + p for p in pars] + [-1] * (self.max_new - len(toks)))
        return np.array(seqs, np.int64), np.array(lens, np.int64), self.fin_score.copy(), np.array(bidx, np.int64)


def beam_search(step_fn: Callable[[List[List[int]]], np.ndarray], K: int, V: int, max_new: int, eos: int = -1, pad: int = 0,
                length_penalty: float = 1.0, early_stopping=False, gaps: bool = False):
    """One group, driven like the device: step 0 over the single prompt row, then K rows per step until the group is done."""
    g = BeamGroup(K, V, max_new, eos, length_penalty, early_stopping)
    trace = [g.step(np.asarray(step_fn([[]]))[:1], gaps=gaps)]
    while not g.done and g.t < max_new:
        trace.append(g.step(step_fn(g.sequences_of_running()), gaps=gaps))
    seqs, lens, scores, bidx = g.result(pad)
    return {"sequences": seqs, "lengths": lens, "scores": scores, "beam_indices": bidx, "trace": trace, "min_gap": g.min_gap, "group": g}
