"""Scoring without logits against the parent's way of getting the same three numbers, on one MI355X (not the headline bench).

Emma-X-7B shapes, synthetic weights, language-only prefills of 768 ids per row: one frame's worth of rows (B = 1, 768 rows) and eight (B = 8, 6144
rows).  Behind each prefill two routes to (lse, target logit, argmax) of every row alternate in one process, `--reps` times each after `--warmup`
untimed rounds on every shape, timed with device events; median and the min .. max spread are reported:
  (a) fused   emmax_prefill_score: the final norm, the scoring launch and its merge; three [rows] arrays leave the chip
  (b) logits  emmax_prefill_logits into a FRESH fp32 [rows, vocab] buffer, then torch.logsumexp, gather and argmax on it
with torch.cuda.max_memory_allocated above the level before the call for both, and the scoring launches alone (emmax_op_score_rows on operands of
the same shape: no norm) with their achieved TFLOP/s, 2 x rows x K x Np over their time.  Writes profiles/score_bench.txt (or --out)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd")]
import torch

from emmax import _lib
from emmax.config import EmmaXConfig
from emmax.modeling import EmmaXForActionPrediction

LEN = 768
BS = (1, 8)


def timed(fn):
    """(ms between two device events around fn, bytes the allocator's peak rose above the level before the call, fn's result)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base, out


def spread(ts):
    return f"{statistics.median(ts):8.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiny", action="store_true", help="the tiny config (a dry run of the tool, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = EmmaXConfig.tiny() if args.tiny else EmmaXConfig.emma_x_7b()
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=5, device=dev, max_batch=max(BS), max_prompt=LEN, max_ctx=cfg.n_patches + LEN + 16)
    eng, lib = model.engine, model.engine.lib
    V, K = cfg.llm.vocab_size, cfg.llm.hidden_size
    Np = (V + 127) // 128 * 128
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, min(V, 31744), (max(BS), LEN), generator=g).tolist()
    st = _lib.current_stream()
    lines = [f"score_bench: {'tiny' if args.tiny else 'Emma-X-7B shapes'} (vocab {V}, hidden {K}), {LEN} rows per sequence, {args.reps} alternating runs after {args.warmup} "
             "warm-up rounds per shape, device events; ms: median (min .. max)",
             "   B  rows | (a) fused score           peak bytes | (b) logits + torch reduce   peak bytes | (a)/(b) | plan rt x slices (tiles/slice) | scoring launches alone: ms, TFLOP/s"]
    same = True
    for B in BS:
        rows = B * LEN
        eng.prefill([r for r in ids[:B]], None)
        tg = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32).to(dev)
        out = torch.empty(3, rows, dtype=torch.float32, device=dev)

        def fused():
            _lib.check(lib.emmax_prefill_score(eng._session, tg.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), st), "emmax_prefill_score")
            return out

        def through_logits():
            z = torch.empty(rows, V, dtype=torch.float32, device=dev)
            _lib.check(lib.emmax_prefill_logits(eng._session, z.data_ptr(), st), "emmax_prefill_logits")
            return torch.logsumexp(z, -1), z.gather(1, tg.long()[:, None])[:, 0], z.argmax(-1)

        ta, tb, pa, pb = [], [], 0, 0
        for i in range(args.warmup + args.reps):
            a_ms, a_peak, a = timed(fused)
            a = [x.clone() for x in (a[0], a[1], a[2].view(torch.int32))]
            b_ms, b_peak, b = timed(through_logits)
            if i >= args.warmup:
                ta.append(a_ms); tb.append(b_ms); pa, pb = max(pa, a_peak), max(pb, b_peak)
        # the two routes agree: ids wherever the logits are not tied, lse / logit to fp32 noise
        same = same and bool((a[0] - b[0]).abs().max() < 1e-3) and bool((a[1] - b[1]).abs().max() < 1e-3) and float((a[2].long() != b[2]).float().mean()) < 1e-3
        o = [C.c_int(0) for _ in range(4)]
        ws_bytes = 64 << 20
        _lib.check(lib.emmax_score_plan(rows, V, K, ws_bytes, *[C.byref(x) for x in o]), "emmax_score_plan")
        # the launches alone, on operands of the same shape
        X = torch.randn(rows, K, generator=g).to(torch.bfloat16).to(dev)
        W = (torch.randn(Np, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)

        def alone():
            _lib.check(lib.emmax_op_score_rows(X.data_ptr(), K, W.data_ptr(), K, rows, V, Np, K, tg.data_ptr(), 0, ws.data_ptr(), ws_bytes, out[0].data_ptr(),
                                               out[1].data_ptr(), out[2].data_ptr(), st), "emmax_op_score_rows")

        tk = [timed(alone)[0] for _ in range(args.warmup + args.reps)][args.warmup:]
        k_ms = statistics.median(tk)
        tf = 2.0 * rows * K * Np / (k_ms * 1e-3) / 1e12
        lines.append(f"{B:4d} {rows:5d} | {spread(ta)} {pa:12d} | {spread(tb)} {pb:12d} | {statistics.median(ta) / statistics.median(tb):7.3f} | "
                     f"{o[0].value} x {o[2].value} ({o[3].value}) | {spread(tk)} {tf:7.1f}")
        print(lines[-1], flush=True)
        del X, W, ws
    lines.append(f"the two routes agree on every shape (lse / logit within 1e-3, ids but for < 0.1 % near-ties): {'yes' if same else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
