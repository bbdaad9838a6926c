"""Draft-verified greedy decoding against plain greedy decoding of the same build, on one MI355X (not the headline bench).

Emma-X-7B shapes, synthetic PLANTED weights (the answer is a known chain of ids), one frame, a 512-token prompt, 512 new tokens, EOS off as
bench.py has it.  The draft is the answer itself with m in {0, 4, 16, 64} evenly spaced substitutions, with one deletion and one insertion, and
a draft that has nothing to do with the answer.  Drafted and plain generate_ids alternate in one process (one box, one model build), `--reps`
times each, median reported: ms per call, verify passes, plain steps, tokens per pass; the ids must equal the plain run's in every case.
Then one verify pass alone at windows of 8 / 32 / 128 ids on the 768-token context against emmax_extend of as many ids, alternating.
Writes profiles/draft_bench.txt (or --out)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd")]
import numpy as np
import torch

from emmax.config import EmmaXConfig, default_norm_stats
from emmax.drafting import DraftParams
from emmax.modeling import EmmaXForActionPrediction
from emmax.weights import planted_start_token, synthetic_state_dict

PROMPT, NEW = 512, 512
WINDOWS = (8, 32, 128)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def drafts(answer, rng):
    def sub(m):
        d = list(answer)
        for k in np.linspace(8, len(d) - 8, m).astype(int) if m else []:
            d[int(k)] = 3 + (d[int(k)] + 4321) % 30000
        return d
    out = {f"{m} substitutions": sub(m) for m in (0, 4, 16, 64)}
    k = len(answer) // 2
    out["1 deletion + 1 insertion"] = answer[:k // 2] + answer[k // 2 + 1:k] + [12345] + answer[k:]
    out["unrelated"] = [int(x) for x in rng.integers(3, 30000, size=len(answer))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="the tiny config (a dry run of the tool, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draft_bench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = EmmaXConfig.tiny() if args.tiny else EmmaXConfig.emma_x_7b()
    # the planted weights are generated with the config's real EOS id (the successor map names it as a row of the lm-head), EOS goes off afterwards
    sd = synthetic_state_dict(cfg, seed=5, device=dev, dtype=torch.bfloat16, planted=True)
    cfg.eos_token_id = -1
    cfg.norm_stats = cfg.norm_stats or default_norm_stats()
    model = EmmaXForActionPrediction(cfg, sd).to(dev, max_batch=1, max_prompt=PROMPT, max_ctx=cfg.n_patches + PROMPT + NEW + 16)
    eng = model.engine
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, size=(1, 224, 224, 3), dtype=np.uint8)).to(dev)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=PROMPT - 2)] + [planted_start_token(cfg, 1000)]]
    params = DraftParams()

    def plain():
        ids, lens = model.generate_ids(rows, frames_u8=frames, max_new_tokens=NEW, stop_on_eos=False)
        return ids[0, : int(lens[0])].cpu().tolist(), None

    def drafted(d):
        ids, lens, st = model.generate_ids(rows, frames_u8=frames, max_new_tokens=NEW, stop_on_eos=False, draft=[d], draft_params=params, return_draft_stats=True)
        return ids[0, : int(lens[0])].cpu().tolist(), st

    answer, _ = plain()   # (warms up: allocations, graph capture)
    assert len(answer) == NEW, len(answer)
    lines = [f"draft_bench: {'tiny' if args.tiny else 'Emma-X-7B shapes'}, planted weights, 1 frame, {PROMPT}-token prompt, {NEW} new tokens, EOS off; "
             f"DraftParams(window={params.window}, ngram={params.ngram}, burst={params.burst}, give_up={params.give_up}); median of {args.reps} alternating runs",
             "draft                      | drafted ms   plain ms  drafted/plain | passes  plain steps  tokens/pass | ids equal"]
    ok = True
    for name, d in drafts(answer, rng).items():
        td, tp, st, same = [], [], None, True
        drafted(d)   # (the first drafted call of a shape plans its passes)
        for _ in range(args.reps):
            t, (got, st) = wall(lambda: drafted(d))
            td.append(t)
            same = same and got == answer
            t, (got, _) = wall(plain)
            tp.append(t)
            same = same and got == answer
        a, b = statistics.median(td), statistics.median(tp)
        ok = ok and same
        lines.append(f"{name:26s} | {a:10.2f} {b:10.2f} {a / b:14.3f} | {st.passes:6d} {st.plain_steps:12d} {st.tokens_per_pass:12.1f} | {'yes' if same else 'NO'}")
        print(lines[-1], flush=True)
    # one verify pass alone against emmax_extend of as many ids, on the prompt's 768-token context
    lines.append("one pass at context 768   | verify ms  extend ms  verify - extend")
    for n in WINDOWS:
        tv, te = [], []
        for _ in range(args.reps + 1):
            model._prefill(rows, None, frames, max_new=NEW)
            w = [answer[0]] + answer[1:n]
            t, (emitted, _, _) = wall(lambda: eng.verify([w], max_new=NEW))
            assert emitted == [n], (n, emitted)
            tv.append(t)
            model._prefill(rows, None, frames, max_new=NEW)
            t, _ = wall(lambda: eng.extend([w], max_new_tokens=1))
            te.append(t)
        a, b = statistics.median(tv[1:]), statistics.median(te[1:])
        lines.append(f"window {n:4d}               | {a:9.3f} {b:10.3f} {a - b:16.3f}")
        print(lines[-1], flush=True)
    lines.append(f"ids equal to the plain run in every case: {'yes' if ok else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
