"""ms per decode step with top-N / watched-token log-probabilities bound (include/emmax.h: emmax_session_set_top_logprobs) against the same
sampled step without them, on the synthetic Emma-X-7B shapes at B = 1 and 64 rows.

  off        sampling on (temperature 1, top-k 50: the HF defaults), nothing bound -- the step of the parent commit
  n5 / n20   the 5 / 20 most likely ids of every emitted token
  n20w256    the 20 most likely ids and the 256 action-bin ids watched

The modes ALTERNATE inside one process on one box (round r runs every mode once, in order), the time of one generate call after its prefill
divided by its decode steps (new tokens - 1); per mode the median over the rounds and the spread (min .. max).  EOS is disabled, so every
row decodes every step.  `cost_us` is a mode's median minus off's, in microseconds per step; `x_draw` is that over the yardstick, the sampled
finish that reads the same rows (--draw-us, 45 us per draw at B = 1: README / DESIGN.md 6).

--vs-lib PATH: the feature-off path of another build of the library (the parent commit's libemmax_hip.so) against this build's: fresh child
processes, alternating other / this / other / this, each measuring `greedy` (sampling off) and `off`; per build the median and the spread.
One JSON line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd")]


def measure(args, modes):
    import numpy as np
    import torch

    from emmax import _lib

    if args.lib:   # another build: bind the symbols it exports (an older one lacks the newest; the feature-off path calls none of them)
        import ctypes

        _lib.LIB_PATH = os.path.abspath(args.lib)
        other = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(other, n)]:
            del _lib.SIGNATURES[name]
    from emmax.actions import action_bin_token_ids
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.sampling import SamplingParams

    dev = "cuda:0"
    batches = [int(b) for b in args.batches.split(",")]
    cfg = EmmaXConfig.tiny() if args.tiny else EmmaXConfig.emma_x_7b()
    cfg.eos_token_id = -1
    P, T = args.prompt_tokens, args.new_tokens
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=0, device=dev, max_batch=max(batches), max_prompt=P, max_ctx=cfg.n_patches + P + T + 1)
    eng = model.engine
    rng = np.random.default_rng(1234)
    frames = torch.from_numpy(rng.integers(0, 256, size=(max(batches), 224, 224, 3), dtype=np.uint8)).to(dev)
    prompts = [[1] + [int(x) for x in rng.integers(3, 31744, size=P - 1)] for _ in range(max(batches))]
    hf = SamplingParams(1.0, 50, 1.0, seed=1)
    bins = action_bin_token_ids(model.vocab_size, cfg.n_action_bins) if hasattr(eng, "set_top_logprobs") else []
    table = {"greedy": (None, None), "off": (hf, None), "n5": (hf, (5, [])), "n20": (hf, (20, [])), "n20w256": (hf, (20, bins))}
    out = []
    for B in batches:
        times = {m: [] for m in modes}
        for rnd in range(args.reps + 1):   # (round 0 warms up: graph capture, first touch of the logit rows and of the bound buffers)
            for m in modes:
                samp, top = table[m]
                kw = {} if top is None else {"top": top}
                model._prefill(prompts[:B], frames_u8=frames[:B], max_new=T, sampling=samp, **kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids, lens = eng.generate(T, stop_on_eos=False)
                torch.cuda.synchronize()
                if rnd:
                    times[m].append(1e3 * (time.perf_counter() - t0) / (T - 1))
                assert int(lens.min()) == T, "a row ended early"
        for m in modes:
            out.append({"batch": B, "mode": m, "ms_per_step": round(float(np.median(times[m])), 4), "min": round(min(times[m]), 4),
                        "max": round(max(times[m]), 4), "prompt": P, "new_tokens": T, "rounds": args.reps})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--prompt-tokens", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draw-us", type=float, default=45.0, help="the yardstick: one sampled draw at B = 1, top-k 50 (DESIGN.md section 6)")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--lib", default="", help="(child) the libemmax_hip.so to load instead of this tree's")
    ap.add_argument("--child", action="store_true", help="(child) measure greedy and off only, print the JSON lines")
    ap.add_argument("--vs-lib", default="", help="another build's libemmax_hip.so: its feature-off step against this build's, alternating child processes")
    ap.add_argument("--alternations", type=int, default=2)
    args = ap.parse_args()
    if args.child:
        for rec in measure(args, ["greedy", "off"]):
            print(json.dumps(rec), flush=True)
        return
    if args.vs_lib:
        import numpy as np

        runs = {}
        for k in range(2 * args.alternations):
            who = "other" if k % 2 == 0 else "this"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batches", args.batches, "--prompt-tokens", str(args.prompt_tokens), "--new-tokens",
                   str(args.new_tokens), "--reps", str(args.reps)] + (["--tiny"] if args.tiny else []) + (["--lib", args.vs_lib] if who == "other" else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.exit(f"child ({who}) failed with {res.returncode}:\n{res.stderr[-2000:]}")
            for line in res.stdout.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    runs.setdefault((who, r["batch"], r["mode"]), []).append(r["ms_per_step"])
        for (who, B, m), v in sorted(runs.items(), key=lambda kv: (kv[0][1], kv[0][2], kv[0][0])):
            print(json.dumps({"build": who, "batch": B, "mode": m, "ms_per_step": round(float(np.median(v)), 4), "min": min(v), "max": max(v), "processes": len(v)}), flush=True)
        return
    recs = measure(args, ["off", "n5", "n20", "n20w256"])
    base = {r["batch"]: r["ms_per_step"] for r in recs if r["mode"] == "off"}
    for r in recs:
        if r["mode"] != "off":
            r["cost_us"] = round(1e3 * (r["ms_per_step"] - base[r["batch"]]), 1)
            r["x_draw"] = round(r["cost_us"] / args.draw_us, 2)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
