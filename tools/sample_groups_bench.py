"""Sample groups (generate(do_sample=True, num_return_sequences=N); include/emmax.h: emmax_session_set_sample_groups) against the same prompt
expanded N times in Python, at the shapes of the headline bench: Emma-X-7B synthetic weights, context 768 (256 patch rows + 512 prompt ids),
100 new tokens, one prompt, N = 4 and 8.

  group     one frame, one prompt, num_samples = N: one vision pass, a one-row prefill, the fork, then N sampled rows
  expanded  the frame and the prompt repeated N times: N vision passes, an N-row prefill, N copies of the prompt's KV pages

Both decode N sampled rows with the same per-row (seed, subseq), so the step launches the same kernels; what differs is everything before
the first token, and that the group's rows read the prompt's pages at the same addresses.  Per variant:
  first_token_ms  vision + prefill (+ fork) + the draw of token 0
  ms_per_step     one generate call after its prefill, divided by its decode steps (new tokens - 1)
  actions_ms      generate_actions_batch end to end: frames + prompts -> actions
The two variants are measured INTERLEAVED, --rounds times on one box; each figure is the median over the rounds, and `spread` is max - min
over the rounds of the same variant -- the noise a difference between the variants has to clear.  EOS is disabled (as in bench.py).
Prints one JSON line per N.

--attn-ab POINTS: the grouped decode attention (tuning switch attn_group; include/emmax.h: emmax_session_attn_grouped) against the launch of a
plain batch, on the same build: attn_group = 0 / 1 ALTERNATE in this process on this box, --rounds times after a warm-up round; each figure is
the median over the rounds and `spread` is max - min.  attn_group = 0 launches the attention the build before the route launched (the
route function returns 0 and the step takes the old branch).  POINTS: "GxN" = G prompts of context 256 + --prompt-tokens with N samples
each (1x8, 2x8, 8x8 = 64 rows), "beamK" = one group of K beams.  Per point and switch value: ms_per_step as above, and attn_us = one
attention stage (both launches of the grouped route) timed by emmax_profile_decode_stage on the forked session (sample groups only: beams
fork inside generate).  One JSON line per point."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd")]
import numpy as np
import torch

from emmax.config import EmmaXConfig
from emmax.modeling import EmmaXForActionPrediction
from emmax.sampling import SamplingParams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8")
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--variants", default="group,expanded", help="one of them alone: a run to put under `rocprofv3 --kernel-trace --stats`")
    ap.add_argument("--attn-ab", default="", help='operating points of the attn_group A/B, e.g. "1x8,2x8,8x8,beam8" (replaces the group / expanded run)')
    args = ap.parse_args()
    dev = "cuda:0"
    ns = [int(n) for n in args.samples.split(",")]
    cfg = EmmaXConfig.tiny() if args.tiny else EmmaXConfig.emma_x_7b()
    cfg.eos_token_id = -1
    P, T = args.prompt_tokens, args.new_tokens
    if args.attn_ab:
        return attn_ab(args, cfg, dev)
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=0, device=dev, max_batch=max(ns), max_prompt=P, max_ctx=cfg.n_patches + P + T + 1)
    eng = model.engine
    rng = np.random.default_rng(1234)
    frame = torch.from_numpy(rng.integers(0, 256, size=(1, 224, 224, 3), dtype=np.uint8)).to(dev)
    prompt = [1] + [int(x) for x in rng.integers(3, 31744, size=P - 1)]
    samp = SamplingParams(1.0, 50, 1.0, seed=1)   # the HF defaults; row r draws with subseq r in both variants

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for N in ns:
        frames_n = frame.expand(N, -1, -1, -1).contiguous()
        variants = {
            "group": dict(rows=[prompt], fr=frame, kw=dict(num_samples=N)),
            "expanded": dict(rows=[prompt] * N, fr=frames_n, kw={}),
        }
        variants = {k: v for k, v in variants.items() if k in args.variants.split(",")}
        figs = {v: {"first_token_ms": [], "ms_per_step": [], "actions_ms": []} for v in variants}
        ids = {}
        for rnd in range(args.rounds + 1):   # (round 0 warms up: weight copies of the batch, graph capture, first touch of the logit rows)
            for name, v in variants.items():
                pre = lambda: model._prefill(v["rows"], frames_u8=v["fr"], max_new=T, sampling=samp, **v["kw"])
                first = timed(lambda: (pre(), eng.generate(1, stop_on_eos=False)))
                pre()
                out = []
                step = timed(lambda: out.append(eng.generate(T, stop_on_eos=False))) / (T - 1)
                assert int(out[0][1].min()) == T and out[0][0].shape[0] == N
                ids[name] = out[0][0].cpu()
                act = timed(lambda: model.generate_actions_batch(v["fr"], v["rows"], T, stop_on_eos=False, sampling=samp, **v["kw"]))
                if rnd:
                    for k, x in (("first_token_ms", first), ("ms_per_step", step), ("actions_ms", act)):
                        figs[name][k].append(x)
        rec = {"num_samples": N, "context": cfg.n_patches + P, "new_tokens": T, "rounds": args.rounds,
               "same_first_tokens": bool(torch.equal(ids["group"][:, 0], ids["expanded"][:, 0])) if len(ids) == 2 else None}
        for name in variants:
            for k, xs in figs[name].items():
                rec[f"{name}_{k}"] = round(float(np.median(xs)), 4)
                rec[f"{name}_{k}_spread"] = round(float(max(xs) - min(xs)), 4)
        print(json.dumps(rec), flush=True)
    eng.clear_sample_groups()
    eng.clear_sampling()


def attn_ab(args, cfg, dev):
    from emmax import _lib
    from emmax.sampling import BeamParams

    P, T = args.prompt_tokens, args.new_tokens
    points = []
    for name in args.attn_ab.split(","):
        points.append((name, 1, int(name[4:]), True) if name.startswith("beam") else (name, int(name.split("x")[0]), int(name.split("x")[1]), False))
    rows_max = max(g * n for _, g, n, _ in points)
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=0, device=dev, max_batch=rows_max, max_prompt=P, max_ctx=cfg.n_patches + P + T + 1)
    eng = model.engine
    rng = np.random.default_rng(1234)
    samp = SamplingParams(1.0, 50, 1.0, seed=1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for name, G, N, beam in points:
        frames = torch.from_numpy(rng.integers(0, 256, size=(G, 224, 224, 3), dtype=np.uint8)).to(dev)
        prompts = [[1] + [int(x) for x in rng.integers(3, 31744, size=P - 1)] for _ in range(G)]
        kw = dict(beams=BeamParams(N, 1.0, False, N)) if beam else dict(sampling=samp, num_samples=N)
        figs = {sw: {"ms_per_step": [], "attn_us": []} for sw in (0, 1)}
        for rnd in range(args.rounds + 1):   # (round 0 warms up)
            for sw in (0, 1):
                with _lib.tuning(attn_group=sw):
                    us = float("nan")
                    if not beam:   # (beams fork inside generate and are done behind it: rows flagged done read nothing -- not covered)
                        model._prefill(prompts, frames_u8=frames, max_new=T, **kw)
                        us = eng.profile_decode_stage(1, 5)   # the forked rows at the prompt's context; leaves garbage rows: prefill again
                    model._prefill(prompts, frames_u8=frames, max_new=T, **kw)
                    out = []
                    step = timed(lambda: out.append(eng.generate(T, stop_on_eos=False))) / (T - 1)
                    assert out[0][0].shape[0] == G * N and (sw or not eng.attn_grouped(G * N))
                    if sw and not eng.attn_grouped(G * N):
                        raise SystemExit(f"{name}: a step of {G * N} rows does not take the grouped route (fewer than 5 rows at 32 heads?): nothing to compare")
                if rnd:
                    figs[sw]["ms_per_step"].append(step)
                    figs[sw]["attn_us"].append(us)
        rec = {"point": name, "groups": G, "rows_per_group": N, "context": cfg.n_patches + P, "new_tokens": T, "layers": cfg.llm.num_layers, "rounds": args.rounds}
        for sw in (0, 1):
            for k, xs in figs[sw].items():
                rec[f"attn_group{sw}_{k}"] = round(float(np.median(xs)), 4)
                rec[f"attn_group{sw}_{k}_spread"] = round(float(max(xs) - min(xs)), 4)
        print(json.dumps(rec), flush=True)
        (eng.clear_beams() if beam else eng.clear_sample_groups())
    eng.clear_sampling() if eng.sampling else None


if __name__ == "__main__":
    main()
