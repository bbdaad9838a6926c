"""ms per decode step of generate with sampling (include/emmax.h ABI 7) or logits processing / scores (ABI 8) in the step against the
greedy step, at the shapes of the headline bench (Emma-X-7B synthetic weights, 512-token prompts, 512 new tokens) and batches 1, 8 and 64.

  greedy   sampling off: the kernels of a session that never sampled
  t0       sampling on, every row at temperature 0 (the argmax of the fp32 logit rows)
  hf       temperature 1, top-k 50 (the HF defaults)
  topp     temperature 1, top-p 0.9
  pgreedy  repetition penalty 1.1 and no_repeat_ngram_size 3, greedy (the processing finish)
  phf      the same with the HF-default draw
  pscores  pgreedy with output_scores: the processed rows stored at every step ([new tokens, B, vocab] fp32)
  minp / typ / eps / eta   hf with min_p 0.05 / typical_p 0.9 / epsilon_cutoff 3e-4 / eta_cutoff 1e-3 (the EXT finish)
  warp4    hf with all four;  rules256   hf with a table of 256 rules (the 256 action ids suppressed)

--beams K1,K2,..  (ABI 9) instead: one K-beam group (`generate(num_beams=K)`: G = 1, K rows on shared KV pages) against K independent greedy
rows of the same prompt -- ms per step, time to the first token (prefill + first step: the beam group prefills ONE row) and end-to-end
`generate_actions_batch`; one JSON line per K.  For the kernel split run it under `rocprofv3 --kernel-trace --stats`.

EOS is disabled (as in bench.py), so every row decodes every step.  The time of one generate call after its prefill, divided by its decode
steps (new tokens - 1), median over --reps calls.  Prints one JSON line per (batch, mode)."""
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
from emmax.sampling import LogitsProcessing, SamplingParams

HF = SamplingParams(1.0, 50, 1.0, seed=1)
PROC = LogitsProcessing(1.1, 3, 0)
# mode -> (sampling, processing, scores)
MODES = {"greedy": (None, None, False), "t0": (SamplingParams(0.0, 0, 1.0, seed=1), None, False), "hf": (HF, None, False),
         "topp": (SamplingParams(1.0, 0, 0.9, seed=1), None, False), "pgreedy": (None, PROC, False), "phf": (HF, PROC, False),
         "pscores": (None, PROC, True)}
if "min_p" in SamplingParams.__dataclass_fields__:
    import dataclasses

    MODES.update({"minp": (dataclasses.replace(HF, min_p=0.05), None, False), "typ": (dataclasses.replace(HF, typical_p=0.9), None, False),
                  "eps": (dataclasses.replace(HF, epsilon_cutoff=3e-4), None, False), "eta": (dataclasses.replace(HF, eta_cutoff=1e-3), None, False),
                  "warp4": (dataclasses.replace(HF, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=1e-3), None, False),
                  "rules256": (HF, LogitsProcessing(suppress_tokens=list(range(31744, 32000))), False)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--beams", default="", help="comma list of num_beams: measure one beam group against as many greedy rows")
    args = ap.parse_args()
    dev = "cuda:0"
    beam_ks = [int(k) for k in args.beams.split(",") if k]
    batches = [int(b) for b in args.batches.split(",")] if not beam_ks else [max(beam_ks)]
    cfg = EmmaXConfig.tiny() if args.tiny else EmmaXConfig.emma_x_7b()
    cfg.eos_token_id = -1
    P, T = args.prompt_tokens, args.new_tokens
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=0, device=dev, max_batch=max(batches), max_prompt=P, max_ctx=cfg.n_patches + P + T + 1)
    eng = model.engine
    rng = np.random.default_rng(1234)
    frames = torch.from_numpy(rng.integers(0, 256, size=(max(batches), 224, 224, 3), dtype=np.uint8)).to(dev)
    prompts = [[1] + [int(x) for x in rng.integers(3, 31744, size=P - 1)] for _ in range(max(batches))]
    if beam_ks:
        return bench_beams(model, eng, cfg, frames, prompts, beam_ks, P, T, args.reps)
    for B in batches:
        for mode in args.modes.split(","):
            times = []
            samp, proc, want_scores = MODES[mode]
            sc = torch.empty(T, B, cfg.llm.vocab_size, dtype=torch.float32, device=dev) if want_scores else None
            for rep in range(args.reps + 1):   # (the first call warms up: graph capture, first-touch of the logit rows)
                model._prefill(prompts[:B], frames_u8=frames[:B], max_new=T, sampling=samp, processing=proc, scores=sc)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids, lens = eng.generate(T, stop_on_eos=False)
                torch.cuda.synchronize()
                if rep:
                    times.append(time.perf_counter() - t0)
            assert int(lens.min()) == T, "a row ended early"
            ms = 1e3 * float(np.median(times)) / (T - 1)
            print(json.dumps({"batch": B, "mode": mode, "ms_per_step": round(ms, 4), "prompt": P, "new_tokens": T, "reps": args.reps}), flush=True)
            del sc
            eng.set_scores(None, None)
    eng.clear_sampling()
    eng.clear_processing()


def bench_beams(model, eng, cfg, frames, prompts, ks, P, T, reps):
    from emmax.sampling import BeamParams

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def med(fn, prep=None):
        out = []
        for rep in range(reps + 1):   # (the first call warms up)
            if prep:
                prep()
            t = timed(fn)
            if rep:
                out.append(t)
        return 1e3 * float(np.median(out))

    for K in ks:
        same = [prompts[0]] * K
        fr_k = frames[:1].expand(K, -1, -1, -1).contiguous()
        bp = BeamParams(K, 1.0, False, 1)
        rec = {"num_beams": K, "prompt": P, "new_tokens": T, "reps": reps}
        # ms per step: generate after its prefill (the beam call includes the first beam step, the fork and the final resolve)
        rec["greedy_rows_ms_per_step"] = round(med(lambda: eng.generate(T, stop_on_eos=False), lambda: model._prefill(same, frames_u8=fr_k, max_new=T)) / (T - 1), 4)
        rec["beam_ms_per_step"] = round(med(lambda: eng.generate(T, stop_on_eos=False), lambda: model._prefill(prompts[:1], frames_u8=frames[:1], max_new=T, beams=bp)) / (T - 1), 4)
        # time to the first token: vision + prefill + the first step
        rec["beam_first_token_ms"] = round(med(lambda: (model._prefill(prompts[:1], frames_u8=frames[:1], max_new=T, beams=bp), eng.generate(1, stop_on_eos=False))), 3)
        rec["greedy_rows_first_token_ms"] = round(med(lambda: (model._prefill(same, frames_u8=fr_k, max_new=T), eng.generate(1, stop_on_eos=False))), 3)
        # end to end: frames + prompts -> actions
        rec["beam_actions_ms"] = round(med(lambda: model.generate_actions_batch(frames[:1], prompts[:1], T, stop_on_eos=False, beams=bp)), 2)
        rec["greedy_rows_actions_ms"] = round(med(lambda: model.generate_actions_batch(fr_k, same, T, stop_on_eos=False)), 2)
        print(json.dumps(rec), flush=True)
    eng.clear_beams()


if __name__ == "__main__":
    main()
