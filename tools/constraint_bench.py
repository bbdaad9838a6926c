"""ms per decode step of generate with a token automaton in the step (include/emmax.h: emmax_session_set_automaton) against the same step
without one, at the shapes of tools/sample_step_bench.py (Emma-X-7B synthetic weights, 512-token prompts) and batches 1 and 64, the modes
alternating in one process.

  greedy     sampling off: the kernels of a session that never sampled
  hf         temperature 1, top-k 50 (the HF defaults)
  policy3    hf with a 3-state policy_line automaton (free text until a one-id trigger, one bin token, free again), every row in it
  big1024    hf with a 1024-state, 256-class automaton (every state allows every class; the state moves with every token), every row in it
  gpolicy3   greedy with the policy3 automaton (the constrained finish at temperature 0)
  rules256   hf with a table of 256 one-id rules (the 256 action ids suppressed): the yardstick, measured alongside

EOS is disabled (as in bench.py) and no automaton here ends a row or leaves it without an allowed id, so every row decodes every step.  The
time of one generate call after its prefill, divided by its decode steps (new tokens - 1), median over --reps calls after one warm-up call.
Prints one JSON line per (batch, mode), then the costs per CALL that the per-step figures do not hold (--setup-reps): building the two automata on
the host, emmax_session_set_automaton (validation, re-layout, three copies behind a stream synchronisation) and what a call pays when the
automaton it names is the one the session holds.  A tree without emmax/constraints.py (the parent commit's) runs the modes it has: that is how the
unchanged paths are compared, this script copied into the other tree and the two builds alternating on one box."""
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

try:
    from emmax import constraints
except ImportError:   # (the parent commit's tree)
    constraints = None

HF = SamplingParams(1.0, 50, 1.0, seed=1)
RULES = LogitsProcessing(suppress_tokens=list(range(31744, 32000)))
# mode -> (sampling, processing, automaton name)
MODES = {"greedy": (None, None, None), "hf": (HF, None, None), "rules256": (HF, RULES, None)}
if constraints is not None:
    MODES.update({"policy3": (HF, None, "policy3"), "big1024": (HF, None, "big1024"), "gpolicy3": (None, None, "policy3")})


def automata(cfg):
    V = cfg.llm.vocab_size
    pol = constraints.policy_line([29871], V, cfg.n_action_bins, 1, token_vocab=cfg.action_vocab_size)
    S, C = constraints.MAX_STATES, constraints.MAX_CLASSES
    nxt = ((np.arange(S)[:, None] * 7 + np.arange(C)[None, :] + 1) % S).astype(np.int16)
    big = constraints.TokenAutomaton(V, (np.arange(V) % C).astype(np.uint8), np.full((S, 8), 0xFFFFFFFF, dtype=np.uint32), nxt, {"start": 0})
    assert pol.n_states == 3 and big.n_states == 1024 and big.n_classes == 256
    return {"policy3": pol, "big1024": big}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--prompt-tokens", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="hf,policy3,big1024,greedy,gpolicy3,rules256,hf")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--setup-reps", type=int, default=20, help="repetitions of the per-call measurements (0: skip them)")
    args = ap.parse_args()
    dev = "cuda:0"
    batches = [int(b) for b in args.batches.split(",")]
    cfg = EmmaXConfig.tiny() if args.tiny else EmmaXConfig.emma_x_7b()
    cfg.eos_token_id = -1
    P, T = args.prompt_tokens, args.new_tokens
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=0, device=dev, max_batch=max(batches), max_prompt=P, max_ctx=cfg.n_patches + P + T + 1)
    eng = model.engine
    auts = automata(cfg) if constraints is not None else {}
    rng = np.random.default_rng(1234)
    frames = torch.from_numpy(rng.integers(0, 256, size=(max(batches), 224, 224, 3), dtype=np.uint8)).to(dev)
    prompts = [[1] + [int(x) for x in rng.integers(3, 31744, size=P - 1)] for _ in range(max(batches))]
    for B in batches:
        for mode in args.modes.split(","):
            if mode not in MODES:
                continue
            samp, proc, aut = MODES[mode]
            kw = {} if aut is None else {"constraint": auts[aut]}
            times = []
            for rep in range(args.reps + 1):   # (the first call warms up: graph capture, first-touch of the logit rows)
                model._prefill(prompts[:B], frames_u8=frames[:B], max_new=T, sampling=samp, processing=proc, **kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids, lens = eng.generate(T, stop_on_eos=False)
                torch.cuda.synchronize()
                if rep:
                    times.append(time.perf_counter() - t0)
            assert int(lens.min()) == T, "a row ended early"
            if aut is not None:   # the rows did move through the automaton
                assert eng.automaton and min(eng.automaton_state(0, B)) >= 0
            ms = 1e3 * float(np.median(times)) / (T - 1)
            print(json.dumps({"batch": B, "mode": mode, "ms_per_step": round(ms, 4), "prompt": P, "new_tokens": T, "reps": args.reps}), flush=True)
    eng.clear_sampling()
    eng.clear_processing()
    if constraints is not None and args.setup_reps > 0:
        setup_costs(model, eng, cfg, args.setup_reps)


def setup_costs(model, eng, cfg, reps):
    """ms per call, median: the host build of the automata, the upload of one, and the same call when the session already holds the object"""
    V = cfg.llm.vocab_size

    def med(fn, prep=None):
        out = []
        for _ in range(reps):
            if prep:
                prep()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return round(1e3 * float(np.median(out)), 4)

    rec = {"vocab": V, "reps": reps}
    rec["build_action_bins_ms"] = med(lambda: constraints.action_bins(V, cfg.n_action_bins, 7, token_vocab=cfg.action_vocab_size))
    rec["build_policy_line_ms"] = med(lambda: constraints.policy_line([29871], V, cfg.n_action_bins, 7, token_vocab=cfg.action_vocab_size))
    rec["cached_action_bins_ms"] = med(lambda: model._bin_automaton(7))
    aut = model._bin_automaton(7)
    rec["set_automaton_upload_ms"] = med(lambda: eng.set_automaton(aut), eng.clear_automaton)
    eng.set_automaton(aut)
    rec["set_automaton_same_object_ms"] = med(lambda: eng.set_automaton(aut))
    rec["set_automaton_starts_ms"] = med(lambda: eng.set_automaton_starts([0]))
    eng.clear_automaton()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
