"""Decode step time and per-launch projection times of the four decode weight formats (bf16, fp8-e4m3, MXFP4, MXFP6) on ONE box, back to back
(not the headline bench): the synthetic 7B model, 512-token prompts over one frame each (context 768), batches 1 / 8 / 16 by default (`--batches 16,32,64`: the MXFP4 model is then created wide -- mxfp4_wide=True, decode_kmp.hip's MX4
form at 17-64 rows -- which leaves its 1-16-row kernels as they are; an MXFP6 model stops at 16 rows and sits those batches out).  The models are
built once and kept; every (format, batch) point is measured `--rounds` times with the formats alternating inside a round, so that a drift of
the box shows up as spread between rounds and not as a difference between formats.

  ms/step      emmax_generate over `--steps` greedy steps (EOS ignored), host clock around a device synchronise, the bench's method;
  us/launch    emmax_profile_decode_stage: HIP events around one launch per layer (every launch streams another layer's weights).

usage: python tools/wfmt_bench.py [--formats bf16,fp8,mxfp4,mxfp6] [--batches 1,8,16] [--rounds 3] [--steps 64] [--out FILE]"""
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

STAGES = ["qkv", "attn", "oproj", "gateup", "down", "lmhead"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="bf16,fp8,mxfp4,mxfp6")
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    formats = args.formats.split(",")
    batches = [int(b) for b in args.batches.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("wfmt_bench needs a HIP device")
    rng = np.random.default_rng(0)
    bmax = max(batches)
    frames = torch.from_numpy(rng.integers(0, 256, size=(bmax, 224, 224, 3), dtype=np.uint8)).cuda()
    prompts = [[1] + [int(x) for x in rng.integers(3, 31744, size=511)] for _ in range(bmax)]
    models, info = {}, {}
    for f in formats:
        t0 = time.perf_counter()
        wide = {"mxfp4_wide": True} if f == "mxfp4" and bmax > 16 else {}   # (opt-in: a narrow MXFP4 model stops at 16 rows)
        cap = min(bmax, 16) if f == "mxfp6" else bmax   # (MXFP6 tiles: 1-16 rows; larger batches are skipped for it below)
        m = EmmaXForActionPrediction.from_synthetic(EmmaXConfig.emma_x_7b(), seed=0, device="cuda:0", decode_weight_dtype=f, max_batch=cap,
                                                    max_prompt=512, max_ctx=256 + 512 + args.steps + 64, **wide)
        m.engine.ensure_decode_batch(cap)
        torch.cuda.synchronize()
        models[f] = m
        info[f] = {"weight_bytes": m.engine.weight_bytes(), "max_decode_batch": m.engine.max_decode_batch(), "mxfp4_wide": bool(m.engine.mxfp4_wide), "build_s": round(time.perf_counter() - t0, 1)}
        print(f"# {f}: {json.dumps(info[f])}", flush=True)
    rows = []
    for B in batches:
        for rnd in range(args.rounds + 1):   # round 0 warms every (format, batch) shape and is dropped
            for f in formats:
                m, eng = models[f], models[f].engine
                if B > info[f]["max_decode_batch"]:
                    continue
                m._prefill(prompts[:B], None, frames[:B].contiguous(), max_new=args.steps + 2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.generate(args.steps + 1, False)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / args.steps * 1e3
                m._prefill(prompts[:B], None, frames[:B].contiguous(), max_new=args.steps + 2)
                us = {n: round(eng.profile_decode_stage(i, reps=3), 2) for i, n in enumerate(STAGES)}
                if rnd:
                    rows.append({"format": f, "batch": B, "round": rnd, "ms_per_step": round(ms, 4), "us_per_launch": us})
                    print(json.dumps(rows[-1]), flush=True)
    # summary: median over the rounds
    summary = []
    for B in batches:
        for f in formats:
            sel = [r for r in rows if r["format"] == f and r["batch"] == B]
            if not sel:
                continue
            ms = sorted(r["ms_per_step"] for r in sel)
            summary.append({"format": f, "batch": B, "ms_per_step_median": ms[len(ms) // 2], "ms_per_step_min": ms[0], "ms_per_step_max": ms[-1],
                            "us_per_launch_median": {n: sorted(r["us_per_launch"][n] for r in sel)[len(sel) // 2] for n in STAGES}})
            print("# " + json.dumps(summary[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"models": info, "rows": rows, "summary": summary, "device": torch.cuda.get_device_name(0)}, fh, indent=1)


if __name__ == "__main__":
    main()
