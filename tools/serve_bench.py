"""Continuous batching vs static batching on one MI355X (not the headline bench).

Emma-X-7B shapes, margin-boosted synthetic weights whose greedy chain is known a priori: request i emits k_i - 1 ordinary
ids, the 29871 prefix, 8 action ids and EOS, so the natural lengths k_i + 9 are spread like real reasoning chains of
different depth.  Every request = one 224x224 frame + a 32-token prompt.
  static      batches of `slots` requests through generate(); a batch ends when its longest row reaches EOS
  continuous  SlotScheduler: a finished slot is refilled at once
  + early     the same with the stop rule (29871 + 8 ids): EOS is never decoded
Agreement of the emitted ids between the modes is reported per request (see the comment in main).

--samples N: every request is a SAMPLE GROUP (Request.num_samples = N: one prefill, one fork into N slots that read the prompt's KV pages);
--samples N --unforked submits the same work as N independent requests per frame, copy j drawing with the group's seed and subseq j (matched
through the engine: the scheduler itself gives every request subseq 0) -- each copy pays its own vision + prefill and streams its own copy of
the prompt's K/V.  --alternate R runs the two R times in turn in one process (one box, one model build); N may be a comma-separated list.
Reported per run: samples (actions) per second with overlapped and with blocking admission, and from the blocking serve (where admissions sit
on the decode stream and can be timed) the admission work per group (frame encode + prefill + fork) and the time per decode step."""
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
from emmax.serving import Request, SlotScheduler
from emmax.weights import planted_chain, planted_start_token


class _Timed:
    """The engine behind a scheduler, with two things added.  Subseqs: the j-th request admitted with a seed draws with subseq j % copies (the
    unforked baseline submits the copies of a frame in order, and admission is FIFO).  Times: device-synchronised seconds spent in admission
    calls and in decode steps (meaningful with blocking admission, where both sit on the decode stream)."""

    ADMISSION = ("slot_prefill", "slots_prefill", "slots_fork", "vision_encode")

    def __init__(self, eng, copies=1, timed=False):
        self._eng, self._copies, self._timed, self._seen = eng, copies, timed, {}
        self.t_admission = self.t_steps = 0.0

    def _subseqs(self, seeds):
        out = []
        for sd in seeds:
            out.append(self._seen.get(sd, 0) % self._copies)
            self._seen[sd] = self._seen.get(sd, 0) + 1
        return out

    def set_sampling(self, params, seeds=None, subseqs=None, **kw):
        return self._eng.set_sampling(params, seeds, self._subseqs(seeds) if self._copies > 1 else subseqs, **kw)

    def set_sampling_staged(self, params, seeds=None, subseqs=None, **kw):
        return self._eng.set_sampling_staged(params, seeds, self._subseqs(seeds) if self._copies > 1 else subseqs, **kw)

    def __getattr__(self, name):
        fn = getattr(self._eng, name)
        if not self._timed or (name not in self.ADMISSION and name != "slots_step"):
            return fn

        def timed(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if name == "slots_step":
                self.t_steps += dt
            else:
                self.t_admission += dt
            return out

        return timed


def bench_samples(args, model, cfg, dev, n_samples):
    """--samples: `requests` frames, each served as a group of n_samples (forked) or as n_samples independent requests (unforked)."""
    from emmax.sampling import SamplingParams

    eng = model.engine
    rng = np.random.default_rng(3)
    G = args.requests
    ks = [int(k) for k in rng.integers(16, 96, size=G)]
    frames = torch.from_numpy(rng.integers(0, 256, size=(G, 224, 224, 3), dtype=np.uint8)).to(dev)
    rows = []
    for k in ks:
        r = [1] + [int(x) for x in rng.integers(3, 31744, size=31)]
        r[-1] = planted_start_token(cfg, k)
        rows.append(r)
    BUDGET = 128

    def serve(forked, overlap, timed):
        proxy = _Timed(eng, copies=1 if forked else n_samples, timed=timed)

        def encode(fs):
            pe = proxy.vision_encode(torch.stack(fs))
            return [pe[i] for i in range(len(fs))]

        sch = SlotScheduler(proxy, encode, n_slots=args.slots, poll_every=args.poll, encode_ahead=0 if timed else args.slots, overlap=overlap)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(G):
            p = SamplingParams(1.0, 0, 1.0, seed=1000 + i)
            if forked:   # (N = 1 is a plain request: the same call a build without sample groups takes)
                sch.submit(Request(i, frames[i], rows[i], BUDGET, sampling=p, **({"num_samples": n_samples} if n_samples > 1 else {})))
            else:
                for j in range(n_samples):
                    sch.submit(Request((i, j), frames[i], rows[i], BUDGET, sampling=p))
        res = sch.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ids = {((r.rid, getattr(r, "sample", 0)) if forked else r.rid): r.ids for r in res}
        return dt, ids, sch, proxy

    serve(True, True, False); serve(False, False, False)   # warm-up of both admission paths and both modes
    modes = [not args.unforked] if not args.alternate else [True, False] * args.alternate
    runs, ids_by_mode = [], {}
    for forked in modes:
        t_over, ids_o, sch_o, _ = serve(forked, True, False)
        t_block, ids_b, sch_b, px = serve(forked, False, True)
        ids_by_mode[forked] = ids_b
        runs.append({"mode": "forked" if forked else "unforked", "samples": n_samples, "groups": G, "slots": args.slots,
                     "actions_per_s_overlapped": round(G * n_samples / t_over, 2), "actions_per_s_blocking": round(G * n_samples / t_block, 2),
                     "admission_ms_per_group": round(1e3 * px.t_admission / G, 3), "ms_per_step": round(1e3 * px.t_steps / sch_b.steps, 4),
                     "decode_steps_blocking": sch_b.steps, "decode_steps_overlapped": sch_o.steps,
                     "tokens": sum(len(v) for v in ids_b.values()),
                     "overlapped_vs_blocking_identical": sum(int(ids_o[k] == ids_b[k]) for k in ids_b)})
    out = {"model": "tiny" if args.tiny else "Emma-X-7B shapes (planted synthetic weights)", "runs": runs}
    if len(ids_by_mode) == 2:   # reported, not asserted, as below: at this size near-ties flip between differently batched prefills
        out["samples_with_identical_ids_forked_vs_unforked"] = {"same": sum(int(ids_by_mode[True][k] == ids_by_mode[False][k]) for k in ids_by_mode[True]),
                                                                "of": len(ids_by_mode[True])}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--poll", type=int, default=4, help="decode steps between two device polls")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--samples", type=str, default="", help="N (or N1,N2,...): every request is a sample group of N (Request.num_samples)")
    ap.add_argument("--unforked", action="store_true", help="with --samples: the same work as N independent requests per frame (the baseline)")
    ap.add_argument("--alternate", type=int, default=0, help="with --samples: run forked and unforked this many times in turn")
    ap.add_argument("--weights", default="", help="decode_weight_dtype (bf16 / fp8 / mxfp4; default: the config's); mxfp4 with more than 16 slots is created wide")
    args = ap.parse_args()
    cfg = EmmaXConfig.tiny() if args.tiny else EmmaXConfig.emma_x_7b()
    dev = "cuda:0"
    wide = {"mxfp4_wide": True} if args.weights == "mxfp4" and args.slots > 16 else {}
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=5, device=dev, planted=True, decode_weight_dtype=args.weights or None, max_batch=args.slots,
                                                    max_prompt=64, max_ctx=1024, **wide)
    eng = model.engine
    if args.samples:
        for n in [int(v) for v in args.samples.split(",")]:
            bench_samples(args, model, cfg, dev, n)
        return
    rng = np.random.default_rng(3)
    N = args.requests
    ks = [int(k) for k in rng.integers(16, 480, size=N)]
    frames = torch.from_numpy(rng.integers(0, 256, size=(N, 224, 224, 3), dtype=np.uint8)).to(dev)
    rows = []
    for k in ks:
        r = [1] + [int(x) for x in rng.integers(3, 31744, size=31)]
        r[-1] = planted_start_token(cfg, k)
        rows.append(r)
    MAXN = 512
    # reference answers: every request alone (bs = 1); the planted chain is the a-priori answer while its margin holds
    want, n_chain = [], 0
    for i in range(N):
        ids, lens = model.generate_ids(rows[i:i + 1], frames_u8=frames[i:i + 1], max_new_tokens=MAXN)
        want.append(ids[0, : int(lens[0])].cpu().tolist())
        n_chain += int(want[-1] == planted_chain(cfg, rows[i][-1], 600))

    def sync():
        torch.cuda.synchronize()

    # ---- static batches
    sync(); t0 = time.perf_counter()
    got_static, lat_static = [], []
    for i in range(0, N, args.slots):
        ids, lens = model.generate_ids(rows[i:i + args.slots], frames_u8=frames[i:i + args.slots], max_new_tokens=MAXN)
        ids, lens = ids.cpu(), lens.cpu().tolist()
        t = time.perf_counter() - t0
        for b in range(len(lens)):
            got_static.append(ids[b, : lens[b]].tolist())
            lat_static.append(t)
    t_static = time.perf_counter() - t0

    def encode(fs):
        pe = eng.vision_encode(torch.stack(fs))
        return [pe[i] for i in range(len(fs))]

    def serve(trigger, after, overlap=True):
        sch = SlotScheduler(eng, encode, n_slots=args.slots, poll_every=args.poll, stop_trigger=trigger, stop_after=after,
                            encode_ahead=args.slots, overlap=overlap)
        sync(); t0 = time.perf_counter()
        for i in range(N):
            sch.submit(Request(i, frames[i], rows[i], MAXN))
        res = sch.run()
        sync()
        dt = time.perf_counter() - t0
        eng.set_stop([], 0)
        return dt, {r.rid: r for r in res}, sch

    serve([], 0)                                        # warm-up of both admission paths (allocator, first launches)
    t_block, res_block, sch_b = serve([], 0, overlap=False)   # round-3 behaviour: admissions on the decode stream
    t_cont, res_cont, sch_c = serve([], 0)
    t_early, res_early, sch_e = serve([29871], 8)
    # Agreement between the serving modes is REPORTED, not asserted, at this size: the launch plan picks tile geometry and
    # split-K factor from the problem size, so a frame encoded / prefilled alone and the same frame inside a batch of 8 see
    # different fp32 summation orders, and these synthetic weights keep their top-1 margin for ~80 steps only -- a near-tie
    # flips now and then (hundreds of steps x 32 requests).  The bit-exact comparison of a slot-served request with its own
    # bs = 1 run is the tiny-config GPU test (tests/test_serving_gpu.py), where the margins are wide.
    def cut_at_stop(ids):
        full = ids[:-1] if ids and ids[-1] == cfg.eos_token_id else ids
        return full[: next((t + 9 for t, v in enumerate(full) if v == 29871 and t + 9 <= len(full)), len(full))]

    assert sorted(res_cont) == list(range(N)) and sorted(res_early) == list(range(N))
    same_bs1_static = sum(int(got_static[i] == want[i]) for i in range(N))
    same_bs1_cont = sum(int(res_cont[i].ids == want[i]) for i in range(N))
    same_static_cont = sum(int(res_cont[i].ids == got_static[i]) for i in range(N))
    early_prefix = sum(int(res_early[i].ids == cut_at_stop(res_cont[i].ids)) for i in range(N))

    def pct(v, q):
        return float(np.percentile(np.asarray(v), q))

    lb = [res_block[i].latency_s for i in range(N)]
    lc = [res_cont[i].latency_s for i in range(N)]
    le = [res_early[i].latency_s for i in range(N)]
    out = {
        "model": "tiny" if args.tiny else "Emma-X-7B shapes (planted synthetic weights)", "weights": cfg.decode_weight_dtype, "requests": N, "slots": args.slots, "poll_every": args.poll,
        "new_tokens_to_eos": {"min": min(len(w) for w in want), "mean": float(np.mean([len(w) for w in want])), "max": max(len(w) for w in want)},
        "requests_following_the_planted_chain": n_chain,
        "static": {"seconds": round(t_static, 3), "actions_per_s": round(N / t_static, 3), "latency_p50_s": round(pct(lat_static, 50), 3),
                   "latency_p95_s": round(pct(lat_static, 95), 3)},
        "continuous_blocking_admission": {"seconds": round(t_block, 3), "actions_per_s": round(N / t_block, 3), "latency_p50_s": round(pct(lb, 50), 3),
                                          "latency_p95_s": round(pct(lb, 95), 3), "decode_steps": sch_b.steps},
        "continuous": {"admission": "overlapped (staging rows, second stream)", "overlapped_admissions": sch_c.overlapped_admissions, "seconds": round(t_cont, 3), "actions_per_s": round(N / t_cont, 3), "latency_p50_s": round(pct(lc, 50), 3),
                       "latency_p95_s": round(pct(lc, 95), 3), "decode_steps": sch_c.steps, "polls": sch_c.polls},
        "continuous_early_exit": {"seconds": round(t_early, 3), "actions_per_s": round(N / t_early, 3), "latency_p50_s": round(pct(le, 50), 3),
                                  "latency_p95_s": round(pct(le, 95), 3), "decode_steps": sch_e.steps},
        "requests_with_identical_ids": {"static_vs_bs1": same_bs1_static, "continuous_vs_bs1": same_bs1_cont,
                                        "continuous_vs_static": same_static_cont,
                                        "overlapped_vs_blocking_admission": sum(int(res_cont[i].ids == res_block[i].ids) for i in range(N)), "early_exit_is_prefix_of_continuous": early_prefix, "of": N},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
