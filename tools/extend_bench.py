"""Extending a cached context against the two ways the parent pays for it, on one MI355X (not the headline bench).

Emma-X-7B shapes, synthetic weights, a cached context of 768 tokens per row; n new tokens per row, n in {8, 32, 128}, B in {1, 8} rows, bf16 KV
cache and kv_fp8.  Three things alternate in one process (one box, one model build), `--reps` times each, median reported:
  (a) extend      emmax_extend: one pass over the B x n new rows, attention over the paged cache
  (b) steps       n teacher-forced decode steps (emmax_set_current_tokens + emmax_decode_step): the weights stream n times
  (c) re-prefill  a vision-less emmax_prefill_text of all 768 + n tokens
(a) and (b) start from a fresh 768-token prefill that is not timed.  Also reported per point: the planner's split choice
(emmax_extend_attn_plan) and the extension attention launch alone at these shapes -- kernel time from the profiler's kernel records where it
has them, else the op call between two events (an upper bound: the op reads its lengths back before it launches) -- with the achieved bytes/s
of the K / V it reads against the 8 TB/s of the spec sheet.  Writes profiles/extend_bench.txt (or --out)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd")]
import torch

from emmax import _lib
from emmax.config import EmmaXConfig
from emmax.modeling import EmmaXForActionPrediction

CTX = 768
NS, BS = (8, 32, 128), (1, 8)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def plan(lib, B, n, Hq, Hkv, kv8):
    o = [C.c_int(0) for _ in range(5)]
    _lib.check(lib.emmax_extend_attn_plan(B, n, CTX + n, Hq, Hkv, 0, kv8, *[C.byref(x) for x in o]), "emmax_extend_attn_plan")
    return [x.value for x in o]


def attention_alone(lib, B, n, Hq, Hkv, kv8, dev, reps=20):
    """the extension attention launch at these shapes over a synthetic cache: (us per launch, how it was measured, K / V bytes read)"""
    pages = -(-(CTX + n) // 64)
    g = torch.Generator(device="cpu").manual_seed(1)
    q = torch.randn(B * n, Hq * 128, generator=g).to(torch.bfloat16).to(dev)
    out = torch.empty_like(q)
    cu = torch.arange(0, B * n + 1, n, dtype=torch.int32, device=dev)
    base = torch.full((B,), CTX, dtype=torch.int32, device=dev)
    table = torch.randperm(B * pages, generator=g).view(B, pages).to(torch.int32).to(dev)
    shape = (B * pages, Hkv, 64, 128)
    ws = torch.empty(B * n * Hq * 16 * 132, dtype=torch.float32, device=dev)
    st = _lib.current_stream()
    if kv8:
        kc = torch.randint(0, 120, shape, dtype=torch.uint8, device=dev)
        vc = torch.randint(0, 120, shape, dtype=torch.uint8, device=dev)
        ks = torch.ones(shape[:3], dtype=torch.float32, device=dev)
        call = lambda: lib.emmax_op_extend_attention_kv8(q.data_ptr(), Hq * 128, 0, kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), ks.data_ptr(), table.data_ptr(),
                                                         cu.data_ptr(), base.data_ptr(), B, B * n, Hq, Hkv, 64, pages, 0, 128 ** -0.5, out.data_ptr(), Hq * 128,
                                                         ws.data_ptr(), ws.numel(), None, st)
    else:
        kc = torch.randn(shape, device=dev).to(torch.bfloat16)
        vc = torch.randn(shape, device=dev).to(torch.bfloat16)
        call = lambda: lib.emmax_op_extend_attention(q.data_ptr(), Hq * 128, 0, kc.data_ptr(), vc.data_ptr(), table.data_ptr(), cu.data_ptr(), base.data_ptr(), B,
                                                     B * n, Hq, Hkv, 64, pages, 0, 128 ** -0.5, out.data_ptr(), Hq * 128, ws.data_ptr(), ws.numel(), None, st)
    for _ in range(3):
        _lib.check(call(), "extend attention")
    kv_bytes = B * Hkv * (CTX + n) * 128 * 2 * (1 if kv8 else 2) + (B * Hkv * (CTX + n) * 8 if kv8 else 0)   # every key and value row once (+ scales)
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        us = 0.0
        for e in prof.key_averages():
            if "emmax_extend_attn" in e.key:   # the attention launch and, in the split form, its merge pass
                us += float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0))) / reps
        if us > 0.0:
            return us, "kernel records", kv_bytes
    except Exception:
        pass
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), "op call between events (upper bound)", kv_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="the tiny config (a dry run of the tool, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_bench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = EmmaXConfig.tiny() if args.tiny else EmmaXConfig.emma_x_7b()
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=5, device=dev, max_batch=max(BS), max_prompt=CTX + max(NS), max_ctx=cfg.n_patches + CTX + max(NS) + 16)
    eng, lib = model.engine, model.engine.lib
    eng.ensure_decode_batch(max(BS))
    Hq, Hkv, V = cfg.llm.num_heads, cfg.llm.num_kv_heads, cfg.llm.vocab_size
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, min(V, 31744), (max(BS), CTX + max(NS)), generator=g).tolist()
    lines = [f"extend_bench: {'tiny' if args.tiny else 'Emma-X-7B shapes'}, context {CTX}, median of {args.reps} alternating runs, ms",
             "kv    B    n | (a) extend  (b) n steps  (c) re-prefill | (a)/(b)  (a)/(c) | splits | attention alone: us, GB/s of K/V read, % of 8 TB/s (how)"]
    ok = True
    for kv8 in (0, 1):
        with _lib.tuning(kv_fp8=kv8):
            eng.new_session(max(BS), CTX + max(NS), cfg.n_patches + CTX + max(NS) + 16)
        for B in BS:
            for n in NS:
                ctx_rows, new_rows = [r[:CTX] for r in ids[:B]], [r[CTX:CTX + n] for r in ids[:B]]
                toks = torch.tensor(new_rows, dtype=torch.int32).t().contiguous().to(dev)   # [n, B]
                st = _lib.current_stream()

                def steps():
                    for t in range(n):
                        _lib.check(lib.emmax_set_current_tokens(eng._session, toks[t].data_ptr(), st), "emmax_set_current_tokens")
                        _lib.check(lib.emmax_decode_step(eng._session, st), "emmax_decode_step")

                ta, tb, tc = [], [], []
                for _ in range(args.reps + 1):   # (the first round warms up: graph capture, plans)
                    eng.prefill(ctx_rows, None)
                    ta.append(wall(lambda: eng.extend(new_rows, max_new_tokens=1)))
                    eng.prefill(ctx_rows, None)
                    tb.append(wall(steps))
                    tc.append(wall(lambda: eng.prefill([r[:CTX + n] for r in ids[:B]], None)))
                a, b, c = (statistics.median(t[1:]) for t in (ta, tb, tc))
                ok = ok and a < b
                p = plan(lib, B, n, Hq, Hkv, kv8)
                us, how, kvb = attention_alone(lib, B, n, Hq, Hkv, kv8, dev)
                gbs = kvb / (us * 1e-6) / 1e9
                lines.append(f"{'fp8 ' if kv8 else 'bf16'} {B:3d} {n:4d} | {a:10.3f} {b:12.3f} {c:14.3f} | {a / b:7.3f} {a / c:8.3f} | {p[3]:6d} | "
                             f"{us:8.1f} {gbs:8.1f} {100.0 * gbs / 8000.0:5.1f} ({how})")
                print(lines[-1], flush=True)
    lines.append(f"(a) < (b) at every measured point: {'yes' if ok else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
