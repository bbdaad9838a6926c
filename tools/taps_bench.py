"""What the taps (output_hidden_states / output_attentions) cost, on one MI355X (not the headline bench).

Emma-X-7B shapes, synthetic weights, a text prompt of 768 ids per row (the flagship's 256 patch rows + 512 ids as rows of a vision-less prefill),
B in {1, 8}.  Per B a prefill and a decode step (emmax_set_current_tokens + emmax_decode_step, the single-step form of the step taps), each in
four modes that ALTERNATE in one process -- round r runs every mode once, `--reps` rounds, median reported:
  none     nothing bound                      last     the normed last hidden state only
  hidden   all n_layers + 1 hidden states     map      one layer's attention map (layer n_layers - 1)
and the probability launch alone (emmax_op_attn_probs over a synthetic cache, the prefill's shape and the step's) against the bytes it stores:
kernel time from the profiler's kernel records where it has them, else the op call between two events (an upper bound: the op reads its lengths
back first), with the fraction of the spec sheet's 8 TB/s.
`--unbound-only --lib PATH`: the `none` column alone on the library at PATH (the parent's build): a job script alternates processes on the two
builds for the claim that a session that binds nothing runs the parent's passes.
`--lib-b PATH`: the probability kernel's stores, non-temporal (the product) against plain (`make -C emma-x_amd/csrc plain-stores` builds
emma-x_amd/emmax/libemmax_hip_plain_stores.so, which differs in that one store): both libraries in one process, five alternating rounds of ten launches.
Writes profiles/taps_bench.txt (or --out; appends with --append)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd")]
import torch

CTX, STEPS = 768, 16
MODES = ("none", "last", "hidden", "map")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def probs_alone(lib, _lib, B, n, base, Hq, Hkv, dev, reps=10):
    """(us per launch, how, bytes stored) of emmax_op_attn_probs: B sequences of n new rows over base cached keys, ld_keys = base + n"""
    pages = -(-(base + n) // 64)
    g = torch.Generator(device="cpu").manual_seed(1)
    q = torch.randn(B * n, Hq * 128, generator=g).to(torch.bfloat16).to(dev)
    ld = (base + n + 3) // 4 * 4
    out = torch.empty(B * n, Hq, ld, dtype=torch.float32, device=dev)
    cu = torch.arange(0, B * n + 1, n, dtype=torch.int32, device=dev)
    bs = torch.full((B,), base, dtype=torch.int32, device=dev)
    table = torch.randperm(B * pages, generator=g).view(B, pages).to(torch.int32).to(dev)
    kc = torch.randn((B * pages, Hkv, 64, 128), device=dev).to(torch.bfloat16)
    st = _lib.current_stream()
    call = lambda: lib.emmax_op_attn_probs(q.data_ptr(), Hq * 128, 0, kc.data_ptr(), table.data_ptr(), cu.data_ptr(), bs.data_ptr(), B, B * n, Hq, Hkv, 64, pages,
                                           128 ** -0.5, out.data_ptr(), ld, st)
    for _ in range(3):
        _lib.check(call(), "attn probs")
    nbytes = out.numel() * 4
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        us = sum(float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0))) / reps for e in prof.key_averages() if "emmax_attn_probs" in e.key)
        if us > 0.0:
            return us, "kernel records", nbytes
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
    return statistics.median(ts), "op call between events (upper bound)", nbytes


def stores_ab(path_b, _lib, dev, out_path, append):
    """this build's emmax_op_attn_probs against the one of the library at path_b, alternating"""
    import ctypes

    a = _lib.load()
    b = ctypes.CDLL(os.path.abspath(path_b))
    b.emmax_op_attn_probs.restype, b.emmax_op_attn_probs.argtypes = _lib.SIGNATURES["emmax_op_attn_probs"]
    lines = [f"emmax_attn_probs_kernel, this build (A) against {os.path.basename(path_b)} (B) (Hq = Hkv = 32, bf16 cache; sequences, new rows, cached keys):"]
    for B, n, base in ((1, CTX, 0), (8, CTX, 0), (8, 128, CTX), (8, 1, CTX)):
        res = {"A": [], "B": []}
        for _ in range(5):
            for tag, lib in (("A", a), ("B", b)):
                us, how, nb = probs_alone(lib, _lib, B, n, base, 32, 32, dev)
                res[tag].append(us)
        p, q = statistics.median(res["A"]), statistics.median(res["B"])
        lines.append(f"B {B} n {n:4d} base {base:4d} | {nb / 1e6:8.2f} MB | A {p:8.1f} us {nb / p / 1e3:7.1f} GB/s | B {q:8.1f} us {nb / q / 1e3:7.1f} GB/s | A / B {p / q:.3f} "
                     f"({how}; rounds: A {min(res['A']):.1f}-{max(res['A']):.1f}, B {min(res['B']):.1f}-{max(res['B']):.1f})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a" if append else "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the tiny config (a dry run of the tool, not a measurement)")
    ap.add_argument("--lib", default=None, help="another build of libemmax_hip.so to load (the parent's)")
    ap.add_argument("--lib-b", default=None, help="only the probability launch: this build against the library at this path, alternating")
    ap.add_argument("--unbound-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--tag", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taps_bench.txt"))
    args = ap.parse_args()
    from emmax import _lib

    if args.lib_b:
        return stores_ab(args.lib_b, _lib, "cuda:0", args.out, args.append)
    if args.lib:   # (an older build exports fewer symbols: the binding attaches what it finds there)
        import ctypes

        _lib.LIB_PATH = os.path.abspath(args.lib)
        old = ctypes.CDLL(_lib.LIB_PATH)
        for name in [k for k in _lib.SIGNATURES if not hasattr(old, k)]:
            _lib.SIGNATURES.pop(name)
    from emmax import taps as T
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction

    dev = "cuda:0"
    cfg = EmmaXConfig.tiny(gqa=True) if args.tiny else EmmaXConfig.emma_x_7b()
    BS = (1, 3) if args.tiny else (1, 8)
    model = EmmaXForActionPrediction.from_synthetic(cfg, seed=5, device=dev, max_batch=max(BS), max_prompt=CTX, max_ctx=cfg.n_patches + CTX + STEPS + 64)
    eng, lib = model.engine, model.engine.lib
    eng.ensure_decode_batch(max(BS))
    nl, Hq, Hkv, V = cfg.llm.num_layers, cfg.llm.num_heads, cfg.llm.num_kv_heads, cfg.llm.vocab_size
    specs = {"none": None, "last": T.TapSpec([nl], []), "hidden": T.TapSpec(list(range(nl + 1)), []), "map": T.TapSpec([], [nl - 1])}
    modes = ("none",) if args.unbound_only else MODES
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, min(V, 31744), (max(BS), CTX), generator=g).tolist()
    toks = torch.randint(3, min(V, 31744), (STEPS, max(BS)), generator=g, dtype=torch.int32).to(dev)
    st = _lib.current_stream()
    lines = [f"taps_bench [{args.tag}]: {'tiny' if args.tiny else 'Emma-X-7B shapes'}, prompt {CTX} rows, median of {args.reps} alternating rounds; prefill ms, decode step us "
             f"(mean of {STEPS} steps)", "pass     B | " + " ".join(f"{m:>10s}" for m in modes) + " | over none: " + " ".join(f"{m:>7s}" for m in modes[1:])]
    for B in BS:
        rows = [r[:CTX] for r in ids[:B]]
        tp = {m: [] for m in modes}
        ts = {m: [] for m in modes}
        for r in range(args.reps + 1):   # (the first round warms up)
            for m in modes:
                def prefill():
                    if specs[m] is not None:
                        eng.bind_pass_taps(specs[m], B * CTX, CTX)
                    eng.prefill(rows, None)

                tp[m].append(wall(prefill))

                def steps():
                    for t in range(STEPS):
                        _lib.check(lib.emmax_set_current_tokens(eng._session, toks[t].data_ptr(), st), "emmax_set_current_tokens")
                        _lib.check(lib.emmax_decode_step(eng._session, st), "emmax_decode_step")

                if specs[m] is not None:
                    eng.bind_step_taps(specs[m], 1, CTX + STEPS + 1)
                ts[m].append(wall(steps) * 1e3 / STEPS)
                if specs[m] is not None:
                    eng.clear_taps()
        for name, t, unit in (("prefill", tp, "ms"), ("step", ts, "us")):
            med = {m: statistics.median(t[m][1:]) for m in modes}
            lines.append(f"{name:8s} {B:1d} | " + " ".join(f"{med[m]:10.3f}" for m in modes) + " |            " + " ".join(f"{med[m] / med['none']:7.3f}" for m in modes[1:]))
            print(lines[-1], flush=True)
    if not args.unbound_only:
        lines.append("the probability launch alone (bf16 cache): B, new rows, cached keys | us | MB stored | GB/s | % of 8 TB/s (how)")
        for B, n, base in ((1, CTX, 0), (8, CTX, 0), (1, 1, CTX), (8, 1, CTX)) if not args.tiny else ((1, 40, 0), (3, 1, 40)):
            us, how, nb = probs_alone(lib, _lib, B, n, base, Hq, Hkv, dev)
            gbs = nb / (us * 1e-6) / 1e9
            lines.append(f"  B {B} n {n:4d} base {base:4d} | {us:9.1f} | {nb / 1e6:9.2f} | {gbs:8.1f} | {100.0 * gbs / 8000.0:5.1f} ({how})")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
