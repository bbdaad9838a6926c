"""Host cost of the decode planner: ns per emmax_op_decode_route call (one stage's route = what launch_proj adds to a launch, plus the
shape's set-up) and per emmax_model_max_decode_batch call (what a prefill / emmax_generate / emmax_slots_open pays once).  Host only: no GPU.

    python tools/route_cost.py [calls]
"""
import copy
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd")]

from emmax import _lib  # noqa: E402
from emmax.config import EmmaXConfig  # noqa: E402
from emmax.engine import _config_c  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    so = _lib.load()
    for fmt in ("bf16", "fp8", "mxfp4"):
        cfg = copy.deepcopy(EmmaXConfig.emma_x_7b())
        cfg.decode_weight_dtype = fmt
        h, cc = C.c_void_p(), _config_c(cfg)
        _lib.check(so.emmax_model_create(C.byref(cc), C.byref(h)), "emmax_model_create")
        via = C.c_int(0)
        route = so.emmax_op_decode_route
        for B in (1, 8):
            for stage, name in ((0, "qkv"), (2, "o-proj"), (3, "gate/up"), (4, "down"), (5, "lm-head")):
                t0 = time.perf_counter_ns()
                for _ in range(n):
                    route(h, stage, B, 0, C.byref(via))
                dt = (time.perf_counter_ns() - t0) / n
                t0 = time.perf_counter_ns()
                for _ in range(n):
                    so.emmax_abi_version()
                base = (time.perf_counter_ns() - t0) / n
                print(f"{fmt} B={B} {name}: via {via.value}, {dt:.0f} ns per call through ctypes, {base:.0f} ns of that the ctypes call itself "
                      f"(emmax_abi_version) -> ~{max(dt - base, 0):.0f} ns for the route")
        t0 = time.perf_counter_ns()
        for _ in range(200):
            lim = so.emmax_model_max_decode_batch(h)
        print(f"{fmt}: emmax_model_max_decode_batch = {lim}, {(time.perf_counter_ns() - t0) / 200 / 1000:.1f} us per call")
        so.emmax_model_destroy(h)


if __name__ == "__main__":
    main()
