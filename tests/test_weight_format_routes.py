"""What the decode planner answers per weight format, pinned: tests/golden/decode_routes.json holds, for a set of configs and tuning switches, the
launcher family of every projection stage at 1-64 rows (default and exact numerics), the three decode-batch limits, emmax_model_mxfp4_wide, what
emmax_session_bytes answers at 1 / 17 / 64 rows, and the return code and error text of every create the library refuses.  The file was recorded from the library as it stood BEFORE the weight format
became one value (csrc/kernels.h: WFMT) and is compared entry for entry, texts included; everything here is host-only.

`python tests/test_weight_format_routes.py` rewrites the file from the built library: only for a commit that changes a route or a text on purpose.
"""

import copy
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_stage_ref as R  # noqa: E402
from test_decode_plan import CONFIGS, STAGES, Model, _seven_b  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_routes.json")
SWITCHES = ("", "km=0", "km_down=0")
VIA_CHAR = {R.REFUSED: "-", **{v: str(v) for v in (0, R.KS, R.GEMV, R.GEMV_FP8, R.KM, R.KMP, R.MFMA)}}


def _with(cfg, **llm):
    cfg = copy.deepcopy(cfg)
    for k, v in llm.items():
        setattr(cfg.llm, k, v)
    return cfg


def _cases():
    """name -> (config factory, tuning switches held while the model is created, emmax_config.decode_fp8 forced or None)"""
    cases = {name: (make, {}, None) for name, make in CONFIGS.items()}
    cases["7b-mxfp6"] = (lambda: _seven_b("mxfp6"), {}, None)
    cases["7b-mxfp4-wide"] = (lambda: _seven_b("mxfp4"), {"mx4_wide": 1}, None)
    # creates the library refuses: every shape rule of the block-scaled formats (no bf16 or fp8 shape is refused for its format alone: hidden and
    # n_heads * head_dim are multiples of 128 before the fp8 rule K % 64 is asked), and the codes that are no format
    for fmt in ("mxfp4", "mxfp6"):
        cases[f"refused-{fmt}-hidden"] = (lambda fmt=fmt: _with(_seven_b(fmt), hidden_size=1536), {}, None)
        cases[f"refused-{fmt}-inter"] = (lambda fmt=fmt: _with(_seven_b(fmt), intermediate_size=4096), {}, None)
        cases[f"refused-{fmt}-rows"] = (lambda fmt=fmt: _with(_seven_b(fmt), vocab_size=40000), {}, None)
    cases["refused-code-3"] = (lambda: _seven_b("bf16"), {}, 3)
    cases["refused-code-5"] = (lambda: _seven_b("bf16"), {}, 5)
    return cases


class _Forced(Model):
    """Model with emmax_config.decode_fp8 overwritten after the Python mapping"""

    def __init__(self, so, cfg, code):
        from emmax.engine import _config_c

        self.so, self.h = so, C.c_void_p()
        self.cc = _config_c(cfg)
        self.cc.decode_fp8 = code
        self.rc = so.emmax_model_create(C.byref(self.cc), C.byref(self.h))
        self.err = so.emmax_last_error().decode() if self.rc else ""


def collect(L, so):
    out = {}
    for name, (make, create_sw, code) in _cases().items():
        with L.tuning(**create_sw):
            m = Model(so, make()) if code is None else _Forced(so, make(), code)
        rec = {"create_rc": m.rc, "create_err": m.err, "config_limit": {}, "config_limit_err": {}}
        for exact in (0, 1):
            with L.tuning(**create_sw):
                r = so.emmax_config_max_decode_batch(C.byref(m.cc), exact)
            rec["config_limit"][str(exact)] = r
            rec["config_limit_err"][str(exact)] = so.emmax_last_error().decode() if r < 0 else ""
        if m.rc == 0:
            rec["mxfp4_wide"] = so.emmax_model_mxfp4_wide(m.h)
            rec["switches"] = {}
            for sw in SWITCHES:
                with L.tuning(**{k: int(v) for k, v in (kv.split("=") for kv in sw.split(",") if kv)}):
                    rec["switches"][sw] = {
                        "limit": m.limit(), "limit_exact": m.limit(True),
                        "routes": {f"{st}/{exact}": "".join(VIA_CHAR[m.route(st, B, bool(exact))] for B in range(1, 65))
                                   for st in STAGES for exact in (0, 1)},
                    }
            # what a session of 1 / 17 / 64 rows is told, exact numerics off and on (host only: sizes alone)
            rec["session"] = {}
            for max_batch in (1, 17, 64):
                for exact in (0, 1):
                    ws, kv = C.c_int64(), C.c_int64()
                    with L.tuning(exact=exact):
                        r = so.emmax_session_bytes(m.h, max_batch, 8, 256 + 8 + 64, C.byref(ws), C.byref(kv))
                    rec["session"][f"{max_batch}/{exact}"] = [r, so.emmax_last_error().decode() if r else ""]
        m.close()
        out[name] = rec
    return out


@pytest.fixture(scope="module")
def lib():
    from emmax import _lib

    return _lib, _lib.load()


@pytest.fixture(scope="module")
def recomputed(lib):
    return collect(*lib)


with open(GOLDEN) as _f:
    PINNED = json.load(_f)


def test_the_cases_are_the_recorded_ones(recomputed):
    assert sorted(recomputed) == sorted(PINNED)
    refused = [n for n, r in PINNED.items() if r["create_rc"]]
    assert len(refused) == 8 and all(PINNED[n]["create_err"] for n in refused)   # every refusal carries its text


@pytest.mark.parametrize("name", sorted(PINNED))
def test_routes_limits_and_refusals_are_the_recorded_ones(recomputed, name):
    got, want = recomputed[name], PINNED[name]
    assert {k: v for k, v in got.items() if k != "switches"} == {k: v for k, v in want.items() if k != "switches"}
    for sw, w in want.get("switches", {}).items():
        g = got["switches"][sw]
        assert (g["limit"], g["limit_exact"]) == (w["limit"], w["limit_exact"]), (name, sw)
        for key, row in w["routes"].items():
            assert g["routes"][key] == row, (name, sw, key)


if __name__ == "__main__":
    from emmax import _lib

    with open(GOLDEN, "w") as f:
        json.dump(collect(_lib, _lib.load()), f, indent=1, sort_keys=True)
        f.write("\n")
