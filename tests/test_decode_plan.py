"""The decode planner on the CPU: emmax_model_max_decode_batch (+ _exact) and emmax_op_decode_route are host-only and ask the launcher families'
own shape checks (csrc/kernels.h: ProjShape, <family>_takes; step.hip: proj_route, model_max_decode_batch), so everything here runs on a model
that was only created.
  1. PINNED: the limits the library gave BEFORE the planner existed (hand-written predicates on the model dimensions), recorded on that commit.  The
     planner reproduces them, except the one entry commented below, where the old predicate promised what launch_proj itself refuses.
  2. the routing table of tests/decode_stage_ref.py (what tests/test_decode_stages_gpu.py asserts against real launches) from the pure route.
  3. limit == route, over a grid of shapes; check_config accepts an MXFP4 config exactly when its limit is >= 8.
  4. the two recorded drift cases.
"""

import copy
import ctypes as C
import itertools

import pytest

import decode_stage_ref as R
import mxfp4_ref as M

STAGES = (R.QKV, R.OPROJ, R.GATEUP, R.DOWN, R.LMHEAD)
EXACT_B = (1, 2, 3, 8, 9, 64)
NP_7B = 256   # patches of a frame: max_ctx below leaves room for them at every config


@pytest.fixture(scope="module")
def lib():
    from emmax import _lib

    return _lib, _lib.load()


def _seven_b(fmt, kv=None):
    from emmax.config import EmmaXConfig

    cfg = copy.deepcopy(EmmaXConfig.emma_x_7b())
    cfg.decode_weight_dtype = fmt
    if kv:
        cfg.llm.num_kv_heads = kv
    return cfg


def _tiny():
    from emmax.config import EmmaXConfig

    return EmmaXConfig.tiny()


CONFIGS = {
    "7b-bf16": lambda: _seven_b("bf16"), "7b-fp8": lambda: _seven_b("fp8"), "7b-mxfp4": lambda: _seven_b("mxfp4"), "tiny": _tiny,
    "G": lambda: R.make_cfg("G"), "G8": lambda: R.make_cfg("G", True), "W": lambda: R.make_cfg("W"), "W8": lambda: R.make_cfg("W", True),
    "H": lambda: R.make_cfg("H"), "H8": lambda: R.make_cfg("H", True), "G4": lambda: M.make_cfg4("G4"), "W4": lambda: M.make_cfg4("W4"),
    "7b-gqa8": lambda: _seven_b("bf16", 8),   # LLaMA-2-7B shapes with 8 kv heads
}


class Model:
    """a created (never finalized) model: all the planner needs"""

    def __init__(self, so, cfg):
        from emmax.engine import _config_c

        self.so, self.h = so, C.c_void_p()
        self.cc = _config_c(cfg)
        self.rc = so.emmax_model_create(C.byref(self.cc), C.byref(self.h))
        self.err = so.emmax_last_error().decode() if self.rc else ""

    def close(self):
        if self.rc == 0:
            self.so.emmax_model_destroy(self.h)

    def limit(self, exact=False):
        return (self.so.emmax_model_max_decode_batch_exact if exact else self.so.emmax_model_max_decode_batch)(self.h)

    def route(self, stage, B, exact=False):
        via = C.c_int(0)
        rc = self.so.emmax_op_decode_route(self.h, stage, B, int(exact), C.byref(via))
        assert (rc == 0) == (via.value > 0)
        return via.value if rc == 0 else R.REFUSED

    def routed_limit(self, exact=False):
        """the largest B such that every stage of every step of 1 .. B rows has a route"""
        for B in range(1, 65):
            if any(self.route(st, B, exact) == R.REFUSED for st in STAGES):
                return B - 1
        return 64

    def exact_session_ok(self, lib, max_batch):
        ws, kv = C.c_int64(), C.c_int64()
        with lib.tuning(exact=1):
            return int(self.so.emmax_session_bytes(self.h, max_batch, 8, NP_7B + 8 + 64, C.byref(ws), C.byref(kv)) == 0)


# ---- 1. the pinned limits ------------------------------------------------------------------------------------------------------------------
# config -> switches -> (emmax_model_max_decode_batch, [emmax_session_bytes accepts max_batch 1, 2, 3, 8, 9, 64 with exact on])
PINNED = {
    "7b-bf16": {
        "": (64, [1, 1, 1, 1, 1, 1]),
        "km=0": (8, [1, 1, 0, 0, 0, 0]),
        "km_down=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_direct=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_nsplit=2": (8, [1, 1, 1, 1, 1, 1]),
    },
    "7b-fp8": {
        "": (64, [0, 0, 0, 0, 0, 0]),
        "km=0": (8, [0, 0, 0, 0, 0, 0]),
        "km_down=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_direct=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_nsplit=2": (8, [0, 0, 0, 0, 0, 0]),
    },
    "7b-mxfp4": {
        "": (16, [0, 0, 0, 0, 0, 0]),
        "km=0": (16, [0, 0, 0, 0, 0, 0]),
        "km_down=0": (16, [0, 0, 0, 0, 0, 0]),
        "attn_direct=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_nsplit=2": (8, [0, 0, 0, 0, 0, 0]),
    },
    "tiny": {
        "": (8, [1, 1, 1, 1, 1, 1]),
        "km=0": (8, [1, 1, 0, 0, 0, 0]),
        "km_down=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_direct=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_nsplit=2": (8, [1, 1, 1, 1, 1, 1]),
    },
    "G": {
        "": (8, [1, 1, 1, 1, 1, 1]),
        "km=0": (8, [1, 1, 0, 0, 0, 0]),
        "km_down=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_direct=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_nsplit=2": (8, [1, 1, 1, 1, 1, 1]),
    },
    "G8": {
        "": (8, [0, 0, 0, 0, 0, 0]),
        "km=0": (8, [0, 0, 0, 0, 0, 0]),
        "km_down=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_direct=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_nsplit=2": (8, [0, 0, 0, 0, 0, 0]),
    },
    "W": {
        "": (64, [1, 1, 1, 1, 1, 1]),
        "km=0": (8, [1, 1, 0, 0, 0, 0]),
        "km_down=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_direct=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_nsplit=2": (8, [1, 1, 1, 1, 1, 1]),
    },
    "W8": {
        # was 64: decode_km.hip / decode_kmp.hip refuse the fp8 qkv, gate/up and lm-head at 9-32 rows (K = 256 is not whole 64-element steps
        # for eight waves) and decode_mfma.hip stops at 8 -- the one entry that moved, down to what launch_proj runs
        "": (8, [0, 0, 0, 0, 0, 0]),
        "km=0": (8, [0, 0, 0, 0, 0, 0]),
        "km_down=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_direct=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_nsplit=2": (8, [0, 0, 0, 0, 0, 0]),
    },
    "H": {
        "": (64, [1, 1, 1, 1, 1, 1]),
        "km=0": (8, [1, 1, 0, 0, 0, 0]),
        "km_down=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_direct=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_nsplit=2": (8, [1, 1, 1, 1, 1, 1]),
    },
    "H8": {
        "": (64, [0, 0, 0, 0, 0, 0]),
        "km=0": (8, [0, 0, 0, 0, 0, 0]),
        "km_down=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_direct=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_nsplit=2": (8, [0, 0, 0, 0, 0, 0]),
    },
    "G4": {
        "": (8, [0, 0, 0, 0, 0, 0]),
        "km=0": (8, [0, 0, 0, 0, 0, 0]),
        "km_down=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_direct=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_nsplit=2": (8, [0, 0, 0, 0, 0, 0]),
    },
    "W4": {
        "": (16, [0, 0, 0, 0, 0, 0]),
        "km=0": (16, [0, 0, 0, 0, 0, 0]),
        "km_down=0": (16, [0, 0, 0, 0, 0, 0]),
        "attn_direct=0": (8, [0, 0, 0, 0, 0, 0]),
        "attn_nsplit=2": (8, [0, 0, 0, 0, 0, 0]),
    },
    "7b-gqa8": {
        "": (8, [1, 1, 1, 1, 1, 1]),
        "km=0": (8, [1, 1, 0, 0, 0, 0]),
        "km_down=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_direct=0": (8, [1, 1, 1, 1, 1, 1]),
        "attn_nsplit=2": (8, [1, 1, 1, 1, 1, 1]),
    },
}


@pytest.mark.parametrize("name", list(PINNED))
def test_pinned_limits(lib, name):
    L, so = lib
    m = Model(so, CONFIGS[name]())
    assert m.rc == 0, m.err
    for sw, (rows, exact_ok) in PINNED[name].items():
        with L.tuning(**{k: int(v) for k, v in (kv.split("=") for kv in sw.split(",") if kv)}):
            assert m.limit() == rows, (name, sw, m.limit(), rows)
            assert [m.exact_session_ok(L, b) for b in EXACT_B] == exact_ok, (name, sw)
    m.close()


# ---- 2. the routing table, from the pure route ---------------------------------------------------------------------------------------------
ENGINES = {"G": ("G", False, False), "W": ("W", False, False), "G8": ("G", True, False), "W8": ("W", True, False), "GX": ("G", False, True),
           "H8": ("H", True, False)}   # the engines of tests/test_decode_stages_gpu.py: (model, fp8, exact)


@pytest.mark.parametrize("eng,B,sw,via", R.CASES)
def test_route_gives_the_routing_table(lib, eng, B, sw, via):
    L, so = lib
    model, fp8, exact = ENGINES[eng]
    m = Model(so, R.make_cfg(model, fp8))
    assert m.rc == 0, m.err
    with L.tuning(**sw):
        got = {st: m.route(st, B, exact) for st in STAGES}
    m.close()
    assert got == via, {st: (R.VIA_NAME[got[st]], R.VIA_NAME[via[st]]) for st in STAGES if got[st] != via[st]}


def test_route_of_the_mxfp4_models(lib):
    """decode_km.hip at every batch it serves; nine rows on 2 kv heads split the attention, and the o-proj's 16-row form takes no partials"""
    _, so = lib
    for name, batches in (("G4", (1, 8)), ("W4", (1, 8, 16))):
        m = Model(so, M.make_cfg4(name))
        assert m.rc == 0, m.err
        for B in batches:
            assert {st: m.route(st, B) for st in STAGES} == R._all(R.KM), (name, B)
        if name == "G4":
            assert m.route(R.OPROJ, 9) == R.REFUSED and b"o-proj" in so.emmax_last_error()
        assert m.route(R.QKV, 17) == R.REFUSED
        m.close()


def test_route_rejects_what_is_not_a_projection_stage(lib):
    _, so = lib
    m = Model(so, R.make_cfg("G"))
    via = C.c_int(7)
    assert so.emmax_op_decode_route(m.h, 1, 1, 0, C.byref(via)) == -1 and b"stage" in so.emmax_last_error()
    assert so.emmax_op_decode_route(m.h, 0, 65, 0, C.byref(via)) == -1 and so.emmax_op_decode_route(m.h, 0, 0, 0, C.byref(via)) == -1
    assert so.emmax_op_decode_route(None, 0, 1, 0, C.byref(via)) == -1
    m.close()


# ---- 3. limit == route, by sweep -----------------------------------------------------------------------------------------------------------
def _grid_cfg(hidden, heads, inter, vocab, fmt):
    cfg = _tiny()
    L = cfg.llm
    L.hidden_size, L.intermediate_size, L.vocab_size, L.head_dim, L.num_layers = hidden, inter, vocab, 128, 2
    L.num_heads, L.num_kv_heads = heads
    cfg.decode_weight_dtype = fmt
    return cfg


@pytest.mark.parametrize("hidden", [256, 512, 1024, 4096, 5120])
@pytest.mark.parametrize("fmt", ["bf16", "fp8", "mxfp4", "mxfp6"])
def test_limit_equals_route(lib, hidden, fmt):
    _, so = lib
    for heads, inter, vocab in itertools.product(((4, 2), (32, 32), (32, 8)), (1024, 4096, 4160, 11008, 12288, 13824), (4096, 32064)):
        cfg = _grid_cfg(hidden, heads, inter, vocab, fmt)
        m = Model(so, cfg)
        what = (hidden, heads, inter, vocab, fmt)
        if fmt in ("mxfp4", "mxfp6"):   # check_config speaks before a model exists: it accepts exactly what the planner serves at 8 rows
            planned = so.emmax_config_max_decode_batch(C.byref(m.cc), 0)
            assert (m.rc == 0) == (planned >= 8), (what, m.rc, m.err, planned)
            if m.rc:
                assert f"{fmt.upper()} decode weights need" in m.err, (what, m.err)
                continue
            assert planned == m.limit()
        assert m.rc == 0, (what, m.err)
        for exact in (False, True):
            assert m.limit(exact) == m.routed_limit(exact), (what, exact, m.limit(exact), m.routed_limit(exact))
        m.close()


# ---- 4. the two drift cases ------------------------------------------------------------------------------------------------------------------
def test_fp8_hidden_256_answers_eight(lib):
    """DESIGN.md, decode-stage tests, finding (ii): no kernel serves the fp8 qkv / gate-up / lm-head of model W at 9-32 rows"""
    _, so = lib
    m = Model(so, R.make_cfg("W", True))
    assert m.limit() == 8 and m.routed_limit() == 8
    assert [m.route(st, 9) for st in STAGES] == [R.REFUSED, R.KM, R.REFUSED, R.KM, R.REFUSED]
    m.close()


def test_exact_engine_on_a_hidden_384_model_answers_two(lib):
    """hidden 384: a multiple of 64 (decode_ks.hip's two-term kernel takes it at 1-2 rows), not of 256 (decode_km.hip's EX kernels do not at 3-8).
    The engine's limit was 64 for every exact engine; a 3-row exact session is refused, naming the stage"""
    L, so = lib
    cfg = R.make_cfg("G")
    cfg.llm.hidden_size = 384
    m = Model(so, cfg)
    assert m.rc == 0, m.err
    assert m.limit(exact=True) == 2 and m.routed_limit(exact=True) == 2
    assert m.exact_session_ok(L, 2) == 1 and m.exact_session_ok(L, 3) == 0
    err = so.emmax_last_error().decode()
    assert "exact numerics" in err and "qkv" in err and "batch 3" in err, err
    m.close()
