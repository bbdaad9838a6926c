"""MXFP4 decode weights at 17-64 rows (tuning switch mx4_wide) on the CPU, through the host-only planner calls as tests/test_decode_plan.py does.
The switch is read once, at emmax_model_create, and frozen into the model: with it off every answer is the one the library gave before the
switch existed; a model created under it serves 64 rows on the shapes decode_kmp.hip's MX4 form takes, whatever the switch says later."""

import copy
import ctypes as C
import itertools
import os
import re

import pytest

import decode_stage_ref as R
import mxfp4_ref as M
from test_decode_plan import Model, STAGES, _grid_cfg, _seven_b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from emmax import _lib

    return _lib, _lib.load()


def _wide(L, so, cfg):
    with L.tuning(mx4_wide=1):
        return Model(so, cfg)


def _session_ok(so, m, rows):
    ws, kv = C.c_int64(), C.c_int64()
    return so.emmax_session_bytes(m.h, rows, 8, 320, C.byref(ws), C.byref(kv))


def test_switch_off_every_answer_is_the_narrow_one(lib):
    L, so = lib
    assert L.tuning_get("mx4_wide") == 0            # the default
    for cfg, rows in ((_seven_b("mxfp4"), 16), (M.make_cfg4("W4"), 16), (M.make_cfg4("G4"), 8)):
        m = Model(so, cfg)
        assert m.rc == 0, m.err
        assert m.limit() == rows and so.emmax_model_mxfp4_wide(m.h) == 0
        assert so.emmax_config_max_decode_batch(C.byref(m.cc), 0) == rows
        assert m.route(R.QKV, 17) == R.REFUSED
        m.close()
    m = Model(so, M.make_cfg4("W4"))
    assert _session_ok(so, m, 16) == 0
    assert _session_ok(so, m, 17) == -1
    assert so.emmax_last_error() == b"MXFP4 decode weights serve batches of 1-16 rows; max_batch 17"
    m.close()
    assert so.emmax_model_mxfp4_wide(None) == -1
    bf = Model(so, R.make_cfg("W"))
    with L.tuning(mx4_wide=1):
        bf_w = Model(so, R.make_cfg("W"))
    assert so.emmax_model_mxfp4_wide(bf.h) == 0 and so.emmax_model_mxfp4_wide(bf_w.h) == 0   # (only MXFP4 models freeze it)
    assert bf_w.limit() == bf.limit() == 64
    bf.close(); bf_w.close()


def test_a_model_created_under_the_switch_serves_64_rows(lib):
    L, so = lib
    for cfg in (_seven_b("mxfp4"), M.make_cfg4("W4")):
        m = _wide(L, so, cfg)
        assert m.rc == 0, m.err
        assert L.tuning_get("mx4_wide") == 0        # the switch is back: the model keeps what it froze
        assert so.emmax_model_mxfp4_wide(m.h) == 1
        assert m.limit() == 64 and m.routed_limit() == 64
        assert _session_ok(so, m, 17) == 0 and _session_ok(so, m, 64) == 0
        assert _session_ok(so, m, 65) == -1
        assert m.limit(exact=True) == 0             # exact numerics: still refused on quantised weights
        with L.tuning(exact=1):
            assert _session_ok(so, m, 1) == -1 and b"MXFP4" in so.emmax_last_error()
        m.close()


def test_a_model_created_before_the_switch_keeps_sixteen(lib):
    L, so = lib
    m = Model(so, M.make_cfg4("W4"))
    with L.tuning(mx4_wide=1):
        assert m.limit() == 16 and so.emmax_model_mxfp4_wide(m.h) == 0
        assert m.route(R.QKV, 17) == R.REFUSED
        assert _session_ok(so, m, 17) == -1 and so.emmax_last_error() == b"MXFP4 decode weights serve batches of 1-16 rows; max_batch 17"
        # emmax_config_max_decode_batch has no model: it reads the switch as it stands at the call
        assert so.emmax_config_max_decode_batch(C.byref(m.cc), 0) == 64
    assert so.emmax_config_max_decode_batch(C.byref(m.cc), 0) == 16
    m.close()


def test_route_per_stage_of_a_wide_model(lib):
    """km at 1-16 rows, kmp at 17, 32, 33 and 64; at 40 rows down and lm-head run as 32 + 8 and the route reports the last launch: the 8-row km chunk"""
    L, so = lib
    for cfg in (M.make_cfg4("W4"), _seven_b("mxfp4")):
        m = _wide(L, so, cfg)
        for B in (1, 8, 9, 16):
            assert {st: m.route(st, B) for st in STAGES} == R._all(R.KM), B
        for B in (17, 32, 64):
            assert {st: m.route(st, B) for st in STAGES} == R._all(R.KMP), B
        # 33 = 32 + 1: the one-row tail of down / lm-head is a decode_km.hip launch (the only family that reads the 4-bit tiles at 1-16 rows)
        assert {st: m.route(st, 33) for st in STAGES} == {R.QKV: R.KMP, R.OPROJ: R.KMP, R.GATEUP: R.KMP, R.DOWN: R.KM, R.LMHEAD: R.KM}
        assert {st: m.route(st, 40) for st in STAGES} == {R.QKV: R.KMP, R.OPROJ: R.KMP, R.GATEUP: R.KMP, R.DOWN: R.KM, R.LMHEAD: R.KM}
        assert {st: m.route(st, 48) for st in STAGES} == {R.QKV: R.KMP, R.OPROJ: R.KMP, R.GATEUP: R.KMP, R.DOWN: R.KM, R.LMHEAD: R.KM}   # 32 + 16
        assert {st: m.route(st, 49) for st in STAGES} == R._all(R.KMP)                                                                   # 32 + 17
        m.close()


def test_what_stays_narrow_under_the_switch(lib):
    """2 kv heads: nine rows would split the attention -- still 8.  hidden 4096 / intermediate 12288: K = 12288 is twelve phases of a wave, the down
    projection has no 17-row route -- still 16"""
    L, so = lib
    g = _wide(L, so, M.make_cfg4("G4"))
    assert so.emmax_model_mxfp4_wide(g.h) == 1 and g.limit() == 8 and g.routed_limit() == 8
    g.close()
    big = _wide(L, so, _grid_cfg(4096, (32, 32), 12288, 32064, "mxfp4"))
    assert big.rc == 0, big.err
    assert big.limit() == 16 and big.routed_limit() == 16
    assert big.route(R.DOWN, 17) == R.REFUSED and big.route(R.QKV, 17) == R.KMP
    big.close()
    ok = _wide(L, so, _grid_cfg(4096, (32, 32), 11008, 32064, "mxfp4"))
    assert ok.limit() == 64
    ok.close()


@pytest.mark.parametrize("hidden", [256, 512, 1024, 4096, 5120])
def test_limit_equals_route_under_the_switch(lib, hidden):
    """tests/test_decode_plan.py's grid for fmt = "mxfp4", every model created wide"""
    L, so = lib
    seen = set()
    for heads, inter, vocab in itertools.product(((4, 2), (32, 32), (32, 8)), (1024, 4096, 4160, 11008, 12288, 13824), (4096, 32064)):
        cfg = _grid_cfg(hidden, heads, inter, vocab, "mxfp4")
        m = _wide(L, so, cfg)
        what = (hidden, heads, inter, vocab)
        with L.tuning(mx4_wide=1):
            planned = so.emmax_config_max_decode_batch(C.byref(m.cc), 0)
        assert (m.rc == 0) == (planned >= 8), (what, m.rc, m.err, planned)
        if m.rc:
            assert "MXFP4 decode weights need" in m.err, (what, m.err)
            continue
        assert planned == m.limit(), what
        for exact in (False, True):
            assert m.limit(exact) == m.routed_limit(exact), (what, exact, m.limit(exact), m.routed_limit(exact))
        seen.add(m.limit())
        m.close()
    if hidden in (1024, 4096):
        assert seen == {8, 16, 64}, seen   # 2 / 8 kv heads; intermediate 12288; the rest


def test_abi_version_and_the_new_symbols(lib):
    L, so = lib
    assert L.ABI_VERSION == 12 and so.emmax_abi_version() == 12
    header = open(os.path.join(ROOT, "include", "emmax.h")).read()
    assert re.search(r"^#define EMMAX_ABI_VERSION 12$", header, re.M)
    for name in ("emmax_model_mxfp4_wide", "emmax_op_gemm_wide_mxfp4"):
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in L.SIGNATURES and hasattr(so, name)
    assert "mx4_wide" in header
    with pytest.raises(L.EmmaxError):
        L.tuning_get("mx4_wider")


def test_mxfp4_wide_on_another_weight_format_is_a_value_error():
    """before anything touches a device: no GPU here, and none is asked for"""
    import torch

    from emmax.config import EmmaXConfig
    from emmax.engine import EmmaxEngine
    from emmax.modeling import EmmaXForActionPrediction

    cfg = EmmaXConfig.tiny()
    assert cfg.decode_weight_dtype == "bf16"
    with pytest.raises(ValueError, match="mxfp4_wide"):
        EmmaxEngine(cfg, {}, device="cuda:0", mxfp4_wide=True)
    model = EmmaXForActionPrediction(cfg, {"x": torch.zeros(1)})
    with pytest.raises(ValueError, match="mxfp4_wide"):
        model.to("cuda:0", mxfp4_wide=True)
    with pytest.raises(ValueError, match="mxfp4_wide"):
        EmmaXForActionPrediction.from_synthetic(copy.deepcopy(cfg), device="cuda:0", decode_weight_dtype="fp8", mxfp4_wide=True)
