"""CPU: what the grouped decode attention answers without a device.  The route rule itself (step.hip: attn_group_rows) reads a live session
-- its groups, its numerics, its model's heads -- and a session needs a device to exist, so the route witness lives in
tests/test_group_attn_session_gpu.py; here: the switch, the null answers and the refusals the ops make before they touch the device."""
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from emmax import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib, _lib.load()


def test_the_switch_is_in_the_table_and_defaults_to_the_rule(lib):
    L, so = lib
    assert L.tuning_get("attn_group") == int(os.environ.get("EMMAX_ATTN_GROUP", "-1"))
    with L.tuning(attn_group=0):
        assert L.tuning_get("attn_group") == 0
    assert L.tuning_get("attn_group") == int(os.environ.get("EMMAX_ATTN_GROUP", "-1"))
    header = open(os.path.join(ROOT, "include", "emmax.h")).read()
    assert re.search(r"\battn_group\b", header)


def test_null_session_and_null_operands(lib):
    L, so = lib
    assert so.emmax_session_attn_grouped(None, 8) == -1
    # the ops check their operands and shapes on the host first: nothing here reaches a device
    assert so.emmax_op_decode_attention_group(None, None, None, None, None, None, None, 8, 2, 2, 64, 8, 0.088, 4, None, None, None) == -1
    assert b"emmax_op_decode_attention_group" in so.emmax_last_error()
    assert so.emmax_op_decode_attention_group_kv8(None, None, None, None, None, None, None, None, None, None, None, 8, 2, 2, 64, 8, 4, None, 0.088, None) == -1
    assert so.emmax_op_decode_attention_group(None, None, None, None, None, None, None, 8, 3, 2, 64, 8, 0.088, 4, None, None, None) == -1   # 3 q heads on 2 kv heads
