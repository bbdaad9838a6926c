"""CPU: the host side of output_hidden_states / output_attentions (emmax/taps.py and the refusals of modeling / serving / dist): tap_layers to
masks, buffer shapes, the stacked-or-list rule, every refusal before an engine is touched, and the new symbols in the header and the binding."""

import ctypes as C
import os
import re

import pytest
import torch

from emmax import taps as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"emmax_session_set_pass_taps": 7, "emmax_session_set_step_taps": 8, "emmax_session_clear_taps": 2, "emmax_session_taps": 1,
               "emmax_op_attn_probs": 17, "emmax_op_attn_probs_kv8": 18, "emmax_op_tap_rows": 9}


def test_tap_layers_to_indices_and_masks():
    assert T.select_layers(None, 4, "hidden_states") == [0, 1, 2, 3]
    assert T.select_layers([-1], 4, "hidden_states") == [3] and T.select_layers([-4, 0], 4, "hidden_states") == [0]   # negative, duplicates once
    assert T.select_layers([2, 0, 2], 4, "hidden_states") == [0, 2] and T.select_layers((1,), 3, "attentions") == [1]
    for bad in ([4], [-5], [], 3, [1.0], [True], "01"):
        with pytest.raises(ValueError):
            T.select_layers(bad, 4, "hidden_states")
    assert T.layer_mask([0, 2]) == 0b101 and T.layer_mask([]) == 0 and T.layer_mask([32]) == 1 << 32
    # one keyword, two tuples: hidden_states has n_layers + 1 entries, attentions n_layers
    s = T.tap_spec(3, True, True, [-1])
    assert s.hidden == [3] and s.attn == [2] and s.any
    s = T.tap_spec(3, True, False, None)
    assert s.hidden == [0, 1, 2, 3] and s.attn == []
    assert T.tap_spec(3, False, False, None) is None and T.tap_spec(3, None, None, [0]) is None
    with pytest.raises(ValueError):
        T.tap_spec(3, True, True, [3])        # entry 3 of hidden_states exists, layer 3 of attentions does not
    with pytest.raises(ValueError):
        T.tap_spec(3, False, False, [9])      # checked even when nothing is asked for
    assert T.tap_spec(3, True, False, [3]).hidden == [3]


def test_buffer_shapes_and_ld_keys():
    s = T.TapSpec([0, 3], [1])
    assert T.pass_shapes(s, 40, 256, 4, 36) == ((2, 40, 256), (1, 40, 4, 36))
    assert T.step_shapes(s, 6, 3, 256, 4, 300) == ((6, 2, 3, 256), (6, 1, 3, 4, 300))
    assert T.pass_shapes(T.TapSpec([], [0]), 5, 8, 2, 8) == (None, (1, 5, 2, 8)) and T.step_shapes(T.TapSpec([1], []), 2, 1, 8, 2, 8)[1] is None
    assert [T.round_keys(n) for n in (1, 4, 5, 263, 1028)] == [4, 4, 8, 264, 1028]
    h, a = T.pass_shapes(T.TapSpec([], list(range(32))), 768, 4096, 32, T.round_keys(768))
    assert h is None and 4 * a[0] * a[1] * a[2] * a[3] == 2415919104   # the docstring's 2.4 GB: all maps of a 7B prompt of 768 rows


def test_cut_pass_follows_the_stacked_or_list_rule():
    H, Hq = 8, 2
    hid = torch.arange(2 * 7 * H, dtype=torch.float32).view(2, 7, H)
    att = torch.rand(1, 7, Hq, 12)
    hs, at = T.cut_pass(hid, att, [3, 4], [3, 4])          # ragged: a list per row
    assert len(hs) == 2 and isinstance(hs[0], list) and hs[1][1].shape == (4, H) and torch.equal(hs[1][1], hid[1, 3:7])
    assert isinstance(at[0], list) and at[0][0].shape == (Hq, 3, 3) and at[0][1].shape == (Hq, 4, 4) and torch.equal(at[0][1][1, 2], att[0, 5, 1, :4])
    hs, at = T.cut_pass(hid[:, :6], att[:, :6], [3, 3], [3, 3])   # equal rows: stacked [B, n, H] / [B, Hq, n, L]
    assert hs[0].shape == (2, 3, H) and at[0].shape == (2, Hq, 3, 3)
    hs, at = T.cut_pass(hid[:, :6], att[:, :6], [3, 3], [5, 9])   # a continuation: equal n, different contexts -> the maps are a list
    assert hs[0].shape == (2, 3, H) and isinstance(at[0], list) and at[0][1].shape == (Hq, 3, 9)
    assert T.cut_pass(None, att, [3, 4], [3, 4])[0] is None and T.cut_pass(hid, None, [3, 4], [3, 4])[1] is None
    sh, sa = torch.rand(4, 2, 3, H), torch.rand(4, 1, 3, Hq, 16)
    hs, at = T.cut_step(sh, sa, 2, [10, 10, 10])
    assert hs[1].shape == (3, 1, H) and torch.equal(hs[1][:, 0], sh[2, 1]) and at[0].shape == (3, Hq, 1, 10)
    hs, at = T.cut_step(sh, sa, 1, [9, 12, 10])
    assert isinstance(at[0], list) and at[0][1].shape == (Hq, 1, 12) and torch.equal(at[0][1][:, 0], sa[1, 0, 1, :, :12])


# ---- refusals, each with its own message, before an engine is touched ---------------------------------------------------------------------------------
class _NoEngine:
    """a model without an engine: whatever reaches for one fails the test"""

    def __init__(self, exact=0):
        from emmax.config import EmmaXConfig
        from emmax.modeling import EmmaXForActionPrediction

        self.m = EmmaXForActionPrediction.__new__(EmmaXForActionPrediction)
        self.m.config = EmmaXConfig.tiny(gqa=True)
        self.m.engine = type("E", (), {"exact": exact})() if exact else None

        def boom(*a, **k):
            raise AssertionError("the engine was touched")

        self.m._need_engine = boom
        self.m._prefill = boom


def test_generate_refuses_beams_sample_groups_and_exact_models_with_taps():
    m = _NoEngine().m
    rows = [[1, 5, 6]]
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(rows, max_new_tokens=2, return_dict_in_generate=True, output_hidden_states=True, num_beams=2)
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        m.generate(rows, max_new_tokens=2, return_dict_in_generate=True, output_attentions=True, do_sample=True, num_return_sequences=2)
    with pytest.raises(ValueError, match="tap_layers"):
        m.generate(rows, max_new_tokens=2, return_dict_in_generate=True, output_attentions=True, tap_layers=[3])
    with pytest.raises(NotImplementedError, match="num_beams"):
        m._tap_args(True, False, [-1], 2, 1)   # (what predict_action(return_hidden_states=True, num_beams=2) asks)
    x = _NoEngine(exact=1).m
    with pytest.raises(NotImplementedError, match="exact"):
        x.generate(rows, max_new_tokens=2, return_dict_in_generate=True, output_hidden_states=True)
    with pytest.raises(NotImplementedError, match="exact"):
        x._tap_args(False, True, None)
    from emmax.sampling import BeamParams

    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate_ids(rows, max_new_tokens=2, hidden=[0], beams=BeamParams(2))
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        m.generate_ids(rows, max_new_tokens=2, attentions=[0], num_samples=2)
    with pytest.raises(ValueError, match="hidden takes"):
        m.generate_ids(rows, max_new_tokens=2, hidden=[4])
    with pytest.raises(NotImplementedError, match="exact"):
        x.generate_ids(rows, max_new_tokens=2, hidden=[0])


def test_slot_serving_and_the_data_parallel_call_refuse_taps():
    from emmax import dist, serving

    sch = serving.SlotScheduler.__new__(serving.SlotScheduler)
    for kw in ({"output_hidden_states": True}, {"output_attentions": True}):
        with pytest.raises(NotImplementedError, match="request slots"):
            sch.submit(serving.Request(rid=0, frame=None, prompt_ids=[1, 2], **kw))
    for kw in ({"output_hidden_states": True}, {"output_attentions": True}):
        with pytest.raises(NotImplementedError, match="data-parallel"):
            dist.generate_actions_dp(None, None, [[1]], **kw)


def test_forward_no_longer_refuses_the_outputs_by_name():
    src = open(os.path.join(ROOT, "emma-x_amd", "emmax", "modeling.py")).read()
    assert "not materialised by the fused kernels" not in src and "tap_layers" in src


# ---- bindings ---------------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported_at_abi_12():
    from emmax import _lib

    so = _lib.load()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "emmax.h")).read())
    assert "#define EMMAX_ABI_VERSION 12" in flat and _lib.ABI_VERSION == 12 and so.emmax_abi_version() == 12
    for name, nargs in NEW_SYMBOLS.items():
        m = re.search(r"\bint %s\(([^)]*)\)" % name, flat)
        assert m and name in _lib.SIGNATURES and hasattr(so, name), name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]) and _lib.SIGNATURES[name][0] is C.c_int, name
    assert _lib.SIGNATURES["emmax_session_set_pass_taps"][1][2] is C.c_uint64 and "uint64_t hidden_layers" in flat   # 64-bit masks on both sides
    assert so.emmax_session_taps(None) == -1 and so.emmax_session_clear_taps(None, None) == -1                    # host only, no GPU
    assert so.emmax_session_set_pass_taps(None, None, 0, None, 0, 0, None) == -1 and so.emmax_op_tap_rows(None, 1, 8, None, 1, 8, None, 1e-5, None) == -1
