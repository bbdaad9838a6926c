"""The references of tests/test_mxfp4_wide_gpu.py, checked on the CPU: the tolerance table of the 17-64-row MXFP4 stage tests re-measured
(the fp32 emulation of the documented roundings against the float64 reference, both on de-quantised weights: no kernel output anywhere), the
pinned count of (row, step) pairs that clear the id line in the end-to-end test, and the planted chain on the de-quantised W4-shape weights."""

import torch

import mxfp4_ref as M
import mxfp4_wide_ref as W
from conftest import ID_BUDGET_SHALLOW


def test_tolerance_table_matches_the_emulation():
    spread, rel = W.measure(quiet=True)
    for out in W.OUTPUTS:
        assert spread[out] <= 1.05 * W.SPREAD_W[out] + 1e-9, (out, spread[out], W.SPREAD_W[out])
        assert rel[out] <= 1.05 * W.REL_W[out] + 1e-9, (out, rel[out], W.REL_W[out])
        if W.SPREAD_W[out] > 1e-6:    # not padded
            assert spread[out] >= 0.66 * W.SPREAD_W[out], (out, spread[out], W.SPREAD_W[out])
        rtol, atol, tol = W.tolerances(out)
        assert rtol == 1e-2 and atol == max(4e-3, 2 * W.SPREAD_W[out]) and tol == max(1e-2, 2 * W.REL_W[out])


def test_the_stage_models_reach_the_forms_they_are_there_for():
    """tile and step counts, a priori: W4 -- qkv 768 tiles and gate/up 528 on 256 blocks (three per block), lm-head 2004 tiles (six per block), down K =
    33 steps (wave 0 five, the others four: the eleven-phase form); T4 -- gate/up 784 and lm-head 770 tiles (four per block: TMAX 6), K = 4096 = 32
    steps (four per wave of eight, eight per wave of four), down K = 49 steps"""
    w, t = W.MODELS["W4"], W.MODELS["T4"]
    cdiv = lambda a, b: (a + b - 1) // b
    assert cdiv(3 * 4096 // 16, 256) == 3 and cdiv(2 * w["inter"] // 16, 256) == 3 and cdiv(w["vocab"] // 16, 256) > 6 and cdiv(w["vocab"] // 16, cdiv(w["vocab"] // 16, 6)) == 6
    assert w["inter"] // 128 == 33 and w["inter"] % 128 == 0 and w["hidden"] // 128 == 8
    assert 2 * t["inter"] // 16 == 784 and t["vocab"] // 16 == 770 and cdiv(784, 256) == 4 and cdiv(770, 256) == 4
    assert t["hidden"] // 128 == 32 and t["inter"] // 128 == 49 and t["vocab"] % 8 == 0


def test_the_id_line_count_of_the_end_to_end_test():
    """the oracle alone, on the de-quantised random weights of seed E2E_RANDOM_SEED: how many of the 40 x 16 teacher-forced (row, step) pairs clear the
    a-priori id line -- pinned in the GPU test, and at least a quarter of them (a condition on the inputs, not a measurement of the kernel)"""
    cfg = W.e2e_cfg()
    sd_q = M.dequant_state_dict(W.e2e_state_dict(False, W.E2E_RANDOM_SEED))
    frames, rows = W.random_e2e_inputs()
    assert len(rows) == W.E2E_B == 40 and W.E2E_STEPS == 16 and W.E2E_B <= W.E2E_MAX_BATCH
    gens, traces = W.oracle_trace_batch(cfg, sd_q, frames, rows, W.E2E_STEPS)
    n = W.count_above_line(traces, ID_BUDGET_SHALLOW)
    assert n == W.E2E_ABOVE_LINE, n
    assert 4 * n >= W.E2E_B * W.E2E_STEPS
    # the batched trace is the oracle's own greedy_generate, row by row (spot check: the first row)
    g0, t0 = M.oracle_trace(cfg, sd_q, frames[:1], rows[0], 4)
    assert g0 == gens[0][:4]
    assert (torch.stack(t0) - traces[0, :4]).abs().max().item() <= 1e-4 * traces[0, :4].abs().max().item()


def test_planted_chain_survives_quantisation_on_the_wide_shape():
    """the oracle on the DE-QUANTISED planted weights emits the a-priori chain on every row of the ragged batch of 24"""
    from emmax.weights import planted_chain

    cfg = W.e2e_cfg()
    sd_q = M.dequant_state_dict(W.e2e_state_dict(True, W.E2E_PLANTED_SEED))
    frames, rows, steps = W.planted_batch(cfg)
    assert len(rows) == 24 and len({len(r) for r in rows}) == len(W.PLANTED_LENS)
    ref = W.planted_oracle(cfg, sd_q, frames, rows)
    for b, row in enumerate(rows):
        chain = planted_chain(cfg, row[-1], W.PLANTED_MAX_NEW)
        assert len(chain) == steps[b] + 8 + 1 <= W.PLANTED_MAX_NEW and chain[-1] == cfg.eos_token_id
        assert ref[b][: len(chain)] == chain, (b, ref[b], chain)
