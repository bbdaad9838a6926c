"""CPU: the host reference sampler (tests/sampling_ref.py) against Philox known answers and transformers' logits warpers, and the
host-side checks of emmax/sampling.py (SamplingParams, sample_logits arguments, seeds)."""
import numpy as np
import pytest
import torch

import sampling_ref as ref


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds."""
    cases = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for ctr, key, want in cases:
        got = ref.philox4x32_10(np.array([ctr], dtype=np.uint64), key)[0]
        assert [int(v) for v in got] == list(want), [hex(int(v)) for v in got]


def test_noise_stream_layout():
    """word i % 4 of counter (i / 4, step, subseq, 0) under key (seed lo, seed hi)"""
    seed = 0x0123456789ABCDEF
    x = ref.noise_words(10, seed, 5, 7)
    blk = ref.philox4x32_10(np.array([[2, 5, 7, 0]], dtype=np.uint64), (0x89ABCDEF, 0x01234567))[0]
    assert [int(v) for v in x[8:10]] == [int(blk[0]), int(blk[1])]
    g = ref.gumbel(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert np.all(np.isfinite(g)) and g[0] < g[1]


def _hf_kept(l, T, k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    scores = torch.from_numpy(np.asarray(l, dtype=np.float32))[None].double()
    ids = torch.zeros(1, 1, dtype=torch.long)
    scores = TemperatureLogitsWarper(T)(ids, scores)
    if k > 0:
        scores = TopKLogitsWarper(k)(ids, scores)
    if p < 1:
        scores = TopPLogitsWarper(p)(ids, scores)
    return torch.isfinite(scores[0]).numpy()


def test_kept_set_matches_transformers_warpers():
    pytest.importorskip("transformers")
    rng = np.random.default_rng(11)
    checked = 0
    for V in (64, 1000, 4096):
        for T in (0.5, 1.0, 1.7):
            for k in (0, 1, 5, 50):
                for p in (1.0, 0.9, 0.5, 0.1):
                    for _ in range(2):
                        l = (rng.standard_normal(V) * 3).astype(np.float32)
                        if len(np.unique(l / np.float32(T))) != V:
                            continue
                        keep, _, slack = ref.kept_set(l, T, k, p)
                        if slack < 1e-6:
                            continue
                        np.testing.assert_array_equal(keep, _hf_kept(l, T, k, p), err_msg=f"V={V} T={T} k={k} p={p}")
                        checked += 1
    assert checked > 250


def test_sample_row_draws_from_the_kept_set_and_greedy_is_argmax():
    rng = np.random.default_rng(3)
    l = (rng.standard_normal(500) * 2).astype(np.float32)
    keep, _, _ = ref.kept_set(l, 0.8, 20, 0.7)
    toks = {ref.sample_row(l, 0.8, 20, 0.7, 99, s, 0)[0] for s in range(300)}
    assert toks <= set(np.flatnonzero(keep)) and len(toks) > 1
    t, lp, _ = ref.sample_row(l, 0.0, 0, 1.0, 0, 0, 0)
    assert t == int(np.argmax(l)) and abs(lp - float(torch.log_softmax(torch.from_numpy(l).double(), 0)[t])) < 1e-12


def test_sampling_params_validation():
    from emmax.sampling import SamplingParams

    assert SamplingParams() == SamplingParams(1.0, 50, 1.0, None)
    SamplingParams(temperature=0.0, top_k=0, top_p=1.0, seed=(1 << 64) - 1)
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)


def test_sample_logits_checks_its_arguments_before_any_launch():
    from emmax.sampling import SamplingParams, sample_logits

    p = SamplingParams(0.8, 20, 0.9, seed=1)
    with pytest.raises(ValueError):
        sample_logits(torch.zeros(2, 100), p)                     # a host tensor: the kernel runs on the device only
    with pytest.raises(ValueError):
        sample_logits(torch.zeros(100), p)                        # one row must still be 2-D
    with pytest.raises(ValueError):
        sample_logits(torch.zeros(2, 100, dtype=torch.float64), p)


def test_draw_seed_follows_torch_manual_seed():
    from emmax.sampling import draw_seed

    torch.manual_seed(5)
    a = draw_seed()
    torch.manual_seed(5)
    b = draw_seed()
    assert a == b == draw_seed(torch.Generator().manual_seed(5)) and 0 <= a < 1 << 64
