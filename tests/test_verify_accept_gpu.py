"""GPU: the accept walk of a verify pass as a pure op (include/emmax.h: emmax_op_verify_accept; csrc/verify.hip) against its numpy restatement
(tests/verify_ref.py), bit for bit on every state array, the emitted counts and the emitted ids.

The shapes are the smallest at which the kernel can go wrong: one lane's worth of window rows and one more (63 / 64 / 65: the lanes' strided
search for the first mismatch), windows of 1 and 2, a long one (4096 rows: what a session of 64 x 64-token pages holds); B = 1 and a ragged
B = 3; the first mismatch at row 0, in the middle, at the last row and nowhere; EOS, the token budget and the stop rule ending the row at the
first, an inner and the last accepted token, the trigger straddling two passes; a done row first, in the middle and last; the output row one short
of full; the cache one short of max_ctx."""
import numpy as np
import pytest
import torch

import verify_ref as R

pytestmark = pytest.mark.gpu

EOS, PAD, MAX_OUT, MAX_CTX = 2, 0, 96, 1 << 20
STOP_IDS = np.array([701, 702, 703] + [0] * 13, np.int32)


def _window(rng, n, mismatch=None, eos_at=None, trigger_at=None):
    """ids [n] (pending token + guess) and argmax [n] that agrees with the guess everywhere but at row `mismatch`; eos_at / trigger_at: the
    model emits EOS / the three trigger ids from that row on, and the guess agrees."""
    ids = rng.integers(10, 600, size=n).astype(np.int32)
    am = np.concatenate([ids[1:], rng.integers(10, 600, size=1)]).astype(np.int32)
    if eos_at is not None:
        am[eos_at] = EOS
        if eos_at + 1 < n:
            ids[eos_at + 1] = EOS
    if trigger_at is not None:
        for j, t in enumerate(STOP_IDS[:3]):
            if trigger_at + j < n:
                am[trigger_at + j] = t
                if trigger_at + j + 1 < n:
                    ids[trigger_at + j + 1] = t
    if mismatch is not None:
        am[mismatch] = 5000 + mismatch
    return ids, am


def _run(device, windows, state, stop_cfg=(0, 0)):
    """windows: [(ids, argmax)] per row.  The op against the reference; returns the state after (numpy) for a second pass."""
    from emmax import _lib

    lib = _lib.load()
    B = len(windows)
    lens = [len(w[0]) for w in windows]
    P_max = max(lens)
    ids = np.full((B, P_max), PAD, np.int32)
    for b, (w, _) in enumerate(windows):
        ids[b, :len(w)] = w
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    am = np.concatenate([w[1] for w in windows]).astype(np.int32)
    cfg = np.array(stop_cfg, np.int32)
    want, want_em, want_new = R.accept(am, ids, cu, state, STOP_IDS, cfg, EOS, PAD, MAX_CTX)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    d = {k: dev(state[k]) for k in R.STATE_KEYS}
    d_am, d_ids, d_cu, d_sid, d_cfg = dev(am), dev(ids), dev(cu), dev(STOP_IDS), dev(cfg)
    d_em = torch.full((B,), -9, dtype=torch.int32, device=device)
    d_new = torch.full((int(cu[B]),), -1, dtype=torch.int32, device=device)
    _lib.check(lib.emmax_op_verify_accept(d_am.data_ptr(), d_ids.data_ptr(), P_max, d_cu.data_ptr(), B, d["cur_tok"].data_ptr(), d["ctx_len"].data_ptr(),
                                          d["done"].data_ptr(), d["n_out"].data_ptr(), d["max_new"].data_ptr(), d["stop_m"].data_ptr(),
                                          d["stop_after"].data_ptr(), d["out_ids"].data_ptr(), state["out_ids"].shape[1], d_sid.data_ptr(), d_cfg.data_ptr(),
                                          EOS, PAD, MAX_CTX, d_em.data_ptr(), d_new.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "emmax_op_verify_accept")
    torch.cuda.synchronize()
    got = {k: d[k].cpu().numpy() for k in R.STATE_KEYS}
    for k in R.STATE_KEYS:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert np.array_equal(d_em.cpu().numpy(), want_em), (d_em.cpu().numpy(), want_em)
    assert np.array_equal(d_new.cpu().numpy(), want_new)
    for k in ("max_new",):   # read-only inputs
        assert np.array_equal(got[k], state[k])
    return got, want_em


def _state(B, **kw):
    return R.make_state(B, kw.pop("max_out", MAX_OUT), PAD, **{"ctx_len": 300, **kw})


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096])
def test_window_lengths_and_the_first_mismatch(device, n):
    rng = np.random.default_rng(n)
    # (the token behind the window's last row is the bonus token: a mismatch can sit at rows 0 .. n - 2)
    for mismatch in [None] + sorted({m for m in (0, n // 2, n - 2) if 0 <= m <= n - 2}):
        _, em = _run(device, [_window(rng, n, mismatch)], _state(1, max_out=4200))
        assert em[0] == (n if mismatch is None else mismatch + 1)


def test_ragged_batch_with_every_mismatch_place(device):
    rng = np.random.default_rng(3)
    wins = [_window(rng, 65, 0), _window(rng, 7, None), _window(rng, 130, 128)]
    _, em = _run(device, wins, _state(3, ctx_len=[300, 17, 4000]))
    assert list(em) == [1, 7, 129]


@pytest.mark.parametrize("at", [0, 5, 11])
def test_eos_budget_and_stop_rule_end_the_row(device, at):
    """each end at the first, an inner and the last token of a 12-row run the guess agrees with"""
    rng = np.random.default_rng(at)
    n = 12
    _, em = _run(device, [_window(rng, n, eos_at=at)], _state(1))
    assert em[0] == at + 1
    _, em = _run(device, [_window(rng, n)], _state(1, n_out=4, max_new=4 + at + 1))
    assert em[0] == at + 1
    # the trigger's three ids end at row `at` (so it starts up to two rows before the pass: the matcher state comes in through stop_m)
    start = at - 2
    pre = max(-start, 0)
    _, em = _run(device, [_window(rng, n, trigger_at=max(start, 0)) if pre == 0 else _trigger_tail(rng, n, pre)], _state(1, stop_m=pre), stop_cfg=(3, 0))
    assert em[0] == at + 1


def _trigger_tail(rng, n, pre):
    """a window whose model tokens begin with the trigger's ids pre .. 2 (ids 0 .. pre - 1 were emitted by the pass before)"""
    ids, am = _window(rng, n)
    for j, t in enumerate(STOP_IDS[pre:3]):
        am[j] = t
        ids[j + 1] = t
    return ids, am


def test_stop_trigger_straddles_two_passes_and_n_after_runs_out(device):
    rng = np.random.default_rng(9)
    ids, am = _window(rng, 6, mismatch=5)
    am[3], am[4] = STOP_IDS[0], STOP_IDS[1]          # the pass ends (mismatch at its last row) with two of the three trigger ids out
    ids[4], ids[5] = STOP_IDS[0], STOP_IDS[1]
    am[5] = 5005
    st, em = _run(device, [(ids, am)], _state(1), stop_cfg=(3, 2))
    assert em[0] == 6 and st["stop_m"][0] == 0       # (the mismatching token 5005 itself reset the matcher)
    ids, am = _window(rng, 5, mismatch=4)
    am[3], ids[4] = STOP_IDS[0], STOP_IDS[0]
    am[4] = STOP_IDS[1]                               # the last row's token is the bonus token: emitted whatever the guess said
    st, em = _run(device, [(ids, am)], _state(1), stop_cfg=(3, 2))
    assert em[0] == 5 and st["stop_m"][0] == 2 and st["done"][0] == 0
    st["out_ids"] = st["out_ids"].copy()
    ids2, am2 = _window(rng, 8)
    ids2[0] = STOP_IDS[1]
    am2[0], ids2[1] = STOP_IDS[2], STOP_IDS[2]        # the second pass completes the trigger at its first token; two more tokens, then done
    st2, em = _run(device, [(ids2, am2)], st, stop_cfg=(3, 2))
    assert em[0] == 3 and st2["done"][0] == 1 and st2["stop_after"][0] == 2


@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_done_row_anywhere_in_the_batch_is_left_as_it_is(device, where):
    rng = np.random.default_rng(20 + where)
    done = [int(b == where) for b in range(3)]
    wins = [_window(rng, 1 if d else 9) for d in done]
    st = _state(3, done=done, cur_tok=[77, 78, 79], ctx_len=[300, 301, 302])
    after, em = _run(device, wins, st)
    assert em[where] == 0 and after["cur_tok"][where] == 77 + where and after["ctx_len"][where] == 300 + where
    assert all(em[b] == 9 for b in range(3) if b != where)


def test_output_row_one_short_of_full_and_cache_one_short_of_max_ctx(device):
    rng = np.random.default_rng(31)
    after, em = _run(device, [_window(rng, 5)], _state(1, n_out=MAX_OUT - 1))
    assert em[0] == 5 and after["n_out"][0] == MAX_OUT + 4                      # counted on, written once
    after, em = _run(device, [_window(rng, 5)], _state(1, ctx_len=MAX_CTX - 2))
    assert em[0] == 1 and after["done"][0] == 1 and after["ctx_len"][0] == MAX_CTX - 1
    after, em = _run(device, [_window(rng, 5)], _state(1, ctx_len=MAX_CTX - 3))
    assert em[0] == 2 and after["done"][0] == 1
    after, em = _run(device, [_window(rng, 4)], _state(1, n_out=6, max_new=6))  # the budget was spent before the pass: nothing is emitted
    assert em[0] == 0 and after["done"][0] == 1 and after["cur_tok"][0] == PAD


def test_bad_arguments_are_refused_before_the_launch(device):
    from emmax import _lib

    rng = np.random.default_rng(1)
    lib = _lib.load()
    z = torch.zeros(64, dtype=torch.int32, device=device)
    cu = torch.tensor([0, 9], dtype=torch.int32, device=device)   # a window of 9 rows, P_max = 4
    args = [z.data_ptr(), z.data_ptr(), 4, cu.data_ptr(), 1] + [z.data_ptr()] * 8 + [16, z.data_ptr(), z.data_ptr(), EOS, PAD, 100, z.data_ptr(), None,
                                                                                      torch.cuda.current_stream().cuda_stream]
    assert lib.emmax_op_verify_accept(*args) == -1 and b"P_max" in lib.emmax_last_error()
