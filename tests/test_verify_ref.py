"""CPU: the numpy restatement of the verify pass's accept walk (tests/verify_ref.py), pinned by hand-written cases whose answers are written
out here.  test_verify_accept_gpu.py holds the kernel to this reference bit for bit."""
import numpy as np

from verify_ref import accept, make_state

EOS, PAD, MAX_OUT, MAX_CTX = 2, 0, 16, 100
NO_STOP = (np.zeros(16, np.int32), np.array([0, 0], np.int32))


def _one(window, argmax, stop=NO_STOP, **state):
    """One row: window = pending token + guess, argmax = the model's token behind every window row.  The row has emitted its pending token."""
    st = make_state(1, MAX_OUT, PAD, **{"ctx_len": 10, "cur_tok": window[0], **state})
    st["out_ids"][0, 0] = window[0]
    cu = np.array([0, len(window)], np.int32)
    after, emitted, new_ids = accept(np.array(argmax, np.int32), np.array([window], np.int32), cu, st, stop[0], stop[1], EOS, PAD, MAX_CTX)
    return st, after, int(emitted[0]), list(new_ids)


def _row(after, key):
    return int(after[key][0])


def test_full_acceptance_emits_a_token_per_window_row():
    before, after, emitted, new_ids = _one([5, 6, 7, 8], [6, 7, 8, 9])
    assert emitted == 4 and new_ids == [6, 7, 8, 9]
    assert _row(after, "ctx_len") == 14 and _row(after, "n_out") == 5 and _row(after, "cur_tok") == 9 and _row(after, "done") == 0
    assert list(after["out_ids"][0, :6]) == [5, 6, 7, 8, 9, PAD]
    assert _row(before, "ctx_len") == 10 and _row(before, "n_out") == 1   # the input state is not touched


def test_mismatch_at_row_0_is_one_plain_decode_step():
    _, after, emitted, new_ids = _one([5, 6, 7, 8], [11, 7, 8, 9])
    assert emitted == 1 and new_ids == [11, -1, -1, -1]
    assert _row(after, "ctx_len") == 11 and _row(after, "n_out") == 2 and _row(after, "cur_tok") == 11 and _row(after, "done") == 0
    assert list(after["out_ids"][0, :3]) == [5, 11, PAD]


def test_mismatch_in_the_middle_keeps_the_models_token():
    _, after, emitted, new_ids = _one([5, 6, 7, 8], [6, 12, 8, 9])
    assert emitted == 2 and new_ids == [6, 12, -1, -1]
    assert _row(after, "ctx_len") == 12 and _row(after, "cur_tok") == 12 and list(after["out_ids"][0, :4]) == [5, 6, 12, PAD]


def test_eos_inside_the_run_ends_the_row_there():
    _, after, emitted, new_ids = _one([5, 6, EOS, 8], [6, EOS, 8, 9])   # (the guess agrees beyond EOS: the walk must not follow it)
    assert emitted == 2 and new_ids == [6, EOS, -1, -1]
    assert _row(after, "done") == 1 and _row(after, "ctx_len") == 12 and _row(after, "n_out") == 3 and _row(after, "cur_tok") == EOS


def test_budget_ends_inside_the_run():
    _, after, emitted, new_ids = _one([5, 6, 7, 8], [6, 7, 8, 9], max_new=3)
    assert emitted == 2 and new_ids == [6, 7, -1, -1]
    assert _row(after, "done") == 1 and _row(after, "n_out") == 3 and _row(after, "ctx_len") == 12 and _row(after, "cur_tok") == 7


def test_budget_spent_before_the_pass_emits_nothing():
    _, after, emitted, new_ids = _one([5, 6], [6, 7], n_out=3, max_new=3)
    assert emitted == 0 and new_ids == [-1, -1]
    assert _row(after, "done") == 1 and _row(after, "n_out") == 3 and _row(after, "ctx_len") == 10 and _row(after, "cur_tok") == PAD


def test_stop_trigger_completes_and_n_after_runs_out_inside_the_run():
    stop = (np.array([7, 8] + [0] * 14, np.int32), np.array([2, 1], np.int32))
    _, after, emitted, new_ids = _one([5, 6, 7, 8, 9, 10], [6, 7, 8, 9, 10, 11], stop=stop)
    # 6: no match; 7: one id matched; 8: the trigger is complete (0 tokens after it); 9: one token after it -> done
    assert emitted == 4 and new_ids[:4] == [6, 7, 8, 9]
    assert _row(after, "done") == 1 and _row(after, "stop_after") == 1 and _row(after, "stop_m") == 0 and _row(after, "ctx_len") == 14


def test_stop_trigger_straddles_two_passes():
    stop = (np.array([7, 8] + [0] * 14, np.int32), np.array([2, 1], np.int32))
    _, after, emitted, new_ids = _one([7, 8, 9, 10], [8, 9, 10, 11], stop=stop, stop_m=1)   # 7 was matched by the pass before
    assert emitted == 2 and new_ids[:2] == [8, 9] and _row(after, "done") == 1 and _row(after, "stop_after") == 1
    _, after, emitted, _ = _one([7, 8, 9, 10], [8, 9, 10, 11], stop=stop, stop_m=0)           # without the carried match nothing stops
    assert emitted == 4 and _row(after, "done") == 0 and _row(after, "stop_after") == -1


def test_a_done_row_is_left_exactly_as_it_is():
    before, after, emitted, new_ids = _one([5, 6, 7], [6, 7, 8], done=1)
    assert emitted == 0 and new_ids == [-1, -1, -1]
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_cache_end_inside_the_run():
    _, after, emitted, _ = _one([5, 6, 7, 8], [6, 7, 8, 9], ctx_len=MAX_CTX - 3)
    assert emitted == 2 and _row(after, "done") == 1 and _row(after, "ctx_len") == MAX_CTX - 1


def test_output_row_full_counts_on_without_writing():
    st = make_state(1, 4, PAD, ctx_len=10, n_out=3, cur_tok=5)
    after, emitted, _ = accept(np.array([6, 7, 8], np.int32), np.array([[5, 6, 7]], np.int32), np.array([0, 3], np.int32), st, *NO_STOP, EOS, PAD, MAX_CTX)
    assert int(emitted[0]) == 3 and int(after["n_out"][0]) == 6 and list(after["out_ids"][0]) == [PAD, PAD, PAD, 6]


def test_ragged_batch_rows_are_independent():
    st = make_state(3, MAX_OUT, PAD, ctx_len=[10, 20, 30], cur_tok=[5, 5, 5], done=[0, 1, 0])
    ids = np.array([[5, 6, 7], [5, PAD, PAD], [5, 9, PAD]], np.int32)
    cu = np.array([0, 3, 4, 6], np.int32)
    after, emitted, new_ids = accept(np.array([6, 7, 8, 99, 9, 10], np.int32), ids, cu, st, *NO_STOP, EOS, PAD, MAX_CTX)
    assert list(emitted) == [3, 0, 2] and list(new_ids) == [6, 7, 8, -1, 9, 10]
    assert list(after["ctx_len"]) == [13, 20, 32] and list(after["cur_tok"]) == [8, 5, 10]
