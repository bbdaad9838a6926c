"""The accept walk of a verify pass restated in numpy (csrc/verify.hip: emmax_verify_accept_kernel), which is a decode step's bookkeeping
(csrc/kernels.h: emmax_finish_row, is_prefill = 0) restated once per emitted token.  Shared by test_verify_ref.py (pinned by hand-written cases)
and test_verify_accept_gpu.py (the kernel against it, bit for bit).  No torch, no GPU."""
import numpy as np

STATE_KEYS = ("cur_tok", "ctx_len", "done", "n_out", "max_new", "stop_m", "stop_after", "out_ids")


def make_state(B, max_out, pad_id, ctx_len, n_out=1, max_new=1 << 30, done=0, cur_tok=0, stop_m=0, stop_after=-1):
    """Per-row state arrays of B rows (scalars are broadcast), int32; the output rows pad-filled."""
    def col(v):
        return np.broadcast_to(np.asarray(v, dtype=np.int32), (B,)).copy()
    return {"cur_tok": col(cur_tok), "ctx_len": col(ctx_len), "done": col(done), "n_out": col(n_out), "max_new": col(max_new),
            "stop_m": col(stop_m), "stop_after": col(stop_after), "out_ids": np.full((B, max_out), pad_id, dtype=np.int32)}


def finish_row(st, b, tok, stop_ids, stop_cfg, eos_id, pad_id, max_out, max_ctx):
    """One decode step's bookkeeping of row b once its token is known."""
    was_done = int(st["done"][b])
    n = int(st["n_out"][b])
    budget_n = int(st["max_new"][b])
    if not was_done and n >= budget_n:   # the budget was spent before this step
        was_done = 1
        st["done"][b] = 1
    if not was_done:
        st["ctx_len"][b] += 1            # the token consumed by this step now sits in the cache
    if was_done:
        tok = pad_id
    else:
        if n < max_out:
            st["out_ids"][b, n] = tok
        n += 1
        st["n_out"][b] = n
        budget = n >= budget_n
        stop = False
        n_trig, n_after = int(stop_cfg[0]), int(stop_cfg[1])
        if n_trig > 0:
            aft = int(st["stop_after"][b])
            if aft >= 0:
                aft += 1
            else:
                mp = int(st["stop_m"][b])
                mp = mp + 1 if tok == int(stop_ids[mp]) else (1 if tok == int(stop_ids[0]) else 0)
                if mp == n_trig:
                    aft, mp = 0, 0
                st["stop_m"][b] = mp
            st["stop_after"][b] = aft
            stop = aft >= 0 and aft >= n_after
        if tok == eos_id or budget or stop or int(st["ctx_len"][b]) + 1 >= max_ctx:
            st["done"][b] = 1
    st["cur_tok"][b] = tok


def accept(argmax, ids, cu, state, stop_ids, stop_cfg, eos_id, pad_id, max_ctx):
    """argmax [cu[B]] packed, ids [B][P_max], cu [B + 1] -> (state after, emitted [B], new_ids packed like argmax, -1 where nothing was emitted).
    The input state is left as it is."""
    st = {k: np.array(state[k], dtype=np.int32, copy=True) for k in STATE_KEYS}
    B = len(cu) - 1
    max_out = st["out_ids"].shape[1]
    emitted = np.zeros(B, dtype=np.int32)
    new_ids = np.full(int(cu[B]), -1, dtype=np.int32)
    for b in range(B):
        if st["done"][b]:
            continue                      # a row that is done when the pass starts is left exactly as it is
        start, n = int(cu[b]), int(cu[b + 1] - cu[b])
        i = 0
        while True:
            tok = int(argmax[start + i])
            n0 = int(st["n_out"][b])
            finish_row(st, b, tok, stop_ids, stop_cfg, eos_id, pad_id, max_out, max_ctx)
            if int(st["n_out"][b]) > n0:
                new_ids[start + emitted[b]] = tok
                emitted[b] += 1
            if st["done"][b] or i + 1 >= n or tok != int(ids[b][i + 1]):
                break
            i += 1
    return st, emitted, new_ids
