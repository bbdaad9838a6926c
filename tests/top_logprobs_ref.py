"""Host reference of the top-N and watched-token log-probabilities (include/emmax.h: emmax_op_top_logprobs; the kernel:
emma-x_amd/csrc/sample.hip).  float64 log_softmax of the raw row; the order is (fp32 value descending, id ascending) over the entries that
are not NaN; places past them hold (-1, -inf); a row that holds a NaN has NaN for every entry's log-probability."""
import numpy as np

MAX_TOP = 20      # EMMAX_MAX_TOP_LOGPROBS
MAX_WATCH = 256   # EMMAX_MAX_WATCH_IDS


def log_softmax64(row):
    """float64 log_softmax of an fp32 row: NaN everywhere when the row holds a NaN (or no finite maximum)."""
    x = np.asarray(row, dtype=np.float32).astype(np.float64)
    if np.isnan(x).any():
        return np.full(x.shape, np.nan)
    m = x.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return x - (m + np.log(np.exp(x - m).sum()))


def top_order(row):
    """ids of the entries that are not NaN, by (fp32 value descending, id ascending); -0 and +0 are one value."""
    x = np.asarray(row, dtype=np.float32)
    ids = np.nonzero(~np.isnan(x))[0]
    # lexsort: last key first; -x puts the larger value first, equal values keep the lower id first
    return ids[np.lexsort((ids, -(x[ids].astype(np.float64) + 0.0)))]


def top_row(row, n):
    """(ids int32 [n], log-probabilities float64 [n]) of one row."""
    order = top_order(row)[:n]
    lp = log_softmax64(row)
    ids = np.full(n, -1, dtype=np.int32)
    out = np.full(n, -np.inf, dtype=np.float64)
    ids[: len(order)] = order
    out[: len(order)] = lp[order]
    return ids, out


def watch_row(row, watch_ids):
    return log_softmax64(row)[np.asarray(list(watch_ids), dtype=np.int64)] if len(watch_ids) else np.zeros(0)


def top_rows(rows, n, watch_ids=()):
    """(ids [B, n], log-probabilities [B, n], watched log-probabilities [B, W]) of every row."""
    rows = np.asarray(rows, dtype=np.float32)
    t = [top_row(r, n) for r in rows]
    return (np.stack([a for a, _ in t]), np.stack([b for _, b in t]), np.stack([watch_row(r, watch_ids) for r in rows]))


def close(got, want, tol):
    """got (fp32) against want (float64): NaN where want is NaN, the same infinity where want is infinite, else within tol."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan, inf = np.isnan(want), np.isinf(want)
    fin = ~nan & ~inf
    return bool(np.isnan(got[nan]).all() and (got[inf] == want[inf]).all() and (np.abs(got[fin] - want[fin]) <= tol).all())


def same_bits(a, b):
    """bit-for-bit equality of two fp32 arrays, every NaN counting as one value"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())
