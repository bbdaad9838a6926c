"""Host reference of the logits processors of the decode step (include/emmax.h ABI 8: emmax_session_set_processing; the processing
finish in emma-x_amd/csrc/sample.hip) and of HF's post-warper scores.  All arithmetic is float32, as the device does it: the penalty is
rounded to float32 and division is correctly rounded, so a processed row is bit-exact against the device's."""
import numpy as np

import sampling_ref


def banned_ngram_ids(hist, n):
    """Ids that would complete an n-gram already in `hist` (HF NoRepeatNGramLogitsProcessor): the n-grams whose first n - 1 ids equal
    the last n - 1 ids of the history."""
    hist = [int(x) for x in hist]
    L = len(hist)
    if n <= 0 or L < n:
        return set()
    key = hist[L - n + 1:]
    return {hist[j + n - 1] for j in range(L - n + 1) if hist[j:j + n - 1] == key}


def process_row(logits, hist, n_out, penalty=1.0, ngram=0, min_new=0, eos_id=2):
    """One fp32 logit row through repetition penalty, n-gram ban and min-new-tokens EOS ban, in HF's order.  hist = the row's prompt ids
    followed by its n_out emitted ids."""
    x = np.array(logits, dtype=np.float32, copy=True)
    V = x.shape[0]
    p = np.float32(penalty)
    if p != np.float32(1.0):
        ids = np.unique(np.asarray([i for i in hist if 0 <= int(i) < V], dtype=np.int64))
        v = x[ids]
        x[ids] = np.where(v < 0, v * p, v / p).astype(np.float32)
    for i in banned_ngram_ids(hist, ngram):
        if 0 <= i < V:
            x[i] = -np.inf
    if n_out < min_new and 0 <= eos_id < V:
        x[eos_id] = -np.inf
    return x


def scores_row(processed, T=0.0, top_k=0, top_p=1.0):
    """HF `scores` of a row: the processed row when greedy; z / T on the kept set and -inf elsewhere when sampling."""
    processed = np.asarray(processed, dtype=np.float32)
    if not T > 0:
        return processed.copy()
    keep, z, _ = sampling_ref.kept_set(processed, T, top_k, top_p)
    return np.where(keep, z, np.float32(-np.inf)).astype(np.float32)


def greedy(processed):
    """The argmax of a processed row, lowest id on ties; -1 when no finite entry is left (the row emits pad and is done)."""
    processed = np.asarray(processed, dtype=np.float32)
    if not (processed > -np.inf).any():
        return -1
    return int(np.argmax(processed))
