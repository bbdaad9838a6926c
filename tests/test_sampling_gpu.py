"""Seeded sampling on a real MI355X (include/emmax.h ABI 6: emmax_op_sample, emma-x_amd/csrc/sample.hip): the kernel against the host
reference (tests/sampling_ref.py), on crafted rows, its distribution, its bitwise reproducibility and batch independence, and an external
sampling loop over the tiny model (emmax_last_logits + emmax_set_current_tokens) against the CPU oracle."""
import numpy as np
import pytest
import torch

import sampling_ref as ref

pytestmark = pytest.mark.gpu


def _op_sample(logits, T, k, p, seed, subseq, step):
    from emmax import _lib

    lib = _lib.load()
    B, V = logits.shape
    dev = logits.device
    t = torch.as_tensor(np.asarray(T, dtype=np.float32), device=dev)
    kk = torch.as_tensor(np.asarray(k, dtype=np.int32), device=dev)
    pp = torch.as_tensor(np.asarray(p, dtype=np.float32), device=dev)
    sd = torch.as_tensor(np.asarray(seed, dtype=np.uint64).view(np.int64), device=dev)
    sq = torch.as_tensor(np.asarray(subseq, dtype=np.uint32).view(np.int32), device=dev)
    st = torch.as_tensor(np.asarray(step, dtype=np.int32), device=dev)
    assert all(x.numel() == B for x in (t, kk, pp, sd, sq, st))
    tok = torch.full((B,), -1, dtype=torch.int32, device=dev)
    lp = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    ld = logits.stride(0) if B > 1 else V
    _lib.check(lib.emmax_op_sample(logits.data_ptr(), ld, B, V, t.data_ptr(), kk.data_ptr(), pp.data_ptr(), sd.data_ptr(),
                                   sq.data_ptr(), st.data_ptr(), tok.data_ptr(), lp.data_ptr(), _lib.current_stream()), "emmax_op_sample")
    torch.cuda.synchronize()
    return tok.cpu().numpy(), lp.cpu().numpy()


GRID = [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.9, 20, 0.8), (2.0, 1000, 0.95), (1.0, 1, 1.0), (0.5, 5, 0.3)]


@pytest.mark.parametrize("V,B", [(32064, 1), (32064, 64), (1000, 17), (31, 5)])
def test_kernel_matches_reference(device, V, B):
    rng = np.random.default_rng(V + B)
    l = (rng.standard_normal((B, V)) * 2.5).astype(np.float32)
    x = torch.from_numpy(l).to(device)
    total = cleared = 0
    for gi, (T, k, p) in enumerate(GRID):
        k = min(k, V)
        seeds = [int(s) for s in rng.integers(0, 1 << 63, size=B)]
        subs = list(range(B))
        steps = [int(s) for s in rng.integers(0, 4096, size=B)]
        tok, lp = _op_sample(x, [T] * B, [k] * B, [p] * B, seeds, subs, steps)
        for b in range(B):
            rt, rlp, margin = ref.sample_row(l[b], T, k, p, seeds[b], subs[b], steps[b])
            assert abs(float(lp[b]) - rlp) <= 1e-5, (V, b, T, k, p, lp[b], rlp)
            slack = ref.kept_set(l[b], T, k, p)[2] if T > 0 else np.inf
            total += 1
            if margin > 1e-4 and slack > 1e-6:
                cleared += 1
                assert int(tok[b]) == rt, (V, b, T, k, p, int(tok[b]), rt, margin)
            if T > 0:
                keep = ref.kept_set(l[b], T, k, p)[0]
                assert keep[int(tok[b])]
    assert cleared >= 0.99 * total


def test_kernel_crafted_rows(device):
    V = 1000
    base = np.linspace(-5, 0, V).astype(np.float32)[::-1].copy()   # strictly decreasing: id 0 is the argmax
    # ties at the k-th value are kept: ids 3, 4, 5 share the 4th-largest value -> with k = 4 all three may be drawn
    tie = base.copy()
    tie[3:6] = tie[3]
    seen = set()
    for s in range(64):
        t, _ = _op_sample(torch.from_numpy(np.tile(tie, (8, 1))).to(device), [50.0] * 8, [4] * 8, [1.0] * 8, [s] * 8, list(range(8)), [0] * 8)
        seen |= set(int(v) for v in t)
    assert seen == {0, 1, 2, 3, 4, 5}
    # top-p boundary: masses 0.5, 0.3, 0.2 (rest negligible): p = 0.79 keeps {0, 1}, p = 0.81 keeps {0, 1, 2}
    row = np.full(V, -60.0, dtype=np.float32)
    row[:3] = np.log(np.array([0.5, 0.3, 0.2], dtype=np.float64)).astype(np.float32)
    for p, want in ((0.79, {0, 1}), (0.81, {0, 1, 2})):
        t, _ = _op_sample(torch.from_numpy(np.tile(row, (64, 1))).to(device), [1.0] * 64, [0] * 64, [p] * 64, [7] * 64, list(range(64)), [1] * 64)
        assert set(int(v) for v in t) == want, (p, sorted(set(t.tolist())))
    # top_k = 1 and a tiny top_p give the argmax; T = 0 gives the argmax with the lowest id on ties
    rnd = np.random.default_rng(1).standard_normal(V).astype(np.float32)
    am = int(np.argmax(rnd))
    t, _ = _op_sample(torch.from_numpy(np.tile(rnd, (4, 1))).to(device), [3.0] * 4, [1, 1, 0, 0], [1.0, 1.0, 1e-6, 1e-6], [1, 2, 3, 4], [0] * 4, [0] * 4)
    assert t.tolist() == [am] * 4
    dup = rnd.copy()
    dup[[10, 700]] = rnd.max() + 1.0
    t, _ = _op_sample(torch.from_numpy(dup[None]).to(device), [0.0], [0], [1.0], [0], [0], [0])
    assert int(t[0]) == 10


def test_distribution_chi_square(device):
    from scipy import stats

    rng = np.random.default_rng(5)
    row = (rng.standard_normal(16) * 1.5).astype(np.float32)
    T, k, p = 0.8, 10, 0.9
    keep, z, _ = ref.kept_set(row, T, k, p)
    assert 5 <= keep.sum() <= 10
    N = 100_000
    x = torch.from_numpy(np.tile(row, (N, 1))).to(device)
    tok, _ = _op_sample(x, [T] * N, [k] * N, [p] * N, [0x5EED] * N, list(range(N)), [3] * N)
    assert keep[tok].all(), "a draw outside the kept set"
    pr = np.exp(z.astype(np.float64) - z.max()) * keep
    pr /= pr.sum()
    obs = np.bincount(tok, minlength=16)[keep]
    chi = stats.chisquare(obs, pr[keep] * N)
    assert chi.pvalue > 1e-6, (obs, pr[keep] * N, chi)


def test_kernel_is_bitwise_reproducible(device):
    rng = np.random.default_rng(9)
    l = torch.from_numpy((rng.standard_normal((64, 32064)) * 3).astype(np.float32)).to(device)
    args = ([0.9] * 64, [0, 50] * 32, [0.9, 1.0] * 32, list(range(64)), [3] * 64, [17] * 64)
    a = _op_sample(l, *args)
    b = _op_sample(l, *args)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_rows_are_independent_of_the_batch(device):
    """a row's draw depends on its (logits, parameters, seed, subseq, step) only: the same row alone, or at another place of a 64-row batch"""
    from emmax.sampling import SamplingParams, sample_logits

    rng = np.random.default_rng(13)
    l = torch.from_numpy((rng.standard_normal((64, 32064)) * 3).astype(np.float32)).to(device)
    ps = [SamplingParams(1.2, [0, 50, 200][i % 3], [1.0, 0.9][i % 2], seed=1000 + i) for i in range(64)]
    tok, lp = sample_logits(l, ps, subseqs=list(range(64)), steps=7)
    perm = list(reversed(range(64)))
    tok_r, lp_r = sample_logits(l[perm], [ps[i] for i in perm], subseqs=perm, steps=7)
    for j in (0, 17, 63):
        t1, l1 = sample_logits(l[j:j + 1], ps[j], subseqs=j, steps=7)
        assert int(t1[0]) == int(tok[j]) and float(l1[0]) == float(lp[j])
    assert torch.equal(tok_r.flip(0), tok) and torch.equal(lp_r.flip(0), lp)
    want = torch.log_softmax(l.double(), dim=1).gather(1, tok.long()[:, None])[:, 0]
    assert (lp.double() - want).abs().max().item() < 1e-5


@pytest.mark.parametrize("exact", [False, True])
def test_sampling_loop_on_the_tiny_model_matches_the_oracle(device, exact):
    """prefill, then 24 steps of: logits of the current position (emmax_last_logits) -> sample_logits -> emmax_set_current_tokens -> decode
    step.  The emitted ids are teacher-forced through the fp32 oracle: every step whose perturbed margin clears 2 budget max|logit| / T draws
    the reference sampler's token, the log-probabilities agree within the budget, and at least a quarter of the steps leave the argmax."""
    from conftest import ID_BUDGET_EXACT, ID_BUDGET_TINY
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.sampling import SamplingParams, sample_logits
    from emmax.weights import synthetic_state_dict
    from oracle import emmax_oracle as orc

    cfg = EmmaXConfig.tiny()
    sd = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=6).items()}
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, size=(2, 224, 224, 3), dtype=np.uint8)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=n)] for n in (9, 12)]
    model = EmmaXForActionPrediction(cfg, dict(sd)).to(device, max_batch=2, max_prompt=24, exact=exact)
    eng = model.engine
    B, n_steps = 2, 24
    budget = ID_BUDGET_EXACT if exact else ID_BUDGET_TINY
    model._prefill(rows, frames_u8=torch.from_numpy(frames).to(device), max_new=n_steps + 2)
    first = eng.last_logits()[:B].float()
    top = torch.topk(first[0], 20).values
    T = float((top[0] - top[19]) / 3.0)            # from the data: steps far from one-hot
    params = SamplingParams(T, 0, 1.0)
    seed = 4242
    got = [[] for _ in range(B)]
    lps = [[] for _ in range(B)]
    for t in range(n_steps):
        logits = eng.last_logits()[:B].float().contiguous()
        tok, lp = sample_logits(logits, params, seeds=seed, subseqs=list(range(B)), steps=t)
        for b in range(B):
            got[b].append(int(tok[b]))
            lps[b].append(float(lp[b]))
        eng.set_current_tokens(tok.tolist())
        eng.decode_step()
    sd_ref = {k: v.float() for k, v in sd.items()}
    required = nonargmax = steps = 0
    for b in range(B):
        logits, _, _ = orc.vla_prefill_logits(torch.tensor([rows[b] + got[b]]), orc.preprocess_frames(frames[b:b + 1], cfg), sd_ref, cfg)
        L = logits[0, -len(got[b]) - 1:-1].float().numpy()
        for t, tok in enumerate(got[b]):
            rt, rlp, margin = ref.sample_row(L[t], T, 0, 1.0, seed, b, t)
            line = 2 * budget * np.abs(L[t]).max()
            steps += 1
            nonargmax += int(tok != int(np.argmax(L[t])))
            assert abs(lps[b][t] - rlp) <= line, (exact, b, t, lps[b][t], rlp)
            if margin > line / T:
                required += 1
                assert tok == rt, (exact, b, t, tok, rt, margin)
    assert required >= steps // 4 and nonargmax >= steps // 4, (required, nonargmax, steps)
