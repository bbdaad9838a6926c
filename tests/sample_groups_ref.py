"""What the sample-group tests share (no GPU needed to import): the pinned inputs, per-row sampling parameters and seeds of every case whose
GPU test asserts that the rows of a group DIVERGE, and the check that makes that a property of the inputs -- tests/test_sample_groups.py
runs it on the CPU with the fp32 oracle and tests/sampling_ref.py; tests/test_sample_groups_gpu.py only uses the cases.

A case is (prompt lengths, N, per-row (temperature factor, top_k, top_p), seed): G = len(prompt lengths) prompts of the tiny configuration
(weights seed 6, 256 patch rows), row g N + j drawing with (seed, subseq g N + j).  The temperature is the factor times
T0 = (top1 - top20) / 3 of the oracle's first row, as test_sampled_generate_matches_the_oracle takes it.

The pinned property (diverge): in every group, the step-0 reference draws that are CLEAR -- Gumbel margin and kept-set slack above
2 ID_BUDGET_TINY max|logit| / T, so a device within the budget must draw the same token -- hold at least two distinct tokens.  Draws that are
not clear (a top-p row on this nearly flat model never is: some token's mass always sits next to the boundary) are not counted."""
import numpy as np

WEIGHT_SEED = 6
# factor 0 = greedy (the row that must equal a plain one-row greedy run)
MIXED = [(0.0, 0, 1.0), (1.0, 0, 1.0), (1.3, 50, 1.0), (0.8, 20, 1.0), (1.0, 0, 0.9), (1.6, 0, 1.0)]
PLAIN = [(1.0, 0, 1.0)]

CASES = {
    # name: (input seed, prompt lengths, N, per-row grid (cycled over the G N rows), sampling seed)
    "mixed": (5, (14, 9), 3, MIXED, 101),          # tests 1, 4 (fp8 weights, fp8 cache) and 5
    "cross": (50, (50, 50), 3, PLAIN, 211),        # test 2: crosses a page boundary while generating
    "ctx64": (50, (64, 64), 3, PLAIN, 212),        # ... context % 64 == 0: no copy
    "ctx63": (50, (63, 63), 3, PLAIN, 213),
    "long": (50, (20,), 2, PLAIN, 214),            # ... 136 new tokens: two pages per row
    "private": (61, (40,), 2, PLAIN, 216),         # test 3: context 296, 70 tokens
    "indep": (81, (12, 17, 9), 2, PLAIN, 218),     # test 5: three groups, each also run alone
}


# T0 of every case: (top1 - top20) / 3 of the fp32 oracle's first row (tests/test_sample_groups.py recomputes them), kept here so that the GPU
# tests do not run the oracle's vision towers for a constant
T0 = {"mixed": 0.11287307739257812, "cross": 0.10012022405862808, "ctx64": 0.09057283401489258, "ctx63": 0.07608278840780258,
      "long": 0.08859805017709732, "private": 0.10060397535562515, "indep": 0.11376607418060303}


def inputs(name):
    """(frames uint8 [G, 224, 224, 3], prompt rows) of a case: the generator of the beam tests' _inputs."""
    seed, lens = CASES[name][0], CASES[name][1]
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(len(lens), 224, 224, 3), dtype=np.uint8)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=n - 1)] for n in lens]
    return frames, rows


def row_grid(name):
    """[(temperature factor, top_k, top_p)] of the G N rows of a case."""
    _, lens, N, grid, _ = CASES[name]
    return [grid[r % len(grid)] for r in range(len(lens) * N)]


def params(name):
    """The SamplingParams of the G N rows (row r draws with subseq r, the default)."""
    from emmax.sampling import SamplingParams

    seed = CASES[name][4]
    return [SamplingParams(f * T0[name], k, p, seed=seed) for f, k, p in row_grid(name)]


def first_rows(name, cfg, sd_ref):
    """The oracle's fp32 logit row behind every prompt of a case, [G, vocab]."""
    import torch
    from oracle import emmax_oracle as orc

    frames, rows = inputs(name)
    out = []
    for g, r in enumerate(rows):
        logits, _, _ = orc.vla_prefill_logits(torch.tensor([r]), orc.preprocess_frames(frames[g: g + 1], cfg), sd_ref, cfg)
        out.append(logits[0, -1].float().numpy())
    return np.stack(out)


def temperature(row0):
    """T0 from the oracle's first row of a case: (top1 - top20) / 3."""
    top = np.sort(np.asarray(row0, dtype=np.float32))[::-1]
    return float((top[0] - top[19]) / np.float32(3.0))


def diverge(draws):
    """The pinned property over step0_draws' result."""
    return all(len({tok for tok, clear in grp if clear}) >= 2 for grp in draws)


def step0_draws(name, L, budget):
    """The reference draws of every row at step 0 over the groups' oracle rows L [G, vocab]: a list per group of (token, clear) with clear =
    the draw's Gumbel margin and kept-set slack are both above 2 budget max|logit| / T (a greedy row: its top-2 logit gap above
    2 budget max|logit|)."""
    import sampling_ref as ref

    _, lens, N, _, seed = CASES[name]
    out = []
    for g in range(len(lens)):
        line = 2 * budget * float(np.abs(L[g]).max())
        grp = []
        for j in range(N):
            r = g * N + j
            f, k, p = row_grid(name)[r]
            if f == 0.0:
                top = np.sort(L[g])[::-1]
                grp.append((int(np.argmax(L[g])), bool(top[0] - top[1] > line)))
                continue
            T = f * T0[name]
            tok, _, margin = ref.sample_row(L[g], T, k, p, seed, r, 0)
            grp.append((tok, bool(margin > line / T and ref.kept_set(L[g], T, k, p)[2] > line / T)))
        out.append(grp)
    return out
