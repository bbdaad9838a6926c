"""What the slot-group tests share (no GPU needed to import): the pinned inputs of tests/test_slot_groups_gpu.py, and the checks that make
"the samples of a group diverged" and "at least half of the emitted steps are compared" properties of those inputs --
tests/test_slot_groups.py runs them on the CPU with the fp32 oracle and tests/sampling_ref.py.

FORK: the engine-level cases.  Each is group 0 of a case of tests/sample_groups_ref.py (tiny configuration, weights seed 6, 256 patch rows):
the first prompt of that case, its temperature and seed, sample j drawing with (seed, subseq j) -- which is what rows 0 .. N - 1 of that case
draw with, so its pinned step-0 property covers this group.  The value is the number of decode steps the GPU tests run.

WORKLOAD: the scheduler-level requests -- (prompt length, num_samples, (temperature, top_k, top_p) or None = greedy, token budget), request i
with input seed 700 + i and sampling seed 1300 + i."""
import numpy as np

import sample_groups_ref as sg

WEIGHT_SEED = sg.WEIGHT_SEED
N = 3
FORK = {"ctx64": 8, "ctx63": 8, "cross": 24}   # (256 + prompt) % 64 = 0 (no copy), 63, 50 (24 tokens: the followers grow onto their own pages)

WORKLOAD = [
    (9, 2, (1.0, 50, 1.0), 14),
    (14, 1, None, 12),
    (7, 3, (0.8, 0, 0.9), 18),
    (12, 1, (1.0, 0, 1.0), 10),
    (17, 1, None, 16),
    (6, 3, (1.2, 40, 1.0), 11),
    (11, 2, (0.7, 0, 1.0), 20),
    (15, 1, (1.0, 50, 0.9), 13),
    (8, 2, (1.0, 0, 1.0), 9),
    (10, 1, None, 15),
]
INPUT_SEED, SAMPLING_SEED = 700, 1300


def fork_inputs(name):
    """(frame uint8 [1, 224, 224, 3], prompt ids, SamplingParams) of an engine-level case."""
    frames, rows = sg.inputs(name)
    return frames[:1], rows[0], sg.params(name)[0]


def fork_step0(name, cfg, sd_ref, budget):
    """[(token, clear)] of the N samples at step 0 by the fp32 oracle (sample_groups_ref.step0_draws, group 0)."""
    L = sg.first_rows(name, cfg, sd_ref)
    return sg.step0_draws(name, L, budget)[0]


def workload():
    """[(frame uint8 [1, 224, 224, 3], prompt ids, num_samples, SamplingParams or None, budget)]"""
    from emmax.sampling import SamplingParams

    out = []
    for i, (n, k, p, budget) in enumerate(WORKLOAD):
        rng = np.random.default_rng(INPUT_SEED + i)
        frame = rng.integers(0, 256, size=(1, 224, 224, 3), dtype=np.uint8)
        row = [1] + [int(x) for x in rng.integers(3, 31744, size=n - 1)]
        out.append((frame, row, k, None if p is None else SamplingParams(p[0], p[1], p[2], seed=SAMPLING_SEED + i), budget))
    return out


def clear_steps(L, ids, p, subseq, budget):
    """How many leading steps of a chain are REQUIRED to match: up to the first step whose reference draw over the oracle's row L[t] has a
    Gumbel margin or a kept-set slack at or below 2 budget max|logit| / T (a greedy chain: a top-2 gap at or below 2 budget max|logit|) --
    the rule of test_exact_numerics_batch_position_does_not_matter."""
    import sampling_ref as ref

    for t in range(len(ids)):
        amax = float(np.abs(L[t]).max())
        if p is None or p.temperature == 0.0:
            top = np.sort(L[t])[::-1]
            if top[0] - top[1] <= 2 * budget * amax:
                return t
            continue
        _, _, margin = ref.sample_row(L[t], p.temperature, p.top_k, p.top_p, p.seed, subseq, t)
        line = 2 * budget * amax / p.temperature
        if margin <= line or ref.kept_set(L[t], p.temperature, p.top_k, p.top_p)[2] <= line:
            return t
    return len(ids)


def oracle_chain(orc, cfg, sd_ref, patches, row, p, subseq, budget_tokens):
    """The fp32 oracle's own chain of one sample: (ids, logit rows [len(ids), vocab]) -- the reference draw of tests/sampling_ref.py at every
    step over a KV-cached forward, ended by EOS or the token budget as a slot ends."""
    import sampling_ref as ref
    import torch

    ids_t = torch.tensor([row], dtype=torch.long)
    logits, cache = orc.llama_forward(orc.splice(ids_t, patches, sd_ref), sd_ref, cfg.llm, None, last_only=True)
    ids, rows = [], []
    for t in range(budget_tokens):
        l = logits[0, -1].float().numpy()
        rows.append(l)
        tok = int(np.argmax(l)) if p is None or p.temperature == 0.0 else ref.sample_row(l, p.temperature, p.top_k, p.top_p, p.seed, subseq, t)[0]
        ids.append(tok)
        if tok == cfg.eos_token_id or t + 1 == budget_tokens:
            break
        logits, cache = orc.llama_forward(orc.embed_tokens(torch.tensor([[tok]]), sd_ref), sd_ref, cfg.llm, cache, last_only=True)
    return ids, np.stack(rows)


def oracle_patches(orc, cfg, sd_ref, frame):
    return orc.projector(orc.vision_backbone(orc.preprocess_frames(frame, cfg), sd_ref, cfg), sd_ref)
