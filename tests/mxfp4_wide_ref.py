"""References, inputs and tolerances of tests/test_mxfp4_wide_gpu.py and tests/test_mxfp4_wide_ref.py: MXFP4 decode weights at 17-64 rows (tuning
switch mx4_wide, decode_kmp.hip's MX4 form).  TEST INFRASTRUCTURE ONLY (plain torch on the CPU); the format, the de-quantiser and the float64
stage references are tests/mxfp4_ref.py's and tests/decode_stage_ref.py's, by import.

  * the stage models: W4 of tests/mxfp4_ref.py (hidden 1024: one load step of 128 k per wave; intermediate 4224 = 33 steps: the eleven-phase down
    form, wave 0 owns five steps) and T4 (hidden 4096, intermediate 6272, ONE layer, vocabulary 12320): 784 gate/up tiles and 770 lm-head tiles are
    four per block (TMAX 6), K = 4096 is four phases per wave at 17-32 rows and eight at 33-64 -- the many-tile rings that hidden 1024 cannot reach;
  * their inputs: the GPU tests stage ROWS rows and use the first B, and so does the measurement here;
  * the tolerance table for the new batches, by the project's rule (decode_stage_ref.py): atol_frac = max(4e-3, 2 x SPREAD), TOL = max(1e-2, 2 x REL),
    SPREAD / REL of the fp32 "mirror" emulation against the float64 reference, both on the de-quantised weights, worst over exactly the
    (model, batch, layer) inputs of the GPU tests.  Reference against reference: no number comes from a kernel (`python tests/mxfp4_wide_ref.py`
    prints the measurement, tests/test_mxfp4_wide_ref.py re-checks it);
  * the end-to-end configuration (the W4 shape with the tiny towers), its planted, random and slot-serving inputs, and a batched oracle trace (rows of
    one prompt length run through the fp32 oracle's own prefill and decoder stack together).
"""

import functools

import numpy as np
import torch

import decode_stage_ref as R
import mxfp4_ref as M

ROWS = 64                                   # rows every stage engine stages (max_batch); a test of B rows uses the first B
T4_HIDDEN, T4_INTER, T4_VOCAB = 4096, 6272, 12320
MODELS = {"W4": dict(hidden=M.HIDDEN4, inter=M.INTER4, vocab=R.VOCAB, layers=R.LAYERS, heads=(32, 32)),
          "T4": dict(hidden=T4_HIDDEN, inter=T4_INTER, vocab=T4_VOCAB, layers=1, heads=(32, 32))}
# W4: 17 and 32 (two batch tiles, the second partly / wholly filled), 33 and 64 (two halves; down and lm-head as 32 + 1 and 32 + 32), 40 = 32 + 8
# (the tail chunk of down / lm-head is an 8-row decode_km.hip launch)
BATCHES = {"W4": [17, 32, 33, 40, 64], "T4": [32, 64]}
# T4 runs the stages whose rings hidden 1024 cannot fill: qkv / gate-up / lm-head at 32 rows, qkv / gate-up at 64
T4_STAGES = {32: ("qkv", "gateup", "lmhead"), 64: ("qkv", "gateup")}
OUTPUTS = ("q", "k", "v", "gateup", "oproj", "down", "lmhead")   # (no split partials above 8 rows: decode_batch_served)


def make_cfg(model):
    from emmax.config import EmmaXConfig

    d = MODELS[model]
    cfg = EmmaXConfig.tiny()
    L = cfg.llm
    L.intermediate_size, L.num_layers, L.head_dim, L.vocab_size, L.hidden_size = d["inter"], d["layers"], R.HEAD_DIM, d["vocab"], d["hidden"]
    L.num_heads, L.num_kv_heads = d["heads"]
    cfg.decode_weight_dtype = "mxfp4"
    return cfg


@functools.lru_cache(maxsize=None)
def make_state_dict(model, seed=3):
    from emmax.weights import synthetic_state_dict

    if model == "W4":
        return M.make_state_dict4("W4", seed)
    return {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(make_cfg(model), seed=seed).items()}


class WeightsW(M.Weights4):
    """Weights4 that can forget: T4's float64 matrices are 0.2-0.4 GB each, built per stage and dropped"""

    def drop(self):
        self.cache.clear()


def hidden_rows(model, seed, scale=1.0):
    return R.hidden_rows(ROWS, seed, scale, MODELS[model]["hidden"])


def act_rows(model, seed):
    """the SwiGLU rows of the down projection, ROWS of them (both intermediate sizes are their own padded width)"""
    return R.bf(torch.randn(ROWS, MODELS[model]["inter"], generator=R.gen(23, seed)))


def attn_rows(model, seed):
    return R.attn_rows(ROWS, MODELS[model]["heads"][0] * R.HEAD_DIM, seed)


# ---- tolerances ------------------------------------------------------------------------------------------------------------------------------
# (o-proj and down take bf16 rows as they are: only the fp32 summation order differs, padded to 1e-7; the floors 4e-3 / 1e-2 bind there)
SPREAD_W = {"q": 1.11e-2, "k": 1.30e-2, "v": 9.97e-3, "gateup": 5.13e-2, "oproj": 1.0e-7, "down": 1.0e-7, "lmhead": 1.06e-2}
REL_W = {"q": 5.99e-3, "k": 6.79e-3, "v": 4.00e-3, "gateup": 4.63e-3, "oproj": 1.66e-7, "down": 1.56e-7, "lmhead": 2.59e-3}


def tolerances(out):
    """(rtol, atol_frac, TOL) of output `out`"""
    return R.RTOL, max(4e-3, 2.0 * SPREAD_W[out]), max(1e-2, 2.0 * REL_W[out])


def measure(quiet=False, models=("W4", "T4")):
    worst = {k: 0.0 for k in OUTPUTS}
    rel = {k: 0.0 for k in OUTPUTS}

    def note(name, e, r):
        worst[name] = max(worst[name], R.spread(e, r, R.RTOL))
        rel[name] = max(rel[name], ((e.double() - r.double()).abs().max() / r.double().abs().max()).item())

    for model in models:
        W = WeightsW(make_state_dict(model), make_cfg(model))
        for B in BATCHES[model]:
            stages = T4_STAGES[B] if model == "T4" else ("qkv", "gateup", "oproj", "down", "lmhead")
            for li in range(MODELS[model]["layers"]):
                h32 = hidden_rows(model, (B, li))[0][:B]
                if "qkv" in stages:
                    ctx = R.ctx_rows(B, li)
                    for name, e, r in zip("qkv", R.emu_qkv(W, li, h32, ctx, "mirror"), R.ref_qkv(W, li, h32, ctx)):
                        note(name, e, r)
                if "gateup" in stages:
                    h3 = hidden_rows(model, (B, li, 3))[0][:B]
                    note("gateup", R.emu_gateup(W, li, h3, "mirror"), R.ref_gateup(W, li, h3))
                if "oproj" in stages:
                    x = attn_rows(model, (B, li))[:B]
                    note("oproj", R.emu_oproj(W, li, x), R.ref_oproj(W, li, x))
                if "down" in stages:
                    a = act_rows(model, (B, li))[:B]
                    note("down", M.emu_down4(W, li, a), M.ref_down4(W, li, a))
            if "lmhead" in stages:
                h32 = hidden_rows(model, (B, 99))[0][:B]
                note("lmhead", R.emu_lmhead(W, h32, "mirror"), R.ref_lmhead(W, h32))
        W.drop()
    if not quiet:
        print("mxfp4-wide spread " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        print("mxfp4-wide relerr " + "  ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    return worst, rel


# ---- end to end: the W4 shape with the tiny towers -------------------------------------------------------------------------------------------
E2E_MAX_BATCH = 40
E2E_B = 40                          # rows of the teacher-forced random-weight test
E2E_STEPS = M.E2E_STEPS             # 16
E2E_PROMPT = 14                     # one prompt length: the 40 rows go through the oracle's prefill and decoder stack together
E2E_PLANTED_SEED = 5
# picked on the CPU (`python tests/mxfp4_wide_ref.py`; seeds 21-24 give 640, 274, 491, 350 pairs above the line): 22 -- at least a quarter of the
# pairs clear the line, and most of the others sit near it, where an error past the budget shows first
E2E_RANDOM_SEED = 22
# (row, step) pairs of the E2E_B x E2E_STEPS teacher-forced steps whose oracle margin clears above_id_line(ref, ID_BUDGET_SHALLOW), counted with the
# CPU oracle on the de-quantised weights
E2E_ABOVE_LINE = 274
# planted weights: a ragged batch of 24 -- four prompt lengths, ordinary steps 0..9 before the action prefix
PLANTED_B = 24
PLANTED_LENS = [5, 12, 17, 30]
PLANTED_MAX_NEW = 24
# slot serving: 24 slots, 40 ragged requests on the planted model
SLOTS, REQUESTS = 24, 40


def e2e_cfg():
    return make_cfg("W4")


@functools.lru_cache(maxsize=None)
def e2e_state_dict(planted, seed):
    from emmax.weights import synthetic_state_dict

    return {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(e2e_cfg(), seed=seed, planted=planted).items()}


def planted_batch(cfg, n=PLANTED_B, seed=91):
    """(frames, rows, steps): n rows of ragged lengths whose last token starts a planted chain of steps[b] ordinary steps + 8 actions + EOS"""
    from emmax.weights import planted_start_token

    lens = [PLANTED_LENS[(b * 7 + b // 4) % len(PLANTED_LENS)] for b in range(n)]
    steps = [(3 * b + 1) % 10 for b in range(n)]
    frames, rows = M.e2e_inputs(n, lens, seed=seed, last=[planted_start_token(cfg, k) for k in steps])
    return frames, rows, steps


def serving_requests(cfg, n=REQUESTS, seed=133):
    """n ragged planted requests: (frames [n], rows, max_new per request)"""
    frames, rows, steps = planted_batch(cfg, n, seed)
    return frames, rows, [min(PLANTED_MAX_NEW, 4 + (5 * i) % 21) for i in range(n)]


def oracle_trace_batch(cfg, sd_ref, frames, rows, T, keep_logits=True):
    """greedy ids [B][T] and per-step last-position logits [B][T][V] of rows of ONE prompt length over T steps (step 0 from the prefill): the
    fp32 oracle's own prefill and decoder stack (oracle/emmax_oracle.py) on `sd_ref`, every row attending to itself alone; no stop at EOS"""
    from oracle import emmax_oracle as orc

    assert len({len(r) for r in rows}) == 1
    with torch.inference_mode():
        ids = torch.tensor(rows)
        proj = orc.projector(orc.vision_backbone(orc.preprocess_frames(frames, cfg), sd_ref, cfg, torch.float32), sd_ref, torch.float32)
        logits, cache = orc.llama_forward(orc.splice(ids, proj, sd_ref, torch.float32), sd_ref, cfg.llm, None, torch.float32, last_only=True)
        gens, trace = [], []
        for _ in range(T):
            last = logits[:, -1].float()
            if keep_logits:
                trace.append(last.clone())
            nxt = last.argmax(-1)
            gens.append(nxt)
            logits, cache = orc.llama_forward(orc.embed_tokens(nxt[:, None], sd_ref, torch.float32), sd_ref, cfg.llm, cache, torch.float32)
    gens = torch.stack(gens, 1).tolist()
    return gens, (torch.stack(trace, 1) if keep_logits else None)


def planted_oracle(cfg, sd_q, frames, rows, T=PLANTED_MAX_NEW):
    """the oracle's greedy ids of ragged rows: one batched trace per prompt length"""
    out = [None] * len(rows)
    for n in sorted({len(r) for r in rows}):
        sel = [i for i, r in enumerate(rows) if len(r) == n]
        gens, _ = oracle_trace_batch(cfg, sd_q, frames[sel], [rows[i] for i in sel], T, keep_logits=False)
        for i, g in zip(sel, gens):
            out[i] = g
    return out


def random_e2e_inputs():
    return M.e2e_inputs(E2E_B, E2E_PROMPT, seed=2025)


def count_above_line(traces, budget):
    from conftest import above_id_line

    return sum(int(above_id_line(traces[b, t], budget)) for b in range(traces.shape[0]) for t in range(traces.shape[1]))


if __name__ == "__main__":
    import os
    import sys
    import time

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "emma-x_amd"), os.path.join(root, "tests")]
    torch.set_num_threads(8)
    t0 = time.time()
    measure()
    print(f"measure: {time.time() - t0:.1f} s")
    from conftest import ID_BUDGET_SHALLOW

    cfg = e2e_cfg()
    frames, rows = random_e2e_inputs()
    for seed in (21, 22, 23, 24):
        t0 = time.time()
        sd_q = M.dequant_state_dict(e2e_state_dict(False, seed))
        _, tr = oracle_trace_batch(cfg, sd_q, frames, rows, E2E_STEPS)
        print(f"seed {seed}: pairs above the id line {count_above_line(tr, ID_BUDGET_SHALLOW)} of {E2E_B * E2E_STEPS} ({time.time() - t0:.1f} s)")
