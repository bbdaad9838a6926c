"""GPU: scoring through the session (emmax_prefill_score) and the Python layers on top -- engine.score, forward(labels=...), score(...).

EmmaXConfig.tiny(), planted weights, ragged B = 3 prompts.
  (a) against the session's own materialised logits (emmax_prefill_logits reduced in float64: the same operands, another fp32 summation order);
  (b) against the CPU oracle at the line tests/test_e2e_gpu.py draws for a forward's logits (|lse(a) - lse(b)| <= max |a - b| carries it over);
  (c) every branch: multimodal from frames and from pixel_values, language-only, extensions, the fp8 KV cache, fp8 / MXFP4 decode weights, resid32;
  (d) a score between a prefill and what follows changes nothing; (e) the losses; (f) no logits are allocated.
"""

import math

import numpy as np
import pytest
import torch

import mxfp4_ref as M4
import score_ref as S
from conftest import GOLDEN, ID_BUDGET_TINY, above_id_line
from test_e2e_gpu import FEAT_TOL, _inputs, _mk

pytestmark = pytest.mark.gpu

P_LENS = [20, 9, 33]
SEED = 5          # synthetic_state_dict seed (the wrapper golden's)
N_STEPS, X_LENS = 3, [12, 2, 7]
# (a): two fp32 evaluations of the same operands at K = 256, each within FACTOR x SPREAD of float64
OWN = {k: 2.0 * S.FACTOR * v for k, v in S.SPREAD[256]["random"].items()}


def _targets(rows, n_patches=0, new_rows_only=False, vocab=None):
    from emmax.scoring import targets_for

    return targets_for(None, rows, n_patches=n_patches, new_rows_only=new_rows_only, vocab=vocab)


def _stats64(logits, tg):
    """float64 (lse, target logit -- 0 where not scored --, argmax) of one sequence's logit rows"""
    z = logits.double().cpu()
    t = torch.tensor(tg)
    ok = t != -100
    tl = torch.where(ok, z.gather(1, t.clamp_min(0)[:, None])[:, 0], torch.zeros(len(tg), dtype=torch.float64))
    return torch.logsumexp(z, -1), tl, z.argmax(-1)


def _loss64(ref_rows, targets):
    tot, n = 0.0, 0
    for z, tg in zip(ref_rows, targets):
        lse, tl, _ = _stats64(z, tg)
        ok = torch.tensor(tg) != -100
        tot -= (tl - lse)[ok].sum().item()
        n += int(ok.sum())
    return tot / n


def _check_own(eng, got, targets, what):
    """(a): engine.score's three lists against the session's own emmax_prefill_logits, per row in the row's max |logit|"""
    worst = {"lse": 0.0, "logit": 0.0}
    for b, z in enumerate(eng.prefill_logits()):
        lse, tl, am = _stats64(z, targets[b])
        unit = z.double().abs().amax(-1).cpu()
        worst["lse"] = max(worst["lse"], ((got[0][b].double().cpu() - lse).abs() / unit).max().item())
        worst["logit"] = max(worst["logit"], ((got[1][b].double().cpu() - tl).abs() / unit).max().item())
        top2 = z.double().cpu().topk(2, -1).values
        clear = (top2[:, 0] - top2[:, 1]) / unit > 2.0 * OWN["logit"]
        assert torch.equal(got[2][b].cpu().long()[clear], am[clear]), (what, b)
        assert bool(clear.float().mean() > 0.5), (what, b)
    print(f"{what}: against the session's own logits: lse {worst['lse']:.3g} / {OWN['lse']:.3g}  logit {worst['logit']:.3g} / {OWN['logit']:.3g}")
    assert worst["lse"] <= OWN["lse"] and worst["logit"] <= OWN["logit"], (what, worst)


def _check_oracle(got, ref_rows, targets, what):
    """(b): lse / target logit within FEAT_TOL of the sequence's max |logit_ref|; ids equal above the a-priori id line; half the rows clear it"""
    worst, clear, total = 0.0, 0, 0
    for b, ref in enumerate(ref_rows):
        lse, tl, am = _stats64(ref, targets[b])
        unit = ref.abs().max().item()
        assert got[0][b].shape == lse.shape, (what, b, got[0][b].shape, lse.shape)
        worst = max(worst, (got[0][b].double().cpu() - lse).abs().max().item() / unit, (got[1][b].double().cpu() - tl).abs().max().item() / unit)
        ids = got[2][b].cpu().long()
        for r in range(ref.shape[0]):
            if above_id_line(ref[r], ID_BUDGET_TINY):
                clear += 1
                assert int(ids[r]) == int(am[r]), (what, b, r)
        total += ref.shape[0]
    print(f"{what}: against the oracle: worst {worst:.4f} of max|logit|, {clear} of {total} rows above the id line")
    assert worst <= FEAT_TOL, (what, worst)
    assert 2 * clear >= total, (what, clear, total)


def _as_lists(out):
    return [[x for x in t] if not isinstance(t, list) else t for t in (out.lse, out.token_logprobs, out.predicted_ids)]


def _got_from_output(out, targets):
    """EmmaXScoreOutput -> (lse, target logit, argmax) lists: the target logit is token_logprobs + lse where a row was scored"""
    lse, lp, am = _as_lists(out)
    tl = [torch.where(torch.tensor(t).to(l.device) != -100, p + l, torch.zeros_like(l)) for p, l, t in zip(lp, lse, targets)]
    for p, t in zip(lp, targets):
        assert torch.equal(torch.isnan(p).cpu(), torch.tensor(t) == -100)   # NaN exactly where nothing was scored
    return lse, tl, am


def _oracle_mm(cfg, sd_ref, frames, rows):
    from oracle import emmax_oracle as orc

    with torch.inference_mode():
        return [orc.vla_prefill_logits(torch.tensor([r]), orc.preprocess_frames(frames[b:b + 1], cfg), sd_ref, cfg)[0][0].float() for b, r in enumerate(rows)]


@pytest.fixture(scope="module")
def planted(device):
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny()
    model, sd_ref = _mk(cfg, SEED, True, device, max_batch=3, max_prompt=128, max_ctx=448)
    frames, full = _inputs(cfg, 3, [p + N_STEPS + x for p, x in zip(P_LENS, X_LENS)], seed=77)
    yield cfg, model, sd_ref, frames, full, _oracle_mm(cfg, sd_ref, frames, full)
    model.engine.close()


@pytest.mark.parametrize("resid32", [0, 1])
@pytest.mark.parametrize("images", ["frames_u8", "pixel_values"])
def test_multimodal_score(device, planted, tune, images, resid32):
    from oracle import emmax_oracle as orc

    cfg, model, sd_ref, frames, full, ref_full = planted
    tune(resid32=resid32)
    rows = [r[:p] for r, p in zip(full, P_LENS)]
    ref = [z[: cfg.n_patches + p] for z, p in zip(ref_full, P_LENS)]   # (causal: a prefix's rows are the whole sequence's first rows)
    kw = dict(frames_u8=torch.from_numpy(frames).to(device)) if images == "frames_u8" else dict(pixel_values=orc.preprocess_frames(frames, cfg).to(torch.bfloat16).to(device))
    out = model.score(rows, **kw)
    tg = _targets(rows, cfg.n_patches)
    assert [len(t) for t in tg] == [cfg.n_patches + p for p in P_LENS] and out.n_scored == sum(P_LENS) - 3
    got = _got_from_output(out, tg)
    _check_oracle(got, ref, tg, f"multimodal {images} resid32={resid32}")
    _check_own(model.engine, model.engine.score(tg), tg, f"multimodal {images} resid32={resid32}")
    assert abs(out.loss.item() - _loss64(ref, tg)) <= 2.0 * FEAT_TOL * max(z.abs().max().item() for z in ref)
    assert out.loss.dtype == torch.float32 and out.loss.ndim == 0 and out.loss.is_cuda


def test_language_only_score(device, planted):
    from oracle import emmax_oracle as orc

    cfg, model, sd_ref, _, full, _ = planted
    rows = [r[:p] for r, p in zip(full, P_LENS)]
    with torch.inference_mode():
        ref = [orc.llama_forward(orc.embed_tokens(torch.tensor([r]), sd_ref), sd_ref, cfg.llm, None)[0][0].float() for r in rows]
    out = model.score(rows)
    tg = _targets(rows)
    _check_oracle(_got_from_output(out, tg), ref, tg, "language-only")
    _check_own(model.engine, model.engine.score(tg), tg, "language-only")
    # equal lengths: stacked [B, S], as logits are
    out2 = model.score(torch.tensor([rows[0], rows[0]]))
    assert out2.lse.shape == out2.token_logprobs.shape == out2.predicted_ids.shape == (2, P_LENS[0])
    assert torch.equal(out2.lse[0], out2.lse[1]) and torch.equal(out2.predicted_ids[0], out2.predicted_ids[1])


@pytest.mark.parametrize("steps", [0, N_STEPS])
def test_extension_score(device, planted, steps):
    """the new ids on a cached context -- right behind the prefill, and behind the prefill plus 3 cached one-token steps -- against the oracle's
    whole-sequence rows"""
    cfg, model, sd_ref, frames, full, ref_full = planted
    P = [r[:p] for r, p in zip(full, P_LENS)]
    out = model.forward(input_ids=P, frames_u8=torch.from_numpy(frames).to(device), use_cache=True)
    h = out.past_key_values
    for t in range(steps):
        h = model.forward(input_ids=torch.tensor([[r[p + t]] for r, p in zip(full, P_LENS)]), past_key_values=h).past_key_values
    X = [r[p + steps:] for r, p in zip(full, P_LENS)]
    base = [cfg.n_patches + p + steps for p in P_LENS]
    sc = model.score(X, past_key_values=h)
    tg = _targets(X, new_rows_only=True)
    assert sc.past_key_values is h and h.lengths == [b + len(x) for b, x in zip(base, X)]
    ref = [z[b:b + len(x)] for z, b, x in zip(ref_full, base, X)]
    _check_oracle(_got_from_output(sc, tg), ref, tg, f"extension behind {steps} steps")
    _check_own(model.engine, model.engine.score(tg), tg, f"extension behind {steps} steps")


def test_extension_over_the_fp8_kv_cache(device):
    from emmax import _lib
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny(gqa=True)
    with _lib.tuning(kv_fp8=1):
        model, _ = _mk(cfg, SEED, True, device, max_batch=3, max_prompt=128, max_ctx=448)
    frames, full = _inputs(cfg, 3, [p + x for p, x in zip(P_LENS, X_LENS)], seed=78)
    h = model.forward(input_ids=[r[:p] for r, p in zip(full, P_LENS)], frames_u8=torch.from_numpy(frames).to(device), use_cache=True).past_key_values
    X = [r[p:] for r, p in zip(full, P_LENS)]
    sc = model.score(X, past_key_values=h)
    tg = _targets(X, new_rows_only=True)
    _got_from_output(sc, tg)
    _check_own(model.engine, model.engine.score(tg), tg, "extension over the fp8 KV cache")
    model.engine.close()


@pytest.mark.parametrize("dtype", ["fp8", "mxfp4"])
def test_quantised_decode_weights_score_on_their_prefill_lm_head(device, dtype):
    """fp8: the prefill and emmax_prefill_score read the bf16 rows; MXFP4: the de-quantised copy, which the oracle gets too"""
    from emmax.config import EmmaXConfig
    from emmax.modeling import EmmaXForActionPrediction
    from emmax.weights import synthetic_state_dict

    if dtype == "mxfp4":
        cfg = M4.e2e_cfg()
        sd_bf = M4.e2e_state_dict(True, M4.E2E_RANDOM_SEED)
        sd_ref = M4.dequant_state_dict(sd_bf)
    else:
        cfg = EmmaXConfig.tiny()
        cfg.decode_weight_dtype = "fp8"
        sd_bf = {k: v.to(torch.bfloat16) for k, v in synthetic_state_dict(cfg, seed=SEED, planted=True).items()}
        sd_ref = {k: v.float() for k, v in sd_bf.items()}
    model = EmmaXForActionPrediction(cfg, dict(sd_bf)).to(device, max_batch=3, max_prompt=64)
    frames, rows = _inputs(cfg, 3, P_LENS, seed=79)
    ref = _oracle_mm(cfg, sd_ref, frames, rows)
    out = model.score(rows, frames_u8=torch.from_numpy(frames).to(device))
    tg = _targets(rows, cfg.n_patches)
    _check_oracle(_got_from_output(out, tg), ref, tg, dtype)
    if cfg.llm.hidden_size == 256:   # (the bound of (a) is the table's K = 256 entry; the MXFP4 shape has hidden 1024)
        _check_own(model.engine, model.engine.score(tg), tg, dtype)
    model.engine.close()


def test_wrapper_prompt_last_row_is_the_goldens(device, planted):
    import os

    cfg, model, _, _, _, _ = planted
    g = np.load(os.path.join(GOLDEN, "wrapper.npz"))
    assert int(g["seed"]) == SEED
    out = model.score([g["prompt"].tolist()], frames_u8=torch.from_numpy(g["frames"]).to(device))
    assert int(out.predicted_ids[0][-1]) == int(g["logits_argmax"][-1])


def test_score_changes_nothing_that_follows(device, planted):
    cfg, model, _, frames, full, _ = planted
    eng = model.engine
    rows = [r[:p] for r, p in zip(full, P_LENS)]
    fr = torch.from_numpy(frames).to(device)
    tg = _targets(rows, cfg.n_patches)
    model._prefill(rows, None, fr, max_new=10)
    want = [x.clone() for x in eng.generate(8)]
    model._prefill(rows, None, fr, max_new=10)
    before = torch.cat(eng.prefill_logits()).clone()
    a = eng.score(tg)
    after = torch.cat(eng.prefill_logits())
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    b = eng.score(tg)
    for x, y in zip(a, b):
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(x, y))
    got = eng.generate(8)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_forward_labels_loss_is_scores_loss_and_leaves_the_logits(device, planted):
    cfg, model, _, frames, full, ref_full = planted
    rows = [r[:p] for r, p in zip(full, P_LENS)]
    fr = torch.from_numpy(frames).to(device)
    labels = [list(r) for r in rows]
    labels[0][3:6] = [-100] * 3
    labels[1] = [-100] * len(labels[1])
    plain = model.forward(input_ids=rows, frames_u8=fr)
    out = model.forward(input_ids=rows, frames_u8=fr, labels=labels)
    sc = model.score(rows, frames_u8=fr, labels=labels)
    assert plain.loss is None and out.loss.dtype == torch.float32 and out.loss.ndim == 0 and out.loss.is_cuda
    assert torch.equal(out.loss, sc.loss)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out.logits, plain.logits))
    from emmax.scoring import targets_for

    tg = targets_for(labels, rows, n_patches=cfg.n_patches)
    ref = [z[: cfg.n_patches + p] for z, p in zip(ref_full, P_LENS)]
    assert sc.n_scored == sum(t != -100 for r in tg for t in r) == (P_LENS[0] - 1 - 3) + (P_LENS[2] - 1)
    assert abs(out.loss.item() - _loss64(ref, tg)) <= 2.0 * FEAT_TOL * max(z.abs().max().item() for z in ref)
    # predicted_ids are what the logits' argmax would be, wherever the logits are not tied at their top
    for b, z in enumerate(plain.logits):
        top2 = z.topk(2, -1).values
        sure = top2[:, 0] > top2[:, 1]
        assert torch.equal(sc.predicted_ids[b].long()[sure], z.argmax(-1)[sure])
    # nothing scored: NaN, as HF's mean over nothing
    none = model.forward(input_ids=rows, frames_u8=fr, labels=[[-100] * len(r) for r in rows])
    assert math.isnan(none.loss.item())
    # the one-token cached branch keeps the reference's assertion
    h = model.forward(input_ids=rows, frames_u8=fr, use_cache=True).past_key_values
    with pytest.raises(AssertionError, match="labels"):
        model.forward(input_ids=torch.tensor([[5], [6], [7]]), past_key_values=h, labels=torch.tensor([[5], [6], [7]]))


def test_exact_engine_refuses(device):
    from emmax.config import EmmaXConfig

    cfg = EmmaXConfig.tiny()
    model, _ = _mk(cfg, SEED, True, device, max_batch=1, max_prompt=32, exact=True)
    rows = [[1, 50, 600, 7000]]
    with pytest.raises(NotImplementedError, match="exact"):
        model.score(rows)
    with pytest.raises(NotImplementedError, match="exact"):
        model.forward(input_ids=rows, labels=rows)
    model.forward(input_ids=rows)
    with pytest.raises(NotImplementedError, match="exact"):
        model.engine.score([[50, 600, 7000, -100]])
    from emmax import _lib

    tg = torch.zeros(4, dtype=torch.int32, device=device)
    o = torch.zeros(3, 4, device=device)
    r = model.engine.lib.emmax_prefill_score(model.engine._session, tg.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), _lib.current_stream())
    assert r == -5   # EMMAX_ERR_STATE
    model.engine.close()


def test_score_allocates_no_logits(device, planted):
    cfg, model, _, _, _, _ = planted
    rng = np.random.default_rng(9)
    rows = [[1] + [int(x) for x in rng.integers(3, 31744, size=n - 1)] for n in (120, 100, 80)]   # 300 packed rows: their logits would be 38 MB
    model.engine.ensure_capacity(3, 120, 1)
    model.score(rows)   # warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = model.score(rows)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"score over 300 rows: peak rises by {rise} bytes (logits: {300 * cfg.llm.vocab_size * 4})")
    assert out.n_scored == 297 and rise < (1 << 20), rise
