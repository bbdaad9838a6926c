#!/usr/bin/env python3
"""Writes tests/golden/llama_loss.npz: HF's own `loss` for a handful of label patterns, the fixture tests/test_scoring.py checks the host's label
alignment (emmax/scoring.py: targets_for) against.

`transformers.LlamaForCausalLM` (CPU fp32) is rebuilt from the weights and `embeds` already stored in tests/golden/llama_mha.npz / llama_gqa.npz
(tools/make_llama_taps.py: rebuild); the script first checks that the rebuilt model reproduces those files' `prefill_logits` with difference 0.0,
then stores, per variant, the labels [PATTERNS, 9] and HF's loss [PATTERNS] of the fixture's 9 rows for these patterns -- all valid; a mix of valid
and -100; only the last label valid; all -100 (HF: NaN) -- and a right-padded batch of two rows (9 and 6 positions; the short row is the long one's
prefix): its labels [2, 9] (-100 on the padding), attention mask and HF's one loss.  Arrays only, a few KB.  Needs transformers; reads nothing but
those two files.

    python tools/make_llama_loss.py
"""

import os

import numpy as np
import torch

from make_llama_taps import GOLDEN, rebuild

SHORT = 6


def main():
    out = {}
    for name in ("mha", "gqa"):
        g = np.load(os.path.join(GOLDEN, f"llama_{name}.npz"))
        m = rebuild(g)
        vocab = int(g["cfg"][6])
        emb = torch.from_numpy(g["embeds"])
        n = emb.shape[1]
        rng = np.random.default_rng(5 if name == "mha" else 6)
        base = rng.integers(0, vocab, size=n)
        pats = np.stack([base, np.where(rng.random(n) < 0.5, base, -100), np.where(np.arange(n) == n - 1, base, -100), np.full(n, -100)]).astype(np.int64)
        pats[1, 3], pats[1, 4] = base[3], -100   # (the mix holds both kinds whatever the draw)
        with torch.no_grad():
            o = m(inputs_embeds=emb)
            diff = (o.logits[0] - torch.from_numpy(g["prefill_logits"])).abs().max().item()
            assert diff == 0.0, f"{name}: the rebuilt model is {diff} from the stored prefill logits"
            loss = [m(inputs_embeds=emb, labels=torch.from_numpy(p)[None]).loss.item() for p in pats]
            assert np.isfinite(loss[:3]).all() and np.isnan(loss[3]), loss
            two = torch.cat([emb, torch.cat([emb[:, :SHORT], torch.zeros(1, n - SHORT, emb.shape[2])], 1)])
            mask = torch.ones(2, n, dtype=torch.long)
            mask[1, SHORT:] = 0
            lab2 = np.stack([pats[1], np.where(np.arange(n) < SHORT, rng.integers(0, vocab, size=n), -100)]).astype(np.int64)
            loss2 = m(inputs_embeds=two, attention_mask=mask, labels=torch.from_numpy(lab2)).loss.item()
        out[f"{name}__labels"], out[f"{name}__loss"] = pats, np.array(loss, dtype=np.float64)
        out[f"{name}__batch_labels"], out[f"{name}__batch_mask"], out[f"{name}__batch_loss"] = lab2, mask.numpy(), np.array(loss2, dtype=np.float64)
    path = os.path.join(GOLDEN, "llama_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
