#!/usr/bin/env python3
"""Writes tests/golden/llama_taps.npz: HF's own output_hidden_states / output_attentions, the fixture tests/test_taps_ref.py checks the float64
restatement (tests/taps_ref.py: llama_stack) against.

`transformers.LlamaForCausalLM` (eager attention, CPU fp32) is rebuilt from the weights and `embeds` already stored in
tests/golden/llama_mha.npz / llama_gqa.npz; the script first checks that the rebuilt model reproduces those files' `prefill_logits` with difference
0.0, then stores, per variant: the prompt pass's hidden_states [n_layers + 1, 9, H] (entry 0 = embeds, the last one normed) and attentions
[n_layers, Hq, 9, 9], and the same of the first STEPS cached one-token steps on the fixture's greedy ids ([STEPS, n_layers + 1, H] and, padded with
zeros to the longest context, [STEPS, n_layers, Hq, 9 + STEPS]).  Arrays only, a few KB.  Needs transformers; reads nothing but those two files.

    python tools/make_llama_taps.py
"""

import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEPS = 2


def rebuild(g):
    from transformers import LlamaConfig, LlamaForCausalLM

    h, inter, nl, nh, nkv, hd, vocab = [int(x) for x in g["cfg"]]
    cfg = LlamaConfig(hidden_size=h, intermediate_size=inter, num_hidden_layers=nl, num_attention_heads=nh, num_key_value_heads=nkv, head_dim=hd,
                      vocab_size=vocab, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=2048, attention_bias=False,
                      tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    m = LlamaForCausalLM(cfg).eval().to(torch.float32)
    sd = {k.replace("__", ".")[len("language_model."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("language_model")}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    return m


def main():
    out = {}
    for name in ("mha", "gqa"):
        g = np.load(os.path.join(GOLDEN, f"llama_{name}.npz"))
        m = rebuild(g)
        with torch.no_grad():
            o = m(inputs_embeds=torch.from_numpy(g["embeds"]), use_cache=True, output_hidden_states=True, output_attentions=True)
            diff = (o.logits[0] - torch.from_numpy(g["prefill_logits"])).abs().max().item()
            assert diff == 0.0, f"{name}: the rebuilt model is {diff} from the stored prefill logits"
            nl = len(o.attentions)
            assert len(o.hidden_states) == nl + 1 and torch.equal(o.hidden_states[0][0], torch.from_numpy(g["embeds"][0]))
            assert torch.equal(m.lm_head(o.hidden_states[-1]), o.logits)   # the last entry is normed
            assert all(float(a[0].triu(1).abs().max()) == 0.0 for a in o.attentions)
            out[f"{name}__hidden"] = torch.stack([x[0] for x in o.hidden_states]).numpy()
            out[f"{name}__attn"] = torch.stack([a[0] for a in o.attentions]).numpy()
            cache, T0 = o.past_key_values, g["embeds"].shape[1]
            sh, sa = [], []
            for t in range(STEPS):
                s = m(input_ids=torch.tensor([[int(g["ids"][t])]]), past_key_values=cache, use_cache=True, output_hidden_states=True, output_attentions=True)
                cache = s.past_key_values
                assert (s.logits[0, -1] - torch.from_numpy(g["step_logits"][t])).abs().max().item() == 0.0
                sh.append(torch.stack([x[0, 0] for x in s.hidden_states]))
                a = torch.zeros(nl, s.attentions[0].shape[1], T0 + STEPS)
                a[:, :, : T0 + t + 1] = torch.stack([x[0, :, 0] for x in s.attentions])
                sa.append(a)
            out[f"{name}__step_hidden"] = torch.stack(sh).numpy()
            out[f"{name}__step_attn"] = torch.stack(sa).numpy()
    path = os.path.join(GOLDEN, "llama_taps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
