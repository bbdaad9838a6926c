"""What MXFP4 does to the MODEL, on the CPU (fp32 oracle against fp32 oracle, no kernel involved): the logits of the 2-layer end-to-end
configuration of tests/mxfp4_ref.py with every LLM projection de-quantised from MXFP4, against the same model unquantised, over the
teacher-forced steps the GPU test runs (each model follows its own greedy ids from the same prompt; step 0 is the prefill).  Random gaussian
weights: the worst case of a 4-bit grid, every block uses its whole range.  The tests never assert this figure; profiles/mxfp4_quant_error.txt
is this script's output."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd"), os.path.join(ROOT, "tests")]
import torch

import mxfp4_ref as M


def main():
    cfg = M.e2e_cfg()
    sd = M.e2e_state_dict(False, M.E2E_RANDOM_SEED)
    sd_q, sd_f = M.dequant_state_dict(sd), {k: v.float() for k, v in sd.items()}
    frames, rows = M.e2e_inputs(8, M.E2E_LENS8, seed=2024)
    step0, same = [], 0
    for b in range(8):
        gq, tq = M.oracle_trace(cfg, sd_q, frames[b:b + 1], rows[b], M.E2E_STEPS)
        gf, tf = M.oracle_trace(cfg, sd_f, frames[b:b + 1], rows[b], M.E2E_STEPS)
        e0 = ((tq[0] - tf[0]).abs().max() / tf[0].abs().max()).item()
        step0.append(e0)
        same += int(gq[0] == gf[0])
        print(f"row {b}: prefill logits |quantised - unquantised| / max|unquantised| {e0:.3e}, first greedy id {'equal' if gq[0] == gf[0] else 'differs'}")
    print(f"worst {max(step0):.2e}, best {min(step0):.2e} of max|logit| over 8 rows; first greedy id equal on {same} of 8 rows")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
