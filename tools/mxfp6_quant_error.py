"""What the decode weight formats do to the MODEL, on the CPU (fp32 oracle against fp32 oracle, no kernel involved), by the procedure of
tools/mxfp4_quant_error.py: the prefill logits of the 2-layer end-to-end configuration of tests/mxfp6_ref.py with every LLM projection
de-quantised from MXFP6 e2m3, from MXFP4 and from e4m3 with one scale per row (fp8 -- which the fp8 ENGINE applies to its decode steps only; here
the whole model, to compare the formats), against the same model unquantised, over the eight rows of the GPU test.  Random gaussian weights: the
worst case, every block uses its whole range.  The tests never assert these figures; profiles/mxfp6_quant_error.txt holds this script's output."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "emma-x_amd"), os.path.join(ROOT, "tests")]
import torch

import mxfp4_ref as M4
import mxfp6_ref as M


def dequant_e4m3_rows(w):
    """a projection as the fp8 engine streams it: e4m3 x one fp32 scale per row (tests/test_operating_point_gpu.py)"""
    w = w.float()
    scale = (w.abs().amax(dim=1, keepdim=True) / 448.0).clamp_min(1e-30)
    return (w / scale).to(torch.float8_e4m3fn).float() * scale


def main():
    cfg = M.e2e_cfg()
    sd = M.e2e_state_dict(False, M.E2E_RANDOM_SEED)
    sds = {"mxfp6": M.dequant_state_dict(sd), "fp8": {k: (dequant_e4m3_rows(v) if M.is_decode_projection(k) else v.float()) for k, v in sd.items()},
           "mxfp4": M4.dequant_state_dict(sd)}
    sd_f = {k: v.float() for k, v in sd.items()}
    frames, rows = M.e2e_inputs(8, M.E2E_LENS8, seed=2024)
    errs = {f: [] for f in sds}
    same = {f: 0 for f in sds}
    for b in range(8):
        gf, tf = M.oracle_trace(cfg, sd_f, frames[b:b + 1], rows[b], 1)
        line = []
        for f, sd_q in sds.items():
            gq, tq = M.oracle_trace(cfg, sd_q, frames[b:b + 1], rows[b], 1)
            e0 = ((tq[0] - tf[0]).abs().max() / tf[0].abs().max()).item()
            errs[f].append(e0)
            same[f] += int(gq[0] == gf[0])
            line.append(f"{f} {e0:.3e} ({'equal' if gq[0] == gf[0] else 'differs'})")
        print(f"row {b}: prefill logits |quantised - unquantised| / max|unquantised|, first greedy id: " + "  ".join(line))
    for f in sds:
        print(f"{f}: worst {max(errs[f]):.2e}, best {min(errs[f]):.2e} of max|logit| over 8 rows; first greedy id equal on {same[f]} of 8 rows")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
