"""CPU: the tolerance table of tests/test_decode_stages_gpu.py is what the fp32 emulation of the documented roundings measures against the
float64 reference (decode_stage_ref.py) -- not a number taken from a kernel's output, and not a stale or padded one."""

import pytest

import decode_stage_ref as R


@pytest.mark.parametrize("form,fp8", [("f32", False), ("mirror", True), ("hf", False), ("hf", True), ("exact", False)])
def test_tolerance_table_matches_the_emulation(form, fp8):
    spread, rel = R.measure(form, fp8=fp8, quiet=True)
    for out in R.OUTPUTS:
        # the table holds the worst of bf16 and de-quantised fp8 weights: each measurement must sit under it (5 % for another BLAS's summation
        # order), and the table may not be padded: the larger of the two weight types is at least 2/3 of it
        assert spread[out] <= 1.05 * R.SPREAD[form][out] + 1e-9, (out, spread[out], R.SPREAD[form][out])
        assert rel[out] <= 1.05 * R.REL[form][out] + 1e-9, (out, rel[out], R.REL[form][out])
        if R.SPREAD[form][out] > 1e-6:
            assert spread[out] >= 0.66 * R.SPREAD[form][out], (out, spread[out], R.SPREAD[form][out])


def test_bounds_never_fall_below_the_projects_bf16_line():
    for form in R.FORMS:
        for out in R.OUTPUTS:
            rtol, atol, tol = R.tolerances(form, out)
            assert rtol == 1e-2 and atol >= 4e-3 and tol >= 1e-2 and atol == max(4e-3, 2 * R.SPREAD[form][out])
    for out in R.OUTPUTS:
        rtol, atol, tol = R.tolerances("exact", out)
        assert rtol == 2.0 ** -15 and atol < 1e-4 and tol < 1e-4   # near 1e-5 relative: the two-term operand
