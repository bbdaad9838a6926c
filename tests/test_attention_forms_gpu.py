"""The prefill / ViT attention in every launched form (attention.hip: the ring kernel's seven instantiations and the resident kernel's three) against
the float64 reference of tests/attention_ref.py: cases, input families, NaN-poisoned buffers and the tolerance table live there (measured on the CPU
as |fp32 emulation - float64|; the bound is twice that, between the project's bf16 line and the line of test_ops_gpu.py::test_attention).

Every case asserts its launch plan (emmax_attention_plan -- the launcher dispatches on the same struct) before it launches;
tests/test_attention_plan.py proves on the CPU that the tags cover all ten instantiations, tests/test_attention_ref.py that a subtly wrong kernel
(a dropped or doubled key at a tile edge, a shifted diagonal, a skipped or misplaced lazy rescale, the neighbouring kv head, swapped merge weights,
a sequence one key short) fails these bounds.  Each case launches twice and requires bit-equal results (a ring or barrier race is not
deterministic), finite live rows, and bit-untouched padding columns and guard rows.  The module prints the worst measured error of every
(form, family) next to its bound (pytest -s).

The symbol is looked up without a skip: on a library without it this file fails."""

import pytest
import torch

import attention_ref as R
from test_attention_plan import attn_plan
from test_ops_gpu import _lib, assert_elementwise, stream

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\n== attention forms: worst measured error / bound ==")
    for key in sorted(WORST):
        print(f"{key[0]:14s} {key[1]:12s} " + "  ".join(f"{k} {v:.3g} / {b:.3g}" for k, (v, b) in sorted(WORST[key].items())))


def launch_twice(c, device):
    """-> (out of launch 1, out of launch 2) as CPU bf16 [total + 2, ld_out], and the geometry"""
    L, lib = _lib()
    qkv, cu, out, (q_off, k_off, v_off, ld, ld_out) = c.buffers()
    qkv_d, cu_d = qkv.to(device), cu.to(device)
    outs = []
    with L.tuning(**c.tune):
        plan = attn_plan(lib, c.B, c.max_seqlen, c.Hq, c.Hkv, c.hd, c.causal)
        assert plan == c.tag, (c.name, plan, c.tag)   # the plan first, the launch second
        for _ in range(2):
            o = out.to(device)   # NaN everywhere, again
            rc = lib.emmax_op_attention(qkv_d[1:].data_ptr(), ld, q_off, k_off, v_off, o[1:].data_ptr(), ld_out, cu_d.data_ptr(), c.B, c.max_seqlen, c.Hq, c.Hkv,
                                        c.hd, c.scale, c.causal, stream())
            torch.cuda.synchronize()
            L.check(rc, c.name)
            outs.append(o.cpu())
    return outs[0], outs[1], ld_out


def check_case(c, device, fails):
    a, b, ld_out = launch_twice(c, device)
    qd = c.Hq * c.hd
    bits = a.view(torch.int16)
    if not torch.equal(bits, b.view(torch.int16)):
        fails.append(f"{c.name}: two launches differ in {int((bits != b.view(torch.int16)).sum())} values")
    nan = torch.tensor(R.NAN_BITS, dtype=torch.int16)
    if not ((bits[0] == nan).all() and (bits[-1] == nan).all()):
        fails.append(f"{c.name}: a guard row of the output was written")
    if not (bits[1:-1, qd:] == nan).all():
        fails.append(f"{c.name}: a padding column of the output was written")
    got = a[1:-1, :qd].float().view(c.total, c.Hq, c.hd)
    if not torch.isfinite(got).all():   # every packed row is live: a NaN column, a guard row or an unmasked key was read, or a row was not written
        fails.append(f"{c.name}: {int((~torch.isfinite(got)).sum())} values of live rows are not finite")
        return
    ref, tol = R.ref64(c), R.tolerances(c.form, c.family)
    errs = R.errors(c, got, ref)
    w = WORST.setdefault((c.form, c.family), {})
    for k, bound in tol.items():
        w[k] = (max(w.get(k, (0.0, 0.0))[0], errs[k]), bound)
        if errs[k] > bound:
            fails.append(f"{c.name}: {k} {errs[k]:.3g} > {bound:.3g}")
    if "spread" in tol:   # the project's elementwise line at this family's atol, on every sequence by itself (as the measure)
        o = 0
        for n in c.lens:
            if n:
                try:
                    assert_elementwise(got[o:o + n], ref[o:o + n], rtol=R.BF16_RTOL, atol_frac=tol["spread"], what=f"{c.name} sequence at row {o}")
                except AssertionError as e:
                    fails.append(str(e))
                o += n


def _params():
    return [(form, fam) for form in R.FORMS for fam in R.FAMILIES + (R.K2_FAMILIES if R.FORMS[form]["kg"] == 2 else ())]


@pytest.mark.parametrize("form,family", _params(), ids=lambda x: x)
def test_every_form_at_every_loop_edge(device, form, family):
    """Every case of one (instantiation, input family): the ragged batch of every loop-edge length with empty sequences, under both masks where the
    form has both, the long sequence of many ring wraps, at every GQA shape (random), the resident pipeline at one, two and three items per block,
    and the launches that reach the form with no switch set."""
    cases = R.cases_of(form, family)
    assert cases
    fails = []
    for c in cases:
        check_case(c, device, fails)
    assert not fails, "\n".join(fails)

