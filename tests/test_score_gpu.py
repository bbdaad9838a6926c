"""GPU: emmax_op_score_rows (emma-x_amd/csrc/score.hip) on every case of tests/score_ref.py against the float64 reference, within the bounds that
module measured on the CPU; the plan of every launch through emmax_score_plan; the refusals; two launches of one case bit for bit."""

import ctypes as C
import math

import pytest
import torch

import score_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from emmax import _lib

    lib = _lib.load()
    for name in ("emmax_op_score_rows", "emmax_score_plan", "emmax_prefill_score"):   # looked up, not skipped: a library without them fails here
        getattr(lib, name)
    return _lib


def lib_plan(L, rows, V, K, ws_bytes):
    o = [C.c_int(0) for _ in range(4)]
    L.check(L.load().emmax_score_plan(rows, V, K, ws_bytes, *[C.byref(x) for x in o]), "emmax_score_plan")
    return tuple(x.value for x in o)


def launch(L, device, c, o, slices=None, ws_bytes=S.WS_BYTES):
    """-> (Got of the live rows, the two sentinel rows behind them of every output)"""
    X = o.X.to(torch.bfloat16).to(device)
    W = o.W.to(torch.bfloat16).to(device)
    tg = o.targets.to(device)
    ws = torch.full((ws_bytes // 4,), S.NAN, device=device)
    lse = torch.full((c.rows + 2,), S.NAN, device=device)
    logit = torch.full((c.rows + 2,), S.NAN, device=device)
    am = torch.full((c.rows + 2,), -7, dtype=torch.int32, device=device)
    L.check(L.load().emmax_op_score_rows(X.data_ptr(), c.K, W.data_ptr(), c.K, c.rows, c.V, c.Np, c.K, tg.data_ptr(), c.slices if slices is None else slices,
                                         ws.data_ptr(), ws_bytes, lse.data_ptr(), logit.data_ptr(), am.data_ptr(), L.current_stream()), "emmax_op_score_rows")
    torch.cuda.synchronize()
    lse, logit, am = lse.cpu(), logit.cpu(), am.cpu()
    return S.Got(lse[:c.rows], logit[:c.rows], am[:c.rows]), (lse[c.rows:], logit[c.rows:], am[c.rows:])


@pytest.mark.parametrize("c", S.CASES, ids=[c.name for c in S.CASES])
def test_case_against_ref64(L, device, c):
    o = S.operands(c)
    ref = S.ref64(c, o)
    # the plan: a forced count is what the restated rule says; the planner's is the library's own answer
    if c.slices == 0:
        assert lib_plan(L, c.rows, c.V, c.K, S.WS_BYTES) == S.case_plan(c)
    else:   # (the planner reaches a forced count where the scratch caps it there)
        assert S.case_plan(c)[2] == c.slices and lib_plan(L, c.rows, c.V, c.K, 12 * c.rows * c.slices) == S.case_plan(c)
    got, (s_lse, s_logit, s_am) = launch(L, device, c, o)
    e = S.errors(c, o, got, ref)
    tol = S.tolerances(c)
    print(f"{c.name}: lse {e['lse']:.3g} / {tol['lse']:.3g}  logit {e['logit']:.3g} / {tol['logit']:.3g}  argmax {e['argmax']} of {e['clear']}  planted {e['planted']}")
    assert torch.isfinite(got.lse).all() and torch.isfinite(got.logit).all()
    assert ((got.argmax >= 0) & (got.argmax < c.V)).all()
    assert torch.isnan(s_lse).all() and torch.isnan(s_logit).all() and (s_am == -7).all()   # nothing behind the live rows was written
    assert e["zero"] == 0                      # exactly 0.0 where the target is -100
    assert e["planted"] == 0                   # ties resolve to the lower id, an all-zero row gives id 0
    for r in o.flat_rows:
        assert got.argmax[r] == 0 and abs(got.lse[r].item() - math.log(c.V)) <= tol["lse"] * math.log(c.V)
    assert e["argmax"] == 0
    assert e["lse"] <= tol["lse"] and e["logit"] <= tol["logit"], e


def test_two_launches_are_bit_identical(L, device):
    for name in ("random-r129-k128-v1000-s3", "ties-r300-k256-v1000-s3"):
        c = S.BY_NAME[name]
        o = S.operands(c)
        a, _ = launch(L, device, c, o)
        b, _ = launch(L, device, c, o)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def test_plan_closure(L):
    """the library's planner is the rule tests/score_ref.py restates, at the cases' shapes, at 7B shapes and where the scratch caps the slices"""
    shapes = {(c.rows, c.V, c.K) for c in S.CASES} | {(768, 32000, 4096), (6144, 32064, 4096), (1, 32000, 4096)}
    for rows, V, K in sorted(shapes):
        for ws in (S.WS_BYTES, 64 << 20, 12 * rows, 12 * rows * 2 + 5):
            assert lib_plan(L, rows, V, K, ws) == S.plan(rows, V, ws), (rows, V, K, ws)
    assert L.load().emmax_score_plan(129, 1000, 128, 12 * 129 - 1, None, None, None, None) != 0


def test_refusals(L, device):
    lib = L.load()
    c = S.BY_NAME["random-r129-k128-v1000-s3"]
    o = S.operands(c)
    X = o.X.to(torch.bfloat16).to(device)
    W = o.W.to(torch.bfloat16).to(device)
    tg = o.targets.to(device)
    ws = torch.zeros(S.WS_BYTES // 4, device=device)
    out = [torch.zeros(c.rows, device=device), torch.zeros(c.rows, device=device), torch.zeros(c.rows, dtype=torch.int32, device=device)]

    def call(rows=c.rows, V=c.V, Np=c.Np, K=c.K, slices=0, ws_bytes=S.WS_BYTES):
        r = lib.emmax_op_score_rows(X.data_ptr(), c.K, W.data_ptr(), c.K, rows, V, Np, K, tg.data_ptr(), slices, ws.data_ptr(), ws_bytes,
                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), L.current_stream())
        return r, lib.emmax_last_error().decode()

    assert call()[0] == 0
    for kw, word in ((dict(K=96), "multiple of 64"), (dict(K=0), "multiple of 64"), (dict(Np=896), "Np"), (dict(Np=1000), "Np"), (dict(rows=0), "rows"),
                     (dict(V=0, Np=0), "V"), (dict(slices=9), "slices"), (dict(slices=3, ws_bytes=12 * c.rows * 3 - 1), "scratch"),
                     (dict(ws_bytes=12 * c.rows - 1), "scratch")):
        r, msg = call(**kw)
        assert r == -1 and word in msg, (kw, r, msg)
    torch.cuda.synchronize()
