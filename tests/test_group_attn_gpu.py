"""The grouped decode attention (emmax_op_decode_attention_group / _kv8; decode_attn.hip: launch_group_attn) against a float64 reference.

The B rows of a launch are B / N groups; the rows of a group reference the same physical pages for their first shared_pages[g] table entries
and own every later page.  For each row the reference is softmax(q k^T / sqrt(128)) v over the row's OWN gathered keys 0 .. ctx_len, in
float64.  Every page no row references and every position past a row's context holds NaN, so a wrong page or an unmasked key shows as NaN.
Tolerance: the project's own for the one-split direct form (tests/test_ops_gpu.py: relerr < 8e-3 plus assert_elementwise) -- the arithmetic
is the same: bf16 operands, fp32 accumulation, one fp32 merge, one bf16 rounding of the result.

The symbols are looked up without a skip: on a library without the feature this file fails."""

import ctypes as C

import pytest
import torch

from test_ops_gpu import _lib, _quant_rows_e4m3, assert_elementwise, bf, relerr, stream

pytestmark = pytest.mark.gpu

PAGE = 64
ERR_INVALID = -1
MAX_SPLITS = 8   # partials per (row, head) the workspace holds (include/emmax.h)


def _case(groups, Hq, Hkv, max_pages, seed, kv8=False, done=()):
    """groups: [(N, shared_pages, [ctx_len of each of the N rows])].  Returns the device operands and the float64 reference [B, Hq, 128]."""
    g = torch.Generator().manual_seed(seed)
    B = sum(n for n, _, _ in groups)
    n_pages = B * max_pages
    table = torch.randperm(n_pages, generator=g).view(B, max_pages).to(torch.int32)   # random physical placement
    vary = (lambda n: 0.5 + 2.0 * torch.rand(n, Hkv, 1, generator=g)) if kv8 else (lambda n: 1.0)
    rows_k, rows_v, r0 = [], [], 0
    for N, sh, ctxs in groups:
        assert len(ctxs) == N and all(sh * PAGE <= c < max_pages * PAGE for c in ctxs)
        ks, vs = bf(torch.randn(sh * PAGE, Hkv, 128, generator=g) * vary(sh * PAGE)), bf(torch.randn(sh * PAGE, Hkv, 128, generator=g) * vary(sh * PAGE))
        for j, c in enumerate(ctxs):
            n = c + 1 - sh * PAGE   # the row's own keys sh * 64 .. ctx inclusive
            rows_k.append(torch.cat([ks, bf(torch.randn(n, Hkv, 128, generator=g) * vary(n))]))
            rows_v.append(torch.cat([vs, bf(torch.randn(n, Hkv, 128, generator=g) * vary(n))]))
            table[r0 + j, :sh] = table[r0, :sh]   # the same physical ids; the ids row j held there are referenced by nobody now
        r0 += N
    ctx = [c for _, _, cs in groups for c in cs]
    q = bf(torch.randn(B, Hq, 128, generator=g))
    nan = float("nan")
    if kv8:
        K8, KS, KD = zip(*[_quant_rows_e4m3(k) for k in rows_k])
        V8, VS, VD = zip(*[_quant_rows_e4m3(v) for v in rows_v])
        kc = torch.full((n_pages, Hkv, PAGE, 128), 0x7F, dtype=torch.uint8)   # e4m3 NaN
        vc = torch.full((n_pages, Hkv, PAGE, 128), 0x7F, dtype=torch.uint8)
        ksc, vsc = torch.full((n_pages, Hkv, PAGE), nan), torch.full((n_pages, Hkv, PAGE), nan)
        n_cached = ctx   # keys 0 .. ctx - 1; the new key waits in the staging rows
        ref_k, ref_v = KD, VD
    else:
        kc, vc = bf(torch.full((n_pages, Hkv, PAGE, 128), nan)), bf(torch.full((n_pages, Hkv, PAGE, 128), nan))
        n_cached = [c + 1 for c in ctx]
        ref_k, ref_v = rows_k, rows_v
    for b in range(B):
        for t0 in range(0, n_cached[b], PAGE):
            pg, n = int(table[b, t0 // PAGE]), min(PAGE, n_cached[b] - t0)
            if kv8:
                kc[pg, :, :n], vc[pg, :, :n] = K8[b][t0:t0 + n].transpose(0, 1), V8[b][t0:t0 + n].transpose(0, 1)
                ksc[pg, :, :n], vsc[pg, :, :n] = KS[b][t0:t0 + n].transpose(0, 1), VS[b][t0:t0 + n].transpose(0, 1)
            else:
                kc[pg, :, :n], vc[pg, :, :n] = rows_k[b][t0:t0 + n].transpose(0, 1), rows_v[b][t0:t0 + n].transpose(0, 1)
    rep = Hq // Hkv
    ref = torch.zeros(B, Hq, 128, dtype=torch.float64)
    for b in range(B):
        if b in done:
            continue   # a row flagged done: zeros
        kk, vv = ref_k[b].double().repeat_interleave(rep, dim=1), ref_v[b].double().repeat_interleave(rep, dim=1)
        att = torch.einsum("hd,lhd->hl", q[b].double(), kk) * (128 ** -0.5)
        ref[b] = torch.einsum("hl,lhd->hd", torch.softmax(att, dim=-1), vv)
    dev = "cuda"
    ops = dict(B=B, q=q.view(B, Hq * 128).contiguous().to(dev), kc=kc.to(dev), vc=vc.to(dev), table=table.to(dev),
               ctx=torch.tensor(ctx, dtype=torch.int32, device=dev), shared=torch.tensor([s for _, s, _ in groups], dtype=torch.int32, device=dev),
               done=torch.tensor([1 if b in done else 0 for b in range(B)], dtype=torch.int32, device=dev) if done else None)
    if kv8:
        ops.update(ks=ksc.to(dev), vs=vsc.to(dev),
                   stage=torch.stack([torch.stack([rows_k[b][ctx[b]], rows_v[b][ctx[b]]], dim=1) for b in range(B)]).contiguous().to(dev))
    return ops, ref


def _launch(ops, N, Hq, Hkv, max_pages, kv8=False, B=None, shared=None, want_ws=False):
    _, lib = _lib()
    B = ops["B"] if B is None else B
    o = torch.full((ops["B"], Hq * 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    ws = torch.full((ops["B"] * Hq * MAX_SPLITS * 132,), float("nan"), dtype=torch.float32, device="cuda")
    done = ops["done"].data_ptr() if ops["done"] is not None else None
    sh = (ops["shared"] if shared is None else shared).data_ptr()
    if kv8:
        rc = lib.emmax_op_decode_attention_group_kv8(ops["q"].data_ptr(), ops["kc"].data_ptr(), ops["vc"].data_ptr(), ops["ks"].data_ptr(), ops["vs"].data_ptr(),
                                                     ops["stage"].data_ptr(), ops["table"].data_ptr(), ops["ctx"].data_ptr(), done, ws.data_ptr(), o.data_ptr(),
                                                     B, Hq, Hkv, PAGE, max_pages, N, sh, 128 ** -0.5, stream())
    else:
        rc = lib.emmax_op_decode_attention_group(ops["q"].data_ptr(), ops["kc"].data_ptr(), ops["vc"].data_ptr(), ops["table"].data_ptr(), ops["ctx"].data_ptr(),
                                                 done, o.data_ptr(), B, Hq, Hkv, PAGE, max_pages, 128 ** -0.5, N, sh, ws.data_ptr(), stream())
    torch.cuda.synchronize()
    if want_ws:
        return rc, o.float().cpu().view(ops["B"], Hq, 128), ws.cpu()
    return rc, o.float().cpu().view(ops["B"], Hq, 128)


def _check(groups, Hq, Hkv, max_pages, seed, kv8=False, done=()):
    L_, lib = _lib()
    ops, ref = _case(groups, Hq, Hkv, max_pages, seed, kv8, done)
    rc, got = _launch(ops, groups[0][0], Hq, Hkv, max_pages, kv8)
    L_.check(rc, "grouped decode attention")
    assert torch.isfinite(got).all(), "a NaN page or an unmasked key was read"
    for b in done:
        assert (got[b] == 0).all(), b
    err = relerr(got, ref)
    print(f"groups {groups} heads ({Hq}, {Hkv}) kv8 {kv8}: relerr {err:.3e}")
    assert err < 8e-3, err
    assert_elementwise(got, ref)


# N, shared pages, ctx -- what it checks
SMALL = [
    (2, 1, 64),    # the tail is the one new key
    (3, 2, 130),   # masked padded query
    (8, 3, 255),   # the tail is exactly one full page
    (8, 2, 191),   # ... one key short of a page edge (the span cannot reach past the context: two pages)
    (8, 3, 192),   # ... and the first key of a page
    (9, 1, 100),   # two query chunks
    (4, 0, 40),    # empty span
]
THREE_GROUPS = [(4, 0, [40, 40, 40, 40]), (4, 1, [64, 100, 127, 64]), (4, 3, [200, 200, 230, 255])]   # unequal ctx_len inside a group: the tail is per row


@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 2)])
@pytest.mark.parametrize("N,shared,ctx", SMALL)
def test_one_group_matches_float64(device, Hq, Hkv, N, shared, ctx):
    _check([(N, shared, [ctx] * N)], Hq, Hkv, 8, seed=1000 * N + ctx + Hq)


@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 2)])
def test_three_groups_one_done_row_unequal_contexts(device, Hq, Hkv):
    _check(THREE_GROUPS, Hq, Hkv, 8, seed=31 + Hq, done=(5,))


@pytest.mark.parametrize("n_groups", [1, 2])
def test_workload_shape(device, n_groups):
    """32 heads, N = 8, twelve shared pages of a 867-token context: one group (eight splits of the span) and two (four)."""
    _check([(8, 12, [867] * 8)] * n_groups, 32, 32, 21, seed=867 + n_groups)


def test_one_split_span_eight_groups_at_32_heads(device):
    """Eight groups of N = 4 at 32 kv heads are 256 span blocks: ONE split per (row, head), the form of the 64-row steps.  The workspace shows
    it: exactly one partial per (row, head) is written, the rest of the NaN-filled buffer is untouched."""
    L_, _ = _lib()
    groups = [(4, 2, [150 + 5 * g, 128, 191, 130 + g]) for g in range(8)]
    ops, ref = _case(groups, 32, 32, 4, seed=3232)
    rc, got, ws = _launch(ops, 4, 32, 32, 4, want_ws=True)
    L_.check(rc, "grouped decode attention")
    n = 32 * 32 * 132
    assert torch.isfinite(ws[:n].view(-1, 132)[:, :130]).all() and torch.isnan(ws[n:]).all()
    assert torch.isfinite(got).all()
    err = relerr(got, ref)
    print(f"8 groups x 4 rows, 32 heads, one split: relerr {err:.3e}")
    assert err < 8e-3, err
    assert_elementwise(got, ref)


@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 2)])
@pytest.mark.parametrize("groups,done", [([(3, 2, [130] * 3)], ()), ([(8, 3, [255] * 8)], ()), (THREE_GROUPS, (5,))])
def test_fp8_cache(device, Hq, Hkv, groups, done):
    """e4m3 rows + row scales; the reference attends over the de-quantised values (_quant_rows_e4m3), the step's key waits in the staging rows."""
    _check(groups, Hq, Hkv, 8, seed=88 + Hq + len(groups), kv8=True, done=done)


def test_refusals_launch_nothing(device):
    _, lib = _lib()
    ops, _ = _case([(4, 1, [70] * 4)], 2, 2, 8, seed=5)
    too_many = torch.tensor([9], dtype=torch.int32, device="cuda")
    past_ctx = torch.tensor([2], dtype=torch.int32, device="cuda")           # 128 shared keys, rows of 70: the tails would be empty
    for kw, N in ((dict(B=3), 2), (dict(), 1), (dict(shared=too_many), 4), (dict(shared=past_ctx), 4)):   # B % N != 0; N = 1; a shared count above max_pages; above the context
        rc, got = _launch(ops, N, 2, 2, 8, **kw)
        assert rc == ERR_INVALID, (kw, N, rc)
        assert b"emmax_op_decode_attention_group" in lib.emmax_last_error()
        assert torch.isnan(got).all(), (kw, N)
