"""The taps' kernels (emma-x_amd/csrc/taps.hip) as pure ops.

1. emmax_op_attn_probs(_kv8) against the float64 reference of tests/taps_ref.py: extend_attn_ref's (base, n) pairs at every loop edge in ONE launch
   of 23 sequences and its ragged B = 3 launch, GQA groups 1 / 2 / 4 / 8, bf16 and e4m3 caches poisoned with NaN wherever no row reads (fp8: the
   reference attends over the de-quantised keys).  The output buffer is NaN before the launch: afterwards every entry of every live row is finite,
   the entries behind the diagonal are exactly 0.0 through ld_keys - 1, and the padding rows past total_rows are still NaN.  ld_keys at its minimum
   and larger than needed.  Bounds: FACTOR x the CPU-measured |emu32 - ref64|, no floor.
2. emmax_op_tap_rows against float64: the plain copy bit for bit, the normed form within its bound; fp32 and bf16 sources, a padded source pitch.

The symbols are looked up without a skip: on a library without them this file fails."""

import pytest
import torch

import taps_ref as T
from test_ops_gpu import _lib, stream

pytestmark = pytest.mark.gpu

ERR_INVALID = -1   # include/emmax.h: emmax_status
PAD_ROWS = 2
_CASES, _REFS = {}, {}


def case_of(kind, G, which):
    key = (kind, G, which)
    if key not in _CASES:   # built once, shared, never changed
        _CASES[key] = T.edge_case(kind, G) if which == "edge" else T.ragged_case(kind, G)
    return _CASES[key]


def ref_of(kind, G, which, ld_keys):
    key = (kind, G, which, ld_keys)
    if key not in _REFS:
        _REFS[key] = T.ref64_probs(case_of(kind, G, which), ld_keys)
    return _REFS[key]


def call(lib, c, q, kc, ks, table, cu, base, probs, ld_keys, Hq=None, Hkv=None, page=T.PAGE):
    Hq, Hkv = Hq or c.Hq, Hkv or c.Hkv
    if c.kind == "bf16":
        return lib.emmax_op_attn_probs(q.data_ptr(), c.Hq * T.HD, 0, kc.data_ptr(), table.data_ptr(), cu.data_ptr(), base.data_ptr(), c.B, c.total, Hq, Hkv, page,
                                       c.max_pages, T.SCALE, probs.data_ptr(), ld_keys, stream())
    return lib.emmax_op_attn_probs_kv8(q.data_ptr(), c.Hq * T.HD, 0, kc.data_ptr(), ks.data_ptr(), table.data_ptr(), cu.data_ptr(), base.data_ptr(), c.B, c.total, Hq,
                                       Hkv, page, c.max_pages, T.SCALE, probs.data_ptr(), ld_keys, stream())


def device_case(c):
    dev = "cuda"
    return dict(q=c.q.to(torch.bfloat16).view(c.total, c.Hq * T.HD).contiguous().to(dev), kc=c.kc.to(dev), ks=c.ks.to(dev) if c.kind == "fp8" else None,
                table=c.table.to(dev), cu=torch.tensor(c.cu, dtype=torch.int32, device=dev), base=torch.tensor(c.base, dtype=torch.int32, device=dev))


def launch(c, ld_keys):
    L_, lib = _lib()
    d = device_case(c)
    probs = torch.full((c.total + PAD_ROWS, c.Hq, ld_keys), T.NAN, dtype=torch.float32, device="cuda")
    rc = call(lib, c, probs=probs, ld_keys=ld_keys, **d)
    torch.cuda.synchronize()
    L_.check(rc, f"attn probs {c.kind} G={c.G} ld_keys={ld_keys}")
    return probs.cpu()


def check(c, ref, got, what):
    live, pad = got[: c.total], got[c.total:]
    assert torch.isnan(pad).all(), f"{what}: rows past total_rows were written"
    assert torch.isfinite(live).all(), f"{what}: a live row holds an entry that was not written, or a NaN page / poisoned position was read"
    errs, tol = T.errors(c, live, ref), T.tolerances(c.kind)
    print(f"{what}: above {errs['above']}  " + "  ".join(f"{k} {errs[k]:.3g} / {tol[k]:.3g}" for k in sorted(tol)))
    assert errs["above"] == 0, f"{what}: {errs['above']} non-zero entries behind the diagonal"
    bad = [f"{k} {errs[k]:.3g} > {tol[k]:.3g}" for k in tol if errs[k] > tol[k]]
    assert not bad, f"{what}: " + ", ".join(bad)


@pytest.mark.parametrize("G", sorted(T.HEADS))
@pytest.mark.parametrize("kind", T.KINDS)
def test_probabilities_at_every_loop_edge(device, kind, G):
    c = case_of(kind, G, "edge")
    ld = T.min_ld_keys(c)   # 1028: the 17-page row's keys exactly
    assert ld == T.max_keys(c)
    check(c, ref_of(kind, G, "edge", ld), launch(c, ld), f"{kind} G={G} ld_keys={ld}")


@pytest.mark.parametrize("G", sorted(T.HEADS))
@pytest.mark.parametrize("kind", T.KINDS)
def test_probabilities_ragged_three_sequences_at_the_smallest_and_a_larger_ld_keys(device, kind, G):
    c = case_of(kind, G, "ragged")
    for ld in (T.min_ld_keys(c), T.min_ld_keys(c) + 4, 5 * T.PAGE + 8):   # 204: inside a tile; 208; 328: a tile no block computes, and a partial one
        check(c, ref_of(kind, G, "ragged", ld), launch(c, ld), f"ragged {kind} G={G} ld_keys={ld}")


def test_probabilities_refuse_what_they_cannot_index(device):
    L_, lib = _lib()
    c = case_of("bf16", 2, "ragged")
    d = device_case(c)
    ld = T.min_ld_keys(c)
    probs = torch.full((c.total, c.Hq, ld), T.NAN, dtype=torch.float32, device="cuda")
    assert call(lib, c, probs=probs, ld_keys=ld, **d) == 0
    assert call(lib, c, probs=probs, ld_keys=ld - 4, **d) == ERR_INVALID and "ld_keys" in lib.emmax_last_error().decode()   # too small for the longest row
    assert call(lib, c, probs=probs, ld_keys=ld + 2, **d) == ERR_INVALID and "multiple of 4" in lib.emmax_last_error().decode()
    assert call(lib, c, probs=probs, ld_keys=ld, Hq=6, Hkv=2, **d) == ERR_INVALID and "GQA" in lib.emmax_last_error().decode()   # group 3
    assert call(lib, c, probs=probs, ld_keys=ld, page=32, **d) == ERR_INVALID
    far = dict(d, base=torch.tensor([c.max_pages * T.PAGE] + c.base[1:], dtype=torch.int32, device="cuda"))
    assert call(lib, c, probs=probs, ld_keys=ld, **far) == ERR_INVALID and "page table" in lib.emmax_last_error().decode()
    torch.cuda.synchronize()


# ---- the row copy --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["f32", "bf16"])
@pytest.mark.parametrize("rows,H", T.ROWS_SHAPES)
def test_tap_rows_copy_is_exact_and_the_norm_is_within_its_bound(device, rows, H, src):
    L_, lib = _lib()
    x, w = T.rows_case(rows, H, 77 + T.ROWS_SHAPES.index((rows, H)))
    if src == "bf16":
        x = T.X.bf(x)
    ld = H + 16   # a padded pitch: the row stride is the source's, not H
    xs = torch.full((rows, ld), T.NAN)
    xs[:, :H] = x
    xd = (xs if src == "f32" else xs.to(torch.bfloat16)).cuda()
    wd = w.to(torch.bfloat16).cuda()
    for normed in (False, True):
        out = torch.full((rows + 1, H), T.NAN, dtype=torch.float32, device="cuda")
        L_.check(lib.emmax_op_tap_rows(xd.data_ptr(), 1 if src == "f32" else 0, ld, out.data_ptr(), rows, H, wd.data_ptr() if normed else None, 1e-6, stream()),
                 "tap_rows")
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.isnan(got[rows]).all(), "a row past `rows` was written"
        if not normed:
            assert torch.equal(got[:rows], x.float()), "the copy is not bit for bit"
        else:
            e, tol = T.err_rows(got[:rows], T.ref64_rows(x, w)), T.tolerances("rows")["normed"]
            print(f"tap_rows {src} [{rows}, {H}] normed: {e:.3g} / {tol:.3g}")
            assert e <= tol
    assert lib.emmax_op_tap_rows(xd.data_ptr(), 1, ld, out.data_ptr(), rows, H + 4, None, 1e-6, stream()) == ERR_INVALID
