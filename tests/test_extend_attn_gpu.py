"""The extension attention and the offset RoPE / append (emma-x_amd/csrc/extend_attn.hip) as pure ops.

1. emmax_op_extend_attention(_kv8) against the float64 reference of tests/extend_attn_ref.py: the (base, n) pairs at every loop edge in ONE launch
   of 23 sequences (a ragged B = 3 launch as well), GQA groups 1 / 2 / 4 / 8, 1 / 2 / 3 splits and the planner's choice, bf16 and e4m3 caches
   poisoned with NaN wherever no row reads.  Bounds: 2 x the CPU-measured |emu32 - ref64| (the bf16 rows: never below the project's line; the fp32
   partials: no floor).  Every launch asserts its plan first; tests/test_extend_attn_ref.py proves the tags cover every plan.
2. emmax_op_rope_kv_write_at against emmax_op_rope_kv_write over the whole sequence at the same positions: bit for bit, and nothing outside
   [base, base + n) is touched in a NaN-poisoned cache.

The symbols are looked up without a skip: on a library without them this file fails."""

import ctypes as C

import pytest
import torch

import extend_attn_ref as X
from test_extend_attn_ref import plan
from test_ops_gpu import _lib, stream

pytestmark = pytest.mark.gpu

ERR_INVALID = -1   # include/emmax.h: emmax_status
_CASES, _REFS = {}, {}


def case_of(kind, G, which):
    key = (kind, G, which)
    if key not in _CASES:   # built once, shared by the split counts, never changed
        c = _CASES[key] = X.edge_case(kind, G) if which == "edge" else X.ragged_case(kind, G)
        _REFS[key] = X.ref64(c)
    return _CASES[key], _REFS[key]


def launch(c, nsplit):
    """one launch through the op of the case's cache kind: dict(o [total, Hq, 128], ns, and with more than one split po / plse from the partials)"""
    L_, lib = _lib()
    dev = "cuda"
    q = c.q.to(torch.bfloat16).view(c.total, c.Hq * X.HD).contiguous().to(dev)
    cu = torch.tensor(c.cu, dtype=torch.int32, device=dev)
    base = torch.tensor(c.base, dtype=torch.int32, device=dev)
    table, kc, vc = c.table.to(dev), c.kc.to(dev), c.vc.to(dev)
    out = torch.full((c.total, c.Hq * X.HD), X.NAN, dtype=torch.bfloat16, device=dev)
    ws_floats = c.total * c.Hq * 16 * X.PSTRIDE
    ws = torch.full((ws_floats + 64,), X.NAN, dtype=torch.float32, device=dev)
    max_n, max_L = max(c.n), max(b + n for b, n in c.pairs)
    p = plan(lib, c.B, max_n, max_L, c.Hq, c.Hkv, nsplit, 1 if c.kind == "fp8" else 0)
    want = X.expected_nsplit(c.B, max_n, max_L, c.Hq, c.Hkv, nsplit)
    assert p is not None and p[0] == c.G and p[3] == want and X.plan_tag(p[0], c.kind == "fp8", p[4]) in X.case_plans(), p
    ns_out = C.c_int(-1)
    if c.kind == "bf16":
        rc = lib.emmax_op_extend_attention(q.data_ptr(), c.Hq * X.HD, 0, kc.data_ptr(), vc.data_ptr(), table.data_ptr(), cu.data_ptr(), base.data_ptr(), c.B, c.total,
                                           c.Hq, c.Hkv, X.PAGE, c.max_pages, nsplit, X.SCALE, out.data_ptr(), c.Hq * X.HD, ws.data_ptr(), ws_floats, C.byref(ns_out),
                                           stream())
    else:
        ks, vs = c.ks.to(dev), c.vs.to(dev)
        rc = lib.emmax_op_extend_attention_kv8(q.data_ptr(), c.Hq * X.HD, 0, kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), table.data_ptr(),
                                               cu.data_ptr(), base.data_ptr(), c.B, c.total, c.Hq, c.Hkv, X.PAGE, c.max_pages, nsplit, X.SCALE, out.data_ptr(),
                                               c.Hq * X.HD, ws.data_ptr(), ws_floats, C.byref(ns_out), stream())
    torch.cuda.synchronize()
    L_.check(rc, f"extend attention {c.kind} G={c.G} nsplit={nsplit}")
    ns = ns_out.value
    assert ns == want
    got = dict(o=out.float().cpu().view(c.total, c.Hq, X.HD), ns=ns)
    used = c.total * c.Hq * ns * X.PSTRIDE if ns > 1 else 0
    assert torch.isnan(ws[used:]).all(), "wrote past the partials"
    if ns > 1:
        part = ws[:used].view(c.total, c.Hq, ns, X.PSTRIDE).cpu()
        got["part"] = part
        got["po"], got["plse"] = X.merge_partials(part)
    return got


def check(c, ref, got, what):
    ns = got["ns"]
    tol = X.tolerances(c.kind, ns > 1)
    assert torch.isfinite(got["o"]).all(), f"{what}: a NaN page, an unmasked key or a poisoned position was read"
    if ns > 1:
        o, m, l = got["part"][..., : X.HD], got["part"][..., X.HD], got["part"][..., X.HD + 1]
        assert torch.isfinite(o).all() and torch.isfinite(l).all() and not torch.isnan(m).any(), f"{what}: NaN in the partials"
        # the empty (row, split) pairs are the rule's: split s of a row at position pos holds keys [k0, min(k1, pos + 1))
        for b in range(c.B):
            L = c.base[b] + c.n[b]
            for s in range(ns):
                k0, _ = X.split_range(L, ns, s)
                pos = c.base[b] + torch.arange(c.n[b])
                empty = (pos < k0)[:, None].expand(-1, c.Hq)
                mm = m[c.cu[b]:c.cu[b + 1], :, s]
                assert torch.equal(torch.isinf(mm) & (mm < 0), empty), f"{what}: sequence {b} split {s}: the empty partials are not the rule's"
                assert (l[c.cu[b]:c.cu[b + 1], :, s][empty] == 0).all() and (o[c.cu[b]:c.cu[b + 1], :, s][empty] == 0).all()
    errs = X.errors(c, got, ref, ns > 1)
    print(f"{what}: " + "  ".join(f"{k} {errs[k]:.3g} / {tol[k]:.3g}" for k in sorted(errs)))
    bad = [f"{k} {errs[k]:.3g} > {tol[k]:.3g}" for k in errs if errs[k] > tol[k]]
    assert not bad, f"{what}: " + ", ".join(bad)


@pytest.mark.parametrize("nsplit", X.NSPLITS)
@pytest.mark.parametrize("G", sorted(X.HEADS))
@pytest.mark.parametrize("kind", X.KINDS)
def test_extend_attention_at_every_loop_edge(device, kind, G, nsplit):
    c, ref = case_of(kind, G, "edge")
    check(c, ref, launch(c, nsplit), f"{kind} G={G} nsplit={nsplit}")


@pytest.mark.parametrize("G", sorted(X.HEADS))
@pytest.mark.parametrize("kind", X.KINDS)
def test_extend_attention_ragged_three_sequences(device, kind, G):
    c, ref = case_of(kind, G, "ragged")
    for nsplit in (1, 0):
        check(c, ref, launch(c, nsplit), f"ragged {kind} G={G} nsplit={nsplit}")


def test_extend_attention_refuses_what_it_cannot_index(device):
    L_, lib = _lib()
    c, _ = case_of("bf16", 2, "ragged")
    dev = "cuda"
    q = torch.zeros(c.total, c.Hq * X.HD, dtype=torch.bfloat16, device=dev)
    out = torch.zeros_like(q)
    cu = torch.tensor(c.cu, dtype=torch.int32, device=dev)
    table, kc, vc = c.table.to(dev), c.kc.to(dev), c.vc.to(dev)

    def call(base, max_pages=c.max_pages, nsplit=1, ws=None, ws_floats=0, page=X.PAGE):
        b = torch.tensor(base, dtype=torch.int32, device=dev)
        return lib.emmax_op_extend_attention(q.data_ptr(), c.Hq * X.HD, 0, kc.data_ptr(), vc.data_ptr(), table.data_ptr(), cu.data_ptr(), b.data_ptr(), c.B, c.total, c.Hq,
                                             c.Hkv, page, max_pages, nsplit, X.SCALE, out.data_ptr(), c.Hq * X.HD, ws, ws_floats, None, stream())

    assert call(c.base) == 0
    assert call([c.max_pages * X.PAGE] + c.base[1:]) == ERR_INVALID and "page table" in lib.emmax_last_error().decode()   # base + n past the table
    assert call([-1] + c.base[1:]) == ERR_INVALID
    assert call(c.base, nsplit=2) == ERR_INVALID and "workspace" in lib.emmax_last_error().decode()                          # splits without partials
    assert call(c.base, page=32) == ERR_INVALID
    torch.cuda.synchronize()


# ---- the offset RoPE / append ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (2, 2)])
def test_rope_kv_write_at_equals_the_whole_sequence_pass_bit_for_bit(device, Hq, Hkv):
    L_, lib = _lib()
    dev, hd, page, max_pages, max_pos = "cuda", 128, 64, 6, 384
    pairs = [(0, 3), (63, 2), (64, 65), (200, 31), (1, 1)]
    B = len(pairs)
    g = torch.Generator().manual_seed(5)
    ld = (Hq + 2 * Hkv) * hd
    pos = torch.arange(max_pos, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(0, hd, 2, dtype=torch.float64) / hd))[None, :]
    cos_t, sin_t = pos.cos().float().to(dev), pos.sin().float().to(dev)
    table = torch.randperm(B * max_pages, generator=g).view(B, max_pages).to(torch.int32).to(dev)
    poison = torch.full((B * max_pages, Hkv, page, hd), X.NAN).to(torch.bfloat16).to(dev)
    # the whole sequences (reference) and their last n rows (the extension), packed
    whole = [torch.randn(b + n, ld, generator=g).to(torch.bfloat16) for b, n in pairs]
    cu_w = torch.tensor([0] + list(torch.tensor([b + n for b, n in pairs]).cumsum(0)), dtype=torch.int32, device=dev)
    cu_x = torch.tensor([0] + list(torch.tensor([n for _, n in pairs]).cumsum(0)), dtype=torch.int32, device=dev)
    base = torch.tensor([b for b, _ in pairs], dtype=torch.int32, device=dev)
    qkv_w = torch.cat(whole).to(dev)
    qkv_x = torch.cat([w[b:] for w, (b, n) in zip(whole, pairs)]).to(dev)
    total_w, total_x = qkv_w.shape[0], qkv_x.shape[0]
    kc_w, vc_w, kc_x, vc_x = poison.clone(), poison.clone(), poison.clone(), poison.clone()
    L_.check(lib.emmax_op_rope_kv_write(qkv_w.data_ptr(), ld, 0, Hq * hd, (Hq + Hkv) * hd, cu_w.data_ptr(), B, total_w, cos_t.data_ptr(), sin_t.data_ptr(), kc_w.data_ptr(),
                                        vc_w.data_ptr(), table.data_ptr(), max_pages, Hq, Hkv, hd, page, stream()), "rope_kv_write")
    L_.check(lib.emmax_op_rope_kv_write_at(qkv_x.data_ptr(), ld, 0, Hq * hd, (Hq + Hkv) * hd, cu_x.data_ptr(), base.data_ptr(), B, total_x, cos_t.data_ptr(),
                                           sin_t.data_ptr(), max_pos, kc_x.data_ptr(), vc_x.data_ptr(), table.data_ptr(), max_pages, Hq, Hkv, hd, page, stream()),
             "rope_kv_write_at")
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16).cpu()
    # the rotated rows themselves
    want = torch.cat([qkv_w[int(cu_w[i]) + b: int(cu_w[i + 1])] for i, (b, n) in enumerate(pairs)])
    assert torch.equal(bits(qkv_x), bits(want)), "the rotated q / k rows differ from the whole-sequence pass"
    # the cache: the new positions equal the whole-sequence pass, every other position still holds the poison
    tab = table.cpu()
    new = torch.zeros(B * max_pages, page, dtype=torch.bool)
    for i, (b, n) in enumerate(pairs):
        for p in range(b, b + n):
            new[int(tab[i, p // page]), p % page] = True
    for got, ref in ((kc_x, kc_w), (vc_x, vc_w)):
        gb, rb, pb = bits(got), bits(ref), bits(poison)
        sel = new[:, None, :, None].expand_as(gb)
        assert torch.equal(gb[sel], rb[sel]), "the appended rows differ from the whole-sequence pass"
        assert not torch.isnan(got.float().cpu()[sel]).any()
        assert torch.equal(gb[~sel], pb[~sel]), "a position outside [base, base + n) was written"
    # refusals: a position past the RoPE tables / the page table
    far = torch.tensor([max_pos] + [b for b, _ in pairs[1:]], dtype=torch.int32, device=dev)
    assert lib.emmax_op_rope_kv_write_at(qkv_x.data_ptr(), ld, 0, Hq * hd, (Hq + Hkv) * hd, cu_x.data_ptr(), far.data_ptr(), B, total_x, cos_t.data_ptr(), sin_t.data_ptr(),
                                         max_pos, kc_x.data_ptr(), vc_x.data_ptr(), table.data_ptr(), max_pages, Hq, Hkv, hd, page, stream()) == ERR_INVALID
    torch.cuda.synchronize()
