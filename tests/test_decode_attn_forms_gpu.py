"""The decode attention in every launched form (decode_attn.hip: launch_decode_attn, launch_group_attn; exact.hip: launch_x_decode_attn) against
the float64 reference of tests/decode_attn_ref.py: cases, input families, NaN-poisoned caches and the tolerance table live there (measured on the
CPU as |fp32 emulation - float64|; the bound is twice that, with the project's bf16 line as a floor for the bf16 rows only).

Every case asserts its launch plan (emmax_decode_attn_plan / emmax_group_attn_plan -- the launchers dispatch on the same struct) before it launches;
tests/test_decode_attn_plan.py proves on the CPU that the tags cover every plan a step or a group route can reach.  Each test prints the worst
measured error of every form next to its bound (pytest -s).

The symbols are looked up without a skip: on a library without them this file fails."""

import ctypes as C

import pytest
import torch

import decode_attn_ref as R
from test_decode_attn_plan import attn_plan, group_plan
from test_ops_gpu import _lib, assert_elementwise, stream

pytestmark = pytest.mark.gpu

MAX_SPLITS = 8   # partials per (row, head) the grouped workspace holds (include/emmax.h)
DONE_ROWS = (2, 7)


# ---- device operands -------------------------------------------------------------------------------------------------------------------------
def upload(c):
    dev = "cuda"
    d = dict(table=c.table.to(dev), ctx=torch.tensor(c.ctxs, dtype=torch.int32, device=dev), kv24=0)
    if c.kind in ("bf16", "fp8"):
        d["q"] = c.q.to(torch.bfloat16).view(c.B, c.Hq * R.HD).contiguous().to(dev)
        d["kc"], d["vc"] = c.kc.to(dev), c.vc.to(dev)
        if c.kind == "fp8":
            d["ks"], d["vs"], d["stage"] = c.ks.to(dev), c.vs.to(dev), c.stage.to(dev)
    else:
        d["q"] = c.q.view(c.B, c.Hq * R.HD).contiguous().to(dev)
        if c.kind == "x24":   # per operand: the bf16 plane, then the 8-bit extension plane (fp32 NaN: a bf16 NaN in the first, 0 in the second)
            for name, t in (("kc", c.kc), ("vc", c.vc)):
                hi, ext, back = R.x24_planes(t)
                assert torch.equal(torch.isnan(back), torch.isnan(t))
                d[name] = torch.cat([hi.view(torch.uint8).flatten(), ext.flatten()]).to(dev)
            d["kv24"] = c.kc.numel()
        else:
            d["kc"], d["vc"] = c.kc.to(dev), c.vc.to(dev)
    if c.groups:
        d["shared"] = torch.tensor([sh for _, sh in c.groups], dtype=torch.int32, device=dev)
    return d


def done_flags(c, rows):
    return torch.tensor([1 if b in rows else 0 for b in range(c.B)], dtype=torch.int32, device="cuda") if rows else None


def launch(c, d, direct, nsplit, done=None):
    """One launch through the pure op of the case's cache kind.  Returns dict(o [B, Hq, 128] float64 or fp32, and for the split forms part (raw), lse,
    on); the fp8 forms work on a copy of the cache and return it (kc, vc, ks, vs) for the append check."""
    L_, lib = _lib()
    B, Hq, Hkv, sc = c.B, c.Hq, c.Hkv, R.SCALE
    dn = done.data_ptr() if done is not None else None
    out = {}
    ns_out = C.c_int(nsplit)
    part = torch.full((B, Hq, 16, R.PSTRIDE), R.NAN, dtype=torch.float32, device="cuda")
    if c.kind == "bf16":
        if direct:
            o = torch.full((B, Hq * R.HD), R.NAN, dtype=torch.bfloat16, device="cuda")
            rc = lib.emmax_op_decode_attention_direct(d["q"].data_ptr(), d["kc"].data_ptr(), d["vc"].data_ptr(), d["table"].data_ptr(), d["ctx"].data_ptr(), dn,
                                                      o.data_ptr(), B, Hq, Hkv, c.page, c.max_pages, sc, stream())
        else:
            rc = lib.emmax_op_decode_attention(d["q"].data_ptr(), d["kc"].data_ptr(), d["vc"].data_ptr(), d["table"].data_ptr(), d["ctx"].data_ptr(), dn,
                                               part.data_ptr(), B, Hq, Hkv, c.page, c.max_pages, nsplit, sc, C.byref(ns_out), stream())
    elif c.kind == "fp8":
        kc, vc, ks, vs = d["kc"].clone(), d["vc"].clone(), d["ks"].clone(), d["vs"].clone()   # the launch appends the step's key
        o = torch.full((B, Hq * R.HD), R.NAN, dtype=torch.bfloat16, device="cuda")
        rc = lib.emmax_op_decode_attention_kv8(d["q"].data_ptr(), kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), d["stage"].data_ptr(),
                                               d["table"].data_ptr(), d["ctx"].data_ptr(), dn, None if direct else part.data_ptr(), o.data_ptr() if direct else None,
                                               B, Hq, Hkv, c.page, c.max_pages, nsplit, sc, stream())
        out.update(kc=kc, vc=vc, ks=ks, vs=vs)
    else:
        if direct:   # in place over q: a copy with a guard row on either side
            buf = torch.full((B + 2, Hq * R.HD), 12345.0, dtype=torch.float32, device="cuda")
            buf[1:B + 1] = d["q"]
            o = buf[1:B + 1]
            rc = lib.emmax_op_x_decode_attention_direct(o.data_ptr(), d["kc"].data_ptr(), d["vc"].data_ptr(), d["kv24"], d["table"].data_ptr(), d["ctx"].data_ptr(), dn,
                                                        B, Hq, Hkv, c.page, c.max_pages, sc, stream())
            torch.cuda.synchronize()
            assert (buf[0] == 12345.0).all() and (buf[B + 1] == 12345.0).all(), "the in-place row left its own columns"
        else:
            rc = lib.emmax_op_x_decode_attention(d["q"].data_ptr(), d["kc"].data_ptr(), d["vc"].data_ptr(), d["kv24"], d["table"].data_ptr(), d["ctx"].data_ptr(), dn,
                                                 part.data_ptr(), B, Hq, Hkv, c.page, c.max_pages, nsplit, sc, stream())
    torch.cuda.synchronize()
    L_.check(rc, f"decode attention {c.kind} direct={direct} nsplit={nsplit}")
    if direct:
        out["o"] = o.float().cpu().view(B, Hq, R.HD)
        out["raw"] = o.cpu()
    else:
        ns = ns_out.value if c.kind == "bf16" else nsplit
        out["ns"] = ns
        p = part.view(-1)[: B * Hq * ns * R.PSTRIDE].view(B, Hq, ns, R.PSTRIDE).cpu()
        assert torch.isnan(part.view(-1)[B * Hq * ns * R.PSTRIDE:]).all(), "wrote past the partials"
        out["raw"] = p
        out["o"], out["lse"], out["on"] = R.merge_partials(p, ns)
    return out


# ---- checks ----------------------------------------------------------------------------------------------------------------------------------
WORST = {}


def record(key, errs, tol):
    w = WORST.setdefault(key, {})
    for k, v in errs.items():
        if k in tol:
            w[k] = (max(w.get(k, (0.0, 0.0))[0], v), tol[k])


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\n== decode attention forms: worst measured error / bound ==")
    for key in sorted(WORST):
        print(f"{key}: " + "  ".join(f"{k} {v:.3g} / {b:.3g}" for k, (v, b) in sorted(WORST[key].items())))


def check_split(c, got, ref, refp, tol, what, fails):
    p, (lse_ref, _) = got["raw"], refp
    m, l, o = p[..., R.HD], p[..., R.HD + 1], p[..., : R.HD]
    if not torch.isfinite(o).all() or not torch.isfinite(l).all() or torch.isnan(m).any():
        fails.append(f"{what}: a NaN page, an unmasked key or a poisoned position was read ({int((~torch.isfinite(o)).sum())} o values not finite)")
        return
    empty = torch.isinf(lse_ref)
    assert torch.equal(torch.isinf(m) & (m < 0), empty), f"{what}: the empty splits are not the rule's"
    assert (l[empty] == 0).all() and (o[empty] == 0).all(), f"{what}: an empty split holds something"   # exactly (-inf, 0, 0 ...)
    errs = R.errors(c, dict(nsplit=got["ns"]), got, ref, refp)
    record(" ".join(what.split(" ")[:1] + [c.family]), errs, tol)
    for k, bound in tol.items():
        if errs[k] > bound:
            fails.append(f"{what}: {k} {errs[k]:.3g} > {bound:.3g}")


def check_row(c, got, ref, tol, what, fails):
    if not torch.isfinite(got["o"]).all():
        fails.append(f"{what}: a NaN page, an unmasked key or a poisoned position was read ({int((~torch.isfinite(got['o'])).sum())} values not finite)")
        return
    for b in c.done:
        assert (got["o"][b] == 0).all(), f"{what}: done row {b} is not zeros"
    errs = R.errors(c, dict(direct=1), got, ref)
    record(" ".join(what.split(" ")[:1] + [c.family]), errs, tol)
    for k, bound in tol.items():
        if errs[k] > bound:
            fails.append(f"{what}: {k} {errs[k]:.3g} > {bound:.3g}")
    if "spread" in tol:   # a bf16 row: the project's elementwise line at this form's atol
        try:
            assert_elementwise(got["o"], ref, rtol=R.BF16_RTOL, atol_frac=tol["spread"], what=what)
        except AssertionError as e:
            fails.append(str(e))


def check_append(c, got, rows_done, what):
    """fp8: bytes and scale of the step's key sit at position ctx of every live row; every other byte and scale is bit-unchanged"""
    for name, host, want8, wants in (("kc", c.kc, c.k8, c.ksc), ("vc", c.vc, c.v8, c.vsc)):
        exp8, exps = host.clone(), (c.ks if name == "kc" else c.vs).clone()
        for b, ctx in enumerate(c.ctxs):
            if b in rows_done:
                continue   # a done row appends nothing
            pg, sl = int(c.table[b, ctx // c.page]), ctx % c.page
            exp8[pg, :, sl], exps[pg, :, sl] = want8[b][ctx], wants[b][ctx]
        assert torch.equal(got[name].cpu(), exp8), f"{what}: {name} bytes"
        gs = got["ks" if name == "kc" else "vs"].cpu()
        assert torch.equal(gs.view(torch.int32), exps.view(torch.int32)), f"{what}: {name} scales"   # bit for bit, NaN poison included


def plan_of(lib, c, direct, nsplit):
    p = attn_plan(lib, c.B, c.Hq, c.Hkv, nsplit, direct, int(c.kind == "fp8"))
    return ("attn",) + p + (int(c.kind == "fp8"),)


def run_variants(kind, G, family, c, d, vs, fails, done=None):
    L_, lib = _lib()
    ref, refp = R.ref64(c), {}
    outs = {}
    for name, tune, direct, ns, plan in vs:
        with L_.tuning(**tune):
            if kind in ("bf16", "fp8"):
                assert plan_of(lib, c, direct, ns) == plan, (name, plan_of(lib, c, direct, ns), plan)   # the plan first, the launch second
            got = launch(c, d, direct, ns, done)
        what = f"{kind}/{'direct' if direct else 'split'} G{G} {family} {name}"
        tol = R.tolerances(kind, "direct" if direct else "split", family)
        if direct:
            check_row(c, got, ref, tol, what, fails)
        else:
            if ns not in refp:
                refp[ns] = R.ref_partials64(c, ns)
            check_split(c, got, ref, refp[ns], tol, what, fails)
        if kind == "fp8":
            check_append(c, got, c.done, what)
        outs[name] = got["raw"]
    return outs


# ---- every variant x every family at every context edge --------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("G", sorted(R.HEADS))
@pytest.mark.parametrize("kind", R.KINDS)
def test_every_form_at_every_context_edge(device, kind, G, family):
    """One launch of 19 rows (ragged: 14) per variant: L = ctx + 1 at every edge of the chunk loops of every CHK, empty trailing splits, a last split
    of exactly the new key -- under NaN poison."""
    c = R.edge_case(kind, G, family)
    fails = []
    run_variants(kind, G, family, c, upload(c), R.variants(kind, G), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("G", sorted(R.HEADS))
@pytest.mark.parametrize("kind", R.KINDS)
def test_done_rows_in_every_form(device, kind, G):
    """A done row: zeros from a direct form, empty partials from a split form, no fp8 append; every other row bit-equal to the launch without the flag."""
    live = R.edge_case(kind, G, "random")
    flagged = R.edge_case(kind, G, "random", done=DONE_ROWS)
    d = upload(live)
    fails = []
    a = run_variants(kind, G, "random", live, d, R.variants(kind, G), fails)
    b = run_variants(kind, G, "random", flagged, d, R.variants(kind, G), fails, done=done_flags(live, DONE_ROWS))
    assert not fails, "\n".join(fails)
    keep = [r for r in range(live.B) if r not in DONE_ROWS]
    for name in a:
        assert torch.equal(a[name][keep].view(torch.int32) if a[name].dtype == torch.float32 else a[name][keep].view(torch.int16),
                           b[name][keep].view(torch.int32) if b[name].dtype == torch.float32 else b[name][keep].view(torch.int16)), (name, "live rows changed")


# ---- bf16 forms a step reaches by shape, no switch set -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.BY_SHAPE, ids=lambda x: x[0])
def test_forms_reached_by_shape(device, case):
    name, B, Hq, Hkv, ns, direct, plan = case
    L_, lib = _lib()
    c = R.by_shape_case(case)
    p = attn_plan(lib, B, Hq, Hkv, ns, direct) if ns else attn_plan(lib, B, Hq, Hkv)
    assert ("attn",) + p + (0,) == plan
    got = launch(c, upload(c), direct, ns)
    fails, ref = [], R.ref64(c)
    if direct:
        check_row(c, got, ref, R.tolerances("bf16", None, None, shape="direct"), f"bf16/direct-by-shape {name}", fails)
    else:
        assert got["ns"] == plan[5]
        check_split(c, got, ref, R.ref_partials64(c, got["ns"]), R.tolerances("bf16", None, None, shape="split"), f"bf16/split-by-shape {name}", fails)
    assert not fails, "\n".join(fails)


# ---- the page table ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_pages,page,ctx", R.TABLES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_page_table_halves_clamp_and_page_size(device, kind, max_pages, page, ctx):
    """Up to 512 page ids sit in LDS in two halves (one with eight waves): a context that reaches the LAST entry of a 512-entry table, tables of
    256 and 257 entries around the min(tid + NT, max_pages - 1) clamp, a table of one entry, and 16-token pages through the ops."""
    c = R.table_case(kind, max_pages, page, ctx)
    vs = [("split1", {}, 0, 1, None), ("split8", {}, 0, 8, None), ("direct", {"attn_deep": 0}, 1, 1, None)]
    if kind == "bf16":
        vs += [("direct-nw8", {"attn_nw": 8, "attn_deep": 0}, 1, 1, None), ("direct-deep", {"attn_deep": 1}, 1, 1, None), ("split8-deep", {"attn_deep": 1}, 0, 8, None)]
    L_, lib = _lib()
    d, ref, fails = upload(c), R.ref64(c), []
    for name, tune, direct, ns, _ in vs:
        with L_.tuning(**tune):
            got = launch(c, d, direct, ns)
        what = f"{kind}/{'direct' if direct else 'split'}-table {max_pages}x{page} ctx {ctx} {name}"
        tol = R.tolerances(kind, None, None, table="direct" if direct else "split")
        if direct:
            check_row(c, got, ref, tol, what, fails)
        else:
            check_split(c, got, ref, R.ref_partials64(c, ns), tol, what, fails)
        if kind == "fp8":
            check_append(c, got, (), what)
    assert not fails, "\n".join(fails)


# ---- grouped: the shared span once per group, then the rows' tails -----------------------------------------------------------------------------
def launch_group(c, d, N, done=None):
    L_, lib = _lib()
    o = torch.full((c.B, c.Hq * R.HD), R.NAN, dtype=torch.bfloat16, device="cuda")
    ws = torch.full((c.B * c.Hq * MAX_SPLITS * R.PSTRIDE,), R.NAN, dtype=torch.float32, device="cuda")
    dn = done.data_ptr() if done is not None else None
    if c.kind == "fp8":
        kc, vc, ks, vs = d["kc"].clone(), d["vc"].clone(), d["ks"].clone(), d["vs"].clone()
        rc = lib.emmax_op_decode_attention_group_kv8(d["q"].data_ptr(), kc.data_ptr(), vc.data_ptr(), ks.data_ptr(), vs.data_ptr(), d["stage"].data_ptr(),
                                                     d["table"].data_ptr(), d["ctx"].data_ptr(), dn, ws.data_ptr(), o.data_ptr(), c.B, c.Hq, c.Hkv, c.page, c.max_pages, N,
                                                     d["shared"].data_ptr(), R.SCALE, stream())
        extra = dict(kc=kc, vc=vc, ks=ks, vs=vs)
    else:
        rc = lib.emmax_op_decode_attention_group(d["q"].data_ptr(), d["kc"].data_ptr(), d["vc"].data_ptr(), d["table"].data_ptr(), d["ctx"].data_ptr(), dn, o.data_ptr(),
                                                 c.B, c.Hq, c.Hkv, c.page, c.max_pages, R.SCALE, N, d["shared"].data_ptr(), ws.data_ptr(), stream())
        extra = {}
    torch.cuda.synchronize()
    L_.check(rc, "grouped decode attention")
    return dict(o=o.float().cpu().view(c.B, c.Hq, R.HD), **extra)


def _grouped(kind, family, g, done=()):
    name, groups, Hq, Hkv, plan = g
    _, lib = _lib()
    B, N = sum(n for n, _, _ in groups), groups[0][0]
    assert ("group",) + group_plan(lib, B, N, Hq, Hkv, int(kind == "fp8")) == plan
    c = R.grouped_case(name, kind, family)
    c.done = tuple(done)
    got = launch_group(c, upload(c), N, done_flags(c, done))
    fails = []
    check_row(c, got, R.ref64(c), R.tolerances(kind, "group", family), f"{kind}/group {name} {family}", fails)
    if kind == "fp8":
        check_append(c, got, done, name)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", R.GROUP_FAMILIES)
@pytest.mark.parametrize("g", R.GROUPED, ids=lambda g: g[0])
@pytest.mark.parametrize("kind", ("bf16", "fp8"))
def test_grouped_every_tail_and_span_width(device, kind, g, family):
    """Tail G 1 / 2 / 4 / 8, span widths 2 / 4 / 8, two and nine query chunks; sink = the dominant key inside the shared span, last = the row's own"""
    _grouped(kind, family, g, done=(1,) if family == "random" and g[0] == "g4-w8-2chunks" else ())


@pytest.mark.parametrize("g", R.GROUPED_WIDE, ids=lambda g: g[0])
@pytest.mark.parametrize("kind", ("bf16", "fp8"))
def test_grouped_span_split_counts(device, kind, g):
    """4 / 2 / 1 splits of the shared span, at every width and tail G that a step of 32 / 8 / 4 kv heads reaches"""
    _grouped(kind, "random", g)


# ---- exact numerics: the in-place one-split row ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", sorted(R.HEADS))
@pytest.mark.parametrize("kind", ("x32", "x24"))
def test_exact_in_place_row_is_the_one_split_merge(device, kind, G):
    """emmax_op_x_decode_attention_direct writes over q what the merge of the one-split partials gives: the same arithmetic, so within twice the
    emulation's spread of each other as well as of the reference; rows above and below the launch's are untouched (launch() holds guard rows)."""
    c = R.edge_case(kind, G, "random")
    d = upload(c)
    row, part = launch(c, d, 1, 1), launch(c, d, 0, 1)
    tol = R.tolerances(kind, "direct", "random")
    assert R.err_o(row["o"], part["o"]) <= tol["o"], R.err_o(row["o"], part["o"])
    _, lib = _lib()
    assert lib.emmax_op_x_decode_attention_direct(None, d["kc"].data_ptr(), d["vc"].data_ptr(), d["kv24"], d["table"].data_ptr(), d["ctx"].data_ptr(), None, c.B, c.Hq,
                                                  c.Hkv, c.page, c.max_pages, R.SCALE, stream()) == -1
    assert b"emmax_op_x_decode_attention_direct" in lib.emmax_last_error()
