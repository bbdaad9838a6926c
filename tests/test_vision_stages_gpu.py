"""The vision encode's stages and glue kernels one by one on a real MI355X: the glue kernels through their pure ops (include/emmax.h), the
stages of the bf16 encode through emmax_op_vision_stage -- the encode's own stage functions (csrc/vision.hip) -- each against the float64 or
exact reference of tests/vision_stage_ref.py.  The weights are that module's discriminating state dict, not synthetic_state_dict.

Every output is pre-filled with a finite sentinel bit pattern, and everything an op must not write -- padding columns, rows past the last,
the other tower's feature columns -- is compared bitwise afterwards.  The bounds are the CPU emulation's (vision_stage_ref.py, pinned by
tests/test_vision_stage_ref.py); the ops with one right answer are compared bit for bit.

What the obvious breaks do to this file -- each was built into a scratch copy of the library (all in-bounds value errors) and this file run
against it once:
  ls1 and ls2 swapped (vision.hip)             -> test_block_stages fails at proj on all 8 tower-0 cases: 2.3e5 .. 6.2e6 x the bound (tower 1 has
                                                  no LayerScale)
  proj_b and fc2_b swapped                     -> test_block_stages fails at proj on all 16 cases: 2.4e4 .. 5e4 x (tower 0), 1.2e6 .. 1.8e6 x (tower 1)
  std[1] and std[2] swapped in the gather      -> the uint8 gather differs from the fp32 emulation at tower 0's and the odd normalisation (10584 of
                                                  17280 elements at (42, 14, 640, 3)); pixels != uint8 on preprocessed frames, in the gather op and in
                                                  the embed stage of tower 0.  (Tower 1's std is 0.5 everywhere: it cannot tell.  The embed stage's
                                                  BOUND does not see 0.224 for 0.225 either -- the exact comparisons do.)
  chan0 ignored in the pixel form              -> all 3 test_patch_gather_from_pixels cases fail at chan0 = 3; pixels != uint8 in the gather op (tower 1)
                                                  and in test_embed_stage[siglip]
  registers in reverse order                   -> test_assemble_tokens fails in the forms with registers, (1, 4) and (0, 2), bf16 and fp32;
                                                  test_embed_stage[dino] misses the bound by 108 x
  col_off 0 for tower 1                        -> test_features_stage fails at tower 1, and the chain's features differ from the encode's
  first pass only of misc.hip's vision loops   -> every gather case (the padding and everything past column 256 keep the sentinel), assemble at
                                                  D = 264, test_copy_rows_wider_than_one_pass, every embed stage (61 .. 84 x), the shared-scratch case
  row_stats without its stride                 -> both test_row_stats_grid_stride_loop cases: the rows of the second pass keep the sentinel
  ln_c without the bias                        -> test_ln_fold wherever there is a bias (ln_c off by 0.26 of its terms' magnitudes against a bound of
                                                  1.2e-7), every folded qkv / fc1 stage: 110 .. 167 x
  variance about zero                          -> every row_stats case, every folded qkv / fc1 stage: 37 .. 117 x
"""

import ctypes as C

import pytest
import torch

import vision_stage_ref as R

pytestmark = pytest.mark.gpu

S16, S32 = 0x5A5B, 0x5A5B5C5D   # sentinel bit patterns (finite values in every format)
EPS = 1e-6


def _lib():
    from emmax import _lib

    return _lib, _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sent_bf16(shape, device):
    return torch.full(shape, S16, dtype=torch.int16, device=device).view(torch.bfloat16)


def sent_f32(shape, device):
    return torch.full(shape, S32, dtype=torch.int32, device=device).view(torch.float32)


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


def untouched(t):
    """every element of `t` still holds its sentinel"""
    return t.numel() == 0 or bool((bits(t) == (S16 if t.element_size() == 2 else S32)).all())


def f3(v):
    return (C.c_float * 3)(*v)


def finite_bf16(shape, seed, device):
    """random finite bf16 values that are no sentinel: what a padding column or a neighbour's column may hold"""
    return R.bf(torch.randn(shape, generator=R.gen(211, seed)) * 3.0).to(device)


# =============================================================================================================================================
# patch gather
# =============================================================================================================================================
def _u8_frames(B, img, seed):
    """uint8 [B, img, img, 3] with all 256 values in every channel of every frame"""
    u = torch.randint(0, 256, (B, img, img, 3), generator=R.gen(201, seed, B, img), dtype=torch.uint8)
    u.view(B, img * img, 3)[:, :256, :] = torch.arange(256, dtype=torch.uint8).view(1, 256, 1)
    return u


def _gather(device, src, B, img, patch, kpad, chan0, mean, std, from_u8, hl):
    L, lib = _lib()
    rows, w = B * (img // patch) ** 2, (2 if hl else 1) * kpad
    out = sent_bf16((rows + 1, w), device)
    rc = lib.emmax_op_patch_gather(src.data_ptr(), out.data_ptr(), B, img, patch, kpad, chan0, f3(mean), f3(std), int(from_u8), int(hl), stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.emmax_last_error()
    assert untouched(out[rows:]), "a row past the last patch was written"
    return bits(out[:rows])


GATHER_SHAPES = [(28, 14, 640, 2), (32, 16, 768, 1), (42, 14, 640, 3)]   # three passes of the 256-thread loop + zero padding; no padding; a 3 x 3 grid


@pytest.mark.parametrize("norm", ["tower0", "tower1", "odd"])
@pytest.mark.parametrize("img,patch,kpad,B", GATHER_SHAPES)
def test_patch_gather_from_uint8(device, img, patch, kpad, B, norm):
    """bf16 of the three fp32 operations, and both planes of the HL form, bit for bit (HIP's fp32 divide is correctly rounded; no fast-math)"""
    cfg = R.cfg_tiny()
    mean, std = {"tower0": (cfg.towers[0].mean, cfg.towers[0].std), "tower1": (cfg.towers[1].mean, cfg.towers[1].std), "odd": (R.ODD_MEAN, R.ODD_STD)}[norm]
    u = _u8_frames(B, img, 0)
    v32 = R.pad_cols(R.patches_of(R.emu_normalize(u, mean, std), patch), kpad)
    ud = u.to(device)
    got = _gather(device, ud, B, img, patch, kpad, 0, mean, std, True, False)
    ref = R.bf16_bits_rne(v32)
    n_bad = int((got != ref).sum())
    print(f"uint8 gather {norm} ({img}, {patch}, {kpad}, {B}): {n_bad} of {ref.numel()} elements differ from the fp32 emulation")
    assert n_bad == 0
    got_hl = _gather(device, ud, B, img, patch, kpad, 0, mean, std, True, True)
    assert torch.equal(got_hl, R.hl_rows(v32)), "HL planes: hi = bf16(v), lo = bf16(v - hi)"


@pytest.mark.parametrize("img,patch,kpad,B", GATHER_SHAPES)
def test_patch_gather_from_pixels(device, img, patch, kpad, B):
    """pixel_values bf16 [B, 6, img, img] whose two halves differ: chan0 = 0 and 3 pick their own half; HL: lo = +0"""
    px = R.bf(torch.randn(B, 6, img, img, generator=R.gen(203, img)))
    pd = px.to(device)
    for chan0 in (0, 3):
        ref = R.bits16(R.pad_cols(R.patches_of(px[:, chan0:chan0 + 3], patch), kpad))
        assert torch.equal(_gather(device, pd, B, img, patch, kpad, chan0, (0, 0, 0), (1, 1, 1), False, False), ref), chan0
        ref_hl = R.hl_rows(R.pad_cols(R.patches_of(px[:, chan0:chan0 + 3].float(), patch), kpad))
        assert torch.equal(_gather(device, pd, B, img, patch, kpad, chan0, (0, 0, 0), (1, 1, 1), False, True), ref_hl), chan0


def test_patch_gather_pixels_equal_uint8_on_preprocessed_frames(device):
    """The pixel path reads bf16(preprocess(u)); the uint8 path rounds the same fp32 values once: the two gathers are bit-identical, tower by
    tower -- which is why emmax_vision_encode_pixels reproduces emmax_vision_encode exactly on such pixels (tests/test_e2e_gpu.py)"""
    from oracle import emmax_oracle as orc

    cfg = R.cfg_tiny()
    u = _u8_frames(2, 28, 1)
    pix = orc.preprocess_frames(u.numpy(), cfg).to(torch.bfloat16).to(device).contiguous()   # (the oracle hands back channels-last strides)
    for t, tw in enumerate(cfg.towers):
        a = _gather(device, u.to(device), 2, 28, 14, 640, 0, tw.mean, tw.std, True, False)
        b = _gather(device, pix, 2, 28, 14, 640, 3 * t, tw.mean, tw.std, False, False)
        assert torch.equal(a, b), t


# =============================================================================================================================================
# assemble tokens, copy rows, x_to_bf16
# =============================================================================================================================================
@pytest.mark.parametrize("f32", [0, 1], ids=["bf16", "fp32"])
@pytest.mark.parametrize("has_cls,n_reg", [(1, 4), (0, 0), (1, 0), (0, 2)])
def test_assemble_tokens(device, has_cls, n_reg, f32):
    """(D, ld) = (128, 128), (144, 256), (264, 384: two loop passes); 4 patches; B = 1, 3.  Real columns bit for bit (one fp32 add of two bf16
    values and one rounding; fp32 form: the exact sum).  Columns D .. ld: the bf16 form leaves them alone, the fp32 form writes zeros."""
    L, lib = _lib()
    n_p = 4
    for D, ld in ((128, 128), (144, 256), (264, 384)):
        for B in (1, 3):
            g = R.gen(205, has_cls, n_reg, D, B)
            pos, cls = R.bf(torch.randn(n_p, D, generator=g)), R.bf(2.0 + torch.randn(D, generator=g))
            reg = R.bf(torch.randn(n_reg, D, generator=g) + torch.arange(1, n_reg + 1).view(-1, 1)) if n_reg else None
            pe = torch.randn(B * n_p, ld, generator=g)            # the padding columns of pe hold finite values too
            pe = pe if f32 else R.bf(pe)
            N = has_cls + n_reg + n_p
            tokens = (sent_f32 if f32 else sent_bf16)((B * N + 1, ld), device)
            dv = [None if t is None else t.to(device) for t in (pe, pos, cls if has_cls else None, reg)]
            rc = lib.emmax_op_assemble_tokens(dv[0].data_ptr(), dv[1].data_ptr(), L.ptr(dv[2]), L.ptr(dv[3]), tokens.data_ptr(), B, n_p, has_cls, n_reg, D, ld, f32, stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.emmax_last_error()
            ref = R.ref_assemble_bits(pe[:, :D], pos, cls, reg, B, has_cls, f32=bool(f32)).reshape(B * N, D)
            got = tokens[: B * N]
            what = (has_cls, n_reg, D, ld, B)
            if f32:
                assert torch.equal(bits(got[:, :D]), bits(ref)), what
                assert bool((bits(got[:, D:]) == 0).all()), ("the fp32 form zeroes the padding columns", what)
            else:
                assert torch.equal(bits(got[:, :D]), ref), what
                assert untouched(got[:, D:]), ("the bf16 form leaves the padding columns alone", what)
            assert untouched(tokens[B * N:]), what


@pytest.mark.parametrize("B", [1, 3])
def test_copy_rows_into_the_feature_columns(device, B):
    """the tiny towers' shapes: 256 of 261 rows of D = 128 (pitch 128, r_off 5) to columns 0 .. 127, then 256 rows of D = 144 (pitch 256) to
    columns 128 .. 271 of one [B 256, 384] buffer: neither launch touches the other's columns, the padding or the row behind"""
    L, lib = _lib()
    n_p = 256
    out = sent_bf16((B * n_p + 1, 384), device)
    a = finite_bf16((B * 261, 128), 1, device)
    b = finite_bf16((B * 256, 256), 2, device)
    L.check(lib.emmax_op_copy_rows(a.data_ptr(), 128, out.data_ptr(), B, 261, 5, n_p, 128, 384, 0, stream()), "copy_rows")
    torch.cuda.synchronize()
    ref_a = a.view(B, 261, 128)[:, 5:].reshape(B * n_p, 128)
    assert torch.equal(bits(out[:-1, :128]), bits(ref_a)) and untouched(out[:, 128:]) and untouched(out[-1:])
    L.check(lib.emmax_op_copy_rows(b.data_ptr(), 256, out.data_ptr(), B, 256, 0, n_p, 144, 384, 128, stream()), "copy_rows")
    torch.cuda.synchronize()
    assert torch.equal(bits(out[:-1, :128]), bits(ref_a)), "tower 1's copy wrote tower 0's columns"
    assert torch.equal(bits(out[:-1, 128:272]), bits(b[:, :144])) and untouched(out[:, 272:]) and untouched(out[-1:])


def test_copy_rows_wider_than_one_pass(device):
    """D = 1152 (the full-size SigLIP): 144 sixteen-byte pieces per row for 128 threads, so the loop runs twice; into columns 1024 .. 2175"""
    L, lib = _lib()
    B, rows_in, r_off, rows_out = 2, 7, 2, 5
    src = finite_bf16((B * rows_in, 1160), 4, device)
    out = sent_bf16((B * rows_out + 1, 2184), device)
    L.check(lib.emmax_op_copy_rows(src.data_ptr(), 1160, out.data_ptr(), B, rows_in, r_off, rows_out, 1152, 2184, 1024, stream()), "copy_rows")
    torch.cuda.synchronize()
    ref = src.view(B, rows_in, 1160)[:, r_off:r_off + rows_out, :1152].reshape(B * rows_out, 1152)
    assert torch.equal(bits(out[:-1, 1024:2176]), bits(ref))
    assert untouched(out[:, :1024]) and untouched(out[:, 2176:]) and untouched(out[-1:])


@pytest.mark.parametrize("rows,D,ldx,ldy", [(5, 272, 384, 280), (4100, 1088, 1088, 1096)], ids=["small", "grid-stride"])
def test_x_to_bf16(device, rows, D, ldx, ldy):
    """round to nearest even, written out on the integer bits; (4100, 1088): more 16-byte pieces than the capped grid has threads"""
    L, lib = _lib()
    g = R.gen(207, rows)
    x = torch.randn(rows, ldx, generator=g) * torch.exp2(torch.randint(-12, 12, (rows, ldx), generator=g).float())
    x[0, :4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0])   # ties
    y = sent_bf16((rows + 1, ldy), device)
    L.check(lib.emmax_op_x_to_bf16(x.to(device).data_ptr(), ldx, y.data_ptr(), ldy, rows, D, stream()), "x_to_bf16")
    torch.cuda.synchronize()
    assert torch.equal(bits(y[:rows, :D]), R.bf16_bits_rne(x[:, :D]))
    assert untouched(y[:rows, D:]) and untouched(y[rows:])


# =============================================================================================================================================
# row statistics and the LayerNorm fold
# =============================================================================================================================================
def _row_stats(device, x, rows, D, ldx):
    """x: [rows, D] on the device; runs the op on rows of pitch ldx; returns (mean, rstd) after the sentinel checks"""
    L, lib = _lib()
    buf = finite_bf16((rows, ldx), 3, device) if ldx > D else torch.empty(rows, ldx, dtype=torch.bfloat16, device=device)
    buf[:, :D] = x
    stats = sent_f32(((rows + 3) * 2,), device)
    rc = lib.emmax_op_row_stats(buf.data_ptr(), ldx, stats.data_ptr(), rows, D, EPS, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.emmax_last_error()
    assert untouched(stats[rows * 2:]), "statistics past the last row were written"
    st = stats[: rows * 2].view(rows, 2)
    return st[:, 0], st[:, 1]


def _assert_stats(mean, rstd, x, D, what):
    em, er = R.stats_err(mean, rstd, x, EPS)
    bm, br = R.sum_bound(R.STATS[D][0]), R.sum_bound(R.STATS[D][1])
    print(f"row_stats {what}: mean error {em:.3g} of the row rms (bound {bm:.3g}), rstd relative error {er:.3g} (bound {br:.3g})")
    assert torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    assert em <= bm and er <= br, (what, em, bm, er, br)


@pytest.mark.parametrize("D", R.STATS_DS)
def test_row_stats_every_instantiation(device, D):
    """one D per template form (<1, 4> <2, 4> <4, 2> <8, 1> <16, 1>) and the towers' own; rows 1, 5, 261 of pitch D + 8 whose padding holds
    other values: against float64 at the emulation's bound"""
    for rows in (1, 5, 261):
        x = R.stats_rows(261, D)[:rows].to(device)
        mean, rstd = _row_stats(device, x, rows, D, D + 8)
        _assert_stats(mean, rstd, x, D, f"D {D} rows {rows}")


@pytest.mark.parametrize("rows,D", [(32768 + 7, 8), (16384 + 3, 1152)])
def test_row_stats_grid_stride_loop(device, rows, D):
    """more rows than the capped grid takes in one pass (2048 blocks x 4 waves x R rows: 32768 at <1, 4>, 16384 at <4, 2>, the 256-frame
    operating point): the rows of the second pass, the ragged last group included"""
    x = R.stats_rows(rows, D, seed=1).to(device)
    mean, rstd = _row_stats(device, x, rows, D, D + 8)
    _assert_stats(mean, rstd, x, D, f"D {D} rows {rows}")
    _assert_stats(mean[-16:], rstd[-16:], x[-16:], D, f"D {D}, the last 16 rows")


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("with_beta", [True, False], ids=["beta", "nobeta"])
@pytest.mark.parametrize("N,K,ldw", [(384, 128, 128), (432, 144, 256), (8, 1152, 1152)])
def test_ln_fold(device, N, K, ldw, with_beta, with_bias):
    """W' = bf16(W gamma) bit for bit, in place, the weight's padding columns and the row behind untouched; ln_s and ln_c against float64"""
    L, lib = _lib()
    W, gamma, beta, bias = R.fold_case(N, K, 0)
    beta, bias = (beta if with_beta else None), (bias if with_bias else None)
    Wd = sent_bf16((N + 1, ldw), device)
    Wd[:N, :K] = R.bf(W).to(device)
    dv = [None if t is None else R.bf(t).to(device) for t in (gamma, beta, bias)]
    sums = sent_f32((2, N + 2), device)
    L.check(lib.emmax_op_ln_fold(Wd.data_ptr(), ldw, N, K, dv[0].data_ptr(), L.ptr(dv[1]), L.ptr(dv[2]), sums[0].data_ptr(), sums[1].data_ptr(), stream()), "ln_fold")
    torch.cuda.synchronize()
    assert torch.equal(bits(Wd[:N, :K]), R.fold_bits(W, gamma)), "W' = bf16(W gamma)"
    assert untouched(Wd[:N, K:]) and untouched(Wd[N:]) and untouched(sums[:, N:])
    es, ec = R.fold_err(sums[0, :N].cpu(), sums[1, :N].cpu(), W, gamma, beta, bias)
    bs, bc = R.sum_bound(R.FOLD[(N, K)][0]), R.sum_bound(R.FOLD[(N, K)][1])
    print(f"ln_fold ({N}, {K}) beta={with_beta} bias={with_bias}: ln_s error {es:.3g} (bound {bs:.3g}), ln_c error {ec:.3g} (bound {bc:.3g}) of the terms' magnitudes")
    assert es <= bs and ec <= bc


# =============================================================================================================================================
# what the ops refuse: nothing is launched, nothing is written
# =============================================================================================================================================
def test_pure_ops_refuse_what_their_kernels_cannot_do(device):
    L, lib = _lib()
    out = sent_bf16((4096,), device)
    outf = sent_f32((4096,), device)
    src = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    o, of, s, st = out.data_ptr(), outf.data_ptr(), src.data_ptr(), stream()
    m, sd = f3((0.5, 0.5, 0.5)), f3((0.5, 0.5, 0.5))
    bad = {
        "gather: img % patch": lambda: lib.emmax_op_patch_gather(s, o, 1, 30, 14, 640, 0, m, sd, 1, 0, st),
        "gather: kpad < 3 patch^2": lambda: lib.emmax_op_patch_gather(s, o, 1, 28, 14, 584, 0, m, sd, 1, 0, st),
        "gather: HL kpad % 64": lambda: lib.emmax_op_patch_gather(s, o, 1, 28, 14, 600, 0, m, sd, 1, 1, st),
        "gather: chan0 = 1": lambda: lib.emmax_op_patch_gather(s, o, 1, 28, 14, 640, 1, m, sd, 0, 0, st),
        "gather: chan0 = 6": lambda: lib.emmax_op_patch_gather(s, o, 1, 28, 14, 640, 6, m, sd, 0, 0, st),
        "gather: null src": lambda: lib.emmax_op_patch_gather(None, o, 1, 28, 14, 640, 0, m, sd, 1, 0, st),
        "gather: null mean": lambda: lib.emmax_op_patch_gather(s, o, 1, 28, 14, 640, 0, None, sd, 1, 0, st),
        "assemble: ld < D": lambda: lib.emmax_op_assemble_tokens(s, s, s, s, o, 1, 4, 1, 4, 144, 128, 0, st),
        "assemble: null cls": lambda: lib.emmax_op_assemble_tokens(s, s, None, s, o, 1, 4, 1, 4, 128, 128, 0, st),
        "assemble: null reg": lambda: lib.emmax_op_assemble_tokens(s, s, s, None, o, 1, 4, 1, 4, 128, 128, 0, st),
        "assemble: null tokens": lambda: lib.emmax_op_assemble_tokens(s, s, s, s, None, 1, 4, 1, 4, 128, 128, 0, st),
        "copy_rows: r_off + rows_out > rows_in": lambda: lib.emmax_op_copy_rows(s, 128, o, 1, 8, 5, 4, 128, 128, 0, st),
        "copy_rows: ld_in % 8": lambda: lib.emmax_op_copy_rows(s, 132, o, 1, 8, 0, 4, 128, 128, 0, st),
        "copy_rows: col_off % 8": lambda: lib.emmax_op_copy_rows(s, 128, o, 1, 8, 0, 4, 128, 384, 4, st),
        "copy_rows: D % 8": lambda: lib.emmax_op_copy_rows(s, 128, o, 1, 8, 0, 4, 124, 128, 0, st),
        "copy_rows: col_off + D > ld_out": lambda: lib.emmax_op_copy_rows(s, 128, o, 1, 8, 0, 4, 128, 128, 8, st),
        "copy_rows: null": lambda: lib.emmax_op_copy_rows(None, 128, o, 1, 8, 0, 4, 128, 128, 0, st),
        "row_stats: D > 8192": lambda: lib.emmax_op_row_stats(s, 8200, of, 1, 8200, EPS, st),
        "row_stats: D % 8": lambda: lib.emmax_op_row_stats(s, 128, of, 1, 124, EPS, st),
        "row_stats: ldx < D": lambda: lib.emmax_op_row_stats(s, 120, of, 1, 128, EPS, st),
        "row_stats: ldx % 8": lambda: lib.emmax_op_row_stats(s, 132, of, 1, 128, EPS, st),
        "row_stats: null": lambda: lib.emmax_op_row_stats(s, 128, None, 1, 128, EPS, st),
        "ln_fold: ldw < K": lambda: lib.emmax_op_ln_fold(o, 120, 4, 128, s, s, s, of, of + 64, st),
        "ln_fold: null gamma": lambda: lib.emmax_op_ln_fold(o, 128, 4, 128, None, s, s, of, of + 64, st),
        "ln_fold: null ln_c": lambda: lib.emmax_op_ln_fold(o, 128, 4, 128, s, s, s, of, None, st),
        "x_to_bf16: ldy < D": lambda: lib.emmax_op_x_to_bf16(s, 128, o, 120, 1, 128, st),
        "x_to_bf16: ldx % 8": lambda: lib.emmax_op_x_to_bf16(s, 132, o, 128, 1, 128, st),
        "x_to_bf16: null": lambda: lib.emmax_op_x_to_bf16(None, 128, o, 128, 1, 128, st),
    }
    for what, call in bad.items():
        assert call() != 0, f"{what}: accepted"
        assert lib.emmax_last_error(), what
    torch.cuda.synchronize()
    assert untouched(out) and untouched(outf), "a refused call wrote"


# =============================================================================================================================================
# the stages of the encode
# =============================================================================================================================================
@pytest.fixture(scope="module")
def world():
    cfg = R.cfg_tiny()
    sd = R.state_dict(cfg)
    return cfg, sd, R.chain(sd, cfg, R.frames())


def _engine(device, cfg, sd, lnfuse):
    from emmax.modeling import EmmaXForActionPrediction

    L, _ = _lib()
    with L.tuning(gemm_lnfuse=lnfuse):   # read when the model is finalized
        model = EmmaXForActionPrediction(cfg, {k: v.to(torch.bfloat16) for k, v in sd.items()}).to(device, max_batch=R.B_MAX, max_prompt=32)
    return model


@pytest.fixture(scope="module")
def models(device, world):
    """the tiny model finalized with the LayerNorms folded into qkv / fc1 (gemm_lnfuse = 1, the default) and with separate LayerNorms (0)"""
    cfg, sd, _ = world
    return {"fold": _engine(device, cfg, sd, 1), "ln": _engine(device, cfg, sd, 0)}


_REFS = {}


def _case(world, case, B):
    """(x, tok, float64 reference) of a bounded case, computed once"""
    cfg, sd, act = world
    key = (case[:3], B)
    if key not in _REFS:
        _REFS[key] = R.case_io(case, sd, cfg, act, B)
    return _REFS[key]


def _stage(model, device, tower, block, stage, B, x, tok, rows, width):
    """one call of emmax_op_vision_stage: the packed output rows [rows, width] after the sentinel check on the row behind them"""
    L, lib = _lib()
    out = sent_bf16((rows + 1, width), device)
    as_rows = lambda v: (v.to(torch.bfloat16) if v.is_floating_point() else v).to(device).contiguous()   # (the references hold bf16 values as fp32)
    xd = as_rows(x)
    td = None if tok is None else as_rows(tok)
    rc = lib.emmax_op_vision_stage(model.engine._session, -1 if tower is None else tower, block, stage, B, xd.data_ptr(), L.ptr(td), out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.emmax_last_error()
    assert untouched(out[rows:]), "a row past the last was written"
    return out[:rows]


def _assert_stage(got, ref, entry, what, act=False):
    w = R.worst(got.float().cpu(), ref, entry, act)
    print(f"{what}: worst |err| / allowed = {w:.3g} (PRE {entry:.3g}; max|err| {(got.double().cpu() - ref).abs().max().item():.3g}, rms(ref) {R.rms(ref):.3g})")
    assert torch.isfinite(got.float()).all(), what
    assert w <= 1.0, f"{what}: misses the bound by {w:.3g} x"


def _widths(tw):
    return {"qkv": 3 * tw.embed_dim, "attn": tw.embed_dim, "proj": tw.embed_dim, "fc1": tw.mlp_hidden, "fc2": tw.embed_dim}


VS = {"embed": 0, "qkv": 1, "attn": 2, "proj": 3, "fc1": 4, "fc2": 5, "features": 6, "pj1": 7, "pj2": 8, "pj3": 9, "embed_pixels": 10}


@pytest.mark.parametrize("form", ["fold", "ln"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("last", [False, True], ids=["block0", "last_block"])
@pytest.mark.parametrize("t", [0, 1], ids=["dino", "siglip"])
def test_block_stages(device, world, models, t, last, B, form):
    """qkv, proj, fc1, fc2 of block 0 and the last block of both tiny towers (261 and 256 rows per frame), each on the bf16 rounding of the
    reference chain's own activations, against its float64 reference at its table bound"""
    cfg = world[0]
    tw = cfg.towers[t]
    i = R.n_blocks(tw) - 1 if last else 0
    rows = B * tw.n_tokens
    for stage in ("qkv", "proj", "fc1", "fc2"):
        case = (stage, t, i, form if stage in ("qkv", "fc1") else "")
        x, tok, ref = _case(world, case, B)
        got = _stage(models[form], device, t, i, VS[stage], B, x, tok, rows, _widths(tw)[stage])
        _assert_stage(got, ref, R.PRE[case], f"{stage} tower {t} block {i} B {B} {form}", act=stage == "fc1")


@pytest.mark.parametrize("stage", ["qkv", "fc1"])
@pytest.mark.parametrize("t", [0, 1], ids=["dino", "siglip"])
def test_ln_stages_on_massive_rows_and_both_forms_against_each_other(device, world, models, t, stage):
    """rows with a large common offset and massive channels (the mean term must cancel exactly): both forms against float64, and against each
    other at the sum of their bounds -- on those rows and on the chain's"""
    cfg = world[0]
    tw = cfg.towers[t]
    for name, B in ((stage + "_massive", 1), (stage, 3)):
        got = {}
        for form in ("fold", "ln"):
            case = (name, t, 0, form)
            x, _, ref = _case(world, case, B)
            got[form] = _stage(models[form], device, t, 0, VS[stage], 1 if name.endswith("massive") else B, x, None, x.shape[0], _widths(tw)[stage])
            _assert_stage(got[form], ref, R.PRE[case], f"{name} tower {t} {form}", act=stage == "fc1")
        both = R.allowed(ref, R.PRE[(name, t, 0, "fold")], stage == "fc1") + R.allowed(ref, R.PRE[(name, t, 0, "ln")], stage == "fc1")
        assert ((got["fold"].double().cpu() - got["ln"].double().cpu()).abs() <= both).all(), f"{name} tower {t}: the two forms differ by more than the sum of their bounds"


@pytest.mark.parametrize("resident", [-1, 2], ids=["planned", "resident"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("t", [0, 1], ids=["dino", "siglip"])
def test_attention_stage(device, world, models, tune, t, B, resident):
    """the attention stage on the chain's qkv rows, on the planned kernel and on the resident one: the reference and the tolerance
    test_attention (tests/test_ops_gpu.py) holds that kernel to"""
    from test_ops_gpu import ATTN_ATOL, TOL, _attn_ref, assert_elementwise, relerr

    tune(attn_resident=resident)
    cfg = world[0]
    tw = cfg.towers[t]
    D, N = tw.embed_dim, tw.n_tokens
    x, _, ref64 = _case(world, ("attn", t, 0, ""), B)
    got = _stage(models["fold"], device, t, 0, VS["attn"], B, x, None, B * N, D)
    ref = _attn_ref(R.bf(x), [b * N for b in range(B + 1)], tw.num_heads, tw.num_heads, tw.head_dim, 0, D, 2 * D, tw.head_dim ** -0.5, 0)
    assert relerr(ref, ref64) < 1e-5        # test_attention's fp32 reference is this module's float64 one
    assert torch.isfinite(got.float()).all()
    assert relerr(got, ref) < TOL
    assert_elementwise(got, ref, atol_frac=ATTN_ATOL, what=f"attention stage tower {t} B {B}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("t", [0, 1], ids=["dino", "siglip"])
def test_embed_stage(device, world, models, t, B):
    """gather + patch GEMM + assemble from uint8 frames against PatchEmbed and _pos_embed in float64; the cls and register rows bit for bit and
    in order; the pixel form on bf16(preprocess(frames)) bit-identical to the uint8 form"""
    from oracle import emmax_oracle as orc

    cfg, sd, _ = world
    tw = cfg.towers[t]
    fr, _, ref = _case(world, ("embed", t, 0, ""), B)
    got = _stage(models["fold"], device, t, 0, VS["embed"], B, fr, None, B * tw.n_tokens, tw.embed_dim)
    _assert_stage(got, ref, R.PRE[("embed", t, 0, "")], f"embed tower {t} B {B}")
    if tw.n_prefix:
        p = R.TOWER_PREFIXES[t]
        pre = torch.cat([sd[p + "cls_token"], sd[p + "reg_token"]], 1).view(tw.n_prefix, tw.embed_dim)
        for b in range(B):
            assert torch.equal(bits(got.view(B, tw.n_tokens, -1)[b, : tw.n_prefix]), R.bits16(R.bf(pre))), "cls, then the registers in order"
    pix = orc.preprocess_frames(fr.numpy(), cfg).to(torch.bfloat16)
    got_px = _stage(models["fold"], device, t, 0, VS["embed_pixels"], B, pix, None, B * tw.n_tokens, tw.embed_dim)
    assert torch.equal(bits(got_px), bits(got)), "the pixel form differs from the uint8 form"


@pytest.mark.parametrize("B", [1, 3])
def test_features_stage_places_each_tower_in_its_columns(device, world, models, B):
    """tower 0's patch rows to columns 0 .. 127, tower 1's to 128 .. 271 of the feature rows, prefix rows dropped; the other tower's columns
    keep what they held, bit for bit"""
    cfg = world[0]
    V, n_p = cfg.vision_dim, cfg.n_patches
    feats = finite_bf16((B * n_p, V), 5, device)
    for t, tw in enumerate(cfg.towers):
        tok = finite_bf16((B * tw.n_tokens, tw.embed_dim), 6 + t, device)
        got = _stage(models["fold"], device, t, 0, VS["features"], B, tok, feats, B * n_p, V)
        ref = R.ref_features(tok.cpu(), feats.cpu(), t, cfg)
        assert torch.equal(bits(got), bits(ref)), f"tower {t}"
        feats = got.clone()


@pytest.mark.parametrize("B", [1, 3])
def test_projector_stages(device, world, models, B):
    cfg = world[0]
    _, p1, h, _ = cfg.projector_dims
    for stage, width in (("pj1", p1), ("pj2", h), ("pj3", h)):
        x, _, ref = _case(world, (stage, None, 0, ""), B)
        got = _stage(models["fold"], device, None, 0, VS[stage], B, x, None, B * cfg.n_patches, width)
        _assert_stage(got, ref, R.PRE[(stage, None, 0, "")], f"{stage} B {B}", act=stage != "pj3")


def test_stage_op_refusals(device, world, models):
    L, lib = _lib()
    cfg, sd, _ = world
    s = models["fold"].engine._session
    x = torch.zeros(R.B_MAX * 261 * 1088, dtype=torch.bfloat16, device=device)
    out = sent_bf16((R.B_MAX * 261 * 1088,), device)
    for what, args in {"tower 2": (2, 0, 1, 1), "block 3": (0, 3, 1, 1), "block -1": (1, -1, 4, 1), "stage 11": (0, 0, 11, 1), "stage -1": (0, 0, -1, 1), "B 0": (0, 0, 1, 0),
                       "B max_batch + 1": (0, 0, 1, R.B_MAX + 1)}.items():
        assert lib.emmax_op_vision_stage(s, *args, x.data_ptr(), x.data_ptr(), out.data_ptr(), stream()) != 0, what
    assert lib.emmax_op_vision_stage(s, 0, 0, 3, 1, x.data_ptr(), None, out.data_ptr(), stream()) != 0, "proj without the token rows"
    assert lib.emmax_op_vision_stage(s, 0, 0, 1, 1, None, None, out.data_ptr(), stream()) != 0, "null input"
    assert lib.emmax_op_vision_stage(None, 0, 0, 1, 1, x.data_ptr(), None, out.data_ptr(), stream()) != 0, "null session"
    torch.cuda.synchronize()
    assert untouched(out)


def test_exact_session_is_refused(device, world):
    from emmax.modeling import EmmaXForActionPrediction

    L, lib = _lib()
    cfg, sd, _ = world
    xm = EmmaXForActionPrediction(cfg, {k: v.to(torch.bfloat16) for k, v in sd.items()}).to(device, max_batch=1, max_prompt=32, exact=True)
    x = torch.zeros(261 * 128, dtype=torch.bfloat16, device=device)
    out = sent_bf16((261 * 384,), device)
    assert lib.emmax_op_vision_stage(xm.engine._session, 0, 0, 1, 1, x.data_ptr(), None, out.data_ptr(), stream()) != 0
    torch.cuda.synchronize()
    assert untouched(out)


def test_tower1_on_scratch_tower0_used_equals_a_fresh_session(device, world, models):
    """Scratch set 0 serves both towers at each tower's own pitch: after tower 0 (rows of 128) the tiny SigLIP (D 144 in rows of 256) finds tower
    0's values in its padding columns -- the bf16 assemble writes the real columns only.  Its embed and qkv must equal, bit for bit, those of a
    session that never ran tower 0, and meet the reference: the padded weight columns are zero and the leftovers finite."""
    cfg, sd, act = world
    B = R.B_MAX
    used, fresh = models["fold"], _engine(device, cfg, sd, 1)
    tw0, tw1 = cfg.towers
    fr = R.frames(B)
    tok = _stage(used, device, 0, 0, VS["embed"], B, fr, None, B * tw0.n_tokens, tw0.embed_dim)
    for i in range(R.n_blocks(tw0)):   # tower 0's stages in order over the shared scratch: every buffer ends up holding tower 0's rows
        qkv = _stage(used, device, 0, i, VS["qkv"], B, tok, None, B * tw0.n_tokens, 3 * tw0.embed_dim)
        att = _stage(used, device, 0, i, VS["attn"], B, qkv, None, B * tw0.n_tokens, tw0.embed_dim)
        tok = _stage(used, device, 0, i, VS["proj"], B, att, tok, B * tw0.n_tokens, tw0.embed_dim)
        mlp = _stage(used, device, 0, i, VS["fc1"], B, tok, None, B * tw0.n_tokens, tw0.mlp_hidden)
        tok = _stage(used, device, 0, i, VS["fc2"], B, mlp, tok, B * tw0.n_tokens, tw0.embed_dim)
    out = {}
    for name, m in (("used", used), ("fresh", fresh)):
        e = _stage(m, device, 1, 0, VS["embed"], B, fr, None, B * tw1.n_tokens, tw1.embed_dim)
        out[name] = (e, _stage(m, device, 1, 0, VS["qkv"], B, e, None, B * tw1.n_tokens, 3 * tw1.embed_dim))
    assert torch.equal(bits(out["used"][0]), bits(out["fresh"][0])), "embed differs after tower 0 used the scratch"
    assert torch.equal(bits(out["used"][1]), bits(out["fresh"][1])), "qkv differs after tower 0 used the scratch"
    _assert_stage(out["used"][0], _case(world, ("embed", 1, 0, ""), B)[2], R.PRE[("embed", 1, 0, "")], "embed tower 1 on used scratch")
    e = out["used"][0].float().cpu()
    _assert_stage(out["used"][1], R.ref_qkv(e, sd, 1, 0, tw1), R.PRE[("qkv", 1, 0, "fold")], "qkv tower 1 on used scratch")


def test_stage_chain_is_the_encode(device, world, models):
    """the stage op called stage after stage over both towers and the projector reproduces emmax_vision_encode + emmax_vision_features bit for
    bit (B = 2, one stream): the op runs the encode's own code"""
    L, _ = _lib()
    cfg = world[0]
    B = 2
    m = models["fold"]
    fr = R.frames(B).to(device)
    with L.tuning(vis_streams=0):
        proj = m.engine.vision_encode(fr).clone()
        feats_ref = m.engine.vision_features(B).clone()
    torch.cuda.synchronize()
    feats = torch.zeros(B * cfg.n_patches, cfg.vision_dim, dtype=torch.bfloat16, device=device)
    for t, tw in enumerate(cfg.towers):
        rows = B * tw.n_tokens
        tok = _stage(m, device, t, 0, VS["embed"], B, fr, None, rows, tw.embed_dim)
        for i in range(R.n_blocks(tw)):
            qkv = _stage(m, device, t, i, VS["qkv"], B, tok, None, rows, 3 * tw.embed_dim)
            att = _stage(m, device, t, i, VS["attn"], B, qkv, None, rows, tw.embed_dim)
            tok = _stage(m, device, t, i, VS["proj"], B, att, tok, rows, tw.embed_dim)
            mlp = _stage(m, device, t, i, VS["fc1"], B, tok, None, rows, tw.mlp_hidden)
            tok = _stage(m, device, t, i, VS["fc2"], B, mlp, tok, rows, tw.embed_dim)
        feats = _stage(m, device, t, 0, VS["features"], B, tok, feats, B * cfg.n_patches, cfg.vision_dim).clone()
    assert torch.equal(bits(feats), bits(feats_ref.view(B * cfg.n_patches, -1))), "the features differ from the encode's"
    _, p1, h, _ = cfg.projector_dims
    x = feats
    for stage, width in (("pj1", p1), ("pj2", h), ("pj3", h)):
        x = _stage(m, device, None, 0, VS[stage], B, x, None, B * cfg.n_patches, width)
    assert torch.equal(bits(x), bits(proj.view(B * cfg.n_patches, -1))), "the patch embeddings differ from the encode's"
