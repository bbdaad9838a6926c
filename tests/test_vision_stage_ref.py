"""tests/vision_stage_ref.py on the CPU: the bound tables are what the emulations measure, the float64 references are the model's operations
(composed, they reproduce oracle.emmax_oracle), the fp32 gather is within half a bf16 ulp of float64 on every byte, and the module's state
dict discriminates -- every mis-wiring tests/test_vision_stages_gpu.py lists moves a reference by at least 10 x the stage's bound."""

import pytest
import torch

import vision_stage_ref as R


@pytest.fixture(scope="module")
def world():
    cfg = R.cfg_tiny()
    sd = R.state_dict(cfg)
    return cfg, sd, R.chain(sd, cfg, R.frames())


def _pinned(measured, entry, what):
    print(f"{what}: measured {measured:.4g}, entry {entry:.4g}")
    assert measured <= 1.05 * entry and measured >= entry * 2.0 / 3.0, f"{what}: measured {measured:.4g} against the entry {entry:.4g}"


def test_stage_table_is_the_emulations_measurement(world):
    cfg, sd, act = world
    cases = R.stage_cases(cfg)
    assert set(cases) == set(R.PRE), "one entry per case"
    for c in cases:
        _pinned(R.measure_case(c, sd, cfg, act), R.PRE[c], f"PRE{c}")


def test_statistics_and_fold_tables_are_the_emulations_measurement():
    assert set(R.STATS) == set(R.STATS_DS) and set(R.FOLD) == set(R.FOLD_SHAPES)
    for D in R.STATS_DS:
        for k, what in enumerate(("mean", "rstd")):
            _pinned(R.measure_stats(D)[k], R.STATS[D][k], f"STATS[{D}] {what}")
    for s in R.FOLD_SHAPES:
        for k, what in enumerate(("ln_s", "ln_c")):
            _pinned(R.measure_fold(*s)[k], R.FOLD[s][k], f"FOLD[{s}] {what}")


def test_references_composed_are_the_oracle(world):
    """the float64 stage references over all blocks and the projector against oracle.vision_backbone and oracle.projector in fp32, same weights and
    frames: to fp32 accuracy"""
    from oracle import emmax_oracle as orc

    cfg, sd, act = world
    fr = R.frames()
    pix = orc.preprocess_frames(fr.numpy(), cfg)
    feats = orc.vision_backbone(pix, sd, cfg)
    proj = orc.projector(feats, sd)
    B = fr.shape[0]
    for got, ref, what in ((act["feats"].view(B, cfg.n_patches, -1), feats, "features"), (act["pj3"].view(B, cfg.n_patches, -1), proj, "projector")):
        err = ((got - ref.double()).abs().max() / ref.double().abs().max()).item()
        print(f"{what}: max|err| / max|ref| = {err:.3g}")
        assert err < 1e-5, (what, err)
    # the stage inputs look like token streams: O(1) and finite, nothing saturated
    for k, v in act.items():
        assert torch.isfinite(v).all() and 1e-2 < R.rms(v) < 1e2, (k, R.rms(v))


@pytest.mark.parametrize("norm", ["tower0", "tower1", "odd"])
def test_fp32_gather_is_within_half_a_bf16_ulp_of_float64(norm):
    """all 256 byte values x 3 channels: bf16 of the three fp32 operations against (u / 255 - mean) / std in float64.  The fp32 value carries three
    roundings (2^-22 relative to the largest intermediate), so half an ulp of bf16 holds up to that -- a factor 1 + 2^-12 on the half ulp."""
    cfg = R.cfg_tiny()
    mean, std = {"tower0": (cfg.towers[0].mean, cfg.towers[0].std), "tower1": (cfg.towers[1].mean, cfg.towers[1].std), "odd": (R.ODD_MEAN, R.ODD_STD)}[norm]
    u = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    ref = R.ref_normalize(u, mean, std)
    got = R.bf16_bits_rne(R.emu_normalize(u, mean, std)).view(torch.bfloat16).double()
    half_ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 8)
    assert ((got - ref).abs() <= half_ulp * (1 + 2.0 ** -12) + 2.0 ** -24).all()


def test_bf16_rounding_on_the_integer_bits_is_torchs():
    x = torch.randn(4096, generator=R.gen(3)) * torch.exp2(torch.randint(-20, 20, (4096,), generator=R.gen(4)).float())
    x[:4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0])   # ties: to even
    assert torch.equal(R.bf16_bits_rne(x), R.bits16(x.to(torch.bfloat16)))
    hi, lo = R.hl_split(x)
    assert ((hi.view(torch.bfloat16).double() + lo.view(torch.bfloat16).double() - x.double()).abs() <= x.double().abs() * 2.0 ** -16).all()


# ---- the state dict discriminates ---------------------------------------------------------------------------------------------------------------
def _moved(broken, ref, entry, act=False):
    return ((broken.double() - ref.double()).abs() / R.allowed(ref, entry, act)).max().item()


def _swapped(sd, a, b):
    out = dict(sd)
    out[a], out[b] = sd[b], sd[a]
    return out


def test_miswirings_move_the_references_by_ten_bounds(world):
    cfg, sd, act = world
    moved = {}
    p0 = R.TOWER_PREFIXES[0] + "blocks.0."
    # ls1 <-> ls2 (tower 0 has the LayerScales)
    bad = _swapped(sd, p0 + "ls1.scale_factor", p0 + "ls2.scale_factor")
    for stage in ("proj", "fc2"):
        x, tok, ref = R.case_io((stage, 0, 0, ""), sd, cfg, act)
        moved[f"ls swap / {stage}"] = _moved(R.ref_stage(stage, bad, cfg, 0, 0, x, tok), ref, R.PRE[(stage, 0, 0, "")])
    # proj_b <-> fc2_b, both towers
    for t in (0, 1):
        p = f"{R.TOWER_PREFIXES[t]}blocks.0."
        bad = _swapped(sd, p + "attn.proj.bias", p + "mlp.fc2.bias")
        for stage in ("proj", "fc2"):
            x, tok, ref = R.case_io((stage, t, 0, ""), sd, cfg, act)
            moved[f"bias swap / {stage} tower {t}"] = _moved(R.ref_stage(stage, bad, cfg, t, 0, x, tok), ref, R.PRE[(stage, t, 0, "")])
    # patch_b dropped; the registers in reverse order
    for t in (0, 1):
        x, _, ref = R.case_io(("embed", t, 0, ""), sd, cfg, act)
        tw = cfg.towers[t]
        bad = dict(sd)
        bad[R.TOWER_PREFIXES[t] + "patch_embed.proj.bias"] = torch.zeros(tw.embed_dim)
        moved[f"patch_b dropped / embed tower {t}"] = _moved(R.ref_embed(R.ref_normalize(x, tw.mean, tw.std), bad, t, tw), ref, R.PRE[("embed", t, 0, "")])
    x, _, ref = R.case_io(("embed", 0, 0, ""), sd, cfg, act)
    tw = cfg.towers[0]
    bad = dict(sd)
    bad[R.TOWER_PREFIXES[0] + "reg_token"] = sd[R.TOWER_PREFIXES[0] + "reg_token"].flip(1)
    moved["registers reversed / embed"] = _moved(R.ref_embed(R.ref_normalize(x, tw.mean, tw.std), bad, 0, tw), ref, R.PRE[("embed", 0, 0, "")])
    # norm1 <-> norm2 parameters
    for t in (0, 1):
        p = f"{R.TOWER_PREFIXES[t]}blocks.0."
        bad = _swapped(_swapped(sd, p + "norm1.weight", p + "norm2.weight"), p + "norm1.bias", p + "norm2.bias")
        x, tok, ref = R.case_io(("qkv", t, 0, "fold"), sd, cfg, act)
        moved[f"norm1 <-> norm2 / qkv tower {t}"] = _moved(R.ref_stage("qkv", bad, cfg, t, 0, x), ref, max(R.PRE[("qkv", t, 0, "fold")], R.PRE[("qkv", t, 0, "ln")]))
    # ln_c without the bias; the variance about zero -- against the fp32 sums' bounds, in their own units
    for N, K in R.FOLD_SHAPES:
        W, gamma, beta, bias = R.fold_case(N, K, 0)
        s, c = R.ref_fold_sums(W, gamma, beta, None)
        moved[f"ln_c without bias / fold {N} x {K}"] = R.fold_err(s, c, W, gamma, beta, bias)[1] / R.sum_bound(R.FOLD[(N, K)][1])
    for D in R.STATS_DS:
        x = R.stats_rows(261, D)
        mean, _ = R.ref_row_stats(x, 1e-6)
        about_zero = torch.rsqrt(x.double().pow(2).mean(-1) + 1e-6)
        moved[f"variance about zero / row_stats {D}"] = R.stats_err(mean, about_zero, x, 1e-6)[1] / R.sum_bound(R.STATS[D][1])
    for k, v in moved.items():
        print(f"{k}: {v:.3g} x the bound")
    assert all(v >= 10.0 for v in moved.values()), {k: v for k, v in moved.items() if v < 10.0}


def test_exact_ops_see_their_miswirings():
    """the gather, the feature copy: compared bit for bit, so a mis-wiring only has to change bits -- here it changes most of them"""
    g = R.gen(11)
    u = torch.randint(0, 256, (2, 28, 28, 3), generator=g, dtype=torch.uint8)
    good = R.gather_u8_bits(u, 14, 640, R.ODD_MEAN, R.ODD_STD)
    swapped = R.gather_u8_bits(u, 14, 640, R.ODD_MEAN, (R.ODD_STD[0], R.ODD_STD[2], R.ODD_STD[1]))
    assert (good[:, :588] != swapped[:, :588]).float().mean() > 0.6          # two of three channels, all but a few bytes
    assert torch.equal(good[:, :196], swapped[:, :196]) and (good[:, 588:] == 0).all()
    px = R.bfr(torch.randn(2, 6, 28, 28, generator=g))
    assert (R.patches_of(px[:, 0:3], 14) != R.patches_of(px[:, 3:6], 14)).float().mean() > 0.99   # chan0 ignored
    cfg = R.cfg_tiny()
    tok = torch.randn(cfg.towers[1].n_tokens, cfg.towers[1].embed_dim, generator=g)
    zero = torch.zeros(cfg.n_patches, cfg.vision_dim)
    at_128 = R.ref_features(tok, zero, 1, cfg)
    assert (at_128[:, :128] == 0).all() and (at_128[:, 128:] != 0).all()      # col_off 0 would land in tower 0's columns
