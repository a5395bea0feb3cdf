"""CPU: the judges of tests/test_gpu_temporal.py can fail, and do not fail a correct kernel.  For one small shape per kernel
(a) a faithful float32 emulation of the kernel's arithmetic (temporal_ref.*_compute in float32: two-pass statistics, a float32 softmax
    over the 32 positions) passes the judge on every input family -- the evidence that the derived bounds hold for a correct
    implementation -- and
(b) each deliberate error is rejected on the family built to show it."""
import pytest
import torch

import temporal_ref as R

DEV = torch.device("cpu")
EPS = 1e-6


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_ROWS, GN_SITES, GN_C, GN_GROUPS = 3, 37, 64, 32            # CPG 2: groupnorm_reg_kernel<.,2,1>
GN_DEPTH = R.norm_depth_groupnorm(True, 2, 1, GN_SITES)


def gn_case(fam, bf16, sites=GN_SITES, seed=1):
    g = gen(seed)
    cpg = GN_C // GN_GROUPS
    x = R.norm_family(fam, (GN_ROWS, GN_GROUPS, sites, cpg), bf16, g, DEV).permute(0, 2, 1, 3).reshape(GN_ROWS, sites, GN_C).contiguous()
    gamma = 1.0 + 0.5 * torch.randn(GN_C, generator=g)
    beta = torch.randn(GN_C, generator=g)
    xs = x.to(torch.bfloat16) if bf16 else x
    ref, mu, var = R.groupnorm_compute(xs, gamma, beta, EPS, GN_GROUPS, torch.float64)
    delta = R.groupnorm_delta(xs, gamma, EPS, GN_GROUPS, R.norm_depth_groupnorm(True, cpg, 1, sites), ref, mu, var)
    return xs, gamma, beta, ref, delta


def gn_judge(xs, gamma, beta, ref, delta, bf16, mut=""):
    fmt = "bf16" if bf16 else "f32"
    y = R.groupnorm_compute(xs, gamma, beta, EPS, GN_GROUPS, torch.float32, mut)[0]
    ok, ratio, _ = R.judge(R.store(y, fmt), ref, delta, fmt)
    return bool(ok.all()), ratio


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fam,sites", [("G1", GN_SITES), ("G2", GN_SITES), ("G3", GN_SITES), ("G3", 1), ("G4", GN_SITES)])
def test_groupnorm_emulation_passes(fam, sites, bf16):
    c = gn_case(fam, bf16, sites)
    ok, ratio = gn_judge(*c, bf16)
    assert ok and ratio < 1.0, (fam, sites, ratio)


@pytest.mark.parametrize("mut,fam,sites", [("unbiased", "G3", 1), ("unbiased", "G3", GN_SITES), ("rows", "G1", GN_SITES),
                                           ("onepass", "G2", GN_SITES), ("eps", "G3", GN_SITES)])
def test_groupnorm_mutant_is_rejected(mut, fam, sites):
    c = gn_case(fam, False, sites)
    assert gn_judge(*c, False)[0]
    ok, ratio = gn_judge(*c, False, mut)
    assert not ok and ratio > 1.0, (mut, fam, ratio)


def test_constant_group_is_beta():
    xs, gamma, beta, ref, delta = gn_case("G4", False)
    assert torch.equal(ref, beta.double().expand_as(ref))
    # the bound there: the mean's error (depth + 1) u |x|, |x| <= 40, times rstd = 1000, times |gamma|; plus the last rounding
    cap = (GN_DEPTH + 1) * R.U * 40.0 * 1000.0 * float(gamma.abs().max()) + R.U * float(beta.abs().max())
    assert float(delta.max()) <= cap * (1 + 1e-6)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_ROWS, LN_D = 5, 252


def ln_case(fam, eps, seed=2):
    g = gen(seed)
    x = R.norm_family(fam, (LN_ROWS, 1, LN_D), False, g, DEV).view(LN_ROWS, LN_D)
    gamma = 1.0 + 0.5 * torch.randn(LN_D, generator=g)
    beta = torch.randn(LN_D, generator=g)
    ref, mu, var = R.layernorm_compute(x, gamma, beta, eps, torch.float64)
    return x, gamma, beta, ref, R.layernorm_delta(x, gamma, eps, ref, mu, var)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("fam", ["G1", "G2", "G3", "G4"])
@pytest.mark.parametrize("fmt", ["f32", "bf16", "e4m3"])
def test_layernorm_emulation_passes(fam, eps, fmt):
    x, gamma, beta, ref, delta = ln_case(fam, eps)
    qs = 1.0
    if fmt == "e4m3":                                             # ~1 % of the elements saturate
        srt = ref.abs().flatten().sort().values
        qs = R.f32(448.0 / float(srt[int(0.99 * (srt.numel() - 1))]))
        delta = delta + R.U * ref.abs()
    y = R.layernorm_compute(x, gamma, beta, eps, torch.float32)[0]
    raw = R.store(y, fmt, qs)
    ok, ratio, got = R.judge(raw, ref, delta, fmt, qs)
    assert bool(ok.all()) and ratio < 1.0, (fam, eps, fmt, ratio)
    if fmt == "e4m3":
        assert bool((got.abs()[(ref.abs() - delta) * qs > 448.0] == 448.0).all())


def test_layernorm_bx3_emulation_passes():
    g = gen(3)
    x = R.norm_family("G1", (4, 1, 256), False, g, DEV).view(4, 256)
    gamma, beta = 1.0 + 0.5 * torch.randn(256, generator=g), torch.randn(256, generator=g)
    ref, mu, var = R.layernorm_compute(x, gamma, beta, 1e-6, torch.float64)
    y = R.layernorm_compute(x, gamma, beta, 1e-6, torch.float32)[0]
    ok, ratio, got = R.judge(R.store(y, "bx3"), ref, R.layernorm_delta(x, gamma, 1e-6, ref, mu, var), "bx3")
    assert bool(ok.all()) and ratio < 1.0 and float((got - y.double()).abs().max()) <= 2.0 ** -16 * float(y.abs().max())


@pytest.mark.parametrize("mut,fam", [("unbiased", "G3"), ("onepass", "G2"), ("eps", "G3")])
def test_layernorm_mutant_is_rejected(mut, fam):
    x, gamma, beta, ref, delta = ln_case(fam, 1e-6)
    y = R.layernorm_compute(x, gamma, beta, 1e-6, torch.float32, mut)[0]
    ok, ratio, _ = R.judge(y, ref, delta, "f32")
    assert not bool(ok.all()) and ratio > 1.0, (mut, ratio)


# ------------------------------------------------------------------------------------------------ temporal attention
TA_C, TA_S = 96, 5                                             # head dim 12: CH 4, 4 lanes per unit, one of them padding
TA_HEAD, TA_TW = [29, 0, 15], [32, 1, 32]


def ta_case(fam, bf16, case_idx=0, seed=4):
    store = [h if fam == "T4" else (-1 if r == 0 else h) for r, h in enumerate(TA_HEAD)]
    cur, rings, ptab, pi = R.tattn_family(fam, TA_C, TA_S, TA_HEAD, TA_TW, case_idx, bf16, gen(seed + case_idx), DEV)
    ref, rings_ref, b = R.tattn_compute(cur, rings, ptab, TA_HEAD, TA_TW, store, torch.float64, bounds=True)
    return cur, rings, ptab, store, pi, ref, b


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fam", ["T1", "T2", "T3", "T4"])
def test_temporal_attn_emulation_passes(fam, bf16):
    for case_idx in range(4):
        cur, rings, ptab, store, pi, ref, b = ta_case(fam, bf16, case_idx)
        assert bool(torch.isfinite(ref).all())                  # (the fresh row's NaN ring is never read)
        if pi is not None:
            assert R.tattn_target_weight(b, pi, TA_TW) >= 0.99
        out, rings_after = R.tattn_compute(cur, rings, ptab, TA_HEAD, TA_TW, store, torch.float32)
        fmt = "bf16" if bf16 else "f32"
        ok, ratio, _ = R.judge(R.store(out, fmt), ref, R.tattn_delta(TA_C, b), fmt)
        assert bool(ok.all()) and ratio < 1.0, (fam, case_idx, ratio)
        # a fresh row's output is its own value row plus the table's row 0
        C = TA_C
        fresh = cur[1, :, C:2 * C].double() + ptab[0, C:2 * C].double()
        assert float((ref[1] - fresh).abs().max()) <= 1e-12 * float(fresh.abs().max())
        for r in range(3):
            if store[r] >= 0:
                assert torch.equal(rings_after[r][store[r]].view(torch.int16 if bf16 else torch.int32),
                                   cur[r, :, :2 * C].contiguous().view(torch.int16 if bf16 else torch.int32))


def test_peaked_families_cover_every_window_position():
    seen2, seen3 = set(), set()
    for case_idx in range(4):
        seen2 |= set(ta_case("T2", False, case_idx)[4].flatten().tolist())
        seen3 |= set(ta_case("T3", False, case_idx)[4].flatten().tolist())
    assert seen2 == set(range(32)) and seen3 == set(range(32))


@pytest.mark.parametrize("mut,fam", [("slot", "T2"), ("ptab", "T3"), ("store_first", "T4"), ("mask_last", "T2")])
def test_temporal_attn_mutant_is_rejected(mut, fam):
    cur, rings, ptab, store, pi, ref, b = ta_case(fam, False)
    out = R.tattn_compute(cur, rings, ptab, TA_HEAD, TA_TW, store, torch.float32, mut)[0]
    delta = R.tattn_delta(TA_C, b)
    ok, ratio, _ = R.judge(out, ref, delta, "f32")
    assert not bool(ok.all()) and ratio > 1000.0, (mut, ratio)
    assert float((out.double() - ref).abs().max()) > 1.0         # a wrong key moves an output by about 4


# ------------------------------------------------------------------------------------------------ GEGLU
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_geglu_emulation_passes(bf16):
    u = R.geglu_family(7, 37, bf16, gen(5), DEV)
    ref = R.geglu_compute(u, torch.float64)
    assert bool(torch.isfinite(ref).all())
    fmt = "bf16" if bf16 else "f32"
    ok, ratio, _ = R.judge(R.store(R.geglu_compute(u, torch.float32), fmt), ref, R.geglu_delta(u, ref), fmt)
    assert bool(ok.all()) and ratio < 1.0, ratio


@pytest.mark.parametrize("mut", ["swap", "tanh"])
def test_geglu_mutant_is_rejected(mut):
    u = R.geglu_family(7, 37, False, gen(5), DEV)
    ref = R.geglu_compute(u, torch.float64)
    ok, ratio, _ = R.judge(R.geglu_compute(u, torch.float32, mut), ref, R.geglu_delta(u, ref), "f32")
    assert not bool(ok.all()) and ratio > 1.0, (mut, ratio)


def test_e4m3_store_round_trips():
    from f64_ref import e4m3_value, rne_e4m3
    v = torch.cat([torch.linspace(-500, 500, 4001), torch.linspace(-0.05, 0.05, 2001)])
    assert torch.equal(e4m3_value(R.store(v, "e4m3")), rne_e4m3(v.float().double()))
