"""CPU: the float64 references, bounds and judges of the frame-side kernel tests (frame_ref.py) hold what they should and nothing more.
  * float32 numpy emulations of preprocess_kernel, preprocess_aa_kernel, upsample_depth_kernel and stereo_warp_generic, and an integer
    emulation of the gather kernel's blend, pass EVERY judge on the cases of test_gpu_frame_ops.py (its warp tests are run here with
    the device call replaced by the emulation, so the case builders and their path-class assertions are checked too);
  * each of fourteen deliberate errors is rejected on a stated case;
  * d2s_warp_plan (host code) is held to a table with one case either side of every threshold of plan_warp;
  * d2s_preprocess returns the bicubic over-scale error without launching;
  * the float64 warp reference agrees with oracle/d2s_oracle.py::make_sbs_core within that oracle's float32 coordinate noise."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_ref as R
import test_gpu_frame_ops as G
from desktop2stereo_amd import _lib, ops

M3 = (G.MEAN2, G.STD2)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ emulations pass every judge
def test_preprocess_and_upsample_emulations_pass():
    rng = np.random.default_rng(1)
    worst = 0.0
    for (B, H, W, h, w, stride, square, ms) in G.PRE_CASES:
        px = R.noise_u8(rng, B, H, W).astype(np.float64)
        s = 1 if square else stride
        ref, delta = R.preprocess_bilinear(px, s, h, w, *M3)
        em = R.preprocess_bilinear(px, s, h, w, *M3, dt=np.float32)
        ok, r = R.judge_float(em, ref, delta)
        assert ok.all(), (H, W, h, w, stride, r)
        worst = max(worst, r)
    assert 0.05 < worst <= 1.0                                     # the bound is of the size of the float32 noise, not orders above it
    for (B, H, W, p, gh, gw, Kp, stride, D, _) in G.PATCH_CASES:
        px = R.noise_u8(rng, B, H, W).astype(np.float64)
        ref, delta = R.preprocess_bilinear(px, stride, gh * p, gw * p, *M3)
        em = R.preprocess_bilinear(px, stride, gh * p, gw * p, *M3, dt=np.float32)
        refA, dA, emA = R.patch_rows(ref, p, Kp), R.patch_rows(delta, p, Kp), R.patch_rows(em.astype(np.float64), p, Kp)
        live = ~np.isnan(refA)
        assert live.sum() == refA.shape[0] * 3 * p * p
        assert R.judge_float(emA[live], refA[live], dA[live])[0].all()
        assert R.judge_bf16(R.rne_bf16(emA[live]), refA[live], dA[live])[0].all()
    for (B, H, W, h, w) in G.AA_CASES:
        px = R.noise_u8(rng, B, H, W).astype(np.float64)
        ref, delta = R.preprocess_aa(px, h, w, *M3)
        ok, r = R.judge_float(R.preprocess_aa(px, h, w, *M3, dt=np.float32), ref, delta)
        assert ok.all(), (H, W, h, w, r)
    for (B, h, w, H, W, big) in G.UP_CASES:
        d = (rng.random((B, h, w)) + (1e4 if big else 0.0)).astype(np.float32)
        ref, delta = R.upsample(d, H, W)
        ok, r = R.judge_float(R.upsample(d, H, W, dt=np.float32), ref, delta)
        assert ok.all(), (h, w, H, W, r)
    assert R.aa_taps_needed(210, 14) == 62 and R.aa_taps_needed(224, 14) == 66 and R.aa_taps_needed(154, 14) == 46


def _emulated_run_warp(dev, px, in_fmt, depth, out_fmt, mode, *, fill=False, ipd_uv=0.064, ratio=2.0, conv=0.0, wpc=None, expect=None,
                       misalign=0, expect_rpw=None):
    """test_gpu_frame_ops.run_warp with the device call replaced by the emulations (the plan is the library's: host code)"""
    B, H, W, _ = px.shape
    dh, dw = depth.shape[1:]
    sp = ops.sbs_params(ipd_uv, ratio, conv, mode, fill)
    with G.env(D2S_WARP_WPC=None if wpc is None else str(wpc)):
        plan = ops.warp_plan(G.FMT[in_fmt], dh, dw, B, H, W, sp, G.FMT[out_fmt], rgb_align=1 if misalign else 256)
    want = expect or G.expect_warp(in_fmt, out_fmt, mode, fill, B, H, W, dh, dw, aligned=not misalign)
    assert plan["kernel"] == want, (plan, want)
    if plan["gather"]:
        assert 1 <= plan["rpw"] <= H and (mode != "Half-TAB" or plan["rpw"] % 2 == 0), plan
        assert expect_rpw is None or plan["rpw"] == expect_rpw, (plan, expect_rpw)
    kw = dict(ipd_uv=ipd_uv, ratio=ratio, conv=conv, mode=mode, fill=fill)
    ref = R.warp_ref(px.astype(np.float64), depth, kernel="gather" if plan["gather"] else "generic", **kw)
    u8 = out_fmt == "U8_HWC"
    for kind in (("fx", "f32") if plan["gather"] else ("f32",)):
        if kind == "fx" and np.abs(ref["shift"]).max() >= W - 1:    # (the fixed-point form reflects once: the kernel leaves such rows to the float path)
            continue
        got = R.warp_emulate(px.astype(np.float64), depth, kind=kind, u8=u8, **kw)
        ok, r = R.judge_range(got, ref["lo"], ref["hi"], ref["db"], u8)
        assert ok.all(), (want, kind, mode, px.shape, depth.shape, kw, G.where_bad(ok), r)
        assert r <= 1.0
    return ref, plan


@pytest.mark.parametrize("mode", list(R.MODES))
def test_warp_emulations_pass_on_the_gpu_cases(lib, mode, monkeypatch):
    monkeypatch.setattr(G, "run_warp", _emulated_run_warp)
    G.test_warp_generic_every_instantiation(None, mode)
    G.test_warp_generic_shapes_and_shifts(None, mode)
    G.test_warp_gather_shapes(None, mode)
    if mode in ("Full-SBS", "Half-TAB"):
        G.test_warp_gather_column_rule_thresholds(None, mode)
    G.test_warp_gather_bands(None, mode)
    G.test_warp_gather_in_kernel_paths(None, mode)
    G.test_warp_gather_path_changes_inside_a_band(None, mode)


# ------------------------------------------------------------------------------------------------ deliberate errors are rejected
def _warp_rejects(mut, kind, px, depth, **kw):
    ref = R.warp_ref(px.astype(np.float64), depth, kernel="gather" if kind == "fx" else "generic", **kw)
    good = R.warp_emulate(px.astype(np.float64), depth, kind=kind, **kw)
    bad = R.warp_emulate(px.astype(np.float64), depth, kind=kind, mut=mut, **kw)
    assert R.judge_range(good, ref["lo"], ref["hi"], ref["db"], True)[0].all(), mut
    return not R.judge_range(bad, ref["lo"], ref["hi"], ref["db"], True)[0].all()


def test_deliberate_warp_errors_are_rejected():
    rng = np.random.default_rng(2)
    nam = R.naming_u8(2, 6, 260)
    dep = (R.depth_frames(2, 3, 64) + R.depth_smooth(2, 3, 64, 0.3)).astype(np.float32)
    kw = dict(ratio=6.0, conv=0.45, mode="Full-SBS")
    # tap x0 + 1 taken from x0 at a 32-pixel chunk boundary (the pad slot): the naming image's R ramp, fractional shifts
    assert _warp_rejects("pad_slot", "fx", nam, dep, **kw)
    # the window of row r + 1 used for row r: G = 29 y
    assert _warp_rejects("row_next_window", "fx", nam, dep, **kw)
    assert _warp_rejects("eye_swap", "fx", nam, dep, **kw) and _warp_rejects("eye_swap", "f32", nam, dep, **kw)
    # reflection about W instead of W - 1: shifts past the right edge (ratio 30 on a 36-pixel frame)
    small = R.naming_u8(2, 6, 36)
    sdep = (R.depth_frames(2, 6, 36) + R.depth_smooth(2, 6, 36, 0.3)).astype(np.float32)
    assert _warp_rejects("reflect_W", "f32", small, sdep, ratio=30.0, conv=0.45, mode="Full-SBS")
    assert _warp_rejects("reflect_W", "fx", small, sdep, ratio=30.0, conv=0.45, mode="Full-TAB")
    # depth row tap + 1 / depth of frame b + 1: per-frame constants plus a ramp down the rows, depth at a third of the frame
    rdep = R.depth_frames(2, 3, 64, ramp=0.4)
    assert _warp_rejects("depth_row_plus1", "fx", nam, rdep, **kw) and _warp_rejects("depth_frame_plus1", "fx", nam, rdep, **kw)
    assert _warp_rejects("depth_frame_plus1", "f32", nam, rdep, **kw)
    # NC = 3 columns where 4 are needed: dw = 40 under W = 64 (3 dw >= W), rough depth
    n64 = R.naming_u8(1, 4, 64)
    assert _warp_rejects("nc3", "fx", n64, rng.random((1, 2, 40)).astype(np.float32), ratio=8.0, conv=0.5, mode="Full-SBS")
    # Half-SBS pair (2 x - 1, 2 x)
    assert _warp_rejects("hsbs_pair_shift", "fx", nam, dep, ratio=6.0, conv=0.45, mode="Half-SBS")
    assert _warp_rejects("hsbs_pair_shift", "f32", nam, dep, ratio=6.0, conv=0.45, mode="Half-SBS")
    # truncation instead of rounding of the byte: noise frames, fractional shifts
    noi = R.noise_u8(rng, 2, 6, 260)
    assert _warp_rejects("trunc_byte", "fx", noi, dep, **kw) and _warp_rejects("trunc_byte", "f32", noi, dep, **kw)
    assert _warp_rejects("trunc_byte", "fx", noi, dep, ratio=6.0, conv=0.45, mode="Half-TAB")


def test_deliberate_preprocess_errors_are_rejected():
    rng = np.random.default_rng(3)
    px = R.noise_u8(rng, 1, 31, 45).astype(np.float64)

    def rejected(fn, mut, *a):
        ref, delta = fn(px, *a, *M3)
        assert R.judge_float(fn(px, *a, *M3, dt=np.float32), ref, delta)[0].all()
        return not R.judge_float(fn(px, *a, *M3, dt=np.float32, mut=mut), ref, delta)[0].all()
    assert rejected(R.preprocess_bilinear, "align_corners", 1, 14, 28)                  # align_corners = True taps
    assert rejected(R.preprocess_bilinear, "decim_floor", 2, 14, 28)                    # (31, 45) stride 2: Hs = 16, not 15
    assert rejected(R.preprocess_bilinear, "mean_wrong_channel", 1, 14, 28)             # non-default mean / std, distinct per channel
    assert rejected(R.preprocess_aa, "cubic_unnormalised", 14, 28)                      # scale 2.2 / 1.6: raw weights sum to the scale
    d = rng.random((1, 4, 5)).astype(np.float32)
    ref, delta = R.upsample(d, 15, 17)
    assert not R.judge_float(R.upsample(d, 15, 17, dt=np.float32, mut="align_corners"), ref, delta)[0].all()
    ref, delta = R.preprocess_bilinear(px, 1, 4, 6, *M3)                                 # p = 2, grid 2 x 3: i and j swapped in the column map
    good, bad = R.patch_rows(ref, 2, 16), R.patch_rows(ref, 2, 16, mut="patch_ij_swap")
    live = ~np.isnan(good)
    assert not R.judge_float(bad[live], good[live], R.patch_rows(delta, 2, 16)[live])[0].all()


# ------------------------------------------------------------------------------------------------ d2s_warp_plan
def plan(lib, in_fmt="U8_HWC", out_fmt="U8_HWC", mode="Full-SBS", fill=False, B=1, H=8, W=64, dh=None, dw=None, ra=256, oa=256):
    dh, dw = H if dh is None else dh, W if dw is None else dw
    return ops.warp_plan(G.FMT[in_fmt], dh, dw, B, H, W, ops.sbs_params(display_mode=mode, fill_16_9=fill), G.FMT[out_fmt], ra, oa)


def test_warp_plan_table(lib):
    GEN, GA = "stereo_warp_generic<U8_HWC,U8_HWC>", "stereo_warp_gather<FULL_SBS,NC=%d,DIRECT=%d>"
    table = [
        (dict(W=64), GA % (4, 1)), (dict(W=62), GEN), (dict(W=66), GEN),                                    # W % 4
        (dict(W=4), GEN), (dict(W=8), GA % (4, 1)), (dict(W=16380), GA % (4, 1)), (dict(W=16384), GEN),       # W in [8, 16384)
        (dict(W=124, dw=40, dh=4), GA % (3, 0)), (dict(W=120, dw=40, dh=4), GA % (4, 0)),                     # 3 dw < W
        (dict(W=64, dw=40, dh=4), GA % (4, 0)), (dict(W=60, dw=40, dh=4), GEN),                               # 3 dw < 2 W
        (dict(W=12, dw=3, dh=4), GA % (3, 0)), (dict(W=12, dw=2, dh=4), GEN),                                 # dw >= nc
        (dict(W=8, dw=4, dh=4), GA % (4, 0)), (dict(W=8, dw=3, dh=4), GEN),
        (dict(W=64, dh=9, dw=20), GEN), (dict(W=64, dh=8, dw=20), GA % (3, 0)),                               # dh <= H
        (dict(mode="Half-TAB", H=7), GEN), (dict(mode="Half-TAB", H=8), "stereo_warp_gather<HALF_TAB,NC=4,DIRECT=1>"),
        (dict(mode="Half-SBS", H=7), "stereo_warp_gather<HALF_SBS,NC=4,DIRECT=1>"),
        (dict(mode="Full-TAB", H=7, W=64), "stereo_warp_gather<FULL_TAB,NC=4,DIRECT=1>"),
        (dict(fill=True, H=9, W=16), GA % (4, 1)), (dict(fill=True, H=8, W=16), GEN), (dict(fill=True, H=36, W=16), GEN),   # padding (16:9 itself: none)
        (dict(in_fmt="U8_CHW"), "stereo_warp_generic<U8_CHW,U8_HWC>"), (dict(in_fmt="F32_CHW"), "stereo_warp_generic<F32_CHW,U8_HWC>"),
        (dict(out_fmt="F32_HWC"), "stereo_warp_generic<U8_HWC,F32_HWC>"), (dict(out_fmt="F32_CHW"), "stereo_warp_generic<U8_HWC,F32_CHW>"),
        (dict(in_fmt="F32_CHW", out_fmt="F32_CHW"), "stereo_warp_generic<F32_CHW,F32_CHW>"),
        (dict(ra=2), GEN), (dict(oa=1), GEN), (dict(ra=4, oa=4), GA % (4, 1)),                                # misaligned pointers
        (dict(H=1, W=8), GA % (4, 1)), (dict(H=3, W=12), GA % (4, 1)),                                        # H W 3 % 4 (always 0 when W % 4 == 0)
        (dict(B=1073, H=1000, W=1000), GA % (4, 1)), (dict(B=1074, H=1000, W=1000), GEN),                     # batch dh dw 4 < 2^32 depth bytes
    ]
    for kw, want in table:
        assert plan(lib, **kw)["kernel"] == want, (kw, want)
    # the 12 288 row-tile switch of wpc: rows ntx <= 12288 -> 12 waves per CU, else 32
    p = plan(lib, B=6, H=1024, W=512); assert (p["wpc"], p["ntx"], p["rpw"]) == (12, 2, 4)                    # 12 288 tiles
    p = plan(lib, B=6, H=1024, W=516); assert (p["wpc"], p["ntx"], p["rpw"]) == (32, 3, 3)                    # 18 432 tiles
    p = plan(lib, B=1, H=1080, W=1920, dh=294, dw=518); assert (p["wpc"], p["ntx"], p["rpw"], p["waves"], p["grid"]) == (12, 8, 3, 2880, 720)
    p = plan(lib, B=32, H=1080, W=1920, dh=294, dw=518); assert (p["wpc"], p["rpw"], p["waves"]) == (32, 34, 1017 * 8)
    # rpw parity: Half-TAB rounds up to whole row pairs
    assert plan(lib, mode="Half-TAB", B=1, H=1080, W=1920, dh=294, dw=518)["rpw"] == 4
    assert plan(lib, mode="Half-TAB", B=32, H=1080, W=1920, dh=294, dw=518)["rpw"] == 34
    # a band is never longer than a frame (the kernel's tap table wraps into the next frame once)
    for kw in (dict(B=7000, H=1, W=8), dict(B=7000, H=2, W=8), dict(B=4000, H=2, W=8, mode="Half-TAB"), dict(B=6000, H=3, W=260, dh=1, dw=64)):
        p = plan(lib, **kw)
        assert p["gather"] and p["rpw"] == kw["H"] and p["waves"] == kw["B"] * p["ntx"], (kw, p)
    with G.env(D2S_WARP_WPC="1"):
        assert plan(lib, B=600, H=2, W=8)["rpw"] == 2 and plan(lib, B=2, H=8300, W=8)["rpw"] == 65
        assert plan(lib, B=2, H=8300, W=8, mode="Half-TAB")["rpw"] == 66
    with G.env(D2S_WARP_GATHER="0"):
        assert plan(lib)["kernel"] == GEN
    r = _lib.WarpPlanResult()                                                                               # a short struct is refused
    r.struct_size = 8
    sp = ops.sbs_params()
    assert lib.d2s_warp_plan(0, 8, 8, 1, 8, 8, C.byref(sp), 0, 256, 256, C.byref(r)) != 0 and lib.d2s_last_error()


def test_preprocess_aa_overscale_is_refused_without_a_launch(lib):
    """(224, 28) -> (14, 14): sy = 16 needs 66 taps > 64.  The check precedes every use of the pointers: non-null host addresses stand in
    for device buffers and are never dereferenced."""
    pre = ops.pre_params(resample="bicubic_aa")
    host = (C.c_uint8 * 16)()
    rc = lib.d2s_preprocess(C.cast(host, C.c_void_p), 0, 1, 224, 28, C.cast(host, C.c_void_p), 14, 14, 1, C.byref(pre), None)
    assert rc == 1 and b"15x" in lib.d2s_last_error()
    rc = lib.d2s_preprocess(C.cast(host, C.c_void_p), 0, 1, 28, 224, C.cast(host, C.c_void_p), 14, 14, 1, C.byref(pre), None)
    assert rc == 1


# ------------------------------------------------------------------------------------------------ the two references agree
def test_float64_warp_reference_agrees_with_the_oracle():
    """oracle/d2s_oracle.py::make_sbs_core follows the reference's float32 normalised-coordinate round trip; its coordinate noise is a
    few ulp of W in pixels (the oracle's own documentation: 2^-13 .. 2^-14 px at x ~ 1000), here 16 u (W + |shift|), times the largest
    step between neighbouring pixels."""
    from oracle import d2s_oracle as O
    rng = np.random.default_rng(4)
    for mode in R.MODES:
        for (H, W, dh, dw, fill, ratio) in ((9, 35, 9, 35, True, 8.0), (12, 40, 12, 40, False, 30.0), (7, 22, 7, 22, False, 2.0)):
            px = R.noise_u8(rng, 1, H, W)
            dep = R.depth_smooth(1, dh, dw)
            ref = R.warp_ref(px.astype(np.float64), dep, ratio=ratio, conv=0.3, mode=mode, fill=fill)
            got = O.make_sbs_core(px[0].transpose(2, 0, 1).astype(np.float32), dep[0], depth_ratio=ratio, display_mode=mode, fill_16_9=fill,
                                  convergence=0.3).transpose(1, 2, 0)
            noise = 16 * R.U * (W + np.abs(ref["shift"]).max()) * 255.0
            lo, hi = ref["lo"][0] - noise, ref["hi"][0] + noise
            assert ((got >= lo - ref["db"]) & (got <= hi + ref["db"])).all(), (mode, H, W)
