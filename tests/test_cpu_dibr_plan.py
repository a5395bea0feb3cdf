"""CPU: d2s_dibr_warp_plan (host code, no GPU) -- the function the f1 launcher takes its decision from -- is held to a restatement of
the window rule of DESIGN.md 3.4 ("The DIBR launch plan") over a sweep of shapes and parameters, to the LDS bound of a block (no row
kernel plan above 65 536 bytes: f1's rows_words is 1 983, formed from the kernel's own static arrays), to one case either side of
every threshold, and to what the comments in dibr.hip say of the three D2S_DIBR_* switches.
"""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

from desktop2stereo_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KEYS = ("D2S_DIBR_NO_ROLL0", "D2S_DIBR_NO_ROWS", "D2S_DIBR_COLS")
LDS_LIMIT = 65536
ROWS_WORDS = (LDS_LIMIT - (2 * 256 * 4 + 4)) // 32          # the largest WW with 32 WW + 2 052 <= 65 536
CROPS = [None, (0.0, 0.0, 1.0, 1.0), (0.1, 0.125, 0.8, 0.75), (0.25, 0.0, 0.5, 1.0)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@pytest.fixture()
def env(lib, monkeypatch):
    from desktop2stereo_amd import ops

    def set_env(**kw):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            monkeypatch.setenv(k, str(v))
        ops.reload_env()
    set_env()
    yield set_env
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    ops.reload_env()


def _eye(H, W, mode, crop):
    """(oh, ow, tex_per_col) as the launcher forms them: crop.pixel_bounds (Python's round = half to even) and the Half modes"""
    eh, ew, cw = H, W, 1.0
    if crop is not None:
        x0 = min(max(round(crop[0] * W), 0), W - 1)
        y0 = min(max(round(crop[1] * H), 0), H - 1)
        x1 = max(x0 + 1, min(round((crop[0] + crop[2]) * W), W))
        y1 = max(y0 + 1, min(round((crop[1] + crop[3]) * H), H))
        eh, ew, cw = y1 - y0, x1 - x0, float(F32(crop[2]))
    oh = eh // 2 if mode == "Half-TAB" else eh
    ow = ew // 2 if mode == "Half-SBS" else ew
    return oh, ow, W / ow * cw


def _rule(H, W, mode, crop, *, ipd_uv, depth_ratio, convergence, search_radius, resolution, roll=0.0, up=False, cols_env=512, no_rows=False,
          no_roll0=False):
    """DESIGN.md 3.4 restated: margin, the halving of cols, WW and the choice of the row kernel"""
    oh, ow, tpc = _eye(H, W, mode, crop)
    psx = float(F32(1) / (F32(resolution[0]) if resolution[0] > 0 else F32(W)))
    half_ipd, strength, conv = float(F32(ipd_uv / 2.0)), float(F32(0.1 * depth_ratio)), float(F32(convergence))
    reach = max(max(2.0, float(int(search_radius))) * (W * psx), abs(half_ipd) * (1.0 + abs(conv)) * abs(strength) * W)
    margin = int(math.ceil(reach)) + 2
    ww = lambda c: int(math.ceil((c - 1) * tpc)) + 2 * margin + 4
    roll0 = float(F32(math.sin(F32(roll)))) == 0.0 and float(F32(math.cos(F32(roll)))) == 1.0 and not no_roll0
    wide = cols_env >= 1024 and not up and crop is None
    cols, widen = (1024, 1536) if wide else ((512 if cols_env >= 512 else 256), 640)
    while cols > 256 and (ww(cols) > widen or ow <= cols // 2):
        cols //= 2
    rows = roll0 and not no_rows and ww(256) <= ROWS_WORDS
    return dict(rows=rows, cols=cols, margin=margin, WW=ww(cols), roll0=roll0, oh=oh, ow=ow)


def _plan(H, W, mode="Full-SBS", crop=None, out_u8=True, dhw=None, batch=1, **kw):
    from desktop2stereo_amd import ops
    dh, dw = dhw or (H, W)
    return ops.dibr_warp_plan(dh, dw, batch, H, W, ops.dibr_params(display_mode=mode, **kw), out_u8=out_u8, crop=crop)


def test_no_row_plan_exceeds_the_lds_of_a_block(lib, env):
    """The sweep: every plan agrees with the restated rule, and no plan with `rows` asks for more than 65 536 bytes of LDS."""
    n = n_rows = 0
    worst = 0
    for cols_env in (512, 256, 1024):
        env(**({} if cols_env == 512 else {"D2S_DIBR_COLS": cols_env}))
        for W, ipd, dr, conv, sr, mode, crop in itertools.product(
                (2, 64, 256, 257, 530, 1030, 1920, 2400, 3840, 7680), (0.064, 0.2, 0.5, 1.0), (1.0, 5.0, 20.0, 60.0), (0.0, -1.0),
                (0.0, 5.0, 15.0), ("Full-SBS", "Half-SBS", "Full-TAB", "Half-TAB"), CROPS):
            H = 8
            if crop is not None and W < 16:
                continue
            for res in ((0.0, 0.0), (W / 3.0, 5.0), (2.0 * W, 16.0)):
                kw = dict(ipd_uv=ipd, depth_ratio=dr, convergence=conv, search_radius=sr, resolution=res)
                pl = _plan(H, W, mode, crop, **kw)
                want = _rule(H, W, mode, crop, cols_env=cols_env, **kw)
                got = {k: pl[k] for k in want}
                assert got == want, (W, mode, crop, kw, cols_env, pl)
                n += 1
                if pl["rows"]:
                    n_rows += 1
                    worst = max(worst, pl["lds_bytes"])
                    assert pl["lds_dynamic"] == 32 * pl["WW"] and pl["lds_static"] == 8 * pl["cols"] + 4, pl
                    assert pl["lds_bytes"] <= LDS_LIMIT and pl["WW"] <= ROWS_WORDS, pl
                    assert pl["kernel"].startswith(f"dibr_rows<u8,fx=0,{pl['cols']},FullDep") and pl["block"] == 256, pl
                    assert pl["grid"] == (-(-pl["ow"] // pl["cols"]), pl["oh"], 1), pl
                else:
                    assert pl["lds_bytes"] == 0 and pl["kernel"].startswith("dibr<u8,roll0,FullDep"), pl
                    assert pl["grid"] == (-(-pl["ow"] // 256), 2 * pl["oh"], 1), pl
                assert pl["kernel"].endswith(",crop>") == (crop is not None), pl
    print(f"[dibr plan sweep] {n} plans, {n_rows} with rows, largest LDS request {worst} bytes")
    assert n_rows > n // 4 and n - n_rows > n // 20           # the sweep lies on both sides
    assert worst > 60000                                       # ... and comes near the bound (its exact edge: test_rows_words_is_the_lds_bound)


def test_rows_words_is_the_lds_bound(lib, env):
    """WW = 1 983 is the last window of the row kernel; 1 984 (the first whose 8 planes and the static queue exceed 64 KB) and above take
    the gather kernel.  Full-SBS windows are odd (259 + 2 margin), Half-SBS even (514 + 2 margin)."""
    assert ROWS_WORDS == 1983 and 32 * 1983 + 2052 <= LDS_LIMIT < 32 * 1984 + 2052
    for mode, dr, WW, rows in (("Half-SBS", 7.315, 1982, True), ("Full-SBS", 8.595, 1983, True), ("Half-SBS", 7.325, 1984, False),
                               ("Full-SBS", 8.605, 1985, False), ("Full-SBS", 8.915, 2047, False), ("Full-SBS", 8.925, 2049, False)):
        pl = _plan(6, 4000, mode, ipd_uv=0.5, depth_ratio=dr)
        assert (pl["WW"], pl["rows"], pl["cols"]) == (WW, rows, 256), (mode, dr, pl)
        if rows:
            assert pl["kernel"] == "dibr_rows<u8,fx=0,256,FullDep>" and pl["lds_bytes"] == 32 * WW + 2052 <= LDS_LIMIT
        else:
            assert pl["kernel"] == "dibr<u8,roll0,FullDep>" and pl["lds_bytes"] == 0
    # the same with a crop and with a depth map of the model's size
    pl = _plan(6, 4000, "Full-SBS", crop=(0.0, 0.0, 1.0, 1.0), dhw=(5, 19), out_u8=False, ipd_uv=0.5, depth_ratio=8.605)
    assert not pl["rows"] and pl["kernel"] == "dibr<f32,roll0,UpDep,crop>"
    pl = _plan(6, 4000, "Full-SBS", crop=(0.0, 0.0, 1.0, 1.0), dhw=(5, 19), out_u8=False, ipd_uv=0.5, depth_ratio=8.595)
    assert pl["rows"] and pl["kernel"] == "dibr_rows<f32,fx=0,256,UpDep,crop>" and pl["WW"] == 1983


def test_the_composites_bound_is_unchanged(lib):
    """The composites plan their window with 512 columns while it stays <= 640 words and take the row kernel while the 256-column window
    stays <= 1 536 words (48 KB of planes), stated through their own plan query one case either side of each number; f1's rows_words
    is the named constant, no literal."""
    from desktop2stereo_amd import ops
    f1 = open(os.path.join(REPO, "desktop2stereo_amd", "csrc", "dibr.hip")).read()
    calls = re.findall(r"dibr_plan_window\(([^;]*)\);", f1)
    assert len(calls) == 1 and calls[0].split(",")[-1].strip() == "DIBR_F1_ROWS_WORDS", calls      # no literal

    def plan(H, W, mode="Anaglyph", **kw):
        return ops.dibr_composite_plan(H, W, 1, H, W, ops.dibr_params(**kw), mode)
    for mode, tag in (("Anaglyph", "ana"), ("Interleaved", "il"), ("Interleaved-V", "ilv")):
        pl = plan(8, 1200, mode, viewport=(0, 0, 204, 8))                       # ceil(255 * 1200 / 204) + 2 * 15 + 4 = 1 534 <= 1 536
        assert (pl["rows"], pl["cols"], pl["margin"], pl["WW"], pl["kernel"]) == (True, 256, 15, 1534, f"comp_rows<{tag},u8,fx=0,256,FullDep>"), pl
        assert pl["lds_dynamic"] == 32 * 1534 and pl["lds_static"] == 4 * 256 + 4 and pl["lds_bytes"] <= LDS_LIMIT, pl
        pl = plan(8, 1200, mode, viewport=(0, 0, 200, 8))                       # 1 530 + 34 = 1 564 > 1 536: the gather kernel
        assert (pl["rows"], pl["WW"], pl["kernel"], pl["lds_bytes"]) == (False, 1564, f"comp<{tag},u8,roll0,FullDep>", 0), pl
        pl = plan(24, 512, mode, search_radius=15.0, resolution=(128.0, 6.0))   # 511 + 124 + 4 = 639 <= 640: 512 columns
        assert (pl["rows"], pl["cols"], pl["margin"], pl["WW"]) == (True, 512, 62, 639), pl
        assert pl["kernel"] == f"comp_rows<{tag},u8,fx=0,512,FullDep>" and pl["lds_static"] == 4 * 512 + 4, pl
        pl = plan(24, 512, mode, search_radius=15.0, resolution=(126.0, 6.0))   # 641 > 640: 256 columns, margin 63
        assert (pl["rows"], pl["cols"], pl["margin"], pl["WW"]) == (True, 256, 63, 255 + 126 + 4), pl
    # the largest row plan the composites can form stays inside a block's LDS
    assert 32 * 1536 + 4 * 256 + 4 <= LDS_LIMIT


def test_cols_follow_the_halving_rule(lib, env):
    """cols starts at 512 and halves to 256 when the 512-column window exceeds 640 words or when ow <= cols / 2."""
    table = [  # H, W, mode, kw -> cols, margin, WW.  margin = ceil(12 W psx) + 2: 14 where float32(1 / W) W <= 1, else 15
        (24, 512, "Full-SBS", {}, 512, 14, 511 + 28 + 4),
        (24, 530, "Full-SBS", {}, 512, 15, 511 + 30 + 4),                       # two blocks, the second ragged
        (24, 257, "Full-SBS", {}, 512, 14, 543),                                # ow = 257 > 512 / 2: one ragged block of 512
        (24, 256, "Full-SBS", {}, 256, 14, 255 + 28 + 4),                       # ow = 256 <= 512 / 2
        (24, 512, "Half-SBS", {}, 256, 14, 510 + 28 + 4),                       # ow = 256; two texels per column
        (24, 2048, "Half-SBS", {}, 256, 14, 510 + 28 + 4),                      # 1 022 + 32 > 640
        (24, 512, "Full-SBS", dict(search_radius=15.0, resolution=(128.0, 6.0)), 512, 62, 511 + 124 + 4),      # 639 <= 640
        (24, 512, "Full-SBS", dict(search_radius=15.0, resolution=(126.0, 6.0)), 256, 63, 255 + 126 + 4),      # 641 > 640
        (24, 512, "Full-TAB", {}, 512, 14, 543), (24, 512, "Half-TAB", {}, 512, 14, 543)]
    for H, W, mode, kw, cols, margin, WW in table:
        pl = _plan(H, W, mode, **kw)
        assert (pl["rows"], pl["cols"], pl["margin"], pl["WW"]) == (True, cols, margin, WW), (H, W, mode, kw, pl)
    env(D2S_DIBR_COLS=1024)                                                  # the wide form: 1 024 -> 512 -> 256 on 1 536 words and on ow
    for W, cols, margin in ((1024, 1024, 14), (1030, 1024, 15), (520, 1024, 15), (512, 512, 14), (256, 256, 14)):
        pl = _plan(24, W)
        assert (pl["rows"], pl["cols"], pl["margin"], pl["WW"]) == (True, cols, margin, cols - 1 + 2 * margin + 4), (W, pl)
    pl = _plan(24, 2048, "Half-SBS")                                         # 2 * 1 023 + 32 > 1 536 -> 512: 1 054 (640 bounds the narrow forms only)
    assert (pl["cols"], pl["WW"]) == (512, 1022 + 32), pl
    pl = _plan(24, 1024, search_radius=15.0, resolution=(61.0, 6.0))          # margin = ceil(15 * 1024 / 61) + 2 = 254: 1 535 <= 1 536
    assert (pl["cols"], pl["margin"], pl["WW"]) == (1024, 254, 1023 + 508 + 4), pl
    pl = _plan(24, 1024, search_radius=15.0, resolution=(59.0, 6.0))          # margin 263: 1 553 > 1 536 -> 512
    assert (pl["cols"], pl["margin"], pl["WW"]) == (512, 263, 511 + 526 + 4), pl


def test_the_three_switches(lib, env):
    """dibr.hip: D2S_DIBR_NO_ROLL0 = the general per-tap evaluation for roll == 0 too; D2S_DIBR_NO_ROWS = the gather kernel instead of the
    LDS-window kernel; D2S_DIBR_COLS = 256 | 512 | 1024 caps the columns per block (1 024: the uncropped FullDep kernels only)."""
    fx = dict(feather=True, corner_radius=0.03)
    assert _plan(24, 530)["kernel"] == "dibr_rows<u8,fx=0,512,FullDep>"
    assert _plan(24, 530, out_u8=False, **fx)["kernel"] == "dibr_rows<f32,fx=1,512,FullDep>"
    assert _plan(24, 530, corner_radius=0.03)["fx"] and _plan(24, 530, feather=True)["fx"] and not _plan(24, 530)["fx"]
    assert _plan(24, 530, dhw=(5, 19))["kernel"] == "dibr_rows<u8,fx=0,512,UpDep>"
    assert _plan(24, 530, dhw=(24, 19))["up"] and not _plan(24, 530)["up"]
    assert _plan(96, 128, crop=(0.1, 0.125, 0.8, 0.75), out_u8=False)["kernel"] == "dibr_rows<f32,fx=0,256,FullDep,crop>"
    assert _plan(24, 530, roll=0.3, out_u8=False)["kernel"] == "dibr<f32,general,FullDep>"
    pl = _plan(24, 530, roll=-1.2, dhw=(5, 19), crop=(0.0, 0.0, 1.0, 1.0))
    assert pl["kernel"] == "dibr<u8,general,UpDep,crop>" and not pl["roll0"] and pl["grid"] == (3, 48, 1)
    pl = _plan(24, 530, "Half-TAB", batch=2)
    assert pl["grid"] == (2, 12, 2) and (pl["oh"], pl["ow"], pl["out_h"], pl["out_w"]) == (12, 530, 24, 530)
    env(D2S_DIBR_NO_ROWS=1)
    pl = _plan(24, 530)
    assert pl["kernel"] == "dibr<u8,roll0,FullDep>" and not pl["rows"] and pl["roll0"] and pl["grid"] == (3, 48, 1) and pl["lds_bytes"] == 0
    env(D2S_DIBR_NO_ROLL0=1)
    pl = _plan(24, 530, dhw=(5, 19), out_u8=False)
    assert pl["kernel"] == "dibr<f32,general,UpDep>" and not pl["rows"] and not pl["roll0"]
    env(D2S_DIBR_COLS=256)
    assert _plan(24, 530)["kernel"] == "dibr_rows<u8,fx=0,256,FullDep>" and _plan(24, 530)["grid"] == (3, 24, 1)
    env(D2S_DIBR_COLS=1024)
    assert _plan(24, 1030)["kernel"] == "dibr_rows<u8,fx=0,1024,FullDep>" and _plan(24, 1030)["lds_static"] == 8196
    assert _plan(24, 1030, dhw=(5, 19))["kernel"] == "dibr_rows<u8,fx=0,512,UpDep>"                 # no wide form of UpDep
    assert _plan(24, 1030, crop=(0.0, 0.0, 1.0, 1.0))["kernel"] == "dibr_rows<u8,fx=0,512,FullDep,crop>"      # ... nor with a crop
    env(D2S_DIBR_COLS=1024, D2S_DIBR_NO_ROWS=1)
    assert _plan(24, 1030)["kernel"] == "dibr<u8,roll0,FullDep>"
    env()
    assert _plan(24, 530)["kernel"] == "dibr_rows<u8,fx=0,512,FullDep>"


def test_plan_refusals(lib, env):
    from desktop2stereo_amd import ops
    dp = ops.dibr_params()
    r = _lib.DibrWarpPlanResult()
    assert lib.d2s_dibr_warp_plan(24, 530, 1, 24, 530, C.byref(dp), None, 0, C.byref(r)) == 1 and b"struct_size" in lib.d2s_last_error()
    r.struct_size = C.sizeof(_lib.DibrWarpPlanResult)
    assert lib.d2s_dibr_warp_plan(24, 530, 1, 24, 530, C.byref(dp), None, 0, C.byref(r)) == 0
    assert lib.d2s_dibr_warp_plan(24, 530, 1, 24, 530, None, None, 0, C.byref(r)) == 1 and b"null pointer" in lib.d2s_last_error()
    assert lib.d2s_dibr_warp_plan(24, 530, 1, 24, 530, C.byref(dp), None, 0, None) == 1
    # what the launcher refuses of these arguments
    for args, msg in (((24, 530, 0, 24, 530), b"bad batch"), ((24, 530, 1, 1, 530), b"bad shape"), ((0, 530, 1, 24, 530), b"bad depth shape")):
        assert lib.d2s_dibr_warp_plan(*args, C.byref(dp), None, 0, C.byref(r)) == 1 and msg in lib.d2s_last_error(), args
    assert lib.d2s_dibr_warp_plan(24, 530, 1, 24, 530, C.byref(dp), None, 99, C.byref(r)) == 1 and b"out_fmt" in lib.d2s_last_error()
    for kw, msg in ((dict(search_radius=16.0), b"search_radius"), (dict(corner_radius=0.6), b"corner_radius"),
                    (dict(viewport=(0.0, 0.0, -1.0, 4.0)), b"viewport")):
        bad = ops.dibr_params(**kw)
        assert lib.d2s_dibr_warp_plan(24, 530, 1, 24, 530, C.byref(bad), None, 0, C.byref(r)) == 1 and msg in lib.d2s_last_error(), kw
    c4 = (C.c_double * 4)(0.5, 0.5, 0.6, 0.5)
    assert lib.d2s_dibr_warp_plan(24, 530, 1, 24, 530, C.byref(dp), c4, 0, C.byref(r)) == 1 and b"crop" in lib.d2s_last_error()
