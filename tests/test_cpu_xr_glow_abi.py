"""CPU: the C ABI and the host side of the colour mip chain and the glow around the flat OpenXR screen (include/d2s.h
d2s_version() >= 119: d2s_mip_shape, d2s_mip_chain, d2s_xr_glow, d2s_dibr_xr_eyes_glow, d2s_view_pipeline_xr_glow_streams;
desktop2stereo_amd/xr.py XrGlow, glow_range_m).  Symbols and the struct; every refusal the header lists, made with pointers that are
never dereferenced (a refused call launches nothing and makes no HIP call, so no device is needed); d2s_mip_shape's level lists and
offsets; xr.glow_range_m and the host uniforms against what the reference's own _glow_range_m / _render_glow produced on a stub
object (tests/golden/xr_glow.json, make_golden_xr_glow.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from desktop2stereo_amd import _lib, ops, xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned pointer that a refused call never touches
F32 = _lib.FMT_F32_HWC
NEW = ("d2s_mip_shape", "d2s_mip_chain", "d2s_dibr_xr_eyes_glow", "d2s_view_pipeline_xr_glow_streams")
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def manifest(golden_dir):
    with open(os.path.join(golden_dir, "xr_glow.json")) as f:
        return json.load(f)


def _vp(eye=0):
    fov = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))[eye]
    return xr.fov_to_proj_mat4(*fov) @ xr.pose_to_view_mat4((0, 0, 0, 1), (-0.032 if eye == 0 else 0.032, 0, 0))


def _call(lib, glow, levels=FAKE, screen=None, H=96, W=160, dp=None):
    dp = dp if dp is not None else ops.dibr_params()
    sc = screen if screen is not None else xr.XrScreen(width=1.6, height=0.96, distance=1.4).c_struct()
    ea = xr.eye_array([xr.xr_eye(_vp(i), 130, 100, i) for i in range(2)])
    return lib.d2s_dibr_xr_eyes_glow(FAKE, FAKE, 24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, 2, FAKE, F32, FAKE, 1 << 16,
                                     C.byref(glow) if glow is not None else None, levels, None)


def test_symbols_struct_and_version(lib):
    assert lib.d2s_version() >= 119
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in hdr, name
    assert "d2s_version() >= 119" in hdr and "sizeof(d2s_xr_glow) = 24" in hdr and "LINEAR_MIPMAP_LINEAR" in hdr
    assert C.sizeof(_lib.XrGlow) == 24 and _lib.XrGlow.mode.offset == 4 and _lib.XrGlow.range_m.offset == 8 and _lib.XrGlow.inner_edge_fraction.offset == 16
    a, b = _lib.SYMBOLS["d2s_dibr_xr_eyes"][1], _lib.SYMBOLS["d2s_dibr_xr_eyes_glow"][1]
    assert b[:len(a) - 1] == a[:-1] and b[-1] == a[-1] and len(b) == len(a) + 2          # ... as d2s_dibr_xr_eyes ..., glow, levels, stream
    a, b = _lib.SYMBOLS["d2s_view_pipeline_xr_streams"][1], _lib.SYMBOLS["d2s_view_pipeline_xr_glow_streams"][1]
    assert b[:len(a) - 1] == a[:-1] and b[-1] == a[-1] and len(b) == len(a) + 2
    g = xr.XrGlow("glow2", 3.5, 0.1).c_struct()
    assert (g.struct_size, g.mode, g.range_m, g.inner_edge_fraction) == (24, 2, 3.5, 0.1)
    with pytest.raises(ValueError):
        xr.XrGlow("halo").c_struct()


def test_every_glow_refusal_without_a_device(lib):
    err = lib.d2s_last_error
    G = lambda *a: xr.XrGlow(*a).c_struct()
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        assert _call(lib, G("glow", bad)) == INVALID and b"range_m" in err(), bad
    for bad in (-0.01, float("nan")):
        assert _call(lib, G("glow", 10.0, bad)) == INVALID and b"inner_edge_fraction" in err(), bad
    for mode in (-1, 3):
        g = G("glow", 10.0)
        g.mode = mode
        assert _call(lib, g) == INVALID and b"glow mode" in err()
    g = G("glow", 10.0)
    g.struct_size = 16
    assert _call(lib, g) == INVALID and b"d2s_xr_glow.struct_size" in err()
    for mode in ("glow", "glow2"):
        assert _call(lib, G(mode, 10.0), levels=None) == INVALID and b"levels" in err()
        for curve in ("horizontal", "vertical"):
            sc = xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve=curve).c_struct()
            assert _call(lib, G(mode, 10.0), screen=sc) == UNSUPPORTED and b"curved" in err(), (mode, curve)
        sc = xr.XrScreen(width=1.6, height=0.96, distance=1.4, normal_offset=0.01).c_struct()
        assert _call(lib, G(mode, 10.0), screen=sc) == INVALID and b"normal_offset" in err()
        assert _call(lib, G(mode, 10.0), H=96, W=8200) == INVALID
    # what d2s_dibr_xr_eyes refuses is refused first, whatever the glow says
    assert _call(lib, G("glow", 10.0), dp=ops.dibr_params(feather=True)) == INVALID and b"feather" in err()
    assert _call(lib, G("glow", 10.0), screen=xr.XrScreen(width=-1.0).c_struct()) == INVALID and b"> 0" in err()
    # the view pipeline checks its own arguments first (a null engine), with the same leading checks
    sc = xr.XrScreen().c_struct()
    ea = xr.eye_array([xr.xr_eye(_vp(0), 130, 100, 0)])
    dp, g, pp = ops.dibr_params(), G("glow", 10.0), _lib.PostParams()
    assert lib.d2s_view_pipeline_xr_glow_streams(None, FAKE, 1, None, 96, 160, 140, None, C.byref(pp), C.byref(dp), None, C.byref(sc), ea, 1, 0, FAKE,
                                                 F32, None, FAKE, 1 << 16, C.byref(g), FAKE, None) == INVALID and b"engine" in err()


def test_mip_shape_levels_offsets_and_refusals(lib):
    want = {
        (512, 1024): [(256, 512), (128, 256), (64, 128), (32, 64), (16, 32), (8, 16), (4, 8), (2, 4), (1, 2), (1, 1)],
        (562, 1000): [(281, 500), (140, 250), (70, 125), (35, 62), (17, 31), (8, 15), (4, 7), (2, 3), (1, 1)],
        (1080, 1920): [(540, 960), (270, 480), (135, 240), (67, 120), (33, 60), (16, 30), (8, 15), (4, 7), (2, 3), (1, 1)],
        (96, 160): [(48, 80), (24, 40), (12, 20), (6, 10), (3, 5), (1, 2), (1, 1)],
    }
    for (H, W), sizes in want.items():
        levels, total = ops.mip_shape(H, W)
        assert [(h, w) for _, h, w in levels] == sizes and len(levels) == int(np.floor(np.log2(max(H, W)))), (H, W)
        at = 0
        for off, h, w in levels:
            assert off == at
            at += h * w * 3
        assert total == at
    assert len(ops.mip_shape(8192, 8192)[0]) == 13 and ops.mip_shape(2, 2) == ([(0, 1, 1)], 3) and ops.mip_shape(2, 3)[0] == [(0, 1, 1)]
    n, total = C.c_int(), C.c_uint64()
    offs, hs, ws = (C.c_uint64 * 14)(), (C.c_int * 14)(), (C.c_int * 14)()
    for H, W in ((1, 100), (100, 1), (8193, 100), (100, 9000), (0, 0)):
        assert lib.d2s_mip_shape(H, W, C.byref(n), offs, hs, ws, C.byref(total)) == INVALID and b"2 .. 8192" in lib.d2s_last_error()
        assert lib.d2s_mip_chain(FAKE, 1, H, W, FAKE, None) == INVALID and b"2 .. 8192" in lib.d2s_last_error()
    assert lib.d2s_mip_shape(96, 160, None, offs, hs, ws, C.byref(total)) == INVALID
    assert lib.d2s_mip_shape(96, 160, C.byref(n), offs, hs, ws, None) == INVALID
    assert lib.d2s_mip_chain(None, 1, 96, 160, FAKE, None) == INVALID and lib.d2s_mip_chain(FAKE, 1, 96, 160, None, None) == INVALID
    for batch in (0, -1, 65536):
        assert lib.d2s_mip_chain(FAKE, batch, 96, 160, FAKE, None) == INVALID and b"batch" in lib.d2s_last_error()


def test_glow_range_and_uniforms_are_the_reference_s(manifest):
    """The manifest's numbers come from the reference's own _glow_range_m and _render_glow, executed on a stub object."""
    assert abs(xr.glow_range_m(xr.XrScreen(width=2.4, height=1.35, distance=2.0)) - 15.0) < 1e-12          # the reference's defaults: 15 m
    for c in manifest["cases"]:
        screen = xr.XrScreen(**c["screen"])
        assert abs(xr.glow_range_m(screen, c["head"]) - c["glow_range_m"]) <= 1e-12 * c["glow_range_m"], c["name"]
        u = xr.XrGlow({1: "glow", 2: "glow2"}[c["mode"]], c["range_m"], c["inner_edge_fraction"]).uniforms(screen)
        ref = c["glow_uniforms"]
        assert np.allclose(u["u_screen_half"], ref["u_screen_half"], rtol=1e-14, atol=0)
        assert abs(u["u_glow_inv_range"] - ref["u_glow_inv_range"]) <= 1e-14 * ref["u_glow_inv_range"]
        assert abs(u["u_glow_inner"] - ref["u_glow_inner"]) <= 1e-16 and (c["mode"] == 1) == (ref["u_glow_inner"] > 0)
        assert ref["u_glow_alpha_cap"] == 1.0 and ref["u_glow_use_source"] == 1 and ref["u_source_crop"] == [float(v) for v in c["crop"]]
        assert c["draw"] == {"outer": [24, 0], "inner": [24, 24]}
        # the glow quad is the screen's plane: the reference's glow model matrix is the screen's basis scaled by (glow_w, glow_h) / 2
        R, centre = screen.basis()
        S = np.diag([u["glow_w"] / 2.0, u["glow_h"] / 2.0, 1.0, 1.0])
        T = np.eye(4)
        T[:3, 3] = centre
        assert np.allclose(np.array(c["glow_model"]), T @ R @ S, rtol=2e-6, atol=2e-6), c["name"]
        # and the band vertices' uv are 0.5 + (screen a, b - 0.5) * (inner_w, inner_h) at the screen's corners
        v = np.array(c["band_verts"])
        assert v.shape == (48, 4) and np.allclose(v[:, :2], v[:, 2:] * 2 - 1, atol=1e-6)
        for col, size in ((2, u["inner_w"]), (3, u["inner_h"])):
            lo, hi, i = 0.5 - size / 2, 0.5 + size / 2, u["u_glow_inner"]
            want = np.unique(np.float32([0.0, lo, min(0.5, lo + i), max(0.5, hi - i), hi, 1.0]))
            assert np.allclose(np.unique(v[:, col]), want, atol=1e-6), (c["name"], col)
