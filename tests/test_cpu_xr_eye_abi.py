"""CPU: the C ABI and the host side of the OpenXR eye views (include/d2s.h d2s_version() >= 115: d2s_xr_screen, d2s_xr_eye,
d2s_dibr_xr_shape, d2s_dibr_xr_workspace, d2s_dibr_xr_eyes, d2s_view_pipeline_xr_streams; desktop2stereo_amd/xr.py).  Symbols and
struct sizes; every refusal the header lists, made with pointers that are never dereferenced (a refused call launches nothing and
makes no HIP call, so no device is needed); the offsets d2s_dibr_xr_shape documents; the xr.py helpers against the reference's own
matrices and strip vertices, which make_golden_xr_eye.py recorded in tests/golden/xr_eye.json (float32 there, float64 here: agreement
to float32 rounding of values of magnitude <= ~3, i.e. 1e-6)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from desktop2stereo_amd import _lib, ops, xr
from desktop2stereo_amd.config import PipelineParams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned pointer that a refused call never touches
F32, U8 = _lib.FMT_F32_HWC, _lib.FMT_U8_HWC
NEW = ("d2s_dibr_xr_shape", "d2s_dibr_xr_workspace", "d2s_dibr_xr_eyes", "d2s_view_pipeline_xr_streams")
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def manifest(golden_dir):
    with open(os.path.join(golden_dir, "xr_eye.json")) as f:
        return json.load(f)


def _vp(eye=0):
    fov = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))[eye]
    return xr.fov_to_proj_mat4(*fov) @ xr.pose_to_view_mat4((0, 0, 0, 1), (-0.032 if eye == 0 else 0.032, 0, 0))


def _eyes(n=2, w=130, h=100, **kw):
    return xr.eye_array([xr.xr_eye(kw.get("vp", _vp(i)), w, h, i) for i in range(n)])


def _call(lib, dp=None, screen=None, eyes=None, n_eyes=None, crop=None, rgb=FAKE, depth=FAKE, dh=24, dw=40, batch=1, H=96, W=160, out=FAKE,
          fmt=F32, ws=FAKE, ws_bytes=1 << 16):
    dp = dp if dp is not None else ops.dibr_params()
    sc = screen if screen is not None else xr.XrScreen(width=1.6, height=0.96, distance=1.4).c_struct()
    ea = eyes if eyes is not None else _eyes()
    return lib.d2s_dibr_xr_eyes(rgb, depth, dh, dw, batch, H, W, C.byref(dp), crop, C.byref(sc) if sc else None, ea,
                                len(ea) if n_eyes is None else n_eyes, out, fmt, ws, ws_bytes, None)


def test_symbols_structs_and_version(lib):
    assert lib.d2s_version() >= 115
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in hdr, name
    assert "d2s_version() >= 115" in hdr and "xr_viewer/effects.py:1023-1137" in hdr and "mipmap" in hdr and "flip_y" in hdr
    assert C.sizeof(_lib.XrScreen) == 96 and _lib.XrScreen.width.offset == 8 and _lib.XrScreen.normal_offset.offset == 72 and _lib.XrScreen.clear.offset == 80
    assert C.sizeof(_lib.XrEye) == 144 and _lib.XrEye.width.offset == 128 and _lib.XrEye.eye.offset == 136 and _lib.XrEye.struct_size.offset == 140
    assert "sizeof(d2s_xr_screen) = 96" in hdr and "sizeof(d2s_xr_eye) = 144" in hdr
    a, b = _lib.SYMBOLS["d2s_view_pipeline_crop_streams"][1], _lib.SYMBOLS["d2s_view_pipeline_xr_streams"][1]
    assert b[:10] == a[:10] and b[-1] == a[-1]                               # the same leading pipeline arguments, the stream last


def test_shape_offsets_and_workspace(lib):
    ea = xr.eye_array([xr.xr_eye(_vp(0), 130, 100, 0), xr.xr_eye(_vp(1), 70, 50, 1)])
    offs, total = (C.c_uint64 * 2)(), C.c_uint64()
    assert lib.d2s_dibr_xr_shape(ea, 2, 3, 0, offs, C.byref(total)) == 0
    assert list(offs) == [0, 3 * 100 * 130 * 3] and total.value == 3 * 3 * (100 * 130 + 50 * 70)
    assert lib.d2s_dibr_xr_shape(ea, 2, 1, 2, offs, C.byref(total)) == 0                 # RGBA: four channels
    assert list(offs) == [0, 100 * 130 * 4] and total.value == 4 * (100 * 130 + 50 * 70)
    assert lib.d2s_dibr_xr_shape(ea, 1, 2, 0, offs, C.byref(total)) == 0 and total.value == 2 * 100 * 130 * 3
    assert ops.dibr_xr_shape(ea, 3) == ([0, 3 * 100 * 130 * 3], 3 * 3 * (100 * 130 + 50 * 70))
    for n in (0, 3, -1):
        assert lib.d2s_dibr_xr_shape(ea, n, 1, 0, offs, C.byref(total)) == INVALID and b"n_eyes" in lib.d2s_last_error()
    assert lib.d2s_dibr_xr_shape(None, 1, 1, 0, offs, C.byref(total)) == INVALID
    assert lib.d2s_dibr_xr_shape(ea, 2, 1, 0, None, C.byref(total)) == INVALID and lib.d2s_dibr_xr_shape(ea, 2, 1, 0, offs, None) == INVALID
    assert lib.d2s_dibr_xr_shape(ea, 2, 0, 0, offs, C.byref(total)) == INVALID and b"batch" in lib.d2s_last_error()
    assert lib.d2s_dibr_xr_shape(ea, 2, 1, 3, offs, C.byref(total)) == INVALID and b"alpha_mode" in lib.d2s_last_error()
    assert lib.d2s_dibr_xr_shape(_eyes(1, w=1), 1, 1, 0, offs, C.byref(total)) == INVALID and b"2 .. 8192" in lib.d2s_last_error()
    n = C.c_uint64()
    assert lib.d2s_dibr_xr_workspace(1, C.byref(n)) == 0 and n.value == 48 * 96
    assert lib.d2s_dibr_xr_workspace(2, C.byref(n)) == 0 and n.value == 2 * 48 * 96
    assert lib.d2s_dibr_xr_workspace(3, C.byref(n)) == INVALID and lib.d2s_dibr_xr_workspace(1, None) == INVALID


def _screen(**kw):
    return xr.XrScreen(**dict(dict(width=1.6, height=0.96, distance=1.4), **kw)).c_struct()


def test_every_refusal_without_a_device(lib):
    err = lib.d2s_last_error
    # the screen
    for kw in (dict(width=float("nan")), dict(yaw=float("inf")), dict(normal_offset=float("-inf")), dict(clear=(0, float("nan"), 0, 1))):
        assert _call(lib, screen=_screen(**kw)) == INVALID and b"finite" in err(), kw
    for curve in (-1, 3):
        sc = _screen()
        sc.curve = curve
        assert _call(lib, screen=sc) == INVALID and b"curve" in err()
    for kw in (dict(width=0.0), dict(height=-1.0), dict(distance=0.0)):
        assert _call(lib, screen=_screen(**kw)) == INVALID and b"> 0" in err(), kw
    sc = _screen()
    sc.struct_size = 88
    assert _call(lib, screen=sc) == INVALID and b"d2s_xr_screen.struct_size" in err()
    # the eyes
    for w, h in ((1, 100), (130, 1), (8193, 100), (130, 9000)):
        assert _call(lib, eyes=_eyes(w=w, h=h)) == INVALID and b"2 .. 8192" in err(), (w, h)
    for n in (0, 3, -2):
        assert _call(lib, n_eyes=n) == INVALID and b"n_eyes" in err(), n
    ea = _eyes()
    ea[1].struct_size = 136
    assert _call(lib, eyes=ea) == INVALID and b"d2s_xr_eye.struct_size" in err()
    ea = _eyes()
    ea[0].eye = 2
    assert _call(lib, eyes=ea) == INVALID and b"eye must be" in err()
    bad = _vp(0).copy()
    bad[2, 1] = float("nan")
    assert _call(lib, eyes=_eyes(1, vp=bad)) == INVALID and b"finite" in err()
    # the workspace
    assert _call(lib, ws_bytes=2 * 48 * 96 - 1) == INVALID and b"workspace_bytes" in err()
    assert _call(lib, eyes=_eyes(1), ws_bytes=48 * 96 - 1) == INVALID and b"workspace_bytes" in err()
    assert _call(lib, ws=None) == INVALID and b"workspace" in err()
    assert _call(lib, ws=C.c_void_p(4100)) == INVALID and b"aligned" in err()
    # the shader's uniforms: feathering, and everything d2s_dibr_warp_crop refuses
    assert _call(lib, dp=ops.dibr_params(feather=True)) == INVALID and b"feather" in err()
    dp = ops.dibr_params()
    dp.struct_size = 72
    assert _call(lib, dp=dp) == INVALID and b"struct_size" in err()
    assert _call(lib, dp=ops.dibr_params(search_radius=16.0)) == INVALID and b"search_radius" in err()
    assert _call(lib, dp=ops.dibr_params(corner_radius=0.6)) == INVALID and b"corner_radius" in err()
    for bad in ((float("nan"), 0, 1, 1), (-0.01, 0, 1, 1), (0, 0, 0, 1), (0.5, 0, 0.51, 1), (0, 0, 0.004, 1)):
        assert _call(lib, crop=(C.c_double * 4)(*bad)) == INVALID and b"crop" in err(), bad
    for kw in (dict(rgb=None), dict(depth=None), dict(out=None)):
        assert _call(lib, **kw) == INVALID and b"null" in err(), kw
    assert _call(lib, screen=False) == INVALID and b"null" in err()
    assert _call(lib, dh=0) == INVALID and b"depth shape" in err()
    assert _call(lib, H=1) == INVALID and _call(lib, batch=0) == INVALID and _call(lib, batch=40000) == INVALID
    assert _call(lib, fmt=_lib.FMT_F32_CHW) == INVALID and b"out_fmt" in err()
    # the screen crosses the eye plane: a vertex with clip w <= 1e-6
    assert _call(lib, screen=_screen(distance=0.2, yaw=1.2)) == UNSUPPORTED and b"eye plane" in err()
    assert _call(lib, screen=_screen(distance=0.1, curve="horizontal", width=3.0)) == UNSUPPORTED
    behind = xr.pose_to_view_mat4((0, 1, 0, 0), (0, 0, 0))                   # looking away from the screen
    assert _call(lib, eyes=_eyes(1, vp=xr.fov_to_proj_mat4(-0.7, 0.7, 0.6, -0.6) @ behind)) == UNSUPPORTED


def test_view_pipeline_xr_refusals_without_a_device(lib):
    pp, dp, sc, ea = ops.post_params(PipelineParams()), ops.dibr_params(), _screen(), _eyes()

    def view(e=None, frames=FAKE, dp=dp, sc=sc, ea=ea, n=2, out=FAKE):
        return lib.d2s_view_pipeline_xr_streams(e, frames, 1, None, 96, 160, 84, None, C.byref(pp), C.byref(dp), None, C.byref(sc) if sc else None,
                                                ea, n, 0, out, F32, None, FAKE, 1 << 16, None)
    assert view() == INVALID and b"null engine" in lib.d2s_last_error()       # everything before the engine passed
    assert view(frames=None) == INVALID and view(out=None) == INVALID and view(sc=None) == INVALID and view(ea=None) == INVALID
    assert view(n=3) == INVALID and b"n_eyes" in lib.d2s_last_error()
    bad = ops.dibr_params()
    bad.struct_size = 72
    assert view(dp=bad) == INVALID and b"struct_size" in lib.d2s_last_error()


def test_xr_helpers_restate_the_reference_geometry(manifest):
    assert abs(xr.CURVED_HALF_ANGLE_RAD - 0.48) < 1e-15 and xr.CURVED_SEGMENTS == 48
    tol = 1e-6
    for c in manifest["cases"]:
        s = xr.XrScreen(**c["screen"])
        assert np.abs(s.model_mat4() - np.array(c["model"])).max() <= tol, c["name"]
        if c["strip"] is not None:
            v = s.curved_verts()
            assert v.shape == (98, 5) and np.abs(v - np.array(c["strip"])).max() <= tol, c["name"]
        for e in c["eyes"]:
            proj, view = xr.fov_to_proj_mat4(*e["fov"]), xr.pose_to_view_mat4(e["orientation"], e["position"])
            assert np.abs(proj - np.array(e["proj"])).max() <= tol and np.abs(view - np.array(e["view"])).max() <= tol
            assert np.abs(proj @ view - np.array(e["vp"])).max() <= 2 * tol
    q = (0.1, -0.2, 0.05, math.sqrt(1 - 0.01 - 0.04 - 0.0025))
    v = xr.pose_to_view_mat4(q, (0.3, 1.6, -0.2))
    assert np.abs(v[:3, :3] @ v[:3, :3].T - np.eye(3)).max() < 1e-12 and np.abs(v @ np.array([0.3, 1.6, -0.2, 1.0]) - [0, 0, 0, 1]).max() < 1e-12
    e = xr.xr_eye(_vp(0), 130, 100, 1, flip_y=True)
    assert np.allclose(np.array(e.vp[4:8]), -_vp(0)[1]) and np.allclose(np.array(e.vp[:4]), _vp(0)[0]) and e.eye == 1


def test_python_surface():
    import inspect
    from desktop2stereo_amd import depth
    assert callable(ops.dibr_xr_eyes) and callable(ops.dibr_xr_shape) and "view_pipeline_xr" in dir(ops.Engine)
    assert list(inspect.signature(depth.xr_eye_views).parameters)[:4] == ["frames", "screen", "eyes", "crop"]
    with pytest.raises(ValueError):
        xr.XrScreen(curve="diagonal").c_struct()
    with pytest.raises(ValueError):
        xr.eye_array([])
