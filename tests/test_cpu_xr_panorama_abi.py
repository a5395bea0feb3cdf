"""CPU: the C ABI and the host side of the panorama background behind the OpenXR screen (include/d2s.h d2s_version() >= 127:
d2s_xr_panorama, d2s_dibr_xr_eyes_panorama, d2s_dibr_xr_panorama_plan, d2s_view_pipeline_xr_panorama_streams; desktop2stereo_amd/xr.py
XrPanorama, panorama_rays).  Symbols, the struct and the header's words; every refusal the header lists, reached through the host-only
plan AND through the entry with pointers that are never dereferenced -- the same code and the same words (a refused call launches
nothing and makes no HIP call, so no device is needed); the kind chosen with and without a panorama; xr.panorama_rays against the
reference's own formula (xr_viewer/effects.py:992-1015, xr_viewer/glsl.py:81-83) on a fov_to_proj_mat4 / pose_to_view_mat4 pair."""
import ctypes as C
import os

import numpy as np
import pytest

from desktop2stereo_amd import _lib, depth, ops, xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned pointer that a refused call never touches
F32 = _lib.FMT_F32_HWC
NEW = ("d2s_dibr_xr_eyes_panorama", "d2s_dibr_xr_panorama_plan", "d2s_view_pipeline_xr_panorama_streams")
OK, INVALID, UNSUPPORTED = 0, 1, 5
FOVS = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def _pv(eye=0):
    return xr.fov_to_proj_mat4(*FOVS[eye]), xr.pose_to_view_mat4((0, 0, 0, 1), (-0.032 if eye == 0 else 0.032, 0, 0))


def _pano(n_eyes=2, shape=(512, 1024), **kw):
    return xr.XrPanorama(**kw).c_struct([_pv(i) for i in range(n_eyes)], shape)


def _both(lib, pano, glow=None, frost=None, screen=None, H=96, W=160, dp=None, ws_bytes=1 << 16, levels=FAKE, pano_rgb=FAKE, pano_levels=FAKE,
          n_eyes=2):
    """The plan's and the entry's (code, words) for one set of arguments.  The entry gets fake device pointers."""
    dp = dp if dp is not None else ops.dibr_params()
    sc = screen if screen is not None else xr.XrScreen(width=1.6, height=0.96, distance=1.4).c_struct()
    ea = xr.eye_array([xr.xr_eye(np.matmul(*_pv(i)), 130, 100, i) for i in range(n_eyes)])
    ref = lambda s: C.byref(s) if s is not None else None
    r = _lib.XrPlanResult()
    r.struct_size = C.sizeof(r)
    plan = lib.d2s_dibr_xr_panorama_plan(24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, n_eyes, F32, ref(frost), ref(glow), ref(pano), C.byref(r))
    plan = (plan, lib.d2s_last_error() if plan else b"")
    call = lib.d2s_dibr_xr_eyes_panorama(FAKE, FAKE, 24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, n_eyes, FAKE, F32, FAKE, ws_bytes,
                                         ref(frost), levels, ref(glow), ref(pano), pano_rgb, pano_levels, None)
    call = (call, lib.d2s_last_error() if call else b"")
    return plan, call, r


def _refused(lib, code, word, pano, **kw):
    plan, call, _ = _both(lib, pano, **kw)
    assert plan[0] == code and word in plan[1], (word, plan)
    assert call == plan, (call, plan)


def test_symbols_struct_version_and_header(lib):
    assert lib.d2s_version() >= 127
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in hdr, name
    for words in ("d2s_version() >= 127", "sizeof(d2s_xr_panorama) = 176", "_render_panorama_background", "effects.py:930-1021", "glsl.py:57-94",
                  "2 x 2 quad", "a change of their own", "tests/golden/xr_panorama.npz"):
        assert words in hdr, words
    S = _lib.XrPanorama
    assert C.sizeof(S) == 176
    assert [getattr(S, n).offset for n in ("struct_size", "flip_y", "height", "width", "yaw_offset", "exposure", "ray")] == [0, 4, 8, 12, 16, 24, 32]
    a, b = _lib.SYMBOLS["d2s_dibr_xr_eyes_frost"][1], _lib.SYMBOLS["d2s_dibr_xr_eyes_panorama"][1]
    assert b[:len(a) - 1] == a[:-1] and b[-1] == a[-1]                      # the frost entry's list, four more before the stream
    assert b[len(a) - 1:-1] == [C.POINTER(_lib.XrGlow), C.POINTER(_lib.XrPanorama), C.c_void_p, C.c_void_p]
    a, b = _lib.SYMBOLS["d2s_view_pipeline_xr_frost_streams"][1], _lib.SYMBOLS["d2s_view_pipeline_xr_panorama_streams"][1]
    assert b[:len(a) - 1] == a[:-1] and b[len(a) - 1:-1] == [C.POINTER(_lib.XrGlow), C.POINTER(_lib.XrPanorama), C.c_void_p, C.c_void_p]
    p = xr.XrPanorama(yaw_offset_deg=90.0, exposure=1.7, flip_y=True).c_struct([_pv(0)], (562, 1000))
    assert (p.struct_size, p.flip_y, p.height, p.width, p.yaw_offset, p.exposure) == (176, 1, 562, 1000, 0.25, 1.7)
    assert np.allclose(np.array(p.ray[0][:]).reshape(3, 3), xr.panorama_rays(*_pv(0)), rtol=0, atol=0) and not any(p.ray[1][:])
    with pytest.raises(ValueError):
        xr.XrPanorama().c_struct([], (512, 1024))
    assert callable(ops.dibr_xr_eyes_panorama) and callable(ops.dibr_xr_panorama_plan) and "view_pipeline_xr_panorama" in dir(ops.Engine)
    assert callable(depth.xr_eye_views_panorama)


def test_every_panorama_refusal_is_the_plan_s_and_the_entry_s(lib):
    bad = _pano()
    bad.struct_size = 168
    _refused(lib, INVALID, b"d2s_xr_panorama.struct_size", bad)
    for shape in ((1, 1024), (512, 1), (8193, 1024), (512, 8200), (0, 0), (-4, 16)):
        _refused(lib, INVALID, b"2 .. 8192", _pano(shape=shape))
    for kw in (dict(yaw_offset_deg=float("nan")), dict(yaw_offset_deg=float("inf")), dict(exposure=float("nan")), dict(exposure=float("-inf"))):
        _refused(lib, INVALID, b"finite", _pano(**kw))
    bad = _pano()
    bad.flip_y = 2
    _refused(lib, INVALID, b"flip_y", bad)
    for eye, k, v in ((0, 4, float("nan")), (1, 8, float("inf"))):
        bad = _pano()
        bad.ray[eye][k] = v
        _refused(lib, INVALID, b"finite", bad)
    bad = _pano()
    for k in range(9):
        bad.ray[1][k] = 0.0
    _refused(lib, INVALID, b"all zero", bad)
    plan, call, _ = _both(lib, bad, n_eyes=1)                                # ... of an eye in use: with one eye the second matrix is not read
    assert plan[0] == OK
    # a curved screen with a look on and a panorama: not built
    for curve in ("horizontal", "vertical"):
        sc = xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve=curve).c_struct()
        for look in (dict(glow=xr.XrGlow("glow", 1.2).c_struct()), dict(glow=xr.XrGlow("glow2", 1.2).c_struct()),
                     dict(frost=xr.XrFrost.veil().c_struct()), dict(frost=xr.XrFrost.frosted().c_struct())):
            _refused(lib, UNSUPPORTED, b"CURVED", _pano(), screen=sc, **look)
    # glow and frost both on, with or without a panorama
    for pano in (_pano(), None):
        _refused(lib, INVALID, b"at most one of glow and frost", pano, glow=xr.XrGlow("glow", 1.2).c_struct(), frost=xr.XrFrost.veil().c_struct())
    plan, _, r = _both(lib, _pano(), glow=xr.XrGlow("off").c_struct(), frost=xr.XrFrost.veil().c_struct())      # one of them off: fine
    assert plan[0] == OK and _lib.XR_KIND[r.kind] == "frost"
    # everything the underlying entries refuse, with their words
    _refused(lib, INVALID, b"feather", _pano(), dp=ops.dibr_params(feather=True))
    _refused(lib, INVALID, b"> 0", _pano(), screen=xr.XrScreen(width=-1.0).c_struct())
    _refused(lib, UNSUPPORTED, b"clip w", _pano(), screen=xr.XrScreen(width=1.6, height=0.96, distance=0.2, yaw=1.2).c_struct())
    _refused(lib, INVALID, b"range_m", _pano(), glow=xr.XrGlow("glow", -1.0).c_struct())
    _refused(lib, INVALID, b"lod", _pano(), frost=xr.XrFrost.frosted(lod=-0.5).c_struct())
    _refused(lib, INVALID, b"normal_offset", _pano(), frost=xr.XrFrost.veil().c_struct(),
             screen=xr.XrScreen(width=1.6, height=0.96, distance=1.4, normal_offset=0.01).c_struct())
    _refused(lib, INVALID, b"8192", _pano(), glow=xr.XrGlow("glow", 1.2).c_struct(), H=96, W=8200)
    # the pointers are the entry's last checks: the plan accepts, the entry refuses
    for kw, word in ((dict(pano_rgb=None), b"pano_rgb"), (dict(pano_levels=None), b"pano_rgb"), (dict(ws_bytes=0), b"d2s_dibr_xr_workspace"),
                     (dict(glow=xr.XrGlow("glow", 1.2).c_struct(), levels=None), b"levels")):
        plan, call, r = _both(lib, _pano(), **kw)
        assert plan[0] == OK and r.reserved == 1 and call[0] == INVALID and word in call[1], (plan, call)
    plan, _, _ = _both(lib, None, pano_rgb=None, pano_levels=None)           # no panorama: its image and chain are not looked at
    assert plan[0] == OK
    # the plan's own arguments, and the view pipeline's leading checks (a null engine)
    sc = xr.XrScreen().c_struct()
    ea = xr.eye_array([xr.xr_eye(np.matmul(*_pv(0)), 130, 100, 0)])
    dp, p1, pp = ops.dibr_params(), _pano(1), _lib.PostParams()
    assert lib.d2s_dibr_xr_panorama_plan(24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), ea, 1, F32, None, None, C.byref(p1), None) == INVALID
    blank = _lib.XrPlanResult()
    assert lib.d2s_dibr_xr_panorama_plan(24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), ea, 1, F32, None, None, C.byref(p1), C.byref(blank)) == INVALID
    assert b"struct_size" in lib.d2s_last_error()
    assert lib.d2s_view_pipeline_xr_panorama_streams(None, FAKE, 1, None, 96, 160, 140, None, C.byref(pp), C.byref(dp), None, C.byref(sc), ea, 1, 0,
                                                     FAKE, F32, None, FAKE, 1 << 16, None, None, None, C.byref(p1), FAKE, FAKE, None) == INVALID
    assert b"engine" in lib.d2s_last_error()


def test_the_kind_is_the_look_s_with_and_without_a_panorama(lib):
    flat = xr.XrScreen(width=1.6, height=0.96, distance=1.4)
    curved = xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve="horizontal")
    eyes = [xr.xr_eye(np.matmul(*_pv(i)), 130, 100, i) for i in range(2)]
    dp = ops.dibr_params(alpha="rgba")
    glow, veil, frosted = xr.XrGlow("glow", 1.2), xr.XrFrost.veil(), xr.XrFrost.frosted()
    want = [(flat, None, None, "plain"), (curved, None, None, "plain"), (flat, glow, None, "glow"), (flat, None, veil, "frost"),
            (flat, None, frosted, "frost"), (flat, xr.XrGlow("off"), xr.XrFrost(mode="off"), "plain"), (flat, None, xr.XrFrost.veil(intensity=0.0), "plain")]
    for screen, g, f, kind in want:
        with_p = ops.dibr_xr_panorama_plan(24, 40, 1, 512, 1024, dp, screen, eyes, _pano(), glow=g, frost=f, out_u8=False)
        without = ops.dibr_xr_panorama_plan(24, 40, 1, 512, 1024, dp, screen, eyes, None, glow=g, frost=f, out_u8=False)
        assert with_p["kind"] == without["kind"] == kind and with_p["panorama"] and not without["panorama"]
        assert {k: v for k, v in with_p.items() if k != "panorama"} == {k: v for k, v in without.items() if k != "panorama"}
        # ... and what the existing entry of that look plans
        if f is not None:
            old = ops.dibr_xr_frost_plan(24, 40, 1, 512, 1024, dp, screen, eyes, f, out_u8=False)
        else:
            old = ops.dibr_xr_plan("glow" if g is not None else "eyes", 24, 40, 1, 512, 1024, dp, screen, eyes, glow=g, out_u8=False)
        assert old == {k: v for k, v in without.items() if k != "panorama"}, (kind, old, without)
    # without a panorama the curved looks are drawn as their own entries draw them
    for g, f, kind in ((glow, None, "glow_curved"), (None, veil, "frost_curved")):
        d = ops.dibr_xr_panorama_plan(24, 40, 1, 512, 1024, dp, curved, eyes, None, glow=g, frost=f, out_u8=False)
        assert d["kind"] == kind and not d["panorama"]
    d = ops.dibr_xr_panorama_plan(24, 40, 3, 96, 160, dp, flat, [eyes[0], xr.xr_eye(np.matmul(*_pv(1)), 70, 51, 1)], _pano())
    assert d["grid"] == (9, 7, 6) and d["offsets"] == [0, 3 * 100 * 130 * 4] and d["out_elems"] == 3 * 4 * (100 * 130 + 51 * 70)
    assert d["lds_dynamic_bytes"] == 0 and d["lds_static_bytes"] == 0 and d["setup_launches"] == 2


def test_panorama_rays_are_the_reference_s_formula():
    """_render_panorama_background hands the shader inv(proj) and the view's rotation transposed; the shader forms
    inv_view_rot . normalize((inv_proj . (ndc, 1, 1)).xyz / max(|w|, 1e-6)), normalised.  panorama_rays . (ndc, 1) must point the same
    way for every pixel -- flipped projection or not, any head orientation."""
    rng = np.random.default_rng(5)
    for flip in (False, True):
        for q in ((0.0, 0.0, 0.0, 1.0), (0.1, -0.7, 0.2, 0.68), (0.0, 1.0, 0.0, 0.0)):
            q = np.array(q) / np.linalg.norm(q)
            proj = xr.fov_to_proj_mat4(-0.3, 0.9, 0.7, -0.2)
            view = xr.pose_to_view_mat4(q, (0.3, -1.2, 2.0))
            if flip:
                proj = proj.copy()
                proj[1, :] = -proj[1, :]
            rays = xr.panorama_rays(proj, view)
            assert rays.shape == (3, 3) and rays.dtype == np.float64
            inv_proj = np.linalg.inv(proj)
            view_rot = view.copy()
            view_rot[:3, 3] = 0.0
            inv_view_rot = view_rot.T
            ndc = rng.uniform(-1.3, 1.3, (200, 2))
            for x, y in ndc:
                vh = inv_proj @ np.array([x, y, 1.0, 1.0])
                vd = vh[:3] / max(abs(vh[3]), 1e-6)
                vd /= np.linalg.norm(vd)
                want = (inv_view_rot @ np.append(vd, 0.0))[:3]
                want /= np.linalg.norm(want)
                got = rays @ np.array([x, y, 1.0])
                assert np.allclose(got / np.linalg.norm(got), want, rtol=0, atol=1e-12), (flip, q, x, y)
    # the centre of a symmetric frustum looks along the head's -z
    d = xr.panorama_rays(xr.fov_to_proj_mat4(-0.5, 0.5, 0.5, -0.5), np.eye(4)) @ [0.0, 0.0, 1.0]
    assert abs(d[0]) < 1e-9 and abs(d[1]) < 1e-9 and d[2] < 0
