"""CPU: the C ABI and the host side of the panorama behind the CURVED OpenXR screen's looks (include/d2s.h d2s_version() >= 129:
d2s_dibr_xr_eyes_panorama_curved, d2s_dibr_xr_panorama_curved_plan, d2s_view_pipeline_xr_panorama_curved_streams).  Symbols and the
header's words; the plan accepts the four curved looks with a panorama, both curves, kind and `reserved` as the header says; every
refusal of the siblings, with their words, through the host-only plan AND through the entry with pointers that are never dereferenced
(a refused call launches nothing and makes no HIP call, so no device is needed); on flat cases, on the plain curved screen and without
a panorama the plan is the old entry's; and the old entry keeps refusing the curved looks."""
import ctypes as C
import os

import numpy as np
import pytest

from desktop2stereo_amd import _lib, depth, ops, xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned pointer that a refused call never touches
F32 = _lib.FMT_F32_HWC
NEW = ("d2s_dibr_xr_eyes_panorama_curved", "d2s_dibr_xr_panorama_curved_plan", "d2s_view_pipeline_xr_panorama_curved_streams")
OLD = ("d2s_dibr_xr_eyes_panorama", "d2s_dibr_xr_panorama_plan", "d2s_view_pipeline_xr_panorama_streams")
OK, INVALID, UNSUPPORTED = 0, 1, 5
FOVS = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def _pv(eye=0, pos=(0.0, 0.0, 0.0)):
    return xr.fov_to_proj_mat4(*FOVS[eye]), xr.pose_to_view_mat4((0, 0, 0, 1), (pos[0] + (-0.032 if eye == 0 else 0.032), pos[1], pos[2]))


def _pano(n_eyes=2, shape=(512, 1024), **kw):
    return xr.XrPanorama(**kw).c_struct([_pv(i) for i in range(n_eyes)], shape)


def _curved(curve="horizontal", **kw):
    return xr.XrScreen(**dict(dict(width=1.6, height=0.96, distance=1.5, curve=curve), **kw))


def _looks():
    return (("glow_curved", dict(glow=xr.XrGlow("glow", 1.2).c_struct())), ("glow_curved", dict(glow=xr.XrGlow("glow2", 1.2).c_struct())),
            ("frost_curved", dict(frost=xr.XrFrost.veil().c_struct())), ("frost_curved", dict(frost=xr.XrFrost.frosted().c_struct())))


def _both(lib, pano, glow=None, frost=None, screen=None, H=96, W=160, dp=None, ws_bytes=1 << 17, levels=FAKE, pano_rgb=FAKE, pano_levels=FAKE,
          n_eyes=2, names=NEW, eye_pos=(0.0, 0.0, 0.0)):
    """The plan's and the entry's (code, words) for one set of arguments.  The entry gets fake device pointers."""
    dp = dp if dp is not None else ops.dibr_params()
    sc = screen if screen is not None else _curved().c_struct()
    ea = xr.eye_array([xr.xr_eye(np.matmul(*_pv(i, eye_pos)), 130, 100, i) for i in range(n_eyes)])
    ref = lambda s: C.byref(s) if s is not None else None
    r = _lib.XrPlanResult()
    r.struct_size = C.sizeof(r)
    plan = getattr(lib, names[1])(24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, n_eyes, F32, ref(frost), ref(glow), ref(pano), C.byref(r))
    plan = (plan, lib.d2s_last_error() if plan else b"")
    call = getattr(lib, names[0])(FAKE, FAKE, 24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, n_eyes, FAKE, F32, FAKE, ws_bytes,
                                  ref(frost), levels, ref(glow), ref(pano), pano_rgb, pano_levels, None)
    call = (call, lib.d2s_last_error() if call else b"")
    return plan, call, r


def _refused(lib, code, word, pano, **kw):
    plan, call, _ = _both(lib, pano, **kw)
    assert plan[0] == code and word in plan[1], (word, plan)
    assert call == plan, (call, plan)


def test_symbols_version_and_header(lib):
    assert lib.d2s_version() >= 129
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for new, old in zip(NEW, OLD):
        assert new in _lib.SYMBOLS and getattr(lib, new) is not None
        assert f"int {new}(" in hdr, new
        assert _lib.SYMBOLS[new] == _lib.SYMBOLS[old], new                     # its sibling's argument types
    for words in ("d2s_version() >= 129", "tests/golden/xr_panorama_curved.npz", "GLOW_CURVED", "FROST_CURVED", "reserved = 1",
                  "keeps refusing", "a change of their own"):
        assert words in hdr, words
    assert callable(ops.dibr_xr_eyes_panorama_curved) and callable(ops.dibr_xr_panorama_curved_plan)
    assert "view_pipeline_xr_panorama_curved" in dir(ops.Engine) and "panorama_curved" in ops._XR_ENTRIES
    row = ops._XR_ENTRIES["panorama_curved"]
    assert ("d2s_" + row.direct, row.plan, "d2s_" + row.pipeline + "_streams") == NEW
    assert callable(depth.xr_eye_views_panorama) and "view_pipeline_xr_panorama_curved" in depth.xr_eye_views_panorama.__doc__


def test_the_plan_accepts_the_four_curved_looks_with_a_panorama(lib):
    for curve in ("horizontal", "vertical"):
        sc = _curved(curve).c_struct()
        for kind, look in _looks():
            plan, call, r = _both(lib, _pano(), screen=sc, H=512, W=1024, **look)
            assert plan == (OK, b"") and _lib.XR_KIND[r.kind] == kind and r.reserved == 1, (curve, kind, plan, r.kind, r.reserved)
            # ... and plans what the look's own entry plans: rows, set-up launches, grid, LDS and the workspace do not change
            without, _, r0 = _both(lib, None, screen=sc, H=512, W=1024, **look)
            assert without == (OK, b"") and r0.reserved == 0 and _lib.XR_KIND[r0.kind] == kind
            for f in ("rows_per_eye", "setup_launches", "lds_dynamic_bytes", "lds_static_bytes", "workspace_bytes", "out_elems"):
                assert getattr(r, f) == getattr(r0, f), f
            assert tuple(r.grid) == tuple(r0.grid)
            ws = C.c_uint64()
            assert lib.d2s_dibr_xr_frost_curved_workspace(2, C.byref(ws)) == OK and r.workspace_bytes <= ws.value
            # the old door still refuses, with the same code and the same words
            old_plan, old_call, _ = _both(lib, _pano(), screen=sc, H=512, W=1024, names=OLD, **look)
            assert old_plan[0] == UNSUPPORTED and b"CURVED" in old_plan[1] and b"a change of their own" in old_plan[1] and old_call == old_plan
    # the Python wrapper says the same
    eyes = [xr.xr_eye(np.matmul(*_pv(i)), 130, 100, i) for i in range(2)]
    dp = ops.dibr_params(alpha="rgba")
    d = ops.dibr_xr_panorama_curved_plan(24, 40, 1, 512, 1024, dp, _curved("vertical"), eyes, _pano(), glow=xr.XrGlow("glow2", 1.2), out_u8=False)
    assert d["kind"] == "glow_curved" and d["panorama"] and d["rows_per_eye"] == 52 and d["lds_static_bytes"] > 0
    d = ops.dibr_xr_panorama_curved_plan(24, 40, 1, 512, 1024, dp, _curved(), eyes, _pano(), frost=xr.XrFrost.frosted(), out_u8=False)
    assert d["kind"] == "frost_curved" and d["panorama"] and d["rows_per_eye"] == 244 and d["grid"] == (3, 2, 2)
    with pytest.raises(_lib.D2SError):
        ops.dibr_xr_panorama_plan(24, 40, 1, 512, 1024, dp, _curved(), eyes, _pano(), frost=xr.XrFrost.frosted(), out_u8=False)


def test_every_refusal_of_the_siblings_with_their_words(lib):
    glow, veil = xr.XrGlow("glow", 1.2).c_struct(), xr.XrFrost.veil().c_struct()
    # the curved glow's draw-order case: an eye outside the convex region (beyond an end of the arc)
    _refused(lib, UNSUPPORTED, b"convex region", _pano(), glow=glow, eye_pos=(3.0, 0.0, -1.0))
    _refused(lib, UNSUPPORTED, b"convex region", None, glow=glow, eye_pos=(3.0, 0.0, -1.0))
    plan, _, _ = _both(lib, _pano(), frost=veil, eye_pos=(0.9, 0.0, 0.2))                # (the walls have no such condition)
    assert plan[0] == OK
    # normal_offset with a look on
    off = _curved(normal_offset=0.01).c_struct()
    _refused(lib, INVALID, b"normal_offset must be 0 with frost on", _pano(), frost=veil, screen=off)
    _refused(lib, INVALID, b"normal_offset must be 0 with glow on", _pano(), glow=glow, screen=off)
    # a bad struct_size, anywhere
    bad = _pano()
    bad.struct_size = 168
    _refused(lib, INVALID, b"d2s_xr_panorama.struct_size", bad, glow=glow)
    g = xr.XrGlow("glow", 1.2).c_struct()
    g.struct_size = 16
    _refused(lib, INVALID, b"d2s_xr_glow.struct_size", _pano(), glow=g)
    f = xr.XrFrost.veil().c_struct()
    f.struct_size = 112
    _refused(lib, INVALID, b"d2s_xr_frost.struct_size", _pano(), frost=f)
    s = _curved().c_struct()
    s.struct_size = 88
    _refused(lib, INVALID, b"d2s_xr_screen.struct_size", _pano(), glow=glow, screen=s)
    # glow and frost both on, with or without a panorama
    for pano in (_pano(), None):
        _refused(lib, INVALID, b"at most one of glow and frost", pano, glow=glow, frost=veil)
    # the panorama's own fields
    for shape in ((1, 1024), (512, 8200)):
        _refused(lib, INVALID, b"2 .. 8192", _pano(shape=shape), glow=glow)
    _refused(lib, INVALID, b"finite", _pano(exposure=float("nan")), frost=veil)
    bad = _pano()
    bad.flip_y = 2
    _refused(lib, INVALID, b"flip_y", bad, frost=veil)
    bad = _pano()
    for k in range(9):
        bad.ray[1][k] = 0.0
    _refused(lib, INVALID, b"all zero", bad, glow=glow)
    # everything the underlying entries refuse
    _refused(lib, INVALID, b"feather", _pano(), glow=glow, dp=ops.dibr_params(feather=True))
    _refused(lib, UNSUPPORTED, b"clip w", _pano(), glow=glow, screen=_curved(distance=0.2, yaw=1.2).c_struct())
    _refused(lib, INVALID, b"range_m", _pano(), glow=xr.XrGlow("glow", -1.0).c_struct())
    _refused(lib, INVALID, b"lod", _pano(), frost=xr.XrFrost.frosted(lod=-0.5).c_struct())
    _refused(lib, INVALID, b"8192", _pano(), glow=glow, H=96, W=8200)
    # the pointers are the entry's last checks: the plan accepts, the entry refuses
    for kw, word in ((dict(pano_rgb=None, glow=glow), b"pano_rgb"), (dict(pano_levels=None, frost=veil), b"pano_rgb"),
                     (dict(ws_bytes=0, glow=glow), b"d2s_dibr_xr_glow_curved_workspace"), (dict(ws_bytes=0, frost=veil), b"d2s_dibr_xr_frost_curved_workspace"),
                     (dict(glow=glow, levels=None), b"levels"), (dict(frost=xr.XrFrost.frosted().c_struct(), levels=None), b"levels")):
        plan, call, r = _both(lib, _pano(), **kw)
        assert plan[0] == OK and r.reserved == 1 and call[0] == INVALID and word in call[1], (plan, call)
    # the plan's own arguments, and the view pipeline's leading checks (a null engine)
    sc = _curved().c_struct()
    ea = xr.eye_array([xr.xr_eye(np.matmul(*_pv(0)), 130, 100, 0)])
    dp, p1, pp = ops.dibr_params(), _pano(1), _lib.PostParams()
    assert lib.d2s_dibr_xr_panorama_curved_plan(24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), ea, 1, F32, None, None, C.byref(p1), None) == INVALID
    blank = _lib.XrPlanResult()
    assert lib.d2s_dibr_xr_panorama_curved_plan(24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), ea, 1, F32, None, None, C.byref(p1),
                                                C.byref(blank)) == INVALID
    assert b"struct_size" in lib.d2s_last_error()
    assert lib.d2s_view_pipeline_xr_panorama_curved_streams(None, FAKE, 1, None, 96, 160, 140, None, C.byref(pp), C.byref(dp), None, C.byref(sc), ea, 1,
                                                            0, FAKE, F32, None, FAKE, 1 << 17, C.byref(xr.XrFrost.veil().c_struct()), None, None,
                                                            C.byref(p1), FAKE, FAKE, None) == INVALID
    assert b"engine" in lib.d2s_last_error()


def test_a_superset_the_old_entry_s_answers_where_it_answers(lib):
    flat = xr.XrScreen(width=1.6, height=0.96, distance=1.4)
    eyes = [xr.xr_eye(np.matmul(*_pv(i)), 130, 100, i) for i in range(2)]
    dp = ops.dibr_params(alpha="rgba")
    glow, veil, frosted = xr.XrGlow("glow", 1.2), xr.XrFrost.veil(), xr.XrFrost.frosted()
    want = [(flat, None, None, "plain"), (_curved(), None, None, "plain"), (_curved("vertical"), None, None, "plain"), (flat, glow, None, "glow"),
            (flat, None, veil, "frost"), (flat, None, frosted, "frost"), (flat, xr.XrGlow("off"), xr.XrFrost(mode="off"), "plain"),
            (_curved(), xr.XrGlow("off"), xr.XrFrost.veil(intensity=0.0), "plain")]
    for screen, g, f, kind in want:
        for pano in (_pano(), None):
            new = ops.dibr_xr_panorama_curved_plan(24, 40, 1, 512, 1024, dp, screen, eyes, pano, glow=g, frost=f, out_u8=False)
            old = ops.dibr_xr_panorama_plan(24, 40, 1, 512, 1024, dp, screen, eyes, pano, glow=g, frost=f, out_u8=False)
            assert new == old and new["kind"] == kind and new["panorama"] == (pano is not None), (kind, new, old)
    # without a panorama the curved looks are what their own entries plan
    for g, f, kind in ((glow, None, "glow_curved"), (None, veil, "frost_curved")):
        d = ops.dibr_xr_panorama_curved_plan(24, 40, 1, 512, 1024, dp, _curved(), eyes, None, glow=g, frost=f, out_u8=False)
        own = ops.dibr_xr_plan("glow_curved", 24, 40, 1, 512, 1024, dp, _curved(), eyes, glow=g, out_u8=False) if g is not None else \
            ops.dibr_xr_frost_curved_plan(24, 40, 1, 512, 1024, dp, _curved(), eyes, f, out_u8=False)
        assert d["kind"] == kind and not d["panorama"] and own == {k: v for k, v in d.items() if k != "panorama"}, (kind, d, own)
