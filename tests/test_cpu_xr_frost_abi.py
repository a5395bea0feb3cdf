"""CPU: the C ABI and the host side of the veil and frosted looks around the flat OpenXR screen (include/d2s.h d2s_version() >= 124:
d2s_xr_frost, d2s_dibr_xr_eyes_frost, d2s_dibr_xr_frost_workspace, d2s_dibr_xr_frost_plan, d2s_view_pipeline_xr_frost_streams;
desktop2stereo_amd/xr.py XrFrost).  Symbols and the struct; every refusal the header lists, reached through the host-only plan AND
through the entry with pointers that are never dereferenced -- the same code and the same words (a refused call launches nothing and
makes no HIP call, so no device is needed); the plans of the undrawn looks; xr.XrFrost's layout, model matrix, vertices and uniforms
against what the reference's own code produced on a stub object (tests/golden/xr_frost.json / .npz, make_golden_xr_frost.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from desktop2stereo_amd import _lib, ops, xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned pointer that a refused call never touches
F32 = _lib.FMT_F32_HWC
NEW = ("d2s_dibr_xr_eyes_frost", "d2s_dibr_xr_frost_workspace", "d2s_dibr_xr_frost_plan", "d2s_view_pipeline_xr_frost_streams")
OK, INVALID, UNSUPPORTED = 0, 1, 5
MODES = {1: "veil", 2: "frosted"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_frost.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_frost.npz")), json.load(f)


def _vp(eye=0):
    fov = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))[eye]
    return xr.fov_to_proj_mat4(*fov) @ xr.pose_to_view_mat4((0, 0, 0, 1), (-0.032 if eye == 0 else 0.032, 0, 0))


def _both(lib, frost, levels=FAKE, screen=None, H=96, W=160, dp=None, ws_bytes=1 << 16):
    """The plan's and the entry's (code, words) for one set of arguments.  The entry gets fake device pointers; levels: its chain."""
    dp = dp if dp is not None else ops.dibr_params()
    sc = screen if screen is not None else xr.XrScreen(width=1.6, height=0.96, distance=1.4).c_struct()
    ea = xr.eye_array([xr.xr_eye(_vp(i), 130, 100, i) for i in range(2)])
    fp = C.byref(frost) if frost is not None else None
    r = _lib.XrPlanResult()
    r.struct_size = C.sizeof(r)
    plan = lib.d2s_dibr_xr_frost_plan(24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, 2, F32, fp, C.byref(r))
    plan = (plan, lib.d2s_last_error() if plan else b"")
    call = lib.d2s_dibr_xr_eyes_frost(FAKE, FAKE, 24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, 2, FAKE, F32, FAKE, ws_bytes, fp, levels, None)
    call = (call, lib.d2s_last_error() if call else b"")
    return plan, call, r


def _refused(lib, code, word, frost, **kw):
    plan, call, _ = _both(lib, frost, **kw)
    assert plan[0] == code and word in plan[1], (word, plan)
    assert call == plan, (call, plan)


def test_symbols_struct_and_version(lib):
    assert lib.d2s_version() >= 124
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in hdr, name
    for words in ("d2s_version() >= 124", "sizeof(d2s_xr_frost) = 120", "_build_curved_frost_verts", "D2S_XR_KIND_FROST = 3", "effects.py:659",
                  "_frost_front_layout"):
        assert words in hdr, words
    assert "Frost, veil and border stay with the caller" not in hdr and "Frost, veil, border" not in hdr
    S = _lib.XrFrost
    assert C.sizeof(S) == 120 and S.struct_size.offset == 0 and S.mode.offset == 4 and S.head.offset == 8
    names = ["intensity", "alpha", "edge_inset", "beam_softness", "beam_thickness", "lod", "threshold", "noise_scale", "blend", "diffuse", "time"]
    assert [getattr(S, n).offset for n in names] == [32 + 8 * i for i in range(11)]
    a, b = _lib.SYMBOLS["d2s_dibr_xr_eyes_glow"][1], _lib.SYMBOLS["d2s_dibr_xr_eyes_frost"][1]
    assert len(a) == len(b) and [x for x, y in zip(a, b) if x is not y] == [C.POINTER(_lib.XrGlow)]      # the glow's list, the frost in its place
    a, b = _lib.SYMBOLS["d2s_view_pipeline_xr_glow_streams"][1], _lib.SYMBOLS["d2s_view_pipeline_xr_frost_streams"][1]
    assert len(a) == len(b) and [x for x, y in zip(a, b) if x is not y] == [C.POINTER(_lib.XrGlow)]
    a, b = _lib.SYMBOLS["d2s_dibr_xr_plan"][1], _lib.SYMBOLS["d2s_dibr_xr_frost_plan"][1]
    assert b[:-2] == a[1:-2] and b[-1] == a[-1] and b[-2] == C.POINTER(_lib.XrFrost)                     # d2s_dibr_xr_plan's without `entry`
    assert _lib.XR_KIND[3] == "frost" and _lib.XR_FROST == {"off": 0, "veil": 1, "frosted": 2}
    v, f = xr.XrFrost.veil().c_struct(), xr.XrFrost.frosted(head=(0.1, 0.2, 0.3), multiplier=2.0, time=1.5).c_struct()
    assert (v.struct_size, v.mode, v.intensity, v.alpha, v.edge_inset, v.beam_softness, v.beam_thickness) == (120, 1, 1.5, 1.0, 0.02, 0.34, 3.0)
    assert (f.mode, list(f.head), f.intensity, f.alpha, f.edge_inset, f.beam_softness, f.beam_thickness) == (2, [0.1, 0.2, 0.3], 2.0, 0.42, 0.045, 0.34, 1.6)
    assert (f.lod, f.threshold, f.noise_scale, f.blend, f.diffuse, f.time) == (5.4, 0.46, 54.0, 1.35, 0.85, 1.5)
    with pytest.raises(ValueError):
        xr.XrFrost(mode="mist").c_struct()
    assert callable(ops.dibr_xr_eyes_frost) and callable(ops.dibr_xr_frost_plan) and "view_pipeline_xr_frost" in dir(ops.Engine)
    n = C.c_uint64()
    for eyes in (1, 2):
        assert lib.d2s_dibr_xr_frost_workspace(eyes, C.byref(n)) == OK and n.value == eyes * 52 * 96      # the screen's 48 rows + 4 walls
    assert lib.d2s_dibr_xr_frost_workspace(3, C.byref(n)) == INVALID and lib.d2s_dibr_xr_frost_workspace(1, None) == INVALID


def test_every_frost_refusal_is_the_plan_s_and_the_entry_s(lib):
    V, Fr = (lambda **kw: xr.XrFrost.veil(**kw).c_struct()), (lambda **kw: xr.XrFrost.frosted(**kw).c_struct())
    for make in (V, Fr):
        for curve in ("horizontal", "vertical"):
            sc = xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve=curve).c_struct()
            _refused(lib, UNSUPPORTED, b"_build_curved_frost_verts", make(), screen=sc)
        sc = xr.XrScreen(width=1.6, height=0.96, distance=1.4, normal_offset=0.01).c_struct()
        _refused(lib, INVALID, b"normal_offset", make(), screen=sc)
        bad = make()
        bad.struct_size = 112
        _refused(lib, INVALID, b"d2s_xr_frost.struct_size", bad)
        for mode in (-1, 3):
            bad = make()
            bad.mode = mode
            _refused(lib, INVALID, b"frost mode", bad)
        for field in ("intensity", "alpha", "edge_inset", "beam_softness", "beam_thickness", "lod", "threshold", "noise_scale", "blend", "diffuse", "time"):
            for v in (float("nan"), float("inf")):
                _refused(lib, INVALID, b"finite", make(**{field: v}))
        for k in range(3):
            head = [0.0, 0.0, 0.0]
            head[k] = float("nan")
            _refused(lib, INVALID, b"finite", make(head=tuple(head)))
        _refused(lib, INVALID, b"noise_scale", make(noise_scale=-1.0))
        _refused(lib, INVALID, b"lod", make(lod=-0.5))
        # everything d2s_dibr_xr_eyes refuses, with its words, whatever the frost says
        _refused(lib, INVALID, b"feather", make(), dp=ops.dibr_params(feather=True))
        _refused(lib, INVALID, b"> 0", make(), screen=xr.XrScreen(width=-1.0).c_struct())
        _refused(lib, UNSUPPORTED, b"clip w", make(), screen=xr.XrScreen(width=1.6, height=0.96, distance=0.2, yaw=1.2).c_struct())
    _refused(lib, INVALID, b"8192", Fr(), H=96, W=8200)
    # the pointers are the entry's last checks: the plan accepts, the entry refuses
    for frost, kw, word in ((Fr(), dict(levels=None), b"levels"), (V(), dict(ws_bytes=2 * 48 * 96), b"d2s_dibr_xr_frost_workspace"),
                            (Fr(), dict(ws_bytes=0), b"d2s_dibr_xr_frost_workspace")):
        plan, call, r = _both(lib, frost, **kw)
        assert plan[0] == OK and _lib.XR_KIND[r.kind] == "frost" and call[0] == INVALID and word in call[1], (plan, call)
    plan, call, _ = _both(lib, V(), levels=None)          # the veil never reads levels: NULL passes (the next check meets no device: none is made)
    assert plan[0] == OK
    # the view pipeline checks its own arguments first (a null engine), with the same leading checks
    sc = xr.XrScreen().c_struct()
    ea = xr.eye_array([xr.xr_eye(_vp(0), 130, 100, 0)])
    dp, g, pp = ops.dibr_params(), V(), _lib.PostParams()
    assert lib.d2s_view_pipeline_xr_frost_streams(None, FAKE, 1, None, 96, 160, 140, None, C.byref(pp), C.byref(dp), None, C.byref(sc), ea, 1, 0, FAKE,
                                                  F32, None, FAKE, 1 << 16, C.byref(g), FAKE, None) == INVALID and b"engine" in lib.d2s_last_error()


def test_undrawn_looks_plan_to_the_plain_kernel_and_drawn_ones_to_frost(lib):
    n = C.c_uint64()
    assert lib.d2s_dibr_xr_workspace(2, C.byref(n)) == OK
    plain_ws = n.value
    off = xr.XrFrost(mode="off", intensity=float("nan")).c_struct()          # mode 0: nothing else is read
    for frost in (None, off, xr.XrFrost.veil(intensity=0.0).c_struct(), xr.XrFrost.frosted(multiplier=-1.0).c_struct(),
                  xr.XrFrost.veil(alpha=0.002).c_struct(), xr.XrFrost.veil(alpha=0.0).c_struct()):
        for curve in ("flat", "horizontal"):                                 # an undrawn look refuses no curved screen
            sc = xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve=curve).c_struct()
            plan, _, r = _both(lib, frost, screen=sc, ws_bytes=plain_ws)
            assert plan[0] == OK and _lib.XR_KIND[r.kind] == "plain" and r.workspace_bytes == plain_ws, (plan, r.kind)
            assert (r.rows_per_eye, r.setup_launches) == ((1, 2) if curve == "flat" else (48, 4))
    for frost in (xr.XrFrost.veil().c_struct(), xr.XrFrost.frosted().c_struct(), xr.XrFrost.frosted(alpha=0.002).c_struct()):
        plan, _, r = _both(lib, frost)
        assert plan[0] == OK and _lib.XR_KIND[r.kind] == "frost"
        assert (r.rows_per_eye, r.setup_launches, tuple(r.grid), r.lds_dynamic_bytes, r.lds_static_bytes) == (5, 2, (9, 7, 2), 0, 0)
        assert lib.d2s_dibr_xr_frost_workspace(2, C.byref(n)) == OK and r.workspace_bytes == n.value
    d = ops.dibr_xr_frost_plan(24, 40, 3, 96, 160, ops.dibr_params(alpha="rgba"), xr.XrScreen(width=1.6, height=0.96, distance=1.4),
                               [xr.xr_eye(_vp(0), 130, 100, 0), xr.xr_eye(_vp(1), 70, 51, 1)], xr.XrFrost.frosted())
    assert d["kind"] == "frost" and d["grid"] == (9, 7, 6) and d["offsets"] == [0, 3 * 100 * 130 * 4] and d["out_elems"] == 3 * 4 * (100 * 130 + 51 * 70)


def test_d2s_dibr_xr_plan_still_knows_three_entries(lib):
    sc = xr.XrScreen(width=1.6, height=0.96, distance=1.4).c_struct()
    ea = xr.eye_array([xr.xr_eye(_vp(0), 130, 100, 0)])
    dp = ops.dibr_params()
    r = _lib.XrPlanResult()
    r.struct_size = C.sizeof(r)
    assert C.sizeof(r) == 72 and _lib.XR_ENTRY == {"eyes": 0, "glow": 1, "glow_curved": 2}
    assert lib.d2s_dibr_xr_plan(3, 24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), ea, 1, F32, None, C.byref(r)) == INVALID
    assert b"entry" in lib.d2s_last_error()
    assert lib.d2s_dibr_xr_frost_plan(24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), ea, 1, F32, None, None) == INVALID
    bad = _lib.XrPlanResult()
    assert lib.d2s_dibr_xr_frost_plan(24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), ea, 1, F32, None, C.byref(bad)) == INVALID
    assert b"struct_size" in lib.d2s_last_error()


def test_layout_vertices_and_uniforms_are_the_reference_s(fixtures):
    """The manifest's numbers come from the reference's own _frost_front_layout, _build_flat_frost_verts, _frost_model_bytes and the two
    uniform setters, executed on a stub object.  The reference forms the head's local position and the model matrix in float32 and
    the library in float64: the layout and the matrix agree to float32's resolution (2e-6, the bound the glow's model matrix is
    held to), the vertices -- float32 in the mesh -- to 2 ulp of the largest coordinate."""
    z, meta = fixtures
    assert [c["name"] for c in meta["cases"]] == ["veil_front", "veil_oblique", "veil_crop_corner", "veil_outside", "veil_near", "frosted_default",
                                                  "frosted_time", "frosted_odd", "frosted_small", "frosted_lod_low", "frosted_lod_high",
                                                  "frosted_dark", "frosted_empty", "veil_empty"]
    splayed = 0
    for c in meta["cases"]:
        screen = xr.XrScreen(**c["screen"])
        fr = dict(c["frost"])
        frost = xr.XrFrost(**dict(fr, mode=MODES[fr["mode"]], head=tuple(fr["head"])))
        assert frost.draws() == (not c.get("empty", False)), c["name"]
        lay = frost.layout(screen)
        assert np.allclose(lay, c["layout"], rtol=2e-6, atol=0), (c["name"], lay, c["layout"])
        assert np.allclose(frost.model_mat4(screen), np.array(c["frost_model"]), rtol=2e-6, atol=2e-6), c["name"]
        verts = z[f"{c['name']}_verts"]
        mine = frost.wall_verts(screen)
        assert mine.shape == (4, 158, 5) and verts.shape == (632, 5) and verts.dtype == np.float32
        ulp = float(np.spacing(np.float32(np.abs(verts).max())))
        assert np.abs(mine.reshape(-1, 5) - verts.astype(np.float64)).max() <= 2 * ulp, (c["name"], np.abs(mine.reshape(-1, 5) - verts).max(), ulp)
        assert np.array_equal(mine[..., 2:].astype(np.float32).reshape(-1, 3), verts[:, 2:])      # t, u, v: exact eighths
        splayed += lay[1] > screen.width * 0.5 and lay[2] > screen.height * 0.5
        if c.get("empty"):
            assert c["frost_uniforms"] is None and c["draws"] == []
            continue
        assert c["draws"] == [[158, 158 * k] for k in range(4)]
        ref, u = c["frost_uniforms"], frost.uniforms(screen, c["crop"])
        assert set(ref) - {"u_model", "u_vp"} == set(u), (c["name"], sorted(ref), sorted(u))
        for k, v in u.items():
            assert np.allclose(ref[k], v, rtol=0, atol=0), (c["name"], k, ref[k], v)
    assert splayed >= 1          # fx != 1 != fy somewhere
    assert xr.XrFrost.veil().uniforms() == dict(u_source_crop=(0.0, 0.0, 1.0, 1.0), u_edge_inset=0.02, u_intensity=1.5, u_frost_alpha=1.0,
                                                u_beam_softness=0.34, u_beam_thickness=3.0)
