"""CPU: the veil and frosted looks around the curved OpenXR screen (include/d2s.h d2s_version() >= 126: d2s_dibr_xr_eyes_frost_curved,
d2s_dibr_xr_frost_curved_workspace, d2s_dibr_xr_frost_curved_plan, d2s_view_pipeline_xr_frost_curved_streams; desktop2stereo_amd/xr.py
XrFrost.curved_wall_verts).  No device: a refused call launches nothing and makes no HIP call.

  * symbols, header words, the version; the plan door: kind 4, 244 rows, 22 set-up launches, 46 848 bytes, the 64 x 64 grid;
  * every refusal in xr_plan's order, the same code and words from the query and from the entry; a flat screen plans to FROST, an
    undrawn look to PLAIN;
  * XrFrost.curved_wall_verts against the vertices the reference's own _build_curved_frost_verts wrote on a stub
    (tests/golden/xr_frost_curved.npz, make_golden_xr_frost_curved.py);
  * watertightness at headset size: the float32 cover rule against the float64 one over random poses, and the per-triangle form, which
    fails it.
"""
import ctypes as C
import os

import numpy as np
import pytest

from desktop2stereo_amd import _lib, ops, xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned pointer that a refused call never touches
F32 = _lib.FMT_F32_HWC
OK, INVALID, UNSUPPORTED = 0, 1, 5
NEW = ["d2s_dibr_xr_eyes_frost_curved", "d2s_dibr_xr_frost_curved_workspace", "d2s_dibr_xr_frost_curved_plan",
       "d2s_view_pipeline_xr_frost_curved_streams"]
MODES = {1: "veil", 2: "frosted"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    import xr_frost_curved_ref as K
    return K.load(golden_dir)


def _vp(eye=0, pos=(0.0, 0.0, 0.0), quat=(0, 0, 0, 1)):
    fov = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))[eye]
    return xr.fov_to_proj_mat4(*fov) @ xr.pose_to_view_mat4(quat, (pos[0] + (-0.032 if eye == 0 else 0.032), pos[1], pos[2]))


def _curved(curve="horizontal", **kw):
    return xr.XrScreen(**dict(dict(width=1.6, height=0.96, distance=1.4, curve=curve), **kw)).c_struct()


def _both(lib, frost, levels=FAKE, screen=None, H=96, W=160, dp=None, ws_bytes=1 << 16, sizes=((130, 100), (130, 100))):
    """The plan's and the entry's (code, words) for one set of arguments.  The entry gets a fake workspace pointer; levels: its chain."""
    dp = dp if dp is not None else ops.dibr_params()
    sc = screen if screen is not None else _curved()
    ea = xr.eye_array([xr.xr_eye(_vp(i), w, h, i) for i, (w, h) in enumerate(sizes)])
    fp = C.byref(frost) if frost is not None else None
    r = _lib.XrPlanResult()
    r.struct_size = C.sizeof(r)
    plan = lib.d2s_dibr_xr_frost_curved_plan(24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, len(ea), F32, fp, C.byref(r))
    plan = (plan, lib.d2s_last_error() if plan else b"")
    # rgb, depth and out are NULL: the entry looks at them last, so a call that passes every other check is refused there ("null
    # pointer") and can launch nothing; that refusal is reported as (OK, b"")
    call = lib.d2s_dibr_xr_eyes_frost_curved(None, None, 24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, len(ea), None, F32, FAKE, ws_bytes, fp,
                                             levels, None)
    call = (call, lib.d2s_last_error() if call else b"")
    if call[0] == INVALID and call[1].endswith(b": null pointer"):
        call = (OK, b"")
    return plan, call, r


def _refused(lib, code, word, frost, **kw):
    plan, call, _ = _both(lib, frost, **kw)
    assert plan[0] == code and word in plan[1], (word, plan)
    assert call == plan, (call, plan)


def test_symbols_header_and_version(lib):
    assert lib.d2s_version() >= 126
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in hdr, name
    for words in ("d2s_version() >= 126", "D2S_XR_KIND_FROST_CURVED = 4", "effects.py:189-254", "effects.py:759-787", "glsl.py:683-696", "D2S_XR_BIN=0",
                  "588 vertices", "sizeof(d2s_xr_frost) = 120", "d2s_dibr_xr_eyes_frost_curved below"):
        assert words in hdr, words
    assert C.sizeof(_lib.XrFrost) == 120
    for a, b in (("d2s_dibr_xr_eyes_frost", "d2s_dibr_xr_eyes_frost_curved"), ("d2s_dibr_xr_frost_plan", "d2s_dibr_xr_frost_curved_plan"),
                 ("d2s_view_pipeline_xr_frost_streams", "d2s_view_pipeline_xr_frost_curved_streams"),
                 ("d2s_dibr_xr_frost_workspace", "d2s_dibr_xr_frost_curved_workspace")):
        assert _lib.SYMBOLS[a] == _lib.SYMBOLS[b]
    assert _lib.XR_KIND[4] == "frost_curved"
    assert callable(ops.dibr_xr_eyes_frost_curved) and callable(ops.dibr_xr_frost_curved_plan) and "view_pipeline_xr_frost_curved" in dir(ops.Engine)
    n = C.c_uint64()
    for eyes in (1, 2):
        assert lib.d2s_dibr_xr_frost_curved_workspace(eyes, C.byref(n)) == OK and n.value == eyes * 244 * 96
    assert n.value == 46848
    assert lib.d2s_dibr_xr_frost_curved_workspace(3, C.byref(n)) == INVALID and lib.d2s_dibr_xr_frost_curved_workspace(1, None) == INVALID


def test_the_plan_door(lib):
    n = C.c_uint64()
    for make in (xr.XrFrost.veil, xr.XrFrost.frosted):
        for curve in ("horizontal", "vertical"):
            plan, call, r = _both(lib, make().c_struct(), screen=_curved(curve))
            assert plan[0] == OK and call[0] == OK and r.kind == 4 and _lib.XR_KIND[r.kind] == "frost_curved"
            assert (r.rows_per_eye, r.setup_launches, tuple(r.grid), r.lds_dynamic_bytes, r.lds_static_bytes) == (244, 22, (3, 2, 2), 0, 32)
            assert lib.d2s_dibr_xr_frost_curved_workspace(2, C.byref(n)) == OK and r.workspace_bytes == n.value == 46848
    d = ops.dibr_xr_frost_curved_plan(24, 40, 3, 96, 160, ops.dibr_params(alpha="rgba"), xr.XrScreen(width=1.6, height=0.96, distance=1.4, curve="vertical"),
                                      [xr.xr_eye(_vp(0), 2064, 2208, 0), xr.xr_eye(_vp(1), 2001, 2101, 1)], xr.XrFrost.frosted())
    assert d["kind"] == "frost_curved" and d["grid"] == (33, 35, 6) and d["rows_per_eye"] == 244 and d["setup_launches"] == 22
    assert d["offsets"] == [0, 3 * 2208 * 2064 * 4] and d["workspace_bytes"] == 46848 and d["lds_static_bytes"] == 32
    one = ops.dibr_xr_frost_curved_plan(24, 40, 1, 96, 160, ops.dibr_params(), xr.XrScreen(width=1.6, height=0.96, distance=1.4, curve="horizontal"),
                                        [xr.xr_eye(_vp(0), 130, 100, 0)], xr.XrFrost.veil())
    assert (one["setup_launches"], one["workspace_bytes"], one["grid"]) == (11, 244 * 96, (3, 2, 1))
    # d2s_dibr_xr_frost_plan, the flat entry's door, still refuses the curved screen
    with pytest.raises(_lib.D2SError, match="_build_curved_frost_verts"):
        ops.dibr_xr_frost_plan(24, 40, 1, 96, 160, ops.dibr_params(), xr.XrScreen(width=1.6, height=0.96, distance=1.4, curve="horizontal"),
                               [xr.xr_eye(_vp(0), 130, 100, 0)], xr.XrFrost.veil())


def test_a_flat_screen_plans_to_frost_and_an_undrawn_look_to_plain(lib):
    n = C.c_uint64()
    assert lib.d2s_dibr_xr_workspace(2, C.byref(n)) == OK
    plain_ws = n.value
    assert lib.d2s_dibr_xr_frost_workspace(2, C.byref(n)) == OK
    flat = xr.XrScreen(width=1.6, height=0.96, distance=1.4).c_struct()
    for frost in (xr.XrFrost.veil().c_struct(), xr.XrFrost.frosted().c_struct()):
        plan, call, r = _both(lib, frost, screen=flat, ws_bytes=n.value)
        assert plan[0] == OK and call[0] == OK and _lib.XR_KIND[r.kind] == "frost" and r.workspace_bytes == n.value
        assert (r.rows_per_eye, r.setup_launches, tuple(r.grid), r.lds_static_bytes) == (5, 2, (9, 7, 2), 0)
    off = xr.XrFrost(mode="off", intensity=float("nan")).c_struct()
    for frost in (None, off, xr.XrFrost.veil(intensity=0.0).c_struct(), xr.XrFrost.frosted(multiplier=-1.0).c_struct(),
                  xr.XrFrost.veil(alpha=0.002).c_struct()):
        for curve in ("flat", "horizontal", "vertical"):
            plan, call, r = _both(lib, frost, screen=_curved(curve), ws_bytes=plain_ws)
            assert plan[0] == OK and call[0] == OK and _lib.XR_KIND[r.kind] == "plain" and r.workspace_bytes == plain_ws
            assert (r.rows_per_eye, tuple(r.grid)) == ((1 if curve == "flat" else 48), (9, 7, 2))
        # an undrawn look refuses no normal_offset
        assert _both(lib, frost, screen=_curved(normal_offset=0.01), ws_bytes=plain_ws)[0][0] == OK


def test_every_refusal_in_order_is_the_plan_s_and_the_entry_s(lib):
    V, Fr = (lambda **kw: xr.XrFrost.veil(**kw).c_struct()), (lambda **kw: xr.XrFrost.frosted(**kw).c_struct())
    for make in (V, Fr):
        for curve in ("horizontal", "vertical"):
            _refused(lib, INVALID, b"normal_offset", make(), screen=_curved(curve, normal_offset=0.01))
        bad = make()
        bad.struct_size = 112
        _refused(lib, INVALID, b"d2s_xr_frost.struct_size", bad)
        for mode in (-1, 3):
            bad = make()
            bad.mode = mode
            _refused(lib, INVALID, b"frost mode", bad)
        for field in ("intensity", "alpha", "edge_inset", "beam_softness", "beam_thickness", "lod", "threshold", "noise_scale", "blend", "diffuse", "time"):
            _refused(lib, INVALID, b"finite", make(**{field: float("nan")}))
        _refused(lib, INVALID, b"finite", make(head=(0.0, float("inf"), 0.0)))
        _refused(lib, INVALID, b"noise_scale", make(noise_scale=-1.0))
        _refused(lib, INVALID, b"lod", make(lod=-0.5))
        _refused(lib, INVALID, b"feather", make(), dp=ops.dibr_params(feather=True))
        _refused(lib, INVALID, b"> 0", make(), screen=_curved(width=-1.0))
        # the order: the screen before the frost, the frost's fields before normal_offset, normal_offset before clip w
        _refused(lib, INVALID, b"> 0", make(lod=-1.0), screen=_curved(width=-1.0, normal_offset=0.01))
        _refused(lib, INVALID, b"lod", make(lod=-1.0), screen=_curved(normal_offset=0.01))
        _refused(lib, INVALID, b"normal_offset", make(), screen=_curved(distance=0.2, yaw=1.2, normal_offset=0.01))
        # the clip-w rule looks at the SCREEN's vertices only: the walls run past the eye in every accepted call above
        _refused(lib, UNSUPPORTED, b"clip w", make(), screen=_curved(distance=0.2, yaw=1.2))
    _refused(lib, INVALID, b"8192", Fr(), H=96, W=8200)
    # the pointers are the entry's last checks -- the workspace, then levels -- and the message names the new size query
    for frost, kw, word in ((Fr(), dict(levels=None), b"levels"), (V(), dict(ws_bytes=2 * 52 * 96), b"d2s_dibr_xr_frost_curved_workspace"),
                            (Fr(), dict(ws_bytes=46847, levels=None), b"d2s_dibr_xr_frost_curved_workspace")):
        plan, call, r = _both(lib, frost, **kw)
        assert plan[0] == OK and r.kind == 4 and call[0] == INVALID and word in call[1], (plan, call)
    assert _both(lib, V(), levels=None)[1][0] == OK          # the veil never reads levels
    sc = _curved()
    ea = xr.eye_array([xr.xr_eye(_vp(0), 130, 100, 0)])
    dp, g, pp = ops.dibr_params(), V(), _lib.PostParams()
    assert lib.d2s_view_pipeline_xr_frost_curved_streams(None, FAKE, 1, None, 96, 160, 140, None, C.byref(pp), C.byref(dp), None, C.byref(sc), ea, 1, 0,
                                                         FAKE, F32, None, FAKE, 1 << 16, C.byref(g), FAKE, None) == INVALID
    assert b"engine" in lib.d2s_last_error()


def test_curved_wall_verts_are_the_reference_s(fixtures):
    """The recorded vertices are what the reference's _build_curved_frost_verts wrote on a stub (float32 arithmetic in places, float32
    storage); the library's restatement is float64: rtol 2e-6, the bound the other host-side restatements are held to."""
    z, meta = fixtures
    curves = set()
    for c in meta["cases"]:
        screen = xr.XrScreen(**c["screen"])
        fr = dict(c["frost"])
        frost = xr.XrFrost(**dict(fr, mode=MODES[fr["mode"]], head=tuple(fr["head"])))
        assert frost.draws() == (not c.get("empty", False)), c["name"]
        assert np.allclose(frost.layout(screen), c["layout"], rtol=2e-6, atol=0), c["name"]
        verts, mine = z[f"{c['name']}_verts"], frost.curved_wall_verts(screen)
        assert mine.shape == (588, 8) and verts.shape == (588, 8) and verts.dtype == np.float32
        assert np.allclose(mine, verts, rtol=2e-6, atol=2e-7), (c["name"], float(np.abs(mine - verts).max()))
        assert np.array_equal(mine[:, 7], verts[:, 7]) and set(np.unique(verts[:, 7])) == {0.0, 1.0}
        if not c.get("empty"):
            curves.add((c["frost"]["mode"], screen.curve))
    assert curves == {(1, "horizontal"), (1, "vertical"), (2, "horizontal"), (2, "vertical")}
    with pytest.raises(ValueError):
        xr.XrFrost.veil().curved_wall_verts(xr.XrScreen())
    # the four walls are a closed tube: consecutive quads of a long wall share their edge bit for bit, the end quads' edges are the long
    # walls' first and last edges
    v = xr.XrFrost.veil(head=(0.3, -0.2, 0.1)).curved_wall_verts(xr.XrScreen(width=1.6, height=0.96, distance=1.4, curve="vertical", yaw=0.3))
    q = v.reshape(98, 6, 8)
    for wall in (0, 48):
        for i in range(47):
            assert np.array_equal(q[wall + i, 1], q[wall + i + 1, 0]) and np.array_equal(q[wall + i, 5], q[wall + i + 1, 2])
    for end, col in ((96, 0), (97, 47)):
        k = 0 if col == 0 else 1                     # the quad's first or second rear / front pair
        r, f = (0, 2) if k == 0 else (1, 5)
        assert np.array_equal(q[end, 0, :3], q[0 + col, r, :3]) and np.array_equal(q[end, 2, :3], q[0 + col, f, :3])
        assert np.array_equal(q[end, 1, :3], q[48 + col, r, :3]) and np.array_equal(q[end, 5, :3], q[48 + col, f, :3])


def _random_pose(rng, curve):
    screen = dict(width=float(rng.uniform(1.2, 2.6)), height=float(rng.uniform(0.7, 1.5)), distance=float(rng.uniform(1.0, 2.2)),
                  pan_x=float(rng.uniform(-0.2, 0.2)), pan_y=float(rng.uniform(-0.2, 0.2)), yaw=float(rng.uniform(-0.4, 0.4)),
                  pitch=float(rng.uniform(-0.2, 0.2)), roll=float(rng.uniform(-0.15, 0.15)), curve=curve, normal_offset=0.0)
    head = tuple(float(v) for v in rng.uniform(-0.25, 0.25, 3))
    pos = tuple(head[k] + float(rng.uniform(-0.1, 0.1)) for k in range(3))
    return screen, head, pos


def test_the_walls_are_watertight_in_float32_at_headset_size():
    """At 2064 x 2208, over 8 random poses (both curves): wherever a wall's float64 hit count is uniform on 3 x 3 -- off the wall's
    outline, off a fold, off the near plane's cut -- the float32 count of the library's form equals it: no hole and no double hit along
    an interior edge.  The per-triangle form, every triangle testing its own three float32 edges, fails that on the same poses."""
    import xr_frost_curved_ref as K
    import xr_glow_ref as R
    W, H = 2064, 2208
    rng = np.random.default_rng(126)
    bad_shared = bad_own = checked = 0
    for k in range(8):
        screen, head, pos = _random_pose(rng, ("horizontal", "vertical")[k % 2])
        vp = _vp(k % 2, pos)
        verts = xr.XrFrost(head=head).curved_wall_verts(xr.XrScreen(**screen))
        bx = K.boxes(verts, vp, W, H)
        rows = K.lib_rows(screen, head, vp, W, H)
        c64 = K.wall_counts(K.walk_hits(rows, W, H, np.float64, bx=bx, attrs=False), W, H)
        c32 = K.wall_counts(K.walk_hits(rows, W, H, np.float32, bx=bx, attrs=False), W, H)
        own = K.wall_counts(K.walk_hits(rows, W, H, np.float32, shared=False, bx=bx, attrs=False), W, H)
        for wall in range(4):
            ok = R.uniform3x3(c64[wall]) & (c64[wall] > 0)
            checked += int(ok.sum())
            bad_shared += int((c32[wall] != c64[wall])[ok].sum())
            bad_own += int((own[wall] != c64[wall])[ok].sum())
    print(f"\n[watertight, 8 poses at {W} x {H}] {checked} wall pixels checked; float32 count differs from float64: shared edge rows {bad_shared}, "
          f"per-triangle edges {bad_own}")
    assert checked >= 8 * 500000
    assert bad_shared == 0
    assert bad_own > 0
