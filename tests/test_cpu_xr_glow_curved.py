"""CPU: the glow around the curved OpenXR screen (include/d2s.h d2s_version() >= 122: d2s_dibr_xr_glow_curved_workspace,
d2s_dibr_xr_eyes_glow_curved, d2s_view_pipeline_xr_glow_curved_streams; desktop2stereo_amd/xr.py XrScreen.glow_pieces, eye_inside).

  * the reference's recorded band mesh (tests/golden/xr_glow_curved.npz, make_golden_xr_glow_curved.py) lies on the library's planar
    pieces and carries their affine uv;
  * the kernel's search, emulated in float32 at 2064 x 2208 over 24 random eye poses, against the float64 rasteriser of the recorded
    triangles: the same region class and piece wherever the class is uniform on 3 x 3, and no hole;
  * XrScreen.eye_inside;
  * symbols, version, header text and every refusal -- made WITHOUT device pointers: the new entry looks at them last, so a call
    that names none is refused whatever else it says and can launch nothing;
  * the two restatements against the renders and each other, within the bounds the generator measured.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import xr_eye_ref as X
import xr_glow_curved_ref as K
import xr_glow_ref as R
from desktop2stereo_amd import _lib, ops, xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned WORKSPACE / levels pointer that a refused call never touches
F32 = _lib.FMT_F32_HWC
NEW = ("d2s_dibr_xr_glow_curved_workspace", "d2s_dibr_xr_eyes_glow_curved", "d2s_view_pipeline_xr_glow_curved_streams")
INVALID, UNSUPPORTED = 1, 5
FOV = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_glow_curved.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, "xr_glow_curved.npz"))


def _vp(eye=0, head=(0.0, 0.0, 0.0), q=(0.0, 0.0, 0.0, 1.0)):
    return xr.fov_to_proj_mat4(*FOV[eye]) @ xr.pose_to_view_mat4(q, (head[0] + (-0.032 if eye == 0 else 0.032), head[1], head[2]))


def test_recorded_mesh_lies_on_the_pieces(fixtures):
    meta, z = fixtures
    assert len(meta["cases"]) == 8
    for c in meta["cases"]:
        sc, glow, U, _ = K.case_objects(c)
        m = K.check_mesh(z[c["name"] + "_verts"], sc, glow, U)
        radius = (sc.height if sc.curve == "vertical" else sc.width) / 2.0 / xr.CURVED_HALF_ANGLE_RAD
        assert m["plane_m"] <= 1e-5 and m["uv"] <= 1e-6, (c["name"], m)
        # a vertical curve's long inner bands: chords of the arc between points that are no facet seams; a point of the arc is at most
        # the facets' sagitta from the facet under it
        assert m["arc_m"] <= radius * (1.0 - math.cos(xr.CURVED_HALF_ANGLE_RAD / xr.CURVED_SEGMENTS)) + 1e-5 and m["arc_uv"] <= 2e-6, (c["name"], m)
        assert (m["arc_m"] > 0) == (sc.curve == "vertical")
        assert c["draw"] == dict(outer=[K.N_OUTER_QUADS * 6, 0], inner=[K.N_INNER_QUADS * 6, K.N_OUTER_QUADS * 6])


def _random_pose(rng, sc, facets):
    """A head pose whose two eyes see the screen from inside the convex region, every strip vertex in front of them."""
    while True:
        head = rng.uniform([-0.35, -0.25, -0.3], [0.35, 0.25, 0.3])
        ax = rng.normal(size=3)
        ang = rng.uniform(-0.35, 0.35)
        q = np.append(ax / np.linalg.norm(ax) * math.sin(ang / 2), math.cos(ang / 2))
        vps = [_vp(e, head, q) for e in (0, 1)]
        if all(sc.eye_inside(vp) and X.min_clip_w(facets, vp) > 1e-6 for vp in vps):
            return vps


def test_search_float32_at_headset_size_random_poses(fixtures):
    """24 poses (8 recorded meshes: both curves, both modes; 3 head poses each, one eye of each in turn), 2064 x 2208, 1500 pixels with
    their 3 x 3 neighbourhoods each."""
    meta, z = fixtures
    w, h = 2064, 2208
    rng = np.random.default_rng(2208)
    compared = holes_checked = 0
    seen = set()
    for ci, c in enumerate(meta["cases"]):
        sc, glow, U, facets = K.case_objects(c)
        vertical, mode = sc.curve == "vertical", c["mode"]
        ids = np.array(K.quad_pieces(vertical))
        e_u, e_v = min(0.5, U["inner"] / U["inner_w"]), min(0.5, U["inner"] / U["inner_h"])
        verts = z[c["name"] + "_verts"]
        for k in range(3):
            vp = _random_pose(rng, sc, facets)[(ci + k) & 1]
            px, py = rng.integers(1, w - 1, 1500), rng.integers(1, h - 1, 1500)
            dx, dy = np.meshgrid([-1, 0, 1], [-1, 0, 1])
            xs, ys = (px[:, None] + dx.ravel()[None]), (py[:, None] + dy.ravel()[None])            # [1500, 9], centre = column 4
            xc, yc = xs + 0.5 - w / 2.0, ys + 0.5 - h / 2.0
            cls64, quad = K.classes(verts, c["draw"]["outer"][0], c["draw"]["inner"][0], facets, vp, w, h, U, mode, xc, yc)
            uni = (cls64 == cls64[:, 4:5]).all(1)
            s = K.search(K.piece_table(sc, glow, vp, w, h), vertical, e_v if vertical else e_u, e_u if vertical else e_v, mode,
                         xc[:, 4], yc[:, 4], np.float32)
            cls32, piece = K.search_classes(s, U, mode, np.float32)
            c64, q64 = cls64[:, 4], quad[:, 4]
            assert np.array_equal(cls32[uni], c64[uni]), (c["name"], k, np.nonzero(uni & (cls32 != c64))[0][:5])
            want = np.where(c64 == K.SCREEN, q64, np.where(c64 == K.NONE, -1, ids[np.maximum(q64, 0)]))
            arc = (c64 == K.SCREEN_INNER) & (want == K.ARC)                               # the facet under the arc's chord: any facet
            agree = (piece == want) | (arc & (piece >= 0) & (piece < K.N)) | (c64 == K.NONE)
            assert agree[uni].all(), (c["name"], k, piece[uni & ~agree][:5], want[uni & ~agree][:5])
            drawn = (cls64 != K.NONE).all(1)                                              # zero holes
            assert (cls32[drawn] != K.NONE).all(), (c["name"], k)
            compared += int(uni.sum())
            holes_checked += int(drawn.sum())
            seen |= set(np.unique(piece[uni]).tolist())
    assert compared > 24 * 1200 and holes_checked > 24 * 1200
    assert {K.T0, K.T1, K.C0, K.C1} <= seen and len(seen & set(range(K.N))) >= 40, sorted(seen)


def test_eye_inside(fixtures, golden_dir):
    meta, _ = fixtures
    for c in meta["cases"]:
        sc = K.case_objects(c)[0]
        for e in c["eyes"]:
            assert sc.eye_inside(np.array(e["vp"])), (c["name"], e["eye"])
    with open(os.path.join(golden_dir, "xr_eye.json")) as f:
        eye_cases = {c["name"]: c for c in json.load(f)["cases"]}
    c = eye_cases["curved_occluded"]                        # the arc seen from beyond its end
    sc = xr.XrScreen(**c["screen"])
    assert not any(sc.eye_inside(np.array(e["vp"])) for e in c["eyes"])
    for name in ("curved_h", "curved_v_yaw"):
        c = eye_cases[name]
        assert all(xr.XrScreen(**c["screen"]).eye_inside(np.array(e["vp"])) for e in c["eyes"])
    assert xr.XrScreen().eye_inside(_vp(0))                 # flat: nothing to be inside of
    behind = xr.XrScreen(curve="horizontal", distance=-1.5)                               # the screen behind the viewer: its back
    assert not behind.eye_inside(_vp(0))


def test_symbols_version_and_header(lib):
    assert lib.d2s_version() >= 122
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in hdr, name
    for text in ("d2s_version() >= 122", "xr_viewer/effects.py:408-474", "effects.py:314-406", "ordered multi-hit kernel", "1e-4 of the arc's radius",
                 "d2s_dibr_xr_eyes_glow_curved below draws it"):
        assert text in hdr, text
    assert _lib.SYMBOLS["d2s_dibr_xr_eyes_glow_curved"][1] == _lib.SYMBOLS["d2s_dibr_xr_eyes_glow"][1]
    assert _lib.SYMBOLS["d2s_view_pipeline_xr_glow_curved_streams"][1] == _lib.SYMBOLS["d2s_view_pipeline_xr_glow_streams"][1]
    n = C.c_uint64()
    for eyes, want in ((1, 52 * 96), (2, 2 * 52 * 96)):
        assert lib.d2s_dibr_xr_glow_curved_workspace(eyes, C.byref(n)) == 0 and n.value == want
    assert lib.d2s_dibr_xr_glow_curved_workspace(3, C.byref(n)) == INVALID and lib.d2s_dibr_xr_glow_curved_workspace(1, None) == INVALID


def _call(lib, glow, levels=FAKE, screen=None, H=96, W=160, dp=None, eyes=None, ws_bytes=1 << 16, ws=FAKE):
    """d2s_dibr_xr_eyes_glow_curved with NO device pointer for rgb, depth and out."""
    dp = dp if dp is not None else ops.dibr_params()
    sc = screen if screen is not None else xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve="horizontal").c_struct()
    ea = xr.eye_array(eyes if eyes is not None else [xr.xr_eye(_vp(i), 130, 100, i) for i in range(2)])
    return lib.d2s_dibr_xr_eyes_glow_curved(None, None, 24, 40, 1, H, W, C.byref(dp), None, C.byref(sc), ea, len(ea), None, F32, ws, ws_bytes,
                                            C.byref(glow) if glow is not None else None, levels, None)


def test_every_refusal_without_a_device(lib, golden_dir):
    err = lib.d2s_last_error
    G = lambda *a: xr.XrGlow(*a).c_struct()
    curved = lambda **kw: xr.XrScreen(**dict(dict(width=1.6, height=0.96, distance=1.5, curve="horizontal"), **kw)).c_struct()
    # a call that passes every other check ends at the device pointers: nothing is launched
    for mode in ("glow", "glow2"):
        for curve in ("horizontal", "vertical"):
            assert _call(lib, G(mode, 10.0), screen=curved(curve=curve)) == INVALID and b"null pointer" in err(), (mode, curve)
    # what d2s_dibr_xr_eyes_glow refuses about the glow, curvature apart
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        assert _call(lib, G("glow", bad)) == INVALID and b"range_m" in err(), bad
    for bad in (-0.01, float("nan")):
        assert _call(lib, G("glow", 10.0, bad)) == INVALID and b"inner_edge_fraction" in err(), bad
    g = G("glow", 10.0)
    g.mode = 3
    assert _call(lib, g) == INVALID and b"glow mode" in err()
    for mode in ("glow", "glow2"):
        assert _call(lib, G(mode, 10.0), levels=None) == INVALID and b"levels" in err()
        assert _call(lib, G(mode, 10.0), screen=curved(normal_offset=0.01)) == INVALID and b"normal_offset" in err()
        assert _call(lib, G(mode, 10.0), H=96, W=8200) == INVALID
    assert _call(lib, G("glow", 10.0), H=8192, W=8192) == UNSUPPORTED and b"64 KB" in err()
    # what d2s_dibr_xr_eyes refuses
    assert _call(lib, G("glow", 10.0), dp=ops.dibr_params(feather=True)) == INVALID and b"feather" in err()
    assert _call(lib, G("glow", 10.0), screen=curved(width=-1.0)) == INVALID and b"> 0" in err()
    assert _call(lib, G("glow", 10.0), ws=None) == INVALID and b"workspace" in err()
    assert _call(lib, G("glow", 10.0), ws=C.c_void_p(4100)) == INVALID and b"aligned" in err()
    # the larger table: d2s_dibr_xr_workspace's size is not enough
    assert _call(lib, G("glow", 10.0), ws_bytes=2 * 48 * 96) == INVALID and b"d2s_dibr_xr_glow_curved_workspace" in err()
    assert _call(lib, G("glow", 10.0), ws_bytes=2 * 52 * 96) == INVALID and b"null pointer" in err()
    # an eye outside the convex region: the existing fixtures' arc seen from beyond its end
    with open(os.path.join(golden_dir, "xr_eye.json")) as f:
        c = {c["name"]: c for c in json.load(f)["cases"]}["curved_occluded"]
    eyes = [xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in c["eyes"]]
    for mode in ("glow", "glow2"):
        assert _call(lib, G(mode, 10.0), screen=xr.XrScreen(**c["screen"]).c_struct(), eyes=eyes) == UNSUPPORTED and b"convex region" in err()
    # a flat screen, no glow or mode 0: d2s_dibr_xr_eyes_glow's own checks (its null-pointer check comes first)
    flat = xr.XrScreen(width=1.6, height=0.96, distance=1.4).c_struct()
    assert _call(lib, G("glow", 10.0), screen=flat) == INVALID and b"null pointer" in err()
    assert _call(lib, None) == INVALID and b"null pointer" in err()
    assert _call(lib, G("off", 10.0)) == INVALID and b"null pointer" in err()
    # the old entry still refuses a curved screen with glow on
    ea = xr.eye_array([xr.xr_eye(_vp(i), 130, 100, i) for i in range(2)])
    dp, sc, g = ops.dibr_params(), curved(), G("glow", 10.0)
    assert lib.d2s_dibr_xr_eyes_glow(FAKE, FAKE, 24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), ea, 2, FAKE, F32, FAKE, 1 << 16, C.byref(g), FAKE,
                                     None) == UNSUPPORTED and b"curved" in err()
    # the view pipeline checks its own arguments first (a null engine)
    pp = _lib.PostParams()
    assert lib.d2s_view_pipeline_xr_glow_curved_streams(None, FAKE, 1, None, 96, 160, 140, None, C.byref(pp), C.byref(dp), None, C.byref(sc), ea, 2, 0,
                                                        FAKE, F32, None, FAKE, 1 << 16, C.byref(g), FAKE, None) == INVALID and b"engine" in err()


def test_python_surface():
    import inspect
    from desktop2stereo_amd import depth
    assert list(inspect.signature(ops.dibr_xr_eyes_glow_curved).parameters) == list(inspect.signature(ops.dibr_xr_eyes_glow).parameters)
    assert list(inspect.signature(ops.Engine.view_pipeline_xr_glow_curved).parameters) == \
        list(inspect.signature(ops.Engine.view_pipeline_xr_glow).parameters)
    assert "_render_curved_glow" in depth.xr_eye_views_glow.__doc__
    sc = xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve="vertical")
    names = [p[0] for p in sc.glow_pieces(xr.XrGlow("glow", 10.0))]
    assert names == [f"facet{i}" for i in range(48)] + ["tangent0", "tangent1", "chord0", "chord1"]
    assert len(sc.glow_pieces()) == 50
    with pytest.raises(ValueError):
        xr.XrScreen().glow_pieces()


def _stats(a, b, ok):
    d = np.abs(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))[ok]
    da = np.abs(a[..., 3].astype(np.float64) - b[..., 3].astype(np.float64))[ok]
    return float((d > 1.0).mean()), float(d.mean()), float(da.max())


def test_restatements_against_the_renders(fixtures):
    """The float64 rasteriser of the recorded triangles against the SwiftShader render, and the float32 emulation of the kernel's
    search against that rasteriser: the figures the generator measured and stored (they bound the GPU test), reproduced."""
    meta, z = fixtures
    for c in meta["cases"]:
        img, dep = R.case_scene(c)
        levels = R.chain(img)
        for e in c["eyes"][:1] if c["name"].endswith("front") else c["eyes"]:            # (the front cases' eyes mirror each other)
            r64, cls = K.case_render(c, e, z[c["name"] + "_verts"], img, dep, levels, np.float64)
            r32, _ = K.case_search(c, e, img, dep, levels, np.float32)
            ok = R.uniform3x3(cls)
            assert abs((1.0 - ok.mean()) - e["excluded"]) < 1e-12 and e["excluded"] <= 0.10, (c["name"], e["eye"])
            assert [int(((cls == k) & ok).sum()) for k in range(4)] == e["classes"]
            gl, f32 = _stats(r64, K.golden_eye(z, c, e["eye"]), ok), _stats(r32, r64, ok)
            assert np.allclose(gl, e["gl"], rtol=1e-9, atol=1e-12), (c["name"], e["eye"], gl, e["gl"])
            assert all(a <= b * 1.05 + 1e-7 for a, b in zip(f32, e["f32"])), (c["name"], e["eye"], f32, e["f32"])
    # the oblique case: a tangent plane's horizon inside an image
    c = {c["name"]: c for c in meta["cases"]}["curved_h_glow_oblique"]
    assert max(e["behind"] for e in c["eyes"]) >= 0.05
