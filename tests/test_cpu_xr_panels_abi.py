"""CPU: the C ABI and the host side of the world-space panels of the OpenXR eye image (include/d2s.h d2s_version() >= 133: d2s_xr_panel,
d2s_xr_texture, d2s_dibr_xr_panels, d2s_dibr_xr_panels_workspace, d2s_dibr_xr_panels_plan; csrc/dibr_xr.h xr_panels_plan; xr.XrPanel,
ops.dibr_xr_panels, ops.dibr_xr_panels_plan, depth.xr_eye_views*(panels=)) -- host code, no GPU.  The plan for a known layout (rows,
launches, each eye's tile rectangle from the float64 pixel boxes of tests/xr_panels_ref.py), zero launches for panels off the images,
every refusal by its words from the plan door AND from the entry called with NULL device pointers, and the Python constructors against
the matrices tests/golden/xr_panels.json recorded from the reference's own _render_fps_overlay / _render_keyboard."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

import xr_panels_ref as P
from desktop2stereo_amd import _lib, depth, ops, xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 5
U8, F32 = _lib.FMT_U8_HWC, _lib.FMT_F32_HWC
RGBA, WINDOW, PREMULT = _lib.DIBR_ALPHA["rgba"], _lib.DIBR_ALPHA["window"], _lib.DIBR_ALPHA["premultiplied"]
FOV = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))
NEW = ("d2s_dibr_xr_panels", "d2s_dibr_xr_panels_workspace", "d2s_dibr_xr_panels_plan")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(REPO, "tests", "golden", "xr_panels.json")) as f:
        return json.load(f)


def _vp(eye=0):
    return xr.fov_to_proj_mat4(*FOV[eye]) @ xr.pose_to_view_mat4((0, 0, 0, 1), (-0.032 if eye == 0 else 0.032, 0, 0))


def _eyes(sizes=((130, 100), (130, 100))):
    return [xr.xr_eye(_vp(i), w, h, i) for i, (w, h) in enumerate(sizes)]


SCREEN = xr.XrScreen(width=1.6, height=0.96, distance=1.5)


def test_abi_surface(lib):
    assert lib.d2s_version() >= 133
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None and f"int {name}(" in hdr
    for words in ("d2s_version() >= 133", "sizeof(d2s_xr_panel) = 160", "sizeof(d2s_xr_texture) = 24", "sizeof(d2s_xr_panels_plan_result) = 104",
                  "overlay.py:81-249", "overlay.py:1427-1510", "glsl.py:3-13, 28-40", "D2S_XR_PANEL_DEPTH_TEST = 1", "D2S_XR_WRAP_REPEAT = 0",
                  "row 0 = the TOP row", "tests/golden/xr_panels.npz", "D2S_DIBR_ALPHA_PREMULTIPLIED"):
        assert words in hdr, words
    S = _lib.XrPanel
    assert C.sizeof(S) == 160 and [getattr(S, n).offset for n in ("model", "texture", "flags", "color", "alpha", "struct_size")] == [0, 128, 132, 136, 152, 156]
    T = _lib.XrTexture
    assert C.sizeof(T) == 24 and [getattr(T, n).offset for n in ("rgba", "width", "height", "wrap", "struct_size")] == [0, 8, 12, 16, 20]
    R = _lib.XrPanelsPlanResult
    assert C.sizeof(R) == 104 and [getattr(R, n).offset for n in ("rows_per_eye", "drawn", "tile0", "tiles", "grid", "workspace_bytes", "offsets")] == \
        [4, 16, 24, 40, 56, 72, 88]
    assert (_lib.XR_PANEL_DEPTH_TEST, _lib.XR_PANEL_DEPTH_WRITE, _lib.XR_PANEL_BLEND, _lib.XR_MAX_PANELS) == (1, 2, 4, 32)
    nbytes = C.c_uint64()
    assert lib.d2s_dibr_xr_panels_workspace(2, C.byref(nbytes)) == 0 and nbytes.value == 2 * (48 + 32) * 96
    assert lib.d2s_dibr_xr_panels_workspace(3, C.byref(nbytes)) == INVALID
    row = ops._XR_ENTRIES["panels"]                                       # the entry table's row: plan and launch share one description
    assert ("d2s_" + row.direct, row.workspace, row.plan) == NEW and row.pipeline == ""
    for fn in (depth.xr_eye_views, depth.xr_eye_views_glow, depth.xr_eye_views_frost, depth.xr_eye_views_panorama):
        ps = inspect.signature(fn).parameters
        assert ps["panels"].default is None and ps["panel_textures"].default is None
    q = xr.XrPanel(np.eye(4), texture=None, color=(0.1, 0.2, 0.3, 0.4), alpha=0.5, depth_write=False).c_struct()
    assert (q.texture, q.flags, q.struct_size) == (-1, 1 | 4, 160) and q.alpha == 0.5 and list(q.model[:]) == list(np.eye(4).ravel())
    with pytest.raises(ValueError):
        xr.XrPanel(np.eye(3)).c_struct()


def _tiles(boxes):
    """The rectangle of 16 x 16 tiles the boxes touch: ((tile0 x, y), (tiles across, down))."""
    x0, y0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
    x1, y1 = max(b[2] for b in boxes), max(b[3] for b in boxes)
    return (x0 // 16, y0 // 16), (-(-x1 // 16) - x0 // 16, -(-y1 // 16) - y0 // 16)


def test_the_plan_of_a_known_layout(lib):
    eyes = _eyes(((130, 100), (111, 87)))
    status = xr.XrPanel.below_screen(SCREEN, (768, 238))
    kb = xr.XrPanel.keyboard_group(xr.XrPanel.keyboard_world(0.0, -0.75, 1.1, 0.0, -0.6), 1.2, 0.25, 0.8, [((-0.3, -0.05, -0.2, 0.05), (0.5, 0.85, 1.0, 0.7))])
    panels = [status] + kb
    plan = ops.dibr_xr_panels_plan(2, SCREEN, eyes, panels, [(238, 768), (384, 1280)])
    assert (plan["rows_per_eye"], plan["setup_launches"], plan["render_launches"], plan["drawn"]) == (1 + 4, 2, 1, [4, 4])
    want = []
    for e in eyes:
        boxes = [P.pixel_box(q.model, np.array(e.vp[:]).reshape(4, 4), e.width, e.height) for q in panels]
        assert all(b is not None for b in boxes)
        want.append(_tiles(boxes))
    assert plan["tile0"] == [w[0] for w in want] and plan["tiles"] == [w[1] for w in want]
    assert plan["grid"] == (max(w[1][0] for w in want), max(w[1][1] for w in want), 2 * 2)
    assert plan["tiles"][0][0] * 16 <= 130 + 15 and plan["tiles"][0] != (9, 7)      # (fewer tiles than the image has)
    offs, total = ops.dibr_xr_shape(eyes, 2, RGBA)
    assert (plan["workspace_bytes"], plan["out_elems"], plan["offsets"]) == (2 * 80 * 96, total, offs)
    # a curved screen: its 48 facets' rows come first; 49 rows are three chunks of 24 per eye
    curved = ops.dibr_xr_panels_plan(1, xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve="horizontal"), eyes, [status], [(8, 8)], alpha_mode=WINDOW, out_u8=False)
    assert (curved["rows_per_eye"], curved["setup_launches"], curved["render_launches"]) == (49, 6, 1)
    one = ops.dibr_xr_panels_plan(1, SCREEN, eyes[:1], [status] * 32, [(8, 8)])
    assert (one["rows_per_eye"], one["setup_launches"], one["drawn"], one["grid"][2]) == (33, 2, [32], 1)


def test_nothing_on_the_images_is_no_launch(lib):
    eyes = _eyes()
    behind, beside = np.eye(4), np.eye(4)
    behind[2, 3] = 1.0                                                      # z = +1: every vertex behind the eyes
    beside[:3, 3] = (40.0, 0.0, -2.0)                                       # in front, far off to the right of both images
    edge_on = np.eye(4)
    edge_on[:3, :3] = [[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]  # a quad collapsed to a line towards the viewer: covers no pixel centre
    edge_on[:3, 3] = (0.032, 0.0, -2.0)
    lone = ops.dibr_xr_panels_plan(1, SCREEN, eyes[1:], [xr.XrPanel(edge_on)])      # (the right eye, at x = 0.032, lies in the quad's plane)
    assert (lone["render_launches"], lone["drawn"]) == (0, [0])
    for panels in ([], [xr.XrPanel(behind)], [xr.XrPanel(beside)], [xr.XrPanel(behind), xr.XrPanel(beside)]):
        plan = ops.dibr_xr_panels_plan(1, SCREEN, eyes, panels)
        assert (plan["setup_launches"], plan["render_launches"], plan["drawn"], plan["grid"]) == (0, 0, [0, 0], (0, 0, 0)), panels
        assert plan["tiles"] == [(0, 0), (0, 0)] and plan["rows_per_eye"] == 1 + len(panels)
    # on one eye's image only: that eye's tiles alone
    right_only = np.diag([0.05, 0.05, 1.0, 1.0])
    right_only[:3, 3] = (1.45, 0.0, -2.0)
    plan = ops.dibr_xr_panels_plan(1, SCREEN, eyes, [xr.XrPanel(right_only)])
    boxes = [P.pixel_box(right_only, _vp(i), 130, 100) for i in range(2)]
    assert boxes[0] is None and boxes[1] is not None
    assert plan["drawn"] == [0, 1] and plan["tiles"][0] == (0, 0) and (plan["tile0"][1], plan["tiles"][1]) == _tiles([boxes[1]]) and plan["render_launches"] == 1


def _door(lib, panels, textures=(), eyes=None, screen=None, alpha_mode=RGBA, out_fmt=U8, batch=1, n_panels=None, n_textures=None):
    """(rc, words) of the plan door and of the entry called with NULL for out and workspace -- which can launch nothing."""
    ea = xr.eye_array(eyes or _eyes())
    sc = (screen or SCREEN).c_struct() if not isinstance(screen, _lib.XrScreen) else screen
    ps = [q if isinstance(q, _lib.XrPanel) else q.c_struct() for q in panels]
    pa = (_lib.XrPanel * len(ps))(*ps) if ps else None
    ta = (_lib.XrTexture * len(textures))(*textures) if textures else None
    n_p = len(ps) if n_panels is None else n_panels
    n_t = len(textures) if n_textures is None else n_textures
    r = _lib.XrPanelsPlanResult()
    r.struct_size = C.sizeof(r)
    rc = lib.d2s_dibr_xr_panels_plan(out_fmt, batch, alpha_mode, C.byref(sc), ea, len(ea), pa, n_p, ta, n_t, C.byref(r))
    said = lib.d2s_last_error() if rc else b""
    rc2 = lib.d2s_dibr_xr_panels(None, out_fmt, batch, alpha_mode, C.byref(sc), ea, len(ea), pa, n_p, ta, n_t, None, 0, None)
    said2 = lib.d2s_last_error()
    if rc:
        assert (rc2, said2) == (rc, said)
    else:
        assert (rc2, said2) == (INVALID, b"invalid argument: null pointer (workspace)")
    return rc, said


def _tex(w=8, h=8, wrap=0, size=24):
    return _lib.XrTexture(None, w, h, wrap, size)


def test_every_refusal_by_its_words(lib):
    m = np.diag([0.3, 0.2, 1.0, 1.0])
    m[2, 3] = -1.2                                                          # 0.6 x 0.4 m, 1.2 m in front of the eyes
    good = xr.XrPanel(m, texture=0)
    assert _door(lib, [good], [_tex()]) == (0, b"")
    assert _door(lib, [good], [_tex()], alpha_mode=WINDOW, out_fmt=F32) == (0, b"")

    def refused(code, words, *a, **kw):
        rc, said = _door(lib, *a, **kw)
        assert rc == code and words in said, (rc, said)

    refused(UNSUPPORTED, b"D2S_DIBR_ALPHA_PREMULTIPLIED", [good], [_tex()], alpha_mode=PREMULT)
    refused(INVALID, b"bad alpha_mode", [good], [_tex()], alpha_mode=3)
    refused(INVALID, b"bad out_fmt", [good], [_tex()], out_fmt=_lib.FMT_F32_CHW)
    refused(INVALID, b"bad batch", [good], [_tex()], batch=0)
    refused(INVALID, b"n_panels must be 0 .. 32", [good] * 33, [_tex()])
    refused(INVALID, b"n_panels must be 0 .. 32", [good], [_tex()], n_panels=-1)
    refused(INVALID, b"n_textures must be 0 .. 32", [good], [_tex()] * 33)
    refused(INVALID, b"null pointer (panels, textures)", [], [], n_panels=1)
    refused(INVALID, b"null pointer (panels, textures)", [], [], n_textures=1)
    bad = good.c_struct()
    bad.struct_size = 152
    refused(INVALID, b"d2s_xr_panel.struct_size must be sizeof(d2s_xr_panel) = 160", [bad], [_tex()])
    refused(INVALID, b"d2s_xr_texture.struct_size must be sizeof(d2s_xr_texture) = 24", [good], [_tex(size=16)])
    for w, h in ((0, 8), (8, 0), (8193, 8), (8, 9000)):
        refused(INVALID, b"a panel texture must be 1 .. 8192 on a side", [good], [_tex(w, h)])
    refused(INVALID, b"bad texture wrap", [good], [_tex(wrap=2)])
    for t in (1, -2):
        refused(INVALID, b"a panel's texture must be -1 (solid) or an index into textures", [xr.XrPanel(good.model, texture=t)], [_tex()])
    refused(INVALID, b"a panel's texture must be -1", [good], [])
    m = np.array(good.model)
    m[0, 0] = float("inf")
    refused(INVALID, b"model matrix must be finite", [xr.XrPanel(m)])
    for r_, c_, v in ((3, 0, 0.01), (3, 2, -1.0), (3, 3, 2.0)):
        m = np.array(good.model)
        m[r_, c_] = v
        refused(INVALID, b"model matrix must be affine (last row 0 0 0 1)", [xr.XrPanel(m)])
    bad = xr.XrPanel(good.model).c_struct()
    bad.flags = 8
    refused(INVALID, b"unknown panel flags", [bad])
    refused(INVALID, b"alpha and color must be finite", [xr.XrPanel(good.model, alpha=float("nan"))])
    refused(INVALID, b"alpha and color must be finite", [xr.XrPanel(good.model, color=(0.0, float("inf"), 0.0, 1.0))])
    crossing = np.eye(4)
    crossing[:3, :3] = [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]      # spans z = -1 .. 1, through the eyes' plane
    refused(UNSUPPORTED, b"the panel crosses the eye plane", [xr.XrPanel(crossing)])
    refused(UNSUPPORTED, b"the screen crosses the eye plane", [good], [_tex()],
            screen=xr.XrScreen(width=1.6, height=0.96, distance=0.2, yaw=1.2, curve="horizontal"))
    refused(INVALID, b"screen width, height and distance must be > 0", [good], [_tex()], screen=xr.XrScreen(width=0.0))
    sc = SCREEN.c_struct()
    sc.struct_size = 88
    refused(INVALID, b"d2s_xr_screen.struct_size", [good], [_tex()], screen=sc)
    refused(INVALID, b"eye image must be 2 .. 8192 on a side", [good], [_tex()], eyes=[xr.xr_eye(_vp(0), 1, 100, 0)])
    r = _lib.XrPanelsPlanResult()
    assert lib.d2s_dibr_xr_panels_plan(U8, 1, RGBA, C.byref(SCREEN.c_struct()), xr.eye_array(_eyes()), 2, None, 0, None, 0, C.byref(r)) == INVALID
    assert b"d2s_xr_panels_plan_result.struct_size" in lib.d2s_last_error()
    with pytest.raises(KeyError):
        ops.dibr_xr_panels_plan(1, SCREEN, _eyes(), [good], [(8, 8)], wrap="mirror")


def test_constructors_restate_the_reference_s_placements(meta):
    """Against what the reference's own methods uploaded (float32): the status panel's T @ R @ T_local @ S, the keyboard's world
    matrix and its three layers."""
    tol = 4e-7                                                           # float32 products of numbers of size <= 2: a few ulp
    for name in ("status", "status_faded_oblique"):
        c = next(c for c in meta["cases"] if c["name"] == name)
        got = xr.XrPanel.below_screen(xr.XrScreen(**c["screen"]), (768, 238), alpha=c["panels"][0]["alpha"])
        assert np.abs(got.model - np.array(c["recorded"]["status_model"])).max() <= tol, name
        assert (got.depth_test, got.depth_write, got.blend, got.texture) == (True, True, True, 0) and got.alpha == pytest.approx(c["panels"][0]["alpha"])
    assert np.array(next(c for c in meta["cases"] if c["name"] == "status_faded_oblique")["recorded"]["status_model"])[0, 2] != 0.0      # (yawed)
    c = next(c for c in meta["cases"] if c["name"] == "keyboard")
    rec = c["recorded"]
    kb = rec["kb"]
    world = xr.XrPanel.keyboard_world(kb["pan_x"], kb["pan_y"], kb["distance"], kb["yaw"], kb["pitch"])
    assert np.abs(world - np.array(rec["kb_world"])).max() <= tol
    group = xr.XrPanel.keyboard_group(world, kb["width"], kb["height"], rec["border_alpha"], [(rec["held_rect"], rec["highlight_color"])], texture=0)
    assert len(group) == len(c["panels"]) == 3
    for got, want in zip(group, c["panels"]):
        assert np.abs(got.model - np.array(want["model"])).max() <= tol
        assert (got.texture, got.depth_test, got.depth_write, got.blend) == (want["texture"], want["depth_test"], want["depth_write"], want["blend"])
        if want["texture"] is None:
            assert np.allclose(got.color, want["color"], rtol=0, atol=1e-7)
    assert [q.texture for q in xr.XrPanel.keyboard_group(world, 1.0, 0.3)] == [0]      # no border, no highlight: the keyboard alone
