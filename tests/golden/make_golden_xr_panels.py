"""Golden vectors for the world-space panels of the OpenXR eye image (d2s_dibr_xr_panels): the REFERENCE's screen, then its panels,
drawn per eye off-screen on SwiftShader into an RGBA8 colour + DEPTH24 target, as EffectsMixin._render_eye does (effects.py:1023-1225).

    python tests/golden/make_golden_xr_panels.py        # -> tests/golden/xr_panels.npz + xr_panels.json

Everything of the reference is read from its checkout with `ast` at generation time and none of its text is stored:
  * _WORLD_VERT, _CURVED_VERT, _OVERLAY_FRAG, _SOLID_VERT, _SOLID_FRAG (xr_viewer/glsl.py) through gl_harness.to_es300; the XR fragment
    shader as make_golden_xr_eye.py takes it (asserted: it has no `discard`, so the screen's rounded corners write depth too);
  * OverlayMixin._render_fps_overlay, _render_keyboard and _kb_world_mat (xr_viewer/overlay.py), compiled on their own and EXECUTED on
    a stub object whose fake ctx, programs, textures and vaos record every draw: the program, u_mvp, u_alpha / u_color and the GL state
    (DEPTH_TEST, depth_mask, BLEND, blend_func) at the moment of the draw.  They are called with vp_mat = identity, so the recorded
    u_mvp IS the float32 model matrix; the eye's draw uploads float32(vp) @ model, as the reference forms it.
The state _render_eye leaves for them is what the stub starts from: DEPTH_TEST on, depth_mask True, BLEND off (effects.py:1044-1046;
every effect pass restores it: effects.py:473-474, 584-585, 786-787, 816-817, 1020-1021).
Asserted of the recordings: the status panel draws blended SRC_ALPHA / ONE_MINUS_SRC_ALPHA, depth-tested, depth_mask True; every draw
of the keyboard group blended the same way, depth-tested, depth_mask False, the border first (z -1 mm), the highlight last (z +1 mm).
The panels no reference method places here (in front of, behind and beside the screen, the pairs, the opaque quad) are this file's own
matrices, drawn in the status panel's recorded state with the flags the case names.
Textures: RGBA8, LINEAR / LINEAR, no mip levels, uploaded bottom row first (np.flipud, overlay.py:191), wrap REPEAT: nothing in the
reference sets repeat_x / repeat_y on them (it does on the frame and the panorama: frame.py:39-40, effects.py:959-960), and
moderngl's default is repeat.  The wrap is written into the manifest.

Stored per case and eye: dst = the RGBA8 target read back after the screen pass, and delta = (final - dst) mod 256, the target after the
panels.  Compared pixels (tests/xr_panels_ref.py compared()): class (screen coverage + the set of panels that pass) uniform on 3 x 3,
and no depth near-tie; asserted here: excluded <= 15 % per case and eye, and the case's own minimum of compared panel pixels.
Measured and recorded per case and eye: gl = the float64 restatement over dst against the render (max |rgb| in levels, max |alpha| in
levels), f32 = the float32 emulation against float64 (max |rgb| in levels, max |alpha| in 0..1).
What was measured: 0.5 level (the target's own rounding) for every solid panel and for the opaque texture, whose 255-level texel steps
show that the bilinear taps agree; up to 2.1 levels, mean 0.43, no bias, where a TEXTURED panel of alpha < 1 is blended.  That pattern
is what a renderer gives that rounds the fragment colour to the RGBA8 target's format before it blends and once more after (the
blended alpha s * s + (1 - s) * d doubles the first rounding); it was not traced further.  The restatement blends in float64 and
rounds nothing.
"""
from __future__ import annotations

import ast
import ctypes as C
import json
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
REF = "/root/reference/xr_viewer"

SRC_H, SRC_W = 96, 160
BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0, corner_radius=0.03, crop=[0.0, 0.0, 1.0, 1.0], clear=[0.1, 0.2, 0.3, 1.0],
            depth_hw=None, head=[0.0, 0.0, 0.0], eye_sizes=[[130, 100], [130, 100]], min_panel=150)
SCREEN = dict(width=1.6, height=0.96, distance=1.4, pan_x=0.0, pan_y=0.0, yaw=0.0, pitch=0.0, roll=0.0, curve="flat", normal_offset=0.0)
TEX_A = dict(seed=701, size=[8, 16], alpha_lo=40)
TEX_STATUS = dict(seed=702, size=[10, 32], alpha_lo=120)
TEX_KB = dict(seed=703, size=[6, 20], alpha_lo=160)
TEX_EDGE = dict(seed=704, size=[3, 4], alpha_lo=255, opaque=True)      # texels 40 pixels wide: the wrapped half texel at each edge shows
ALL = dict(depth_test=True, depth_write=True, blend=True)
# a quad: centre (cx, cy) and offset dz towards the viewer in the screen's frame, half sizes (hw, hh), and what it draws
Q = lambda cx, cy, dz, hw, hh, **kw: dict(dict(kind="quad", at=[cx, cy, dz, hw, hh], texture=None, color=[1.0, 1.0, 1.0, 1.0], alpha=1.0, **ALL), **kw)
CASES = [
    dict(BASE, name="front", seed=61, screen=dict(SCREEN), textures=[TEX_A], draws=[Q(0.1, 0.05, 0.3, 0.4, 0.25, texture=0)]),
    # 0.3 m behind the screen's plane, centred on its right edge: hidden under the screen, visible beside it
    dict(BASE, name="behind", seed=62, screen=dict(SCREEN), textures=[TEX_A], draws=[Q(0.8, 0.0, -0.3, 0.45, 0.3, texture=0)],
         min_hidden=300),
    dict(BASE, name="status", seed=63, screen=dict(SCREEN, width=1.3, height=1.3, pan_y=0.25), textures=[TEX_STATUS],
         draws=[dict(kind="status", texture=0, trigger=False)], min_panel=100),
    # the faded status panel under an oblique screen, seen from a head off to the side; eyes no multiple of 16 and of two sizes
    dict(BASE, name="status_faded_oblique", seed=64, screen=dict(SCREEN, width=1.3, height=1.3, pan_y=0.3, yaw=0.4, pitch=-0.15),
         head=[-0.3, 0.1, 0.2], eye_sizes=[[130, 100], [111, 87]], textures=[TEX_STATUS], draws=[dict(kind="status", texture=0, trigger=True)],
         min_panel=80),
    dict(BASE, name="solid_alpha", seed=65, screen=dict(SCREEN), textures=[], draws=[Q(-0.7, 0.3, 0.2, 0.35, 0.3, color=[0.2, 0.9, 0.4, 0.6])]),
    dict(BASE, name="keyboard", seed=66, screen=dict(SCREEN, pan_y=0.35), textures=[TEX_KB],
         draws=[dict(kind="keyboard", texture=0, border_alpha=0.8, kb=dict(pan_x=0.05, pan_y=-0.42, distance=1.1, yaw=0.1, pitch=-0.6,
                                                                         width=1.2, height=0.36), held_rect=[-0.3, -0.1, 0.1, 0.08])],
         min_panel=400),
    # two writing panels, the later one behind the earlier one (and in front of the screen): it shows only beside the first
    dict(BASE, name="two_writers", seed=67, screen=dict(SCREEN), textures=[TEX_A],
         draws=[Q(-0.2, 0.0, 0.4, 0.35, 0.3, texture=0), Q(0.2, 0.1, 0.2, 0.4, 0.3, color=[0.9, 0.3, 0.1, 0.7])], min_hidden=200),
    # the same pair, the first not writing depth: the second blends over it
    dict(BASE, name="two_no_write", seed=68, screen=dict(SCREEN), textures=[TEX_A],
         draws=[Q(-0.2, 0.0, 0.4, 0.35, 0.3, texture=0, depth_write=False), Q(0.2, 0.1, 0.2, 0.4, 0.3, color=[0.9, 0.3, 0.1, 0.7])]),
    # the opaque laser pass draws with blending off (effects.py:1197); a quad of alpha 0.5 unblended overwrites alpha too
    dict(BASE, name="opaque", seed=69, screen=dict(SCREEN), textures=[],
         draws=[Q(0.3, -0.2, 0.5, 0.5, 0.06, color=[1.0, 0.1, 0.1, 1.0], blend=False), Q(-0.4, 0.35, 0.1, 0.2, 0.2, color=[0.1, 0.4, 1.0, 0.5], blend=False)]),
    # a curved screen: its ends come 0.19 m towards the viewer, past the panel 0.1 m in front of its middle
    dict(BASE, name="curved", seed=70, screen=dict(SCREEN, curve="horizontal", distance=1.5), textures=[TEX_A],
         draws=[Q(0.0, 0.1, 0.1, 0.75, 0.3, texture=0)], min_hidden=200),
    # half off the left edge of the image; a second panel wholly behind the eyes draws nothing; small eyes of two sizes
    dict(BASE, name="half_off_behind_eye", seed=71, screen=dict(SCREEN), eye_sizes=[[97, 75], [130, 100]], textures=[TEX_A],
         draws=[Q(-0.95, 0.0, 0.4, 0.5, 0.3, texture=0), Q(0.0, 0.0, 2.4, 0.5, 0.3, color=[1.0, 1.0, 0.0, 1.0])], off_image=True),
    dict(BASE, name="wrap_edge", seed=72, screen=dict(SCREEN), textures=[TEX_EDGE], draws=[Q(0.0, 0.0, 0.25, 0.6, 0.4, texture=0)], wrap_band=True),
]


class _Uniform:
    def __init__(self):
        self.value, self.bytes = None, None

    def write(self, b):
        self.bytes = bytes(b)


class _Prog(dict):
    def __missing__(self, k):
        self[k] = _Uniform()
        return self[k]


def reference_overlay():
    """make() -> the stub object on which the reference's _render_fps_overlay / _render_keyboard run; stub.draws collects, per
    vao.render, dict(prog "overlay" | "solid", mvp float32 [4,4] (numpy convention), alpha | color, depth_test, depth_mask, blend,
    blend_func, mode)."""
    from make_golden_xr_eye import _defs
    fns = _defs(os.path.join(REF, "overlay.py"), ("_render_fps_overlay", "_render_keyboard", "_kb_world_mat"), "OverlayMixin")
    mgl = types.SimpleNamespace(DEPTH_TEST="DEPTH_TEST", BLEND="BLEND", SRC_ALPHA="SRC_ALPHA", ONE_MINUS_SRC_ALPHA="ONE_MINUS_SRC_ALPHA",
                                TRIANGLE_STRIP="TRIANGLE_STRIP")
    ns = {"np": np, "math": math, "moderngl": mgl}
    exec(compile(ast.Module(body=list(fns.values()), type_ignores=[]), REF, "exec"), ns)
    Stub = type("Stub", (), {k: ns[k] for k in fns})

    def make(screen):
        s = Stub()
        s.screen_width, s.screen_height, s.screen_distance = screen["width"], screen["height"], screen["distance"]
        s.screen_pan_x, s.screen_pan_y, s.screen_yaw, s.screen_pitch = screen["pan_x"], screen["pan_y"], screen["yaw"], screen["pitch"]
        s.draws, s.flags = [], {"DEPTH_TEST": True, "BLEND": False}               # what _render_eye leaves (effects.py:1044-1046)
        s.ctx = types.SimpleNamespace(enable=lambda f: s.flags.__setitem__(f, True), disable=lambda f: s.flags.__setitem__(f, False),
                                      depth_mask=True, blend_func=None)
        s._overlay_prog, s._border_prog = _Prog(), _Prog()

        def vao(name, prog):
            def render(mode):
                p = getattr(s, prog)
                rec = dict(prog=name, mode=mode, mvp=np.frombuffer(p["u_mvp"].bytes, np.float32).reshape(4, 4).T.copy(),
                           depth_test=s.flags["DEPTH_TEST"], depth_mask=bool(s.ctx.depth_mask), blend=s.flags["BLEND"], blend_func=s.ctx.blend_func)
                if name == "overlay":
                    rec["alpha"] = 1.0 if p["u_alpha"].value is None else float(p["u_alpha"].value)      # (the program's default, 1.0)
                else:
                    rec["color"] = [float(v) for v in p["u_color"].value]
                s.draws.append(rec)
            return types.SimpleNamespace(render=render)
        s._overlay_vao = s._keyboard_vao = vao("overlay", "_overlay_prog")
        s._border_vao = vao("solid", "_border_prog")
        tex = types.SimpleNamespace(use=lambda location=0: None)
        s._overlay_tex = s._keyboard_tex = tex
        # _render_fps_overlay: within a second of the last text rebuild, so the PIL path (the caller's picture) is not entered
        s._frame_now, s._last_overlay_update, s._overlay_tex_size, s.font = 10.0, 9.5, (768, 238), None
        s._ov_ltrig_held = s._ov_rtrig_held = False
        s._status_panel_alpha, s._last_frame_dt = 1.0, 0.016
        return s
    return make


def record_status(make, screen, trigger):
    s = make(screen)
    if trigger:                                            # held long enough: the fade has reached its floor (overlay.py:236)
        s._ov_ltrig_held, s._status_panel_alpha = True, 0.15
    s._render_fps_overlay(0, types.SimpleNamespace(use=lambda: None), np.eye(4, dtype=np.float32))
    assert len(s.draws) == 1 and s.flags == {"DEPTH_TEST": True, "BLEND": False} and s.ctx.depth_mask is True
    d = s.draws[0]
    assert (d["prog"], d["mode"], d["depth_test"], d["depth_mask"], d["blend"], d["blend_func"]) == \
        ("overlay", "TRIANGLE_STRIP", True, True, True, ("SRC_ALPHA", "ONE_MINUS_SRC_ALPHA")), d
    assert abs(d["alpha"] - (0.15 if trigger else 1.0)) < 1e-12 and s._overlay_prog["u_alpha"].value == 1.0      # (restored after the draw)
    return s.draws


def record_keyboard(make, screen, kb, border_alpha, held_rect):
    s = make(screen)
    s._keyboard_width, s._keyboard_height = kb["width"], kb["height"]
    s._keyboard_pan_x, s._keyboard_pan_y, s._keyboard_distance = kb["pan_x"], kb["pan_y"], kb["distance"]
    s._keyboard_yaw, s._keyboard_pitch = kb["yaw"], kb["pitch"]
    s._kb_border_alpha = border_alpha
    s._mod_state = {k: (False, False, 0.0) for k in ("shift", "ctrl", "alt", "win")}
    s._caps_lock = False
    s._keyboard_keys = [types.SimpleNamespace(vk=0x41, rect_local=tuple(held_rect))]
    s._kb_held_key_l, s._kb_held_key_r, s._kb_hover_l, s._kb_hover_r = 0, None, None, None
    s._grip_l_now = s._grip_r_now = False
    s._render_keyboard(types.SimpleNamespace(use=lambda: None), np.eye(4, dtype=np.float32))
    assert [d["prog"] for d in s.draws] == ["solid", "overlay", "solid"] and s.flags == {"DEPTH_TEST": True, "BLEND": False} and s.ctx.depth_mask is True
    for d in s.draws:
        assert (d["mode"], d["depth_test"], d["depth_mask"], d["blend"], d["blend_func"]) == \
            ("TRIANGLE_STRIP", True, False, True, ("SRC_ALPHA", "ONE_MINUS_SRC_ALPHA")), d
    kbw = np.asarray(s._kb_world_mat(), np.float64)
    local = [np.linalg.inv(kbw) @ d["mvp"].astype(np.float64) for d in s.draws]
    assert abs(local[0][2, 3] + 0.001) < 1e-6 and abs(local[1][2, 3]) < 1e-6 and abs(local[2][2, 3] - 0.001) < 1e-6      # -1 mm, 0, +1 mm
    assert s.draws[0]["color"][:3] == [0.3, 0.7, 1.0] and s.draws[2]["color"] == [0.5, 0.85, 1.0, 0.70]
    return s.draws, np.asarray(s._kb_world_mat(), np.float32)


def quad_model(screen, at):
    """This file's own placement: T @ R @ T_local(cx, cy, dz) @ S(hw, hh) in the screen's frame (xr.XrScreen.basis), as float32."""
    from desktop2stereo_amd import xr
    R, centre = xr.XrScreen(**{k: screen[k] for k in ("width", "height", "distance", "pan_x", "pan_y", "yaw", "pitch", "roll")}).basis()
    cx, cy, dz, hw, hh = at
    T, Tl = np.eye(4), np.eye(4)
    T[:3, 3] = centre
    Tl[:3, 3] = (cx, cy, dz)
    return (T @ R @ Tl @ np.diag([hw, hh, 1.0, 1.0])).astype(np.float32)


def rgba_texture(gl, img_top_first, unit):
    """uint8 [h,w,4], top row first -> RGBA8, LINEAR / LINEAR, REPEAT, no mip levels, uploaded bottom row first (overlay.py:191)."""
    g = gl.gl
    t = C.c_uint()
    g.glGenTextures(1, C.byref(t))
    g.glActiveTexture(0x84C0 + unit)
    g.glBindTexture(0x0DE1, t)
    g.glPixelStorei(0x0CF5, 1)
    data = np.ascontiguousarray(np.flipud(img_top_first))
    g.glTexImage2D(0x0DE1, 0, 0x8058, data.shape[1], data.shape[0], 0, 0x1908, 0x1401, data.ctypes.data)
    for k, v in ((0x2801, 0x2601), (0x2800, 0x2601), (0x2802, 0x2901), (0x2803, 0x2901)):
        g.glTexParameteri(0x0DE1, k, v)
    gl._check("rgba_texture")
    return t.value


def draw_eye(gl, screen_pass, panel_passes, w, h, clear):
    """An RGBA8 colour + DEPTH24 target: clear (colour, depth 1); the screen pass (depth test LESS, depth mask on, blending off);
    read back; every panel pass in its own state; read back -> (dst, final) uint8 [h,w,4], row 0 = top."""
    from make_golden_xr_glow import _set_uniforms
    g = gl.gl
    g.glClearDepthf.argtypes = [C.c_float]
    g.glUniformMatrix4fv.argtypes = [C.c_int, C.c_int, C.c_ubyte, C.c_void_p]
    g.glUniform3f.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float]
    fbo, tex, rbo = C.c_uint(), C.c_uint(), C.c_uint()
    g.glGenTextures(1, C.byref(tex))
    g.glActiveTexture(0x84C0 + 7)
    g.glBindTexture(0x0DE1, tex)
    g.glTexImage2D(0x0DE1, 0, 0x8058, w, h, 0, 0x1908, 0x1401, None)                  # RGBA8
    g.glTexParameteri(0x0DE1, 0x2801, 0x2600)
    g.glTexParameteri(0x0DE1, 0x2800, 0x2600)
    g.glGenRenderbuffers(1, C.byref(rbo))
    g.glBindRenderbuffer(0x8D41, rbo)
    g.glRenderbufferStorage(0x8D41, 0x81A6, w, h)                                     # DEPTH_COMPONENT24
    g.glGenFramebuffers(1, C.byref(fbo))
    g.glBindFramebuffer(0x8D40, fbo)
    g.glFramebufferTexture2D(0x8D40, 0x8CE0, 0x0DE1, tex, 0)
    g.glFramebufferRenderbuffer(0x8D40, 0x8D00, 0x8D41, rbo)
    if g.glCheckFramebufferStatus(0x8D40) != 0x8CD5:
        raise RuntimeError("framebuffer incomplete")
    g.glViewport(0, 0, w, h)
    g.glDepthMask(1)
    g.glClearColor(*[float(c) for c in clear])
    g.glClearDepthf(1.0)
    g.glClear(0x4000 | 0x0100)
    g.glDepthFunc(0x0201)                                                             # LESS

    def read():
        g.glFinish()
        out = np.empty((h, w, 4), np.uint8)
        g.glPixelStorei(0x0D05, 1)
        g.glReadPixels(0, 0, w, h, 0x1908, 0x1401, out.ctypes.data)
        gl._check("read")
        return out[::-1].copy()

    def run(p):
        (g.glEnable if p["blend"] else g.glDisable)(0x0BE2)
        g.glBlendFunc(0x0302, 0x0303)                                                 # SRC_ALPHA, ONE_MINUS_SRC_ALPHA (overlay.py:243)
        (g.glEnable if p["depth_test"] else g.glDisable)(0x0B71)
        g.glDepthMask(1 if p["depth_mask"] else 0)
        for unit, t in p["textures"].items():
            g.glActiveTexture(0x84C0 + unit)
            g.glBindTexture(0x0DE1, t)
        g.glUseProgram(p["prog"])
        _set_uniforms(g, p["prog"], p["uniforms"])
        loc = g.glGetUniformLocation(p["prog"], b"u_mvp")
        assert loc >= 0
        mt = np.ascontiguousarray(np.asarray(p["mvp"], np.float32).T)
        g.glUniformMatrix4fv(loc, 1, 0, mt.ctypes.data)
        verts = np.ascontiguousarray(p["verts"], np.float32)
        ncomp, stride = p["ncomp"], (p["ncomp"] + 2) * 4
        vbo = C.c_uint()
        g.glGenBuffers(1, C.byref(vbo))
        g.glBindBuffer(0x8892, vbo)
        g.glBufferData(0x8892, verts.nbytes, verts.ctypes.data, 0x88E4)
        g.glEnableVertexAttribArray(0)
        g.glEnableVertexAttribArray(1)
        g.glVertexAttribPointer(0, ncomp, 0x1406, 0, stride, C.c_void_p(0))
        g.glVertexAttribPointer(1, 2, 0x1406, 0, stride, C.c_void_p(ncomp * 4))
        g.glDrawArrays(0x0005, 0, verts.shape[0])
        g.glDeleteBuffers(1, C.byref(vbo))
    run(screen_pass)
    dst = read()
    for p in panel_passes:
        run(p)
    final = read()
    g.glDisable(0x0B71)
    g.glDisable(0x0BE2)
    g.glDepthMask(1)
    g.glBindFramebuffer(0x8D40, 0)
    g.glDeleteFramebuffers(1, C.byref(fbo))
    g.glDeleteRenderbuffers(1, C.byref(rbo))
    g.glDeleteTextures(1, C.byref(tex))
    return dst, final


def main():
    import gl_harness as G
    import xr_eye_ref as X
    import xr_panels_ref as P
    from make_golden_xr_crop import xr_shader_patch
    from make_golden_xr_eye import FOV, _strings, case_inputs, reference_geometry
    make_screen, fov_to_proj, pose_to_view = reference_geometry()
    make_stub = reference_overlay()
    (_, _, _), (fs, l0, l1) = G.reference_shaders()
    patch, p0, p1 = xr_shader_patch()
    assert "discard" not in patch(fs), "the XR fragment shader discards: the screen's depth would have holes"
    src = _strings(os.path.join(REF, "glsl.py"), ("_WORLD_VERT", "_CURVED_VERT", "_OVERLAY_FRAG", "_SOLID_VERT", "_SOLID_FRAG"))
    fs2, defaults = G.to_es300(patch(fs))
    gl = G.Gles()
    es = {k: G.to_es300(v)[0] for k, v in src.items()}
    progs = {"flat": gl.program(es["_WORLD_VERT"], fs2), "curved": gl.program(es["_CURVED_VERT"], fs2),
             "overlay": gl.program(es["_WORLD_VERT"], es["_OVERLAY_FRAG"]), "solid": gl.program(es["_SOLID_VERT"], es["_SOLID_FRAG"])}
    quad = np.array([[-1, -1, 0, 0], [1, -1, 1, 0], [-1, 1, 0, 1], [1, 1, 1, 1]], np.float32)      # implementation.py:1060-1065
    data = {}
    meta = {"cases": [], "gl": {"version": gl.version, "renderer": gl.renderer}, "fov": FOV, "source": [SRC_H, SRC_W], "wrap": "repeat",
            "shader": f"panels: xr_viewer/glsl.py _WORLD_VERT + _OVERLAY_FRAG, _SOLID_VERT + _SOLID_FRAG; screen: viewer.py:{l0}-{l1} through "
                      f"xr_viewer/implementation.py:{p0}-{p1} behind _WORLD_VERT / _CURVED_VERT (no discard: asserted); ES 3.00 patches: see gl_harness.py",
            "textures": "RGBA8, LINEAR / LINEAR, no mip levels, REPEAT (moderngl's default; the reference sets no wrap on them), uploaded "
                        "bottom row first; the pictures come from their seeds (tests/xr_panels_ref.py case_textures)",
            "target": "RGBA8 + DEPTH_COMPONENT24; depth test LESS; panels blended SRC_ALPHA, ONE_MINUS_SRC_ALPHA where the draw says so",
            "encoding": "<case>_<eye>_dst = uint8 [h,w,4] read back after the screen pass; <case>_<eye>_delta = (final - dst) mod 256",
            "bounds": "per case and eye over the compared pixels: gl = [max |rgb| in levels, max |alpha| in levels] of the float64 restatement "
                      "over dst against the render; f32 = [max |rgb| in levels, max |alpha| in 0..1] of the float32 emulation against float64",
            "depth_steps": P.DEPTH_STEPS}
    for c in CASES:
        img, dep, _ = case_inputs(c)
        tc, td = gl.texture(img, 0), gl.texture(dep, 1)
        sc = c["screen"]
        s = make_screen(**sc)
        curved = sc["curve"] != "flat"
        model = np.asarray(s._build_model_mat4(normal_offset=sc["normal_offset"]), np.float32)
        strip = np.asarray(s._build_curved_screen_verts(normal_offset=sc["normal_offset"]), np.float32).reshape(-1, 5) if curved else None
        facets = X.facets_strip(strip, sc["curve"] == "vertical") if curved else X.facets_flat(model)
        pics = P.case_textures(c)
        gl_tex = [rgba_texture(gl, t, 2) for t in pics]
        # the draws: the reference's recordings or this file's quads -> manifest panels (model float32, flags) in draw order
        panels, recorded = [], {}
        for d in c["draws"]:
            if d["kind"] == "status":
                rec = record_status(make_stub, sc, d["trigger"])
                recorded["status_model"] = rec[0]["mvp"].tolist()
                panels.append(dict(model=rec[0]["mvp"].tolist(), texture=d["texture"], color=[1.0, 1.0, 1.0, 1.0], alpha=rec[0]["alpha"],
                                   depth_test=True, depth_write=rec[0]["depth_mask"], blend=True, source="_render_fps_overlay"))
            elif d["kind"] == "keyboard":
                rec, kbw = record_keyboard(make_stub, sc, d["kb"], d["border_alpha"], d["held_rect"])
                recorded.update(kb_world=kbw.tolist(), kb=d["kb"], border_alpha=d["border_alpha"], held_rect=d["held_rect"],
                                highlight_color=rec[2]["color"])
                for r in rec:
                    solid = r["prog"] == "solid"
                    panels.append(dict(model=r["mvp"].tolist(), texture=None if solid else d["texture"], color=r["color"] if solid else [1.0, 1.0, 1.0, 1.0],
                                       alpha=1.0 if solid else r["alpha"], depth_test=r["depth_test"], depth_write=r["depth_mask"], blend=r["blend"],
                                       source="_render_keyboard"))
            else:
                panels.append(dict(model=quad_model(sc, d["at"]).tolist(), texture=d["texture"], color=d["color"], alpha=d["alpha"],
                                   depth_test=d["depth_test"], depth_write=d["depth_write"], blend=d["blend"], source="generator"))
        rec_case = dict({k: v for k, v in c.items() if k != "draws"}, model=model.tolist(), strip=strip.tolist() if curved else None,
                        panels=panels, recorded=recorded, eyes=[])
        ref_panels = P.case_panels(rec_case)
        for eye in (0, 1):
            w, h = c["eye_sizes"][eye]
            l, r, u, dn = FOV[eye]
            fov = types.SimpleNamespace(angle_left=l, angle_right=r, angle_up=u, angle_down=dn)
            pos = [c["head"][0] + (-0.032 if eye == 0 else 0.032), c["head"][1], c["head"][2]]
            pose = types.SimpleNamespace(orientation=types.SimpleNamespace(x=0.0, y=0.0, z=0.0, w=1.0),
                                         position=types.SimpleNamespace(x=pos[0], y=pos[1], z=pos[2]))
            proj, view = fov_to_proj(fov), pose_to_view(pose)
            vp = proj @ view
            assert vp.dtype == np.float32 and X.min_clip_w(facets, vp) > 1e-6
            uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(SRC_W), float(SRC_H)),
                       u_eye_offset=float((1.0 if eye else -1.0) * c["ipd_uv"] / 2.0), u_depth_strength=float(0.1 * c["depth_ratio"]),
                       u_convergence=float(c["convergence"]), u_roll=float(sc["roll"]), u_feather_enabled=0, u_feather_width=0.02,
                       u_viewport=(0.0, 0.0, float(w), float(h)), u_source_crop=tuple(float(v) for v in c["crop"]),
                       **{k: float(v) for k, v in defaults.items()})
            uni["u_corner_radius"] = float(c["corner_radius"])
            base = dict(textures={0: tc, 1: td}, uniforms=uni, blend=False, depth_test=True, depth_mask=True)
            screen_pass = dict(base, prog=progs["curved"], mvp=vp, verts=strip, ncomp=3) if curved else \
                dict(base, prog=progs["flat"], mvp=vp @ model, verts=quad, ncomp=2)
            passes = []
            for q in panels:
                m = np.asarray(q["model"], np.float32)
                if q["texture"] is None:
                    passes.append(dict(prog=progs["solid"], uniforms=dict(u_color=tuple(q["color"])), textures={}, mvp=vp @ m, verts=quad, ncomp=2,
                                       blend=q["blend"], depth_test=q["depth_test"], depth_mask=q["depth_write"]))
                else:
                    passes.append(dict(prog=progs["overlay"], uniforms=dict(tex=2, u_alpha=float(q["alpha"])), textures={2: gl_tex[q["texture"]]},
                                       mvp=vp @ m, verts=quad, ncomp=2, blend=q["blend"], depth_test=q["depth_test"], depth_mask=q["depth_write"]))
            dst, final = draw_eye(gl, screen_pass, passes, w, h, c["clear"])
            d64 = np.concatenate([dst[..., :3].astype(np.float64), dst[..., 3:].astype(np.float64) / 255.0], -1)
            r64, info = P.render(d64, facets, vp, w, h, ref_panels, pics, "repeat", np.float64)
            r32, _ = P.render(d64, facets, vp, w, h, ref_panels, pics, "repeat", np.float32)
            ok = P.compared(info)
            excluded = float(1.0 - ok.mean())
            assert excluded <= 0.15, (c["name"], eye, excluded)
            drawn = info["passed"].any(0)
            n_panel = int((ok & drawn).sum())
            assert n_panel >= c["min_panel"], (c["name"], eye, n_panel)
            extra = {}
            if "min_hidden" in c:      # pixels a panel covers but fails its depth test at, away from any outline
                extra["hidden"] = int((ok & (info["covers"] & ~info["passed"]).any(0)).sum())
                assert extra["hidden"] >= c["min_hidden"], (c["name"], eye, extra)
            if c.get("off_image"):
                box = [P.pixel_box(q["model"], vp, w, h) for q in ref_panels]
                assert box[0] is not None and box[0][0] == 0 and box[1] is None, box
                cc = P.corners_clip(ref_panels[0]["model"], vp)
                assert (cc[:, 0] / cc[:, 3]).min() < -1.2 and (P.corners_clip(ref_panels[1]["model"], vp)[:, 3] <= 1e-6).all()
            if c.get("wrap_band"):     # the panel's compared pixels whose bilinear taps wrap (within half a texel of an edge)
                th, tw = pics[0].shape[:2]
                rr = X.facet_table([P.panel_facet(ref_panels[0]["model"])], vp, w, h)[0]
                yc, xc = P._grid(w, h, np.float64)
                nw_ = rr[6] * xc + rr[7] * yc + rr[8]
                a, b = (rr[0] * xc + rr[1] * yc + rr[2]) / nw_, (rr[3] * xc + rr[4] * yc + rr[5]) / nw_
                band = (np.minimum(a, 1 - a) * tw < 0.5) | (np.minimum(b, 1 - b) * th < 0.5)
                extra["wrap_pixels"] = int((ok & info["passed"][0] & band).sum())
                assert extra["wrap_pixels"] >= 150, extra
            g64 = np.concatenate([final[..., :3].astype(np.float64), final[..., 3:].astype(np.float64) / 255.0], -1)
            gl_b = [float(np.abs(r64[..., :3] - g64[..., :3])[ok].max()), float(np.abs(r64[..., 3] - g64[..., 3])[ok].max() * 255.0)]
            f32_b = [float(np.abs(r32[..., :3].astype(np.float64) - r64[..., :3])[ok].max()), float(np.abs(r32[..., 3].astype(np.float64) - r64[..., 3])[ok].max())]
            outside = ~np.any([_in_box(P.pixel_box(q["model"], vp, w, h), w, h) for q in ref_panels], 0)
            assert (final[outside] == dst[outside]).all(), "the render changed a pixel outside every panel's box"
            print(f"{c['name']} eye {eye}: excluded {excluded:.3f} panel pixels {n_panel} | f64 vs GL {gl_b} | f32 vs f64 {f32_b} {extra}")
            data[f"{c['name']}_{eye}_dst"], data[f"{c['name']}_{eye}_delta"] = dst, (final.astype(np.int16) - dst.astype(np.int16)).astype(np.uint8)
            rec_case["eyes"].append(dict(eye=eye, size=[w, h], fov=[l, r, u, dn], position=pos, orientation=[0.0, 0.0, 0.0, 1.0], proj=proj.tolist(),
                                         view=view.tolist(), vp=vp.tolist(), excluded=excluded, panel_pixels=n_panel, gl=gl_b, f32=f32_b,
                                         boxes=[P.pixel_box(q["model"], vp, w, h) for q in ref_panels], **extra))
        for t in [tc, td] + gl_tex:
            gl.delete_texture(t)
        meta["cases"].append(rec_case)
    meta["gl_bound"] = max(max(e["gl"]) for c in meta["cases"] for e in c["eyes"])
    np.savez_compressed(os.path.join(HERE, "xr_panels.npz"), **data)
    with open(os.path.join(HERE, "xr_panels.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote xr_panels", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "xr_panels.npz")), "bytes; gl bound", meta["gl_bound"])


def _in_box(box, w, h):
    m = np.zeros((h, w), bool)
    if box is not None:
        m[box[1]:box[3], box[0]:box[2]] = True
    return m


if __name__ == "__main__":
    main()
