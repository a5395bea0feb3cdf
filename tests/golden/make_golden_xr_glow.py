"""Golden vectors for the colour mip chain (d2s_mip_chain) and the glow around the flat OpenXR screen (d2s_dibr_xr_eyes_glow): the
REFERENCE's glow passes drawn around its screen per eye, off-screen on SwiftShader, and glGenerateMipmap's levels read back.

    python tests/golden/make_golden_xr_glow.py        # -> tests/golden/xr_glow.npz + xr_glow_mips.npz + xr_glow.json

Everything of the reference is read from its checkout with `ast` at generation time and none of its text is stored:
  * _GLOW_VERT / _GLOW_FRAG (xr_viewer/glsl.py) through gl_harness.to_es300; the screen's shaders as make_golden_xr_eye.py takes them;
  * EffectsMixin._render_glow, _glow_range_m, _mat4_uniform_bytes (xr_viewer/effects.py) and CropMixin._set_source_crop_uniform
    (xr_viewer/crop.py), compiled on their own and EXECUTED on a stub object whose fake ctx, _glow_vbo, _glow_prog and _glow_vao record
    the band vertices, every uniform and the (vertices, first) of the draw.  The manifest holds those numbers: they are what the
    library's host side (xr.XrGlow.uniforms, xr.glow_range_m) is tested against.
Draw sequence per eye into one RGBA32F target, _render_eye's (effects.py:1050-1145): clear (colour, depth 1); the outer band (the
recorded 24 vertices from `first` = 0) blended ONE / ONE_MINUS_SRC_ALPHA with the depth test off; the screen as
make_golden_xr_eye.draw draws it (depth test LESS, blending off); mode 1: the inner band (first = 24), blended.

Textures.  The glow passes sample an RGB8 texture after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, CLAMP_TO_EDGE (the XR colour
texture's repeat_x = repeat_y = False, xr_viewer/frame.py:39-40).  The SCREEN pass samples a plain LINEAR copy of the same image: with
glow on the reference's screen pass would itself be trilinear where the screen is minified (frame.py:34, effects.py:601-608), a
filter that needs implicit derivatives, is driver-dependent and is out of the library's scope -- its screen pass stays GL_LINEAR.

Mip levels are read back per level through a framebuffer attached at that level: of a 1024 x 512 noise image every level, of a
1000 x 562 one levels >= 3 (to stay small).

Compared pixels: those whose float64 region class (none / outer band / screen / screen + inner band, tests/xr_glow_ref.py) is
uniform on their 3 x 3 neighbourhood; asserted: excluded <= 10 % per eye, >= 500 compared outer-band pixels per case, and per mode-1
case >= 50 compared inner-band pixels with glow > 0.05.  The bounds are measured: per case and eye the float32 restatement against
the float64 one and the float64 one against the render (share of rgb values beyond 1 level, mean, alpha maximum).
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

EYE_W, EYE_H = 130, 100
RGB_STEPS = 16.0      # the renders are stored to 1 / 16 level: every pixel of these images carries glow, and finer steps are incompressible
BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0, corner_radius=0.0, crop=[0.0, 0.0, 1.0, 1.0], clear=[0.0, 0.0, 0.0, 1.0],
            head=[0.0, 0.0, 0.0], inner_edge_fraction=0.075, mode=1, range_m=1.2, source=[512, 1024])
SCREEN = dict(width=1.6, height=0.96, distance=1.4, pan_x=0.0, pan_y=0.0, yaw=0.0, pitch=0.0, roll=0.0, curve="flat", normal_offset=0.0)
CASES = [
    # a 1024 x 512 source: levels 7 .. 10 are 8 x 4, 4 x 2, 2 x 1, 1 x 1; a range short enough that the fall-off, and with it LOD 7 .. 10, lies inside the image
    dict(BASE, name="glow_front", seed=61, screen=dict(SCREEN)),
    dict(BASE, name="glow2_front", seed=62, screen=dict(SCREEN), mode=2, range_m=2.4),
    # the glow quad (the screen + 12 m) passes behind the eye
    dict(BASE, name="glow_oblique", seed=63, screen=dict(SCREEN, yaw=0.5, pitch=-0.2, roll=0.15, pan_y=0.3, distance=1.2), range_m=None),
    dict(BASE, name="glow_crop_corner", seed=64, screen=dict(SCREEN, height=0.64), crop=[0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0], corner_radius=0.03,
         clear=[0.1, 0.2, 0.3, 1.0], source=[256, 512]),
    dict(BASE, name="glow_odd", seed=65, screen=dict(SCREEN, pan_x=0.1), source=[562, 1000]),
    dict(BASE, name="glow_small", seed=66, screen=dict(SCREEN), source=[96, 160]),                 # q = 7: every LOD clamps to the 1 x 1 level
    dict(BASE, name="glow_far", seed=67, screen=dict(SCREEN, distance=2.42), range_m=None),      # range_m None: _glow_range_m's
    # beyond the issue's seven: the plane's horizon inside the image (pixels whose plane point has clip w <= 0 draw nothing)
    dict(BASE, name="glow_horizon", seed=68, screen=dict(SCREEN, yaw=1.0, distance=1.7), range_m=None, min_behind=300),
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


def reference_glow():
    """make(screen dict, head, inner_edge_fraction, crop) -> the stub object; its render_glow(vp, inner_only, glow2) runs the
    reference's _render_glow and returns dict(verts [48, 4], uniforms, u_model [4,4] and u_vp [4,4] as uploaded (column-major bytes
    read back row-major = the transposes), vertices, first)."""
    from make_golden_xr_eye import _defs
    fns = {}
    fns.update(_defs(os.path.join(REF, "effects.py"), ("_render_glow", "_glow_range_m", "_mat4_uniform_bytes"), "EffectsMixin"))
    fns.update(_defs(os.path.join(REF, "crop.py"), ("_set_source_crop_uniform",), "CropMixin"))
    mgl = types.SimpleNamespace(DEPTH_TEST="DEPTH_TEST", BLEND="BLEND", ONE="ONE", ONE_MINUS_SRC_ALPHA="ONE_MINUS_SRC_ALPHA", TRIANGLES="TRIANGLES")
    ns = {"np": np, "math": math, "moderngl": mgl}
    exec(compile(ast.Module(body=list(fns.values()), type_ignores=[]), REF, "exec"), ns)
    Stub = type("Stub", (), {k: ns[k] for k in fns})

    def make(screen, head, inner_edge_fraction, crop):
        s = Stub()
        s.screen_width, s.screen_height, s.screen_distance = screen["width"], screen["height"], screen["distance"]
        s.screen_pan_x, s.screen_pan_y = screen["pan_x"], screen["pan_y"]
        s.screen_yaw, s.screen_pitch, s.screen_roll = screen["yaw"], screen["pitch"], screen["roll"]
        s._screen_curved, s._head_pos_w = False, tuple(head)
        s._glow_intensity, s._glow_intensity_multiplier, s._glow_inner_edge_fraction = 1.0, 1.0, inner_edge_fraction
        s._glow_color = s._glow_target_color = (1.0, 1.0, 1.0)
        s._advance_glow_color = lambda: None
        s._movie_crop_render_uv_fast = lambda: tuple(crop)
        s._frost_source_texture = lambda: types.SimpleNamespace(use=lambda location=0: None)
        s.state = []
        s.ctx = types.SimpleNamespace(enable=lambda f: s.state.append(("enable", f)), disable=lambda f: s.state.append(("disable", f)),
                                      depth_mask=True, blend_func=None)
        s.rec = {}
        s._glow_vbo = types.SimpleNamespace(write=lambda b: s.rec.__setitem__("verts", np.frombuffer(bytes(b), np.float32).reshape(-1, 4).copy()))
        s._glow_vao = types.SimpleNamespace(render=lambda mode, vertices, first: s.rec.update(mode=mode, vertices=int(vertices), first=int(first)))

        def render_glow(vp, inner_only, glow2, range_override=None):
            s._glow_band_params, s._glow_model_params, s._glow_prog = None, None, _Prog()
            if range_override is not None:
                s._glow_range_m = lambda: range_override
            s._render_glow(None, vp, inner_only=inner_only, glow2=glow2)
            assert s.ctx.blend_func == ("ONE", "ONE_MINUS_SRC_ALPHA") and ("disable", "DEPTH_TEST") in s.state and s.rec["mode"] == "TRIANGLES"
            p = s._glow_prog
            uni = {k: (list(v.value) if isinstance(v.value, tuple) else v.value) for k, v in p.items() if v.value is not None}
            mats = {k: np.frombuffer(p[k].bytes, np.float32).reshape(4, 4).copy() for k in ("u_model", "u_vp")}
            return dict(verts=s.rec["verts"], uniforms=uni, vertices=s.rec["vertices"], first=s.rec["first"], **mats)
        s.render_glow = render_glow
        return s
    return make, Stub


def _set_uniforms(g, prog, uniforms):
    for name, val in uniforms.items():
        loc = g.glGetUniformLocation(prog, name.encode())
        if loc < 0:
            continue
        if isinstance(val, int):
            g.glUniform1i(loc, val)
        elif isinstance(val, float):
            g.glUniform1f(loc, val)
        elif len(val) == 2:
            g.glUniform2f(loc, *[float(v) for v in val])
        elif len(val) == 3:
            g.glUniform3f(loc, *[float(v) for v in val])
        else:
            g.glUniform4f(loc, *[float(v) for v in val])


def draw_eye(gl, passes, w, h, clear):
    """One RGBA32F colour + 24-bit depth target cleared to `clear` / 1.0, then every pass in order -> float32 [h,w,4], row 0 = top.
    A pass: dict(prog, uniforms, mats {name: float32 [4,4] in numpy convention, uploaded transposed}, textures {unit: id}, verts
    [n, ncomp + 2], ncomp, mode (GL enum), first, count, blend, depth)."""
    g = gl.gl
    g.glClearDepthf.argtypes = [C.c_float]
    g.glUniformMatrix4fv.argtypes = [C.c_int, C.c_int, C.c_ubyte, C.c_void_p]
    g.glUniform3f.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float]
    fbo, tex, rbo = C.c_uint(), C.c_uint(), C.c_uint()
    g.glGenTextures(1, C.byref(tex))
    g.glActiveTexture(0x84C0 + 7)
    g.glBindTexture(0x0DE1, tex)
    g.glTexImage2D(0x0DE1, 0, 0x8814, w, h, 0, 0x1908, 0x1406, None)                  # RGBA32F
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
    for p in passes:
        if p["blend"]:
            g.glEnable(0x0BE2)
            g.glBlendFunc(1, 0x0303)                                                  # ONE, ONE_MINUS_SRC_ALPHA (effects.py:538)
        else:
            g.glDisable(0x0BE2)
        if p["depth"]:
            g.glEnable(0x0B71)
            g.glDepthMask(1)
        else:
            g.glDisable(0x0B71)
            g.glDepthMask(0)
        for unit, t in p["textures"].items():
            g.glActiveTexture(0x84C0 + unit)
            g.glBindTexture(0x0DE1, t)
        g.glUseProgram(p["prog"])
        _set_uniforms(g, p["prog"], p["uniforms"])
        for name, m in p["mats"].items():
            loc = g.glGetUniformLocation(p["prog"], name.encode())
            assert loc >= 0, name
            mt = np.ascontiguousarray(np.asarray(m, np.float32).T)
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
        g.glDrawArrays(p["mode"], p["first"], p["count"])
        g.glFinish()
        g.glDeleteBuffers(1, C.byref(vbo))
    out = np.empty((h, w, 4), np.float32)
    g.glPixelStorei(0x0D05, 1)
    g.glReadPixels(0, 0, w, h, 0x1908, 0x1406, out.ctypes.data)
    gl._check("draw_eye")
    g.glDisable(0x0B71)
    g.glDisable(0x0BE2)
    g.glDepthMask(1)
    g.glBindFramebuffer(0x8D40, 0)
    g.glDeleteFramebuffers(1, C.byref(fbo))
    g.glDeleteRenderbuffers(1, C.byref(rbo))
    g.glDeleteTextures(1, C.byref(tex))
    return out[::-1].copy()


def mip_texture(gl, img, unit=0):
    """uint8 [H,W,3] -> an RGB8 texture after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, CLAMP_TO_EDGE."""
    g = gl.gl
    t = gl.texture(img, unit)
    g.glGenerateMipmap(0x0DE1)
    for k, v in ((0x2801, 0x2703), (0x2800, 0x2601), (0x2802, 0x812F), (0x2803, 0x812F)):
        g.glTexParameteri(0x0DE1, k, v)
    gl._check("mip_texture")
    return t


def read_levels(gl, t, H, W):
    """Every level of texture t, read through a framebuffer attached at that level -> [uint8 [h, w, 3]] for levels 0 .. q (row 0 =
    the texture's v = 0 row = the image's top row: no flip)."""
    import xr_glow_ref as R
    g = gl.gl
    out = []
    for k, (h, w) in enumerate(R.level_sizes(H, W)):
        fbo = C.c_uint()
        g.glGenFramebuffers(1, C.byref(fbo))
        g.glBindFramebuffer(0x8D40, fbo)
        g.glFramebufferTexture2D(0x8D40, 0x8CE0, 0x0DE1, t, k)
        if g.glCheckFramebufferStatus(0x8D40) != 0x8CD5:
            raise RuntimeError(f"level {k}: framebuffer incomplete")
        buf = np.empty((h, w, 4), np.uint8)
        g.glPixelStorei(0x0D05, 1)
        g.glReadPixels(0, 0, w, h, 0x1908, 0x1401, buf.ctypes.data)
        gl._check(f"read level {k}")
        g.glBindFramebuffer(0x8D40, 0)
        g.glDeleteFramebuffers(1, C.byref(fbo))
        out.append(buf[..., :3].copy())
    return out


def stats(a, b, ok):
    from make_golden_xr_eye import stats as s
    return s(a, b, ok)


def main():
    import gl_harness as G
    import xr_eye_ref as X
    import xr_glow_ref as R
    from desktop2stereo_amd import synth, xr
    from make_golden_xr_crop import xr_shader_patch
    from make_golden_xr_eye import FOV, _strings, reference_geometry
    make_screen, fov_to_proj, pose_to_view = reference_geometry()
    make_glow, _ = reference_glow()
    (_, _, _), (fs, l0, l1) = G.reference_shaders()
    patch, p0, p1 = xr_shader_patch()
    src = _strings(os.path.join(REF, "glsl.py"), ("_WORLD_VERT", "_GLOW_VERT", "_GLOW_FRAG"))
    fs2, defaults = G.to_es300(patch(fs))
    gl = G.Gles()
    screen_prog = gl.program(G.to_es300(src["_WORLD_VERT"])[0], fs2)
    glow_prog = gl.program(G.to_es300(src["_GLOW_VERT"])[0], G.to_es300(src["_GLOW_FRAG"])[0])
    data, mips = {}, {}
    meta = {"cases": [], "gl": {"version": gl.version, "renderer": gl.renderer}, "eye": [EYE_H, EYE_W], "fov": FOV,
            "shader": f"glow: xr_viewer/glsl.py _GLOW_VERT / _GLOW_FRAG; screen: viewer.py:{l0}-{l1} through xr_viewer/implementation.py:{p0}-{p1} "
                      "behind _WORLD_VERT; ES 3.00 patches: see gl_harness.py",
            "textures": "glow passes: RGB8 after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, CLAMP_TO_EDGE.  Screen pass: a LINEAR / "
                        "REPEAT copy of the same image WITHOUT mipmaps -- the reference's own screen pass is trilinear with glow on "
                        "(frame.py:34, effects.py:601-608); that filter is out of the library's scope (implicit derivatives, driver-dependent)",
            "encoding": "xr_glow.npz: <case>_<eye>_rgb = uint16 rint(clip(rgb, 0, 1) * 255 * 16); <case>_<eye>_a = uint16 rint(alpha * 65535).  xr_glow_mips.npz: mip_<name>_<k> = level k, uint8 [h, w, 3]",
            "bounds": "per case and eye, over the pixels whose float64 region class is uniform on 3 x 3: [share of rgb values beyond 1 level, "
                      "mean |rgb diff| in levels, max |alpha diff|] of f32 = float32 vs float64 restatement and gl = float64 restatement vs "
                      "the render; excluded = the share of pixels not compared; classes = compared pixels per region class (none, outer, "
                      "screen, screen + inner)"}
    # ---- glGenerateMipmap's levels ----
    meta["mips"] = []
    for name, (H, W), first in (("1024x512", (512, 1024), 1), ("1000x562", (562, 1000), 3)):
        img = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
        t = mip_texture(gl, img)
        got = read_levels(gl, t, H, W)
        gl.delete_texture(t)
        assert np.array_equal(got[0], img)
        want64 = R.chain(img, np.float64)
        rec = dict(name=name, seed=7, size=[H, W], first_level=first, levels=[], rule="rng = numpy default_rng(seed).integers(0, 256, (H, W, 3), uint8)")
        # each level is checked as ONE step from the render's own level above it, so a difference does not carry down the chain
        for k in range(1, len(got)):
            step64, step32 = R.next_level(got[k - 1], np.float64), R.next_level(got[k - 1], np.float32)
            d = np.abs(step64.astype(int) - got[k].astype(int))
            d32 = np.abs(step32.astype(int) - step64.astype(int))
            rec["levels"].append(dict(level=k, size=list(got[k].shape[:2]), differ=float((d > 0).mean()), max=int(d.max()),
                                      f32_differ=float((d32 > 0).mean()), f32_max=int(d32.max()),
                                      chain_differ=float((want64[k] != got[k]).mean())))
            print(f"mip {name} level {k} {got[k].shape[:2]}: one step from the render's level {k - 1} differs in {(d > 0).mean():.4%} (max {d.max()}); "
                  f"f32 vs f64 step {(d32 > 0).mean():.4%}; whole chain {(want64[k] != got[k]).mean():.4%}")
            if k >= first:
                mips[f"mip_{name}_{k}"] = got[k]
        if first > 1:
            mips[f"mip_{name}_{first - 1}"] = got[first - 1]                       # the level the first stored step starts from
        meta["mips"].append(rec)
    # ---- the eyes ----
    for c in CASES:
        H, W = c["source"]
        img, dep = synth.dibr_scene(H, W, c["seed"], "boxes")
        t_lin, t_dep = gl.texture(img, 0), gl.texture(dep, 1)
        t_mip = mip_texture(gl, img, 2)
        levels = R.chain(img)                                                      # the restated chain, as the tests have it; the render samples its own
        gl_levels = read_levels(gl, t_mip, H, W)
        sc = c["screen"]
        s = make_screen(**sc)
        model = np.asarray(s._build_model_mat4(normal_offset=0.0), np.float32)
        facets = X.facets_flat(model)
        stub = make_glow(sc, c["head"], c["inner_edge_fraction"], c["crop"])
        ref_range = float(stub._glow_range_m())
        lib_range = xr.glow_range_m(xr.XrScreen(**sc), c["head"])
        assert abs(ref_range - lib_range) <= 1e-12 * ref_range, (ref_range, lib_range)
        range_m = ref_range if c["range_m"] is None else float(c["range_m"])
        rec = dict(c, range_m=range_m, glow_range_m=ref_range, model=model.tolist(), eyes=[], chain_is_restated=bool(
            all(np.array_equal(a, b) for a, b in zip(levels, gl_levels))))
        n_outer = n_inner = 0
        for eye in (0, 1):
            l, r, u, d = FOV[eye]
            fov = types.SimpleNamespace(angle_left=l, angle_right=r, angle_up=u, angle_down=d)
            pos = [c["head"][0] + (-0.032 if eye == 0 else 0.032), c["head"][1], c["head"][2]]
            pose = types.SimpleNamespace(orientation=types.SimpleNamespace(x=0.0, y=0.0, z=0.0, w=1.0),
                                         position=types.SimpleNamespace(x=pos[0], y=pos[1], z=pos[2]))
            proj, view = fov_to_proj(fov), pose_to_view(pose)
            vp = proj @ view
            assert vp.dtype == np.float32 and X.min_clip_w(facets, vp) > 1e-6
            glow2 = c["mode"] == 2
            outer = stub.render_glow(vp, False, glow2, range_m)
            inner = stub.render_glow(vp, True, glow2, range_m)
            assert (outer["vertices"], outer["first"], inner["vertices"], inner["first"]) == (24, 0, 24, 24)
            assert np.array_equal(outer["verts"], inner["verts"])

            def glow_pass(g, inner_only):
                uni = {k: (float(v) if isinstance(v, float) else v) for k, v in g["uniforms"].items()}
                uni["u_source"] = 2
                return dict(prog=glow_prog, uniforms=uni, mats=dict(u_model=g["u_model"].T, u_vp=g["u_vp"].T), textures={2: t_mip},
                            verts=g["verts"], ncomp=2, mode=0x0004, first=g["first"], count=g["vertices"], blend=True, depth=False)
            uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(W), float(H)),
                       u_eye_offset=float((1.0 if eye else -1.0) * c["ipd_uv"] / 2.0), u_depth_strength=float(0.1 * c["depth_ratio"]),
                       u_convergence=float(c["convergence"]), u_roll=float(sc["roll"]), u_feather_enabled=0, u_feather_width=0.02,
                       u_viewport=(0.0, 0.0, float(EYE_W), float(EYE_H)), u_source_crop=tuple(float(v) for v in c["crop"]),
                       **{k: float(v) for k, v in defaults.items()})
            uni["u_corner_radius"] = float(c["corner_radius"])
            quad = np.array([[-1, -1, 0, 0], [1, -1, 1, 0], [-1, 1, 0, 1], [1, 1, 1, 1]], np.float32)
            passes = [glow_pass(outer, False),
                      dict(prog=screen_prog, uniforms=uni, mats=dict(u_mvp=vp @ model), textures={0: t_lin, 1: t_dep}, verts=quad, ncomp=2,
                           mode=0x0005, first=0, count=4, blend=False, depth=True)]
            if c["mode"] == 1:                                                      # effects.py:1137-1145: glow only, after the screen
                passes.append(glow_pass(inner, True))
            out = draw_eye(gl, passes, EYE_W, EYE_H, c["clear"])
            assert np.isfinite(out).all()
            enc_rgb = np.rint(np.clip(out[..., :3], 0, 1) * (255.0 * RGB_STEPS)).astype(np.uint16)
            enc_a = np.rint(np.clip(out[..., 3], 0, 1) * 65535.0).astype(np.uint16)
            golden = np.concatenate([enc_rgb / RGB_STEPS, enc_a[..., None] / 65535.0], -1)      # (as the tests decode it: the bounds below are taken on this)
            crec = dict(c, model=model.tolist(), range_m=range_m)
            e = dict(eye=eye, vp=vp.tolist())
            r64, cls = R.case_render(crec, e, img, dep, levels, EYE_W, EYE_H, np.float64)
            r32, _ = R.case_render(crec, e, img, dep, levels, EYE_W, EYE_H, np.float32)
            ok = R.uniform3x3(cls)
            excluded = float(1.0 - ok.mean())
            assert excluded <= 0.10, (c["name"], eye, excluded)
            classes = [int(((cls == k) & ok).sum()) for k in range(4)]
            n_outer += classes[R.OUTER]
            inner_glow = 0
            if c["mode"] == 1:                                                      # the inner band's own glow at the compared pixels it drew
                U = R.uniforms(sc["width"], sc["height"], 1, range_m, c["inner_edge_fraction"])
                plane, a, b = R.plane_coords(X.facet_table(facets, vp, EYE_W, EYE_H), EYE_W, EYE_H, np.float64)
                m = (cls == R.SCREEN_INNER) & ok
                _, srcg = R.glow_frag(levels, a[m], b[m], U, c["crop"], True, np.float64)
                inner_glow = int((srcg[:, 3] > 0.05).sum())
                n_inner += inner_glow
            extra = {}
            if "min_behind" in c:
                tab = X.facet_table(facets, vp, EYE_W, EYE_H)[0]
                yc, xc = np.meshgrid(np.arange(EYE_H) + 0.5 - EYE_H / 2, np.arange(EYE_W) + 0.5 - EYE_W / 2, indexing="ij")
                extra["behind_pixels"] = int(((tab[6] * xc + tab[7] * yc + tab[8] <= 0) & ok).sum())
            b32, bgl = stats(r32, r64, ok), stats(r64, golden, ok)
            print(f"{c['name']} eye {eye}: classes {classes} excluded {excluded:.3f} inner glow > 0.05: {inner_glow} | f32 vs f64 {b32} | f64 vs GL {bgl} {extra}")
            data[f"{c['name']}_{eye}_rgb"], data[f"{c['name']}_{eye}_a"] = enc_rgb, enc_a
            rec["eyes"].append(dict(eye=eye, vp=vp.tolist(), excluded=excluded, classes=classes, inner_glow_pixels=inner_glow, f32=list(b32),
                                    gl=list(bgl), **extra))
            if eye == 0:                                                            # what _render_glow handed GL (the same for both eyes but u_vp)
                rec["glow_uniforms"] = {k: v for k, v in outer["uniforms"].items()}
                rec["glow_model"] = outer["u_model"].T.tolist()
                rec["band_verts"] = outer["verts"].tolist()
                rec["draw"] = dict(outer=[outer["vertices"], outer["first"]], inner=[inner["vertices"], inner["first"]])
        assert n_outer >= 500, (c["name"], n_outer)
        if c["mode"] == 1:
            assert n_inner >= 50, (c["name"], n_inner)
        if "min_behind" in c:
            assert sum(e["behind_pixels"] for e in rec["eyes"]) >= c["min_behind"], c["name"]
        for t in (t_lin, t_dep, t_mip):
            gl.delete_texture(t)
        meta["cases"].append(rec)
    np.savez_compressed(os.path.join(HERE, "xr_glow.npz"), **data)
    np.savez_compressed(os.path.join(HERE, "xr_glow_mips.npz"), **mips)
    with open(os.path.join(HERE, "xr_glow.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote xr_glow", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "xr_glow.npz")), "bytes")


if __name__ == "__main__":
    main()
