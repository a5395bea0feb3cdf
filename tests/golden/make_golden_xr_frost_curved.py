"""Golden vectors for the veil and frosted looks around the CURVED OpenXR screen (d2s_dibr_xr_eyes_frost_curved): the REFERENCE's one
TRIANGLES draw of 588 vertices after its curved strip per eye, off-screen on SwiftShader.

    python tests/golden/make_golden_xr_frost_curved.py        # -> tests/golden/xr_frost_curved.npz + xr_frost_curved.json

Method and texture state as make_golden_xr_frost.py; read from the reference's checkout with `ast` at generation time, none of its text
stored.  Beside that generator's list: EffectsMixin._build_curved_frost_verts, _render_curved_frost_with_uniforms (xr_viewer/effects.py),
ScreenMixin._screen_uv_to_world, _screen_curve_mode, _build_curved_screen_verts (xr_viewer/screen.py) and _FROST_CURVED_VERT
(xr_viewer/glsl.py), EXECUTED on a stub whose fake ctx, _curved_frost_vbo, programs and vaos record the vertices, every uniform, the
draw and the GL state -- asserted: one TRIANGLES draw of 588 vertices, depth test off, depth writes off, blend ONE /
ONE_MINUS_SRC_ALPHA, the other look's program untouched.  Draw sequence per eye into one RGBA32F target: clear (colour, depth 1); the
curved strip (depth test LESS, blending off); the recorded triangles with the recorded program, blended, depth test off.

Stored and compared pixels: those a triangle covers (the empty cases: would cover) whose float64 class (tests/xr_frost_curved_ref.py
render_eye: screen / each wall's hit count / for frosted the noise cells) is uniform on their 3 x 3 neighbourhood.  Asserted here, with
poses chosen so that the restatement alone meets them: excluded <= 15 % per eye; >= 500 compared wall pixels per case that draws;
min_two / min_over: compared pixels two walls cover / a wall covers over the screen; min_cut: pixels inside a triangle that the near
plane cuts; min_end: compared pixels an end wall covers.  The render cases use noise_scale 6, as the flat fixture does.
The bounds are measured: per case and eye gl = the float64 rasteriser of the RECORDED triangles against the render, f32 = the float32
emulation of the kernel's walk, started from the library's double-precision geometry, against that rasteriser, walk = the library's rows
walked in float64 against the recorded triangles (maximum |v_uv| and |t| difference over the pixels both cover).
"""
from __future__ import annotations

import ast
import ctypes as C
import json
import math
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
REF = "/root/reference/xr_viewer"

RGB_STEPS = 16.0
N_VERTS = 12 * 48 + 12
VEIL = dict(mode=1, head=[0.0, 0.0, 0.0], intensity=1.5, alpha=1.0, edge_inset=0.02, beam_softness=0.34, beam_thickness=3.0,
            lod=5.4, threshold=0.46, noise_scale=54.0, blend=1.35, diffuse=0.85, time=0.0)
FROSTED = dict(VEIL, mode=2, intensity=1.0, alpha=0.42, edge_inset=0.045, beam_thickness=1.6, noise_scale=6.0)
BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0, corner_radius=0.0, crop=[0.0, 0.0, 1.0, 1.0], clear=[0.0, 0.0, 0.0, 1.0],
            source=[96, 160], eye_sizes=[[130, 100], [130, 100]], eye_shift=[0.0, 0.0, 0.0], alpha_mode="rgba", dim=1.0)
SCREEN = dict(width=1.6, height=0.96, distance=1.4, pan_x=0.0, pan_y=0.0, yaw=0.0, pitch=0.0, roll=0.0, curve="horizontal", normal_offset=0.0)
VERT = dict(SCREEN, curve="vertical")
NEAR_H, NEAR_V = dict(SCREEN, distance=1.0), dict(VERT, distance=1.0)      # a nearer screen keeps the noise-cell seams (excluded pixels) short
CASES = [
    dict(BASE, name="veil_h_front", seed=101, screen=dict(SCREEN), frost=dict(VEIL), source=[512, 1024]),
    dict(BASE, name="veil_v_front", seed=102, screen=dict(VERT), frost=dict(VEIL)),
    # the head off-centre in both axes: the front rectangle splays
    dict(BASE, name="veil_h_oblique", seed=103, screen=dict(SCREEN, yaw=0.4, pitch=-0.15, roll=0.12, pan_x=0.2, pan_y=0.1),
         frost=dict(VEIL, head=[0.35, -0.25, 0.1]), eye_sizes=[[130, 100], [111, 87]]),
    dict(BASE, name="veil_v_crop_corner", seed=104, screen=dict(VERT, height=0.64), crop=[0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0], corner_radius=0.03,
         clear=[0.1, 0.2, 0.3, 1.0], frost=dict(VEIL), alpha_mode="premultiplied"),
    # the eyes about 1.1 m from the head the walls were laid out for, outside the tube beyond the arc's right end: they look through that
    # end's wall at the top wall and at the screen
    dict(BASE, name="veil_h_outside", seed=105, screen=dict(SCREEN), frost=dict(VEIL), eye_shift=[1.0, 0.3, 0.3], min_two=50, min_over=50),
    # the eyes 1.5 cm below the top long wall: the near plane (0.05 m) cuts it
    dict(BASE, name="veil_h_near", seed=106, screen=dict(SCREEN), frost=dict(VEIL), eye_shift=[0.0, 0.63, 0.3], min_cut=300),
    # the screen yawed and the eyes beyond the arc's right end: that end's wall crosses the image centre
    dict(BASE, name="veil_h_end", seed=107, screen=dict(SCREEN, yaw=0.5), frost=dict(VEIL), eye_shift=[0.9, 0.0, 0.2], min_end=200),
    dict(BASE, name="frosted_h_default", seed=108, screen=dict(NEAR_H), frost=dict(FROSTED), source=[512, 1024]),
    dict(BASE, name="frosted_v_time", seed=109, screen=dict(NEAR_V, pan_x=-0.1), frost=dict(FROSTED, time=3.7, head=[0.1, 0.05, 0.0]),
         source=[512, 1024]),
    dict(BASE, name="frosted_h_odd", seed=110, screen=dict(NEAR_H), source=[562, 1000], frost=dict(FROSTED)),
    dict(BASE, name="frosted_v_small_lod9", seed=111, screen=dict(NEAR_V, distance=0.9), frost=dict(FROSTED, lod=9.0)),      # clamps to q = 7
    # a source dimmed to a quarter: luma < threshold everywhere, the scatter's max takes luma * diffuse * 0.35
    dict(BASE, name="frosted_h_dark", seed=112, screen=dict(NEAR_H), frost=dict(FROSTED, intensity=4.0), dim=0.25, source=[512, 1024]),
    # the reference's early returns: nothing but the screen is drawn
    dict(BASE, name="frosted_v_empty", seed=113, screen=dict(VERT), frost=dict(FROSTED, intensity=0.0), empty=True),
    dict(BASE, name="veil_h_empty", seed=114, screen=dict(SCREEN), frost=dict(VEIL, alpha=0.002), empty=True),
]


def reference_curved_frost():
    """make(screen dict, frost dict, crop) -> the stub; its render(vp) runs the reference's _render_frost_veil or _render_frost_glow on
    a curved screen and returns None (an early return) or dict(verts [588, 8], uniforms, u_vp as uploaded, layout)."""
    from make_golden_xr_eye import _defs
    from make_golden_xr_glow import _Prog
    names = ("_frost_front_layout", "_build_curved_frost_verts", "_screen_effect_basis", "_mat4_uniform_bytes", "_set_frost_uniforms",
             "_set_frost_uniform_values", "_set_frost_veil_uniforms", "_render_curved_frost_with_uniforms", "_render_frost_veil",
             "_render_frost_glow")
    mgl = types.SimpleNamespace(DEPTH_TEST="DEPTH_TEST", BLEND="BLEND", ONE="ONE", ONE_MINUS_SRC_ALPHA="ONE_MINUS_SRC_ALPHA",
                                TRIANGLE_STRIP="TRIANGLE_STRIP", TRIANGLES="TRIANGLES")
    ns = {"np": np, "math": math, "moderngl": mgl, "time": types.SimpleNamespace(perf_counter=lambda: 0.0)}
    with open(os.path.join(REF, "constants.py")) as f:
        for n in ast.parse(f.read()).body:
            if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id in ("_CURVED_CURVATURE_SCALE", "_CURVED_HALF_ANGLE_RAD"):
                exec(compile(ast.Module(body=[n], type_ignores=[]), "constants.py", "exec"), ns)
    fns = {}
    fns.update(_defs(os.path.join(REF, "effects.py"), names, "EffectsMixin"))
    fns.update(_defs(os.path.join(REF, "screen.py"), ("_screen_uv_to_world", "_screen_curve_mode", "_build_curved_screen_verts"), "ScreenMixin"))
    fns.update(_defs(os.path.join(REF, "crop.py"), ("_set_source_crop_uniform",), "CropMixin"))
    exec(compile(ast.Module(body=list(fns.values()), type_ignores=[]), REF, "exec"), ns)
    Stub = type("Stub", (), {k: ns[k] for k in fns})

    def make(screen, frost, crop):
        s = Stub()
        s.screen_width, s.screen_height, s.screen_distance = screen["width"], screen["height"], screen["distance"]
        s.screen_pan_x, s.screen_pan_y = screen["pan_x"], screen["pan_y"]
        s.screen_yaw, s.screen_pitch, s.screen_roll = screen["yaw"], screen["pitch"], screen["roll"]
        s._screen_curved, s._screen_curve_axis, s._head_pos_w = True, screen["curve"], tuple(frost["head"])
        s._glow_intensity_multiplier = 1.0
        s._frost_veil_intensity = s._frost_glow_intensity = frost["intensity"]
        s._frost_veil_alpha = s._frost_glow_alpha = frost["alpha"]
        s._frost_glow_inset, s._frost_glow_lod, s._frost_glow_threshold = frost["edge_inset"], frost["lod"], frost["threshold"]
        s._frost_glow_noise_scale, s._frost_glow_blend, s._frost_glow_thickness = frost["noise_scale"], frost["blend"], frost["beam_thickness"]
        s._frost_glow_diffuse, s._frame_now = frost["diffuse"], frost["time"]
        s._movie_crop_render_uv_fast = lambda: tuple(crop)
        s._frost_source_texture = lambda: types.SimpleNamespace(use=lambda location=0: None)

        def render(vp):
            s.state, s.rec = [], dict(draws=[])
            s.ctx = types.SimpleNamespace(enable=lambda f: s.state.append(("enable", f)), disable=lambda f: s.state.append(("disable", f)),
                                          depth_mask=True, blend_func=None)
            s._curved_frost_verts_params = None
            for a in ("_frost_uniform_cache", "_frost_layout_cache_key", "_source_crop_uniform_cache"):
                if hasattr(s, a):
                    delattr(s, a)
            s._curved_frost_vbo = types.SimpleNamespace(write=lambda b: s.rec.__setitem__("verts", np.frombuffer(bytes(b), np.float32).reshape(-1, 8).copy()))
            vao = types.SimpleNamespace(render=lambda mode, vertices: s.rec["draws"].append((mode, int(vertices), s.ctx.blend_func, s.ctx.depth_mask,
                                                                                           tuple(s.state))))
            s._curved_frost_vao = s._curved_veil_vao = vao
            s._curved_frost_prog, s._curved_veil_prog = _Prog(), _Prog()
            (s._render_frost_veil if frost["mode"] == 1 else s._render_frost_glow)(None, vp)
            if not s.rec["draws"]:
                return None
            p = s._curved_veil_prog if frost["mode"] == 1 else s._curved_frost_prog
            other = s._curved_frost_prog if frost["mode"] == 1 else s._curved_veil_prog
            assert not other, "the other look's program was touched"
            assert len(s.rec["draws"]) == 1
            mode, n, blend, mask, state = s.rec["draws"][0]
            on = {}
            for what, flag in state:
                on[flag] = what == "enable"
            assert mode == "TRIANGLES" and n == N_VERTS and blend == ("ONE", "ONE_MINUS_SRC_ALPHA") and mask is False, (mode, n, blend, mask)
            assert on.get("DEPTH_TEST") is False and on.get("BLEND") is True, state
            assert s.ctx.depth_mask is True and s.state[-2:] == [("disable", "BLEND"), ("enable", "DEPTH_TEST")]
            assert s.rec["verts"].shape == (N_VERTS, 8)
            uni = {k: (list(v.value) if isinstance(v.value, tuple) else v.value) for k, v in p.items() if v.value is not None}
            _, _, fd, fhw, fhh = s._frost_front_layout()
            return dict(verts=s.rec["verts"], uniforms=uni, u_vp=np.frombuffer(p["u_vp"].bytes, np.float32).reshape(4, 4).copy(),
                        layout=[float(fd), float(fhw), float(fhh)])
        s.render = render
        return s
    return make


def draw_eye(gl, passes, w, h, clear):
    """make_golden_xr_glow.draw_eye for passes whose vertices carry any number of attributes: a pass has attribs = [(name | location,
    components)] over verts [n, sum of components] instead of ncomp."""
    from make_golden_xr_glow import _set_uniforms
    g = gl.gl
    g.glClearDepthf.argtypes = [C.c_float]
    g.glUniformMatrix4fv.argtypes = [C.c_int, C.c_int, C.c_ubyte, C.c_void_p]
    g.glGetAttribLocation.argtypes = [C.c_uint, C.c_char_p]
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
        (g.glEnable if p["blend"] else g.glDisable)(0x0BE2)
        if p["blend"]:
            g.glBlendFunc(1, 0x0303)                                                  # ONE, ONE_MINUS_SRC_ALPHA
        (g.glEnable if p["depth"] else g.glDisable)(0x0B71)
        g.glDepthMask(1 if p["depth"] else 0)
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
        stride = verts.shape[1] * 4
        vbo = C.c_uint()
        g.glGenBuffers(1, C.byref(vbo))
        g.glBindBuffer(0x8892, vbo)
        g.glBufferData(0x8892, verts.nbytes, verts.ctypes.data, 0x88E4)
        at, locs = 0, []
        for name, n in p["attribs"]:
            loc = g.glGetAttribLocation(p["prog"], name.encode())
            if loc >= 0:                                                              # (an attribute the program does not read has none)
                g.glEnableVertexAttribArray(loc)
                g.glVertexAttribPointer(loc, n, 0x1406, 0, stride, C.c_void_p(at * 4))
                locs.append(loc)
            at += n
        assert at == verts.shape[1]
        g.glDrawArrays(p["mode"], p["first"], p["count"])
        g.glFinish()
        for loc in locs:
            g.glDisableVertexAttribArray(loc)
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


def main(render=True):
    import xr_eye_ref as X
    import xr_frost_curved_ref as K
    import xr_frost_ref as F
    import xr_glow_ref as R
    from desktop2stereo_amd import xr
    from make_golden_xr_eye import FOV, _strings, reference_geometry
    from make_golden_xr_frost import clamp_texture, stats4
    _, fov_to_proj, pose_to_view = reference_geometry()
    make_frost = reference_curved_frost()
    data = {}
    meta = {"cases": [], "fov": FOV,
            "shader": "walls: xr_viewer/glsl.py _FROST_CURVED_VERT with _FROST_VEIL_FRAG / _FROST_GLOW_FRAG; screen: as tests/golden/xr_glow_curved.json",
            "textures": "as tests/golden/xr_frost.json",
            "encoding": "as tests/golden/xr_frost.json; <case>_verts = float32 [588, 8]: what _build_curved_frost_verts wrote, world x y z, v_uv, "
                        "v_local per vertex (the empty cases: the library's own, nothing was written); <case>_strip = float32 [98, 5]: the "
                        "screen's own TRIANGLE_STRIP as _build_curved_screen_verts wrote it, x y z u v",
            "bounds": "per case and eye, over the pixels whose float64 class is uniform on 3 x 3: gl = the float64 rasteriser of the recorded "
                      "triangles vs the render, f32 = the float32 emulation of the kernel's walk vs that rasteriser: [share of rgb values beyond "
                      "1 level, mean |rgb diff| in levels, max |alpha diff|, max |rgb diff|]; walk = [max |v_uv diff|, max |t diff|] of the "
                      "library's rows walked in float64 vs the recorded triangles; excluded = the share of pixels not compared; counts = "
                      "compared pixels [no wall, one wall, two or more walls, wall over screen]; end = compared pixels an end wall covers; cut "
                      "= pixels inside a triangle with clip w > 0 but beyond the near or far plane",
            "eyes": "eye i of a case looks from frost.head + eye_shift + (-+0.032, 0, 0) with identity orientation"}
    if render:
        import gl_harness as G
        from make_golden_xr_crop import xr_shader_patch
        from make_golden_xr_glow import mip_texture
        (_, _, _), (fs, l0, l1) = G.reference_shaders()
        patch, p0, p1 = xr_shader_patch()
        src = _strings(os.path.join(REF, "glsl.py"), ("_CURVED_VERT", "_FROST_CURVED_VERT", "_FROST_VEIL_FRAG", "_FROST_GLOW_FRAG"))
        fs2, defaults = G.to_es300(patch(fs))
        gl = G.Gles()
        meta["gl"] = {"version": gl.version, "renderer": gl.renderer}
        screen_prog = gl.program(G.to_es300(src["_CURVED_VERT"])[0], fs2)
        progs = {1: gl.program(G.to_es300(src["_FROST_CURVED_VERT"])[0], G.to_es300(src["_FROST_VEIL_FRAG"])[0]),
                 2: gl.program(G.to_es300(src["_FROST_CURVED_VERT"])[0], G.to_es300(src["_FROST_GLOW_FRAG"])[0])}
    for c in CASES:
        H, W = c["source"]
        img, dep = F.case_scene(c)
        levels = R.chain(img)
        sc, fr = c["screen"], c["frost"]
        stub = make_frost(sc, fr, c["crop"])
        strip = np.asarray(stub._build_curved_screen_verts(normal_offset=0.0), np.float32).reshape(-1, 5)
        facets = X.facets_strip(strip, sc["curve"] == "vertical")
        lib_screen = xr.XrScreen(**sc, clear=tuple(c["clear"]))
        lib_frost = xr.XrFrost(**dict(fr, mode={1: "veil", 2: "frosted"}[fr["mode"]], head=tuple(fr["head"])))
        crec = dict(c, strip=strip, eyes=[])                  # (the strip travels in the .npz: tests put it back into the case)
        data[f"{c['name']}_strip"] = strip
        if render:
            t_lin, t_dep = gl.texture(img, 0), gl.texture(dep, 1)
            t_src = clamp_texture(gl, img, 2) if fr["mode"] == 1 else mip_texture(gl, img, 2)
        n_wall = n_two = n_over = n_cut = n_end = 0
        for eye in (0, 1):
            ew, eh = c["eye_sizes"][eye]
            l, r, u, d = FOV[eye]
            fov = types.SimpleNamespace(angle_left=l, angle_right=r, angle_up=u, angle_down=d)
            pos = [fr["head"][k] + c["eye_shift"][k] + ((-0.032 if eye == 0 else 0.032) if k == 0 else 0.0) for k in range(3)]
            pose = types.SimpleNamespace(orientation=types.SimpleNamespace(x=0.0, y=0.0, z=0.0, w=1.0),
                                         position=types.SimpleNamespace(x=pos[0], y=pos[1], z=pos[2]))
            vp = fov_to_proj(fov) @ pose_to_view(pose)
            assert vp.dtype == np.float32 and X.min_clip_w(facets, vp) > 1e-6
            rec = stub.render(vp)
            assert (rec is None) == bool(c.get("empty")) == (not lib_frost.draws()), c["name"]
            if rec is not None and eye == 0:
                crec.update(layout=rec["layout"], frost_uniforms=rec["uniforms"])
                verts = rec["verts"]
            if rec is not None:
                assert np.array_equal(rec["verts"], verts) and np.array_equal(rec["u_vp"].T, vp)
            if rec is None and eye == 0:      # nothing drawn: the library's own numbers say where the walls WOULD lie (the stored pixels)
                crec.update(layout=list(lib_frost.layout(lib_screen)), frost_uniforms=None)
                verts = lib_frost.curved_wall_verts(lib_screen).astype(np.float32)
            data[f"{c['name']}_verts"] = verts
            e = dict(eye=eye, vp=vp.tolist(), size=[ew, eh], pos=pos)
            mh = K.mesh_hits(verts, vp, ew, eh)
            r64, cls, info = K.case_render(crec, e, img, dep, levels, verts, np.float64)
            r32, _, _ = K.case_render(crec, e, img, dep, levels, None, np.float32)
            ok = K.uniform3x3(cls)
            excluded = float(1.0 - ok.mean())
            assert excluded <= 0.15, (c["name"], eye, excluded)
            nw, cov, cnt = info["n_walls"], info["covered"], info["counts"]
            counts = [int(((nw == 0) & ok).sum()), int(((nw == 1) & ok).sum()), int(((nw >= 2) & ok).sum()), int(((nw >= 1) & cov & ok).sum())]
            end = int((((cnt[2] + cnt[3]) > 0) & ok).sum())
            stored = ok & (nw > 0)
            cut = int(sum(m["cut"] for m in mh))
            wh = K.walk_hits(K.lib_rows(sc, fr["head"], vp, ew, eh), ew, eh, np.float64)
            walk_uv = walk_t = 0.0
            for k in range(K.TRIS):
                both, ia, ib = np.intersect1d(mh[k]["idx"], wh[k]["idx"], return_indices=True)
                assert mh[k]["idx"].size + wh[k]["idx"].size - 2 * both.size <= 0.02 * max(mh[k]["idx"].size, 50), (c["name"], eye, k)
                if both.size:
                    walk_uv = max(walk_uv, float(np.abs(mh[k]["u"][ia] - wh[k]["u"][ib]).max()), float(np.abs(mh[k]["v"][ia] - wh[k]["v"][ib]).max()))
                    walk_t = max(walk_t, float(np.abs(mh[k]["t"][ia] - wh[k]["t"][ib]).max()))
            b32 = stats4(r32, r64, ok)
            e.update(excluded=excluded, counts=counts, end=end, cut=cut, f32=list(b32), walk=[walk_uv, walk_t])
            if render:
                uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(W), float(H)),
                           u_eye_offset=float((1.0 if eye else -1.0) * c["ipd_uv"] / 2.0), u_depth_strength=float(0.1 * c["depth_ratio"]),
                           u_convergence=float(c["convergence"]), u_roll=float(sc["roll"]), u_feather_enabled=0, u_feather_width=0.02,
                           u_viewport=(0.0, 0.0, float(ew), float(eh)), u_source_crop=tuple(float(v) for v in c["crop"]),
                           **{k: float(v) for k, v in defaults.items()})
                uni["u_corner_radius"] = float(c["corner_radius"])
                passes = [dict(prog=screen_prog, uniforms=uni, mats=dict(u_mvp=vp), textures={0: t_lin, 1: t_dep}, verts=strip,
                               attribs=[("in_position", 3), ("in_uv", 2)], mode=0x0005, first=0, count=strip.shape[0], blend=False, depth=True)]
                if rec is not None:
                    wuni = {k: (float(v) if isinstance(v, float) else v) for k, v in rec["uniforms"].items()}
                    wuni["u_source"] = 2
                    passes.append(dict(prog=progs[fr["mode"]], uniforms=wuni, mats=dict(u_vp=rec["u_vp"].T), textures={2: t_src}, verts=rec["verts"],
                                       attribs=[("in_position", 3), ("in_uv", 2), ("in_local", 3)], mode=0x0004, first=0, count=N_VERTS,
                                       blend=True, depth=False))
                out = draw_eye(gl, passes, ew, eh, c["clear"])
                assert np.isfinite(out).all()
                enc_rgb = np.rint(np.clip(out[..., :3], 0, 1) * (255.0 * RGB_STEPS)).astype(np.uint16) * stored[..., None]
                enc_a = np.rint(np.clip(out[..., 3], 0, 1) * 65535.0).astype(np.uint16) * stored
                golden = np.concatenate([enc_rgb / RGB_STEPS, enc_a[..., None] / 65535.0], -1)
                e["gl"] = list(stats4(r64, golden, stored)[:3]) if stored.any() else [0.0, 0.0, 0.0]
                e["stored"] = int(stored.sum())
                data[f"{c['name']}_{eye}_rgb"], data[f"{c['name']}_{eye}_a"] = (enc_rgb >> 4).astype(np.uint8), enc_a
                data[f"{c['name']}_{eye}_rgbf"] = (enc_rgb & 15).astype(np.uint8)
            print(f"{c['name']} eye {eye} {ew}x{eh}: counts {counts} end {end} cut {cut} excluded {excluded:.3f} | walk {walk_uv:.2e} {walk_t:.2e} "
                  f"| f32 vs f64 {['%.3g' % v for v in b32]} | f64 vs GL {['%.3g' % v for v in e.get('gl', [])]}", flush=True)
            n_wall += counts[1] + counts[2]
            n_two += counts[2]
            n_over += counts[3]
            n_cut += cut
            n_end += end
            crec["eyes"].append(e)
        if not c.get("empty"):
            assert n_wall >= 500, (c["name"], n_wall)
        assert n_two >= c.get("min_two", 0) and n_over >= c.get("min_over", 0) and n_cut >= c.get("min_cut", 0) and n_end >= c.get("min_end", 0), \
            (c["name"], n_two, n_over, n_cut, n_end)
        # the library's host side is the reference's: the layout and the vertices
        assert np.allclose(lib_frost.layout(lib_screen), crec["layout"], rtol=2e-6, atol=0), (lib_frost.layout(lib_screen), crec["layout"])
        assert np.allclose(lib_frost.curved_wall_verts(lib_screen), verts, rtol=2e-6, atol=2e-7)
        if render:
            for t in (t_lin, t_dep, t_src):
                gl.delete_texture(t)
        del crec["strip"]
        meta["cases"].append(crec)
    assert {c["screen"]["curve"] for c in CASES if c["frost"]["mode"] == 1 and not c.get("empty")} == {"horizontal", "vertical"}
    assert {c["screen"]["curve"] for c in CASES if c["frost"]["mode"] == 2 and not c.get("empty")} == {"horizontal", "vertical"}
    if not render:
        return meta
    np.savez_compressed(os.path.join(HERE, "xr_frost_curved.npz"), **data)
    text = json.dumps(meta, indent=1)
    text = re.sub(r"\[[^\[\]{}]*\]", lambda m: re.sub(r"\s+", " ", m.group(0)).replace("[ ", "[").replace(" ]", "]"), text)      # a flat list: one line
    assert json.loads(text) == json.loads(json.dumps(meta))
    with open(os.path.join(HERE, "xr_frost_curved.json"), "w") as f:
        f.write(text + "\n")
    print("wrote xr_frost_curved", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "xr_frost_curved.npz")), "bytes")


if __name__ == "__main__":
    main(render="--no-render" not in sys.argv)
