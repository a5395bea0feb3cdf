"""Golden vectors for the veil and frosted looks around the flat OpenXR screen (d2s_dibr_xr_eyes_frost): the REFERENCE's four "beam"
walls drawn after its screen per eye, off-screen on SwiftShader.

    python tests/golden/make_golden_xr_frost.py        # -> tests/golden/xr_frost.npz + xr_frost.json

Everything of the reference is read from its checkout with `ast` at generation time and none of its text is stored:
  * _FROST_GLOW_VERT, _FROST_VEIL_FRAG, _FROST_GLOW_FRAG (xr_viewer/glsl.py) through gl_harness.to_es300; the screen's shaders as
    make_golden_xr_eye.py takes them;
  * EffectsMixin._frost_front_layout, _build_flat_frost_verts, _screen_effect_basis, _screen_effect_model, _frost_model_bytes,
    _write_frost_model_uniform, _mat4_uniform_bytes, _set_frost_uniforms, _set_frost_uniform_values, _set_frost_veil_uniforms,
    _render_flat_frost_with_uniforms, _render_frost_veil, _render_frost_glow (xr_viewer/effects.py) and
    CropMixin._set_source_crop_uniform (xr_viewer/crop.py), compiled on their own and EXECUTED on a stub object whose fake ctx,
    _frost_glow_vbo, programs and vaos record the vertices, every uniform, the four (vertices, first) draws and the GL state --
    asserted: depth test off, blend ONE / ONE_MINUS_SRC_ALPHA, TRIANGLE_STRIP, four draws of 158 vertices at 0, 158, 316, 474.
Draw sequence per eye into one RGBA32F target, _render_eye's (effects.py:1023-1145): clear (colour, depth 1); the screen as
make_golden_xr_eye.draw draws it (depth test LESS, blending off); the four recorded strips with the recorded program, blended, depth
test off.  Frosted samples an RGB8 texture after glGenerateMipmap (LINEAR_MIPMAP_LINEAR / LINEAR, CLAMP_TO_EDGE); the veil, whose
_frost_veil_lod is 0, a plain LINEAR / CLAMP_TO_EDGE copy without mipmaps (effects.py:590-608); the screen the LINEAR copy the other
eye-view fixtures give it.

Stored and compared pixels: those a wall's geometry covers (the empty cases: would cover) whose float64 class
(tests/xr_frost_ref.py render_eye: screen / the walls whose geometry covers the pixel / for frosted the noise cells) is uniform on
their 3 x 3 neighbourhood; what no wall covers is a plain d2s_dibr_xr_eyes pixel, which tests/golden/xr_eye.npz pins.  The renders
are stored as two uint8 planes, whole levels and sixteenths.  Asserted here, with inputs chosen so that the restatement alone
meets them: excluded <= 15 % per eye; >= 500 compared wall pixels per case that draws; veil_outside: >= 50 compared two-wall pixels
and >= 50 wall-over-screen pixels; veil_near: >= 300 pixels whose wall hit the near plane cuts.  The render cases use noise_scale 6:
the reference's 54 gives cells about 1.5 pixels wide at this eye size and the class rule would exclude nearly everything.
The bounds are measured: per case and eye gl = the float64 restatement over the RECORDED triangles against the render, f32 = the
float32 emulation of the kernel's walk against that restatement (share of rgb values beyond 1 level, mean, alpha maximum; for f32
also the rgb maximum), and walk = the kernel's walk in float64 against the recorded triangles (maximum |v_uv| and |t| difference).
analytic_s: how far the analytic px = a / g(t) lies from the mesh's piecewise-linear v_uv, maximum over the wall pixels.
"""
from __future__ import annotations

import ast
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

RGB_STEPS = 16.0
STRIDE = 158
VEIL = dict(mode=1, head=[0.0, 0.0, 0.0], intensity=1.5, alpha=1.0, edge_inset=0.02, beam_softness=0.34, beam_thickness=3.0,
            lod=5.4, threshold=0.46, noise_scale=54.0, blend=1.35, diffuse=0.85, time=0.0)
FROSTED = dict(VEIL, mode=2, intensity=1.0, alpha=0.42, edge_inset=0.045, beam_thickness=1.6, noise_scale=6.0)
BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0, corner_radius=0.0, crop=[0.0, 0.0, 1.0, 1.0], clear=[0.0, 0.0, 0.0, 1.0],
            source=[512, 1024], eye_sizes=[[130, 100], [130, 100]], eye_shift=[0.0, 0.0, 0.0], alpha_mode="rgba", dim=1.0)
SCREEN = dict(width=1.6, height=0.96, distance=1.4, pan_x=0.0, pan_y=0.0, yaw=0.0, pitch=0.0, roll=0.0, curve="flat", normal_offset=0.0)
NEAR = dict(SCREEN, distance=1.15)      # the frosted cases: a nearer screen keeps the walls' noise-cell seams (excluded pixels) short
# (veil_front has the 1024 x 512 source, minified on the walls; the other veils a 160 x 96 one, magnified: a LOD-0 tap of a minified
#  frame is noise along the wall, which no compressor shrinks, and the fixture has a size to keep)
CASES = [
    dict(BASE, name="veil_front", seed=81, screen=dict(SCREEN), frost=dict(VEIL)),
    # the head off-centre in both axes: fx != 1 != fy, the walls splay
    dict(BASE, name="veil_oblique", seed=82, screen=dict(SCREEN, yaw=0.4, pitch=-0.15, roll=0.12, pan_x=0.2, pan_y=0.1),
         frost=dict(VEIL, head=[0.35, -0.25, 0.1]), eye_sizes=[[130, 100], [111, 87]], source=[96, 160]),
    dict(BASE, name="veil_crop_corner", seed=83, screen=dict(SCREEN, height=0.64), crop=[0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0], corner_radius=0.03,
         clear=[0.1, 0.2, 0.3, 1.0], source=[96, 160], frost=dict(VEIL), alpha_mode="premultiplied"),
    # the eyes 1.09 m from the head the walls were laid out for, outside the tube beyond its right wall: they look through that wall
    # at the top wall and at the screen
    dict(BASE, name="veil_outside", seed=84, screen=dict(SCREEN), frost=dict(VEIL), eye_shift=[1.0, 0.3, 0.3], min_two=50, min_over=50,
         source=[96, 160]),
    # the right eye 1.3 cm inside the right wall: the near plane (0.05 m) cuts that wall 0.25 rad from the image centre
    dict(BASE, name="veil_near", seed=85, screen=dict(SCREEN), frost=dict(VEIL), eye_shift=[0.755, 0.0, 0.3], min_cut=300, source=[96, 160]),
    dict(BASE, name="frosted_default", seed=86, screen=dict(NEAR), frost=dict(FROSTED)),
    dict(BASE, name="frosted_time", seed=87, screen=dict(NEAR, pan_x=-0.1), frost=dict(FROSTED, time=3.7, head=[0.1, 0.05, 0.0])),
    dict(BASE, name="frosted_odd", seed=88, screen=dict(NEAR), source=[562, 1000], frost=dict(FROSTED)),
    dict(BASE, name="frosted_small", seed=89, screen=dict(NEAR), source=[96, 160], frost=dict(FROSTED)),      # levels 5, 6: 5 x 3, 2 x 1
    dict(BASE, name="frosted_lod_low", seed=90, screen=dict(NEAR), source=[96, 160], frost=dict(FROSTED, lod=0.5)),      # level 0 is the frame
    dict(BASE, name="frosted_lod_high", seed=91, screen=dict(NEAR), source=[96, 160], frost=dict(FROSTED, lod=9.0)),     # clamps to q = 7
    # a source dimmed to a quarter: luma < threshold everywhere, bright = 0, the scatter's max takes luma * diffuse * 0.35
    dict(BASE, name="frosted_dark", seed=92, screen=dict(NEAR), frost=dict(FROSTED, intensity=4.0), dim=0.25),
    # the reference's early returns: nothing but the screen is drawn
    dict(BASE, name="frosted_empty", seed=93, screen=dict(SCREEN), frost=dict(FROSTED, intensity=0.0), empty=True),
    dict(BASE, name="veil_empty", seed=94, screen=dict(SCREEN), frost=dict(VEIL, alpha=0.002), empty=True),
]


def reference_frost():
    """make(screen dict, frost dict, crop) -> the stub object; its render(vp) runs the reference's _render_frost_veil or
    _render_frost_glow and returns None (an early return: nothing drawn) or dict(verts [632, 5], uniforms, u_model, u_vp as uploaded
    (column-major bytes read back row-major = the transposes), draws [(vertices, first)], layout (front_depth, half_w, half_h))."""
    from make_golden_xr_eye import _defs
    from make_golden_xr_glow import _Prog
    names = ("_frost_front_layout", "_build_flat_frost_verts", "_screen_effect_basis", "_screen_effect_model", "_frost_model_bytes",
             "_write_frost_model_uniform", "_mat4_uniform_bytes", "_set_frost_uniforms", "_set_frost_uniform_values", "_set_frost_veil_uniforms",
             "_render_flat_frost_with_uniforms", "_render_frost_veil", "_render_frost_glow")
    fns = {}
    fns.update(_defs(os.path.join(REF, "effects.py"), names, "EffectsMixin"))
    fns.update(_defs(os.path.join(REF, "crop.py"), ("_set_source_crop_uniform",), "CropMixin"))
    mgl = types.SimpleNamespace(DEPTH_TEST="DEPTH_TEST", BLEND="BLEND", ONE="ONE", ONE_MINUS_SRC_ALPHA="ONE_MINUS_SRC_ALPHA",
                                TRIANGLE_STRIP="TRIANGLE_STRIP", TRIANGLES="TRIANGLES")
    clock = types.SimpleNamespace(perf_counter=lambda: 0.0)      # (_frame_now 0.0 falls through to the clock: time 0 stays 0)
    ns = {"np": np, "math": math, "moderngl": mgl, "time": clock}
    exec(compile(ast.Module(body=list(fns.values()), type_ignores=[]), REF, "exec"), ns)
    Stub = type("Stub", (), dict({k: ns[k] for k in fns}, _FLAT_FROST_STRIDE=STRIDE))

    def make(screen, frost, crop):
        s = Stub()
        s.screen_width, s.screen_height, s.screen_distance = screen["width"], screen["height"], screen["distance"]
        s.screen_pan_x, s.screen_pan_y = screen["pan_x"], screen["pan_y"]
        s.screen_yaw, s.screen_pitch, s.screen_roll = screen["yaw"], screen["pitch"], screen["roll"]
        s._screen_curved, s._head_pos_w = False, tuple(frost["head"])
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
            s._frost_glow_verts_params = None
            for a in ("_frost_uniform_cache", "_frost_model_uniform_cache", "_frost_model_cache_key", "_frost_layout_cache_key", "_source_crop_uniform_cache"):
                if hasattr(s, a):
                    delattr(s, a)
            s._frost_glow_vbo = types.SimpleNamespace(write=lambda b: s.rec.__setitem__("verts", np.frombuffer(bytes(b), np.float32).reshape(-1, 5).copy()))
            vao = types.SimpleNamespace(render=lambda mode, vertices, first: s.rec["draws"].append((mode, int(vertices), int(first), s.ctx.blend_func,
                                                                                                  s.ctx.depth_mask, tuple(s.state))))
            s._frost_glow_vao = s._frost_veil_vao = vao
            s._frost_glow_prog, s._frost_veil_prog = _Prog(), _Prog()
            (s._render_frost_veil if frost["mode"] == 1 else s._render_frost_glow)(None, vp)
            if not s.rec["draws"]:
                return None
            p = s._frost_veil_prog if frost["mode"] == 1 else s._frost_glow_prog
            other = s._frost_glow_prog if frost["mode"] == 1 else s._frost_veil_prog
            assert not other, "the other look's program was touched"
            for mode, n, first, blend, mask, state in s.rec["draws"]:
                on = {}
                for what, flag in state:
                    on[flag] = what == "enable"
                assert mode == "TRIANGLE_STRIP" and blend == ("ONE", "ONE_MINUS_SRC_ALPHA") and mask is False, (mode, blend, mask)
                assert on.get("DEPTH_TEST") is False and on.get("BLEND") is True, state
            assert [(n, first) for _, n, first, *_ in s.rec["draws"]] == [(STRIDE, k * STRIDE) for k in range(4)]
            assert s.ctx.depth_mask is True and s.state[-2:] == [("disable", "BLEND"), ("enable", "DEPTH_TEST")]
            uni = {k: (list(v.value) if isinstance(v.value, tuple) else v.value) for k, v in p.items() if v.value is not None}
            mats = {k: np.frombuffer(p[k].bytes, np.float32).reshape(4, 4).copy() for k in ("u_model", "u_vp")}
            _, _, fd, fhw, fhh = s._frost_front_layout()
            return dict(verts=s.rec["verts"], uniforms=uni, draws=[(n, first) for _, n, first, *_ in s.rec["draws"]],
                        layout=[float(fd), float(fhw), float(fhh)], **mats)
        s.render = render
        return s
    return make


def clamp_texture(gl, img, unit):
    """uint8 [H,W,3] -> a plain LINEAR, CLAMP_TO_EDGE RGB8 texture without mipmaps (the veil's: effects.py:603-607, frame.py:39-40)."""
    t = gl.texture(img, unit)
    for k in (0x2802, 0x2803):
        gl.gl.glTexParameteri(0x0DE1, k, 0x812F)
    gl._check("clamp_texture")
    return t


def stats4(a, b, ok):
    d = np.abs(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))[ok]
    da = np.abs(a[..., 3].astype(np.float64) - b[..., 3].astype(np.float64))[ok]
    return float((d > 1).mean()), float(d.mean()), float(da.max()), float(d.max())


def main(render=True):
    import gl_harness as G
    import xr_eye_ref as X
    import xr_frost_ref as F
    import xr_glow_ref as R
    from desktop2stereo_amd import xr
    from make_golden_xr_crop import xr_shader_patch
    from make_golden_xr_eye import FOV, _strings, reference_geometry
    from make_golden_xr_glow import draw_eye, mip_texture
    make_screen, fov_to_proj, pose_to_view = reference_geometry()
    make_frost = reference_frost()
    (_, _, _), (fs, l0, l1) = G.reference_shaders()
    patch, p0, p1 = xr_shader_patch()
    src = _strings(os.path.join(REF, "glsl.py"), ("_WORLD_VERT", "_FROST_GLOW_VERT", "_FROST_VEIL_FRAG", "_FROST_GLOW_FRAG"))
    fs2, defaults = G.to_es300(patch(fs))
    gl = G.Gles()
    screen_prog = gl.program(G.to_es300(src["_WORLD_VERT"])[0], fs2)
    progs = {1: gl.program(G.to_es300(src["_FROST_GLOW_VERT"])[0], G.to_es300(src["_FROST_VEIL_FRAG"])[0]),
             2: gl.program(G.to_es300(src["_FROST_GLOW_VERT"])[0], G.to_es300(src["_FROST_GLOW_FRAG"])[0])}
    data = {}
    meta = {"cases": [], "gl": {"version": gl.version, "renderer": gl.renderer}, "fov": FOV,
            "shader": f"walls: xr_viewer/glsl.py _FROST_GLOW_VERT with _FROST_VEIL_FRAG / _FROST_GLOW_FRAG; screen: viewer.py:{l0}-{l1} through "
                      f"xr_viewer/implementation.py:{p0}-{p1} behind _WORLD_VERT; ES 3.00 patches: see gl_harness.py",
            "textures": "frosted: RGB8 after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, CLAMP_TO_EDGE.  Veil: LINEAR, CLAMP_TO_EDGE, no "
                        "mipmaps.  Screen pass: a LINEAR / REPEAT copy of the same image, as tests/golden/xr_glow.json has it",
            "encoding": "xr_frost.npz: rint(clip(rgb, 0, 1) * 255 * 16) = 16 * <case>_<eye>_rgb + <case>_<eye>_rgbf (uint8 whole levels and uint8 "
                        "sixteenths: two planes compress where one 16-bit plane does not); <case>_<eye>_a = uint16 rint(alpha * 65535), "
                        "both at the STORED pixels only, 0 elsewhere: the compared pixels (class uniform on 3 x 3) that a wall's geometry covers "
                        "-- for the two empty cases, would cover.  What no wall covers is a plain d2s_dibr_xr_eyes pixel: tests/golden/xr_eye.npz "
                        "pins those, and the GPU test holds them bit-identical to that call.  <case>_verts = float32 [632, 5]: the four strips "
                        "_build_flat_frost_verts wrote, x y t u v per vertex (the empty cases: the library's own, nothing was written)",
            "bounds": "per case and eye, over the pixels whose float64 class is uniform on 3 x 3: gl = the float64 restatement over the "
                      "recorded triangles vs the render, f32 = the float32 emulation of the kernel's walk vs that restatement: [share of rgb "
                      "values beyond 1 level, mean |rgb diff| in levels, max |alpha diff|, max |rgb diff|]; walk = [max |v_uv diff|, max |t "
                      "diff|] of the kernel's walk in float64 vs the recorded triangles over the wall pixels; analytic_s: max |a / g(t) "
                      "mapped to 0..1 - the mesh's s|; excluded = the share of pixels not compared; counts = compared pixels [no wall, one "
                      "wall, two or more walls, wall over screen], cut = pixels whose wall hit lies beyond the near or far plane",
            "eyes": "eye i of a case looks from frost.head + eye_shift + (-+0.032, 0, 0) with identity orientation"}
    for c in CASES:
        H, W = c["source"]
        img, dep = F.case_scene(c)
        levels = R.chain(img)
        sc, fr = c["screen"], c["frost"]
        s = make_screen(**sc)
        model = np.asarray(s._build_model_mat4(normal_offset=0.0), np.float32)
        facets = X.facets_flat(model)
        stub = make_frost(sc, fr, c["crop"])
        lib_screen = xr.XrScreen(**sc, clear=tuple(c["clear"]))
        lib_frost = xr.XrFrost(**dict(fr, mode={1: "veil", 2: "frosted"}[fr["mode"]], head=tuple(fr["head"])))
        crec = dict(c, screen_model=model.tolist(), eyes=[])
        if render:
            t_lin, t_dep = gl.texture(img, 0), gl.texture(dep, 1)
            t_src = clamp_texture(gl, img, 2) if fr["mode"] == 1 else mip_texture(gl, img, 2)
        n_wall = n_two = n_over = n_cut = 0
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
                crec.update(layout=rec["layout"], frost_model=rec["u_model"].T.tolist(), frost_uniforms=rec["uniforms"], draws=rec["draws"])
                verts = rec["verts"]
            if rec is not None:
                assert np.array_equal(rec["verts"], verts) and rec["u_model"].T.tolist() == crec["frost_model"]
            if rec is None and eye == 0:      # nothing drawn: the library's own numbers say where the walls WOULD lie (the stored pixels)
                crec.update(layout=list(lib_frost.layout(lib_screen)), frost_model=lib_frost.model_mat4(lib_screen).tolist(),
                            frost_uniforms=None, draws=[])
                verts = lib_frost.wall_verts(lib_screen).reshape(-1, 5).astype(np.float32)
            data[f"{c['name']}_verts"] = verts
            e = dict(eye=eye, vp=vp.tolist(), size=[ew, eh], pos=pos)
            r64, cls, info = F.case_render(crec, e, img, dep, levels, verts, np.float64, mesh=True)
            r32, _, _ = F.case_render(crec, e, img, dep, levels, verts, np.float32, mesh=False)
            ok = F.uniform3x3(cls)
            excluded = float(1.0 - ok.mean())
            assert excluded <= 0.15, (c["name"], eye, excluded)
            nw, cov = info["n_walls"], info["covered"]
            counts = [int(((nw == 0) & ok).sum()), int(((nw == 1) & ok).sum()), int(((nw >= 2) & ok).sum()), int(((nw >= 1) & cov & ok).sum())]
            mh = F.mesh_hits(verts.reshape(4, -1, 5), np.array(crec["frost_model"]), vp, ew, eh)
            stored = ok & np.any([m["hit"] for m in mh], 0)
            wh = F.walk_hits(F.wall_rows(sc, fr["head"], vp, ew, eh), ew, eh, np.float64)
            cut = int(sum(m["cut"].sum() for m in mh))
            walk_uv = walk_t = analytic = 0.0
            for k in range(4):
                m = mh[k]["hit"] & wh[k]["hit"]
                assert (mh[k]["hit"] ^ wh[k]["hit"]).sum() <= 0.02 * max(int(mh[k]["hit"].sum()), 50), (c["name"], eye, k)
                if m.any():
                    walk_uv = max(walk_uv, float(np.abs(mh[k]["u"] - wh[k]["u"])[m].max()), float(np.abs(mh[k]["v"] - wh[k]["v"])[m].max()))
                    walk_t = max(walk_t, float(np.abs(mh[k]["t"] - wh[k]["t"])[m].max()))
                    s_mesh = mh[k]["v"] if k >= 2 else mh[k]["u"]
                    analytic = max(analytic, float(np.abs(wh[k]["s_analytic"] - s_mesh)[m].max()))
            b32 = stats4(r32, r64, ok)
            e.update(excluded=excluded, counts=counts, cut=cut, f32=list(b32), walk=[walk_uv, walk_t], analytic_s=analytic)
            if render:
                uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(W), float(H)),
                           u_eye_offset=float((1.0 if eye else -1.0) * c["ipd_uv"] / 2.0), u_depth_strength=float(0.1 * c["depth_ratio"]),
                           u_convergence=float(c["convergence"]), u_roll=float(sc["roll"]), u_feather_enabled=0, u_feather_width=0.02,
                           u_viewport=(0.0, 0.0, float(ew), float(eh)), u_source_crop=tuple(float(v) for v in c["crop"]),
                           **{k: float(v) for k, v in defaults.items()})
                uni["u_corner_radius"] = float(c["corner_radius"])
                quad = np.array([[-1, -1, 0, 0], [1, -1, 1, 0], [-1, 1, 0, 1], [1, 1, 1, 1]], np.float32)
                passes = [dict(prog=screen_prog, uniforms=uni, mats=dict(u_mvp=vp @ model), textures={0: t_lin, 1: t_dep}, verts=quad, ncomp=2,
                               mode=0x0005, first=0, count=4, blend=False, depth=True)]
                if rec is not None:
                    wuni = {k: (float(v) if isinstance(v, float) else v) for k, v in rec["uniforms"].items()}
                    wuni["u_source"] = 2
                    for n, first in rec["draws"]:
                        passes.append(dict(prog=progs[fr["mode"]], uniforms=wuni, mats=dict(u_model=rec["u_model"].T, u_vp=rec["u_vp"].T),
                                           textures={2: t_src}, verts=rec["verts"], ncomp=3, mode=0x0005, first=first, count=n, blend=True,
                                           depth=False))
                out = draw_eye(gl, passes, ew, eh, c["clear"])
                assert np.isfinite(out).all()
                enc_rgb = np.rint(np.clip(out[..., :3], 0, 1) * (255.0 * RGB_STEPS)).astype(np.uint16) * stored[..., None]
                enc_a = np.rint(np.clip(out[..., 3], 0, 1) * 65535.0).astype(np.uint16) * stored
                golden = np.concatenate([enc_rgb / RGB_STEPS, enc_a[..., None] / 65535.0], -1)
                e["gl"] = list(stats4(r64, golden, stored)[:3])
                e["stored"] = int(stored.sum())
                data[f"{c['name']}_{eye}_rgb"], data[f"{c['name']}_{eye}_a"] = (enc_rgb >> 4).astype(np.uint8), enc_a
                data[f"{c['name']}_{eye}_rgbf"] = (enc_rgb & 15).astype(np.uint8)
            print(f"{c['name']} eye {eye} {ew}x{eh}: counts {counts} cut {cut} excluded {excluded:.3f} | walk {walk_uv:.2e} {walk_t:.2e} analytic "
                  f"{analytic:.2e} | f32 vs f64 {['%.3g' % v for v in b32]} | f64 vs GL {['%.3g' % v for v in e.get('gl', [])]}", flush=True)
            n_wall += counts[1] + counts[2]
            n_two += counts[2]
            n_over += counts[3]
            n_cut += cut
            crec["eyes"].append(e)
        if not c.get("empty"):
            assert n_wall >= 500, (c["name"], n_wall)
        else:
            assert n_wall == 0
        assert n_two >= c.get("min_two", 0) and n_over >= c.get("min_over", 0) and n_cut >= c.get("min_cut", 0), (c["name"], n_two, n_over, n_cut)
        # the library's host side is the reference's: the layout, the model matrix, the vertices, the uniforms
        assert np.allclose(lib_frost.layout(lib_screen), crec["layout"], rtol=2e-6, atol=0), (lib_frost.layout(lib_screen), crec["layout"])
        assert np.allclose(lib_frost.model_mat4(lib_screen), np.array(crec["frost_model"]), rtol=2e-6, atol=2e-6)
        assert np.allclose(lib_frost.wall_verts(lib_screen).reshape(-1, 5), verts, rtol=2e-6, atol=2e-7)
        if render:
            for t in (t_lin, t_dep, t_src):
                gl.delete_texture(t)
        meta["cases"].append(crec)
    if not render:
        return meta
    np.savez_compressed(os.path.join(HERE, "xr_frost.npz"), **data)
    with open(os.path.join(HERE, "xr_frost.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote xr_frost", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "xr_frost.npz")), "bytes")


if __name__ == "__main__":
    main(render="--no-render" not in sys.argv)
