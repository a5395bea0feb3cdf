"""Golden vectors for the OpenXR eye views (d2s_dibr_xr_eyes): the REFERENCE's screen drawn per eye, off-screen on SwiftShader.

    python tests/golden/make_golden_xr_eye.py        # -> tests/golden/xr_eye.npz + xr_eye.json

Everything of the reference is read from its checkout with `ast` at generation time and none of its text is stored:
  * _WORLD_VERT and _CURVED_VERT (xr_viewer/glsl.py), the vertex shaders of the flat quad and of the curved strip;
  * the XR fragment shader: viewer.py's FRAGMENT_SHADER through _make_xr_fragment_shader (make_golden_xr_crop.xr_shader_patch);
  * the function definitions _build_model_mat4 and _build_curved_screen_verts (xr_viewer/screen.py), _screen_effect_basis
    (xr_viewer/effects.py), _fov_to_proj_mat4 and _pose_to_view_mat4 (xr_viewer/render.py), compiled on their own and called on a
    plain object that carries the screen_* attributes; _CURVED_HALF_ANGLE_RAD is evaluated from xr_viewer/constants.py.
Each eye image is drawn as EffectsMixin._render_eye draws it (effects.py:1023-1137): cleared to the background with alpha 1 and depth
1, depth test LESS, blending off, the flat quad with u_mvp = vp @ model or the 98-vertex strip with u_mvp = vp, every matrix the
float32 the reference uploads.  draw() below is this file's own small render routine on gl_harness.Gles (vertex array, mat4 uniform,
depth renderbuffer, clear colour).  Encoding: xr_crop.npz's (rgb * 255 * 256 and alpha * 65535 as uint16).

The manifest records, per case, the matrices and strip vertices (what the xr.py helpers are tested against) and the MEASURED bounds
the GPU test uses: over the pixels whose float64 coverage is uniform on their 3 x 3 neighbourhood (the rasteriser's fill rule owns
the outline; asserted <= 10 % of an image), (a) a float32 run of the restatement (tests/xr_eye_ref.py) against its float64 run and
(b) the float64 run against the SwiftShader render: the share of values beyond 1 level, the mean, and the alpha maximum.
"""
from __future__ import annotations

import ast
import ctypes as C
import json
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

SRC_H, SRC_W, EYE_W, EYE_H = 96, 160, 130, 100
BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0, corner_radius=0.0, crop=[0.0, 0.0, 1.0, 1.0], clear=[0.0, 0.0, 0.0, 1.0],
            depth_hw=None, head=[0.0, 0.0, 0.0])
SCREEN = dict(width=1.6, height=0.96, distance=1.4, pan_x=0.0, pan_y=0.0, yaw=0.0, pitch=0.0, roll=0.0, curve="flat", normal_offset=0.0)
# OpenXR's asymmetric per-eye frusta (angle_left, angle_right, angle_up, angle_down)
FOV = [(-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60)]
CASES = [
    dict(BASE, name="flat_front", seed=41, screen=dict(SCREEN)),
    # about a third of the screen outside BOTH eye images (over the top edge: the two frusta share their vertical angles): asserted
    dict(BASE, name="flat_oblique", seed=42, screen=dict(SCREEN, yaw=0.5, pitch=-0.2, roll=0.15, pan_y=0.58, distance=1.2), off_image=[0.25, 0.45]),
    dict(BASE, name="flat_crop_corner", seed=43, screen=dict(SCREEN, height=0.64), crop=[0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0], corner_radius=0.03,
         clear=[0.1, 0.2, 0.3, 1.0]),
    dict(BASE, name="curved_h", seed=44, screen=dict(SCREEN, curve="horizontal", distance=1.5)),
    dict(BASE, name="curved_v_yaw", seed=45, screen=dict(SCREEN, curve="vertical", yaw=0.3, distance=1.5, pan_x=0.2)),
    dict(BASE, name="far", seed=46, screen=dict(SCREEN, distance=2.42)),                       # ~53 pixels across 160 texels
    dict(BASE, name="near", seed=47, screen=dict(SCREEN, distance=0.27)),                      # ~480 pixels across 160 texels
    dict(BASE, name="model_depth", seed=48, screen=dict(SCREEN, pan_y=0.1), depth_hw=[24, 40]),
    # beyond the issue's eight: the depth rule and the rounded corners away from the outline
    # the arc seen from beyond its end: the near end (its back face) hides part of the far end, every vertex in front of the eye
    dict(BASE, name="curved_occluded", seed=49, screen=dict(SCREEN, curve="horizontal", yaw=1.3, pan_x=0.1, distance=1.0), min_overlap=200),
    # corners wide enough that the SDF's transition band lies inside the compared pixels (at 0.03 it is within a pixel of the outline)
    dict(BASE, name="flat_corner_wide", seed=50, screen=dict(SCREEN, distance=1.25), corner_radius=0.3, min_alpha_band=20),
]


def _defs(path, names, cls=None):
    """{name: FunctionDef} of module-level functions (cls None) or of the methods of class `cls`."""
    with open(path) as f:
        tree = ast.parse(f.read())
    body = tree.body
    if cls:
        body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    out = {n.name: n for n in body if isinstance(n, ast.FunctionDef) and n.name in names}
    assert set(out) == set(names), (path, set(names) - set(out))
    return out


def _strings(path, names):
    with open(path) as f:
        tree = ast.parse(f.read())
    out = {n.targets[0].id: n.value.value for n in tree.body if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name)
           and n.targets[0].id in names and isinstance(n.value, ast.Constant)}
    assert set(out) == set(names)
    return out


def reference_geometry():
    """The reference's geometry functions as callables: (make_screen(**screen) -> object with _build_model_mat4 /
    _build_curved_screen_verts, fov_to_proj, pose_to_view)."""
    import math
    ns = {"np": np, "math": math}
    with open(os.path.join(REF, "constants.py")) as f:
        for n in ast.parse(f.read()).body:
            if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id in ("_CURVED_CURVATURE_SCALE", "_CURVED_HALF_ANGLE_RAD"):
                exec(compile(ast.Module(body=[n], type_ignores=[]), "constants.py", "exec"), ns)
    fns = {}
    fns.update(_defs(os.path.join(REF, "screen.py"), ("_build_model_mat4", "_build_curved_screen_verts"), "ScreenMixin"))
    fns.update(_defs(os.path.join(REF, "effects.py"), ("_screen_effect_basis",), "EffectsMixin"))
    fns.update(_defs(os.path.join(REF, "render.py"), ("_fov_to_proj_mat4", "_pose_to_view_mat4")))
    exec(compile(ast.Module(body=list(fns.values()), type_ignores=[]), REF, "exec"), ns)
    Screen = type("Screen", (), {k: ns[k] for k in ("_build_model_mat4", "_build_curved_screen_verts", "_screen_effect_basis")})
    Screen._screen_curve_mode = lambda self: self.curve_axis

    def make_screen(width, height, distance, pan_x, pan_y, yaw, pitch, roll, curve, normal_offset):
        s = Screen()
        s.screen_width, s.screen_height, s.screen_distance, s.screen_pan_x, s.screen_pan_y = width, height, distance, pan_x, pan_y
        s.screen_yaw, s.screen_pitch, s.screen_roll = yaw, pitch, roll
        s.curve_axis = {"flat": "none", "horizontal": "horizontal", "vertical": "vertical"}[curve]
        return s
    return make_screen, ns["_fov_to_proj_mat4"], ns["_pose_to_view_mat4"]


def draw(gl, prog, uniforms, mvp, verts, ncomp, w, h, clear):
    """verts [n, ncomp + 2] float32 (position, uv) as a TRIANGLE_STRIP under u_mvp = mvp (numpy convention: uploaded transposed, as
    the reference writes mvp.T), into an RGBA32F colour + 24-bit depth target cleared to `clear` / 1.0, depth test LESS, no blending
    -> float32 [h,w,4], row 0 = top."""
    g = gl.gl
    g.glClearDepthf.argtypes = [C.c_float]
    g.glUniformMatrix4fv.argtypes = [C.c_int, C.c_int, C.c_ubyte, C.c_void_p]
    fbo, tex, rbo, vbo = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    g.glGenTextures(1, C.byref(tex))
    g.glActiveTexture(0x84C0 + 7)
    g.glBindTexture(0x0DE1, tex)
    g.glTexImage2D(0x0DE1, 0, 0x8814, w, h, 0, 0x1908, 0x1406, None)                  # RGBA32F
    g.glTexParameteri(0x0DE1, 0x2801, 0x2600)
    g.glTexParameteri(0x0DE1, 0x2800, 0x2600)
    g.glGenRenderbuffers(1, C.byref(rbo))
    g.glBindRenderbuffer(0x8D41, rbo)
    g.glRenderbufferStorage(0x8D41, 0x81A6, w, h)                                     # DEPTH_COMPONENT24 (screen.py:193)
    g.glGenFramebuffers(1, C.byref(fbo))
    g.glBindFramebuffer(0x8D40, fbo)
    g.glFramebufferTexture2D(0x8D40, 0x8CE0, 0x0DE1, tex, 0)
    g.glFramebufferRenderbuffer(0x8D40, 0x8D00, 0x8D41, rbo)
    if g.glCheckFramebufferStatus(0x8D40) != 0x8CD5:
        raise RuntimeError("framebuffer incomplete")
    g.glViewport(0, 0, w, h)
    g.glDisable(0x0BE2)                                                               # BLEND off (effects.py:1046)
    g.glEnable(0x0B71)                                                                # DEPTH_TEST (effects.py:1044)
    g.glDepthFunc(0x0201)                                                             # LESS
    g.glDepthMask(1)
    g.glClearColor(*[float(c) for c in clear])
    g.glClearDepthf(1.0)
    g.glClear(0x4000 | 0x0100)
    g.glUseProgram(prog)
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
        else:
            g.glUniform4f(loc, *[float(v) for v in val])
    loc = g.glGetUniformLocation(prog, b"u_mvp")
    assert loc >= 0
    m = np.ascontiguousarray(np.asarray(mvp, np.float32).T)
    g.glUniformMatrix4fv(loc, 1, 0, m.ctypes.data)
    verts = np.ascontiguousarray(verts, np.float32)
    stride = (ncomp + 2) * 4
    g.glGenBuffers(1, C.byref(vbo))
    g.glBindBuffer(0x8892, vbo)
    g.glBufferData(0x8892, verts.nbytes, verts.ctypes.data, 0x88E4)
    g.glEnableVertexAttribArray(0)
    g.glEnableVertexAttribArray(1)
    g.glVertexAttribPointer(0, ncomp, 0x1406, 0, stride, C.c_void_p(0))
    g.glVertexAttribPointer(1, 2, 0x1406, 0, stride, C.c_void_p(ncomp * 4))
    g.glDrawArrays(0x0005, 0, verts.shape[0])
    g.glFinish()
    out = np.empty((h, w, 4), np.float32)
    g.glPixelStorei(0x0D05, 1)
    g.glReadPixels(0, 0, w, h, 0x1908, 0x1406, out.ctypes.data)
    gl._check("draw")
    g.glDisable(0x0B71)
    g.glBindFramebuffer(0x8D40, 0)
    g.glDeleteFramebuffers(1, C.byref(fbo))
    g.glDeleteRenderbuffers(1, C.byref(rbo))
    g.glDeleteTextures(1, C.byref(tex))
    g.glDeleteBuffers(1, C.byref(vbo))
    return out[::-1].copy()


def case_inputs(c):
    """(rgb, the H x W depth texture, the depth map handed to the library) of a case."""
    from desktop2stereo_amd import synth
    from oracle import d2s_oracle as O
    img, dep = synth.dibr_scene(SRC_H, SRC_W, c["seed"], "boxes")
    if c["depth_hw"]:
        small = synth.dibr_scene(c["depth_hw"][0], c["depth_hw"][1], c["seed"], "boxes")[1]
        return img, O.upsample_depth(small, SRC_H, SRC_W).astype(np.float32), small
    return img, dep, dep


def off_image_share(mvp):
    """The share of the flat quad (a uniform 64 x 64 grid over +-1) that projects outside the image."""
    g = (np.arange(64) + 0.5) / 32.0 - 1.0
    xx, yy = np.meshgrid(g, g)
    c = np.asarray(mvp, np.float64) @ np.stack([xx.ravel(), yy.ravel(), np.zeros(xx.size), np.ones(xx.size)])
    return float(((np.abs(c[:2] / c[3]) > 1).any(0) | (c[3] <= 0)).mean())


def stats(a, b, ok):
    """a, b [h,w,4] (rgb 0..255, alpha 0..1) over the pixels ok -> (share of rgb values beyond 1 level, mean |rgb diff|, max |alpha diff|)"""
    d = np.abs(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))[ok]
    da = np.abs(a[..., 3].astype(np.float64) - b[..., 3].astype(np.float64))[ok]
    return float((d > 1.0).mean()), float(d.mean()), float(da.max())


def main():
    import gl_harness as G
    import xr_eye_ref as X
    from make_golden_xr_crop import xr_shader_patch
    make_screen, fov_to_proj, pose_to_view = reference_geometry()
    (_, _, _), (fs, l0, l1) = G.reference_shaders()
    patch, p0, p1 = xr_shader_patch()
    vtx = _strings(os.path.join(REF, "glsl.py"), ("_WORLD_VERT", "_CURVED_VERT"))
    fs2, defaults = G.to_es300(patch(fs))
    gl = G.Gles()
    progs = {k: gl.program(G.to_es300(v)[0], fs2) for k, v in vtx.items()}
    data, meta = {}, {"cases": [], "gl": {"version": gl.version, "renderer": gl.renderer},
                      "shader": f"viewer.py:{l0}-{l1} through xr_viewer/implementation.py:{p0}-{p1}; vertex shaders xr_viewer/glsl.py "
                                "_WORLD_VERT / _CURVED_VERT; ES 3.00 patches: see gl_harness.py",
                      "source": [SRC_H, SRC_W], "eye": [EYE_H, EYE_W], "fov": FOV,
                      "encoding": "<case>_<eye>_rgb = uint16 rint(frag_color.rgb * 255 * 256); <case>_<eye>_a = uint16 rint(frag_color.a * 65535)",
                      "bounds": "per case and eye, over the pixels with uniform 3 x 3 float64 coverage: [share of rgb values beyond 1 "
                                "level, mean |rgb diff| in levels, max |alpha diff|] of f32 = float32 vs float64 restatement and gl = "
                                "float64 restatement vs the SwiftShader render; excluded = the share of pixels not compared"}
    for c in CASES:
        img, dep, dep_lib = case_inputs(c)
        tc, td = gl.texture(img, 0), gl.texture(dep, 1)
        sc = c["screen"]
        s = make_screen(**sc)
        curved = sc["curve"] != "flat"
        model = np.asarray(s._build_model_mat4(normal_offset=sc["normal_offset"]), np.float32)
        strip = np.asarray(s._build_curved_screen_verts(normal_offset=sc["normal_offset"]), np.float32).reshape(-1, 5) if curved else None
        facets = X.facets_strip(strip, sc["curve"] == "vertical") if curved else X.facets_flat(model)
        rec = dict(c, model=model.tolist(), strip=strip.tolist() if curved else None, eyes=[])
        for eye in (0, 1):
            l, r, u, d = FOV[eye]
            fov = types.SimpleNamespace(angle_left=l, angle_right=r, angle_up=u, angle_down=d)
            pos = [c["head"][0] + (-0.032 if eye == 0 else 0.032), c["head"][1], c["head"][2]]
            pose = types.SimpleNamespace(orientation=types.SimpleNamespace(x=0.0, y=0.0, z=0.0, w=1.0),
                                         position=types.SimpleNamespace(x=pos[0], y=pos[1], z=pos[2]))
            proj, view = fov_to_proj(fov), pose_to_view(pose)
            vp = proj @ view                                                           # effects.py:1060, float32
            assert vp.dtype == np.float32 and X.min_clip_w(facets, vp) > 1e-6
            uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(SRC_W), float(SRC_H)),
                       u_eye_offset=float((1.0 if eye else -1.0) * c["ipd_uv"] / 2.0), u_depth_strength=float(0.1 * c["depth_ratio"]),
                       u_convergence=float(c["convergence"]), u_roll=float(sc["roll"]), u_feather_enabled=0, u_feather_width=0.02,
                       u_viewport=(0.0, 0.0, float(EYE_W), float(EYE_H)), u_source_crop=tuple(float(v) for v in c["crop"]),
                       **{k: float(v) for k, v in defaults.items()})
            uni["u_corner_radius"] = float(c["corner_radius"])
            if curved:
                out = draw(gl, progs["_CURVED_VERT"], uni, vp, strip, 3, EYE_W, EYE_H, c["clear"])
            else:
                quad = np.array([[-1, -1, 0, 0], [1, -1, 1, 0], [-1, 1, 0, 1], [1, 1, 1, 1]], np.float32)      # implementation.py:1060-1065
                out = draw(gl, progs["_WORLD_VERT"], uni, vp @ model, quad, 2, EYE_W, EYE_H, c["clear"])
            assert np.isfinite(out).all()
            enc_rgb = np.rint(np.clip(out[..., :3], 0, 1) * (255.0 * 256.0)).astype(np.uint16)
            enc_a = np.rint(np.clip(out[..., 3], 0, 1) * 65535.0).astype(np.uint16)
            golden = np.concatenate([enc_rgb / 256.0, enc_a[..., None] / 65535.0], -1)      # (as the tests decode it)
            kw = dict(crop=c["crop"], ipd_uv=c["ipd_uv"], depth_strength=0.1 * c["depth_ratio"], convergence=c["convergence"],
                      roll=sc["roll"], corner_radius=c["corner_radius"])
            r64, cov = X.render_eye(img, dep, facets, vp, EYE_W, EYE_H, eye, c["clear"], T=np.float64, **kw)
            r32, _ = X.render_eye(img, dep, facets, vp, EYE_W, EYE_H, eye, c["clear"], T=np.float32, **kw)
            ok = X.uniform3x3(cov)
            excluded = float(1.0 - ok.mean())
            assert excluded <= 0.10, (c["name"], eye, excluded)                        # a pose that breaks the cap is replaced
            assert (ok & cov).sum() > 500, (c["name"], eye)
            extra = {}
            if "off_image" in c:
                extra["off_image"] = off_image_share(vp.astype(np.float64) @ model.astype(np.float64))
                assert c["off_image"][0] <= extra["off_image"] <= c["off_image"][1], (c["name"], eye, extra)
            if "min_overlap" in c:      # pixels that two facets cover, neither a neighbour of the other: the depth rule decides them
                _, count = X.coverage(facets, vp, EYE_W, EYE_H)
                extra["overlap_pixels"] = int(((count >= 2) & ok).sum())
                assert extra["overlap_pixels"] >= c["min_overlap"], (c["name"], eye, extra)
            if "min_alpha_band" in c:
                extra["alpha_band_pixels"] = int(((r64[..., 3] > 0.02) & (r64[..., 3] < 0.98) & ok).sum())
                assert extra["alpha_band_pixels"] >= c["min_alpha_band"], (c["name"], eye, extra)
            b32, bgl = stats(r32, r64, ok), stats(r64, golden, ok)
            print(f"{c['name']} eye {eye}: covered {cov.mean():.3f} excluded {excluded:.3f} | f32 vs f64 {b32} | f64 vs GL {bgl} {extra}")
            data[f"{c['name']}_{eye}_rgb"], data[f"{c['name']}_{eye}_a"] = enc_rgb, enc_a
            rec["eyes"].append(dict(eye=eye, fov=[l, r, u, d], position=pos, orientation=[0.0, 0.0, 0.0, 1.0], proj=proj.tolist(),
                                    view=view.tolist(), vp=vp.tolist(), covered=float(cov.mean()), excluded=excluded, f32=list(b32), gl=list(bgl), **extra))
        gl.delete_texture(tc)
        gl.delete_texture(td)
        meta["cases"].append(rec)
    np.savez_compressed(os.path.join(HERE, "xr_eye.npz"), **data)
    with open(os.path.join(HERE, "xr_eye.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote xr_eye", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "xr_eye.npz")), "bytes")


if __name__ == "__main__":
    main()
