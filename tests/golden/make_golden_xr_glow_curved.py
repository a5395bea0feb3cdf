"""Golden vectors for the glow around the CURVED OpenXR screen (d2s_dibr_xr_eyes_glow_curved): the REFERENCE's curved glow mesh drawn
around its curved screen per eye, off-screen on SwiftShader.

    python tests/golden/make_golden_xr_glow_curved.py        # -> tests/golden/xr_glow_curved.npz + xr_glow_curved.json

Everything of the reference is read from its checkout with `ast` at generation time and none of its text is stored:
  * _CURVED_VERT / _GLOW_FRAG (xr_viewer/glsl.py) through gl_harness.to_es300; the screen's shaders as make_golden_xr_eye.py takes them;
  * EffectsMixin._render_curved_glow, _build_curved_glow_band_verts, _screen_effect_basis, _glow_range_m (xr_viewer/effects.py),
    ScreenMixin._screen_uv_to_world, _build_curved_screen_verts (xr_viewer/screen.py) and CropMixin._set_source_crop_uniform
    (xr_viewer/crop.py), compiled on their own and EXECUTED on a stub object whose fake ctx, _curved_glow_vbo, _curved_glow_prog and
    _curved_glow_vao record the mesh, every uniform and the (vertices, first) of each draw.
Draw sequence per eye into one RGBA32F target, _render_eye's (effects.py:1050-1145): clear (colour, depth 1); the mesh's outer vertices
blended ONE / ONE_MINUS_SRC_ALPHA with the depth test off; the curved strip as make_golden_xr_eye.py draws it (depth test LESS,
blending off) with the GL_LINEAR copy of the frame, as the flat glow's fixtures do; mode 1: the mesh's inner vertices, blended.

Asserted here: every recorded quad is coplanar with the piece the library's model claims for it (tests/xr_glow_curved_ref.py
quad_pieces / check_mesh, desktop2stereo_amd/xr.py XrScreen.glow_pieces) to 1e-5 m and carries that piece's affine uv to 1e-6 -- but
for a VERTICAL curve's two long inner bands: 48 chords of the arc from strip coordinate e to 1 - e, which do not start at a facet seam;
they are held to the facets within radius * (1 - cos(0.01)) + 1e-5 m and 2e-6 uv --; every eye is inside the convex region
(XrScreen.eye_inside); excluded pixels <= 10 % per eye image for the reference alone (the float64 rasteriser's region class not
uniform on 3 x 3); curved_h_glow_oblique: >= 5 % of one image's pixels have a tangent-plane point with clip w <= 0.
The bounds are measured: per case and eye the float32 emulation of the kernel's search against the float64 rasteriser of the recorded
triangles, and that rasteriser against the render (share of rgb values beyond 1 level, mean, alpha maximum).
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

BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0, corner_radius=0.0, crop=[0.0, 0.0, 1.0, 1.0], clear=[0.0, 0.0, 0.0, 1.0],
            head=[0.0, 0.0, 0.0], inner_edge_fraction=0.075, mode=1, range_m=1.2, source=[512, 1024], eye_size=[130, 100])
SCREEN = dict(width=1.6, height=0.96, distance=1.5, pan_x=0.0, pan_y=0.0, yaw=0.0, pitch=0.0, roll=0.0, curve="horizontal", normal_offset=0.0)
CASES = [
    dict(BASE, name="curved_h_glow_front", seed=71, screen=dict(SCREEN)),
    dict(BASE, name="curved_h_glow2_front", seed=72, screen=dict(SCREEN), mode=2, range_m=2.4),
    dict(BASE, name="curved_v_glow_front", seed=73, screen=dict(SCREEN, curve="vertical")),
    # the head moved sideways and the screen yawed: the far end's tangent plane fills a large share of the image and passes behind the eye
    dict(BASE, name="curved_h_glow_oblique", seed=74, screen=dict(SCREEN, yaw=0.55, distance=1.3), head=[-0.45, 0.0, 0.0], range_m=None,
         min_behind=0.05),
    dict(BASE, name="curved_v_glow2_tilt", seed=75, screen=dict(SCREEN, curve="vertical", pitch=-0.25, roll=0.2, pan_y=0.15), mode=2, range_m=None),
    dict(BASE, name="curved_h_glow_crop_corner", seed=76, screen=dict(SCREEN, height=0.64), crop=[0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0],
         corner_radius=0.3, clear=[0.1, 0.2, 0.3, 1.0], source=[256, 512]),
    dict(BASE, name="curved_h_glow_odd", seed=77, screen=dict(SCREEN, pan_x=0.75, distance=0.8, height=1.3), source=[562, 1000], eye_size=[70, 51]),
    # (at 70 x 51 a whole outline is > 10 % of the image: one end of the arc crosses it, the other three edges lie outside)
    # both arc ends and both tangent pieces inside the image
    dict(BASE, name="curved_h_glow_near", seed=78, screen=dict(SCREEN, width=1.2, height=0.72, distance=1.25), range_m=0.8),
]


def reference_curved_glow():
    """make(screen dict, head, inner_edge_fraction, crop) -> the stub; its render(vp, inner_only, glow2, range) runs the reference's
    _render_curved_glow and returns dict(verts [n, 5], uniforms, u_mvp [4,4] as uploaded, vertices, first, outer_count)."""
    from make_golden_xr_eye import _defs
    from make_golden_xr_glow import _Prog
    ns = {"np": np, "math": math, "moderngl": types.SimpleNamespace(DEPTH_TEST="DEPTH_TEST", BLEND="BLEND", ONE="ONE",
                                                                    ONE_MINUS_SRC_ALPHA="ONE_MINUS_SRC_ALPHA", TRIANGLES="TRIANGLES")}
    with open(os.path.join(REF, "constants.py")) as f:
        for n in ast.parse(f.read()).body:
            if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id in ("_CURVED_CURVATURE_SCALE", "_CURVED_HALF_ANGLE_RAD"):
                exec(compile(ast.Module(body=[n], type_ignores=[]), "constants.py", "exec"), ns)
    fns = {}
    fns.update(_defs(os.path.join(REF, "effects.py"), ("_render_curved_glow", "_build_curved_glow_band_verts", "_screen_effect_basis",
                                                      "_glow_range_m"), "EffectsMixin"))
    fns.update(_defs(os.path.join(REF, "screen.py"), ("_screen_uv_to_world",), "ScreenMixin"))
    fns.update(_defs(os.path.join(REF, "crop.py"), ("_set_source_crop_uniform",), "CropMixin"))
    exec(compile(ast.Module(body=list(fns.values()), type_ignores=[]), REF, "exec"), ns)
    Stub = type("Stub", (), {k: ns[k] for k in fns})

    def make(screen, head, inner_edge_fraction, crop):
        s = Stub()
        s.screen_width, s.screen_height, s.screen_distance = screen["width"], screen["height"], screen["distance"]
        s.screen_pan_x, s.screen_pan_y = screen["pan_x"], screen["pan_y"]
        s.screen_yaw, s.screen_pitch, s.screen_roll = screen["yaw"], screen["pitch"], screen["roll"]
        s._screen_curved, s._head_pos_w = True, tuple(head)
        s._screen_curve_mode = lambda: screen["curve"]
        s._glow_intensity, s._glow_intensity_multiplier, s._glow_inner_edge_fraction = 1.0, 1.0, inner_edge_fraction
        s._glow_color = s._glow_target_color = (1.0, 1.0, 1.0)
        s._advance_glow_color = lambda: None
        s._movie_crop_render_uv_fast = lambda: tuple(crop)
        s._frost_source_texture = lambda: types.SimpleNamespace(use=lambda location=0: None)
        s.state = []
        s.ctx = types.SimpleNamespace(enable=lambda f: s.state.append(("enable", f)), disable=lambda f: s.state.append(("disable", f)),
                                      depth_mask=True, blend_func=None)
        s.rec = {}
        s._curved_glow_vbo = types.SimpleNamespace(write=lambda b: s.rec.__setitem__("verts", np.frombuffer(bytes(b), np.float32).reshape(-1, 5).copy()))
        s._curved_glow_vao = types.SimpleNamespace(render=lambda mode, vertices, first: s.rec.update(mode=mode, vertices=int(vertices), first=int(first)))

        def render(vp, inner_only, glow2, range_override=None):
            s._curved_glow_verts_params, s._curved_glow_prog = None, _Prog()
            if range_override is not None:
                s._glow_range_m = lambda: range_override
            s._render_curved_glow(None, vp, 1.0, inner_only=inner_only, glow2=glow2)
            assert s.ctx.blend_func == ("ONE", "ONE_MINUS_SRC_ALPHA") and ("disable", "DEPTH_TEST") in s.state and s.rec["mode"] == "TRIANGLES"
            p = s._curved_glow_prog
            uni = {k: (list(v.value) if isinstance(v.value, tuple) else v.value) for k, v in p.items() if v.value is not None}
            return dict(verts=s.rec["verts"], uniforms=uni, vertices=s.rec["vertices"], first=s.rec["first"],
                        u_mvp=np.frombuffer(p["u_mvp"].bytes, np.float32).reshape(4, 4).copy(), outer_count=int(s._curved_glow_outer_count))
        s.render = render
        return s
    return make


def main():
    import gl_harness as G
    import xr_eye_ref as X
    import xr_glow_ref as R
    import xr_glow_curved_ref as K
    from desktop2stereo_amd import synth, xr
    from make_golden_xr_crop import xr_shader_patch
    from make_golden_xr_eye import FOV, _strings, reference_geometry, stats
    from make_golden_xr_glow import draw_eye, mip_texture
    make_screen, fov_to_proj, pose_to_view = reference_geometry()
    make_glow = reference_curved_glow()
    (_, _, _), (fs, l0, l1) = G.reference_shaders()
    patch, p0, p1 = xr_shader_patch()
    src = _strings(os.path.join(REF, "glsl.py"), ("_CURVED_VERT", "_GLOW_FRAG"))
    fs2, defaults = G.to_es300(patch(fs))
    gl = G.Gles()
    screen_prog = gl.program(G.to_es300(src["_CURVED_VERT"])[0], fs2)
    glow_prog = gl.program(G.to_es300(src["_CURVED_VERT"])[0], G.to_es300(src["_GLOW_FRAG"])[0])
    data = {}
    meta = {"cases": [], "gl": {"version": gl.version, "renderer": gl.renderer}, "fov": FOV,
            "shader": f"glow: xr_viewer/glsl.py _CURVED_VERT / _GLOW_FRAG; screen: viewer.py:{l0}-{l1} through xr_viewer/implementation.py:{p0}-{p1} "
                      "behind _CURVED_VERT; ES 3.00 patches: see gl_harness.py",
            "textures": "glow passes: RGB8 after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, CLAMP_TO_EDGE.  Screen pass: a LINEAR copy "
                        "of the same image without mipmaps, as tests/golden/xr_glow.json has it",
            "encoding": "xr_glow_curved.npz: <case>_<eye>_rgb = uint8 rint(clip(rgb, 0, 1) * 255); <case>_<eye>_a = uint8 rint(alpha * 255); "
                        "<case>_verts = float32 [n, 5]: the mesh _build_curved_glow_band_verts wrote, x y z u v per vertex (TRIANGLES)",
            "bounds": "per case and eye, over the pixels whose float64 region class is uniform on 3 x 3: [share of rgb values beyond 1 level, "
                      "mean |rgb diff| in levels, max |alpha diff|] of f32 = the float32 emulation of the kernel's search vs the float64 "
                      "rasteriser of the recorded triangles and gl = that rasteriser vs the render; excluded = the share of pixels not "
                      "compared; classes = compared pixels per region class (none, outer, screen, screen + inner)",
            "mesh": "per case: check_mesh's maxima of the recorded mesh against the library's pieces (plane_m, uv; arc_m, arc_uv: a "
                    "vertical curve's long inner bands against the facets)"}
    for c in CASES:
        H, W = c["source"]
        ew, eh = c["eye_size"]
        img, dep = synth.dibr_scene(H, W, c["seed"], "boxes")
        t_lin, t_dep, t_mip = gl.texture(img, 0), gl.texture(dep, 1), mip_texture(gl, img, 2)
        levels = R.chain(img)
        sc = c["screen"]
        s = make_screen(**sc)
        strip = np.asarray(s._build_curved_screen_verts(normal_offset=0.0), np.float32).reshape(-1, 5)
        facets = X.facets_strip(strip, sc["curve"] == "vertical")
        stub = make_glow(sc, c["head"], c["inner_edge_fraction"], c["crop"])
        ref_range = float(stub._glow_range_m())
        lib_screen = xr.XrScreen(**sc, clear=tuple(c["clear"]))
        assert abs(ref_range - xr.glow_range_m(lib_screen, c["head"])) <= 1e-12 * ref_range
        range_m = ref_range if c["range_m"] is None else float(c["range_m"])
        crec = dict(c, range_m=range_m, glow_range_m=ref_range, strip=strip.tolist(), eyes=[])
        lib_glow = xr.XrGlow("glow" if c["mode"] == 1 else "glow2", range_m, c["inner_edge_fraction"])
        U = K.uniforms(sc["width"], sc["height"], c["mode"], range_m, c["inner_edge_fraction"])
        behind = 0.0
        for eye in (0, 1):
            l, r, u, d = FOV[eye]
            fov = types.SimpleNamespace(angle_left=l, angle_right=r, angle_up=u, angle_down=d)
            pos = [c["head"][0] + (-0.032 if eye == 0 else 0.032), c["head"][1], c["head"][2]]
            pose = types.SimpleNamespace(orientation=types.SimpleNamespace(x=0.0, y=0.0, z=0.0, w=1.0),
                                         position=types.SimpleNamespace(x=pos[0], y=pos[1], z=pos[2]))
            vp = fov_to_proj(fov) @ pose_to_view(pose)
            assert vp.dtype == np.float32 and X.min_clip_w(facets, vp) > 1e-6 and lib_screen.eye_inside(vp), (c["name"], eye)
            glow2 = c["mode"] == 2
            outer, inner = stub.render(vp, False, glow2, range_m), stub.render(vp, True, glow2, range_m)
            verts = outer["verts"]
            assert np.array_equal(verts, inner["verts"]) and outer["first"] == 0 and inner["first"] == outer["outer_count"] == outer["vertices"]
            assert (outer["vertices"], inner["vertices"]) == (K.N_OUTER_QUADS * 6, K.N_INNER_QUADS * 6), (outer["vertices"], inner["vertices"])
            if eye == 0:
                mesh = K.check_mesh(verts, lib_screen, lib_glow, U)
                radius = (sc["height"] if sc["curve"] == "vertical" else sc["width"]) / 2.0 / 0.48
                assert mesh["plane_m"] <= 1e-5 and mesh["uv"] <= 1e-6, (c["name"], mesh)
                assert mesh["arc_m"] <= radius * (1.0 - math.cos(0.01)) + 1e-5 and mesh["arc_uv"] <= 2e-6, (c["name"], mesh)
                for k, v in outer["uniforms"].items():      # the host's uniforms are the reference's
                    want = {"u_screen_half": U["half"], "u_glow_inv_range": U["inv_range"], "u_glow_inner": U["inner"]}.get(k)
                    if want is not None:
                        assert np.allclose(v, want, rtol=1e-12, atol=0), (k, v, want)
                crec.update(glow_uniforms=outer["uniforms"], draw=dict(outer=[outer["vertices"], 0], inner=[inner["vertices"], inner["first"]]),
                            mesh=mesh)
                data[f"{c['name']}_verts"] = verts

            def glow_pass(g):
                uni = {k: (float(v) if isinstance(v, float) else v) for k, v in g["uniforms"].items()}
                uni["u_source"] = 2
                return dict(prog=glow_prog, uniforms=uni, mats=dict(u_mvp=g["u_mvp"].T), textures={2: t_mip}, verts=verts, ncomp=3,
                            mode=0x0004, first=g["first"], count=g["vertices"], blend=True, depth=False)
            uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(W), float(H)),
                       u_eye_offset=float((1.0 if eye else -1.0) * c["ipd_uv"] / 2.0), u_depth_strength=float(0.1 * c["depth_ratio"]),
                       u_convergence=float(c["convergence"]), u_roll=float(sc["roll"]), u_feather_enabled=0, u_feather_width=0.02,
                       u_viewport=(0.0, 0.0, float(ew), float(eh)), u_source_crop=tuple(float(v) for v in c["crop"]),
                       **{k: float(v) for k, v in defaults.items()})
            uni["u_corner_radius"] = float(c["corner_radius"])
            passes = [glow_pass(outer), dict(prog=screen_prog, uniforms=uni, mats=dict(u_mvp=vp), textures={0: t_lin, 1: t_dep}, verts=strip,
                                             ncomp=3, mode=0x0005, first=0, count=strip.shape[0], blend=False, depth=True)]
            if c["mode"] == 1:
                passes.append(glow_pass(inner))
            out = draw_eye(gl, passes, ew, eh, c["clear"])
            assert np.isfinite(out).all()
            enc_rgb = np.rint(np.clip(out[..., :3], 0, 1) * 255.0).astype(np.uint8)
            enc_a = np.rint(np.clip(out[..., 3], 0, 1) * 255.0).astype(np.uint8)
            golden = np.concatenate([enc_rgb.astype(np.float64), enc_a[..., None] / 255.0], -1)
            e = dict(eye=eye, vp=vp.tolist(), size=[ew, eh])
            r64, cls = K.case_render(crec, e, verts, img, dep, levels, np.float64)
            r32, _ = K.case_search(crec, e, img, dep, levels, np.float32)
            ok = R.uniform3x3(cls)
            excluded = float(1.0 - ok.mean())
            assert excluded <= 0.10, (c["name"], eye, excluded)
            classes = [int(((cls == k) & ok).sum()) for k in range(4)]
            tab = K.piece_table(lib_screen, lib_glow, vp, ew, eh)
            yc, xc = K._grid(ew, eh, np.float64)
            e["behind"] = float(max(((tab[k, 6] * xc + tab[k, 7] * yc + tab[k, 8]) <= 0).mean() for k in (K.T0, K.T1)))
            behind = max(behind, e["behind"])
            b32, bgl = stats(r32, r64, ok), stats(r64, golden, ok)
            print(f"{c['name']} eye {eye}: classes {classes} excluded {excluded:.3f} behind {e['behind']:.3f} | f32 vs f64 {b32} | f64 vs GL {bgl}")
            data[f"{c['name']}_{eye}_rgb"], data[f"{c['name']}_{eye}_a"] = enc_rgb, enc_a
            crec["eyes"].append(dict(e, excluded=excluded, classes=classes, f32=list(b32), gl=list(bgl)))
        if "min_behind" in c:
            assert behind >= c["min_behind"], (c["name"], behind)
        for t in (t_lin, t_dep, t_mip):
            gl.delete_texture(t)
        meta["cases"].append(crec)
    np.savez_compressed(os.path.join(HERE, "xr_glow_curved.npz"), **data)
    with open(os.path.join(HERE, "xr_glow_curved.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote xr_glow_curved", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "xr_glow_curved.npz")), "bytes")


if __name__ == "__main__":
    main()
