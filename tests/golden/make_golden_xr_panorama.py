"""Golden vectors for the panorama background behind the OpenXR screen (d2s_dibr_xr_eyes_panorama): the REFERENCE's panorama pass
drawn before its screen, glow or walls per eye, off-screen on SwiftShader.

    python tests/golden/make_golden_xr_panorama.py        # -> tests/golden/xr_panorama.npz + xr_panorama.json

Everything of the reference is read from its checkout with `ast` at generation time and none of its text is stored:
  * _PANORAMA_VERT and _PANORAMA_FRAG (xr_viewer/glsl.py) through gl_harness.to_es300 (the patches that apply are listed in the
    manifest); the screen's, the glow's and the walls' shaders as make_golden_xr_eye / _glow / _frost take them;
  * EffectsMixin._render_panorama_background (xr_viewer/effects.py), compiled on its own and EXECUTED on a stub object whose fake ctx,
    program, vertex array and texture record every uniform, the draw and the GL state -- asserted: depth test off, depth mask off,
    blending off, one TRIANGLE_STRIP, texture unit 8;
  * the glow and the walls through make_golden_xr_glow.reference_glow and make_golden_xr_frost.reference_frost, unchanged.
Draw sequence per eye into one RGBA32F target, _render_eye's (effects.py:1023-1145): clear; the panorama quad (-1..1, z 0.999) with
the recorded uniforms; then the outer glow band, the screen (flat quad or curved strip), the inner band or the four wall strips, each
exactly as the generator of that look draws it.  The panorama is an RGB8 texture after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR,
REPEAT in s, CLAMP_TO_EDGE in t (effects.py:956-964).  It is synthesised (tests/xr_panorama_ref.py synth_panorama: sinusoids, a
gradient and +-3 levels of noise) from the seed in the manifest and never stored.

An eye's head pose is a position and (yaw, pitch, roll) in degrees; eye i stands at position + (-+0.032, 0, 0).  An eye with flip_y
has its projection's row 1 negated, as _render_eye(flip_y=True) does; every pass then uses that projection.

Asserted fixture conditions (a float32 rounding must not move a quad across the seam or through a pole): over every point the LOD rule
evaluates -- the pixel centres and the helper points one pixel beyond the image -- u is further than 1e-5 from an integer and |dir.y|
further than 1e-6 from 1.  Excluded pixels (3 x 3 class not uniform) <= 10 % per eye.

Recorded per case and eye: gl = the float64 restatement (tests/xr_panorama_ref.py) against the render [share of rgb values beyond 1
level, mean, alpha maximum]; f32 = the float32 emulation of the kernel over the library's own geometry against that restatement
[share, mean, alpha maximum, rgb maximum]; lam_gt_half = compared uncovered pixels with lambda > 0.5; seam = compared uncovered pixels
whose quad the u seam crosses; background = compared pixels no facet covers; blended = those of them over which a glow or a wall
leaves between 5 % and 95 % of the panorama (asserted >= 2000 per look case).
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

RGB_STEPS = 2.0       # the renders are stored to half a level: the bounds are "beyond 1 level" and a mean of half a level
FOV = [(-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60)]
PANO = dict(size=[512, 1024], seed=301, yaw_offset_deg=0.0, exposure=1.0, flip_y=False)
BASE = dict(kind="plain", ipd_uv=0.064, depth_ratio=4.0, convergence=0.0, corner_radius=0.0, crop=[0.0, 0.0, 1.0, 1.0],
            clear=[0.1, 0.2, 0.3, 1.0], source=[96, 160], eye_sizes=[[130, 100], [130, 100]], eye_flip=False, fov=FOV,
            position=[0.0, 0.0, 0.0], look=[0.0, 0.0, 0.0], alpha_mode="rgba")
SCREEN = dict(width=1.6, height=0.96, distance=1.4, pan_x=0.0, pan_y=0.0, yaw=0.0, pitch=0.0, roll=0.0, curve="flat", normal_offset=0.0)
VEIL = dict(mode=1, head=[0.0, 0.0, 0.0], intensity=1.5, alpha=1.0, edge_inset=0.02, beam_softness=0.34, beam_thickness=3.0,
            lod=5.4, threshold=0.46, noise_scale=54.0, blend=1.35, diffuse=0.85, time=0.0)
FROSTED = dict(VEIL, mode=2, intensity=1.0, alpha=0.42, edge_inset=0.045, beam_thickness=1.6, noise_scale=6.0)
CASES = [
    # 0.42 texel per pixel: lambda = 0 everywhere
    dict(BASE, name="magnified", seed=101, screen=dict(SCREEN), panorama=dict(PANO, size=[128, 256], seed=301)),
    # 3.4 texels per pixel at the horizon, lambda about 1.8 there; seen from below, looking up 50 degrees (the zenith stays outside the
    # image): towards the top of the image the meridians crowd and lambda rises by up to 0.1 per pixel, so a quad's shared level shows
    dict(BASE, name="minified", seed=102, screen=dict(SCREEN), position=[0.0, -3.0, 0.0], look=[0.0, 50.0, 0.0],
         panorama=dict(PANO, size=[1024, 2048], seed=302), min_lam=5000),
    # from behind the screen, looking along +z at its back: u wraps on a vertical line through the image
    dict(BASE, name="seam", seed=103, screen=dict(SCREEN), position=[0.0, 0.0, -3.4], look=[180.0, 0.0, 0.0],
         panorama=dict(PANO, seed=303), min_seam=60),
    # from below, looking up: the zenith 10 degrees above the image centre
    dict(BASE, name="pole", seed=104, screen=dict(SCREEN), position=[0.0, -3.0, 0.0], look=[0.0, 80.0, 0.0], panorama=dict(PANO, seed=304)),
    # every setting at once; exposure 1.7 runs into the clamp at 255, and the pattern's zeros stay 0
    dict(BASE, name="yaw_exposure_flip", seed=105, screen=dict(SCREEN), look=[20.0, -10.0, 0.0],
         panorama=dict(PANO, size=[256, 512], seed=305, yaw_offset_deg=77.0, exposure=1.7, flip_y=True), clamp=True),
    # the chain's odd steps: 1000 x 562 -> 500 x 281 -> 250 x 140 -> ...
    dict(BASE, name="odd_panorama", seed=106, screen=dict(SCREEN), look=[-35.0, 15.0, 0.0], panorama=dict(PANO, size=[562, 1000], seed=306)),
    # an eye with flip_y and an odd image height, around the zenith, where lambda changes from one row of quads to the next: the quads
    # pair window rows, not image rows.  (The seam runs straight up the image here; an oblique one passes within 1e-5 of some pixel.)
    dict(BASE, name="flip_odd_height", seed=107, screen=dict(SCREEN), position=[0.0, -3.0, 0.0], look=[0.0, 78.0, 0.0], eye_flip=True,
         eye_sizes=[[130, 101], [130, 101]], panorama=dict(PANO, seed=307), min_seam=40),
    # a far more lopsided frustum than OpenXR's own, and two eyes of different sizes
    dict(BASE, name="asymmetric_two_sizes", seed=108, screen=dict(SCREEN, pan_x=0.2), fov=[(-0.30, 0.90, 0.70, -0.20), (-0.60, 0.75, 0.55, -0.60)],
         eye_sizes=[[130, 100], [111, 87]], look=[10.0, 0.0, 0.0], panorama=dict(PANO, size=[1024, 2048], seed=308)),
    dict(BASE, name="glow_flat", kind="glow", seed=109, screen=dict(SCREEN), source=[256, 512],
         glow=dict(mode=1, range_m=1.2, inner_edge_fraction=0.075), panorama=dict(PANO, seed=309), min_blend=2000),
    # (the veil's own intensity 1.5 saturates its alpha at 1 over the whole wall here: nothing would show through)
    dict(BASE, name="veil_flat", kind="frost", seed=110, screen=dict(SCREEN), frost=dict(VEIL, intensity=0.6), min_blend=2000,
         panorama=dict(PANO, seed=310)),
    dict(BASE, name="frosted_flat", kind="frost", seed=111, screen=dict(SCREEN, distance=1.15), source=[256, 512], frost=dict(FROSTED, noise_scale=3.0),
         panorama=dict(PANO, seed=311), min_blend=2000),
    dict(BASE, name="curved_plain", seed=112, screen=dict(SCREEN, curve="horizontal", distance=1.5), panorama=dict(PANO, size=[1024, 2048], seed=312)),
]


def quaternion(yaw_deg, pitch_deg, roll_deg):
    """(x, y, z, w) of yaw about +y, then pitch about the turned +x, then roll about the turned +z (degrees): yaw 180 looks along +z."""
    def q(axis, deg):
        a = math.radians(deg) / 2.0
        return np.array([math.sin(a) * axis[0], math.sin(a) * axis[1], math.sin(a) * axis[2], math.cos(a)])

    def mul(a, b):
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                         aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
    return mul(mul(q((0, 1, 0), yaw_deg), q((1, 0, 0), pitch_deg)), q((0, 0, 1), roll_deg))


def reference_panorama():
    """render(settings dict, view, proj) -> dict(u_inv_proj, u_inv_view_rot [4,4] in numpy convention, u_yaw_offset, u_exposure,
    u_flip_y): the reference's _render_panorama_background run on a stub, its GL state asserted."""
    from make_golden_xr_eye import _defs
    from make_golden_xr_glow import _Prog
    fns = _defs(os.path.join(REF, "effects.py"), ("_render_panorama_background",), "EffectsMixin")
    mgl = types.SimpleNamespace(DEPTH_TEST="DEPTH_TEST", BLEND="BLEND", TRIANGLE_STRIP="TRIANGLE_STRIP")
    ns = {"np": np, "math": math, "moderngl": mgl}
    exec(compile(ast.Module(body=list(fns.values()), type_ignores=[]), REF, "exec"), ns)
    Stub = type("Stub", (), {k: ns[k] for k in fns})

    def render(settings, view, proj):
        s = Stub()
        state, rec = [], dict(draws=[], units=[], masks=[])
        class Ctx:                                                          # (records every assignment to depth_mask)
            enable = staticmethod(lambda f: state.append(("enable", f)))
            disable = staticmethod(lambda f: state.append(("disable", f)))
            depth_mask = property(lambda self: rec["masks"][-1] if rec["masks"] else True, lambda self, v: rec["masks"].append(v))
        s.ctx = Ctx()
        s._panorama_prog = _Prog()
        s._panorama_vao = types.SimpleNamespace(render=lambda mode: rec["draws"].append((mode, tuple(state), list(rec["masks"]))))
        s._get_panorama_texture = lambda: types.SimpleNamespace(use=lambda location=0: rec["units"].append(location))
        s._panorama_background_settings = dict(settings)
        s._render_panorama_background(types.SimpleNamespace(use=lambda: None), view, proj)
        assert len(rec["draws"]) == 1 and rec["units"] == [8], rec
        mode, st, masks = rec["draws"][0]
        on = {}
        for what, flag in st:
            on[flag] = what == "enable"
        assert mode == "TRIANGLE_STRIP" and on == {"DEPTH_TEST": False, "BLEND": False} and masks == [False], (mode, st, masks)
        assert rec["masks"] == [False, True] and state[-1] == ("enable", "DEPTH_TEST")
        p = s._panorama_prog
        mats = {k: np.frombuffer(p[k].bytes, np.float32).reshape(4, 4).T.copy() for k in ("u_inv_proj", "u_inv_view_rot")}
        return dict(u_yaw_offset=float(p["u_yaw_offset"].value), u_exposure=float(p["u_exposure"].value), u_flip_y=int(p["u_flip_y"].value), **mats)
    return render


def pano_texture(gl, img, unit):
    """uint8 [H,W,3] -> RGB8 after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, REPEAT s, CLAMP_TO_EDGE t (effects.py:956-964)."""
    g = gl.gl
    t = gl.texture(img, unit)
    g.glGenerateMipmap(0x0DE1)
    for k, v in ((0x2801, 0x2703), (0x2800, 0x2601), (0x2802, 0x2901), (0x2803, 0x812F)):
        g.glTexParameteri(0x0DE1, k, v)
    gl._check("pano_texture")
    return t


def stats4(a, b, ok):
    d = np.abs(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))[ok]
    da = np.abs(a[..., 3].astype(np.float64) - b[..., 3].astype(np.float64))[ok]
    return float((d > 1).mean()), float(d.mean()), float(da.max()), float(d.max())


def es300_patches(src):
    """The ES 3.00 patches of gl_harness.to_es300 that change this source, by name."""
    import re
    out = ["#version 330 -> #version 300 es + highp default precisions", "leading blank line of the string constant removed"]
    if re.search(r"uniform\s+(float|int)\s+\w+\s*=", src):
        out.append("uniform initialisers -> set as uniform values")
    return out


def main():
    import gl_harness as G
    import xr_eye_ref as X
    import xr_glow_ref as R
    import xr_panorama_ref as P
    from desktop2stereo_amd import xr
    from make_golden_xr_crop import xr_shader_patch
    from make_golden_xr_eye import _strings, reference_geometry
    from make_golden_xr_frost import clamp_texture, reference_frost
    from make_golden_xr_glow import draw_eye, mip_texture, read_levels, reference_glow
    make_screen, fov_to_proj, pose_to_view = reference_geometry()
    make_glow, _ = reference_glow()
    make_frost = reference_frost()
    render_pano = reference_panorama()
    (_, _, _), (fs, l0, l1) = G.reference_shaders()
    patch, p0, p1 = xr_shader_patch()
    src = _strings(os.path.join(REF, "glsl.py"), ("_PANORAMA_VERT", "_PANORAMA_FRAG", "_WORLD_VERT", "_CURVED_VERT", "_GLOW_VERT", "_GLOW_FRAG",
                                                  "_FROST_GLOW_VERT", "_FROST_VEIL_FRAG", "_FROST_GLOW_FRAG"))
    fs2, defaults = G.to_es300(patch(fs))
    es = lambda k: G.to_es300(src[k])[0]
    gl = G.Gles()
    pano_prog = gl.program(es("_PANORAMA_VERT"), es("_PANORAMA_FRAG"))
    screen_progs = {False: gl.program(es("_WORLD_VERT"), fs2), True: gl.program(es("_CURVED_VERT"), fs2)}
    glow_prog = gl.program(es("_GLOW_VERT"), es("_GLOW_FRAG"))
    wall_progs = {1: gl.program(es("_FROST_GLOW_VERT"), es("_FROST_VEIL_FRAG")), 2: gl.program(es("_FROST_GLOW_VERT"), es("_FROST_GLOW_FRAG"))}
    data = {}
    meta = {"cases": [], "gl": {"version": gl.version, "renderer": gl.renderer},
            "shader": f"panorama: xr_viewer/glsl.py _PANORAMA_VERT / _PANORAMA_FRAG; screen: viewer.py:{l0}-{l1} through "
                      f"xr_viewer/implementation.py:{p0}-{p1} behind _WORLD_VERT / _CURVED_VERT; glow: _GLOW_VERT / _GLOW_FRAG; walls: "
                      "_FROST_GLOW_VERT with _FROST_VEIL_FRAG / _FROST_GLOW_FRAG",
            "es300_patches": {"_PANORAMA_VERT": es300_patches(src["_PANORAMA_VERT"]), "_PANORAMA_FRAG": es300_patches(src["_PANORAMA_FRAG"]),
                              "others": "see gl_harness.py"},
            "textures": "panorama: RGB8 after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, REPEAT s, CLAMP_TO_EDGE t, synthesised by "
                        "tests/xr_panorama_ref.py synth_panorama(height, width, seed).  The other textures as the generator of that look has them",
            "encoding": "xr_panorama.npz: rint(clip(rgb, 0, 1) * 255 * 2) = 2 * <case>_<eye>_rgb + <case>_<eye>_rgbf (uint8 whole levels and "
                        "uint8 halves); <case>_<eye>_a = uint16 rint(alpha * 65535); all at the compared pixels (class uniform on 3 x 3), 0 "
                        "elsewhere.  <case>_verts = float32 [632, 5]: the four wall strips (frost cases)",
            "bounds": "per case and eye over the compared pixels: gl = float64 restatement vs the render [share of rgb values beyond 1 level, "
                      "mean |rgb diff| in levels, max |alpha diff|]; f32 = the float32 emulation of the kernel over the library's geometry vs "
                      "that restatement [share, mean, max |alpha diff|, max |rgb diff|]; excluded = the share of pixels not compared; "
                      "background = compared pixels no facet covers; lam_gt_half, seam = those of them with lambda > 0.5 / in a quad the u "
                      "seam crosses; lam_range = their smallest and largest lambda",
            "eyes": "eye i of a case looks from position + (-+0.032, 0, 0) with orientation quaternion(look = yaw, pitch, roll in degrees); "
                    "eye_flip: the projection's row 1 negated (_render_eye's flip_y)"}
    for c in CASES:
        H, W = c["source"]
        img, dep, pano = P.case_scene(c)
        levels, pano_levels = R.chain(img), R.chain(pano)
        sc, pn = c["screen"], c["panorama"]
        curved = sc["curve"] != "flat"
        s = make_screen(**sc)
        model = np.asarray(s._build_model_mat4(normal_offset=0.0), np.float32)
        strip = np.asarray(s._build_curved_screen_verts(normal_offset=0.0), np.float32).reshape(-1, 5) if curved else None
        facets = X.facets_strip(strip, sc["curve"] == "vertical") if curved else X.facets_flat(model)
        crec = dict(c, screen_model=model.tolist(), model=model.tolist(), strip=strip.tolist() if curved else None, eyes=[])
        t_lin, t_dep = gl.texture(img, 0), gl.texture(dep, 1)
        t_pano = pano_texture(gl, pano, 3)
        crec["chain_is_restated"] = bool(all(np.array_equal(a, b) for a, b in zip(pano_levels, read_levels(gl, t_pano, *pn["size"]))))
        t_src = None
        verts = None
        if c["kind"] == "glow":
            t_src = mip_texture(gl, img, 2)
            gstub = make_glow(sc, [0.0, 0.0, 0.0], c["glow"]["inner_edge_fraction"], c["crop"])
        if c["kind"] == "frost":
            t_src = clamp_texture(gl, img, 2) if c["frost"]["mode"] == 1 else mip_texture(gl, img, 2)
            fstub = make_frost(sc, c["frost"], c["crop"])
        quat = quaternion(*c["look"])
        n_lam = n_seam = n_blend = 0
        lo255 = [False, False]
        for eye in (0, 1):
            ew, eh = c["eye_sizes"][eye]
            l, r, u, d = c["fov"][eye]
            fov = types.SimpleNamespace(angle_left=l, angle_right=r, angle_up=u, angle_down=d)
            pos = [c["position"][k] + ((-0.032 if eye == 0 else 0.032) if k == 0 else 0.0) for k in range(3)]
            pose = types.SimpleNamespace(orientation=types.SimpleNamespace(x=quat[0], y=quat[1], z=quat[2], w=quat[3]),
                                         position=types.SimpleNamespace(x=pos[0], y=pos[1], z=pos[2]))
            proj, view = fov_to_proj(fov), pose_to_view(pose)
            if c["eye_flip"]:                                                   # effects.py:1032-1034
                proj = proj.copy()
                proj[1, :] = -proj[1, :]
            vp = proj @ view
            assert vp.dtype == np.float32 and X.min_clip_w(facets, vp) > 1e-6, (c["name"], X.min_clip_w(facets, vp))
            prec = render_pano(dict(yaw_offset_deg=pn["yaw_offset_deg"], exposure=pn["exposure"], flip_y=pn["flip_y"]), view, proj)
            assert prec["u_flip_y"] == int(pn["flip_y"]) and abs(prec["u_yaw_offset"] - pn["yaw_offset_deg"] / 360.0) < 1e-12
            e = dict(eye=eye, size=[ew, eh], pos=pos, proj=proj.tolist(), view=view.tolist(), vp=vp.tolist(),
                     u_inv_proj=prec["u_inv_proj"].tolist(), u_inv_view_rot=prec["u_inv_view_rot"].tolist(),
                     u_yaw_offset=prec["u_yaw_offset"], u_exposure=prec["u_exposure"])
            # the library's rays are the reference's matrices
            rays = xr.panorama_rays(proj, view)
            a = prec["u_inv_proj"].astype(np.float64)
            want = prec["u_inv_view_rot"].astype(np.float64)[:3, :3] @ np.stack([a[:3, 0], a[:3, 1], a[:3, 2] + a[:3, 3]], 1)
            assert np.allclose(rays / np.abs(rays).max(), want / np.abs(want).max(), rtol=0, atol=5e-6), (c["name"], eye)
            # the fixture conditions, over every point the LOD rule evaluates
            coord = P.case_coord(crec, e, lib=False)
            yy, xx = np.mgrid[-1:eh + 1, -1:ew + 1].astype(np.float64)
            ur, _, ady = coord.raw(xx, yy)
            e["min_seam_distance"], e["min_pole_distance"] = float(np.abs(ur - np.rint(ur)).min()), float((1.0 - ady).min())
            assert e["min_seam_distance"] > 1e-5 and e["min_pole_distance"] > 1e-6, (c["name"], eye, e)
            passes = [dict(prog=pano_prog, uniforms=dict(u_tex=3, u_yaw_offset=prec["u_yaw_offset"], u_exposure=prec["u_exposure"],
                                                         u_flip_y=prec["u_flip_y"]),
                           mats=dict(u_inv_proj=prec["u_inv_proj"], u_inv_view_rot=prec["u_inv_view_rot"]), textures={3: t_pano},
                           verts=np.array([[-1, -1, 0, 0], [1, -1, 0, 0], [-1, 1, 0, 0], [1, 1, 0, 0]], np.float32), ncomp=2, mode=0x0005, first=0,
                           count=4, blend=False, depth=False)]
            uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(W), float(H)),
                       u_eye_offset=float((1.0 if eye else -1.0) * c["ipd_uv"] / 2.0), u_depth_strength=float(0.1 * c["depth_ratio"]),
                       u_convergence=float(c["convergence"]), u_roll=float(sc["roll"]), u_feather_enabled=0, u_feather_width=0.02,
                       u_viewport=(0.0, 0.0, float(ew), float(eh)), u_source_crop=tuple(float(v) for v in c["crop"]),
                       **{k: float(v) for k, v in defaults.items()})
            uni["u_corner_radius"] = float(c["corner_radius"])
            if curved:
                screen_pass = dict(prog=screen_progs[True], uniforms=uni, mats=dict(u_mvp=vp), textures={0: t_lin, 1: t_dep}, verts=strip, ncomp=3,
                                   mode=0x0005, first=0, count=strip.shape[0], blend=False, depth=True)
            else:
                quad = np.array([[-1, -1, 0, 0], [1, -1, 1, 0], [-1, 1, 0, 1], [1, 1, 1, 1]], np.float32)
                screen_pass = dict(prog=screen_progs[False], uniforms=uni, mats=dict(u_mvp=vp @ model), textures={0: t_lin, 1: t_dep}, verts=quad,
                                   ncomp=2, mode=0x0005, first=0, count=4, blend=False, depth=True)
            if c["kind"] == "glow":
                gw = c["glow"]
                outer = gstub.render_glow(vp, False, gw["mode"] == 2, gw["range_m"])
                inner = gstub.render_glow(vp, True, gw["mode"] == 2, gw["range_m"])

                def glow_pass(g):
                    gu = {k: (float(v) if isinstance(v, float) else v) for k, v in g["uniforms"].items()}
                    gu["u_source"] = 2
                    return dict(prog=glow_prog, uniforms=gu, mats=dict(u_model=g["u_model"].T, u_vp=g["u_vp"].T), textures={2: t_src},
                                verts=g["verts"], ncomp=2, mode=0x0004, first=g["first"], count=g["vertices"], blend=True, depth=False)
                passes += [glow_pass(outer), screen_pass] + ([glow_pass(inner)] if gw["mode"] == 1 else [])
            elif c["kind"] == "frost":
                rec = fstub.render(vp)
                assert rec is not None
                if eye == 0:
                    crec.update(layout=rec["layout"], frost_model=rec["u_model"].T.tolist(), frost_uniforms=rec["uniforms"], draws=rec["draws"])
                    verts = rec["verts"]
                    data[f"{c['name']}_verts"] = verts
                assert np.array_equal(rec["verts"], verts)
                wuni = {k: (float(v) if isinstance(v, float) else v) for k, v in rec["uniforms"].items()}
                wuni["u_source"] = 2
                passes.append(screen_pass)
                for n, first in rec["draws"]:
                    passes.append(dict(prog=wall_progs[c["frost"]["mode"]], uniforms=wuni, mats=dict(u_model=rec["u_model"].T, u_vp=rec["u_vp"].T),
                                       textures={2: t_src}, verts=rec["verts"], ncomp=3, mode=0x0005, first=first, count=n, blend=True, depth=False))
            else:
                passes.append(screen_pass)
            out = draw_eye(gl, passes, ew, eh, c["clear"])
            assert np.isfinite(out).all()
            r64, cls, info = P.case_render(crec, e, img, dep, levels, pano_levels, verts, np.float64, lib=False)
            r32, _, _ = P.case_render(crec, e, img, dep, levels, pano_levels, verts, np.float32, lib=True)
            ok = P.uniform3x3(cls)
            excluded = float(1.0 - ok.mean())
            assert excluded <= 0.10, (c["name"], eye, excluded)
            enc_rgb = np.rint(np.clip(out[..., :3], 0, 1) * (255.0 * RGB_STEPS)).astype(np.uint16) * ok[..., None]
            enc_a = np.rint(np.clip(out[..., 3], 0, 1) * 65535.0).astype(np.uint16) * ok
            golden = np.concatenate([enc_rgb / RGB_STEPS, enc_a[..., None] / 65535.0], -1)
            bgm = ok & ~info["covered"]
            e.update(excluded=excluded, gl=list(stats4(r64, golden, ok)[:3]), f32=list(stats4(r32, r64, ok)), background=int(bgm.sum()),
                     lam_gt_half=int((bgm & (info["lam"] > 0.5)).sum()), seam=int((bgm & info["seam"]).sum()),
                     lam_range=[float(info["lam"][bgm].min()), float(info["lam"][bgm].max())])
            e["blended"] = int((bgm & (info["K"] > 0.05) & (info["K"] < 0.95)).sum())      # the panorama shows THROUGH a glow or a wall
            n_blend += e["blended"]
            n_lam += e["lam_gt_half"]
            n_seam += e["seam"]
            plain_bg = bgm & (info["K"] == 1.0)
            lo255[0] |= bool((np.rint(golden[..., :3])[plain_bg] == 0).any())
            lo255[1] |= bool((np.rint(golden[..., :3])[plain_bg] == 255).any())
            data[f"{c['name']}_{eye}_rgb"], data[f"{c['name']}_{eye}_rgbf"] = (enc_rgb >> 1).astype(np.uint8), (enc_rgb & 1).astype(np.uint8)
            data[f"{c['name']}_{eye}_a"] = enc_a
            print(f"{c['name']} eye {eye} {ew}x{eh}: background {e['background']} lam {e['lam_range'][0]:.2f}..{e['lam_range'][1]:.2f} > 0.5: "
                  f"{e['lam_gt_half']} seam {e['seam']} excluded {excluded:.3f} | f32 vs f64 {['%.3g' % v for v in e['f32']]} | f64 vs GL "
                  f"{['%.3g' % v for v in e['gl']]}", flush=True)
            assert e["gl"][0] <= 0.10 and e["gl"][1] <= 0.5, (c["name"], eye, e["gl"])
            crec["eyes"].append(e)
        assert n_lam >= c.get("min_lam", 0) and n_seam >= c.get("min_seam", 0) and n_blend >= c.get("min_blend", 0), (c["name"], n_lam, n_seam, n_blend)
        if c.get("clamp"):
            assert all(lo255), (c["name"], lo255)
        for t in (t_lin, t_dep, t_pano) + ((t_src,) if t_src is not None else ()):
            gl.delete_texture(t)
        meta["cases"].append(crec)
    np.savez_compressed(os.path.join(HERE, "xr_panorama.npz"), **data)
    with open(os.path.join(HERE, "xr_panorama.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote xr_panorama", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "xr_panorama.npz")), "bytes")


if __name__ == "__main__":
    main()
