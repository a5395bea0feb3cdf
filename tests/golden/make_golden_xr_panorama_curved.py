"""Golden vectors for the panorama background behind the CURVED OpenXR screen's glow, glow2, veil and frosted looks
(d2s_dibr_xr_eyes_panorama_curved): the REFERENCE's panorama pass drawn before its curved glow mesh, curved strip and curved walls
per eye, off-screen on SwiftShader.

    python tests/golden/make_golden_xr_panorama_curved.py            # -> tests/golden/xr_panorama_curved.npz + xr_panorama_curved.json
    python tests/golden/make_golden_xr_panorama_curved.py --check    # the fixture conditions from the float64 restatement alone, no GL

Everything of the reference is read from its checkout with `ast` at generation time and none of its text is stored:
  * _PANORAMA_VERT / _PANORAMA_FRAG and EffectsMixin._render_panorama_background as make_golden_xr_panorama.py takes them
    (reference_panorama: executed on the recording stub, the GL state asserted);
  * the curved glow through make_golden_xr_glow_curved.reference_curved_glow (the band mesh, every uniform, the two draws) and the
    curved walls through make_golden_xr_frost_curved.reference_curved_frost (the 588 vertices, every uniform, the one draw), unchanged;
  * the screen's shaders as make_golden_xr_eye.py takes them.
Draw sequence per eye into one RGBA32F target, _render_eye's (effects.py:1023-1145): clear; the panorama quad (-1..1, depth test and
blending off) with the recorded uniforms; then ONE of
  * glow_curved: the mesh's outer vertices blended, the curved strip (depth test LESS, blending off), mode 1: the mesh's inner
    vertices blended -- exactly make_golden_xr_glow_curved.py's passes;
  * frost_curved: the curved strip, then the 196 recorded triangles blended with the depth test off -- make_golden_xr_frost_curved.py's.
The panorama is an RGB8 texture after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, REPEAT in s, CLAMP_TO_EDGE in t; it is
synthesised (tests/xr_panorama_ref.py synth_panorama) from the seed in the manifest and never stored.

An eye's head pose is a position and (yaw, pitch, roll) in degrees; eye i stands at position + (-+0.032, 0, 0).  An eye with flip_y
has its projection's row 1 negated, as _render_eye(flip_y=True) does; every pass then uses that projection.  A frost case's walls
are laid out for frost.head, which need not be where the eyes stand.

The cases are the smallest set in which each new instantiation (curved glow, curved veil, curved frosted, with the panorama) can go
wrong; see CASES.  The u seam lies behind a viewer who faces the screen, so glow_h_seam_flip brings it into the band with the
panorama's own yaw offset; the head is level there, so the seam is a vertical line of the image and passes between two pixel columns.

Asserted fixture conditions, each met by the float64 restatement alone (--check): over every point the LOD rule evaluates -- the pixel
centres and the helper points one pixel beyond the image -- u is further than 1e-5 from an integer and |dir.y| further than 1e-6
from 1; every eye of a glow case is inside the convex region (XrScreen.eye_inside); excluded pixels (3 x 3 class not uniform) <= 10 %
per eye on glow cases and <= 15 % on frost cases, the caps of those looks' own fixtures; per case >= 2000 compared uncovered pixels
over which the glow or the walls leave between 5 % and 95 % of the panorama; min_lam: compared uncovered pixels under the band (K <
0.95) with lambda > 0.5; min_seam: compared uncovered pixels in a quad the u seam crosses; clamp: >= 100 compared uncovered pixels
whose panorama value reached the clamp at 255 and shows through the walls (K > 0.05).

Recorded per case and eye, as xr_panorama.json records them: gl = the float64 restatement (tests/xr_panorama_curved_ref.py) against
the render [share of rgb values beyond 1 level, mean, alpha maximum]; f32 = the float32 emulation of the kernel's search / walk and
panorama arithmetic over the library's own geometry against that restatement [share, mean, alpha maximum, rgb maximum].
"""
from __future__ import annotations

import ctypes as C
import json
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

RGB_STEPS = 2.0       # stored to half a level, as xr_panorama.npz is
FOV = [(-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60)]
PANO = dict(size=[512, 1024], seed=401, yaw_offset_deg=0.0, exposure=1.0, flip_y=False)
BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0, corner_radius=0.0, crop=[0.0, 0.0, 1.0, 1.0], clear=[0.1, 0.2, 0.3, 1.0],
            source=[256, 512], eye_sizes=[[130, 100], [130, 100]], eye_flip=False, fov=FOV, position=[0.0, 0.0, 0.0], look=[0.0, 0.0, 0.0],
            alpha_mode="rgba")
GLOW = dict(BASE, kind="glow_curved", mode=1, range_m=1.2, inner_edge_fraction=0.075, head=[0.0, 0.0, 0.0])
FROST = dict(BASE, kind="frost_curved")
SCREEN_G = dict(width=1.6, height=0.96, distance=1.5, pan_x=0.0, pan_y=0.0, yaw=0.0, pitch=0.0, roll=0.0, curve="horizontal", normal_offset=0.0)
SCREEN_F = dict(SCREEN_G, distance=1.4)
VEIL = dict(mode=1, head=[0.0, 0.0, 0.0], intensity=1.5, alpha=1.0, edge_inset=0.02, beam_softness=0.34, beam_thickness=3.0,
            lod=5.4, threshold=0.46, noise_scale=54.0, blend=1.35, diffuse=0.85, time=0.0)
FROSTED = dict(VEIL, mode=2, intensity=1.0, alpha=0.42, edge_inset=0.045, beam_thickness=1.6, noise_scale=6.0)
CASES = [
    dict(GLOW, name="glow_h", seed=201, screen=dict(SCREEN_G), panorama=dict(PANO, seed=401)),
    dict(GLOW, name="glow2_v", seed=202, screen=dict(SCREEN_G, curve="vertical"), mode=2, range_m=2.4, panorama=dict(PANO, seed=402)),
    # the viewer below, looking up: 3.4 texels per pixel at the horizon and more towards the top of the image, where the meridians
    # crowd -- a quad's shared level shows through the translucent band
    dict(GLOW, name="glow_h_minified", seed=203, screen=dict(SCREEN_G), position=[0.0, -0.6, 0.0], look=[0.0, 25.0, 0.0],
         panorama=dict(PANO, size=[1024, 2048], seed=403), min_lam=2000),
    # an eye with flip_y and an odd height: the quads pair window rows, not image rows.  The panorama's yaw offset brings the u seam
    # 33 degrees to the right of straight ahead, into the band beside the arc's end (which both eyes see at 30 degrees)
    dict(GLOW, name="glow_h_seam_flip", seed=204, screen=dict(SCREEN_G), eye_flip=True, eye_sizes=[[130, 101], [130, 101]],
         panorama=dict(PANO, seed=404, yaw_offset_deg=147.0), min_seam=40),
    # (the veil's own intensity 1.5 saturates its alpha over the whole wall: nothing would show through; xr_panorama.json's veil_flat)
    dict(FROST, name="veil_h", seed=205, screen=dict(SCREEN_F), source=[96, 160], frost=dict(VEIL, intensity=0.6), panorama=dict(PANO, seed=405)),
    # a nearer screen and a coarser noise keep the noise-cell seams (excluded pixels) short, as xr_frost_curved.json's NEAR cases do
    dict(FROST, name="frosted_v", seed=206, screen=dict(SCREEN_F, curve="vertical", distance=1.0), frost=dict(FROSTED, noise_scale=3.0),
         panorama=dict(PANO, seed=406)),
    # eyes of two sizes, a far more lopsided frustum than OpenXR's own, the head the walls are laid out for off-centre
    dict(FROST, name="veil_v_two_sizes", seed=207, screen=dict(SCREEN_F, curve="vertical", pan_x=0.2), source=[96, 160],
         frost=dict(VEIL, intensity=0.6, head=[0.35, -0.25, 0.1]), position=[0.35, -0.25, 0.1], look=[10.0, 0.0, 0.0],
         fov=[(-0.30, 0.90, 0.70, -0.20), (-0.60, 0.75, 0.55, -0.60)], eye_sizes=[[130, 100], [111, 87]],
         panorama=dict(PANO, size=[1024, 2048], seed=407)),
    # every panorama setting at once; exposure 1.7 runs into the clamp at 255
    dict(FROST, name="frosted_h_yaw_exposure_flip", seed=208, screen=dict(SCREEN_F, distance=1.0), frost=dict(FROSTED, noise_scale=3.0),
         look=[20.0, -10.0, 0.0], panorama=dict(PANO, size=[256, 512], seed=408, yaw_offset_deg=77.0, exposure=1.7, flip_y=True), clamp=True),
]


def attribs_of(vert_src):
    """[(name, components)] of a vertex shader's inputs, in declaration order: what draw_eye binds a pass's vertex columns to."""
    out = [(m.group(2), int(m.group(1))) for m in re.finditer(r"^\s*(?:layout\s*\([^)]*\)\s*)?in\s+vec([234])\s+(\w+)\s*;", vert_src, re.M)]
    assert out, "no vertex inputs found"
    return out


# The viewer's swapchain is UNORM8: a panorama value that exposure pushes past 1 is clamped when the panorama pass writes it, before
# anything blends over it (the library clamps likewise, include/d2s.h).  The RGBA32F target used here keeps it.  For a `clamp` case the
# panorama pass is therefore drawn on its own, read back, clamped to 0..1 and put back -- unquantised, three R32F textures fetched
# texel for pixel by the two shaders below, which are this file's own -- as the first pass of the one sequence in which the strip and
# the walls are then drawn and blended by GL.
RESTORE_VERT = "#version 300 es\nin vec2 in_position;\nvoid main() { gl_Position = vec4(in_position, 0.0, 1.0); }\n"
RESTORE_FRAG = ("#version 300 es\nprecision highp float;\nuniform highp sampler2D u_r;\nuniform highp sampler2D u_g;\nuniform highp sampler2D u_b;\n"
                "out vec4 fragColor;\nvoid main() {\n    ivec2 p = ivec2(gl_FragCoord.xy);\n"
                "    fragColor = vec4(texelFetch(u_r, p, 0).r, texelFetch(u_g, p, 0).r, texelFetch(u_b, p, 0).r, 1.0);\n}\n")


def main(render=True):
    import xr_eye_ref as X
    import xr_frost_curved_ref as FC
    import xr_glow_curved_ref as GC
    import xr_glow_ref as R
    import xr_panorama_curved_ref as PC
    import xr_panorama_ref as P
    from desktop2stereo_amd import xr
    from make_golden_xr_eye import _strings, reference_geometry
    from make_golden_xr_frost_curved import N_VERTS, draw_eye, reference_curved_frost
    from make_golden_xr_glow_curved import reference_curved_glow
    from make_golden_xr_panorama import es300_patches, pano_texture, quaternion, reference_panorama, stats4
    make_screen, fov_to_proj, pose_to_view = reference_geometry()
    make_glow = reference_curved_glow()
    make_frost = reference_curved_frost()
    render_pano = reference_panorama()
    data = {}
    meta = {"cases": [],
            "shader": "panorama: xr_viewer/glsl.py _PANORAMA_VERT / _PANORAMA_FRAG; glow: as tests/golden/xr_glow_curved.json; walls and "
                      "screen: as tests/golden/xr_frost_curved.json",
            "textures": "panorama: RGB8 after glGenerateMipmap, LINEAR_MIPMAP_LINEAR / LINEAR, REPEAT s, CLAMP_TO_EDGE t, synthesised by "
                        "tests/xr_panorama_ref.py synth_panorama(height, width, seed).  The other textures as the generator of that look has them",
            "encoding": "xr_panorama_curved.npz: rint(clip(rgb, 0, 1) * 255 * 2) = 2 * <case>_<eye>_rgb + <case>_<eye>_rgbf (uint8 whole levels "
                        "and uint8 halves); <case>_<eye>_a = uint16 rint(alpha * 65535); all at the compared pixels (class uniform on 3 x 3), "
                        "0 elsewhere.  <case>_strip = float32 [98, 5]: the screen's TRIANGLE_STRIP as _build_curved_screen_verts wrote it; "
                        "<case>_verts: glow cases float32 [n, 5], the band mesh (TRIANGLES, x y z u v); frost cases float32 [588, 8], the walls",
            "bounds": "per case and eye over the compared pixels: gl = float64 restatement vs the render [share of rgb values beyond 1 level, "
                      "mean |rgb diff| in levels, max |alpha diff|]; f32 = the float32 emulation of the kernel over the library's geometry vs "
                      "that restatement [share, mean, max |alpha diff|, max |rgb diff|]; excluded = the share of pixels not compared; "
                      "background = compared pixels no facet covers; blended = those of them with 0.05 < K < 0.95; lam_gt_half = those under "
                      "the band or a wall (K < 0.95) with lambda > 0.5; seam = those in a quad the u seam crosses",
            "clamp": "a case with clamp: the panorama pass is drawn on its own, clamped to 0..1 as the viewer's UNORM8 swapchain clamps it, and "
                     "put back unquantised as the first pass of the sequence (the float target would keep values above 1 under the walls)",
            "eyes": "eye i of a case looks from position + (-+0.032, 0, 0) with orientation quaternion(look = yaw, pitch, roll in degrees); "
                    "eye_flip: the projection's row 1 negated (_render_eye's flip_y)"}
    if render:
        import gl_harness as G
        from make_golden_xr_crop import xr_shader_patch
        from make_golden_xr_frost import clamp_texture
        from make_golden_xr_glow import mip_texture
        (_, _, _), (fs, l0, l1) = G.reference_shaders()
        patch, p0, p1 = xr_shader_patch()
        src = _strings(os.path.join(REF, "glsl.py"), ("_PANORAMA_VERT", "_PANORAMA_FRAG", "_CURVED_VERT", "_GLOW_FRAG", "_FROST_CURVED_VERT",
                                                      "_FROST_VEIL_FRAG", "_FROST_GLOW_FRAG"))
        fs2, defaults = G.to_es300(patch(fs))
        es = lambda k: G.to_es300(src[k])[0]
        gl = G.Gles()
        gl.gl.glUniform3f.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float]      # (the glow's colour: make_golden_xr_glow.draw_eye sets this for itself)
        meta["gl"] = {"version": gl.version, "renderer": gl.renderer}
        meta["es300_patches"] = {"_PANORAMA_VERT": es300_patches(src["_PANORAMA_VERT"]), "_PANORAMA_FRAG": es300_patches(src["_PANORAMA_FRAG"]),
                                 "others": "see gl_harness.py"}
        meta["shader"] += f"; screen fragment: viewer.py:{l0}-{l1} through xr_viewer/implementation.py:{p0}-{p1}"
        pano_prog = gl.program(es("_PANORAMA_VERT"), es("_PANORAMA_FRAG"))
        restore_prog = gl.program(RESTORE_VERT, RESTORE_FRAG)
        screen_prog = gl.program(es("_CURVED_VERT"), fs2)
        glow_prog = gl.program(es("_CURVED_VERT"), es("_GLOW_FRAG"))
        wall_progs = {1: gl.program(es("_FROST_CURVED_VERT"), es("_FROST_VEIL_FRAG")), 2: gl.program(es("_FROST_CURVED_VERT"), es("_FROST_GLOW_FRAG"))}
        at_pano, at_curved, at_wall = attribs_of(es("_PANORAMA_VERT")), attribs_of(es("_CURVED_VERT")), attribs_of(es("_FROST_CURVED_VERT"))
        assert [n for _, n in at_pano] == [2] and [n for _, n in at_curved] == [3, 2] and [n for _, n in at_wall] == [3, 2, 3], (at_pano, at_curved, at_wall)
    for c in CASES:
        H, W = c["source"]
        img, dep, pano = PC.case_scene(c)
        levels, pano_levels = R.chain(img), R.chain(pano)
        sc, pn = c["screen"], c["panorama"]
        glow_case = c["kind"] == "glow_curved"
        s = make_screen(**sc)
        strip = np.asarray(s._build_curved_screen_verts(normal_offset=0.0), np.float32).reshape(-1, 5)
        facets = X.facets_strip(strip, sc["curve"] == "vertical")
        lib_screen = xr.XrScreen(**sc, clear=tuple(c["clear"]))
        crec = dict(c, strip=strip, eyes=[])                  # (the strip travels in the .npz: xr_panorama_curved_ref.load puts it back)
        data[f"{c['name']}_strip"] = strip
        if glow_case:
            gstub = make_glow(sc, c["head"], c["inner_edge_fraction"], c["crop"])
            lib_glow = xr.XrGlow("glow" if c["mode"] == 1 else "glow2", c["range_m"], c["inner_edge_fraction"])
            U = GC.uniforms(sc["width"], sc["height"], c["mode"], c["range_m"], c["inner_edge_fraction"])
        else:
            fr = c["frost"]
            fstub = make_frost(sc, fr, c["crop"])
            lib_frost = xr.XrFrost(**dict(fr, mode={1: "veil", 2: "frosted"}[fr["mode"]], head=tuple(fr["head"])))
            assert lib_frost.draws()
        if render:
            t_lin, t_dep = gl.texture(img, 0), gl.texture(dep, 1)
            t_pano = pano_texture(gl, pano, 3)
            t_src = clamp_texture(gl, img, 2) if (not glow_case and fr["mode"] == 1) else mip_texture(gl, img, 2)
        quat = quaternion(*c["look"])
        verts = None
        n_lam = n_seam = n_blend = 0
        n_clamp = 0
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
            # the fixture conditions, over every point the LOD rule evaluates
            coord = P.case_coord(crec, e, lib=False)
            yy, xx = np.mgrid[-1:eh + 1, -1:ew + 1].astype(np.float64)
            ur, _, ady = coord.raw(xx, yy)
            e["min_seam_distance"], e["min_pole_distance"] = float(np.abs(ur - np.rint(ur)).min()), float((1.0 - ady).min())
            assert e["min_seam_distance"] > 1e-5 and e["min_pole_distance"] > 1e-6, (c["name"], eye, e["min_seam_distance"], e["min_pole_distance"])
            if glow_case:
                assert lib_screen.eye_inside(vp), (c["name"], eye, "outside the convex region")
                glow2 = c["mode"] == 2
                outer, inner = gstub.render(vp, False, glow2, c["range_m"]), gstub.render(vp, True, glow2, c["range_m"])
                assert np.array_equal(outer["verts"], inner["verts"]) and outer["first"] == 0 and inner["first"] == outer["outer_count"] == outer["vertices"]
                assert (outer["vertices"], inner["vertices"]) == (GC.N_OUTER_QUADS * 6, GC.N_INNER_QUADS * 6)
                if eye == 0:
                    verts = outer["verts"]
                    mesh = GC.check_mesh(verts, lib_screen, lib_glow, U)
                    assert mesh["plane_m"] <= 1e-5 and mesh["uv"] <= 1e-6, (c["name"], mesh)
                    crec.update(glow_uniforms=outer["uniforms"], draw=dict(outer=[outer["vertices"], 0], inner=[inner["vertices"], inner["first"]]))
                assert np.array_equal(outer["verts"], verts)
            else:
                rec = fstub.render(vp)
                assert rec is not None
                if eye == 0:
                    verts = rec["verts"]
                    crec.update(layout=rec["layout"], frost_uniforms=rec["uniforms"])
                    assert np.allclose(lib_frost.layout(lib_screen), rec["layout"], rtol=2e-6, atol=0)
                    assert np.allclose(lib_frost.curved_wall_verts(lib_screen), verts, rtol=2e-6, atol=2e-7)
                assert np.array_equal(rec["verts"], verts) and np.array_equal(rec["u_vp"].T, vp)
            data[f"{c['name']}_verts"] = verts
            r64, cls, info = PC.case_render(crec, e, img, dep, levels, pano_levels, verts, np.float64, lib=False)
            r32, _, _ = PC.case_render(crec, e, img, dep, levels, pano_levels, None, np.float32, lib=True)
            ok = PC.uniform3x3(cls)
            excluded = float(1.0 - ok.mean())
            assert excluded <= (0.10 if glow_case else 0.15), (c["name"], eye, excluded)
            bgm = ok & ~info["covered"]
            K = info["K"]
            e.update(excluded=excluded, f32=list(stats4(r32, r64, ok)), background=int(bgm.sum()),
                     blended=int((bgm & (K > 0.05) & (K < 0.95)).sum()), lam_gt_half=int((bgm & (K < 0.95) & (info["lam"] > 0.5)).sum()),
                     seam=int((bgm & info["seam"]).sum()), lam_range=[float(info["lam"][bgm].min()), float(info["lam"][bgm].max())])
            n_blend += e["blended"]
            n_lam += e["lam_gt_half"]
            n_seam += e["seam"]
            e["clamped"] = int((bgm & (K > 0.05) & (info["bg"] == 255.0).any(-1)).sum())      # (the walls cover every uncovered pixel here: K < 1)
            n_clamp += e["clamped"]
            if render:
                quad = np.array([[-1, -1], [1, -1], [-1, 1], [1, 1]], np.float32)
                passes = [dict(prog=pano_prog, uniforms=dict(u_tex=3, u_yaw_offset=prec["u_yaw_offset"], u_exposure=prec["u_exposure"],
                                                             u_flip_y=prec["u_flip_y"]),
                               mats=dict(u_inv_proj=prec["u_inv_proj"], u_inv_view_rot=prec["u_inv_view_rot"]), textures={3: t_pano}, verts=quad,
                               attribs=at_pano, mode=0x0005, first=0, count=4, blend=False, depth=False)]
                kept = []
                if c.get("clamp"):
                    first = np.clip(draw_eye(gl, passes, ew, eh, c["clear"]), 0.0, 1.0)
                    assert (first[..., :3] == 1.0).any() and (first[..., 3] == 1.0).all()
                    kept = [gl.texture(np.ascontiguousarray(first[::-1, :, k]), 4 + k) for k in range(3)]      # texel row j = window row j
                    passes = [dict(prog=restore_prog, uniforms=dict(u_r=4, u_g=5, u_b=6), mats={}, textures={4 + k: t for k, t in enumerate(kept)},
                                   verts=quad, attribs=at_pano, mode=0x0005, first=0, count=4, blend=False, depth=False)]
                uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(W), float(H)),
                           u_eye_offset=float((1.0 if eye else -1.0) * c["ipd_uv"] / 2.0), u_depth_strength=float(0.1 * c["depth_ratio"]),
                           u_convergence=float(c["convergence"]), u_roll=float(sc["roll"]), u_feather_enabled=0, u_feather_width=0.02,
                           u_viewport=(0.0, 0.0, float(ew), float(eh)), u_source_crop=tuple(float(v) for v in c["crop"]),
                           **{k: float(v) for k, v in defaults.items()})
                uni["u_corner_radius"] = float(c["corner_radius"])
                screen_pass = dict(prog=screen_prog, uniforms=uni, mats=dict(u_mvp=vp), textures={0: t_lin, 1: t_dep}, verts=strip,
                                   attribs=at_curved, mode=0x0005, first=0, count=strip.shape[0], blend=False, depth=True)
                if glow_case:
                    def glow_pass(g):
                        gu = {k: (float(v) if isinstance(v, float) else v) for k, v in g["uniforms"].items()}
                        gu["u_source"] = 2
                        return dict(prog=glow_prog, uniforms=gu, mats=dict(u_mvp=g["u_mvp"].T), textures={2: t_src}, verts=verts,
                                    attribs=at_curved, mode=0x0004, first=g["first"], count=g["vertices"], blend=True, depth=False)
                    passes += [glow_pass(outer), screen_pass] + ([glow_pass(inner)] if c["mode"] == 1 else [])
                else:
                    wuni = {k: (float(v) if isinstance(v, float) else v) for k, v in rec["uniforms"].items()}
                    wuni["u_source"] = 2
                    passes += [screen_pass, dict(prog=wall_progs[fr["mode"]], uniforms=wuni, mats=dict(u_vp=rec["u_vp"].T), textures={2: t_src},
                                                 verts=rec["verts"], attribs=at_wall, mode=0x0004, first=0, count=N_VERTS, blend=True, depth=False)]
                out = draw_eye(gl, passes, ew, eh, c["clear"])
                for t in kept:
                    gl.delete_texture(t)
                assert np.isfinite(out).all()
                enc_rgb = np.rint(np.clip(out[..., :3], 0, 1) * (255.0 * RGB_STEPS)).astype(np.uint16) * ok[..., None]
                enc_a = np.rint(np.clip(out[..., 3], 0, 1) * 65535.0).astype(np.uint16) * ok
                golden = np.concatenate([enc_rgb / RGB_STEPS, enc_a[..., None] / 65535.0], -1)
                e["gl"] = list(stats4(r64, golden, ok)[:3])
                data[f"{c['name']}_{eye}_rgb"], data[f"{c['name']}_{eye}_rgbf"] = (enc_rgb >> 1).astype(np.uint8), (enc_rgb & 1).astype(np.uint8)
                data[f"{c['name']}_{eye}_a"] = enc_a
                assert e["gl"][0] <= 0.10 and e["gl"][1] <= 0.5, (c["name"], eye, e["gl"])
            print(f"{c['name']} eye {eye} {ew}x{eh}: background {e['background']} blended {e['blended']} lam {e['lam_range'][0]:.2f}.."
                  f"{e['lam_range'][1]:.2f} under the look > 0.5: {e['lam_gt_half']} seam {e['seam']} excluded {excluded:.3f} | f32 vs f64 "
                  f"{['%.3g' % v for v in e['f32']]} | f64 vs GL {['%.3g' % v for v in e.get('gl', [])]}", flush=True)
            crec["eyes"].append(e)
        assert n_blend >= 2000, (c["name"], "blended", n_blend)
        assert n_lam >= c.get("min_lam", 0) and n_seam >= c.get("min_seam", 0), (c["name"], n_lam, n_seam)
        if c.get("clamp"):
            assert n_clamp >= 100, (c["name"], n_clamp)
        if render:
            for t in (t_lin, t_dep, t_pano, t_src):
                gl.delete_texture(t)
        del crec["strip"]
        meta["cases"].append(crec)
    if not render:
        return meta
    np.savez_compressed(os.path.join(HERE, "xr_panorama_curved.npz"), **data)
    with open(os.path.join(HERE, "xr_panorama_curved.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote xr_panorama_curved", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "xr_panorama_curved.npz")), "bytes")


if __name__ == "__main__":
    main(render="--check" not in sys.argv[1:])
