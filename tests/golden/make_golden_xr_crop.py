"""Golden vectors for the OpenXR screen's cropped DIBR warp: the REFERENCE's XR fragment shader -- the desktop FRAGMENT_SHADER
(viewer.py:386-631) passed through _make_xr_fragment_shader (xr_viewer/implementation.py:111-126), both read from the reference
checkout with `ast` at generation time -- compiled as OpenGL ES 3.0 and run off-screen on SwiftShader (gl_harness.py).

    python tests/golden/make_golden_xr_crop.py        # -> tests/golden/xr_crop.npz + xr_crop.json

_make_xr_fragment_shader is extracted as a function definition, compiled on its own and APPLIED to the text gl_harness.
reference_shaders() returns; neither text is stored.  Each case renders both eyes into the crop's eye viewport -- the pixel size of
_movie_crop_pixel_bounds (crop.py:165-173), halved for the Half-SBS case -- with u_source_crop = the crop, u_resolution = the source
size and u_viewport = the eye viewport, and stores frag_color as dibr.npz does (rgb * 255 * 256 and alpha * 65535 as uint16, every
`row_stride`-th row).  Inputs are regenerated from seeds (desktop2stereo_amd.synth.dibr_scene).
"""
from __future__ import annotations

import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
REF_XR = "/root/reference/xr_viewer/implementation.py"

BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0)
# (name, h, w, seed, scene kind, row stride, crop (x, y, w, h), "half" = a Half-SBS eye viewport, uniforms)
CASES = [
    ("xr_letterbox", 96, 160, 31, "boxes", 1, (0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0), False, dict(BASE)),
    # the OpenXR screen's state: rounded corners, frag_color.a kept (400 x 730, the pillarbox the detector finds on m730_noisy_lr;
    # every 13th row keeps the file under 1 MiB: rows 0 and 390 cross the 12-pixel corners, top and bottom)
    ("xr_pillarbox", 400, 730, 32, "boxes", 13, (0.1273972602739726, 0.0, 0.7575342465753425, 1.0), False, dict(BASE, corner_radius=0.03)),
    ("xr_both_roll", 90, 160, 33, "boxes", 1, (0.125, 0.2, 0.75, 0.6), False, dict(BASE, roll=0.2)),                 # the gather kernel
    ("xr_half_sbs", 96, 128, 34, "boxes", 1, (0.0, 0.125, 1.0, 0.75), True, dict(BASE, depth_ratio=2.0, convergence=0.2)),
    ("xr_right_edge", 90, 160, 35, "boxes", 1, (0.4, 0.1, 0.6, 0.8), False, dict(BASE)),                             # ends at u = 1.0
    ("xr_feather", 96, 160, 36, "boxes", 1, (0.05, 1.0 / 6.0, 0.9, 2.0 / 3.0), False,
     dict(BASE, convergence=0.1, feather=True, feather_width=0.08, corner_radius=0.06)),
    ("xr_hd_239", 1080, 1920, 37, "boxes", 45, (0.0, 0.13148148148148148, 1.0, 0.7351851851851852), False, dict(BASE)),
]


def xr_shader_patch():
    """_make_xr_fragment_shader of the reference (implementation.py:111-126) as a callable: the FunctionDef alone, compiled here."""
    with open(REF_XR) as f:
        tree = ast.parse(f.read())
    for n in tree.body:
        if isinstance(n, ast.FunctionDef) and n.name == "_make_xr_fragment_shader":
            ns = {}
            exec(compile(ast.Module(body=[n], type_ignores=[]), REF_XR, "exec"), ns)
            return ns[n.name], n.lineno, n.end_lineno
    raise RuntimeError("_make_xr_fragment_shader not found in " + REF_XR)


def pixel_bounds(w, h, crop):
    """_movie_crop_pixel_bounds of the reference (loaded by path; crop.py imports numpy alone)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_xr_crop", os.path.join(os.path.dirname(REF_XR), "crop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CropMixin()._movie_crop_pixel_bounds(w, h, crop)


def main():
    import gl_harness as G
    from desktop2stereo_amd import synth
    (vs, _, _), (fs, l0, l1) = G.reference_shaders()
    patch, p0, p1 = xr_shader_patch()
    xr = patch(fs)
    assert xr != fs and "u_source_crop" in xr
    vs2, _ = G.to_es300(vs)
    fs2, defaults = G.to_es300(xr)
    gl = G.Gles()
    prog = gl.program(vs2, fs2)
    data, meta = {}, {"cases": [], "gl": {"version": gl.version, "renderer": gl.renderer},
                      "shader": f"viewer.py:{l0}-{l1} (FRAGMENT_SHADER) through xr_viewer/implementation.py:{p0}-{p1} "
                                "(_make_xr_fragment_shader), ES 3.00 patches: see gl_harness.py",
                      "uniform_defaults_from_the_shader_text": defaults,
                      "encoding": "<case>_<eye>_rgb = uint16 rint(frag_color.rgb * 255 * 256); <case>_<eye>_a = uint16 rint(frag_color.a * 65535)"}
    for name, h, w, seed, kind, rs, crop, half, u in CASES:
        img, dep = synth.dibr_scene(h, w, seed, kind)
        tc, td = gl.texture(img, 0), gl.texture(dep, 1)
        x0, y0, x1, y1 = pixel_bounds(w, h, crop)
        ow, oh = ((x1 - x0) // 2 if half else x1 - x0), y1 - y0
        for eye, sign in (("left", -1.0), ("right", 1.0)):
            uni = dict(tex_color=0, tex_depth=1, u_resolution=(float(w), float(h)), u_eye_offset=float(sign * u["ipd_uv"] / 2.0),
                       u_depth_strength=float(0.1 * u["depth_ratio"]), u_convergence=float(u["convergence"]), u_roll=float(u.get("roll", 0.0)),
                       u_feather_enabled=int(bool(u.get("feather", False))), u_feather_width=float(u.get("feather_width", 0.02)),
                       u_viewport=(0.0, 0.0, float(ow), float(oh)), u_source_crop=tuple(float(c) for c in crop),
                       **{k: float(v) for k, v in defaults.items()})
            if "corner_radius" in u:
                uni["u_corner_radius"] = float(u["corner_radius"])
            out = gl.render(prog, uni, ow, oh)
            assert np.isfinite(out).all()
            data[f"{name}_{eye}_rgb"] = np.rint(np.clip(out[::rs, :, :3], 0, 1) * (255.0 * 256.0)).astype(np.uint16)
            data[f"{name}_{eye}_a"] = np.rint(np.clip(out[::rs, :, 3], 0, 1) * 65535.0).astype(np.uint16)
        gl.delete_texture(tc)
        gl.delete_texture(td)
        meta["cases"].append(dict(name=name, h=h, w=w, seed=seed, scene=kind, row_stride=rs, crop=list(crop), half_sbs=half,
                                  pixel_bounds=[int(x0), int(y0), int(x1), int(y1)], eye_w=int(ow), eye_h=int(oh), **u))
        print("rendered", name, (oh, ow))
    np.savez_compressed(os.path.join(HERE, "xr_crop.npz"), **data)
    with open(os.path.join(HERE, "xr_crop.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote xr_crop", len(data), "arrays")


if __name__ == "__main__":
    main()
