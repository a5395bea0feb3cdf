"""Golden vectors for the viewer's composite display modes: the REFERENCE's own DEPTH_FRAGMENT, ANAGLYPH_FRAGMENT,
INTERLEAVED_FRAGMENT and VERTICAL_INTERLEAVED_FRAGMENT programs (viewer.py:633-1197), read from the reference checkout
(gl_harness.REF_VIEWER) at generation time,
compiled as OpenGL ES 3.0 and run off-screen on SwiftShader (gl_harness.py) in the build container.

    python tests/golden/make_golden_composite.py        # -> tests/golden/composite.npz + composite.json

The shader text is read with `ast` and never stored.  ES patches: gl_harness.to_es300()'s four, plus one more for ANAGLYPH and
VERTICAL_INTERLEAVED (`search_dir * i * pixel_size.x` is int * float, which ES does not convert): listed in the manifest.
Each case draws the viewer's full-screen quad with the program's uniforms as viewer.py:2604-2662 sets them (u_eye_offset =
+ipd_uv / 2, u_depth_strength = 0.1 * depth_ratio, blending off) through glViewport(x, y, w, h) into an RGBA32F target of
(x + w) x (y + h) -- gl_FragCoord counts from the window origin, so the viewport offset decides which eye an interleaved row /
column shows -- and keeps the h x w viewport: rgb * 255 * 256 and alpha * 65535 as uint16, like dibr.npz (every `row_stride`-th
row).  u_resolution is set to the source size, except in the `as_shipped_*` cases, which leave it at (0, 0) as the reference does
(recorded, not a target; include/d2s.h).  Inputs are regenerated from seeds through desktop2stereo_amd.synth.dibr_scene.
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

PROGRAMS = {"Depth Map": "DEPTH_FRAGMENT", "Anaglyph": "ANAGLYPH_FRAGMENT", "Interleaved": "INTERLEAVED_FRAGMENT",
            "Interleaved-V": "VERTICAL_INTERLEAVED_FRAGMENT"}
# the one patch beyond gl_harness.to_es300(): ES has no implicit int -> float in `search_dir * i * pixel_size.x`
EXTRA_PATCHES = [("search_dir * i * pixel_size.x", "float(search_dir * i) * pixel_size.x")]

WARP = ("Anaglyph", "Interleaved", "Interleaved-V")
BASE = dict(ipd_uv=0.064, depth_ratio=4.0, convergence=0.0)
# (name, mode, h, w, seed, scene kind, row stride of stored outputs, viewport (x, y, w, h) in window pixels or None = (0, 0, w, h), uniforms)
CASES = []
for k, m in enumerate(WARP):
    t = m.lower().replace("-", "_")
    CASES += [
        (f"{t}_boxes", m, 48, 88, 20 + k, "boxes", 1, None, dict(BASE)),
        (f"{t}_roll", m, 48, 88, 23 + k, "boxes", 1, None, dict(BASE, roll=0.2)),
        (f"{t}_conv", m, 48, 80, 26 + k, "boxes", 1, None, dict(BASE, depth_ratio=2.0, convergence=0.3)),
        (f"{t}_feather", m, 48, 80, 29 + k, "boxes", 1, (2, 2, 80, 48), dict(BASE, convergence=0.1, feather=True, feather_width=0.08,
                                                                             corner_radius=0.06)),
        (f"{t}_odd", m, 48, 80, 20 + k, "boxes", 1, (3, 1, 80, 48), dict(BASE)),          # odd (x, y): row / column parity flips
        (f"{t}_even", m, 48, 80, 20 + k, "boxes", 1, (2, 4, 80, 48), dict(BASE)),
        (f"{t}_up2", m, 30, 52, 32 + k, "boxes", 1, (0, 0, 104, 60), dict(BASE)),            # a panel with twice the source's pixels
        (f"{t}_down", m, 64, 112, 35 + k, "smooth", 1, (5, 2, 80, 45), dict(BASE, depth_ratio=2.0)),
        (f"{t}_hd", m, 1080, 1920, 38 + k, "boxes", 180, None, dict(BASE)),
    ]
CASES += [
    ("depth_map_smooth", "Depth Map", 48, 88, 41, "smooth", 1, None, {}),
    ("depth_map_up2", "Depth Map", 30, 52, 42, "boxes", 1, (1, 3, 104, 60), {}),
    ("depth_map_down", "Depth Map", 64, 112, 43, "smooth", 1, (0, 0, 80, 45), {}),
    ("depth_map_hd", "Depth Map", 1080, 1920, 44, "smooth", 180, None, {}),
]
# The reference AS SHIPPED (u_resolution never assigned: pixel_size = 1 / 0, taps at non-finite coordinates, undefined in GL): what
# SwiftShader renders for that state is recorded, not a target.
CASES += [(f"as_shipped_{m.lower().replace('-', '_')}", m, 48, 88, 20 + k, "boxes", 1, None, dict(BASE, as_shipped=True))
          for k, m in enumerate(WARP)]


def reference_programs():
    """{constant name: (text, first line, last line)} of the four programs in the reference's viewer.py, read with ast."""
    import gl_harness as G
    with open(G.REF_VIEWER) as f:
        tree = ast.parse(f.read())
    out = {}
    for n in tree.body:
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name) \
                and n.targets[0].id in PROGRAMS.values() and isinstance(n.value, ast.Constant):
            out[n.targets[0].id] = (n.value.value, n.lineno, n.end_lineno)
    assert set(out) == set(PROGRAMS.values()), set(PROGRAMS.values()) - set(out)
    return out


def render(mode, path):
    """The cases of one program, rendered in a process of their own (SwiftShader stalled on the second program of a context that
    had run another with many in-painted fragments) -> an npz + json pair at `path`."""
    import gl_harness as G
    from desktop2stereo_amd import synth
    (vs, _, _), _ = G.reference_shaders()
    vs2, _ = G.to_es300(vs)
    gl = G.Gles()
    progs, defaults, lines = {}, {}, {}
    for name in (PROGRAMS[mode],):
        text, l0, l1 = reference_programs()[name]
        fs, dflt = G.to_es300(text)
        for a, b in EXTRA_PATCHES:
            fs = fs.replace(a, b)
        progs[mode], defaults[mode], lines[mode] = gl.program(vs2, fs), dflt, f"viewer.py:{l0}-{l1} ({name})"
    data = {}
    meta = {"cases": [], "gl": {"version": gl.version, "renderer": gl.renderer}, "programs": lines,
            "es_patches": "gl_harness.to_es300() (its docstring: #version, uniform initialisers, global pixel_size, int * float in "
                          "`dy * pixel_size.y` / `x * pixel_size.x`) + " + "; ".join(f"`{a}` -> `{b}`" for a, b in EXTRA_PATCHES),
            "uniform_defaults_from_the_shader_text": defaults,
            "encoding": "<case>_rgb = uint16 rint(frag_color.rgb * 255 * 256); <case>_a = uint16 rint(frag_color.a * 65535); "
                        "rows 0.. = top of the viewport, every row_stride-th"}
    for name, m, h, w, seed, kind, rs, vp, u in CASES:
        if m != mode:
            continue
        img, dep = synth.dibr_scene(h, w, seed, kind)
        tc, td = gl.texture(img, 0), gl.texture(dep, 1)
        x, y, ow, oh = vp or (0, 0, w, h)
        uni = dict(tex_color=0, tex_depth=1, u_resolution=(0.0, 0.0) if u.get("as_shipped") else (float(w), float(h)),
                   u_eye_offset=float(u.get("ipd_uv", 0.064) / 2.0), u_depth_strength=float(0.1 * u.get("depth_ratio", 1.0)),
                   u_convergence=float(u.get("convergence", 0.0)), u_roll=float(u.get("roll", 0.0)),
                   u_feather_enabled=int(bool(u.get("feather", False))), u_feather_width=float(u.get("feather_width", 0.02)),
                   u_viewport=(float(x), float(y), float(ow), float(oh)), **{k: float(v) for k, v in defaults[mode].items()})
        if "corner_radius" in u:
            uni["u_corner_radius"] = float(u["corner_radius"])
        out = gl.render(progs[mode], uni, x + ow, y + oh, viewport=(x, y, ow, oh))[:oh, x:x + ow]
        assert np.isfinite(out).all()
        data[f"{name}_rgb"] = np.rint(np.clip(out[::rs, :, :3], 0, 1) * (255.0 * 256.0)).astype(np.uint16)
        data[f"{name}_a"] = np.rint(np.clip(out[::rs, :, 3], 0, 1) * 65535.0).astype(np.uint16)
        gl.delete_texture(tc)
        gl.delete_texture(td)
        meta["cases"].append(dict(name=name, mode=mode, h=h, w=w, seed=seed, scene=kind, row_stride=rs,
                                  viewport=[x, y, ow, oh], **u))
        print("rendered", name, mode, (oh, ow))
    np.savez(path + ".npz", **data)
    with open(path + ".json", "w") as f:
        json.dump(meta, f)


def main():
    import subprocess
    import tempfile
    data, meta = {}, None
    with tempfile.TemporaryDirectory() as tmp:
        for k, mode in enumerate(PROGRAMS):
            path = os.path.join(tmp, str(k))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--render", mode, path], check=True)
            with np.load(path + ".npz") as z:
                data.update({n: z[n] for n in z.files})
            with open(path + ".json") as f:
                part = json.load(f)
            if meta is None:
                meta = dict(part, cases=[], programs={}, uniform_defaults_from_the_shader_text={})
            meta["programs"].update(part["programs"])
            meta["uniform_defaults_from_the_shader_text"].update(part["uniform_defaults_from_the_shader_text"])
            meta["cases"] += part["cases"]
    order = [c[0] for c in CASES]
    meta["cases"].sort(key=lambda c: order.index(c["name"]))
    np.savez_compressed(os.path.join(HERE, "composite.npz"), **{n: data[n] for n in sorted(data)})
    with open(os.path.join(HERE, "composite.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote composite", len(data), "arrays")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--render"]:
        render(sys.argv[2], sys.argv[3])
    else:
        main()
