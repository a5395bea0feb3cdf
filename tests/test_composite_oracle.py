"""The CPU restatement of the viewer's composite programs (tests/composite_ref.py) against renders of the REFERENCE's own shader text
(tests/golden/composite.npz: ANAGLYPH / INTERLEAVED / VERTICAL_INTERLEAVED / DEPTH_FRAGMENT, viewer.py:633-1197, compiled as OpenGL
ES 3.0 and run off-screen on SwiftShader, tests/golden/make_golden_composite.py).  frag_color.rgb and frag_color.a separately.

Tolerances are f1's (tests/test_oracle_golden.py): GL_LINEAR filters RGB8 with 8-bit sub-texel weights where the restatement filters
in float32 -> every value within 1 level on the small cases; at 1920 columns the programs' hard thresholds flip isolated pixels on a
1-ulp coordinate difference -> >= 99.9 % within 1 level, mean <= 0.06 (Anaglyph: 0.08 -- its disocclusion test is a hard
`jump > 0.08` for both eyes at once, with no soft ramp; measured 0.069); alpha within 1e-3."""
import json
import os

import numpy as np
import pytest

from composite_ref import composite_frag


HD_MEAN = {"Anaglyph": 0.08, "Interleaved": 0.06, "Interleaved-V": 0.06, "Depth Map": 0.06}


def _cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "composite.npz"))
    with open(os.path.join(golden_dir, "composite.json")) as f:
        meta = json.load(f)
    return z, meta


def _run(c):
    from desktop2stereo_amd import synth
    img, dep = synth.dibr_scene(c["h"], c["w"], c["seed"], c["scene"])
    kw = dict(ipd_uv=c.get("ipd_uv", 0.064), depth_ratio=c.get("depth_ratio", 1.0), convergence=c.get("convergence", 0.0),
              viewport=tuple(c["viewport"]), roll=c.get("roll", 0.0), feather=c.get("feather", False),
              feather_width=c.get("feather_width", 0.02), corner_radius=c.get("corner_radius", 0.0))
    return composite_frag(img, dep, c["mode"], **kw)


def test_fixture_manifest(golden_dir):
    z, meta = _cases(golden_dir)
    assert "SwiftShader" in meta["gl"]["renderer"]
    assert "float(search_dir * i) * pixel_size.x" in meta["es_patches"]
    modes = {c["mode"] for c in meta["cases"]}
    assert modes == {"Anaglyph", "Interleaved", "Interleaved-V", "Depth Map"}
    for c in meta["cases"]:
        x, y, w, h = c["viewport"]
        assert z[c["name"] + "_rgb"].shape == (len(range(0, h, c["row_stride"])), w, 3)


@pytest.mark.parametrize("mode", ["Anaglyph", "Interleaved", "Interleaved-V", "Depth Map"])
def test_restatement_matches_reference_renders(golden_dir, mode):
    z, meta = _cases(golden_dir)
    saw_alpha, n = False, 0
    for c in meta["cases"]:
        if c["mode"] != mode:
            continue
        o = _run(c)[::c["row_stride"]]
        rgb = z[c["name"] + "_rgb"].astype(np.float32) / 256.0
        a = z[c["name"] + "_a"].astype(np.float32) / 65535.0
        d = np.abs(o[..., :3] - rgb)
        if c.get("as_shipped"):
            print(f"[{mode} restatement vs the as-shipped render (u_resolution = 0), {c['name']}] rgb max {d.max():.1f} "
                  f"mean {d.mean():.3f}, {(d.max(-1) > 1).mean():.3f} of the pixels beyond 1 level")
            continue
        n += 1
        assert np.abs(o[..., 3] - a).max() <= 1e-3, (c["name"], float(np.abs(o[..., 3] - a).max()))
        saw_alpha |= bool(a.min() < 0.9)
        if c["w"] <= 320:
            assert d.max() <= 1.0, (c["name"], float(d.max()))
        else:
            assert (d <= 1.0).mean() >= 0.999 and d.mean() <= HD_MEAN[mode], (c["name"], float((d > 1).mean()), float(d.mean()))
    assert n >= 3
    assert saw_alpha or mode == "Depth Map"


def test_renders_are_not_vacuous(golden_dir):
    """The fixtures show what the modes are about: interleaved rows / columns differ, Anaglyph's red eye differs from its cyan
    eye, an odd viewport offset swaps the eyes."""
    from desktop2stereo_amd import synth
    z, meta = _cases(golden_dir)
    rgb = {c["name"]: z[c["name"] + "_rgb"].astype(np.float32) / 256.0 for c in meta["cases"]}
    assert np.abs(rgb["interleaved_boxes"][0::2] - rgb["interleaved_boxes"][1::2]).max() > 20
    assert np.abs(rgb["interleaved_v_boxes"][:, 0::2] - rgb["interleaved_v_boxes"][:, 1::2]).max() > 20
    # Anaglyph: R comes from the left eye, G / B from the right; with the same source pixel R and G would follow one another
    a = rgb["anaglyph_boxes"]
    c = next(c for c in meta["cases"] if c["name"] == "anaglyph_boxes")
    img, _ = synth.dibr_scene(c["h"], c["w"], c["seed"], c["scene"])
    assert np.abs(a[..., 0] - img[..., 0]).max() > 20 and np.abs(a[..., 1] - img[..., 1]).max() > 20
    # the odd (x, y) viewport shows the other eye on every row / column than the even one (same frame, same viewport size)
    for m, ax in (("interleaved", 0), ("interleaved_v", 1)):
        odd, even = rgb[f"{m}_odd"], rgb[f"{m}_even"]
        assert np.abs(odd - even).max() > 20, m
        p = _run(next(c for c in meta["cases"] if c["name"] == f"{m}_odd"))
        q = _run(dict(next(c for c in meta["cases"] if c["name"] == f"{m}_odd"), viewport=[2, 4, 80, 48]))
        assert np.abs(p[..., :3] - q[..., :3]).max() > 20
    assert min(float((z[c["name"] + "_a"] / 65535.0).min()) for c in meta["cases"] if not c.get("as_shipped")) < 0.9
