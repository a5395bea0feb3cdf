"""The panorama background behind the CURVED OpenXR screen's glow, glow2, veil and frosted looks (d2s_dibr_xr_eyes_panorama_curved)
restated in numpy, composed from the existing restatements: xr_panorama_ref (the panorama pass and its 2 x 2 quad LOD),
xr_glow_curved_ref (the band mesh around the curved strip) and xr_frost_curved_ref (the 196 wall triangles after it).

xr_panorama_ref.case_render's construction with a curved base.  Every blend of _render_eye is ONE, ONE_MINUS_SRC_ALPHA, so the eye
image is affine in what it started from: final = S + background * K, K the product of the (1 - alpha) of what drew over an uncovered
pixel (0 under the screen, which overwrites).  The case is rendered over clear (0, 0, 0, 0) and over (1, 1, 1, 1) by the look's own
restatement; S is the first, K the difference of the two alphas.

A manifest case (tests/golden/xr_panorama_curved.json) carries kind "glow_curved" or "frost_curved", the panorama's settings, and per
eye the (proj, view) pair and the uniforms the reference recorded, as xr_panorama.json's cases do.  A glow case also carries the
fields xr_glow_curved_ref.case_render reads (mode, range_m, inner_edge_fraction, strip, draw); a frost case carries frost and, put back
from the .npz by load(), strip.
"""
import json
import os

import numpy as np

import xr_frost_curved_ref as FC
import xr_glow_curved_ref as GC
import xr_glow_ref as R
import xr_panorama_ref as P

uniform3x3 = R.uniform3x3
synth_panorama = P.synth_panorama


def _base(c, e, clear, img, dep, levels, verts, T, lib):
    """The eye image of case c over a constant clear colour -> (framebuffer, class, covered).  lib False: the float64 rasteriser of the
    RECORDED triangles (verts) behind the recorded strip; lib True: the kernel's own search / walk over the library's geometry, in T."""
    cc = dict(c, clear=list(clear))
    if c["kind"] == "glow_curved":
        if lib:
            out, cls = GC.case_search(cc, e, img, dep, levels, T)
        else:
            out, cls = GC.case_render(cc, e, verts, img, dep, levels, T)
        return out, cls, (cls == GC.SCREEN) | (cls == GC.SCREEN_INNER)
    assert c["kind"] == "frost_curved", c["kind"]
    out, cls, info = FC.case_render(cc, e, img, dep, levels, None if lib else verts, T)
    return out, cls, info["covered"]


def case_render(c, e, img, dep, levels, pano_levels, verts=None, T=np.float64, lib=False):
    """A manifest case's eye -> (framebuffer [h, w, 4] T: rgb 0..255, alpha 0..1; class [h, w]; info dict(covered, lam, seam, bg, K)).
    lib False: float64 over the reference's recorded mesh and matrices; lib True: the library's geometry and, with T float32, the
    kernel's arithmetic for the search, the walk and the panorama."""
    w, h = e["size"]
    out0, cls, cov = _base(c, e, (0.0, 0.0, 0.0, 0.0), img, dep, levels, verts, T, lib)
    out1, _, _ = _base(c, e, (1.0, 1.0, 1.0, 1.0), img, dep, levels, verts, T, lib)
    K = (out1[..., 3] - out0[..., 3]).astype(T)
    bg = P.background(pano_levels, P.case_coord(c, e, lib), w, h, c["panorama"]["exposure"], T)
    bg4 = np.concatenate([bg["rgb"], np.ones((h, w, 1), T)], -1)
    out = (out0 + bg4 * K[..., None]).astype(T)
    return out, cls, dict(covered=cov, lam=bg["lam"], seam=bg["seam"], bg=bg["rgb"], K=K)


def case_scene(c):
    """(frame rgb, depth, panorama) of a manifest case."""
    from desktop2stereo_amd import synth
    H, W = c["source"]
    img, dep = synth.dibr_scene(H, W, c["seed"], "boxes")
    ph, pw = c["panorama"]["size"]
    return img, dep, P.synth_panorama(ph, pw, c["panorama"]["seed"])


def load(golden_dir):
    """(npz, manifest) of tests/golden/xr_panorama_curved.*, each case given its recorded strip (<case>_strip of the .npz) as c["strip"]."""
    z = np.load(os.path.join(golden_dir, "xr_panorama_curved.npz"))
    with open(os.path.join(golden_dir, "xr_panorama_curved.json")) as f:
        meta = json.load(f)
    for c in meta["cases"]:
        c["strip"] = z[f"{c['name']}_strip"]
    return z, meta


golden_eye = P.golden_eye
