"""CPU: the restatement of the panorama background (tests/xr_panorama_ref.py) against the reference's own shader, drawn off-screen on
SwiftShader behind its screen, glow and walls (tests/golden/xr_panorama.npz, make_golden_xr_panorama.py).

  * Every case and eye, on the pixels whose 3 x 3 neighbourhood is of one region class (at most 10 % excluded): the float64 restatement
    is within the recorded bounds of the render, and the recorded bounds are what the glow's test demands -- at most 10 % of the rgb
    values beyond 1 level, a mean of at most half a level.  A rule that cannot meet that is wrong; the bound is not.
  * The quad rule matters: on the seam and the minified case a per-pixel analytic-derivative LOD lies further from the render than the
    renderer's 2 x 2 quad rule -- on the pixels of the quads the u seam crosses by a wide margin (the analytic derivative knows no
    seam; the renderer's forward difference of fract(u) does, and takes the coarsest levels there).
  * The fixtures contain what they are for: lambda > 0.5 in the minified cases, seam quads in the seam case, 0 and 255 after the
    exposure clamp."""
import json
import os

import numpy as np
import pytest

import xr_glow_ref as R
import xr_panorama_ref as P

CASES = ["magnified", "minified", "seam", "pole", "yaw_exposure_flip", "odd_panorama", "flip_odd_height", "asymmetric_two_sizes", "glow_flat",
         "veil_flat", "frosted_flat", "curved_plain"]


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_panorama.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_panorama.npz")), json.load(f)


_SCENES = {}


def _scene(c):
    """(frame, depth, the frame's chain, the panorama's chain) of a case, once per module."""
    if c["name"] not in _SCENES:
        img, dep, pano = P.case_scene(c)
        _SCENES[c["name"]] = (img, dep, R.chain(img), R.chain(pano))
    return _SCENES[c["name"]]


def _case(fixtures, name):
    return next(c for c in fixtures[1]["cases"] if c["name"] == name)


def _stats(a, b, ok):
    d = np.abs(a[..., :3] - b[..., :3])[ok]
    return float((d > 1).mean()), float(d.mean()), float(np.abs(a[..., 3] - b[..., 3])[ok].max())


def test_manifest_names_the_renderer_and_the_cases(fixtures):
    z, meta = fixtures
    assert [c["name"] for c in meta["cases"]] == CASES
    assert "SwiftShader" in meta["gl"]["renderer"] and "OpenGL ES 3.0" in meta["gl"]["version"]
    assert meta["es300_patches"]["_PANORAMA_FRAG"] and "_PANORAMA_FRAG" in meta["shader"]
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "xr_panorama.npz")) < 1 << 20
    kinds = {c["name"]: (c["kind"], c["screen"]["curve"]) for c in meta["cases"]}
    assert kinds["glow_flat"] == ("glow", "flat") and kinds["veil_flat"][0] == kinds["frosted_flat"][0] == "frost"
    assert kinds["curved_plain"] == ("plain", "horizontal")
    sizes = {tuple(e["size"]) for c in meta["cases"] for e in c["eyes"]}
    assert (130, 101) in sizes and (111, 87) in sizes
    assert _case(fixtures, "flip_odd_height")["eye_flip"] and _case(fixtures, "odd_panorama")["panorama"]["size"] == [562, 1000]
    for c in meta["cases"]:
        for e in c["eyes"]:
            assert e["min_seam_distance"] > 1e-5 and e["min_pole_distance"] > 1e-6, (c["name"], e["eye"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_render(fixtures, name):
    z, _ = fixtures
    c = _case(fixtures, name)
    img, dep, levels, pano_levels = _scene(c)
    verts = z[f"{name}_verts"] if c["kind"] == "frost" else None
    for e in c["eyes"]:
        r64, cls, info = P.case_render(c, e, img, dep, levels, pano_levels, verts)
        ok = P.uniform3x3(cls)
        assert 1.0 - ok.mean() <= 0.10, (name, e["eye"], 1.0 - ok.mean())
        assert abs((1.0 - ok.mean()) - e["excluded"]) < 1e-9
        golden = P.golden_eye(z, c, e["eye"])
        assert not golden[~ok].any() and golden[ok][:, 3].min() > 0
        share, mean, amax = _stats(r64, golden, ok)
        print(f"\n[panorama restatement vs render, {name} eye {e['eye']}] beyond 1 level {share:.4f} mean {mean:.4f} alpha max {amax:.2e} "
              f"(recorded {e['gl']}); background {int((ok & ~info['covered']).sum())} px")
        assert e["gl"][0] <= 0.10 and e["gl"][1] <= 0.5
        assert share <= e["gl"][0] + 1e-6 and mean <= e["gl"][1] + 1e-6 and amax <= e["gl"][2] + 1e-6, (name, e["eye"], share, mean, amax, e["gl"])
        assert (ok & ~info["covered"]).sum() >= 2000 and int((ok & ~info["covered"]).sum()) == e["background"]


@pytest.mark.parametrize("name", ["seam", "minified"])
def test_the_quad_rule_is_nearer_the_render_than_a_per_pixel_derivative(fixtures, name):
    z, _ = fixtures
    c = _case(fixtures, name)
    img, dep, levels, pano_levels = _scene(c)
    for e in c["eyes"]:
        quad, cls, info = P.case_render(c, e, img, dep, levels, pano_levels)
        pixel, _, pinfo = P.case_render(c, e, img, dep, levels, pano_levels, rule="pixel")
        golden = P.golden_eye(z, c, e["eye"])
        bg = P.uniform3x3(cls) & ~info["covered"]
        dq, dp = np.abs(quad[..., :3] - golden[..., :3]), np.abs(pixel[..., :3] - golden[..., :3])
        print(f"\n[quad rule vs per-pixel derivative, {name} eye {e['eye']}] background mean |diff| {dq[bg].mean():.4f} vs {dp[bg].mean():.4f} level; "
              f"lambda differs by up to {np.abs(info['lam'] - pinfo['lam'])[bg].max():.2f}")
        assert dq[bg].mean() < dp[bg].mean(), (name, e["eye"])
        # where the two rules agree both means are the stored half-level steps' rounding (0.125): the values on which they disagree
        # by more than 0.05 level say which one the renderer follows
        differ = bg[..., None] & (np.abs(quad[..., :3] - pixel[..., :3]) > 0.05)
        print(f"    values the rules disagree on by > 0.05 level: {int(differ.sum())}, mean |diff| {dq[differ].mean():.4f} vs {dp[differ].mean():.4f} level")
        assert differ.sum() >= 100 and dq[differ].mean() < dp[differ].mean(), (name, e["eye"])
        if name == "seam":
            sm = bg & info["seam"]
            print(f"    seam-quad pixels: {int(sm.sum())}, mean |diff| {dq[sm].mean():.3f} vs {dp[sm].mean():.3f} level")
            assert sm.sum() >= 60 and 4.0 * dq[sm].mean() < dp[sm].mean(), (e["eye"], dq[sm].mean(), dp[sm].mean())


def test_fixtures_contain_what_they_are_for(fixtures):
    z, meta = fixtures
    by = {c["name"]: c for c in meta["cases"]}
    for name in ("minified", "curved_plain", "asymmetric_two_sizes"):
        for e in by[name]["eyes"]:
            assert e["lam_gt_half"] >= 0.9 * e["background"] >= 1800 and e["lam_range"][1] > 1.5, (name, e["eye"])
    for e in by["magnified"]["eyes"]:
        assert e["lam_gt_half"] == 0 and e["lam_range"] == [0.0, 0.0]
    for name in ("seam", "pole", "flip_odd_height"):
        for e in by[name]["eyes"]:
            assert e["seam"] >= 40 and e["lam_range"][1] > 9.0, (name, e["eye"])          # the seam quads take the coarsest levels (q = 10)
    for name in CASES:
        if name not in ("seam", "pole", "flip_odd_height"):
            assert all(e["seam"] == 0 for e in by[name]["eyes"]), name
    c = by["yaw_exposure_flip"]
    assert c["panorama"]["exposure"] == 1.7 and c["panorama"]["flip_y"] and c["panorama"]["yaw_offset_deg"] != 0.0
    img, dep, levels, pano_levels = _scene(c)
    lo = hi = False
    for e in c["eyes"]:
        golden = P.golden_eye(z, c, e["eye"])
        r64, cls, info = P.case_render(c, e, img, dep, levels, pano_levels)
        bg = P.uniform3x3(cls) & ~info["covered"]
        lo |= bool((golden[..., :3][bg] == 0).any()) and bool((r64[..., :3][bg] == 0).any())
        hi |= bool((golden[..., :3][bg] == 255).any()) and bool((r64[..., :3][bg] == 255).any())
    assert lo and hi


def test_float32_emulation_is_within_its_recorded_maximum(fixtures):
    """The bound the GPU test doubles: the float32 emulation of the kernel over the library's own geometry against the float64
    restatement, recomputed here for one plain, one look and the seam case."""
    z, _ = fixtures
    for name in ("minified", "seam", "veil_flat"):
        c = _case(fixtures, name)
        img, dep, levels, pano_levels = _scene(c)
        verts = z[f"{name}_verts"] if c["kind"] == "frost" else None
        for e in c["eyes"]:
            r64, cls, _ = P.case_render(c, e, img, dep, levels, pano_levels, verts)
            r32, _, _ = P.case_render(c, e, img, dep, levels, pano_levels, verts, np.float32, lib=True)
            ok = P.uniform3x3(cls)
            d = np.abs(r32[..., :3].astype(np.float64) - r64[..., :3])[ok]
            assert abs(d.max() - e["f32"][3]) <= 1e-9 + 1e-6 * e["f32"][3] and d.max() < 0.05, (name, e["eye"], d.max(), e["f32"])
