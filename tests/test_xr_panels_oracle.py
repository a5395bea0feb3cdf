"""CPU: the restatement of the world-space panels (tests/xr_panels_ref.py) against renders of the reference's own shaders and its own
_render_fps_overlay / _render_keyboard state (tests/golden/xr_panels.npz, make_golden_xr_panels.py) -- no GPU, no library.

Per case and eye the float64 restatement runs over the render's own image after the screen pass and is held to the render after the
panels, on the pixels whose class (the screen's coverage plus the set of panels that pass) is uniform on 3 x 3 and that have no depth
near-tie.  The bound is the one the generator measured and wrote into the manifest, per case and eye (0.5 level for solid panels and
the opaque texture; up to 2.1 levels where a textured panel of alpha < 1 is blended: the manifest's generator says why)."""
import json
import os

import numpy as np
import pytest

import xr_eye_ref as X
import xr_panels_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "xr_panels.json")) as f:
    META = json.load(f)
CASES = {c["name"]: c for c in META["cases"]}
WANTED = ("front", "behind", "status", "status_faded_oblique", "solid_alpha", "keyboard", "two_writers", "two_no_write", "opaque", "curved",
          "half_off_behind_eye", "wrap_edge")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "xr_panels.npz"))


def images(z, name, eye):
    """(dst, final) as [h,w,4] float64: rgb in levels, alpha 0..1"""
    dst = z[f"{name}_{eye}_dst"]
    final = (dst.astype(np.int16) + z[f"{name}_{eye}_delta"].astype(np.int16)).astype(np.uint8)      # (mod 256)
    f = lambda a: np.concatenate([a[..., :3].astype(np.float64), a[..., 3:].astype(np.float64) / 255.0], -1)
    return f(dst), f(final), dst, final


def test_the_manifest_has_the_cases_and_records_the_wrap():
    assert set(WANTED) <= set(CASES)
    assert META["wrap"] == "repeat" and "no discard" in META["shader"] and "DEPTH_COMPONENT24" in META["target"]
    sizes = {tuple(e["size"]) for c in META["cases"] for e in c["eyes"]}
    assert any(w % 16 and h % 16 for w, h in sizes)
    assert any(c["eyes"][0]["size"] != c["eyes"][1]["size"] for c in META["cases"])
    kb = CASES["keyboard"]["panels"]
    assert [q["source"] for q in kb] == ["_render_keyboard"] * 3 and [q["depth_write"] for q in kb] == [False] * 3
    assert CASES["status"]["panels"][0]["depth_write"] is True and CASES["status_faded_oblique"]["panels"][0]["alpha"] == pytest.approx(0.15)
    assert os.path.getsize(os.path.join(HERE, "golden", "xr_panels.npz")) < 1 << 20


@pytest.mark.parametrize("name", WANTED)
def test_restatement_matches_the_render(golden, name):
    c = CASES[name]
    facets, panels, pics = X.case_facets(c), P.case_panels(c), P.case_textures(c)
    for e in c["eyes"]:
        w, h = e["size"]
        d64, g64, dst, final = images(golden, name, e["eye"])
        r64, info = P.render(d64, facets, np.array(e["vp"]), w, h, panels, pics, META["wrap"], np.float64)
        ok = P.compared(info)
        assert 1.0 - ok.mean() <= 0.15 and 1.0 - ok.mean() == pytest.approx(e["excluded"])
        assert int((ok & info["passed"].any(0)).sum()) == e["panel_pixels"] >= c["min_panel"]
        rgb = float(np.abs(r64[..., :3] - g64[..., :3])[ok].max())
        a = float(np.abs(r64[..., 3] - g64[..., 3])[ok].max() * 255.0)
        print(f"{name} eye {e['eye']}: rgb {rgb:.4f} alpha {a:.4f} levels (manifest {e['gl']})")
        assert rgb <= e["gl"][0] + 1e-9 and a <= e["gl"][1] + 1e-9
        # outside every panel's box the render itself changed nothing, and neither does the restatement
        boxes = [P.pixel_box(q["model"], np.array(e["vp"]), w, h) for q in panels]
        assert [list(b) if b else None for b in boxes] == e["boxes"]
        out = np.ones((h, w), bool)
        for b in boxes:
            if b:
                out[b[1]:b[3], b[0]:b[2]] = False
        assert (final[out] == dst[out]).all() and (r64[out] == d64[out]).all()


def test_solid_and_opaque_panels_are_within_the_targets_own_rounding():
    for name in ("solid_alpha", "opaque", "wrap_edge"):
        for e in CASES[name]["eyes"]:
            assert e["gl"][0] <= 0.8 and e["gl"][1] <= 0.51, (name, e["gl"])


def test_float32_emulation_is_where_the_manifest_says(golden):
    for name in ("front", "keyboard", "curved"):
        c = CASES[name]
        for e in c["eyes"]:
            w, h = e["size"]
            d64 = images(golden, name, e["eye"])[0]
            args = (d64, X.case_facets(c), np.array(e["vp"]), w, h, P.case_panels(c), P.case_textures(c), META["wrap"])
            r64, info = P.render(*args, np.float64)
            r32, _ = P.render(*args, np.float32)
            ok = P.compared(info)
            assert float(np.abs(r32[..., :3].astype(np.float64) - r64[..., :3])[ok].max()) == pytest.approx(e["f32"][0], rel=1e-6, abs=1e-12)
            assert e["f32"][0] < 0.01      # hundredths of a level at the most: rounding of the blend, never a flipped tap


def test_the_flip_and_the_wrap_are_what_the_render_has(golden):
    """Each wrong reading of the picture misses the render by tens of levels: rows bottom first, or the taps clamped at the edge."""
    c = CASES["wrap_edge"]
    e = c["eyes"][0]
    w, h = e["size"]
    d64, g64, _, _ = images(golden, "wrap_edge", 0)
    pics = P.case_textures(c)
    args = (d64, X.case_facets(c), np.array(e["vp"]), w, h, P.case_panels(c))
    _, info = P.render(*args, pics, "repeat")
    ok = P.compared(info) & info["passed"][0]
    for wrong_pics, wrap in (([p[::-1] for p in pics], "repeat"), (pics, "clamp")):
        r, _ = P.render(*args, wrong_pics, wrap)
        assert np.abs(r[..., :3] - g64[..., :3])[ok].max() > 20.0
