"""CPU: the restatement tests/xr_frost_ref.py (the veil and frosted walls around the flat OpenXR screen) against what the reference's own
code draws -- its four wall strips after its screen, per eye, on SwiftShader, recorded by tests/golden/make_golden_xr_frost.py in
xr_frost.npz / xr_frost.json.  The GPU test holds the kernel to this restatement (tests/test_gpu_xr_frost.py); this file holds the
restatement to the reference.
  * Compared: the stored pixels -- class (screen / covering walls / noise cells) uniform on 3 x 3 and covered by a wall's geometry.
    Per eye at most 15 % of the image is excluded by the class rule; per drawing case >= 500 wall pixels are compared; veil_outside
    has >= 50 compared two-wall and >= 50 wall-over-screen pixels; veil_near >= 300 pixels whose wall hit the near plane cuts.
  * Bounds: the figures the generator measured for the float64 restatement against the render (share of rgb values beyond 1 level,
    mean, alpha maximum), held as tests/test_xr_glow_oracle.py holds the glow's: recorded + 1e-9, and below the same caps -- share <=
    0.10, mean <= 0.5 level, alpha <= 1e-3.
  * The library's walk (grid cell, triangle, affine s) in float64 IS the recorded mesh: v_uv and t to 1e-6, while the analytic
    a / g(t) lies up to 5e-3 away -- the kernel follows the mesh."""
import json
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_frost.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_frost.npz")), json.load(f)


@pytest.fixture(scope="module")
def renders(fixtures):
    """{(case, eye): (float64 restatement, class, info, stored mask)}, computed once."""
    import xr_frost_ref as F
    import xr_glow_ref as R
    z, meta = fixtures
    out = {}
    for c in meta["cases"]:
        img, dep = F.case_scene(c)
        levels = R.chain(img)
        verts = z[f"{c['name']}_verts"]
        for e in c["eyes"]:
            want, cls, info = F.case_render(c, e, img, dep, levels, verts)
            out[c["name"], e["eye"]] = (want, cls, info, F.case_stored(c, e, verts, cls))
    return out


def test_the_fixture_is_small_and_the_cases_are_the_issue_s(fixtures, golden_dir):
    z, meta = fixtures
    assert os.path.getsize(os.path.join(golden_dir, "xr_frost.npz")) <= os.path.getsize(os.path.join(golden_dir, "xr_glow_curved.npz"))
    by = {c["name"]: c for c in meta["cases"]}
    assert len(by) == 14 and by["veil_front"]["source"] == [512, 1024] and by["veil_front"]["frost"]["head"] == [0.0, 0.0, 0.0]
    assert by["frosted_odd"]["source"] == [562, 1000] and by["frosted_small"]["source"] == [96, 160] and by["frosted_lod_high"]["source"] == [96, 160]
    assert by["frosted_lod_low"]["frost"]["lod"] == 0.5 and by["frosted_lod_high"]["frost"]["lod"] == 9.0 and by["frosted_time"]["frost"]["time"] == 3.7
    assert all(c["frost"]["noise_scale"] == 6.0 for c in meta["cases"] if c["frost"]["mode"] == 2)
    assert by["veil_crop_corner"]["alpha_mode"] == "premultiplied" and by["veil_crop_corner"]["corner_radius"] > 0 and by["veil_crop_corner"]["clear"][:3] != [0, 0, 0]
    assert by["frosted_empty"]["frost"]["intensity"] == 0.0 and by["veil_empty"]["frost"]["alpha"] == 0.002
    assert float(np.linalg.norm(by["veil_outside"]["eye_shift"])) > 0.65
    assert any(c["eyes"][0]["size"] != c["eyes"][1]["size"] for c in meta["cases"])
    assert all(e["size"] == [130, 100] for c in meta["cases"] for e in c["eyes"] if c["name"] != "veil_oblique")
    lay = by["veil_oblique"]["layout"]
    assert lay[1] > by["veil_oblique"]["screen"]["width"] / 2 and lay[2] > by["veil_oblique"]["screen"]["height"] / 2      # fx != 1 != fy


def test_the_restated_eyes_are_within_the_recorded_bounds_of_the_renders(fixtures, renders):
    import xr_frost_ref as F
    z, meta = fixtures
    for c in meta["cases"]:
        n_wall = n_two = n_over = n_cut = 0
        for e in c["eyes"]:
            want, cls, info, stored = renders[c["name"], e["eye"]]
            ok = F.uniform3x3(cls)
            assert 1.0 - ok.mean() <= 0.15, (c["name"], e["eye"], 1.0 - ok.mean())
            nw, cov = info["n_walls"], info["covered"]
            counts = [int(((nw == 0) & ok).sum()), int(((nw == 1) & ok).sum()), int(((nw >= 2) & ok).sum()), int(((nw >= 1) & cov & ok).sum())]
            assert counts == e["counts"] and int(stored.sum()) == e["stored"], (c["name"], counts, e["counts"])
            n_wall, n_two, n_over, n_cut = n_wall + counts[1] + counts[2], n_two + counts[2], n_over + counts[3], n_cut + e["cut"]
            g = F.golden_eye(z, c, e["eye"])
            assert not g[~stored].any()
            if not stored.any():
                continue
            dd, da = np.abs(want[..., :3] - g[..., :3])[stored], np.abs(want[..., 3] - g[..., 3])[stored]
            share, mean, amax = e["gl"]
            print(f"[{c['name']} eye {e['eye']}] {int(stored.sum())} pixels: beyond 1 level {(dd > 1).mean():.3e} (recorded {share:.3e}) mean "
                  f"{dd.mean():.4f} ({mean:.4f}) max {dd.max():.2f} alpha max {da.max():.2e} ({amax:.2e})")
            assert (dd > 1).mean() <= share + 1e-9 and dd.mean() <= mean + 1e-9 and da.max() <= amax + 1e-9
            assert share <= 0.10 and mean <= 0.5 and amax <= 1e-3      # the restatement IS the reference's walls, to the render's own texture filtering
        if c.get("empty"):
            assert n_wall == 0          # nothing drawn: the would-be wall pixels hold the clear colour or the screen
        else:
            assert n_wall >= 500, (c["name"], n_wall)
        if c["name"] == "veil_outside":
            assert n_two >= 50 and n_over >= 50, (n_two, n_over)
        if c["name"] == "veil_near":
            assert n_cut >= 300, n_cut


def test_an_undrawn_look_leaves_the_would_be_wall_pixels_alone(fixtures, renders):
    """frosted_empty (intensity 0) and veil_empty (alpha 0.002): the reference returns early; the render shows the clear colour where the
    walls would lie (from inside the tube no wall lies over the screen)."""
    z, meta = fixtures
    for name in ("frosted_empty", "veil_empty"):
        c = next(c for c in meta["cases"] if c["name"] == name)
        for e in c["eyes"]:
            import xr_frost_ref as F
            stored = renders[name, e["eye"]][3]
            g = F.golden_eye(z, c, e["eye"])[stored]
            assert stored.sum() >= 3000 and np.array_equal(g[:, :3], np.zeros_like(g[:, :3])) and np.all(g[:, 3] == 1.0)


def test_the_walk_is_the_recorded_mesh_and_the_analytic_shortcut_is_not(fixtures):
    import xr_frost_ref as F
    z, meta = fixtures
    worst_walk = worst_analytic = 0.0
    for c in meta["cases"]:
        if c.get("empty"):
            continue
        verts = z[f"{c['name']}_verts"].reshape(4, -1, 5)
        for e in c["eyes"]:
            w, h = e["size"]
            vp = np.array(e["vp"])
            mh = F.mesh_hits(verts, np.array(c["frost_model"]), vp, w, h)
            wh = F.walk_hits(F.wall_rows(c["screen"], c["frost"]["head"], vp, w, h), w, h, np.float64)
            for k in range(4):
                m = mh[k]["hit"] & wh[k]["hit"]
                assert (mh[k]["hit"] ^ wh[k]["hit"]).sum() <= 0.02 * max(int(mh[k]["hit"].sum()), 50), (c["name"], e["eye"], k)
                if m.any():
                    d = max(np.abs(mh[k]["u"] - wh[k]["u"])[m].max(), np.abs(mh[k]["v"] - wh[k]["v"])[m].max(), np.abs(mh[k]["t"] - wh[k]["t"])[m].max())
                    worst_walk = max(worst_walk, float(d))
                    worst_analytic = max(worst_analytic, float(np.abs(wh[k]["s_analytic"] - (mh[k]["v"] if k >= 2 else mh[k]["u"]))[m].max()))
    print(f"walk vs recorded mesh: max {worst_walk:.2e}; analytic a / g(t) vs mesh: max {worst_analytic:.2e}")
    assert worst_walk <= 1e-6          # float32 vertices and a float32 model matrix in the recording: a few 1e-7
    assert 1e-3 <= worst_analytic <= 1e-2          # at a 1024-wide source 5e-3 is five texels: the shortcut would show


def test_hash12_is_the_float32_order_the_renders_show(fixtures, renders):
    """The frosted cases agree with the renders only if SwiftShader's hash12 is the restatement's float32 order: a float64 hash moves n
    by up to 0.02 in most cells (and by ~1 where fract wraps), 0.30 * n of alpha."""
    import xr_frost_ref as F
    cx, cy = np.meshgrid(np.arange(-8.0, 64.0), np.arange(-8.0, 64.0))
    n32 = F.hash12(cx, cy).astype(np.float64)
    fr = lambda x: x - np.floor(x)
    x, y = fr(cx * 0.1031), fr(cy * 0.1031)
    d = x * (y + 33.33) + y * (x + 33.33) + x * (x + 33.33)
    n64 = fr((x + d + y + d) * (x + d))
    diff = np.minimum(np.abs(n32 - n64), 1.0 - np.abs(n32 - n64))
    assert n32.min() >= 0.0 and n32.max() < 1.0 and 1e-4 < diff.max() < 0.1          # the orders differ visibly, so the order matters
