"""CPU: the restatement tests/xr_frost_curved_ref.py (the veil and frosted walls around the curved OpenXR screen) against what the
reference's own code draws -- its one TRIANGLES draw of 588 vertices after its curved strip, per eye, on SwiftShader, recorded by
tests/golden/make_golden_xr_frost_curved.py in xr_frost_curved.npz / xr_frost_curved.json.  The GPU test holds the kernel to this
restatement (tests/test_gpu_xr_frost_curved.py); this file holds the restatement to the reference, as tests/test_xr_frost_oracle.py
does for the flat screen.
  * Compared: the stored pixels -- class (screen / each wall's hit count / noise cells) uniform on 3 x 3 and covered by a triangle.
    The issue's caps: per eye at most 15 % of the image excluded; per drawing case >= 500 compared wall pixels; the outside case >= 50
    compared two-wall and >= 50 wall-over-screen pixels; the near case >= 300 pixels the near plane cuts; the end case >= 200 compared
    pixels on an end wall; both curves among the veil and among the frosted cases.
  * Bounds: the figures the generator measured for the float64 rasteriser of the RECORDED triangles against the render (share of rgb
    values beyond 1 level, mean, alpha maximum): recorded + 1e-9, and below the flat fixture's caps -- share <= 0.10, mean <= 0.5 level,
    alpha <= 1e-3.
  * The library's rows walked in float64 ARE the recorded triangles: v_uv and t to 1e-5 (1e-6 away from the grazing near case)."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    import xr_frost_curved_ref as K
    return K.load(golden_dir)


@pytest.fixture(scope="module")
def renders(fixtures):
    """{(case, eye): (float64 restatement, class, info)}, computed once."""
    import xr_frost_curved_ref as K
    import xr_glow_ref as R
    z, meta = fixtures
    out = {}
    for c in meta["cases"]:
        img, dep = K.case_scene(c)
        levels = R.chain(img)
        for e in c["eyes"]:
            out[c["name"], e["eye"]] = K.case_render(c, e, img, dep, levels, z[f"{c['name']}_verts"])
    return out


def test_the_fixture_is_small_and_the_cases_are_the_issue_s(fixtures, golden_dir):
    z, meta = fixtures
    assert os.path.getsize(os.path.join(golden_dir, "xr_frost_curved.npz")) < 1 << 20
    by = {c["name"]: c for c in meta["cases"]}
    assert len(by) == 14
    drawn = [c for c in meta["cases"] if not c.get("empty")]
    for mode in (1, 2):
        assert {c["screen"]["curve"] for c in drawn if c["frost"]["mode"] == mode} == {"horizontal", "vertical"}
    assert {tuple(c["source"]) for c in meta["cases"]} == {(96, 160), (512, 1024), (562, 1000)}
    assert all(c["frost"]["noise_scale"] == 6.0 for c in meta["cases"] if c["frost"]["mode"] == 2)
    assert all(e["size"] == [130, 100] for c in meta["cases"] for e in c["eyes"] if c["name"] != "veil_h_oblique")
    assert by["veil_h_oblique"]["eyes"][1]["size"] == [111, 87]
    lay = by["veil_h_oblique"]["layout"]
    assert lay[1] > by["veil_h_oblique"]["screen"]["width"] / 2 and lay[2] > by["veil_h_oblique"]["screen"]["height"] / 2      # the front rectangle splays
    cc = by["veil_v_crop_corner"]
    assert cc["alpha_mode"] == "premultiplied" and cc["corner_radius"] > 0 and cc["clear"][:3] != [0, 0, 0] and cc["crop"] != [0.0, 0.0, 1.0, 1.0]
    assert float(np.linalg.norm(by["veil_h_outside"]["eye_shift"])) > 1.0
    assert by["frosted_v_time"]["frost"]["time"] == 3.7 and by["frosted_h_odd"]["source"] == [562, 1000]
    assert by["frosted_v_small_lod9"]["source"] == [96, 160] and by["frosted_v_small_lod9"]["frost"]["lod"] == 9.0 and by["frosted_h_dark"]["dim"] == 0.25
    assert by["frosted_v_empty"]["frost"]["intensity"] == 0.0 and by["veil_h_empty"]["frost"]["alpha"] == 0.002


def test_the_restated_eyes_are_within_the_recorded_bounds_of_the_renders(fixtures, renders):
    import xr_frost_curved_ref as K
    z, meta = fixtures
    for c in meta["cases"]:
        n_wall = n_two = n_over = n_cut = n_end = 0
        for e in c["eyes"]:
            want, cls, info = renders[c["name"], e["eye"]]
            ok = K.uniform3x3(cls)
            assert 1.0 - ok.mean() <= 0.15, (c["name"], e["eye"], 1.0 - ok.mean())
            nw, cov, cnt = info["n_walls"], info["covered"], info["counts"]
            counts = [int(((nw == 0) & ok).sum()), int(((nw == 1) & ok).sum()), int(((nw >= 2) & ok).sum()), int(((nw >= 1) & cov & ok).sum())]
            stored = ok & (nw > 0)
            assert counts == e["counts"] and int(stored.sum()) == e["stored"], (c["name"], counts, e["counts"])
            n_wall, n_two, n_over, n_cut = n_wall + counts[1] + counts[2], n_two + counts[2], n_over + counts[3], n_cut + e["cut"]
            n_end += int((((cnt[2] + cnt[3]) > 0) & ok).sum())
            g = K.golden_eye(z, c, e["eye"])
            assert not g[~stored].any()
            dd, da = np.abs(want[..., :3] - g[..., :3])[stored], np.abs(want[..., 3] - g[..., 3])[stored]
            share, mean, amax = e["gl"]
            print(f"[{c['name']} eye {e['eye']}] {int(stored.sum())} pixels: beyond 1 level {(dd > 1).mean():.3e} (recorded {share:.3e}) mean "
                  f"{dd.mean():.4f} ({mean:.4f}) max {dd.max():.2f} alpha max {da.max():.2e} ({amax:.2e})")
            assert (dd > 1).mean() <= share + 1e-9 and dd.mean() <= mean + 1e-9 and da.max() <= amax + 1e-9
            assert share <= 0.10 and mean <= 0.5 and amax <= 1e-3
        if not c.get("empty"):
            assert n_wall >= 500, (c["name"], n_wall)
        if c["name"] == "veil_h_outside":
            assert n_two >= 50 and n_over >= 50, (n_two, n_over)
        if c["name"] == "veil_h_near":
            assert n_cut >= 300, n_cut
        if c["name"] == "veil_h_end":
            assert n_end >= 200, n_end


def test_an_undrawn_look_leaves_the_would_be_wall_pixels_alone(fixtures, renders):
    """The two empty cases: the reference returns early; from inside the tube no wall lies over the screen, so the render shows the
    clear colour where the walls would lie."""
    import xr_frost_curved_ref as K
    z, meta = fixtures
    for name in ("frosted_v_empty", "veil_h_empty"):
        c = next(c for c in meta["cases"] if c["name"] == name)
        for e in c["eyes"]:
            _, cls, info = renders[name, e["eye"]]
            stored = K.uniform3x3(cls) & (info["n_walls"] > 0)
            g = K.golden_eye(z, c, e["eye"])[stored]
            assert stored.sum() >= 3000 and np.array_equal(g[:, :3], np.zeros_like(g[:, :3])) and np.all(g[:, 3] == 1.0)


def test_the_library_s_rows_are_the_recorded_triangles(fixtures):
    import xr_frost_curved_ref as K
    z, meta = fixtures
    worst = {}
    for c in meta["cases"]:
        if c.get("empty"):
            continue
        verts = z[f"{c['name']}_verts"]
        for e in c["eyes"]:
            w, h = e["size"]
            vp = np.array(e["vp"])
            mh = K.mesh_hits(verts, vp, w, h)
            wh = K.walk_hits(K.lib_rows(c["screen"], c["frost"]["head"], vp, w, h), w, h, np.float64)
            d = 0.0
            for k in range(K.TRIS):
                both, ia, ib = np.intersect1d(mh[k]["idx"], wh[k]["idx"], return_indices=True)
                assert mh[k]["idx"].size + wh[k]["idx"].size - 2 * both.size <= 0.02 * max(mh[k]["idx"].size, 50), (c["name"], e["eye"], k)
                for a in "uvt":
                    if both.size:
                        d = max(d, float(np.abs(mh[k][a][ia] - wh[k][a][ib]).max()))
            assert d <= max(e["walk"]) + 1e-12
            worst[c["name"]] = max(worst.get(c["name"], 0.0), d)
    print("library rows vs recorded triangles, max |v_uv|, |t|:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert all(v <= (1e-5 if k == "veil_h_near" else 1e-6) for k, v in worst.items()), worst
