"""CPU: the float64 restatement of the panorama behind the curved screen's looks (tests/xr_panorama_curved_ref.py) against the
reference's own shaders drawn off-screen in _render_eye's order (tests/golden/xr_panorama_curved.npz, make_golden_xr_panorama_curved.py)
-- every stored render within the figures the generator recorded -- and the fixture conditions, re-asserted from the manifest."""
import numpy as np
import pytest

import xr_glow_ref as R
import xr_panorama_curved_ref as PC

CASES = ["glow_h", "glow2_v", "glow_h_minified", "glow_h_seam_flip", "veil_h", "frosted_v", "veil_v_two_sizes", "frosted_h_yaw_exposure_flip"]


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return PC.load(golden_dir)


def test_the_manifest_holds_the_cases_and_their_fixture_conditions(fixtures):
    z, meta = fixtures
    cases = {c["name"]: c for c in meta["cases"]}
    assert list(cases) == CASES
    assert "SwiftShader" in meta["gl"]["renderer"]
    looks = {(c["kind"], c.get("mode", c.get("frost", {}).get("mode")), c["screen"]["curve"]) for c in cases.values()}
    assert {("glow_curved", 1, "horizontal"), ("glow_curved", 2, "vertical"), ("frost_curved", 1, "horizontal"), ("frost_curved", 2, "vertical"),
            ("frost_curved", 1, "vertical"), ("frost_curved", 2, "horizontal")} <= looks
    for c in cases.values():
        glow = c["kind"] == "glow_curved"
        assert len(c["eyes"]) == 2 and sum(e["blended"] for e in c["eyes"]) >= 2000, c["name"]
        for e in c["eyes"]:
            assert e["min_seam_distance"] > 1e-5 and e["min_pole_distance"] > 1e-6, (c["name"], e["eye"])
            assert e["excluded"] <= (0.10 if glow else 0.15), (c["name"], e["eye"], e["excluded"])
            assert e["size"][0] <= 130 and e["size"][1] <= 101 and e["gl"][0] <= 0.10 and e["gl"][1] <= 0.5
        assert c["panorama"]["size"][0] <= 1024 and c["panorama"]["size"][1] <= 2048 and c["source"] in ([96, 160], [256, 512])
        if glow:
            from desktop2stereo_amd import xr
            sc = xr.XrScreen(**c["screen"])
            assert all(sc.eye_inside(np.array(e["vp"])) for e in c["eyes"]), c["name"]
    c = cases["glow_h_minified"]
    assert c["panorama"]["size"] == [1024, 2048] and sum(e["lam_gt_half"] for e in c["eyes"]) >= 2000 and c["position"][1] < 0 and c["look"][1] > 0
    c = cases["glow_h_seam_flip"]
    assert c["eye_flip"] and all(e["size"][1] == 101 for e in c["eyes"]) and sum(e["seam"] for e in c["eyes"]) >= 40
    assert cases["veil_h"]["frost"]["intensity"] == 0.6 and cases["frosted_v"]["frost"]["noise_scale"] <= 3.0
    c = cases["veil_v_two_sizes"]
    assert [e["size"] for e in c["eyes"]] == [[130, 100], [111, 87]] and c["fov"][0] != c["fov"][1] and c["frost"]["head"] != [0.0, 0.0, 0.0]
    c = cases["frosted_h_yaw_exposure_flip"]
    p = c["panorama"]
    assert (p["yaw_offset_deg"], p["exposure"], p["flip_y"]) == (77.0, 1.7, True) and sum(e["clamped"] for e in c["eyes"]) >= 100


@pytest.mark.parametrize("name", CASES)
def test_the_float64_restatement_matches_the_stored_render(fixtures, name):
    z, meta = fixtures
    c = next(c for c in meta["cases"] if c["name"] == name)
    img, dep, pano = PC.case_scene(c)
    levels, pano_levels = R.chain(img), R.chain(pano)
    verts = z[f"{name}_verts"]
    for e in c["eyes"]:
        want, cls, info = PC.case_render(c, e, img, dep, levels, pano_levels, verts)
        ok = PC.uniform3x3(cls)
        assert abs((1.0 - ok.mean()) - e["excluded"]) < 1e-12
        golden = PC.golden_eye(z, c, e["eye"])
        d = np.abs(want[..., :3] - golden[..., :3])[ok]
        da = np.abs(want[..., 3] - golden[..., 3])[ok]
        share, mean, amax = float((d > 1).mean()), float(d.mean()), float(da.max())
        print(f"\n[{name} eye {e['eye']}] float64 restatement vs the render: beyond 1 level {share:.4f} (recorded {e['gl'][0]:.4f}) mean {mean:.4f} "
              f"({e['gl'][1]:.4f}) alpha max {amax:.2e} ({e['gl'][2]:.2e})")
        assert share <= e["gl"][0] + 1e-9 and mean <= e["gl"][1] + 1e-9 and amax <= e["gl"][2] + 1e-9
        bgm = ok & ~info["covered"]
        K = info["K"]
        assert int((bgm & (K > 0.05) & (K < 0.95)).sum()) == e["blended"] and int((bgm & info["seam"]).sum()) == e["seam"]
        assert int((bgm & (K < 0.95) & (info["lam"] > 0.5)).sum()) == e["lam_gt_half"]
        assert (golden[~ok] == 0).all()
