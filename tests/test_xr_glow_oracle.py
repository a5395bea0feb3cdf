"""CPU: the restatement tests/xr_glow_ref.py (the colour mip chain and the glow around the flat OpenXR screen) against what the
reference's own code draws -- glGenerateMipmap's levels and the glow passes around the screen on SwiftShader, recorded by
tests/golden/make_golden_xr_glow.py in xr_glow.npz / xr_glow_mips.npz / xr_glow.json.  The GPU tests hold the kernels to this
restatement (tests/test_gpu_xr_glow.py); this file holds the restatement to the reference.
  * the restated chain equals the render's levels EXACTLY on 1024 x 512 (every step a 2 x 2 box);
  * on 1000 x 562 (steps from odd sizes), each stored level formed in one step from the render's own level above it differs by at
    most 1, on a share no larger than twice what the generator measured for that level;
  * the restated eyes are within the recorded float64-against-render bounds."""
import json
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_glow.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(golden_dir, "xr_glow.npz")), np.load(os.path.join(golden_dir, "xr_glow_mips.npz")), meta


def _noise(rec):
    H, W = rec["size"]
    return np.random.default_rng(rec["seed"]).integers(0, 256, (H, W, 3), dtype=np.uint8)


def test_the_restated_chain_is_the_reference_chain_on_even_sizes(fixtures):
    import xr_glow_ref as R
    _, mips, meta = fixtures
    rec = next(m for m in meta["mips"] if m["name"] == "1024x512")
    levels = R.chain(_noise(rec))
    assert [list(l.shape[:2]) for l in levels[1:]] == [l["size"] for l in rec["levels"]] and len(levels) == 11
    for k in range(1, len(levels)):
        assert np.array_equal(levels[k], mips[f"mip_1024x512_{k}"]), k
    assert np.array_equal(R.pack(levels)[:levels[1].size].reshape(levels[1].shape), levels[1])


def test_the_restated_chain_on_odd_sizes_is_within_one_level_of_the_reference(fixtures):
    import xr_glow_ref as R
    _, mips, meta = fixtures
    rec = next(m for m in meta["mips"] if m["name"] == "1000x562")
    assert [l["size"] for l in rec["levels"]] == [[281, 500], [140, 250], [70, 125], [35, 62], [17, 31], [8, 15], [4, 7], [2, 3], [1, 1]]
    worst = 0.0
    for lv in rec["levels"]:
        k = lv["level"]
        if k < rec["first_level"]:
            continue
        got = R.next_level(mips[f"mip_1000x562_{k - 1}"])
        d = np.abs(got.astype(int) - mips[f"mip_1000x562_{k}"].astype(int))
        print(f"[level {k} {lv['size']}] differs in {(d > 0).mean():.4%} (allowed {2 * lv['differ']:.4%}), max {d.max()}")
        assert d.max() <= 1 and (d > 0).mean() <= 2.0 * lv["differ"], (k, float((d > 0).mean()), int(d.max()))
        worst = max(worst, float((d > 0).mean()))
    assert worst > 0.0          # the odd steps are where the render's own arithmetic shows: the fixture must contain some
    # a plain 2 x 2 box with floor indexing is NOT the rule there
    prev, ref = mips["mip_1000x562_4"].astype(int), mips["mip_1000x562_5"].astype(int)      # 35 x 62 -> 17 x 31
    box = (prev[0:34:2, 0:62:2] + prev[1:34:2, 0:62:2] + prev[0:34:2, 1:62:2] + prev[1:34:2, 1:62:2] + 2) // 4
    assert np.abs(box - ref).max() > 8


def test_the_restated_eyes_are_within_the_recorded_bounds_of_the_renders(fixtures):
    import xr_glow_ref as R
    z, _, meta = fixtures
    eh, ew = meta["eye"]
    assert [c["name"] for c in meta["cases"]][:7] == ["glow_front", "glow2_front", "glow_oblique", "glow_crop_corner", "glow_odd", "glow_small", "glow_far"]
    for c in meta["cases"]:
        img, dep = R.case_scene(c)
        levels = R.chain(img)
        outer = inner = 0
        for e in c["eyes"]:
            want, cls = R.case_render(c, e, img, dep, levels, ew, eh)
            ok = R.uniform3x3(cls)
            assert 1.0 - ok.mean() <= 0.10
            assert [int(((cls == k) & ok).sum()) for k in range(4)] == e["classes"]
            outer += e["classes"][R.OUTER]
            inner += e["inner_glow_pixels"]
            g = R.golden_eye(z, c, e["eye"])
            dd, da = np.abs(want[..., :3] - g[..., :3])[ok], np.abs(want[..., 3] - g[..., 3])[ok]
            share, mean, amax = e["gl"]
            print(f"[{c['name']} eye {e['eye']}] beyond 1 level {(dd > 1).mean():.3e} (recorded {share:.3e}) mean {dd.mean():.4f} ({mean:.4f}) "
                  f"alpha max {da.max():.2e} ({amax:.2e})")
            assert (dd > 1).mean() <= share + 1e-9 and dd.mean() <= mean + 1e-9 and da.max() <= amax + 1e-9
            assert share <= 0.10 and mean <= 0.5 and amax <= 1e-3          # the restatement IS the reference's glow, to the render's own texture filtering
        assert outer >= 500 and (c["mode"] != 1 or inner >= 50), (c["name"], outer, inner)
