"""GPU: the glow around the curved OpenXR screen (d2s_dibr_xr_eyes_glow_curved, ops.dibr_xr_eyes_glow_curved,
Engine.view_pipeline_xr_glow_curved; reference xr_viewer/effects.py:314-474, xr_viewer/glsl.py:580-666).

PINNED by tests/golden/xr_glow_curved.npz -- the reference's curved glow mesh drawn around its curved screen per eye on SwiftShader
(make_golden_xr_glow_curved.py) -- and by tests/xr_glow_curved_ref.py, whose float64 rasteriser of the RECORDED triangles
tests/test_cpu_xr_glow_curved.py holds to those renders.
  * The eyes: compared where the float64 region class (none / outer band / screen / screen + inner band) is uniform on 3 x 3, at
    most 10 % of an eye image excluded; the bounds are measured, not chosen -- per case and eye the manifest records the float32
    emulation of the kernel's search against the float64 rasteriser, and that rasteriser against the render, and the kernel is allowed
    TWICE THE LARGER of the two, against both (the factor 2: the project's margin for SwiftShader's 8-bit sub-texel weights).
  * Everything else is bit identity or an exact rule: a screen pixel outside the inner band is dibr_xr_eyes' pixel; a flat screen or
    glow off through the new entry is dibr_xr_eyes_glow / dibr_xr_eyes; uint8 is the rounded float32; one eye is the matching half of
    two; a batch is its frames; the view pipeline is pipeline(depth_full) + mip_chain + the eye call; a refused call leaves `out`
    untouched."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = {1: "glow", 2: "glow2"}
CASES = ["curved_h_glow_front", "curved_h_glow2_front", "curved_v_glow_front", "curved_h_glow_oblique", "curved_v_glow2_tilt",
         "curved_h_glow_crop_corner", "curved_h_glow_odd", "curved_h_glow_near"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_glow_curved.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_glow_curved.npz")), json.load(f)


@pytest.fixture(scope="module")
def scenes(fixtures):
    """{case: (rgb, depth, restated chain)}, computed once."""
    import xr_glow_ref as R
    out = {}
    for c in fixtures[1]["cases"]:
        img, dep = R.case_scene(c)
        out[c["name"]] = (img, dep, R.chain(img))
    return out


def _eq(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        pytest.fail(f"{what}: differ in {int((d > 0).sum())} of {d.size} values, max |diff| {d.max():.3e}")


def _case(fixtures, name):
    return next(c for c in fixtures[1]["cases"] if c["name"] == name)


def _case_args(dev, c, scenes, alpha="rgba"):
    from desktop2stereo_amd import ops, xr
    img, dep, _ = scenes[c["name"]]
    dp = ops.dibr_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], corner_radius=c["corner_radius"], alpha=alpha)
    screen = xr.XrScreen(clear=tuple(c["clear"]), **c["screen"])
    eyes = [xr.xr_eye(np.array(e["vp"]), e["size"][0], e["size"][1], e["eye"]) for e in c["eyes"]]
    glow = xr.XrGlow(MODES[c["mode"]], c["range_m"], c["inner_edge_fraction"])
    f = torch.from_numpy(img).to(dev)
    return f, torch.from_numpy(dep).to(dev), dp, screen, eyes, glow, ops.mip_chain(f)


@pytest.mark.parametrize("name", CASES)
def test_curved_glow_eyes_match_the_restatement_and_the_reference_renders(dev, fixtures, scenes, name):
    import xr_glow_curved_ref as K
    import xr_glow_ref as R
    from desktop2stereo_amd import ops
    z, _ = fixtures
    c = _case(fixtures, name)
    f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, scenes)
    got = ops.dibr_xr_eyes_glow_curved(f, d, dp, screen, eyes, glow, levels, crop=c["crop"], out_u8=False)
    assert len(got) == 2
    failures = []
    for e, g in zip(c["eyes"], got):
        ew, eh = e["size"]
        assert tuple(g.shape) == (1, eh, ew, 4)
        g = g[0].cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all()
        want, cls = K.case_render(c, e, z[name + "_verts"], *scenes[name])
        ok = R.uniform3x3(cls)
        assert 1.0 - ok.mean() <= 0.10
        share_b, mean_b, alpha_b = (2.0 * max(a, b) for a, b in zip(e["f32"], e["gl"]))
        for what, ref in (("float64 rasteriser", want), ("reference render", K.golden_eye(z, c, e["eye"]))):
            dd = np.abs(g[..., :3] - ref[..., :3])[ok]
            da = np.abs(g[..., 3] - ref[..., 3])[ok]
            print(f"[curved glow eye vs {what}, {name} eye {e['eye']}] beyond 1 level {(dd > 1).mean():.3e} (allowed {share_b:.3e}) mean "
                  f"{dd.mean():.5f} (allowed {mean_b:.5f}) max {dd.max():.3f} alpha max {da.max():.2e} (allowed {alpha_b:.2e})")
            if not ((dd > 1).mean() <= share_b and dd.mean() <= mean_b and da.max() <= alpha_b):
                failures.append((what, e["eye"], float((dd > 1).mean()), float(dd.mean()), float(da.max())))
    assert not failures, failures


def _plain_screen_mask(c, e, mode):
    """Pixels the float32 emulation of the search classes as screen and outside the inner band (glow2: every screen pixel)."""
    import xr_glow_curved_ref as K
    sc, glow, U, _ = K.case_objects(c)
    vertical = sc.curve == "vertical"
    ew, eh = e["size"]
    e_u, e_v = min(0.5, U["inner"] / U["inner_w"]), min(0.5, U["inner"] / U["inner_h"])
    yc, xc = K._grid(ew, eh, np.float32)
    s = K.search(K.piece_table(sc, glow, np.array(e["vp"]), ew, eh), vertical, e_v if vertical else e_u, e_u if vertical else e_v, mode,
                 xc.ravel(), yc.ravel(), np.float32)
    return ((s["best"] >= 0) & ~s["fband"] & ~s["cband"]).reshape(eh, ew)


@pytest.mark.parametrize("name", ["curved_h_glow_front", "curved_v_glow_front", "curved_v_glow2_tilt", "curved_h_glow_crop_corner",
                                  "curved_h_glow_odd"])
def test_screen_pixels_are_dibr_xr_eyes_pixels_bit_for_bit(dev, fixtures, scenes, name):
    from desktop2stereo_amd import ops, synth
    c = _case(fixtures, name)
    f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, scenes)
    small = torch.from_numpy(synth.dibr_scene(f.shape[0] // 4, f.shape[1] // 4, c["seed"], "boxes")[1]).to(dev)      # a model-resolution map
    n = 0
    for depth in (d, small):                                # FullDep, UpDep
        for u8 in (False, True):
            got = ops.dibr_xr_eyes_glow_curved(f, depth, dp, screen, eyes, glow, levels, crop=c["crop"], out_u8=u8)
            want = ops.dibr_xr_eyes(f, depth, dp, screen, eyes, crop=c["crop"], out_u8=u8)
            for e, g, w in zip(c["eyes"], got, want):
                m = torch.from_numpy(_plain_screen_mask(c, e, c["mode"])).to(dev)
                assert int(m.sum()) > 200
                n += int(m.sum())
                _eq(g[0][m], w[0][m], (name, "screen pixels", "u8" if u8 else "f32", tuple(depth.shape), e["eye"]))
                assert not torch.equal(g[0][~m], w[0][~m])  # and the rest carries the glow
    assert n > 0


def test_a_flat_screen_or_no_glow_through_the_new_entry_is_the_old_calls(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, xr
    c = _case(fixtures, "curved_h_glow_crop_corner")
    f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, scenes)
    flat = xr.XrScreen(**dict(c["screen"], curve="flat"), clear=tuple(c["clear"]))
    for u8 in (False, True):
        want = ops.dibr_xr_eyes_glow(f, d, dp, flat, eyes, glow, levels, crop=c["crop"], out_u8=u8)
        got = ops.dibr_xr_eyes_glow_curved(f, d, dp, flat, eyes, glow, levels, crop=c["crop"], out_u8=u8)
        for i in range(2):
            _eq(got[i], want[i], ("flat", u8, i))
        want = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=u8)
        for g, lv in ((None, None), (xr.XrGlow("off", 5.0), None), (xr.XrGlow("off", float("nan")), levels)):
            got = ops.dibr_xr_eyes_glow_curved(f, d, dp, screen, eyes, g, lv, crop=c["crop"], out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], ("glow off, curved", u8, i))


def test_uint8_is_the_rounded_float32_and_alpha_modes(dev, fixtures, scenes):
    from desktop2stereo_amd import ops
    for name in ("curved_h_glow_crop_corner", "curved_v_glow2_tilt"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, scenes)
        run = lambda dpx, u8: ops.dibr_xr_eyes_glow_curved(f, d, dpx, screen, eyes, glow, levels, crop=c["crop"], out_u8=u8)
        f32, u8 = run(dp, False), run(dp, True)
        for a, b in zip(f32, u8):
            want = torch.cat([a[..., :3], a[..., 3:] * 255.0], -1).clamp(0, 255).round().to(torch.uint8)      # round(): half to even
            _eq(b, want, (name, "uint8 vs rounded float32"))
        rgb = run(_case_args(dev, c, scenes, alpha="window")[2], False)
        pre = run(_case_args(dev, c, scenes, alpha="premultiplied")[2], False)
        for a, b, m in zip(f32, rgb, pre):
            _eq(b, a[..., :3].contiguous(), (name, "window = the rgb of rgba"))
            _eq(m, (a[..., :3] * a[..., 3:]).contiguous(), (name, "premultiplied = rgb * a of rgba"))      # (every pixel of these cases is drawn)


def test_one_eye_is_the_matching_half_and_a_batch_is_its_frames(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, synth, xr
    for name in ("curved_h_glow_oblique", "curved_v_glow_front"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, scenes)
        run = lambda fr, de, ey, lv: ops.dibr_xr_eyes_glow_curved(fr, de, dp, screen, ey, glow, lv, crop=c["crop"], out_u8=False)
        both = run(f, d, eyes, levels)
        for i in range(2):
            _eq(run(f, d, [eyes[i]], levels)[0], both[i], (name, "n_eyes = 1, eye", i))
        other = synth.dibr_scene(f.shape[0], f.shape[1], 77, "boxes")
        f2, d2 = torch.stack([f, torch.from_numpy(other[0]).to(dev)]), torch.stack([d, torch.from_numpy(other[1]).to(dev)])
        lv2 = ops.mip_chain(f2)
        small = xr.xr_eye(np.array(c["eyes"][1]["vp"]), 70, 51, 1)                 # eye images of different sizes in one call
        batch = run(f2, d2, [eyes[0], small], lv2)
        assert tuple(batch[0].shape) == (2, 100, 130, 4) and tuple(batch[1].shape) == (2, 51, 70, 4)
        for b in range(2):
            one = run(f2[b], d2[b], [eyes[0], small], lv2[b:b + 1])
            for i in range(2):
                _eq(batch[i][b:b + 1], one[i], (name, "batch row", b, "eye", i))
        _eq(batch[0][0:1], both[0], (name, "row 0 of the batch"))
        assert not torch.equal(batch[0][0], batch[0][1])


def test_view_pipeline_xr_glow_curved_equals_pipeline_then_mip_chain_then_the_eye_call(dev, fixtures):
    from desktop2stereo_amd import ops, synth, xr
    from desktop2stereo_amd.config import MODELS, PipelineParams, engine_shape
    from desktop2stereo_amd.weights import make_weights
    H, W, res, batch = 270, 480, 140, 2
    cfg = MODELS["tiny"]
    h, w, _ = engine_shape(H, W, res)
    p = PipelineParams(depth_resolution=res)
    wts = make_weights(cfg, 0)
    fused, plain = (ops.Engine(cfg, wts, h, w, batch, "fp32") for _ in range(2))
    sp = ops.sbs_params(p.ipd, p.depth_strength, p.convergence, "Half-SBS", False)
    try:
        for call, (name, mode, crop, u8) in enumerate([("curved_h_glow_front", "glow", None, False),
                                                       ("curved_v_glow_front", "glow2", (0.0, 0.13, 1.0, 0.74), True)]):
            c = _case(fixtures, name)
            eyes = [xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in c["eyes"]]
            screen = xr.XrScreen(**c["screen"])
            glow = xr.XrGlow(mode, 1.5)
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, corner_radius=0.03, alpha="rgba")
            f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 60 + 7 * call + b, "boxes")[0] for b in range(batch)])).to(dev)
            levels = ops.mip_chain(f)
            got, got_depth = fused.view_pipeline_xr_glow_curved(f, p, dp, screen, eyes, glow, levels, crop=crop, use_ema=True, out_u8=u8,
                                                                want_depth=True)
            _, depth = plain.pipeline(f, p, sp, use_ema=True, want_depth=True)
            _eq(got_depth, depth, (call, "depth_full"))
            want = ops.dibr_xr_eyes_glow_curved(f, depth, dp, screen, eyes, glow, levels, crop=crop, out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], (call, mode, "eye", i))
            off = fused.view_pipeline_xr_glow_curved(f, p, dp, screen, eyes, xr.XrGlow("off"), None, crop=crop, use_ema=False, out_u8=u8)
            assert not torch.equal(off[0], want[0])                               # and the glow is there
    finally:
        fused.close(); plain.close()


def test_a_refused_call_leaves_out_untouched(dev, fixtures, scenes, golden_dir):
    from desktop2stereo_amd import _lib, ops, xr
    c = _case(fixtures, "curved_h_glow_front")
    f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, scenes)
    _, total = ops.dibr_xr_shape(eyes, 1, dp.alpha_mode)
    out = torch.full((total,), -7.0, dtype=torch.float32, device=dev)                   # (no output value is negative)
    with open(os.path.join(golden_dir, "xr_eye.json")) as fh:
        occ = {k["name"]: k for k in json.load(fh)["cases"]}["curved_occluded"]
    refused = [
        dict(screen=xr.XrScreen(**dict(c["screen"], normal_offset=0.02))),
        dict(glow=xr.XrGlow("glow", 0.0)), dict(glow=xr.XrGlow("glow2", float("inf"))), dict(glow=xr.XrGlow("glow", 5.0, -0.1)),
        dict(levels=None),
        dict(screen=xr.XrScreen(**dict(c["screen"], distance=0.2, yaw=1.2))),                 # what dibr_xr_eyes refuses
        dict(screen=xr.XrScreen(**occ["screen"]), eyes=[xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in occ["eyes"]]),      # an eye outside
        dict(screen=xr.XrScreen(**dict(c["screen"], curve="flat", normal_offset=0.02))),      # the flat screen's own refusal, forwarded
    ]
    for kw in refused:
        a = dict(dict(screen=screen, glow=glow, levels=levels, eyes=eyes), **kw)
        with pytest.raises(_lib.D2SError):
            ops.dibr_xr_eyes_glow_curved(f, d, dp, a["screen"], a["eyes"], a["glow"], a["levels"], out_u8=False, out=out)
    small_ws = torch.empty(2 * 48 * 96, dtype=torch.uint8, device=dev)                    # d2s_dibr_xr_workspace's size
    with pytest.raises(_lib.D2SError):
        ops.dibr_xr_eyes_glow_curved(f, d, dp, screen, eyes, glow, levels, out_u8=False, out=out, workspace=small_ws)
    with pytest.raises(ValueError):
        ops.dibr_xr_eyes_glow_curved(f, d, dp, screen, eyes, glow, levels[:, :-1], out_u8=False, out=out)
    with pytest.raises(_lib.D2SError):                                                    # the old entry keeps refusing the curved glow
        ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, out_u8=False, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    ops.dibr_xr_eyes_glow_curved(f, d, dp, screen, eyes, glow, levels, out_u8=False, out=out)  # and an accepted one writes every element
    assert not bool((out == -7.0).any())


def test_depth_xr_eye_views_glow_takes_a_curved_screen(dev, fixtures):
    """depth.xr_eye_views_glow sends a curved screen to Engine.view_pipeline_xr_glow_curved (it used to raise): bit-identical to that
    method on the module's engine, and a flat screen still goes where it went."""
    from desktop2stereo_amd import depth as D, ops, synth, xr
    from desktop2stereo_amd.config import PipelineParams
    c = _case(fixtures, "curved_v_glow_front")
    eyes = [xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in c["eyes"]]
    p = PipelineParams(depth_resolution=140)
    D.configure("tiny", params=p, precision="fp32", max_batch=2)
    frames = np.stack([synth.dibr_scene(270, 480, 90 + b, "boxes")[0] for b in range(2)])
    try:
        for curve in ("vertical", "horizontal", "flat"):
            screen = xr.XrScreen(**dict(c["screen"], curve=curve))
            got = D.xr_eye_views_glow(frames, screen, eyes, glow="glow2", range_m=1.5)
            assert len(got) == 2 and all(tuple(g.shape) == (2, 100, 130, 4) and g.dtype == torch.uint8 for g in got)
            eng = D._state["engine"]
            f = torch.from_numpy(frames).to(dev)
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, corner_radius=0.03, alpha="rgba")
            run = eng.view_pipeline_xr_glow if curve == "flat" else eng.view_pipeline_xr_glow_curved
            want = run(f, p, dp, screen, eyes, xr.XrGlow("glow2", 1.5), ops.mip_chain(f))
            plain = D.xr_eye_views(frames, screen, eyes)
            for i in range(2):
                _eq(got[i], want[i], (curve, "eye", i))
                assert not torch.equal(got[i], plain[i])        # and the glow is there
    finally:                                                # (the module's engine is this test's: leave none behind)
        if D._state["engine"] is not None:
            D._state["engine"].close()
        D._state["engine"], D._state["engine_key"] = None, None
