"""GPU: the OpenXR eye views (d2s_dibr_xr_eyes, ops.dibr_xr_eyes, Engine.view_pipeline_xr; reference xr_viewer/effects.py:1023-1137).

PINNED by tests/golden/xr_eye.npz -- the reference's XR fragment shader behind its own vertex shaders, drawn per eye with depth test
and clear colour on SwiftShader (make_golden_xr_eye.py) -- and by the float64 restatement tests/xr_eye_ref.py, which
tests/test_xr_eye_oracle.py holds to those renders.  Pixels are compared where the float64 coverage mask is uniform over their 3 x 3
neighbourhood (the rasteriser's fill rule owns the outline; at most 10 % of an image).  The bounds are not chosen here: per case and
eye the manifest records, measured on the CPU, a float32 run of the restatement against its float64 run and the float64 run against
the render (share of values beyond 1 level, mean, alpha maximum), and the kernel is allowed TWICE THE LARGER of the two, against the
restatement and against the render alike.  Everything else is bit identity or an exact rule: uint8 is the rounded float32; one eye
is the matching half of two; a batch is its frames one by one; the view pipeline is pipeline(depth_full) + dibr_xr_eyes; a refused
call leaves `out` untouched.  An eye whose vp @ model maps the quad exactly onto its image is d2s_dibr_warp_crop's eye to the
identity bound of tests/test_gpu_xr_crop.py (>= 99.9 % within 0.02 level): the same shader on a uv formed differently.
Shapes: 130 x 100 eye images (no multiple of the 16 x 16 block, several blocks), a 160 x 96 source, 1 and 48 facets."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_eye.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_eye.npz")), json.load(f)


@pytest.fixture(scope="module")
def reference(fixtures):
    """{(case, eye): (float64 frag [h,w,4], compared-pixel mask)}, computed once."""
    import xr_eye_ref as X
    _, meta = fixtures
    eh, ew = meta["eye"]
    out = {}
    for c in meta["cases"]:
        img, dep, _ = X.case_scene(c, meta)
        for e in c["eyes"]:
            want, cov = X.render_eye(img, dep, X.case_facets(c), np.array(e["vp"]), ew, eh, e["eye"], c["clear"], **X.case_kw(c))
            out[c["name"], e["eye"]] = (want, X.uniform3x3(cov))
    return out


def _eq(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        pytest.fail(f"{what}: differ in {int((d > 0).sum())} of {d.size} values, max |diff| {d.max():.3e}")


def _case_args(dev, c, meta, alpha="rgba"):
    import xr_eye_ref as X
    from desktop2stereo_amd import ops, xr
    eh, ew = meta["eye"]
    img, _, dep_lib = X.case_scene(c, meta)
    dp = ops.dibr_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], corner_radius=c["corner_radius"], alpha=alpha)
    screen = xr.XrScreen(clear=tuple(c["clear"]), **c["screen"])
    eyes = [xr.xr_eye(np.array(e["vp"]), ew, eh, e["eye"]) for e in c["eyes"]]
    return torch.from_numpy(img).to(dev), torch.from_numpy(dep_lib).to(dev), dp, screen, eyes


def _case(fixtures, name):
    return next(c for c in fixtures[1]["cases"] if c["name"] == name)


CASES = ["flat_front", "flat_oblique", "flat_crop_corner", "curved_h", "curved_v_yaw", "far", "near", "model_depth",      # the issue's eight
         "curved_occluded", "flat_corner_wide"]      # + two facets over one pixel (the depth rule), + the corner SDF away from the outline


@pytest.mark.parametrize("name", CASES)
def test_eye_views_match_the_restatement_and_the_reference_renders(dev, fixtures, reference, name):
    import xr_eye_ref as X
    from desktop2stereo_amd import ops
    z, meta = fixtures
    c = _case(fixtures, name)
    f, d, dp, screen, eyes = _case_args(dev, c, meta)
    got = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=False)
    assert len(got) == 2 and all(tuple(g.shape) == (1, meta["eye"][0], meta["eye"][1], 4) for g in got)
    failures = []
    for e, g in zip(c["eyes"], got):
        g = g[0].cpu().numpy().astype(np.float64)
        want, ok = reference[name, e["eye"]]
        assert 1.0 - ok.mean() <= 0.10
        share_b, mean_b, alpha_b = (2.0 * max(a, b) for a, b in zip(e["f32"], e["gl"]))
        for what, ref in (("float64 restatement", want), ("reference render", X.golden_eye(z, c, e["eye"]))):
            dd = np.abs(g[..., :3] - ref[..., :3])[ok]
            da = np.abs(g[..., 3] - ref[..., 3])[ok]
            print(f"[eye view vs {what}, {name} eye {e['eye']}] beyond 1 level {(dd > 1).mean():.3e} (allowed {share_b:.3e}) mean {dd.mean():.5f} "
                  f"(allowed {mean_b:.5f}) max {dd.max():.3f} alpha max {da.max():.2e} (allowed {alpha_b:.2e})")
            if not ((dd > 1).mean() <= share_b and dd.mean() <= mean_b and da.max() <= alpha_b):
                failures.append((what, e["eye"], float((dd > 1).mean()), float(dd.mean()), float(da.max())))
    assert not failures, failures


def test_uint8_is_the_rounded_float32_and_alpha_modes(dev, fixtures):
    from desktop2stereo_amd import ops
    _, meta = fixtures
    for name in ("flat_crop_corner", "curved_h"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes = _case_args(dev, c, meta)
        f32 = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=False)
        u8 = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=True)
        for a, b in zip(f32, u8):
            want = torch.cat([a[..., :3], a[..., 3:] * 255.0], -1).clamp(0, 255).round().to(torch.uint8)      # round(): half to even
            _eq(b, want, (name, "uint8 vs rounded float32"))
        _, _, dp3, _, _ = _case_args(dev, c, meta, alpha="window")
        rgb = ops.dibr_xr_eyes(f, d, dp3, screen, eyes, crop=c["crop"], out_u8=False)
        for a, b in zip(f32, rgb):
            _eq(b, a[..., :3].contiguous(), (name, "window = the rgb of rgba"))


def test_one_eye_is_the_matching_half_and_a_batch_is_its_frames(dev, fixtures):
    from desktop2stereo_amd import ops, synth, xr
    _, meta = fixtures
    for name in ("flat_oblique", "curved_v_yaw", "model_depth"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes = _case_args(dev, c, meta)
        both = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=False)
        for i in range(2):
            _eq(ops.dibr_xr_eyes(f, d, dp, screen, [eyes[i]], crop=c["crop"], out_u8=False)[0], both[i], (name, "n_eyes = 1, eye", i))
        f2 = torch.stack([f, torch.from_numpy(synth.dibr_scene(f.shape[0], f.shape[1], 77, "boxes")[0]).to(dev)])
        d2 = torch.stack([d, torch.from_numpy(synth.dibr_scene(d.shape[0], d.shape[1], 77, "boxes")[1]).to(dev)])
        small = xr.xr_eye(np.array(c["eyes"][1]["vp"]), 70, 51, 1)                 # eye images of different sizes in one call
        batch = ops.dibr_xr_eyes(f2, d2, dp, screen, [eyes[0], small], crop=c["crop"], out_u8=False)
        assert tuple(batch[0].shape) == (2, 100, 130, 4) and tuple(batch[1].shape) == (2, 51, 70, 4)
        for b in range(2):
            one = ops.dibr_xr_eyes(f2[b], d2[b], dp, screen, [eyes[0], small], crop=c["crop"], out_u8=False)
            for i in range(2):
                _eq(batch[i][b:b + 1], one[i], (name, "batch row", b, "eye", i))
        _eq(batch[0][0:1], both[0], (name, "row 0 of the batch"))


def test_an_eye_that_maps_the_quad_onto_its_image_is_the_cropped_warp(dev):
    """vp @ model = identity on (x, y): the facet's homography gives uv = pixel centre / size, the cropped warp's own uv."""
    from desktop2stereo_amd import ops, synth, xr
    H, W = 96, 160
    img, dep = synth.dibr_scene(H, W, 95, "boxes")
    f, d = torch.from_numpy(img).to(dev), torch.from_numpy(dep).to(dev)
    vp = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 1.0], [0, 0, 0, 1.0]])
    screen = xr.XrScreen(width=2.0, height=2.0, distance=1.0)
    for crop, kw in (((0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0), dict(corner_radius=0.03)), ((0.25, 0.1, 0.5, 0.8), dict()), (None, dict())):
        dp = ops.dibr_params(depth_ratio=3.0, display_mode="Full-SBS", alpha="rgba", **kw)
        want = ops.dibr_warp(f, d, dp, out_u8=False, crop=crop).cpu().numpy()
        eh, ew = want.shape[0], want.shape[1] // 2
        got = ops.dibr_xr_eyes(f, d, dp, screen, [xr.xr_eye(vp, ew, eh, 0), xr.xr_eye(vp, ew, eh, 1)], crop=crop, out_u8=False)
        for i, g in enumerate(got):
            dd = np.abs(g[0].cpu().numpy() - want[:, i * ew:(i + 1) * ew])
            print(f"[identity eye vs cropped warp, crop {crop} eye {i}] max {dd[..., :3].max():.4f} beyond 0.02: {(dd[..., :3] > 0.02).mean():.2e}")
            assert (dd[..., :3] <= 0.02).mean() >= 0.999, (crop, i, float((dd[..., :3] > 0.02).mean()))
            assert (dd[..., 3] <= 1e-3).mean() >= 0.999, (crop, i)


def test_view_pipeline_xr_equals_pipeline_then_eye_views(dev, fixtures):
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
    c = _case(fixtures, "curved_h")
    eyes = [xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in c["eyes"]]
    try:
        for call, (curve, crop, u8) in enumerate([("horizontal", None, False), ("flat", (0.0, 0.13, 1.0, 0.74), True)]):
            screen = xr.XrScreen(**dict(c["screen"], curve=curve))
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, corner_radius=0.03, alpha="rgba")
            f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 60 + 7 * call + b, "boxes")[0] for b in range(batch)])).to(dev)
            got, got_depth = fused.view_pipeline_xr(f, p, dp, screen, eyes, crop=crop, use_ema=True, out_u8=u8, want_depth=True)
            _, depth = plain.pipeline(f, p, sp, use_ema=True, want_depth=True)
            _eq(got_depth, depth, (call, "depth_full"))
            # (depth: the engine's map as pipeline(depth_full) up-sampled it; the kernel up-samples the same texels itself, bit for bit)
            want = ops.dibr_xr_eyes(f, depth, dp, screen, eyes, crop=crop, out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], (call, curve, "eye", i))
    finally:
        fused.close(); plain.close()


def test_a_refused_call_leaves_out_untouched(dev, fixtures):
    from desktop2stereo_amd import _lib, ops, xr
    _, meta = fixtures
    c = _case(fixtures, "flat_front")
    f, d, dp, screen, eyes = _case_args(dev, c, meta)
    _, total = ops.dibr_xr_shape(eyes, 1, dp.alpha_mode)
    out = torch.full((total,), -7.0, dtype=torch.float32, device=dev)                   # (no output value is negative)
    for bad in (xr.XrScreen(width=1.6, height=0.96, distance=0.2, yaw=1.2), xr.XrScreen(width=1.6, height=-1.0)):
        with pytest.raises(_lib.D2SError):
            ops.dibr_xr_eyes(f, d, dp, bad, eyes, out_u8=False, out=out)
    with pytest.raises(_lib.D2SError):
        ops.dibr_xr_eyes(f, d, ops.dibr_params(feather=True, alpha="rgba"), screen, eyes, out_u8=False, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    ops.dibr_xr_eyes(f, d, dp, screen, eyes, out_u8=False, out=out)                # and an accepted one writes every element
    assert not bool((out == -7.0).any())


KINDS = [("plain", "flat", None), ("glow", "flat", "glow"), ("glow_curved", "horizontal", "glow"), ("glow_curved", "vertical", "glow")]


@pytest.mark.parametrize("kind,curve,mode", KINDS, ids=[f"{k}-{c}" for k, c, _ in KINDS])
def test_each_eye_of_two_unequal_eyes_is_its_one_eye_call(dev, kind, curve, mode):
    """Two eye images of different sizes, neither a multiple of the 16 x 16 block: 34 x 20 (3 x 2 blocks) and 18 x 18 (2 x 2), batch 2.
    The grid is the larger eye's, so whole blocks and parts of blocks lie outside the smaller eye's image while the other eye's blocks
    stage the chain: every such thread must pass the kernels' barriers and write nothing.  Each eye's image is, bit for bit, the image
    of a call with that eye alone."""
    from desktop2stereo_amd import ops, synth, xr
    H, W, dh, dw, B = 96, 160, 24, 40, 2
    f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 31 + b, "boxes")[0] for b in range(B)])).to(dev)
    d = torch.from_numpy(np.stack([synth.dibr_scene(dh, dw, 31 + b, "boxes")[1] for b in range(B)])).to(dev)
    fov = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))
    vp = [xr.fov_to_proj_mat4(*fov[i]) @ xr.pose_to_view_mat4((0, 0, 0, 1), (-0.032 if i == 0 else 0.032, 0, 0)) for i in range(2)]
    eyes = [xr.xr_eye(vp[0], 34, 20, 0), xr.xr_eye(vp[1], 18, 18, 1)]
    screen = xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve=curve, clear=(0.1, 0.2, 0.3, 1.0))
    dp = ops.dibr_params(corner_radius=0.03, alpha="rgba")
    want_kind = ops.dibr_xr_plan({"plain": "eyes"}.get(kind, kind), dh, dw, B, H, W, dp, screen, eyes, glow=xr.XrGlow(mode, 10.0) if mode else None,
                                 out_u8=False)
    assert want_kind["kind"] == kind and want_kind["grid"] == (3, 2, 2 * B)
    if kind == "plain":
        call = lambda e: ops.dibr_xr_eyes(f, d, dp, screen, e, out_u8=False)
    else:
        levels = ops.mip_chain(f)
        fn = ops.dibr_xr_eyes_glow if kind == "glow" else ops.dibr_xr_eyes_glow_curved
        call = lambda e: fn(f, d, dp, screen, e, xr.XrGlow(mode, 10.0), levels, out_u8=False)
    both = call(eyes)
    assert tuple(both[0].shape) == (B, 20, 34, 4) and tuple(both[1].shape) == (B, 18, 18, 4)
    for i in range(2):
        _eq(call([eyes[i]])[0], both[i], (kind, curve, "eye", i))
    if kind != "plain":                                  # the glow is in the picture: it differs from the plain screen's
        plain = ops.dibr_xr_eyes(f, d, dp, screen, eyes, out_u8=False)
        assert all(not torch.equal(a, b) for a, b in zip(plain, both))
