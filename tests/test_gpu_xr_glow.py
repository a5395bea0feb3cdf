"""GPU: the colour mip chain (d2s_mip_chain, ops.mip_chain) and the glow around the flat OpenXR screen (d2s_dibr_xr_eyes_glow,
ops.dibr_xr_eyes_glow, Engine.view_pipeline_xr_glow; reference xr_viewer/effects.py:476-646, xr_viewer/glsl.py:580-666).

PINNED by tests/golden/xr_glow.npz -- the reference's glow passes drawn around its screen per eye on SwiftShader
(make_golden_xr_glow.py) -- and by the restatement tests/xr_glow_ref.py, which tests/test_xr_glow_oracle.py holds to those renders and
to glGenerateMipmap's levels.
  * The chain: the kernels are all-integer and the float64 restatement is exact, so every size is compared bit for bit where the
    chain is the 2 x 2 box, and within twice the float32-against-float64 share of the restatement (at most 1 level) where a step
    starts from an odd size.  Sizes: 1024 x 512 (the tiled box kernel, three levels per launch, then the LDS tail), 160 x 96 (one
    box launch of partial tiles, then the tail), 77 x 101 (the tail alone, from the frame), 328 x 200 (box tiles cut at the right
    and bottom edges, then a general step), 1000 x 562 (box, general step, box, tail), a batch of 2.
  * The eyes: compared where the float64 region class (none / outer band / screen / screen + inner band) is uniform on 3 x 3; the
    bounds are measured, not chosen -- per case and eye the manifest records a float32 run of the restatement against its float64
    run and the float64 run against the render, and the kernel is allowed TWICE THE LARGER of the two, against both.
  * Everything else is bit identity or an exact rule: glow off through the new entry is dibr_xr_eyes; uint8 is the rounded float32;
    one eye is the matching half of two; a batch is its frames; the view pipeline is pipeline(depth_full) + mip_chain +
    dibr_xr_eyes_glow; a refused call leaves `out` untouched."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = {1: "glow", 2: "glow2"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_glow.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_glow.npz")), json.load(f)


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


def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _unpack(flat, H, W):
    from desktop2stereo_amd import ops
    levels, total = ops.mip_shape(H, W)
    assert flat.shape == (total,)
    return [flat[o:o + h * w * 3].reshape(h, w, 3) for o, h, w in levels]


@pytest.mark.parametrize("H,W", [(512, 1024), (96, 160), (200, 328)])
def test_mip_chain_is_the_restatement_bit_for_bit(dev, H, W):
    import xr_glow_ref as R
    from desktop2stereo_amd import ops
    img = _noise(H, W, 7)
    got = ops.mip_chain(torch.from_numpy(img).to(dev))
    assert tuple(got.shape) == (1, ops.mip_shape(H, W)[1]) and got.dtype == torch.uint8
    want = R.chain(img)
    for k, g in enumerate(_unpack(got[0].cpu().numpy(), H, W), 1):
        assert np.array_equal(g, want[k]), (k, g.shape, int((g != want[k]).sum()))


def test_mip_chain_of_a_batch_is_its_frames_and_out_is_honoured(dev):
    import xr_glow_ref as R
    from desktop2stereo_amd import ops
    H, W = 96, 160
    imgs = np.stack([_noise(H, W, 11), _noise(H, W, 12)])
    out = torch.zeros((2, ops.mip_shape(H, W)[1]), dtype=torch.uint8, device=dev)
    got = ops.mip_chain(torch.from_numpy(imgs).to(dev), out=out)
    assert got.data_ptr() == out.data_ptr()
    for b in range(2):
        assert np.array_equal(got[b].cpu().numpy(), R.pack(R.chain(imgs[b]))), b
    big = np.stack([_noise(512, 1024, 13), _noise(512, 1024, 14)])                  # the tiled kernel's batch index
    got = ops.mip_chain(torch.from_numpy(big).to(dev))
    for b in range(2):
        _eq(got[b:b + 1], ops.mip_chain(torch.from_numpy(big[b]).to(dev)), ("batch row", b))
    with pytest.raises(ValueError):
        ops.mip_chain(torch.from_numpy(imgs).to(dev), out=out[:, :-1])


@pytest.mark.parametrize("H,W", [(562, 1000), (101, 77)])
def test_mip_chain_from_odd_sizes_is_within_the_restatement_s_own_rounding(dev, H, W):
    import xr_glow_ref as R
    from desktop2stereo_amd import ops
    img = _noise(H, W, 7)
    got = _unpack(ops.mip_chain(torch.from_numpy(img).to(dev))[0].cpu().numpy(), H, W)
    w64, w32 = R.chain(img, np.float64), R.chain(img, np.float32)
    for k, g in enumerate(got, 1):
        d = np.abs(g.astype(int) - w64[k].astype(int))
        allowed = 2.0 * float((w32[k] != w64[k]).mean())
        print(f"[mip {W}x{H} level {k} {g.shape[:2]}] differs from float64 in {(d > 0).mean():.4%} (allowed {allowed:.4%}), max {d.max()}")
        assert d.max() <= 1 and (d > 0).mean() <= allowed, (k, float((d > 0).mean()), allowed)


def _case(fixtures, name):
    return next(c for c in fixtures[1]["cases"] if c["name"] == name)


def _case_args(dev, c, meta, scenes, alpha="rgba"):
    from desktop2stereo_amd import ops, xr
    eh, ew = meta["eye"]
    img, dep, _ = scenes[c["name"]]
    dp = ops.dibr_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], corner_radius=c["corner_radius"], alpha=alpha)
    screen = xr.XrScreen(clear=tuple(c["clear"]), **c["screen"])
    eyes = [xr.xr_eye(np.array(e["vp"]), ew, eh, e["eye"]) for e in c["eyes"]]
    glow = xr.XrGlow(MODES[c["mode"]], c["range_m"], c["inner_edge_fraction"])
    f = torch.from_numpy(img).to(dev)
    return f, torch.from_numpy(dep).to(dev), dp, screen, eyes, glow, ops.mip_chain(f)


CASES = ["glow_front", "glow2_front", "glow_oblique", "glow_crop_corner", "glow_odd", "glow_small", "glow_far",      # the issue's seven
         "glow_horizon"]      # + the plane's horizon inside the image: pixels whose plane point has clip w <= 0


@pytest.mark.parametrize("name", CASES)
def test_glow_eyes_match_the_restatement_and_the_reference_renders(dev, fixtures, scenes, name):
    import xr_glow_ref as R
    from desktop2stereo_amd import ops
    z, meta = fixtures
    eh, ew = meta["eye"]
    c = _case(fixtures, name)
    f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, meta, scenes)
    if c["chain_is_restated"]:
        assert np.array_equal(levels[0].cpu().numpy(), R.pack(scenes[name][2]))
    got = ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, crop=c["crop"], out_u8=False)
    assert len(got) == 2 and all(tuple(g.shape) == (1, eh, ew, 4) for g in got)
    failures = []
    for e, g in zip(c["eyes"], got):
        g = g[0].cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all()
        want, cls = R.case_render(c, e, *scenes[name], ew, eh)
        ok = R.uniform3x3(cls)
        assert 1.0 - ok.mean() <= 0.10
        share_b, mean_b, alpha_b = (2.0 * max(a, b) for a, b in zip(e["f32"], e["gl"]))
        for what, ref in (("float64 restatement", want), ("reference render", R.golden_eye(z, c, e["eye"]))):
            dd = np.abs(g[..., :3] - ref[..., :3])[ok]
            da = np.abs(g[..., 3] - ref[..., 3])[ok]
            print(f"[glow eye vs {what}, {name} eye {e['eye']}] beyond 1 level {(dd > 1).mean():.3e} (allowed {share_b:.3e}) mean {dd.mean():.5f} "
                  f"(allowed {mean_b:.5f}) max {dd.max():.3f} alpha max {da.max():.2e} (allowed {alpha_b:.2e})")
            if not ((dd > 1).mean() <= share_b and dd.mean() <= mean_b and da.max() <= alpha_b):
                failures.append((what, e["eye"], float((dd > 1).mean()), float(dd.mean()), float(da.max())))
    assert not failures, failures


def test_glow_off_through_the_new_entry_is_dibr_xr_eyes(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, xr
    _, meta = fixtures
    c = _case(fixtures, "glow_crop_corner")
    f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, meta, scenes)
    for u8 in (False, True):
        want = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=u8)
        for g, lv in ((None, None), (xr.XrGlow("off", 5.0), None), (xr.XrGlow("off", float("nan")), levels)):
            got = ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, g, lv, crop=c["crop"], out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], ("glow off", u8, i))
    curved = xr.XrScreen(**dict(c["screen"], curve="horizontal", distance=1.5))        # a curved screen is refused only with glow ON
    want = ops.dibr_xr_eyes(f, d, dp, curved, eyes, out_u8=False)
    got = ops.dibr_xr_eyes_glow(f, d, dp, curved, eyes, xr.XrGlow("off"), None, out_u8=False)
    for i in range(2):
        _eq(got[i], want[i], ("glow off, curved", i))


def test_uint8_is_the_rounded_float32_and_alpha_modes(dev, fixtures, scenes):
    from desktop2stereo_amd import ops
    _, meta = fixtures
    for name in ("glow_crop_corner", "glow2_front"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, meta, scenes)
        f32 = ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, crop=c["crop"], out_u8=False)
        u8 = ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, crop=c["crop"], out_u8=True)
        for a, b in zip(f32, u8):
            want = torch.cat([a[..., :3], a[..., 3:] * 255.0], -1).clamp(0, 255).round().to(torch.uint8)      # round(): half to even
            _eq(b, want, (name, "uint8 vs rounded float32"))
        dp3 = _case_args(dev, c, meta, scenes, alpha="window")[2]
        rgb = ops.dibr_xr_eyes_glow(f, d, dp3, screen, eyes, glow, levels, crop=c["crop"], out_u8=False)
        dpm = _case_args(dev, c, meta, scenes, alpha="premultiplied")[2]
        pre = ops.dibr_xr_eyes_glow(f, d, dpm, screen, eyes, glow, levels, crop=c["crop"], out_u8=False)
        for a, b, m in zip(f32, rgb, pre):
            _eq(b, a[..., :3].contiguous(), (name, "window = the rgb of rgba"))
            _eq(m, (a[..., :3] * a[..., 3:]).contiguous(), (name, "premultiplied = rgb * a of rgba"))      # (every pixel of these cases is drawn)


def test_one_eye_is_the_matching_half_and_a_batch_is_its_frames(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, synth, xr
    _, meta = fixtures
    for name in ("glow_oblique", "glow_small"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, meta, scenes)
        both = ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, crop=c["crop"], out_u8=False)
        for i in range(2):
            _eq(ops.dibr_xr_eyes_glow(f, d, dp, screen, [eyes[i]], glow, levels, crop=c["crop"], out_u8=False)[0], both[i], (name, "n_eyes = 1, eye", i))
        other = synth.dibr_scene(f.shape[0], f.shape[1], 77, "boxes")
        f2, d2 = torch.stack([f, torch.from_numpy(other[0]).to(dev)]), torch.stack([d, torch.from_numpy(other[1]).to(dev)])
        lv2 = ops.mip_chain(f2)
        small = xr.xr_eye(np.array(c["eyes"][1]["vp"]), 70, 51, 1)                 # eye images of different sizes in one call
        batch = ops.dibr_xr_eyes_glow(f2, d2, dp, screen, [eyes[0], small], glow, lv2, crop=c["crop"], out_u8=False)
        assert tuple(batch[0].shape) == (2, 100, 130, 4) and tuple(batch[1].shape) == (2, 51, 70, 4)
        for b in range(2):
            one = ops.dibr_xr_eyes_glow(f2[b], d2[b], dp, screen, [eyes[0], small], glow, lv2[b:b + 1], crop=c["crop"], out_u8=False)
            for i in range(2):
                _eq(batch[i][b:b + 1], one[i], (name, "batch row", b, "eye", i))
        _eq(batch[0][0:1], both[0], (name, "row 0 of the batch"))
        assert not torch.equal(batch[0][0], batch[0][1])


def test_view_pipeline_xr_glow_equals_pipeline_then_mip_chain_then_glow_eyes(dev, fixtures):
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
    c = _case(fixtures, "glow_front")
    eyes = [xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in c["eyes"]]
    try:
        for call, (mode, crop, u8) in enumerate([("glow", None, False), ("glow2", (0.0, 0.13, 1.0, 0.74), True)]):
            screen = xr.XrScreen(**c["screen"])
            glow = xr.XrGlow(mode, 1.5)
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, corner_radius=0.03, alpha="rgba")
            f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 60 + 7 * call + b, "boxes")[0] for b in range(batch)])).to(dev)
            levels = ops.mip_chain(f)
            got, got_depth = fused.view_pipeline_xr_glow(f, p, dp, screen, eyes, glow, levels, crop=crop, use_ema=True, out_u8=u8, want_depth=True)
            _, depth = plain.pipeline(f, p, sp, use_ema=True, want_depth=True)
            _eq(got_depth, depth, (call, "depth_full"))
            want = ops.dibr_xr_eyes_glow(f, depth, dp, screen, eyes, glow, levels, crop=crop, out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], (call, mode, "eye", i))
            off = ops.dibr_xr_eyes(f, depth, dp, screen, eyes, crop=crop, out_u8=u8)
            assert not torch.equal(off[0], want[0])                               # and the glow is there
    finally:
        fused.close(); plain.close()


def test_a_refused_call_leaves_out_untouched(dev, fixtures, scenes):
    from desktop2stereo_amd import _lib, ops, xr
    _, meta = fixtures
    c = _case(fixtures, "glow_front")
    f, d, dp, screen, eyes, glow, levels = _case_args(dev, c, meta, scenes)
    _, total = ops.dibr_xr_shape(eyes, 1, dp.alpha_mode)
    out = torch.full((total,), -7.0, dtype=torch.float32, device=dev)                   # (no output value is negative)
    refused = [
        dict(screen=xr.XrScreen(**dict(c["screen"], curve="horizontal", distance=1.5))),      # curved + glow: unsupported
        dict(screen=xr.XrScreen(**dict(c["screen"], curve="vertical", distance=1.5))),
        dict(screen=xr.XrScreen(**dict(c["screen"], normal_offset=0.02))),
        dict(glow=xr.XrGlow("glow", 0.0)), dict(glow=xr.XrGlow("glow2", float("inf"))), dict(glow=xr.XrGlow("glow", 5.0, -0.1)),
        dict(levels=None),
        dict(screen=xr.XrScreen(width=1.6, height=0.96, distance=0.2, yaw=1.2)),              # what dibr_xr_eyes refuses
    ]
    for kw in refused:
        a = dict(dict(screen=screen, glow=glow, levels=levels), **kw)
        with pytest.raises(_lib.D2SError):
            ops.dibr_xr_eyes_glow(f, d, dp, a["screen"], eyes, a["glow"], a["levels"], out_u8=False, out=out)
    bad = xr.XrGlow("glow", 5.0).c_struct()
    bad.mode = 3
    with pytest.raises(_lib.D2SError):
        ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, bad, levels, out_u8=False, out=out)
    with pytest.raises(ValueError):
        ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels[:, :-1], out_u8=False, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, out_u8=False, out=out)  # and an accepted one writes every element
    assert not bool((out == -7.0).any())
