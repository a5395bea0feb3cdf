"""GPU: the OpenXR screen's cropped DIBR warp (d2s_dibr_warp_crop, ops.dibr_warp(crop=), Engine.view_pipeline_crop; reference
xr_viewer/implementation.py:111-126: flipped_uv = u_source_crop.xy + screen_flipped_uv * u_source_crop.zw).

PINNED by tests/golden/xr_crop.npz: renders of the reference's own XR shader (make_golden_xr_crop.py), at tests/test_gpu_dibr.py's
bounds -- small cases every value within 1 level, alpha within 1e-3; beyond 320 columns >= 99.9 % within 1 level, mean <= 0.06.
Against the float32 restatement (tests/xr_crop_ref.py, itself held to those renders by tests/test_cpu_crop.py): >= 99.9 % within
0.02 of a level, mean <= 2e-3.  Everything else is BIT identity (np.array_equal on float32 output): the identity crop is
d2s_dibr_warp_depth; the cropped row kernels are the cropped gather kernel; cropped model-resolution depth is d2s_upsample_depth +
the cropped full-resolution warp; a batch is its frames one by one; the cropped view pipeline is pipeline(depth_full) +
d2s_dibr_warp_crop.  Shapes: 90 x 160 and 96 x 128 frames with crops whose x0 > 0, whose LDS window leaves the texture on the left,
and whose right edge is u = 1 -- the smallest at which the window arithmetic can go wrong -- plus widths past one 256- and one
512-column block."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ENV_KEYS = ("D2S_DIBR_NO_ROLL0", "D2S_DIBR_NO_ROWS", "D2S_DIBR_COLS")
MODES = ("Full-SBS", "Half-SBS", "Full-TAB", "Half-TAB")
# x0 > 0; a window that starts left of the texture (x0 = 4 texels < the margin); right edge u = 1; both axes; the full width
CROPS = [(0.25, 0.1, 0.5, 0.8), (0.025, 0.0, 0.95, 1.0), (0.4, 0.1, 0.6, 0.8), (0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


def _scene(dev, H, W, seed, dh=None, dw=None, batch=None):
    from desktop2stereo_amd import synth
    n = batch or 1
    f = np.stack([synth.dibr_scene(H, W, seed + i, "boxes")[0] for i in range(n)])
    d = np.stack([synth.dibr_scene(dh or H, dw or W, seed + i, "boxes")[1] for i in range(n)])
    f, d = torch.from_numpy(f).to(dev), torch.from_numpy(d).to(dev)
    return (f, d) if batch else (f[0], d[0])


def _eq(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        pytest.fail(f"{what}: differ in {int((d > 0).sum())} of {d.size} values, max |diff| {d.max():.3e}")


def _eyes(got, mode, eh, ew):
    return (got[:, :ew], got[:, ew:]) if mode.endswith("SBS") else (got[:eh], got[eh:])


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_crop.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_crop.npz")), json.load(f)


def _run_case(dev, c):
    from desktop2stereo_amd import ops, synth
    img, dep = synth.dibr_scene(c["h"], c["w"], c["seed"], c["scene"])
    mode = "Half-SBS" if c["half_sbs"] else "Full-SBS"
    dp = ops.dibr_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], mode, roll=c.get("roll", 0.0), feather=c.get("feather", False),
                         feather_width=c.get("feather_width", 0.02), corner_radius=c.get("corner_radius", 0.0), alpha="rgba")
    got = ops.dibr_warp(torch.from_numpy(img).to(dev), torch.from_numpy(dep).to(dev), dp, out_u8=False, crop=c["crop"]).cpu().numpy()
    assert got.shape == (c["eye_h"], 2 * c["eye_w"], 4), (c["name"], got.shape)
    return img, dep, _eyes(got, mode, c["eye_h"], c["eye_w"])


def test_cropped_warp_matches_the_reference_xr_shader_renders(dev, fixtures):
    z, meta = fixtures
    assert len(meta["cases"]) == 7
    for c in meta["cases"]:
        _, _, eyes = _run_case(dev, c)
        for eye, g in zip(("left", "right"), eyes):
            g = g[::c["row_stride"]]
            rgb = z[f"{c['name']}_{eye}_rgb"].astype(np.float32) / 256.0
            a = z[f"{c['name']}_{eye}_a"].astype(np.float32) / 65535.0
            d, da = np.abs(g[..., :3] - rgb), np.abs(g[..., 3] - a)
            print(f"[cropped warp vs the reference XR shader's render, {c['name']} {eye}] rgb max {d.max():.3f} mean {d.mean():.4f} "
                  f"{(d > 1).mean():.2e} beyond 1 level | alpha max diff {da.max():.1e} (min alpha {a.min():.3f})")
            assert da.max() <= 1e-3, (c["name"], eye, float(da.max()))
            if c["w"] <= 320:
                assert d.max() <= 1.0, (c["name"], eye, float(d.max()))
            else:
                assert (d <= 1.0).mean() >= 0.999 and d.mean() <= 0.06, (c["name"], eye, float((d > 1).mean()), float(d.mean()))


def test_cropped_warp_matches_the_restatement(dev, fixtures):
    import xr_crop_ref as X
    _, meta = fixtures
    for c in meta["cases"]:
        if c["h"] > 400:                                   # (the 1080p restatement takes CPU-minutes; the render pins that case)
            continue
        img, dep, eyes = _run_case(dev, c)
        kw = dict(roll=c.get("roll", 0.0), feather=c.get("feather", False), feather_width=c.get("feather_width", 0.02),
                  corner_radius=c.get("corner_radius", 0.0))
        for sign, g in zip((-1.0, 1.0), eyes):
            want = X.dibr_eye_crop(img, dep, c["crop"], sign * c["ipd_uv"] / 2.0, 0.1 * c["depth_ratio"], c["convergence"], c["eye_h"],
                                   c["eye_w"], **kw)
            d = np.abs(g[..., :3] - want[..., :3])
            print(f"[cropped warp vs restatement, {c['name']} eye {sign:+.0f}] max {d.max():.4f} mean {d.mean():.2e} {(d > 0.02).mean():.2e} beyond 0.02")
            assert (d <= 0.02).mean() >= 0.999 and d.mean() <= 2e-3, (c["name"], sign, float((d > 0.02).mean()), float(d.mean()))
            assert np.abs(g[..., 3] - want[..., 3]).max() <= 1e-4, (c["name"], sign)


@pytest.mark.parametrize("kw", [dict(), dict(feather=True, corner_radius=0.03), dict(alpha="rgba", corner_radius=0.03), dict(roll=0.2),
                                dict(roll=-0.1, feather=True)], ids=lambda kw: "-".join(kw) or "plain")
def test_identity_crop_is_the_uncropped_warp(dev, kw):
    """crop = (0, 0, 1, 1) == d2s_dibr_warp_depth bit for bit: full-resolution and model-resolution depth, float32 and uint8, FX on
    and off, RGBA, roll 0 (row kernels) and != 0 (gather kernel), all four modes."""
    from desktop2stereo_amd import ops
    for (H, W, dh, dw) in ((90, 160, None, None), (270, 600, 84, 196)):
        f, d = _scene(dev, H, W, 71, dh, dw)
        for mode in MODES:
            dp = ops.dibr_params(display_mode=mode, depth_ratio=3.0, **kw)
            for u8 in (False, True):
                _eq(ops.dibr_warp(f, d, dp, out_u8=u8, crop=(0.0, 0.0, 1.0, 1.0)), ops.dibr_warp(f, d, dp, out_u8=u8), (H, W, dh, mode, kw, u8))


def test_cropped_row_kernels_are_the_cropped_gather_kernel(dev, monkeypatch):
    """The LDS-window kernels (512 and 256 columns per block) against the row gather and the general per-tap kernel, with every crop:
    FullDep and UpDep, FX off and on, all four modes."""
    from desktop2stereo_amd import ops
    try:
        for (H, W, dh, dw, seed) in ((90, 160, None, None, 81), (96, 128, None, None, 82), (120, 700, 50, 290, 83)):
            f, d = _scene(dev, H, W, seed, dh, dw)
            for crop in CROPS:
                for kw in (dict(), dict(feather=True, corner_radius=0.03, alpha="rgba"), dict(depth_ratio=20.0, ipd_uv=0.2)):
                    for mode in MODES:
                        dp = ops.dibr_params(display_mode=mode, **dict(dict(depth_ratio=3.0), **kw))
                        outs = {}
                        for name, env in (("rows", {}), ("rows_256", {"D2S_DIBR_COLS": "256"}), ("row_gather", {"D2S_DIBR_NO_ROWS": "1"}),
                                          ("general", {"D2S_DIBR_NO_ROLL0": "1"})):
                            for k in ENV_KEYS:
                                monkeypatch.delenv(k, raising=False)
                            for k, v in env.items():
                                monkeypatch.setenv(k, v)
                            ops.reload_env()
                            outs[name] = ops.dibr_warp(f, d, dp, out_u8=False, crop=crop)
                        for name in ("rows", "rows_256", "row_gather"):
                            _eq(outs[name], outs["general"], (H, W, dh, crop, kw, mode, name))
    finally:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        ops.reload_env()


def test_cropped_model_depth_and_batches(dev):
    """Cropped UpDep == d2s_upsample_depth + cropped FullDep; a batch of two == two calls; the uint8 store."""
    from desktop2stereo_amd import ops
    for (H, W, dh, dw) in ((90, 160, 42, 70), (270, 600, 84, 196)):
        f, d = _scene(dev, H, W, 91, dh, dw, batch=2)
        full = ops.upsample_depth(d, H, W)
        for crop in CROPS:
            for kw in (dict(), dict(feather=True, corner_radius=0.03), dict(roll=0.15)):
                for mode in ("Full-SBS", "Half-TAB"):
                    dp = ops.dibr_params(display_mode=mode, depth_ratio=3.0, **kw)
                    both = ops.dibr_warp(f, d, dp, out_u8=False, crop=crop)
                    _eq(both, ops.dibr_warp(f, full, dp, out_u8=False, crop=crop), (H, W, crop, kw, mode, "UpDep vs upsample + FullDep"))
                    for b in range(2):
                        _eq(both[b], ops.dibr_warp(f[b], d[b], dp, out_u8=False, crop=crop), (H, W, crop, kw, mode, "batch row", b))
            dp = ops.dibr_params(display_mode="Full-SBS", depth_ratio=3.0)
            _eq(ops.dibr_warp(f, d, dp, crop=crop), ops.dibr_warp(f, full, dp, crop=crop), (H, W, crop, "uint8"))


def test_cropped_warp_shape_and_content(dev):
    """The eye is the crop's pixel size, and away from the edges it shows the cropped part of the uncropped eye: a letterbox crop of whole
    rows samples the same texels as the uncropped warp's rows y0..y1."""
    from desktop2stereo_amd import crop as K, ops
    f, d = _scene(dev, 96, 160, 95)
    dp = ops.dibr_params(display_mode="Full-SBS", depth_ratio=3.0)
    crop = (0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0)
    x0, y0, x1, y1 = K.pixel_bounds(160, 96, crop)
    got = ops.dibr_warp(f, d, dp, out_u8=False, crop=crop).cpu().numpy()
    assert got.shape == (y1 - y0, 2 * (x1 - x0), 3) == (64, 320, 3)
    whole = ops.dibr_warp(f, d, dp, out_u8=False).cpu().numpy()
    diff = np.abs(got - whole[y0:y1])
    assert (diff <= 0.05).mean() >= 0.98, float((diff > 0.05).mean())          # same texels up to the rounding of cy + v * ch
    assert np.abs(got - whole[:64]).max() > 20                                  # and it is not the uncropped top


def test_view_pipeline_crop_equals_pipeline_then_cropped_warp(dev):
    """Engine.view_pipeline_crop on the tiny engine == Engine.pipeline(want_depth=True)'s depth + dibr_warp(crop=), over two calls with
    the EMA state advancing in both; its depth_full is that map; depth.pipeline's refusals."""
    from desktop2stereo_amd import _lib, ops, synth
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
        for call, (crop, mode, u8) in enumerate([((0.0, 0.13, 1.0, 0.74), "Full-SBS", False), ((0.125, 0.0, 0.75, 1.0), "Half-TAB", True)]):
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, mode, corner_radius=0.03, alpha="rgba")
            f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 60 + 7 * call + b, "boxes")[0] for b in range(batch)])).to(dev)
            got, got_depth = fused.view_pipeline_crop(f, p, dp, crop, use_ema=True, out_u8=u8, want_depth=True)
            _, depth = plain.pipeline(f, p, sp, use_ema=True, want_depth=True)
            _eq(got_depth, depth, (call, "depth_full"))
            _eq(got, ops.dibr_warp(f, depth, dp, out_u8=u8, crop=crop), (call, crop, mode))
            assert tuple(got.shape[1:3]) == ops.dibr_crop_shape(H, W, crop, dp.display_mode)
        with pytest.raises(_lib.D2SError):
            fused.view_pipeline_crop(f, p, dp, (0.0, 0.5, 1.0, 0.6))
        with pytest.raises(_lib.D2SError):
            fused.view_pipeline_crop(torch.zeros((1, 300, 300, 3), dtype=torch.uint8, device=dev), p, dp, (0.0, 0.1, 1.0, 0.8))
    finally:
        fused.close(); plain.close()


def test_depth_pipeline_crop_surface(dev):
    """depth.pipeline(inpaint=True, crop=...): a fixed rectangle equals Engine.view_pipeline_crop; "auto" keeps one MovieCrop per stream
    slot, the first call shows the full frame (its detection is still in flight), a later call the detected picture; slots that
    disagree give a list of rows; the refusals."""
    from desktop2stereo_amd import crop as K, depth as D, ops, synth
    from desktop2stereo_amd.config import PipelineParams
    saved = dict(D._state)
    p = PipelineParams(depth_resolution=140)
    H, W = 270, 480
    try:
        D._state["engine"] = None
        D.configure("tiny", params=p, precision="fp32", max_batch=2)
        film = np.stack([synth.letterbox_frame(H, W, 40 + s, top=34, bottom=35) for s in range(2)])
        t = torch.from_numpy(film).to(dev)
        crop = (0.0, 0.13, 1.0, 0.74)
        out = D.pipeline(film, display_mode="Full-SBS", inpaint=True, crop=crop)
        dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, "Full-SBS")
        _eq(out, D._state["engine"].view_pipeline_crop(t, p, dp, crop), "fixed crop")
        now = [5.0]
        for s in range(2):
            D.movie_crop(s).clock = lambda: now[0]
        first = D.pipeline(film, display_mode="Full-SBS", inpaint=True, crop="auto")
        assert first.shape == (2, H, 2 * W, 3) and all(D.movie_crop(s).pending for s in range(2))
        torch.cuda.synchronize(dev)
        now[0] += 0.1                                                        # inside the interval: the call only polls
        second = D.pipeline(film, display_mode="Full-SBS", inpaint=True, crop="auto")
        want = K.crop_from_stats(ops.crop_detect(t[0]).tolist(), W, H)
        assert K.is_active(want) and D.movie_crop(0).crop_uv == want == D.movie_crop(1).crop_uv
        x0, y0, x1, y1 = K.pixel_bounds(W, H, want)
        assert second.shape == (2, y1 - y0, 2 * (x1 - x0), 3) and y1 - y0 < H - 60
        _eq(second, D._state["engine"].view_pipeline_crop(t, p, dp, want), "auto crop")
        D.movie_crop(1).mode = "off"                                         # the slots disagree: rows of different sizes
        rows = D.pipeline(film, display_mode="Full-SBS", inpaint=True, crop="auto")
        assert isinstance(rows, list) and rows[0].shape == (1, y1 - y0, 2 * (x1 - x0), 3) and rows[1].shape == (1, H, 2 * W, 3)
        with pytest.raises(ValueError):
            D.pipeline(film, crop=crop)                                      # the torch warp has no crop
        with pytest.raises(ValueError):
            D.pipeline(film, display_mode="Anaglyph", crop=crop)
        with pytest.raises(ValueError):
            D.pipeline(film, display_mode="Full-SBS", inpaint=True, crop="sometimes")
    finally:
        if D._state.get("engine") is not None:
            D._state["engine"].close()
        D._state.clear()
        D._state.update(saved)


def test_depth_pipeline_crop_rows_keep_their_stream_slots(dev):
    """Slots that disagree on the crop are served row by row.  On a Video-Depth-Anything engine each of those calls must name the
    row's OWN slot -- with streams=None too (row r is slot r) -- so that the slot's temporal window and EMA advance as in the one-call
    form: over three calls with per-stream EMA every row is bit-identical to view_pipeline_crop(..., streams=[slot]) on an engine
    that only ever saw that stream; then the same with the slots named in another order."""
    from desktop2stereo_amd import depth as D, ops, synth
    from desktop2stereo_amd.config import PipelineParams, engine_shape
    saved = dict(D._state)
    H, W, res = 90, 160, 84
    p = PipelineParams(depth_resolution=res)
    h, w, _ = engine_shape(H, W, res)
    solo = {}
    try:
        D._state["engine"] = None
        D.configure("vda_tiny", params=p, precision="fp32", max_batch=2)
        solo = {k: ops.Engine(D._state["cfg"], D._state["weights"], h, w, 2, "fp32", temporal=True) for k in range(2)}
        for k, size in enumerate([(1.0, 0.7), (0.8, 1.0)]):                 # a letterboxed film in slot 0, a pillarboxed one in slot 1
            D.movie_crop(k).mode = "manual"
            D.movie_crop(k).set_manual(*size)
        dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, "Full-SBS")
        frame = lambda k, i: synth.dibr_scene(H, W, 100 * (k + 1) + i, "boxes")[0]
        seen = {0: 0, 1: 0}
        for ids in (None, None, [1, 0], None):
            order = ids or [0, 1]
            f = np.stack([frame(k, seen[k]) for k in order])
            rows = D.pipeline(f, display_mode="Full-SBS", use_temporal_smooth=True, out_u8=False, inpaint=True, crop="auto", streams=ids)
            assert isinstance(rows, list) and rows[0].shape != rows[1].shape
            t = torch.from_numpy(f).to(dev)
            for r, k in enumerate(order):
                alone = solo[k].view_pipeline_crop(t[r:r + 1], p, dp, D.movie_crop(k).crop_uv, use_ema=True, out_u8=False, streams=[k])
                _eq(rows[r], alone, ("slot", k, "row", r, "streams", ids, "frame", seen[k]))
                seen[k] += 1
    finally:
        for e in solo.values():
            e.close()
        if D._state.get("engine") is not None:
            D._state["engine"].close()
        D._state.clear()
        D._state.update(saved)


def test_crop_detect_workspaces_are_per_stream(dev):
    """The detector's partial sums live in its workspace between the two launches: the shared one is kept per (device, stream, size),
    a MovieCrop owns its own, and two streams running the detector at once give each its own result."""
    from desktop2stereo_amd import crop as K, ops, synth
    a = torch.from_numpy(synth.letterbox_frame(96, 160, 4, top=16, bottom=16)).to(dev)
    b = torch.from_numpy(synth.letterbox_frame(96, 160, 6, left=20, right=20)).to(dev)
    want_a, want_b = ops.crop_detect(a).clone(), ops.crop_detect(b).clone()
    torch.cuda.synchronize(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    outs = []
    for _ in range(20):
        with torch.cuda.stream(s1):
            ga = ops.crop_detect(a)
        with torch.cuda.stream(s2):
            gb = ops.crop_detect(b)
        outs.append((ga, gb))
    torch.cuda.synchronize(dev)
    keys = [k for k in ops._CROP_WS if k[2:] == (1, 96, 160)]
    assert len({k[1] for k in keys}) >= 3 and len({ops._CROP_WS[k].data_ptr() for k in keys}) == len(keys)
    for ga, gb in outs:
        assert torch.equal(ga, want_a) and torch.equal(gb, want_b)
    m1, m2 = K.MovieCrop(), K.MovieCrop()
    assert m1.update(a) and m2.update(a)
    torch.cuda.synchronize(dev)
    assert next(iter(m1._bufs.values()))[0].data_ptr() != next(iter(m2._bufs.values()))[0].data_ptr()
