"""GPU: the veil and frosted looks around the curved OpenXR screen (d2s_dibr_xr_eyes_frost_curved, ops.dibr_xr_eyes_frost_curved,
Engine.view_pipeline_xr_frost_curved, depth.xr_eye_views_frost; reference xr_viewer/effects.py:189-254, 759-787).

PINNED by tests/golden/xr_frost_curved.npz -- the reference's 588 vertices drawn after its curved strip per eye on SwiftShader
(make_golden_xr_frost_curved.py) -- through the restatement tests/xr_frost_curved_ref.py, which tests/test_xr_frost_curved_oracle.py
holds to those renders.
  * Every case against the float64 rasteriser of the RECORDED triangles, on the pixels whose class is uniform on 3 x 3.  The bound is
    measured, not chosen: the manifest records, per case and eye, the maximum |rgb| difference of a float32 emulation of the kernel's
    walk against that rasteriser; the kernel is allowed TWICE that (its rounding order and its exp2 / log2 are not numpy's), the
    margin the flat frost uses.  Quantised, no rgb value is more than 1 level off; alpha is exact where the emulation's is.
  * Pixels no wall covers are bit-identical to dibr_xr_eyes on the same curved screen; the empty looks and frost off over the whole
    image; a flat screen through the new entry is dibr_xr_eyes_frost.
  * D2S_XR_BIN=0 (every pixel walks all 244 rows) against the default, bit for bit: every case, float32 and uint8, a full- and a
    model-resolution depth map; one 2064 x 2208 call with eyes of different sizes that are no multiple of the 64-pixel region.
  * noise_scale 54 against the float32 emulation pixel by pixel, as the flat test holds it.
  * A batch is its frames; a model-resolution depth map is its up-sampled self; the view pipeline is pipeline + eye call;
    depth.xr_eye_views_frost with a curved screen is the engine method; a refused call leaves `out` untouched."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = {1: "veil", 2: "frosted"}
CASES = ["veil_h_front", "veil_v_front", "veil_h_oblique", "veil_v_crop_corner", "veil_h_outside", "veil_h_near", "veil_h_end", "frosted_h_default",
         "frosted_v_time", "frosted_h_odd", "frosted_v_small_lod9", "frosted_h_dark", "frosted_v_empty", "veil_h_empty"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    import xr_frost_curved_ref as K
    return K.load(golden_dir)


@pytest.fixture(scope="module")
def scenes(fixtures):
    """{case: (rgb, depth, restated chain)}, computed once."""
    import xr_frost_curved_ref as K
    import xr_glow_ref as R
    out = {}
    for c in fixtures[1]["cases"]:
        img, dep = K.case_scene(c)
        out[c["name"]] = (img, dep, R.chain(img))
    return out


@contextlib.contextmanager
def _no_bins():
    """D2S_XR_BIN=0 for the calls inside: the library reads it at every call."""
    old = os.environ.get("D2S_XR_BIN")
    os.environ["D2S_XR_BIN"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["D2S_XR_BIN"]
        else:
            os.environ["D2S_XR_BIN"] = old


def _eq(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        pytest.fail(f"{what}: differ in {int((d > 0).sum())} of {d.size} values, max |diff| {d.max():.3e}")


def _case(fixtures, name):
    return next(c for c in fixtures[1]["cases"] if c["name"] == name)


def _frost(c, **kw):
    from desktop2stereo_amd import xr
    fr = dict(c["frost"], **kw)
    return xr.XrFrost(**dict(fr, mode=MODES[fr["mode"]], head=tuple(fr["head"])))


def _case_args(dev, c, scenes, alpha=None):
    from desktop2stereo_amd import ops, xr
    img, dep, _ = scenes[c["name"]]
    dp = ops.dibr_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], corner_radius=c["corner_radius"], alpha=alpha or c["alpha_mode"])
    screen = xr.XrScreen(clear=tuple(c["clear"]), **c["screen"])
    eyes = [xr.xr_eye(np.array(e["vp"]), e["size"][0], e["size"][1], e["eye"]) for e in c["eyes"]]
    f = torch.from_numpy(img).to(dev)
    frost = _frost(c)
    levels = ops.mip_chain(f) if frost.mode == "frosted" else None          # the veil never reads levels: None is what it gets
    return f, torch.from_numpy(dep).to(dev), dp, screen, eyes, frost, levels


_RUNS = {}


def _run(dev, fixtures, scenes, name):
    """One case through the library and the restatement, once per module."""
    if name in _RUNS:
        return _RUNS[name]
    import xr_frost_curved_ref as K
    from desktop2stereo_amd import ops
    z, _ = fixtures
    c = _case(fixtures, name)
    f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes)
    got = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
    got8 = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=True)
    plain = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=False)
    pre = c["alpha_mode"] == "premultiplied"
    recs = []
    for e, g, g8, p in zip(c["eyes"], got, got8, plain):
        w, h = e["size"]
        assert tuple(g.shape) == (1, h, w, 3 if pre else 4) and g8.dtype == torch.uint8
        g, g8, p = (t[0].cpu().numpy().astype(np.float64) for t in (g, g8, p))
        assert np.isfinite(g).all()
        want, cls, info = K.case_render(c, e, *scenes[name], z[f"{name}_verts"])
        ok = K.uniform3x3(cls)
        assert 1.0 - ok.mean() <= 0.15
        hits32 = K.walk_hits(K.lib_rows(c["screen"], c["frost"]["head"], np.array(e["vp"]), w, h), w, h, np.float32, attrs=False)
        free = ok & (K.wall_counts(hits32, w, h).sum(0) == 0) & (info["n_walls"] == 0)
        recs.append(dict(e=e, g=g, g8=g8, plain=p, ref=want[..., :3] * want[..., 3:] if pre else want[..., :3], want_a=None if pre else want[..., 3],
                         ok=ok, info=info, free=np.ones((h, w), bool) if c.get("empty") else free))
    _RUNS[name] = (c, recs)
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_curved_frost_eyes_match_the_float64_restatement(dev, fixtures, scenes, name):
    """Over EVERY compared pixel: twice the float32 emulation's recorded maximum against float64, per case and eye; uint8 never more
    than 1 level off; alpha exact where the emulation's is."""
    c, recs = _run(dev, fixtures, scenes, name)
    failures = []
    for r in recs:
        e, ok, info = r["e"], r["ok"], r["info"]
        dd = np.abs(r["g"][..., :3] - r["ref"])[ok]
        bound = 2.0 * e["f32"][3]
        q = np.abs(r["g8"][..., :3] - np.rint(np.clip(r["ref"], 0, 255)))[ok]
        line = f"[curved frost eye vs float64 restatement, {name} eye {e['eye']}] max |rgb| {dd.max():.5f} level (allowed {bound:.5f}) mean {dd.mean():.6f} uint8 max {q.max():.0f}"
        if r["want_a"] is not None:
            da = np.abs(r["g"][..., 3] - r["want_a"])[ok]
            line += f" alpha max {da.max():.2e} (emulation {e['f32'][2]:.2e})"
            if not da.max() <= 2.0 * e["f32"][2]:
                failures.append(("alpha", e["eye"], float(da.max())))
        print("\n" + line)
        dfull = np.abs(r["g"][..., :3] - r["ref"]).max(-1)
        parts = {"walls beside the screen": ok & (info["n_walls"] >= 1) & ~info["covered"], "walls over the screen": ok & (info["n_walls"] >= 1) & info["covered"],
                 "screen alone": ok & (info["n_walls"] == 0) & info["covered"], "clear": ok & (info["n_walls"] == 0) & ~info["covered"]}
        print("    " + "; ".join(f"{k}: {int(m.sum())} px max {dfull[m].max() if m.any() else 0.0:.5f}" for k, m in parts.items()))
        if not dd.max() <= bound:
            failures.append(("rgb", e["eye"], float(dd.max()), bound))
        if not q.max() <= 1:
            failures.append(("uint8", e["eye"], float(q.max())))
    assert not failures, failures


@pytest.mark.parametrize("name", CASES)
def test_wall_pixels_meet_the_bound_and_the_rest_is_dibr_xr_eyes(dev, fixtures, scenes, name):
    """Every compared pixel a wall covers is within the doubled emulation maximum; what no wall covers is dibr_xr_eyes' pixel on the same
    curved screen bit for bit (an undrawn look: every pixel of the image); and a drawn look does change the image."""
    c, recs = _run(dev, fixtures, scenes, name)
    for r in recs:
        e, wall = r["e"], r["ok"] & (r["info"]["n_walls"] >= 1)
        if c.get("empty"):
            assert np.array_equal(r["g"], r["plain"])
            continue
        dd = np.abs(r["g"][..., :3] - r["ref"])[wall]
        print(f"\n[wall pixels vs float64 restatement, {name} eye {e['eye']}] {int(wall.sum())} px max |rgb| {dd.max():.5f} level (allowed {2.0 * e['f32'][3]:.5f})")
        assert dd.max() <= 2.0 * e["f32"][3], (e["eye"], float(dd.max()))
        assert r["free"].sum() >= 1500 and np.array_equal(r["g"][r["free"]], r["plain"][r["free"]]), (e["eye"], "pixels no wall covers differ from dibr_xr_eyes")
        assert not np.array_equal(r["g"], r["plain"]), "no wall was drawn"


@pytest.mark.parametrize("name", CASES)
def test_walking_every_row_is_the_binned_walk_bit_for_bit(dev, fixtures, scenes, name):
    from desktop2stereo_amd import ops, synth
    c = _case(fixtures, name)
    f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes)
    ds = torch.from_numpy(synth.dibr_scene(24, 40, c["seed"], "boxes")[1]).to(dev)
    for depth in (d, ds):                                    # FullDep, UpDep
        for u8 in (False, True):
            binned = ops.dibr_xr_eyes_frost_curved(f, depth, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=u8)
            with _no_bins():
                every = ops.dibr_xr_eyes_frost_curved(f, depth, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=u8)
            for i in range(2):
                _eq(binned[i], every[i], (name, "binned vs all rows", "u8" if u8 else "f32", tuple(depth.shape), "eye", i))


def test_the_bins_at_headset_size_with_eyes_that_are_no_multiple_of_the_region(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, xr
    for name in ("veil_h_outside", "frosted_v_time"):
        c = _case(fixtures, name)
        f, d, dp, screen, _, frost, levels = _case_args(dev, c, scenes)
        eyes = [xr.xr_eye(np.array(c["eyes"][0]["vp"]), 2064, 2208, 0), xr.xr_eye(np.array(c["eyes"][1]["vp"]), 2001, 2101, 1)]
        assert 2064 % 64 and 2208 % 64 and 2001 % 64 and 2101 % 64
        binned = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=True)
        with _no_bins():
            every = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=True)
        plain = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=True)
        for i in range(2):
            assert bool(torch.equal(binned[i], every[i])), (name, "binned vs all rows at headset size, eye", i)
            assert not bool(torch.equal(binned[i], plain[i]))


def test_an_undrawn_look_is_dibr_xr_eyes_and_a_flat_screen_is_dibr_xr_eyes_frost(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, xr
    c = _case(fixtures, "veil_v_crop_corner")
    f, d, dp, screen, eyes, frost, _ = _case_args(dev, c, scenes)
    levels = ops.mip_chain(f)
    for u8 in (False, True):
        want = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=u8)
        for fr, lv in ((None, None), (xr.XrFrost(mode="off"), None), (xr.XrFrost(mode="off", intensity=float("nan")), levels),
                       (_frost(c, intensity=0.0), None), (xr.XrFrost.frosted(multiplier=0.0), levels), (_frost(c, alpha=0.002), None)):
            got = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, fr, lv, crop=c["crop"], out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], ("undrawn", fr, u8, i))
        flat = xr.XrScreen(**dict(c["screen"], curve="flat"), clear=tuple(c["clear"]))
        for fr, lv in ((frost, None), (xr.XrFrost.frosted(time=1.5), levels)):
            got = ops.dibr_xr_eyes_frost_curved(f, d, dp, flat, eyes, fr, lv, crop=c["crop"], out_u8=u8)
            want_flat = ops.dibr_xr_eyes_frost(f, d, dp, flat, eyes, fr, lv, crop=c["crop"], out_u8=u8)
            for i in range(2):
                _eq(got[i], want_flat[i], ("flat screen", fr.mode, u8, i))


def test_uint8_alpha_modes_and_model_resolution_depth(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, synth
    for name in ("veil_h_outside", "frosted_v_time"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes, alpha="rgba")
        f32 = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        u8 = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=True)
        for a, b in zip(f32, u8):
            want = torch.cat([a[..., :3], a[..., 3:] * 255.0], -1).clamp(0, 255).round().to(torch.uint8)      # round(): half to even
            _eq(b, want, (name, "uint8 vs rounded float32"))
        dp3 = _case_args(dev, c, scenes, alpha="window")[2]
        rgb = ops.dibr_xr_eyes_frost_curved(f, d, dp3, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        dpm = _case_args(dev, c, scenes, alpha="premultiplied")[2]
        pre = ops.dibr_xr_eyes_frost_curved(f, d, dpm, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        for a, b, m in zip(f32, rgb, pre):
            _eq(b, a[..., :3].contiguous(), (name, "window = the rgb of rgba"))
            _eq(m, (a[..., :3] * a[..., 3:]).contiguous(), (name, "premultiplied = rgb * a of rgba"))      # (clear alpha 1: every pixel)
        # a depth map at the model's resolution equals its up-sampled self: the wall pixels beside the screen do not read it at all, the
        # screen's read it as dibr_xr_eyes does
        small = synth.dibr_scene(24, 40, c["seed"], "boxes")[1]
        ds = torch.from_numpy(small).to(dev)
        got = ops.dibr_xr_eyes_frost_curved(f, ds, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        plain_s = ops.dibr_xr_eyes(f, ds, dp, screen, eyes, crop=c["crop"], out_u8=False)
        plain_f = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=False)
        for g, a, ps, pf in zip(got, f32, plain_s, plain_f):
            same_screen = (ps == pf).all(-1)                 # pixels whose screen value does not depend on the map: there the two runs agree
            assert bool(((g == a).all(-1) | ~same_screen).all()), name
            off_wall = (a == pf).all(-1)                     # no wall drew at full resolution: none draws here, the pixel is dibr_xr_eyes'
            assert bool(((g == ps).all(-1) | ~off_wall).all()), name
            assert not torch.equal(g, a) and bool(off_wall.any()) and not bool(off_wall.all())


def test_a_batch_is_its_frames_with_eyes_of_two_sizes(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, synth, xr
    for name in ("veil_h_oblique", "frosted_v_small_lod9"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes, alpha="rgba")
        both = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        for i in range(2):
            _eq(ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, [eyes[i]], frost, levels, crop=c["crop"], out_u8=False)[0], both[i],
                (name, "n_eyes = 1, eye", i))
        other = synth.dibr_scene(f.shape[0], f.shape[1], 77, "boxes")
        f2, d2 = torch.stack([f, torch.from_numpy(other[0]).to(dev)]), torch.stack([d, torch.from_numpy(other[1]).to(dev)])
        lv2 = ops.mip_chain(f2) if levels is not None else None
        small = xr.xr_eye(np.array(c["eyes"][1]["vp"]), 70, 51, 1)
        batch = ops.dibr_xr_eyes_frost_curved(f2, d2, dp, screen, [eyes[0], small], frost, lv2, crop=c["crop"], out_u8=False)
        assert tuple(batch[0].shape) == (2, 100, 130, 4) and tuple(batch[1].shape) == (2, 51, 70, 4)
        for b in range(2):
            one = ops.dibr_xr_eyes_frost_curved(f2[b], d2[b], dp, screen, [eyes[0], small], frost, None if lv2 is None else lv2[b:b + 1],
                                                crop=c["crop"], out_u8=False)
            for i in range(2):
                _eq(batch[i][b:b + 1], one[i], (name, "batch row", b, "eye", i))
        _eq(batch[0][0:1], both[0], (name, "row 0 of the batch"))
        assert not torch.equal(batch[0][0], batch[0][1])


def test_noise_scale_54_matches_the_float32_emulation_pixel_by_pixel(dev, fixtures, scenes):
    import xr_frost_curved_ref as K
    from desktop2stereo_amd import ops
    z, meta = fixtures
    c = dict(_case(fixtures, "frosted_v_time"))
    c["frost"] = dict(c["frost"], noise_scale=54.0)
    f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes)
    assert frost.noise_scale == 54.0
    got = ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
    # the frosted cases' largest recorded emulation-against-float64 maximum, doubled: the same arithmetic differences, no cell flips
    bound = 2.0 * max(e["f32"][3] for k in meta["cases"] if k["frost"]["mode"] == 2 for e in k["eyes"])
    verts = z["frosted_v_time_verts"]
    for e, g in zip(c["eyes"], got):
        g = g[0].cpu().numpy().astype(np.float64)
        emu, _, i32 = K.case_render(c, e, *scenes["frosted_v_time"], None, np.float32)
        _, _, i64 = K.case_render(c, e, *scenes["frosted_v_time"], verts, np.float64)
        geom_ok = K.uniform3x3(i64["geom"]) & (i32["geom"] == i64["geom"])
        wall = geom_ok & (i64["n_walls"] >= 1)
        flip = wall & (i32["cells"] != i64["cells"])
        ok = geom_ok & ~flip
        dd = np.abs(g[..., :3] - emu[..., :3].astype(np.float64))[ok]
        da = np.abs(g[..., 3] - emu[..., 3].astype(np.float64))[ok]
        cells = len(np.unique(i64["cells"][wall]))
        print(f"\n[noise_scale 54, eye {e['eye']}] {int(wall.sum())} wall pixels in {cells} noise cells, {int(flip.sum())} skipped (cell ids differ: "
              f"{flip.sum() / max(wall.sum(), 1):.3%}); max |rgb| {dd.max():.5f} level (allowed {bound:.5f}) alpha max {da.max():.2e}")
        assert wall.sum() >= 1500 and cells >= 54 and flip.sum() <= 0.02 * wall.sum()
        assert dd.max() <= bound and da.max() <= 1e-6, (e["eye"], float(dd.max()), float(da.max()))


def test_view_pipeline_xr_frost_curved_equals_pipeline_then_the_eye_call(dev, fixtures):
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
    c = _case(fixtures, "veil_v_front")
    eyes = [xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in c["eyes"]]
    try:
        for call, (frost, crop, u8, curve) in enumerate([(xr.XrFrost.veil(), None, False, "vertical"),
                                                         (xr.XrFrost.frosted(time=2.5), (0.0, 0.13, 1.0, 0.74), True, "horizontal")]):
            screen = xr.XrScreen(**dict(c["screen"], curve=curve))
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, corner_radius=0.03, alpha="rgba")
            f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 60 + 7 * call + b, "boxes")[0] for b in range(batch)])).to(dev)
            levels = ops.mip_chain(f) if frost.mode == "frosted" else None
            got, got_depth = fused.view_pipeline_xr_frost_curved(f, p, dp, screen, eyes, frost, levels, crop=crop, use_ema=True, out_u8=u8, want_depth=True)
            _, depth = plain.pipeline(f, p, sp, use_ema=True, want_depth=True)
            _eq(got_depth, depth, (call, "depth_full"))
            want = ops.dibr_xr_eyes_frost_curved(f, depth, dp, screen, eyes, frost, levels, crop=crop, out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], (call, frost.mode, "eye", i))
            off = ops.dibr_xr_eyes(f, depth, dp, screen, eyes, crop=crop, out_u8=u8)
            assert not torch.equal(off[0], want[0])                               # and the walls are there
    finally:
        fused.close(); plain.close()


def test_depth_xr_eye_views_frost_takes_a_curved_screen(dev, fixtures):
    """depth.xr_eye_views_frost sends a curved screen to Engine.view_pipeline_xr_frost_curved (it used to raise): bit-identical to that
    method on the module's engine, and a flat screen still goes where it went."""
    from desktop2stereo_amd import depth as D, ops, synth, xr
    from desktop2stereo_amd.config import PipelineParams
    c = _case(fixtures, "veil_v_front")
    eyes = [xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in c["eyes"]]
    p = PipelineParams(depth_resolution=140)
    D.configure("tiny", params=p, precision="fp32", max_batch=2)
    frames = np.stack([synth.dibr_scene(270, 480, 90 + b, "boxes")[0] for b in range(2)])
    try:
        for curve, look in (("vertical", "veil"), ("horizontal", "frosted"), ("flat", "veil")):
            screen = xr.XrScreen(**dict(c["screen"], curve=curve))
            got = D.xr_eye_views_frost(frames, screen, eyes, frost=look, time=1.25)
            assert len(got) == 2 and all(tuple(g.shape) == (2, 100, 130, 4) and g.dtype == torch.uint8 for g in got)
            eng = D._state["engine"]
            f = torch.from_numpy(frames).to(dev)
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, corner_radius=0.03, alpha="rgba")
            run = eng.view_pipeline_xr_frost if curve == "flat" else eng.view_pipeline_xr_frost_curved
            frost = xr.XrFrost.veil() if look == "veil" else xr.XrFrost.frosted(time=1.25)
            want = run(f, p, dp, screen, eyes, frost, ops.mip_chain(f) if look == "frosted" else None)
            plain = D.xr_eye_views(frames, screen, eyes)
            for i in range(2):
                _eq(got[i], want[i], (curve, "eye", i))
                assert not torch.equal(got[i], plain[i])        # and the walls are there
    finally:                                                # (the module's engine is this test's: leave none behind)
        if D._state["engine"] is not None:
            D._state["engine"].close()
        D._state["engine"], D._state["engine_key"] = None, None


def test_a_refused_call_leaves_out_untouched(dev, fixtures, scenes):
    from desktop2stereo_amd import _lib, ops, xr
    c = _case(fixtures, "frosted_v_small_lod9")
    f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes)
    _, total = ops.dibr_xr_shape(eyes, 1, dp.alpha_mode)
    out = torch.full((total,), -7.0, dtype=torch.float32, device=dev)                   # (no output value is negative)
    refused = [
        dict(screen=xr.XrScreen(**dict(c["screen"], normal_offset=0.02))),
        dict(frost=_frost(c, lod=-1.0)), dict(frost=_frost(c, noise_scale=-2.0)), dict(frost=_frost(c, time=float("inf"))),
        dict(frost=_frost(c, head=(0.0, float("nan"), 0.0))),
        dict(levels=None),                                                                    # frosted without its chain
        dict(screen=xr.XrScreen(width=1.6, height=0.96, distance=0.2, yaw=1.2, curve="horizontal")),      # the screen crosses the eye plane
    ]
    for kw in refused:
        a = dict(dict(screen=screen, frost=frost, levels=levels), **kw)
        with pytest.raises(_lib.D2SError):
            ops.dibr_xr_eyes_frost_curved(f, d, dp, a["screen"], eyes, a["frost"], a["levels"], out_u8=False, out=out)
    with pytest.raises(_lib.D2SError):                                                    # the flat entry keeps its refusal
        ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, out_u8=False, out=out)
    bad = frost.c_struct()
    bad.mode = 3
    with pytest.raises(_lib.D2SError):
        ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, bad, levels, out_u8=False, out=out)
    small_ws = torch.empty(2 * 52 * 96, dtype=torch.uint8, device=dev)                   # d2s_dibr_xr_frost_workspace's bytes: too few for 244 rows
    with pytest.raises(_lib.D2SError, match="d2s_dibr_xr_frost_curved_workspace"):
        ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, out_u8=False, out=out, workspace=small_ws)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, xr.XrFrost(mode="off"), None, out_u8=False, out=out, workspace=small_ws)      # undrawn: fewer bytes suffice
    assert not bool((out == -7.0).any())
    out.fill_(-7.0)
    ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, out_u8=False, out=out)      # and an accepted one writes every element
    assert not bool((out == -7.0).any())
