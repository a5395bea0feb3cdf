"""GPU: the veil and frosted looks around the flat OpenXR screen (d2s_dibr_xr_eyes_frost, ops.dibr_xr_eyes_frost,
Engine.view_pipeline_xr_frost; reference xr_viewer/effects.py:102-187, 789-857, xr_viewer/glsl.py:668-791).

PINNED by tests/golden/xr_frost.npz -- the reference's four wall strips drawn after its screen per eye on SwiftShader
(make_golden_xr_frost.py) -- through the restatement tests/xr_frost_ref.py, which tests/test_xr_frost_oracle.py holds to those renders.
  * Every case of the manifest against the float64 restatement over the RECORDED triangles, on the pixels whose class (screen / covering
    walls / noise cells) is uniform on 3 x 3.  The bound is measured, not chosen: the manifest records, per case and eye, the maximum
    |rgb| difference of a float32 emulation of the kernel's arithmetic against that restatement; the kernel is allowed TWICE that
    (its rounding order and its exp2 / log2 are not numpy's).  Quantised, no rgb value is more than 1 level from the restatement's;
    alpha is exact where the emulation's is (every case here).  Pixels no wall covers are bit-identical to dibr_xr_eyes.
  * noise_scale 54, the reference's default, GPU only: 1.5-pixel noise cells leave no 3 x 3 neighbourhood in one cell, so this case is
    held to the FLOAT32 emulation pixel by pixel on the pixels whose geometry class (screen / covering walls) is uniform, skipping only
    those where the emulation's and the float64 restatement's cell ids differ -- counted, at most 2 % of the wall pixels.
  * Everything else is bit identity or an exact rule: an undrawn look is dibr_xr_eyes over the whole image; uint8 is the rounded
    float32; a batch is its frames; a model-resolution depth map is its up-sampled self; the view pipeline is pipeline(depth_full) +
    dibr_xr_eyes_frost; a refused call leaves `out` untouched."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = {1: "veil", 2: "frosted"}
CASES = ["veil_front", "veil_oblique", "veil_crop_corner", "veil_outside", "veil_near", "frosted_default", "frosted_time", "frosted_odd",
         "frosted_small", "frosted_lod_low", "frosted_lod_high", "frosted_dark", "frosted_empty", "veil_empty"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    with open(os.path.join(golden_dir, "xr_frost.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_frost.npz")), json.load(f)


@pytest.fixture(scope="module")
def scenes(fixtures):
    """{case: (rgb, depth, restated chain)}, computed once."""
    import xr_frost_ref as F
    import xr_glow_ref as R
    out = {}
    for c in fixtures[1]["cases"]:
        img, dep = F.case_scene(c)
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
    """One case through the library and the restatement, once per module -> (case, [per eye: dict(g, g8, plain: the library's float32,
    uint8 and dibr_xr_eyes images as float64; ref: the float64 restatement's rgb as alpha_mode leaves it; want_a; ok; info; free: the
    compared pixels that neither the restatement's nor the kernel's own float32 walk puts under a wall)])."""
    if name in _RUNS:
        return _RUNS[name]
    import xr_frost_ref as F
    from desktop2stereo_amd import ops
    z, _ = fixtures
    c = _case(fixtures, name)
    f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes)
    got = ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
    got8 = ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=True)
    plain = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=False)
    pre = c["alpha_mode"] == "premultiplied"
    recs = []
    for e, g, g8, p in zip(c["eyes"], got, got8, plain):
        w, h = e["size"]
        assert tuple(g.shape) == (1, h, w, 3 if pre else 4) and g8.dtype == torch.uint8
        g, g8, p = (t[0].cpu().numpy().astype(np.float64) for t in (g, g8, p))
        assert np.isfinite(g).all()
        want, cls, info = F.case_render(c, e, *scenes[name], z[f"{name}_verts"])
        ok = F.uniform3x3(cls)
        assert 1.0 - ok.mean() <= 0.15
        hits32 = F.walk_hits(F.wall_rows(c["screen"], c["frost"]["head"], np.array(e["vp"]), w, h), w, h, np.float32)
        free = ok & ~np.any([k["hit"] for k in hits32], 0) & (info["n_walls"] == 0)
        recs.append(dict(e=e, g=g, g8=g8, plain=p, ref=want[..., :3] * want[..., 3:] if pre else want[..., :3], want_a=None if pre else want[..., 3],
                         ok=ok, info=info, free=np.ones((h, w), bool) if c.get("empty") else free))
    _RUNS[name] = (c, recs)
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_frost_eyes_match_the_float64_restatement(dev, fixtures, scenes, name):
    """Over EVERY compared pixel: twice the float32 emulation's recorded maximum against float64, per case and eye.  The emulation starts
    from the library's own geometry -- the screen and the walls formed in double precision from the screen's numbers, not from the
    reference's recorded float32 matrices, which the float64 restatement keeps -- and is then the kernel's pixel bit for bit on 98 to
    99.8 % of the screen's pixels (measured on an MI355X), so its maximum is the kernel's: the worst pixel is one where float32
    rounding of the texture coordinate meets a steep edge of the frame, up to 0.018 level."""
    c, recs = _run(dev, fixtures, scenes, name)
    failures = []
    for r in recs:
        e, ok, info = r["e"], r["ok"], r["info"]
        dd = np.abs(r["g"][..., :3] - r["ref"])[ok]
        bound = 2.0 * e["f32"][3]
        q = np.abs(r["g8"][..., :3] - np.rint(np.clip(r["ref"], 0, 255)))[ok]
        line = f"[frost eye vs float64 restatement, {name} eye {e['eye']}] max |rgb| {dd.max():.5f} level (allowed {bound:.5f}) mean {dd.mean():.6f} uint8 max {q.max():.0f}"
        if r["want_a"] is not None:
            da = np.abs(r["g"][..., 3] - r["want_a"])[ok]
            line += f" alpha max {da.max():.2e} (emulation {e['f32'][2]:.2e})"
            if not da.max() <= 2.0 * e["f32"][2]:          # 0 where the emulation's alpha is exact: every case of this manifest
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
    """The part of the check above that the new code answers for: every compared pixel a wall covers -- beside the screen or over it --
    is within the same doubled emulation maximum; what no wall covers is dibr_xr_eyes' pixel bit for bit (an undrawn look: every
    pixel of the image); and a drawn look does change the image."""
    c, recs = _run(dev, fixtures, scenes, name)
    for r in recs:
        e, wall = r["e"], r["ok"] & (r["info"]["n_walls"] >= 1)
        if c.get("empty"):
            assert not wall.any() and np.array_equal(r["g"], r["plain"])
            continue
        dd = np.abs(r["g"][..., :3] - r["ref"])[wall]
        print(f"\n[wall pixels vs float64 restatement, {name} eye {e['eye']}] {int(wall.sum())} px max |rgb| {dd.max():.5f} level (allowed {2.0 * e['f32'][3]:.5f})")
        assert dd.max() <= 2.0 * e["f32"][3], (e["eye"], float(dd.max()))
        assert r["free"].sum() >= 2000 and np.array_equal(r["g"][r["free"]], r["plain"][r["free"]]), (e["eye"], "pixels no wall covers differ from dibr_xr_eyes")
        assert not np.array_equal(r["g"], r["plain"]), "no wall was drawn"


def test_an_undrawn_look_is_dibr_xr_eyes_over_the_whole_image(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, xr
    c = _case(fixtures, "veil_crop_corner")
    f, d, dp, screen, eyes, frost, _ = _case_args(dev, c, scenes)
    levels = ops.mip_chain(f)
    for u8 in (False, True):
        want = ops.dibr_xr_eyes(f, d, dp, screen, eyes, crop=c["crop"], out_u8=u8)
        for fr, lv in ((None, None), (xr.XrFrost(mode="off"), None), (xr.XrFrost(mode="off", intensity=float("nan")), levels),
                       (_frost(c, intensity=0.0), None), (xr.XrFrost.frosted(multiplier=0.0), None), (xr.XrFrost.frosted(multiplier=0.0), levels),
                       (_frost(c, alpha=0.002), None)):
            got = ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, fr, lv, crop=c["crop"], out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], ("undrawn", fr, u8, i))
    curved = xr.XrScreen(**dict(c["screen"], curve="horizontal", distance=1.5))        # a curved screen is refused only with frost ON
    want = ops.dibr_xr_eyes(f, d, dp, curved, eyes, out_u8=False)
    got = ops.dibr_xr_eyes_frost(f, d, dp, curved, eyes, xr.XrFrost(mode="off"), None, out_u8=False)
    for i in range(2):
        _eq(got[i], want[i], ("frost off, curved", i))


def test_uint8_alpha_modes_and_model_resolution_depth(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, synth
    for name in ("veil_outside", "frosted_time"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes, alpha="rgba")
        f32 = ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        u8 = ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=True)
        for a, b in zip(f32, u8):
            want = torch.cat([a[..., :3], a[..., 3:] * 255.0], -1).clamp(0, 255).round().to(torch.uint8)      # round(): half to even
            _eq(b, want, (name, "uint8 vs rounded float32"))
        dp3 = _case_args(dev, c, scenes, alpha="window")[2]
        rgb = ops.dibr_xr_eyes_frost(f, d, dp3, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        dpm = _case_args(dev, c, scenes, alpha="premultiplied")[2]
        pre = ops.dibr_xr_eyes_frost(f, d, dpm, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        for a, b, m in zip(f32, rgb, pre):
            _eq(b, a[..., :3].contiguous(), (name, "window = the rgb of rgba"))
            _eq(m, (a[..., :3] * a[..., 3:]).contiguous(), (name, "premultiplied = rgb * a of rgba"))      # (clear alpha 1: every pixel)
        # a depth map at the model's resolution: the wall pixels beside the screen do not read it at all, the screen's read its
        # up-sampled self as dibr_xr_eyes does
        H, W = c["source"]
        small = synth.dibr_scene(24, 40, c["seed"], "boxes")[1]
        ds = torch.from_numpy(small).to(dev)
        got = ops.dibr_xr_eyes_frost(f, ds, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
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
    for name in ("veil_oblique", "frosted_small"):
        c = _case(fixtures, name)
        f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes, alpha="rgba")
        both = ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
        for i in range(2):
            _eq(ops.dibr_xr_eyes_frost(f, d, dp, screen, [eyes[i]], frost, levels, crop=c["crop"], out_u8=False)[0], both[i], (name, "n_eyes = 1, eye", i))
        other = synth.dibr_scene(f.shape[0], f.shape[1], 77, "boxes")
        f2, d2 = torch.stack([f, torch.from_numpy(other[0]).to(dev)]), torch.stack([d, torch.from_numpy(other[1]).to(dev)])
        lv2 = ops.mip_chain(f2) if levels is not None else None
        small = xr.xr_eye(np.array(c["eyes"][1]["vp"]), 70, 51, 1)
        batch = ops.dibr_xr_eyes_frost(f2, d2, dp, screen, [eyes[0], small], frost, lv2, crop=c["crop"], out_u8=False)
        assert tuple(batch[0].shape) == (2, 100, 130, 4) and tuple(batch[1].shape) == (2, 51, 70, 4)
        for b in range(2):
            one = ops.dibr_xr_eyes_frost(f2[b], d2[b], dp, screen, [eyes[0], small], frost, None if lv2 is None else lv2[b:b + 1], crop=c["crop"],
                                         out_u8=False)
            for i in range(2):
                _eq(batch[i][b:b + 1], one[i], (name, "batch row", b, "eye", i))
        _eq(batch[0][0:1], both[0], (name, "row 0 of the batch"))
        assert not torch.equal(batch[0][0], batch[0][1])


def test_noise_scale_54_matches_the_float32_emulation_pixel_by_pixel(dev, fixtures, scenes):
    import xr_frost_ref as F
    from desktop2stereo_amd import ops
    z, meta = fixtures
    c = dict(_case(fixtures, "frosted_time"))
    c["frost"] = dict(c["frost"], noise_scale=54.0)
    f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes)
    assert frost.noise_scale == 54.0
    got = ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, crop=c["crop"], out_u8=False)
    # the frosted cases' largest recorded emulation-against-float64 maximum, doubled: the same arithmetic differences, no cell flips
    bound = 2.0 * max(e["f32"][3] for k in meta["cases"] if k["frost"]["mode"] == 2 for e in k["eyes"])
    verts = z["frosted_time_verts"]
    for e, g in zip(c["eyes"], got):
        g = g[0].cpu().numpy().astype(np.float64)
        emu, _, i32 = F.case_render(c, e, *scenes["frosted_time"], verts, np.float32, mesh=False)
        _, _, i64 = F.case_render(c, e, *scenes["frosted_time"], verts, np.float64, mesh=True)
        geom_ok = F.uniform3x3(i64["geom"]) & (i32["geom"] == i64["geom"])
        wall = geom_ok & (i64["n_walls"] >= 1)
        flip = wall & (i32["cells"] != i64["cells"])
        ok = geom_ok & ~flip
        dd = np.abs(g[..., :3] - emu[..., :3].astype(np.float64))[ok]
        da = np.abs(g[..., 3] - emu[..., 3].astype(np.float64))[ok]
        cells = len(np.unique(i64["cells"][wall]))
        print(f"\n[noise_scale 54, eye {e['eye']}] {int(wall.sum())} wall pixels in {cells} noise cells, {int(flip.sum())} skipped (cell ids differ: "
              f"{flip.sum() / max(wall.sum(), 1):.3%}); max |rgb| {dd.max():.5f} level (allowed {bound:.5f}) alpha max {da.max():.2e}")
        assert wall.sum() >= 3000 and cells >= 2 * 54 and flip.sum() <= 0.02 * wall.sum()          # (54 cells along a wall: more than two walls' worth are seen)
        assert dd.max() <= bound and da.max() <= 1e-6, (e["eye"], float(dd.max()), float(da.max()))


def test_view_pipeline_xr_frost_equals_pipeline_then_frost_eyes(dev, fixtures):
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
    c = _case(fixtures, "veil_front")
    eyes = [xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in c["eyes"]]
    try:
        for call, (frost, crop, u8) in enumerate([(xr.XrFrost.veil(), None, False), (xr.XrFrost.frosted(time=2.5), (0.0, 0.13, 1.0, 0.74), True)]):
            screen = xr.XrScreen(**c["screen"])
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, corner_radius=0.03, alpha="rgba")
            f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 60 + 7 * call + b, "boxes")[0] for b in range(batch)])).to(dev)
            levels = ops.mip_chain(f) if frost.mode == "frosted" else None
            got, got_depth = fused.view_pipeline_xr_frost(f, p, dp, screen, eyes, frost, levels, crop=crop, use_ema=True, out_u8=u8, want_depth=True)
            _, depth = plain.pipeline(f, p, sp, use_ema=True, want_depth=True)
            _eq(got_depth, depth, (call, "depth_full"))
            want = ops.dibr_xr_eyes_frost(f, depth, dp, screen, eyes, frost, levels, crop=crop, out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], (call, frost.mode, "eye", i))
            off = ops.dibr_xr_eyes(f, depth, dp, screen, eyes, crop=crop, out_u8=u8)
            assert not torch.equal(off[0], want[0])                               # and the walls are there
    finally:
        fused.close(); plain.close()


def test_a_refused_call_leaves_out_untouched(dev, fixtures, scenes):
    from desktop2stereo_amd import _lib, ops, xr
    c = _case(fixtures, "frosted_small")
    f, d, dp, screen, eyes, frost, levels = _case_args(dev, c, scenes)
    _, total = ops.dibr_xr_shape(eyes, 1, dp.alpha_mode)
    out = torch.full((total,), -7.0, dtype=torch.float32, device=dev)                   # (no output value is negative)
    refused = [
        dict(screen=xr.XrScreen(**dict(c["screen"], curve="horizontal", distance=1.5))),      # curved + frost: unsupported
        dict(screen=xr.XrScreen(**dict(c["screen"], curve="vertical", distance=1.5)), frost=xr.XrFrost.veil()),
        dict(screen=xr.XrScreen(**dict(c["screen"], normal_offset=0.02))),
        dict(frost=_frost(c, lod=-1.0)), dict(frost=_frost(c, noise_scale=-2.0)), dict(frost=_frost(c, time=float("inf"))),
        dict(frost=_frost(c, head=(0.0, float("nan"), 0.0))),
        dict(levels=None),                                                                    # frosted without its chain
        dict(screen=xr.XrScreen(width=1.6, height=0.96, distance=0.2, yaw=1.2)),              # what dibr_xr_eyes refuses
    ]
    for kw in refused:
        a = dict(dict(screen=screen, frost=frost, levels=levels), **kw)
        with pytest.raises(_lib.D2SError):
            ops.dibr_xr_eyes_frost(f, d, dp, a["screen"], eyes, a["frost"], a["levels"], out_u8=False, out=out)
    bad = frost.c_struct()
    bad.mode = 3
    with pytest.raises(_lib.D2SError):
        ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, bad, levels, out_u8=False, out=out)
    small_ws = torch.empty(2 * 48 * 96, dtype=torch.uint8, device=dev)                   # d2s_dibr_xr_workspace's bytes: too few with walls
    with pytest.raises(_lib.D2SError):
        ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, out_u8=False, out=out, workspace=small_ws)
    with pytest.raises(ValueError):
        ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels[:, :-1], out_u8=False, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, xr.XrFrost(mode="off"), None, out_u8=False, out=out, workspace=small_ws)      # undrawn: the plain bytes suffice
    assert not bool((out == -7.0).any())
    out.fill_(-7.0)
    ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, out_u8=False, out=out)      # and an accepted one writes every element
    assert not bool((out == -7.0).any())
