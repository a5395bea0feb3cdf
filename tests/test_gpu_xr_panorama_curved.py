"""GPU: the panorama behind the CURVED OpenXR screen's glow, glow2, veil and frosted looks (d2s_dibr_xr_eyes_panorama_curved,
ops.dibr_xr_eyes_panorama_curved, Engine.view_pipeline_xr_panorama_curved).

PINNED by tests/golden/xr_panorama_curved.npz -- the reference's panorama pass drawn before its curved glow mesh, strip and walls per
eye on SwiftShader (make_golden_xr_panorama_curved.py) -- through the restatement tests/xr_panorama_curved_ref.py, which
tests/test_xr_panorama_curved_oracle.py holds to those renders.
  * Every case of the manifest against the float64 restatement over every compared pixel (class uniform on 3 x 3).  The rgb bound is
    measured, not chosen: the manifest records, per case and eye, the maximum |rgb| difference of a float32 emulation of the kernel's
    arithmetic against that restatement; the kernel is allowed TWICE that (its atan2 and log2 are not numpy's), alpha twice the
    recorded alpha figure.  Quantised, no rgb value is more than 1 level from the restatement's.
  * Everything else is bit identity or an exact rule: covered pixels are the curved look's own entry's; without a panorama the whole
    image is; on flat screens and the plain curved one the new entry is the old panorama entry; uint8 is the rounded float32; the
    alpha modes; a batch is its frames, with one panorama; a model-resolution depth map moves screen pixels only; the view pipeline is
    pipeline(depth_full) + dibr_xr_eyes_panorama_curved; a refused call leaves `out` untouched; the old door still refuses."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = {1: "veil", 2: "frosted"}
CASES = ["glow_h", "glow2_v", "glow_h_minified", "glow_h_seam_flip", "veil_h", "frosted_v", "veil_v_two_sizes", "frosted_h_yaw_exposure_flip"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    import xr_panorama_curved_ref as PC
    return PC.load(golden_dir)


@pytest.fixture(scope="module")
def scenes(fixtures):
    """{case: (rgb, depth, the frame's restated chain, the panorama, its restated chain)}, computed once."""
    import xr_glow_ref as R
    import xr_panorama_curved_ref as PC
    out = {}
    for c in fixtures[1]["cases"]:
        img, dep, pano = PC.case_scene(c)
        out[c["name"]] = (img, dep, R.chain(img), pano, R.chain(pano))
    return out


def _eq(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        pytest.fail(f"{what}: differ in {int((d > 0).sum())} of {d.size} values, max |diff| {d.max():.3e}")


def _case(fixtures, name):
    return next(c for c in fixtures[1]["cases"] if c["name"] == name)


def _looks(c):
    from desktop2stereo_amd import xr
    if c["kind"] == "glow_curved":
        return xr.XrGlow({1: "glow", 2: "glow2"}[c["mode"]], c["range_m"], c["inner_edge_fraction"]), None
    fr = c["frost"]
    return None, xr.XrFrost(**dict(fr, mode=MODES[fr["mode"]], head=tuple(fr["head"])))


def _pano_struct(c, eyes, shape):
    from desktop2stereo_amd import xr
    p = c["panorama"]
    return xr.XrPanorama(p["yaw_offset_deg"], p["exposure"], p["flip_y"]).c_struct([(np.array(e["proj"]), np.array(e["view"])) for e in eyes], shape)


def _case_args(dev, c, scenes, alpha=None):
    """dict of everything ops.dibr_xr_eyes_panorama_curved takes for a manifest case."""
    from desktop2stereo_amd import ops, xr
    img, dep, _, pano, _ = scenes[c["name"]]
    dp = ops.dibr_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], corner_radius=c["corner_radius"], alpha=alpha or c["alpha_mode"])
    screen = xr.XrScreen(clear=tuple(c["clear"]), **c["screen"])
    eyes = [xr.xr_eye(np.array(e["vp"]), e["size"][0], e["size"][1], e["eye"]) for e in c["eyes"]]      # (vp is already flipped where the eye is)
    f, pr = torch.from_numpy(img).to(dev), torch.from_numpy(pano).to(dev)
    glow, frost = _looks(c)
    need = glow is not None or frost.mode == "frosted"
    return dict(frames=f, depth=torch.from_numpy(dep).to(dev), dp=dp, screen=screen, eyes=eyes, panorama=_pano_struct(c, c["eyes"], pano.shape[:2]),
                pano_rgb=pr, pano_levels=ops.mip_chain(pr).view(-1), glow=glow, frost=frost, levels=ops.mip_chain(f) if need else None, crop=c["crop"])


def _own(a, out_u8, **kw):
    """The curved look's own entry, which knows no panorama."""
    from desktop2stereo_amd import ops
    a = dict(a, **kw)
    if a["frost"] is not None:
        return ops.dibr_xr_eyes_frost_curved(a["frames"], a["depth"], a["dp"], a["screen"], a["eyes"], a["frost"], a["levels"], crop=a["crop"], out_u8=out_u8)
    return ops.dibr_xr_eyes_glow_curved(a["frames"], a["depth"], a["dp"], a["screen"], a["eyes"], a["glow"], a["levels"], crop=a["crop"], out_u8=out_u8)


def _call(a, out_u8=False, fn=None, **kw):
    from desktop2stereo_amd import ops
    a = dict(a, **kw)
    return (fn or ops.dibr_xr_eyes_panorama_curved)(a["frames"], a["depth"], a["dp"], a["screen"], a["eyes"], a["panorama"], a["pano_rgb"],
                                                    a["pano_levels"], glow=a["glow"], frost=a["frost"], levels=a["levels"], crop=a["crop"],
                                                    out_u8=out_u8, out=a.get("out"), workspace=a.get("workspace"))


NO_PANO = dict(panorama=None, pano_rgb=None, pano_levels=None)


@pytest.mark.parametrize("name", CASES)
def test_curved_looks_over_the_panorama_match_the_float64_restatement(dev, fixtures, scenes, name):
    """Over EVERY compared pixel: twice the float32 emulation's recorded maximum against float64, per case and eye; uint8 within 1;
    alpha within twice the recorded figure.  Covered pixels are the look's own entry's bit for bit; without a panorama the whole
    image is, in float32 and uint8; and the panorama is there: uncovered pixels it shows through are not what the clear colour gives."""
    import xr_panorama_curved_ref as PC
    z, _ = fixtures
    c = _case(fixtures, name)
    a = _case_args(dev, c, scenes)
    got, got8 = _call(a), _call(a, out_u8=True)
    old, none = _own(a, False), _call(a, **NO_PANO)
    none8, old8 = _call(a, out_u8=True, **NO_PANO), _own(a, True)
    img, dep, levels, _, pano_levels = scenes[name]
    verts = z[f"{name}_verts"]
    failures = []
    for i, e in enumerate(c["eyes"]):
        w, h = e["size"]
        assert tuple(got[i].shape) == (1, h, w, 4) and got8[i].dtype == torch.uint8
        _eq(none[i], old[i], (name, "no panorama = the look's own entry, eye", i))
        _eq(none8[i], old8[i], (name, "no panorama = the look's own entry, uint8, eye", i))
        g, g8, o = (t[0].cpu().numpy().astype(np.float64) for t in (got[i], got8[i], old[i]))
        assert np.isfinite(g).all()
        want, cls, info = PC.case_render(c, e, img, dep, levels, pano_levels, verts)
        ok = PC.uniform3x3(cls)
        assert abs((1.0 - ok.mean()) - e["excluded"]) < 1e-12
        dd = np.abs(g[..., :3] - want[..., :3])[ok]
        da = np.abs(g[..., 3] - want[..., 3])[ok]
        q = np.abs(g8[..., :3] - np.rint(np.clip(want[..., :3], 0, 255)))[ok]
        bound, abound = 2.0 * e["f32"][3], max(2.0 * e["f32"][2], 1e-6)
        bgm = ok & ~info["covered"]
        dbg = np.abs(g[..., :3] - want[..., :3])[bgm]
        print(f"\n[curved look over the panorama vs float64 restatement, {name} eye {e['eye']}] max |rgb| {dd.max():.5f} level (allowed {bound:.5f}) "
              f"mean {dd.mean():.6f} uint8 max {q.max():.0f} alpha max {da.max():.2e} (allowed {abound:.2e}); background {int(bgm.sum())} px max "
              f"{dbg.max():.5f}, blended {int((bgm & (info['K'] > 0.05) & (info['K'] < 0.95)).sum())}, seam-quad px {int((bgm & info['seam']).sum())}")
        if not dd.max() <= bound:
            failures.append(("rgb", e["eye"], float(dd.max()), bound))
        if not q.max() <= 1:
            failures.append(("uint8", e["eye"], float(q.max())))
        if not da.max() <= abound:
            failures.append(("alpha", e["eye"], float(da.max()), abound))
        cov = info["covered"] & ok                                            # where the restatement and the kernel agree that a facet covers
        assert cov.sum() >= 100 and np.array_equal(g[cov], o[cov]), (name, e["eye"], "covered pixels differ from the look's own entry")
        seen = bgm & (info["K"] > 1e-3)                                       # uncovered, and what drew over it is not opaque: the panorama shows
        assert seen.sum() >= 1000 and (g[seen] != o[seen]).any(-1).all(), "an uncovered pixel is still what the clear colour gives"
    assert not failures, failures


def test_a_superset_flat_looks_and_the_plain_curved_screen_are_the_old_entry_s(dev, golden_dir):
    """xr_panorama.json's flat glow, flat veil and plain curved case through the new entry: bit for bit ops.dibr_xr_eyes_panorama."""
    import xr_glow_ref as R
    import xr_panorama_ref as P
    from desktop2stereo_amd import ops, xr
    with open(os.path.join(golden_dir, "xr_panorama.json")) as f:
        cases = {c["name"]: c for c in json.load(f)["cases"]}
    for name in ("glow_flat", "veil_flat", "curved_plain"):
        c = cases[name]
        img, dep, pano = P.case_scene(c)
        glow = frost = None
        if c["kind"] == "glow":
            glow = xr.XrGlow({1: "glow", 2: "glow2"}[c["glow"]["mode"]], c["glow"]["range_m"], c["glow"]["inner_edge_fraction"])
        if c["kind"] == "frost":
            frost = xr.XrFrost(**dict(c["frost"], mode=MODES[c["frost"]["mode"]], head=tuple(c["frost"]["head"])))
        f, pr = torch.from_numpy(img).to(dev), torch.from_numpy(pano).to(dev)
        a = dict(frames=f, depth=torch.from_numpy(dep).to(dev), screen=xr.XrScreen(clear=tuple(c["clear"]), **c["screen"]),
                 dp=ops.dibr_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], corner_radius=c["corner_radius"], alpha=c["alpha_mode"]),
                 eyes=[xr.xr_eye(np.array(e["vp"]), e["size"][0], e["size"][1], e["eye"]) for e in c["eyes"]],
                 panorama=_pano_struct(c, c["eyes"], pano.shape[:2]), pano_rgb=pr, pano_levels=ops.mip_chain(pr).view(-1), glow=glow, frost=frost,
                 levels=ops.mip_chain(f) if glow is not None else None, crop=c["crop"])
        for u8 in (False, True):
            new, old = _call(a, out_u8=u8), _call(a, out_u8=u8, fn=ops.dibr_xr_eyes_panorama)
            for i in range(2):
                _eq(new[i], old[i], (name, "the new entry = the old one, uint8" if u8 else "the new entry = the old one", i))
        assert not torch.equal(_call(a)[0], _call(a, **NO_PANO)[0])


def test_uint8_alpha_modes_and_model_resolution_depth(dev, fixtures, scenes):
    from desktop2stereo_amd import synth
    for name in ("glow_h", "frosted_h_yaw_exposure_flip", "veil_v_two_sizes"):
        c = _case(fixtures, name)
        a = _case_args(dev, c, scenes, alpha="rgba")
        f32, u8 = _call(a), _call(a, out_u8=True)
        for x, y in zip(f32, u8):
            want = torch.cat([x[..., :3], x[..., 3:] * 255.0], -1).clamp(0, 255).round().to(torch.uint8)      # round(): half to even
            _eq(y, want, (name, "uint8 vs rounded float32"))
        rgb = _call(a, dp=_case_args(dev, c, scenes, alpha="window")["dp"])
        pre = _call(a, dp=_case_args(dev, c, scenes, alpha="premultiplied")["dp"])
        for x, y, m in zip(f32, rgb, pre):
            assert tuple(y.shape[-1:]) == (3,) and tuple(m.shape[-1:]) == (3,)
            _eq(y, x[..., :3].contiguous(), (name, "window = the rgb of rgba"))
            _eq(m, (x[..., :3] * x[..., 3:]).contiguous(), (name, "premultiplied = rgb * a of rgba"))         # (the panorama's alpha is 1)
        # a depth map at the model's resolution: the background does not read it at all, the screen reads its up-sampled self
        small = torch.from_numpy(synth.dibr_scene(24, 40, c["seed"], "boxes")[1]).to(dev)
        got, old_s, old_f = _call(a, depth=small), _own(a, False, depth=small), _own(a, False)
        for g, x, os_, of in zip(got, f32, old_s, old_f):
            same_screen = (os_ == of).all(-1)                    # pixels whose value does not depend on the map
            assert bool(((g == x).all(-1) | ~same_screen).all()), name
            changed = ~same_screen                               # screen pixels: the look's own entry's, whatever lies behind
            assert bool(changed.any()) and bool((g[changed] == os_[changed]).all()), name


def test_a_batch_is_its_frames_with_one_panorama_and_one_eye_is_each_of_the_pair(dev, fixtures, scenes):
    from desktop2stereo_amd import ops, synth
    for name in ("glow2_v", "veil_v_two_sizes"):
        c = _case(fixtures, name)
        a = _case_args(dev, c, scenes, alpha="rgba")
        both = _call(a)
        for i in range(2):
            one = dict(a, eyes=[a["eyes"][i]], panorama=_pano_struct(c, [c["eyes"][i]], a["pano_rgb"].shape[:2]))
            _eq(_call(one)[0], both[i], (name, "n_eyes = 1, eye", i))
        f, d = a["frames"], a["depth"]
        other = synth.dibr_scene(f.shape[0], f.shape[1], 77, "boxes")
        f2, d2 = torch.stack([f, torch.from_numpy(other[0]).to(dev)]), torch.stack([d, torch.from_numpy(other[1]).to(dev)])
        lv2 = ops.mip_chain(f2) if a["levels"] is not None else None
        batch = _call(a, frames=f2, depth=d2, levels=lv2)
        sizes = [tuple(e["size"]) for e in c["eyes"]]
        assert [tuple(b.shape) for b in batch] == [(2, h, w, 4) for w, h in sizes]
        for b in range(2):
            one = _call(a, frames=f2[b], depth=d2[b], levels=None if lv2 is None else lv2[b:b + 1])
            for i in range(2):
                _eq(batch[i][b:b + 1], one[i], (name, "batch row", b, "eye", i))
        _eq(batch[0][0:1], both[0], (name, "row 0 of the batch"))
        assert not torch.equal(batch[0][0], batch[0][1])


def test_view_pipeline_xr_panorama_curved_equals_pipeline_then_the_eye_call(dev, fixtures, scenes):
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
    c = _case(fixtures, "glow_h")
    a = _case_args(dev, c, scenes)
    try:
        for call, (glow, frost, crop, u8) in enumerate([(xr.XrGlow("glow", 1.2), None, (0.0, 0.13, 1.0, 0.74), True),
                                                        (None, xr.XrFrost.frosted(time=2.5), None, False)]):
            dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, corner_radius=0.03, alpha="rgba")
            f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 60 + 7 * call + b, "boxes")[0] for b in range(batch)])).to(dev)
            levels = ops.mip_chain(f)
            got, got_depth = fused.view_pipeline_xr_panorama_curved(f, p, dp, a["screen"], a["eyes"], a["panorama"], a["pano_rgb"], a["pano_levels"],
                                                                    glow=glow, frost=frost, levels=levels, crop=crop, use_ema=True, out_u8=u8,
                                                                    want_depth=True)
            _, depth = plain.pipeline(f, p, sp, use_ema=True, want_depth=True)
            _eq(got_depth, depth, (call, "depth_full"))
            want = ops.dibr_xr_eyes_panorama_curved(f, depth, dp, a["screen"], a["eyes"], a["panorama"], a["pano_rgb"], a["pano_levels"], glow=glow,
                                                    frost=frost, levels=levels, crop=crop, out_u8=u8)
            for i in range(2):
                _eq(got[i], want[i], (call, "eye", i))
            off = ops.dibr_xr_eyes_panorama_curved(f, depth, dp, a["screen"], a["eyes"], None, None, None, glow=glow, frost=frost, levels=levels,
                                                   crop=crop, out_u8=u8)
            assert not torch.equal(off[0], want[0])                               # and the panorama is there
            with pytest.raises(_lib_error()):                                     # the old pipeline door refuses, before the model starts
                fused.view_pipeline_xr_panorama(f, p, dp, a["screen"], a["eyes"], a["panorama"], a["pano_rgb"], a["pano_levels"], glow=glow, frost=frost,
                                                levels=levels, crop=crop, out_u8=u8)
    finally:
        fused.close(); plain.close()


def _lib_error():
    from desktop2stereo_amd import _lib
    return _lib.D2SError


def test_a_refused_call_leaves_out_untouched_and_the_old_door_still_refuses(dev, fixtures, scenes):
    from desktop2stereo_amd import _lib, ops, xr
    c = _case(fixtures, "glow_h")
    a = _case_args(dev, c, scenes)
    _, total = ops.dibr_xr_shape(a["eyes"], 1, a["dp"].alpha_mode)
    out = torch.full((total,), -7.0, dtype=torch.float32, device=dev)                   # (no output value is negative)

    def pano(**kw):
        s = _case_args(dev, c, scenes)["panorama"]
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    outside = [xr.xr_eye(np.matmul(xr.fov_to_proj_mat4(-0.75, 0.60, 0.55, -0.60), xr.pose_to_view_mat4((0, 0, 0, 1), (3.0, 0.0, -1.0))), 130, 100, 0),
               a["eyes"][1]]
    refused = [dict(eyes=outside),                                                        # the curved glow's draw-order case
               dict(frost=xr.XrFrost.veil()),                                             # glow and frost both on
               dict(screen=xr.XrScreen(**dict(c["screen"], normal_offset=0.01))),
               dict(panorama=pano(struct_size=160)), dict(panorama=pano(exposure=float("nan"))), dict(panorama=pano(flip_y=3)),
               dict(pano_rgb=None), dict(pano_levels=None),                               # the panorama without its image or chain
               dict(levels=None),                                                         # the glow without the frames' chain
               dict(screen=xr.XrScreen(**dict(c["screen"], distance=0.2, yaw=1.2)))]      # what dibr_xr_eyes refuses
    for kw in refused:
        with pytest.raises(_lib.D2SError):
            _call(a, out=out, **kw)
    # the old door: the curved looks with a panorama, glow and walls
    with pytest.raises(_lib.D2SError, match="CURVED"):
        _call(a, out=out, fn=ops.dibr_xr_eyes_panorama)
    with pytest.raises(_lib.D2SError, match="CURVED"):
        _call(a, out=out, fn=ops.dibr_xr_eyes_panorama, glow=None, frost=xr.XrFrost.veil())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    _call(a, out=out)                                                                     # an accepted call writes every element
    assert not bool((out == -7.0).any())
    out.fill_(-7.0)
    _call(a, out=out, glow=None, frost=xr.XrFrost.frosted())                              # ... the walls' kernel too
    assert not bool((out == -7.0).any())
