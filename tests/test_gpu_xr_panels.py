"""GPU: the world-space panels drawn in place over finished eye images (d2s_dibr_xr_panels, ops.dibr_xr_panels,
depth.xr_eye_views*(panels=); reference xr_viewer/overlay.py:81-249, 1427-1510, xr_viewer/effects.py:1157-1225).

PINNED by tests/golden/xr_panels.npz -- the reference's screen, then its panels, drawn per eye on SwiftShader with its own shaders and
its own recorded _render_fps_overlay / _render_keyboard state (make_golden_xr_panels.py) -- through the restatement
tests/xr_panels_ref.py, which tests/test_xr_panels_oracle.py holds to those renders.
  * Every case of the manifest goes through ops.dibr_xr_panels over the library's OWN dibr_xr_eyes image, and is held to the float64
    restatement over that same image on the pixels whose class (screen coverage + the set of panels that pass) is uniform on 3 x 3 and
    that have no depth near-tie.  The bound is measured, not chosen: the manifest records, per case and eye, the maximum difference
    of a float32 emulation of the kernel's arithmetic from float64; the kernel is allowed TWICE that, for rgb and for alpha (exact
    where the emulation's is).  Quantised, no value is more than 1 level from the restatement's.
  * Everything else is an exact rule: pixels outside every panel's box are bit-identical to the input; no panels is the input and a
    plan of 0 launches; uint8 is within 1 level of the rounded float32; a batch is its frames; over a frosted and over a panorama eye
    image nothing outside the boxes changes and the inside is the restatement over that image; depth.xr_eye_views(panels=) is the two
    calls; a refused call leaves `out` untouched."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = ["front", "behind", "status", "status_faded_oblique", "solid_alpha", "keyboard", "two_writers", "two_no_write", "opaque", "curved",
         "half_off_behind_eye", "wrap_edge"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def meta(golden_dir):
    with open(os.path.join(golden_dir, "xr_panels.json")) as f:
        return json.load(f)


def _case(meta, name):
    return next(c for c in meta["cases"] if c["name"] == name)


def _lib_facets(c):
    """The screen as the LIBRARY forms it, in double precision from the screen's numbers (the manifest's model is the reference's
    float32): its depth decides the panels' depth test."""
    import xr_eye_ref as X
    from desktop2stereo_amd import xr
    s = xr.XrScreen(**c["screen"])
    return X.facets_flat(s.model_mat4()) if s.curve == "flat" else X.facets_strip(s.curved_verts(), s.curve == "vertical")


def _args(dev, meta, c, alpha="rgba", batch=1):
    import xr_eye_ref as X
    import xr_panels_ref as P
    from desktop2stereo_amd import ops, synth, xr
    img, _, dep = X.case_scene(c, meta)
    if batch > 1:
        more = [synth.dibr_scene(img.shape[0], img.shape[1], c["seed"] + 100 * b, "boxes") for b in range(1, batch)]
        img, dep = np.stack([img] + [m[0] for m in more]), np.stack([dep] + [m[1] for m in more])
    dp = ops.dibr_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], corner_radius=c["corner_radius"], alpha=alpha)
    screen = xr.XrScreen(clear=tuple(c["clear"]), **c["screen"])
    eyes = [xr.xr_eye(np.array(e["vp"]), e["size"][0], e["size"][1], e["eye"]) for e in c["eyes"]]
    panels = [xr.XrPanel(np.array(q["model"]), q["texture"], tuple(q["color"]), q["alpha"], q["depth_test"], q["depth_write"], q["blend"])
              for q in c["panels"]]
    pics = P.case_textures(c)
    return dict(f=torch.from_numpy(img).to(dev), d=torch.from_numpy(dep).to(dev), dp=dp, screen=screen, eyes=eyes, panels=panels,
                texs=[torch.from_numpy(p).to(dev) for p in pics], pics=pics, ref_panels=P.case_panels(c), crop=c["crop"])


def _outside(c, e):
    import xr_panels_ref as P
    w, h = e["size"]
    out = np.ones((h, w), bool)
    for q in c["panels"]:
        b = P.pixel_box(q["model"], np.array(e["vp"]), w, h)
        if b:
            out[b[1]:b[3], b[0]:b[2]] = False
    return out


def _held(c, e, before, after, bound_scale=2.0, what=""):
    """before, after: one eye's float32 image [h,w,4] (rgb levels, alpha 0..1) as numpy.  The restatement over `before` against `after`
    on the compared pixels -> failures."""
    import xr_panels_ref as P
    w, h = e["size"]
    want, info = P.render(before.astype(np.float64), _lib_facets(c), np.array(e["vp"]), w, h, P.case_panels(c), P.case_textures(c), "repeat")
    ok = P.compared(info)
    assert 1.0 - ok.mean() <= 0.15
    drawn = ok & info["passed"].any(0)
    assert int(drawn.sum()) >= c["min_panel"] // 2
    d = np.abs(after[..., :3].astype(np.float64) - want[..., :3])[ok]
    da = np.abs(after[..., 3].astype(np.float64) - want[..., 3])[ok]
    print(f"\n[panels vs float64 restatement{what}, {c['name']} eye {e['eye']}] max |rgb| {d.max():.6f} level (allowed {bound_scale * e['f32'][0]:.6f}) "
          f"alpha max {da.max():.2e} (allowed {bound_scale * e['f32'][1]:.2e}); {int(drawn.sum())} panel pixels of {int(ok.sum())} compared")
    fails = []
    if not d.max() <= bound_scale * e["f32"][0]:
        fails.append((c["name"], e["eye"], "rgb", float(d.max()), bound_scale * e["f32"][0]))
    if not da.max() <= bound_scale * e["f32"][1]:
        fails.append((c["name"], e["eye"], "alpha", float(da.max()), bound_scale * e["f32"][1]))
    out = _outside(c, e)
    if not np.array_equal(after[out], before[out]):
        fails.append((c["name"], e["eye"], "changed outside every box"))
    if np.array_equal(after[drawn], before[drawn]):
        fails.append((c["name"], e["eye"], "nothing drawn"))
    return fails, want, ok


@pytest.mark.parametrize("name", CASES)
def test_panels_match_the_float64_restatement(dev, meta, name):
    from desktop2stereo_amd import ops
    c = _case(meta, name)
    a = _args(dev, meta, c)
    imgs = ops.dibr_xr_eyes(a["f"], a["d"], a["dp"], a["screen"], a["eyes"], crop=a["crop"], out_u8=False)
    before = [t[0].cpu().numpy() for t in imgs]
    got = ops.dibr_xr_panels(imgs, a["screen"], a["eyes"], a["panels"], a["texs"])
    assert all(g is t for g, t in zip(got, imgs))                       # the same tensors, drawn in place
    imgs8 = ops.dibr_xr_eyes(a["f"], a["d"], a["dp"], a["screen"], a["eyes"], crop=a["crop"], out_u8=True)
    before8 = [t[0].cpu().numpy() for t in imgs8]
    ops.dibr_xr_panels(imgs8, a["screen"], a["eyes"], a["panels"], a["texs"])
    fails = []
    for e, b, g, b8, g8 in zip(c["eyes"], before, got, before8, imgs8):
        g, g8 = g[0].cpu().numpy(), g8[0].cpu().numpy()
        assert np.isfinite(g).all() and g8.dtype == np.uint8
        f, want, ok = _held(c, e, b, g)
        fails += f
        lv = lambda x: np.concatenate([x[..., :3], x[..., 3:] * 255.0], -1)
        q = np.abs(g8.astype(np.float64) - np.rint(np.clip(lv(want), 0, 255)))[ok]      # (the uint8 images differ from the float32 ones by rounding only)
        q32 = np.abs(g8.astype(np.float64) - np.rint(np.clip(lv(g.astype(np.float64)), 0, 255)))
        print(f"    uint8 vs rounded restatement max {q.max():.0f}, vs rounded float32 path max {q32.max():.0f}")
        if not q.max() <= 1 or not q32.max() <= 1:
            fails.append((name, e["eye"], "uint8", float(q.max()), float(q32.max())))
        out = _outside(c, e)
        if not np.array_equal(g8[out], b8[out]):
            fails.append((name, e["eye"], "uint8 changed outside every box"))
    assert not fails, fails


def test_no_panels_is_the_input_and_no_launch(dev, meta):
    from desktop2stereo_amd import ops, xr
    c = _case(meta, "front")
    a = _args(dev, meta, c)
    imgs = ops.dibr_xr_eyes(a["f"], a["d"], a["dp"], a["screen"], a["eyes"], crop=a["crop"], out_u8=False)
    before = [t.clone() for t in imgs]
    ops.dibr_xr_panels(imgs, a["screen"], a["eyes"], [], [])
    behind = xr.XrPanel(np.array(_case(meta, "half_off_behind_eye")["panels"][1]["model"]))
    ops.dibr_xr_panels(imgs, a["screen"], a["eyes"], [behind], a["texs"])
    assert all(torch.equal(x, y) for x, y in zip(imgs, before))
    for panels in ([], [behind]):
        plan = ops.dibr_xr_panels_plan(1, a["screen"], a["eyes"], panels, [])
        assert (plan["setup_launches"], plan["render_launches"], plan["drawn"], plan["grid"]) == (0, 0, [0, 0], (0, 0, 0))


def test_a_batch_is_its_frames_and_three_channels_are_the_rgb(dev, meta):
    from desktop2stereo_amd import ops
    c = _case(meta, "status_faded_oblique")                             # eyes of two sizes, neither a multiple of 16
    a = _args(dev, meta, c, batch=3)
    both = ops.dibr_xr_eyes(a["f"], a["d"], a["dp"], a["screen"], a["eyes"], crop=a["crop"], out_u8=False)
    ops.dibr_xr_panels(both, a["screen"], a["eyes"], a["panels"], a["texs"])
    for b in range(3):
        one = ops.dibr_xr_eyes(a["f"][b:b + 1], a["d"][b:b + 1], a["dp"], a["screen"], a["eyes"], crop=a["crop"], out_u8=False)
        ops.dibr_xr_panels(one, a["screen"], a["eyes"], a["panels"], a["texs"])
        for i in range(2):
            assert torch.equal(both[i][b], one[i][0]), (b, i)
    # alpha_mode "window": three channels, the same rgb blend
    a3 = _args(dev, meta, c, alpha="window")
    rgb = ops.dibr_xr_eyes(a3["f"], a3["d"], a3["dp"], a3["screen"], a3["eyes"], crop=a3["crop"], out_u8=False)
    before = [t.clone() for t in rgb]
    ops.dibr_xr_panels(rgb, a3["screen"], a3["eyes"], a3["panels"], a3["texs"])
    import xr_panels_ref as P
    for e, b4, g in zip(c["eyes"], before, rgb):
        assert g.shape[-1] == 3
        w, h = e["size"]
        dst = np.concatenate([b4[0].cpu().numpy().astype(np.float64), np.ones((h, w, 1))], -1)
        want, info = P.render(dst, _lib_facets(c), np.array(e["vp"]), w, h, a3["ref_panels"], a3["pics"], "repeat")
        ok = P.compared(info)
        assert np.abs(g[0].cpu().numpy().astype(np.float64) - want[..., :3])[ok].max() <= 2.0 * e["f32"][0]
        assert not torch.equal(g, b4)


def test_over_a_frosted_and_over_a_panorama_eye_image(dev, meta):
    """The pass reads only the finished image and the screen's geometry: whichever entry wrote the image."""
    from desktop2stereo_amd import ops, xr
    c = _case(meta, "two_writers")
    a = _args(dev, meta, c)
    frosted = ops.dibr_xr_eyes_frost(a["f"], a["d"], a["dp"], a["screen"], a["eyes"], xr.XrFrost.frosted(time=0.5), ops.mip_chain(a["f"]),
                                    crop=a["crop"], out_u8=False)
    rng = np.random.default_rng(5)
    pano = torch.from_numpy(rng.integers(0, 256, (64, 128, 3), dtype=np.uint8)).to(dev)
    ps = xr.XrPanorama(exposure=0.9).c_struct([(np.array(e["proj"]), np.array(e["view"])) for e in c["eyes"]], (64, 128))
    behind = ops.dibr_xr_eyes_panorama(a["f"], a["d"], a["dp"], a["screen"], a["eyes"], ps, pano, ops.mip_chain(pano).view(-1), crop=a["crop"],
                                       out_u8=False)
    plain = ops.dibr_xr_eyes(a["f"], a["d"], a["dp"], a["screen"], a["eyes"], crop=a["crop"], out_u8=False)
    fails = []
    for what, imgs in (("frosted", frosted), ("panorama", behind)):
        assert not torch.equal(imgs[0], plain[0])                       # (the look is there)
        before = [t[0].cpu().numpy() for t in imgs]
        ops.dibr_xr_panels(imgs, a["screen"], a["eyes"], a["panels"], a["texs"])
        for e, b, g in zip(c["eyes"], before, imgs):
            fails += _held(c, e, b, g[0].cpu().numpy(), what=" over a " + what + " image")[0]
    assert not fails, fails


def test_depth_xr_eye_views_with_panels_is_the_two_calls(dev, meta):
    from desktop2stereo_amd import depth as D, ops, synth, xr
    from desktop2stereo_amd.config import PipelineParams
    c = _case(meta, "keyboard")
    a = _args(dev, meta, c)
    p = PipelineParams(depth_resolution=140)
    D.configure("tiny", params=p, precision="fp32", max_batch=2)
    frames = np.stack([synth.dibr_scene(270, 480, 95 + b, "boxes")[0] for b in range(2)])
    try:
        want = D.xr_eye_views(frames, a["screen"], a["eyes"])
        plain = [t.clone() for t in want]
        ops.dibr_xr_panels(want, a["screen"], a["eyes"], a["panels"], a["texs"])
        got = D.xr_eye_views(frames, a["screen"], a["eyes"], panels=a["panels"], panel_textures=a["texs"])
        none = D.xr_eye_views(frames, a["screen"], a["eyes"], panels=None)
        veil = D.xr_eye_views_frost(frames, a["screen"], a["eyes"], frost="veil", panels=a["panels"], panel_textures=a["texs"])
        veil_want = D.xr_eye_views_frost(frames, a["screen"], a["eyes"], frost="veil")
        ops.dibr_xr_panels(veil_want, a["screen"], a["eyes"], a["panels"], a["texs"])
        for i in range(2):
            assert got[i].dtype == torch.uint8 and torch.equal(got[i], want[i]) and torch.equal(none[i], plain[i]) and not torch.equal(got[i], plain[i])
            assert torch.equal(veil[i], veil_want[i])
    finally:                                                # (the module's engine is this test's: leave none behind)
        if D._state["engine"] is not None:
            D._state["engine"].close()
        D._state["engine"], D._state["engine_key"] = None, None


def test_a_refused_call_leaves_out_untouched(dev, meta):
    from desktop2stereo_amd import _lib, ops, xr
    c = _case(meta, "front")
    a = _args(dev, meta, c)
    offs, total = ops.dibr_xr_shape(a["eyes"], 1, a["dp"].alpha_mode)
    flat = torch.full((total,), -7.0, dtype=torch.float32, device=dev)
    imgs = ops._xr_views(flat, xr.eye_array(a["eyes"]), 1, 4, offs)
    good = a["panels"][0]
    crossing = np.eye(4)
    crossing[:3, :3] = [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]      # the quad spans z = -1 .. 1 through the eyes' plane
    not_affine = np.array(good.model).copy()
    not_affine[3, 0] = 0.1
    bad_size = good.c_struct()
    bad_size.struct_size = 152
    refused = [
        dict(panels=[xr.XrPanel(crossing)]), dict(panels=[xr.XrPanel(not_affine)]), dict(panels=[bad_size]),
        dict(panels=[xr.XrPanel(good.model, texture=3)]), dict(panels=[xr.XrPanel(good.model, alpha=float("nan"))]),
        dict(panels=[good] * 33),
        dict(screen=xr.XrScreen(width=1.6, height=0.96, distance=0.2, yaw=1.2, curve="horizontal")),      # the screen crosses the eye plane
        dict(workspace=torch.empty(2 * 48 * 96, dtype=torch.uint8, device=dev)),                           # d2s_dibr_xr_workspace's bytes: too few
    ]
    for kw in refused:
        k = dict(dict(screen=a["screen"], panels=a["panels"], alpha_mode=None, workspace=None), **kw)
        with pytest.raises(_lib.D2SError):
            ops.dibr_xr_panels(imgs, k["screen"], a["eyes"], k["panels"], a["texs"], alpha_mode=k["alpha_mode"], workspace=k["workspace"])
    with pytest.raises(ValueError):                         # not the tensors an eye-view call returned
        ops.dibr_xr_panels([imgs[1], imgs[0]], a["screen"], a["eyes"], a["panels"], a["texs"])
    with pytest.raises(ValueError):
        ops.dibr_xr_panels(imgs, a["screen"], a["eyes"], a["panels"], [a["texs"][0][..., :3]])
    torch.cuda.synchronize()
    assert bool((flat == -7.0).all())
    ops.dibr_xr_panels(imgs, a["screen"], a["eyes"], a["panels"], a["texs"])      # and an accepted one draws
    assert not bool((flat == -7.0).all())
    # premultiplied eye images (three channels, rgb already times alpha) are refused in the call's words, and stay as they are
    pm = _args(dev, meta, c, alpha="premultiplied")
    pre = ops.dibr_xr_eyes(pm["f"], pm["d"], pm["dp"], pm["screen"], pm["eyes"], crop=pm["crop"], out_u8=False)
    kept = [t.clone() for t in pre]
    with pytest.raises(_lib.D2SError, match="PREMULTIPLIED"):
        ops.dibr_xr_panels(pre, pm["screen"], pm["eyes"], pm["panels"], pm["texs"], alpha_mode=_lib.DIBR_ALPHA["premultiplied"])
    assert all(torch.equal(x, y) for x, y in zip(pre, kept))
