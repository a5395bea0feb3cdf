"""GPU: the Viewer pipeline -- the DIBR shader warp and the composite modes reading depth at MODEL resolution (csrc/dibr_tex.h UpDep;
d2s_dibr_warp_depth, d2s_dibr_composite_depth) and frames -> in-painted views in one call (d2s_view_pipeline_streams,
ops.Engine.view_pipeline, depth.pipeline(inpaint=True | a composite display_mode)).

The fused form evaluates, per texel of the shader's depth texture, the expression upsample_depth_kernel stores (one shared helper,
no contraction), so it must equal the two-call form -- ops.upsample_depth, then the warp on the full-resolution map -- BIT FOR BIT:
every equality below is np.array_equal on float32 (F32_HWC) output, with a uint8 spot check per group.  The two-call form is pinned
to renders of the reference's own shaders (tests/golden/dibr.npz, composite.npz: test_gpu_dibr.py, test_gpu_composite.py), so the
equality carries that pin over to the fused form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = ("Full-SBS", "Half-SBS", "Full-TAB", "Half-TAB")
COMPOSITES = ("Anaglyph", "Interleaved", "Interleaved-V", "Depth Map")
ENV_KEYS = ("D2S_DIBR_NO_ROLL0", "D2S_DIBR_NO_ROWS", "D2S_DIBR_COLS")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


def _scene(dev, dh, dw, H, W, seed, batch=None):
    """uint8 frames at H x W and a hard-edged depth map at dh x dw (synth.dibr_scene "boxes": the in-painting's work), on the device."""
    from desktop2stereo_amd import synth
    n = batch or 1
    f = np.stack([synth.dibr_scene(H, W, seed + i, "boxes")[0] for i in range(n)])
    d = np.stack([synth.dibr_scene(dh, dw, seed + i, "boxes")[1] for i in range(n)])
    f, d = torch.from_numpy(f).to(dev), torch.from_numpy(d).to(dev)
    return (f, d) if batch else (f[0], d[0])


def _eq(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        pytest.fail(f"{what}: fused != two-call in {int((d > 0).sum())} of {d.size} values, max |diff| {d.max():.3e}")


def _warp_pair(f, d, dp, out_u8=False):
    from desktop2stereo_amd import ops
    H, W = f.shape[-3], f.shape[-2]
    return ops.dibr_warp(f, d, dp, out_u8=out_u8), ops.dibr_warp(f, ops.upsample_depth(d, H, W), dp, out_u8=out_u8)


# (dh, dw, H, W): the two model shapes the reference's 16:9 frames map to, an odd pair (no multiple of any tile, W past one 512- and
# one 256-column block), a DOWN-scale, and 4K (Full modes: an 8 K-wide / 4 K-tall output, the window kernel's widest span)
SIZES = [(294, 518, 1080, 1920), (196, 336, 720, 1280), (113, 201, 451, 803), (294, 518, 200, 360), (294, 518, 2160, 3840)]


@pytest.mark.parametrize("dh,dw,H,W", SIZES)
def test_fused_warp_equals_upsample_then_warp(dev, dh, dw, H, W):
    """All four display modes at every size (roll == 0: the LDS-window kernels, depth rows evaluated by the staging loop), and the
    in-painting really runs: the output differs from the one whose sweeps find nothing (search_radius 0)."""
    from desktop2stereo_amd import ops
    f, d = _scene(dev, dh, dw, H, W, 11)
    big = H >= 2160
    for mode in (("Full-TAB", "Half-SBS") if big else MODES):
        dp = ops.dibr_params(display_mode=mode, depth_ratio=2.0)
        a, b = _warp_pair(f, d, dp)
        _eq(a, b, (dh, dw, H, W, mode))
        if mode in ("Full-SBS", "Full-TAB") and not big:
            none = ops.dibr_warp(f, d, ops.dibr_params(display_mode=mode, depth_ratio=2.0, search_radius=0.0), out_u8=False)
            assert float((a - none).abs().max()) > 1.0, (H, W, mode, "the in-painting did not contribute")
        del a, b
    a, b = _warp_pair(f, d, ops.dibr_params(display_mode="Half-TAB" if big else "Full-SBS", depth_ratio=2.0), out_u8=True)
    assert a.dtype == torch.uint8
    _eq(a, b, (dh, dw, H, W, "uint8"))


@pytest.mark.parametrize("kw", [dict(roll=0.2), dict(roll=-0.05, convergence=0.02), dict(feather=True, corner_radius=0.03),
                                dict(feather=True, feather_width=0.1, corner_radius=0.2, viewport=(10.0, 5.0, 700.0, 400.0)),
                                dict(alpha="rgba"), dict(alpha="premultiplied", corner_radius=0.05),
                                dict(depth_ratio=30.0, ipd_uv=0.2), dict(resolution=(640.0, 360.0)), dict(convergence=0.4)],
                         ids=lambda kw: "-".join(kw))
def test_fused_warp_parameters(dev, kw):
    """roll != 0 (the general gather kernel: every tap evaluated on demand), feathering and rounded corners (FX kernels), rgba,
    a parallax that takes taps out of the LDS window (depth_ratio 30 at ipd 0.2: the row-tap fallback), u_resolution, convergence --
    at the odd size, all four modes, depth scaled past 0..1 for the window-leaving case."""
    from desktop2stereo_amd import ops
    f, d = _scene(dev, 113, 201, 451, 803, 21)
    if "ipd_uv" in kw:
        d = d * 4.0
    for mode in MODES:
        a, b = _warp_pair(f, d, ops.dibr_params(display_mode=mode, **kw))
        assert a.shape[-1] == (4 if kw.get("alpha") == "rgba" else 3)
        _eq(a, b, (mode, kw))
    a, b = _warp_pair(f, d, ops.dibr_params(display_mode="Full-SBS", **kw), out_u8=True)
    _eq(a, b, ("uint8", kw))


def test_fused_warp_batch_and_kernel_switches(dev, monkeypatch):
    """Batch 3 of different frames and maps, and the A/B switches forced on through d2s_debug_reload_env: D2S_DIBR_NO_ROWS (the row
    gather kernel), D2S_DIBR_NO_ROLL0 (the general kernel at roll 0), D2S_DIBR_COLS = 256 / 1024 (the window kernel's narrow form;
    1024 does not exist for the model-resolution source and falls to 512) -- each equal to the two-call form under the same switch,
    and all equal to one another."""
    from desktop2stereo_amd import ops
    f, d = _scene(dev, 98, 168, 360, 640, 31, batch=3)
    try:
        outs = {}
        for name, env in (("rows", {}), ("rows_256", {"D2S_DIBR_COLS": "256"}), ("rows_1024", {"D2S_DIBR_COLS": "1024"}),
                          ("row_gather", {"D2S_DIBR_NO_ROWS": "1"}), ("general", {"D2S_DIBR_NO_ROLL0": "1"})):
            for k in ENV_KEYS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            ops.reload_env()
            for mode in ("Full-SBS", "Half-TAB"):
                a, b = _warp_pair(f, d, ops.dibr_params(display_mode=mode, depth_ratio=3.0))
                _eq(a, b, (name, mode))
                outs[name, mode] = a
            a, b = _warp_pair(f, d, ops.dibr_params(display_mode="Half-SBS"), out_u8=True)
            _eq(a, b, (name, "uint8"))
        for (name, mode), a in outs.items():
            _eq(a, outs["general", mode], ("kernel forms", name, mode))
        assert float((outs["rows", "Full-SBS"][0] - outs["rows", "Full-SBS"][1]).abs().max()) > 1.0       # three different frames
    finally:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        ops.reload_env()


@pytest.mark.parametrize("mode", COMPOSITES)
def test_fused_composites_equal_upsample_then_composite(dev, mode, monkeypatch):
    """The four composite programs: the frame itself, a viewport LARGER than the frame with an odd (x, y) origin (which eye a row /
    column shows), a smaller one, roll (the gather kernel), feather + corners, rgba, a window-leaving parallax, batch 3, 1080p."""
    from desktop2stereo_amd import ops

    def pair(f, d, dp, H, W, out_u8=False):
        fr = None if mode == "Depth Map" else f
        return (ops.dibr_composite(fr, d, dp, mode, out_u8=out_u8, size=(H, W)),
                ops.dibr_composite(fr, ops.upsample_depth(d, H, W), dp, mode, out_u8=out_u8))

    f, d = _scene(dev, 113, 201, 451, 803, 41)
    cases = [dict(), dict(viewport=(3, 1, 1607, 903)), dict(viewport=(1, 3, 333, 187)), dict(roll=0.15), dict(roll=-0.1, viewport=(5, 0, 900, 500)),
             dict(feather=True, feather_width=0.1, corner_radius=0.1, viewport=(3, 2, 640, 360)), dict(alpha="rgba"),
             dict(depth_ratio=30.0, ipd_uv=0.2)]
    for kw in cases:
        dd = d * 4.0 if "ipd_uv" in kw else d
        kw = dict(kw)
        kw.setdefault("depth_ratio", 4.0)
        a, b = pair(f, dd, ops.dibr_params(**kw), 451, 803)
        if "viewport" in kw:
            assert tuple(a.shape[:2]) == (kw["viewport"][3], kw["viewport"][2])
        _eq(a, b, (mode, kw))
    a, b = pair(f, d, ops.dibr_params(depth_ratio=4.0, viewport=(3, 1, 1607, 903)), 451, 803, out_u8=True)
    _eq(a, b, (mode, "uint8"))
    f3, d3 = _scene(dev, 98, 168, 360, 640, 43, batch=3)
    a, b = pair(f3, d3, ops.dibr_params(depth_ratio=4.0), 360, 640)
    assert a.shape[0] == 3
    _eq(a, b, (mode, "batch 3"))
    fh, dh_ = _scene(dev, 294, 518, 1080, 1920, 45)
    a, b = pair(fh, dh_, ops.dibr_params(depth_ratio=2.0), 1080, 1920)
    _eq(a, b, (mode, "1080p"))
    if mode != "Depth Map":
        none = ops.dibr_composite(fh, dh_, ops.dibr_params(depth_ratio=2.0, search_radius=0.0), mode, out_u8=False)
        assert float((a - none).abs().max()) > 1.0, (mode, "the in-painting did not contribute")
        try:                                            # the gather kernels at roll 0 too (a window too wide for LDS takes them)
            monkeypatch.setenv("D2S_DIBR_NO_ROWS", "1")
            ops.reload_env()
            a2, b2 = _warp_pair(f, d, ops.dibr_params())
            _eq(a2, b2, "f1 under NO_ROWS")
        finally:
            monkeypatch.delenv("D2S_DIBR_NO_ROWS", raising=False)
            ops.reload_env()


def test_depth_of_the_frames_size_is_the_existing_call(dev):
    """dh == H && dw == W: the texture itself (the FullDep kernels) -- d2s_dibr_warp_depth is then d2s_dibr_warp."""
    import ctypes as C
    from desktop2stereo_amd import _lib, ops
    f, d = _scene(dev, 180, 320, 180, 320, 51, batch=2)
    dp = ops.dibr_params(display_mode="Full-SBS", depth_ratio=3.0)
    got = ops.dibr_warp(f, d, dp, out_u8=False)
    want = torch.empty_like(got)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().d2s_dibr_warp(C.c_void_p(f.data_ptr()), C.c_void_p(d.data_ptr()), 2, 180, 320, C.byref(dp),
                                         C.c_void_p(want.data_ptr()), _lib.FMT_F32_HWC, st), "d2s_dibr_warp")
    _eq(got, want, "same size")


@pytest.mark.parametrize("name,prec,H,W,res,batch", [("tiny", "fp32", 270, 480, 140, 2), ("vits", "bf16", 1080, 1920, 518, 1)])
@pytest.mark.parametrize("use_ema", [False, True])
def test_view_pipeline_equals_pipeline_then_warp(dev, name, prec, H, W, res, batch, use_ema):
    """view_pipeline(frames) == dibr_warp(frames, depth_full of Engine.pipeline(want_depth=True)) on an identically built engine, over
    three calls (the EMA state advances in both), its own depth_full == that map; one composite and the uint8 output as well."""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS, PipelineParams, engine_shape
    from desktop2stereo_amd.weights import make_weights
    cfg = MODELS[name]
    h, w, _ = engine_shape(H, W, res)
    p = PipelineParams(depth_resolution=res)
    wts = make_weights(cfg, 0)
    fused, plain = (ops.Engine(cfg, wts, h, w, batch, prec) for _ in range(2))
    sp = ops.sbs_params(p.ipd, p.depth_strength, p.convergence, "Half-SBS", False)
    dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, "Full-SBS")
    try:
        for call in range(3):
            f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 60 + 7 * call + b, "boxes")[0] for b in range(batch)])).to(dev)
            view = (None, "Anaglyph", None)[call]
            u8 = call == 2
            got, got_depth = fused.view_pipeline(f, p, dp, view=view, use_ema=use_ema, out_u8=u8, want_depth=True)
            _, depth = plain.pipeline(f, p, sp, use_ema=use_ema, want_depth=True)
            assert depth.shape == (batch, H, W) and float(depth.max() - depth.min()) > 0.05
            _eq(got_depth, depth, (name, call, "depth_full"))
            want = ops.dibr_composite(f, depth, dp, view, out_u8=u8) if view else ops.dibr_warp(f, depth, dp, out_u8=u8)
            _eq(got, want, (name, call, view, "uint8" if u8 else "f32"))
            if call == 0 and not use_ema:                    # (no state to advance) without depth_full: the same output
                _eq(fused.view_pipeline(f, p, dp, out_u8=False), want, (name, "without depth_full"))
    finally:
        fused.close(); plain.close()


def test_view_pipeline_refuses_like_its_parts(dev):
    from desktop2stereo_amd import _lib, ops, synth
    from desktop2stereo_amd.config import MODELS, PipelineParams, engine_shape
    from desktop2stereo_amd.weights import make_weights
    cfg = MODELS["tiny"]
    h, w, _ = engine_shape(270, 480, 140)
    p = PipelineParams(depth_resolution=140)
    eng = ops.Engine(cfg, make_weights(cfg, 0), h, w, 1, "fp32")
    f = torch.from_numpy(synth.structured_frame(270, 480, 1)[None]).to(dev)
    dp = ops.dibr_params()
    try:
        with pytest.raises(_lib.D2SError):
            eng.view_pipeline(torch.zeros((1, 300, 300, 3), dtype=torch.uint8, device=dev), p, dp)      # another model-input shape
        with pytest.raises(_lib.D2SError):
            eng.view_pipeline(f.repeat(2, 1, 1, 1), p, dp)                                               # batch > max_batch
        with pytest.raises(_lib.D2SError):
            eng.view_pipeline(f, p, dp, streams=[0])                                                     # not a temporal engine
        with pytest.raises(_lib.D2SError):
            eng.view_pipeline(f, p, ops.dibr_params(viewport=(0.5, 0, 10, 10)), view="Interleaved")
        with pytest.raises(ValueError):
            eng.view_pipeline(f, p, dp, view="Full-SBS")
        bad = ops.dibr_params()
        bad.struct_size = 72
        with pytest.raises(_lib.D2SError):
            eng.view_pipeline(f, p, bad)
        out = eng.view_pipeline(f, p, dp)                                                                # and it still works afterwards
        assert out.shape == (1, 270, 960, 3) and out.dtype == torch.uint8
    finally:
        eng.close()


def test_view_pipeline_vda_streams(dev):
    """A Video-Depth-Anything engine with three stream slots, fed streams [2, 0], then [1, 2], then [0] with per-stream EMA: every
    row equals pipeline(want_depth) + dibr_warp for that stream on a second engine given the same calls, and equals an engine that
    only ever saw that one stream -- a stream not named in a call is left exactly as it was."""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS, PipelineParams, engine_shape
    from desktop2stereo_amd.vda_weights import make_vda_weights
    cfg = MODELS["tiny"]
    H, W, res = 90, 160, 84
    h, w, _ = engine_shape(H, W, res)
    p = PipelineParams(depth_resolution=res)
    wts = make_vda_weights(cfg, 0)
    mk = lambda: ops.Engine(cfg, wts, h, w, 3, "fp32", temporal=True)
    fused, plain, solo = mk(), mk(), {k: mk() for k in range(3)}
    sp = ops.sbs_params(p.ipd, p.depth_strength, p.convergence, "Half-SBS", False)
    dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, "Full-TAB")
    frame = lambda k, i: torch.from_numpy(synth.dibr_scene(H, W, 100 * (k + 1) + i, "boxes")[0]).to(dev)
    seen = {0: 0, 1: 0, 2: 0}
    try:
        for ids in ([2, 0], [1, 2], [0], [0, 1, 2]):
            f = torch.stack([frame(k, seen[k]) for k in ids])
            got = fused.view_pipeline(f, p, dp, use_ema=True, out_u8=False, streams=ids)
            _, depth = plain.pipeline(f, p, sp, use_ema=True, want_depth=True, streams=ids)
            _eq(got, ops.dibr_warp(f, depth, dp, out_u8=False), ("streams", ids))
            for r, k in enumerate(ids):
                alone = solo[k].view_pipeline(f[r:r + 1], p, dp, use_ema=True, out_u8=False, streams=[k])
                _eq(got[r:r + 1], alone, ("stream", k, "call", ids))
                seen[k] += 1
        assert float((got[0] - got[1]).abs().max()) > 1.0
    finally:
        for e in [fused, plain, *solo.values()]:
            e.close()


def test_view_pipeline_vs_oracle(dev):
    """One end-to-end frame against the CPU restatement of the reference's shader (oracle.dibr_oracle.dibr_sbs) run on the call's OWN
    depth_full -- which isolates the warp from model precision -- with the gates of tests/test_gpu_dibr.py::_check: >= 99.9 % of the
    values within 0.02 of a level, mean <= 2e-3."""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS, PipelineParams, engine_shape
    from desktop2stereo_amd.weights import make_weights
    from oracle import dibr_oracle as R
    cfg = MODELS["tiny"]
    H, W, res = 180, 320, 140
    h, w, _ = engine_shape(H, W, res)
    p = PipelineParams(depth_resolution=res)
    eng = ops.Engine(cfg, make_weights(cfg, 0), h, w, 1, "fp32")
    img = synth.dibr_scene(H, W, 71, "boxes")[0]
    try:
        for mode, ratio in (("Full-SBS", 4.0), ("Half-TAB", 2.0)):
            dp = ops.dibr_params(p.ipd, ratio, p.convergence, mode)
            got, depth = eng.view_pipeline(torch.from_numpy(img[None]).to(dev), p, dp, out_u8=False, want_depth=True)
            want = R.dibr_sbs(img, depth[0].cpu().numpy(), p.ipd, ratio, p.convergence, mode)
            d = np.abs(got[0].cpu().numpy() - want)
            print(f"[view_pipeline vs oracle, {mode}] > 0.02: {(d > 0.02).mean():.2e}, mean {d.mean():.2e}, max {d.max():.3f}")
            assert got[0].shape == want.shape
            assert (d <= 0.02).mean() >= 0.999 and d.mean() <= 2e-3, (mode, float((d > 0.02).mean()), float(d.mean()), float(d.max()))
    finally:
        eng.close()


def test_depth_pipeline_surface(dev):
    """depth.pipeline(inpaint=True) / (display_mode = a composite): shapes, dtypes, equal to the ops results; the default call is
    byte-equal to Engine.pipeline; a present-ring slot as `out`."""
    from desktop2stereo_amd import _lib, depth as D, ops, synth
    from desktop2stereo_amd.config import PipelineParams
    from desktop2stereo_amd.present import PresentRing
    saved = dict(D._state)
    p = PipelineParams(depth_resolution=140)
    try:
        D._state["engine"] = None
        D.configure("tiny", params=p, precision="fp32", max_batch=2)
        frames = np.stack([synth.dibr_scene(270, 480, 80 + s, "boxes")[0] for s in range(2)])
        t = torch.from_numpy(frames).to(dev)
        out = D.pipeline(frames, display_mode="Full-SBS", inpaint=True)
        eng = D._state["engine"]
        sp = ops.sbs_params(p.ipd, p.depth_strength, p.convergence, p.display_mode, p.fill_16_9)
        plain, depth = eng.pipeline(t, p, sp, want_depth=True)
        assert out.shape == (2, 270, 960, 3) and out.dtype == torch.uint8
        _eq(out, ops.dibr_warp(t, depth, ops.dibr_params(p.ipd, p.depth_strength, p.convergence, "Full-SBS")), "inpaint=True")
        ana = D.pipeline(frames, display_mode="Anaglyph")
        assert ana.shape == (2, 270, 480, 3) and ana.dtype == torch.uint8
        dpc = ops.dibr_params(p.ipd, p.depth_strength, p.convergence)
        _eq(ana, ops.dibr_composite(t, depth, dpc, "Anaglyph"), "Anaglyph")
        il, d2 = D.pipeline(frames, display_mode="Interleaved", viewport=(1, 1, 960, 540), out_u8=False, want_depth=True)
        assert il.shape == (2, 540, 960, 3) and il.dtype == torch.float32
        _eq(d2, depth, "want_depth")
        _eq(il, ops.dibr_composite(t, depth, ops.dibr_params(p.ipd, p.depth_strength, p.convergence, viewport=(1, 1, 960, 540)), "Interleaved",
                                   out_u8=False), "Interleaved viewport")
        dm = D.pipeline(frames, display_mode="Depth Map")
        _eq(dm, ops.dibr_composite(None, depth, dpc, "Depth Map"), "Depth Map")
        _eq(D.pipeline(frames), plain, "default call")                          # unchanged: Engine.pipeline, byte for byte
        with pytest.raises(ValueError):
            D.pipeline(frames, viewport=(0, 0, 10, 10))
        # update_frame fed from view_pipeline through the present ring: the slot is the call's `out`
        ring = PresentRing((2, 270, 960, 3), torch.uint8, slots=3)
        slot, buf = ring.acquire()
        eng.view_pipeline(t, p, ops.dibr_params(p.ipd, p.depth_strength, p.convergence, "Full-SBS"), out=buf)
        ring.publish(slot)
        s2, shown, _ = ring.consume(host_wait=True)
        assert s2 == slot
        _eq(shown, out, "present slot")
        ring.release(s2)
        ring.close()
        assert _lib.load().d2s_version() >= 113
    finally:
        if D._state.get("engine") is not None:
            D._state["engine"].close()
        D._state.clear()
        D._state.update(saved)
