"""GPU: the viewer's composite display modes (csrc/dibr_composite.hip; reference viewer.py:633-1197).

test_kernel_matches_reference_renders holds the HIP kernels to renders of the REFERENCE's own programs (tests/golden/composite.npz,
make_golden_composite.py) with the tolerances the CPU restatement meets against them (tests/test_composite_oracle.py); the other
tests compare the kernels with the restatement (tests/composite_ref.py) on inputs the fixtures do not cover.  Against the
restatement (same float32 filtering on both sides): >= 99.9 % of the values within 0.02 of a level, mean <= 2e-3, as for f1."""
import json
import os

import numpy as np
import pytest

from composite_ref import composite, composite_frag

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = ["Anaglyph", "Interleaved", "Interleaved-V", "Depth Map"]
HD_MEAN = {"Anaglyph": 0.08, "Interleaved": 0.06, "Interleaved-V": 0.06, "Depth Map": 0.06}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


def _check(got, want, what):
    d = np.abs(got.astype(np.float32) - want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (d <= 0.02).mean() >= 0.999 and d.mean() <= 2e-3, (what, float((d > 0.02).mean()), float(d.mean()), float(d.max()))


def _run(dev, img, dep, mode, out_u8=False, alpha="window", **kw):
    from desktop2stereo_amd import ops
    dp = ops.dibr_params(kw.pop("ipd_uv", 0.064), kw.pop("depth_ratio", 4.0), kw.pop("convergence", 0.0), alpha=alpha, **kw)
    f = torch.from_numpy(np.ascontiguousarray(img)).to(dev) if img is not None else None
    return ops.dibr_composite(f, torch.from_numpy(np.ascontiguousarray(dep)).to(dev), dp, mode, out_u8=out_u8).cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
def test_kernel_matches_reference_renders(dev, golden_dir, mode):
    from desktop2stereo_amd import synth
    z = np.load(os.path.join(golden_dir, "composite.npz"))
    meta = json.load(open(os.path.join(golden_dir, "composite.json")))
    n = 0
    for c in meta["cases"]:
        if c["mode"] != mode or c.get("as_shipped"):
            continue
        n += 1
        img, dep = synth.dibr_scene(c["h"], c["w"], c["seed"], c["scene"])
        kw = dict(ipd_uv=c.get("ipd_uv", 0.064), depth_ratio=c.get("depth_ratio", 1.0), convergence=c.get("convergence", 0.0),
                  roll=c.get("roll", 0.0), feather=c.get("feather", False), feather_width=c.get("feather_width", 0.02),
                  corner_radius=c.get("corner_radius", 0.0), viewport=tuple(c["viewport"]))
        rs = c["row_stride"]
        got = _run(dev, img, dep, mode, alpha="rgba", **kw)[::rs]
        rgb = z[c["name"] + "_rgb"].astype(np.float32) / 256.0
        a = z[c["name"] + "_a"].astype(np.float32) / 65535.0
        d = np.abs(got[..., :3] - rgb)
        assert np.abs(got[..., 3] - a).max() <= 1e-3, c["name"]
        if c["w"] <= 320:
            assert d.max() <= 1.0, (c["name"], float(d.max()))
        else:
            assert (d <= 1.0).mean() >= 0.999 and d.mean() <= HD_MEAN[mode], (c["name"], float((d > 1).mean()), float(d.mean()))
        u8 = _run(dev, img, dep, mode, out_u8=True, **kw)[::rs]
        lsb = np.abs(u8.astype(int) - np.clip(np.rint(rgb), 0, 255).astype(int))
        assert (lsb <= 1).mean() >= 0.999, (c["name"], float((lsb > 1).mean()))
    assert n >= 3


@pytest.mark.parametrize("mode", MODES)
def test_kernel_vs_restatement_sweeps(dev, mode):
    """batch 3 of different frames, W not a multiple of 4, tiny frames, parallax beyond any staging window, roll (the gather
    kernel), viewports larger / smaller than the source with odd offsets, every alpha mode, f32 and u8."""
    from desktop2stereo_amd import synth
    rgb = None if mode == "Depth Map" else 0
    frames = [synth.dibr_scene(97, 203, s, "boxes") for s in (1, 2, 3)]
    imgs, deps = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    got = _run(dev, imgs if rgb is not None else None, deps, mode)
    assert got.shape == (3, 97, 203, 3)
    for b in range(3):
        _check(got[b], composite(imgs[b], deps[b], mode, depth_ratio=4.0), (mode, "batch", b))
    assert np.abs(got[0] - got[1]).max() > 1
    img, dep = frames[0]
    cases = [dict(), dict(depth_ratio=40.0), dict(roll=0.25), dict(convergence=0.4, depth_ratio=2.0),
             dict(viewport=(1, 3, 406, 194)), dict(viewport=(2, 1, 61, 37)), dict(viewport=(5, 0, 203, 97), roll=-0.1),
             dict(feather=True, feather_width=0.1, corner_radius=0.1, viewport=(3, 2, 150, 80))]
    for kw in cases:
        for alpha in ("window", "premultiplied", "rgba"):
            g = _run(dev, img if rgb is not None else None, dep, mode, alpha=alpha, **dict(kw))
            rk = dict(kw)
            rk.setdefault("depth_ratio", 4.0)
            want = composite(img, dep, mode, alpha=alpha, **rk)
            if alpha == "rgba":
                assert g.shape[-1] == 4
                _check(g[..., :3], want[..., :3], (mode, kw, alpha))
                assert np.abs(g[..., 3] - want[..., 3]).max() <= 1e-4
            else:
                _check(g, want, (mode, kw, alpha))
        u8 = _run(dev, img if rgb is not None else None, dep, mode, out_u8=True, **dict(kw))
        lsb = np.abs(u8.astype(int) - np.clip(np.rint(composite(img, dep, mode, **dict(kw, depth_ratio=kw.get("depth_ratio", 4.0)))), 0, 255).astype(int))
        assert u8.dtype == np.uint8 and (lsb <= 1).mean() >= 0.999, (mode, kw)
    rng = np.random.default_rng(7)
    for h, w in ((2, 2), (3, 5), (7, 9)):                                           # tiny frames
        ti = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        td = rng.random((h, w), dtype=np.float32)
        for alpha in ("window", "rgba"):
            g = _run(dev, ti if rgb is not None else None, td, mode, alpha=alpha)
            _check(g, composite(ti, td, mode, alpha=alpha, depth_ratio=4.0), (mode, "tiny", h, w, alpha))


@pytest.mark.parametrize("mode", ["Anaglyph", "Interleaved", "Interleaved-V"])
def test_gather_kernel_when_the_window_does_not_fit(dev, mode):
    """roll == 0 but the LDS window would exceed 1536 words: a wide frame with very large parallax, and a viewport 16x narrower than
    the frame -- both take the gather kernel (comp_kernel, asserted from the launch plan), which must compute what the restatement
    computes."""
    from desktop2stereo_amd import ops, synth
    img, dep = synth.dibr_scene(24, 1600, 8, "boxes")
    tag = {"Anaglyph": "ana", "Interleaved": "il", "Interleaved-V": "ilv"}[mode]
    for kw in (dict(depth_ratio=150.0), dict(depth_ratio=4.0, viewport=(1, 0, 100, 24))):
        pl = ops.dibr_composite_plan(24, 1600, 1, 24, 1600, ops.dibr_params(0.064, **kw), mode, out_u8=False)
        assert pl["rows"] is False and pl["WW"] > 1536 and pl["kernel"] == f"comp<{tag},f32,roll0,FullDep>", (kw, pl)
        for alpha in ("window", "rgba"):
            got = _run(dev, img, dep, mode, alpha=alpha, **dict(kw))
            _check(got, composite(img, dep, mode, alpha=alpha, **kw), (mode, kw, alpha))


def test_depth_map_odd_tail_and_unaligned_output(dev):
    """Depth Map: an up-sampling viewport whose pixel count is odd (the last thread has fewer than four pixels), batch 1 and 3; and
    an output pointer that is not 16-byte aligned (byte / float stores instead of vector stores), which must give the same bits."""
    import ctypes as C
    from desktop2stereo_amd import _lib, ops, synth
    frames = [synth.dibr_scene(30, 52, s, "smooth")[1] for s in (1, 2, 3)]
    deps = np.stack(frames)
    vp = (0, 0, 61, 37)                                                             # 61 x 37 = 2257 pixels per frame
    for d in (deps[:1], deps):
        got = _run(dev, None, d, "Depth Map", viewport=vp)
        assert got.shape == (len(d), 37, 61, 3)
        for b in range(len(d)):
            _check(got[b], composite(None, d[b], "Depth Map", viewport=vp), ("odd tail", b))
    lib = _lib.load()
    dp = ops.dibr_params(viewport=vp)
    td = torch.from_numpy(deps).to(dev)
    for out_u8, alpha in ((True, "window"), (True, "rgba"), (False, "window"), (False, "rgba")):
        dp.alpha_mode = _lib.DIBR_ALPHA[alpha]
        ref = ops.dibr_composite(None, td, dp, "Depth Map", out_u8=out_u8)
        dt, off = (torch.uint8, 1) if out_u8 else (torch.float32, 1)                # offset by one element: 1 / 4 bytes
        buf = torch.zeros(ref.numel() + off, dtype=dt, device=dev)
        assert (buf.data_ptr() + off * buf.element_size()) % 16 != 0
        with ops._on(td.device) as st:
            ops.check(lib.d2s_dibr_composite(None, C.c_void_p(td.data_ptr()), 3, 30, 52, C.byref(dp), _lib.COMPOSITE["Depth Map"],
                                             C.c_void_p(buf.data_ptr() + off * buf.element_size()),
                                             _lib.FMT_U8_HWC if out_u8 else _lib.FMT_F32_HWC, st), "d2s_dibr_composite")
        got = buf[off:].reshape(ref.shape)
        assert torch.equal(got, ref), (out_u8, alpha)
        assert int(buf[0].item()) == 0                                              # nothing written in front of the output


def test_repeat_is_bit_identical(dev):
    from desktop2stereo_amd import synth
    img, dep = synth.dibr_scene(270, 480, 5, "boxes")
    for mode in MODES:
        a = _run(dev, img, dep, mode, out_u8=False, viewport=(1, 1, 480, 270))
        b = _run(dev, img, dep, mode, out_u8=False, viewport=(1, 1, 480, 270))
        assert np.array_equal(a, b), mode


def test_composite_view_surface(dev):
    from desktop2stereo_amd import _lib, depth as D, synth
    img, dep = synth.dibr_scene(120, 200, 6, "boxes")
    for mode in MODES:
        out = D.composite_view(img, dep, mode, depth_ratio=3.0)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (120, 200, 3)
        _check(out, composite(img, dep, mode, depth_ratio=3.0), ("composite_view", mode))
        chw = torch.from_numpy(img).permute(2, 0, 1).float()
        out2 = D.composite_view(chw, torch.from_numpy(dep), mode, depth_ratio=3.0)
        assert np.array_equal(out, out2)
    vp = (1, 0, 400, 240)
    out = D.composite_view(img, dep, "Interleaved", viewport=vp)
    assert out.shape == (240, 400, 3)
    _check(out, composite(img, dep, "Interleaved", depth_ratio=2.0, viewport=vp), "composite_view viewport")
    dm = D.composite_view(None, dep, "Depth Map")
    _check(dm, composite_frag(img, dep, "Depth Map")[..., :3], "depth map without frames")
    with pytest.raises(ValueError):
        D.composite_view(img, dep, "Half-SBS")
    with pytest.raises(ValueError):
        D.make_sbs(img, dep, inpaint=True, display_mode="Anaglyph")
    with pytest.raises(_lib.D2SError):
        D.composite_view(img, dep, "Anaglyph", viewport=(0.5, 0, 10, 10))
