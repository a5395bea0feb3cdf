"""CPU: the OpenXR viewer's movie crop on the host (desktop2stereo_amd/crop.py, include/d2s.h d2s_version() >= 114).

The host logic -- sample_plan, crop_from_stats, pixel_bounds, MovieCrop's hysteresis and manual crop -- must EQUAL what the reference's
own xr_viewer/crop.py gave (tests/golden/crop_detect.npz/json, made by make_golden_crop_detect.py from its tensor path on CPU torch).
tests/xr_crop_ref.py, the restatement the GPU tests lean on, is held to the recorded stats and to renders of the reference's own XR
shader (tests/golden/xr_crop.npz, make_golden_xr_crop.py) at tests/test_composite_oracle.py's bounds: every value within 1 level on
the small cases, >= 99.9 % within 1 level and mean <= 0.06 beyond 320 columns, alpha within 1e-3.  The C ABI: symbols, header text,
version, and every refusal -- all before any HIP call, so fake device pointers are never touched."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from desktop2stereo_amd import _lib, crop as K, ops, synth
from desktop2stereo_amd.config import PipelineParams
import xr_crop_ref as X

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d2s_crop_detect_workspace", "d2s_crop_detect", "d2s_dibr_crop_shape", "d2s_dibr_warp_crop", "d2s_view_pipeline_crop_streams")
FAKE = C.c_void_p(16)
F32 = _lib.FMT_F32_HWC


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def det(golden_dir):
    with open(os.path.join(golden_dir, "crop_detect.json")) as f:
        return np.load(os.path.join(golden_dir, "crop_detect.npz")), json.load(f)


def test_sample_plan_equals_the_reference(det):
    z, meta = det
    assert {(c["h"], c["w"]) for c in meta["cases"]} == {(64, 64), (96, 160), (400, 731), (400, 730), (1080, 1920)}
    for c in meta["cases"]:
        p = K.sample_plan(c["w"], c["h"])
        assert {k: p[k] for k in c["plan"]} == c["plan"], c["name"]
        assert p["y_rows"] == z[c["name"] + "_y_rows"].tolist() and p["x_cols"] == z[c["name"] + "_x_cols"].tolist(), c["name"]
        assert sum(p["center_mask"]) == c["center_rows"]
        assert 51 <= p["samples_per_row"] <= 255 and 51 <= p["samples_per_col"] <= 255
    p64, p731, p730 = K.sample_plan(64, 64), K.sample_plan(731, 400), K.sample_plan(730, 400)
    assert p64["samples_per_row"] == 51 and p731["samples_per_row"] == 146
    assert (p731["row_stride"], p731["col_stride"]) == (2, 3) and p731["y_rows"][-2:] == [398, 399]
    assert p731["x_cols"][-2:] == [729, 730] and p730["x_cols"][-2:] == [726, 729]       # appended / not appended


def test_crop_from_stats_and_pixel_bounds_equal_the_reference(det):
    z, meta = det
    found = 0
    for c in meta["cases"]:
        crop = K.crop_from_stats(z[c["name"] + "_stats"].tolist(), c["w"], c["h"])
        assert tuple(crop) == tuple(c["crop"]), (c["name"], crop, c["crop"])
        assert list(K.pixel_bounds(c["w"], c["h"], crop)) == c["pixel_bounds"], c["name"]
        found += K.is_active(crop)
    by = {c["name"]: c for c in meta["cases"]}
    assert found >= 8
    for name in ("hd_asymmetric", "m730_under_min_bar", "hd_dark_centre", "m731_gradient", "hd_full"):
        assert by[name]["crop"] == [0.0, 0.0, 1.0, 1.0], name
    assert z["hd_dark_centre_stats"][0] > 0 and z["hd_dark_centre_stats"][2] < 14.0      # bars found, refused by the vote alone
    for b in meta["pixel_bounds"]:
        assert list(K.pixel_bounds(b["w"], b["h"], b["crop"])) == b["bounds"], b
    assert meta["pixel_bounds"][0]["bounds"][:2] == [2, 2] and meta["pixel_bounds"][1]["bounds"][:2] == [4, 2]     # half-to-even


def test_movie_crop_hysteresis_and_manual_equal_the_reference(det):
    _, meta = det
    mc = K.MovieCrop()
    saw_reset = False
    for s in meta["hysteresis"]["steps"]:
        was_active = mc.target_active
        mc.apply_detection(s["detected"], meta["hysteresis"]["h"])
        assert list(mc.target_uv) == s["target_uv"] and mc.target_active == s["target_active"] and mc.full_hits == s["full_hits"], s
        assert list(mc.crop_uv) == s["target_uv"]
        saw_reset |= was_active and not mc.target_active
    assert saw_reset
    for m in meta["manual"]:
        mm = K.MovieCrop(mode="manual")
        assert list(mm.set_manual(m["w"], m["h"])) == m["crop"] and list(mm.crop_uv) == m["crop"]
    off = K.MovieCrop(mode="off")
    off.apply_detection((0.0, 0.2, 1.0, 0.6), 1080)
    assert off.crop_uv == K.FULL
    with pytest.raises(ValueError):
        K.MovieCrop(mode="sometimes")


def test_movie_crop_interval_and_poll_with_an_injected_clock(monkeypatch):
    """update() launches at most once per max(0.2, interval) and never while a result is pending; poll() applies a finished result
    through the hysteresis.  The detector and the event are stand-ins: no device."""
    torch = pytest.importorskip("torch")
    now = [100.0]
    launches = []

    class Event:
        def __init__(self, blocking=False): self.done = False
        def record(self, stream=None): pass
        def query(self): return self.done

    stats = torch.tensor([[46.0, 47.0, 111.4, 1.0, 0.0, 0.0]])

    def fake_detect(frames, out=None, workspace=None):
        assert workspace is not None                       # the capture's own, not the shared one
        launches.append(now[0])
        out.copy_(stats)
        return out
    monkeypatch.setattr(ops, "crop_detect", fake_detect)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    frames = torch.zeros((1080, 1920, 3), dtype=torch.uint8)
    mc = K.MovieCrop(interval=0.05, clock=lambda: now[0])
    assert mc.update(frames) and mc.pending and len(launches) == 1
    now[0] += 10.0
    assert not mc.update(frames) and len(launches) == 1 and mc.crop_uv == K.FULL          # still in flight: nothing new, nothing applied
    mc._pending["event"].done = True
    assert mc.poll() is False and not mc.pending
    assert mc.crop_uv == K.crop_from_stats(stats[0].tolist(), 1920, 1080) and K.is_active(mc.crop_uv)
    now[0] = 200.0
    assert mc.update(frames) and len(launches) == 2
    mc._pending["event"].done = True
    now[0] += 0.1                                                                          # interval 0.05 is floored to 0.2
    assert not mc.update(frames) and len(launches) == 2 and not mc.pending
    now[0] += 0.15
    assert mc.update(frames) and len(launches) == 3
    small = K.MovieCrop(clock=lambda: now[0])
    assert not small.update(torch.zeros((48, 160, 3), dtype=torch.uint8)) and len(launches) == 3      # crop.py:369


def test_float64_stats_restatement_matches_the_recorded_stats(det):
    z, meta = det
    for c in meta["cases"]:
        img = synth.letterbox_frame(c["h"], c["w"], c["seed"], **c["frame"])
        got, want = X.crop_stats(img, K.sample_plan(c["w"], c["h"])), z[c["name"] + "_stats"]
        assert [got[i] for i in (0, 1, 4, 5)] == [want[i] for i in (0, 1, 4, 5)], (c["name"], got, want)
        assert abs(got[2] - want[2]) <= 4e-3 and abs(got[3] - want[3]) <= 2e-5, (c["name"], got, want)


def _xr_cases(golden_dir):
    with open(os.path.join(golden_dir, "xr_crop.json")) as f:
        return np.load(os.path.join(golden_dir, "xr_crop.npz")), json.load(f)


def test_xr_fixture_manifest(golden_dir):
    z, meta = _xr_cases(golden_dir)
    assert "SwiftShader" in meta["gl"]["renderer"] and "_make_xr_fragment_shader" in meta["shader"]
    for c in meta["cases"]:
        x0, y0, x1, y1 = K.pixel_bounds(c["w"], c["h"], c["crop"])
        assert [x0, y0, x1, y1] == c["pixel_bounds"]
        assert (c["eye_w"], c["eye_h"]) == ((x1 - x0) // 2 if c["half_sbs"] else x1 - x0, y1 - y0)
        assert z[c["name"] + "_left_rgb"].shape == (len(range(0, c["eye_h"], c["row_stride"])), c["eye_w"], 3)
    assert any(c["crop"][0] + c["crop"][2] == 1.0 and c["crop"][0] > 0 for c in meta["cases"])
    assert min(float(z[c["name"] + "_left_a"].min()) for c in meta["cases"]) < 0.5 * 65535


XR_NAMES = ["xr_letterbox", "xr_pillarbox", "xr_both_roll", "xr_half_sbs", "xr_right_edge", "xr_feather", "xr_hd_239"]


@pytest.mark.parametrize("name", XR_NAMES)
def test_xr_restatement_matches_the_reference_shader_renders(golden_dir, name):
    z, meta = _xr_cases(golden_dir)
    c = next(c for c in meta["cases"] if c["name"] == name)
    img, dep = synth.dibr_scene(c["h"], c["w"], c["seed"], c["scene"])
    kw = dict(roll=c.get("roll", 0.0), feather=c.get("feather", False), feather_width=c.get("feather_width", 0.02),
              corner_radius=c.get("corner_radius", 0.0))
    for eye, sign in (("left", -1.0), ("right", 1.0)):
        o = X.dibr_eye_crop(img, dep, c["crop"], sign * c["ipd_uv"] / 2.0, 0.1 * c["depth_ratio"], c["convergence"], c["eye_h"], c["eye_w"],
                            **kw)[::c["row_stride"]]
        rgb = z[f"{name}_{eye}_rgb"].astype(np.float32) / 256.0
        a = z[f"{name}_{eye}_a"].astype(np.float32) / 65535.0
        d = np.abs(o[..., :3] - rgb)
        print(f"[xr restatement vs render, {name} {eye}] rgb max {d.max():.3f} mean {d.mean():.4f} {(d > 1).mean():.2e} beyond 1 level | "
              f"alpha max diff {np.abs(o[..., 3] - a).max():.1e}")
        assert np.abs(o[..., 3] - a).max() <= 1e-3, (name, eye, float(np.abs(o[..., 3] - a).max()))
        if c["w"] <= 320:
            assert d.max() <= 1.0, (name, eye, float(d.max()))
        else:
            assert (d <= 1.0).mean() >= 0.999 and d.mean() <= 0.06, (name, eye, float((d > 1).mean()), float(d.mean()))
    full = X.dibr_eye_crop(img, dep, (0.0, 0.0, 1.0, 1.0), -c["ipd_uv"] / 2.0, 0.1 * c["depth_ratio"], c["convergence"], c["eye_h"], c["eye_w"], **kw)
    assert np.abs(full[::c["row_stride"], :, :3] - z[f"{name}_left_rgb"].astype(np.float32) / 256.0).max() > 20      # the crop matters


def test_symbols_header_and_version(lib):
    assert lib.d2s_version() >= 114
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in hdr, name
    assert "xr_viewer/crop.py" in hdr and "xr_viewer/implementation.py:111-126" in hdr
    a, b = _lib.SYMBOLS["d2s_view_pipeline_streams"][1], _lib.SYMBOLS["d2s_view_pipeline_crop_streams"][1]
    assert b == a[:11] + [C.POINTER(C.c_double)] + a[11:]
    assert C.sizeof(_lib.DibrParams) == 80                                   # the crop is a separate argument


def _detect(lib, frames=FAKE, fmt=_lib.FMT_U8_HWC, batch=1, H=96, W=160, stats=FAKE, ws=FAKE, nbytes=1 << 20):
    return lib.d2s_crop_detect(frames, fmt, batch, H, W, stats, ws, nbytes, None)


def test_detector_refusals_without_device(lib):
    n = C.c_uint64()
    assert lib.d2s_crop_detect_workspace(1, 1080, 1920, C.byref(n)) == 0 and 0 < n.value < (1 << 20)
    one = n.value
    assert lib.d2s_crop_detect_workspace(32, 1080, 1920, C.byref(n)) == 0 and n.value == 32 * one
    for kw in (dict(H=63), dict(W=63), dict(H=0), dict(W=-5)):
        assert lib.d2s_crop_detect_workspace(1, kw.get("H", 96), kw.get("W", 160), C.byref(n)) == 1
        assert _detect(lib, **kw) == 1 and b"H and W" in lib.d2s_last_error(), kw
    assert lib.d2s_crop_detect_workspace(1, 96, 160, None) == 1 and b"bytes" in lib.d2s_last_error()
    assert lib.d2s_crop_detect_workspace(0, 96, 160, C.byref(n)) == 1 and b"batch" in lib.d2s_last_error()
    assert _detect(lib, frames=None) == 1 and b"frames" in lib.d2s_last_error()
    assert _detect(lib, stats=None) == 1 and b"stats" in lib.d2s_last_error()
    assert _detect(lib, ws=None) == 1 and b"workspace" in lib.d2s_last_error()
    for fmt in (_lib.FMT_F32_HWC, -1, 7):
        assert _detect(lib, fmt=fmt) == 1 and b"fmt" in lib.d2s_last_error(), fmt
    for batch in (0, -1, 70000):
        assert _detect(lib, batch=batch) == 1 and b"batch" in lib.d2s_last_error(), batch
    assert _detect(lib, nbytes=16) == 1 and b"workspace_bytes" in lib.d2s_last_error()
    assert _detect(lib, ws=C.c_void_p(18)) == 1 and b"aligned" in lib.d2s_last_error()


def _c4(*v):
    return (C.c_double * 4)(*v)


def _warp(lib, dp, crop, rgb=FAKE, depth=FAKE, dh=42, dw=70, batch=1, H=90, W=160, out=FAKE, fmt=F32):
    return lib.d2s_dibr_warp_crop(rgb, depth, dh, dw, batch, H, W, C.byref(dp), crop, out, fmt, None)


BAD_CROPS = [(float("nan"), 0, 1, 1), (0, float("inf"), 1, 1), (0, 0, 1, float("-inf")), (-0.01, 0, 1, 1), (0, -1e-3, 1, 1), (0, 0, 0, 1),
             (0, 0, 1, -0.5), (0.5, 0, 0.51, 1), (0, 0.2, 1, 0.81), (0, 0, 0.004, 1), (0, 0, 1, 0.01)]


def test_cropped_warp_refusals_without_device(lib):
    dp = ops.dibr_params()
    oh, ow = C.c_int(), C.c_int()
    for bad in BAD_CROPS:
        assert lib.d2s_dibr_crop_shape(90, 160, _c4(*bad), 1, C.byref(oh), C.byref(ow)) == 1 and b"crop" in lib.d2s_last_error(), bad
        assert _warp(lib, dp, _c4(*bad)) == 1 and b"crop" in lib.d2s_last_error(), bad
    ok = _c4(0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0)
    assert lib.d2s_dibr_crop_shape(90, 160, _c4(-5e-7, 0.0, 1.0 + 1e-6, 1.0), 1, C.byref(oh), C.byref(ow)) == 0      # the 1e-6 of slack
    assert (oh.value, ow.value) == (90, 320)
    for mode, want in ((0, (60, 160)), (1, (60, 320)), (2, (60, 160)), (3, (120, 160))):
        assert lib.d2s_dibr_crop_shape(90, 160, ok, mode, C.byref(oh), C.byref(ow)) == 0 and (oh.value, ow.value) == want, mode
    assert lib.d2s_dibr_crop_shape(90, 160, ok, 4, C.byref(oh), C.byref(ow)) == 1 and b"display_mode" in lib.d2s_last_error()
    assert lib.d2s_dibr_crop_shape(90, 160, None, 1, C.byref(oh), C.byref(ow)) == 1 and b"crop" in lib.d2s_last_error()
    assert lib.d2s_dibr_crop_shape(90, 160, ok, 1, None, C.byref(ow)) == 1
    assert lib.d2s_dibr_crop_shape(90, 160, _c4(0, 0, 3.0 / 160, 1), 0, C.byref(oh), C.byref(ow)) == 1 and b"viewport" in lib.d2s_last_error()
    assert _warp(lib, dp, None) == 1 and b"crop" in lib.d2s_last_error()
    assert _warp(lib, dp, ok, depth=None) == 1 and _warp(lib, dp, ok, out=None) == 1 and b"null" in lib.d2s_last_error()
    assert _warp(lib, dp, ok, dh=0) == 1 and b"depth shape" in lib.d2s_last_error()
    assert _warp(lib, dp, ok, fmt=_lib.FMT_F32_CHW) == 1 and b"out_fmt" in lib.d2s_last_error()
    bad = ops.dibr_params()
    bad.struct_size = 72
    assert _warp(lib, bad, ok) == 1 and b"struct_size" in lib.d2s_last_error()


def _view(lib, dp, crop, e=None, frames=FAKE, batch=1, H=90, W=160, res=84, view=-1, out=FAKE, fmt=F32):
    pp = ops.post_params(PipelineParams())
    return lib.d2s_view_pipeline_crop_streams(e, frames, batch, None, H, W, res, None, C.byref(pp), C.byref(dp), view, crop, 0, out, fmt, None, None)


def test_view_pipeline_crop_refusals_without_device(lib):
    dp, ok = ops.dibr_params(), _c4(0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0)
    assert _view(lib, dp, ok) == 1 and b"null engine" in lib.d2s_last_error()             # everything else in order
    for view in range(4):
        assert _view(lib, dp, ok, view=view) == 1 and b"view" in lib.d2s_last_error() and b"crop" in lib.d2s_last_error(), view
    assert _view(lib, dp, None) == 1 and b"crop" in lib.d2s_last_error()
    for bad in BAD_CROPS:
        assert _view(lib, dp, _c4(*bad)) == 1 and b"crop" in lib.d2s_last_error(), bad
    assert _view(lib, dp, ok, frames=None) == 1 and _view(lib, dp, ok, out=None) == 1


def test_python_surface():
    import inspect
    from desktop2stereo_amd import depth
    assert inspect.signature(depth.pipeline).parameters["crop"].default is None
    assert inspect.signature(ops.dibr_warp).parameters["crop"].default is None
    assert "view_pipeline_crop" in dir(ops.Engine) and callable(ops.crop_detect)
    with pytest.raises(ValueError):
        ops._crop4((0.0, 0.0, 1.0))
