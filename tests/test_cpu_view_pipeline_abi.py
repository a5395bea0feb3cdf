"""C-ABI of the Viewer pipeline (include/d2s.h: d2s_dibr_warp_depth, d2s_dibr_composite_depth, d2s_view_pipeline_streams), on the
host: the symbols and the refusals.  Every argument check comes before any HIP call, so these run without a device (the fake
device pointers are never dereferenced: each call returns at the first failed check)."""
import ctypes as C
import os

import pytest

from desktop2stereo_amd import _lib, ops
from desktop2stereo_amd.config import PipelineParams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d2s_dibr_warp_depth", "d2s_dibr_composite_depth", "d2s_view_pipeline_streams")
FAKE = C.c_void_p(16)
F32 = _lib.FMT_F32_HWC


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def test_symbols_and_version(lib):
    assert lib.d2s_version() >= 113
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in hdr, name
    # the two _depth entries take (dh, dw) right after the depth pointer, the rest as the entries they extend
    for name in ("d2s_dibr_warp", "d2s_dibr_composite"):
        a, b = _lib.SYMBOLS[name][1], _lib.SYMBOLS[name + "_depth"][1]
        assert b == a[:2] + [C.c_int, C.c_int] + a[2:], name


def _warp(lib, dp, rgb=FAKE, depth=FAKE, dh=42, dw=70, batch=1, H=90, W=160, out=FAKE, fmt=F32):
    return lib.d2s_dibr_warp_depth(rgb, depth, dh, dw, batch, H, W, C.byref(dp), out, fmt, None)


def _comp(lib, dp, rgb=FAKE, depth=FAKE, dh=42, dw=70, batch=1, H=90, W=160, mode=0, out=FAKE, fmt=F32):
    return lib.d2s_dibr_composite_depth(rgb, depth, dh, dw, batch, H, W, C.byref(dp), mode, out, fmt, None)


def test_depth_entries_refuse_before_any_pointer_is_touched(lib):
    dp = ops.dibr_params()
    for call in (_warp, _comp):
        for kw in (dict(dh=0), dict(dw=0), dict(dh=-3), dict(dw=-1)):
            assert call(lib, dp, **kw) == 1, (call.__name__, kw)
            assert b"depth shape" in lib.d2s_last_error(), (call.__name__, kw, lib.d2s_last_error())
        for kw in (dict(batch=0), dict(batch=-2), dict(H=0), dict(W=-3)):
            assert call(lib, dp, **kw) == 1, (call.__name__, kw)
        bad = ops.dibr_params()
        bad.struct_size = 72
        assert call(lib, bad) == 1 and b"struct_size" in lib.d2s_last_error()
        assert call(lib, dp, depth=None) == 1 and call(lib, dp, out=None) == 1
        assert b"null" in lib.d2s_last_error()
        assert call(lib, dp, fmt=_lib.FMT_F32_CHW) == 1 and b"out_fmt" in lib.d2s_last_error()
    assert _warp(lib, dp, rgb=None) == 1
    assert _comp(lib, dp, mode=4) == 1 and _comp(lib, dp, mode=-1) == 1 and b"composite" in lib.d2s_last_error()
    for m in ("Anaglyph", "Interleaved", "Interleaved-V"):
        assert _comp(lib, dp, rgb=None, mode=_lib.COMPOSITE[m]) == 1 and b"rgb" in lib.d2s_last_error()
    for vp in ((0, 0, -5, 10), (0.5, 0, 10, 10), (0, 0, 10, 0), (-1, 0, 10, 10)):
        assert _comp(lib, ops.dibr_params(viewport=vp)) == 1 and b"viewport" in lib.d2s_last_error(), vp
    assert _warp(lib, ops.dibr_params(viewport=(0, 0, -5, 10))) == 1 and b"viewport" in lib.d2s_last_error()


def _view(lib, dp, e=None, frames=FAKE, batch=1, ids=None, H=90, W=160, res=84, view=-1, out=FAKE, fmt=F32):
    pp = ops.post_params(PipelineParams())
    return lib.d2s_view_pipeline_streams(e, frames, batch, ids, H, W, res, None, C.byref(pp), C.byref(dp), view, 0, out, fmt, None, None)


def test_view_pipeline_refusals_without_device(lib):
    dp = ops.dibr_params()
    assert _view(lib, dp) == 1 and b"null engine" in lib.d2s_last_error()           # everything else in order: the engine is what is missing
    for view in range(4):
        assert _view(lib, dp, view=view) == 1 and b"null engine" in lib.d2s_last_error(), view
    for view in (-2, 4, 17):
        assert _view(lib, dp, view=view) == 1 and b"view" in lib.d2s_last_error(), view
    bad = ops.dibr_params()
    bad.struct_size = 72
    for view in (-1, 0, 3):
        assert _view(lib, bad, view=view) == 1 and b"struct_size" in lib.d2s_last_error(), view
    for vp in ((0, 0, -5, 10), (0.5, 0, 10, 10), (0, 0, 10, 0), (-1, 0, 10, 10)):
        assert _view(lib, ops.dibr_params(viewport=vp), view=_lib.COMPOSITE["Interleaved"]) == 1, vp
        assert b"viewport" in lib.d2s_last_error(), (vp, lib.d2s_last_error())
    bad_mode = ops.dibr_params()
    bad_mode.display_mode = 9
    assert _view(lib, bad_mode) == 1 and b"display_mode" in lib.d2s_last_error()
    assert _view(lib, dp, frames=None) == 1 and _view(lib, dp, out=None) == 1 and b"null pointer" in lib.d2s_last_error()
    assert _view(lib, dp, H=0) == 1 and _view(lib, dp, W=-4, view=1) == 1


def test_python_surface_refusals():
    with pytest.raises(ValueError):
        ops.dibr_composite(None, None, ops.dibr_params(), "Full-SBS")
    assert "view_pipeline" in dir(ops.Engine)
    import inspect
    from desktop2stereo_amd import depth
    sig = inspect.signature(depth.pipeline)
    assert sig.parameters["inpaint"].default is False and sig.parameters["viewport"].default is None
    assert list(inspect.signature(ops.Engine.view_pipeline).parameters)[1:] == ["frames", "p", "dp", "view", "use_ema", "out_u8", "want_depth",
                                                                               "out", "streams"]
