"""C-ABI of the viewer's composite modes (include/d2s.h: d2s_dibr_composite, d2s_dibr_composite_shape), on the host: the symbols,
the output shape of a viewport, and the refusals -- every argument check comes before any HIP call, so these run without a device
(null device pointers are never dereferenced: the call returns at the first failed check)."""
import ctypes as C
import os

import pytest

from desktop2stereo_amd import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def _shape(lib, H, W, dp, mode):
    oh, ow = C.c_int(-1), C.c_int(-1)
    rc = lib.d2s_dibr_composite_shape(H, W, C.byref(dp), mode, C.byref(oh), C.byref(ow))
    return rc, (oh.value, ow.value)


def test_symbols_and_version(lib):
    assert lib.d2s_version() >= 111
    for name in ("d2s_dibr_composite", "d2s_dibr_composite_shape"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for k, v in _lib.COMPOSITE.items():
        enum = "D2S_COMPOSITE_" + k.upper().replace("-", "_").replace(" ", "_")
        assert f"{enum} = {v}" in hdr, enum


def test_plan_symbol_struct_and_refusals(lib):
    """d2s_dibr_composite_plan (d2s_version() >= 134): declared, exported, its result 128 bytes, a wrong struct_size refused, and what
    the launcher refuses of these arguments refused here too"""
    assert lib.d2s_version() >= 134
    assert "d2s_dibr_composite_plan" in _lib.SYMBOLS and lib.d2s_dibr_composite_plan is not None
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    assert "int d2s_dibr_composite_plan(" in hdr and "} d2s_dibr_composite_plan_result;" in hdr
    R = _lib.DibrCompositePlanResult
    assert C.sizeof(R) == 4 + 4 * 4 + 4 * 4 + 2 * 4 + 4 * 4 + 2 * 4 + 64 == 132
    assert [f[0] for f in R._fields_] == ["struct_size", "rows", "cols", "margin", "ww", "roll0", "up", "fx", "vec", "out_h", "out_w", "grid",
                                          "block", "lds_dynamic_bytes", "lds_static_bytes", "kernel"]
    dp = ops.dibr_params()
    r = R()

    def call(dh=90, dw=160, batch=1, H=90, W=160, p=dp, mode=0, fmt=_lib.FMT_U8_HWC, align=0, res=r):
        return lib.d2s_dibr_composite_plan(dh, dw, batch, H, W, C.byref(p) if p is not None else None, mode, fmt, align,
                                           C.byref(res) if res is not None else None)
    assert call() == 1 and b"struct_size" in lib.d2s_last_error()              # struct_size 0
    r.struct_size = C.sizeof(R) - 4
    assert call() == 1 and b"struct_size" in lib.d2s_last_error()
    r.struct_size = C.sizeof(R)
    assert call() == 0 and r.kernel == b"comp_rows<ana,u8,fx=0,256,FullDep>" and (r.out_h, r.out_w) == (90, 160)
    assert call(p=None) == 1 and b"null pointer" in lib.d2s_last_error() and call(res=None) == 1
    assert call(mode=4) == 1 and b"composite" in lib.d2s_last_error()
    for kw, msg in ((dict(batch=0), b"bad batch"), (dict(H=1), b"bad shape"), (dict(dh=0), b"bad depth shape"), (dict(fmt=99), b"out_fmt"),
                    (dict(p=ops.dibr_params(viewport=(0.5, 0, 10, 10))), b"viewport"), (dict(p=ops.dibr_params(search_radius=16.0)), b"search_radius")):
        assert call(**kw) == 1 and msg in lib.d2s_last_error(), kw
    assert call(mode=3, align=4) == 0 and r.kernel == b"depth_map<u8,3,scalar,FullDep>" and r.vec == 0
    assert call(mode=3, dh=5, dw=19, fmt=_lib.FMT_F32_HWC, p=ops.dibr_params(alpha="rgba")) == 0 and r.kernel == b"depth_map<f32,4,vec,UpDep>"
    assert ops.dibr_composite_plan(90, 160, 1, 90, 160, dp, "Interleaved-V", out_u8=False)["kernel"] == "comp_rows<ilv,f32,fx=0,256,FullDep>"
    with pytest.raises(ValueError):
        ops.dibr_composite_plan(90, 160, 1, 90, 160, dp, "Full-SBS")


def test_shape(lib):
    dp = ops.dibr_params()
    for mode in range(4):
        assert _shape(lib, 1080, 1920, dp, mode) == (0, (1080, 1920))          # zero viewport: the frame itself
    dp = ops.dibr_params(viewport=(0, 0, 3840, 2160))                         # a 1080p frame on a 4K panel
    assert _shape(lib, 1080, 1920, dp, _lib.COMPOSITE["Interleaved"]) == (0, (2160, 3840))
    dp = ops.dibr_params(viewport=(7, 3, 101, 55))
    assert _shape(lib, 90, 160, dp, _lib.COMPOSITE["Anaglyph"]) == (0, (55, 101))


def test_rejections_without_device(lib):
    dp = ops.dibr_params()
    fake = C.c_void_p(16)                      # never dereferenced: every case fails a check first
    f32 = _lib.FMT_F32_HWC

    def call(rgb=fake, depth=fake, batch=1, H=90, W=160, p=dp, mode=0, out=fake, fmt=f32):
        return lib.d2s_dibr_composite(rgb, depth, batch, H, W, C.byref(p), mode, out, fmt, None)
    assert call(mode=4) == 1 and call(mode=-1) == 1
    assert b"composite" in lib.d2s_last_error()
    assert _shape(lib, 90, 160, dp, 7)[0] == 1
    bad = ops.dibr_params()
    bad.struct_size = 72
    assert call(p=bad) == 1 and b"struct_size" in lib.d2s_last_error()
    assert _shape(lib, 90, 160, bad, 0)[0] == 1
    for kw in (dict(batch=0), dict(H=0), dict(W=-3), dict(batch=-1)):
        assert call(**kw) == 1, kw
    assert _shape(lib, 0, 160, dp, 0)[0] == 1 and _shape(lib, 90, -1, dp, 0)[0] == 1
    for m in ("Anaglyph", "Interleaved", "Interleaved-V"):
        assert call(rgb=None, mode=_lib.COMPOSITE[m]) == 1 and b"rgb" in lib.d2s_last_error()
    assert call(depth=None) == 1 and call(out=None) == 1
    assert call(fmt=_lib.FMT_F32_CHW) == 1
    for vp in ((0, 0, -5, 10), (0.5, 0, 10, 10), (0, 0, 10, 0), (-1, 0, 10, 10)):
        assert call(p=ops.dibr_params(viewport=vp)) == 1, vp
        assert _shape(lib, 90, 160, ops.dibr_params(viewport=vp), 1)[0] == 1, vp


def test_python_surface_refusals():
    with pytest.raises(ValueError):
        ops.dibr_composite(None, None, ops.dibr_params(), "Full-SBS")


def test_shape_accepts_what_the_call_accepts(lib):
    """d2s_dibr_composite_shape and d2s_dibr_composite apply the same frame / viewport limits: a shape is never handed out for a
    call that would then be refused (checked on inputs the call refuses before touching any pointer)."""
    fake = C.c_void_p(16)
    for H, W, vp in ((1, 160, None), (90, 1, None), (70000, 2, None), (90, 160, (0, 0, 10, 0)), (90, 160, (0.5, 0, 10, 10)),
                     (30000, 30000, None)):
        dp = ops.dibr_params(viewport=vp or (0.0, 0.0, 0.0, 0.0))
        for mode in range(4):
            rc_shape = _shape(lib, H, W, dp, mode)[0]
            rc_call = lib.d2s_dibr_composite(fake, fake, 1, H, W, C.byref(dp), mode, fake, _lib.FMT_F32_HWC, None)
            assert rc_shape == 1 and rc_call == 1, (H, W, vp, mode, rc_shape, rc_call)
    assert _shape(lib, 2, 2, ops.dibr_params(), 0) == (0, (2, 2))
