"""CPU: the C ABI of several Video-Depth-Anything streams on one engine (include/d2s.h, d2s_version() >= 112) -- the three symbols
are exported and bound, their argument checks answer without a device, and depth.configure accepts a temporal engine with more
than one stream slot (no engine is built before the first frame, so none of this needs a GPU)."""
import ctypes as C
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("d2s_model_forward_streams", "d2s_pipeline_streams", "d2s_engine_reset_stream_at")


@pytest.fixture(scope="module")
def lib():
    from desktop2stereo_amd import _lib
    return _lib.load()


def test_stream_symbols_are_declared_bound_and_exported(lib):
    from desktop2stereo_amd import _lib
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in hdr, name
        assert getattr(lib, name) is not None
    assert lib.d2s_version() >= 112
    assert "#define D2S_MAX_STREAMS 32" in hdr


def test_stream_entry_points_refuse_null_without_a_device(lib):
    assert lib.d2s_engine_reset_stream_at(None, 0) != 0
    assert b"null" in lib.d2s_last_error()
    ids = (C.c_int * 2)(0, 1)
    assert lib.d2s_model_forward_streams(None, None, None, 2, ids, None) != 0
    assert b"null" in lib.d2s_last_error()
    assert lib.d2s_pipeline_streams(None, None, 2, ids, 1080, 1920, 336, None, None, None, 0, None, 0, None, None) != 0
    assert b"null" in lib.d2s_last_error()


def test_configure_accepts_a_multi_stream_vda_engine():
    from desktop2stereo_amd import _lib, depth
    saved = dict(depth._state)
    try:
        # (seeded synthetic weights; configure only records them -- the engine is built on the first frame)
        depth.configure("depth-anything/Video-Depth-Anything-Small", max_batch=4)
        assert depth._state["max_batch"] == 4 and depth._state["temporal"] is True and depth._state["engine"] is None
        depth.reset_stream()                                    # nothing built yet: a no-op
        depth.reset_stream(3)
        with pytest.raises(_lib.D2SError):
            depth.reset_stream(4)                               # a slot the configured engine will not have
    finally:
        depth._state.clear()
        depth._state.update(saved)                              # leave the module as other tests expect to find it
