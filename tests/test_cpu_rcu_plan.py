"""CPU: which fusion stages run their residual unit (+ 1x1 projection) and which taps their RCU1 as one launch -- plan_forward's
rcu_fused / rcu1_fused (desktop2stereo_amd/csrc/forward_plan.h, the rule is c3_rcu_ok in conv3.hip), reported by d2s_forward_plan.
Without a GPU the library plans for 256 CUs, the MI355X's count.  The rule: a bf16 engine with plain row epilogues, fusion width 128,
and every block of the launch resident at once, one per CU -- 4 x 8-pixel tiles x frames <= 256."""
import contextlib
import ctypes as C
import os

import pytest

from desktop2stereo_amd import _lib, ops
from desktop2stereo_amd.config import MODELS


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    ops.reload_env()
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        ops.reload_env()


def fused(model="vitb", B=1, prec="bf16", h=294, w=518, **kw):
    p = ops.forward_plan(MODELS[model], h, w, B, prec, **kw)
    return p["rcu_fused"], p["rcu1_fused"]


def tiles(H, W):
    return -(-H // 4) * -(-W // 8)


def test_vitb_frame(lib):
    """294 x 518: stages work on 11 x 19, 21 x 37, 42 x 74, 84 x 148 (9 / 30 / 110 / 399 tiles); taps 0..2 own the 84 x 148, 42 x 74 and
    21 x 37 maps"""
    assert lib.d2s_version() >= 125
    p = ops.forward_plan(MODELS["vitb"], 294, 518, 1)
    assert (p["fH"], p["fW"]) == ([84, 42, 21, 11], [148, 74, 37, 19])
    assert [tiles(H, W) for H, W in zip(p["fH"], p["fW"])] == [399, 110, 30, 9]
    assert fused() == ([True, True, True, False], [False, True, True])
    # profiling keeps the plan (the fused launch is bracketed like any other convolution)
    assert fused(profiling=True) == ([True, True, True, False], [False, True, True])


def test_batch_thresholds(lib):
    """tiles x frames against 256: the 42 x 74 map (110 tiles) leaves at 3 frames, 21 x 37 (30) at 9, 11 x 19 (9) at 29"""
    assert fused(B=2) == ([True, True, True, False], [False, True, True])
    assert fused(B=3) == ([True, True, False, False], [False, False, True])
    assert fused(B=8) == ([True, True, False, False], [False, False, True])
    assert fused(B=9) == ([True, False, False, False], [False, False, False])
    assert fused(B=28) == ([True, False, False, False], [False, False, False])
    assert fused(B=29) == ([False] * 4, [False] * 3)
    assert 2 * 110 <= 256 < 3 * 110 and 8 * 30 <= 256 < 9 * 30 and 28 * 9 <= 256 < 29 * 9


def test_other_engines_keep_the_separate_launches(lib):
    none = ([False] * 4, [False] * 3)
    assert fused("vits") == none and fused("vitl") == none                       # fusion width 64 / 256
    assert fused(prec="fp32") == none and fused(prec="bf16x3") == none
    assert fused(prec="fp8") == none and fused(prec="fp8_mlp") == none
    assert fused(prec="fp8", calibrating=True, calibrated=False) == none               # the calibration pass of an e4m3 engine
    with env(D2S_RCU_FUSE="0"):
        assert fused() == none
    assert fused() == ([True, True, True, False], [False, True, True])


def test_temporal_engine_takes_the_same_rule(lib):
    """ViT-B Video-Depth-Anything: RCU2 + projection of every stage whose map fits, the temporal modules sit behind the projection"""
    assert fused(temporal=True) == ([True, True, True, False], [False, True, True])
    assert fused("vits", h=196, w=336, temporal=True) == ([False] * 4, [False] * 3)


def test_result_struct_keeps_its_size(lib):
    """rcu_fused took the padding word in front of splitk_elems: a caller built against the 328-byte struct still works"""
    R = _lib.ForwardPlanResult
    assert C.sizeof(R) == 328 and R.rcu_fused.offset == 308 and R.ln_launches.offset == 304 and R.splitk_elems.offset == 312
