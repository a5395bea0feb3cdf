"""CPU: which fusion stages run their residual unit (+ 1x1 projection) and which taps their RCU1 as one launch of the kernel's WIDE
form (8 x 8-pixel tiles, conv3.hip conv3_rcu_kernel<PROJ, 1>) -- plan_forward's rcu_wide / rcu1_wide (forward_plan.h; the rule is
c3_rcu_wide_ok in conv3.hip), reported by d2s_forward_plan in bits 16-19 / 24-26 of the rcu_fused word.  Without a GPU the library plans
for 256 CUs, the MI355X's count.  The rule: the conditions of the 4 x 8 form (a bf16 engine with plain row epilogues, fusion width 128),
a map the 4 x 8 form does not admit, and 8 x 8-pixel tiles x frames <= 256."""
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


def plan(model="vitb", B=1, prec="bf16", h=294, w=518, **kw):
    return ops.forward_plan(MODELS[model], h, w, B, prec, **kw)


def wide(*a, **kw):
    p = plan(*a, **kw)
    return p["rcu_wide"], p["rcu1_wide"]


def tiles48(H, W):
    return -(-H // 4) * -(-W // 8)


def tiles88(H, W):
    return -(-H // 8) * -(-W // 8)


NONE = ([False] * 4, [False] * 3)


def test_vitb_frame(lib):
    """294 x 518: the 84 x 148 map (399 tiles of 4 x 8, 209 of 8 x 8) is stage 3's and tap 0's; the smaller maps stay with the 4 x 8 form"""
    assert lib.d2s_version() >= 131
    p = plan()
    assert (p["fH"], p["fW"]) == ([84, 42, 21, 11], [148, 74, 37, 19])
    assert [tiles48(H, W) for H, W in zip(p["fH"], p["fW"])] == [399, 110, 30, 9]
    assert [tiles88(H, W) for H, W in zip(p["fH"], p["fW"])] == [209, 60, 15, 6]
    assert (p["rcu_wide"], p["rcu1_wide"]) == ([False, False, False, True], [True, False, False])
    assert (p["rcu_fused"], p["rcu1_fused"]) == ([True, True, True, False], [False, True, True])          # unchanged, and never both
    assert wide(profiling=True) == ([False, False, False, True], [True, False, False])


def test_batch_thresholds(lib):
    """8 x 8 tiles x frames against 256, on the maps the 4 x 8 tiles no longer fit: nothing at 2 frames (84 x 148: 418; 42 x 74 still fits
    the 4 x 8 form), the 42 x 74 map (60 tiles) at 3-4 frames, nothing at 5-8, the 21 x 37 map at 9-17, nothing beyond"""
    assert wide(B=2) == NONE
    assert wide(B=3) == ([False, False, True, False], [False, True, False])
    assert wide(B=4) == ([False, False, True, False], [False, True, False])
    assert wide(B=5) == NONE and wide(B=8) == NONE
    assert 2 * 209 > 256 and 2 * 110 <= 256 < 3 * 110 and 4 * 60 <= 256 < 5 * 60
    # the 21 x 37 map (30 tiles of 4 x 8, 15 of 8 x 8) from 9 frames to 17
    assert wide(B=9) == ([False, True, False, False], [False, False, True])
    assert wide(B=17) == ([False, True, False, False], [False, False, True])
    assert wide(B=18) == NONE
    assert 8 * 30 <= 256 < 9 * 30 and 17 * 15 <= 256 < 18 * 15
    # the 11 x 19 map (9 / 6 tiles) would fit from 29 frames to 42: beyond the batches the keep / drop table was measured at, so it keeps
    # its launches -- batch 32 is unchanged
    assert 28 * 9 <= 256 < 29 * 9 and 42 * 6 <= 256
    assert wide(B=29) == NONE and wide(B=32) == NONE and wide(B=42) == NONE
    for B in (1, 2, 3, 4, 5, 9, 17, 32):
        p = plan(B=B)
        assert not any(a and b for a, b in zip(p["rcu_fused"], p["rcu_wide"])) and not any(a and b for a, b in zip(p["rcu1_fused"], p["rcu1_wide"]))


def test_other_engines_keep_the_separate_launches(lib):
    assert wide("vits") == NONE and wide("vitl") == NONE                         # fusion width 64 / 256
    assert wide(prec="fp32") == NONE and wide(prec="bf16x3") == NONE
    assert wide(prec="fp8") == NONE and wide(prec="fp8_mlp") == NONE
    assert wide(prec="fp8", calibrating=True, calibrated=False) == NONE                # the calibration pass of an e4m3 engine
    with env(D2S_RCU_FUSE="0"):
        assert wide() == NONE
    assert wide() == ([False, False, False, True], [True, False, False])


def test_temporal_engine_takes_the_same_rule(lib):
    """ViT-B Video-Depth-Anything: RCU2 + projection of the last stage and tap 0's RCU1 have no temporal module in between"""
    assert wide(temporal=True) == ([False, False, False, True], [True, False, False])
    assert wide("vits", h=196, w=336, temporal=True) == NONE


def test_result_struct_keeps_its_size(lib):
    """the wide bits live in the rcu_fused word: the struct keeps its 328 bytes and its offsets"""
    R = _lib.ForwardPlanResult
    assert C.sizeof(R) == 328 and R.rcu_fused.offset == 308 and R.ln_launches.offset == 304 and R.splitk_elems.offset == 312
