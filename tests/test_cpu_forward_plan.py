"""CPU: d2s_forward_plan (host code, no GPU) is held to a table with one case either side of every threshold of plan_forward
(desktop2stereo_amd/csrc/forward_plan.h): which LayerNorms of a frame are launches and which fold into the linears either side of them,
which linears take e4m3 operands, which neck branches run on the side stream, the head's folds and fused tail, the temporal modules'
folded forms, and the engine geometry -- for the four models at 1080p -> 518 (294 x 518: 778 tokens).  Without a GPU the library plans
for 256 CUs, the MI355X's count, so the table is the same on both kinds of machine."""
import contextlib
import ctypes as C
import dataclasses
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


def plan(model="vitb", B=1, prec="bf16", h=294, w=518, cfg=None, **kw):
    return ops.forward_plan(cfg or MODELS[model], h, w, B, prec, **kw)


def ln_count(cfg, p):
    """LayerNorm launches the flags imply: layer 0's LN1 always, LN1 of the other layers / LN2 / the four taps unless folded."""
    s = p["sites"]
    return 1 + (cfg.layers - 1) * (not s["qkv"]["folded"]) + cfg.layers * (not s["fc1"]["folded"]) + 4 * (not s["neck0"]["folded"])


# (model, batch, precision, environment) -> (lnf, pp_fold, tap_fold, [slots after proj, after FC2], LayerNorm launches)
REGIMES = [
    # bf16: LN1 / LN2 fold up to 3 frames; the taps at 1 frame only (12 / 2 / 6 / 16 column blocks of the 32 x 64 tile)
    ("vitb", 1, "bf16", {}, True, False, True, [12, 12], 1), ("vitb", 2, "bf16", {}, True, False, False, [12, 12], 5),
    ("vitb", 3, "bf16", {}, True, False, False, [12, 12], 5), ("vitb", 4, "bf16", {}, False, False, False, [0, 0], 28),
    ("tiny", 1, "bf16", {}, True, False, True, [2, 2], 1), ("tiny", 3, "bf16", {}, True, False, False, [2, 2], 5),
    ("tiny", 4, "bf16", {}, False, False, False, [0, 0], 12),
    ("vits", 1, "bf16", {}, True, False, True, [6, 6], 1), ("vitl", 1, "bf16", {}, True, False, True, [16, 16], 1),
    # pp_fold: ceil(778 B / 256) * (D / 256) >= 100 -- ViT-B from 11 frames (34 * 3), ViT-L from 8 (25 * 4); one partial per 256 columns
    ("vitb", 10, "bf16", {}, False, False, False, [0, 0], 28), ("vitb", 11, "bf16", {}, True, True, True, [3, 3], 1),
    ("vitl", 7, "bf16", {}, False, False, False, [0, 0], 52), ("vitl", 8, "bf16", {}, True, True, True, [4, 4], 1),
    ("vitb", 32, "bf16", {}, True, True, True, [3, 3], 1),
    # tiny and ViT-S never (D % 256)
    ("tiny", 32, "bf16", {}, False, False, False, [0, 0], 12), ("vits", 32, "bf16", {}, False, False, False, [0, 0], 28),
    # bf16x3: up to 8 frames (no ping-pong kernel to give way to), the taps never; fp32 never
    ("vitb", 8, "bf16x3", {}, True, False, False, [6, 6], 5), ("vitb", 9, "bf16x3", {}, False, False, False, [0, 0], 28),
    ("vitb", 1, "bf16x3", {}, True, False, False, [12, 12], 5), ("vitb", 32, "bf16x3", {}, False, False, False, [0, 0], 28),
    ("vitb", 1, "fp32", {}, False, False, False, [0, 0], 28),
    # the switches
    ("vitb", 1, "bf16", dict(D2S_NO_LNFUSE="1"), False, False, False, [0, 0], 28),
    ("vitb", 11, "bf16", dict(D2S_NO_LNFUSE="1"), False, False, False, [0, 0], 28),
    ("vitb", 11, "bf16", dict(D2S_LNF_PP="0"), False, False, False, [0, 0], 28),
    ("vitb", 1, "bf16", dict(D2S_LNF_PP="0"), True, False, True, [12, 12], 1),
    ("vitb", 11, "bf16", dict(D2S_GEMM_PP="0"), False, False, False, [0, 0], 28),
    ("vitb", 10, "bf16", dict(D2S_GEMM_PP="94"), False, False, False, [0, 0], 28),      # (the threshold is the switch's: 31 * 3 = 93 tiles)
    ("vitb", 10, "bf16", dict(D2S_GEMM_PP="93"), True, True, True, [3, 3], 1),
    ("vitb", 11, "bf16", dict(D2S_TAPS="1"), False, False, False, [0, 0], 28),
    ("vitb", 1, "bf16", dict(D2S_TAPS="1"), True, False, True, [12, 12], 1),
]


def test_forward_plan_regimes(lib):
    assert lib.d2s_version() >= 121
    for model, B, prec, ev, lnf, pp_fold, tap_fold, slots, ln in REGIMES:
        with env(**ev):
            p = plan(model, B, prec)
        what = (model, B, prec, ev, p)
        assert (p["lnf"], p["pp_fold"], p["tap_fold"], p["ln_slots"], p["ln_launches"]) == (lnf, pp_fold, tap_fold, slots, ln), what
        assert p["ln_launches"] == ln_count(MODELS[model], p), what
        s = p["sites"]
        assert s["proj"]["stats"] == s["fc1"]["folded"] == lnf and s["fc2"]["stats"] == s["qkv"]["folded"] == lnf, what
        assert s["fc2_last"]["stats"] == tap_fold and all(s[f"neck{i}"]["folded"] == tap_fold for i in range(4)), what
        assert not s["qkv0"]["folded"] and not s["patch"]["folded"] and not any(v["e4m3"] for v in s.values()), what
        assert (p["x3"], p["f8"], p["f8a"]) == (prec == "bf16x3", False, False), what


def test_forward_plan_pp_threshold_arithmetic():
    """the two pp_fold boundaries of the table, from the rule: ceil(778 B / 256) * (D / 256) against 100 tiles"""
    tiles = lambda B, D: -(-778 * B // 256) * (D // 256)
    assert tiles(10, 768) == 93 < 100 <= tiles(11, 768) == 102 and tiles(7, 1024) == 88 < 100 <= tiles(8, 1024) == 100


def test_forward_plan_e4m3(lib):
    """D2S_PREC_FP8 against D2S_PREC_FP8_MLP: which linears take e4m3 operands, and LN1 staying a kernel on the MLP-only scheme (its
    output is QKV's bf16 operand); calibration runs the bf16 forms with every LayerNorm a kernel; not calibrated: refused."""
    e4 = lambda p: {k for k, v in p["sites"].items() if v["e4m3"]}
    p = plan("vitl", 1, "fp8")
    assert (p["f8"], p["f8a"], p["lnf"], p["tap_fold"], p["ln_launches"]) == (True, True, True, False, 1 + 4), p
    assert e4(p) == {"qkv0", "qkv", "proj", "fc1", "fc2", "fc2_last"} and p["sites"]["qkv"]["folded"] and p["sites"]["fc2"]["stats"], p
    p = plan("vitl", 1, "fp8_mlp")
    assert (p["f8"], p["f8a"], p["lnf"], p["ln_launches"]) == (True, False, True, 24 + 4), p
    assert e4(p) == {"fc1", "fc2", "fc2_last"} and not p["sites"]["qkv"]["folded"] and not p["sites"]["fc2"]["stats"], p
    assert p["sites"]["fc1"]["folded"] and p["sites"]["proj"]["stats"], p
    for prec, B in (("fp8", 4), ("fp8_mlp", 32)):                  # beyond 3 frames nothing folds, the operands stay e4m3
        p = plan("vitl", B, prec)
        assert (p["f8"], p["lnf"], p["pp_fold"], p["ln_launches"]) == (True, False, False, 52), p
    p = plan("vitl", 1, "fp8", calibrating=True, calibrated=False)
    assert (p["f8"], p["f8a"], p["lnf"], p["ln_launches"]) == (False, False, False, 52) and not e4(p), p
    with pytest.raises(_lib.D2SError, match="activation scales are not set, call d2s_engine_calibrate first"):
        plan("vitl", 1, "fp8", calibrated=False)
    with pytest.raises(_lib.D2SError, match="D2S_PLAN_CALIBRATING"):
        plan("vitb", 1, "bf16", calibrating=True)


def test_forward_plan_streams(lib):
    """taps 0..2 on the side stream, tap 3 too on a temporal engine (its branch queues behind branch 2's temporal module); profiling
    and D2S_NO_OVERLAP=1 keep everything on the caller's stream"""
    p = plan()
    assert p["use_side"] and p["tap_side"] == [True, True, True, False], p
    p = plan("vits", h=196, w=336, temporal=True)
    assert p["use_side"] and p["tap_side"] == [True] * 4, p
    for p in (plan(profiling=True), plan("vits", h=196, w=336, temporal=True, profiling=True)):
        assert not p["use_side"] and p["tap_side"] == [False] * 4, p
    with env(D2S_NO_OVERLAP="1"):
        p = plan()
    assert not p["use_side"] and p["tap_side"] == [False] * 4, p


def test_forward_plan_head(lib):
    """head2_fused either side of 224 tiles of 256 pixels (tiny, one frame: 291 / 292 patches of 196 pixels = 223 / 224 tiles); the
    up-sample folds are bf16 only and follow the kernels conv3_upsample_ok finds (tests/test_gpu_conv3.py EXPECTED_ENGINE pins them on
    the GPU: ViT-B at 1 and 8 frames runs both "-ups" cases on conv3.hip kernels, tiny -- 32 / 16 channels -- has them UNSUPPORTED)"""
    assert -(-42 * 1358 // 256) == 223 and -(-56 * 1022 // 256) == 224
    below, at = plan("tiny", h=42, w=1358), plan("tiny", h=56, w=1022)
    assert (below["head2_fused"], below["head2_ups"], at["head2_fused"], at["bn"]) == (False, False, True, 32), (below, at)
    for B in (1, 8):
        p = plan("vitb", B)
        assert (p["head1_ups"], p["head2_fused"], p["head2_ups"], p["bn"]) == (True, True, True, 32), p
        p = plan("tiny", B)
        assert (p["head1_ups"], p["head2_fused"], p["head2_ups"], p["bn"]) == (False, True, False, 32), p
    for prec in ("fp32", "bf16x3"):
        p = plan("vitb", 1, prec)
        assert (p["head1_ups"], p["head2_fused"], p["head2_ups"]) == (False, True, False), p
    p = plan(cfg=dataclasses.replace(MODELS["vitb"], head_hidden=128))          # more columns than a WN == 1 tile has
    assert not p["head2_fused"] and not p["head2_ups"], p


def test_forward_plan_more_than_16_slots(lib):
    """D = 1088 at one frame: the 32 x 64 tile leaves 17 partials per row, more than a consumer takes -- lnf holds, the producers run,
    and every LayerNorm is a launch"""
    cfg = dataclasses.replace(MODELS["vitb"], hidden=1088, heads=17)
    p = plan(cfg=cfg)
    s = p["sites"]
    assert p["lnf"] and p["tap_fold"] and p["ln_slots"] == [17, 17] and s["proj"]["stats"] and s["fc2"]["stats"], p
    assert not s["fc1"]["folded"] and not s["qkv"]["folded"] and not s["neck0"]["folded"] and p["ln_launches"] == 28 == ln_count(cfg, p), p
    p = plan(cfg=dataclasses.replace(MODELS["vitb"], hidden=1024, heads=16))    # 16: the most a consumer takes
    assert p["ln_slots"] == [16, 16] and p["ln_launches"] == 1, p


def test_forward_plan_temporal(lib):
    """a Video-Depth-Anything engine (ViT-S @ 196 x 336): the modules' (channels, sites), their three LayerNorms folded on bf16 (not on
    fp32, not with D2S_VDA_FUSE=0), and the ring store left to the attention kernel once the window is filled"""
    p = plan("vits", h=196, w=336, temporal=True)
    assert (p["gh"], p["gw"], p["fH"], p["fW"]) == (14, 24, [56, 28, 14, 7], [96, 48, 24, 12]), p
    assert p["tm_C"] == [192, 384, 64, 64] and p["tm_sites"] == [14 * 24, 7 * 12, 14 * 24, 28 * 48], p
    assert p["tm_fold"] and p["tm_folded"] == [[True] * 3] * 4 and p["tm_slots"] == [[3] * 3, [6] * 3, [1] * 3, [1] * 3], p
    assert p["ln_launches"] == 1 and p["tm_cache_store"], p
    assert not plan("vits", h=196, w=336, temporal=True, window_filled=True)["tm_cache_store"]
    for q in (plan("vits", 1, "fp32", h=196, w=336, temporal=True, window_filled=True),):
        assert not q["tm_fold"] and q["tm_folded"] == [[False] * 3] * 4 and q["ln_launches"] == 28 + 12 and q["tm_cache_store"], q
    with env(D2S_VDA_FUSE="0"):
        q = plan("vits", h=196, w=336, temporal=True)
    assert not q["tm_fold"] and q["tm_folded"] == [[False] * 3] * 4 and q["ln_launches"] == 1 + 12, q
    assert plan()["tm_C"] == [0] * 4 and not plan()["tm_fold"]


def test_forward_plan_geometry(lib):
    """engine_geom: what d2s_engine_finalize sizes the engine with"""
    p = plan("vitl", 7)
    assert (p["gh"], p["gw"], p["P"], p["N"], p["Npad"]) == (21, 37, 777, 778, 832), p
    assert p["fH"] == [84, 42, 21, 11] and p["fW"] == [148, 74, 37, 19], p
    assert p["splitk_elems"] == 7 * 16 * 21 * 37 * 1024 and p["scr_elems"] == 7 * max(64 * 777 * 256, 294 * 518 * 128), p
    p = plan("tiny", h=84, w=84)
    assert (p["P"], p["N"], p["Npad"], p["fH"], p["splitk_elems"]) == (36, 37, 64, [24, 12, 6, 3], 16 * 36 * 128), p


def test_forward_plan_refusals(lib):
    desc = ops.model_desc(MODELS["vitb"])
    r = _lib.ForwardPlanResult()
    r.struct_size = 8                                                                          # a short struct is refused
    assert lib.d2s_forward_plan(C.byref(desc), 294, 518, 1, 0, C.byref(r)) == 1 and b"struct_size" in lib.d2s_last_error()
    r.struct_size = C.sizeof(_lib.ForwardPlanResult)
    assert C.sizeof(_lib.ForwardPlanResult) == 328 and _lib.ForwardPlanResult.site.offset == 40 and _lib.ForwardPlanResult.gh.offset == 220
    assert _lib.ForwardPlanResult.splitk_elems.offset == 312
    assert lib.d2s_forward_plan(C.byref(desc), 294, 518, 1, 0, C.byref(r)) == 0
    assert lib.d2s_forward_plan(None, 294, 518, 1, 0, C.byref(r)) == 1 and b"null pointer" in lib.d2s_last_error()
    # d2s_engine_finalize's words
    assert lib.d2s_forward_plan(C.byref(desc), 295, 518, 1, 0, C.byref(r)) == 1 and b"h, w must be patch multiples" in lib.d2s_last_error()
    assert lib.d2s_forward_plan(C.byref(desc), 294, 518, 0, 0, C.byref(r)) == 1 and b"h, w must be patch multiples" in lib.d2s_last_error()
    vda = ops.model_desc(MODELS["vits"], temporal=True)
    assert lib.d2s_forward_plan(C.byref(vda), 196, 336, 33, 0, C.byref(r)) == 1 and b"at most D2S_MAX_STREAMS (32) stream slots" in lib.d2s_last_error()
    # d2s_engine_create's words
    for kw, msg in ((dict(heads=11), b"head_dim must be 64"), (dict(fusion=12), b"bad model desc"), (dict(head_hidden=30), b"bad head_hidden / mlp"),
                    (dict(out_indices=(3, 6, 9, 13)), b"bad neck / out_indices")):
        bad = ops.model_desc(dataclasses.replace(MODELS["vitb"], **kw))
        assert lib.d2s_forward_plan(C.byref(bad), 294, 518, 1, 0, C.byref(r)) == 1 and msg in lib.d2s_last_error(), kw
    bad = ops.model_desc(MODELS["vitb"])
    bad.precision = 7
    assert lib.d2s_forward_plan(C.byref(bad), 294, 518, 1, 0, C.byref(r)) == 1 and b"bad precision" in lib.d2s_last_error()
    bad = ops.model_desc(MODELS["vits"], temporal=True, max_depth=20.0)
    assert lib.d2s_forward_plan(C.byref(bad), 196, 336, 1, 0, C.byref(r)) == 1 and b"max_depth must be >= 0, and 0 for a Video-Depth-Anything engine" in lib.d2s_last_error()
