"""CPU: d2s_post_plan (host code, no GPU) is held to a table with one case either side of every threshold of plan_post
(desktop2stereo_amd/csrc/post.hip): which of the three forms of the depth post-process a call takes, which kernels, how many taps,
how much dynamic LDS, and the subsample the percentile bounds are taken from."""
import contextlib
import ctypes as C
import dataclasses
import os

import pytest

from desktop2stereo_amd import _lib, ops
from desktop2stereo_amd.config import PipelineParams


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


def plan(B=1, h=294, w=518, in_place=False, **kw):
    return ops.post_plan(B, h, w, dataclasses.replace(PipelineParams(), **kw), in_place)


def sb_bytes(r):
    return 4 * ((8 + 2 * r) * (128 + 2 * r) + (8 + 2 * r) * 128)


FUSED13, FUSED0 = ["post_fused<13>"], ["post_fused<0>"]
REL, MET = "percentile_bounds<relative>", "percentile_bounds<metric>"
ROWS13, ROWS0 = [REL, "shape_hblur<13>", "vblur<13>"], [REL, "shape_hblur<0>", "vblur<0>"]
# (arguments, environment) -> (form, kernels, k)
TABLE = [
    (dict(B=2), {}, "fused", FUSED13, 13), (dict(B=3), {}, "rows", ROWS13, 13),                             # batch against D2S_POST_FUSE_MAXB
    (dict(metric=False), {}, "fused", FUSED13, 13), (dict(metric=True), {}, "tile", [MET, "shape_blur"], 13),           # metric
    (dict(in_place=False), {}, "fused", FUSED13, 13), (dict(in_place=True), {}, "rows", ROWS13, 13),        # in place
    (dict(aa_strength=5.9), {}, "fused", FUSED0, 17), (dict(aa_strength=6.0), {}, "tile", [REL, "shape_blur"], 19),     # radius against 8
    (dict(aa_strength=15.9), {}, "tile", [REL, "shape_blur"], 47), (dict(aa_strength=16.0), {}, "rows", ROWS0, 49),     # tile LDS against 64 KiB
    (dict(aa_strength=4.0), {}, "fused", FUSED13, 13), (dict(aa_strength=2.0), {}, "fused", FUSED0, 7),     # tap instantiation
    (dict(aa_strength=4.0, B=3), {}, "rows", ROWS13, 13), (dict(aa_strength=2.0, B=3), {}, "rows", ROWS0, 7),
    (dict(aa_strength=0.2), {}, "fused", FUSED0, 1), (dict(aa_strength=0.6, B=3), {}, "rows", ROWS0, 1),    # blur off: one run-time tap
    (dict(metric=True, in_place=True), {}, "rows", [MET, "shape_hblur<13>", "vblur<13>"], 13),
    (dict(), dict(D2S_POST_ONE="0"), "tile", [REL, "shape_blur"], 13),
    (dict(), dict(D2S_POST_FUSE_MAXB="0"), "rows", ROWS13, 13),
    (dict(B=3), dict(D2S_POST_FUSE_MAXB="3"), "fused", FUSED13, 13),
]
# every name plan_post can return
NAMES = {"post_fused<13>", "post_fused<0>", REL, MET, "shape_blur", "shape_hblur<13>", "shape_hblur<0>", "vblur<13>", "vblur<0>"}


def test_post_plan_table(lib):
    assert lib.d2s_version() >= 120
    for kw, ev, form, kernels, k in TABLE:
        with env(**ev):
            p = plan(**kw)
        assert (p["form"], p["kernels"], p["k"], p["r"]) == (form, kernels, k, k // 2), (kw, ev, p)
        w = kw.get("w", 518)
        want_lds = {"fused": [0], "tile": [0, sb_bytes(k // 2)], "rows": [0, 4 * (w + 2 * (k // 2)), 0]}[form]
        assert p["lds_bytes"] == want_lds, (kw, ev, p)
    assert sb_bytes(23) == 65232 and sb_bytes(24) == 68096 and sb_bytes(23) <= 65536 < sb_bytes(24)


def test_every_kernel_name_is_expected_by_a_case():
    assert {n for _, _, _, kernels, _ in TABLE for n in kernels} == NAMES


def test_post_plan_subsample(lib):
    """step = ceil(n / cap) above the cap, m = ceil(n / step), tail = round-half-even(0.02 (m - 1)) + 1 within [1, m]."""
    for (h, w), want in {(294, 518): (25, 6092, 123), (64, 96): (1, 6144, 124), (3, 3): (1, 9, 1), (65, 96): (2, 3120, 63)}.items():
        p = plan(h=h, w=w)
        assert (p["step"], p["m"], p["tail"]) == want, (h, w, p)
        n = h * w
        step = -(-n // 6144) if n > 6144 else 1
        m = -(-n // step)
        assert (step, m, min(m, max(1, round(0.02 * (m - 1)) + 1))) == want
    # metric parameters: the host's values for h * w valid pixels (the kernel derives its own from the data)
    assert [plan(h=294, w=518, metric=True)[f] for f in ("step", "m", "tail")] == [25, 6092, 123]
    assert plan(h=64, w=96, percentile=100.0)["tail"] == 6144 and plan(h=64, w=96, percentile=0.0)["tail"] == 1


def test_post_plan_refusals(lib):
    pp = ops.post_params(PipelineParams())
    r = _lib.PostPlanResult()
    r.struct_size = 8                                                                          # a short struct is refused
    assert lib.d2s_post_plan(1, 294, 518, C.byref(pp), 0, C.byref(r)) == 1 and b"struct_size" in lib.d2s_last_error()
    r.struct_size = C.sizeof(_lib.PostPlanResult)
    assert C.sizeof(_lib.PostPlanResult) == 140 and _lib.PostPlanResult.lds_bytes.offset == 32 and _lib.PostPlanResult.kernel.offset == 44
    assert lib.d2s_post_plan(1, 294, 518, C.byref(pp), 0, C.byref(r)) == 0
    for kw, msg in ((dict(aa_strength=21.4), b"aa_strength too large"), (dict(subsample_cap=8193), b"subsample_cap must be <= 8192"),
                    (dict(subsample_cap=0), b"subsample_cap"), (dict(foreground_scale=-1.0), b"scale must be greater than -1.0")):
        bad = ops.post_params(dataclasses.replace(PipelineParams(), **kw))
        assert lib.d2s_post_plan(1, 294, 518, C.byref(bad), 0, C.byref(r)) == 1 and msg in lib.d2s_last_error(), kw
    assert plan(aa_strength=21.3)["k"] == 63                                                   # the largest the kernels take
    assert lib.d2s_post_plan(0, 294, 518, C.byref(pp), 0, C.byref(r)) == 1 and b"bad shape" in lib.d2s_last_error()
    assert lib.d2s_post_plan(1, 294, 518, None, 0, C.byref(r)) == 1 and b"null pointer" in lib.d2s_last_error()
