"""CPU: the eye views' plan (include/d2s.h d2s_version() >= 123: d2s_dibr_xr_plan, ops.dibr_xr_plan; csrc/dibr_xr.h xr_plan, DESIGN.md
3.4.3) -- host code, no GPU.

  * the plan matrix: the three kinds, one and two eyes, eyes of different sizes, the three alpha modes, two frame sizes: rows per eye,
    set-up launches, grid, LDS bytes, workspace bytes against the size queries, the out layout against ops.dibr_xr_shape;
  * every refusal d2s.h names for d2s_dibr_xr_eyes, d2s_dibr_xr_eyes_glow and d2s_dibr_xr_eyes_glow_curved that needs no device
    pointer: the query and the entry -- called with NULL for rgb, depth, out, workspace and levels, so it can launch nothing --
    return the same code and the same d2s_last_error text;
  * what is left to the entries, in its order: the workspace (NULL, misaligned, short, named after the kind's size query), levels,
    then rgb / depth / out.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from desktop2stereo_amd import _lib, ops, xr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned pointer that a refused call never touches
F32, U8 = _lib.FMT_F32_HWC, _lib.FMT_U8_HWC
INVALID, UNSUPPORTED = 1, 5
ENTRIES = ("eyes", "glow", "glow_curved")
ENTRY_FN = {"eyes": "d2s_dibr_xr_eyes", "glow": "d2s_dibr_xr_eyes_glow", "glow_curved": "d2s_dibr_xr_eyes_glow_curved"}
FOV = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))
CURVED_LDS = (52 * 25 + 49 * 3) * 4          # the curved glow's kernel: 52 rows padded to 25 floats, 49 seams of 3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def _vp(eye=0):
    return xr.fov_to_proj_mat4(*FOV[eye]) @ xr.pose_to_view_mat4((0, 0, 0, 1), (-0.032 if eye == 0 else 0.032, 0, 0))


def _eyes(n=2, w=130, h=100, **kw):
    return xr.eye_array([xr.xr_eye(kw.get("vp", _vp(i)), w, h, i) for i in range(n)])


def _screen(**kw):
    return xr.XrScreen(**dict(dict(width=1.6, height=0.96, distance=1.5), **kw)).c_struct()


def _glow(*a):
    return xr.XrGlow(*a).c_struct()


def _args(**kw):
    """The arguments of the three entries that are no device pointers: a 96 x 160 frame, 24 x 40 depth, two 130 x 100 eyes."""
    a = dict(dp=ops.dibr_params(), screen=_screen(), eyes=_eyes(), n_eyes=None, crop=None, dh=24, dw=40, batch=1, H=96, W=160, fmt=F32, glow=None)
    a.update(kw)
    return a


def _front(a):
    n = len(a["eyes"]) if a["n_eyes"] is None else a["n_eyes"]
    return (a["dh"], a["dw"], a["batch"], a["H"], a["W"], C.byref(a["dp"]) if a["dp"] is not None else None, a["crop"],
            C.byref(a["screen"]) if a["screen"] is not None else None, a["eyes"], n)


def _plan(lib, entry, a):
    r = _lib.XrPlanResult()
    r.struct_size = C.sizeof(_lib.XrPlanResult)
    g = a["glow"] if entry != "eyes" else None
    rc = lib.d2s_dibr_xr_plan(_lib.XR_ENTRY[entry], *_front(a), a["fmt"], C.byref(g) if g is not None else None, C.byref(r))
    return rc, lib.d2s_last_error() if rc else b"", r


def _entry(lib, entry, a, rgb=None, depth=None, out=None, ws=None, ws_bytes=0, levels=None):
    f = _front(a)
    tail = () if entry == "eyes" else (C.byref(a["glow"]) if a["glow"] is not None else None, levels)
    rc = getattr(lib, ENTRY_FN[entry])(rgb, depth, *f, out, a["fmt"], ws, ws_bytes, *tail, None)
    return rc, lib.d2s_last_error() if rc else b""


def _chain_bytes(H, W):
    levels, _ = ops.mip_shape(H, W)                       # levels 1 .. q
    q = len(levels)
    return 12 * sum(h * w for _, h, w in levels[min(7, q) - 1:])


def test_symbol_struct_and_version(lib):
    assert lib.d2s_version() >= 123
    hdr = open(os.path.join(REPO, "include", "d2s.h")).read()
    assert "d2s_dibr_xr_plan" in _lib.SYMBOLS and "int d2s_dibr_xr_plan(" in hdr and "d2s_version() >= 123" in hdr
    assert C.sizeof(_lib.XrPlanResult) == 72 and _lib.XrPlanResult.struct_size.offset == 0 and _lib.XrPlanResult.workspace_bytes.offset == 40
    a = _args()
    r = _lib.XrPlanResult()
    assert lib.d2s_dibr_xr_plan(0, *_front(a), F32, None, C.byref(r)) == INVALID and b"struct_size" in lib.d2s_last_error()
    assert lib.d2s_dibr_xr_plan(0, *_front(a), F32, None, None) == INVALID and b"res" in lib.d2s_last_error()
    r.struct_size = C.sizeof(r)
    for entry in (-1, 3):
        assert lib.d2s_dibr_xr_plan(entry, *_front(a), F32, None, C.byref(r)) == INVALID and b"entry" in lib.d2s_last_error()
    g = _glow("glow", 10.0)
    assert lib.d2s_dibr_xr_plan(0, *_front(a), F32, C.byref(g), C.byref(r)) == INVALID and b"takes no glow" in lib.d2s_last_error()


# (label, screen keywords, glow or None, the entries that accept the call, kind, rows per eye, set-up launches per eye)
KINDS = (("plain flat", {}, None, ENTRIES, "plain", 1, 1),
         ("plain flat, glow off", {}, ("off", 10.0), ENTRIES[1:], "plain", 1, 1),
         ("plain curved", dict(curve="horizontal"), None, ENTRIES, "plain", 48, 2),
         ("plain curved, glow off", dict(curve="vertical"), ("off", 10.0), ENTRIES[1:], "plain", 48, 2),
         ("flat glow", {}, ("glow", 10.0), ENTRIES[1:], "glow", 1, 1),
         ("flat glow2", {}, ("glow2", 10.0), ENTRIES[1:], "glow", 1, 1),
         ("curved glow h", dict(curve="horizontal"), ("glow", 10.0), ENTRIES[2:], "glow_curved", 52, 3),
         ("curved glow2 h", dict(curve="horizontal"), ("glow2", 10.0), ENTRIES[2:], "glow_curved", 52, 3),
         ("curved glow v", dict(curve="vertical"), ("glow", 10.0), ENTRIES[2:], "glow_curved", 52, 3))
EYE_SETS = (((130, 100),), ((130, 100), (130, 100)), ((34, 20), (18, 18)), ((70, 50), (2064, 2208)))


def test_plan_matrix(lib):
    cdiv = lambda a, b: (a + b - 1) // b
    n = C.c_uint64()
    cases = 0
    for label, skw, glow, entries, kind, rows, launches in KINDS:
        for sizes in EYE_SETS:
            eyes = xr.eye_array([xr.xr_eye(_vp(i), w, h, i) for i, (w, h) in enumerate(sizes)])
            for alpha in ("window", "premultiplied", "rgba"):
                for (H, W, batch, fmt) in ((96, 160, 1, F32), (1080, 1920, 3, U8)):
                    dp = ops.dibr_params(alpha=alpha)
                    a = _args(dp=dp, screen=_screen(**skw), eyes=eyes, glow=_glow(*glow) if glow else None, H=H, W=W, batch=batch, fmt=fmt)
                    for entry in entries:
                        rc, err, r = _plan(lib, entry, a)
                        what = (label, sizes, alpha, H, entry)
                        assert rc == 0, (what, err)
                        assert (_lib.XR_KIND[r.kind], r.rows_per_eye, r.setup_launches) == (kind, rows, launches * len(sizes)), what
                        assert tuple(r.grid) == (cdiv(max(w for w, _ in sizes), 16), cdiv(max(h for _, h in sizes), 16), len(sizes) * batch), what
                        assert r.lds_dynamic_bytes == (0 if kind == "plain" else _chain_bytes(H, W)), what
                        assert r.lds_static_bytes == (CURVED_LDS if kind == "glow_curved" else 0), what
                        query = lib.d2s_dibr_xr_glow_curved_workspace if kind == "glow_curved" else lib.d2s_dibr_xr_workspace
                        assert query(len(sizes), C.byref(n)) == 0 and r.workspace_bytes == n.value, what
                        offs, total = ops.dibr_xr_shape(eyes, batch, dp.alpha_mode)
                        assert (list(r.offsets[:len(sizes)]), r.out_elems) == (offs, total), what
                        cases += 1
    assert cases == (3 * 2 + 2 * 4 + 1 * 3) * len(EYE_SETS) * 3 * 2
    assert _chain_bytes(96, 160) == 12 and _chain_bytes(1080, 1920) == 12 * (8 * 15 + 4 * 7 + 2 * 3 + 1)
    # ops.dibr_xr_plan: the same answer as a dict
    d = ops.dibr_xr_plan("glow_curved", 24, 40, 2, 96, 160, ops.dibr_params(alpha="rgba"), xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve="vertical"),
                         [xr.xr_eye(_vp(0), 34, 20, 0), xr.xr_eye(_vp(1), 18, 18, 1)], glow=xr.XrGlow("glow", 10.0), out_u8=False)
    assert d == dict(kind="glow_curved", rows_per_eye=52, setup_launches=6, grid=(3, 2, 4), lds_dynamic_bytes=12, lds_static_bytes=CURVED_LDS,
                     workspace_bytes=2 * 52 * 96, out_elems=2 * 4 * (34 * 20 + 18 * 18), offsets=[0, 2 * 4 * 34 * 20])
    with pytest.raises(_lib.D2SError, match="curved"):
        ops.dibr_xr_plan("glow", 24, 40, 1, 96, 160, ops.dibr_params(), xr.XrScreen(curve="horizontal"), [xr.xr_eye(_vp(0), 34, 20, 0)],
                         glow=xr.XrGlow("glow", 10.0))


def _defects(golden_dir):
    """(label, entries it applies to, argument overrides, code, a word of the message): every refusal d2s.h names for the three entries
    that needs no device pointer."""
    nan, inf = float("nan"), float("inf")
    crop = lambda *v: (C.c_double * 4)(*v)
    with open(os.path.join(golden_dir, "xr_eye.json")) as f:
        occ = {c["name"]: c for c in json.load(f)["cases"]}["curved_occluded"]          # the arc seen from beyond its end
    occ_eyes = xr.eye_array([xr.xr_eye(np.array(e["vp"]), 130, 100, e["eye"]) for e in occ["eyes"]])
    G, ALL, GLOW, CURVED = _glow("glow", 10.0), ENTRIES, ENTRIES[1:], ENTRIES[2:]
    out = []
    add = lambda label, entries, code, word, **kw: out.append((label, entries, kw, code, word))
    # d2s_dibr_xr_eyes: the uniforms and the frame (everything d2s_dibr_warp_crop refuses), the screen, the eyes
    add("p NULL", ALL, INVALID, b"null pointer", dp=None)
    bad = ops.dibr_params()
    bad.struct_size = 72
    add("d2s_dibr_params.struct_size", ALL, INVALID, b"d2s_dibr_params.struct_size", dp=bad)
    add("batch 0", ALL, INVALID, b"batch", batch=0)
    add("batch 70000", ALL, INVALID, b"batch", batch=70000)
    add("H 1", ALL, INVALID, b"shape", H=1)
    add("frame too large", ALL, INVALID, b"too large", H=30000, W=30000)
    add("dh 0", ALL, INVALID, b"depth shape", dh=0)
    add("out_fmt", ALL, INVALID, b"out_fmt", fmt=_lib.FMT_F32_CHW)
    add("search_radius", ALL, INVALID, b"search_radius", dp=ops.dibr_params(search_radius=16.0))
    add("corner_radius", ALL, INVALID, b"corner_radius", dp=ops.dibr_params(corner_radius=0.6))
    bad = ops.dibr_params()
    bad.alpha_mode = 3
    add("alpha_mode", ALL, INVALID, b"alpha_mode", dp=bad)
    add("feather_enabled", ALL, INVALID, b"feather", dp=ops.dibr_params(feather=True))
    for v in ((nan, 0, 1, 1), (-0.01, 0, 1, 1), (0, 0, 0, 1), (0.5, 0, 0.51, 1), (0, 0, 0.004, 1)):
        add(f"crop {v}", ALL, INVALID, b"crop", crop=crop(*v))
    add("screen NULL", ALL, INVALID, b"null pointer (screen, eyes)", screen=None)
    bad = _screen()
    bad.struct_size = 88
    add("d2s_xr_screen.struct_size", ALL, INVALID, b"d2s_xr_screen.struct_size", screen=bad)
    for n in (0, 3, -2):
        add(f"n_eyes {n}", ALL, INVALID, b"n_eyes", n_eyes=n)
    for c in (-1, 3):
        bad = _screen()
        bad.curve = c
        add(f"curve {c}", ALL, INVALID, b"curve", screen=bad)
    for kw in (dict(width=nan), dict(yaw=inf), dict(normal_offset=-inf), dict(clear=(0, nan, 0, 1))):
        add(f"screen {kw}", ALL, INVALID, b"finite", screen=_screen(**kw))
    for kw in (dict(width=0.0), dict(height=-1.0), dict(distance=0.0)):
        add(f"screen {kw}", ALL, INVALID, b"> 0", screen=_screen(**kw))
    bad = _eyes()
    bad[1].struct_size = 136
    add("d2s_xr_eye.struct_size", ALL, INVALID, b"d2s_xr_eye.struct_size", eyes=bad)
    vp = _vp(0).copy()
    vp[2, 1] = nan
    add("eye vp", ALL, INVALID, b"finite", eyes=_eyes(1, vp=vp))
    for w, h in ((1, 100), (130, 1), (8193, 100), (130, 9000)):
        add(f"eye image {w} x {h}", ALL, INVALID, b"2 .. 8192", eyes=_eyes(w=w, h=h))
    bad = _eyes()
    bad[0].eye = 2
    add("eye 2", ALL, INVALID, b"eye must be", eyes=bad)
    add("n_eyes * batch", ALL, INVALID, b"n_eyes * batch", batch=40000)
    add("clip w, flat", ALL, UNSUPPORTED, b"eye plane", screen=_screen(distance=0.2, yaw=1.2))
    add("clip w, curved", ALL, UNSUPPORTED, b"eye plane", screen=_screen(distance=0.1, curve="horizontal", width=3.0))
    # d2s_dibr_xr_eyes_glow: the glow
    bad = _glow("glow", 10.0)
    bad.struct_size = 16
    add("d2s_xr_glow.struct_size", GLOW, INVALID, b"d2s_xr_glow.struct_size", glow=bad)
    for m in (-1, 3):
        bad = _glow("glow", 10.0)
        bad.mode = m
        add(f"glow mode {m}", GLOW, INVALID, b"glow mode", glow=bad)
    for v in (nan, inf, 0.0, -1.0):
        add(f"range_m {v}", GLOW, INVALID, b"range_m", glow=_glow("glow", v))
    for v in (-0.01, nan):
        add(f"inner_edge_fraction {v}", GLOW, INVALID, b"inner_edge_fraction", glow=_glow("glow2", 10.0, v))
    for mode in ("glow", "glow2"):
        for curve in ("horizontal", "vertical"):
            add(f"curved {curve} {mode}", ("glow",), UNSUPPORTED, b"curved", glow=_glow(mode, 10.0), screen=_screen(curve=curve))
        add(f"normal_offset flat {mode}", GLOW, INVALID, b"normal_offset", glow=_glow(mode, 10.0), screen=_screen(normal_offset=0.01))
        add(f"frame 96 x 8200 {mode}", GLOW, INVALID, b"2 .. 8192", glow=_glow(mode, 10.0), W=8200)
        # d2s_dibr_xr_eyes_glow_curved
        add(f"normal_offset curved {mode}", CURVED, INVALID, b"normal_offset", glow=_glow(mode, 10.0), screen=_screen(curve="vertical", normal_offset=0.01))
        add(f"convex region {mode}", CURVED, UNSUPPORTED, b"convex region", glow=_glow(mode, 10.0), screen=xr.XrScreen(**occ["screen"]).c_struct(), eyes=occ_eyes)
    add("64 KB of LDS", CURVED, UNSUPPORTED, b"64 KB", glow=G, screen=_screen(curve="horizontal"), H=8192, W=8192)
    add("clip w, curved glow", CURVED, UNSUPPORTED, b"eye plane", glow=G, screen=_screen(distance=0.1, curve="horizontal", width=3.0))
    return out


def test_every_refusal_is_the_entrys(lib, golden_dir):
    checked = 0
    for label, entries, kw, code, word in _defects(golden_dir):
        a = _args(**kw)
        for entry in entries:
            if entry == "eyes" and "glow" in kw:
                continue
            prc, perr, _ = _plan(lib, entry, a)
            erc, eerr = _entry(lib, entry, a)
            assert prc == code and word in perr, (label, entry, prc, perr)
            assert (erc, eerr) == (prc, perr), (label, entry, erc, eerr, perr)
            checked += 1
    assert checked > 150
    # a flat screen's 8192 x 8192 frame with glow is no refusal of the flat entry: its chain alone fits
    big = _args(glow=_glow("glow", 10.0), H=8192, W=8192)
    assert _plan(lib, "glow", big)[0] == 0 and _plan(lib, "glow_curved", big)[0] == 0


def test_the_pointers_come_last_in_one_order(lib):
    """What the plan leaves to the entries: workspace NULL, misaligned, short (named after the kind's size query), levels with glow on,
    then rgb / depth / out -- for the flat entries as for the curved one."""
    for entry, a, query, need in (("eyes", _args(), b"d2s_dibr_xr_workspace", 2 * 48 * 96),
                                  ("glow", _args(glow=_glow("glow", 10.0)), b"d2s_dibr_xr_workspace", 2 * 48 * 96),
                                  ("glow_curved", _args(glow=_glow("glow", 10.0)), b"d2s_dibr_xr_workspace", 2 * 48 * 96),
                                  ("glow_curved", _args(glow=_glow("glow2", 10.0), screen=_screen(curve="vertical")),
                                   b"d2s_dibr_xr_glow_curved_workspace", 2 * 52 * 96)):
        rc, _, r = _plan(lib, entry, a)
        assert rc == 0 and r.workspace_bytes == need
        glow_on = a["glow"] is not None and entry != "eyes"
        assert _entry(lib, entry, a) == (INVALID, b"invalid argument: null pointer (workspace)")
        rc, err = _entry(lib, entry, a, ws=C.c_void_p(4100), ws_bytes=1 << 16)
        assert rc == INVALID and b"aligned" in err
        rc, err = _entry(lib, entry, a, ws=FAKE, ws_bytes=need - 1)
        assert rc == INVALID and err.endswith(b"workspace_bytes below " + query), err
        rc, err = _entry(lib, entry, a, ws=FAKE, ws_bytes=need)
        assert rc == INVALID and (b"levels" in err) == glow_on and b"null pointer" in err
        for kw in (dict(depth=FAKE, out=FAKE), dict(rgb=FAKE, out=FAKE), dict(rgb=FAKE, depth=FAKE)):
            assert _entry(lib, entry, a, ws=FAKE, ws_bytes=need, levels=FAKE, **kw) == (INVALID, b"invalid argument: null pointer")
