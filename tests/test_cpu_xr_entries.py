"""CPU: the rules of the seven OpenXR eye-view entries as a whole (csrc/dibr_xr.h xr_plan; the table in DESIGN.md, "The eye views'
plan") -- host code, no GPU.  test_cpu_xr_plan.py's matrix knows the first three entries; here every cell an entry's argument list can express is
asked: two screens (flat, curve="horizontal"), the five looks (none, glow, glow2, veil, frosted) the entry takes, and for the two
panorama entries no panorama or one.  66 cells.  Per cell the plan door's kind, rows per eye, set-up launches, grid, LDS bytes, workspace
bytes and `reserved`, or its refusal; and the entry itself, called with NULL for rgb, depth, out, workspace, levels, pano_rgb and
pano_levels so that it can launch nothing: a refused cell gives the door's code and text, an accepted one the workspace's NULL message."""
import ctypes as C
import os

import pytest

from desktop2stereo_amd import _lib, ops, xr

F32 = _lib.FMT_F32_HWC
INVALID, UNSUPPORTED = 1, 5
FOV = ((-0.75, 0.60, 0.55, -0.60), (-0.60, 0.75, 0.55, -0.60))

# kind, flat or curved screen: (rows per eye, set-up launches, grid, dynamic LDS, static LDS, workspace bytes) of a 96 x 160 frame and two
# 130 x 100 eyes.  The glow's 12 bytes: the frame's chain ends in ONE texel at level 7.  5788 = (52 * 25 + 49 * 3) * 4.
KINDS = {("plain", False): (1, 2, (9, 7, 2), 0, 0, 9216), ("plain", True): (48, 4, (9, 7, 2), 0, 0, 9216),
         ("glow", False): (1, 2, (9, 7, 2), 12, 0, 9216), ("glow_curved", True): (52, 6, (9, 7, 2), 12, 5788, 9984),
         ("frost", False): (5, 2, (9, 7, 2), 0, 0, 9984), ("frost_curved", True): (244, 22, (3, 2, 2), 0, 32, 46848)}
LOOKS = {"glow": ("glow", xr.XrGlow("glow", 10.0)), "glow2": ("glow", xr.XrGlow("glow2", 10.0)),
         "veil": ("frost", xr.XrFrost("veil")), "frosted": ("frost", xr.XrFrost("frosted"))}
NO_CURVED_GLOW = (UNSUPPORTED, b"the glow of a curved screen")
NO_CURVED_FROST = (UNSUPPORTED, b"the frost and veil of a curved screen")
NO_CURVED_PANO = (UNSUPPORTED, b"a panorama behind the glow, veil or frosted look")
ALL = (None, "glow", "glow2", "veil", "frosted")
# entry: (the C entry, the looks its argument list takes, its answer to a curved screen's glow, to a curved screen's veil or frosted
# look (None: draws it), whether it takes a panorama, its answer to a curved screen's look over one)
ENTRIES = {"eyes": ("d2s_dibr_xr_eyes", (None,), None, None, False, None),
           "glow": ("d2s_dibr_xr_eyes_glow", (None, "glow", "glow2"), NO_CURVED_GLOW, None, False, None),
           "glow_curved": ("d2s_dibr_xr_eyes_glow_curved", (None, "glow", "glow2"), None, None, False, None),
           "frost": ("d2s_dibr_xr_eyes_frost", (None, "veil", "frosted"), None, NO_CURVED_FROST, False, None),
           "frost_curved": ("d2s_dibr_xr_eyes_frost_curved", (None, "veil", "frosted"), None, None, False, None),
           "panorama": ("d2s_dibr_xr_eyes_panorama", ALL, None, None, True, NO_CURVED_PANO),
           "panorama_curved": ("d2s_dibr_xr_eyes_panorama_curved", ALL, None, None, True, None)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def _pv(eye):
    return xr.fov_to_proj_mat4(*FOV[eye]), xr.pose_to_view_mat4((0, 0, 0, 1), (-0.032 if eye == 0 else 0.032, 0, 0))


def _vp(eye=0):
    proj, view = _pv(eye)
    return proj @ view


def _expected(entry, curved, look, pano):
    """The kind the cell draws, or (code, words) of its refusal."""
    _, _, curved_glow, curved_frost, _, curved_pano = ENTRIES[entry]
    if look is None:
        return "plain"
    family = LOOKS[look][0]
    if not curved:
        return family
    refusal = curved_glow if family == "glow" else curved_frost
    if refusal is None and pano:
        refusal = curved_pano
    return refusal if refusal is not None else family + "_curved"


def _cells():
    for entry, (_, looks, _, _, takes_pano, _) in ENTRIES.items():
        for curved in (False, True):
            for look in looks:
                for pano in ((False, True) if takes_pano else (False,)):
                    yield entry, curved, look, pano


def test_the_cells_are_every_one_an_argument_list_can_express():
    assert len(list(_cells())) == 66


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_cell_of_the_entry(lib, entry):
    dp = ops.dibr_params()
    eyes = xr.eye_array([xr.xr_eye(_vp(i), 130, 100, i) for i in range(2)])
    pano_struct = xr.XrPanorama().c_struct([_pv(i) for i in range(2)], (512, 1024))
    fn, _, _, _, takes_pano, _ = ENTRIES[entry]
    for e, curved, look, pano in _cells():
        if e != entry:
            continue
        what = f"{entry}, {'curved' if curved else 'flat'}, {look}, {'panorama' if pano else 'no panorama'}"
        sc = xr.XrScreen(width=1.6, height=0.96, distance=1.5, curve="horizontal" if curved else "flat").c_struct()
        front = (24, 40, 1, 96, 160, C.byref(dp), None, C.byref(sc), eyes, 2)
        glow = LOOKS[look][1].c_struct() if look and LOOKS[look][0] == "glow" else None
        frost = LOOKS[look][1].c_struct() if look and LOOKS[look][0] == "frost" else None
        g, f, p = (C.byref(glow) if glow else None), (C.byref(frost) if frost else None), (C.byref(pano_struct) if pano else None)
        r = _lib.XrPlanResult()
        r.struct_size = C.sizeof(_lib.XrPlanResult)
        # the plan door and the entry's tail between workspace_bytes and the stream, every device pointer NULL
        if entry in _lib.XR_ENTRY:
            rc = lib.d2s_dibr_xr_plan(_lib.XR_ENTRY[entry], *front, F32, g, C.byref(r))
            tail = () if entry == "eyes" else (g, None)
        elif takes_pano:
            rc = getattr(lib, f"d2s_dibr_xr_{entry}_plan")(*front, F32, f, g, p, C.byref(r))
            tail = (f, None, g, p, None, None)
        else:
            rc = getattr(lib, f"d2s_dibr_xr_{entry}_plan")(*front, F32, f, C.byref(r))
            tail = (f, None)
        door = lib.d2s_last_error() if rc else b""
        rc_entry = getattr(lib, fn)(None, None, *front, None, F32, None, 0, *tail, None)
        said = lib.d2s_last_error()
        want = _expected(entry, curved, look, pano)
        if isinstance(want, tuple):
            assert (rc, want[1] in door) == (want[0], True), (what, rc, door)
            assert (rc_entry, said) == (rc, door), (what, rc_entry, said)
            continue
        assert rc == 0, (what, rc, door)
        got = (r.rows_per_eye, r.setup_launches, tuple(r.grid), r.lds_dynamic_bytes, r.lds_static_bytes, r.workspace_bytes)
        assert (_lib.XR_KIND[r.kind], got) == (want, KINDS[(want, curved)]), what
        assert r.reserved == (1 if pano else 0), what
        assert rc_entry == INVALID and said == b"invalid argument: null pointer (workspace)", (what, rc_entry, said)
