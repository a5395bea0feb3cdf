"""CPU: the float64 reference and judge of the composite display modes (tests/composite_f64_ref.py) hold on their own.

  * For every case and mode test_gpu_composite_f64.py runs, the reference alone meets the condition on its classes (exempt pixels
    <= 0.1 % and <= 8, decided + branch-judged >= 99 %); the tie-free cases have no undecided pixel at all.
  * The judge accepts the float32 restatement tests/composite_ref.py, unmodified, on every FullDep case, and a float32 emulation in the
    kernels' forms in float32 and u8 and all three alpha modes.
  * Through ops.dibr_composite_plan (host code) every case names its kernel, (rows, cols), both output formats and an LDS request
    <= 65 536 bytes, and every mode meets every kernel family.
  * The judge rejects twenty-four deliberate errors applied to that emulation, each on the cases named in MUTANT_CASES, and accepts
    the two listed "errors" that are none (the feather is symmetric under fv <-> 1 - fv: composite_f64_ref.py's docstring).
"""
import os

import numpy as np
import pytest

import composite_f64_ref as Q
import dibr_ref as R
from composite_ref import composite
from desktop2stereo_amd import ops

_REF = {}
ALPHAS = ("window", "premultiplied", "rgba")
TIE_FREE = ("res", "sr0")


@pytest.fixture(scope="module", autouse=True)
def lib():
    from desktop2stereo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def case_of(name):
    return Q.CASES.get(name) or Q.DM_CASES[name]


def ref_of(name, mode):
    if (name, mode) not in _REF:
        c = case_of(name)
        if name not in _REF:
            _REF[name] = Q.case_inputs(c)
        rgb, dep = _REF[name]
        _REF[name, mode] = (c, rgb, dep, Q.reference(c, mode, rgb, dep))
    return _REF[name, mode]


def plan_of(c, mode, **kw):
    return ops.dibr_composite_plan(c["dhw"][0], c["dhw"][1], c["batch"], c["H"], c["W"], ops.dibr_params(**c["kw"]), mode, **kw)


PAIRS = [(n, m) for n, c in Q.CASES.items() for m in c["modes"]]


@pytest.mark.parametrize("name,mode", PAIRS + [(n, "Depth Map") for n in Q.DM_CASES])
def test_reference_condition_and_emulation(name, mode):
    c, rgb, dep, ref = ref_of(name, mode)
    for alpha in ALPHAS:
        for u8 in (False, True):
            j = R.judge(ref, Q.emulate(c, mode, rgb, dep, alpha, u8), alpha, u8)
            assert j["ok"], (name, mode, alpha, u8, j["nbad"], j["bad"])
    print(f"[composite f64, {name}, {mode}] {j['n']} pixels: decided {j['decided']}, branch-judged {j['branch']}, exempt {j['exempt']}")
    assert R.condition(j), (name, mode, j)
    if name in TIE_FREE:
        assert j["decided"] == j["n"], (name, mode, j)
    if name == "dm_black":                     # texels at 1.125 and an ulp below are undecided on total > 0; above: decided, black; 1.12: decided, red
        cls, hi = ref["cls"][0], ref["hi"][0, 0]
        assert (cls[2:4, 10:14] == 1).all() and (cls[5:7, 20:24] == 1).all() and (cls[5:7, 30:34] == 0).all() and j["exempt"] == 0
        assert ((hi[..., :3].max(-1) == 0) & (cls == 0)).sum() > 8 and (ref["lo"][0, 0, 5:7, 30:34, 0] > 250).all()      # 0.988 * 255 = 251.94


@pytest.mark.parametrize("name,mode", [(n, m) for n, m in PAIRS if Q.CASES[n]["dhw"] == (Q.CASES[n]["H"], Q.CASES[n]["W"])]
                         + [(n, "Depth Map") for n, c in Q.DM_CASES.items() if c["dhw"] == (c["H"], c["W"])])
def test_judge_accepts_the_float32_restatement(name, mode):
    c, rgb, dep, ref = ref_of(name, mode)
    p = dict(R.DEFAULTS, **c["kw"])
    kw = dict(ipd_uv=p["ipd_uv"], depth_ratio=p["depth_ratio"], convergence=p["convergence"], roll=p["roll"], search_radius=p["search_radius"],
              tol=p["depth_tolerance"], blur=p["blur_radius"], feather=p["feather"], feather_width=p["feather_width"],
              corner_radius=p["corner_radius"], viewport=c["vp"] if any(c["vp"]) else None)
    if p["resolution"][0] > 0:
        kw["res"] = p["resolution"]
    got = np.stack([composite(rgb[b], dep[b], mode, alpha="rgba", **kw) for b in range(c["batch"])])
    j = R.judge(ref, got, "rgba", False)
    assert j["ok"], (name, mode, j["nbad"], j["bad"])


def test_cases_name_the_kernels_they_were_built_for():
    """what test_gpu_composite_f64.py asserts before it runs a case, checked here without a GPU"""
    met = {m: set() for m in Q.WARP_MODES}
    for name, c in Q.CASES.items():
        for mode in c["modes"]:
            for u8 in (True, False):
                pl = plan_of(c, mode, out_u8=u8)
                assert pl["kernel"] == Q.kernel_name(c, mode, u8) and pl["lds_bytes"] <= 65536, (name, mode, pl)
                kind, cols = c["expect"]
                assert pl["rows"] == (kind == "rows") and (not pl["rows"] or pl["cols"] == cols), (name, mode, pl)
                assert pl["roll0"] == (kind != "general") and pl["block"] == 256
                if pl["rows"]:
                    assert pl["lds_dynamic"] == 32 * pl["WW"] and pl["lds_static"] == 4 * pl["cols"] + 4 and pl["WW"] <= 1536, pl
                    assert pl["grid"] == (-(-pl["out_w"] // pl["cols"]), pl["out_h"], c["batch"]), pl
                else:
                    assert pl["lds_bytes"] == 0 and pl["grid"] == (-(-pl["out_w"] // 256), pl["out_h"], c["batch"]), pl
            met[mode].add(Q.family(c))
    for mode in Q.WARP_MODES:
        assert met[mode] == set(Q.FAMILIES), (mode, met[mode])
    assert len(Q.CASES) == 23 and all(len(Q.CASES[n]["modes"]) == 3 for n in Q.ALL3)
    assert plan_of(Q.CASES["down2x"], "Anaglyph")["grid"][0] == 3 and plan_of(Q.CASES["fits1534"], "Interleaved")["WW"] == 1534
    assert plan_of(Q.CASES["over1564"], "Interleaved")["WW"] == 1564
    for name, c in Q.DM_CASES.items():
        for u8 in (True, False):
            for alpha, nch in (("window", 3), ("rgba", 4)):
                for align, vec in ((0, True), (1 if u8 else 4, False)):
                    pl = ops.dibr_composite_plan(c["dhw"][0], c["dhw"][1], c["batch"], c["H"], c["W"], ops.dibr_params(alpha=alpha, **c["kw"]),
                                                 "Depth Map", out_u8=u8, out_align=align)
                    assert pl["kernel"] == Q.dm_kernel_name(c, u8, nch, vec) and pl["vec"] == vec and not pl["rows"] and pl["lds_bytes"] == 0, pl
                    assert pl["grid"] == (-(-c["batch"] * pl["out_h"] * pl["out_w"] // 1024), 1, 1), pl


MUTANT_CASES = {   # mutant -> [(case, mode)]
    "tap_off_one": [("full530", m) for m in Q.WARP_MODES], "repeat_clamp": [("full530", "Anaglyph"), ("tiny", "Interleaved-V"), ("parallax", "Interleaved-V")],
    "parity_no_origin": [("up2x", "Interleaved"), ("up2x", "Interleaved-V")], "parity_output_row": [("full530", "Interleaved")],
    "eyes_swapped": [("full530", m) for m in Q.WARP_MODES], "sweep_other_program": [("full530", "Interleaved"), ("full530", "Interleaved-V"), ("roll03", "Interleaved-V")],
    "ana_f1_shaping": [("full530", "Anaglyph"), ("roll03", "Anaglyph")], "ana_channels": [("full530", "Anaglyph"), ("over1564", "Anaglyph")],
    "ana_jump_006": [("up2x", "Anaglyph"), ("roll03", "Anaglyph"), ("up5x19", "Anaglyph")], "conf_edges_f1": [("full530", "Interleaved"), ("up2x", "Interleaved-V")],
    "inpaint_mixed": [("up2x", "Interleaved"), ("up2x", "Interleaved-V"), ("roll03", "Interleaved"), ("up5x19", "Interleaved-V")], "edge_margin_005": [("full530", m) for m in Q.WARP_MODES],
    "ana_border_001": [("full530", "Anaglyph"), ("dscale4", "Anaglyph")], "feather_no_origin": [("fxvp", m) for m in Q.WARP_MODES] + [("roll12fx", "Anaglyph")],
    "no_premult": [("fxvp", m) for m in Q.WARP_MODES], "updep_align_corners": [("up5x19", m) for m in Q.WARP_MODES] + [("dm_up", "Depth Map")],
    "u8_trunc": [("full530", m) for m in Q.WARP_MODES] + [("smooth", "Anaglyph"), ("dm_odd", "Depth Map")],
    "corner_pixel": [("full530", m) for m in Q.WARP_MODES] + [("tiny", "Interleaved-V")], "wrong_row": [("rows270", "Interleaved")],
    "win_neighbour": [("winedge", "Interleaved")], "wx0_tpc1": [("up2x", m) for m in Q.WARP_MODES] + [("down2x", "Anaglyph")],
    "dm_no_norm": [("dm_black", "Depth Map"), ("dm_odd", "Depth Map")], "dm_straddle": [("dm_odd_b3", "Depth Map")], "dm_tail_dropped": [("dm_odd", "Depth Map")]}


def test_every_mutant_is_listed():
    assert set(MUTANT_CASES) == set(Q.MUTANTS) and len(Q.MUTANTS) == 24
    for v in MUTANT_CASES.values():
        for n, m in v:
            assert m == "Depth Map" or m in Q.CASES[n]["modes"], (n, m)


def _mutant_judgement(mut, name, mode):
    c, rgb, dep, ref = ref_of(name, mode)
    alpha = "premultiplied" if mut == "no_premult" else "rgba"
    u8 = mut == "u8_trunc"
    plan = plan_of(c, mode)
    return R.judge(ref, Q.emulate(c, mode, rgb, dep, alpha, u8, mut, plan), alpha, u8)


@pytest.mark.parametrize("mut", list(Q.MUTANTS))
def test_judge_rejects(mut):
    for name, mode in MUTANT_CASES[mut]:
        j = _mutant_judgement(mut, name, mode)
        assert not j["ok"] and j["nbad"] >= 1, (mut, name, mode)
        print(f"[composite f64 mutant {mut}, {name}, {mode}] {j['nbad']} pixels rejected")


@pytest.mark.parametrize("mut", list(Q.EQUIVALENT))
def test_two_listed_errors_are_the_same_picture(mut):
    """u_viewport is the output rectangle: fu == u, fv == 1 - v, and the feather and the corner SDF are symmetric in fv <-> 1 - fv"""
    for name, mode in [("fxvp", m) for m in Q.WARP_MODES] + [("roll12fx", "Anaglyph"), ("fx530", "Interleaved-V")]:
        j = _mutant_judgement(mut, name, mode)
        assert j["ok"], (mut, name, mode, j["nbad"], j["bad"])
