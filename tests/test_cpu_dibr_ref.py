"""CPU: the float64 reference and judge of the DIBR warp (tests/dibr_ref.py) hold on their own.

  * For every case test_gpu_dibr_f64.py runs, the reference alone meets the condition on its classes (exempt pixels <= 0.1 % and <= 8,
    decided + branch-judged >= 99 %), and a tie-free case has no undecided pixel at all.
  * The judge accepts the float32 restatement oracle/dibr_oracle.py, unmodified, on every case it can express (everything but a crop),
    and a float32 emulation in the kernel's forms (smoothstep_inv, the shared PixTaps with dm and dp exchanged for the right eye, the
    weight tables; crop, UpDep and the u8 store included) in float32 and u8 and all three alpha modes.
  * The judge rejects twenty-one deliberate errors applied to that emulation, each on the cases named in MUTANT_CASES.
"""
import numpy as np
import pytest

import dibr_ref as R
from desktop2stereo_amd import ops
from oracle import dibr_oracle as O

_REF = {}


@pytest.fixture(scope="module", autouse=True)
def lib():
    import os
    from desktop2stereo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def ref_of(name):
    if name not in _REF:
        c = R.CASES[name]
        rgb, dep = R.inputs(c)
        _REF[name] = (c, rgb, dep, R.reference(c, rgb, dep))
    return _REF[name]


def plan_of(c, **kw):
    return ops.dibr_warp_plan(c["dhw"][0], c["dhw"][1], c["batch"], c["H"], c["W"], ops.dibr_params(display_mode=c["mode"], **c["kw"]),
                              crop=c["crop"], **kw)


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_condition_and_emulation(name):
    c, rgb, dep, ref = ref_of(name)
    for alpha in ("window", "premultiplied", "rgba"):
        for u8 in (False, True):
            j = R.judge(ref, R.emulate(c, rgb, dep, alpha, u8), alpha, u8)
            assert j["ok"], (name, alpha, u8, j["nbad"], j["bad"])
    print(f"[dibr f64, {name}] {j['n']} pixels: decided {j['decided']}, branch-judged {j['branch']}, exempt {j['exempt']}")
    assert R.condition(j), (name, j)
    if name in ("sr5_b225", "res", "sr0"):                     # tie-free: blur_radius 2.25, or a resolution that is not the viewport
        assert j["decided"] == j["n"], (name, j)
    if name == "sbs530":                                       # the default parameters: rows 2 and oh - 3 tie on the vertical taps
        cls = ref["cls"][0]
        assert (cls[2] > 0).any() and (cls[c["H"] - 3] > 0).any()


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["crop"] is None])
def test_judge_accepts_the_float32_restatement(name):
    c, rgb, dep, ref = ref_of(name)
    p = dict(R.DEFAULTS, **c["kw"])
    kw = dict(roll=p["roll"], search_radius=p["search_radius"], tol=p["depth_tolerance"], blur=p["blur_radius"], feather=p["feather"],
              feather_width=p["feather_width"], corner_radius=p["corner_radius"])
    if p["resolution"][0] > 0:
        kw["res"] = p["resolution"]
    if p["viewport"][2] > 0:
        kw["viewport"] = p["viewport"]
    got = np.stack([O.dibr_sbs(rgb[b], R.depth_texels(c, dep[b]), p["ipd_uv"], p["depth_ratio"], p["convergence"], c["mode"], alpha="rgba", **kw)
                    for b in range(c["batch"])])
    j = R.judge(ref, got, "rgba", False)
    assert j["ok"], (name, j["nbad"], j["bad"])


KEYS = ("D2S_DIBR_NO_ROLL0", "D2S_DIBR_NO_ROWS", "D2S_DIBR_COLS")


def test_cases_name_the_kernels_they_were_built_for(monkeypatch):
    """what test_gpu_dibr_f64.py asserts before it runs a case, checked here without a GPU"""
    try:
        for name, c in R.CASES.items():
            for spec, want in [(None, c["expect"][0])] + list(c["env"].items()):
                for k in KEYS:
                    monkeypatch.delenv(k, raising=False)
                if spec:
                    monkeypatch.setenv(*spec.split("="))
                ops.reload_env()
                pl = plan_of(c)
                assert pl["kernel"] == want and pl["lds_bytes"] <= 65536, (name, spec, pl)
                assert plan_of(c, out_u8=False)["kernel"] == want.replace("<u8", "<f32")
                if spec is None:
                    assert (pl["rows"], pl["cols"]) == c["expect"][1:], (name, pl)
    finally:
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        ops.reload_env()
    kernels = {c["expect"][0] for c in R.CASES.values()} | {k for c in R.CASES.values() for k in c["env"].values()}
    for k in ("dibr_rows<u8,fx=0,256,FullDep>", "dibr_rows<u8,fx=0,512,FullDep>", "dibr_rows<u8,fx=0,1024,FullDep>", "dibr_rows<u8,fx=1,512,FullDep>",
              "dibr_rows<u8,fx=0,512,UpDep>", "dibr_rows<u8,fx=1,256,FullDep,crop>", "dibr_rows<u8,fx=0,256,UpDep,crop>", "dibr<u8,roll0,FullDep>",
              "dibr<u8,general,FullDep>", "dibr<u8,roll0,UpDep>", "dibr<u8,general,UpDep>", "dibr<u8,roll0,FullDep,crop>"):
        assert k in kernels, k


MUTANT_CASES = {
    "tap_off_one": ("sbs530", "crop1"), "repeat_clamp": ("sbs530", "parallax"), "sweep_other_eye": ("sbs530", "roll03"), "sy_psy": ("roll03",),
    "w1_prev": ("sbs530", "crop0"), "no_break": ("sbs530", "hsbs"), "no_phase2": ("sbs530", "up5x19"), "vblur_psx": ("sbs530", "htab"),
    "vblur_tol": ("sr15_tol",), "no_smooth": ("sbs530", "sr0"), "no_falloff": ("sbs530", "hsbs"), "eyes_swapped": ("sbs530", "ftab"),
    "half_offset": ("htab", "hsbs"), "no_premult": ("parallax", "crop0"), "sdf_on_crop_uv": ("crop0", "crop2"),
    "feather_no_flip": ("fxvp", "roll12fx"), "updep_align_corners": ("up5x19", "crop3"), "u8_trunc": ("sbs530", "smooth"),
    "corner_pixel": ("sbs530", "tiny"), "wrong_row": ("rows270",), "win_neighbour": ("winedge",)}


def test_every_mutant_is_listed():
    assert set(MUTANT_CASES) == set(R.MUTANTS) and len(R.MUTANTS) == 21
    assert all(R.CASES[n]["colors"] == "noise" for v in MUTANT_CASES.values() for n in v[:1])


@pytest.mark.parametrize("mut", list(R.MUTANTS))
def test_judge_rejects(mut):
    for name in MUTANT_CASES[mut]:
        c, rgb, dep, ref = ref_of(name)
        alpha = "premultiplied" if mut == "no_premult" else "rgba"
        u8 = mut == "u8_trunc"
        plan = plan_of(c)
        if mut == "win_neighbour":
            assert plan["rows"], name
        j = R.judge(ref, R.emulate(c, rgb, dep, alpha, u8, mut, plan), alpha, u8)
        assert not j["ok"] and j["nbad"] >= 1, (mut, name)
        print(f"[dibr f64 mutant {mut}, {name}] {j['nbad']} pixels rejected")
