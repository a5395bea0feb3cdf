"""Golden vectors for the OpenXR viewer's movie-crop detector: the REFERENCE's own xr_viewer/crop.py (CropMixin), loaded by path
at generation time and run on CPU torch -- its tensor path, the one a ROCm capture takes.

    python tests/golden/make_golden_crop_detect.py        # -> tests/golden/crop_detect.npz + crop_detect.json

Per case: the six numbers of stats_t (crop.py:413; caught by wrapping _movie_crop_from_stats), the crop rectangle
_detect_movie_letterbox_crop(tensor, True, w, h) returns, _movie_crop_pixel_bounds of it, and the sample plan's integers.  Plus a
scripted _apply_movie_crop_detection sequence (the hysteresis), _set_manual_crop_uv, and _movie_crop_pixel_bounds on crops whose
edges fall on half pixels (round() is half-to-even).  Frames are regenerated from seeds (desktop2stereo_amd.synth.letterbox_frame);
nothing of the reference's text is kept.

CONDITION, asserted here in float64: every sampled line's unbiased luma std lies outside [4, 8] (the reference's threshold is 6) and
center_mean / center_bright are not within 10 % of 14.0 / 0.035 -- so the reference alone is unambiguous on every case and a float32
detector that sums in another order must give the same integers.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF_CROP = "/root/reference/xr_viewer/crop.py"

# (name, h, w, seed, letterbox_frame keywords)
CASES = [
    ("s64_black", 64, 64, 1, dict(top=10, bottom=10)),                                   # 51 samples per line: a partial wave
    ("s64_noisy_lr", 64, 64, 19, dict(left=10, right=11, bar="noisy")),
    ("s64_full", 64, 64, 3, dict()),
    ("s96_noisy", 96, 160, 21, dict(top=16, bottom=16, bar="noisy")),                     # stride 1
    ("s96_full", 96, 160, 5, dict()),
    ("s96_both_solid", 96, 160, 6, dict(top=14, bottom=13, left=20, right=20, bar="solid")),
    ("m731_solid_lr", 400, 731, 7, dict(left=60, right=62, bar="solid")),                # stride 2 / 3, last row AND column appended
    ("m731_gradient", 400, 731, 8, dict(top=50, bottom=50, bar="gradient")),             # a bar that is not uniform: nothing found
    ("m731_black", 400, 731, 9, dict(top=48, bottom=52)),
    ("m730_both", 400, 730, 10, dict(top=40, bottom=40, left=70, right=70)),             # last column NOT appended
    ("m730_under_min_bar", 400, 730, 11, dict(top=10, bottom=10)),                       # min_bar = 14
    ("m730_noisy_lr", 400, 730, 12, dict(left=90, right=80, bar="noisy")),
    ("hd_239", 1080, 1920, 13, dict(top=138, bottom=139)),                               # a 2.39:1 film
    ("hd_asymmetric", 1080, 1920, 14, dict(top=60, bottom=200)),                         # refused by the asymmetry test
    ("hd_dark_centre", 1080, 1920, 15, dict(top=138, bottom=139, dark_centre=True)),     # fails the centre vote
    ("hd_noisy_43", 1080, 1920, 16, dict(left=240, right=240, bar="noisy")),             # a 4:3 picture
    ("hd_full", 1080, 1920, 17, dict()),
]


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_xr_crop", REF_CROP)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Viewer(mod.CropMixin):
        pass
    return Viewer


def check_condition(name, img, plan):
    """float64: no sampled line within [4, 8] of std; the centre vote not within 10 % of its thresholds."""
    a = img.astype(np.float64)
    luma = a[..., 0] * 0.2126 + a[..., 1] * 0.7152 + a[..., 2] * 0.0722
    rows = luma[plan["y_rows"]][:, plan["x0"]:plan["x1"]:plan["step_x"]]
    cols = luma[plan["y0_col"]:plan["y1_col"]:plan["step_y"]][:, plan["x_cols"]]
    rs, cs = rows.std(axis=1, ddof=1), cols.std(axis=0, ddof=1)
    assert not ((rs >= 4.0) & (rs <= 8.0)).any(), (name, "row std in [4, 8]", rs[(rs >= 4) & (rs <= 8)])
    assert not ((cs >= 4.0) & (cs <= 8.0)).any(), (name, "column std in [4, 8]", cs[(cs >= 4) & (cs <= 8)])
    m = np.asarray(plan["center_mask_np"])
    cm, cb = rows.mean(axis=1)[m].mean(), (rows > 20.0).mean(axis=1)[m].mean()
    assert abs(cm - 14.0) > 1.4 and abs(cb - 0.035) > 0.0035, (name, cm, cb)
    return rs, cs


def main():
    import torch
    from desktop2stereo_amd import synth
    Viewer = load_reference()
    data, meta = {}, {"cases": [], "reference": "xr_viewer/crop.py: _detect_movie_letterbox_crop(tensor, True, w, h) on CPU torch "
                                                 f"{torch.__version__}; stats = stats_t (:413) as _movie_crop_from_stats receives it",
                      "stats": "<case>_stats float64 [6] = (top_i, bottom_count, center_mean, center_bright, left_i, right_count)"}
    crops = {}
    for name, h, w, seed, kw in CASES:
        img = synth.letterbox_frame(h, w, seed, **kw)
        v = Viewer()
        v._reset_movie_crop()
        seen = {}
        orig = v._movie_crop_from_stats

        def wrapped(stats, y_rows, ww, hh, _orig=orig, _seen=seen):
            _seen["stats"] = [float(s) for s in stats]
            return _orig(stats, y_rows, ww, hh)
        v._movie_crop_from_stats = wrapped
        t = torch.from_numpy(img).permute(2, 0, 1).contiguous()                      # the reference's capture tensor is CHW
        crop = tuple(float(c) for c in v._detect_movie_letterbox_crop(t, True, w, h))
        crop_np = tuple(float(c) for c in Viewer()._detect_movie_letterbox_crop(img, False, w, h))
        assert crop == crop_np, (name, crop, crop_np)                                 # its numpy path agrees
        plan = v._movie_crop_sample_plan(w, h)
        rs, cs = check_condition(name, img, plan)
        data[f"{name}_stats"] = np.asarray(seen["stats"], np.float64)
        data[f"{name}_y_rows"] = np.asarray(plan["y_rows"], np.int32)
        data[f"{name}_x_cols"] = np.asarray(plan["x_cols"], np.int32)
        crops[name] = crop
        meta["cases"].append(dict(name=name, h=h, w=w, seed=seed, frame=kw, crop=list(crop),
                                  pixel_bounds=[int(b) for b in v._movie_crop_pixel_bounds(w, h, crop)],
                                  plan={k: int(plan[k]) for k in ("x0", "x1", "step_x", "y0_col", "y1_col", "step_y")},
                                  center_rows=int(np.sum(plan["center_mask_np"])),
                                  line_std_range=[float(min(rs.min(), cs.min())), float(max(rs.max(), cs.max()))]))
        print(name, seen["stats"], crop)
    # the hysteresis (_apply_movie_crop_detection, :202-216): the state after every step of a scripted sequence
    a, h = crops["hd_239"], 1080
    near = (a[0], a[1] + 1.0 / h, a[2], a[3] - 1.0 / h)             # moves by less than 2 / h: not a new target
    far = (a[0], a[1] + 2.0 / h, a[2], a[3] - 4.0 / h)              # moves by 2 / h or more
    full = (0.0, 0.0, 1.0, 1.0)
    script = [full, a, near, far, full, full, a, full, full, full, full, crops["hd_noisy_43"], near, full]
    v = Viewer()
    v._reset_movie_crop()
    steps = []
    for det in script:
        v._apply_movie_crop_detection(det, h)
        steps.append(dict(detected=list(det), target_uv=list(v._movie_crop_target_uv), target_active=bool(v._movie_crop_target_active),
                          full_hits=int(v._movie_crop_full_hits)))
    meta["hysteresis"] = dict(h=h, steps=steps)
    meta["manual"] = [dict(w=mw, h=mh, crop=list(Viewer()._set_manual_crop_uv(mw, mh)))
                      for mw, mh in ((1.0, 0.75), (0.8, 1.0), (1.2, -0.1), (0.5, 0.5))]
    # half-pixel edges (exactly representable products): Python's round() is half-to-even
    meta["pixel_bounds"] = [dict(w=bw, h=bh, crop=list(c), bounds=[int(b) for b in Viewer()._movie_crop_pixel_bounds(bw, bh, c)])
                            for bw, bh, c in ((128, 64, (2.5 / 128, 1.5 / 64, 100.0 / 128, 60.0 / 64)),
                                              (128, 64, (3.5 / 128, 2.5 / 64, 100.0 / 128, 50.0 / 64)),
                                              (128, 64, (0.0, 0.0, 1.0, 1.0)), (128, 64, (0.999, 0.999, 0.001, 0.001)),
                                              (1920, 1080, crops["hd_239"]), (730, 400, crops["m730_both"]))]
    np.savez_compressed(os.path.join(HERE, "crop_detect.npz"), **data)
    with open(os.path.join(HERE, "crop_detect.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote crop_detect", len(data), "arrays")


if __name__ == "__main__":
    main()
