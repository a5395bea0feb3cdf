"""CPU restatement (numpy) of the OpenXR viewer's movie crop.  TEST INFRASTRUCTURE ONLY.

dibr_eye_crop: one eye of the XR screen shader -- FRAGMENT_SHADER.main (viewer.py:533-631) with the one line
_make_xr_fragment_shader changes (xr_viewer/implementation.py:111-126): flipped_uv = u_source_crop.xy + screen_flipped_uv *
u_source_crop.zw.  It is oracle.dibr_oracle.dibr_eye with that line, built on the oracle's _tex / _inpaint / _smoothstep: the depth
taps, the edge fall-off, the shift, the in-painting and the border alpha follow the cropped coordinate; the rounded-corner SDF and
the feathering stay on the quad's uv / u_viewport.  tests/test_cpu_crop.py holds it to renders of the reference's own XR shader
(tests/golden/xr_crop.npz), tests/test_gpu_xr_crop.py holds the HIP kernels to it.

crop_stats: the detector's six numbers (xr_viewer/crop.py:386-413) in float64.
"""
from __future__ import annotations

import numpy as np

from oracle.dibr_oracle import _inpaint, _smoothstep, _tex

F32 = np.float32


def dibr_eye_crop(rgb_u8_hwc, depth, crop, eye_offset, depth_strength, convergence=0.0, out_h=0, out_w=0, roll=0.0, res=None,
                  search_radius=12.0, tol=0.012, blur=2.5, feather=False, feather_width=0.02, corner_radius=0.0, viewport=None):
    """-> frag_color [out_h,out_w,4] float32: rgb 0..255, alpha 0..1, un-multiplied.  crop = (x, y, w, h) in uv, top-left origin."""
    H, W = depth.shape
    oh, ow = out_h or H, out_w or W
    rw, rh = res or (W, H)
    ps = (F32(1) / F32(rw), F32(1) / F32(rh))
    cx, cy, cw, ch = (F32(c) for c in crop)
    rgb = rgb_u8_hwc.astype(F32)
    dep = depth.astype(F32)
    vs, us = np.meshgrid((np.arange(oh, dtype=F32) + F32(0.5)) / F32(oh), (np.arange(ow, dtype=F32) + F32(0.5)) / F32(ow),
                         indexing="ij")
    u, v = (cx + us * cw).astype(F32), (cy + vs * ch).astype(F32)                   # implementation.py:123
    c, s = F32(np.cos(roll)), F32(np.sin(roll))
    sg = F32(np.sign(eye_offset))
    par = (c * sg, s * sg)
    sweep_sign = -1.0 if eye_offset > 0 else 1.0
    dsx, dsy = F32(par[0] * ps[0] * F32(1.5)), F32(par[1] * ps[1] * F32(1.5))
    d0 = _tex(dep, u, v)
    dm = _tex(dep, u - dsx, v - dsy)
    dp = _tex(dep, u + dsx, v + dsy)
    d = (d0 * F32(0.7) + dm * F32(0.15) + dp * F32(0.15)).astype(F32)
    dinv = -d
    shaped = dinv * (F32(1) + F32(0.35) * (F32(1) - d))
    shift = shaped + F32(convergence)
    fall = _smoothstep(0.0, 0.05, u) * _smoothstep(1.0, 0.95, u)                    # on flipped_uv.x: relative to the FULL source
    px = (F32(eye_offset) * shift * F32(depth_strength) * fall).astype(F32)
    su, sv = (u - px * c).astype(F32), (v - px * s).astype(F32)
    oob = (su < 0) | (su > 1) | (sv < 0) | (sv > 1)
    s2x, s2y = F32(par[0] * ps[0] * F32(2)), F32(par[1] * ps[1] * F32(2))
    jump = np.abs(_tex(dep, u - s2x, v - s2y) - _tex(dep, u + s2x, v + s2y))
    conf = np.where(oob, F32(1), _smoothstep(0.04, 0.10, jump)).astype(F32)
    color = _tex(rgb, su, sv)
    m = conf > F32(0.001)
    if m.any():
        filled = _inpaint(rgb, dep, u[m], v[m], dinv[m], par, sweep_sign, ps, search_radius, tol, blur)
        cm = conf[m][:, None]
        color[m] = color[m] * (F32(1) - cm) + filled * cm
    bx = _smoothstep(-0.001, 0.001, su) * _smoothstep(1.001, 0.999, su)
    by = _smoothstep(-0.001, 0.001, sv) * _smoothstep(1.001, 0.999, sv)
    alpha = np.minimum(bx, by)
    if feather:                                                                      # gl_FragCoord / u_viewport: the quad, y up
        vx, vy, vw_, vh_ = viewport if viewport is not None and viewport[2] > 0 else (0.0, 0.0, float(ow), float(oh))
        xs = np.arange(ow, dtype=F32)[None, :] + F32(0.5)
        ys = F32(oh) - (np.arange(oh, dtype=F32)[:, None] + F32(0.5))
        fu = np.broadcast_to((xs - F32(vx)) / F32(vw_), (oh, ow)).astype(F32)
        fv = np.broadcast_to((ys - F32(vy)) / F32(vh_), (oh, ow)).astype(F32)
        fw = F32(feather_width)
        fo = (_smoothstep(0.0, fw, fu) * _smoothstep(0.0, fw, F32(1) - fu) * _smoothstep(0.0, fw, fv)
              * _smoothstep(0.0, fw, F32(1) - fv))
        color = color * np.power(fo, F32(0.7))[..., None]
    if corner_radius > 0:                                                            # the quad's own uv, not the cropped one
        r = F32(corner_radius)
        dx, dy = np.abs(us - F32(0.5)) - F32(0.5) + r, np.abs(vs - F32(0.5)) - F32(0.5) + r
        sdf = np.sqrt(np.maximum(dx, 0) ** 2 + np.maximum(dy, 0) ** 2).astype(F32) + np.minimum(np.maximum(dx, dy), 0) - r
        alpha = np.minimum(alpha, F32(1) - _smoothstep(0.0, 0.01, sdf.astype(F32)))
    return np.concatenate([color.astype(F32), alpha[..., None].astype(F32)], -1)


def dibr_crop(rgb_u8_hwc, depth, crop, eye_hw, ipd_uv=0.064, depth_ratio=1.0, convergence=0.0, display_mode="Full-SBS",
              viewer_depth_strength=0.1, **kw):
    """Both eyes, each eye_hw = (h, w) pixels, packed as d2s_dibr_warp_crop packs them -> [.., .., 4] (rgb 0..255, alpha)."""
    ds = viewer_depth_strength * depth_ratio
    left = dibr_eye_crop(rgb_u8_hwc, depth, crop, -ipd_uv / 2.0, ds, convergence, eye_hw[0], eye_hw[1], **kw)
    right = dibr_eye_crop(rgb_u8_hwc, depth, crop, ipd_uv / 2.0, ds, convergence, eye_hw[0], eye_hw[1], **kw)
    return np.concatenate([left, right], 1 if display_mode.endswith("SBS") else 0)


def crop_stats(rgb_u8_hwc, plan):
    """(top_i, bottom_count, center_mean, center_bright, left_i, right_count) of xr_viewer/crop.py:386-413 in float64; plan:
    desktop2stereo_amd.crop.sample_plan(w, h)."""
    a = rgb_u8_hwc.astype(np.float64)
    luma = a[..., 0] * 0.2126 + a[..., 1] * 0.7152 + a[..., 2] * 0.0722
    rows = luma[np.asarray(plan["y_rows"])][:, plan["x0"]:plan["x1"]:plan["step_x"]]
    cols = luma[plan["y0_col"]:plan["y1_col"]:plan["step_y"]][:, np.asarray(plan["x_cols"])]

    def runs(uniform):
        n = len(uniform)
        lead = next((i for i in range(n) if not uniform[i]), n)
        trail = next((i for i in range(n) if not uniform[n - 1 - i]), n)
        return float(lead), float(trail)
    top_i, bottom_count = runs(rows.std(axis=1, ddof=1) < 6.0)
    left_i, right_count = runs(cols.std(axis=0, ddof=1) < 6.0)
    m = np.asarray(plan["center_mask"], bool)
    n = max(1.0, float(m.sum()))
    center_mean = float((rows.mean(axis=1) * m).sum() / n)
    center_bright = float(((rows > 20.0).mean(axis=1) * m).sum() / n)
    return (top_i, bottom_count, center_mean, center_bright, left_i, right_count)
