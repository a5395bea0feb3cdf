"""CPU restatement (numpy, float32) of the reference viewer's composite display programs, line by line per shader:
ANAGLYPH_FRAGMENT (viewer.py:678-832), INTERLEAVED_FRAGMENT (:835-1017), VERTICAL_INTERLEAVED_FRAGMENT (:1020-1197) and
DEPTH_FRAGMENT (:633-675).  TEST INFRASTRUCTURE ONLY: tests/test_composite_oracle.py holds it to renders of the reference's own
shader text (tests/golden/composite.npz, make_golden_composite.py), tests/test_gpu_composite.py holds the HIP kernels
(csrc/dibr_composite.hip) to it on inputs the fixtures do not cover.

texture() is oracle.dibr_oracle._tex (exact float32 GL_LINEAR + GL_REPEAT); u_resolution = the source size unless `res` is given
(the reference never assigns it, see include/d2s.h).  A program runs over its viewport (x, y, w, h) in window pixels, y up: output
row r (0 = top), column c is the fragment at gl_FragCoord = (x + c + 0.5, y + h - 1 - r + 0.5), flipped_uv = ((c + 0.5) / w,
(r + 0.5) / h).  Returns frag_color: [h, w, 4] float32, rgb in 0..255, alpha 0..1.
"""
from __future__ import annotations

import numpy as np

from oracle.dibr_oracle import _smoothstep, _tex

F32 = np.float32
MODES = ("Anaglyph", "Interleaved", "Interleaved-V", "Depth Map")


def _inpaint(rgb, dep, u, v, cdi, step, ps, search_radius, tol, blur):
    """push_pull_inpaint of the three warp programs for flat pixel arrays; step(i) -> (du, dv): the program's sweep offset of tap i
    (phase 1 samples uv + (du, dv), phase 2 uv - (du, dv))."""
    n = u.shape[0]
    best = np.zeros((n, 3), F32)
    bw = np.zeros(n, F32)
    active = np.ones(n, bool)
    for i in range(1, int(search_radius) + 1):                                     # phase 1
        du, dv = step(i)
        su, sv = (u + du).astype(F32), (v + dv).astype(F32)
        ok = active & ~((su < 0) | (sv < 0) | (su > 1) | (sv > 1))
        sdi = F32(1) - _tex(dep, su, sv)
        ok &= sdi > cdi + F32(tol)
        w = (np.exp(F32(-i * 0.15), dtype=F32) * (F32(1) + (sdi - cdi) * F32(10))).astype(F32)
        col = _tex(rgb, su, sv)
        best[ok] += col[ok] * w[ok, None]
        bw[ok] += w[ok]
        active &= ~(ok & (bw > 5))                                                  # early exit
    need2 = bw < 2                                                                  # phase 2: the opposite sweep
    for i in range(1, int(search_radius) + 1):
        du, dv = step(i)
        su, sv = (u - du).astype(F32), (v - dv).astype(F32)
        ok = need2 & ~((su < 0) | (sv < 0) | (su > 1) | (sv > 1))
        sdi = F32(1) - _tex(dep, su, sv)
        ok &= sdi > cdi + F32(tol)
        w = np.exp(F32(-i * 0.2), dtype=F32)
        col = _tex(rgb, su, sv)
        best[ok] += col[ok] * w
        bw[ok] += w
    out = _tex(rgb, u, v)                                                           # fallback
    has = bw > F32(0.01)                                                            # phase 3: 3-tap vertical blur
    blurred = best / np.maximum(bw, F32(1e-30))[:, None]
    va = blurred * F32(0.5)
    vw = np.full(n, 0.5, F32)
    for dy in (-1, 1):
        vv = (v + F32(dy) * F32(ps[1]) * F32(blur)).astype(F32)
        ok = has & (vv >= 0) & (vv <= 1)
        vdi = F32(1) - _tex(dep, u, vv)
        ok &= vdi > cdi + F32(tol * 0.5)
        col = _tex(rgb, u, vv)
        va[ok] += col[ok] * F32(0.25)
        vw[ok] += F32(0.25)
    out[has] = (va / vw[:, None])[has]
    return out.astype(F32)


def _sweep(mode, eye, c, s, psx):
    """The sweep step of tap i for pixels of eye_dir `eye` (flat array).  Interleaved (:871, 875): sweep = vec2(c, s) * eye_dir,
    uv +- sweep * pixel_size.x * float(i).  Anaglyph / Interleaved-V (:717-720, 1058-1062): search_dir = eye_dir > 0 ? -1 : 1,
    uv +- vec2(float(search_dir * i) * pixel_size.x * c, ... * s)."""
    if mode == "Interleaved":
        kx, ky = (F32(c) * eye * F32(psx)).astype(F32), (F32(s) * eye * F32(psx)).astype(F32)
        return lambda i: ((kx * F32(i)).astype(F32), (ky * F32(i)).astype(F32))
    sd = np.where(eye > 0, -1, 1)

    def step(i):
        t = ((sd * i).astype(F32) * F32(psx)).astype(F32)
        return (t * F32(c)).astype(F32), (t * F32(s)).astype(F32)
    return step


def _fx(col, alpha, fu, fv, feather, feather_width, corner_radius):
    """Feathering (frag_color.rgb *= pow(falloff, 0.7)) and the rounded-corner SDF, both over fuv."""
    if feather:
        fw = F32(feather_width)
        fo = (_smoothstep(0.0, fw, fu) * _smoothstep(0.0, fw, F32(1) - fu) * _smoothstep(0.0, fw, fv)
              * _smoothstep(0.0, fw, F32(1) - fv))
        col = (col * np.power(fo, F32(0.7))[..., None]).astype(F32)
    if corner_radius > 0:
        r = F32(corner_radius)
        dx, dy = np.abs(fu - F32(0.5)) - F32(0.5) + r, np.abs(fv - F32(0.5)) - F32(0.5) + r
        sdf = np.sqrt(np.maximum(dx, 0) ** 2 + np.maximum(dy, 0) ** 2).astype(F32) + np.minimum(np.maximum(dx, dy), 0) - r
        alpha = np.minimum(alpha, F32(1) - _smoothstep(0.0, 0.01, sdf.astype(F32)))
    return col, alpha


def spectral_r_ultrafast(t):
    """DEPTH_FRAGMENT's colour map (:640-664) -> [..., 3] in 0..1."""
    t = t.astype(F32)
    w = [np.maximum(F32(0), F32(1) - np.abs(t - F32(k)) * F32(4)).astype(F32) for k in (0.125, 0.375, 0.625, 0.875)]
    total = (w[0] + w[1] + w[2] + w[3]).astype(F32)
    pos = total > 0
    w = [np.where(pos, wk / np.where(pos, total, F32(1)), wk).astype(F32) for wk in w]
    keys = ((0.0, 0.298, 0.651), (0.0, 0.5, 0.0), (1.0, 0.851, 0.0), (0.988, 0.0, 0.0))
    out = [F32(keys[0][k]) * w[0] + F32(keys[1][k]) * w[1] + F32(keys[2][k]) * w[2] + F32(keys[3][k]) * w[3] for k in range(3)]
    return np.stack(out, -1).astype(F32)


def composite_frag(rgb_u8_hwc, depth, mode, ipd_uv=0.064, depth_ratio=2.0, convergence=0.0, viewport=None, roll=0.0, res=None,
                   search_radius=12.0, tol=0.012, blur=2.5, feather=False, feather_width=0.02, corner_radius=0.0,
                   viewer_depth_strength=0.1):
    """frag_color of `mode` over the viewport (x, y, w, h) (None: (0, 0, W, H)) -> float32 [h, w, 4]: rgb 0..255, alpha 0..1."""
    assert mode in MODES, mode
    H, W = depth.shape
    vx, vy, ow, oh = viewport if viewport is not None else (0, 0, W, H)
    dep = depth.astype(F32)
    v, u = np.meshgrid((np.arange(oh, dtype=F32) + F32(0.5)) / F32(oh), (np.arange(ow, dtype=F32) + F32(0.5)) / F32(ow),
                       indexing="ij")
    if mode == "Depth Map":                                                         # :666-674
        col = spectral_r_ultrafast(_tex(dep, u, v)) * F32(255)
        return np.concatenate([col, np.ones((oh, ow, 1), F32)], -1).astype(F32)
    rgb = rgb_u8_hwc.astype(F32)
    rw, rh = res or (W, H)
    ps = (F32(1) / F32(rw), F32(1) / F32(rh))
    c, s = F32(np.cos(roll)), F32(np.sin(roll))
    off = F32(ipd_uv / 2.0)                                                         # u_eye_offset = +ipd_uv / 2 (viewer.py:2638)
    strength = F32(viewer_depth_strength * depth_ratio)
    conv = F32(convergence)
    gx = np.broadcast_to(F32(vx) + np.arange(ow, dtype=F32)[None, :] + F32(0.5), (oh, ow))          # gl_FragCoord, y up
    gy = np.broadcast_to(F32(vy) + (F32(oh - 1) - np.arange(oh, dtype=F32)[:, None]) + F32(0.5), (oh, ow))
    fu, fv = ((gx - F32(vx)) / F32(ow)).astype(F32), ((gy - F32(vy)) / F32(oh)).astype(F32)
    fall = (_smoothstep(0.0, 0.02, u) * _smoothstep(1.0, F32(1.0) - F32(0.02), u)).astype(F32)      # edge_margin = 0.02

    if mode == "Anaglyph":                                                          # :780-831
        dsx, dsy = F32(c * ps[0] * F32(1.5)), F32(s * ps[1] * F32(1.5))
        d = (_tex(dep, u, v) * F32(0.7) + _tex(dep, u - dsx, v - dsy) * F32(0.15) + _tex(dep, u + dsx, v + dsy) * F32(0.15)).astype(F32)
        dinv = -d
        sa = ((dinv + conv) * strength * fall).astype(F32)
        ox, oy = (off * sa * c).astype(F32), (off * sa * s).astype(F32)
        lu, lv, ru, rv = u + ox, v + oy, u - ox, v - oy
        s2x, s2y = F32(c * ps[0] * F32(2)), F32(s * ps[1] * F32(2))
        jump = np.abs(_tex(dep, u + s2x, v + s2y) - _tex(dep, u - s2x, v - s2y)) > F32(0.08)
        cols = []
        for eu, ev, eye in ((lu, lv, -1.0), (ru, rv, 1.0)):
            occ = (eu < 0) | (eu > 1) | (ev < 0) | (ev > 1) | jump
            col = _tex(rgb, eu, ev)
            if occ.any():
                e = np.full(int(occ.sum()), F32(eye), F32)
                col[occ] = _inpaint(rgb, dep, u[occ], v[occ], dinv[occ], _sweep(mode, e, c, s, ps[0]), ps, search_radius, tol, blur)
            cols.append(col)
        col = np.stack([cols[0][..., 0], cols[1][..., 1], cols[1][..., 2]], -1).astype(F32)
        bl = _smoothstep(0.0, 0.015, lu) * _smoothstep(1.0, 0.985, lu), _smoothstep(0.0, 0.015, lv) * _smoothstep(1.0, 0.985, lv)
        br = _smoothstep(0.0, 0.015, ru) * _smoothstep(1.0, 0.985, ru), _smoothstep(0.0, 0.015, rv) * _smoothstep(1.0, 0.985, rv)
        alpha = np.minimum(np.minimum(bl[0], bl[1]), np.minimum(br[0], br[1])).astype(F32)
    else:                                                                           # :933-1016 / :1095-1196
        par = (gy if mode == "Interleaved" else gx).astype(np.int64) % 2
        eye = np.where(par == 0, F32(-1), F32(1)).astype(F32)
        my_off = (eye * off).astype(F32)
        parx, pary = (c * eye).astype(F32), (s * eye).astype(F32)
        dsx, dsy = (parx * ps[0] * F32(1.5)).astype(F32), (pary * ps[1] * F32(1.5)).astype(F32)
        d = (_tex(dep, u, v) * F32(0.7) + _tex(dep, u - dsx, v - dsy) * F32(0.15) + _tex(dep, u + dsx, v + dsy) * F32(0.15)).astype(F32)
        dinv = -d
        shaped = dinv * (F32(1) + F32(0.35) * (F32(1) - d))
        px = (my_off * (shaped + conv) * strength * fall).astype(F32)
        su, sv = (u - px * c).astype(F32), (v - px * s).astype(F32)
        oob = (su < 0) | (su > 1) | (sv < 0) | (sv > 1)
        s2x, s2y = (parx * ps[0] * F32(2)).astype(F32), (pary * ps[1] * F32(2)).astype(F32)
        jump = np.abs(_tex(dep, u - s2x, v - s2y) - _tex(dep, u + s2x, v + s2y))
        conf = np.where(oob, F32(1), _smoothstep(0.06, 0.12, jump)).astype(F32)
        col = _tex(rgb, su, sv)
        m = conf > F32(0.001)
        if m.any():                                                                 # the in-painting REPLACES the colour
            col[m] = _inpaint(rgb, dep, u[m], v[m], dinv[m], _sweep(mode, eye[m], c, s, ps[0]), ps, search_radius, tol, blur)
        bx = _smoothstep(-0.001, 0.001, su) * _smoothstep(1.001, 0.999, su)
        by = _smoothstep(-0.001, 0.001, sv) * _smoothstep(1.001, 0.999, sv)
        alpha = np.minimum(bx, by).astype(F32)
    col, alpha = _fx(col, alpha, fu, fv, feather, feather_width, corner_radius)
    return np.concatenate([col, alpha[..., None]], -1).astype(F32)


def composite(rgb_u8_hwc, depth, mode, alpha="window", **kw):
    """What d2s_dibr_composite writes (F32_HWC): "window" = frag_color.rgb, "premultiplied" = rgb * a, "rgba" = four channels."""
    out = composite_frag(rgb_u8_hwc, depth, mode, **kw)
    if alpha == "rgba":
        return out
    return (out[..., :3] * out[..., 3:4]).astype(F32) if alpha == "premultiplied" else np.ascontiguousarray(out[..., :3])
