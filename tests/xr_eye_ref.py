"""CPU restatement (numpy) of the OpenXR viewer's eye views (d2s_dibr_xr_eyes).  TEST INFRASTRUCTURE ONLY.

What EffectsMixin._render_eye draws (xr_viewer/effects.py:1023-1137): the screen -- a flat quad or the 48-segment curved strip -- as
planar facets, each with a homography from the pixel centre to the interpolated vertex uv (GL's perspective-correct interpolation);
a pixel is covered when its centre lies inside a projected facet, the smallest NDC depth wins and ties go to the lower facet index
(GL_LESS against a cleared buffer); covered pixels run the XR fragment shader at that uv, the others keep the clear colour.

The shader is oracle.dibr_oracle.dibr_eye / xr_crop_ref.dibr_eye_crop restated over an ARBITRARY uv array and a number type: the
oracle's _tex / _inpaint / _smoothstep take any uv but compute in float32, so they are written out here once over `T` (float64: the
reference the GPU test compares with; float32: the same expressions in the kernel's precision, which is what measures how often
rounding flips one of the shader's thresholds).  tests/test_xr_eye_oracle.py holds the float32 form to xr_crop_ref.dibr_eye_crop on
the regular grid, and the float64 form to renders of the reference's own shaders (tests/golden/xr_eye.npz).
"""
from __future__ import annotations

import numpy as np


def facets_flat(model):
    """The flat quad: corners model @ (+-1, +-1, 0, 1), uv as quad_vao has them -> [(p00, p10, p01, uv00, uv10, uv01)]."""
    m = np.asarray(model, np.float64).reshape(4, 4)
    c = lambda x, y: (m @ np.array([x, y, 0.0, 1.0]))[:3]
    return [(c(-1, -1), c(1, -1), c(-1, 1), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0))]


def facets_strip(verts, vertical):
    """The curved TRIANGLE_STRIP [(N + 1) * 2, 5] = x y z u v: column pair i and i + 1 bound facet i."""
    v = np.asarray(verts, np.float64).reshape(-1, 5)
    out = []
    for i in range(v.shape[0] // 2 - 1):
        p00, a, b = v[2 * i], v[2 * i + 2], v[2 * i + 1]      # a runs along the strip for both curves, b across it
        out.append((p00[:3], a[:3], b[:3], tuple(p00[3:]), tuple(a[3:]), tuple(b[3:])))
    return out


def facet_table(facets, vp, w, h):
    """Per facet, in float64: rows ha, hb, hw, hz over (xc, yc, 1), (xc, yc) = pixel centre - image centre with y down, and the uv
    affine (u0, ua, ub, v0, va, vb), then he = hw - ha, the upper a-edge as a row of its own -> [F, 21]."""
    vp = np.asarray(vp, np.float64).reshape(4, 4)
    tab = []
    for p00, p10, p01, t00, t10, t01 in facets:
        C0 = vp @ np.append(p00, 1.0)
        CA = vp @ np.append(np.asarray(p10) - p00, 0.0)
        CB = vp @ np.append(np.asarray(p01) - p00, 0.0)
        M = np.array([[CA[0], CB[0], C0[0]], [CA[1], CB[1], C0[1]], [CA[3], CB[3], C0[3]]])
        M = np.diag([w / 2.0, -h / 2.0, 1.0]) @ M
        if abs(np.linalg.det(M)) <= 1e-14 * np.abs(M).max() ** 3:
            tab.append([0, 0, -1.0] + [0.0] * 18)
            continue
        N = np.linalg.inv(M)
        hz = CA[2] * N[0] + CB[2] * N[1] + C0[2] * N[2]
        tab.append(list(N[0]) + list(N[1]) + list(N[2]) + list(hz) +
                   [t00[0], t10[0] - t00[0], t01[0] - t00[0], t00[1], t10[1] - t00[1], t01[1] - t00[1]] + list(N[2] - N[0]))
    return np.array(tab, np.float64)


def min_clip_w(facets, vp):
    vp = np.asarray(vp, np.float64).reshape(4, 4)
    ws = []
    for p00, p10, p01, *_ in facets:
        for p in (p00, p10, p01, np.asarray(p10) + p01 - p00):
            ws.append((vp @ np.append(p, 1.0))[3])
    return min(ws)


def eye_uv(tab, w, h, T=np.float64):
    """-> (covered [h,w] bool, us, vs [h,w] T): the screen's own uv of every pixel, top-left origin (u, 1 - v of the vertex uv).
    The table is rounded to T; then, as the library does, facet f's upper a-edge becomes the exact negation of facet f + 1's ha row (one
    edge function per interior seam of a strip: watertight in any precision).  Depth: LESS against a buffer cleared to 1, and GL's near
    plane (NDC z >= -1)."""
    t = _rows(tab, T)
    yc, xc = np.meshgrid((np.arange(h, dtype=T) + T(0.5)) - T(0.5) * T(h), (np.arange(w, dtype=T) + T(0.5)) - T(0.5) * T(w), indexing="ij")
    bz = np.full((h, w), 1.0, T)
    ba, bb, bw = np.zeros((h, w), T), np.zeros((h, w), T), np.ones((h, w), T)
    best = np.full((h, w), -1, np.int64)
    for f in range(t.shape[0]):
        r = t[f]
        na, nb, nw = r[0] * xc + r[1] * yc + r[2], r[3] * xc + r[4] * yc + r[5], r[6] * xc + r[7] * yc + r[8]
        z = r[9] * xc + r[10] * yc + r[11]
        ne = r[18] * xc + r[19] * yc + r[20]
        hit = (na >= 0) & (ne >= 0) & (nb >= 0) & (nb <= nw) & (nw > 0) & (z >= -1) & (z < bz)
        bz, ba, bb, bw = np.where(hit, z, bz), np.where(hit, na, ba), np.where(hit, nb, bb), np.where(hit, nw, bw)
        best = np.where(hit, f, best)
    a, b = (ba / bw).astype(T), (bb / bw).astype(T)
    k = np.maximum(best, 0)
    u = t[k, 12] + a * t[k, 13] + b * t[k, 14]
    v = t[k, 15] + a * t[k, 16] + b * t[k, 17]
    return best >= 0, u.astype(T), (T(1) - v).astype(T)


def _rows(tab, T):
    """The table rounded to T with the library's shared seams (see eye_uv)."""
    t = tab.astype(T)
    live = ~((t[:, 0] == 0) & (t[:, 1] == 0) & (t[:, 2] == -1))
    for f in range(t.shape[0] - 1):
        if live[f] and live[f + 1]:
            t[f, 18:21] = -t[f + 1, 0:3]
    return t


def coverage(facets, vp, w, h, T=np.float64, shared_seams=True):
    """The kernel's coverage test alone, in T, at any image size: each facet is evaluated on the bounding box of its projected corners
    (+ 2 pixels), which is where it can cover anything (every vertex has clip w > 0).  -> (covered [h,w] bool, count [h,w]: how many
    facets cover the pixel).  shared_seams=False: every facet tests its own upper edge na <= nw (NOT what the library does: the
    form that leaves holes along seams in float32, kept to show that the hole test can fail)."""
    tab = facet_table(facets, vp, w, h)
    t = _rows(tab, T) if shared_seams else tab.astype(T)
    vp = np.asarray(vp, np.float64).reshape(4, 4)
    count = np.zeros((h, w), np.int32)
    for f, (p00, p10, p01, *_) in enumerate(facets):
        cs = np.array([vp @ np.append(p, 1.0) for p in (p00, p10, p01, np.asarray(p10) + p01 - p00)])
        px, py = (cs[:, 0] / cs[:, 3] + 1) * w / 2.0, (1 - cs[:, 1] / cs[:, 3]) * h / 2.0
        x0, x1 = int(max(0, np.floor(px.min()) - 2)), int(min(w, np.ceil(px.max()) + 3))
        y0, y1 = int(max(0, np.floor(py.min()) - 2)), int(min(h, np.ceil(py.max()) + 3))
        if x0 >= x1 or y0 >= y1:
            continue
        yc, xc = np.meshgrid((np.arange(y0, y1, dtype=T) + T(0.5)) - T(0.5) * T(h), (np.arange(x0, x1, dtype=T) + T(0.5)) - T(0.5) * T(w),
                             indexing="ij")
        r = t[f]
        na, nb, nw = r[0] * xc + r[1] * yc + r[2], r[3] * xc + r[4] * yc + r[5], r[6] * xc + r[7] * yc + r[8]
        z = r[9] * xc + r[10] * yc + r[11]
        upper = (r[18] * xc + r[19] * yc + r[20] >= 0) if shared_seams else (na <= nw)
        count[y0:y1, x0:x1] += (na >= 0) & upper & (nb >= 0) & (nb <= nw) & (nw > 0) & (z >= -1) & (z < 1)
    return count > 0, count


def interior(cov):
    """Covered pixels whose whole 3 x 3 neighbourhood is covered: strictly inside the surface's image, off the outline."""
    return cov & uniform3x3(cov)


def uniform3x3(cov):
    """Pixels whose 3 x 3 neighbourhood (clamped at the image border) has one coverage value: the rasteriser's fill rule owns the rest."""
    p = np.pad(cov, 1, mode="edge")
    h, w = cov.shape
    ok = np.ones_like(cov, bool)
    for dy in range(3):
        for dx in range(3):
            ok &= p[dy:dy + h, dx:dx + w] == cov
    return ok


# ---- the XR fragment shader over arbitrary uv, number type T (viewer.py:386-631 through xr_viewer/implementation.py:111-126) ----

def _tex(img, u, v, T):
    H, W = img.shape[:2]
    x, y = u * T(W) - T(0.5), v * T(H) - T(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f).astype(T), (y - y0f).astype(T)
    x0, y0 = np.mod(x0f.astype(np.int64), W), np.mod(y0f.astype(np.int64), H)
    x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
    if img.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    top, bot = a + (b - a) * fx, c + (d - c) * fx
    return (top + (bot - top) * fy).astype(T)


def _smoothstep(e0, e1, x, T):
    t = np.clip((x - T(e0)) / T(e1 - e0), T(0), T(1)).astype(T)
    return (t * t * (T(3) - T(2) * t)).astype(T)


def _inpaint(rgb, dep, u, v, cdi, par, sweep_sign, ps, search, tol, blur, T):
    n = u.shape[0]
    best, bw = np.zeros((n, 3), T), np.zeros(n, T)
    sx, sy = T(par[0] * ps[0] * T(sweep_sign)), T(par[1] * ps[0] * T(sweep_sign))
    active = np.ones(n, bool)
    for i in range(1, int(search) + 1):
        su, sv = u + sx * T(i), v + sy * T(i)
        ok = active & ~((su < 0) | (sv < 0) | (su > 1) | (sv > 1))
        sdi = T(1) - _tex(dep, su, sv, T)
        ok &= sdi > cdi + T(tol)
        wgt = (T(np.exp(np.float32(-i * 0.15), dtype=np.float32)) * (T(1) + (sdi - cdi) * T(10))).astype(T)
        col = _tex(rgb, su, sv, T)
        best[ok] += col[ok] * wgt[ok, None]
        bw[ok] += wgt[ok]
        active &= ~(ok & (bw > 5))
    need2 = bw < 2
    for i in range(1, int(search) + 1):
        su, sv = u - sx * T(i), v - sy * T(i)
        ok = need2 & ~((su < 0) | (sv < 0) | (su > 1) | (sv > 1))
        sdi = T(1) - _tex(dep, su, sv, T)
        ok &= sdi > cdi + T(tol)
        wgt = T(np.exp(np.float32(-i * 0.2), dtype=np.float32))
        col = _tex(rgb, su, sv, T)
        best[ok] += col[ok] * wgt
        bw[ok] += wgt
    out = _tex(rgb, u, v, T)
    has = bw > T(0.01)
    va = best / np.maximum(bw, T(1e-30))[:, None] * T(0.5)
    vw = np.full(n, 0.5, T)
    for dy in (-1, 1):
        vv = v + T(dy) * ps[1] * T(blur)
        ok = has & (vv >= 0) & (vv <= 1)
        vdi = T(1) - _tex(dep, u, vv, T)
        ok &= vdi > cdi + T(tol) * T(0.5)
        col = _tex(rgb, u, vv, T)
        va[ok] += col[ok] * T(0.25)
        vw[ok] += T(0.25)
    out[has] = (va / vw[:, None])[has]
    return out.astype(T)


def shade(rgb_u8_hwc, depth, us, vs, crop, eye_offset, depth_strength, convergence=0.0, roll=0.0, corner_radius=0.0,
          search_radius=12.0, tol=0.012, blur=2.5, T=np.float64):
    """frag_color at the flat arrays us, vs (the screen's own uv, top-left origin) -> [n, 4]: rgb 0..255, alpha 0..1.  The uniforms are
    the float32 values GL receives; the arithmetic runs in T.  Depth at the frame's own size (up-sample a model-resolution map first)."""
    f32 = np.float32
    H, W = depth.shape
    rgb, dep = rgb_u8_hwc.astype(T), depth.astype(f32).astype(T)
    ps = (T(1) / T(W), T(1) / T(H))
    cx, cy, cw, ch = (T(f32(c)) for c in crop)
    us, vs = us.astype(T), vs.astype(T)
    u, v = (cx + us * cw).astype(T), (cy + vs * ch).astype(T)
    c, s = T(np.cos(f32(roll))), T(np.sin(f32(roll)))
    eye_offset, depth_strength, convergence = T(f32(eye_offset)), T(f32(depth_strength)), T(f32(convergence))
    sg = T(np.sign(eye_offset))
    par = (c * sg, s * sg)
    sweep_sign = -1.0 if eye_offset > 0 else 1.0
    dsx, dsy = par[0] * ps[0] * T(1.5), par[1] * ps[1] * T(1.5)
    d = (_tex(dep, u, v, T) * T(0.7) + _tex(dep, u - dsx, v - dsy, T) * T(0.15) + _tex(dep, u + dsx, v + dsy, T) * T(0.15)).astype(T)
    dinv = -d
    shift = dinv * (T(1) + T(0.35) * (T(1) - d)) + convergence
    fall = _smoothstep(0.0, 0.05, u, T) * _smoothstep(1.0, 0.95, u, T)
    px = (eye_offset * shift * depth_strength * fall).astype(T)
    su, sv = (u - px * c).astype(T), (v - px * s).astype(T)
    oob = (su < 0) | (su > 1) | (sv < 0) | (sv > 1)
    s2x, s2y = par[0] * ps[0] * T(2), par[1] * ps[1] * T(2)
    jump = np.abs(_tex(dep, u - s2x, v - s2y, T) - _tex(dep, u + s2x, v + s2y, T))
    conf = np.where(oob, T(1), _smoothstep(0.04, 0.10, jump, T)).astype(T)
    color = _tex(rgb, su, sv, T)
    m = conf > T(0.001)
    if m.any():
        filled = _inpaint(rgb, dep, u[m], v[m], dinv[m], par, sweep_sign, ps, search_radius, f32(tol), f32(blur), T)
        cm = conf[m][:, None]
        color[m] = color[m] * (T(1) - cm) + filled * cm
    bx = _smoothstep(-0.001, 0.001, su, T) * _smoothstep(1.001, 0.999, su, T)
    by = _smoothstep(-0.001, 0.001, sv, T) * _smoothstep(1.001, 0.999, sv, T)
    alpha = np.minimum(bx, by)
    if corner_radius > 0:
        r = T(f32(corner_radius))
        dx, dy = np.abs(us - T(0.5)) - T(0.5) + r, np.abs(vs - T(0.5)) - T(0.5) + r
        sdf = np.sqrt(np.maximum(dx, 0) ** 2 + np.maximum(dy, 0) ** 2).astype(T) + np.minimum(np.maximum(dx, dy), 0) - r
        alpha = np.minimum(alpha, T(1) - _smoothstep(0.0, 0.01, sdf, T))
    return np.concatenate([color.astype(T), alpha[:, None].astype(T)], -1)


def render_eye(rgb_u8_hwc, depth, facets, vp, w, h, eye, clear, crop=(0.0, 0.0, 1.0, 1.0), ipd_uv=0.064, depth_strength=0.1,
               convergence=0.0, roll=0.0, corner_radius=0.0, T=np.float64):
    """One eye image -> (frag [h,w,4] T: rgb 0..255, alpha 0..1; covered [h,w] bool).  The facet table is formed in float64 and
    rounded to T, as the library rounds its own to float32."""
    cov, us, vs = eye_uv(facet_table(facets, vp, w, h), w, h, T)
    out = np.empty((h, w, 4), T)
    out[...] = [T(np.float32(clear[0])) * T(255), T(np.float32(clear[1])) * T(255), T(np.float32(clear[2])) * T(255), T(np.float32(clear[3]))]
    if cov.any():
        out[cov] = shade(rgb_u8_hwc, depth, us[cov], vs[cov], crop, (ipd_uv / 2.0) * (1.0 if eye else -1.0), depth_strength, convergence,
                         roll, corner_radius, T=T)
    return out, cov


# ---- the cases of tests/golden/xr_eye.json (make_golden_xr_eye.py) ----

def case_scene(c, meta):
    """(rgb, the H x W depth texture, the depth map handed to the library) of a manifest case of tests/golden/xr_eye.json."""
    from desktop2stereo_amd import synth
    from oracle import d2s_oracle as O
    H, W = meta["source"]
    img, dep = synth.dibr_scene(H, W, c["seed"], "boxes")
    if c["depth_hw"]:
        small = synth.dibr_scene(c["depth_hw"][0], c["depth_hw"][1], c["seed"], "boxes")[1]
        return img, O.upsample_depth(small, H, W).astype(np.float32), small
    return img, dep, dep


def case_facets(c):
    if c["screen"]["curve"] == "flat":
        return facets_flat(np.array(c["model"]))
    return facets_strip(np.array(c["strip"]), c["screen"]["curve"] == "vertical")


def case_kw(c):
    return dict(crop=c["crop"], ipd_uv=c["ipd_uv"], depth_strength=0.1 * c["depth_ratio"], convergence=c["convergence"],
                roll=c["screen"]["roll"], corner_radius=c["corner_radius"])


def golden_eye(z, c, eye):
    return np.concatenate([z[f"{c['name']}_{eye}_rgb"].astype(np.float64) / 256.0, z[f"{c['name']}_{eye}_a"].astype(np.float64)[..., None] / 65535.0], -1)
